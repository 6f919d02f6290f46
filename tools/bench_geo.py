#!/usr/bin/env python3
"""Times OVMono3D-GEO's lifting (ovm_geo_lift, csrc/geo.hip) on one image with 20 instances - the scenes of tests/geo_oracle.py
side by side, ten of them at the 40,000-point cap - per image and per stage, against the numpy / scipy restatement on the host
and, where scikit-learn is importable, against sklearn.cluster.DBSCAN itself on the same clouds.

    python tools/bench_geo.py [--runs 5] [--warmup 2] [--no-host]

Device times are HIP event times around the launch sequence alone (inputs resident, no read inside), warm, median of the runs.
A stage's time is the difference of two runs that stop after consecutive stages (OvmGeoParams.last_stage). One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geo_oracle as G  # noqa: E402
from ovmono3d_amd.geo import LiftCall  # noqa: E402

STAGES = ["points", "mean_yaw", "rotate_gather", "trial1", "trial2", "trial3", "trial4"]


def instances():
    depth, K, inst = G.make_composite()
    ok = [it for it in inst if it["name"] not in ("empty", "too_few", "nonfinite", "outside", "degenerate")]
    return depth, K, ok + ok


def event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="device runs only (e.g. under a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the lifting needs the GPU"
    dev = torch.device("cuda", 0)
    depth, K, inst = instances()
    d = torch.from_numpy(depth).to(dev)
    masks = [torch.from_numpy(it["mask"]).to(dev) if "mask" in it else None for it in inst]
    boxes = np.array([it.get("box", (0.0, 0.0, 0.0, 0.0)) for it in inst], np.float64)
    call = LiftCall(d, K, boxes_xyxy=boxes, masks=masks)
    call.launch(0)
    res, _ = call.read()
    out = {"instances": len(inst), "at_cap": sum(r.n_used == 40000 for r in res), "points": sum(r.n_points for r in res),
           "clustered_points": sum(r.n_used for r in res), "trials_run": sum((r.trial or 4) for r in res)}
    out["device_image_ms"] = event_ms(lambda: call.launch(0), a.runs, a.warmup)
    out["device_instance_ms"] = out["device_image_ms"] / len(inst)
    cum = [event_ms(lambda k=k: call.launch(k), a.runs, a.warmup) for k in range(1, len(STAGES) + 1)]
    out["device_stage_ms"] = {s: round(c - p, 4) for s, c, p in zip(STAGES, cum, [0.0] + cum[:-1])}
    if not a.no_host:
        t0 = time.perf_counter()
        refs = [G.lift_points(depth, it.get("mask"), K, rect=G.box_to_rect(it["box"]) if "box" in it else None) for it in inst]
        out["host_restatement_s"] = time.perf_counter() - t0
        out["speedup_vs_restatement"] = out["host_restatement_s"] * 1e3 / out["device_image_ms"]
        out["identical_counts"] = all((r.n_used, r.n_kept, r.trial) == (q["n_used"], q["n_kept"], q["trial"]) for r, q in zip(res, refs))
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            DBSCAN = None
        if DBSCAN is not None:
            t0 = time.perf_counter()
            for q in refs:
                eps = 0.01
                for _ in range(q["trial"] or 4):
                    DBSCAN(eps=eps, min_samples=100).fit(q["T"])
                    eps *= 2
            out["sklearn_dbscan_s"] = time.perf_counter() - t0
    print(json.dumps(out))
    if not a.no_host and not out["identical_counts"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
