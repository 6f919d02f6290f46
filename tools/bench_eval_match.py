#!/usr/bin/env python3
"""Times the evaluator's matching stage (Omni3Deval._match_cells) with matcher="host" against matcher="device" on a seeded
synthetic set and checks that both give the same per-cell results and precision / recall tables.

    python tools/bench_eval_match.py [--images 1000] [--mode 2D] [--runs 5] [--host-runs 3] [--eval-prox] [--no-host]

The stage starts from built cells (``_build_cells``); on the device it includes the packing, the upload, the 2D IoU launch, the
matcher launch, the download and filling ``per_cell``. Times are wall clock around a ``torch.cuda.synchronize()``, warm, median
of the runs. One JSON line is printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval  # noqa: E402


def synthetic_set(n_images, n_cats=3, seed=0):
    """About 9 ground-truth boxes and 103 detections per image over ``n_cats`` categories; half of the detections lie near a
    ground-truth box of their cell, the rest anywhere in a 1280 x 720 image."""
    g = np.random.default_rng(seed)
    gts, dts = [], []
    for img in range(n_images):
        for cat in range(n_cats):
            n_gt = int(g.poisson(3.0))
            boxes = np.column_stack([g.uniform(0, 1100, n_gt), g.uniform(0, 600, n_gt), g.uniform(8, 180, n_gt), g.uniform(8, 120, n_gt)])
            for b in boxes:
                gts.append({"image_id": img, "category_id": cat, "bbox": b.tolist(), "depth": float(g.uniform(1, 60)),
                            "ignore2D": int(g.random() < 0.1), "ignore3D": int(g.random() < 0.1)})
            n_dt = int(g.poisson(34.4))
            near = g.random(n_dt) < 0.5 if n_gt else np.zeros(n_dt, bool)
            d = np.column_stack([g.uniform(0, 1100, n_dt), g.uniform(0, 600, n_dt), g.uniform(8, 180, n_dt), g.uniform(8, 120, n_dt)])
            if near.any():
                src = boxes[g.integers(0, n_gt, int(near.sum()))]
                d[near] = src + g.normal(0, 1, src.shape) * np.maximum(src[:, 2:3], src[:, 3:4]) * 0.1
                d[near, 2:] = np.abs(d[near, 2:])
            for b, s in zip(d, g.random(n_dt)):
                dts.append({"image_id": img, "category_id": cat, "bbox": b.tolist(), "score": float(s), "depth": float(g.uniform(1, 60))})
    return gts, dts


def time_stage(e, runs, dev):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e._match_cells()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--cats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", choices=("2D", "3D"), default="2D")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--eval-prox", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="device runs only (e.g. under a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the device matcher needs the GPU"
    dev = torch.device("cuda", 0)
    gts, dts = synthetic_set(a.images, a.cats, a.seed)
    kw = dict(device=dev, fork_compat_2d_iou=True, eval_prox=a.eval_prox)
    out = {"images": a.images, "detections": len(dts), "ground_truth": len(gts), "mode": a.mode, "eval_prox": a.eval_prox}
    d = Omni3Deval(gts, dts, a.mode, matcher="device", **kw)
    d._build_cells(with_iou=False)
    d._match_cells()                                                            # warm-up: code objects, allocator
    ts = time_stage(d, a.runs, dev)
    out["device_s"] = statistics.median(ts)
    out["device_runs_s"] = [round(t, 4) for t in ts]
    if not a.no_host:
        h = Omni3Deval(gts, dts, a.mode, matcher="host", **kw)
        h._build_cells(with_iou=True)
        ts = time_stage(h, a.host_runs, dev)
        out["host_s"] = statistics.median(ts)
        out["host_runs_s"] = [round(t, 3) for t in ts]
        out["speedup"] = out["host_s"] / out["device_s"]
        same = set(h.per_cell) == set(d.per_cell) and all(
            np.array_equal(r[f], d.per_cell[k][f]) for k, r in h.per_cell.items() for f in ("matched", "ignored", "pick", "gt_order")) and all(
            r["n_gt"] == d.per_cell[k]["n_gt"] for k, r in h.per_cell.items())
        h.accumulate(); d.accumulate()
        out["identical"] = bool(same and all(np.array_equal(h.eval[k], d.eval[k]) for k in ("precision", "recall", "scores")))
    print(json.dumps(out))
    if not a.no_host and not out["identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
