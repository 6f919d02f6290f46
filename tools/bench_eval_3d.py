#!/usr/bin/env python3
"""Times the evaluator's true-3D route (Omni3Deval.evaluate() up to and excluding accumulate()) with matcher="device" and
stage3d="host" against stage3d="device" on a seeded synthetic set, and checks that both give the same results.

    python tools/bench_eval_3d.py [--images 1000] [--runs 5] [--split]

The set is ``bench_eval_match.synthetic_set`` (about 9 ground-truth boxes and 103 detections per image) with a seeded cuboid on
every record: ``center_cam``, ``dimensions``, ``R_cam`` / ``pose`` and the ``bbox3D`` corners of ``oracle/box3d.make_box``; half of
the detections carry a perturbed copy of a ground-truth cuboid of their cell. ``evaluate()`` covers building the cells, the 3D
IoU, the matching and the NHD. Times are wall clock between two ``torch.cuda.synchronize()``, warm, median of the runs.
Identity: per-cell picks / ignore flags / ground-truth counts and every cell's IoU block equal exactly, precision / recall /
scores ``array_equal``, the same (detection, ground truth) NHD pairs in the same order, and every NHD value within 2 x e_host of
the host's, where e_host is the host path's own largest error on these pairs against an fp64 restatement computed here (the same
fp32-rounded fields, float64 corners, ``linear_sum_assignment``): the host path builds corners and distances in fp32, the device in
fp64, and a device at least as close to fp64 as the host is within 2 x e_host of it. The device's own error against that
restatement is reported too and must not exceed e_host. One JSON line is printed; the exit status is 1 when the check fails. ``--split`` adds the device route's stages, each timed around a
synchronize in a further run."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_eval_match import synthetic_set  # noqa: E402
from oracle.box3d import make_box  # noqa: E402
from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval  # noqa: E402

NHD_KEYS = ("overall", "xy", "z", "dimensions", "pose")


def _yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _attach(rec, centre, dims_whl, R, rot_key):
    w, h, l = dims_whl
    rec["center_cam"] = [float(v) for v in centre]
    rec["depth"] = float(centre[2])
    rec["dimensions"] = [float(w), float(h), float(l)]
    rec[rot_key] = R.tolist()
    rec["bbox3D"] = make_box(centre, [l, h, w], R).tolist()


def synthetic_set_3d(n_images, n_cats=3, seed=0):
    """``synthetic_set`` with cuboids: ground truth 1-60 m away, 0.3-3 m on a side, any yaw; a detection is with probability 1/2
    (when its cell has ground truth) a copy of one of the cell's cuboids with the centre moved by about 5 % of its size, the
    dimensions scaled by up to 10 % and the yaw by about 0.1 rad, else a cuboid of its own."""
    gts, dts = synthetic_set(n_images, n_cats, seed)
    g = np.random.default_rng([seed, 3])
    by_cell = {}

    def own():
        z = g.uniform(1, 60)
        return np.array([g.uniform(-0.5, 0.5) * z, g.uniform(-0.2, 0.2) * z, z]), g.uniform(0.3, 3.0, 3), _yaw(g.uniform(-np.pi, np.pi))
    for r in gts:
        c, dims, R = own()
        _attach(r, c, dims, R, "R_cam")
        by_cell.setdefault((r["image_id"], r["category_id"]), []).append((c, dims, R))
    for r in dts:
        mine = by_cell.get((r["image_id"], r["category_id"]))
        if mine and g.random() < 0.5:
            c, dims, R = mine[int(g.integers(0, len(mine)))]
            c, dims, R = c + g.normal(0, 0.05, 3) * dims.mean(), dims * (1 + g.uniform(-0.1, 0.1, 3)), _yaw(g.normal(0, 0.1)) @ R
        else:
            c, dims, R = own()
        _attach(r, c, dims, R, "pose")
    return gts, dts


def time_evaluate(e, runs, dev):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e.evaluate()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    return ts


def stage_split(e, dev):
    """Wall clock of the device route's stages in one further run: every library call is followed by a synchronize (which the
    route itself does not do between launches). ``pack_and_upload`` runs from the built cells to the first launch and
    contains ``pack_3d``; ``download_and_fill`` from the last kernel's end to the filled ``per_cell`` and ``nhd_pairs``."""
    from ovmono3d_amd import lib as _lib
    L = _lib.load()
    spans = []

    def timed(name, fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize(dev)
            spans.append((name, t0, time.perf_counter()))
            return r
        return wrapper
    names = ("ovm_eval_iou3d", "ovm_eval_iou2d", "ovm_eval_match", "ovm_eval_nhd")
    saved = {n: getattr(L, n) for n in names}
    saved_pack = e._pack_3d
    try:
        for n in names:
            setattr(L, n, timed(n, saved[n]))
        e._pack_3d = timed("pack_3d", saved_pack)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e._build_cells(with_iou=False)
        t1 = time.perf_counter()
        e._match_cells()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
    finally:
        for n in names:
            setattr(L, n, saved[n])
        e._pack_3d = saved_pack
    out = {name: b - a for name, a, b in spans}
    kernels = [s for s in spans if s[0] != "pack_3d"]
    out["build_cells"] = t1 - t0
    out["pack_and_upload"] = kernels[0][1] - t1
    out["download_and_fill"] = t2 - kernels[-1][2]
    out["total"] = t2 - t0
    return {k: round(v, 4) for k, v in out.items()}


_SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64)


def _corners64(xy, z, dims, R):
    """nhd.cuboid_corners with the same fp32 rounding of the fields and float64 after it."""
    w, h, l = (float(np.float32(v)) for v in dims)
    c = np.array([xy[0], xy[1], z], dtype=np.float32).astype(np.float64)
    return (_SIGNS * (np.array([l, h, w]) / 2.0)) @ np.asarray(R, np.float32).reshape(3, 3).astype(np.float64).T + c


def nhd_fp64(e):
    """[n, 5] fp64 restatement of ``e.nhd_pairs`` (a host-route evaluator), from the records behind ``e.nhd_pair_ids``."""
    from scipy.optimize import linear_sum_assignment
    dt_by_id = {d["id"]: d for c in e.cells.values() for d in c.dt}
    gt_by_id = {g["id"]: g for c in e.cells.values() for g in c.gt}
    out = np.zeros((len(e.nhd_pair_ids), 5))
    for n, (di, gi) in enumerate(e.nhd_pair_ids):
        d, g = dt_by_id[di], gt_by_id[gi]
        pred = (d["center_cam"][:2], d["depth"], d["dimensions"], d["pose"])
        true = (g["center_cam"][:2], g["depth"], g["dimensions"], g["R_cam"])
        gc = _corners64(*true)
        diag = np.linalg.norm(gc.max(axis=0) - gc.min(axis=0))
        for k in range(5):                                                      # overall, then only xy / z / dimensions / pose of the prediction
            mixed = pred if k == 0 else tuple(pred[f] if f == k - 1 else true[f] for f in range(4))
            cost = np.linalg.norm(_corners64(*mixed)[:, None, :] - gc[None, :, :], axis=2)
            rows, cols = linear_sum_assignment(cost)
            out[n, k] = cost[rows, cols].sum() / diag
    return out


def compare(h, d):
    same = set(h.per_cell) == set(d.per_cell) and all(
        np.array_equal(r[f], d.per_cell[k][f]) for k, r in h.per_cell.items() for f in ("matched", "ignored", "pick", "gt_order")) and all(
        r["n_gt"] == d.per_cell[k]["n_gt"] for k, r in h.per_cell.items())
    same_iou = all(c.iou.shape == d.cells[k].iou.shape and np.ascontiguousarray(c.iou).tobytes() == np.ascontiguousarray(d.cells[k].iou).tobytes()
                   for k, c in h.cells.items())
    h.accumulate(); d.accumulate()
    same_tables = all(np.array_equal(h.eval[k], d.eval[k]) for k in ("precision", "recall", "scores"))
    same_pairs = h.nhd_pair_ids == d.nhd_pair_ids and len(h.nhd_pairs) == len(d.nhd_pairs) == len(h.nhd_pair_ids)
    res = {"per_cell": bool(same), "iou_bytes": bool(same_iou), "tables": bool(same_tables), "nhd_same_pairs_in_order": bool(same_pairs)}
    nhd_ok = same_pairs
    if same_pairs and h.nhd_pairs:
        a = np.array([[p[k] for k in NHD_KEYS] for p in h.nhd_pairs])
        b = np.array([[p[k] for k in NHD_KEYS] for p in d.nhd_pairs])
        ref = nhd_fp64(h)
        e_host, e_dev, diff = float(np.abs(a - ref).max()), float(np.abs(b - ref).max()), float(np.abs(a - b).max())
        res.update({"nhd_host_vs_fp64": e_host, "nhd_device_vs_fp64": e_dev, "nhd_device_vs_host": diff})
        nhd_ok = bool(np.isfinite(ref).all() and e_dev <= e_host and diff <= 2 * e_host)
    res["nhd_within_bound"] = bool(nhd_ok)
    res["identical"] = bool(same and same_iou and same_tables and same_pairs and nhd_ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--cats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--eval-prox", action="store_true")
    ap.add_argument("--split", action="store_true", help="also time the device route's stages, one synchronize after each")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the device stages need the GPU"
    dev = torch.device("cuda", 0)
    gts, dts = synthetic_set_3d(a.images, a.cats, a.seed)
    out = {"images": a.images, "detections": len(dts), "ground_truth": len(gts), "eval_prox": a.eval_prox, "runs": a.runs}
    legs = {}
    for stage in ("host", "device"):
        e = Omni3Deval(gts, dts, "3D", device=dev, matcher="device", stage3d=stage, eval_prox=a.eval_prox)
        e.evaluate()                                                            # warm-up: code objects, allocator
        ts = time_evaluate(e, a.runs, dev)
        out[f"{stage}_s"] = statistics.median(ts)
        out[f"{stage}_runs_s"] = [round(t, 4) for t in ts]
        legs[stage] = e
    out["speedup"] = out["host_s"] / out["device_s"]
    out["nhd_pairs"] = len(legs["device"].nhd_pairs)
    if a.split:
        out["device_split_s"] = stage_split(legs["device"], dev)
    out.update(compare(legs["host"], legs["device"]))
    print(json.dumps(out))
    if not out["identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
