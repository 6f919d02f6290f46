#!/usr/bin/env python3
"""Times the ground plane on the device (ovm_geo_ground_plane: points, hypotheses, counts, refinement, frame; csrc/ground.hip) on
rendered rooms (tests/ground_oracle.render_room: floor, back wall, one cuboid, camera pitched 20 and rolled 5 degrees, 3 mm noise)
at 1024 x 768 and 1920 x 1440, strides 1 and 4, 512 hypotheses, the other settings at their defaults.

Per set: ``plane_ms`` - device time between two HIP events around the C call alone (workspace and result allocated before, nothing
read inside), warm, the median of ``--runs`` (at least 7) after ``--warmup`` calls, with min and max; the result is read once after the
timing. With ``--yardstick`` also the vectorised numpy fp64 restatement of the same steps on the host (tests/ground_oracle.ground_plane),
wall clock, once (``yardstick_ms``), and whether the device's counts and integers equal it and how far its plane is from it. One JSON
line per set. The rooms and the yardstick are those of the test tree: the tool runs from a checkout, not from an installed package.

``--write-demo-inputs DIR``: no timing; writes three 480 x 640 rooms (images, depth files, a boxes file, a labels file) and prints the
demo/demo_geo.py command lines whose ``--stage-times`` laps show what the plane adds to a GEO demo image.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ground_oracle as O  # noqa: E402

SIZES = ((768, 1024), (1440, 1920))                                          # (H, W)
STRIDES = (1, 4)


def event_ms(fn, runs, warmup):
    import torch
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
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def room(H, W, seed=0, pitch=20.0, roll=5.0):
    return O.render_room(H, W, 1.25 * H, pitch, roll, cuboid=O.CUBOID_A, seed=seed)


def bench_set(H, W, stride, a, dev):
    import torch
    from ovmono3d_amd.geo import GroundCall, GroundParams
    s = room(H, W)
    p = O.Params(stride=stride)
    call = GroundCall(torch.from_numpy(s["depth"]).to(dev), s["K"], GroundParams(stride=stride), want_counts=True)
    med, lo, hi = event_ms(call.launch, a.runs, a.warmup)
    g = call.read()
    angle = float(np.degrees(np.arccos(min(1.0, float(np.array(g.normal) @ s["normal"])))))
    res = {"size": [H, W], "stride": stride, "hypotheses": p.hypotheses, "runs": a.runs, "warmup": a.warmup, "plane_ms": med,
           "plane_min_max_ms": [lo, hi], "workspace_mb": round(call.nbytes / 2 ** 20, 1), "status": int(g.status), "n_points": int(g.n_points),
           "n_valid_hyp": int(g.n_valid_hyp), "n_inliers": int(g.n_inliers), "point_plane_pairs_per_s": round(g.n_points * p.hypotheses / med * 1e3),
           "angle_to_rendered_floor_deg": round(angle, 4), "offset_error_m": round(abs(g.offset - s["offset"]), 5)}
    if a.yardstick:
        t0 = time.perf_counter()
        ref = O.ground_plane(s["depth"], s["K"], p)
        res["yardstick_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["counts_equal"] = bool(np.array_equal(call.counts.cpu().numpy().astype(np.int64), ref["hyp_counts"]))
        res["integers_equal"] = all(getattr(g, f) == ref[f] for f in ("status", "n_points", "n_valid_hyp", "best_hyp", "hyp_inliers", "n_inliers"))
        res["normal_from_yardstick_rad"] = float(np.linalg.norm(np.cross(np.array(g.normal), ref["normal"])))
        res["offset_from_yardstick_m"] = abs(g.offset - ref["offset"])
    print(json.dumps(res), flush=True)


def write_demo_inputs(out):
    from PIL import Image
    H, W = 480, 640
    os.makedirs(os.path.join(out, "in"), exist_ok=True)
    os.makedirs(os.path.join(out, "maps"), exist_ok=True)
    boxes, K = {}, None
    for k, (pitch, roll) in enumerate(((20.0, 5.0), (15.0, -4.0), (25.0, 2.0))):
        s = room(H, W, seed=10 + k, pitch=pitch, roll=roll)
        K, name = s["K"], f"room{k}"
        rgb = np.clip(40.0 * s["surface"][..., None] + np.array([30.0, 60.0, 90.0]), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(out, "in", name + ".jpg"), quality=92)
        np.savez(os.path.join(out, "maps", name + ".npz"), depth=s["depth"])
        ys, xs = np.nonzero(s["surface"] == O.CUBOID)
        boxes[name] = [{"bbox": [float(xs.min()), float(ys.min()), float(xs.max() + 1 - xs.min()), float(ys.max() + 1 - ys.min())], "category_id": 0, "score": 0.9}]
    with open(os.path.join(out, "boxes.json"), "w") as f:
        json.dump(boxes, f)
    with open(os.path.join(out, "labels.json"), "w") as f:
        json.dump({n: ["box"] for n in boxes}, f)
    base = (f"python demo/demo_geo.py --config-file configs/OVMono3D_dinov2_SFP.yaml --input-folder {out}/in --labels-file {out}/labels.json "
            f"--boxes-file {out}/boxes.json --depth files --depth-dir {out}/maps --mask box --focal-length {float(K[0, 0])!r} --principal-point {float(K[0, 2])!r} {float(K[1, 2])!r} "
            "--stage-times")
    print(base + f" OUTPUT_DIR {out}/level")
    print(base + f" MODEL.AMD.GEO_UPRIGHT True OUTPUT_DIR {out}/upright")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick", action="store_true", help="also time the numpy restatement of the same steps on the host, once, and compare")
    ap.add_argument("--write-demo-inputs", metavar="DIR", default="", help="write three rooms for demo/demo_geo.py --stage-times and print its command lines; no timing")
    a = ap.parse_args()
    if a.write_demo_inputs:
        write_demo_inputs(a.write_demo_inputs)
        return
    if a.runs < 7:
        ap.error("--runs must be at least 7 (the figure is a median)")
    import torch
    assert torch.cuda.is_available(), "the kernels need the GPU"
    dev = torch.device("cuda", 0)
    for H, W in SIZES:
        for stride in STRIDES:
            bench_set(H, W, stride, a, dev)


if __name__ == "__main__":
    main()
