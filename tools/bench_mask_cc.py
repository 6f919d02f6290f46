#!/usr/bin/env python3
"""Times connected components and the small-region clean-up on the device (ovm_mask_cc_label, ovm_mask_remove_small_regions;
csrc/mask_cc.hip) at 1080 x 1920:

  blobs          64 planes of tests/mask_cc_oracle.blobs (a generator of this project: six ellipses per plane with 40 specks and 40
                 pinholes of 1 - 9 pixels; seeds 0 .. 63) - what SAM masks look like to the clean-up
  checkerboard   one plane; under 4-connectivity every pixel is its own component (H W / 2 labels)
  serpentine     one plane; a one-pixel path through every row, the longest chain of unions
  noise0.593     one plane of noise at the site-percolation density

Per set: ``label8_ms`` / ``label4_ms`` (ovm_mask_cc_label) and ``clean_ms`` (ovm_mask_remove_small_regions, mode 3, min_area 100) -
device time between two HIP events around the C call alone (workspace and outputs allocated before), warm, the median of ``--runs``
(at least 7) after ``--warmup`` calls; ``status`` is read once after the timing. With ``--yardstick`` also the host route on the same
planes, wall clock, once: ``cpu()`` of the planes, scipy.ndimage.label, and the numpy clean-up of tests/mask_cc_oracle.py
(``yardstick_copy_ms``, ``yardstick_label8_ms``, ``yardstick_clean_ms``; the clean-up includes its own labelling, not the copy).
One JSON line per set. The plane generators and the yardstick are those of the test tree (tests/mask_cc_oracle.py, which reads
tests/sam_auto_oracle.py): the tool runs from a checkout, not from an installed package.

``--geo``: one more line, the clean-up in front of ``ovm_geo_lift`` on a synthetic 480 x 640 scene - an object of six ellipses at
about 2 m in front of a wall at 6 m, its mask with 40 specks that land on the wall and 40 pinholes (tests/mask_cc_oracle.blobs) -
lifted from the raw and from the cleaned plane (``remove_small_regions(m, 100, "both")``): the DBSCAN trials run (the accepted trial,
or all of them on the fallback), the points kept, the box's dimensions, and the device time of the lift and of the clean-up.
"""
import argparse
import ctypes as C
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

import mask_cc_oracle as O  # noqa: E402

from ovmono3d_amd import lib as _lib  # noqa: E402

H, W = 1080, 1920
MIN_AREA = 100


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
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def bench_set(name, planes, a, dev):
    L = _lib.load()
    n = int(planes.shape[0])
    d = torch.from_numpy(planes).to(dev)
    need_l, need_c = C.c_int64(), C.c_int64()
    assert L.ovm_mask_cc_label_workspace(n, H, W, C.byref(need_l)) == 0 and L.ovm_mask_remove_small_regions_workspace(n, H, W, C.byref(need_c)) == 0
    ws = torch.empty(max(need_l.value, need_c.value), dtype=torch.uint8, device=dev)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    changed = torch.empty((n,), dtype=torch.int32, device=dev)
    status = torch.zeros((4,), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def label(conn):
        rc = L.ovm_mask_cc_label(d.data_ptr(), d.stride(0), d.stride(1), n, H, W, conn, 0, labels.data_ptr(), labels.stride(0), labels.stride(1),
                                 counts.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0

    def clean():
        rc = L.ovm_mask_remove_small_regions(d.data_ptr(), d.stride(0), d.stride(1), n, H, W, MIN_AREA, 3, out.data_ptr(), out.stride(0), out.stride(1),
                                             changed.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0

    res = {"set": name, "planes": n, "size": [H, W], "runs": a.runs, "warmup": a.warmup, "workspace_mb": round(ws.numel() / 2 ** 20, 1)}
    for key, fn in (("label8", lambda: label(8)), ("label4", lambda: label(4)), ("clean", clean)):
        med, lo, hi = event_ms(fn, a.runs, a.warmup)
        res[key + "_ms"], res[key + "_min_max_ms"] = med, [lo, hi]
        assert status.cpu().tolist()[0] == 0, (name, key, status.cpu().tolist())
    label(8)
    res["components8"] = int(counts.sum())
    res["planes_changed"] = int((changed != 0).sum())
    res["label8_gpix_s"] = round(n * H * W / res["label8_ms"] / 1e6, 2)
    if a.yardstick:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = d.cpu().numpy()
        t1 = time.perf_counter()
        ref = [O.label(p, 8) for p in host]
        t2 = time.perf_counter()
        O._regions.cache_clear()
        cleaned = [O.remove_small_regions(p, MIN_AREA, "both") for p in host]
        t3 = time.perf_counter()
        res["yardstick_copy_ms"], res["yardstick_label8_ms"], res["yardstick_clean_ms"] = (round((y - x) * 1e3, 1) for x, y in ((t0, t1), (t1, t2), (t2, t3)))
        got = labels.cpu().numpy()
        assert all(np.array_equal(got[i], ref[i][0]) for i in range(n)) and counts.cpu().tolist() == [r[1] for r in ref]
        clean()
        o, c = out.cpu().numpy(), changed.cpu().tolist()
        assert all(np.array_equal(o[i], cleaned[i][0]) and bool(c[i]) == cleaned[i][1] for i in range(n))
        res["equal_to_yardstick"] = True
    print(json.dumps(res), flush=True)


def bench_geo(a, dev):
    from ovmono3d_amd import geo
    from ovmono3d_amd.masks import remove_small_regions
    h, w = 480, 640
    mask = O.blobs(h, w, seed=3)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    solid, _ = O.remove_small_regions(mask, MIN_AREA, "both")                # the object itself: the wall is everything else
    depth = np.where(solid != 0, 2.0 + 0.0004 * xx + 0.0002 * yy, 6.0 + 0.0005 * xx).astype(np.float32)
    K = np.array([[600.0, 0.0, w / 2], [0.0, 600.0, h / 2], [0.0, 0.0, 1.0]])
    d, m = torch.from_numpy(depth).to(dev), torch.from_numpy(mask[None]).to(dev)
    params = geo.GeoParams()
    res = {"set": "geo_scene", "size": [h, w], "min_area": MIN_AREA, "runs": a.runs, "warmup": a.warmup}
    res["clean_ms"] = event_ms(lambda: remove_small_regions(m, MIN_AREA, "both"), a.runs, a.warmup)[0]
    cleaned = remove_small_regions(m, MIN_AREA, "both")[0]
    for key, plane in (("raw", m[0]), ("clean", cleaned[0])):
        r = geo.lift(d, K, masks=[plane], params=params)[0][0]
        box = geo.host_box(r, K) if r.status == 0 else None
        call = geo.LiftCall(d, K, None, [plane], params, False)            # prepared once (it counts the mask's pixels): launch() alone is timed
        res[key] = {"mask_pixels": int(plane.ne(0).sum()), "status": int(r.status), "accepted_trial": int(r.trial),
                    "trials_run": int(r.trial) if r.trial else params.trials, "points_used": int(r.n_used), "points_kept": int(r.n_kept),
                    "dimensions": [round(v, 4) for v in box["dimensions"]] if box else None,
                    "lift_ms": event_ms(call.launch, a.runs, a.warmup)[0]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blob-planes", type=int, default=64)
    ap.add_argument("--geo", action="store_true", help="also lift a synthetic scene from its raw and its cleaned mask: DBSCAN trials, points kept, times")
    ap.add_argument("--yardstick", action="store_true", help="also time cpu() + scipy.ndimage.label + the numpy clean-up on the same planes, and compare")
    a = ap.parse_args()
    if a.runs < 7:
        ap.error("--runs must be at least 7 (the figure is a median)")
    assert torch.cuda.is_available(), "the kernels need the GPU"
    dev = torch.device("cuda", 0)
    bench_set("blobs", np.stack([O.blobs(H, W, seed=s) for s in range(a.blob_planes)]), a, dev)
    for name, plane in (("checkerboard", O.checkerboard(H, W)), ("serpentine", O.serpentine(H, W)), ("noise0.593", O.noise(H, W, 0.593))):
        bench_set(name, plane[None], a, dev)
    if a.geo:
        bench_geo(a, dev)


if __name__ == "__main__":
    main()
