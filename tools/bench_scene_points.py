#!/usr/bin/env python3
"""Times of the scene view's point cloud (profiles/scene_points/README.md), in HIP events: ``ovm_render_scene`` and
``ovm_render_scene_points`` at ``point_size`` 1 and 3 on one scene - 1080 x 1920 front, 1080 x 1080 novel, 100 labelled boxes, a
depth map through the boxes, every pixel labelled -, each as ``--repeats`` warm medians of ``--iters`` calls, so that the spread of
repeated runs stands beside every figure. ``--lib OTHER.so`` times the render entry points of another build of the library (one
without the point cloud, say) on the layout this build makes. Prints one JSON line; ``--out FILE`` also writes it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_oracle as so  # noqa: E402
from ovmono3d_amd import lib as _lib, vis  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another libovm3d.so whose render entry points are timed")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()

H, W, S, N = 1080, 1920, 1080, 100
corners, colors, K, kw = so.make_scene(77, N, "plain", H, W)
text = [f"obj{i} {((i * 37) % 100) / 100:.2f}" for i in range(N)]
masks = [[vis.text_mask(t, 0.5 * hh / 500) for t in text] for hh in (H, S)]
lay, grid = vis.scene_layout(K, H, W, corners, colors, masks, S, blend_weight=0.5, blend_weight_overlay=0.85, **kw)
glyphs = np.ascontiguousarray(np.concatenate([m.reshape(-1) for v in masks for m in v]), np.uint8)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
img = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
ii, jj = np.mgrid[0:H, 0:W]
depth = torch.from_numpy((8.0 + 4.0 * (jj / W - 0.5) + 6.0 * (0.5 - ii / H) + rng.uniform(-0.5, 0.5, (H, W))).astype(np.float32)).to(dev)
labels = torch.from_numpy(rng.integers(-1, N, (H, W)).astype(np.int32)).to(dev)
both = torch.empty((H, W + S, 3), dtype=torch.uint8, device=dev)
front, novel = both[:, :W], both[:, W:]
Rn = (C.c_double * 9)(*so.euler2mat([np.pi / 3, 0, 0]).reshape(-1).tolist())
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

T = _lib.load()
if args.lib:
    T = _lib.bind(C.CDLL(os.path.abspath(args.lib)), partial=True)
has_points = hasattr(T, "ovm_render_scene_points")
wsb = C.c_int64()
_lib.check((T.ovm_render_scene_points_workspace if has_points else T.ovm_render_scene_workspace)(C.byref(lay), glyphs.size, C.byref(wsb)))
ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=dev)
head = (C.byref(lay), grid.ctypes.data, glyphs.ctypes.data, glyphs.size, img.data_ptr(), img.stride(0), front.data_ptr(), both.stride(0),
        novel.data_ptr(), both.stride(0))


def plain():
    _lib.check(T.ovm_render_scene(*head, ws.data_ptr(), ws.numel(), stream))


def points(ps):
    def call():
        _lib.check(T.ovm_render_scene_points(*head, depth.data_ptr(), 4 * W, labels.data_ptr(), 4 * W, C.byref(Rn), ps, None, ws.data_ptr(),
                                             ws.numel(), stream))
    return call


def medians(call):
    out = []
    for _ in range(args.repeats):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        out.append(round(statistics.median(ev), 4))
    return out


res = {"H": H, "W": W, "scale": S, "n_boxes": N, "n_grid": int(lay.n_grid), "device": torch.cuda.get_device_name(0), "lib": args.lib or "this build",
       "iters": args.iters, "render_scene_ms_medians": medians(plain)}
if has_points:
    for ps in (1, 3):
        res[f"render_scene_points_ps{ps}_ms_medians"] = medians(points(ps))
    hit = torch.empty((S, S), dtype=torch.int64, device=dev)
    _lib.check(T.ovm_render_scene_points(*head, depth.data_ptr(), 4 * W, labels.data_ptr(), 4 * W, C.byref(Rn), 3, hit.data_ptr(), ws.data_ptr(),
                                         ws.numel(), stream))
    torch.cuda.synchronize()
    res["novel_pixels_with_a_point_ps3"] = int((hit != -1).sum())
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
