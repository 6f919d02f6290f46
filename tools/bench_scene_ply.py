#!/usr/bin/env python3
"""Times the point part of <name>_scene.ply (ovmono3d_amd.vis.scene_ply; csrc/scene_ply.hip) on seeded scenes: a smooth depth map
with about 90 % of its pixels valid (the rest NaN, as a depth network's sky or a sensor's holes), a random image, a label map of
eight boxes.

    python tools/bench_scene_ply.py [--runs 9] [--warmup 3] [--cases 768x1024,1536x2048] [--stride 1] [--yardstick]

Warm medians of --runs. One JSON line per case.
    device_ms      HIP event time around ovm_scene_ply_points alone (count, scan, pack; buffers allocated before, nothing read)
    bytes_ms       host clock to bytes in host memory: the call, the 8-byte count read, the copy of 15 P bytes through a pinned buffer
    scene_ply_ms   host clock of vis.scene_ply: bytes_ms plus allocations, the header and the box part
``--yardstick``: the numpy restatement of the same records on host copies of depth, image and labels, including the device-to-host
copies it needs: yardstick_ms (yardstick_copy_ms of it are the three copies); its bytes are compared with the device's.
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

from ovmono3d_amd import lib as ovm_lib  # noqa: E402
from ovmono3d_amd import vis  # noqa: E402
from ovmono3d_amd.vis import ply as vply  # noqa: E402

N_BOXES = 8


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
    return round(statistics.median(ts), 3)


def host_ms(fn, runs, warmup):
    """Host clock around a call whose last step is a read from the device."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def seeded_scene(H, W, dev, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (2.0 + 3.0 * xx / W + 1.5 * yy / H + 0.2 * np.sin(xx / 31.0) * np.cos(yy / 23.0)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.10] = np.nan
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    labels = np.full((H, W), -1, np.int32)
    for b in range(N_BOXES):                                              # rectangles, as --mask box gives them
        y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
        labels[y0:y0 + H // 4, x0:x0 + W // 4] = b
    f = 2.0 * H
    K = np.array([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])
    corners = rng.uniform(-2.0, 6.0, (N_BOXES, 8, 3))
    colors = np.asarray([[c / 255.0 for c in vis.get_color(i)] for i in range(N_BOXES)], np.float32)
    return torch.from_numpy(image).to(dev), torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev), K, corners, colors


def numpy_records(image, depth, labels, K, tint, stride):
    """The rules of include/ovm3d.h ("Scene as a PLY file") on host arrays: the bytes of the P point records."""
    keep = np.zeros(depth.shape, bool)
    keep[::stride, ::stride] = True
    with np.errstate(invalid="ignore"):
        keep &= np.isfinite(depth) & (depth > 0)
    i, j = np.nonzero(keep)
    d = depth[i, j].astype(np.float64)
    rec = np.zeros(len(i), vply._VERTEX)
    rec["xyz"] = np.stack([((j + 0.5) - K[0, 2]) / K[0, 0] * d, ((i + 0.5) - K[1, 2]) / K[1, 1] * d, d], 1).astype(np.float32)
    c = image[i, j].astype(np.int32)
    b = labels[i, j]
    t = (b >= 0) & (b < len(tint))
    c[t] = (c[t] + tint[b[t], :3].astype(np.int32) + 1) >> 1
    rec["rgb"] = c[:, ::-1].astype(np.uint8)
    return rec.tobytes()


def bench_case(a, H, W, dev):
    L = ovm_lib.load()
    image, depth, labels, K, corners, colors = seeded_scene(H, W, dev)
    stride = a.stride
    tint = vply.edge_colors(colors, N_BOXES)
    Kh = np.ascontiguousarray(K.reshape(9))
    worst = -(-H // stride) * -(-W // stride) * vply.RECORD
    ws_bytes = C.c_int64()
    assert L.ovm_scene_ply_points_workspace(H, W, stride, N_BOXES, C.byref(ws_bytes)) == 0
    out = torch.empty(worst, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)

    def call():
        rc = L.ovm_scene_ply_points(image.data_ptr(), image.stride(0), depth.data_ptr(), 4 * depth.stride(0), labels.data_ptr(), 4 * labels.stride(0),
                                    tint.ctypes.data, N_BOXES, H, W, Kh.ctypes.data, stride, 0.0, 0, out.data_ptr(), worst, count.data_ptr(),
                                    ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0

    def to_bytes():
        call()
        P = int(count.item())
        return vply._assemble(b"", out[:vply.RECORD * P], b"")

    res = {"image": [H, W], "stride": stride, "workspace_bytes": int(ws_bytes.value)}
    res["device_ms"] = event_ms(call, a.runs, a.warmup)
    P = int(count.item())
    res["points"], res["valid_share"], res["point_bytes"] = P, round(P / (-(-H // stride) * -(-W // stride)), 3), vply.RECORD * P
    res["bytes_ms"] = host_ms(to_bytes, a.runs, a.warmup)
    full = lambda: vis.scene_ply(image, K, depth=depth, corners=corners, colors=colors, point_labels=labels, stride=stride)   # noqa: E731
    res["scene_ply_ms"] = host_ms(full, a.runs, a.warmup)
    res["file_bytes"] = len(full())
    if a.yardstick:
        def copies():
            return image.cpu().numpy(), depth.cpu().numpy(), labels.cpu().numpy()

        def yardstick():
            return numpy_records(*copies(), K, tint, stride)

        res["yardstick_copy_ms"] = host_ms(copies, a.runs, 1)
        res["yardstick_ms"] = host_ms(yardstick, a.runs, 1)
        res["yardstick_same_bytes"] = bool(yardstick() == to_bytes())
        res["speedup_vs_yardstick"] = round(res["yardstick_ms"] / res["bytes_ms"], 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="768x1024,1536x2048", help="height x width, comma-separated")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--yardstick", action="store_true", help="also time the numpy restatement on host copies, device-to-host copies included")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the point packer needs the GPU"
    dev = torch.device("cuda", 0)
    for case in a.cases.split(","):
        H, W = (int(v) for v in case.split("x"))
        bench_case(a, H, W, dev)


if __name__ == "__main__":
    main()
