#!/usr/bin/env python3
"""Times of the device JPEG encoder (profiles/jpeg_encode/README.md) on the pictures the project writes: a 1080 x 3000
``_combine.jpg`` (demo.py on a 1080p input), the six-panel mosaic ``render_panels`` produces for a 416-high input, both drawn by the
project's own renderers from seeded scenes, and the 480 x 640 COCO fixture. Per picture: ``ovm_jpeg_encode`` in HIP events (and
``ovm_jpeg_forward`` alone, stages 1-2), ``encode_jpeg`` end to end on the wall clock (the copy of the bytes included), and today's
path on the same picture and machine: ``tensor.cpu().numpy()`` + channel reverse + ``Image.save`` into a BytesIO. Warm-up first, then
the median of N (default 30). Prints one JSON line; ``python tools/bench_jpeg_encode.py [OUT.json] [N]``."""
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panels_oracle as po  # noqa: E402
import scene_oracle as so  # noqa: E402
from ovmono3d_amd import lib as _lib, vis  # noqa: E402
from ovmono3d_amd.data import gpu_jpeg  # noqa: E402

N = int(sys.argv[2]) if len(sys.argv) > 2 else 30
WARM = 5
QUALITY = 95
if not torch.cuda.is_available():
    raise SystemExit("bench_jpeg_encode.py measures on the HIP device; none found")
dev = torch.device("cuda", 0)
L = _lib.load()


def pictures():
    """(name, device uint8 [H, W, 3] in BGR - the order both call sites hold)."""
    H, W = 1080, 1920
    corners, colors, K, kw = so.make_scene(11, 12, "plain", H, W)
    img = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)).to(dev)
    img = img.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()       # a blocky photograph stand-in, not white noise
    front, novel = vis.draw_scene_view(img, K, corners, colors, text=[f"obj{i} 0.{50 + i}" for i in range(12)], scale=H,
                                       blend_weight=0.5, blend_weight_overlay=0.85, **kw)
    yield "combine_1080x3000", vis.concat_views(front, novel)
    with Image.open(os.path.join(ROOT, "tests", "golden", "coco_000000101762.jpg")) as im:
        coco = np.asarray(im.convert("RGB"))
    h, w = 416, 554                                                               # the COCO fixture at the evaluation's short edge
    small = np.asarray(Image.fromarray(coco).resize((w, h), Image.BILINEAR))
    Kp, gt_all, gt_eval, preds = po.make_scene(4242, 12, 30, h, w)
    yield "panels_832x1662", vis.render_panels(torch.from_numpy(small[:, :, ::-1].copy()).to(dev), Kp, gt_all, gt_eval, preds)
    yield "coco_480x640", torch.from_numpy(coco[:, :, ::-1].copy()).to(dev)


def med(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def device_times(pic):
    """HIP events around ovm_jpeg_encode and around ovm_jpeg_forward, buffers allocated once."""
    info, header, base, sc = gpu_jpeg._encode_plan(pic, QUALITY, "4:2:0", "BGR", True)
    wsb, cap = C.c_int64(), C.c_int64()
    _lib.check(L.ovm_jpeg_encode_workspace(C.byref(info), C.byref(wsb), C.byref(cap)))
    ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=dev)
    out = torch.empty(int(cap.value), dtype=torch.uint8, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    coef = torch.empty((int(info.coef_blocks), 64), dtype=torch.int16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def enc():
        _lib.check(L.ovm_jpeg_encode(base, pic.stride(0), pic.stride(1), sc, C.byref(info), header, ws.data_ptr(), ws.numel(),
                                     out.data_ptr(), out.numel(), n.data_ptr(), stream))

    def fwd():
        _lib.check(L.ovm_jpeg_forward(base, pic.stride(0), pic.stride(1), sc, C.byref(info), ws.data_ptr(), ws.numel(), coef.data_ptr(),
                                      stream))

    res = {}
    for name, fn in (("ovm_jpeg_encode_device", enc), ("ovm_jpeg_forward_device", fwd)):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(N):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        res[name] = med(ts)
    res["workspace_bytes"], res["coef_blocks"] = int(wsb.value), int(info.coef_blocks)
    return res


def host_path(pic):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(pic.cpu().numpy()[:, :, ::-1])).save(b, format="JPEG", quality=QUALITY)
    return b.getvalue()


def device_path(pic):
    return gpu_jpeg.encode_jpeg(pic, quality=QUALITY, channel_order="BGR")


def wall(fn, pic):
    for _ in range(WARM):
        fn(pic)
    ts = []
    for _ in range(N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(pic)
        ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts)


res = {"device": torch.cuda.get_device_name(0), "quality": QUALITY, "subsampling": "4:2:0", "n": N, "warmup": WARM, "pictures": {}}
for name, pic in pictures():
    torch.cuda.synchronize()
    r = {"shape": list(pic.shape), "picture_bytes": int(pic.numel())}
    ref, got = host_path(pic), device_path(pic)
    r["file_bytes"], r["equal_to_pillow"] = len(got), got == ref
    r.update(device_times(pic))
    # the two end-to-end paths alternate, so that whatever else the host is doing falls on both
    a1, b1 = wall(device_path, pic), wall(host_path, pic)
    a2, b2 = wall(device_path, pic), wall(host_path, pic)
    r["encode_jpeg_end_to_end_wall"] = min((a1, a2), key=lambda t: t["median_ms"])
    r["host_copy_and_pillow_wall"] = min((b1, b2), key=lambda t: t["median_ms"])
    r["both_rounds_median_ms"] = {"encode_jpeg": [a1["median_ms"], a2["median_ms"]], "host": [b1["median_ms"], b2["median_ms"]]}
    res["pictures"][name] = r
big = res["pictures"]["combine_1080x3000"]
res["device_path_faster_on_combine"] = big["encode_jpeg_end_to_end_wall"]["median_ms"] < big["host_copy_and_pillow_wall"]["median_ms"]
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
