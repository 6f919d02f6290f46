#!/usr/bin/env python3
"""Times of the evaluation sample panels (profiles/evalvis/README.md): ``ovm_render_panels`` in HIP events, one sample of
``visualize_from_instances`` end to end, and the numpy restatement tests/panels_oracle.py on the same scene. Prints one JSON line;
``python tools/bench_evalvis.py [OUT.json]``."""
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panels_oracle as po  # noqa: E402
from ovmono3d_amd import lib as _lib, vis  # noqa: E402

H, W, NGT, NPRED = 375, 1242, 30, 100
K, gt_all, gt_eval, preds = po.make_scene(4242, NGT, NPRED, H, W)
img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
dev = torch.device("cuda", 0)
d_img = torch.from_numpy(img).to(dev)
res = {"H": H, "W": W, "n_gt": NGT, "n_pred": NPRED, "device": torch.cuda.get_device_name(0)}

t0 = time.perf_counter()
lay, prims, glyphs = vis.panels_layout(K, H, W, gt_all, gt_eval, preds)
res["layout_first_ms"] = (time.perf_counter() - t0) * 1e3                       # includes the Pillow glyph masks
ts = []
for _ in range(20):
    t0 = time.perf_counter()
    vis.panels_layout(K, H, W, gt_all, gt_eval, preds)
    ts.append((time.perf_counter() - t0) * 1e3)
res["layout_ms_median20"] = statistics.median(ts)
res["n_prims"] = int(lay.n_prims)

L = _lib.load()
wsb = C.c_int64()
_lib.check(L.ovm_render_panels_workspace(C.byref(lay), C.byref(wsb)))
ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=dev)
out = torch.empty((2 * H, 3 * W, 3), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def call():
    _lib.check(L.ovm_render_panels(C.byref(lay), prims, glyphs.ctypes.data, glyphs.size, d_img.data_ptr(), d_img.stride(0), out.data_ptr(),
                                   out.stride(0), ws.data_ptr(), ws.numel(), stream))


for _ in range(5):
    call()
torch.cuda.synchronize()
ev = []
for _ in range(20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    ev.append(a.elapsed_time(b))
res["render_panels_device_ms_median20"] = statistics.median(ev)
res["render_panels_device_ms_min"] = min(ev)

# one sample end to end: read the JPEG, boxes, layout, render, download, JPEG encode and write
from PIL import Image  # noqa: E402
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "im.jpg")
Image.fromarray(img[:, :, ::-1].copy()).save(path, quality=90)
names = list(po.NAMES)
annos = [{k: b[k] for k in ("category_id", "bbox", "center_cam", "dimensions", "pose")} for b in gt_all]
insts = [{"category_id": p["category_id"], "score": 0.9 if p.get("draw3d", True) else 0.1, "bbox": p["bbox"],
          "center_2D": [p["bbox"][0] + p["bbox"][2] / 2, p["bbox"][1] + p["bbox"][3] / 2], "center_cam": p["center_cam"],
          "dimensions": p["dimensions"], "pose": p["pose"]} for p in preds]
ds = vis.SampleDataset([{"file_name": path, "image_id": 0, "annotations": annos}])
dets = [{"image_id": 0, "K": K.tolist(), "height": H, "width": W, "instances": insts}]
ts = []
for _ in range(6):
    t0 = time.perf_counter()
    s = vis.visualize_from_instances(dets, ds, "BENCH", 512, tmp, names, names, "final", every=50)
    ts.append((time.perf_counter() - t0) * 1e3)
res["sample_end_to_end_wall_ms_median5_warm"] = statistics.median(ts[1:])
res["sample_end_to_end_wall_ms_first"] = ts[0]
res["log_line"] = s.strip()
shutil.rmtree(tmp, ignore_errors=True)

t0 = time.perf_counter()
ref, band = po.render(img, po.layout(K, H, W, gt_all, gt_eval, preds))
res["numpy_restatement_cpu_ms"] = (time.perf_counter() - t0) * 1e3
dev_out = out.cpu().numpy()
off = (dev_out != ref).any(-1)
res["pixels_differing_outside_band"] = int((off & ~band).sum())
res["band_pixels"] = int(band.sum())
res["band_pixels_differing"] = int((off & band).sum())
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
