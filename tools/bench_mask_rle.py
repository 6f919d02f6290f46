#!/usr/bin/env python3
"""Times the mask outputs (ovmono3d_amd.masks; csrc/mask_rle.hip, csrc/mask_overlay.hip) on seeded --everything-like planes: 100
planes at 1080 x 1920 and 20 planes at 480 x 640, a few ellipses each.

    python tools/bench_mask_rle.py [--runs 5] [--warmup 2] [--cases 100x1080x1920,20x480x640] [--yardstick]

Warm medians of --runs. Device times are HIP event times around the call alone (buffers allocated before, nothing read inside);
end-to-end times are host clock times of a call that ends in its device-to-host read.
    encode_device_ms   ovm_mask_rle_encode alone, buffers of the size the planes need
    encode_ms          masks.encode_rle: workspace, the call, the 16-byte status read, the offsets and the strings' bytes
    decode_ms          masks.decode_rle of those records: strings -> counts on the host, upload, ovm_mask_rle_decode, status read
    decode_device_ms   ovm_mask_rle_decode alone
    dump_npz_ms        what tools/ovmono3d_geo.py --dump-masks does today: planes.cpu() + np.savez_compressed to a file
    dump_rle_ms        the same step with --mask-format rle: encode_rle + json.dump to a file
    load_npz_ms        np.load of that file + upload; load_rle_ms: json.load + decode_rle
    labels_ms          masks.mask_labels; labels_torch_ms: vis.labels_from_masks (eager torch, the n x H x W int32 temporary)
    overlay_ms         masks.overlay_masks from the label map
``--yardstick``: transformers' _mask_to_rle algorithm, restated here in eager torch (the package is imported by tests only), on the
same device tensor: yardstick_ms; its counts are compared with the device coder's. One JSON line per case.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ovmono3d_amd import lib as ovm_lib  # noqa: E402
from ovmono3d_amd import masks as M  # noqa: E402
from ovmono3d_amd import vis  # noqa: E402


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
    """Host clock around a call whose last step is a read from the device (or a file write after one)."""
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


def planes_like_everything(n, H, W, dev, seed=0):
    """uint8 [n, H, W]: per plane one to three seeded ellipses, the sizes of SAM's masks (a few percent to a third of the image)."""
    rng = np.random.RandomState(seed)
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, W)
    out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    for i in range(n):
        for _ in range(rng.randint(1, 4)):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(0.03, 0.3) * H, rng.uniform(0.03, 0.3) * W
            out[i] |= (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).to(torch.uint8)
    return out


def torch_mask_to_rle(input_mask):
    """transformers.models.sam.image_processing_sam._mask_to_rle, restated: bool [n, H, W] on the device -> uncompressed records."""
    n, H, W = input_mask.shape
    flat = input_mask.permute(0, 2, 1).flatten(1)
    change = (flat[:, 1:] ^ flat[:, :-1]).nonzero()
    out = []
    for i in range(n):
        cur = change[change[:, 0] == i, 1] + 1
        if len(cur) == 0:
            out.append({"size": [H, W], "counts": [H * W] if flat[i, 0] == 0 else [0, H * W]})
            continue
        counts = [] if flat[i, 0] == 0 else [0]
        counts += [cur[0].item()] + (cur[1:] - cur[:-1]).tolist() + [H * W - cur[-1].item()]
        out.append({"size": [H, W], "counts": counts})
    return out


def bench_case(a, n, H, W, dev):
    L = ovm_lib.load()
    t = planes_like_everything(n, H, W, dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)                                # noqa: E731
    out = {"planes": n, "image": [H, W], "plane_bytes": n * H * W}
    records = M.encode_rle(t)
    counts = [M.string_to_counts(r["counts"]) for r in records]
    runs, nbytes = sum(len(c) for c in counts), sum(len(r["counts"]) for r in records)
    out["runs"], out["string_bytes"] = runs, nbytes
    # the encode call alone
    ws_bytes = C.c_int64()
    assert L.ovm_mask_rle_encode_workspace(n, H, W, runs, nbytes, C.byref(ws_bytes)) == 0
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    string = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ro, so = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)

    def encode_call():
        rc = L.ovm_mask_rle_encode(t.data_ptr(), t.stride(0), t.stride(1), n, H, W, None, runs, ro.data_ptr(), string.data_ptr(), nbytes, so.data_ptr(),
                                   status.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        assert rc == 0

    out["encode_device_ms"] = event_ms(encode_call, a.runs, a.warmup)
    assert status.cpu().tolist() == [0, runs, nbytes, 0]
    out["encode_workspace_bytes"] = int(ws_bytes.value)
    out["encode_ms"] = host_ms(lambda: M.encode_rle(t), a.runs, a.warmup)
    out["encode_ms_sized"] = host_ms(lambda: M.encode_rle(t, max_runs=runs), a.runs, a.warmup)          # no second call
    out["decode_ms"] = host_ms(lambda: M.decode_rle(records, dev), a.runs, a.warmup)
    assert torch.equal(M.decode_rle(records, dev), t)
    # the decode call alone
    flat = torch.from_numpy(np.asarray([c for cs in counts for c in cs], np.uint32).view(np.int32)).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in counts])]).astype(np.int64)).to(dev)
    assert L.ovm_mask_rle_decode_workspace(n, H, W, runs, C.byref(ws_bytes)) == 0
    dws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    planes = torch.empty_like(t)

    def decode_call():
        rc = L.ovm_mask_rle_decode(flat.data_ptr(), offs.data_ptr(), runs, n, H, W, planes.data_ptr(), planes.stride(0), planes.stride(1), status.data_ptr(),
                                   dws.data_ptr(), dws.numel(), stream())
        assert rc == 0

    out["decode_device_ms"] = event_ms(decode_call, a.runs, a.warmup)
    assert torch.equal(planes, t)
    # today's --dump-masks / --mask-dir step against the RLE one, files included
    with tempfile.TemporaryDirectory() as d:
        npz, rle = os.path.join(d, "m.npz"), os.path.join(d, "m.rle.json")
        index = np.arange(n, dtype=np.int64)

        def dump_npz():
            np.savez_compressed(npz, masks=t.cpu().numpy(), index=index)

        def dump_rle():
            with open(rle, "w") as f:
                json.dump({"index": index.tolist(), "masks": M.encode_rle(t)}, f)

        def load_npz():
            return torch.from_numpy(np.load(npz)["masks"]).to(dev)

        def load_rle():
            with open(rle) as f:
                return M.decode_rle(json.load(f)["masks"], dev)

        out["dump_npz_ms"] = host_ms(dump_npz, a.runs, 1)
        out["dump_rle_ms"] = host_ms(dump_rle, a.runs, a.warmup)
        out["load_npz_ms"] = host_ms(load_npz, a.runs, 1)
        out["load_rle_ms"] = host_ms(load_rle, a.runs, a.warmup)
        out["npz_file_bytes"], out["rle_file_bytes"] = os.path.getsize(npz), os.path.getsize(rle)
        assert torch.equal(load_npz(), load_rle())
    # label map and picture
    out["labels_ms"] = event_ms(lambda: M.mask_labels(t), a.runs, a.warmup)
    out["labels_torch_ms"] = event_ms(lambda: vis.labels_from_masks(t), a.runs, a.warmup)
    labels = M.mask_labels(t)
    assert torch.equal(labels, vis.labels_from_masks(t))
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    colors = [vis.get_color(i) for i in range(n)]
    out["overlay_ms"] = event_ms(lambda: M.overlay_masks(img, labels, colors), a.runs, a.warmup)
    if a.yardstick:
        b = t.bool()
        out["yardstick_ms"] = host_ms(lambda: torch_mask_to_rle(b), a.runs, 1)
        out["yardstick_same_counts"] = bool([r["counts"] for r in torch_mask_to_rle(b)] == counts)
        out["encode_speedup_vs_yardstick"] = round(out["yardstick_ms"] / out["encode_ms"], 1)
    out["dump_speedup_vs_npz"] = round(out["dump_npz_ms"] / out["dump_rle_ms"], 1)
    out["load_speedup_vs_npz"] = round(out["load_npz_ms"] / out["load_rle_ms"], 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="100x1080x1920,20x480x640", help="planes x height x width, comma-separated")
    ap.add_argument("--yardstick", action="store_true", help="also time the _mask_to_rle algorithm in eager torch on the same device tensor")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the mask coder needs the GPU"
    dev = torch.device("cuda", 0)
    for case in a.cases.split(","):
        n, H, W = (int(v) for v in case.split("x"))
        bench_case(a, n, H, W, dev)


if __name__ == "__main__":
    main()
