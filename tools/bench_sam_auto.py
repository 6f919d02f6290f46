#!/usr/bin/env python3
"""Times SAM's automatic mask generation (ovmono3d_amd.sam.SamAutomaticMaskGenerator; csrc/sam.hip: ovm_sam_auto_candidates,
sam_mask_stats_kernel, ovm_sam_auto_select) per stage, synthetic weights, a 32 x 32 grid, on a 1080 x 1920 and a 480 x 640 image.

    python tools/bench_sam_auto.py [--arch vit_b] [--points-per-side 32] [--runs 5] [--warmup 2] [--sizes 1080x1920,480x640] [--keep 100] [--yardstick]

Stages, HIP event times around the calls alone (inputs resident, no read inside), warm, median of the runs:
    set_image     resize, encoder, neck
    candidates    ovm_sam_auto_candidates over the grid in batches of 64 points: decoder + mask statistics + rows (pred_iou_thresh 0:
                  every plane is counted, the most the stage can cost)
    stats         the statistics kernel alone (ovm_op_sam_mask_stats) on the same low-resolution logits, 192 planes per call
    decoder       candidates - stats
    select        ovm_sam_auto_select (filters + NMS) on the table
    emission      predict_prompts for the kept (point, plane) pairs + mask_boxes
    generate      generate_device, everything including its one read

Synthetic weights give near-whole-image masks, of which segment_anything's thresholds keep one. The selection and the emission are
therefore timed at thresholds set from the table so that --keep (100) masks survive: pred_iou_thresh = the (keep + 1)-th largest IoU
prediction, the stability filter off, box_nms_thresh 1.0 (nothing suppressed). The kept count is printed.

``--yardstick``: the same table from the calls the library had before this generator plus eager torch on the same card:
predict_prompts(want_iou, want_lowres) in batches of 64, F.interpolate twice, the three counts and the boxes in torch
(yardstick_stats), the filters in torch and ovm_op_nms (yardstick_select). Its counts are compared with the fused table's.
One JSON line per image size.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ovmono3d_amd.sam import CAND_WORDS, SamAutomaticMaskGenerator, build_sam, candidate_fields  # noqa: E402
from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict  # noqa: E402

BATCH = 64


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


def torch_stats(low, S, nh, nw, H, W, offset):
    """low [n, L, L] -> (cnt_hi, cnt_mid, cnt_lo int32 [n], inclusive boxes int32 [n, 4]) in eager torch: the image-size logits exist"""
    v = F.interpolate(low[:, None], (S, S), mode="bilinear", align_corners=False)[..., :nh, :nw]
    v = F.interpolate(v, (H, W), mode="bilinear", align_corners=False)[:, 0]
    m = v > 0
    hi, mid, lo = (v > offset).sum((1, 2)), m.sum((1, 2)), (v > -offset).sum((1, 2))
    rows, cols = m.any(2).to(torch.int32), m.any(1).to(torch.int32)
    y0, y1 = rows.argmax(1), H - 1 - rows.flip(1).argmax(1)
    x0, x1 = cols.argmax(1), W - 1 - cols.flip(1).argmax(1)
    box = torch.stack([x0, y0, x1, y1], 1) * (mid > 0)[:, None]
    return hi.int(), mid.int(), lo.int(), box.int()


def bench_size(a, pred, H, W, dev):
    import sam_oracle as so
    eng, lib = pred.engine, pred.engine.L
    img = torch.from_numpy(so.test_image(H, W, seed=4)).to(dev)
    gen = SamAutomaticMaskGenerator(pred, points_per_side=a.points_per_side, points_per_batch=BATCH)
    out = {"arch": a.arch, "image": [H, W], "points": a.points_per_side ** 2, "batch": BATCH}
    out["set_image_ms"] = event_ms(lambda: pred.set_image(img), a.runs, a.warmup)
    pts = torch.from_numpy(gen.grid_points(H, W)).to(dev)
    n = pts.shape[0]
    table = torch.empty((3 * n, CAND_WORDS), dtype=torch.int32, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)                                # noqa: E731

    def candidates():
        for b0 in range(0, n, BATCH):
            eng.auto_candidates(pts[b0:b0 + BATCH], 0.0, 1.0, out=table[3 * b0:3 * min(n, b0 + BATCH)])

    out["candidates_ms"] = event_ms(candidates, a.runs, a.warmup)
    # the statistics kernel alone, on one batch's real logits (every batch has the same shape)
    ones = torch.ones((BATCH, 1), dtype=torch.int32, device=dev)
    nb = min(BATCH, n)
    _, iou0, low0 = eng.predict_prompts(pts[:nb].reshape(-1, 1, 2).contiguous(), ones[:nb], None, None, H, W, want_iou=True, want_lowres=True)
    Ls, S = low0.shape[-1], eng.cfg.image_size
    scale = S / max(H, W)
    nh, nw = int(H * scale + 0.5), int(W * scale + 0.5)
    st = torch.empty((3 * nb, 7), dtype=torch.int32, device=dev)
    calls = (n + BATCH - 1) // BATCH

    def stats():
        for _ in range(calls):
            rc = lib.ovm_op_sam_mask_stats(low0.data_ptr(), Ls * Ls, 3 * nb, Ls, S, nh, nw, H, W, 1.0, None, st.data_ptr(), stream())
            assert rc == 0

    out["stats_ms"] = event_ms(stats, a.runs, a.warmup)
    out["decoder_ms"] = round(out["candidates_ms"] - out["stats_ms"], 3)
    out["stats_pixel_evaluations"] = 3 * n * H * W                                                  # a count, not a measurement
    ious = np.sort(candidate_fields(table)["iou"])[::-1]
    pthr, sthr, nthr = float(ious[min(a.keep, len(ious) - 1)]), 0.0, 1.0
    gen.pred_iou_thresh, gen.stability_score_thresh, gen.box_nms_thresh = pthr, sthr, nthr
    out["thresholds"] = [round(pthr, 4), sthr, nthr]
    out["select_ms"] = event_ms(lambda: eng.auto_select(table, pthr, sthr, nthr), a.runs, a.warmup)
    res = gen.generate_device(img)
    m = int(res["index"].numel())
    out["kept"] = m
    keep = res["index"]
    lab = torch.ones((max(m, 1), 1), dtype=torch.int32, device=dev)
    idx = keep.cpu().numpy()

    def emission():
        masks = torch.empty((m, H, W), dtype=torch.uint8, device=dev)
        for k in range(3):
            rows = np.nonzero(idx % 3 == k)[0]
            if len(rows):
                sel = torch.from_numpy(rows).to(dev)
                masks[sel] = eng.predict_prompts(pts[keep[sel] // 3].reshape(-1, 1, 2).contiguous(), lab[:len(rows)], None, None, H, W, mask_index=k)[0]
        return eng.mask_boxes(masks)

    out["emission_ms"] = event_ms(emission, a.runs, a.warmup) if m else 0.0
    out["generate_ms"] = event_ms(lambda: gen.generate_device(img), a.runs, a.warmup)
    if a.yardstick:
        pred.set_image(img)
        f = candidate_fields(table)
        lows, ious = [], []

        def y_decode():
            lows.clear(), ious.clear()
            for b0 in range(0, n, BATCH):
                p = pts[b0:b0 + BATCH].reshape(-1, 1, 2).contiguous()
                _, i, l = eng.predict_prompts(p, ones[:p.shape[0]], None, None, H, W, want_iou=True, want_lowres=True)
                lows.append(l), ious.append(i)

        out["yardstick_decoder_ms"] = event_ms(y_decode, a.runs, a.warmup)
        ystats = []

        def y_stats():
            ystats.clear()
            for l in lows:
                ystats.append(torch_stats(l.reshape(-1, Ls, Ls), S, nh, nw, H, W, 1.0))

        out["yardstick_stats_ms"] = event_ms(y_stats, a.runs, a.warmup)
        hi, mid, lo, box = (torch.cat([s[k] for s in ystats]) for k in range(4))
        iou = torch.cat(ious).reshape(-1)
        keep_y, nk = torch.empty((3 * n,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)

        def y_select():
            ok = iou > pthr                                              # the stability filter is off (its threshold is 0)
            rows = ok.nonzero()[:, 0]
            b, s = box[rows].float().contiguous(), iou[rows].contiguous()
            rc = lib.ovm_op_nms(b.data_ptr(), s.data_ptr(), int(rows.numel()), nthr, keep_y.data_ptr(), nk.data_ptr(), stream())
            assert rc == 0
            return rows

        out["yardstick_select_ms"] = event_ms(y_select, a.runs, a.warmup)
        rows = y_select()
        torch.cuda.synchronize()
        out["yardstick_kept"] = int(nk.item())
        out["yardstick_same_keep_list"] = bool(rows[keep_y[:int(nk.item())].long()].cpu().numpy().tolist() == idx.tolist())
        diff = np.abs(np.stack([hi.cpu().numpy() - f["cnt_hi"], mid.cpu().numpy() - f["area"], lo.cpu().numpy() - f["cnt_lo"]]))
        out["yardstick_count_diff_max_pixels"] = int(diff.max())
        out["stats_speedup"] = round(out["yardstick_stats_ms"] / out["stats_ms"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="vit_b")
    ap.add_argument("--points-per-side", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1080x1920,480x640")
    ap.add_argument("--keep", type=int, default=100, help="masks the timed selection and emission keep (thresholds set from the table)")
    ap.add_argument("--yardstick", action="store_true", help="also time the table from predict_prompts + eager torch + ovm_op_nms")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the generator needs the GPU"
    dev = torch.device("cuda", 0)
    sd = synth_sam_predictor_state_dict(a.arch, seed=5)
    pred = build_sam(a.arch, sd, device=dev, max_boxes=BATCH)
    with torch.no_grad():
        for size in a.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            bench_size(a, pred, H, W, dev)


if __name__ == "__main__":
    main()
