#!/usr/bin/env python3
"""Times the SAM predictor (ovm_sam_set_image / ovm_sam_predict_boxes, csrc/sam.hip) on one 1024 x 768 image with 20 box prompts,
synthetic weights, per stage: set_image (resize, encoder, neck) and predict_boxes (prompt encoder, two-way transformer, upscaling,
heads, postprocess_masks to uint8 planes at the image's own resolution).

    python tools/bench_sam.py [--arch vit_b] [--boxes 20] [--runs 7] [--warmup 2] [--precision 3] [--yardstick]
                              [--prompts box|points|box+mask] [--points 1]

``--prompts points`` also times ovm_sam_predict with ``--points`` clicks per prompt (the box centres first, labels 1, no box: one padding
token); ``--prompts box+mask`` the refinement pass (the same boxes with the box pass's plane-2 logits as mask input). Both beside the box
run, same image, same prompt count, inputs resident.

Device times are HIP event times around the calls alone (inputs resident, no read inside), warm, median of the runs. With
``--yardstick`` the same network - Hugging Face SamModel (tests/sam_oracle.py) with the same weights, fp32, eager torch on the same
card - is timed the same way, its stages cut at the same places (the uint8 resize of set_image is not part of it; its
postprocessing is the two F.interpolate calls and the threshold on the device). One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ovmono3d_amd.sam import build_sam  # noqa: E402
from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict  # noqa: E402

H, W = 768, 1024


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
    return statistics.median(ts)


def make_boxes(n, seed=0):
    g = np.random.RandomState(seed)
    x0, y0 = g.uniform(0, W * 0.7, n), g.uniform(0, H * 0.7, n)
    bw, bh = g.uniform(0.05, 0.5, n) * W, g.uniform(0.05, 0.5, n) * H
    return np.stack([x0, y0, np.minimum(x0 + bw, W), np.minimum(y0 + bh, H)], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="vit_b")
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", type=int, default=3, choices=(1, 3))
    ap.add_argument("--max-boxes", type=int, default=32)
    ap.add_argument("--prompts", choices=("box", "points", "box+mask"), default="box", help="a second prompt kind to time beside the boxes")
    ap.add_argument("--points", type=int, default=1, help="--prompts points: clicks per prompt (1..8)")
    ap.add_argument("--yardstick", action="store_true", help="also time Hugging Face SamModel, fp32, eager torch on this card")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the SAM predictor needs the GPU"
    dev = torch.device("cuda", 0)
    import sam_oracle as so
    sd = synth_sam_predictor_state_dict(a.arch, seed=5)
    img_np = so.test_image(H, W, seed=4)
    img = torch.from_numpy(img_np).to(dev)
    boxes = make_boxes(a.boxes)
    bt = torch.from_numpy(boxes).to(dev)
    pred = build_sam(a.arch, sd, device=dev, precision=a.precision, max_boxes=a.max_boxes)
    ws = pred.engine.workspace(a.boxes)
    out = {"arch": a.arch, "image": [H, W], "boxes": a.boxes, "precision": a.precision, "workspace_mb": round(ws.numel() / 2 ** 20, 1)}
    out["set_image_ms"] = round(event_ms(lambda: pred.set_image(img), a.runs, a.warmup), 3)
    out["predict_boxes_ms"] = round(event_ms(lambda: pred.predict_boxes(bt, 2, workspace=ws), a.runs, a.warmup), 3)
    out["predict_per_box_ms"] = round(out["predict_boxes_ms"] / a.boxes, 4)
    masks = pred.predict_boxes(bt, 2, workspace=ws)
    out["mask_fill"] = round(float(masks.float().mean()), 4)
    eng = pred.engine
    if a.prompts == "points":
        g = np.random.RandomState(1)
        pts = np.concatenate([(boxes[:, None, :2] + boxes[:, None, 2:]) / 2, g.uniform(0, 1, (a.boxes, a.points - 1, 2)) * np.array([W, H])], 1)
        pt, lt = torch.from_numpy(pts.astype(np.float32)).to(dev), torch.ones((a.boxes, a.points), dtype=torch.int32, device=dev)
        ws2 = eng.prompt_workspace(a.boxes, a.points, False, False)
        out["points_per_prompt"] = a.points
        out["predict_points_ms"] = round(event_ms(lambda: eng.predict_prompts(pt, lt, None, None, H, W, mask_index=2, workspace=ws2), a.runs, a.warmup), 3)
        out["predict_per_point_prompt_ms"] = round(out["predict_points_ms"] / a.boxes, 4)
    elif a.prompts == "box+mask":
        low = eng.predict_boxes(bt, H, W, 2, want_lowres=True)[2]
        mi = low[:, 2].contiguous()
        ws2 = eng.prompt_workspace(a.boxes, 0, True, True)
        out["predict_box_mask_ms"] = round(event_ms(lambda: eng.predict_prompts(None, None, bt, mi, H, W, mask_index=2, workspace=ws2), a.runs, a.warmup), 3)
        out["predict_per_box_mask_prompt_ms"] = round(out["predict_box_mask_ms"] / a.boxes, 4)
    if a.yardstick:
        import torch.nn.functional as F
        model = so.build_model(a.arch, sd, 1024, torch.float32).to(dev)
        nh, nw = so.preprocess_shape(H, W, 1024)
        pre = so.preprocess(img_np, 1024, False, torch.float32).to(dev)
        sb = boxes.astype(np.float64).reshape(-1, 2, 2).copy()
        sb[..., 0] *= nw / W
        sb[..., 1] *= nh / H
        hb = torch.from_numpy(sb.reshape(1, -1, 4)).float().to(dev)
        with torch.no_grad():
            emb = model.get_image_embeddings(pre)

            def decode():
                low = model(image_embeddings=emb, input_boxes=hb, multimask_output=True).pred_masks[0][:, 2:3]
                m = F.interpolate(low, (1024, 1024), mode="bilinear", align_corners=False)[..., :nh, :nw]
                return (F.interpolate(m, (H, W), mode="bilinear", align_corners=False) > 0).to(torch.uint8)

            out["torch_fp32_set_image_ms"] = round(event_ms(lambda: model.get_image_embeddings(pre), a.runs, a.warmup), 3)
            out["torch_fp32_predict_boxes_ms"] = round(event_ms(decode, a.runs, a.warmup), 3)
            out["masks_equal_torch_fp32"] = round(float((decode()[:, 0] == masks).float().mean()), 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
