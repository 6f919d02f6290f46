"""The checker of the SAM predictor's point, box + point and mask-input prompts and of its single-mask output: the cases, the
Hugging Face ``SamModel`` driver (tests/sam_oracle.py builds the model) and numpy restatements of the three prompt kernels of
csrc/sam.hip (point tokens, mask embedding; the image -> token attention is tests/sam_dp_glue_ref.py's).

The HF call is the per-prompt batch form: the image embedding repeated n times, points [n, 1, P, 2], labels [n, 1, P], boxes
[n, 1, 4], mask inputs [n, 1, L, L]. Every prompt of a case has the same shape, as one ``ovm_sam_predict`` call has.

A case's ``mask_from`` names the case whose fp64 low-resolution logits (plane 2, rounded to fp32 once) are fed back as its mask
input: the refinement pass segment_anything documents. The fp64 run, the fp32 run and the device all receive those same values.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

import roi_glue_ref as R
import sam_dp_glue_ref as G
import sam_oracle as so
from roi_glue_ref import F32, F64

# TINY's image is 70 x 100 (H x W). Coordinates are (x, y) in original pixels, exactly representable in fp32.
CASES = {
    # one click per prompt: foreground, foreground on the image border (the last column and row), background
    "points1": dict(points=[[[35.0, 30.0]], [[99.0, 69.0]], [[60.0, 50.0]]], labels=[[1], [1], [0]]),
    # three clicks: foreground / background / padding in every order a user produces
    "points3": dict(points=[[[30.0, 20.0], [80.0, 55.0], [0.0, 0.0]], [[70.5, 35.25], [20.0, 60.0], [50.0, 10.0]]],
                    labels=[[1, 0, -1], [1, 1, 0]]),
    # a box with two clicks (no padding token)
    "box_points2": dict(points=[[[45.0, 35.0], [25.0, 20.0]], [[10.0, 10.0], [90.0, 60.0]]], labels=[[1, 0], [0, 1]],
                        boxes=[[20.0, 15.0, 70.0, 55.0], [0.0, 0.0, 100.0, 70.0]]),
    # the box prompts of two of TINY's boxes, refined with their own previous logits
    "box": dict(boxes=[[20.0, 15.0, 70.0, 55.0], [-10.0, -5.0, 60.0, 90.0]]),
    "box_mask": dict(boxes=[[20.0, 15.0, 70.0, 55.0], [-10.0, -5.0, 60.0, 90.0]], mask_from="box"),
    "points1_mask": dict(points=[[[35.0, 30.0]], [[99.0, 69.0]], [[60.0, 50.0]]], labels=[[1], [1], [0]], mask_from="points1"),
    # the single-mask output (mask token 0, IoU column 0), three clicks
    "points3_single": dict(points=[[[30.0, 20.0], [80.0, 55.0], [0.0, 0.0]], [[70.5, 35.25], [20.0, 60.0], [50.0, 10.0]]],
                           labels=[[1, 0, -1], [1, 1, 0]], multimask=False),
    # the most one prompt takes: eight clicks and a box, 15 tokens
    "box_points8": dict(points=[[[30.0, 20.0], [40.0, 30.0], [50.0, 40.0], [60.0, 50.0], [25.0, 50.0], [65.0, 20.0], [5.0, 5.0], [95.0, 65.0]],
                                [[10.0, 60.0], [20.0, 50.0], [30.0, 40.0], [40.0, 30.0], [50.0, 20.0], [60.0, 10.0], [90.0, 5.0], [0.0, 0.0]]],
                        labels=[[1, 1, 1, 1, 0, 0, 0, -1], [1, 0, 1, 0, 1, 0, -1, -1]],
                        boxes=[[20.0, 15.0, 70.0, 55.0], [0.0, 0.0, 100.0, 70.0]]),
}
GPU_CASES = ("points1", "points3", "box_points2", "box_mask", "points1_mask", "points3_single", "box_points8")     # "box" only feeds box_mask
# PORTRAIT's image is 99 x 71 and its engine takes max_boxes = 2: three prompts run as two chunks, the second chunk's masks at an odd offset
PORTRAIT_CASES = {
    "portrait_points1": dict(points=[[[20.0, 30.0]], [[0.0, 98.0]], [[50.0, 70.0]]], labels=[[1], [1], [0]]),
}
CASES.update(PORTRAIT_CASES)
TINY_CASES = tuple(k for k in CASES if k not in PORTRAIT_CASES)


def case_shape(case):
    """(n, P, has_box, ns, nt)"""
    P = len(case["points"][0]) if "points" in case else 0
    hb = "boxes" in case
    n = len(case["points"]) if P else len(case["boxes"])
    ns = P + (2 if hb else 1)
    return n, P, hb, ns, 5 + ns


@torch.no_grad()
def run(model, image_u8: np.ndarray, case, mask_input: Optional[np.ndarray] = None) -> Dict[str, torch.Tensor]:
    """Every stage the GPU tests compare, in the model's dtype: sparse [n, ns, C], dense [n, G, G, C], tokens [n, nt, C], low
    [n, K, L, L], iou [n, K], logits [n, K, H, W]. mask_input: fp32 [n, L, L] or None."""
    dtype = next(model.parameters()).dtype
    S = model.config.vision_config.image_size
    H, W = image_u8.shape[:2]
    nh, nw = so.preprocess_shape(H, W, S)
    n, P, hb, _, _ = case_shape(case)
    pts = lab = bt = mk = None
    if P:
        c = np.asarray(case["points"], np.float64).copy()                      # ResizeLongestSide.apply_coords, fp64 as numpy does it
        c[..., 0] *= nw / W
        c[..., 1] *= nh / H
        pts = torch.from_numpy(c.reshape(n, 1, P, 2)).to(dtype)
        lab = torch.tensor(case["labels"], dtype=torch.int64).reshape(n, 1, P)
    if hb:
        b = np.asarray(case["boxes"], np.float64).reshape(-1, 2, 2).copy()
        b[..., 0] *= nw / W
        b[..., 1] *= nh / H
        bt = torch.from_numpy(b.reshape(n, 1, 4)).to(dtype)
    if mask_input is not None:
        mk = torch.from_numpy(np.asarray(mask_input, np.float32)).to(dtype)[:, None]
    got = {}
    hook = model.mask_decoder.transformer.register_forward_hook(lambda mod, args, out: got.__setitem__("tokens", out[0]))
    try:
        emb = model.get_image_embeddings(so.preprocess(image_u8, S, False, dtype)).expand(n, -1, -1, -1)
        out = model(image_embeddings=emb, input_points=pts, input_labels=lab, input_boxes=bt, input_masks=mk,
                    multimask_output=case.get("multimask", True))
    finally:
        hook.remove()
    sparse, dense = model.prompt_encoder(pts, lab, bt, mk)
    low = out.pred_masks[:, 0]
    return {"sparse": sparse[:, 0], "dense": dense.permute(0, 2, 3, 1).contiguous(), "tokens": got["tokens"][:, 0], "low": low,
            "iou": out.iou_scores[:, 0], "logits": so.postprocess(low, S, (nh, nw), (H, W))}


def reference_set(base=so.TINY, names=None):
    """{case name: (fp64 stages, fp32 stages, mask input | None)}, plus the state dict and the image, for ``base``'s weights and
    image (names: default every case of TINY's image); each HF model is built once. A mask input is plane 2 of the fp64 low-res
    logits of the case ``mask_from`` names."""
    names = TINY_CASES if names is None else names
    sd, img = so.case_inputs(base)
    order = []
    for k in names:                                                           # sources first
        src = CASES[k].get("mask_from")
        for x in ([src] if src else []) + [k]:
            if x not in order:
                order.append(x)
    r64, r32, masks = {}, {}, {}
    m64 = so.build_model(base["arch"], sd, base["image_size"], torch.float64)
    for k in order:
        src = CASES[k].get("mask_from")
        masks[k] = None if src is None else r64[src]["low"][:, 2].to(torch.float32).numpy().copy()
        r64[k] = run(m64, img, CASES[k], masks[k])
    del m64
    m32 = so.build_model(base["arch"], sd, base["image_size"], torch.float32)
    for k in order:
        r32[k] = run(m32, img, CASES[k], masks[k])
    return {k: (r64[k], r32[k], masks[k]) for k in names}, sd, img


# ---- restatements of the kernels (numpy; dtype = F64 for the reference, F32 for the yardstick) ------------------------------------
def point_tokens(points, labels, boxes, out_tokens, gauss, point_emb, not_a_point, corner, H, W, newh, neww, S, dtype):
    """PromptEncoder._embed_points / _embed_boxes behind SamPredictor.predict's apply_coords, and the decoder's token row: per prompt
    [out_tokens (iou, mask tokens), points..., padding (no box) | corner 0, corner 1 (box)]. A point: coordinates * new / old in fp64,
    cast, + 0.5, / S, PE, + point_emb[label] for label 0 / 1; label -1: not_a_point alone. Returns (tok [nb][nout + ns][C], sparse)."""
    cast = lambda a: np.asarray(a, F32).astype(dtype)                                   # noqa: E731
    nout, Cc = out_tokens.shape
    scale = np.array([neww / W, newh / H])
    rows = []
    nb = len(points) if points is not None else len(boxes)
    P = 0 if points is None else np.asarray(points).shape[1]
    if P:
        pts = (np.asarray(points, F32).astype(F64).reshape(nb * P, 2) * scale).astype(dtype)
        enc = G.pe_encode((pts[:, 0] + dtype(0.5)) / dtype(S), (pts[:, 1] + dtype(0.5)) / dtype(S), gauss, dtype).reshape(nb, P, Cc)
        lab = np.asarray(labels).reshape(nb, P)
        pe = cast(point_emb)
        emb = np.where((lab == -1)[..., None], cast(not_a_point)[None, None], enc)
        emb = np.where((lab == 0)[..., None], emb + pe[0], emb)
        emb = np.where((lab == 1)[..., None], emb + pe[1], emb)
        rows.append(emb)
    if boxes is None:
        rows.append(np.broadcast_to(cast(not_a_point)[None, None], (nb, 1, Cc)))
    else:
        c = (np.asarray(boxes, F32).astype(F64).reshape(nb * 2, 2) * scale).astype(dtype)
        enc = G.pe_encode((c[:, 0] + dtype(0.5)) / dtype(S), (c[:, 1] + dtype(0.5)) / dtype(S), gauss, dtype).reshape(nb, 2, Cc)
        rows.append(enc + cast(corner)[None])
    sparse = np.concatenate(rows, axis=1).astype(dtype)
    tok = np.concatenate([np.broadcast_to(cast(out_tokens)[None], (nb, nout, Cc)), sparse], axis=1)
    return tok, sparse


def mask_embed(mask, w, dtype):
    """PromptEncoder.mask_downscaling on mask [n][L][L] -> [n][G*G][C]. w: the ten tensors under their checkpoint names
    ("0.weight" [4][1][2][2], "0.bias", "1.weight", "1.bias", "3.weight" [16][4][2][2], "3.bias", "4.weight", "4.bias", "6.weight"
    [C][16][1][1], "6.bias"). LayerNorm2d: over the channels of a pixel, biased variance, eps 1e-6."""
    cast = lambda a: np.asarray(a, F32).astype(dtype)                                   # noqa: E731
    x = cast(mask)
    n, L, _ = x.shape

    def conv2x2(x, wt, b):                                                             # x [n][h][w][ci] -> [n][h/2][w/2][co]
        n_, h, w_, ci = x.shape
        p = x.reshape(n_, h // 2, 2, w_ // 2, 2, ci)                                    # [n][i][ky][j][kx][ci]
        return np.einsum("niyjxc,ocyx->nijo", p, cast(wt)) + cast(b)

    y = conv2x2(x[..., None], w["0.weight"], w["0.bias"])
    y = R.gelu(R.layer_norm(y, w["1.weight"], w["1.bias"], 1e-6, dtype).astype(dtype))
    y = conv2x2(y, w["3.weight"], w["3.bias"])
    y = R.gelu(R.layer_norm(y, w["4.weight"], w["4.bias"], 1e-6, dtype).astype(dtype))
    w6 = cast(w["6.weight"]).reshape(-1, 16)
    out = y @ w6.T + cast(w["6.bias"])
    return out.reshape(n, (L // 4) ** 2, -1).astype(dtype)


def mask_boxes(masks):
    """(boxes [n][4] = (xmin, ymin, xmax + 1, ymax + 1) float32, counts int32 [n]); zeros for an empty mask."""
    masks = np.asarray(masks)
    boxes, counts = np.zeros((len(masks), 4), F32), np.zeros(len(masks), np.int32)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        counts[i] = len(ys)
        if len(ys):
            boxes[i] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes, counts


MD = "prompt_encoder.mask_downscaling."


def mask_weights(sd):
    return {k[len(MD):]: v.numpy() for k, v in sd.items() if k.startswith(MD)}


# ---- demo/demo_geo.py --points-file: the entries of one image as the tool groups them --------------------------------------------
def group_reference(entries):
    """{(P, has_box): [entry index, ...]} in first-appearance order: the rule of ovmono3d_amd.geo.sources.group_point_prompts restated."""
    out = {}
    for i, e in enumerate(entries):
        out.setdefault((len(e["points"]), "bbox" in e), []).append(i)
    return out

