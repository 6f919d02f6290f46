"""The checker of SAM's automatic mask generation (ovmono3d_amd.sam.SamAutomaticMaskGenerator; csrc/sam.hip: sam_mask_stats_kernel,
ovm_sam_auto_candidates, ovm_sam_auto_select): numpy restatements of segment_anything's automatic_mask_generator.py / utils/amg.py
rules as include/ovm3d.h states them, the cases of the mask-statistics kernel, and the comparison of its counts against fp64.

The package segment_anything is not installed: the rules are restated from its description, and where Hugging Face transformers'
SAM image processor has a helper for the same rule (the point grid, the stability score, the mask's box), tests/test_sam_auto_cpu.py
checks the restatement against it.

The comparison of a count against fp64 (`check_counts`): the device evaluates the resampled logit v in fp32, so a pixel whose fp64
value lies within `band` of a threshold t may fall on either side. For t in {-offset, 0, +offset}:

    count64(v > t + band)  <=  device count  <=  count64(v > t - band)

with band = sam_dp_glue_ref.band_of(r64, r32), the project's factor times the fp32 restatement's own error (never a chosen number), and
at most MAX_LEFT_OUT (1 %) of a plane's pixels within `band` of any of the three thresholds, so that the interval says something.
"""
from __future__ import annotations

import numpy as np

import sam_dp_glue_ref as G
from sam_dp_glue_ref import F32, F64, MAX_LEFT_OUT  # noqa: F401  (re-exported to the tests)

WORDS = 16                       # an OvmSamCandidate as int32 words
SKIPPED = 1                      # OVM_SAM_CAND_SKIPPED
MAX_ROWS = 4096                  # rows the NMS takes
OFFSET = 1.0                     # stability_score_offset


# ------------------------------------------------------------------------------------------------ the grid
def point_grid(n):
    """[n * n, 2] float64 (x, y) in [0, 1]^2: offset = 1 / (2 n), g = linspace(offset, 1 - offset, n), point i * n + j = (g[j], g[i])"""
    off = 1.0 / (2 * n)
    g = np.linspace(off, 1.0 - off, n, dtype=F64)
    out = np.zeros((n * n, 2), F64)
    for i in range(n):
        for j in range(n):
            out[i * n + j] = (g[j], g[i])
    return out


def grid_points(n, H, W):
    """The grid in the pixels of an H x W image (x scaled by W, y by H, in float64), as the float32 the device receives"""
    p = point_grid(n)
    return np.stack([p[:, 0] * W, p[:, 1] * H], axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------ statistics of full-size logits
def plane_stats(v, offset=OFFSET):
    """v [H][W] logits -> (cnt_hi, cnt_mid, cnt_lo, [xmin, ymin, xmax, ymax]); the box is inclusive, zeros for an empty mask"""
    v = np.asarray(v)
    m = v > 0
    ys, xs = np.nonzero(m)
    box = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if len(ys) else [0, 0, 0, 0]
    return int((v > offset).sum()), int(m.sum()), int((v > -offset).sum()), box


def stability(cnt_hi, cnt_lo):
    """float32(cnt_hi) / float32(cnt_lo); 0 / 0 is NaN"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(cnt_hi).astype(F32) / np.asarray(cnt_lo).astype(F32)).astype(F32)


def left_out_share(v64, band, offset=OFFSET):
    """share of the plane's pixels within `band` of -offset, 0 or +offset"""
    v64 = np.asarray(v64, F64)
    near = np.zeros(v64.shape, bool)
    for t in (-offset, 0.0, offset):
        near |= np.abs(v64 - t) <= band
    return float(near.mean())


def check_counts(counts, v64, band, offset=OFFSET, tag=""):
    """counts = (cnt_hi, cnt_mid, cnt_lo) of the device for one plane; v64 its fp64 logits. Asserts the condition and the three intervals."""
    share = left_out_share(v64, band, offset)
    assert share <= MAX_LEFT_OUT, f"{tag}: {share:.3%} of the pixels lie within the band {band:.2e} of a threshold"
    for name, got, t in zip(("cnt_hi", "cnt_mid", "cnt_lo"), counts, (offset, 0.0, -offset)):
        lo, hi = int((v64 > t + band).sum()), int((v64 > t - band).sum())
        assert lo <= int(got) <= hi, f"{tag}: {name} = {int(got)} outside [{lo}, {hi}] (threshold {t:+.1f}, band {band:.2e})"
    return share


# ------------------------------------------------------------------------------------------------ filters and NMS
def table(iou, stability_, boxes, flags=None, area=None):
    """A candidate table as named arrays (the fields `select` reads)"""
    m = len(iou)
    return dict(iou=np.asarray(iou, F32), stability=np.asarray(stability_, F32), box=np.asarray(boxes, np.int32).reshape(m, 4),
                flags=np.zeros(m, np.int32) if flags is None else np.asarray(flags, np.int32),
                area=np.zeros(m, np.int32) if area is None else np.asarray(area, np.int32))


def pack(t):
    """The table as OvmSamCandidate rows: int32 [m][16]"""
    m = len(t["iou"])
    out = np.zeros((m, WORDS), np.int32)
    out[:, 0] = np.asarray(t["iou"], F32).view(np.int32)
    out[:, 1] = np.asarray(t["stability"], F32).view(np.int32)
    out[:, 2] = t["area"]
    out[:, 3:7] = t["box"]
    out[:, 9] = t["flags"]
    return out


def box_iou_gt(a, b, thr):
    """torchvision's test in float32 on the inclusive boxes as floats: inter / (area_a + area_b - inter) > thr; 0 / 0 is not greater"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    w = max(min(a[2], b[2]) - max(a[0], b[0]), F32(0))
    h = max(min(a[3], b[3]) - max(a[1], b[1]), F32(0))
    inter = F32(w * h)
    aa, ab = F32((a[2] - a[0]) * (a[3] - a[1])), F32((b[2] - b[0]) * (b[3] - b[1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return bool(F32(inter / F32(F32(aa + ab) - inter)) > F32(thr))


def valid_rows(t, pred_iou_thresh, stability_score_thresh):
    iou, stab = np.asarray(t["iou"], F32), np.asarray(t["stability"], F32)
    ok = ((np.asarray(t["flags"]) & SKIPPED) == 0) & ~np.isnan(iou)
    with np.errstate(invalid="ignore"):
        if pred_iou_thresh > 0:
            ok &= iou > F32(pred_iou_thresh)                     # strict
        if stability_score_thresh > 0:
            ok &= stab >= F32(stability_score_thresh)            # not strict; NaN fails
    return ok


def select(t, pred_iou_thresh, stability_score_thresh, box_nms_thresh):
    """The kept candidate indices in keep order: both filters (each only when its threshold is > 0), then greedy NMS by decreasing
    iou, ties to the lower index, suppression at IoU > box_nms_thresh."""
    if len(t["iou"]) > MAX_ROWS:
        raise ValueError("more rows than the NMS takes")
    ok = valid_rows(t, pred_iou_thresh, stability_score_thresh)
    idx = [i for i in range(len(ok)) if ok[i]]
    idx.sort(key=lambda i: (-float(t["iou"][i]), i))
    boxes = np.asarray(t["box"], np.int32).astype(F32)
    area = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).astype(F32)
    keep, thr = [], F32(box_nms_thresh)
    for i in idx:
        if keep:                                                 # box_iou_gt of every kept box against box i, as arrays
            k, b = boxes[keep], boxes[i]
            w = np.maximum(np.minimum(k[:, 2], b[2]) - np.maximum(k[:, 0], b[0]), F32(0))
            h = np.maximum(np.minimum(k[:, 3], b[3]) - np.maximum(k[:, 1], b[1]), F32(0))
            inter = (w * h).astype(F32)
            with np.errstate(invalid="ignore", divide="ignore"):
                if np.any((inter / ((area[keep] + area[i]).astype(F32) - inter).astype(F32)).astype(F32) > thr):
                    continue
        keep.append(i)
    return np.asarray(keep, np.int64)


# ------------------------------------------------------------------------------------------------ the statistics kernel's cases
STATS_GEOMETRIES = [dict(hw=hw, L=32, S=128) for hw in ((23, 31), (31, 23), (5, 3), (61, 97), (70, 100), (99, 71))] + [dict(hw=(61, 97), L=64, S=256)]
STATS_SMOOTH = 3                 # smooth planes per geometry
STATS_MUTATIONS = ("out_hw_swapped", "out_crop_ignored", "offset_sign_flipped")
CRAFTED = ("empty", "full", "between", "one_cell")


def stats_id(case):
    return f"{case['hw'][0]}x{case['hw'][1]}-L{case['L']}-S{case['S']}"


def stats_inputs(case):
    """{'smooth': fp32 [3][L][L] of amplitude about 10 (all three thresholds cut it), 'crafted': fp32 [4][L][L] in CRAFTED's order}"""
    L = case["L"]
    g = np.random.default_rng(1000 * case["hw"][0] + 10 * case["hw"][1] + L)
    smooth = G.smooth_field(g, STATS_SMOOTH, L, 10.0)
    crafted = np.zeros((len(CRAFTED), L, L), F32)
    crafted[0] = -5.0                                            # all below -offset: every count 0, stability 0 / 0
    crafted[1] = 5.0                                             # all above +offset
    crafted[2] = 0.5                                             # between 0 and +offset: cnt_hi 0, cnt_mid = cnt_lo = H W
    crafted[3] = -5.0
    crafted[3, L // 3, L // 2] = 200.0                           # one positive low-resolution cell, high enough to reach an output pixel at every geometry
    return dict(smooth=smooth, crafted=crafted)


def stats_logits(case, planes, dtype, mut=None):
    """postprocess_masks of `planes` [n][L][L] at the case's geometry in `dtype`: [n][H][W]"""
    (H, W), S = case["hw"], case["S"]
    nh, nw = G.preprocess_shape(H, W, S)
    return G.mask_logits(planes, S, nh, nw, H, W, dtype, mut if mut in ("out_hw_swapped", "out_crop_ignored") else None)


def as_device(v32, offset=OFFSET, mut=None):
    """The seven words per plane of a device that evaluated exactly v32 [n][H][W] (mut offset_sign_flipped: with the offset negated)"""
    off = -offset if mut == "offset_sign_flipped" else offset
    rows = []
    for v in v32:
        hi, mid, lo, box = plane_stats(v, off)
        rows.append([hi, mid, lo] + box)
    return np.asarray(rows, np.int32)
