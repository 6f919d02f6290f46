"""Plain restatement of the kernels between the GEMMs (csrc/roi_cube.hip, csrc/elementwise.hip), with the inputs and the comparison
that tests/test_gpu_roi_glue.py runs against the ovm_op_* entry points and tests/test_roi_glue_ref_cpu.py checks on the CPU.

Everything is numpy (torch only for erf). Every arithmetic op takes `dtype`: float64 is the reference, float32 is "the fp32 run" whose
distance from the reference (E32) sets the tolerance:

    a kernel passes if  max |got - fp64|  <=  4 * E32 + one fp32 ulp of the largest |fp64| value            (`bound`)

per ROI row, per record field and row, or per case (LayerNorm, LN + GELU, patch gather). The factor 4 is the one the SAM and Depth Pro
stage tests use (a different summation order); the ulp covers the case E32 == 0. Inputs are fp32 (or fp16 pairs, uint8) and enter
both runs with the same values. An op whose output is a split pair ends, in its fp32 run, with split() - that is its definition
(common.hpp) - so E32 carries the 2^-22 the format drops; the fp64 run returns the unrounded value. Outputs that are hi alone (one-pass
mode, lo == NULL) cannot meet an fp32 bound: see `bound_hi_only`.

Layouts are written from their definitions: split(x) = (fp16_rn(x), fp16_rn(x - float(hi))); interleaved image column
il_col(k) = (k // 32) * 64 + k % 32 with lo 32 further; bordered image pixel (y + 1, x + 1) of [B][H + 2][W + 2].
"""
from __future__ import annotations

import math

import numpy as np
import torch

SENTINEL = 7.5                     # exact in fp16 and fp32; none of the ops below can produce it from the inputs used
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ formats
def split(x):
    """fp32 -> (hi, lo) fp16, exact by definition."""
    x = np.asarray(x, dtype=F32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(F32)).astype(np.float16)
    return hi, lo


def join(hi, lo=None):
    v = np.asarray(hi, dtype=np.float16).astype(F64)
    return v if lo is None else v + np.asarray(lo, dtype=np.float16).astype(F64)


def render(y, dtype):
    """The value an output of the fp32 run holds once stored as a split pair; the fp64 run stays unrounded."""
    return join(*split(y)) if dtype == F32 else np.asarray(y, dtype=F64)


def il_col(k):
    return (k // 32) * 64 + k % 32


def ulp32(v):
    return float(np.spacing(F32(np.max(np.abs(v))))) if np.size(v) else 0.0


def bound(ref64, ref32):
    """(E32, tolerance) of one field."""
    e32 = float(np.max(np.abs(np.asarray(ref32, dtype=F64) - ref64))) if np.size(ref64) else 0.0
    return e32, 4.0 * e32 + ulp32(ref64)


def bound_hi_only(ref64, ref32):
    """Per-element tolerance of an output stored as one fp16 (lo == NULL): the fp32 bound plus half the fp16 spacing at that element,
    which is what round-to-nearest of a value inside the fp32 bound can add. ref32 is the unrounded fp32 run."""
    e32, tol = bound(ref64, ref32)
    return e32, tol + 0.5 * np.spacing(np.abs(ref64).astype(np.float16)).astype(F64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ ROIAlign
def roi_level_arg(boxes, dtype):
    """4 + log2(sqrt(area) / 224 + 1e-8) of detectron2's assign_boxes_to_levels, before floor and clamp (NaN for a negative area)."""
    b = np.asarray(boxes, dtype=F32).astype(dtype)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        size = np.sqrt(area)
        return dtype(4) + np.log2(size / dtype(224) + dtype(1e-8))


def roi_levels(boxes, min_level, max_level, dtype):
    """Level index (0 = min_level) per box; -1 where the rule is undefined (negative area)."""
    t = roi_level_arg(boxes, dtype)
    lv = np.clip(np.floor(np.where(np.isnan(t), min_level, t)), min_level, max_level).astype(np.int64) - min_level
    return np.where(np.isnan(t), -1, lv)


def roi_align(feats, scales, boxes, idx, levels, out, dtype, margins=None):
    """torchvision roi_align(aligned=True, sampling_ratio=0) of box r on feats[levels[r]][idx[r]] (NHWC) -> [n][out*out*C] in (ph, pw, c)
    order. margins (dict): receives the closest approach of any quantity to a point where the result jumps - the bin size to an
    integer (the sample grid is its ceiling) and a sample coordinate to -1 or to the level's size (where a sample drops out)."""
    n, C = len(boxes), feats[0].shape[-1]
    res = np.zeros((n, out * out * C), dtype=dtype)
    for r in range(n):
        l = max(int(levels[r]), 0)
        f = feats[l][int(idx[r])].astype(dtype)
        H, W = f.shape[:2]
        sc = dtype(F32(scales[l]))
        x1, y1, x2, y2 = (dtype(F32(v)) * sc - dtype(0.5) for v in boxes[r])
        roi_w, roi_h = x2 - x1, y2 - y1
        bin_w, bin_h = roi_w / dtype(out), roi_h / dtype(out)
        gh, gw = int(math.ceil(bin_h)), int(math.ceil(bin_w))
        if gh <= 0 or gw <= 0:
            continue
        if margins is not None:
            margins["grid"] = min([margins.get("grid", 1.0)] + [abs(float(v) - round(float(v))) for v in (bin_h, bin_w)])
        acc = np.zeros((out, out, C), dtype=dtype)
        for ph in range(out):
            for iy in range(gh):
                yy = y1 + dtype(ph) * bin_h + (dtype(iy) + dtype(0.5)) * bin_h / dtype(gh)
                if margins is not None:
                    margins["edge"] = min(margins.get("edge", 1.0), abs(float(yy) + 1.0), abs(float(yy) - H))
                if yy < -1 or yy > H:
                    continue
                y = max(yy, dtype(0))
                yl = int(y)
                if yl >= H - 1:
                    yl = yh = H - 1
                    y = dtype(yl)
                else:
                    yh = yl + 1
                ly = y - dtype(yl)
                for pw in range(out):
                    for ix in range(gw):
                        xx = x1 + dtype(pw) * bin_w + (dtype(ix) + dtype(0.5)) * bin_w / dtype(gw)
                        if margins is not None and ph == 0 and iy == 0:
                            margins["edge"] = min(margins["edge"], abs(float(xx) + 1.0), abs(float(xx) - W))
                        if xx < -1 or xx > W:
                            continue
                        x = max(xx, dtype(0))
                        xl = int(x)
                        if xl >= W - 1:
                            xl = xh = W - 1
                            x = dtype(xl)
                        else:
                            xh = xl + 1
                        lx = x - dtype(xl)
                        hy, hx = dtype(1) - ly, dtype(1) - lx
                        acc[ph, pw] += hy * hx * f[yl, xl] + hy * lx * f[yl, xh] + ly * hx * f[yh, xl] + ly * lx * f[yh, xh]
        res[r] = (acc / dtype(max(gh * gw, 1))).reshape(-1)
    return res


# ------------------------------------------------------------------------------------------------ cube decode
FIELDS = (("box", 0, 4), ("score", 4, 5), ("bbox3D", 6, 30), ("center_cam", 30, 33), ("center_2D", 33, 35), ("dimensions", 35, 38),
          ("pose", 38, 47))            # float columns of the 48-word record; words 5 (class) and 47 (image) are int32


def _unit(v, dtype):
    return v / max(np.sqrt((v * v).sum()), dtype(1e-12))          # F.normalize


def cube_decode(head, boxes, scores, idx, metas, virtual_focal, postprocess, dtype):
    """ROIHeads3D._forward_cube's eval tail (Z direct, 6D allocentric pose, virtual depth) + detector_postprocess, one box at a time.
    head [n][>= 13] = deltas(2) dims(3) pose6(6) z uncertainty. Returns (rec [n][48] in dtype with the int words zero, keep [n])."""
    f = dtype
    n = len(boxes)
    rec = np.zeros((n, 48), dtype=dtype)
    keep = np.zeros(n, dtype=np.int32)
    for i in range(n):
        m = metas[int(idx[i])]
        K = [f(F32(v)) for v in m["K"]]
        ratio = f(F32(m["oh"] / m["h"]))                               # im_scales_ratio, an fp32 input of the kernel
        fx, fy, cx, cy = K[0] / ratio, K[4] / ratio, K[2] / ratio, K[5] / ratio
        hgt = f(m["h"])
        v2r = (hgt * K[4]) / (f(F32(virtual_focal)) * (hgt * ratio))
        hd = np.asarray(head[i], dtype=F32).astype(dtype)
        bx1, by1, bx2, by2 = (f(F32(v)) for v in boxes[i])
        sw, sh = bx2 - bx1, by2 - by1
        u = bx1 + f(0.5) * sw + sw * hd[0]
        v = by1 + f(0.5) * sh + sh * hd[1]
        dims = np.exp(np.minimum(hd[2:5], f(5)))
        b1 = _unit(hd[5:8], f)
        a2 = hd[8:11]
        b2 = _unit(a2 - (b1 * a2).sum() * b1, f)
        R = np.stack([b1, b2, np.cross(b1, b2)]).astype(dtype)
        ray = np.array([(u - cx) / fx, (v - cy) / fy, f(1)], dtype=dtype)
        ray = ray / np.sqrt((ray * ray).sum())
        angle = np.arccos(ray[2])
        if angle > 0:
            axis = np.array([-ray[1], ray[0], f(0)], dtype=dtype)
            aa = angle * axis / np.sqrt((axis * axis).sum())
            ang = np.sqrt((aa * aa).sum())
            s = (f(0.5) - ang * ang / f(48)) if abs(ang) < 1e-6 else np.sin(ang * f(0.5)) / ang
            qr, (qi, qj, qk) = np.cos(ang * f(0.5)), aa * s
            t = f(2) / (qr * qr + qi * qi + qj * qj + qk * qk)
            M = np.array([[1 - t * (qj * qj + qk * qk), t * (qi * qj - qk * qr), t * (qi * qk + qj * qr)],
                          [t * (qi * qj + qk * qr), 1 - t * (qi * qi + qk * qk), t * (qj * qk - qi * qr)],
                          [t * (qi * qk - qj * qr), t * (qj * qk + qi * qr), 1 - t * (qi * qi + qj * qj)]], dtype=dtype)
            R = (M @ R).astype(dtype)
        z = hd[11] * v2r
        x3, y3 = z * (u - cx) / fx, z * (v - cy) / fy
        unc = max(hd[12], f(F32(0.01)))                               # the clip value as fp32 torch and the kernel hold it
        ow, oh = f(m["ow"]), f(m["oh"])
        sx, sy = ow / f(m["w"]), oh / f(m["h"])
        ox1, ox2 = (min(max(b * sx, f(0)), ow) for b in (bx1, bx2))
        oy1, oy2 = (min(max(b * sy, f(0)), oh) for b in (by1, by2))
        rec[i, 0:4] = (ox1, oy1, ox2, oy2) if postprocess else (bx1, by1, bx2, by2)
        rec[i, 4] = np.sqrt(f(F32(scores[i])) * np.exp(-unc))
        for c in range(8):          # corners: X = -+l/2 (0, 3, 4, 7 negative), Y = -+h/2 (0, 1, 4, 5 negative), Z = -+w/2 (0..3 negative)
            p = np.array([(-1 if c in (0, 3, 4, 7) else 1) * dims[2], (-1 if c in (0, 1, 4, 5) else 1) * dims[1],
                          (-1 if c < 4 else 1) * dims[0]], dtype=dtype) * f(0.5)
            rec[i, 6 + 3 * c:9 + 3 * c] = R @ p + np.array([x3, y3, z], dtype=dtype)
        rec[i, 30:33] = (x3, y3, z)
        rec[i, 33:35] = (u * ratio, v * ratio)
        rec[i, 35:38] = dims
        rec[i, 38:47] = R.reshape(-1)
        keep[i] = 1 if (not postprocess or ((ox2 - ox1) > 0 and (oy2 - oy1) > 0)) else 0
    return rec, keep


# ------------------------------------------------------------------------------------------------ compaction
def compact_records(rec, keep, B):
    """rec [n][48] (any 4-byte dtype; word 47 viewed as int32 is the image) -> (kept rows in order, kept rows per image)."""
    sel = np.asarray(keep) != 0
    img = np.ascontiguousarray(rec[:, 47]).view(np.int32)
    return rec[sel], np.bincount(img[sel], minlength=B).astype(np.int32)


# ------------------------------------------------------------------------------------------------ LayerNorm, GELU
def layer_norm(x, gamma, beta, eps, dtype):
    x = np.asarray(x).astype(dtype)
    mean = x.mean(axis=-1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(F32(eps))) * np.asarray(gamma, F32).astype(dtype) + np.asarray(beta, F32).astype(dtype)


def gelu(z):
    z = np.asarray(z)
    return (0.5 * z * (1.0 + torch.erf(torch.from_numpy(z / z.dtype.type(math.sqrt(2.0)))).numpy())).astype(z.dtype)


def ln_gelu(hi, lo, gamma, beta, eps, dtype):
    """gelu(LayerNorm(hi + lo)) of split rows (lo None: hi alone); hi + lo is exact in fp32."""
    return gelu(layer_norm(join(hi, lo), gamma, beta, eps, dtype))


def bordered_rows(B, H, W):
    """Row of a [B][H + 2][W + 2] image that holds pixel (b, y, x), for rows m = (b*H + y)*W + x."""
    m = np.arange(B * H * W)
    x, y, b = m % W, (m // W) % H, m // (W * H)
    return (b * (H + 2) + y + 1) * (W + 2) + x + 1


# ------------------------------------------------------------------------------------------------ patch gather
def patch_gather(imgs, G, P, Kpad, mean, std, dtype):
    """imgs: uint8 arrays [H][W][3] (any memory layout) -> rows [B G^2][Kpad], column (py*P + px)*3 + c = (u8 - mean[c]) / std[c];
    zero outside the image (the pad value 0 applies after normalisation) and in columns 3 P^2 .. Kpad - 1."""
    out = np.zeros((len(imgs) * G * G, Kpad), dtype=dtype)
    mean, std = np.asarray(mean, F32).astype(dtype), np.asarray(std, F32).astype(dtype)
    for b, im in enumerate(imgs):
        H, W = im.shape[:2]
        for gy in range(G):
            for gx in range(G):
                for py in range(P):
                    for px in range(P):
                        y, x = gy * P + py, gx * P + px
                        if y < H and x < W:
                            k = (py * P + px) * 3
                            out[(b * G + gy) * G + gx, k:k + 3] = (im[y, x].astype(dtype) - mean) / std
    return out


def patch_rows_f32(views, G):
    """views: fp32 arrays [16 G][16 G][3] -> rows [B G^2][768] of the same values (to be split as they are)."""
    out = np.zeros((len(views) * G * G, 768), dtype=F32)
    for b, v in enumerate(views):
        for gy in range(G):
            for gx in range(G):
                out[(b * G + gy) * G + gx] = v[gy * 16:gy * 16 + 16, gx * 16:gx * 16 + 16].reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ re-layouts
def tokens_cast(X, G2, ldo, depth):
    """X [B][T][D] -> fp32 rows [B G2][ldo] to be split: the last G2 tokens, then (ldo > D) the depth column and zeros."""
    B, T, D = X.shape
    out = np.zeros((B * G2, ldo), dtype=F32)
    out[:, :D] = X[:, T - G2:].reshape(B * G2, D)
    if ldo > D and depth is not None:
        out[:, D] = depth
    return out


def tokens_writeback(X, Fm, G2):
    B, T, D = X.shape
    Y = X.copy()
    Y[:, T - G2:] = Fm.reshape(B, G2, D)
    return Y


def cls_init(X, cls, pos, reg, R):
    Y = X.copy()
    Y[:, 0] = cls + pos[0]
    for r in range(R):
        Y[:, 1 + r] = reg[r]
    return Y


def maxpool2(x):
    """[B][G][G][D] -> [B][G//2][G//2][D]; an odd last row and column are dropped."""
    B, G, _, D = x.shape
    Go = G // 2
    out = np.empty((B, Go, Go, D), dtype=x.dtype)
    for yo in range(Go):
        for xo in range(Go):
            out[:, yo, xo] = x[:, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].reshape(B, 4, D).max(axis=1)
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
LEVEL_SIDES = (56.0, 112.0, 224.0, 448.0, 896.0)
LEVEL_BOUNDARIES = (112.0, 224.0, 448.0)
LEVEL_HW = ((232, 240), (116, 120), (58, 60), (29, 30))          # strides 4, 8, 16, 32: each level holds every box below whole
LEVEL_SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)


def level_boxes():
    """Squares on and 0.1 % either side of the ROIPooler's level boundaries, and 56 x 224 (area 112^2). The corner (8, 16) and the
    sides on a boundary are small integers, so the fp32 area is exact and the square root of a power-of-four multiple is too."""
    sides = list(LEVEL_SIDES) + [s * k for s in LEVEL_BOUNDARIES for k in (0.999, 1.001)]
    b = [[8.0, 16.0, 8.0 + s, 16.0 + s] for s in sides] + [[8.0, 16.0, 8.0 + 56.0, 16.0 + 224.0]]
    return np.asarray(b, dtype=F32)


VAL_HW = ((40, 36), (20, 18), (72, 68))                          # levels 2, 3, 4 of the value test: different, non-square
VAL_SCALES = (1 / 4, 1 / 8, 1 / 16)


def value_boxes():
    """Boxes of the ROIAlign value test, images interleaved 1, 0, 1, 0, ... Row 11 has x2 < x1 (level undefined)."""
    b = [[5.0, 5.0, 5.0, 9.0],                    # zero width
         [-50.0, -50.0, 400.0, 400.0],            # far outside on every side
         [10.0, 10.0, 10.5, 10.5],                # sub-pixel
         [20.3, 16.6, 1050.9, 1046.2],            # level 4: 64.4 x 64.35 feature pixels, 10 x 10 samples per bin at out = 7
         [-30.2, 20.4, 40.7, 90.3],               # 7.5 feature pixels over the left border (level 2, scale 1/4)
         [20.6, -30.8, 90.1, 40.3],               # over the top
         [100.4, 20.7, 170.2, 90.9],              # 6.5 over the right border of the 36-wide level
         [20.2, 120.3, 90.7, 190.6],              # 7.6 over the bottom border of the 40-high level
         [-300.0, -300.0, -200.5, -210.0],        # wholly outside
         [31.7, 47.2, 64.9, 71.3],                # ordinary neighbours of the degenerate rows
         [12.3, 8.9, 150.2, 141.5],                # level 3
         [90.0, 20.0, 30.0, 70.0],                # x2 < x1: zeros
         [33.3, 21.1, 97.0, 133.7]]
    b = np.asarray(b, dtype=F32)
    return b, (np.arange(len(b)) + 1).astype(np.int32) % 2


def value_feats(C, seed=0):
    g = np.random.default_rng(100 + seed)
    return [g.standard_normal((2, h, w, C)).astype(F32) for h, w in VAL_HW]


def decode_inputs(n, ldh, seed=0):
    """Two images of different ratio and K; image 0 has ratio 2 and principal point (320, 240), so K[2] / ratio = 160 and
    K[5] / ratio = 120 are exact. The special rows are written first (n = 1 keeps the on-principal-point row); the rest are random.
    a2 parallel to a1 comes twice: `a2_parallel_exact` (a1 = (2, 0, 0), a2 = (3, 0, 0), on the principal point) leaves b2 = a2 - (b1 . a2) b1
    exactly zero in any arithmetic, so R = [b1; 0; 0] is defined and compared; `a2_parallel` (a2 = 2 a1, a1 random) leaves rounding noise
    that F.normalize blows up to a unit vector - fp64, fp32 numpy and the kernel (which contracts to FMAs) each get another one, so its
    pose and corners have no reference value and are only required to be finite; its other fields are compared as usual."""
    g = np.random.default_rng(200 + seed)
    metas = [dict(h=240, w=320, oh=480, ow=640, K=[900.0, 0, 320.0, 0, 900.0, 240.0, 0, 0, 1]),
             dict(h=532, w=400, oh=512, ow=385, K=[1024.0, 0, 190.5, 0, 1000.0, 256.25, 0, 0, 1])]
    head = (g.standard_normal((n, ldh)) * 0.5).astype(F32)
    head[:, 11] = 1.0 + g.random(n) * 3
    head[:, 12] = g.standard_normal(n)
    x1, y1 = g.random(n) * 200, g.random(n) * 150
    boxes = np.stack([x1, y1, x1 + 20 + g.random(n) * 90, y1 + 20 + g.random(n) * 60], 1).astype(F32)
    idx = (np.arange(n) % 3 == 1).astype(np.int32)
    names = {}

    def row(i, name, box=None, image=None, **cols):
        if i >= n:
            return
        names[i] = name
        if box is not None:
            boxes[i] = box
        if image is not None:
            idx[i] = image
        for c, v in cols.items():
            head[i, int(c[1:])] = v

    on_pp = [150.0, 100.0, 170.0, 140.0]              # centre (160, 120) = the scaled principal point of image 0
    row(0, "on_pp", on_pp, 0, c0=0.0, c1=0.0)
    row(1, "off_1e-3", [150.0, 100.0, 170.0, 140.0], 0, c0=1e-3 / 20, c1=0.0)
    row(2, "off_0.1", [150.0, 100.0, 170.0, 140.0], 0, c0=0.0, c1=0.1 / 40)
    row(3, "off_1", [150.0, 100.0, 170.0, 140.0], 0, c0=1.0 / 20, c1=0.0)
    row(4, "a1_zero", c5=0.0, c6=0.0, c7=0.0)
    row(5, "a2_parallel_exact", on_pp, 0, c0=0.0, c1=0.0, c5=2.0, c6=0.0, c7=0.0, c8=3.0, c9=0.0, c10=0.0)
    if n > 6:
        head[6, 8:11] = 2.0 * head[6, 5:8]
        names[6] = "a2_parallel"
    row(7, "uncert_low", c12=0.003)
    row(8, "dims_at_5", c2=5.0, c3=5.0, c4=5.0)
    row(9, "dims_above_5", c2=5.5, c3=9.0, c4=7.25)
    row(10, "neg_z", c11=-2.5)
    row(11, "empty_x", [330.0, 50.0, 390.0, 90.0], 0)             # right of the 320-wide image 0: empty after the clip in x only
    row(12, "empty_y", [50.0, 540.0, 120.0, 600.0], 1)            # below the 532-high image 1: empty in y only
    row(13, "on_pp_far_pose", on_pp, 0, c0=0.0, c1=0.0, c5=0.3, c6=-1.2, c7=0.8, c8=1.1, c9=0.4, c10=-0.6)
    scores = g.random(n).astype(F32)
    classes = g.integers(0, 50, n).astype(np.int32)
    return dict(head=head, boxes=boxes, scores=scores, classes=classes, idx=idx, metas=metas, names=names)


COMPACT_N = (1, 64, 1023, 1024, 1025, 2500)
COMPACT_KEEP = ("all", "none", "alternating", "random", "last")


def compact_inputs(n, pattern, seed=0):
    """Records of random 32-bit words with image indices over B = 3 of which image 1 owns none."""
    g = np.random.default_rng(300 + n + seed)
    rec = g.integers(0, 2 ** 32, (n, 48), dtype=np.uint32)
    rec[:, 47] = 2 * g.integers(0, 2, n).astype(np.uint32)
    keep = {"all": np.ones(n), "none": np.zeros(n), "alternating": np.arange(n) % 2, "random": g.integers(0, 2, n),
            "last": np.arange(n) == n - 1}[pattern].astype(np.int32)
    keep[keep != 0] = g.integers(1, 5, int((keep != 0).sum()))          # any non-zero value keeps
    return rec, keep


LN_D = (4, 252, 256, 260, 1024, 1028, 1536, 2048)
LN_M = (1, 5, 7)
LN_ROWS = ("ordinary", "offset", "constant")


def ln_inputs(M, D, rows, seed=0):
    g = np.random.default_rng(400 + D + 7 * M + seed)
    if rows == "ordinary":
        x = g.standard_normal((M, D)) * 2 + 0.5
    elif rows == "offset":
        x = 1000 + 0.01 * g.standard_normal((M, D))
    else:
        x = np.repeat(g.standard_normal((M, 1)) * 3, D, axis=1)
    return x.astype(F32), (g.random(D) + 0.5).astype(F32), g.standard_normal(D).astype(F32)


PATCH_CASES = ((14, 3, 640), (16, 2, 768))                       # (patch, G, Kpad): 640 is the engine's K for the 588 columns of patch 14
PIXEL_MEAN, PIXEL_STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)


def patch_images(seed=0):
    """Two images of sizes no patch divides, 30 x 37 and 42 x 29: each leaves part of the 42 (patch 14) and of the 32 (patch 16) canvas
    empty, and on the 32 canvas each is also cut on its longer side. Logical [H][W][3]; the GPU test stores the first CHW, the second NHWC."""
    g = np.random.default_rng(500 + seed)
    return [g.integers(0, 256, (30, 37, 3), dtype=np.uint8), g.integers(0, 256, (42, 29, 3), dtype=np.uint8)]


def maxpool_inputs(G, seed=0):
    """fp32 [2][G][G][8] whose first windows hold: an exact tie with a larger third value of the same hi part (lo decides) and a
    fourth below it; an all-negative window; elsewhere random values of both signs."""
    g = np.random.default_rng(600 + G + seed)
    x = (g.standard_normal((2, G, G, 8)) * 2).astype(F32)
    x[0, 0, 0] = x[0, 0, 1] = 1.5 + 2.0 ** -14
    x[0, 1, 0] = 1.5 + 2.0 ** -13
    x[0, 1, 1] = 1.5 - 2.0 ** -13
    x[0, 0:2, 2:4] = -np.abs(x[0, 0:2, 2:4]) - 0.25
    x[1, 2:4, 0:2] = x[1, 2, 0]                                     # a window of four equal values
    return x
