"""Plain restatement of the glue kernels of the SAM and Depth Pro engines (csrc/sam.hip, csrc/depthpro.hip), with the inputs, the case
lists and the comparison that tests/test_gpu_sam_dp_glue.py runs against the ovm_op_sam_* / ovm_op_dp_* entry points and
tests/test_sam_dp_glue_ref_cpu.py checks on the CPU (against torch in float64, and against named wrong evaluations: MUTATIONS).

Everything is numpy, written from the operation's definition (segment_anything / Hugging Face / torch semantics), not from the kernels'
arithmetic. Every arithmetic function takes `dtype`: float64 is the reference, float32 is "the fp32 run" whose distance from the
reference (E32) sets the tolerance (roi_glue_ref.bound: 4 * E32 + one fp32 ulp of the largest |fp64|). Bilinear source indices are
computed in `dtype`, as torch computes them in the tensor's own precision. Inputs are fp32 (or fp16 pairs, uint8) and enter both runs
with the same values.

One protocol for every kernel K in KERNELS:
    CASES[K]                     list of dicts (the shapes of the issue's tables)
    inputs(K, case)              dict of numpy inputs in their logical shape
    run(K, case, inp, dtype, mut=None)   dict name -> logical output; `mut` evaluates it wrongly in a named way
    KINDS[K][name]               how `compare` treats that output: "f32" | "split" | "hi" | "exact" | "mask" | "tail"
    mutations_for(K, case)       the mutations that change this case's result
    compare(K, case, got, r64, r32)      asserts; returns {name: (E32, error)}
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import gemm_epi_ref as GE
import roi_glue_ref as R
from roi_glue_ref import F32, F64, SENTINEL, bound, bound_hi_only, join, render, split, ulp32  # noqa: F401  (re-exported to the tests)

MAX_LEFT_OUT = 0.01            # tests/test_gpu_sam.py: share of a mask's pixels that may lie inside the band
K_MAX_TOK = 8                  # tokens per box the image -> token kernel stages

MUTATIONS = ("prod_yx_swapped", "prod_q_bits_swapped", "out_hw_swapped", "out_crop_ignored", "i2t_unscaled", "i2t_head_stride",
             "i2t_next_box_tokens", "box_xy_scale_swapped", "pe_center_off", "merge_first_keeps_pad", "merge_last_short", "pyr_l2_offset",
             "pyr_flip_ignored", "convs2_add_before_relu", "tail_relu1_dropped", "depth_clamp_missing", "depth_fov_radians",
             "border_corner_missed", "ln_gelu_var_biased_by_D64")


# ------------------------------------------------------------------------------------------------ bilinear resampling (torch, align_corners=False)
def taps(out, inn, dtype):
    """Source rows and the weight of the second one for F.interpolate(mode="bilinear", align_corners=False): scale = in / out and
    src = max(scale * (dst + 0.5) - 0.5, 0), all in `dtype`."""
    sc = dtype(inn) / dtype(out)
    src = np.maximum(sc * (np.arange(out).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(src.astype(np.int64), inn - 1)
    i1 = np.minimum(i0 + 1, inn - 1)
    return i0, i1, (src - i0.astype(dtype)).astype(dtype)


def resize(x, oh, ow, dtype):
    """x [H][W][...] -> [oh][ow][...]"""
    x = np.asarray(x).astype(dtype)
    extra = (1,) * (x.ndim - 2)
    y0, y1, ly = taps(oh, x.shape[0], dtype)
    x0, x1, lx = taps(ow, x.shape[1], dtype)
    ly, lx = ly.reshape((-1, 1) + extra), lx.reshape((1, -1) + extra)
    a, b, c, d = x[y0][:, x0], x[y0][:, x1], x[y1][:, x0], x[y1][:, x1]
    one = dtype(1)
    return ((one - ly) * ((one - lx) * a + lx * b) + ly * ((one - lx) * c + lx * d)).astype(dtype)


def preprocess_shape(h, w, S):
    """ResizeLongestSide.get_preprocess_shape"""
    scale = S * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


# ------------------------------------------------------------------------------------------------ SAM
def pe_encode(cx, cy, gauss, dtype):
    """PositionEmbeddingRandom._pe_encoding of points in [0, 1]^2 (cx, cy arrays [n]) -> [n][2 F] = [sin | cos]"""
    g = np.asarray(gauss, F32).astype(dtype)
    x, y = dtype(2) * cx - dtype(1), dtype(2) * cy - dtype(1)
    v = dtype(2 * math.pi) * (x[:, None] * g[0][None] + y[:, None] * g[1][None])
    return np.concatenate([np.sin(v), np.cos(v)], axis=1).astype(dtype)


def dense_pe(gauss, G, dtype, mut=None):
    """get_dense_pe: row i * G + j is the encoding of the cell centre ((j + 0.5) / G, (i + 0.5) / G)"""
    off = dtype(0) if mut == "pe_center_off" else dtype(0.5)
    i, j = np.divmod(np.arange(G * G), G)
    return pe_encode((j.astype(dtype) + off) / dtype(G), (i.astype(dtype) + off) / dtype(G), gauss, dtype)


def box_tokens(boxes, out_tokens, gauss, corner, H, W, newh, neww, S, dtype, mut=None):
    """SamPredictor.predict's box path: apply_boxes (numpy, fp64) -> a tensor of the model's dtype -> _embed_boxes (+ 0.5, / S, encode,
    + point_embeddings[2 + k]); each box's tokens = [iou_token, mask_tokens, corner 0, corner 1]. Returns (tok [nb][nout+2][C], sparse)."""
    nb, (nout, Cc) = len(boxes), out_tokens.shape
    sx, sy = neww / W, newh / H
    if mut == "box_xy_scale_swapped":
        sx, sy = sy, sx
    pts = np.asarray(boxes, F32).astype(F64).reshape(nb * 2, 2) * np.array([sx, sy])
    pts = pts.astype(dtype)
    enc = pe_encode((pts[:, 0] + dtype(0.5)) / dtype(S), (pts[:, 1] + dtype(0.5)) / dtype(S), gauss, dtype)
    sparse = enc.reshape(nb, 2, Cc) + np.asarray(corner, F32).astype(dtype)[None]
    tok = np.concatenate([np.broadcast_to(np.asarray(out_tokens, F32).astype(dtype)[None], (nb, nout, Cc)), sparse], axis=1)
    return tok, sparse


def sam_ln_gelu(x, gamma, beta, eps, dtype, mut=None):
    """LayerNorm2d over the channels of a pixel, then GELU (erf)"""
    if mut == "ln_gelu_var_biased_by_D64":
        x = np.asarray(x).astype(dtype)
        D = x.shape[-1]
        n = dtype(64 * ((D + 63) // 64))
        mean = x.sum(-1, keepdims=True) / n
        var = ((x - mean) ** 2).sum(-1, keepdims=True) / n
        y = (x - mean) / np.sqrt(var + dtype(F32(eps))) * np.asarray(gamma, F32).astype(dtype) + np.asarray(beta, F32).astype(dtype)
        return R.gelu(y.astype(dtype))
    return R.gelu(R.layer_norm(x, gamma, beta, eps, dtype).astype(dtype))


def softmax(s, dtype):
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return (e / e.sum(axis=-1, keepdims=True)).astype(dtype)


def i2t_attn(q, k, v, nt, heads, G2, nb, scale, dtype, mut=None):
    """Attention of the image rows q [nb * G2][heads * 16] over the nt tokens k, v [nb * nt][heads * 16] of their own box."""
    dh = 16
    q, k, v = (np.asarray(a, F32).astype(dtype) for a in (q, k, v))
    sc = dtype(1) if mut == "i2t_unscaled" else dtype(F32(scale))
    ntk = nt
    if mut == "i2t_next_box_tokens":                       # the staging takes kMaxTok rows: the next box's tokens (or what lies behind)
        fill = np.full((K_MAX_TOK, heads * dh), SENTINEL, dtype=dtype)
        k, v, ntk = np.concatenate([k, fill]), np.concatenate([v, fill]), K_MAX_TOK
    out = np.zeros((nb * G2, heads * dh), dtype=dtype)
    for b in range(nb):
        for h in range(heads):
            hk = 0 if mut == "i2t_head_stride" else h
            qq = q[b * G2:(b + 1) * G2, h * dh:(h + 1) * dh]
            kk, vv = (a[b * nt:b * nt + ntk, hk * dh:(hk + 1) * dh] for a in (k, v))
            p = softmax((qq @ kk.T).astype(dtype) * sc, dtype)
            out[b * G2:(b + 1) * G2, h * dh:(h + 1) * dh] = p @ vv
    return out


def unblock(up, nb, G, C8, mut=None):
    """The blocked upscaled map of csrc/sam.hip's header -> [nb][4G][4G][C8]: pixel (4 i + 2 a + a2, 4 j + 2 b + b2) of box n lives at row
    (n * G*G + i * G + j) * 4 + a * 2 + b, columns (a2 * 2 + b2) * C8 .. + C8."""
    L = 4 * G
    U = np.zeros((nb, L, L, C8), dtype=up.dtype)
    for Y in range(L):
        for X in range(L):
            i, a, a2 = Y // 4, (Y % 4) // 2, Y % 2
            j, b, b2 = X // 4, (X % 4) // 2, X % 2
            if mut == "prod_q_bits_swapped":
                a, a2, b, b2 = a2, a, b2, b
            for n in range(nb):
                U[n, Y, X] = up[(n * G * G + i * G + j) * 4 + a * 2 + b, (a2 * 2 + b2) * C8:(a2 * 2 + b2 + 1) * C8]
    return U


def mask_prod(up, hyper, t0, ntk, C8, G, nb, dtype, mut=None):
    """masks[n][t][Y][X] = hyper[n][t0 + t] . upscaled[n][Y][X]; hyper [nb][tokens][C8]"""
    U = unblock(np.asarray(up, F32).astype(dtype), nb, G, C8, mut)
    hy = np.asarray(hyper, F32).astype(dtype)[:, t0:t0 + ntk]
    out = np.einsum("ntc,nyxc->ntyx", hy, U).astype(dtype)
    return out.transpose(0, 1, 3, 2).copy() if mut == "prod_yx_swapped" else out


def mask_logits(logits, S, newh, neww, H, W, dtype, mut=None):
    """Sam.postprocess_masks: logits [nb][L][L] -> F.interpolate(S x S) -> [:newh, :neww] -> F.interpolate(H x W); [nb][H][W]"""
    if mut == "out_hw_swapped":
        newh, neww = neww, newh
    if mut == "out_crop_ignored":
        newh = neww = S
    x = np.asarray(logits, F32).astype(dtype).transpose(1, 2, 0)
    m = resize(x, S, S, dtype)[:newh, :neww]
    return resize(m, H, W, dtype).transpose(2, 0, 1).copy()


def unpatch(hi, lo, G, P):
    """patch rows [G*G][3 P^2] (column (py * P + px) * 3 + c) -> [3][G P][G P]; one fp32 addition, so exact to the bit"""
    v = hi.astype(F32) + (lo.astype(F32) if lo is not None else F32(0))
    return v.reshape(G, G, P, P, 3).transpose(4, 0, 2, 1, 3).reshape(3, G * P, G * P).copy()


# ------------------------------------------------------------------------------------------------ Depth Pro
def pyramid(img, S, flip, dtype, mut=None):
    """DepthProImageProcessor (rescale 1 / 255, normalise 0.5 / 0.5, bilinear to S x S) and the encoder's 0.5 and 0.25 levels
    (F.interpolate(scale_factor=...) of the S x S image). img: uint8 [H][W][3]. Returns P0, P1, P2 as [s][s][3]."""
    x = np.asarray(img).astype(dtype)
    if flip and mut != "pyr_flip_ignored":
        x = x[..., ::-1]
    x = (x / dtype(255) - dtype(0.5)) / dtype(0.5)
    P0 = resize(x, S, S, dtype)
    P1, P2 = resize(P0, S // 2, S // 2, dtype), resize(P0, S // 4, S // 4, dtype)
    if mut == "pyr_l2_offset":
        P2 = (dtype(0.25) * (P0[0::4, 0::4] + P0[0::4, 1::4] + P0[1::4, 0::4] + P0[1::4, 1::4])).astype(dtype)
    return P0, P1, P2


def merge_axis(n, g, pad, mut=None):
    """(crop, cell) of every coordinate of the merged map along one axis (merge_patches: the first crop loses its last `pad` cells, inner
    crops `pad` on both sides, the last its first `pad`)."""
    ax = []
    for i in range(n):
        lo = pad if i > 0 else 0
        hi = g - pad if i < n - 1 else g
        if n > 1 and mut == "merge_first_keeps_pad" and i == 0:
            lo = pad
        if n > 1 and mut == "merge_last_short" and i == n - 1:
            hi = g - pad
        ax += [(i, c) for c in range(lo, hi)]
    Ms = g if n == 1 else n * g - 2 * (n - 1) * pad
    return (ax + [ax[-1]] * Ms)[:Ms]                      # a wrong evaluation still fills the Ms cells the kernel writes


def merge(tok, crop0, n, g, pad, out, dtype, mut=None):
    """tok [crops][1 + g*g][D]: drop the class token, crop the n x n pieces from crop0 on, concatenate, resize to out x out. [out][out][D]"""
    tok = np.asarray(tok, F32).astype(dtype)
    ax = merge_axis(n, g, pad, mut)
    Ms = len(ax)
    m = np.zeros((Ms, Ms, tok.shape[-1]), dtype=dtype)
    for y, (cy, ly) in enumerate(ax):
        for x, (cx, lx) in enumerate(ax):
            m[y, x] = tok[crop0 + cy * n + cx, 1 + ly * g + lx]
    return m if out == Ms else resize(m, out, out, dtype)


def unsplit(hi, lo):
    """fp32 value of split pixels (one fp32 addition: exact to the bit) and the split of its ReLU"""
    v = hi.astype(F32) + (lo.astype(F32) if lo is not None else F32(0))
    return v, split(np.maximum(v, F32(0)))


def conv_s2(x, w, bias, add, dtype, mut=None):
    """relu(conv2d(x, w, stride 2, pad 1) + bias) + add. x [Si][Si][Cin], w [Cout][3][3][Cin], add [So*So][Cout] or None -> [So][So][Cout]"""
    x, w, bias = (np.asarray(a, F32).astype(dtype) for a in (x, w, bias))
    Si, So = x.shape[0], (x.shape[0] - 1) // 2 + 1
    xp = np.zeros((Si + 2, Si + 2, x.shape[2]), dtype=dtype)
    xp[1:-1, 1:-1] = x
    out = np.zeros((So, So, w.shape[0]), dtype=dtype)
    for oy in range(So):
        for ox in range(So):
            out[oy, ox] = np.einsum("oklc,klc->o", w, xp[2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3]) + bias
    a = None if add is None else np.asarray(add, F32).astype(dtype).reshape(So, So, -1)
    if a is not None and mut == "convs2_add_before_relu":
        return np.maximum(out + a, dtype(0)).astype(dtype)
    out = np.maximum(out, dtype(0))
    return (out if a is None else out + a).astype(dtype)


def dot(x, w, bias, dtype):
    x, w = np.asarray(x, F32).astype(dtype), np.asarray(w, F32).astype(dtype)
    return np.array([(x * w).sum(dtype=dtype) + dtype(F32(bias[0]))], dtype=dtype)


def seen(x, precision):
    """gemm_epi_ref.seen for numpy: the operand as the matrix cores see it, in float64"""
    hi = np.asarray(x, F32).astype(np.float16)
    s = hi.astype(F64)
    return s + (np.asarray(x, F32) - hi.astype(F32)).astype(np.float16).astype(F64) if precision == 3 else s


def head_tail(x, w, b1, w2, b2, precision, mut=None):
    """relu(conv1x1(relu(conv3x3(x, pad 1) + b1), w2) + b2) in float64 on the operands the kernel sees. x [S][S][C], w [32][3][3][C] -> [S][S]"""
    xs, ws = seen(x, precision), seen(w, precision)
    S = xs.shape[0]
    xp = np.zeros((S + 2, S + 2, xs.shape[2]))
    xp[1:-1, 1:-1] = xs
    h = np.zeros((S, S, ws.shape[0]))
    for ky in range(3):
        for kx in range(3):
            h += xp[ky:ky + S, kx:kx + S] @ ws[:, ky, kx].T
    h = h + np.asarray(b1, F64)
    if mut != "tail_relu1_dropped":
        h = np.maximum(h, 0.0)
    return np.maximum(h @ np.asarray(w2, F64) + float(b2[0]), 0.0)


def frame_cleared(side, C, mut=None):
    """[side + 2][side + 2][C]: the one-pixel frame zero, the interior untouched (the sentinel)"""
    a = np.full((side + 2, side + 2, C), SENTINEL, dtype=F32)
    a[0], a[-1], a[:, 0], a[:, -1] = 0, 0, 0, 0
    if mut == "border_corner_missed":
        a[-1, -1] = SENTINEL
    return a


def depth_out(canon, H, W, f_px, fov_deg, dtype, mut=None):
    """post_process_depth_estimation: f = f_px or 0.5 W / tan(0.5 deg2rad(fov)); inverse depth = canon * W / f, bilinear to H x W,
    depth = 1 / clamp(inverse, 1e-4, 1e4). Returns (depth [H][W], f)."""
    if f_px is not None:
        f = dtype(F32(f_px))
    else:
        fov = dtype(F32(fov_deg))
        rad = fov if mut == "depth_fov_radians" else fov * dtype(math.pi / 180.0)
        f = dtype(0.5) * dtype(W) / np.tan(dtype(0.5) * rad)
    inv = resize(np.asarray(canon, F32).astype(dtype) * dtype(W) / f, H, W, dtype)
    if mut != "depth_clamp_missing":
        inv = np.clip(inv, dtype(1e-4), dtype(1e4))
    with np.errstate(divide="ignore"):
        return (dtype(1) / inv).astype(dtype), f


# ------------------------------------------------------------------------------------------------ generic ops as SAM's token attention calls them
def token_scores(Q, K, nb, hd, nt, Tk, dh, alpha, dtype):
    """Q [nb * nt][hd * dh], K [nb * Tk][hd * dh] -> alpha Q_h K_h^T as [nb][hd][nt][Tk]"""
    Q, K = np.asarray(Q, F32).astype(dtype).reshape(nb, nt, hd, dh), np.asarray(K, F32).astype(dtype).reshape(nb, Tk, hd, dh)
    return (np.einsum("bqhd,bkhd->bhqk", Q, K).astype(dtype) * dtype(F32(alpha))).astype(dtype)


def token_context(P, V, nb, hd, nt, Tk, dh, dtype):
    """P [nb][hd][nt][Tk], V [nb * Tk][hd * dh] -> [nb * nt][hd * dh]"""
    P, V = np.asarray(P, F32).astype(dtype), np.asarray(V, F32).astype(dtype).reshape(nb, Tk, hd, dh)
    return np.einsum("bhqk,bkhd->bqhd", P, V).astype(dtype).reshape(nb * nt, hd * dh)


# ------------------------------------------------------------------------------------------------ cases
def _prod(**axes):
    out = [{}]
    for k, vals in axes.items():
        out = [dict(c, **{k: v}) for c in out for v in vals]
    return out


def _merge_cases():
    cases, i = [], 0
    for g, n, pad in ((4, 1, 0), (4, 3, 1), (8, 5, 2), (8, 3, 0), (8, 5, 1)):
        Ms = g if n == 1 else n * g - 2 * (n - 1) * pad
        for D in (4, 128):
            for out in sorted({Ms, g, 2 * g, 4 * g}):
                # crop0 and Olo alternate so that both values of each meet Ms == out and Ms != out on every triple
                cases.append(dict(g=g, n=n, pad=pad, Ms=Ms, D=D, out=out, crop0=(0, 2)[i % 2], lo=bool((i // 2) % 2)))
                i += 1
            i += 1
    return cases


FRAMES = ((70, 100, 128), (99, 71, 128))                    # (H, W, S): sx != sy both ways
MASK_HW = ((23, 31), (31, 23), (32, 32), (5, 3), (61, 97))
PYR_HW = ((5, 7), (64, 64), (150, 97), (33, 130))
DEPTH_HW = ((11, 17), (17, 11), (16, 16), (40, 64))

CASES = {
    "dense_pe": _prod(G=(2, 5), F=(32, 128)),
    "box_tokens": _prod(nb=(1, 3), C=(64, 256), frame=FRAMES),
    "ln_gelu": _prod(M=(1, 5, 64), D=(16, 48, 64, 256)),
    "i2t_attn": _prod(hg=((8, 64), (2, 128), (1, 256)), nt=(1, 7, 8), nb=(1, 3), spread=(False,)) + [dict(hg=(8, 64), nt=7, nb=3, spread=True)],
    "mask_prod": _prod(G=(2, 3), C8=(8, 32), nb=(1, 2), tk=((1, 3, 3), (2, 1, 1))),           # tk = (t0, ntk, out_box_stride / L^2)
    "mask_out": _prod(hw=MASK_HW, nb=(1, 3), plane=(False,)) + _prod(hw=((23, 31), (5, 3)), nb=(3,), plane=(True,)),
    "unpatch": _prod(lo=(True, False)),
    "iou_slice": _prod(n=(1, 5)),
    "add_bcast": [dict(n=64, bmod=16, b=True), dict(n=64, bmod=64, b=True), dict(n=64, bmod=16, b=False), dict(n=2052, bmod=12, b=True)],
    "pyramid": _prod(S=(16, 64), hw=PYR_HW, chw=(False, True), flip=(0, 1)),
    "merge": _merge_cases(),
    "unsplit": _prod(side=(2, 5), C=(4, 64), pad_in=(0, 1), outs=("f32", "split", "both")),
    "conv_s2": _prod(Si=(5, 8), Cin=(4, 32), Cout=(1, 8), add=(False, True)),
    "dot": _prod(n=(1, 255, 256, 1000)),
    "head_tail": _prod(S=(16, 48), C=(32, 64), precision=(1, 3)),
    "clear_borders": [dict(images=((1, 8, True), (4, 32, False)))],                        # (side, C, with lo), one call
    "depth_out": _prod(hw=DEPTH_HW, focal=(("f", 21.5), ("fov", 30.0), ("fov", 90.0)), outs=(True, False)),
}
KERNELS = tuple(CASES)

KINDS = {
    "dense_pe": {"pe": "f32"}, "box_tokens": {"corners": "f32", "head": "exact"}, "ln_gelu": {"y": "f32"}, "i2t_attn": {"o": "f32"},
    "mask_prod": {"masks": "f32"}, "mask_out": {"mask": "mask"}, "unpatch": {"out": "exact"}, "iou_slice": {"iou": "exact"},
    "add_bcast": {"out": "exact"}, "pyramid": {"P0": "f32", "P1": "f32", "P2": "f32"}, "merge": {"map": "split"},
    "unsplit": {"out": "exact", "p_hi": "exact", "p_lo": "exact"}, "conv_s2": {"out": "f32"}, "dot": {"out": "f32"},
    "head_tail": {"out": "tail"}, "clear_borders": {"img0": "exact", "img1": "exact"}, "depth_out": {"depth": "f32", "f": "f32"},
}


def case_id(case):
    return "-".join(f"{k}{v}" for k, v in case.items()).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x")


def _rng(kernel, case):
    """One seeded generator per case (a position-weighted character sum: stable across runs, unlike hash())"""
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(kernel + case_id(case))) % (2 ** 31))


def smooth_field(g, nb, L, std=10.0):
    """Logits with structure at the scale of the plane: a coarse random field resampled to L x L plus a little noise, std about `std`"""
    c = g.standard_normal((L // 2, L // 2, nb))
    f = resize(c, L, L, F64) + 0.25 * g.standard_normal((L, L, nb))
    return (f / f.std() * std).transpose(2, 0, 1).astype(F32)


def inputs(kernel, case):
    g = _rng(kernel, case)
    n32 = lambda *s: g.standard_normal(s).astype(F32)                                       # noqa: E731
    if kernel == "dense_pe":
        return dict(gauss=n32(2, case["F"]))
    if kernel == "box_tokens":
        H, W, S = case["frame"]
        C = case["C"]
        boxes = np.array([[-7.25, 10.5, W + 12.0, H - 3.75],                                # negative, fractional, beyond the image
                          [0.0, 0.0, float(W), float(H)], [W * 0.3 + 0.125, H * 0.4, W * 0.3 + 1.625, H * 1.5]], dtype=F32)[:case["nb"]]
        return dict(boxes=boxes, out_tokens=n32(5, C), gauss=n32(2, C // 2), corner=n32(2, C))
    if kernel == "ln_gelu":
        M, D = case["M"], case["D"]
        return dict(x=(n32(M, D) * 2 + F32(0.5)), gamma=(g.random(D) + 0.5).astype(F32), beta=n32(D))
    if kernel == "i2t_attn":
        (heads, G2), nt, nb = case["hg"], case["nt"], case["nb"]
        w = heads * 16
        q = n32(nb * G2, w) * F32(10.0 if case["spread"] else 1.0)                          # spread: scores of std 10, one token dominates
        return dict(q=q, k=n32(nb * nt, w), v=n32(nb * nt, w))                              # every box has its own tokens
    if kernel == "mask_prod":
        G, C8, nb = case["G"], case["C8"], case["nb"]
        return dict(up=n32(nb * G * G * 4, 4 * C8), hyper=n32(nb, 4, C8))                   # random: every (Y, X) has its own value
    if kernel == "mask_out":
        nb = case["nb"]
        return dict(logits=smooth_field(g, nb * (3 if case["plane"] else 1), 8).reshape(nb, -1, 8, 8))
    if kernel == "unpatch":
        hi, lo = split(n32(4, 768 + 64))
        return dict(hi=hi, lo=lo if case["lo"] else None)
    if kernel == "iou_slice":
        return dict(head=n32(case["n"], 128))
    if kernel == "add_bcast":
        return dict(a=n32(case["n"] if case["b"] else case["bmod"]), b=n32(case["bmod"]) if case["b"] else None)
    if kernel == "pyramid":
        H, W = case["hw"]
        return dict(img=g.integers(0, 256, (H, W, 3), dtype=np.uint8))
    if kernel == "merge":
        gg, n, D = case["g"], case["n"], case["D"]
        tok = n32(case["crop0"] + n * n, 1 + gg * gg, D)
        tok[:, 0] = SENTINEL                                                                # the class-token rows: must never be read
        return dict(tok=tok)
    if kernel == "unsplit":
        side, C = case["side"], case["C"]
        P = side + 2 if case["pad_in"] else side
        hi, lo = split(n32(P, P, C + 4))                                                    # pixel stride ld = C + 4
        return dict(hi=hi, lo=lo)
    if kernel == "conv_s2":
        Si, Cin, Cout = case["Si"], case["Cin"], case["Cout"]
        So = (Si - 1) // 2 + 1
        return dict(x=n32(Si, Si, Cin), w=n32(Cout, 3, 3, Cin) * F32(0.3), bias=n32(Cout), add=n32(So * So, Cout + 3) if case["add"] else None)
    if kernel == "dot":
        return dict(x=n32(case["n"]), w=n32(case["n"]), bias=n32(1))
    if kernel == "head_tail":
        S, C = case["S"], case["C"]
        return dict(x=n32(S, S, C), w=n32(32, 3, 3, C) * F32(1.0 / math.sqrt(9 * C)), b1=n32(32) * F32(0.3),
                    w2=(g.random(32) * 1.3 - 0.3).astype(F32), b2=np.array([0.1], dtype=F32))
    if kernel == "clear_borders":
        return {}
    if kernel == "depth_out":
        canon = (np.abs(n32(16, 16)) * F32(0.5) + F32(0.05))
        canon[0:4, 0:4] = 0.0                        # blocks wide enough that some output pixel has all four taps inside at every (H, W):
        canon[4:7, 4:8] = 1e-5                       # inverse depth 0 and 1e-5 -> the lower clamp, depth 1e4
        canon[8:12, 8:12] = 5e4                      # -> the upper clamp, depth 1e-4
        canon[13:16, 13:16] = 2e4
        return dict(canon=canon)
    raise KeyError(kernel)


def run(kernel, case, inp, dtype, mut=None):
    c = case
    if kernel == "dense_pe":
        return dict(pe=dense_pe(inp["gauss"], c["G"], dtype, mut))
    if kernel == "box_tokens":
        H, W, S = c["frame"]
        nh, nw = preprocess_shape(H, W, S)
        tok, sparse = box_tokens(inp["boxes"], inp["out_tokens"], inp["gauss"], inp["corner"], H, W, nh, nw, S, dtype, mut)
        return dict(corners=sparse, head=np.broadcast_to(inp["out_tokens"][None], (c["nb"],) + inp["out_tokens"].shape).copy())
    if kernel == "ln_gelu":
        return dict(y=sam_ln_gelu(inp["x"], inp["gamma"], inp["beta"], 1e-6, dtype, mut))
    if kernel == "i2t_attn":
        (heads, G2) = c["hg"]
        return dict(o=i2t_attn(inp["q"], inp["k"], inp["v"], c["nt"], heads, G2, c["nb"], 0.25, dtype, mut))
    if kernel == "mask_prod":
        t0, ntk, _ = c["tk"]
        return dict(masks=mask_prod(inp["up"], inp["hyper"], t0, ntk, c["C8"], c["G"], c["nb"], dtype, mut))
    if kernel == "mask_out":
        H, W = c["hw"]
        nh, nw = preprocess_shape(H, W, 32)
        lg = inp["logits"][:, 1 if c["plane"] else 0]
        return dict(mask=mask_logits(lg, 32, nh, nw, H, W, dtype, mut))
    if kernel == "unpatch":
        return dict(out=unpatch(inp["hi"][:, :768], None if inp["lo"] is None else inp["lo"][:, :768], 2, 16))
    if kernel == "iou_slice":
        return dict(iou=inp["head"][:, 1:4].copy())
    if kernel == "add_bcast":
        idx = np.arange(c["n"]) % c["bmod"]
        return dict(out=(inp["a"] + inp["b"][idx]) if c["b"] else inp["a"][idx].copy())
    if kernel == "pyramid":
        P0, P1, P2 = pyramid(inp["img"], c["S"], c["flip"], dtype, mut)
        return dict(P0=P0, P1=P1, P2=P2)
    if kernel == "merge":
        return dict(map=merge(inp["tok"], c["crop0"], c["n"], c["g"], c["pad"], c["out"], dtype, mut))
    if kernel == "unsplit":
        C, pad = c["C"], c["pad_in"]
        hi, lo = (a[1:-1, 1:-1, :C] if pad else a[:, :, :C] for a in (inp["hi"], inp["lo"]))
        v, (ph, pl) = unsplit(hi, lo)
        out = {}
        if c["outs"] in ("f32", "both"):
            out["out"] = v
        if c["outs"] in ("split", "both"):
            out["p_hi"], out["p_lo"] = ph, pl
        return out
    if kernel == "conv_s2":
        add = None if inp["add"] is None else inp["add"][:, :c["Cout"]]
        return dict(out=conv_s2(inp["x"], inp["w"], inp["bias"], add, dtype, mut))
    if kernel == "dot":
        return dict(out=dot(inp["x"], inp["w"], inp["bias"], dtype))
    if kernel == "head_tail":
        return dict(out=head_tail(inp["x"], inp["w"], inp["b1"], inp["w2"], inp["b2"], c["precision"], mut))
    if kernel == "clear_borders":
        return {f"img{i}": frame_cleared(side, C, mut if i == 1 else None) for i, (side, C, _) in enumerate(c["images"])}
    if kernel == "depth_out":
        H, W = c["hw"]
        kind, val = c["focal"]
        d, f = depth_out(inp["canon"], H, W, val if kind == "f" else None, val if kind == "fov" else None, dtype, mut)
        return dict(depth=d, f=np.array([f], dtype=dtype))
    raise KeyError(kernel)


def mutations_for(kernel, case):
    c = case
    if kernel == "dense_pe":
        return ["pe_center_off"]
    if kernel == "box_tokens":
        return ["box_xy_scale_swapped"]
    if kernel == "ln_gelu":
        return ["ln_gelu_var_biased_by_D64"] if c["D"] % 64 else []
    if kernel == "i2t_attn":
        return (["i2t_unscaled"] if c["nt"] > 1 else []) + (["i2t_head_stride"] if c["hg"][0] > 1 else []) + (["i2t_next_box_tokens"] if c["nt"] < K_MAX_TOK else [])
    if kernel == "mask_prod":
        return ["prod_yx_swapped", "prod_q_bits_swapped"]
    if kernel == "mask_out":
        nh, nw = preprocess_shape(*c["hw"], 32)
        return (["out_hw_swapped"] if nh != nw else []) + (["out_crop_ignored"] if (nh, nw) != (32, 32) else [])
    if kernel == "pyramid":
        return ["pyr_l2_offset"] + (["pyr_flip_ignored"] if c["flip"] else [])
    if kernel == "merge":
        # a wrong crop range counts where a merged cell it moves is one the output reads (a resize to a quarter reads two cells in four)
        true_ax = merge_axis(c["n"], c["g"], c["pad"])
        i0, i1, l1 = taps(c["out"], c["Ms"], F64)
        read = set(range(c["Ms"])) if c["out"] == c["Ms"] else set(i0[l1 < 1]) | set(i1[l1 > 0])
        return [m for m in ("merge_first_keeps_pad", "merge_last_short")
                if any(a != b and k in read for k, (a, b) in enumerate(zip(true_ax, merge_axis(c["n"], c["g"], c["pad"], m))))]
    if kernel == "conv_s2":
        return ["convs2_add_before_relu"] if c["add"] else []
    if kernel == "head_tail":
        return ["tail_relu1_dropped"]
    if kernel == "clear_borders":
        return ["border_corner_missed"]
    if kernel == "depth_out":
        return ["depth_clamp_missing"] + (["depth_fov_radians"] if c["focal"][0] == "fov" else [])
    return []


# ------------------------------------------------------------------------------------------------ comparison
def tail_tolerance(case):
    """gemm_epi_ref.tolerance of an fp32 destination with K = 9 C (scale-relative)"""
    gc = GE.Case(name="head_tail", epi=GE.STORE, M=case["S"] ** 2, N=32, K=9 * case["C"])
    return GE.tolerance(gc, case["precision"], SimpleNamespace(kind="f32", e32=0.0))


def band_of(r64, r32):
    """The mask rule's band: the `bound` tolerance of the resampled logit of this case"""
    return bound(r64, r32)[1]


def left_out_share(r64_logits, band):
    """Per mask, the share of pixels whose fp64 logit lies inside the band"""
    return [float((np.abs(p) <= band).mean()) for p in r64_logits]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.bits(a), R.bits(b))


def compare(kernel, case, got, r64, r32):
    """got: the device's outputs in the logical shape of `run` (split outputs already joined to float64; a one-pass output as the
    hi values; masks as uint8). Asserts each output's rule; returns {name: (E32, error)} of the float outputs."""
    figures = {}
    tag = f"{kernel} {case_id(case)}"
    for name, kind in KINDS[kernel].items():
        if name not in r64:
            assert name not in got
            continue
        g, a64, a32 = got[name], r64[name], r32[name]
        if kind == "exact":
            assert same_bits(np.asarray(g), np.asarray(a64)), f"{tag}/{name}: differs from the exact reference"
            continue
        if kind == "mask":
            band = band_of(a64, a32)
            g = np.asarray(g)
            assert g.shape == a64.shape and set(np.unique(g)) <= {0, 1}, f"{tag}/{name}: shape or values"
            worst = 0.0
            for i in range(a64.shape[0]):
                decided = np.abs(a64[i]) > band
                worst = max(worst, 1.0 - float(decided.mean()))
                assert 1.0 - decided.mean() <= MAX_LEFT_OUT, f"{tag}/{name} box {i}: too many pixels inside the band {band:.2e}"
                wrong = int(((g[i].astype(bool) != (a64[i] > 0)) & decided).sum())
                assert wrong == 0, f"{tag}/{name} box {i}: {wrong} pixels outside the band {band:.2e} disagree"
            figures[name] = (bound(a64, a32)[0], worst)
            continue
        g = np.asarray(g, dtype=F64)
        assert g.shape == a64.shape, f"{tag}/{name}: shape {g.shape} != {a64.shape}"
        if kind == "tail":
            err = float(np.max(np.abs(g - a64)) / max(float(np.max(np.abs(a64))), 1e-30))
            tol = tail_tolerance(case)
            figures[name] = (0.0, err)
            assert err <= tol, f"{tag}/{name}: scale-relative error {err:.3e} > {tol:.2e}"
            continue
        with np.errstate(invalid="ignore"):
            diff = np.abs(g - a64)
        assert not np.isnan(diff).any(), f"{tag}/{name}: not a number (or an infinity the reference does not have)"
        if kind == "hi" or (kind == "split" and not case.get("lo", True)):
            e32, tol = bound_hi_only(a64, a32)
            bad = diff > tol
        else:
            e32, tol = bound(a64, render(a32, F32) if kind == "split" else a32)
            bad = diff > tol
        err = float(diff.max()) if diff.size else 0.0
        figures[name] = (e32, err)
        assert not bad.any(), f"{tag}/{name}: |got - fp64| = {err:.3e} > {float(np.max(tol)):.3e} (E32 {e32:.3e})"
    return figures


def as_device(kernel, case, r):
    """What a device that computed exactly `r` (a run in fp32, possibly mutated) would hand to `compare`"""
    out = {}
    for name, v in r.items():
        kind = KINDS[kernel][name]
        if kind == "mask":
            out[name] = (v > 0).astype(np.uint8)
        elif kind == "split":
            out[name] = join(*split(v)) if case.get("lo", True) else join(split(v)[0])
        else:
            out[name] = v
    return out
