"""Plain-torch restatements of the GroundingDINO engine's kernels, evaluated in float64 as the reference of the GPU tests: the three
fused kernels of csrc/gdino_kernels.hip (attn_f32_kernel, msdeform_fused_kernel / msdeform_fused4_kernel, rowop_kernel) for
tests/test_gpu_gdino_ops.py, and the small kernels between them - the top-k of the query selection (csrc/det2d.hip), rowmax_kernel and
normalize_image_kernel (csrc/gops.hip), select_ref_kernel, box_refine_kernel, pad_logits_kernel, bert_embed_kernel and
relpos_tables_kernel (csrc/gdino_kernels.hip) - for tests/test_gpu_gdino_select.py.
No GPU code and nothing from the product package; tests/test_gdino_ops_ref_cpu.py holds each against an independent implementation.

Every function takes `dtype`: float64 is the reference, float32 the same operation as PyTorch evaluates it in the kernels' own
precision - its error against the float64 result is the yardstick the GPU tests bound the kernels with (`bound`). The exact operations
(top-k, row maximum, padding) have one result whatever the dtype.

NaN scores are outside the top-k's contract (the kernel's key order would put a positive NaN first and a negative one last, torch
puts both first): topk_ref is not defined for them and no test uses one.
"""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 2e-6            # the floor test_generic_ops uses for fp32 ops (exact cases make the fp32 error zero)
FACTOR = 4.0            # DESIGN.md's convention for SAM and Depth Pro: 4 x the fp32 evaluation's own error


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """common.rel_err: max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def bound(fp32_result: torch.Tensor, ref64: torch.Tensor) -> float:
    return max(FACTOR * rel_err(fp32_result, ref64), FLOOR)


# ----------------------------------------------------------------------------------------------------------------- attention
def attn_ref(q, k, v, scale, bias_h=None, bias_b=None, rel_h=None, rel_w=None, rel_gw=0, dtype=torch.float64):
    """softmax_k(scale q.k + bias_h[b2][q][k] + bias_b[b1][q][k] + rel_h[b1][q][b2][kh] + rel_w[b1][q][b2][kw]) v.

    q [nb1][nb2][Tq][DH], k / v [nb1][nb2][Tk][DH]: any strided views (the caller builds them the way the descriptor's row and batch
    strides describe the buffers). bias_h [nb2][Tq][Tk]; bias_b [nb1 or 1][Tq][Tk] (1: shared by all b1, the descriptor's sbb = 0);
    rel_h [nb1][Tq][nb2][gh], rel_w [nb1][Tq][nb2][gw] with key = kh * rel_gw + kw. Returns [nb1][nb2][Tq][DH]."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    Tk = k.shape[2]
    s = torch.einsum("abqd,abkd->abqk", q, k) * scale
    if bias_h is not None:
        s = s + bias_h.to(dtype)[None]
    if bias_b is not None:
        s = s + bias_b.to(dtype)[:, None]
    if rel_h is not None:
        key = torch.arange(Tk)
        rh = rel_h.to(dtype).permute(0, 2, 1, 3)                  # [nb1][nb2][Tq][gh]
        rw = rel_w.to(dtype).permute(0, 2, 1, 3)
        s = s + rh[..., key // rel_gw] + rw[..., key % rel_gw]
    return torch.softmax(s, dim=-1) @ v


# ------------------------------------------------------------------------------------------- multi-scale deformable attention
def msdeform_locations(ow, ref, mode, H, L, P, shapes, dtype=torch.float64):
    """sampling locations [Q][H][L][P][2] (x, y in [0, 1] map coordinates) and attention weights [Q][H][L][P] from the kernel's
    operands: ow [Q][H*L*P*2 offsets | H*L*P logits]; mode 0: ref [Q][2] point, loc = ref + off / (W_l, H_l); mode 1: ref [Q][4] box
    (cx, cy, w, h), loc = c + off * wh * 0.5 / P. shapes: [(H_l, W_l)] per level."""
    Q = ow.shape[0]
    n = H * L * P
    ow, ref = ow.to(dtype), ref.to(dtype)
    off = ow[:, :2 * n].reshape(Q, H, L, P, 2)
    w = torch.softmax(ow[:, 2 * n:3 * n].reshape(Q, H, L * P), dim=-1).reshape(Q, H, L, P)
    if mode == 0:
        norm = torch.tensor([[wl, hl] for hl, wl in shapes], dtype=dtype)                     # (W_l, H_l)
        loc = ref[:, None, None, None, :2] + off / norm[None, None, :, None, :]
    else:
        loc = ref[:, None, None, None, :2] + off * ref[:, None, None, None, 2:4] * 0.5 / P
    return loc, w


def msdeform_ref(value, ow, ref, mode, H, dh, L, P, shapes, dtype=torch.float64):
    """out [Q][H*dh]: sum over levels and points of weight * bilinear tap of the level's map (F.grid_sample, align_corners=False,
    zero padding). value [S][H*dh], level l = rows start_l .. start_l + H_l W_l (row-major)."""
    loc, w = msdeform_locations(ow, ref, mode, H, L, P, shapes, dtype)
    Q = ow.shape[0]
    value = value.to(dtype)
    out = torch.zeros(H, dh, Q, dtype=dtype)
    start = 0
    for l, (hl, wl) in enumerate(shapes):
        vl = value[start:start + hl * wl].reshape(hl, wl, H, dh).permute(2, 3, 0, 1)        # [H][dh][hl][wl]
        grid = (2 * loc[:, :, l] - 1).permute(1, 0, 2, 3)                                     # [H][Q][P][2]
        tap = F.grid_sample(vl, grid, mode="bilinear", padding_mode="zeros", align_corners=False)   # [H][dh][Q][P]
        out = out + (tap * w[:, :, l].permute(1, 0, 2)[:, None]).sum(-1)
        start += hl * wl
    return out.permute(2, 0, 1).reshape(Q, H * dh)


# -------------------------------------------------------------------------------------------------------------- row operator
def rowop_ref(x, M, D, idx=None, seg=0, res=None, gamma=None, beta=None, eps=1e-5, zero_masked=False, add=None, add_rows=0,
              dtype=torch.float64):
    """gather -> (+ residual) -> LayerNorm -> zero_masked -> (+ add). Returns (y, y2) as [M][D] (y2 None without `add`).

    idx [M][nidx] int: row r = concat_j x[idx[r][j]][0:seg] (negative: zeros), D = nidx * seg; no idx: x[r][0:D]. res [M][D].
    LayerNorm over D when gamma is given. zero_masked: rows whose FIRST index is negative are zero after the norm (the kernel applies
    it on its LayerNorm path only, which is the only place the engine asks for it). y2 = y + add[r % add_rows]."""
    x = x.to(dtype)
    if idx is not None:
        idx = idx.long()
        rows = torch.zeros(M, idx.shape[1], seg, dtype=dtype)
        ok = idx >= 0
        rows[ok] = x[idx[ok]][:, :seg]
        rows = rows.reshape(M, D)
    else:
        rows = x[:M, :D].clone()
    if res is not None:
        rows = rows + res.to(dtype)[:M, :D]
    if gamma is not None:
        mean = rows.mean(-1, keepdim=True)
        var = ((rows - mean) ** 2).mean(-1, keepdim=True)
        rows = (rows - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)
        if zero_masked and idx is not None:
            rows = torch.where((idx[:, 0] < 0)[:, None], torch.zeros((), dtype=dtype), rows)
    y2 = None
    if add is not None:
        y2 = rows + add.to(dtype)[torch.arange(M) % add_rows, :D]
    return rows, y2


def split_f16(y32: torch.Tensor):
    """the split-fp16 image of an fp32 tensor: hi = fp16(y), lo = fp16(y - hi), round to nearest even, subnormals kept"""
    assert y32.dtype == torch.float32
    hi = y32.half()
    lo = (y32 - hi.float()).half()
    return hi, lo


def il_col(n):
    """column of element n in the interleaved image [row][k/32][hi 32 | lo 32]; the lo half sits 32 further"""
    return (n // 32) * 64 + n % 32


# ------------------------------------------------------------------------------------------------------- two-stage query selection
def topk_ref(scores, k, dtype=torch.float64):
    """indices [k] (int64) of the k largest scores by decreasing score, the lower index first among equal scores, -0.0 equal to +0.0:
    a stable ascending sort of the negated scores, -0.0 replaced by +0.0 first. No NaN (module docstring). Exact: the scores are only
    compared, `dtype` widens them and changes nothing."""
    x = scores.detach().cpu().to(dtype).numpy().copy()
    assert not np.isnan(x).any(), "NaN scores are outside the contract"
    x[x == 0] = 0.0                                               # -0.0 -> +0.0
    return torch.from_numpy(np.argsort(-x, kind="stable")[:k].astype(np.int64))


def rowmax_ref(x, dtype=torch.float64):
    """out[r] = max_j x[r][j], exact (x: the logical [rows][cols] view)"""
    return x.to(dtype).max(dim=1)[0]


def select_ref_ref(coord, prop, idx, dtype=torch.float64):
    """out[i][c] = sigmoid(coord[idx[i]][c] + prop[idx[i]][c]), c < 4. coord: the logical [rows][4] view. A proposal logit of +inf (an
    invalid proposal) gives exactly 1."""
    i = idx.long()
    return torch.sigmoid(coord.to(dtype)[i, :4] + prop.to(dtype)[i, :4])


def box_refine_ref(delta, ref, eps, dtype=torch.float64):
    """sigmoid(delta + logit(clamp(ref, eps, 1 - eps))), [n][4]; eps is the kernel's fp32 value, widened (1 - eps is then evaluated in
    `dtype`). delta: the logical [n][4] view."""
    e = float(np.float32(eps))
    xc = ref.to(dtype).clamp(min=e, max=1.0 - e)
    return torch.sigmoid(delta.to(dtype)[:, :4] + torch.log(xc / (1.0 - xc)))


def pad_logits_ref(x, T, ld):
    """out [Q][ld]: columns 0..T an exact copy of x[:, :T], -inf from column T on"""
    out = torch.full((x.shape[0], ld), float("-inf"), dtype=x.dtype)
    out[:, :T] = x[:, :T]
    return out


def bert_embed_ref(word, pos, typ, ids, pids, gamma, beta, eps=1e-12, dtype=torch.float64):
    """LayerNorm((word[ids] + pos[pids]) + typ) over D with the two-pass (centred) variance; typ: the one row of token type 0"""
    rows = (word.to(dtype)[ids.long()] + pos.to(dtype)[pids.long()]) + typ.to(dtype)
    mean = rows.mean(-1, keepdim=True)
    var = ((rows - mean) ** 2).mean(-1, keepdim=True)
    return (rows - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


def normalize_image_ref(img, mean, std, flip, dtype=torch.float64):
    """out [H][W][3], out[y][x][c] = (img[cs][y][x] - mean[cs]) / std[cs] with the source channel cs = 2 - c when flipped, else c.
    img: the logical uint8 [3][H][W] view of whatever layout the descriptor's strides describe; mean / std: 3 fp32 values each."""
    src = [2, 1, 0] if flip else [0, 1, 2]
    m = torch.as_tensor(mean, dtype=torch.float32).to(dtype)[src]
    s = torch.as_tensor(std, dtype=torch.float32).to(dtype)[src]
    return (img[src].permute(1, 2, 0).to(dtype) - m) / s


def normalize_image_np32(img, mean, std, flip):
    """the same in numpy float32, in the kernel's operation order: (float(pixel) - mean) / std, one rounding each (IEEE division)"""
    src = [2, 1, 0] if flip else [0, 1, 2]
    m, s = np.asarray(mean, np.float32)[src], np.asarray(std, np.float32)[src]
    px = img.numpy()[src].transpose(1, 2, 0).astype(np.float32)
    return torch.from_numpy(((px - m) / s).astype(np.float32))


def relpos_tables_ref(q, Rh, Rw, gh, gw, dtype=torch.float64):
    """decomposed relative-position tables of the rows m of q [M][H][DH] (any strided view), whose position on the gh x gw grid is
    (qh, qw) = divmod(m mod (gh gw), gw): rel_h[m][h][kh] = q[m][h] . Rh[qh - kh + gh - 1], rel_w[m][h][kw] = q[m][h] . Rw[qw - kw +
    gw - 1]. Rh [2 gh - 1][DH], Rw [2 gw - 1][DH]. Returns (rel_h [M][H][gh], rel_w [M][H][gw])."""
    q, Rh, Rw = q.to(dtype), Rh.to(dtype), Rw.to(dtype)
    M, H, _ = q.shape
    t = torch.arange(M) % (gh * gw)
    qh, qw = t // gw, t % gw
    ih = qh[:, None] - torch.arange(gh)[None, :] + gh - 1        # [M][gh]
    iw = qw[:, None] - torch.arange(gw)[None, :] + gw - 1        # [M][gw]
    all_h = torch.einsum("mhd,rd->mhr", q, Rh)                   # every relative offset, then the ones the row's position picks
    all_w = torch.einsum("mhd,rd->mhr", q, Rw)
    return (torch.gather(all_h, 2, ih[:, None, :].expand(M, H, gh)), torch.gather(all_w, 2, iw[:, None, :].expand(M, H, gw)))
