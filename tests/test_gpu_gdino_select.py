"""The small kernels between the GroundingDINO engine's fused ones, one at a time, against the exact or float64 restatements of
tests/gdino_ops_ref.py: the top-k of the two-stage query selection (launch_topk_keys: single_keys_kernel, the bitonic sort,
topk_emit_kernel) through ovm_g_topk_keys and its twin ovm_g_topk, rowmax_kernel (ovm_g_rowmax), select_ref_kernel
(ovm_g_select_ref), box_refine_kernel (ovm_g_box_refine), pad_logits_kernel (ovm_g_pad_logits), bert_embed_kernel (ovm_g_bert_embed),
normalize_image_kernel (ovm_g_normalize_image) and relpos_tables_kernel (ovm_g_relpos_tables, alone and feeding ovm_g_attn_f32).

The exact operations (top-k, row maximum, padding) are compared integer for integer / bit for bit. Every float comparison:
common.rel_err (max |a - b| / max |b|) against the float64 reference, bounded by 4 x the error PyTorch's own fp32 evaluation of the
same operation on the CPU shows against that reference from the same inputs, never below 2e-6 (gdino_ops_ref.bound). Inputs with a
row stride have one larger than the logical width, with values in the padding that would show in the result; every output buffer has
extra rows or trailing elements pre-filled with a sentinel that must survive. Each float case prints
`FIG <kernel> <case> err <measured> fp32 <PyTorch fp32> bound <bound> ratio <err / fp32>`.
tests/test_gdino_ops_ref_cpu.py shows on these very inputs that the slips these kernels could make land outside the bounds.

The case builders (`_*_case`) run on the CPU and are shared with that file; nothing here needs more than a few thousand elements
except the 64 x 64 relative-position grid (4096 rows).

Measured on an MI355X (err = the kernel against fp64, fp32 = PyTorch's fp32 evaluation against fp64, ratio = err / fp32; the bound is
the 2e-6 floor everywhere except bert_embed T22/D768/offset, 2.64e-3). No kernel needed a change.
  select_ref      ldc4 err 8.295e-08 fp32 8.295e-08 ratio 1.00; ldc8 err 7.758e-08 fp32 7.758e-08 ratio 1.00
  box_refine      n1/ldd4/eps1e-05 8.801e-08 8.801e-08 1.00; n1/ldd4/eps0.001 9.486e-08 9.486e-08 1.00; n1/ldd16/eps1e-05 7.043e-08
                  4.878e-08 1.44; n1/ldd16/eps0.001 4.128e-08 4.128e-08 1.00; n5/ldd4/eps1e-05 3.980e-08 3.286e-08 1.21; n5/ldd4/eps0.001
                  4.285e-08 4.285e-08 1.00; n5/ldd16/eps1e-05 6.394e-08 4.839e-08 1.32; n5/ldd16/eps0.001 3.937e-08 4.053e-08 0.97;
                  n900/ldd4/eps1e-05 8.847e-08 8.387e-08 1.05; n900/ldd4/eps0.001 1.094e-07 8.436e-08 1.30; n900/ldd16/eps1e-05 1.002e-07
                  8.291e-08 1.21; n900/ldd16/eps0.001 1.045e-07 8.515e-08 1.23
  bert_embed      (normal) T1: D64 7.705e-08 8.924e-08 0.86, D100 7.201e-08 1.030e-07 0.70, D768 6.757e-08 7.165e-08 0.94; T4: D64 1.051e-07
                  1.025e-07 1.03, D100 8.666e-08 8.675e-08 1.00, D768 1.143e-07 1.574e-07 0.73; T5: D64 1.193e-07 7.801e-08 1.53, D100
                  9.288e-08 1.046e-07 0.89, D768 6.386e-08 9.780e-08 0.65; T22: D64 1.525e-07 1.525e-07 1.00, D100 1.198e-07 1.151e-07 1.04,
                  D768 1.282e-07 1.237e-07 1.04; T256: D64 1.354e-07 1.205e-07 1.12, D100 1.404e-07 1.899e-07 0.74, D768 1.293e-07 1.568e-07
                  0.82; T22/D768/offset (mean 100, spread 0.01) err 6.199e-04 fp32 6.597e-04 bound 2.64e-03 ratio 0.94
  normalize_image bit-equal to the numpy float32 evaluation in the kernel's order in all 12 cases; err = fp32 (ratio 1.00): 1x1 3.168e-08,
                  7x5 hwc 3.640e-08, 7x5 chw 4.348e-08, 37x53 4.509e-08 (either flip)
  relpos_tables   (rel_h; rel_w) g1x1 5.789e-09 5.789e-09 1.00; 4.367e-08 4.367e-08 1.00. g3x5 1.084e-07 8.442e-08 1.28; 1.087e-07 7.926e-08
                  1.37. g64 3.545e-07 3.222e-07 1.10; 3.275e-07 3.853e-07 0.85. sam14 2.963e-07 2.406e-07 1.23; 2.766e-07 2.454e-07 1.13
  relpos_tables+attn_f32 g3x5 err 3.814e-07 fp32 4.645e-07 ratio 0.82
The top-k (23 cases and the long key buffer, ovm_g_topk_keys and ovm_g_topk), the row maxima (20 shapes) and pad_logits (12 shapes) are
equal to their references integer for integer / bit for bit.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import gdino_ops_ref as R
from common import rel_err

pytestmark = pytest.mark.gpu

SENT = -7.5                                  # float outputs
ISENT = -77                                  # out_idx
KSENT = 0x5A5A5A5A5A5A5A5A                   # key words
OVM_ERR_INVALID, OVM_ERR_HIP, OVM_ERR_SHAPE = -1, -2, -4
FLT_MAX = float(torch.finfo(torch.float32).max)
BIG = 1e30                                   # input padding: larger than every value, so a read past the logical width shows
TILE = 2048                                  # csrc/det2d.hip: one bitonic tile


def _lib():
    from ovmono3d_amd import lib
    return lib, lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _finish(rc, what):
    """Synchronise after a launch; a HIP error means the context is lost and every later GPU test would only repeat it."""
    if rc == OVM_ERR_HIP:
        pytest.exit(f"{what}: HIP error inside the launcher, stopping the session", returncode=3)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}; stopping the session", returncode=3)


def _report(kernel, name, got, ref64, ref32):
    err, e32, tol = rel_err(got, ref64), rel_err(ref32, ref64), R.bound(ref32, ref64)
    print(f"FIG {kernel} {name} err {err:.3e} fp32 {e32:.3e} bound {tol:.2e} ratio {err / max(e32, 1e-30):.2f}")
    assert torch.isfinite(got).all(), f"{kernel} {name}: non-finite output"
    assert err <= tol, f"{kernel} {name}: error {err:.3e} against fp64 > bound {tol:.2e} (PyTorch fp32: {e32:.3e})"


def _bits(t):
    return t.contiguous().view(torch.int32)


def pow2_at_least(n):
    p = TILE
    while p < n:
        p <<= 1
    return p


# ==================================================================================================================== top-k
#            (n, k): 1 x 1; one tile with k = n; N = 4096 (the first global pass, 2047 padding keys); N = 8192 mostly padding; N = 8192
TOPK_SIZES = ((1, 1), (2048, 2048), (2049, 900), (4097, 900), (5000, 900))
TOPK_FAMILIES = ("distinct", "seven", "tie", "equal", "mix")
TIE_VALUE, TIE_COUNT, TIE_ABOVE = -0.4375, 300, 750            # the engine's invalid proposals: one score on ~300 scattered tokens


def _topk_fits(family, n, k):
    return family != "tie" or (TIE_ABOVE < k < TIE_ABOVE + TIE_COUNT <= n)


TOPK_CASES = [(f, n, k) for f in TOPK_FAMILIES for n, k in TOPK_SIZES if _topk_fits(f, n, k)]


@lru_cache(maxsize=None)
def _topk_scores(family, n):
    g = torch.Generator().manual_seed(4000 + 10 * TOPK_FAMILIES.index(family) + n % 7)
    if family == "distinct":                                       # distinct normal values of both signs (and one +0.0)
        s = (torch.randperm(n, generator=g) - n // 2).float() * 3.7e-3
        assert len(set(s.tolist())) == n
    elif family == "seven":                                        # the index decides almost every rank
        s = torch.tensor([-3.0, -1.5, -0.25, 0.0, 0.125, 1.0, 2.5])[torch.randint(0, 7, (n,), generator=g)]
    elif family == "tie":
        perm = torch.randperm(n, generator=g)
        s = torch.empty(n)
        s[perm[:TIE_COUNT]] = TIE_VALUE
        above, below = perm[TIE_COUNT:TIE_COUNT + TIE_ABOVE], perm[TIE_COUNT + TIE_ABOVE:]
        s[above] = TIE_VALUE + 0.01 + torch.rand(len(above), generator=g)
        s[below] = TIE_VALUE - 0.01 - torch.rand(len(below), generator=g)
    elif family == "equal":
        s = torch.full((n,), 0.3)
    else:                                                          # 10 % positive, 40 % zeros of both signs, 50 % negative
        pos = torch.tensor([FLT_MAX, 1e-40, 1.4e-45, 3e-39])
        zero = torch.tensor([0.0, -0.0])
        neg = torch.tensor([-1.4e-45, -1e-40, -FLT_MAX, float("-inf"), -3e-39])
        u = torch.rand(n, generator=g)
        pick = torch.randint(0, 60, (n,), generator=g)
        s = torch.where(u < 0.1, pos[pick % 4], torch.where(u < 0.5, zero[pick % 2], neg[pick % 5]))
        if n > 1:
            assert bool(((s == 0) & torch.signbit(s)).any()) and bool(((s == 0) & ~torch.signbit(s)).any())
    assert s.dtype == torch.float32 and not torch.isnan(s).any()
    return s


def _topk_launch(device, scores, k, N, twin=False, n=None, alloc=None):
    """-> (rc, out_idx buffer [k + 8] on the CPU, key buffer [alloc + 16] on the CPU (None for the twin))"""
    _, L = _lib()
    n = len(scores) if n is None else n
    d_s = scores.to(device)
    out = torch.full((max(k, 0) + 8,), ISENT, dtype=torch.int32, device=device)
    if twin:
        rc = L.ovm_g_topk(d_s.data_ptr(), n, k, out.data_ptr(), _stream())
        _finish(rc, "ovm_g_topk")
        return rc, out.cpu(), None
    keys = torch.full(((N if alloc is None else alloc) + 16,), KSENT, dtype=torch.int64, device=device)
    rc = L.ovm_g_topk_keys(d_s.data_ptr(), n, k, out.data_ptr(), keys.data_ptr(), N, _stream())
    _finish(rc, "ovm_g_topk_keys")
    return rc, out.cpu(), keys.cpu()


def _check_topk(scores, k, out, keys, what):
    n, P = len(scores), pow2_at_least(len(scores))
    assert out[:k].tolist() == R.topk_ref(scores, k).tolist(), f"{what}: indices differ from the stable descending sort"
    assert bool((out[k:] == ISENT).all()), f"{what}: out_idx written past k"
    if keys is not None:
        # the sorted key buffer: every real key in the reference's order, then the padding keys, then the caller's words untouched
        assert (keys[:n] & 0xFFFFFF).tolist() == R.topk_ref(scores, n).tolist(), f"{what}: the sorted keys are not the full order"
        assert bool((keys[n:P] == -1).all()), f"{what}: a padding key is not behind every real key"
        assert bool((keys[P:] == KSENT).all()), f"{what}: key words past pow2_at_least(n) written"


@pytest.mark.parametrize("family,n,k", TOPK_CASES)
def test_topk_keys_matches_stable_sort(device, family, n, k):
    s = _topk_scores(family, n)
    if family == "tie":                                            # the tie straddles rank k
        assert int((s > TIE_VALUE).sum()) < k < int((s >= TIE_VALUE).sum())
    rc, out, keys = _topk_launch(device, s, k, pow2_at_least(n))
    assert rc == 0, f"top-k {family} n {n}: ovm_g_topk_keys returned {rc}"
    _check_topk(s, k, out, keys, f"top-k {family} n {n} k {k}")
    rc, out2, _ = _topk_launch(device, s, k, 0, twin=True)
    assert rc == 0
    _check_topk(s, k, out2, None, f"ovm_g_topk {family} n {n} k {k}")


def test_topk_keys_longer_key_buffer(device):
    """N = 8192 words offered for n = 100: one tile is sorted, words past it are not the kernel's"""
    for family in ("seven", "mix"):
        s = _topk_scores(family, 100)
        rc, out, keys = _topk_launch(device, s, 37, 8192)
        assert rc == 0
        assert len(keys) == 8192 + 16
        _check_topk(s, 37, out, keys, f"top-k {family} n 100 N 8192")


def test_topk_keys_refusals_write_nothing(device):
    _, L = _lib()
    s = _topk_scores("distinct", 2049)
    for what, kw in (("k > n", dict(k=2050, N=4096)), ("n = 0", dict(k=1, N=4096, n=0)), ("N too small", dict(k=900, N=2048, alloc=4096)),
                     ("k = 0", dict(k=0, N=4096))):
        rc, out, keys = _topk_launch(device, s, **kw)
        assert rc == OVM_ERR_INVALID, f"{what}: returned {rc}"
        assert bool((out == ISENT).all()) and bool((keys == KSENT).all()), f"{what}: something was written"
    d = s.to(device)
    buf = torch.zeros(4096, dtype=torch.int64, device=device)
    assert L.ovm_g_topk_keys(None, 2049, 900, buf.data_ptr(), buf.data_ptr(), 4096, _stream()) == OVM_ERR_INVALID
    assert L.ovm_g_topk_keys(d.data_ptr(), 2049, 900, None, buf.data_ptr(), 4096, _stream()) == OVM_ERR_INVALID
    assert L.ovm_g_topk_keys(d.data_ptr(), 2049, 900, buf.data_ptr(), None, 4096, _stream()) == OVM_ERR_INVALID
    _finish(0, "ovm_g_topk_keys refusals")


# ============================================================================================================== row maximum
ROWMAX_ROWS, ROWMAX_COLS = (1, 4, 5, 1030), (1, 22, 64, 65, 256)


@lru_cache(maxsize=None)
def _rowmax_case(rows, cols):
    g = torch.Generator().manual_seed(5000 + 7 * rows + cols)
    x = torch.full((rows, cols + 3), BIG)
    x[:, :cols] = torch.randn(rows, cols, generator=g) * 3.0 - 20.0          # all negative: a maximum started at 0 would show
    x[(rows - 1) // 2, :cols] = float("-inf")                                 # one row all -inf (the only row when rows = 1)
    if rows > 2:                                                              # the smallest finite value is still above -inf
        x[rows - 1, :cols] = float("-inf")
        x[rows - 1, cols // 2] = -FLT_MAX
    return x


@pytest.mark.parametrize("cols", ROWMAX_COLS)
@pytest.mark.parametrize("rows", ROWMAX_ROWS)
def test_rowmax_is_exact(device, rows, cols):
    _, L = _lib()
    x = _rowmax_case(rows, cols)
    launches = [x]
    if rows == 1:                                                  # the -inf row took the only row: a second launch with finite values
        y = x.clone()
        y[0, :cols] = torch.arange(cols).float() * -0.5 - 1.0
        launches.append(y)
    for xi in launches:
        want = R.rowmax_ref(xi[:, :cols], dtype=torch.float32)
        d = xi.to(device)
        out = torch.full((rows + 2,), SENT, device=device)
        rc = L.ovm_g_rowmax(d.data_ptr(), rows, cols, cols + 3, out.data_ptr(), _stream())
        _finish(rc, "ovm_g_rowmax")
        out = out.cpu()
        assert rc == 0
        assert torch.equal(_bits(out[:rows]), _bits(want)), f"rowmax {rows} x {cols}: not the exact maximum"
        assert bool((out[rows:] == SENT).all()), f"rowmax {rows} x {cols}: rows past the last written"


# =============================================================================================================== select_ref
SELECT_ROWS, SELECT_N = 300, 37


@lru_cache(maxsize=None)
def _select_case(ldc):
    g = torch.Generator().manual_seed(6000 + ldc)
    coord = torch.full((SELECT_ROWS, ldc), BIG)
    coord[:, :4] = torch.randn(SELECT_ROWS, 4, generator=g) * 2.0
    p = torch.rand(SELECT_ROWS, 4, generator=g) * 0.98 + 0.01
    prop = torch.log(p / (1 - p))
    invalid = torch.rand(SELECT_ROWS, generator=g) < 0.2          # invalid proposals: the whole row is +inf
    invalid[0], invalid[299], invalid[17] = False, True, True
    prop[invalid] = float("inf")
    idx = torch.randint(0, SELECT_ROWS, (SELECT_N,), generator=g, dtype=torch.int32)
    idx[0], idx[1], idx[2], idx[3], idx[4], idx[5] = 299, 0, 17, 0, 299, 150
    assert len(set(idx.tolist())) < SELECT_N and bool(invalid[idx.long()].any()) and not bool(invalid[idx.long()].all())
    c = dict(ldc=ldc, coord=coord, prop=prop, idx=idx, invalid=invalid[idx.long()])
    c["ref64"], c["ref32"] = (R.select_ref_ref(coord, prop, idx, dtype=dt) for dt in (torch.float64, torch.float32))
    return c


@pytest.mark.parametrize("ldc", [4, 8])
def test_select_ref_matches_fp64(device, ldc):
    _, L = _lib()
    c = _select_case(ldc)
    d = {n: c[n].to(device) for n in ("coord", "prop", "idx")}
    out = torch.full((SELECT_N + 2, 4), SENT, device=device)
    rc = L.ovm_g_select_ref(d["coord"].data_ptr(), ldc, d["prop"].data_ptr(), d["idx"].data_ptr(), SELECT_N, out.data_ptr(), _stream())
    _finish(rc, "ovm_g_select_ref")
    out = out.cpu()
    assert rc == 0
    assert bool((out[SELECT_N:] == SENT).all()), "select_ref: rows past n written"
    assert bool((out[:SELECT_N][c["invalid"]] == 1.0).all()), "select_ref: an infinite proposal logit does not give exactly 1"
    _report("select_ref", f"ldc{ldc}", out[:SELECT_N], c["ref64"], c["ref32"])


# =============================================================================================================== box_refine
BOX_N, BOX_LDD, BOX_EPS = (1, 5, 900), (4, 16), (1e-5, 1e-3)


@lru_cache(maxsize=None)
def _box_case(n, ldd, eps):
    g = torch.Generator().manual_seed(7000 + n + ldd + BOX_EPS.index(eps))
    e = float(np.float32(eps))
    ref = torch.rand(n, 4, generator=g)
    special = torch.tensor([0.0, 1.0, e / 2, 1 - e / 2, e, 1 - e, 0.5], dtype=torch.float64).float()
    m = min(len(special), 4 * n)
    ref.view(-1)[:m] = special[:m]
    delta = torch.full((n, ldd), BIG)
    delta[:, :4] = torch.randn(n, 4, generator=g)
    flat = torch.arange(4 * n)
    d4 = delta[:, :4].clone().view(-1)
    d4[flat % 11 == 5], d4[flat % 11 == 9] = 30.0, -30.0
    d4[0] = 30.0                                                   # on ref = 0: without the clamp the result is 0 instead of ~1
    if 4 * n > 1:
        d4[1] = -30.0                                              # on ref = 1: without the clamp 1 instead of ~0
    delta[:, :4] = d4.view(n, 4)
    c = dict(n=n, ldd=ldd, eps=eps, ref=ref, delta=delta)
    c["ref64"], c["ref32"] = (R.box_refine_ref(delta, ref, eps, dtype=dt) for dt in (torch.float64, torch.float32))
    return c


@pytest.mark.parametrize("eps", BOX_EPS)
@pytest.mark.parametrize("ldd", BOX_LDD)
@pytest.mark.parametrize("n", BOX_N)
def test_box_refine_matches_fp64(device, n, ldd, eps):
    _, L = _lib()
    c = _box_case(n, ldd, eps)
    d_delta, d_ref = c["delta"].to(device), c["ref"].to(device)
    out = torch.full((n + 2, 4), SENT, device=device)
    rc = L.ovm_g_box_refine(d_delta.data_ptr(), ldd, d_ref.data_ptr(), eps, out.data_ptr(), n, _stream())
    _finish(rc, "ovm_g_box_refine")
    out = out.cpu()
    assert rc == 0
    assert bool((out[n:] == SENT).all()), "box_refine: rows past n written"
    got = out[:n]
    assert bool(((got >= 0) & (got <= 1)).all()), "box_refine: a coordinate outside [0, 1]"
    _report("box_refine", f"n{n}/ldd{ldd}/eps{eps:g}", got, c["ref64"], c["ref32"])


# =============================================================================================================== pad_logits
PAD_Q, PAD_T, PAD_LD = (1, 900), (1, 22, 256), 256


@lru_cache(maxsize=None)
def _pad_case(Q, T, extra):
    g = torch.Generator().manual_seed(8000 + Q + 3 * T + extra)
    x = torch.full((Q, T + extra), BIG)
    x[:, :T] = torch.randn(Q, T, generator=g) * 10.0
    x[0, 0] = -0.0
    if Q * T > 1:
        x[Q - 1, T - 1] = float("-inf")                           # a -inf of the input's own, before the padding
    return x


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("T", PAD_T)
@pytest.mark.parametrize("Q", PAD_Q)
def test_pad_logits_is_exact(device, Q, T, extra):
    _, L = _lib()
    x = _pad_case(Q, T, extra)
    want = R.pad_logits_ref(x, T, PAD_LD)
    assert int(torch.isinf(want[0]).sum()) - int(torch.isinf(x[0, :T]).sum()) == PAD_LD - T          # T = 256: no -inf written
    d = x.to(device)
    out = torch.full((Q + 2, PAD_LD), SENT, device=device)
    rc = L.ovm_g_pad_logits(d.data_ptr(), T + extra, Q, T, out.data_ptr(), PAD_LD, _stream())
    _finish(rc, "ovm_g_pad_logits")
    out = out.cpu()
    assert rc == 0
    assert torch.equal(_bits(out[:Q]), _bits(want)), f"pad_logits Q {Q} T {T} ldx {T + extra}: not the copy plus -inf"
    assert bool((out[Q:] == SENT).all()), "pad_logits: rows past Q written"


# =============================================================================================================== bert_embed
BERT_T, BERT_D, BERT_VOCAB, BERT_POS = (1, 4, 5, 22, 256), (64, 100, 768), 50, 16
BERT_CASES = [(T, D, "normal") for T in BERT_T for D in BERT_D] + [(22, 768, "offset")]
BERT_EPS = 1e-12


@lru_cache(maxsize=None)
def _bert_case(T, D, kind):
    g = torch.Generator().manual_seed(9000 + 5 * T + D + (1 if kind == "offset" else 0))
    if kind == "normal":
        word, pos, typ = (torch.randn(r, D, generator=g) * 0.05 for r in (BERT_VOCAB, BERT_POS, 1))
    else:                                      # rows with mean ~100 and spread ~0.01: E[x^2] - mean^2 in fp32 keeps nothing of the variance
        word = 100.0 + torch.randn(BERT_VOCAB, D, generator=g) * 0.01
        pos, typ = torch.randn(BERT_POS, D, generator=g) * 0.002, torch.randn(1, D, generator=g) * 0.002
    ids = torch.randint(0, BERT_VOCAB, (T,), generator=g, dtype=torch.int32)
    ids[0] = 0
    if T > 1:
        ids[T - 1] = 49
    if T > 3:
        ids[2] = ids[1]
    # position ids that restart inside the caption, as the sub-sentence ids do: [0 | 0 1 2 3 4 | 0 1 2 | 0 1 2 3 4 5 6 | ...]
    pids, run = [], 1
    while len(pids) < T:
        pids += list(range(min(run, BERT_POS)))
        run = run * 3 % 11 + 2
    pids = torch.tensor(pids[:T], dtype=torch.int32)
    gamma, beta = 1.0 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    c = dict(T=T, D=D, word=word, pos=pos, typ=typ[0], ids=ids, pids=pids, gamma=gamma, beta=beta)
    c["ref64"], c["ref32"] = (R.bert_embed_ref(word, pos, typ[0], ids, pids, gamma, beta, BERT_EPS, dtype=dt) for dt in (torch.float64, torch.float32))
    return c


@pytest.mark.parametrize("T,D,kind", BERT_CASES)
def test_bert_embed_matches_fp64(device, T, D, kind):
    _, L = _lib()
    c = _bert_case(T, D, kind)
    d = {n: c[n].to(device).contiguous() for n in ("word", "pos", "typ", "ids", "pids", "gamma", "beta")}
    out = torch.full((T + 2, D), SENT, device=device)
    rc = L.ovm_g_bert_embed(d["word"].data_ptr(), d["pos"].data_ptr(), d["typ"].data_ptr(), d["ids"].data_ptr(), d["pids"].data_ptr(), T, D,
                            d["gamma"].data_ptr(), d["beta"].data_ptr(), BERT_EPS, out.data_ptr(), _stream())
    _finish(rc, "ovm_g_bert_embed")
    out = out.cpu()
    assert rc == 0
    assert bool((out[T:] == SENT).all()), "bert_embed: rows past T written"
    _report("bert_embed", f"T{T}/D{D}/{kind}", out[:T], c["ref64"], c["ref32"])


# ========================================================================================================== normalize_image
NORM_SIZES, NORM_LAYOUTS = ((1, 1), (7, 5), (37, 53)), ("hwc", "chw")
NORM_MEAN, NORM_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


@lru_cache(maxsize=None)
def _norm_case(H, W, layout, flip):
    """-> the uint8 buffer, the (sC, sH, sW) element strides of the descriptor and the logical [3][H][W] view of the buffer"""
    g = torch.Generator().manual_seed(10000 + 100 * H + W + (50 if layout == "chw" else 0))
    if layout == "hwc":                                            # interleaved, row stride padded by 5 bytes
        strides = (1, 3 * W + 5, 3)
        buf = torch.randint(0, 256, (H * (3 * W + 5),), generator=g, dtype=torch.uint8)
    else:                                                          # planar
        strides = (H * W, W, 1)
        buf = torch.randint(0, 256, (3 * H * W,), generator=g, dtype=torch.uint8)
    img = buf.as_strided((3, H, W), strides)
    buf[0], buf[strides[0] * 2] = 0, 255                           # both ends of the range, in channels 0 and 2 of pixel (0, 0)
    c = dict(H=H, W=W, buf=buf, strides=strides, img=img, flip=flip)
    c["ref64"], c["ref32"] = (R.normalize_image_ref(img, NORM_MEAN, NORM_STD, flip, dtype=dt) for dt in (torch.float64, torch.float32))
    c["np32"] = R.normalize_image_np32(img, NORM_MEAN, NORM_STD, flip)
    return c


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("layout", NORM_LAYOUTS)
@pytest.mark.parametrize("H,W", NORM_SIZES)
def test_normalize_image_matches_fp64(device, H, W, layout, flip):
    lib, L = _lib()
    c = _norm_case(H, W, layout, flip)
    d_buf = c["buf"].to(device)
    im = lib.OvmImage()
    im.data, im.height, im.width, im.orig_height, im.orig_width = d_buf.data_ptr(), H, W, H, W
    im.stride_c, im.stride_h, im.stride_w = c["strides"]
    mean, std = (C.c_float * 3)(*NORM_MEAN), (C.c_float * 3)(*NORM_STD)
    n = H * W * 3
    out = torch.full((n + 8,), SENT, device=device)
    rc = L.ovm_g_normalize_image(C.byref(im), mean, std, flip, out.data_ptr(), _stream())
    _finish(rc, "ovm_g_normalize_image")
    out = out.cpu()
    assert rc == 0
    assert bool((out[n:] == SENT).all()), "normalize_image: elements past H W 3 written"
    got, np32 = out[:n].view(H, W, 3), c["np32"]
    name = f"{H}x{W}/{layout}/flip{flip}"
    print(f"FIG normalize_image {name} bit-equal to numpy float32: {torch.equal(_bits(got), _bits(np32))}")
    # one float32 ulp of the numpy evaluation in the kernel's order (|values| < 4: no binade jumps beyond what nextafter covers)
    a = np32.numpy()
    ulp = np.maximum(np.nextafter(np.abs(a), np.float32(np.inf)) - np.abs(a), np.abs(a) - np.nextafter(np.abs(a), np.float32(0)))
    assert bool((np.abs(got.numpy().astype(np.float64) - a.astype(np.float64)) <= ulp.astype(np.float64)).all()), f"normalize_image {name}: > 1 ulp"
    _report("normalize_image", name, got, c["ref64"], c["ref32"])


# ============================================================================================================ relpos_tables
#            gh  gw  H  DH  sequences
RELPOS = {
    "sam14": (14, 14, 2, 64, 2),             # the SAM window
    "g3x5": (3, 5, 2, 32, 3),                # a non-square grid: gh and gw cannot be confused unnoticed
    "g1x1": (1, 1, 1, 16, 1),
    "g64": (64, 64, 1, 64, 1),               # a global block at a 1024 canvas: 4096 rows
}


@lru_cache(maxsize=None)
def _relpos_case(name):
    gh, gw, H, DH, nseq = RELPOS[name]
    g = torch.Generator().manual_seed(11000 + sorted(RELPOS).index(name))
    M, ldq, ldrel = nseq * gh * gw, 3 * H * DH + 4, max(gh, gw) + 3
    qoff = DH                                                      # q starts one head into the wider row (16-byte aligned: DH % 4 == 0)
    qbuf = torch.randn(M, ldq, generator=g)
    Rh, Rw = torch.randn(2 * gh - 1, DH, generator=g), torch.randn(2 * gw - 1, DH, generator=g)
    q = qbuf[:, qoff:qoff + H * DH].reshape(M, H, DH)
    c = dict(gh=gh, gw=gw, H=H, DH=DH, nseq=nseq, M=M, ldq=ldq, ldrel=ldrel, qoff=qoff, qbuf=qbuf, q=q, Rh=Rh, Rw=Rw)
    c["ref64"], c["ref32"] = (R.relpos_tables_ref(q, Rh, Rw, gh, gw, dtype=dt) for dt in (torch.float64, torch.float32))
    return c


def _relpos_launch(c, device, mutate=None):
    """-> (rc, rel_h buffer, rel_w buffer [M H + 2][ldrel] on the device, the device copies of the inputs)"""
    _, L = _lib()
    a = dict(ldq=c["ldq"], M=c["M"], H=c["H"], DH=c["DH"], gh=c["gh"], gw=c["gw"], ldrel=c["ldrel"])
    if mutate:
        a.update(mutate)
    keep = {n: c[n].to(device).contiguous() for n in ("qbuf", "Rh", "Rw")}
    rows = c["M"] * c["H"] + 2
    rel_h, rel_w = (torch.full((rows, c["ldrel"]), SENT, device=device) for _ in range(2))
    rc = L.ovm_g_relpos_tables(keep["qbuf"].data_ptr() + 4 * c["qoff"], a["ldq"], a["M"], a["H"], a["DH"], a["gh"], a["gw"], keep["Rh"].data_ptr(),
                               keep["Rw"].data_ptr(), rel_h.data_ptr(), rel_w.data_ptr(), a["ldrel"], _stream())
    _finish(rc, "ovm_g_relpos_tables")
    return rc, rel_h, rel_w, keep


def _relpos_check(c, name, rel_h, rel_w):
    MH = c["M"] * c["H"]
    for tag, buf, n, k in (("rel_h", rel_h.cpu(), c["gh"], 0), ("rel_w", rel_w.cpu(), c["gw"], 1)):
        owned = torch.zeros(buf.shape, dtype=torch.bool)
        owned[:MH, :n] = True
        assert bool((buf[~owned] == SENT).all()), f"relpos_tables {name} {tag}: written outside [M H][{n}]"
        _report("relpos_tables", f"{name}/{tag}", buf[:MH, :n].reshape(c["M"], c["H"], n), c["ref64"][k], c["ref32"][k])


@pytest.mark.parametrize("name", sorted(RELPOS))
def test_relpos_tables_match_fp64(device, name):
    c = _relpos_case(name)
    rc, rel_h, rel_w, _ = _relpos_launch(c, device)
    assert rc == 0, f"relpos_tables {name}: returned {rc}"
    _relpos_check(c, name, rel_h, rel_w)


@lru_cache(maxsize=None)
def _relpos_attn_case():
    """the 3 x 5 grid's q with keys and values of its own: attention with the tables, evaluated from the raw Rh and Rw"""
    c = dict(_relpos_case("g3x5"))
    g = torch.Generator().manual_seed(11100)
    nseq, T, H, DH = c["nseq"], c["gh"] * c["gw"], c["H"], c["DH"]
    c["ldk"] = H * DH + 4
    c["k"], c["v"] = torch.randn(nseq, T, c["ldk"], generator=g), torch.randn(nseq, T, c["ldk"], generator=g)
    heads = lambda t: t[:, :, :H * DH].reshape(nseq, T, H, DH).permute(0, 2, 1, 3)
    qv = c["q"].reshape(nseq, T, H, DH).permute(0, 2, 1, 3)
    c["scale"] = DH ** -0.5
    refs = []
    for dt in (torch.float64, torch.float32):
        rh, rw = R.relpos_tables_ref(c["q"], c["Rh"], c["Rw"], c["gh"], c["gw"], dtype=dt)
        refs.append(R.attn_ref(qv, heads(c["k"]), heads(c["v"]), c["scale"], None, None, rh.reshape(nseq, T, H, c["gh"]),
                               rw.reshape(nseq, T, H, c["gw"]), c["gw"], dtype=dt))
    c["attn64"], c["attn32"] = refs
    return c


def test_relpos_tables_feed_attn_f32(device):
    """the layout contract between the two kernels: ovm_g_relpos_tables writes [b1][q][b2][ldrel], ovm_g_attn_f32 reads it with
    key = kh * gw + kw"""
    lib, L = _lib()
    c = _relpos_attn_case()
    rc, rel_h, rel_w, keep = _relpos_launch(c, device)
    assert rc == 0
    nseq, T, H, DH = c["nseq"], c["gh"] * c["gw"], c["H"], c["DH"]
    dk, dv = c["k"].to(device), c["v"].to(device)
    ldo, rows = H * DH + 8, T + 2
    o = torch.full((nseq, rows, ldo), SENT, device=device)
    d = lib.OvmAttnF32Op()
    d.q, d.k, d.v = keep["qbuf"].data_ptr() + 4 * c["qoff"], dk.data_ptr(), dv.data_ptr()
    d.ldq, d.ldk, d.ldv = c["ldq"], c["ldk"], c["ldk"]
    d.sq1, d.sq2, d.sk1, d.sk2, d.sv1, d.sv2 = T * c["ldq"], DH, T * c["ldk"], DH, T * c["ldk"], DH
    d.o, d.ldo, d.so1, d.so2 = o.data_ptr(), ldo, rows * ldo, DH
    d.nb1, d.nb2, d.Tq, d.Tk, d.DH, d.scale = nseq, H, T, T, DH, c["scale"]
    d.rel_h, d.rel_w, d.rel_gw, d.ldrel = rel_h.data_ptr(), rel_w.data_ptr(), c["gw"], c["ldrel"]
    rc = L.ovm_g_attn_f32(C.byref(d), _stream())
    _finish(rc, "ovm_g_attn_f32")
    assert rc == 0
    o = o.cpu()
    owned = torch.zeros(o.shape, dtype=torch.bool)
    owned[:, :T, :H * DH] = True
    assert bool((o[~owned] == SENT).all()), "attn_f32 after relpos_tables: written outside the output"
    got = o[:, :T, :H * DH].reshape(nseq, T, H, DH).permute(0, 2, 1, 3)
    _report("relpos_tables+attn_f32", "g3x5", got, c["attn64"], c["attn32"])


def test_relpos_tables_refusals_write_nothing(device):
    _, L = _lib()
    c = _relpos_case("g3x5")
    for what, mutate, want in (("DH % 4", dict(DH=30), OVM_ERR_SHAPE), ("ldq % 4", dict(ldq=c["ldq"] + 2), OVM_ERR_SHAPE),
                               ("ldrel < gh", dict(gh=c["ldrel"] + 1), OVM_ERR_SHAPE), ("ldrel < gw", dict(ldrel=4), OVM_ERR_SHAPE),
                               ("M = 0", dict(M=0), 0), ("H = 0", dict(H=0), OVM_ERR_INVALID), ("M < 0", dict(M=-1), OVM_ERR_INVALID)):
        rc, rel_h, rel_w, _ = _relpos_launch(c, device, mutate)
        assert rc == want, f"{what}: returned {rc}, expected {want}"
        assert bool((rel_h == SENT).all()) and bool((rel_w == SENT).all()), f"{what}: tables written"
    buf = torch.zeros(64, device=device)
    p = buf.data_ptr()
    assert L.ovm_g_relpos_tables(None, 4, 1, 1, 4, 1, 1, p, p, p, p, 4, _stream()) == OVM_ERR_INVALID
    assert L.ovm_g_relpos_tables(p, 4, 1, 1, 4, 1, 1, p, p, None, p, 4, _stream()) == OVM_ERR_INVALID


def test_glue_adapters_refuse_null_pointers_and_empty_sizes(device):
    _, L = _lib()
    buf = torch.full((64,), SENT, device=device)
    idx = torch.zeros(8, dtype=torch.int32, device=device)
    p, i, s = buf.data_ptr(), idx.data_ptr(), _stream()
    assert L.ovm_g_select_ref(None, 4, p, i, 1, p, s) == OVM_ERR_INVALID
    assert L.ovm_g_select_ref(p, 4, p, i, 0, p, s) == OVM_ERR_INVALID
    assert L.ovm_g_box_refine(p, 4, None, 1e-5, p, 1, s) == OVM_ERR_INVALID
    assert L.ovm_g_box_refine(p, 4, p, 1e-5, p, 0, s) == OVM_ERR_INVALID
    assert L.ovm_g_pad_logits(p, 4, 1, 4, None, 8, s) == OVM_ERR_INVALID
    assert L.ovm_g_pad_logits(p, 4, 0, 4, p, 8, s) == OVM_ERR_INVALID
    assert L.ovm_g_pad_logits(p, 4, 1, 0, p, 8, s) == OVM_ERR_INVALID
    assert L.ovm_g_bert_embed(p, p, p, i, None, 1, 4, p, p, 1e-12, p, s) == OVM_ERR_INVALID
    assert L.ovm_g_bert_embed(p, p, p, i, i, 1, 0, p, p, 1e-12, p, s) == OVM_ERR_INVALID
    _finish(0, "adapter refusals")
    assert bool((buf == SENT).all()), "a refused call wrote something"
