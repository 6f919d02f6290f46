"""The fused two-layer MLP of the detector's image branch (csrc/mlp_fused.hip: fc1 + activation + fc2's k-slices in one kernel, then
the split-K reduce) through ovm_op_mlp_fused, against an fp64 reference, next to today's two-launch route (ovm_op_gemm_epi twice)
on the same inputs.

Shapes are the smallest at which the kernel can still go wrong (row tile 64, hidden chunk 256, 256-column blocks in phase 2):

  case      M    C     hidden  act   output            reaches
  below     37   256   256     GELU  residual in place M below one row tile, one chunk (one slab)
  left4     68   256   512     GELU  residual in place one row tile + 4 leftover rows, two chunks
  stage4    289  1024  4096    GELU  residual in place Swin stage 4 as it is: 5 row tiles, 16 chunks, four 256-column blocks
  c128      70   128   512     GELU  residual in place 4 phase-1 k-steps (fewer than the 8 of a phase-2 block), C below one column block
  encoder   300  256   2048    ReLU  Y = . + b2 + R    the encoder's form (EPI_STORE with R), 8 chunks: middle slabs
  bigh      68   256   1024    GELU  residual in place |H| up to ~1e3: the lo halves of H carry weight; 4 chunks

Inputs: seeded randn. Reference: fp64 on the CPU from the operands as the device sees them (hi + lo of the fp16 split,
gemm_epi_ref.seen), H kept in fp64.

Bound (scale-relative, max |got - ref| / max |ref|), from the project's per-GEMM bounds: t2 + A t1 with
  t1 = gemm_epi_ref.tolerance of a split destination at K = C, activation allowance included (the error of H relative to max |H|),
  t2 = that of an fp32 destination at K = hidden,
  A  = max |H_ref| * max_n sum_k |W2[n][k]| / max |Y_ref|: how far the second layer can carry a scale-relative error of H.
Today's route is held to the same bound and both errors are printed (FIG lines).

Measured on an MI355X (fused / two launches / bound): below 1.6e-07 / 1.6e-07 / 3.1e-05, left4 1.6e-07 / 3.2e-07 / 5.4e-05, stage4
1.8e-07 / 1.7e-07 / 1.3e-04, c128 1.5e-07 / 2.3e-07 / 5.1e-05, encoder 1.5e-07 / 1.5e-07 / 8.4e-05, bigh 3.1e-07 / 3.1e-07 / 1.4e-04
(profiles/mlp_fused/README.md). A is 8.7 - 42, so the bound is 100 - 400 times the error: both routes sit at fp32 accumulation noise.
"""
import ctypes as C
import math
from functools import lru_cache

import pytest
import torch

import gemm_epi_ref as R
from test_gpu_gemm_epilogues import _route, launch

pytestmark = pytest.mark.gpu

SENT = R.SENTINEL
#        name      M    C     hidden act resid  x/w1 scale
CASES = {
    "below":   (37, 256, 256, 2, True, 1.0),
    "left4":   (68, 256, 512, 2, True, 1.0),
    "stage4":  (289, 1024, 4096, 2, True, 1.0),
    "c128":    (70, 128, 512, 2, True, 1.0),
    "encoder": (300, 256, 2048, 1, False, 1.0),
    "bigh":    (68, 256, 1024, 2, True, 16.0),
}


def _lib():
    from ovmono3d_amd import lib
    return lib, lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@lru_cache(maxsize=None)
def _inputs(name):
    M, Cc, Hd, act, resid, sc = CASES[name]
    g = torch.Generator().manual_seed(4100 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(X=rn(M, Cc) * sc, W1=rn(Hd, Cc) * (sc / math.sqrt(Cc)), b1=rn(Hd) * 0.5, W2=rn(Cc, Hd) / math.sqrt(Hd), b2=rn(Cc),
                res=rn(M, Cc))


@lru_cache(maxsize=None)
def _reference(name):
    """-> (Y_ref fp64 [M][C], bound)"""
    M, Cc, Hd, act, resid, sc = CASES[name]
    inp = _inputs(name)
    Z = R.seen(inp["X"], 3) @ R.seen(inp["W1"], 3).T + inp["b1"].double()
    f = R.gelu_erf if act == 2 else torch.relu
    H = f(Z)
    W2 = R.seen(inp["W2"], 3)
    Y = H @ W2.T + inp["b2"].double() + inp["res"].double()
    e32 = R._act_err(R.gelu_erf, Z) if act == 2 else 0.0
    t1 = R.tolerance(R.Case("fc1", R.GELU, M, Hd, Cc), 3, R.Out("H", None, None, None, None, "split", e32=e32))
    t2 = R.tolerance(R.Case("fc2", R.RESID, M, Cc, Hd), 3, R.Out("Y", None, None, None, None, "f32"))
    A = float(H.abs().max() * W2.abs().sum(dim=1).max() / Y.abs().max())
    return Y, t2 + A * t1, dict(t1=t1, t2=t2, A=A, hmax=float(H.abs().max()))


def _image(x, device):
    """fp32 [rows][K] -> the interleaved split image [rows][K/32][hi 32 | lo 32] as the library writes it (int16 [rows][2 K])"""
    _, L = _lib()
    x = x.to(device).contiguous()
    rows, K = x.shape
    hi = torch.empty(rows, K, dtype=torch.int16, device=device)
    lo = torch.empty_like(hi)
    img = torch.empty(rows, 2 * K, dtype=torch.int16, device=device)
    assert L.ovm_op_split_f16(x.data_ptr(), x.numel(), hi.data_ptr(), lo.data_ptr(), _stream()) == 0
    assert L.ovm_op_interleave(hi.data_ptr(), lo.data_ptr(), rows, K, img.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return img


def _fused(name, device, dims=None, act=None, ws_short=0):
    """Runs ovm_op_mlp_fused inside canary regions. -> (rc, Y [M][C] CPU, {region name: untouched?})"""
    _, L = _lib()
    M, Cc, Hd, a, resid, _ = CASES[name]
    inp = _inputs(name)
    x, w1, w2 = _image(inp["X"], device), _image(inp["W1"], device), _image(inp["W2"], device)
    b1, b2 = inp["b1"].to(device), inp["b2"].to(device)
    aM, aC, aH = dims or (M, Cc, Hd)                       # what the call claims (refusal tests)
    G = 64 * Cc                                            # guard: one row tile of output rows
    n_ws = (Hd // 256) * M * Cc
    ws = torch.full((G + n_ws + G,), SENT, device=device)
    ws[G:G + n_ws] = float("nan")                          # a slab element the kernel leaves out surfaces as NaN in the result
    out = torch.full((G + M * Cc + G,), SENT, device=device)
    res = inp["res"].to(device).contiguous()
    if resid:
        out[G:G + M * Cc] = res.flatten()
    ws0, out0 = ws.clone(), out.clone()
    rc = L.ovm_op_mlp_fused(x.data_ptr(), 2 * Cc, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), aM, aC, aH,
                            a if act is None else act, ws.data_ptr() + 4 * G, 4 * n_ws - ws_short,
                            out.data_ptr() + 4 * G if resid else None, None if resid else res.data_ptr(),
                            None if resid else out.data_ptr() + 4 * G, _stream())
    torch.cuda.synchronize()
    same = lambda t, t0, sl: bool(torch.equal(t[sl].view(torch.int32), t0[sl].view(torch.int32)))
    canary = {"ws_front": same(ws, ws0, slice(0, G)), "ws_back": same(ws, ws0, slice(G + n_ws, None)),
              "out_front": same(out, out0, slice(0, G)), "out_back": same(out, out0, slice(G + M * Cc, None)),
              "ws_all": same(ws, ws0, slice(0, None)), "out_all": same(out, out0, slice(0, None))}
    return rc, out[G:G + M * Cc].view(M, Cc).cpu(), canary


def _two_launches(name, device):
    """Today's route on the same inputs: fc1 with the activation epilogue writing the split image, fc2 reading it."""
    M, Cc, Hd, act, resid, _ = CASES[name]
    inp = _inputs(name)
    c1 = (R.Case("fc1", R.GELU, M, Hd, Cc, ldo=Hd) if act == 2 else R.Case("fc1", R.STORE, M, Hd, Cc, relu=1, ldo=Hd))
    rc, got = launch(c1, {"A": inp["X"], "W": inp["W1"], "bias": inp["b1"], "O": torch.full((M * Hd,), SENT)}, _route("p3", 3), device)
    assert rc == 0
    H = got["O"].view(M, Hd)
    if resid:
        c2 = R.Case("fc2", R.RESID, M, Cc, Hd, ldx=Cc)
        rc, got = launch(c2, {"A": H, "W": inp["W2"], "bias": inp["b2"], "X": inp["res"].clone()}, _route("p3", 3), device)
        assert rc == 0
        return got["X"].view(M, Cc)
    c2 = R.Case("fc2", R.STORE, M, Cc, Hd, ldc=Cc, ldr=Cc)
    rc, got = launch(c2, {"A": H, "W": inp["W2"], "bias": inp["b2"], "C": torch.full((M, Cc), SENT), "R": inp["res"]}, _route("p3", 3), device)
    assert rc == 0
    return got["C"].view(M, Cc)


@pytest.mark.parametrize("name", list(CASES))
def test_fused_mlp_against_fp64(device, name):
    Y, bound, fig = _reference(name)
    rc, got, canary = _fused(name, device)
    assert rc == 0, f"{name}: ovm_op_mlp_fused returned {rc}"
    two = _two_launches(name, device)
    scale = float(Y.abs().max())
    assert torch.isfinite(got).all(), f"{name}: non-finite output (a slab element was never written)"
    err_f = float((got.double() - Y).abs().max()) / scale
    err_t = float((two.double() - Y).abs().max()) / scale
    print(f"FIG mlp_fused {name}: fused err {err_f:.3e}, two launches err {err_t:.3e}, bound {bound:.3e} "
          f"(t1 {fig['t1']:.2e}, t2 {fig['t2']:.2e}, A {fig['A']:.2f}, max|H| {fig['hmax']:.3g})")
    for k in ("ws_front", "ws_back", "out_front", "out_back"):
        assert canary[k], f"{name}: canary region {k} was written"           # out_back: the rows at and past M
    assert err_f <= bound, f"{name}: fused route {err_f:.3e} > {bound:.3e}"
    assert err_t <= bound, f"{name}: two-launch route {err_t:.3e} > {bound:.3e}"


@pytest.mark.parametrize("what,dims,act,short,want", [
    ("C % 32", (68, 240, 512), None, 0, -1),
    ("hidden % chunk", (68, 256, 384), None, 0, -1),
    ("hidden below a chunk", (68, 256, 128), None, 0, -1),
    ("activation", None, 0, 0, -1),
    ("workspace too small", None, None, 16, -5),
])
def test_unsupported_shapes_are_refused_and_nothing_is_launched(device, what, dims, act, short, want):
    rc, _, canary = _fused("left4", device, dims=dims, act=act, ws_short=short)
    assert rc == want, (what, rc)
    assert canary["ws_all"] and canary["out_all"], f"{what}: a buffer changed although the call was refused"
