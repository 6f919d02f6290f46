"""Every fused epilogue of csrc/gemm.hpp, the leftover-row body, the split-K reduce pass and the implicit-GEMM 3x3 convolution against the
fp64 restatement of tests/gemm_epi_ref.py, through ovm_op_gemm_epi (one epilogue in isolation, launched as the model path launches it).

A test id names the epilogue case, the shape and the route, e.g. `resid_gamma_map/g256sk-g256_k2`:

  shape    M, N, K                         reaches
  ragged   200, 100, 128                   partial M tile, partial N tile with N % 4 == 0
  tail     132, 192, 128                   4 leftover rows (gemm_tail_body)
  splitk   130, 128, 1024 (2048 at f16)    ksplit = 4: splitk_epilogue_kernel applies the epilogue, leftover path off
  g256     260, 256, 64                    gemm256 kernel + 4 leftover rows
  g256sk   260, 256, 512, hint 2           ... and its split-K reduce pass
  qkv      260, 768, 64 (B 2, T 130)       head split, Tpad 192; gemm256: the 256 x 192 variant and gemm256_n192 = 0
  conv     132, 72, 576 (3 x 44 x 64)      implicit-GEMM addressing on tiles and on leftover rows
  convsk   144, 64, 1152 (12 x 12 x 128)   k-slices that cross taps (f16x3 only: 18 k-steps of 64 do not split at f16)
  convt    162, 128, 64 (B 2, G 9)         2 x 2 scatter; convt_tail: B 33, G 2 -> 132 rows

  route    p1 / p3 = one-pass / split precision, ail = interleaved A, sym = symmetric kernel (gemm_stages 2; default: wave-specialised),
           bm256 = gemm_bm 256, notail = gemm_tail 0, nosplitk = gemm_splitk 0, g256_kH = the 256 x 256 kernel with split-K hint H,
           n192off = gemm256_n192 0

Two input families (as det2d_cases.py): `exact` - small integers, gamma a power of two, compared with torch.equal (Q, scaled by
0.125 log2 e, excepted); `float` - seeded randn, compared with the bounds of gemm_epi_ref.tolerance. Every comparison also asserts
that nothing outside an output's index set changed (bit for bit) and that nothing inside it still holds the sentinel.

Float-family errors measured on an MI355X (scale-relative, the largest over all shapes and routes of the row) next to the bound
of the same test:

  epilogue (output)                       f16x3: error / bound          f16: error / bound
  store, no activation / ReLU (C, fp32)   5.7e-07 / 2.0e-06 (convsk)    3.7e-07 / 3e-03
  store, split O (planar / bordered)      5.7e-07 / 3.0e-06 (convsk)    3.7e-04 / 3e-03
  store, GELU (C / O)                     5.3e-07 / 2.5e-06 (convsk)    3.3e-04 / 3e-03
  resid (X, fp32, in place)               3.9e-07 / 2.0e-06 (splitk)    3.5e-07 / 3e-03
  gelu erf (O, planar / interleaved)      7.6e-07 / 3.4e-06 (splitk)    3.9e-04 / 3e-03
  QuickGELU (O, planar / interleaved)     5.2e-07 / 3.5e-06 (splitk)    3.5e-04 / 3e-03
  qkv (Q / K / V^T)                       1.6e-07 / 3.0e-06             4.0e-04 / 3e-03
  patch (X, fp32)                         1.7e-07 / 2.0e-06             1.2e-07 / 3e-03
  convt (O)                               1.9e-07 / 3.0e-06             3.9e-04 / 3e-03

The largest error / bound ratio is 0.29 (store C through the 3x3 convolution, K = 1152, symmetric kernel), so no case sits above half
its bound. The f16 column is the fp16 rounding of a one-part output (2^-11 relative) where the destination is split fp16, and fp32
accumulation noise where it is fp32: the reference sees the same fp16 operands. Transcendental rows: the fp32 torch evaluation of
the activation is 0.9e-7 .. 1.2e-7 off the fp64 one, so 4 x that adds 0.35e-6 .. 0.48e-6 to the bound. At the split-K shape on the
symmetric kernel the device's error is 7.5e-7 with GELU(erf) and 5.2e-7 with QuickGELU against 4.2e-7 for the plain store (other
seeded inputs, same K): the excess, 3.4e-7 and 1.1e-7, is 0.95 and 0.25 of that allowance.
"""
import ctypes as C
from functools import lru_cache

import pytest
import torch

import gemm_epi_ref as R

pytestmark = pytest.mark.gpu

TUNE_DEFAULTS = {"gemm_stages": 0, "gemm_bm": 0, "gemm_splitk": 1, "gemm_tail": 1, "gemm256_n192": 1}


def _route(name, precision, a_il=0, stages=0, bm=0, tail=1, splitk=1, route=0, hint=1, n192=1):
    return dict(name=name, precision=precision, a_il=a_il, route=route, hint=hint,
                tune={"gemm_stages": stages, "gemm_bm": bm, "gemm_tail": tail, "gemm_splitk": splitk, "gemm256_n192": n192})


BASE = [_route("p3", 3), _route("p1", 1), _route("p3_ail", 3, a_il=1), _route("p3_sym", 3, stages=2), _route("p1_sym", 1, stages=2),
        _route("p3_ail_sym", 3, a_il=1, stages=2), _route("p3_sym_bm256", 3, stages=2, bm=256), _route("p1_sym_bm256", 1, stages=2, bm=256)]
NOTAIL = [_route("p3_notail", 3, tail=0), _route("p1_notail", 1, tail=0), _route("p3_ail_notail", 3, a_il=1, tail=0),
          _route("p3_sym_notail", 3, stages=2, tail=0)]
NOSPLITK = [_route("p3_nosplitk", 3, splitk=0), _route("p1_nosplitk", 1, splitk=0), _route("p3_ail_nosplitk", 3, a_il=1, splitk=0)]
G256 = {"g256": [_route("g256_k1", 3, a_il=1, route=1, hint=1)], "g256sk": [_route("g256_k2", 3, a_il=1, route=1, hint=2)],
        "qkv": [_route("g256_k1", 3, a_il=1, route=1, hint=1), _route("g256_k1_n192off", 3, a_il=1, route=1, hint=1, n192=0)]}
LEFTOVER = ("tail", "g256", "g256sk", "qkv", "conv", "convt_tail")      # M % 128 in 1..8 (splitk too, once split-K is off: NOSPLITK)


def routes_for(case):
    shape = case.name.split("/")[1]
    rs = list(BASE[:2]) if shape in ("g256", "g256sk") else list(BASE)
    if shape in LEFTOVER:
        rs += NOTAIL
    if shape in ("splitk", "convsk"):
        rs += NOSPLITK
    return rs + G256.get(shape, [])


PARAMS = [pytest.param(c, r, id=f"{c.name}-{r['name']}") for c in R.CASES for r in routes_for(c)]


def _lib():
    from ovmono3d_amd import lib
    return lib, lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def case_at(case, precision):
    """Split-K needs 32 k-steps: K = 1024 at f16x3 (steps of 32), K = 2048 at f16 (steps of 64)."""
    if case.name.endswith("/splitk") and precision == 1:
        return R.with_k(case, R.SPLITK_K_F16)
    return case


@lru_cache(maxsize=None)
def _inputs(name, K, family):
    case = R.CASE_BY_NAME[name.split("@")[0]]
    return R.make_inputs(R.with_k(case, K) if K != case.K else case, family)


@lru_cache(maxsize=None)
def _reference(name, K, family, precision):
    case = R.CASE_BY_NAME[name.split("@")[0]]
    case = R.with_k(case, K) if K != case.K else case
    return R.reference(case, _inputs(name, K, family), precision)


def launch(case, inp, route, device):
    """-> (return code, {output name: fp32 CPU buffer}); the tune keys are restored whatever happens."""
    lib, L = _lib()
    dev = {k: v.to(device).contiguous() for k, v in inp.items()}
    d = lib.OvmGemmEpiOp()
    d.epi, d.amode, d.precision, d.a_il, d.route, d.ksplit_hint = case.epi, 1 if case.conv else 0, route["precision"], route["a_il"], route["route"], route["hint"]
    d.M, d.N, d.K = case.M, case.N, case.K
    if case.conv:
        _, d.cH, d.cW, d.cC = case.conv
    ptr = lambda k: dev[k].data_ptr() if k in dev else None
    d.A, d.W, d.bias = ptr("A"), ptr("W"), ptr("bias")
    d.gamma, d.X, d.row_map, d.ldx, d.relu = ptr("gamma"), ptr("X"), ptr("row_map"), case.ldx, case.relu
    d.C, d.ldc, d.ldo = ptr("C"), case.ldc, case.ldo
    if "O" in dev:
        d.O, d.o_elems = dev["O"].data_ptr() + 4 * case.o_off, dev["O"].numel() - case.o_off
    d.o_il, d.relu_o = case.o_il, case.relu_o
    d.R, d.R2, d.ldr, d.ldr2 = ptr("R"), ptr("R2"), case.ldr, case.ldr2
    if case.pad:
        d.padH, d.padW = case.pad[1], case.pad[2]
    if case.epi == R.CONVT and case.border:
        d.padH = d.padW = 2 * case.G
    d.Q, d.Kout, d.Vt, d.T, d.Tpad, d.heads, d.qscale = ptr("Q"), ptr("Kout"), ptr("Vt"), case.T, case.Tpad, case.heads, R.Q_SCALE
    d.pos, d.G2, d.G, d.Cout = ptr("pos"), case.G2, case.G, case.Cout
    try:
        for k, v in route["tune"].items():
            assert L.ovm_tune_set(k.encode(), v) == 0
        rc = L.ovm_op_gemm_epi(C.byref(d), _stream())
        if rc != -2:
            torch.cuda.synchronize()
    finally:
        for k, v in TUNE_DEFAULTS.items():
            L.ovm_tune_set(k.encode(), v)
    if rc == -2:      # OVM_ERR_HIP: the context is lost, every later GPU test would only repeat the error
        pytest.exit(f"{case.name} {route['name']}: HIP error inside ovm_op_gemm_epi, stopping the session", returncode=3)
    return rc, {k: dev[k].cpu() for k in ("C", "O", "X", "Q", "Kout", "Vt") if k in dev}


def run_and_check(case, route, device):
    case = case_at(case, route["precision"])
    for family in R.families(case):
        inp = _inputs(case.name, case.K, family)
        ref = _reference(case.name, case.K, family, route["precision"])
        rc, got = launch(case, inp, route, device)
        assert rc == 0, f"{case.name} [{family}] {route['name']}: ovm_op_gemm_epi returned {rc}"
        report = lambda out, err, tol: print(f"FIG {case.name} {route['name']} {out} err {err:.3e} bound {tol:.2e}")
        R.check(case, family, route["precision"], got, ref, report)


@pytest.mark.parametrize("case,route", PARAMS)
def test_epilogue(device, case, route):
    run_and_check(case, route, device)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.name.split("/")[1] in LEFTOVER],
                         ids=lambda c: c.name)
@pytest.mark.parametrize("precision", [1, 3])
def test_leftover_rows_agree_with_the_tile_path(device, case, precision):
    """gemm_tail 1 (dot-product workgroups for the leftover rows) and gemm_tail 0 (one more row of MFMA tiles) agree: exactly in the
    exact family, within the case's tolerance otherwise."""
    for family in R.families(case):
        inp = _inputs(case.name, case.K, family)
        ref = _reference(case.name, case.K, family, precision)
        rc1, on = launch(case, inp, _route("tail", precision, tail=1), device)
        rc0, off = launch(case, inp, _route("notail", precision, tail=0), device)
        assert rc1 == 0 and rc0 == 0
        for o in ref:
            a, b = R.gather(o, on[o.name]), R.gather(o, off[o.name])
            if family == "exact" and o.exact:
                assert torch.equal(a, b), f"{case.name}/{o.name}"
            else:
                err = float((a - b).abs().max() / o.val.abs().max())
                assert err <= R.tolerance(case, precision, o), f"{case.name}/{o.name}: {err:.3e}"


# ------------------------------------------------------------------------------------------------ what the launchers refuse, or reroute
def _untouched(inp, got):
    return all(torch.equal(got[k], inp[k].reshape(got[k].shape)) for k in got)


def test_convt_with_conv_input_is_refused(device):
    case = R.Case("convt_conv", R.CONVT, 162, 128, 576, conv=(2, 9, 9, 64), B=2, G=9, Cout=32)
    inp = R.make_inputs(case, "exact")
    for precision in (1, 3):
        rc, got = launch(case, inp, _route("p", precision), device)
        assert rc == -1 and _untouched(inp, got)              # OVM_ERR_INVALID: the convolution A mode has the store epilogue only


@pytest.mark.parametrize("name,kw", [("store_plain/ragged", {}), ("patch_lead1/tail", {}), ("convt_plain/convt", {}),
                                     ("store_plain/g256", {"precision": 1}), ("store_plain/g256", {"a_il": 0})])
def test_gemm256_refuses_what_it_does_not_support(device, name, kw):
    """N % 256 != 0, an epilogue it has no instance of, one-pass precision, planar A: OVM_ERR_INVALID, nothing written."""
    case = R.CASE_BY_NAME[name]
    inp = R.make_inputs(case, "exact")
    rc, got = launch(case, inp, _route("g256", **{"precision": 3, "a_il": 1, "route": 1, **kw}), device)
    assert rc == -1 and _untouched(inp, got)


def test_conv_channels_not_a_multiple_of_64(device):
    """cC = 32: K = 288 is no multiple of 64. One-pass mode (k-steps of 64) refuses it with OVM_ERR_SHAPE; split mode (k-steps of 32)
    runs it, with the leftover rows as a row of tiles (the dot-product body needs 64-wide k-groups inside one tap)."""
    case = R._store("full", "conv_c32", 132, 72, 288, (1, 3, 44), "full", conv=(1, 3, 44, 32), seed=901)
    for family in ("exact", "float"):
        inp = R.make_inputs(case, family)
        rc, got = launch(case, inp, _route("p1", 1), device)
        assert rc == -4 and _untouched(inp, got)
        for route in (_route("p3", 3), _route("p3_ail_sym", 3, a_il=1, stages=2)):
            rc, got = launch(case, inp, route, device)
            assert rc == 0
            R.check(case, family, 3, got, R.reference(case, inp, 3))


@pytest.mark.parametrize("epi", ["store", "resid"])
def test_split_k_is_skipped_when_n_is_not_a_multiple_of_4(device, epi):
    """N = 126 at the split-K shape: the reduce pass works on 4-column vectors, so the launcher keeps the whole K in one workgroup
    (and the 2 leftover rows on the dot-product body) and the result is still right."""
    M, N, K = 130, 126, 1024
    case = (R.Case("store_plain/n126", R.STORE, M, N, K, ldc=N + 3, ldo=N + 8, seed=902) if epi == "store" else
            R.Case("resid_gamma_map/n126", R.RESID, M, N, K, gamma=True, row_map=True, ldx=N + 2, seed=903))
    for family in ("exact", "float"):
        inp = R.make_inputs(case, family)
        rc, got = launch(case, inp, _route("p3", 3), device)
        assert rc == 0
        R.check(case, family, 3, got, R.reference(case, inp, 3))


def test_adapter_argument_errors(device):
    lib, L = _lib()
    case = R.Case("k48", R.STORE, 8, 8, 48, ldc=8)
    inp = R.make_inputs(case, "exact")
    rc, got = launch(case, inp, _route("p3", 3), device)
    assert rc == -4 and _untouched(inp, got)                  # no 32-wide k-step: OVM_ERR_SHAPE
    d = lib.OvmGemmEpiOp()
    assert L.ovm_op_gemm_epi(C.byref(d), _stream()) == -1 and L.ovm_op_gemm_epi(None, _stream()) == -1
