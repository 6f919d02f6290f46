"""CPU self-check of tests/gemm_epi_ref.py: the fp64 restatement agrees with torch, and the comparison the GPU tests use rejects every
listed way in which an epilogue could be subtly wrong (no GPU, no library)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_epi_ref as R

ALL_CASES = R.CASES + [R.with_k(c, R.SPLITK_K_F16) for c in R.CASES if c.name.endswith("/splitk")]


def _close(a, b, tol=1e-12):
    assert tuple(a.shape) == tuple(b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ the restatement against torch
def test_conv3x3_matches_conv2d():
    g = torch.Generator().manual_seed(1)
    B, H, Wd, Cc, N = 2, 5, 7, 6, 10
    x = torch.randn(B, Cc, H, Wd, generator=g, dtype=torch.float64)
    w = torch.randn(N, Cc, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(B * H * Wd, N)
    _close(R.conv3x3_preact(x.permute(0, 2, 3, 1), R.conv_rows(w), (B, H, Wd, Cc)), ref)
    # and the transposed-tap mutation is a different function
    assert float((R.conv3x3_preact(x.permute(0, 2, 3, 1), R.conv_rows(w), (B, H, Wd, Cc), True) - ref).abs().max()) > 0.1


@pytest.mark.parametrize("border,ldo,off", [(False, 0, 0), (True, 48, 16)])
def test_convt_scatter_matches_conv_transpose2d(border, ldo, off):
    g = torch.Generator().manual_seed(2)
    B, G, Cin, Cout = 2, 3, 8, 32
    case = R.Case("t", R.CONVT, B * G * G, 4 * Cout, Cin, B=B, G=G, Cout=Cout, ldo=ldo, o_off=off, border=border)
    x = torch.randint(-3, 4, (B, Cin, G, G), generator=g).float()
    w = torch.randint(-3, 4, (Cin, Cout, 2, 2), generator=g).float()
    b = torch.randint(-3, 4, (Cout,), generator=g).float()
    inp = R.make_inputs(case, "exact")
    inp.update(A=x.permute(0, 2, 3, 1).reshape(-1, Cin).contiguous(), W=R.convt_rows(w).contiguous(), bias=b)
    img = R.render(R.reference(case, inp, 3), 3)["O"]
    bd = 1 if border else 0
    side, ps = 2 * G + 2 * bd, ldo or Cout
    img = img.view(B, side, side, ps)
    ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2).permute(0, 2, 3, 1)
    _close(img[:, bd:side - bd, bd:side - bd, off:off + Cout].double(), ref)
    keep = torch.ones_like(img, dtype=torch.bool)
    keep[:, bd:side - bd, bd:side - bd, off:off + Cout] = False
    assert bool((img[keep] == R.SENTINEL).all())


def test_activations_match_torch():
    z = torch.linspace(-9, 9, 4001, dtype=torch.float64)
    _close(R.gelu_erf(z), F.gelu(z))
    _close(R.gelu_quick(z), z * torch.sigmoid(1.702 * z))


def test_qkv_layout_matches_linear_and_head_split():
    case = R.CASE_BY_NAME["qkv/qkv"]
    inp = R.make_inputs(case, "float")
    outs = {o.name: o for o in R.reference(case, inp, 3)}
    got = R.render(list(outs.values()), 3)
    B, T, H, Tp = case.B, case.T, case.heads, case.Tpad
    qkv = F.linear(R.seen(inp["A"], 3), R.seen(inp["W"], 3), inp["bias"].double()).view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    _close(torch.stack([o.val for o in (outs["Q"], outs["Kout"], outs["Vt"])]),
           torch.stack([(qkv[0] * R.Q_SCALE), qkv[1], qkv[2]]).permute(0, 1, 3, 2, 4).reshape(3, B * T, H * 64))
    _close(got["Q"].view(B, H, T, 64).double(), qkv[0] * R.Q_SCALE, 1e-6)
    _close(got["Kout"].view(B, H, T, 64).double(), qkv[1], 1e-6)
    vt = got["Vt"].view(B, H, 64, Tp)
    t = torch.arange(T)
    _close(vt[..., R.vt_token(t)].double(), qkv[2].transpose(-1, -2), 1e-6)
    assert bool((vt[..., T:] == R.SENTINEL).all())
    # the permutation is an involution that stays inside each group of 16 and moves exactly the tokens whose bits 2 and 3 differ
    t = torch.arange(256)
    tp = R.vt_token(t)
    assert torch.equal(R.vt_token(tp), t) and torch.equal(tp // 16, t // 16) and torch.equal(tp & 3, t & 3)
    assert torch.equal(tp != t, ((t >> 2) & 1) != ((t >> 3) & 1))
    assert R.vt_token(torch.tensor([4]))[0] == 8 and R.vt_token(torch.tensor([9]))[0] == 5


def test_padded_nhwc_and_interleaved_maps():
    case = R.CASE_BY_NAME["store_full/ragged"]
    inp = R.make_inputs(case, "exact")
    o = {x.name: x for x in R.reference(case, inp, 3)}["O"]
    Bp, H, Wd = case.pad
    img = R.render([o], 3)["O"].view(Bp, H + 2, Wd + 2, case.ldo)
    _close(img[:, 1:H + 1, 1:Wd + 1, :case.N].reshape(case.M, case.N).double(), o.val)
    edge = torch.ones(Bp, H + 2, Wd + 2, dtype=torch.bool)
    edge[:, 1:H + 1, 1:Wd + 1] = False
    assert bool((img[edge] == R.SENTINEL).all()) and bool((img[..., case.N:] == R.SENTINEL).all())
    n = torch.arange(128)
    assert torch.equal(R.il_col(n), torch.cat([torch.arange(32) + 64 * q for q in range(4)]))


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_case_list_covers_the_issue():
    names = {c.name for c in ALL_CASES}
    assert len(names) == len(ALL_CASES)
    used = set()
    for c in ALL_CASES:
        used.update(R.mutations_for(c))
    assert used == set(R.MUTATIONS)
    for epi in (R.STORE, R.RESID, R.GELU, R.QKV, R.PATCH, R.CONVT):
        assert any(c.epi == epi for c in ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_reference_passes_its_own_check_and_rejects_every_mutation(case):
    """render(reference) passes `check`; render(mutated reference) fails it, in both precisions and both input families."""
    for family in R.families(case):
        inp = R.make_inputs(case, family)
        for precision in (1, 3):
            ref = R.reference(case, inp, precision)
            if family == "exact":
                for o in ref:       # the exact family's promise: every value is an integer that fp32 and one fp16 hold exactly
                    if o.exact:
                        assert float(o.val.abs().max()) <= 2048 and torch.equal(o.val, o.val.round())
                    assert not bool((o.val == R.SENTINEL).any())
            R.check(case, family, precision, R.render(ref, precision), ref)
            for mut in R.mutations_for(case):
                bad = R.render(R.reference(case, inp, precision, mut), precision)
                with pytest.raises(AssertionError):
                    R.check(case, family, precision, bad, ref)
                    pytest.fail(f"{case.name} [{family}, precision {precision}] accepts mutation {mut}", pytrace=False)
