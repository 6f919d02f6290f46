"""tests/sam_dp_glue_ref.py on the CPU: the fp64 restatement against torch itself in float64 wherever torch has the operation, on the
case lists the GPU test runs; every named mutation rejected by the GPU test's own comparison routine on every case it applies to; and
the conditions of the mask band rule met by the reference alone."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import sam_dp_glue_ref as S
from sam_dp_glue_ref import F32, F64

T64 = dict(dtype=torch.float64)
ATOL = 1e-11                       # float64 against float64 on values of order 1 .. 100, sums of at most a few hundred terms


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _close(a, b, what, atol=ATOL):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    err = float(np.max(np.abs(a - b))) if b.size else 0.0
    assert err <= atol * scale, f"{what}: {err:.3e}"


def _cases(kernel):
    return [pytest.param(c, id=S.case_id(c)) for c in S.CASES[kernel]]


def _interp(x_hwc, size=None, scale=None):
    """F.interpolate of a [H][W][C] array"""
    t = _t(x_hwc).permute(2, 0, 1)[None]
    y = Fn.interpolate(t, size=size, scale_factor=scale, mode="bilinear", align_corners=False)
    return y[0].permute(1, 2, 0).numpy()


# ================================================================================================ against torch, float64
@pytest.mark.parametrize("case", _cases("pyramid"))
def test_pyramid_is_f_interpolate(case):
    inp = S.inputs("pyramid", case)
    r = S.run("pyramid", case, inp, F64)
    img = inp["img"][..., ::-1] if case["flip"] else inp["img"]
    x = (img.astype(F64) / 255.0 - 0.5) / 0.5
    P0 = _interp(x, size=(case["S"], case["S"]))
    _close(r["P0"], P0, "level 0")
    _close(r["P1"], _interp(P0, scale=0.5), "level 1")
    _close(r["P2"], _interp(P0, scale=0.25), "level 2")


@pytest.mark.parametrize("case", _cases("merge"))
def test_merge_is_crop_concatenate_resize(case):
    """Hugging Face merge_patches written with torch slicing and torch.cat, then F.interpolate"""
    inp = S.inputs("merge", case)
    g, n, pad, D = case["g"], case["n"], case["pad"], case["D"]
    t = _t(inp["tok"])[case["crop0"]:case["crop0"] + n * n, 1:].reshape(n, n, g, g, D)
    rows = []
    for i in range(n):
        cols = []
        for j in range(n):
            p = t[i, j]
            if n > 1:
                if i != 0:
                    p = p[pad:]
                if j != 0:
                    p = p[:, pad:]
                if i != n - 1:
                    p = p[:p.shape[0] - pad] if pad else p
                if j != n - 1:
                    p = p[:, :p.shape[1] - pad] if pad else p
            cols.append(p)
        rows.append(torch.cat(cols, dim=1))
    m = torch.cat(rows, dim=0).numpy()
    assert m.shape[0] == case["Ms"]
    want = m if case["out"] == case["Ms"] else _interp(m, size=(case["out"], case["out"]))
    _close(S.run("merge", case, inp, F64)["map"], want, "merged map")


@pytest.mark.parametrize("case", _cases("conv_s2"))
def test_conv_s2_is_conv2d(case):
    inp = S.inputs("conv_s2", case)
    y = Fn.conv2d(_t(inp["x"]).permute(2, 0, 1)[None], _t(inp["w"]).permute(0, 3, 1, 2), _t(inp["bias"]), stride=2, padding=1)
    y = torch.relu(y)[0].permute(1, 2, 0)
    if case["add"]:
        y = y + _t(inp["add"][:, :case["Cout"]]).reshape(y.shape)
    _close(S.run("conv_s2", case, inp, F64)["out"], y.numpy(), "conv_s2")


@pytest.mark.parametrize("case", _cases("head_tail"))
def test_head_tail_is_conv_relu_conv_relu(case):
    inp = S.inputs("head_tail", case)
    x, w = _t(S.seen(inp["x"], case["precision"])), _t(S.seen(inp["w"], case["precision"]))
    h = torch.relu(Fn.conv2d(x.permute(2, 0, 1)[None], w.permute(0, 3, 1, 2), _t(inp["b1"]), padding=1))
    y = torch.relu(Fn.conv2d(h, _t(inp["w2"]).reshape(1, 32, 1, 1), _t(inp["b2"])))[0, 0]
    _close(S.run("head_tail", case, inp, F64)["out"], y.numpy(), "head tail")


@pytest.mark.parametrize("case", _cases("ln_gelu"))
def test_ln_gelu_is_layer_norm_gelu(case):
    inp = S.inputs("ln_gelu", case)
    y = Fn.gelu(Fn.layer_norm(_t(inp["x"]), (case["D"],), _t(inp["gamma"]), _t(inp["beta"]), eps=float(F32(1e-6))))
    _close(S.run("ln_gelu", case, inp, F64)["y"], y.numpy(), "ln + gelu")


@pytest.mark.parametrize("case", _cases("i2t_attn"))
def test_i2t_attn_is_softmax_attention(case):
    inp = S.inputs("i2t_attn", case)
    (heads, G2), nt, nb = case["hg"], case["nt"], case["nb"]
    q = _t(inp["q"]).reshape(nb, G2, heads, 16).permute(0, 2, 1, 3)
    k, v = (_t(inp[n]).reshape(nb, nt, heads, 16).permute(0, 2, 1, 3) for n in ("k", "v"))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(16.0), dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(nb * G2, heads * 16)
    _close(S.run("i2t_attn", case, inp, F64)["o"], o.numpy(), "attention")
    if case["spread"]:
        assert float((q @ k.transpose(-1, -2) / 4.0).abs().max()) > 30.0 and float(p.max(dim=-1).values.median()) > 0.9


@pytest.mark.parametrize("case", _cases("mask_out"))
def test_mask_logits_are_postprocess_masks(case):
    inp = S.inputs("mask_out", case)
    H, W = case["hw"]
    nh, nw = S.preprocess_shape(H, W, 32)
    lg = _t(inp["logits"][:, 1 if case["plane"] else 0])[:, None]
    m = Fn.interpolate(lg, (32, 32), mode="bilinear", align_corners=False)[..., :nh, :nw]
    m = Fn.interpolate(m, (H, W), mode="bilinear", align_corners=False)[:, 0]
    _close(S.run("mask_out", case, inp, F64)["mask"], m.numpy(), "postprocess_masks")


@pytest.mark.parametrize("case", _cases("depth_out"))
def test_depth_out_is_interpolate_and_clamp(case):
    inp = S.inputs("depth_out", case)
    H, W = case["hw"]
    kind, val = case["focal"]
    f = float(F32(val)) if kind == "f" else 0.5 * W / math.tan(0.5 * math.radians(float(F32(val))))
    inv = Fn.interpolate((_t(inp["canon"]) * W / f)[None, None], (H, W), mode="bilinear", align_corners=False)[0, 0]
    d = 1.0 / torch.clamp(inv, 1e-4, 1e4)
    r = S.run("depth_out", case, inp, F64)
    _close(r["depth"], d.numpy(), "depth", atol=1e-10)
    assert float(d.max()) == 1e4 and abs(float(d.min()) - 1e-4) < 1e-15, "the case must reach both clamps"
    _close(r["f"], [f], "focal length")


def test_mask_prod_follows_the_transposed_convolutions():
    """The blocked layout is what two ConvTranspose2d(k 2, s 2) leave when run as GEMMs over source pixels: build the map with torch's
    conv_transpose2d and block it by the header's rule; unblock must give the map back."""
    g = np.random.default_rng(5)
    for case in S.CASES["mask_prod"]:
        G, C8, nb = case["G"], case["C8"], case["nb"]
        x = torch.from_numpy(g.standard_normal((nb, 3, G, G)))
        w1, w2 = torch.from_numpy(g.standard_normal((3, 5, 2, 2))), torch.from_numpy(g.standard_normal((5, C8, 2, 2)))
        mid = Fn.conv_transpose2d(x, w1, stride=2)                                   # [nb][5][2G][2G]
        full = Fn.conv_transpose2d(mid, w2, stride=2).permute(0, 2, 3, 1).numpy()    # [nb][4G][4G][C8]
        # rows = (n, i, j, a, b): pixel (2 i + a, 2 j + b) of `mid`; columns (a2, b2, co) = mid_pixel . w2[:, co, a2, b2]
        rows = mid.permute(0, 2, 3, 1).reshape(nb, G, 2, G, 2, 5).permute(0, 1, 3, 2, 4, 5).reshape(nb * G * G * 4, 5)
        up = (rows @ w2.permute(0, 2, 3, 1).reshape(5, 4 * C8)).numpy()
        _close(S.unblock(up, nb, G, C8), full, "unblocked map")
        # the product on fp32 inputs (as the kernel receives them), the map rebuilt by a reshape of the rows (n, i, j, a, b | a2, b2, co)
        up32, hyper = up.astype(F32), g.standard_normal((nb, 4, C8)).astype(F32)
        full32 = _t(up32).reshape(nb, G, G, 2, 2, 2, 2, C8).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(nb, 4 * G, 4 * G, C8)
        _close(full32.numpy(), full, "reshaped map", atol=1e-6)
        t0, ntk, _ = case["tk"]
        want = torch.einsum("ntc,nyxc->ntyx", _t(hyper)[:, t0:t0 + ntk], full32)
        _close(S.mask_prod(up32, hyper, t0, ntk, C8, G, nb, F64), want.numpy(), "mask product")


def test_dense_pe_and_box_tokens_follow_segment_anything():
    """PositionEmbeddingRandom / PromptEncoder._embed_boxes restated with torch"""
    for case in S.CASES["dense_pe"]:
        inp = S.inputs("dense_pe", case)
        G = case["G"]
        grid = torch.ones((G, G), **T64)
        y, x = (grid.cumsum(0) - 0.5) / G, (grid.cumsum(1) - 0.5) / G
        c = (2 * torch.stack([x, y], -1) - 1) @ _t(inp["gauss"]) * (2 * np.pi)
        _close(S.run("dense_pe", case, inp, F64)["pe"], torch.cat([c.sin(), c.cos()], -1).reshape(G * G, -1).numpy(), "dense pe")
    for case in S.CASES["box_tokens"]:
        inp = S.inputs("box_tokens", case)
        H, W, Sz = case["frame"]
        nh, nw = S.preprocess_shape(H, W, Sz)
        b = inp["boxes"].astype(F64).reshape(-1, 2, 2).copy()
        b[..., 0] *= nw / W
        b[..., 1] *= nh / H
        c = (torch.from_numpy(b) + 0.5) / Sz
        c = (2 * c - 1) @ _t(inp["gauss"]) * (2 * np.pi)
        want = torch.cat([c.sin(), c.cos()], -1) + _t(inp["corner"])[None]
        _close(S.run("box_tokens", case, inp, F64)["corners"], want.numpy(), "box corners")
        assert nh != nw


def test_token_attention_helpers_are_torch_bmm():
    g = np.random.default_rng(6)
    nb, hd, nt, Tk, dh = 2, 3, 7, 11, 16
    Q, K, V = (g.standard_normal((nb * t, hd * dh)).astype(F32) for t in (nt, Tk, Tk))
    q, k, v = (_t(a).reshape(nb, -1, hd, dh).permute(0, 2, 1, 3) for a in (Q, K, V))
    s = q @ k.transpose(-1, -2) * 0.25
    _close(S.token_scores(Q, K, nb, hd, nt, Tk, dh, 0.25, F64), s.numpy(), "scores")
    _close(S.softmax(s.numpy(), F64), torch.softmax(s, -1).numpy(), "softmax")
    p = torch.softmax(s, -1).float().double()                      # the probabilities reach the second product as an fp32 buffer
    _close(S.token_context(p.numpy(), V, nb, hd, nt, Tk, dh, F64), (p @ v).permute(0, 2, 1, 3).reshape(nb * nt, hd * dh).numpy(), "context")


# ================================================================================================ the comparison itself
@pytest.mark.parametrize("kernel", S.KERNELS)
def test_fp32_run_passes_and_every_mutation_is_rejected(kernel):
    """compare() is the routine of the GPU test. A device that computes the fp32 run passes on every case; one that computes any
    applicable mutation of any case is rejected."""
    seen = set()
    for case in S.CASES[kernel]:
        inp = S.inputs(kernel, case)
        r64, r32 = S.run(kernel, case, inp, F64), S.run(kernel, case, inp, F32)
        S.compare(kernel, case, S.as_device(kernel, case, r32), r64, r32)
        for mut in S.mutations_for(kernel, case):
            seen.add(mut)
            bad = S.as_device(kernel, case, S.run(kernel, case, inp, F32, mut))
            with pytest.raises(AssertionError):
                S.compare(kernel, case, bad, r64, r32)
    for mut in seen:
        assert mut in S.MUTATIONS


def test_every_listed_mutation_applies_somewhere():
    used = {m for k in S.KERNELS for c in S.CASES[k] for m in S.mutations_for(k, c)}
    assert used == set(S.MUTATIONS), sorted(set(S.MUTATIONS) ^ used)


def test_case_lists_cover_the_branches():
    """The properties the case lists exist for, stated on the lists themselves."""
    mo = S.CASES["mask_out"]
    assert {(c["nb"] * c["hw"][0] * c["hw"][1]) % 4 != 0 for c in mo} == {True, False}          # the byte-store tail both ways
    assert any(c["hw"][0] > c["hw"][1] for c in mo) and any(c["hw"][0] < c["hw"][1] for c in mo)
    for c in S.CASES["box_tokens"]:
        H, W, Sz = c["frame"]
        nh, nw = S.preprocess_shape(H, W, Sz)
        assert nw / W != nh / H
    mg = S.CASES["merge"]
    for trip in {(c["g"], c["n"], c["pad"]) for c in mg}:
        sub = [c for c in mg if (c["g"], c["n"], c["pad"]) == trip]
        assert {c["out"] == c["Ms"] for c in sub} == {True, False}
        assert {c["crop0"] for c in sub} == {0, 2} and {c["lo"] for c in sub} == {True, False}
    for c in mg:                                                                              # class-token rows are poisoned
        assert np.all(S.inputs("merge", c)["tok"][:, 0] == S.SENTINEL)


# ================================================================================================ the mask band rule, on the reference alone
@pytest.mark.parametrize("case", _cases("mask_out"))
def test_mask_band_cap_is_met_by_the_reference(case):
    inp = S.inputs("mask_out", case)
    r64, r32 = (S.run("mask_out", case, inp, d)["mask"] for d in (F64, F32))
    band = S.band_of(r64, r32)
    std = float(inp["logits"].std())
    assert 5.0 < std < 20.0, std
    assert band < 1e-3 * std, f"band {band:.2e} against logits of standard deviation {std:.1f}"
    assert max(S.left_out_share(r64, band)) <= S.MAX_LEFT_OUT
    for plane in r64:                                       # both classes present: a constant mask would prove nothing
        assert (plane > 0).any() and (plane <= 0).any()
