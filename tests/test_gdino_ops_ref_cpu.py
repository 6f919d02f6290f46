"""CPU self-check of tests/gdino_ops_ref.py and tests/gdino_caption_cases.py: each float64 restatement agrees with an independent
implementation, and the seeded captions have the properties the GPU tests rely on (no GPU, no native library)."""
import pytest
import torch
import torch.nn.functional as F

import gdino_caption_cases as CC
import gdino_ops_ref as R

TIGHT = 1e-12           # two float64 evaluations of the same formula


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_attn_ref_matches_scaled_dot_product_attention():
    g = torch.Generator().manual_seed(0)
    nb1, nb2, Tq, Tk, DH, gw = 2, 3, 20, 35, 16, 7
    buf = _randn(g, nb1, Tq, 3 * nb2 * DH + 8)                   # q | k | v of all heads in one row, as the engine lays them out
    q = buf[:, :, :nb2 * DH].reshape(nb1, Tq, nb2, DH).permute(0, 2, 1, 3)
    kbuf, vbuf = _randn(g, nb1, Tk, nb2 * DH), _randn(g, nb1, Tk, nb2 * DH)
    k = kbuf.reshape(nb1, Tk, nb2, DH).permute(0, 2, 1, 3)
    v = vbuf.reshape(nb1, Tk, nb2, DH).permute(0, 2, 1, 3)
    bias_h = _randn(g, nb2, Tq, Tk)
    bias_b = torch.where(torch.rand(nb1, Tq, Tk, generator=g) < 0.3, torch.finfo(torch.float32).min, 0.0).double()
    bias_b[:, :, 0] = 0.0                                        # every row keeps a key
    rel_h, rel_w = _randn(g, nb1, Tq, nb2, 5), _randn(g, nb1, Tq, nb2, gw)
    scale = DH ** -0.5
    got = R.attn_ref(q, k, v, scale, bias_h, bias_b, rel_h, rel_w, gw)
    key = torch.arange(Tk)
    mask = bias_h[None] + bias_b[:, None] + (rel_h[..., key // gw] + rel_w[..., key % gw]).permute(0, 2, 1, 3)
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale)
    assert R.rel_err(got, want) < TIGHT
    # a shared bias_b (sbb = 0) and no tables
    got = R.attn_ref(q, k, v, scale, None, bias_b[:1])
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=bias_b[:1, None].expand(nb1, nb2, Tq, Tk), scale=scale)
    assert R.rel_err(got, want) < TIGHT
    # masked keys do not reach the output, however large their values
    v2 = v.clone()
    v2[:, :, 1:] = torch.where((bias_b[:, None, 0, 1:, None] < 0).expand_as(v2[:, :, 1:]), 1e30, v2[:, :, 1:])
    bb = bias_b[:, :1].expand(nb1, Tq, Tk)
    assert torch.equal(R.attn_ref(q, k, v2, scale, None, bb), R.attn_ref(q, k, v, scale, None, bb))


@pytest.mark.parametrize("P,L", [(4, 4), (3, 3)])
def test_msdeform_ref_matches_hf_module(P, L):
    from transformers.models.grounding_dino.modeling_grounding_dino import MultiScaleDeformableAttention
    g = torch.Generator().manual_seed(1)
    shapes = [(7, 9), (4, 5), (2, 3), (1, 1)][:L]
    S, Q, H, dh = sum(h * w for h, w in shapes), 11, 3, 8
    n = H * L * P
    value = _randn(g, S, H * dh)
    ow = torch.cat([_randn(g, Q, 2 * n) * 2.0, _randn(g, Q, n)], 1)
    ref = torch.rand(Q, 2, generator=g, dtype=torch.float64)
    got = R.msdeform_ref(value, ow, ref, 0, H, dh, L, P, shapes)
    loc, w = R.msdeform_locations(ow, ref, 0, H, L, P, shapes)
    # HF's own location formula (GroundingDinoMultiscaleDeformableAttention.forward, num_coordinates == 2)
    norm = torch.tensor([[w_, h_] for h_, w_ in shapes], dtype=torch.float64)
    off = ow[:, :2 * n].reshape(Q, H, L, P, 2)
    loc_hf = ref[:, None, None, None, :] + off / norm[None, None, :, None, :]
    assert torch.equal(loc, loc_hf)
    start = torch.tensor([0] + [h * w_ for h, w_ in shapes]).cumsum(0)[:-1]
    want = MultiScaleDeformableAttention()(value.reshape(1, S, H, dh), torch.tensor(shapes), shapes, start, loc_hf[None], w[None], 64)[0]
    assert R.rel_err(got, want) < TIGHT
    # mode 1 differs in the locations only: a box with w = h = 0 samples its centre with every point
    box = torch.cat([ref, torch.zeros(Q, 2, dtype=torch.float64)], 1)
    loc1, _ = R.msdeform_locations(ow, box, 1, H, L, P, shapes)
    assert torch.equal(loc1, ref[:, None, None, None, :].expand_as(loc1))
    box[:, 2:] = 0.5
    loc1, _ = R.msdeform_locations(ow, box, 1, H, L, P, shapes)
    assert R.rel_err(loc1, ref[:, None, None, None, :] + off / P * 0.5 * 0.5) < TIGHT


def test_rowop_ref_matches_layer_norm_and_indexing():
    g = torch.Generator().manual_seed(2)
    M, seg, nidx, N = 9, 12, 2, 14
    D = seg * nidx
    x = _randn(g, N, seg + 4)
    idx = torch.randint(-1, N, (M, nidx), generator=g)
    idx[0, 0], idx[1, 1], idx[2] = -1, -1, -1
    res, gamma, beta, add = _randn(g, M, D), _randn(g, D), _randn(g, D), _randn(g, 4, D)
    for zero_masked in (False, True):
        y, y2 = R.rowop_ref(x, M, D, idx, seg, res, gamma, beta, 1e-5, zero_masked, add, 4)
        for r in range(M):
            row = torch.cat([x[int(i), :seg] if i >= 0 else torch.zeros(seg, dtype=torch.float64) for i in idx[r]]) + res[r]
            want = F.layer_norm(row, (D,), gamma, beta, 1e-5)
            if zero_masked and idx[r, 0] < 0:
                want = torch.zeros_like(want)
            assert R.rel_err(y[r], want) < TIGHT or float(want.abs().max()) == float(y[r].abs().max()) == 0.0
            assert torch.equal(y2[r], y[r] + add[r % 4])
    # no gather, no norm: a copy (+ residual)
    y, y2 = R.rowop_ref(x, 5, seg, res=res[:, :seg])
    assert y2 is None and torch.equal(y, x[:5, :seg] + res[:5, :seg])
    # the split image and the interleaved column map
    y32 = (torch.randn(64, generator=g) * torch.tensor([1e-3, 1.0, 300.0, 1e4]).repeat(16)).clamp(-6e4, 6e4)
    hi, lo = R.split_f16(y32)
    # two fp16 significands (22 bits) down to the fp16 subnormal spacing 2^-24
    assert ((hi.double() + lo.double() - y32.double()).abs() <= 2.0 ** -21 * y32.double().abs() + 2.0 ** -25).all()
    assert [R.il_col(n) for n in (0, 31, 32, 63, 64, 255)] == [0, 31, 64, 95, 128, 479]


@pytest.mark.parametrize("T", CC.ENGINE_T)
def test_caption_builder(T):
    from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map
    ids = CC.caption_ids(T, seed=0)
    assert len(ids) == T and ids[0] == CC.CLS and ids[-1] == CC.SEP and ids[-2] == CC.DELIM
    assert ids == CC.caption_ids(T, seed=0) and ids != CC.caption_ids(T, seed=1)
    body = ids[1:-1]
    assert all(t == CC.DELIM or 200 <= t < 1000 for t in body)
    runs = [len(p) for p in " ".join("." if t == CC.DELIM else "w" for t in body).replace(" ", "").split(".")[:-1]]
    assert runs and all(1 <= n <= 3 for n in runs)
    mask = CC.phrase_mask(ids)
    hf_mask, _ = generate_masks_with_special_tokens_and_transfer_map(torch.tensor(ids)[None])
    assert torch.equal(mask, hf_mask[0])
    assert mask.any(dim=1).all()                                  # every query keeps at least one key
    blind = CC.blind_rows(mask)
    print(f"T = {T}: {len(runs)} phrases, {blind} queries whose first {CC.KEY_CHUNK} keys are all masked")
    if T <= CC.KEY_CHUNK:
        assert blind == 0
    if T in (147, 256):
        assert blind >= 1


# ------------------------------------------------------------------------------------------------------------------------
# The bound of tests/test_gpu_gdino_ops.py is tight enough to see the mistakes these kernels can make: each of the slips below,
# applied to PyTorch's fp32 evaluation on that file's own case inputs, lands outside the case's bound (and the unmutated
# evaluation inside it, so the harness itself is not what fails).
def _flash(q, k, v, scale, bias=None, chunk=CC.KEY_CHUNK, rescale=True):
    """fp32 attention the way attn_f32_kernel walks it: key chunks, running maximum, accumulators rescaled between chunks"""
    Tk = k.shape[-2]
    m = torch.full(q.shape[:-1], float("-inf"))
    l = torch.zeros(q.shape[:-1])
    o = torch.zeros(q.shape)
    for kc in range(0, Tk, chunk):
        s = q @ k[..., kc:kc + chunk, :].transpose(-1, -2) * scale
        if bias is not None:
            s = s + bias[..., kc:kc + chunk]
        cmax = s.max(-1)[0]
        mnew = torch.maximum(m, cmax)
        msafe = torch.where(torch.isinf(mnew), torch.zeros(()), mnew)
        alpha = torch.exp(m - msafe) if rescale else torch.ones_like(m)
        p = torch.exp(s - msafe[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p @ v[..., kc:kc + chunk, :]
        m = mnew
    return o / l[..., None]


def _attn_views(c):
    E = c["nb2"] * c["DH"]
    heads = lambda t, T: t[:, :, :E].reshape(c["nb1"], T, c["nb2"], c["DH"]).permute(0, 2, 1, 3)
    return heads(c["q"], c["Tq"]), heads(c["k"], c["Tk"]), heads(c["v"], c["Tk"])


def test_gpu_bounds_reject_attention_slips():
    import test_gpu_gdino_ops as G
    for name, slip in (("h", dict(rescale=False)), ("g", dict(rescale=False))):
        # h: the maximum jumps in the second chunk, so the first chunk's sums must shrink (in its mirror case the second chunk
        # hardly counts: that one guards against a rescale that overflows, not against a missing one)
        c = G._attn_case(name)
        q, k, v = _attn_views(c)
        tol = R.bound(c["ref32"], c["ref64"])
        assert R.rel_err(_flash(q, k, v, c["scale"]), c["ref64"]) <= tol, name
        assert R.rel_err(_flash(q, k, v, c["scale"], **slip), c["ref64"]) > 100 * tol, f"{name}: {slip}"
    for name in ("c", "e", "g", "l"):                            # the last key of a tail tile (of the last chunk) lost
        c = G._attn_case(name)
        q, k, v = _attn_views(c)
        assert R.rel_err(R.attn_ref(q, k[:, :, :-1], v[:, :, :-1], c["scale"], dtype=torch.float32), c["ref64"]) > 100 * R.bound(c["ref32"], c["ref64"])
    for name in ("i", "j"):                                      # the phrase mask applied to the first chunk only
        c = G._attn_case(name)
        q, k, v = _attn_views(c)
        bias = c["bias_b"].clone()
        tol = R.bound(c["ref32"], c["ref64"])
        assert R.rel_err(_flash(q, k, v, c["scale"], bias[:, None]), c["ref64"]) <= tol, name
        bias[:, :, CC.KEY_CHUNK:] = 0.0
        assert R.rel_err(_flash(q, k, v, c["scale"], bias[:, None]), c["ref64"]) > 100 * tol, name
    c = G._attn_case("p")                                        # rel_w indexed with the row stride of another grid
    q, k, v = _attn_views(c)
    gw = c["rel_gw"]
    wrong = R.attn_ref(q, k, v, c["scale"], None, None, c["rel_h"], c["rel_w"], gw + 1, dtype=torch.float32)
    assert R.rel_err(wrong, c["ref64"]) > 100 * R.bound(c["ref32"], c["ref64"])


def test_gpu_bounds_reject_deformable_sampling_slips(monkeypatch):
    import test_gpu_gdino_ops as G
    orig = F.grid_sample

    def run(name, **override):
        c = G._msd_case(name)
        n = c["H"] * c["L"] * c["P"]
        monkeypatch.setattr(R.F, "grid_sample", lambda *a, **kw: orig(*a, **{**kw, **override}))
        try:
            got = R.msdeform_ref(c["value"][:, :c["H"] * c["dh"]], c["ow"][:, :3 * n], c["ref"], c["mode"], c["H"], c["dh"], c["L"], c["P"],
                                 c["shapes"], dtype=torch.float32)
        finally:
            monkeypatch.setattr(R.F, "grid_sample", orig)
        return R.rel_err(got, c["ref64"]), R.bound(c["ref32"], c["ref64"])
    for name in ("enc", "dec", "edges_enc", "edges_dec"):
        err, tol = run(name)
        assert err <= tol, name
        err, tol = run(name, padding_mode="border")             # out-of-range taps clamped instead of dropped
        assert err > 100 * tol, f"{name}: border taps"
        err, tol = run(name, align_corners=True)                # pixel centres half a pixel off
        assert err > 100 * tol, f"{name}: align_corners"
    c = G._msd_case("logits80")                                  # softmax over the points of a level instead of all L * P samples
    n, H, L, P = c["H"] * c["L"] * c["P"], c["H"], c["L"], c["P"]
    ow = c["ow"][:, :3 * n].clone()
    lg = ow[:, 2 * n:].reshape(-1, H, L, P)
    ow[:, 2 * n:] = (torch.log_softmax(lg, -1) - torch.log(torch.tensor(float(L)))).reshape(-1, n)
    got = R.msdeform_ref(c["value"][:, :H * c["dh"]], ow, c["ref"], c["mode"], H, c["dh"], L, P, c["shapes"], dtype=torch.float32)
    assert R.rel_err(got, c["ref64"]) > 100 * R.bound(c["ref32"], c["ref64"])


def test_gpu_bounds_reject_row_operator_slips():
    import test_gpu_gdino_ops as G

    def run(name, M, **override):
        c = G._row_case(name, M)
        D, ln, gather, *_ = G.ROWOP[name]
        kw = dict(idx=c.get("idx"), seg=c["seg"], res=c["res"], gamma=c["gamma"], beta=c["beta"], eps=G.EPS, zero_masked=bool(gather),
                  add=c["add"], add_rows=G.ADD_ROWS)
        kw.update(override)
        y, y2 = R.rowop_ref(c["x"], M, D, dtype=torch.float32, **kw)
        k = 0 if c["ref64"][1] is None else 1
        return R.rel_err((y, y2)[k], c["ref64"][k]), R.bound(c["ref32"][k], c["ref64"][k])
    for name, M, override, what in (("ln256_gather_zm_res_add", 130, dict(zero_masked=False), "zero_masked ignored"),
                                    ("ln70_gather_zm_res", 5, dict(res=None), "residual dropped"),
                                    ("ln4096_add", 130, dict(eps=1e-3), "eps"),
                                    ("ln1028_add", 130, dict(add_rows=5), "add row modulus"),
                                    ("copy70_add", 130, dict(add_rows=6), "add row modulus")):
        err, tol = run(name, M)
        assert err <= tol, name
        err, tol = run(name, M, **override)
        assert err > 100 * tol, f"{name}: {what}"
