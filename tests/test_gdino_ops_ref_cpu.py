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


# ------------------------------------------------------------------------------------------------------------------------
# The references of tests/test_gpu_gdino_select.py (the small kernels between the fused ones), each against an independent
# implementation, and - on that file's own case inputs - the slips those kernels could make, each of which must land outside the
# case's bound (float ops) or change at least one index / word (exact ops).
def test_topk_ref_matches_torch_stable_sort():
    import test_gpu_gdino_select as S
    for family, n, k in S.TOPK_CASES + [("seven", 100, 37), ("mix", 100, 37)]:
        s = S._topk_scores(family, n)
        want = torch.sort(s, stable=True, descending=True)[1][:k]
        assert torch.equal(R.topk_ref(s, k), want), f"{family} n {n}"
        assert torch.equal(R.topk_ref(s, k, dtype=torch.float32), want)
    s = torch.tensor([0.0, -0.0, 1.0, -0.0, 0.0, float("-inf"), 1.0])
    assert R.topk_ref(s, 7).tolist() == [2, 6, 0, 1, 3, 4, 5]
    with pytest.raises(AssertionError):
        R.topk_ref(torch.tensor([1.0, float("nan")]), 1)


def _ord_key(s, fold_zero):
    """the kernel's key order restated: the bits of a float as an unsigned integer that ascends with the value"""
    u = s.numpy().view("uint32").astype("int64")
    if fold_zero:
        u[u == 0x80000000] = 0
    return torch.from_numpy(((u ^ 0xFFFFFFFF) * (u >> 31) + (u | 0x80000000) * (1 - (u >> 31))) & 0xFFFFFFFF)


def test_topk_cases_reject_tie_and_signed_zero_slips():
    import test_gpu_gdino_select as S
    seen = {"tie": 0, "zero": 0}
    for family, n, k in S.TOPK_CASES:
        s = S._topk_scores(family, n)
        ref = R.topk_ref(s, k)
        # the key order itself, with -0.0 folded onto +0.0, is the reference's order
        assert torch.equal(torch.sort(_ord_key(s, True), stable=True, descending=True)[1][:k], ref), f"{family} n {n}"
        if family != "distinct" and n > 1:                        # ties resolved to the higher index
            wrong = (n - 1 - torch.sort(s.flip(0), stable=True, descending=True)[1])[:k]
            assert not torch.equal(wrong, ref), f"{family} n {n}: the case does not see the higher index winning"
            seen["tie"] += 1
        if family == "mix" and n > 1:                             # -0.0 sorted below +0.0
            wrong = torch.sort(_ord_key(s, False), stable=True, descending=True)[1][:k]
            assert not torch.equal(wrong, ref), f"mix n {n}: the case does not see -0.0 sorted below +0.0"
            seen["zero"] += 1
    assert seen["tie"] >= 12 and seen["zero"] == 4


def test_box_refine_ref_matches_special_logit_and_rejects_a_missing_clamp():
    import test_gpu_gdino_select as S
    for n in S.BOX_N:
        for ldd in S.BOX_LDD:
            for eps in S.BOX_EPS:
                c = S._box_case(n, ldd, eps)
                e = float(torch.tensor(eps, dtype=torch.float32))
                want = torch.sigmoid(c["delta"][:, :4].double() + torch.special.logit(c["ref"].double(), eps=e))
                assert R.rel_err(c["ref64"], want) < TIGHT
                assert torch.isfinite(c["ref64"]).all() and bool(((c["ref64"] >= 0) & (c["ref64"] <= 1)).all())
                tol = R.bound(c["ref32"], c["ref64"])
                x = c["ref"]                                      # eps not applied
                wrong = torch.sigmoid(c["delta"][:, :4] + torch.log(x / (1 - x)))
                err = R.rel_err(torch.nan_to_num(wrong, nan=2.0), c["ref64"])
                assert err > 100 * tol, f"n {n} ldd {ldd} eps {eps}: {err} against {tol}"
                other = R.box_refine_ref(c["delta"], c["ref"], 1e-4, dtype=torch.float32)            # another eps is outside the bound too
                assert R.rel_err(other, c["ref64"]) > 10 * tol


def test_select_ref_and_pad_logits_refs():
    import test_gpu_gdino_select as S
    for ldc in (4, 8):
        c = S._select_case(ldc)
        for i, s in enumerate(c["idx"].tolist()):
            want = 1 / (1 + torch.exp(-(c["coord"][s, :4].double() + c["prop"][s].double())))
            assert R.rel_err(c["ref64"][i], want) < TIGHT
        assert bool((c["ref64"][c["invalid"]] == 1.0).all()) and bool((c["ref32"][c["invalid"]] == 1.0).all())
        wrong = torch.sigmoid(c["coord"].view(-1)[c["idx"].long()[:, None] * 4 + torch.arange(4)] + c["prop"][c["idx"].long()])
        if ldc != 4:                                              # the row stride taken for 4
            assert R.rel_err(wrong, c["ref64"]) > 100 * R.bound(c["ref32"], c["ref64"])
    for Q in S.PAD_Q:
        for T in S.PAD_T:
            for extra in (0, 3):
                x = S._pad_case(Q, T, extra)
                want = R.pad_logits_ref(x, T, S.PAD_LD)
                assert want.shape == (Q, S.PAD_LD) and torch.equal(want[:, :T], x[:, :T]) and bool((want[:, T:] == float("-inf")).all())
                if T < S.PAD_LD:                                  # -inf written from column T + 1
                    wrong = want.clone()
                    wrong[:, T] = S.SENT
                    assert not torch.equal(wrong.view(torch.int32), want.view(torch.int32))
    for rows in S.ROWMAX_ROWS:
        for cols in S.ROWMAX_COLS:
            x = S._rowmax_case(rows, cols)
            want = R.rowmax_ref(x[:, :cols])
            assert want.tolist() == [max(r) for r in x[:, :cols].tolist()]
            assert bool(torch.isinf(want).any()) and bool((want < 0).all())
            assert bool((x[:, cols:] > 0).all())                  # a read past the width would win every maximum


def test_bert_embed_ref_matches_hf_bert_embeddings():
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings
    import test_gpu_gdino_select as S
    c = S._bert_case(22, 64, "normal")
    cfg = BertConfig(vocab_size=S.BERT_VOCAB, hidden_size=64, max_position_embeddings=S.BERT_POS, type_vocab_size=2, layer_norm_eps=S.BERT_EPS,
                     hidden_dropout_prob=0.0, pad_token_id=0)
    emb = BertEmbeddings(cfg).double().eval()
    with torch.no_grad():
        emb.word_embeddings.weight.copy_(c["word"])
        emb.position_embeddings.weight.copy_(c["pos"])
        emb.token_type_embeddings.weight[0].copy_(c["typ"])
        emb.token_type_embeddings.weight[1].fill_(1e3)            # token type 1 is never used
        emb.LayerNorm.weight.copy_(c["gamma"])
        emb.LayerNorm.bias.copy_(c["beta"])
        want = emb(input_ids=c["ids"].long()[None], token_type_ids=torch.zeros(1, 22, dtype=torch.long), position_ids=c["pids"].long()[None])[0]
    assert R.rel_err(c["ref64"], want) < TIGHT
    assert c["pids"].tolist()[:9] == [0, 0, 1, 2, 3, 4, 0, 1, 2] and int(c["pids"].max()) < S.BERT_POS
    assert c["ids"][0] == 0 and c["ids"][-1] == 49 and c["ids"][1] == c["ids"][2]


def test_bert_embed_cases_reject_layernorm_slips():
    import test_gpu_gdino_select as S

    def one_pass(c, dtype):
        rows = (c["word"].to(dtype)[c["ids"].long()] + c["pos"].to(dtype)[c["pids"].long()]) + c["typ"].to(dtype)
        mean = rows.mean(-1, keepdim=True)
        var = (rows * rows).mean(-1, keepdim=True) - mean * mean
        return (rows - mean) / torch.sqrt(var.clamp_min(0) + S.BERT_EPS) * c["gamma"].to(dtype) + c["beta"].to(dtype)

    c = S._bert_case(22, 768, "offset")
    tol = R.bound(c["ref32"], c["ref64"])
    rows = c["word"][c["ids"].long()]
    assert 99 < float(rows.mean()) < 101 and 0.005 < float(rows.std(-1).mean()) < 0.02
    assert R.rel_err(one_pass(c, torch.float64), c["ref64"]) < 1e-6          # the same function where the precision suffices
    err = R.rel_err(torch.nan_to_num(one_pass(c, torch.float32), nan=1e3, posinf=1e3, neginf=-1e3), c["ref64"])
    assert err > 100 * tol, f"one-pass variance: {err} against {tol}"
    for T, D, kind in S.BERT_CASES:
        c = S._bert_case(T, D, kind)
        tol = R.bound(c["ref32"], c["ref64"])
        args = (c["word"], c["pos"], c["typ"], c["ids"], c["pids"], c["gamma"], c["beta"])
        err = R.rel_err(R.bert_embed_ref(*args, 1e-5, dtype=torch.float32), c["ref64"])         # the engine's other LayerNorms' eps
        print(f"bert_embed T {T} D {D} {kind}: bound {tol:.2e}, eps 1e-5 instead of 1e-12: {err:.2e}")
        assert err > 10 * tol, f"T {T} D {D} {kind}: eps"
        if T > 1:                                                 # the position ids taken for 0 .. T - 1
            wrong = R.bert_embed_ref(c["word"], c["pos"], c["typ"], c["ids"], torch.arange(T) % S.BERT_POS, c["gamma"], c["beta"], S.BERT_EPS,
                                     dtype=torch.float32)
            assert R.rel_err(wrong, c["ref64"]) > 100 * tol, f"T {T} D {D} {kind}: position ids"


def test_normalize_image_ref_and_the_channel_flip():
    import test_gpu_gdino_select as S
    for H, W in S.NORM_SIZES:
        for layout in S.NORM_LAYOUTS:
            for flip in (0, 1):
                c = S._norm_case(H, W, layout, flip)
                img = c["img"]
                assert img[0, 0, 0] == 0 and img[2, 0, 0] == 255
                for y, x, ch in ((0, 0, 0), (H - 1, W - 1, 2), (H // 2, W // 3, 1)):
                    cs = 2 - ch if flip else ch
                    px = int(c["buf"][cs * c["strides"][0] + y * c["strides"][1] + x * c["strides"][2]])
                    want = (px - float(torch.tensor(S.NORM_MEAN[cs]).float())) / float(torch.tensor(S.NORM_STD[cs]).float())
                    assert abs(float(c["ref64"][y, x, ch]) - want) < 1e-13
                tol = R.bound(c["ref32"], c["ref64"])
                assert R.rel_err(c["np32"], c["ref64"]) <= tol
                wrong = R.normalize_image_ref(img, S.NORM_MEAN, S.NORM_STD, 1 - flip, dtype=torch.float32)       # the flip ignored (or forced)
                assert R.rel_err(wrong, c["ref64"]) > 100 * tol, f"{H} x {W} {layout} flip {flip}"
                m = [S.NORM_MEAN[i] for i in (2, 1, 0)]                                                         # the pixel flipped, not its mean
                assert R.rel_err(R.normalize_image_ref(img, m, S.NORM_STD, flip, dtype=torch.float32), c["ref64"]) > 100 * tol


def test_relpos_tables_ref_matches_decomposed_rel_pos_and_rejects_index_slips():
    from oracle.sam_vit import get_rel_pos
    import test_gpu_gdino_select as S
    for name in sorted(S.RELPOS):
        c = S._relpos_case(name)
        gh, gw, H, DH, nseq = S.RELPOS[name]
        q, Rh, Rw = c["q"].double(), c["Rh"].double(), c["Rw"].double()
        # add_decomposed_rel_pos: r_q [B][h][w][C], tables [h][k_h][C] and [w][k_w][C]
        rq = q.reshape(nseq, gh, gw, H, DH).permute(0, 3, 1, 2, 4).reshape(nseq * H, gh, gw, DH)
        want_h = torch.einsum("bhwc,hkc->bhwk", rq, get_rel_pos(gh, gh, Rh))
        want_w = torch.einsum("bhwc,wkc->bhwk", rq, get_rel_pos(gw, gw, Rw))
        back = lambda t, k: t.reshape(nseq, H, gh, gw, k).permute(0, 2, 3, 1, 4).reshape(c["M"], H, k)
        assert R.rel_err(c["ref64"][0], back(want_h, gh)) < TIGHT and R.rel_err(c["ref64"][1], back(want_w, gw)) < TIGHT
        if name == "g1x1":
            continue                                              # one table row: no index to get wrong
        tol = [R.bound(c["ref32"][k], c["ref64"][k]) for k in (0, 1)]
        # the index qh - kh + gh - 1 off by one: the table read one row further down
        off = R.relpos_tables_ref(c["q"], torch.roll(c["Rh"], 1, 0), torch.roll(c["Rw"], 1, 0), gh, gw, dtype=torch.float32)
        assert R.rel_err(off[0], c["ref64"][0]) > 100 * tol[0] and R.rel_err(off[1], c["ref64"][1]) > 100 * tol[1], name
        # the sign of the offset: kh - qh
        neg = R.relpos_tables_ref(c["q"], c["Rh"].flip(0), c["Rw"].flip(0), gh, gw, dtype=torch.float32)
        assert R.rel_err(neg[0], c["ref64"][0]) > 100 * tol[0] and R.rel_err(neg[1], c["ref64"][1]) > 100 * tol[1], name
    # gh and gw swapped inside the kernel: the row's position taken as divmod(t, gh); only a non-square grid can tell
    c = S._relpos_case("g3x5")
    gh, gw = c["gh"], c["gw"]
    t = torch.arange(c["M"]) % (gh * gw)
    qh, qw = t // gh, t % gh
    q32 = c["q"].float()
    wrong_h = torch.stack([q32[m] @ c["Rh"][(int(qh[m]) - torch.arange(gh) + gh - 1).clamp(0, 2 * gh - 2)].T for m in range(c["M"])])
    wrong_w = torch.stack([q32[m] @ c["Rw"][(int(qw[m]) - torch.arange(gw) + gw - 1).clamp(0, 2 * gw - 2)].T for m in range(c["M"])])
    assert R.rel_err(wrong_h, c["ref64"][0]) > 100 * R.bound(c["ref32"][0], c["ref64"][0])
    assert R.rel_err(wrong_w, c["ref64"][1]) > 100 * R.bound(c["ref32"][1], c["ref64"][1])
    # and the composition case: attention from tables with gh and gw swapped is outside its bound
    a = S._relpos_attn_case()
    nseq, T, H, DH = a["nseq"], gh * gw, a["H"], a["DH"]
    heads = lambda x: x[:, :, :H * DH].reshape(nseq, T, H, DH).permute(0, 2, 1, 3)
    qv = a["q"].reshape(nseq, T, H, DH).permute(0, 2, 1, 3)
    rh, rw = (x.reshape(nseq, T, H, -1) for x in R.relpos_tables_ref(a["q"], a["Rh"], a["Rw"], gh, gw, dtype=torch.float32))
    tol = R.bound(a["attn32"], a["attn64"])
    assert R.rel_err(R.attn_ref(qv, heads(a["k"]), heads(a["v"]), a["scale"], None, None, rh, rw, gw, dtype=torch.float32), a["attn64"]) <= tol
    wrong = R.attn_ref(qv, heads(a["k"]), heads(a["v"]), a["scale"], None, None, wrong_h.reshape(nseq, T, H, gh), wrong_w.reshape(nseq, T, H, gw),
                       gw, dtype=torch.float32)
    assert R.rel_err(wrong, a["attn64"]) > 100 * tol
    # the tables read with the key split the other way round (key = kw * gh + kh)
    key = torch.arange(T)
    s = torch.einsum("abqd,abkd->abqk", qv, heads(a["k"])) * a["scale"] + rh.permute(0, 2, 1, 3)[..., key % gh] + rw.permute(0, 2, 1, 3)[..., key // gh]
    assert R.rel_err(torch.softmax(s, -1) @ heads(a["v"]), a["attn64"]) > 100 * tol
