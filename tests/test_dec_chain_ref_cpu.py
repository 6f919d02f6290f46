"""CPU self-check of tests/dec_chain_ref.py and of the cases of tests/test_gpu_dec_chain.py (no GPU; the native library only for
its host functions): the float64 restatement of the decoder row chains agrees with the Hugging Face port's decoder layer, the
loader's fragment order with a numpy restatement, the bound of every GPU case sees the mistakes this kernel can make, and
dec_chain_supported says what the cases expect."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dec_chain_ref as DR
import gdino_ops_ref as R
import pack_cases

TIGHT = 1e-12           # two float64 evaluations of the same formula


# ------------------------------------------------------------------------------------------------------ the restatement is right
def test_restatement_matches_hf_decoder_layer():
    pytest.importorskip("transformers")
    from transformers import BertConfig, GroundingDinoConfig, SwinConfig
    from transformers.models.grounding_dino import modeling_grounding_dino as M
    D, heads, ffn, P, Q, T = 32, 4, 64, 2, 21, 6
    shapes = [(5, 4), (3, 2), (1, 1)]
    L, S = len(shapes), sum(h * w for h, w in shapes)
    bb = SwinConfig(image_size=64, patch_size=4, embed_dim=8, depths=[1, 1], num_heads=[1, 1], window_size=4, out_indices=[1, 2])
    tc = BertConfig(vocab_size=100, hidden_size=D, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32)
    cfg = GroundingDinoConfig(backbone_config=bb, text_config=tc, d_model=D, decoder_layers=1, decoder_attention_heads=heads,
                              decoder_ffn_dim=ffn, num_queries=Q, num_feature_levels=L, decoder_n_points=P, disable_custom_kernels=True,
                              attn_implementation="eager")
    assert cfg.layer_norm_eps == 1e-5 and cfg.activation_function == "relu" and cfg.query_dim == 4
    torch.manual_seed(0)
    layer = M.GroundingDinoDecoderLayer(cfg).double().eval()
    ref_head = M.GroundingDinoMLPPredictionHead(cfg.query_dim // 2 * D, D, D, 2).double().eval()
    bbox = M.GroundingDinoMLPPredictionHead(D, D, 4, 3).double().eval()
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    with torch.no_grad():
        for m in (layer, ref_head, bbox):                        # HF zero-initialises some of these: every term has to count
            for p in m.parameters():
                p.copy_(rn(*p.shape) * (0.3 if p.dim() > 1 else 0.1))
        hs, text, enc = rn(1, Q, D), rn(1, T, D), rn(1, S, D)
        ref = torch.cat([torch.rand(1, Q, 2, generator=g, dtype=torch.float64), 0.05 + 0.5 * torch.rand(1, Q, 2, generator=g, dtype=torch.float64)], -1)
        ref[0, 0, 0], ref[0, 1, 1], ref[0, 2, 2] = 0.0, 1.0, 3e-6    # both sides of the refinement's clamp
        # --- Hugging Face: GroundingDinoDecoder.forward's loop body for one layer, valid_ratios = 1
        qpos_hf = ref_head(M.encode_sinusoidal_position_embedding(ref, num_pos_feats=D // 2))
        start = torch.tensor([0] + [h * w for h, w in shapes]).cumsum(0)[:-1]
        hs_hf = layer(hidden_states=hs, position_embeddings=qpos_hf, reference_points=ref[:, :, None].expand(1, Q, L, 4),
                      spatial_shapes=torch.tensor(shapes), spatial_shapes_list=shapes, level_start_index=start,
                      vision_encoder_hidden_states=enc, text_encoder_hidden_states=text)[0]
        ref_hf = (bbox(hs_hf) + torch.special.logit(ref, eps=1e-5)).sigmoid()
        # --- the kernels' operands from the same modules
        sa, ca, ms = layer.self_attn, layer.encoder_attn_text, layer.encoder_attn
        lin = {"ref0": ref_head.layers[0], "ref1": ref_head.layers[1], "sa_v": sa.value, "sa_out": sa.out_proj, "ca_q": ca.query,
               "ca_out": ca.out_proj, "msda_out": ms.output_proj, "fc1": layer.fc1, "fc2": layer.fc2, "bb0": bbox.layers[0],
               "bb1": bbox.layers[1], "bb2": bbox.layers[2]}
        op = dict(heads=heads, L=L, P=P, shapes=shapes, eps=cfg.layer_norm_eps, hs=hs[0], ref=ref[0], tk=ca.key(text)[0], tv=ca.value(text)[0],
                  val=ms.value_proj(enc)[0], W={k: m.weight for k, m in lin.items()}, B={k: m.bias for k, m in lin.items()})
        op["W"]["sa_qk"], op["B"]["sa_qk"] = torch.cat([sa.query.weight, sa.key.weight]), torch.cat([sa.query.bias, sa.key.bias])
        op["W"]["offw"] = torch.cat([ms.sampling_offsets.weight, ms.attention_weights.weight])
        op["B"]["offw"] = torch.cat([ms.sampling_offsets.bias, ms.attention_weights.bias])
        op["LN"] = [(m.weight, m.bias) for m in (layer.self_attn_layer_norm, layer.encoder_attn_text_layer_norm, layer.encoder_attn_layer_norm,
                                                 layer.final_layer_norm)]
        Fq = D // 2                                              # HF's own frequency table (float32 arithmetic), one entry per sin / cos pair
        dim_t = torch.arange(Fq, dtype=torch.float32)
        op["dim_t"] = (10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / Fq))[0::2]
        qpos, qk, v = DR.chain_a_ref(op)
        assert R.rel_err(qpos, qpos_hf[0]) < TIGHT
        op["qpos"], op["ctx"] = qpos, DR.self_attention(qk, v, heads)
        hs2, ref_next = DR.chain_b_ref(op)
        assert R.rel_err(hs2, hs_hf[0]) < TIGHT
        assert R.rel_err(ref_next, ref_hf[0]) < TIGHT
        assert DR.chain_b_ref(op, refine=False)[1] is None
        for slip in DR.SLIPS:                                    # and every slip is a different function
            if slip == "tap_x1_weight_wx0":
                continue                                         # lives in this file's bilinear taps (below)
            a, b = DR.chain_a_ref(op, slip=slip), DR.chain_b_ref(op, slip=slip)
            assert max(R.rel_err(x, y) for x, y in zip(a + b, (qpos, qk, v, hs2, ref_next))) > 1e-6, slip


# ----------------------------------------------------------------------------------------------------------- the layout is right
def _frag_order_np(image, N, Kpad):
    """[Npad][Kpad / 32][hi | lo][32] -> [tile][k-step][hi | lo][lane][8], lane = 16 * (group of 8 halves) + row of the tile"""
    Npad = (N + 127) // 128 * 128
    a = image.reshape(Npad // 16, 16, Kpad // 32, 2, 4, 8)       # tile, row, k-step, part, group, e
    return a.transpose(0, 2, 3, 4, 1, 5).reshape(-1)             # tile, k-step, part, group, row, e


@pytest.mark.parametrize("N,K,Kpad", [(4, 256, 256), (12, 32, 32), (512, 160, 160), (256, 2048, 2048)])
def test_frag_order_matches_numpy(N, K, Kpad):
    from ovmono3d_amd import lib
    L = lib.load()
    w = np.random.default_rng(N + K).standard_normal((N, K)).astype(np.float32)
    rc, img = pack_cases.host_image(L, w, Kpad, 3)
    assert rc == 0
    img = np.ascontiguousarray(img).reshape(-1)
    assert len(np.unique(img)) > min(N * K, 1000) // 2          # a permutation of distinct halves, or the comparison shows little
    out = np.full(img.size, 0xABCD, np.uint16)
    assert L.ovm_host_frag_order(img.ctypes.data, N, Kpad, out.ctypes.data) == 0
    assert np.array_equal(out, _frag_order_np(img, N, Kpad))
    # refusals write nothing
    out[:] = 0xABCD
    assert L.ovm_host_frag_order(img.ctypes.data, N, Kpad + 16, out.ctypes.data) == -4
    assert L.ovm_host_frag_order(None, N, Kpad, out.ctypes.data) == -1
    assert L.ovm_host_frag_order(img.ctypes.data, N, Kpad, img.ctypes.data) == -1
    assert L.ovm_host_frag_order(img.ctypes.data, 0, Kpad, out.ctypes.data) == -1
    assert (out == 0xABCD).all()


# ------------------------------------------------------------------------------------------------------------- the bound bites
def _bilinear(inp, grid, mode="bilinear", padding_mode="zeros", align_corners=False, slip=False):
    """F.grid_sample (bilinear, zero padding, align_corners=False) tap by tap as dec_chain_b_kernel walks it; slip: the tap at x1
    gets the weight of the tap at x0"""
    N, Cc, H, W = inp.shape
    ix, iy = ((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2
    x0, y0 = ix.floor(), iy.floor()
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    flat = inp.flatten(2)
    out = torch.zeros(N, Cc, *grid.shape[1:3], dtype=inp.dtype)
    for yy, wy in ((y0, wy0), (y0 + 1, wy1)):
        for xx, wx in ((x0, wx0), (x0 + 1, wx0 if slip else wx1)):
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().flatten(1)
            tap = flat.gather(2, idx[:, None, :].expand(N, Cc, -1)).reshape(out.shape)
            out = out + tap * (wy * wx * ok)[:, None]
    return out


# (case, slip) pairs in which the case does not run the code the slip is in
NOT_REACHED = {("c", "clamp_1e-3"): "the last layer refines no boxes",
               ("d", "no_qpos_in_text_query"): "T = 1: the softmax over one token is 1 whatever the query",
               ("d", "softmax_tail_rows_skipped"): "Q = 1: rows 8..15 of the workgroup hold no query"}


def _outputs(c, dtype, slip=None):
    a = DR.chain_a_ref(c["op"], dtype, slip)
    b = DR.chain_b_ref(c["op"], dtype, slip, refine=c["refine"])
    return dict(zip(("qpos", "qk", "v", "hs", "ref_next"), a + b))


@pytest.mark.parametrize("name", "abcdefghi")
def test_gpu_bounds_reject_dec_chain_slips(monkeypatch, name):
    import test_gpu_dec_chain as G
    c = G._case(name)
    outs = [n for n in ("qpos", "qk", "v", "hs", "ref_next") if c["ref64"][n] is not None]
    tol = {n: R.bound(c["ref32"][n], c["ref64"][n]) for n in outs}

    def worst(got):                                              # the largest error / bound over the outputs
        return max(R.rel_err(got[n], c["ref64"][n]) / tol[n] for n in outs)

    orig = F.grid_sample
    monkeypatch.setattr(R.F, "grid_sample", _bilinear)           # the harness itself stays inside the bound
    clean = _outputs(c, torch.float32)
    clean64 = _outputs(c, torch.float64)
    assert worst(clean) <= 1.0, name
    assert max(R.rel_err(clean64[n], c["ref64"][n]) for n in outs) < TIGHT, name
    monkeypatch.setattr(R.F, "grid_sample", orig)
    for slip in DR.SLIPS:
        if (name, slip) in NOT_REACHED:
            assert worst(_outputs(c, torch.float32, slip)) <= 1.0, f"{name} {slip}: listed as not reached, but it changes the result"
            continue
        if slip == "tap_x1_weight_wx0":
            monkeypatch.setattr(R.F, "grid_sample", lambda *a, **kw: _bilinear(*a, **kw, slip=True))
        ratio = worst(_outputs(c, torch.float32, slip))
        monkeypatch.setattr(R.F, "grid_sample", orig)
        print(f"case {name} {slip}: error / bound = {ratio:.3g}")
        assert ratio > 1.0, f"case {name}: '{slip}' passes the bound (error / bound = {ratio:.3g}): the case does not test that path"


# ----------------------------------------------------------------------------------------------------------------- the predicate
def test_dec_chain_supported_table():
    import test_gpu_dec_chain as G
    from ovmono3d_amd import lib
    L = lib.load()
    for name, (Q, D, heads, ffn, split, shapes, P, T, refine, key) in G.CASES.items():
        assert L.ovm_host_dec_chain_supported(D, heads, ffn, len(shapes), P, T, 3) == 1, name     # i included: the kernel handles heads > 32
        assert set(G.lin_shapes(D, heads, ffn, len(shapes), P)) == set(DR.LIN)
    sup = lambda D=256, heads=8, ffn=512, nl=2, P=2, T=64, prec=3: L.ovm_host_dec_chain_supported(D, heads, ffn, nl, P, T, prec)
    assert sup() == 1
    assert sup(T=65) == 0                                        # case g at T = 65: 8 x 65 scores per row > 516
    assert sup(D=288) == 0
    assert sup(heads=64, ffn=256, nl=1, T=9) == 0                 # case i at T = 9
    assert sup(prec=1) == 0                                      # the chains multiply split-fp16 images only
    assert sup(ffn=768) == 0 and sup(ffn=1024) == 1 and sup(ffn=96) == 1      # above 512: whole 512-column chunks
    assert sup(nl=1, P=1) == 0 and sup(nl=9) == 0                  # samples in pairs; at most 8 levels
    assert sup(heads=0) == 0 and sup(T=0) == 0
