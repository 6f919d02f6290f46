"""The GroundingDINO decoder row chains one at a time - dec_chain_a_kernel, dec_chain_b_kernel and dec_chain_c_kernel through
ovm_g_dec_chain, which is the engine's launcher behind a check of the descriptor - against the float64 restatement of
tests/dec_chain_ref.py. Weights are packed by ovm_host_pack_weight and ovm_host_frag_order, the loader's own layout code.

Conventions of tests/test_gpu_gdino_ops.py: every output (qpos, qk, v of chain A; hs', ref_next of chain B / C) is compared by
common.rel_err with the float64 restatement, bounded by 4 x the error of PyTorch's fp32 evaluation from the same inputs, never below
2e-6 (gdino_ops_ref.bound). Output buffers carry two extra rows, are pre-filled with a sentinel that is exact in fp16 and must still
hold it wherever the kernel owns nothing. Text keys / values and the value image are layer 1 of a two-layer interleaved buffer
(ldt = 4 D, ldv = 2 D, non-zero base offset), as the engine lays them out. Each output prints
`FIG dec_chain_<a|b> <case> <output> err <measured> fp32 <PyTorch fp32> bound <bound> ratio <err / fp32>`.

The case builder runs without a GPU: tests/test_dec_chain_ref_cpu.py imports it to show that the bound of every case sees the
mistakes this kernel can make.
"""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import dec_chain_ref as DR
import test_gpu_gdino_ops as G

pytestmark = pytest.mark.gpu

SENT = G.SENT
OVM_ERR_INVALID, OVM_ERR_SHAPE = G.OVM_ERR_INVALID, G.OVM_ERR_SHAPE
PROD = [(10, 13), (5, 7), (3, 4), (2, 2)]
EPS = 1e-5
#        Q    D  heads ffn  split levels (H, W)              P   T   refine  operands of
CASES = {
    "a": (16, 256, 8, 2048, 1, PROD, 4, 9, True, "a"),          # production geometry: FULL products, four FFN chunks with a k-offset into fc2
    "b": (16, 256, 8, 2048, 4, PROD, 4, 9, True, "a"),          # chain B on a (rows x chunks) grid + chain C: bit-identical to a
    "c": (37, 256, 8, 2048, 4, PROD, 4, 9, False, "c"),         # two full row blocks + one of 5 rows; last layer: no refinement
    "d": (1, 32, 2, 32, 1, [(1, 1)], 2, 1, True, "d"),          # smallest of everything; offsets + weights N = 12 in a tile of 16; one token
    "e": (17, 160, 5, 96, 1, [(1, 7), (4, 1), (3, 3)], 2, 103, True, "e"),   # predicated k path (K = 160, 320); ffn < 512; heads T = 515
    "f": (20, 128, 4, 1024, 2, [(6, 5), (2, 3)], 4, 129, True, "f"),         # heads T = 516 fills the score region; split 2
    "g": (16, 256, 8, 512, 1, [(4, 4), (2, 2)], 2, 64, True, "g"),           # heads T = 512; a single FFN chunk
    "h": (32, 64, 4, 512, 1, [(5, 4), (2, 2)], 2, 5, True, "h"),             # boxes on the clamp's edges, samples outside their level
    "i": (16, 256, 64, 256, 1, [(2, 2)], 2, 8, True, "i"),                   # heads > 32: more (row, head) pairs than threads
}
EDGE_COORDS = (0.0, 1e-6, 1e-5, 0.5, 1 - 1e-5, 1.0)


def lin_shapes(D, heads, ffn, L, P):
    """(N, K) of the fourteen linears, in dec_chain_ref.LIN's (= OvmDecChainOp.lin's) order"""
    return dict(zip(DR.LIN, [(D, 2 * D), (D, D), (2 * D, D), (D, D), (D, D), (D, D), (D, D), (3 * heads * L * P, D), (D, D), (ffn, D), (D, ffn),
                             (D, D), (D, D), (4, D)]))


@lru_cache(maxsize=None)
def _operands(key):
    Q, D, heads, ffn, _, shapes, P, T, _, _ = CASES[key]
    g = torch.Generator().manual_seed(7000 + sorted(CASES).index(key))
    L, S = len(shapes), sum(h * w for h, w in shapes)
    rn = lambda *s: torch.randn(*s, generator=g)
    op = dict(heads=heads, L=L, P=P, shapes=shapes, eps=EPS, W={}, B={})
    for name, (N, K) in lin_shapes(D, heads, ffn, L, P).items():
        op["W"][name], op["B"][name] = rn(N, K) / math.sqrt(K), rn(N) * 0.1
    op["LN"] = [(1 + 0.1 * rn(D), 0.1 * rn(D)) for _ in range(4)]
    op["hs"], op["tk"], op["tv"], op["val"] = rn(Q, D), rn(T, D), rn(T, D), rn(S, D)
    F = D // 2
    op["dim_t"] = torch.pow(torch.tensor(10000.0), 2.0 * torch.arange(F // 2, dtype=torch.float32) / F)
    if key == "h":
        op["ref"] = torch.tensor(EDGE_COORDS)[torch.randint(0, len(EDGE_COORDS), (Q, 4), generator=g)]
        op["W"]["offw"][:2 * heads * L * P] *= 8.0              # sampling offsets of several box widths
    else:
        op["ref"] = torch.cat([0.1 + 0.8 * torch.rand(Q, 2, generator=g), 0.05 + 0.45 * torch.rand(Q, 2, generator=g)], 1)
        op["ref"][0, 0], op["ref"][-1, 3] = 1e-4, 1 - 1e-4        # between the refinement's clamp (1e-5) and a clamp at 1e-3
    return op


@lru_cache(maxsize=None)
def _case(name):
    """-> the operands (CPU fp32; qpos and ctx are the fp32 images of the float64 chain A and self-attention) with the float64
    references and PyTorch's fp32 evaluations of both chains: ref64 / ref32 [output name] -> tensor"""
    Q, D, heads, ffn, split, shapes, P, T, refine, key = CASES[name]
    op = dict(_operands(key))
    a64, a32 = DR.chain_a_ref(op), DR.chain_a_ref(op, torch.float32)
    op["qpos"] = a64[0].float()
    op["ctx"] = DR.self_attention(a64[1], a64[2], heads).float()
    keep = {}
    b64, b32 = DR.chain_b_ref(op, refine=refine, keep=keep), DR.chain_b_ref(op, torch.float32, refine=refine)
    outs = ("qpos", "qk", "v", "hs", "ref_next")
    c = dict(op=op, name=name, Q=Q, D=D, heads=heads, ffn=ffn, split=split, T=T, refine=refine, loc=keep["loc"],
             ref64=dict(zip(outs, a64 + b64)), ref32=dict(zip(outs, a32 + b32)))
    if name == "h":
        loc, ref = c["loc"], op["ref"]
        outside = ((loc < 0) | (loc > 1)).any(-1).float().mean()
        assert outside >= 0.25, f"case h: only {outside:.2f} of the sample points fall outside their level"
        assert (ref < 1e-5).any() and (ref > 1 - 1e-5).any(), "case h: the refinement clamp is not reached on both sides"
    return c


# ------------------------------------------------------------------------------------------------------------------ device side
def _pack_frag(w):
    """[N][K] fp32 -> the fragment-ordered split image (uint16 as int16 tensor), by the library's two host functions; Kpad = K"""
    _, L = G._lib()
    N, K = w.shape
    w = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    n = (N + 127) // 128 * 128 * 2 * K
    img, out = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    assert L.ovm_host_pack_weight(w.ctypes.data, N, K, K, 3, img.ctypes.data) == 0
    assert L.ovm_host_frag_order(img.ctypes.data, N, K, out.ctypes.data) == 0
    return torch.from_numpy(out.view(np.int16))


def _descriptor(c, device, split=None, refine=None, T=None):
    """-> (OvmDecChainOp, dict of the device buffers it points at). Output buffers: [Q + 2][cols], sentinel-filled; `hs` holds the
    decoder state in its first Q rows."""
    lib, _ = G._lib()
    op, Q, D, heads = c["op"], c["Q"], c["D"], c["heads"]
    split = c["split"] if split is None else split
    refine = c["refine"] if refine is None else refine
    T = c["T"] if T is None else T
    dev = lambda t: t.contiguous().to(device)
    sent = lambda rows, cols: torch.full((rows, cols), SENT, device=device)
    b = {}
    b["hs"] = sent(Q + 2, D)
    b["hs"][:Q] = dev(op["hs"])
    for n, cols in (("qpos", D), ("qk", 2 * D), ("v", D), ("ref_next", 4), ("ffn_x", D)):
        b[n] = sent(Q + 2, cols)
    b["ffn_part"] = sent(max(split, 1) * Q + 2, D)
    b["qpos_in"], b["ctx"], b["ref"], b["dim_t"] = dev(op["qpos"]), dev(op["ctx"]), dev(op["ref"]), dev(op["dim_t"])
    # layer 1 of a two-layer interleaved buffer; layer 0 holds values no result survives (one spare row for the refusal at T + 1)
    Tc, S = c["T"], op["val"].shape[0]
    text = torch.full((Tc + 1, 4 * D), 1e4)
    text[:Tc, 2 * D:3 * D], text[:Tc, 3 * D:] = op["tk"], op["tv"]
    val = torch.full((S, 2 * D), 1e4)
    val[:, D:] = op["val"]
    b["text"], b["val"] = dev(text), dev(val)
    d = lib.OvmDecChainOp()
    d.Q, d.D, d.T, d.heads, d.ffn, d.eps = Q, D, T, heads, c["ffn"], EPS
    d.hs, d.ref, d.sine_dim_t, d.ctx = b["hs"].data_ptr(), b["ref"].data_ptr(), b["dim_t"].data_ptr(), b["ctx"].data_ptr()
    d.qpos, d.qk, d.v = b["qpos"].data_ptr(), b["qk"].data_ptr(), b["v"].data_ptr()
    d.ref_next = b["ref_next"].data_ptr() if refine else None
    d.tk, d.tv, d.ldt = b["text"].data_ptr() + 4 * 2 * D, b["text"].data_ptr() + 4 * 3 * D, 4 * D
    d.val, d.ldv = b["val"].data_ptr() + 4 * D, 2 * D
    d.L, d.P = op["L"], op["P"]
    start = 0
    for l, (h, w) in enumerate(op["shapes"]):
        d.lh[l], d.lw[l], d.lstart[l] = h, w, start
        start += h * w
    for i, name in enumerate(DR.LIN):
        if name.startswith("bb") and not refine:                 # the last layer has no bbox MLP
            continue
        b["w_" + name], b["b_" + name] = dev(_pack_frag(op["W"][name])), dev(op["B"][name])
        N, K = op["W"][name].shape
        d.lin[i].w, d.lin[i].bias, d.lin[i].N, d.lin[i].K, d.lin[i].Kpad = b["w_" + name].data_ptr(), b["b_" + name].data_ptr(), N, K, K
    for i, (gm, bt) in enumerate(op["LN"]):
        b[f"g{i}"], b[f"be{i}"] = dev(gm), dev(bt)
        d.ln[i].gamma, d.ln[i].beta = b[f"g{i}"].data_ptr(), b[f"be{i}"].data_ptr()
    d.ffn_split, d.ffn_x, d.ffn_part = split, b["ffn_x"].data_ptr(), b["ffn_part"].data_ptr()
    return d, b


def _launch(d, part):
    _, L = G._lib()
    rc = L.ovm_g_dec_chain(C.byref(d), part, G._stream())
    G._finish(rc, f"ovm_g_dec_chain part {part}")
    return rc


def _all_sentinel(t, what):
    assert bool((t == SENT).all()), f"{what}: written where the kernel owns nothing"


@lru_cache(maxsize=None)
def _run(name, device):
    """both chains of a case, each from the restatement's operands -> CPU tensors of the five outputs (whole buffers)"""
    c = _case(name)
    Q, split = c["Q"], c["split"]
    d, b = _descriptor(c, device)
    hs_before = b["hs"].clone()
    assert _launch(d, 0) == 0, f"dec_chain_a {name}"
    out = {n: b[n].cpu() for n in ("qpos", "qk", "v")}
    assert torch.equal(b["hs"], hs_before), f"dec_chain_a {name}: chain A wrote the decoder state"
    for n in ("ref_next", "ffn_x", "ffn_part"):
        _all_sentinel(b[n], f"dec_chain_a {name} {n}")
    # chain B reads the restatement's qpos, not chain A's: each chain is held against the reference on its own
    d.qpos = b["qpos_in"].data_ptr()
    assert _launch(d, 1) == 0, f"dec_chain_b {name}"
    if split > 1:                                                # chain B ends at the partial products; chain C finishes the layer
        assert torch.equal(b["hs"], hs_before), f"dec_chain_b {name}: the chunk workgroups wrote the decoder state"
        _all_sentinel(b["ref_next"], f"dec_chain_b {name} ref_next before chain C")
        assert bool((b["ffn_x"][:Q] != SENT).any()) and bool((b["ffn_part"][:split * Q] != SENT).any())
        assert _launch(d, 2) == 0, f"dec_chain_c {name}"
        _all_sentinel(b["ffn_x"][Q:], f"dec_chain_b {name} ffn_x rows >= Q")
        _all_sentinel(b["ffn_part"][split * Q:], f"dec_chain_b {name} ffn_part rows >= Q")
    else:
        _all_sentinel(b["ffn_x"], f"dec_chain_b {name} ffn_x (no split)")
        _all_sentinel(b["ffn_part"], f"dec_chain_b {name} ffn_part (no split)")
    out["hs"], out["ref_next"] = b["hs"].cpu(), b["ref_next"].cpu()
    for n in ("qpos", "qk", "v"):
        assert torch.equal(b[n].cpu(), out[n]), f"dec_chain_b {name}: chain B wrote chain A's output {n}"
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_dec_chain_a_matches_fp64(device, name):
    c, out = _case(name), _run(name, device)
    for n in ("qpos", "qk", "v"):
        _all_sentinel(out[n][c["Q"]:], f"dec_chain_a {name} {n} rows >= Q")
    for n in ("qpos", "qk", "v"):
        G._report("dec_chain_a", f"{name} {n}", out[n][:c["Q"]], c["ref64"][n], c["ref32"][n])


@pytest.mark.parametrize("name", sorted(CASES))
def test_dec_chain_b_matches_fp64(device, name):
    c, out = _case(name), _run(name, device)
    Q = c["Q"]
    _all_sentinel(out["hs"][Q:], f"dec_chain_b {name} hs rows >= Q")
    if c["refine"]:
        _all_sentinel(out["ref_next"][Q:], f"dec_chain_b {name} ref_next rows >= Q")
    else:
        _all_sentinel(out["ref_next"], f"dec_chain_b {name} ref_next (not requested)")
    G._report("dec_chain_b", f"{name} hs", out["hs"][:Q], c["ref64"]["hs"], c["ref32"]["hs"])
    if c["refine"]:
        G._report("dec_chain_b", f"{name} ref_next", out["ref_next"][:Q], c["ref64"]["ref_next"], c["ref32"]["ref_next"])


def test_dec_chain_ffn_split_is_bit_identical(device):
    a, b = _run("a", device), _run("b", device)
    for n in ("qpos", "qk", "v", "hs", "ref_next"):
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{n}: chain B + C on the chunk grid differs from the single workgroup"


def test_dec_chain_refusals_leave_the_outputs_alone(device):
    _, L = G._lib()
    assert L.ovm_g_dec_chain(None, 0, G._stream()) == OVM_ERR_INVALID
    c = _case("g")

    def t65(d):
        d.T = 65                                                  # heads T = 520 scores do not fit the LDS region

    def d288(d):
        d.D = 288

    def null_ref(d):
        d.ref = None

    for what, mutate, parts, want in (("T = 65", t65, (0, 1), OVM_ERR_SHAPE), ("D = 288", d288, (0, 1), OVM_ERR_SHAPE),
                                      ("part 2 without an FFN split", None, (2,), OVM_ERR_INVALID), ("null ref", null_ref, (0, 1), OVM_ERR_INVALID),
                                      ("part 3", None, (3, -1), OVM_ERR_INVALID)):
        d, b = _descriptor(c, device)
        hs_before = b["hs"].clone()
        if mutate:
            mutate(d)
        for part in parts:
            assert _launch(d, part) == want, f"{what}, part {part}"
        assert torch.equal(b["hs"], hs_before), what
        for n in ("qpos", "qk", "v", "ref_next", "ffn_x", "ffn_part"):
            _all_sentinel(b[n], f"refusal {what}: {n}")
    assert L.ovm_host_dec_chain_supported(256, 8, 512, 2, 2, 65, 3) == 0
    assert L.ovm_host_dec_chain_supported(288, 8, 512, 2, 2, 64, 3) == 0
