"""Plain-torch restatement of the GroundingDINO decoder row chains (csrc/dec_chain.hip: dec_chain_a_kernel, dec_chain_b_kernel and
dec_chain_c_kernel), evaluated from the kernels' own operands. float64 is the reference of tests/test_gpu_dec_chain.py, float32 the
same operation as PyTorch evaluates it in the kernels' precision (the yardstick of gdino_ops_ref.bound). No GPU code and nothing
from the product package; tests/test_dec_chain_ref_cpu.py holds it against the Hugging Face port's decoder layer.

Operands: a dict `op` with
  heads, L, P, shapes [(H_l, W_l)], eps                                    geometry
  hs [Q][D], ref [Q][4] (cx, cy, w, h), dim_t [D / 4]                      decoder state, reference boxes, sine frequency table
  qpos [Q][D], ctx [Q][D]                                                  chain B only: chain A's qpos, the query self-attention's output
  tk, tv [T][D], val [S][D]                                                this layer's text keys / values and deformable value image
  W[name] [N][K], B[name] [N] for name in LIN; LN [(gamma, beta)] x 4      nn.Linear weights, LayerNorms 1..4
Products are ordinary matmuls in `dtype`: the kernels' split-fp16 passes are theirs to keep inside the bound.

`slip` names one deliberate mistake (SLIPS); tests/test_dec_chain_ref_cpu.py uses them to show that the GPU test's bound would see it.
"""
import math

import torch
import torch.nn.functional as F

import gdino_ops_ref as R

LIN = ("ref0", "ref1", "sa_qk", "sa_v", "sa_out", "ca_q", "ca_out", "offw", "msda_out", "fc1", "fc2", "bb0", "bb1", "bb2")
SLIPS = ("residual_before_ln1", "no_qpos_in_text_query", "ffn_chunk_dropped", "hi_only_products", "clamp_1e-3", "sine_xy_swapped",
         "tap_x1_weight_wx0", "softmax_tail_rows_skipped")
ROWS = 16               # query rows per workgroup
FFN_CHUNK = 512         # hidden columns per FFN chunk


def _lin(op, name, x, dtype, slip):
    w, b = op["W"][name].to(dtype), op["B"][name].to(dtype)
    if slip == "hi_only_products":                               # one fp16 pass: both operands lose their low halves
        x, w = x.float().half().to(dtype), w.float().half().to(dtype)
    return x @ w.T + b


def _ln(op, i, x, dtype):
    g, b = op["LN"][i]
    return F.layer_norm(x, (x.shape[-1],), g.to(dtype), b.to(dtype), op["eps"])


def sine_embed(ref, dim_t, swapped=True):
    """[Q][4] boxes -> [Q][2 D]: slots [y, x, w, h] (DETR's order) x F = D / 2 features, sin at even f, cos at odd f,
    angle = coordinate * 2 pi / dim_t[f // 2]"""
    order = [1, 0, 2, 3] if swapped else [0, 1, 2, 3]
    e = ref[:, order, None] * (2 * math.pi) / dim_t.repeat_interleave(2)
    odd = (torch.arange(e.shape[-1]) % 2).bool()
    return torch.where(odd, e.cos(), e.sin()).flatten(1)


def chain_a_ref(op, dtype=torch.float64, slip=None):
    """-> qpos [Q][D], qk [Q][2 D] = [q | k] of the query self-attention, v [Q][D]"""
    hs, ref = op["hs"].to(dtype), op["ref"].to(dtype)
    emb = sine_embed(ref, op["dim_t"].to(dtype), swapped=slip != "sine_xy_swapped")
    qpos = _lin(op, "ref1", torch.relu(_lin(op, "ref0", emb, dtype, slip)), dtype, slip)
    return qpos, _lin(op, "sa_qk", hs + qpos, dtype, slip), _lin(op, "sa_v", hs, dtype, slip)


def self_attention(qk, v, heads, dtype=torch.float64):
    """the step between the chains (attn_f32_kernel in the engine): ctx [Q][D] from chain A's outputs"""
    Q, D = v.shape
    h = lambda t: t.to(dtype).reshape(Q, heads, D // heads).permute(1, 0, 2)[None]
    return R.attn_ref(h(qk[:, :D]), h(qk[:, D:]), h(v), (D // heads) ** -0.5, dtype=dtype)[0].permute(1, 0, 2).reshape(Q, D)


def chain_b_ref(op, dtype=torch.float64, slip=None, refine=True, keep=None):
    """-> hs' [Q][D], ref_next [Q][4] (None without `refine`: the last layer). keep: a dict that receives "loc", the deformable step's
    sampling locations [Q][H][L][P][2] (map coordinates: [0, 1] is inside the level)"""
    hs, qpos, ctx, ref = (op[n].to(dtype) for n in ("hs", "qpos", "ctx", "ref"))
    Q, D = hs.shape
    H, L, P = op["heads"], op["L"], op["P"]
    dh = D // H
    pre = hs + _lin(op, "sa_out", ctx, dtype, slip)
    x = _ln(op, 0, pre, dtype)
    # text cross-attention over the T tokens
    q = _lin(op, "ca_q", x if slip == "no_qpos_in_text_query" else x + qpos, dtype, slip)
    tk, tv = op["tk"].to(dtype), op["tv"].to(dtype)
    T = tk.shape[0]
    s = torch.einsum("qhd,thd->qht", q.reshape(Q, H, dh), tk.reshape(T, H, dh)) * dh ** -0.5
    p = torch.softmax(s, -1)
    if slip == "softmax_tail_rows_skipped":                      # rows 8..15 of every workgroup keep their raw scores
        p = torch.where((torch.arange(Q) % ROWS >= ROWS // 2)[:, None, None], s, p)
    t = torch.einsum("qht,thd->qhd", p, tv.reshape(T, H, dh)).reshape(Q, D)
    x = _ln(op, 1, (pre if slip == "residual_before_ln1" else x) + _lin(op, "ca_out", t, dtype, slip), dtype)
    # deformable cross-attention: box mode of msdeform_fused
    ow = _lin(op, "offw", x + qpos, dtype, slip)
    if keep is not None:
        keep["loc"] = R.msdeform_locations(ow, ref, 1, H, L, P, op["shapes"], dtype)[0]
    smp = R.msdeform_ref(op["val"], ow, ref, 1, H, dh, L, P, op["shapes"], dtype)
    x = _ln(op, 2, x + _lin(op, "msda_out", smp, dtype, slip), dtype)
    # FFN
    hid = torch.relu(_lin(op, "fc1", x, dtype, slip))
    if slip == "ffn_chunk_dropped":
        hid = hid.clone()
        hid[:, -min(FFN_CHUNK, hid.shape[1]):] = 0
    x = _ln(op, 3, x + _lin(op, "fc2", hid, dtype, slip), dtype)
    if not refine:
        return x, None
    delta = _lin(op, "bb2", torch.relu(_lin(op, "bb1", torch.relu(_lin(op, "bb0", x, dtype, slip)), dtype, slip)), dtype, slip)
    eps = 1e-3 if slip == "clamp_1e-3" else 1e-5
    rc = ref.clamp(eps, 1 - eps)
    return x, torch.sigmoid(delta + torch.log(rc / (1 - rc)))

