"""The encoder's folded offsets projection (ovm_tune_set gdino_enc_fold) as arithmetic, without a GPU.

Today the sampling-offsets | attention-weights projection of an encoder layer reads split rows of vis + pos:
    today  = split3(vis + pos, W) + b
Folded, the position term is a per-plan table and the projection reads the rows of vis alone:
    P      = split3(pos, W) + b                  (once per plan)
    folded = split3(vis, W) + P                  (the GEMM's epilogue adds P)
with split3(A, W) = Ah Wh + Ah Wl + Al Wh accumulated in fp32, (h, l) = (fp16_rn(x), fp16_rn(x - h)): the three-pass product of
csrc/gemm.hpp, emulated here with fp32 matmuls of the fp16-valued parts. Both forms are compared with
(vis + pos) W^T + b in float64 on the same fp32 inputs.

Bound (the convention of tests/test_gpu_roi_glue.py): the folded form's largest distance from fp64 is at most 4 x today's form's own
distance plus one fp32 ulp of max |ref|. Shapes: 515 rows (no multiple of a tile), K = 64 / N = 192 and K = 256 / N = 384 (the
reduced and the real d_model with their offsets | logits widths), rows at unit scale and at 8 x.
"""
import numpy as np
import pytest
import torch

S = 515
CASES = [(64, 192, 1.0), (64, 192, 8.0), (256, 384, 1.0), (256, 384, 8.0)]


def _split(x):
    hi = x.to(torch.float16).to(torch.float32)
    lo = (x - hi).to(torch.float16).to(torch.float32)
    return hi, lo


def _split3(a, w):
    ah, al = _split(a)
    wh, wl = _split(w)
    return (al @ wh.t() + ah @ wl.t()) + ah @ wh.t()


@pytest.mark.parametrize("K,N,scale", CASES)
def test_folded_offsets_projection_is_as_close_to_fp64_as_todays(K, N, scale):
    g = torch.Generator().manual_seed(1000 + K + int(scale))
    vis = torch.randn(S, K, generator=g) * scale
    # sine / cosine position embedding plus a level embedding, as plan_encoder_tables builds it
    pos = torch.sin(torch.rand(S, K, generator=g) * 6.2831853) + torch.randn(1, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ref = (vis.double() + pos.double()) @ w.double().t() + b.double()
    today = _split3(vis + pos, w) + b
    table = _split3(pos, w) + b
    folded = _split3(vis, w) + table
    e_today = float((today.double() - ref).abs().max())
    e_fold = float((folded.double() - ref).abs().max())
    e_both = float((folded - today).abs().max())
    top = float(ref.abs().max())
    ulp = float(np.spacing(np.float32(top)))
    print(f"FIG pos fold K={K} N={N} scale={scale}: max|ref| {top:.3e}; today {e_today / top:.3e}, folded {e_fold / top:.3e}, "
          f"folded vs today {e_both / top:.3e} (of max|ref|); bound {(4 * e_today + ulp) / top:.3e}")
    assert e_today > 0
    assert e_fold <= 4 * e_today + ulp
