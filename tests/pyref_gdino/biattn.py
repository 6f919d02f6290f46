"""Torch-tensor front end of ovm_g_biattn (device memory handles only; no torch arithmetic), beside ops.Ops."""
from __future__ import annotations

import torch

from .ops import Ops


def biattn(o: Ops, q: torch.Tensor, k_text: torch.Tensor, v_img: torch.Tensor, v_text: torch.Tensor, H: int, scale: float,
           generic: bool = False, split: bool = False):
    """q, v_img [S, H*dh]; k_text, v_text [T, H*dh] (row views allowed) -> image context [S, H*dh], text context [T, H*dh];
    split=True also returns the image context's split-fp16 rows (hi, lo). generic=True forces the four-kernel path."""
    for x in (q, k_text, v_img, v_text):
        assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    S, E = q.shape
    T = k_text.shape[0]
    ci, ct = o.empty(S, E), o.empty(T, E)
    hi = torch.empty((S, E), dtype=torch.float16, device=o.dev) if split else None
    lo = torch.empty_like(hi) if split else None
    o._chk(o.L.ovm_g_biattn(q.data_ptr(), q.stride(0), k_text.data_ptr(), k_text.stride(0), v_img.data_ptr(), v_img.stride(0),
                            v_text.data_ptr(), v_text.stride(0), S, T, H, E // H, float(scale), ci.data_ptr(),
                            hi.data_ptr() if split else None, lo.data_ptr() if split else None, E, ct.data_ptr(),
                            1 if generic else 0, o._s()), "ovm_g_biattn")
    return (ci, ct, hi, lo) if split else (ci, ct)
