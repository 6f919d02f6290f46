"""The fusion layer's one-pass bi-attention (biattn_mfma_kernel + combine, through ovm_g_biattn) against the float64 formula.

The tolerance is measured, not fixed: on every input the generic four-kernel path (generic=1) runs first and its error against the
float64 reference, max |a - b| / max |b| per output, is recorded; the matrix-core path must stay within twice that figure (the
arithmetic is the same - exact fp32 products, fp32 sums -, only the summation order differs).

Measured on an MI355X (generic image / text -> matrix-core image / text):
  one_by_one                0         / 0         -> 0         / 0
  last_chunk_of_two_rows    2.237e-07 / 3.738e-07 -> 2.510e-07 / 5.095e-07
  second_text_block_of_one  3.100e-07 / 4.681e-07 -> 4.220e-07 / 3.995e-07
  text_limit                5.801e-07 / 4.770e-07 -> 6.168e-07 / 4.180e-07
  peaked                    6.825e-08 / 1.227e-06 -> 6.513e-08 / 1.515e-06
  headline                  2.479e-07 / 2.664e-07 -> 2.938e-07 / 3.806e-07
(the worst ratio is 1.43, headline text side; with the scores summed as one chain of 256 products instead of a tree of sixteen
accumulators it was 3.0 and the test failed)
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from biattn_cases import make_inputs, reference, rel_err
from common import ROOT

pytestmark = pytest.mark.gpu

H, DH = 4, 256


def _chunk():
    src = open(os.path.join(ROOT, "ovmono3d_amd", "csrc", "gdino_kernels.hip")).read()
    return int(re.search(r"kBiChunk = (\d+)", src).group(1))


CHUNK = _chunk()
CASES = {
    "one_by_one": dict(S=1, T=1),
    "last_chunk_of_two_rows": dict(S=CHUNK + 2, T=20),
    "second_text_block_of_one": dict(S=3 * CHUNK, T=33),
    "text_limit": dict(S=2 * CHUNK + 1, T=256),
    "peaked": dict(S=3 * CHUNK, T=20, peaked_chunk=CHUNK),
    "headline": dict(S=6015, T=22),
}


@functools.lru_cache(maxsize=None)
def _case(name, H_=H, dh=DH):
    q, k, vi, vt = make_inputs(H=H_, dh=dh, seed=3, **CASES[name])
    ri, rt = reference(q, k, vi, vt, H_, 1.0 / np.sqrt(dh))
    assert np.isfinite(ri).all() and np.isfinite(rt).all()
    return (q, k, vi, vt), (ri, rt)


def _run(device, inputs, H_, dh, generic, split=False):
    """inputs laid out as the engine has them: [q | v_img] and [k_text | v_text] share rows (row stride 2 E)"""
    from pyref_gdino.biattn import biattn
    from pyref_gdino.ops import Ops
    o = Ops(device)
    q, k, vi, vt = inputs
    E = H_ * dh
    qv = torch.from_numpy(np.concatenate([q, vi], axis=1)).to(device)
    kv = torch.from_numpy(np.concatenate([k, vt], axis=1)).to(device)
    out = biattn(o, qv[:, :E], kv[:, :E], qv[:, E:], kv[:, E:], H_, 1.0 / np.sqrt(dh), generic=generic, split=split)
    torch.cuda.synchronize(device)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_matrix_core_path_within_twice_the_generic_error(device, name):
    inputs, (ri, rt) = _case(name)
    gi, gt = _run(device, inputs, H, DH, generic=True)
    ni, nt, hi, lo = _run(device, inputs, H, DH, generic=False, split=True)
    for x in (gi, gt, ni, nt):
        assert torch.isfinite(x).all()
    eg = (rel_err(gi.cpu().numpy(), ri), rel_err(gt.cpu().numpy(), rt))
    en = (rel_err(ni.cpu().numpy(), ri), rel_err(nt.cpu().numpy(), rt))
    print(f"biattn {name}: generic image {eg[0]:.3e} text {eg[1]:.3e} -> matrix-core image {en[0]:.3e} text {en[1]:.3e}")
    assert en[0] <= 2 * eg[0] and en[1] <= 2 * eg[1], (name, eg, en)
    # the split-fp16 rows are the fp32 rows split (hi = fp16(x), lo = fp16(x - hi): 2^-21 of the largest value at worst)
    rec = hi.float() + lo.float()
    assert float((rec - ni).abs().max()) <= 2.0 ** -20 * float(ni.abs().max())


def test_unsupported_geometry_takes_the_generic_kernels(device):
    """head dimension 128: biattn_mfma_supported is false, so the default call and generic=1 run the same kernels - same bits"""
    inputs = make_inputs(S=CHUNK + 2, T=20, H=4, dh=128, seed=5)
    ri, rt = reference(*inputs, 4, 1.0 / np.sqrt(128))
    a = _run(device, inputs, 4, 128, generic=False)
    b = _run(device, inputs, 4, 128, generic=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert rel_err(a[0].cpu().numpy(), ri) < 1e-5 and rel_err(a[1].cpu().numpy(), rt) < 1e-5


@pytest.mark.parametrize("name", ["second_text_block_of_one", "headline"])
def test_matrix_core_path_is_a_pure_function_of_its_inputs(device, name):
    inputs, _ = _case(name)
    a = _run(device, inputs, H, DH, generic=False, split=True)
    b = _run(device, inputs, H, DH, generic=False, split=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_null_pointer_or_empty_dimension_is_refused_before_any_launch(device):
    from ovmono3d_amd import lib
    L = lib.load()
    x = torch.zeros(4, 2048, device=device)
    p = x.data_ptr()
    assert L.ovm_g_biattn(None, 2048, p, 2048, p, 2048, p, 2048, 4, 4, 4, 256, 0.0625, p, None, None, 1024, p, 0, None) == -1
    assert L.ovm_g_biattn(p, 2048, p, 2048, p, 2048, p, 2048, 0, 4, 4, 256, 0.0625, p, None, None, 1024, p, 0, None) == -1
    assert L.ovm_g_biattn(p, 2048, p, 2048, p, 2048, p, 2048, 4, 4, 4, 256, 0.0625, None, None, None, 1024, p, 0, None) == -1
