"""ovm_sam_auto_select (csrc/sam.hip: the valid mask of the two filters, then launch_nms_single) on crafted candidate tables: the keep
list, its order and its count equal tests/sam_auto_oracle.select exactly. The boxes are small integers and the NMS compares
inter / (area + area - inter) in float32 on both sides, so there is no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from ovmono3d_amd.sam import SamAutomaticMaskGenerator  # noqa: F401  (the feature under test: without it this module does not load)
import sam_auto_oracle as ao
from sam_auto_oracle import F32

pytestmark = pytest.mark.gpu
GUARD = -77


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _select(t, pthr, sthr, nthr, device, expect_rc=0):
    """(keep list in order, raw keep buffer, n_keep word) of the device"""
    rows = ao.pack(t)
    m = len(rows)
    cands = torch.from_numpy(rows).to(device)
    keep = torch.full((m + 8,), GUARD, dtype=torch.int32, device=device)
    nk = torch.full((3,), GUARD, dtype=torch.int32, device=device)
    nbytes = C.c_int64()
    assert _lib().ovm_sam_auto_select_workspace(min(m, ao.MAX_ROWS), C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    rc = _lib().ovm_sam_auto_select(cands.data_ptr(), m, float(pthr), float(sthr), float(nthr), keep.data_ptr(), nk.data_ptr() + 4, ws.data_ptr(),
                                    ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect_rc
    torch.cuda.synchronize()
    keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
    assert nk[0] == GUARD and nk[2] == GUARD and np.all(keep[m:] == GUARD)
    return keep, int(nk[1])


def _check(t, pthr, sthr, nthr, device):
    ref = ao.select(t, pthr, sthr, nthr)
    keep, n = _select(t, pthr, sthr, nthr, device)
    assert n == len(ref) and keep[:n].tolist() == ref.tolist(), (n, len(ref))
    return ref


def _random_table(m, seed, span=60, ties=False, nan_every=0):
    g = np.random.default_rng(seed)
    x0, y0 = g.integers(0, span, m), g.integers(0, span, m)
    boxes = np.stack([x0, y0, x0 + g.integers(0, 40, m), y0 + g.integers(0, 40, m)], 1)
    iou = g.uniform(0.5, 1.0, m).astype(F32)
    if ties:
        iou = (np.round(iou * 8) / 8).astype(F32)                          # many equal scores
    stab = g.uniform(0.8, 1.0, m).astype(F32)
    if nan_every:
        stab[::nan_every] = np.nan
    flags = (g.random(m) < 0.1).astype(np.int32)
    return ao.table(iou, stab, boxes, flags=flags, area=np.ones(m))


def test_one_candidate(device):
    t = ao.table([0.9], [0.96], [[3, 4, 20, 30]])
    assert _check(t, 0.88, 0.95, 0.7, device).tolist() == [0]
    assert _check(t, 0.95, 0.95, 0.7, device).tolist() == []
    assert _check(ao.table([0.9], [float("nan")], [[0, 0, 0, 0]]), 0.0, 0.0, 0.7, device).tolist() == [0]


@pytest.mark.parametrize("nthr", [0.3, 0.7, 1.0])
def test_4096_candidates(device, nthr):
    t = _random_table(4096, 11, span=400, nan_every=17)
    ref = _check(t, 0.6, 0.85, nthr, device)
    assert 10 < len(ref) < 4096


def test_4097_candidates_are_refused_with_the_outputs_untouched(device):
    from ovmono3d_amd import lib
    keep, n = _select(_random_table(4097, 12), 0.6, 0.85, 0.7, device, expect_rc=lib.OVM_ERR_CAPACITY)
    assert n == GUARD and np.all(keep == GUARD)


def test_everything_filtered_and_nothing_suppressed(device):
    t = _random_table(300, 13)
    assert _check(t, 1.5, 0.85, 0.7, device).tolist() == []                  # filter 1 removes all
    assert _check(t, 0.6, 1.5, 0.7, device).tolist() == []                   # filter 2 removes all
    far = ao.table(np.linspace(0.99, 0.5, 50), np.ones(50), [[20 * i, 0, 20 * i + 10, 10] for i in range(50)])
    assert _check(far, 0.0, 0.0, 0.7, device).tolist() == list(range(50))     # disjoint boxes: all kept, by score
    assert len(_check(t, 0.0, 0.0, 1.0, device)) == int(((t["flags"] & 1) == 0).sum())      # IoU is never > 1


def test_ties_nan_and_filters_off(device):
    t = _random_table(700, 14, ties=True, nan_every=5)
    for pthr, sthr, nthr in ((0.6, 0.85, 0.5), (0.0, 0.0, 0.5), (-1.0, 0.9, 0.7), (0.75, 0.0, 0.7)):
        _check(t, pthr, sthr, nthr, device)
    same = ao.table([0.9] * 5, [1.0] * 5, [[0, 0, 10, 10]] * 5)
    assert _check(same, 0.5, 0.5, 0.7, device).tolist() == [0]
    assert _check(same, 0.5, 0.5, 1.0, device).tolist() == [0, 1, 2, 3, 4]


def test_equality_at_the_thresholds(device):
    a, b = F32(0.88), F32(0.95)
    far = [[0, 0, 10, 10], [100, 100, 110, 110], [200, 0, 210, 10], [0, 200, 10, 210]]
    t = ao.table([a, np.nextafter(a, F32(1)), 0.9, 0.9], [0.99, 0.99, b, np.nextafter(b, F32(0))], far)
    assert _check(t, float(a), float(b), 0.7, device).tolist() == [2, 1]
    half = ao.table([0.9, 0.8], [1, 1], [[0, 0, 10, 10], [0, 0, 10, 5]])      # IoU exactly 0.5
    assert _check(half, 0.5, 0.5, 0.5, device).tolist() == [0, 1]
    assert _check(half, 0.5, 0.5, float(np.nextafter(F32(0.5), F32(0))), device).tolist() == [0]
    empty = ao.table([0.9, 0.8, 0.7], [1, 1, 1], [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 5, 5]])
    assert _check(empty, 0.5, 0.5, 0.0, device).tolist() == [0, 1, 2]
