"""sam_mask_stats_kernel (csrc/sam.hip) through ovm_op_sam_mask_stats: per plane the counts of the postprocess_masks logit above
+offset, 0 and -offset and the tight box of the mask, nothing of image size written.

Exact, because the kernel shares the value with sam_mask_out_kernel (bil_tap, up_sample, mask_blend): the middle count is the byte
sum of ovm_op_sam_mask_out on the same plane, and the box and count are ovm_sam_mask_boxes' on those bytes. Against fp64
(sam_dp_glue_ref.mask_logits): for each threshold t in {-offset, 0, +offset}, count64(v > t + band) <= count <= count64(v > t - band)
with band = sam_dp_glue_ref.band_of of the plane (4 x the fp32 restatement's own error + one ulp), at most 1 % of a plane within the
band of a threshold (tests/test_sam_auto_cpu.py asserts that of the fp64 reference alone). The comparison rejects H / W swapped, the
crop ignored and the offset's sign flipped.

Geometries: (23, 31), (31, 23), (5, 3), (61, 97), (70, 100), (99, 71) at L = 32, S = 128 and (61, 97) at L = 64, S = 256: sx != sy both
ways, odd widths, crops that end off a word; planes at a stride of L * L + 16. Per geometry three smooth fields of amplitude 10 and
four crafted planes: all below -offset (empty, 0 / 0), all above +offset, all between 0 and +offset, one positive low-resolution cell.

Measured on an MI355X: every exact comparison holds; bands of the smooth fields 3.9e-05 .. 3.0e-04 (1.4e-03 for the one-cell plane of
amplitude 200); at most 0.017 % of a plane within the band of a threshold; every count inside its interval.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ovmono3d_amd.sam import SamAutomaticMaskGenerator  # noqa: F401  (the feature under test: without it this module does not load)
import sam_auto_oracle as ao
import sam_dp_glue_ref as G
from sam_auto_oracle import F32, F64

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
PAD = 16                                  # floats between planes, and guard words around the output
SENT = np.float32(G.SENTINEL)


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _planes_dev(planes, device):
    """[n][L][L] -> device buffer of n planes at stride L * L + PAD (the sentinel between them); (tensor, stride)"""
    n, L, _ = planes.shape
    stride = L * L + PAD
    buf = np.full((n, stride), SENT, F32)
    buf[:, :L * L] = planes.reshape(n, -1)
    return torch.from_numpy(buf).to(device), stride


def _geo(case):
    (H, W), L, S = case["hw"], case["L"], case["S"]
    nh, nw = G.preprocess_shape(H, W, S)
    return L, S, nh, nw, H, W


def _stats(lg, stride, n, case, device, offset=ao.OFFSET, skip=None, preset=None):
    """ovm_op_sam_mask_stats into a guarded buffer: int32 [n][7]; the guards are checked"""
    out = torch.full((PAD + 7 * n + PAD,), GUARD, dtype=torch.int32, device=device)
    if preset is not None:
        out[PAD:PAD + 7 * n] = torch.from_numpy(preset.reshape(-1)).to(device)
    sk = None if skip is None else torch.from_numpy(np.asarray(skip, np.int32)).to(device)
    rc = _lib().ovm_op_sam_mask_stats(lg.data_ptr(), stride, n, *_geo(case), float(offset), None if sk is None else sk.data_ptr(),
                                      out.data_ptr() + 4 * PAD, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:PAD] == GUARD) and np.all(o[PAD + 7 * n:] == GUARD), "guard words around the output were overwritten"
    return o[PAD:PAD + 7 * n].reshape(n, 7)


def _mask_out(lg, stride, n, case, device):
    """(uint8 [n][H][W] of ovm_op_sam_mask_out, boxes fp32 [n][4] and counts of ovm_sam_mask_boxes on those bytes)"""
    L, S, nh, nw, H, W = _geo(case)
    masks = torch.zeros((n, H, W), dtype=torch.uint8, device=device)
    assert _lib().ovm_op_sam_mask_out(lg.data_ptr(), stride, L, S, nh, nw, H, W, n, masks.data_ptr(), _stream()) == 0
    boxes = torch.zeros((n, 4), dtype=torch.float32, device=device)
    counts = torch.zeros((n,), dtype=torch.int32, device=device)
    assert _lib().ovm_sam_mask_boxes(masks.data_ptr(), n, H, W, boxes.data_ptr(), counts.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return masks.cpu().numpy(), boxes.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("case", ao.STATS_GEOMETRIES, ids=ao.stats_id)
def test_counts_and_boxes_equal_the_mask_kernel_and_meet_fp64(device, case):
    inp = ao.stats_inputs(case)
    planes = np.concatenate([inp["smooth"], inp["crafted"]])
    n, (H, W) = len(planes), case["hw"]
    lg, stride = _planes_dev(planes, device)
    got = _stats(lg, stride, n, case, device)
    # exact: the mask kernel's bytes and their tight boxes
    masks, boxes, counts = _mask_out(lg, stride, n, case, device)
    assert np.array_equal(got[:, 1], masks.reshape(n, -1).sum(1).astype(np.int32)) and np.array_equal(got[:, 1], counts)
    incl = boxes.astype(np.int32) - np.where(counts[:, None] > 0, np.array([0, 0, 1, 1], np.int32)[None], 0)
    assert np.array_equal(got[:, 3:], incl)
    # the crafted planes
    s = ao.STATS_SMOOTH
    assert got[s].tolist() == [0, 0, 0, 0, 0, 0, 0]
    assert got[s + 1].tolist() == [H * W, H * W, H * W, 0, 0, W - 1, H - 1]
    assert got[s + 2].tolist() == [0, H * W, H * W, 0, 0, W - 1, H - 1]
    assert 0 < got[s + 3][1] < H * W
    # against fp64, per plane
    v64, v32 = ao.stats_logits(case, planes, F64), ao.stats_logits(case, planes, F32)
    for i in range(n):
        band = G.band_of(v64[i], v32[i])
        share = ao.check_counts(got[i, :3], v64[i], band, tag=f"{ao.stats_id(case)} plane {i}")
        print(f"\n{ao.stats_id(case)} plane {i}: counts {got[i, :3].tolist()} band {band:.2e} left out {share:.4%}", end="")
    # two calls: equal bytes
    assert np.array_equal(got, _stats(lg, stride, n, case, device))
    # the offset is an argument: 2.5 moves the outer counts, not the mask
    wide = _stats(lg, stride, n, case, device, offset=2.5)
    assert np.array_equal(wide[:, [1, 3, 4, 5, 6]], got[:, [1, 3, 4, 5, 6]])
    assert np.all(wide[:, 0] <= got[:, 0]) and np.all(wide[:, 2] >= got[:, 2])
    if H * W > 100:
        assert np.all(wide[:s, 0] < got[:s, 0]) and np.all(wide[:s, 2] > got[:s, 2])


@pytest.mark.parametrize("case", [ao.STATS_GEOMETRIES[4], ao.STATS_GEOMETRIES[5]], ids=ao.stats_id)
def test_skipped_planes_keep_what_the_caller_preset(device, case):
    inp = ao.stats_inputs(case)
    planes = np.concatenate([inp["smooth"], inp["crafted"]])
    n = len(planes)
    lg, stride = _planes_dev(planes, device)
    full = _stats(lg, stride, n, case, device)
    skip = np.array([0, 1, 0, 1, 1, 0, 7], np.int32)[:n]
    preset = (np.arange(7 * n, dtype=np.int32).reshape(n, 7) + 1000)
    got = _stats(lg, stride, n, case, device, skip=skip, preset=preset)
    for i in range(n):
        assert np.array_equal(got[i], preset[i] if skip[i] else full[i]), i


@pytest.mark.parametrize("mut", ao.STATS_MUTATIONS)
def test_the_comparison_rejects_wrong_evaluations(mut):
    """No device: what a device that swapped H and W, ignored the crop or flipped the offset's sign would return fails check_counts."""
    for case in ao.STATS_GEOMETRIES:
        if case["hw"] == (5, 3):                                   # 15 pixels: a wrong evaluation may count the same
            continue
        planes = ao.stats_inputs(case)["smooth"]
        v64, v32 = ao.stats_logits(case, planes, F64), ao.stats_logits(case, planes, F32)
        wrong = ao.as_device(ao.stats_logits(case, planes, F32, mut), mut=mut)
        rejected = 0
        for i in range(len(planes)):
            try:
                ao.check_counts(wrong[i][:3], v64[i], G.band_of(v64[i], v32[i]))
            except AssertionError:
                rejected += 1
        assert rejected >= 1, f"{mut} passes on {ao.stats_id(case)}"


def test_refusals_leave_the_output_untouched(device):
    case = ao.STATS_GEOMETRIES[0]
    planes = ao.stats_inputs(case)["smooth"]
    lg, stride = _planes_dev(planes, device)
    out = torch.full((32,), GUARD, dtype=torch.int32, device=device)
    L, S, nh, nw, H, W = _geo(case)
    from ovmono3d_amd import lib
    for args in ((lg.data_ptr(), stride, 1, L, S, S + 1, nw, H, W), (lg.data_ptr(), L * L - 1, 1, L, S, nh, nw, H, W), (lg.data_ptr(), stride, 1, L, S, nh, nw, 0, W),
                 (lg.data_ptr(), stride, 1, L, L // 2, nh, nw, H, W)):
        assert _lib().ovm_op_sam_mask_stats(*args, 1.0, None, out.data_ptr(), _stream()) == lib.OVM_ERR_SHAPE
    assert _lib().ovm_op_sam_mask_stats(lg.data_ptr(), stride, 0, L, S, nh, nw, H, W, 1.0, None, out.data_ptr(), _stream()) == lib.OVM_ERR_INVALID
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD)
