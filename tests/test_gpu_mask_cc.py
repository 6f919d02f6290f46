"""GPU: connected components and the small-region clean-up on the device (ovmono3d_amd.masks.connected_components /
remove_small_regions; csrc/mask_cc.hip) against tests/mask_cc_oracle.py: scipy.ndimage.label and segment_anything's rule restated
on it. Everything is compared for equality.

Shapes (mask_cc_oracle.SHAPES, as (H, W)): 1 x 1, one row and one column of 130, 7 x 5, the widths 63, 64 and 65 - the kernels' only
tile is the 64 pixels of a row that one wave owns: a segment whose last lane is invalid, one wave per row exactly, and a second segment
of one pixel - 65 x 67 (an odd row count too), 130 x 257 (five segments per row: more than one workgroup per row) and one full-HD plane,
where the 4-connected checkerboard has more than 2^16 labels, the serpentine is the longest chain of unions and the full plane is one
component of 2,073,600 pixels. Every content is checked at every shape, for the labels and for the clean-up."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mask_cc_oracle as O
from ovmono3d_amd import lib
from ovmono3d_amd import masks as M

pytestmark = pytest.mark.gpu

FULL_HD = (1080, 1920)


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


@functools.lru_cache(maxsize=2)
def _planes(shape):
    """(names, uint8 [n, H, W]): the edge planes of the shape and one blob plane; computed once per shape, never written to"""
    e = O.edge_planes(*shape)
    e["blobs"] = O.blobs(*shape, seed=shape[0] + shape[1])
    return tuple(e), np.stack(list(e.values()))


@pytest.mark.parametrize("shape", O.SHAPES, ids=_id)
def test_labels_and_counts_equal_scipy(device, shape):
    names, stack = _planes(shape)
    H, W = shape
    d = torch.from_numpy(stack).to(device)
    # the same planes as bool, and as 255s inside a larger tensor: any nonzero byte is foreground, any plane and row stride is taken
    big = torch.zeros((len(names), H + 3, W + 5), dtype=torch.uint8, device=device)
    pitched = big[:, 1:H + 1, 2:W + 2]
    pitched.copy_(d * 255)
    assert not pitched.is_contiguous()
    for conn in (4, 8):
        for invert in (False, True):
            labels, counts = M.connected_components(d, conn, invert)
            assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(labels.shape) == stack.shape
            got, cnt = labels.cpu().numpy(), counts.cpu().tolist()
            for i, name in enumerate(names):
                ref, n = O.label(stack[i], conn, invert)
                print(f"{_id(shape)} {name} conn {conn} invert {int(invert)}: {n} components, device {cnt[i]}")
                assert cnt[i] == n, (name, conn, invert)
                assert np.array_equal(got[i], ref), (name, conn, invert)
            again = M.connected_components(d, conn, invert)
            assert torch.equal(again[0], labels) and torch.equal(again[1], counts)                   # two calls, equal bytes
            for other in (d.bool(), pitched):
                l2, c2 = M.connected_components(other, conn, invert)
                assert torch.equal(l2, labels) and torch.equal(c2, counts)
            for i in range(len(names)):                                                            # one call of n planes = n calls of one
                l1, c1 = M.connected_components(d[i:i + 1], conn, invert)
                assert torch.equal(l1[0], labels[i]) and int(c1[0]) == cnt[i], (names[i], conn, invert)
    if shape == FULL_HD:
        assert O.label(stack[names.index("checkerboard")], 4)[1] == H * W // 2 > 2 ** 16


def test_checkerboard_serpentine_comb_and_u_are_what_they_are(device):
    H, W = 130, 257
    e = O.edge_planes(H, W)
    d = torch.from_numpy(np.stack([e["checkerboard"], e["serpentine"], e["comb"], e["u"], e["full"], e["empty"]])).to(device)
    l8, c8 = M.connected_components(d, 8)
    l4, c4 = M.connected_components(d, 4)
    assert c8.tolist() == [1, 1, 1, 1, 1, 0] and c4.tolist() == [(H * W + 1) // 2, 1, 1, 1, 1, 0]
    assert int(l4[0].max()) == (H * W + 1) // 2 and int(l8[5].max()) == 0 and bool((l8[4] == 1).all())
    assert torch.equal(l4[0].flatten()[0::2], torch.arange(1, (H * W + 1) // 2 + 1, dtype=torch.int32, device=device))    # every pixel its own, in order


def test_chunked_calls_equal_one_call_and_empty_input_gives_empty_output(device, monkeypatch):
    names, stack = _planes((65, 67))
    d = torch.from_numpy(stack).to(device)
    labels, counts = M.connected_components(d, 8)
    cleaned, changed = M.remove_small_regions(d, 5, "both")
    need = C.c_int64()
    assert lib.load().ovm_mask_remove_small_regions_workspace(3, 65, 67, C.byref(need)) == 0
    monkeypatch.setattr(M, "MAX_CC_WORKSPACE", int(need.value))                                    # three planes per call at the most
    l2, c2 = M.connected_components(d, 8)
    m2, ch2 = M.remove_small_regions(d, 5, "both")
    assert torch.equal(l2, labels) and torch.equal(c2, counts) and torch.equal(m2, cleaned) and torch.equal(ch2, changed)
    none = d[:0]
    l0, c0 = M.connected_components(none)
    m0, ch0 = M.remove_small_regions(none, 3, "holes")
    assert tuple(l0.shape) == (0, 65, 67) and l0.dtype == torch.int32 and tuple(c0.shape) == (0,) and c0.dtype == torch.int32
    assert tuple(m0.shape) == (0, 65, 67) and m0.dtype == torch.uint8 and tuple(ch0.shape) == (0,) and ch0.dtype == torch.bool
    with pytest.raises(ValueError):
        M.connected_components(d, 6)
    with pytest.raises(ValueError):
        M.remove_small_regions(d, 3, "specks")
    with pytest.raises(ValueError):
        M.remove_small_regions(d, 0, "both")


@pytest.mark.parametrize("shape", O.SHAPES, ids=_id)
def test_remove_small_regions_equals_the_oracle(device, shape):
    names, stack = _planes(shape)
    H, W = shape
    d = torch.from_numpy(stack).to(device)
    big = torch.zeros((len(names), H + 2, W + 9), dtype=torch.uint8, device=device)
    pitched = big[:, 2:, 9:]
    pitched.copy_(d * 7)
    n_changed = n_unchanged = 0

    def check(i, thresh, mode, plane, flag):
        nonlocal n_changed, n_unchanged
        ref, ch = O.remove_small_regions(stack[i], thresh, mode)
        assert flag == ch, (names[i], thresh, mode)
        assert np.array_equal(plane, ref), (names[i], thresh, mode)
        n_changed += ch
        n_unchanged += not ch

    for mode in O.MODES:
        for thresh in (1, 2, H * W + 1):                                                           # the whole stack in one call
            out, changed = M.remove_small_regions(d, thresh, mode)
            assert out.dtype == torch.uint8 and changed.dtype == torch.bool and int(out.max()) <= 1
            o, c = out.cpu().numpy(), changed.cpu().tolist()
            for i in range(len(names)):
                check(i, thresh, mode, o[i], c[i])
            for other in (d.bool(), pitched):
                o2, c2 = M.remove_small_regions(other, thresh, mode)
                assert torch.equal(o2, out) and torch.equal(c2, changed)
            again = M.remove_small_regions(d, thresh, mode)
            assert torch.equal(again[0], out) and torch.equal(again[1], changed)
        for i in range(len(names)):                                                                # a threshold equal to a region's area
            thresh = O.area_thresholds(stack[i])[2]
            for t in (thresh, thresh + 1):                                                         # that region is not small, then it is
                out, changed = M.remove_small_regions(d[i:i + 1], t, mode)
                assert int(out.max()) <= 1
                check(i, t, mode, out[0].cpu().numpy(), bool(changed[0]))
    if H * W > 1:
        assert n_changed and n_unchanged                                                           # both outcomes were met


def test_keep_the_largest_component(device):
    plane = O.blobs(130, 257, seed=5)
    d = torch.from_numpy(plane[None]).to(device)
    out, changed = M.remove_small_regions(d, 130 * 257 + 1, "islands")
    lab, n = O.label(plane, 8)
    sizes = np.bincount(lab.ravel())[1:]
    assert n > 3 and bool(changed[0])
    assert np.array_equal(out[0].cpu().numpy(), (lab == int(np.argmax(sizes)) + 1).astype(np.uint8))
    l2, c2 = M.connected_components(out, 8)
    assert c2.tolist() == [1]


def test_overlapping_output_is_refused_and_the_status_is_ok(device):
    L = lib.load()
    H, W = 7, 5
    d = torch.from_numpy(O.noise(H, W, 0.5)[None].copy()).to(device)
    before = d.clone()
    out = torch.full((1, H, W), 9, dtype=torch.uint8, device=device)
    changed = torch.full((1,), -3, dtype=torch.int32, device=device)
    status = torch.full((4,), -9, dtype=torch.int32, device=device)
    nbytes = C.c_int64()
    assert L.ovm_mask_remove_small_regions_workspace(1, H, W, C.byref(nbytes)) == 0
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def call(o):
        return L.ovm_mask_remove_small_regions(d.data_ptr(), d.stride(0), d.stride(1), 1, H, W, 2, 3, o, W * H, W, changed.data_ptr(),
                                               status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert call(d.data_ptr()) == lib.OVM_ERR_INVALID and call(d.data_ptr() + H * W - 1) == lib.OVM_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(d, before) and status.tolist() == [-9] * 4 and changed.tolist() == [-3]      # nothing ran
    assert call(out.data_ptr()) == 0
    torch.cuda.synchronize()
    ref, ch = O.remove_small_regions(before[0].cpu().numpy(), 2, "both")
    assert status.tolist() == [0, 0, 0, 0] and changed.tolist() == [int(ch)] and np.array_equal(out[0].cpu().numpy(), ref)
    assert torch.equal(d, before)
