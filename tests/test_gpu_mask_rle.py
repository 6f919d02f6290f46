"""GPU: the device run-length coder (ovm_mask_rle_encode / ovm_mask_rle_decode through ovmono3d_amd.masks) against the numpy
restatement tests/mask_rle_oracle.py: the RLE strings and the counts are equal byte for byte, no tolerance. Shapes straddle the
wave (64 columns), band (64 rows) and workgroup (4 bands) edges; contents are the edge planes of the oracle module."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_rle_oracle as mo
from ovmono3d_amd import lib
from ovmono3d_amd import masks as M

pytestmark = pytest.mark.gpu


def _expect(planes, compressed=True):
    return [mo.encode(p, compressed) for p in planes]


def test_one_by_one(device):
    for v in (0, 1):
        t = torch.full((1, 1, 1), v, dtype=torch.uint8, device=device)
        assert M.encode_rle(t) == _expect([np.full((1, 1), v, np.uint8)])
        assert M.encode_rle(t, compressed=False) == [{"size": [1, 1], "counts": [1] if v == 0 else [0, 1]}]
        assert torch.equal(M.decode_rle(M.encode_rle(t), device), t)


@pytest.mark.parametrize("H,W", mo.SHAPES)
def test_strings_and_counts_equal_the_oracle(device, H, W):
    planes = mo.edge_planes(H, W)
    names = list(planes)
    stack = np.stack([planes[k] for k in names])
    t = torch.from_numpy(stack).to(device)
    got = M.encode_rle(t)
    want = _expect(stack)
    for k, g, w in zip(names, got, want):
        assert g == w, k
    assert M.encode_rle(t, compressed=False) == _expect(stack, False)
    # one call of n planes = n calls of one
    for i in (0, len(names) - 1):
        assert M.encode_rle(t[i:i + 1]) == [want[i]]
    # a bool tensor is the same planes
    assert M.encode_rle(t != 0) == want
    # decode(encode(m)) == (m != 0), from strings and from count lists
    ref = torch.from_numpy((stack != 0).astype(np.uint8)).to(device)
    assert torch.equal(M.decode_rle(got, device), ref)
    assert torch.equal(M.decode_rle(_expect(stack, False), device), ref)
    assert [M.rle_area(r) for r in got] == [int((p != 0).sum()) for p in stack]
    # the run count of the checkerboard is the maximum a plane can have
    assert len(M.string_to_counts(got[names.index("checker")]["counts"])) == H * W + 1


@pytest.mark.parametrize("n", [1, 3, 33])
def test_many_planes_in_one_call_equal_single_calls(device, n):
    H, W = 65, 129
    stack = np.stack([mo.blobs(H, W, seed=100 + i) if i % 3 else mo.edge_planes(H, W)[("zeros", "ones", "checker")[(i // 3) % 3]] for i in range(n)])
    t = torch.from_numpy(stack).to(device)
    got = M.encode_rle(t)
    assert got == _expect(stack)
    assert got == [M.encode_rle(t[i:i + 1])[0] for i in range(n)]
    assert torch.equal(M.decode_rle(got, device), t.ne(0).to(torch.uint8))


def test_pitched_view(device):
    big = torch.from_numpy(np.stack([mo.blobs(80, 150, seed=s) for s in (1, 2, 3)])).to(device)
    crop = big[:, 5:42, 11:64]                                          # 37 x 53 inside 80 x 150: row pitch 150, odd base address
    assert not crop.is_contiguous()
    want = _expect(crop.cpu().numpy())
    assert M.encode_rle(crop) == want
    assert M.encode_rle(crop[::2]) == want[::2]                         # a plane stride of two planes
    assert torch.equal(M.decode_rle(want, device), crop.ne(0).to(torch.uint8))


def test_large_image(device):
    H, W = 1080, 1920
    small = np.zeros((H, W), np.uint8)
    small[500:520, 960:1000] = 1                                        # the first count is 960 * 1080 + 500: four characters
    noise = (np.random.RandomState(3).rand(H, W) < 0.05).astype(np.uint8)
    for plane in (small, noise):
        t = torch.from_numpy(plane[None]).to(device)
        got = M.encode_rle(t)
        assert got == _expect(plane[None])
        assert torch.equal(M.decode_rle(got, device), t)
    assert mo.counts(small)[0] == 960 * 1080 + 500 and len(mo.to_string([960 * 1080 + 500])) >= 4


def _raw_encode(t, max_runs, max_bytes, pad=64):
    """ovm_mask_rle_encode with canaries behind counts_out and string_out: (return code, status, counts, run offsets, string, string
    offsets, the two canary regions)."""
    L = lib.load()
    n, H, W = (int(v) for v in t.shape)
    dev = t.device
    ws_bytes = C.c_int64()
    assert L.ovm_mask_rle_encode_workspace(n, H, W, max_runs, max_bytes, C.byref(ws_bytes)) == 0
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
    counts = torch.full((max_runs + pad,), -1515870811, dtype=torch.int32, device=dev)          # 0xA5A5A5A5
    string = torch.full((max_bytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
    ro = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    so = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    status = torch.full((4,), -99, dtype=torch.int32, device=dev)
    rc = L.ovm_mask_rle_encode(t.data_ptr(), t.stride(0), t.stride(1), n, H, W, counts.data_ptr(), max_runs, ro.data_ptr(), string.data_ptr(), max_bytes,
                               so.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, status.cpu().tolist(), counts.cpu().numpy(), ro.cpu().tolist(), string.cpu().numpy(), so.cpu().tolist()


def test_capacity_is_reported_with_the_totals_and_nothing_is_written_past_the_buffers(device):
    H, W = 37, 53
    stack = np.stack([mo.blobs(H, W, seed=s) for s in (4, 5, 6)])
    t = torch.from_numpy(stack).to(device)
    want_counts = [mo.counts(p) for p in stack]
    want_strings = [mo.to_string(c) for c in want_counts]
    runs, nbytes = sum(len(c) for c in want_counts), sum(len(s) for s in want_strings)
    ro_want = np.concatenate([[0], np.cumsum([len(c) for c in want_counts])]).tolist()
    so_want = np.concatenate([[0], np.cumsum([len(s) for s in want_strings])]).tolist()
    CAP, K = lib.OVM_ERR_CAPACITY, lib.OVM_MASK_RLE_MAX_CHARS
    # one run short: the exact totals and per-plane offsets of both; neither buffer is touched
    rc, st, counts, ro, string, so = _raw_encode(t, runs - 1, K * runs)
    assert rc == 0 and st == [CAP, runs, nbytes, 0] and ro == ro_want and so == so_want
    assert (counts.view(np.uint32) == 0xA5A5A5A5).all() and (string == 0xA5).all()
    # the runs fit, the bytes are one short: both totals exact, the counts written, the string buffer untouched
    rc, st, counts, ro, string, so = _raw_encode(t, runs, nbytes - 1)
    assert rc == 0 and st == [CAP, runs, nbytes, 0] and ro == ro_want and so == so_want
    assert counts[:runs].tolist() == [c for cs in want_counts for c in cs] and (counts[runs:].view(np.uint32) == 0xA5A5A5A5).all()
    assert (string == 0xA5).all()
    # the second call, with the stated totals, succeeds and stays inside its buffers
    rc, st, counts, ro, string, so = _raw_encode(t, runs, nbytes)
    assert rc == 0 and st == [0, runs, nbytes, 0] and ro == ro_want and so == so_want
    assert counts[:runs].tolist() == [c for cs in want_counts for c in cs] and (counts[runs:].view(np.uint32) == 0xA5A5A5A5).all()
    assert string[:nbytes].tobytes().decode() == "".join(want_strings) and (string[nbytes:] == 0xA5).all()
    # the totals without the runs stored, over several bands, column blocks and planes (every edge plane of two larger shapes)
    for H2, W2 in ((65, 129), (250, 333)):
        planes = np.stack(list(mo.edge_planes(H2, W2).values()))
        cs = [mo.counts(p) for p in planes]
        ss = [mo.to_string(c) for c in cs]
        rc, st, counts, ro, string, so = _raw_encode(torch.from_numpy(planes).to(device), 1, K)
        assert rc == 0 and st == [CAP, sum(len(c) for c in cs), sum(len(x) for x in ss), 0]
        assert ro == np.concatenate([[0], np.cumsum([len(c) for c in cs])]).tolist() and so == np.concatenate([[0], np.cumsum([len(x) for x in ss])]).tolist()
        assert (counts.view(np.uint32) == 0xA5A5A5A5).all() and (string == 0xA5).all()
    # the Python layer: a first call that is too small is followed by exactly one that fits
    assert M.encode_rle(t, max_runs=3) == _expect(stack)


def test_decode_reports_counts_that_do_not_sum_to_the_plane(device):
    good = mo.encode(mo.blobs(17, 9, seed=1), compressed=False)
    short = {"size": [17, 9], "counts": [5, 3, 100]}
    long_ = {"size": [17, 9], "counts": [5, 3, 17 * 9]}
    for bad, where in (([good, short], 1), ([long_, good, good], 0)):
        with pytest.raises(ValueError, match=f"first: record {where}"):
            M.decode_rle(bad, device)
    with pytest.raises(ValueError, match="share one size"):
        M.decode_rle([good, {"size": [9, 17], "counts": [153]}], device)
    assert torch.equal(M.decode_rle([good], device)[0].cpu(), torch.from_numpy(mo.decode(good["counts"], 17, 9)))
