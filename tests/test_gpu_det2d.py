"""The RPN and box-head post-processing kernels of csrc/det2d.hip on their own (ovm_op_rpn_proposals, ovm_op_boxhead_post),
against the plain restatement of tests/det2d_oracle.py, which must agree exactly: counts, order and identity of every output.

Identity is checked rank by rank. The device returns boxes and scores, not indices, so the restatement's entry at rank k must have
the same score bits (an RPN score is the input logit, copied through) and the same box; entries of different anchors / proposal
rows differ in their boxes by far more than the tolerance. Exact family: boxes bit for bit. Float family: boxes and scores within
2e-6 (scale-relative) of the float64 values, and only on seeds where every decision of the restatement is safe.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import det2d_cases as cases
import det2d_oracle as plain
from common import assert_close

pytestmark = pytest.mark.gpu

TOL = 2e-6          # the layernorm / gemm fp32 tolerance of test_gpu_ops.py: the same arithmetic over fewer operations
SENTINEL = -12345.0
OVM_ERR_CAPACITY = -5


def _lib():
    from ovmono3d_amd import lib
    return lib, lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _images(lib, image_sizes):
    arr = (lib.OvmImage * len(image_sizes))()
    for im, (h, w) in zip(arr, image_sizes):
        im.height, im.width, im.orig_height, im.orig_width = h, w, h, w
    return arr


def run_rpn(device, levels, geom, image_sizes, pre, post, thr):
    lib, L = _lib()
    nlev, B = len(levels), len(image_sizes)
    dev = [torch.from_numpy(np.ascontiguousarray(o)).to(device) for o in levels]
    ptrs = (C.c_void_p * nlev)(*[t.data_ptr() for t in dev])
    sides = (C.c_int32 * nlev)(*geom["sides"])
    strides = (C.c_float * nlev)(*geom["strides"])
    sizes = (C.c_float * nlev)(*geom["sizes"])
    ratios = (C.c_float * 3)(*geom["ratios"])
    pb = torch.full((B, post, 4), SENTINEL, dtype=torch.float32, device=device)
    ps = torch.full((B, post), SENTINEL, dtype=torch.float32, device=device)
    pc = torch.full((B,), -7, dtype=torch.int32, device=device)
    rc = L.ovm_op_rpn_proposals(ptrs, nlev, sides, strides, sizes, ratios, _images(lib, image_sizes), B, pre, post, thr,
                                pb.data_ptr(), ps.data_ptr(), pc.data_ptr(), _stream())
    return rc, pb.cpu().numpy(), ps.cpu().numpy(), pc.cpu().numpy()


def check_rpn(device, levels, geom, image_sizes, pre, post, thr, exact):
    ref, M = plain.rpn_proposals(levels, geom, image_sizes, pre, post, thr, exact_iou=exact)
    print("margin/discrepancy:", M.summary(("nonempty", "iou")))
    if exact:
        assert M.disc.get("nonempty", 0.0) == 0.0 and M.disc.get("iou_terms", 0.0) == 0.0 and M.safe("nonempty")
    else:
        assert not M.unsafe(), M.summary()
    rc, pb, ps, pc = run_rpn(device, levels, geom, image_sizes, pre, post, thr)
    assert rc == 0
    for b, r in enumerate(ref):
        n = len(r["scores"])
        assert pc[b] == n, f"image {b}: {pc[b]} proposals, the restatement has {n}"
        assert np.array_equal(ps[b, :n].view(np.int32), r["scores"].view(np.int32)), f"image {b}: scores / order differ"
        if exact:
            assert np.array_equal(pb[b, :n], r["boxes32"]), f"image {b}: boxes differ"
        elif n:
            assert_close(torch.from_numpy(pb[b, :n]), torch.from_numpy(r["boxes64"]), TOL, f"image {b} boxes")
        assert not pb[b, n:].any() and not ps[b, n:].any(), "rows past prop_count are zero"
    return ref


# ------------------------------------------------------------------------------------------------ RPN
@pytest.mark.parametrize("thr", [0.5, 0.7])
@pytest.mark.parametrize("post", [100, 1000])                # fewer, and more, than what NMS leaves (about 200)
def test_rpn_exact_edges(device, thr, post):
    """cases.exact_rpn_main: +-0 logits in either index order, a +inf logit, ties inside a level and across levels, IoU exactly
    1/2 (thr 0.5) and exactly 7/10 (thr 0.7f) are not suppressed, zero-area boxes inside every level segment, A > B > C chains
    over three 64-bit words (ranks 63 / 127 / 128 and 61 / 64 / 191), two images of different size."""
    E = cases.exact_rpn_main()
    ref = check_rpn(device, E.levels, E.geom, E.image_sizes, 1000, post, thr, exact=True)
    if post == 1000:
        # the restatement itself resolves the row of the chains and of the 7/10 pair as constructed: at 0.7 B goes, C and the
        # 7/10 pair stay; at 0.5 A suppresses C as well (IoU 3/5) and the 7/10 pair loses its second box
        want = {0.7: lambda W: [100.0, 116.0, 300.0, 316.0, W - 40.0, W - 28.0], 0.5: lambda W: [100.0, 300.0, W - 40.0]}[thr]
        for r, (H, W) in zip(ref, E.image_sizes):
            assert sorted(bx[0] for bx in r["boxes64"].tolist() if bx[1] == 500.0) == want(W)


@pytest.mark.parametrize("thr", [0.5, 0.7])
def test_rpn_exact_tie_across_pre_topk(device, thr):
    """cases.exact_rpn_cut: sides (8, 4, 2), pre_topk 64 - a single sort tile with padding; the cut falls inside ten equal
    logits and takes the four lowest anchor indices."""
    E = cases.exact_rpn_cut()
    check_rpn(device, E.levels, E.geom, E.image_sizes, 64, 1000, thr, exact=True)


@pytest.mark.parametrize("name,seed", cases.RPN_FLOAT_SEEDS)
def test_rpn_float(device, name, seed):
    """Random logits and deltas, some beyond the clamp; NaN and inf deltas; boxes pushed wholly outside the image."""
    levels, geom, image_sizes, pre, post, thr = cases.rpn_float(name, seed)
    check_rpn(device, levels, geom, image_sizes, pre, post, thr, exact=False)


def test_rpn_refuses_pre_topk_above_1024(device):
    E = cases.exact_rpn_cut()
    rc, pb, ps, pc = run_rpn(device, E.levels, E.geom, E.image_sizes, 1025, 100, 0.7)
    assert rc == OVM_ERR_CAPACITY
    assert (pb == SENTINEL).all() and (ps == SENTINEL).all() and (pc == -7).all(), "a refused call writes nothing"


# ------------------------------------------------------------------------------------------------ box head
def run_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk, full=True):
    lib, L = _lib()
    B, R, ldh = HO.shape
    dHO = torch.from_numpy(np.ascontiguousarray(HO)).to(device)
    dpr = torch.from_numpy(np.ascontiguousarray(props)).to(device)
    dpc = torch.tensor(list(counts), dtype=torch.int32, device=device)
    cap = B * topk
    boxes = torch.full((cap, 4), SENTINEL, dtype=torch.float32, device=device)
    scores = torch.full((cap,), SENTINEL, dtype=torch.float32, device=device)
    classes = torch.full((cap,), -7, dtype=torch.int32, device=device)
    image_idx = torch.full((cap,), -7, dtype=torch.int32, device=device)
    sfull = torch.full((cap, K), SENTINEL, dtype=torch.float32, device=device)
    oc = torch.full((B,), -7, dtype=torch.int32, device=device)
    rc = L.ovm_op_boxhead_post(dHO.data_ptr(), ldh, dpr.data_ptr(), dpc.data_ptr(), _images(lib, image_sizes), B, R, K, st, nt, topk,
                               boxes.data_ptr(), scores.data_ptr(), classes.data_ptr(), image_idx.data_ptr(),
                               sfull.data_ptr() if full else None, oc.data_ptr(), _stream())
    return rc, [t.cpu().numpy() for t in (boxes, scores, classes, image_idx, sfull, oc)]


def check_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk, exact):
    ref, M = plain.boxhead_post(HO, props, counts, image_sizes, K, st, nt, topk, exact_iou=exact)
    print("margin/discrepancy:", M.summary(("iou", "score", "order")))
    if exact:
        assert M.disc.get("iou_terms", 0.0) == 0.0 and not M.unsafe(("score", "order")), M.summary()
    else:
        assert not M.unsafe(), M.summary()
    rc, (boxes, scores, classes, image_idx, sfull, oc) = run_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk)
    assert rc == 0
    assert oc.tolist() == [len(r["rows"]) for r in ref]
    base = 0
    for b, r in enumerate(ref):
        n = len(r["rows"])
        sl = slice(base, base + n)
        assert classes[sl].tolist() == r["classes"].tolist(), f"image {b}: classes / order differ"
        assert (image_idx[sl] == b).all()
        if n:
            if exact:
                assert np.array_equal(boxes[sl], r["boxes32"]), f"image {b}: boxes differ"
            else:
                assert_close(torch.from_numpy(boxes[sl]), torch.from_numpy(r["boxes64"]), TOL, f"image {b} boxes")
            assert_close(torch.from_numpy(scores[sl]), torch.from_numpy(r["scores64"]), TOL, f"image {b} scores")
            assert_close(torch.from_numpy(sfull[sl]), torch.from_numpy(r["probs64"]), TOL, f"image {b} scores_full")
        base += n
    assert (boxes[base:] == SENTINEL).all() and (scores[base:] == SENTINEL).all() and (classes[base:] == -7).all()
    assert (image_idx[base:] == -7).all() and (sfull[base:] == SENTINEL).all(), "nothing is written past the counts"
    return ref


# (B, R, K, image sizes, prop counts, score_thresh, topk, one_class)
BOXHEAD_EXACT = {
    "r64k5": (2, 64, 5, ((256, 256), (200, 240)), (64, 40), 0.05, 100, False),          # rows past prop_count are attractive
    "r1000k50": (1, 1000, 50, ((512, 512),), (1000,), 0.05, 100, False),                # 65536 keys
    "r1024k1": (1, 1024, 1, ((1024, 1024),), (1024,), 0.3, 1024, True),                 # one class segment of exactly 1024
    "r16k63": (2, 16, 63, ((128, 128), (160, 128)), (16, 0), 0.02, 10, False),          # lane limit; an image with count 0; topk cut
}


@pytest.mark.parametrize("name", list(BOXHEAD_EXACT))
def test_boxhead_exact(device, name):
    """Integer boxes, probabilities separated by construction, duplicated rows (exact ties ranked by r*K + c), IoU of exactly 1/2
    among the integer boxes; with K = 63 and 16 rows most classes have no candidate at all."""
    B, R, K, image_sizes, counts, st, topk, one = BOXHEAD_EXACT[name]
    HO, props = cases.exact_boxhead_case(1, B, R, K, image_sizes, counts, st, one_class=one)
    ref = check_boxhead(device, HO, props, counts, image_sizes, K, st, 0.5, topk, exact=True)
    if name == "r1024k1":
        assert (plain._softmax(HO[0, :, :2], np.float64)[:, 0] > st).all(), "all 1024 rows are candidates of the one class"


def test_boxhead_class_with_one_candidate_and_with_none(device):
    """K = 5: class 1 has exactly one candidate, class 3 has none, the rest are ordinary."""
    B, R, K, image_sizes, counts, st, topk, _ = BOXHEAD_EXACT["r64k5"]
    HO, props = cases.exact_boxhead_case(2, B, R, K, image_sizes, counts, st)
    HO[:, :, 1] = -30.0
    HO[:, :, 3] = -30.0
    HO[:, 7, :K + 1] = np.asarray([-1.0, 2.0, -2.0, -30.0, -1.5, 0.0], dtype=np.float32)
    ref = check_boxhead(device, HO, props, counts, image_sizes, K, st, 0.5, topk, exact=True)
    for r in ref:
        assert (r["classes"] == 1).sum() == 1 and (r["classes"] == 3).sum() == 0


@pytest.mark.parametrize("name,seed", cases.BOXHEAD_FLOAT_SEEDS)
def test_boxhead_float(device, name, seed):
    """Random logits and deltas, some beyond the clamp; a NaN logit (the whole row goes), NaN and inf deltas."""
    HO, props, counts, image_sizes, K, st, nt, topk = cases.boxhead_float(name, seed)
    check_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk, exact=False)


def test_boxhead_threshold_nothing_passes(device):
    HO, props, counts, image_sizes, K, st, nt, topk = cases.boxhead_float("r64k5", 2)
    ref = check_boxhead(device, HO, props, counts, image_sizes, K, 2.0, nt, topk, exact=False)
    assert all(len(r["rows"]) == 0 for r in ref)


def test_boxhead_without_scores_full(device):
    HO, props, counts, image_sizes, K, st, nt, topk = cases.boxhead_float("r64k5", 2)
    _, a = run_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk, full=True)
    rc, b = run_boxhead(device, HO, props, counts, image_sizes, K, st, nt, topk, full=False)
    assert rc == 0
    for i in (0, 1, 2, 3, 5):
        assert np.array_equal(a[i], b[i])


def test_boxhead_refuses_64_classes(device):
    K = 64
    HO = np.zeros((1, 4, 5 * K + 1), dtype=np.float32)
    props = np.tile(np.asarray([0, 0, 32, 32], dtype=np.float32), (1, 4, 1))
    rc, (boxes, scores, classes, image_idx, sfull, oc) = run_boxhead(device, HO, props, (4,), ((64, 64),), K, 0.05, 0.5, 10)
    assert rc == OVM_ERR_CAPACITY
    assert (oc == -7).all() and (scores == SENTINEL).all(), "a refused call writes nothing"
