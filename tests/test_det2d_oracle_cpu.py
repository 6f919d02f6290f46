"""The plain restatement of tests/det2d_oracle.py against the project's torch oracle (oracle/rpn.py, oracle/heads.py) on the
float family of tests/det2d_cases.py: equal index lists, boxes within 1e-6 (scale-relative). No GPU: this has to hold before
the restatement may judge the HIP kernels (test_gpu_det2d.py)."""
import numpy as np
import pytest
import torch

import det2d_cases as cases
import det2d_oracle as plain
from common import rel_err


def _torch_levels(levels, sides):
    logits, deltas = [], []
    for o, side in zip(levels, sides):
        t = torch.from_numpy(o)
        B = t.shape[0]
        logits.append(t[:, :, :3].reshape(B, side, side, 3).permute(0, 3, 1, 2).contiguous())
        deltas.append(t[:, :, 3:15].reshape(B, side, side, 12).permute(0, 3, 1, 2).contiguous())
    return logits, deltas


@pytest.mark.parametrize("name,seed", cases.RPN_FLOAT_SEEDS)
def test_rpn_restatement_matches_torch_oracle(name, seed):
    from oracle.rpn import rpn_proposals_from_head
    levels, geom, image_sizes, pre, post, thr = cases.rpn_float(name, seed)
    got, M = plain.rpn_proposals(levels, geom, image_sizes, pre, post, thr)
    print(f"{name} seed {seed}: margin/discrepancy {M.summary(('nonempty', 'iou'))}")
    assert not M.unsafe(), M.summary()
    logits, deltas = _torch_levels(levels, geom["sides"])
    ref = rpn_proposals_from_head(logits, deltas, geom["strides"], geom["sizes"], geom["ratios"], image_sizes, pre, post, thr,
                                  with_ids=True)
    for b, (g, (rb, rs, rid)) in enumerate(zip(got, ref)):
        assert g["ids"].tolist() == rid.tolist(), f"image {b}: index lists differ"
        assert np.array_equal(g["scores"], rs.numpy())
        assert rel_err(rb, torch.from_numpy(g["boxes64"])) <= 1e-6


@pytest.mark.parametrize("name,seed", cases.BOXHEAD_FLOAT_SEEDS)
def test_boxhead_restatement_matches_torch_oracle(name, seed):
    from oracle.heads import box_inference
    HO, props, counts, image_sizes, K, st, nt, topk = cases.boxhead_float(name, seed)
    got, M = plain.boxhead_post(HO, props, counts, image_sizes, K, st, nt, topk)
    print(f"{name} seed {seed}: margin/discrepancy {M.summary(('iou', 'score', 'order'))}")
    assert not M.unsafe(), M.summary()
    cls = torch.cat([torch.from_numpy(HO[b, :n, :K + 1]) for b, n in enumerate(counts)])
    dlt = torch.cat([torch.from_numpy(HO[b, :n, K + 1:5 * K + 1]) for b, n in enumerate(counts)])
    proposals = [torch.from_numpy(props[b, :n]) for b, n in enumerate(counts)]
    ref, rows = box_inference(cls, dlt, proposals, image_sizes, st, nt, topk, with_rows=True)
    for b, (g, r, rr) in enumerate(zip(got, ref, rows)):
        assert g["rows"].tolist() == rr.tolist() and g["classes"].tolist() == r["pred_classes"].tolist(), f"image {b}"
        if len(rr):
            assert rel_err(r["pred_boxes"], torch.from_numpy(g["boxes64"])) <= 1e-6
            assert rel_err(r["scores"], torch.from_numpy(g["scores64"])) <= 1e-6
            assert rel_err(r["scores_full"], torch.from_numpy(g["probs64"])) <= 1e-6


def test_exact_family_is_exact():
    """The exact-family inputs keep every box, intersection and union exact in float32, and the restatement resolves the
    constructed edge cases as torchvision does."""
    for E, pre in ((cases.exact_rpn_main(), 1000), (cases.exact_rpn_cut(), 64)):
        for thr in (0.5, 0.7):
            got, M = plain.rpn_proposals(E.levels, E.geom, E.image_sizes, pre, 1000, thr, exact_iou=True)
            assert M.disc.get("nonempty", 0.0) == 0.0 and M.disc.get("iou_terms", 0.0) == 0.0 and M.safe("nonempty")
            for g in got:
                assert np.array_equal(g["boxes64"], g["boxes32"].astype(np.float64))
            # the torch oracle works in float32 throughout: on exact inputs it must take the same decisions, the +-0 tie
            # (torch.sort(stable=True) keeps the lower index) and the float32 quotient at IoU 7/10 included
            from oracle.rpn import rpn_proposals_from_head
            logits, deltas = _torch_levels(E.levels, E.geom["sides"])
            ref = rpn_proposals_from_head(logits, deltas, E.geom["strides"], E.geom["sizes"], E.geom["ratios"], E.image_sizes,
                                          pre, 1000, thr, with_ids=True)
            for g, (rb, rs, rid) in zip(got, ref):
                assert g["ids"].tolist() == rid.tolist() and np.array_equal(g["boxes32"], rb.numpy())
    E = cases.exact_rpn_main()
    got, _ = plain.rpn_proposals(E.levels, E.geom, E.image_sizes, 1000, 1000, 0.7, exact_iou=True)
    for g, (H, W) in zip(got, E.image_sizes):
        ids = [tuple(x) for x in g["ids"].tolist()]
        boxes = {i: tuple(bx) for i, bx in zip(ids, g["boxes64"].tolist())}
        # +-0: the lower anchor index wins in either order; the +inf entry is gone and its neighbour stays
        assert (0, 5 * 3 + 1) in ids and (0, 9 * 3 + 1) not in ids and (0, 6 * 3 + 1) in ids and (0, 10 * 3 + 1) not in ids
        assert (0, 40 * 3 + 1) not in ids and (0, 41 * 3 + 1) in ids
        # equal logits: level-major, then anchor index
        tied = [i for i, s in zip(ids, g["scores"]) if s == np.float32(1.5)]
        assert tied == sorted(tied) and len(tied) == 7
        # chains: A and C stay, B goes; IoU exactly 7/10 is not above 0.7f; the box below the image is gone
        xs = sorted(bx[0] for bx in boxes.values() if bx[1] == 500.0)
        assert xs == [100.0, 116.0, 300.0, 316.0, W - 40.0, W - 28.0]
        assert sorted(bx[0] for bx in boxes.values() if bx[1] == 570.0) == [W - 64.0, W - 32.0]
        assert not any(bx[1] >= H for bx in boxes.values()) and (500.0, H - 128.0, 628.0, float(H)) in boxes.values()
    got5, _ = plain.rpn_proposals(E.levels, E.geom, E.image_sizes, 1000, 1000, 0.5, exact_iou=True)
    for g, (H, W) in zip(got5, E.image_sizes):
        # IoU exactly 1/2 is not above 0.5
        assert sorted(bx[0] for bx in g["boxes64"].tolist() if bx[1] == 570.0) == [W - 64.0, W - 32.0]
    C = cases.exact_rpn_cut()
    got, _ = plain.rpn_proposals(C.levels, C.geom, C.image_sizes, 64, 1000, 0.7, exact_iou=True)
    for b, g in enumerate(got):
        cells = [(37 * i + 11 * b) % 64 for i in range(64)]
        tied = sorted([c * 3 + 1 for c in cells[60:64]] + [c * 3 for c in cells[:6]])[:4]
        lvl0 = [i[1] for i, s in zip(g["ids"].tolist(), g["scores"]) if i[0] == 0 and s == np.float32(0.25)]
        assert lvl0 == tied, "the pre_topk cut inside a tie takes the lowest anchor indices"
