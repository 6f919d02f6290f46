"""Inputs for the RPN / box-head post-processing tests (test_det2d_oracle_cpu.py, test_gpu_det2d.py).

Two families. *Float*: random normal logits and deltas with a few hostile entries. *Exact*: inputs on which every float32
operation of the device is exact (anchor ratios 0.25 / 1 / 4, power-of-two sizes and strides, dw = dh = 0, dx / dy multiples of
1/32, integer pixel boxes, images <= 1024 so that areas and unions stay below 2^24), so that boxes compare bit for bit.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

F32 = np.float32
EXACT_RATIOS = (0.25, 1.0, 4.0)


# ------------------------------------------------------------------------------------------------ float family
def float_rpn_case(seed: int, sides, strides, sizes, ratios, image_sizes, hostile=True):
    """Per level float32 [B][side^2][16]: N(0,1) logits, dx / dy ~ N(0, 0.5), dw / dh ~ N(0, 1.5) (some beyond the
    log(1000/16) clamp). hostile: in every image and level one NaN dx, one NaN dw, one inf dx, one +inf dw, and three boxes
    pushed wholly outside the image (left, right, below)."""
    rng = np.random.default_rng(seed)
    B = len(image_sizes)
    levels = []
    for side in sides:
        n = side * side
        o = np.zeros((B, n, 16), dtype=F32)
        o[:, :, :3] = rng.standard_normal((B, n, 3))
        d = rng.standard_normal((B, n, 3, 4))
        d[..., :2] *= 0.5
        d[..., 2:] *= 1.5
        o[:, :, 3:15] = d.reshape(B, n, 12)
        if hostile:
            for b in range(B):
                cells = rng.choice(n, size=min(7, n), replace=False)
                vals = [(0, math.nan), (2, math.nan), (1, math.inf), (3, math.inf), (0, -60.0), (0, 60.0), (1, 60.0)]
                for cell, (comp, v) in zip(cells, vals):
                    a = int(rng.integers(3))
                    o[b, cell, 3 + a * 4 + comp] = v
                    o[b, cell, a] += 3.0                 # a high objectness: the entry reaches the top-k
        levels.append(o)
    geom = dict(sides=tuple(sides), strides=tuple(strides), sizes=tuple(sizes), ratios=tuple(ratios))
    return levels, geom


def float_boxhead_case(seed: int, B: int, R: int, K: int, image_sizes, counts, logit_scale=2.0, nan_row=True, live=1.0):
    """HO float32 [B][R][5K+1], props float32 [B][R][4] (random boxes inside the image), counts as given. Some dw / dh lie beyond
    the clamp; rows past counts[b] carry a confident class-0 logit and must not appear. nan_row: one NaN among the logits of one
    row per image (the whole row is dropped), one NaN and one inf among the deltas of two more. live < 1: only that fraction of
    the rows, scattered, can pass a threshold; the others are confident background (with R*K = 50000 probabilities no seed keeps
    every neighbouring pair of a dense list apart by the safe gap, so the large case keeps its candidates sparse)."""
    rng = np.random.default_rng(seed)
    ld = 5 * K + 1
    HO = np.zeros((B, R, ld), dtype=F32)
    HO[:, :, :K + 1] = rng.standard_normal((B, R, K + 1)) * logit_scale
    if live < 1.0:
        HO[:, :, K] += np.where(rng.random((B, R)) < live, 0.0, 25.0)
    d = rng.standard_normal((B, R, K, 4))
    d[..., 2:] *= 1.5
    big = rng.random((B, R, K)) < 0.02
    d[..., 2] = np.where(big, 25.0 + d[..., 2], d[..., 2])                   # /5 > log(1000/16)
    HO[:, :, K + 1:] = d.reshape(B, R, 4 * K)
    props = np.zeros((B, R, 4), dtype=F32)
    for b in range(B):
        H, W = image_sizes[b]
        xy = rng.random((R, 2)) * np.array([W * 0.7, H * 0.7])
        wh = rng.random((R, 2)) * np.array([W * 0.3, H * 0.3]) + 4.0
        props[b] = np.concatenate([xy, xy + wh], axis=1)
        n = counts[b]
        HO[b, n:, 0] = 12.0
        if nan_row and n >= 4:
            r = rng.choice(n, size=3, replace=False)
            HO[b, r[0], int(rng.integers(K + 1))] = math.nan
            HO[b, r[1], K + 1 + int(rng.integers(4 * K))] = math.nan
            HO[b, r[2], K + 1 + 4 * int(rng.integers(K))] = math.inf         # an inf dx
    return HO, props


# ------------------------------------------------------------------------------------------------ exact family, RPN
class ExactRpn:
    """Places anchor-shaped boxes at chosen integer positions. Every anchor that is not placed keeps the background logit and a
    dx that pushes it wholly left of the image: a zero-area box after the clip, inside the level's segment."""
    BG_LOGIT, BG_DX = -20.0, -128.0

    def __init__(self, sides, strides, sizes, image_sizes):
        self.geom = dict(sides=tuple(sides), strides=tuple(strides), sizes=tuple(sizes), ratios=EXACT_RATIOS)
        self.image_sizes = list(image_sizes)
        B = len(image_sizes)
        self.levels = []
        for side in sides:
            o = np.zeros((B, side * side, 16), dtype=F32)
            o[:, :, :3] = self.BG_LOGIT
            o[:, :, 3:15:4] = self.BG_DX
            self.levels.append(o)
        self.used = set()

    def shape(self, l, a):
        s, r = self.geom["sizes"][l], EXACT_RATIOS[a]
        w = math.sqrt(s * s / r)
        return w, r * w

    def put(self, b, l, a, x1, y1, logit, cell=None):
        """The box of anchor (cell, a) of level l gets its top-left corner at (x1, y1) and the objectness `logit`."""
        side, stride = self.geom["sides"][l], self.geom["strides"][l]
        if cell is None:
            cell = next(c for c in range(side * side) if (b, l, c) not in self.used)
        assert (b, l, cell) not in self.used, "one placed box per cell keeps the index order easy to read"
        self.used.add((b, l, cell))
        w, h = self.shape(l, a)
        dx = (x1 + w / 2.0 - (cell % side) * stride) / w
        dy = (y1 + h / 2.0 - (cell // side) * stride) / h
        assert dx * 32 == round(dx * 32) and dy * 32 == round(dy * 32), "dx, dy must be multiples of 1/32"
        o = self.levels[l][b, cell]
        o[a] = logit
        o[3 + a * 4 + 0], o[3 + a * 4 + 1] = dx, dy
        return cell * 3 + a


def exact_rpn_main(image_sizes=((1024, 1024), (640, 832))):
    """sides (32, 16, 8), strides 32 / 64 / 128, sizes 32 / 64 / 128; pre_topk 1000 (sort length 4096; levels 1 and 2 have fewer
    anchors than pre_topk). Per image, relative to its own width W and height H:
      level 0 (32 x 32 boxes): a -0.0 and a +0.0 logit on two overlapping boxes, in either index order; a +inf logit on a box
        that overlaps a finite one (the +inf entry is dropped and must not suppress it); five equal logits inside the level.
      level 1 (64 x 64 boxes): 192 boxes in decreasing logit order; A > B > C chains at ranks (63, 127, 128) and (61, 64, 191)
        with offsets 0 / 8 / 16 px (IoU 7/9 between neighbours, 3/5 between A and C); a pair with IoU exactly 1/2 and a pair
        with IoU exactly 7/10, both cut by the right image border.
      level 2 (128 x 128 boxes): a box wholly below the image (zero area after the clip) that would cover a kept box if it were
        moved up, equal logits with level 0 (ties across levels go to the lower level)."""
    E = ExactRpn((32, 16, 8), (32, 64, 128), (32, 64, 128), image_sizes)
    for b, (H, W) in enumerate(image_sizes):
        # ---- level 0
        E.put(b, 0, 1, 100, 40, -0.0, cell=5); E.put(b, 0, 1, 102, 40, 0.0, cell=9)          # IoU 30/34: the lower index wins
        E.put(b, 0, 1, 200, 40, 0.0, cell=6);  E.put(b, 0, 1, 202, 40, -0.0, cell=10)
        E.put(b, 0, 1, 300, 40, math.inf, cell=40); E.put(b, 0, 1, 301, 40, 2.5, cell=41)
        for i, cell in enumerate((70, 3, 66, 2, 68)):
            E.put(b, 0, 1, 20 + 40 * i, 100, 1.5, cell=cell)
        E.put(b, 0, 0, 400, 100, 1.5, cell=1)                                                  # 64 x 16, the same logit again
        # ---- level 1: ranks by logit 8 - rank/32 (exact in float32)
        special = {63: (100, 500), 127: (108, 500), 128: (116, 500), 61: (300, 500), 64: (308, 500), 191: (316, 500)}
        slots = [(x, y) for y in range(0, 7 * 66, 66) for x in range(0, 768, 24)]        # neighbours: IoU 5/11
        it = iter(slots)
        for rank in range(192):
            x, y = special[rank] if rank in special else next(it)
            E.put(b, 1, 1, x, y, 8.0 - rank / 32.0)
        E.put(b, 1, 1, W - 64, 570, 9.0); E.put(b, 1, 1, W - 32, 570, 8.75)                    # 32 x 64 inside 64 x 64: IoU 1/2
        E.put(b, 1, 1, W - 40, 500, 8.5); E.put(b, 1, 1, W - 28, 500, 8.25)                    # 28 x 64 inside 40 x 64: IoU 7/10
        # ---- level 2
        E.put(b, 2, 1, 500, H + 64, 3.0)
        E.put(b, 2, 1, 500, H - 128, 1.0)
        E.put(b, 2, 1, 12, 12, 1.5); E.put(b, 2, 1, 200, 200, 0.0)
    return E


def exact_rpn_cut(image_sizes=((256, 256), (192, 224))):
    """sides (8, 4, 2), pre_topk 64 (sort length 2048: one tile with padding). Level 0 holds 70 boxes; ranks 60 .. 69 share one
    logit, so the pre_topk cut falls inside an exact tie and takes the four lowest anchor indices."""
    E = ExactRpn((8, 4, 2), (32, 64, 128), (32, 64, 128), image_sizes)
    for b, (H, W) in enumerate(image_sizes):
        cells = [(37 * i + 11 * b) % 64 for i in range(64)]             # a permutation of the 64 cells: index order != rank order
        pos = [(x, y) for y in range(0, H - 32, 18) for x in range(0, W - 32, 18)]
        for rank in range(70):
            cell, a = cells[rank % 64], (1 if rank < 64 else 0)
            x, y = pos[rank]
            logit = 4.0 - rank / 16.0 if rank < 60 else 0.25
            side, stride = 8, 32
            w, h = E.shape(0, a)
            dx = (x + w / 2.0 - (cell % side) * stride) / w
            dy = (y + h / 2.0 - (cell // side) * stride) / h
            assert dx * 32 == round(dx * 32) and dy * 32 == round(dy * 32)
            o = E.levels[0][b, cell]
            o[a] = logit; o[3 + a * 4], o[3 + a * 4 + 1] = dx, dy
        E.put(b, 1, 1, 16, 16, 0.25); E.put(b, 1, 2, 100, 20, 5.0)
        E.put(b, 2, 1, 40, 40, 0.25); E.put(b, 2, 0, 0, 100, -1.0)
    return E


# ------------------------------------------------------------------------------------------------ exact family, box head
SAFE_GAP = 1e-5      # >> 8 x the float32 softmax error (a few 1e-8); the tests still assert the measured margins


def exact_boxhead_case(seed: int, B: int, R: int, K: int, image_sizes, counts, score_thresh, one_class=False, dup_every=7):
    """Proposals on integer pixels with sides that are multiples of 32, dx / dy deltas 10 * k / 32 (so that d / 10 and dx * width
    are exact and the decoded boxes are integer), dw = dh = 0. Logits are drawn row by row and a row is re-drawn until every
    probability of it that passes score_thresh lies at least SAFE_GAP from every such probability accepted before and from the
    threshold. Every dup_every-th row repeats the logits and deltas of the row before it on another proposal: exact ties, ranked by
    r*K + c. one_class: every row passes the threshold in class 0 only (K = 1: a segment of exactly R candidates).
    Rows past counts[b] carry an attractive logit."""
    rng = np.random.default_rng(seed)
    ld = 5 * K + 1
    HO = np.zeros((B, R, ld), dtype=F32)
    props = np.zeros((B, R, 4), dtype=F32)
    for b in range(B):
        H, W = image_sizes[b]
        taken = np.zeros(0)
        for r in range(R):
            w, h = 32 * int(rng.integers(1, 5)), 32 * int(rng.integers(1, 5))
            x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            props[b, r] = (x1, y1, x1 + w, y1 + h)
            if r >= counts[b]:
                HO[b, r, 0] = 9.0
                continue
            if dup_every and r % dup_every == dup_every - 1 and r > 0:
                HO[b, r] = HO[b, r - 1]
                continue
            while True:
                if one_class:
                    z = np.array([rng.uniform(0.0, 4.0), 0.0])
                else:
                    z = rng.standard_normal(K + 1) * 3.0
                z = z.astype(F32).astype(np.float64)
                e = np.exp(z - z.max())
                p = (e / e.sum())[:K]
                near = p[np.abs(p - np.float64(F32(score_thresh))) < SAFE_GAP]
                p = np.sort(p[p > score_thresh])
                ok = near.size == 0 and (p.size < 2 or np.diff(p).min() >= SAFE_GAP)
                if ok and taken.size and p.size:
                    i = np.searchsorted(taken, p)
                    lo = np.abs(p - taken[np.clip(i - 1, 0, taken.size - 1)])
                    hi = np.abs(taken[np.clip(i, 0, taken.size - 1)] - p)
                    ok = min(lo.min(), hi.min()) >= SAFE_GAP
                if ok:
                    break
            taken = np.sort(np.concatenate([taken, p]))
            HO[b, r, :K + 1] = z
            k = rng.integers(-8, 9, size=(K, 2))
            d = np.zeros((K, 4))
            d[:, :2] = 10.0 * k / 32.0
            HO[b, r, K + 1:] = d.reshape(-1)
    return HO, props


# ------------------------------------------------------------------------------------------------ parametrisations
RATIOS = (0.5, 1.0, 2.0)
# name: (sides, strides, anchor sizes, ratios, image sizes (h, w), pre_topk, post_topk, nms threshold)
RPN_FLOAT_SHAPES = {
    # sort length 4096, the first that needs bitonic_global_kernel; levels 1 and 2 have fewer anchors than pre_topk;
    # post_topk smaller than what NMS leaves
    "s32": ((32, 16, 8), (8, 16, 32), (32, 64, 128), RATIOS, ((256, 256), (200, 240)), 1000, 300, 0.7),
    # sort length 16384: two global stages
    "s48": ((48, 24, 12), (8, 16, 32), (32, 64, 128), RATIOS, ((384, 384), (300, 360)), 1000, 1000, 0.7),
    # sort length 2048: a single tile with padding; post_topk larger than what NMS leaves
    "s8": ((8, 4, 2), (32, 64, 128), (64, 128, 256), RATIOS, ((256, 256), (250, 190)), 64, 1000, 0.7),
    # four levels, as the 4-level towers
    "l4": ((16, 8, 4, 2), (8, 16, 32, 64), (32, 64, 128, 256), RATIOS, ((128, 128), (100, 120)), 200, 500, 0.5),
}
# name: (B, R, K, image sizes, prop counts, score_thresh, nms_thresh, topk, logit scale, live fraction)
BOXHEAD_FLOAT_SHAPES = {
    "r64k5": (2, 64, 5, ((256, 256), (200, 240)), (64, 40), 0.05, 0.5, 100, 2.0, 1.0),
    "r1000k50": (1, 1000, 50, ((512, 512),), (1000,), 0.05, 0.5, 100, 4.0, 0.15),    # 50000 candidate slots: 65536 keys
    "r1024k1": (1, 1024, 1, ((512, 512),), (1024,), 0.05, 0.5, 1024, 2.0, 1.0),
    "r16k63": (2, 16, 63, ((128, 128), (100, 120)), (16, 0), 0.02, 0.5, 10, 3.0, 1.0),   # the lane limit; an image with no proposals;
                                                                                        # topk smaller than the survivors
}


def rpn_float(name: str, seed: int):
    sides, strides, sizes, ratios, image_sizes, pre, post, thr = RPN_FLOAT_SHAPES[name]
    levels, geom = float_rpn_case(seed, sides, strides, sizes, ratios, image_sizes)
    return levels, geom, list(image_sizes), pre, post, thr


def boxhead_float(name: str, seed: int):
    B, R, K, image_sizes, counts, st, nt, topk, scale, live = BOXHEAD_FLOAT_SHAPES[name]
    HO, props = float_boxhead_case(seed, B, R, K, image_sizes, counts, logit_scale=scale, live=live)
    return HO, props, list(counts), list(image_sizes), K, st, nt, topk


# Seeds chosen on the CPU so that every decision of the restatement is safe (margin > 8 x discrepancy). Measured
# margin/discrepancy per class, as test_det2d_oracle_cpu.py prints them:
RPN_FLOAT_SEEDS = [
    ("s32", 2),      # nonempty 1.4e-02/4.2e-04, iou 1.4e-04/4.5e-06
    ("s32", 8),      # nonempty 3.1e-02/5.4e-04, iou 1.9e-04/5.4e-06
    ("s48", 2),      # nonempty 1.9e-02/1.1e-03, iou 2.2e-04/4.3e-06
    ("s48", 8),      # nonempty 1.7e-02/6.4e-04, iou 1.6e-04/8.0e-06
    ("s8", 2),       # nonempty 6.3e-01/3.7e-04, iou 9.4e-03/1.4e-06
    ("s8", 6),       # nonempty 6.2e-01/7.0e-04, iou 1.8e-02/5.7e-07
    ("l4", 3),       # nonempty 1.4e-01/6.6e-04, iou 2.1e-03/1.8e-06
    ("l4", 4),       # nonempty 1.4e-01/5.9e-04, iou 1.5e-03/1.6e-06
]
BOXHEAD_FLOAT_SEEDS = [
    ("r64k5", 2),        # iou 1.8e-02/8.0e-07, score 5.2e-05/7.6e-08, order 1.1e-05/7.6e-08
    ("r64k5", 5),        # iou 5.9e-02/7.2e-07, score 3.0e-04/8.3e-08, order 1.1e-05/8.3e-08
    ("r1000k50", 4),     # iou 4.0e-02/2.8e-07, score 2.0e-04/2.3e-07, order 8.6e-06/2.3e-07
    ("r1000k50", 6),     # iou 9.3e-03/5.5e-07, score 4.9e-05/2.3e-07, order 6.4e-06/2.3e-07
    ("r1024k1", 3),      # iou 4.8e-05/1.9e-06, score 1.8e-04/7.9e-08, order 8.9e-07/7.9e-08
    ("r1024k1", 5),      # iou 4.0e-05/1.8e-06, score 6.2e-06/8.3e-08, order 1.3e-06/8.3e-08
    ("r16k63", 1),       # iou 3.7e-01/3.8e-08, score 2.9e-04/1.1e-07, order 6.3e-05/1.1e-07
    ("r16k63", 2),       # iou 2.4e-01/9.7e-08, score 4.4e-05/7.7e-08, order 1.1e-04/7.7e-08
]
