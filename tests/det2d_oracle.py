"""Plain restatement of the RPN and box-head post-processing (detectron2 ``find_top_rpn_proposals`` and
``fast_rcnn_inference``) for exact comparison with the HIP kernels of csrc/det2d.hip.

Every float quantity that a decision rests on - the decoded and clipped box, the softmax probability, the IoU - is computed
twice: in float64, and in a float32 replica of the same formula in the same operation order (``np.float32`` arithmetic, IoU as
``inter / (a + b - inter)``, thresholds as ``np.float32``). Decisions are taken on the float64 values; ties in score go to the
lower index and +0 / -0 count as equal. Next to their outputs the functions return a ``Margins`` record: per class of decision
the smallest distance of the float64 quantity from its threshold (for a ranking: the smallest gap between neighbouring float64
probabilities) and the largest |float64 - float32 replica| seen for that quantity. A decision is *safe* when the margin exceeds
``SAFE_FACTOR`` times that discrepancy: the device's expf and FMA contraction differ from numpy float32 by a few ulp, not by
multiples of the whole replica error. Only a run whose every decision is safe may be compared exactly.

Classes of decision:
  nonempty  box non-empty after the clip (RPN). The quantity is the clipped width / height; where both edges were clamped to the
            same image border (the clamp itself is exact in any precision) it is the distance of the nearer raw edge from that
            border, which is what would have to change for the box to become non-empty. A kept box counts with the smaller of
            its two extents, a dropped one with the empty extent that is farther from changing.
  iou       IoU against the NMS threshold, over every (kept box, later box of its group) pair.
  score     box-head probability against score_thresh, over every class of every finite row.
  order     gap between neighbouring probabilities, inside each class before NMS and in the final list. Entries of rows whose
            logits are bit-identical tie exactly on any hardware and are ranked by r*K + c; they are not counted.
  iou_terms (discrepancy only) intersection and union. ``exact_iou=True`` takes the IoU decisions on the float32 quotient
            instead, as torchvision does; that is meaningful only where both terms are exact in float32 (integers below 2^24),
            so that the one rounding left is the correctly rounded division. The call raises when they are not.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

SCALE_CLAMP = np.float32(math.log(1000.0 / 16.0))
SAFE_FACTOR = 8.0
CLASSES = ("nonempty", "iou", "score", "order")


class Margins:
    def __init__(self):
        self.margin: Dict[str, float] = {}
        self.disc: Dict[str, float] = {}

    def note(self, cls: str, margin=None, disc=None):
        if margin is not None:
            m = np.asarray(margin, dtype=np.float64).ravel()
            m = m[~np.isnan(m)]
            if m.size:
                self.margin[cls] = min(self.margin.get(cls, math.inf), float(m.min()))
        if disc is not None:
            d = np.asarray(disc, dtype=np.float64).ravel()
            d = d[~np.isnan(d)]
            if d.size:
                self.disc[cls] = max(self.disc.get(cls, 0.0), float(d.max()))

    def merge(self, other: "Margins"):
        for k, v in other.margin.items():
            self.note(k, margin=v)
        for k, v in other.disc.items():
            self.note(k, disc=v)

    def safe(self, cls: str) -> bool:
        return self.margin.get(cls, math.inf) > SAFE_FACTOR * self.disc.get(cls, 0.0)

    def unsafe(self, classes: Sequence[str] = CLASSES) -> List[str]:
        return [c for c in classes if not self.safe(c)]

    def summary(self, classes: Sequence[str] = CLASSES) -> str:
        return ", ".join(f"{c} {self.margin.get(c, math.inf):.1e}/{self.disc.get(c, 0.0):.1e}" for c in classes)


def cell_anchors(size: float, ratios: Sequence[float]) -> np.ndarray:
    """DefaultAnchorGenerator.generate_cell_anchors: computed in double, stored float32. [len(ratios)][4]"""
    out = []
    for r in ratios:
        w = math.sqrt(float(size) * float(size) / float(r))
        h = float(r) * w
        out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return np.asarray(out, dtype=np.float32)


def _decode(anchors: np.ndarray, deltas: np.ndarray, weights, T) -> np.ndarray:
    """Box2BoxTransform.apply_deltas in the arithmetic T; anchors, deltas [n][4] float32."""
    a, d = anchors.astype(T), deltas.astype(T)
    with np.errstate(all="ignore"):
        widths, heights = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        ctr_x, ctr_y = a[:, 0] + T(0.5) * widths, a[:, 1] + T(0.5) * heights
        dx, dy = d[:, 0] / T(weights[0]), d[:, 1] / T(weights[1])
        dw = np.minimum(d[:, 2] / T(weights[2]), T(SCALE_CLAMP))          # a NaN stays a NaN, as in torch.clamp
        dh = np.minimum(d[:, 3] / T(weights[3]), T(SCALE_CLAMP))
        pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
        pw, ph = np.exp(dw) * widths, np.exp(dh) * heights
        out = np.stack([pcx - T(0.5) * pw, pcy - T(0.5) * ph, pcx + T(0.5) * pw, pcy + T(0.5) * ph], axis=1)
    assert out.dtype == T
    return out


def _clip(b: np.ndarray, hw: Tuple[int, int]) -> np.ndarray:
    T = b.dtype.type
    h, w = T(hw[0]), T(hw[1])
    with np.errstate(invalid="ignore"):
        return np.stack([np.minimum(np.maximum(b[:, 0], T(0)), w), np.minimum(np.maximum(b[:, 1], T(0)), h),
                         np.minimum(np.maximum(b[:, 2], T(0)), w), np.minimum(np.maximum(b[:, 3], T(0)), h)], axis=1)


def _extent_margin(lo64, hi64, lo32, hi32, size: int):
    """Per box, along one axis: (extent > 0 decided in float64, margin of that decision, float64-vs-float32 discrepancy)."""
    S = float(size)
    c64 = np.clip(hi64, 0.0, S) - np.clip(lo64, 0.0, S)
    c32 = (np.clip(hi32, np.float32(0), np.float32(S)) - np.clip(lo32, np.float32(0), np.float32(S))).astype(np.float64)
    margin, disc = np.abs(c64), np.abs(c64 - c32)
    beyond = (lo64 >= S) & (hi64 >= S)                 # both edges clamped to the far border: empty unless lo drops below it
    margin = np.where(beyond, lo64 - S, margin); disc = np.where(beyond, np.abs(lo64 - lo32), disc)
    before = (lo64 <= 0.0) & (hi64 <= 0.0)
    margin = np.where(before, -hi64, margin); disc = np.where(before, np.abs(hi64 - hi32), disc)
    return c64 > 0.0, margin, disc


def _iou_rows(b: np.ndarray, i: int):
    """inter, union and IoU of box i against boxes i+1.. in the arithmetic of b."""
    T = b.dtype.type
    r = b[i + 1:]
    with np.errstate(all="ignore"):
        w = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]), T(0))
        h = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]), T(0))
        inter = w * h
        aa, ab = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]), (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        union = aa + ab - inter
        q = inter / union
    assert q.dtype == T
    return inter, union, q


def nms_sorted(b64: np.ndarray, b32: np.ndarray, thr: float, M: Margins, exact_iou=False) -> np.ndarray:
    """Greedy NMS (torchvision.ops.nms: IoU > thr, strict) over boxes already in decreasing-score order; keep mask."""
    n = len(b64)
    thr32 = np.float32(thr)
    suppressed = np.zeros(n, dtype=bool)
    for i in range(n):
        if suppressed[i] or i + 1 >= n:
            continue
        i64, u64, q64 = _iou_rows(b64, i)
        i32, u32, q32 = _iou_rows(b32, i)
        M.note("iou", margin=np.abs(q64 - np.float64(thr32)), disc=np.abs(q64 - q32.astype(np.float64)))
        M.note("iou_terms", disc=np.maximum(np.abs(i64 - i32), np.abs(u64 - u32)))
        with np.errstate(invalid="ignore"):
            suppressed[i + 1:] |= (q32 > thr32) if exact_iou else (q64 > np.float64(thr32))
    if exact_iou and M.disc.get("iou_terms", 0.0) != 0.0:
        raise ValueError("exact_iou needs intersections and unions that are exact in float32")
    return ~suppressed


def nms(boxes: np.ndarray, scores: np.ndarray, thr: float, M: Margins, exact_iou=False) -> np.ndarray:
    """torchvision.ops.nms on float32 inputs: kept indices in decreasing-score order (ties: lower index, +-0 equal)."""
    scores = np.asarray(scores, dtype=np.float32)
    order = np.argsort(-(scores + np.float32(0)), kind="stable")
    b32 = np.asarray(boxes, dtype=np.float32)[order]
    keep = nms_sorted(b32.astype(np.float64), b32, thr, M, exact_iou)
    return order[keep]


def rpn_proposals(levels_o: List[np.ndarray], geom: dict, image_sizes: List[Tuple[int, int]], pre_topk: int, post_topk: int,
                  thr: float, exact_iou=False):
    """levels_o: per level float32 [B][side*side][16] (3 objectness logits, then 3 x 4 deltas; no NaN logit).
    geom: dict(sides, strides, sizes, ratios). image_sizes: per image (height, width), the clip size.
    Returns (per image dict(boxes64, boxes32 [n][4], scores [n] float32, ids [n][2] = (level, cell*3 + anchor)), Margins)."""
    B = levels_o[0].shape[0]
    M = Margins()
    out = []
    for b in range(B):
        H, W = image_sizes[b]
        c64, c32, csc, cid = [], [], [], []
        for l, o in enumerate(levels_o):
            side, stride = geom["sides"][l], np.float32(geom["strides"][l])
            base = cell_anchors(geom["sizes"][l], geom["ratios"])
            logits = o[b][:, :3].reshape(-1)
            assert not np.isnan(logits).any()
            deltas = o[b][:, 3:15].reshape(-1, 4)
            order = np.argsort(-(logits + np.float32(0)), kind="stable")[:min(len(logits), pre_topk)]     # -0 + 0 = +0
            cell, a = order // 3, order % 3
            shift = np.stack([(cell % side).astype(np.float32) * stride, (cell // side).astype(np.float32) * stride], axis=1)
            anchors = np.concatenate([shift, shift], axis=1) + base[a]
            assert anchors.dtype == np.float32
            r64, r32 = _decode(anchors, deltas[order], (1, 1, 1, 1), np.float64), _decode(anchors, deltas[order], (1, 1, 1, 1), np.float32)
            fin64 = np.isfinite(r64).all(axis=1) & np.isfinite(logits[order])
            fin32 = np.isfinite(r32).all(axis=1) & np.isfinite(logits[order])
            if (fin64 != fin32).any():
                raise ValueError("a box is finite in one precision only")
            r64, r32, sc, ids = r64[fin64], r32[fin64], logits[order][fin64], order[fin64]
            okx, mx, dx = _extent_margin(r64[:, 0], r64[:, 2], r32[:, 0], r32[:, 2], W)
            oky, my, dy = _extent_margin(r64[:, 1], r64[:, 3], r32[:, 1], r32[:, 3], H)
            ok = okx & oky
            # a kept box needs both extents positive; a dropped one stays dropped while one empty extent stays empty
            use_x = np.where(ok, mx <= my, ~okx & (oky | (mx >= my)))
            M.note("nonempty", margin=np.where(use_x, mx, my), disc=np.where(use_x, dx, dy))
            k64, k32 = _clip(r64, (H, W))[ok], _clip(r32, (H, W))[ok]
            keep = nms_sorted(k64, k32, thr, M, exact_iou)
            c64.append(k64[keep]); c32.append(k32[keep]); csc.append(sc[ok][keep])
            cid.append(np.stack([np.full(int(keep.sum()), l, dtype=np.int64), ids[ok][keep]], axis=1))
        c64, c32, csc, cid = np.concatenate(c64), np.concatenate(c32), np.concatenate(csc), np.concatenate(cid)
        order = np.argsort(-(csc + np.float32(0)), kind="stable")[:post_topk]        # level-major slot order breaks ties
        out.append(dict(boxes64=c64[order], boxes32=c32[order], scores=csc[order], ids=cid[order]))
    return out, M


def _softmax(x: np.ndarray, T) -> np.ndarray:
    x = x.astype(T)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    assert p.dtype == T
    return p


def _order_margin(p64, p32, rows, logits, M: Margins):
    """p64 .. of entries already in rank order: notes the neighbour gaps, skipping the exact ties of bit-identical rows."""
    for i in range(len(p64) - 1):
        gap = abs(p64[i] - p64[i + 1])
        if gap == 0.0 and p32[i] == p32[i + 1] and logits[rows[i]].tobytes() == logits[rows[i + 1]].tobytes():
            continue
        M.note("order", margin=gap)


def boxhead_post(HO: np.ndarray, props: np.ndarray, counts: Sequence[int], image_sizes: List[Tuple[int, int]], K: int,
                 score_thr: float, nms_thr: float, topk: int, exact_iou=False):
    """HO float32 [B][R][>= 5K+1] (K+1 logits, then K x 4 deltas), props float32 [B][R][4], counts [B].
    Returns (per image dict(rows, classes [n], boxes64, boxes32 [n][4], scores64, scores32 [n], probs64 [n][K]), Margins)."""
    B = HO.shape[0]
    M = Margins()
    thr32 = np.float32(score_thr)
    out = []
    for b in range(B):
        n = int(counts[b])
        logits = np.ascontiguousarray(HO[b, :n, :K + 1])
        deltas = HO[b, :n, K + 1:5 * K + 1].reshape(n * K, 4)
        anchors = np.repeat(props[b, :n], K, axis=0)
        p64, p32 = _softmax(logits, np.float64), _softmax(logits, np.float32)
        r64 = _decode(anchors, deltas, (10, 10, 5, 5), np.float64).reshape(n, K * 4)
        r32 = _decode(anchors, deltas, (10, 10, 5, 5), np.float32).reshape(n, K * 4)
        fin64 = np.isfinite(r64).all(axis=1) & np.isfinite(p64).all(axis=1)
        fin32 = np.isfinite(r32).all(axis=1) & np.isfinite(p32).all(axis=1)
        if (fin64 != fin32).any():
            raise ValueError("a row is finite in one precision only")
        b64 = _clip(r64.reshape(-1, 4), image_sizes[b]).reshape(n, K, 4)
        b32 = _clip(r32.reshape(-1, 4), image_sizes[b]).reshape(n, K, 4)
        rows_ok = np.where(fin64)[0]
        M.note("score", margin=np.abs(p64[rows_ok, :K] - np.float64(thr32)), disc=np.abs(p64[rows_ok, :K] - p32[rows_ok, :K]))
        M.note("order", disc=np.abs(p64[rows_ok, :K] - p32[rows_ok, :K]))
        surv = []                                        # (r, c) of the NMS survivors
        for c in range(K):
            r = rows_ok[p64[rows_ok, c] > np.float64(thr32)]
            r = r[np.argsort(-p64[r, c], kind="stable")]                    # ties: lower row first
            _order_margin(p64[r, c], p32[r, c], r, logits, M)
            keep = nms_sorted(b64[r, c], b32[r, c], nms_thr, M, exact_iou)
            surv += [(int(x), c) for x in r[keep]]
        surv.sort(key=lambda rc: (-p64[rc[0], rc[1]], rc[0] * K + rc[1]))
        rr = np.asarray([rc[0] for rc in surv], dtype=np.int64)
        cc = np.asarray([rc[1] for rc in surv], dtype=np.int64)
        # the cut at topk is one more ranking decision: the gaps are taken over the whole list
        _order_margin(p64[rr, cc], p32[rr, cc], rr, logits, M)
        rr, cc = rr[:topk], cc[:topk]
        out.append(dict(rows=rr, classes=cc, boxes64=b64[rr, cc].reshape(-1, 4), boxes32=b32[rr, cc].reshape(-1, 4),
                        scores64=p64[rr, cc], scores32=p32[rr, cc], probs64=p64[rr, :K].reshape(-1, K)))
    return out, M
