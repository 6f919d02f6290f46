"""Omni3D AP evaluation with true 3D IoU ("next" row 1 of SURVEY.md 8f).

Upstream Omni3D semantics of the reference's ``Omni3Deval`` (cubercnn/evaluation/omni3d_evaluation.py):
``Omni3DParams`` :1394-1461 (2D: IoU 0.5:0.05:0.95, area ranges; 3D: IoU 0.05:0.05:0.50, depth ranges [0,10,35,1e5]),
``_prepare`` :1515-1545 (ignore2D / ignore3D flags), COCO matching per (image, category, range), ``accumulate``
:1547-1688 (101 recall points, stable sort on scores), ``summarize`` :2072-2224 (AP, AP15 / AP25 / AP50, near / medium /
far), ``Omni3DevalWithNHD`` :2293-2484 (disentangled NHD of IoU-matched pairs, ``nhd.py``). The 3D IoU is
``box3d_overlap`` (:109-169) on the HIP kernel ``ovm_box3d_iou``. Ground-truth construction (filter settings, the ignore
rule, dataset <-> contiguous category ids) is ``omni3d_gt.py``.

The reference FORK lost its ``computeIoU`` override, so its "3D" AP is really computed with pycocotools' 2D IoU
(SURVEY.md 0.5); ``fork_compat_2d_iou=True`` reproduces that behaviour, the default is upstream's.
pycocotools is not a dependency (and not importable here, so AP values are pinned by cases with a known answer and by
a by-definition restatement in tests/test_eval.py, not by running the reference's evaluator: "parity unpinned" for
real-data AP).

``eval_prox`` restores upstream Omni3D's proximity evaluation (reference :263 turns it on for Objectron and SUNRGBD, option
:1483-1485, threshold :1459-1461), whose ``evaluateImg`` / ``computeIoU`` overrides the fork lost; ``matcher="device"`` runs the
2D IoU and the greedy matching of every cell in HIP (``csrc/eval_match.hip``) with results equal to the host's;
``stage3d="device"`` adds the two 3D stages around it: the 3D IoU of every cell in one launch (``ovm_eval_iou3d``, the values of
``ovm_box3d_iou``) and the NHD pairing and scoring (``ovm_eval_nhd``, the assignments solved exactly in fp64), all from one upload.
"""
from __future__ import annotations

import ctypes as C
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import lib as _lib
from . import nhd as _nhd


def box3d_overlap(boxes_dt: torch.Tensor, boxes_gt: torch.Tensor, eps_coplanar: float = 1e-4, eps_nonzero: float = 1e-8) -> torch.Tensor:
    """(N, 8, 3) x (M, 8, 3) corners (pytorch3d order) -> (N, M) IoU on the HIP device. Detections that fail the
    reference's coplanarity / non-zero-area screening get IoU 0 (:160-167). No CPU fallback."""
    L = _lib.load()
    if boxes_dt.device.type != "cuda":
        raise RuntimeError("box3d_overlap runs on the HIP device only (no CPU fallback)")
    dt = boxes_dt.to(torch.float32).reshape(-1, 24).contiguous()
    gt = boxes_gt.to(dt.device, torch.float32).reshape(-1, 24).contiguous()
    N, M = int(dt.shape[0]), int(gt.shape[0])
    out = torch.zeros((N, M), dtype=torch.float32, device=dt.device)
    if N and M:
        stream = C.c_void_p(torch.cuda.current_stream(dt.device).cuda_stream)
        _lib.check(L.ovm_box3d_iou(dt.data_ptr(), gt.data_ptr(), N, M, float(eps_coplanar), float(eps_nonzero), out.data_ptr(), None, stream),
                   what="ovm_box3d_iou")
    return out


def iou2d_xywh(dt: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """pycocotools maskUtils.iou for boxes without crowd regions: (N,4) x (M,4) xywh -> (N,M)."""
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)))
    d, g = np.asarray(dt, np.float64)[:, None, :], np.asarray(gt, np.float64)[None, :, :]
    iw = np.clip(np.minimum(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.maximum(d[..., 0], g[..., 0]), 0, None)
    ih = np.clip(np.minimum(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.maximum(d[..., 1], g[..., 1]), 0, None)
    inter = iw * ih
    union = d[..., 2] * d[..., 3] + g[..., 2] * g[..., 3] - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


class Omni3DParams:
    """reference :1394-1461"""

    def __init__(self, mode: str = "2D"):
        if mode == "2D":
            self.iouThrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
            self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
            self.areaRngLbl = ["all", "small", "medium", "large"]
        elif mode == "3D":
            self.iouThrs = np.linspace(0.05, 0.5, int(np.round((0.5 - 0.05) / 0.05)) + 1, endpoint=True)
            self.areaRng = [[0, 1e5], [0, 10], [10, 35], [35, 1e5]]
            self.areaRngLbl = ["all", "near", "medium", "far"]
        else:
            raise Exception("mode %s not supported" % mode)
        self.recThrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.imgIds: List = []
        self.catIds: List = []
        self.useCats = 1
        self.iouType = "bbox"
        self.mode = mode
        self.proximity_thresh = 0.3


class _Cell:
    """One (image, category) cell: detections in descending score order (stable), cut to the largest maxDets; ground truth
    in file order; ``iou`` [D,G] between them. ``prox``: the proximity rules apply to the cell; ``in_prox`` [D]: some 2D IoU
    with the cell's ground truth (any of it) exceeds ``proximity_thresh``."""
    __slots__ = ("dt", "gt", "iou", "score", "dt_rng", "gt_rng", "gt_flag", "gt_crowd", "dt_box", "gt_box", "prox", "in_prox")


# numpy mirror of include/ovm3d.h OvmEvalCell
_CELL_DTYPE = np.dtype([("iou_off", "<i8"), ("dt_off", "<i4"), ("n_dt", "<i4"), ("gt_off", "<i4"), ("n_gt", "<i4"), ("prox", "<i4"),
                        ("reserved", "<i4")])


def _exclusive_cumsum(n: np.ndarray) -> np.ndarray:
    out = np.zeros(len(n), dtype=np.int64)
    np.cumsum(n[:-1], out=out[1:])
    return out


def _pack_segments(arrays):
    """One contiguous byte buffer holding every array, each at an 8-byte aligned offset: (buffer, offsets)."""
    offs, pos = [], 0
    for a in arrays:
        offs.append(pos)
        pos += (a.nbytes + 7) // 8 * 8
    buf = np.zeros(max(pos, 8), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()
    return buf, offs


class Omni3Deval:
    """COCO-style AP over Omni3D annotations. ``gts`` / ``dts`` are lists of dicts:
    gt: image_id, category_id, bbox [x,y,w,h], bbox3D [8][3], depth, optional area, ignore2D, ignore3D, iscrowd
    dt: image_id, category_id, bbox, score, and for 3D bbox3D + depth (the records of ``instances_to_coco_json``).
    ``img_ids`` / ``cat_ids``: the evaluated images and categories (the reference takes them from the ground-truth dataset,
    :1489-1491); by default every id that occurs. In 3D mode, pairs of a detection and its best-IoU ground truth with
    IoU >= ``nhd_iou_threshold`` also get the disentangled NHD (``Omni3DevalWithNHD`` :2293-2484) when both carry
    centre / dimensions / rotation.

    The evaluation is the published COCOeval procedure (greedy matching per IoU threshold in score order, ignore rules,
    101-point interpolated precision); it is organised here as array operations over the thresholds rather than the
    per-threshold loops of pycocotools, and ``tests/test_eval.py`` holds it against a by-definition restatement.

    ``eval_prox``: upstream Omni3D's proximity evaluation for datasets that are not exhaustively annotated (reference
    :1483-1485) - True / False for every cell, or a collection of image ids whose cells it applies to. In such a cell, per range,
    a detection whose 2D IoU with every ground truth of the cell (ignored, out-of-range and crowd boxes included) is at most
    ``proximity_thresh`` is ignored, and when every ground truth is ignored in the range (or there is none) every detection is.
    ``matcher``: "host" (numpy) or "device" (HIP kernels ``ovm_eval_iou2d`` / ``ovm_eval_match``, same results; no CPU
    fallback). ``stage3d``: "host" (one ``ovm_box3d_iou`` call per image, NHD through scipy) or "device" (``ovm_eval_iou3d`` and
    ``ovm_eval_nhd`` in the device matcher's upload: the same IoU bit for bit, the NHD in fp64 from the same fp32-rounded fields);
    needs ``matcher="device"`` and true 3D mode."""

    def __init__(self, gts: Sequence[Dict], dts: Sequence[Dict], mode: str = "3D", device: Optional[torch.device] = None,
                 fork_compat_2d_iou: bool = False, img_ids: Optional[Sequence] = None, cat_ids: Optional[Sequence] = None,
                 nhd_iou_threshold: float = 0.5, eval_prox=False, matcher: str = "host", stage3d: str = "host"):
        if matcher not in ("host", "device"):
            raise ValueError(f"matcher must be 'host' or 'device', not {matcher!r}")
        if stage3d not in ("host", "device"):
            raise ValueError(f"stage3d must be 'host' or 'device', not {stage3d!r}")
        if stage3d == "device" and (matcher != "device" or mode != "3D" or fork_compat_2d_iou):
            raise ValueError("stage3d='device' needs matcher='device' and 3D mode without fork_compat_2d_iou")
        self.mode = mode
        self.params = Omni3DParams(mode)
        self.device = device
        self.matcher = matcher
        self.stage3d = stage3d
        self.eval_prox = bool(eval_prox) if isinstance(eval_prox, (bool, np.bool_)) else frozenset(eval_prox)
        self.fork_compat_2d_iou = fork_compat_2d_iou
        self.nhd_iou_threshold = nhd_iou_threshold
        self._gts_all, self._dts_all = [dict(g) for g in gts], [dict(d) for d in dts]
        for i, g in enumerate(self._gts_all):
            g.setdefault("id", i + 1)
            g.setdefault("iscrowd", 0)
            if "area" not in g:
                g["area"] = float(g["bbox"][2] * g["bbox"][3])
        for i, d in enumerate(self._dts_all):
            d.setdefault("id", i + 1)
            if "area" not in d:
                d["area"] = float(d["bbox"][2] * d["bbox"][3])
        self.params.imgIds = sorted(img_ids) if img_ids is not None else \
            sorted({g["image_id"] for g in self._gts_all} | {d["image_id"] for d in self._dts_all})
        self.params.catIds = sorted(cat_ids) if cat_ids is not None else \
            sorted({g["category_id"] for g in self._gts_all} | {d["category_id"] for d in self._dts_all})
        self.cells: Dict = {}
        self.per_cell: Dict = {}
        self.eval: Dict = {}
        self.nhd_pairs: List[Dict] = []
        self.nhd_pair_ids: List = []                                            # (detection id, ground-truth id) of each entry of nhd_pairs

    # ---- cells and their IoU ------------------------------------------------------------------------------------------
    def _prox_applies(self, img) -> bool:
        return self.eval_prox if isinstance(self.eval_prox, bool) else img in self.eval_prox

    def _build_cells(self, with_iou: bool = True):
        """``with_iou=False``: leave the 2D IoU (and the proximity flags) to the device matcher."""
        p = self.params
        flag = "ignore2D" if self.mode == "2D" else "ignore3D"                  # _prepare :1515-1545
        rng_key = "area" if self.mode == "2D" else "depth"
        imgs, cats = set(p.imgIds), set(p.catIds)
        by_gt, by_dt = defaultdict(list), defaultdict(list)
        for g in self._gts_all:
            if g["image_id"] in imgs and g["category_id"] in cats:
                by_gt[g["image_id"], g["category_id"]].append(g)
        for d in self._dts_all:
            if d["image_id"] in imgs and d["category_id"] in cats:
                by_dt[d["image_id"], d["category_id"]].append(d)
        top = p.maxDets[-1]
        self.cells = {}
        for key in set(by_gt) | set(by_dt):
            c = _Cell()
            dt = by_dt.get(key, [])
            order = np.argsort(-np.array([d["score"] for d in dt], dtype=np.float64), kind="mergesort")[:top]
            c.dt = [dt[i] for i in order]
            c.gt = by_gt.get(key, [])
            c.score = np.array([d["score"] for d in c.dt], dtype=np.float64)
            c.dt_rng = np.array([d[rng_key] for d in c.dt], dtype=np.float64)
            c.gt_rng = np.array([g[rng_key] for g in c.gt], dtype=np.float64)
            c.gt_flag = np.array([bool(g.get(flag, 0)) for g in c.gt], dtype=bool)
            c.gt_crowd = np.array([bool(g["iscrowd"]) for g in c.gt], dtype=bool)
            c.dt_box = np.array([d["bbox"] for d in c.dt], dtype=np.float64).reshape(-1, 4)
            c.gt_box = np.array([g["bbox"] for g in c.gt], dtype=np.float64).reshape(-1, 4)
            c.prox = self._prox_applies(key[0])
            c.iou = c.in_prox = None
            self.cells[key] = c
        true_3d = self.mode == "3D" and not self.fork_compat_2d_iou
        if not with_iou:
            if true_3d and self.stage3d == "host":
                self._build_iou_3d()
            return
        for c in self.cells.values():
            if c.prox or not true_3d:
                iou2 = iou2d_xywh(c.dt_box, c.gt_box) if c.dt and c.gt else np.zeros((len(c.dt), len(c.gt)))
                if not true_3d:
                    c.iou = iou2
                if c.prox:
                    c.in_prox = (iou2 > self.params.proximity_thresh).any(axis=1)
        if true_3d:
            self._build_iou_3d()

    def _build_iou_3d(self):
        # true 3D IoU: one kernel call per IMAGE (all its detections x all its ground truth), sliced per category
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        per_image = defaultdict(list)
        for (img, cat), c in self.cells.items():
            if c.dt and c.gt:
                per_image[img].append(c)
            else:
                c.iou = np.zeros((len(c.dt), len(c.gt)))
        for img, cs in per_image.items():
            bd = torch.tensor(np.asarray([d["bbox3D"] for c in cs for d in c.dt], np.float32), device=dev)
            bg = torch.tensor(np.nan_to_num(np.asarray([g["bbox3D"] for c in cs for g in c.gt], np.float32), nan=0.0, posinf=0.0, neginf=0.0),
                              device=dev)
            full = np.nan_to_num(box3d_overlap(bd, bg).cpu().numpy().astype(np.float64))
            r = q = 0
            for c in cs:
                c.iou = full[r:r + len(c.dt), q:q + len(c.gt)]
                r, q = r + len(c.dt), q + len(c.gt)

    # ---- greedy matching of one cell for one range, all IoU thresholds at once ----------------------------------------------
    @staticmethod
    def _match(iou: np.ndarray, gt_ign: np.ndarray, gt_crowd: np.ndarray, thrs: np.ndarray):
        """``iou`` [D,G] with the ground truth already ordered not-ignored first. Per threshold, detections pick in score
        order the free ground truth of highest IoU >= threshold - a later one on equal IoU - among the not-ignored ones, and
        only when none qualifies among the ignored ones; crowd ground truth never fills up. Returns the picked index [T,D]
        (-1: none) and whether the pick is an ignored ground truth [T,D]."""
        T, (D, G) = len(thrs), iou.shape
        pick = -np.ones((T, D), dtype=np.int64)
        if D == 0 or G == 0:
            return pick, np.zeros((T, D), dtype=bool)
        floor = np.minimum(thrs, 1 - 1e-10)
        taken = np.zeros((T, G), dtype=bool)
        rows = np.arange(T)
        keep_open = gt_crowd[None, :]
        groups = (~gt_ign[None, :], gt_ign[None, :])
        for d in range(D):
            free = ~taken | keep_open
            chosen = -np.ones(T, dtype=np.int64)
            for grp in groups:
                v = np.where(free & grp, iou[d][None, :], -1.0)
                last_best = G - 1 - np.argmax(v[:, ::-1], axis=1)
                ok = (v[rows, last_best] >= floor) & (chosen < 0)
                chosen = np.where(ok, last_best, chosen)
            hit = chosen >= 0
            taken[rows[hit], chosen[hit]] = True
            pick[:, d] = chosen
        return pick, np.where(pick >= 0, gt_ign[np.clip(pick, 0, None)], False)

    def _evaluate_cell(self, c: _Cell, rng):
        lo, hi = rng
        gt_ign = c.gt_flag | (c.gt_rng < lo) | (c.gt_rng > hi)
        order = np.argsort(gt_ign, kind="mergesort")                           # not-ignored first, file order within
        pick, on_ignored = self._match(c.iou[:, order] if c.iou.size else c.iou.reshape(len(c.dt), len(c.gt)), gt_ign[order],
                                       c.gt_crowd[order], self.params.iouThrs)
        matched = pick >= 0
        outside = (c.dt_rng < lo) | (c.dt_rng > hi)
        ignored = on_ignored | (~matched & outside[None, :])
        if c.prox:                                                             # proximity evaluation: far detections, and every
            far = np.ones(len(c.dt), dtype=bool) if np.all(gt_ign) else ~c.in_prox     # detection of a cell without countable GT
            ignored = ignored | far[None, :]
        return {"score": c.score, "matched": matched, "ignored": ignored, "n_gt": int(np.count_nonzero(~gt_ign)), "gt_order": order,
                "pick": pick}

    def evaluate(self):
        self._build_cells(with_iou=self.matcher == "host")
        self._match_cells()
        if self.mode == "3D" and self.stage3d == "host":                        # stage3d="device": paired and scored in _match_device
            self._collect_nhd()

    def _match_cells(self):
        """Fills ``per_cell``: one entry per (cell, range) with the per-threshold picks and ignore flags."""
        if self.matcher == "device":
            self._match_device()
        else:
            self.per_cell = {(key, a): self._evaluate_cell(c, rng) for key, c in self.cells.items() for a, rng in enumerate(self.params.areaRng)}

    def _match_device(self):
        """Every cell packed CSR-style (vectorised, no loop per detection), one upload, the 2D IoU launch when the IoU or the
        proximity flags are needed, one matcher launch, one download; ``per_cell`` in the host's format. With ``stage3d="device"``
        the corners and cuboid records ride in the same upload, ``ovm_eval_iou3d`` fills the IoU buffer before the matcher and
        ``ovm_eval_nhd`` reads it after; the one download also brings the IoU blocks and ``nhd_pairs``."""
        if not torch.cuda.is_available():
            raise RuntimeError("matcher='device' needs a HIP device (no CPU fallback)")
        L = _lib.load()
        p = self.params
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        keys = list(self.cells)
        cs = [self.cells[k] for k in keys]
        n, A, T = len(cs), len(p.areaRng), len(p.iouThrs)
        true_3d = self.mode == "3D" and not self.fork_compat_2d_iou
        dev3d = self.stage3d == "device"
        nd = np.array([len(c.score) for c in cs], dtype=np.int64)
        ng = np.array([len(c.gt_rng) for c in cs], dtype=np.int64)
        cells = np.zeros(n, dtype=_CELL_DTYPE)
        assert cells.itemsize == C.sizeof(_lib.OvmEvalCell)
        dt_off, gt_off, iou_off = _exclusive_cumsum(nd), _exclusive_cumsum(ng), _exclusive_cumsum(nd * ng)
        n_dt, n_gtb, n_iou = int(nd.sum()), int(ng.sum()), int((nd * ng).sum())
        if max(n_dt, n_gtb) >= 2 ** 31 or n_dt * A * T >= 2 ** 62:
            raise RuntimeError("too many boxes for the device matcher")
        cells["iou_off"], cells["dt_off"], cells["n_dt"], cells["gt_off"], cells["n_gt"] = iou_off, dt_off, nd, gt_off, ng
        cells["prox"] = [c.prox for c in cs]
        any_prox = bool(cells["prox"].any())

        def cat(parts, dtype, shape=(-1,)):
            return np.concatenate([np.asarray(x, dtype=dtype).reshape(shape) for x in parts]) if parts else np.zeros(0, dtype)
        ins = [cells, np.repeat(np.arange(n, dtype=np.int32), nd), cat([c.dt_box for c in cs], np.float64, (-1, 4)),
               cat([c.gt_box for c in cs], np.float64, (-1, 4)), cat([c.dt_rng for c in cs], np.float64), cat([c.gt_rng for c in cs], np.float64),
               cat([c.gt_flag for c in cs], np.uint8), cat([c.gt_crowd for c in cs], np.uint8),
               np.asarray(p.areaRng, dtype=np.float64).reshape(-1), np.minimum(p.iouThrs, 1 - 1e-10).astype(np.float64)]
        if dev3d:
            ins += self._pack_3d(cs, n_dt, n_gtb)
        elif true_3d:
            ins.append(cat([c.iou for c in cs], np.float64))
        buf, io = _pack_segments(ins)
        # outputs: pick int32, ignored uint8, n_gt int32, in_prox uint8, and the IoU when it is computed here; with the 3D stages
        # on the device also pair_gt int32, the NHD status uint8 and nhd fp64 [n_dt][5]
        outs = [np.zeros(n_dt * A * T, np.int32), np.zeros(n_dt * A * T, np.uint8), np.zeros(n * A, np.int32), np.zeros(n_dt, np.uint8)]
        if not true_3d or dev3d:
            outs.append(np.zeros(n_iou, np.float64))
        if dev3d:
            outs += [np.zeros(n_dt, np.int32), np.zeros(n_dt, np.uint8), np.zeros(n_dt * 5, np.float64)]
        obytes, oo = _pack_segments(outs)
        d_in = torch.from_numpy(buf).to(dev)
        d_out = torch.empty(len(obytes), dtype=torch.uint8, device=dev)
        bi, bo = d_in.data_ptr(), d_out.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        iou_ptr = (bi + io[10]) if true_3d and not dev3d else (bo + oo[4])
        prox_ptr = (bo + oo[3]) if any_prox else None
        max_gt = int(ng.max()) if n else 0
        if dev3d:
            _lib.check(L.ovm_eval_iou3d(bi + io[0], bi + io[1], n_dt, bi + io[10], bi + io[11], 1e-4, 1e-8, iou_ptr, stream), what="ovm_eval_iou3d")
        if not true_3d or any_prox:
            _lib.check(L.ovm_eval_iou2d(bi + io[0], bi + io[1], n_dt, bi + io[2], bi + io[3], float(p.proximity_thresh),
                                        None if true_3d else iou_ptr, prox_ptr, stream), what="ovm_eval_iou2d")
        _lib.check(L.ovm_eval_match(bi + io[0], n, max_gt, iou_ptr, bi + io[4], bi + io[5], bi + io[6], bi + io[7], prox_ptr,
                                    bi + io[8], A, bi + io[9], T, bo + oo[0], bo + oo[1], bo + oo[2], stream), what="ovm_eval_match")
        if dev3d:
            _lib.check(L.ovm_eval_nhd(bi + io[0], bi + io[1], n_dt, max_gt, iou_ptr, float(self.nhd_iou_threshold), bi + io[12], bi + io[13],
                                      bi + io[14], bi + io[15], bo + oo[5], bo + oo[7], bo + oo[6], stream), what="ovm_eval_nhd")
        host = d_out.cpu().numpy()
        pick = host[oo[0]:oo[0] + outs[0].nbytes].view(np.int32).astype(np.int64)
        ignored = host[oo[1]:oo[1] + outs[1].nbytes].view(np.bool_)
        matched = pick >= 0
        n_gt = host[oo[2]:oo[2] + outs[2].nbytes].view(np.int32).reshape(n, A)
        if not true_3d or dev3d:
            iou = host[oo[4]:oo[4] + outs[4].nbytes].view(np.float64)
            for i, c in enumerate(cs):
                c.iou = iou[iou_off[i]:iou_off[i] + nd[i] * ng[i]].reshape(nd[i], ng[i])
        if any_prox:
            in_prox = host[oo[3]:oo[3] + outs[3].nbytes].view(np.bool_)
            for i, c in enumerate(cs):
                if c.prox:
                    c.in_prox = in_prox[dt_off[i]:dt_off[i] + nd[i]]
        # the ordered ground truth of every (cell, range): not ignored first, file order within
        gt_cell = np.repeat(np.arange(n), ng)
        gt_local = np.arange(n_gtb) - np.repeat(gt_off, ng)
        flag, rng = ins[6].astype(bool), ins[5]
        orders = []
        for lo, hi in p.areaRng:
            ign = flag | (rng < lo) | (rng > hi)
            orders.append(gt_local[np.lexsort((ign, gt_cell))])
        self.per_cell = {}
        for i, (key, c) in enumerate(zip(keys, cs)):
            b, e = dt_off[i] * A * T, (dt_off[i] + nd[i]) * A * T
            pk, mt, ig = pick[b:e].reshape(A, T, nd[i]), matched[b:e].reshape(A, T, nd[i]), ignored[b:e].reshape(A, T, nd[i])
            g0, g1 = gt_off[i], gt_off[i] + ng[i]
            for a in range(A):
                self.per_cell[key, a] = {"score": c.score, "matched": mt[a], "ignored": ig[a], "n_gt": int(n_gt[i, a]), "gt_order": orders[a][g0:g1],
                                         "pick": pk[a]}
        if dev3d:
            status = host[oo[6]:oo[6] + outs[6].nbytes]
            pair_gt = host[oo[5]:oo[5] + outs[5].nbytes].view(np.int32)
            nhd = host[oo[7]:oo[7] + outs[7].nbytes].view(np.float64).reshape(n_dt, 5)
            # the host's order: cells by (category, image) as strings, detections ascending
            order = sorted(range(n), key=lambda i: (str(keys[i][1]), str(keys[i][0])))
            rows = np.concatenate([np.arange(dt_off[i], dt_off[i] + nd[i]) for i in order]) if n else np.zeros(0, np.int64)
            rows = rows[status[rows] == _lib.OVM_NHD_OK]
            names = ("overall",) + _nhd.COMPONENTS
            self.nhd_pairs = [dict(zip(names, v)) for v in nhd[rows].tolist()]
            cell_of = ins[1]
            self.nhd_pair_ids = [(cs[i].dt[r - dt_off[i]]["id"], cs[i].gt[g]["id"])
                                 for r, i, g in zip(rows.tolist(), cell_of[rows].tolist(), pair_gt[rows].tolist())]

    def _pack_3d(self, cs, n_dt, n_gtb):
        """The 3D stages' inputs in detection / ground-truth row order: corners fp32 [.,8,3] (ground truth through nan_to_num, as
        ``_build_iou_3d``), "carries its NHD fields" uint8, cuboid records fp32 [.,15] = xy, z (the record's depth), dimensions,
        rotation - rounded to fp32 where ``nhd.cuboid_corners`` rounds them."""
        def corners(recs, count):
            a = np.asarray([r["bbox3D"] for r in recs], np.float32).reshape(-1, 8, 3) if recs else np.zeros((0, 8, 3), np.float32)
            assert a.shape[0] == count
            return a

        def cuboids(recs, rot, need):
            ok, out = np.zeros(len(recs), np.uint8), np.zeros((len(recs), 15), np.float32)
            for i, r in enumerate(recs):
                if any(f not in r for f in need):
                    continue
                try:                                                            # a malformed field raises in nhd.cuboid_corners too: no pair
                    out[i, 0:2] = r["center_cam"][:2]
                    out[i, 2] = r["depth"]
                    out[i, 3:6] = r["dimensions"]
                    out[i, 6:15] = np.asarray(r[rot], dtype=np.float32).reshape(9)
                    ok[i] = 1
                except Exception:
                    out[i] = 0
            return ok, out
        dts, gts = [d for c in cs for d in c.dt], [g for c in cs for g in c.gt]
        dt_ok, dt_cub = cuboids(dts, "pose", ("center_cam", "dimensions", "pose", "depth"))
        gt_ok, gt_cub = cuboids(gts, "R_cam", ("center_cam", "dimensions", "R_cam", "depth"))
        return [corners(dts, n_dt), np.nan_to_num(corners(gts, n_gtb), nan=0.0, posinf=0.0, neginf=0.0), dt_ok, gt_ok, dt_cub, gt_cub]

    # ---- precision / recall tables ----------------------------------------------------------------------------------------
    def accumulate(self):
        """precision[T,R,K,A,M], recall[T,K,A,M], scores[T,R,K,A,M] with -1 where a (category, range) has no countable ground
        truth - the layout of COCOeval.accumulate (reference :1547-1688), which the per-category tables read."""
        p = self.params
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        cells_of_cat = defaultdict(list)
        for (img, cat) in self.cells:
            cells_of_cat[cat].append(img)
        img_rank = {img: i for i, img in enumerate(p.imgIds)}
        tiny = np.spacing(1)
        for k, cat in enumerate(p.catIds):
            imgs = sorted(cells_of_cat.get(cat, ()), key=img_rank.__getitem__)     # concatenation order decides ties between images
            if not imgs:
                continue
            for a in range(A):
                res = [self.per_cell[(img, cat), a] for img in imgs]
                n_gt = sum(r["n_gt"] for r in res)
                if n_gt == 0:
                    continue
                for m, cap in enumerate(p.maxDets):
                    sc = np.concatenate([r["score"][:cap] for r in res])
                    order = np.argsort(-sc, kind="mergesort")
                    sc = sc[order]
                    hit = np.concatenate([r["matched"][:, :cap] for r in res], axis=1)[:, order]
                    ign = np.concatenate([r["ignored"][:, :cap] for r in res], axis=1)[:, order]
                    tp = np.cumsum(hit & ~ign, axis=1, dtype=np.float64)
                    fp = np.cumsum(~hit & ~ign, axis=1, dtype=np.float64)
                    nd = sc.shape[0]
                    recall[:, k, a, m] = tp[:, -1] / n_gt if nd else 0.0
                    prec_tab, score_tab = np.zeros((T, R)), np.zeros((T, R))
                    if nd:
                        rc = tp / n_gt
                        pr = tp / (fp + tp + tiny)
                        envelope = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]      # best precision at this recall or beyond
                        for t in range(T):
                            at = np.searchsorted(rc[t], p.recThrs, side="left")
                            reach = at < nd
                            prec_tab[t, reach] = envelope[t, at[reach]]
                            score_tab[t, reach] = sc[at[reach]]
                    precision[:, :, k, a, m] = prec_tab
                    scores[:, :, k, a, m] = score_tab
        self.eval = {"params": p, "counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}
        if self.mode == "3D":
            acc = {key: [pair[key] for pair in self.nhd_pairs] for key in ("overall",) + _nhd.COMPONENTS}
            self.eval["nhd_accumulators"] = acc
            self.eval["average_nhd"] = {key: (float(np.mean(v)) if v else float("nan")) for key, v in acc.items()}

    # ---- disentangled NHD over IoU-matched pairs (reference :2342-2484) -----------------------------------------------------
    def _collect_nhd(self):
        """A detection is paired with its highest-IoU ground truth of the cell (the first one on ties, IoU > 0) when that IoU
        reaches ``nhd_iou_threshold``. The reference evaluates the same pairs once per depth range and averages over all of
        them, which leaves the mean where it is; here each pair is scored once. (Its IoU lookup reads the matrix in
        un-reordered ground-truth order while walking the reordered list, :2363-2392; the pairing here follows the intent.)"""
        need_dt, need_gt = ("center_cam", "dimensions", "pose", "depth"), ("center_cam", "dimensions", "R_cam", "depth")
        self.nhd_pairs, self.nhd_pair_ids = [], []
        for key in sorted(self.cells, key=lambda k: (str(k[1]), str(k[0]))):
            c = self.cells[key]
            if not c.dt or not c.gt or c.iou.size == 0:
                continue
            best = np.argmax(c.iou, axis=1)
            for di, gi in enumerate(best):
                v = c.iou[di, gi]
                d, g = c.dt[di], c.gt[gi]
                if not (v > 0 and v >= self.nhd_iou_threshold) or any(f not in d for f in need_dt) or any(f not in g for f in need_gt):
                    continue
                pred = {"xy": d["center_cam"][:2], "z": d["depth"], "dimensions": d["dimensions"], "pose": d["pose"]}
                true = {"xy": g["center_cam"][:2], "z": g["depth"], "dimensions": g["dimensions"], "pose": g["R_cam"]}
                try:
                    self.nhd_pairs.append(_nhd.disentangled_nhd(pred, true))
                    self.nhd_pair_ids.append((d["id"], g["id"]))
                except Exception:                                               # a degenerate box: the reference logs and moves on (:2424-2426)
                    continue

    # ---- summarize (reference :2072-2224) ----------------------------------------------------------------------------------
    def _summarize(self, ap=1, iouThr=None, areaRng="all", maxDets=100):
        p = self.params
        aind = [i for i, lbl in enumerate(p.areaRngLbl) if lbl == areaRng]
        mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
        s = self.eval["precision"] if ap == 1 else self.eval["recall"]
        if iouThr is not None:
            t = np.where(np.isclose(iouThr, p.iouThrs.astype(float)))[0]
            s = s[t]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    def summarize(self) -> Dict[str, float]:
        if self.mode == "2D":
            keys = [("AP", None, "all"), ("AP50", 0.5, "all"), ("AP75", 0.75, "all"), ("AP95", 0.95, "all"), ("APs", None, "small"),
                    ("APm", None, "medium"), ("APl", None, "large")]
        else:
            keys = [("AP", None, "all"), ("AP15", 0.15, "all"), ("AP25", 0.25, "all"), ("AP50", 0.50, "all"), ("APn", None, "near"),
                    ("APm", None, "medium"), ("APf", None, "far")]
        out = {k: self._summarize(1, thr, rng) * 100 for k, thr, rng in keys}
        for md in (1, 10, 100):                                                 # the reference's AR1 / AR10 / AR100 (:2190-2224)
            out[f"AR{md}"] = self._summarize(0, None, "all", md) * 100
        if self.mode == "3D" and "average_nhd" in self.eval:
            for comp, v in self.eval["average_nhd"].items():
                out["NHD" if comp == "overall" else f"NHD-{comp}"] = v
        self.stats = out
        return out

    def per_category_ap(self, class_names=None) -> Dict:
        """mean precision per category at area 'all', maxDets 100 (reference _derive_omni_results :1729-1819). ``class_names``:
        a dict id -> name, or a sequence indexed by the id."""
        prec = self.eval["precision"]
        out = {}
        for k, cid in enumerate(self.params.catIds):
            s = prec[:, :, k, 0, -1]
            s = s[s > -1]
            if isinstance(class_names, dict):
                name = class_names.get(cid, cid)
            else:
                name = class_names[cid] if class_names is not None and cid < len(class_names) else cid
            out[name] = float(np.mean(s) * 100) if s.size else float("nan")
        return out

    def per_category_ar(self, class_names=None) -> Dict:
        """mean recall per category over the IoU thresholds at area 'all', maxDets 100 (the AR-<category> entries of the
        reference's _derive_omni_results)."""
        rec = self.eval["recall"]
        out = {}
        for k, cid in enumerate(self.params.catIds):
            s = rec[:, k, 0, -1]
            s = s[s > -1]
            if isinstance(class_names, dict):
                name = class_names.get(cid, cid)
            else:
                name = class_names[cid] if class_names is not None and cid < len(class_names) else cid
            out[name] = float(np.mean(s) * 100) if s.size else float("nan")
        return out


def evaluate_omni3d(gts, dts: Sequence[Dict], device=None, only_2d: bool = False, fork_compat_2d_iou: bool = False,
                    category_map=None, passthrough_dataset_ids: bool = False, eval_prox=False, matcher: str = "host",
                    stage3d: str = "host") -> Dict:
    """AP2D and AP3D dictionaries for one dataset (reference _evaluate_predictions_on_omni :1255-1391 without the file plumbing).
    ``eval_prox`` (a bool, or the image ids whose cells it applies to) and ``matcher``: as ``Omni3Deval``; so is ``stage3d``, which
    applies to the 3D pass.

    ``gts``: an ``Omni3DGroundTruth`` (images and categories evaluated = the dataset's, as the reference; detections on unknown
    images or categories are dropped :1319-1334) or a plain list of ground-truth dicts. ``category_map`` (``CategoryMap``): the
    detections carry the model's contiguous class index and are un-mapped to dataset ids first (:1029-1093)."""
    from .omni3d_gt import Omni3DGroundTruth, ground_truth_records
    img_ids = cat_ids = names = None
    if isinstance(gts, Omni3DGroundTruth):
        img_ids, cat_ids = list(gts.image_ids), list(gts.category_ids)
        names = dict(zip(gts.category_ids, gts.category_names))
        gts = ground_truth_records(gts)
    if category_map is not None:
        dts = category_map.detections_to_dataset_ids(dts, passthrough_dataset_ids)
    if img_ids is not None:
        known_i, known_c = set(img_ids), set(cat_ids)
        dts = [d for d in dts if d["image_id"] in known_i and d["category_id"] in known_c]
    res = {}
    e2 = Omni3Deval(gts, dts, "2D", device=device, img_ids=img_ids, cat_ids=cat_ids, eval_prox=eval_prox, matcher=matcher)
    e2.evaluate(); e2.accumulate()
    res["bbox_2D"] = e2.summarize()
    if names is not None:
        res["bbox_2D_per_category"] = e2.per_category_ap(names)
        res["bbox_2D_per_category_AR"] = e2.per_category_ar(names)
    if not only_2d:
        d3 = [d for d in dts if "bbox3D" in d]
        e3 = Omni3Deval(gts, d3, "3D", device=device, fork_compat_2d_iou=fork_compat_2d_iou, img_ids=img_ids, cat_ids=cat_ids,
                        eval_prox=eval_prox, matcher=matcher, stage3d=stage3d)
        e3.evaluate(); e3.accumulate()
        res["bbox_3D"] = e3.summarize()
        if names is not None:
            res["bbox_3D_per_category"] = e3.per_category_ap(names)
            res["bbox_3D_per_category_AR"] = e3.per_category_ar(names)
    return res


def omni3d_json_to_gt(dataset_json: Dict, filter_settings: Optional[Dict] = None) -> List[Dict]:
    """Ground-truth records of an Omni3D annotation dict under the reference's filter settings (defaults: datasets.py:55-66);
    see ``omni3d_gt.Omni3DGroundTruth`` for the rules."""
    from .omni3d_gt import Omni3DGroundTruth, filter_settings_from_cfg, ground_truth_records
    return ground_truth_records(Omni3DGroundTruth(dataset_json, filter_settings if filter_settings is not None else filter_settings_from_cfg(None)))


# Omni3D's indoor / outdoor category groups (cubercnn/data/builtin.py:15-20: facts of the benchmark)
OMNI3D_OUT = frozenset("pedestrian car cyclist van truck bus trailer motorcycle bicycle barrier".split() + ["traffic cone"])
OMNI3D_IN = frozenset(["chair", "table", "cabinet", "lamp", "books", "sofa", "picture", "window", "pillow", "door", "blinds", "sink", "shelves",
                       "television", "shoes", "cup", "bottle", "bookcase", "laptop", "desk", "floor mat", "mirror", "counter", "bicycle", "toilet", "bed",
                       "refrigerator", "box", "oven", "clothes", "towel", "night stand", "stove", "machine", "stationery", "bathtub", "curtain", "bin"])
OMNI3D_ALL = OMNI3D_OUT | OMNI3D_IN | frozenset(["camera", "cereal box"])      # the benchmark's 50 categories (builtin.py:12-14)
# the novel split's 22 categories and its easy ones (reference summarize_all :602-603)
OMNI3D_NOVEL = frozenset(["monitor", "bag", "dresser", "board", "printer", "keyboard", "painting", "drawers", "microwave", "computer", "kitchen pan",
                          "potted plant", "tissues", "rack", "tray", "toys", "phone", "podium", "cart", "soundsystem", "fireplace", "tram"])
OMNI3D_NOVEL_EASY = frozenset(["board", "printer", "painting", "microwave", "tray", "podium", "cart", "tram"])


def collective_summary(results: Dict) -> Dict:
    """The cross-dataset numbers of the reference's ``Omni3DEvaluationHelper.summarize_all`` (:427-620) from ONE ``evaluate_omni3d`` result
    over the concatenation of the datasets (re-accumulating the cached per-image results of every dataset, as the reference does, is the
    same computation: a cell's matching depends on its own image and category only). ``<Concat>`` averages the per-category AP / AR
    over the categories that have ground truth; ``Omni3D_Out`` / ``Omni3D_In`` / ``Omni3D`` over the benchmark's outdoor / indoor / all 50
    categories, NaN unless every one of them was evaluated. When the categories with any result (AP2D, AP3D, AR2D or AR3D not NaN,
    :598) are exactly the novel split's 22, ``Novel_Easy`` / ``Novel_Hard`` hold the plain means over its 8 easy and 14 hard ones
    (``calculate_metrics`` :171-191, a NaN propagates; :601-613)."""
    def mean_over(table, cats):
        vals = [table[c] for c in cats]
        return float(np.mean(vals)) if vals and not any(np.isnan(v) for v in vals) else float("nan")
    ap2, ar2 = results["bbox_2D_per_category"], results["bbox_2D_per_category_AR"]
    ap3, ar3 = results.get("bbox_3D_per_category"), results.get("bbox_3D_per_category_AR")
    have = {c for c, v in ap2.items() if not np.isnan(v)}
    out = {"<Concat>": {"AP2D": mean_over(ap2, sorted(have)), "AR2D": mean_over(ar2, sorted(have)),
                        "AP3D": mean_over(ap3, sorted(have)) if ap3 else float("nan"), "AR3D": mean_over(ar3, sorted(have)) if ar3 else float("nan")}}
    if "bbox_3D" in results:
        out["<Concat>"].update({"AP3D@15": results["bbox_3D"]["AP15"], "AP3D@25": results["bbox_3D"]["AP25"], "AP3D@50": results["bbox_3D"]["AP50"],
                                "AP3D-N": results["bbox_3D"]["APn"], "AP3D-M": results["bbox_3D"]["APm"], "AP3D-F": results["bbox_3D"]["APf"]})
        for k in ("NHD", "NHD-xy", "NHD-z", "NHD-dimensions", "NHD-pose"):
            if k in results["bbox_3D"]:
                out["<Concat>"][k] = results["bbox_3D"][k]
    for label, group in (("Omni3D_Out", OMNI3D_OUT), ("Omni3D_In", OMNI3D_IN), ("Omni3D", OMNI3D_ALL)):
        full = group <= have
        out[label] = {"AP2D": mean_over(ap2, sorted(group)) if full else float("nan"), "AR2D": mean_over(ar2, sorted(group)) if full else float("nan"),
                      "AP3D": mean_over(ap3, sorted(group)) if full and ap3 else float("nan"),
                      "AR3D": mean_over(ar3, sorted(group)) if full and ar3 else float("nan")}
    nan = float("nan")
    results_cat = {c: {"AP2D": ap2[c], "AP3D": (ap3 or {}).get(c, nan), "AR2D": ar2.get(c, nan), "AR3D": (ar3 or {}).get(c, nan)} for c in ap2}
    results_cat = {c: m for c, m in results_cat.items() if not all(np.isnan(v) for v in m.values())}
    if set(results_cat) == OMNI3D_NOVEL:
        for label, group in (("Novel_Easy", OMNI3D_NOVEL_EASY), ("Novel_Hard", OMNI3D_NOVEL - OMNI3D_NOVEL_EASY)):
            out[label] = {k: sum(results_cat[c][k] for c in sorted(group)) / len(group) for k in ("AP2D", "AP3D", "AR2D", "AR3D")}
    return out
