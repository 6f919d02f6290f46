"""Omni3D novel-split evaluation: upstream Omni3D's proximity rule (eval_prox), the easy / hard novel categories of the collective
summary, and the entry point's flags. The device matcher is held against the host one in tests/test_gpu_eval_match.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import box3d as ob


def _ann(img, cat, box, depth=5.0, score=None, **kw):
    x, y, w, h = box
    c3 = ob.make_box([x + w / 2, y + h / 2, depth], [w, h, 1.0], np.eye(3)).tolist()
    d = {"image_id": img, "category_id": cat, "bbox": [float(v) for v in box], "bbox3D": c3, "depth": depth, **kw}
    if score is not None:
        d["score"] = score
    return d


def _ap_with_proximity_by_definition(gts, dts, mode, img_ids, cat_ids, prox_imgs):
    """COCOeval.evaluateImg written out with pycocotools' scalar loops, plus upstream Omni3D's proximity rules for the images in
    ``prox_imgs`` (a detection with no 2D IoU above 0.3 with any ground truth of its cell is ignored; every detection of a cell whose
    ground truth is all ignored in the range is ignored), then the 101-point AP from its definition. The IoU is the 2D one (2D
    mode, and 3D mode with the fork's 2D IoU)."""
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3DParams, iou2d_xywh
    p = Omni3DParams(mode)
    flag, key = ("ignore2D", "area") if mode == "2D" else ("ignore3D", "depth")
    T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(cat_ids), len(p.areaRng), len(p.maxDets)
    prec, rec = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a, (lo, hi) in enumerate(p.areaRng):
            per_img = []                                                        # evaluateImg of each image: (scores, dtm [T][D], dtIg [T][D], npig)
            for img in img_ids:
                G = [g for g in gts if g["image_id"] == img and g["category_id"] == cat]
                D = [d for d in dts if d["image_id"] == img and d["category_id"] == cat]
                if not G and not D:
                    continue
                g_ig = [1 if (g.get(flag, 0) or g[key] < lo or g[key] > hi) else 0 for g in G]
                gtind = sorted(range(len(G)), key=lambda i: g_ig[i])            # stable: not-ignored first
                dtind = sorted(range(len(D)), key=lambda i: -D[i]["score"])[:p.maxDets[-1]]
                iou_file = iou2d_xywh(np.array([D[i]["bbox"] for i in dtind]).reshape(-1, 4), np.array([g["bbox"] for g in G]).reshape(-1, 4))
                gtIg = [g_ig[i] for i in gtind]
                crowd = [bool(G[i].get("iscrowd", 0)) for i in gtind]
                dtm, dtIg = np.zeros((T, len(dtind)), bool), np.zeros((T, len(dtind)), bool)
                for t, thr in enumerate(p.iouThrs):
                    gtm = [0] * len(gtind)
                    for dind in range(len(dtind)):
                        iou, m = min(thr, 1 - 1e-10), -1
                        for gind in range(len(gtind)):
                            if gtm[gind] > 0 and not crowd[gind]:
                                continue
                            if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                                break
                            if iou_file[dind, gtind[gind]] < iou:
                                continue
                            iou, m = iou_file[dind, gtind[gind]], gind
                        if m == -1:
                            continue
                        dtIg[t, dind], dtm[t, dind], gtm[m] = gtIg[m], True, 1
                    for dind, i in enumerate(dtind):
                        out = D[i][key] < lo or D[i][key] > hi
                        if not dtm[t, dind] and out:
                            dtIg[t, dind] = True
                        if img in prox_imgs:
                            in_prox = any(iou_file[dind, gi] > p.proximity_thresh for gi in range(len(G)))
                            if all(gtIg) or not in_prox:                      # all([]) is True: a cell without ground truth
                                dtIg[t, dind] = True
                per_img.append(([D[i]["score"] for i in dtind], dtm, dtIg, sum(1 for v in gtIg if v == 0)))
            n_pos = sum(r[3] for r in per_img)
            if n_pos == 0:
                continue
            for m, cap in enumerate(p.maxDets):
                for t in range(T):
                    rows = [(s[j], dm[t, j], di[t, j]) for s, dm, di, _ in per_img for j in range(min(cap, len(s)))]
                    order = sorted(range(len(rows)), key=lambda i: -rows[i][0])
                    tp = fp = 0
                    curve = []
                    for i in order:
                        _, hit, ign = rows[i]
                        tp += int(hit and not ign)
                        fp += int(not hit and not ign)
                        curve.append((tp / n_pos, tp / (tp + fp + np.spacing(1))))
                    rec[t, k, a, m] = curve[-1][0] if curve else 0.0
                    for r, level in enumerate(p.recThrs):
                        beyond = [pr for rc, pr in curve if rc >= level]
                        prec[t, r, k, a, m] = max(beyond) if beyond else 0.0
    return prec, rec


def _random_scene(seed, n_img=6, far=True):
    """Crowded random scenes: ties in score and IoU, ignored and out-of-range ground truth, cells without ground truth, a cell with
    130 detections, and detections far from every ground truth box."""
    g = np.random.default_rng(seed)
    gts, dts = [], []
    grid = [10, 40, 70, 100] + ([400, 600] if far else [])
    for img in range(1, n_img + 1):
        for cat in range(3):
            if g.random() < 0.15:
                continue
            n_gt = 0 if g.random() < 0.15 else int(g.integers(1, 6))
            mine = []
            for _ in range(n_gt):
                x, y = g.choice(grid[:4]), g.choice(grid[:4])
                w, h = g.choice([20, 30, 110]), g.choice([20, 30, 110])
                mine.append([x, y, w, h])
                gts.append(_ann(img, cat, [x, y, w, h], depth=float(g.choice([5.0, 10.0, 20.0, 35.0, 60.0])),
                                ignore2D=int(g.random() < 0.2), ignore3D=int(g.random() < 0.2)))
            nd = int(g.integers(0, 9)) if (img, cat) != (2, 1) else 130
            for _ in range(nd):
                if mine and g.random() < 0.5:                                   # near a ground truth box: a few pixels off
                    x, y, w, h = mine[int(g.integers(0, len(mine)))]
                    x, y = x + g.choice([0, 0, 4, -6, 12]), y + g.choice([0, 3, -9])
                else:
                    x, y = g.choice(grid), g.choice(grid)
                    w, h = g.choice([20, 30, 110]), g.choice([20, 30, 110])
                dts.append(_ann(img, cat, [x, y, w, h], depth=float(g.choice([5.0, 10.0, 20.0, 35.0, 60.0])),
                                score=float(g.choice([0.9, 0.8, 0.8, 0.5, 0.3, 0.3, 0.1]) if nd < 100 else g.random())))
    return gts, dts


@pytest.mark.parametrize("mode,seed", [("2D", 21), ("2D", 22), ("3D", 23), ("3D", 24)])
def test_proximity_evaluator_equals_the_scalar_definition(mode, seed):
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    gts, dts = _random_scene(seed)
    img_ids, cat_ids = list(range(1, 8)), [0, 1, 2, 3]                          # image 7 and category 3 exist but are empty
    tabs = {}
    for prox in (False, True):
        e = Omni3Deval(gts, dts, mode, fork_compat_2d_iou=True, img_ids=img_ids, cat_ids=cat_ids, eval_prox=prox)
        e.evaluate(); e.accumulate()
        prec, rec = _ap_with_proximity_by_definition(e._gts_all, e._dts_all, mode, img_ids, cat_ids, set(img_ids) if prox else set())
        assert (prec > 0).sum() > 500 and ((prec > 0) & (prec < 1)).sum() > 200
        assert np.array_equal(e.eval["precision"], prec)
        assert np.array_equal(e.eval["recall"], rec)
        tabs[prox] = e.eval["precision"]
    assert not np.array_equal(tabs[False], tabs[True])                       # the rule does change this sample's tables
    # the image-id form applies the rule to the cells of those images only
    e = Omni3Deval(gts, dts, mode, fork_compat_2d_iou=True, img_ids=img_ids, cat_ids=cat_ids, eval_prox={2, 4, 5})
    e.evaluate(); e.accumulate()
    prec, rec = _ap_with_proximity_by_definition(e._gts_all, e._dts_all, mode, img_ids, cat_ids, {2, 4, 5})
    assert np.array_equal(e.eval["precision"], prec) and np.array_equal(e.eval["recall"], rec)


def _ap(gts, dts, mode="2D", **kw):
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    e = Omni3Deval(gts, dts, mode, fork_compat_2d_iou=mode == "3D", **kw)
    e.evaluate(); e.accumulate()
    return e.summarize()["AP"]


def test_proximity_known_values():
    half = 100.0 * 0.5 * 51 / 101                                               # precision 1/2 over recall points 0 .. 0.50
    A = [0.0, 0.0, 10.0, 10.0]
    # a far unmatched detection ranked first stops counting as a false positive
    gts, dts = [_ann(1, 0, A)], [_ann(1, 0, [300, 300, 10, 10], score=0.9), _ann(1, 0, A, score=0.8)]
    assert abs(_ap(gts, dts) - 50.0) < 1e-9 and abs(_ap(gts, dts, eval_prox=True) - 100.0) < 1e-9
    # a detection in a cell without ground truth (image 2) is ignored
    gts, dts = [_ann(1, 0, A)], [_ann(2, 0, A, score=0.9), _ann(1, 0, A, score=0.8)]
    assert abs(_ap(gts, dts) - 50.0) < 1e-9 and abs(_ap(gts, dts, eval_prox=True) - 100.0) < 1e-9
    assert abs(_ap(gts, dts, eval_prox={2}) - 100.0) < 1e-9 and abs(_ap(gts, dts, eval_prox={1}) - 50.0) < 1e-9
    # a cell whose ground truth is all ignored: its detection (2D IoU 0.4 - in proximity, unmatched) is ignored
    near = [0.0, 0.0, 10.0, 4.0]
    gts, dts = [_ann(1, 0, A), _ann(2, 0, A, ignore2D=1)], [_ann(2, 0, near, score=0.9), _ann(1, 0, A, score=0.8)]
    assert abs(_ap(gts, dts) - 50.0) < 1e-9 and abs(_ap(gts, dts, eval_prox=True) - 100.0) < 1e-9
    gts[1]["ignore2D"] = 0                                                      # the same box counted: the detection stays a false positive
    assert abs(_ap(gts, dts, eval_prox=True) - half) < 1e-9
    # IoU exactly 0.3 is not in proximity (strictly greater), 0.31 is
    gts = [_ann(1, 0, A)]
    at = [_ann(1, 0, [0.0, 0.0, 10.0, 3.0], score=0.9), _ann(1, 0, A, score=0.8)]
    above = [_ann(1, 0, [0.0, 0.0, 10.0, 3.1], score=0.9), _ann(1, 0, A, score=0.8)]
    assert abs(_ap(gts, at, eval_prox=True) - 100.0) < 1e-9 and abs(_ap(gts, above, eval_prox=True) - 50.0) < 1e-9
    # 3D mode: a detection matched at 3D thresholds 0.05 .. 0.25 (IoU 0.25) lies outside the 2D proximity and is ignored anyway
    gts = [_ann(1, 0, A), _ann(2, 0, A)]
    dts = [_ann(1, 0, [0.0, 0.0, 10.0, 2.5], score=0.9), _ann(2, 0, A, score=0.8)]
    assert abs(_ap(gts, dts, "3D") - (5 * 100.0 + 5 * half) / 10) < 1e-9
    assert abs(_ap(gts, dts, "3D", eval_prox=True) - 100.0 * 51 / 101) < 1e-9


def _omni_anno(i, img, cat_id, cat_name, proj, **kw):
    x1, y1, x2, y2 = proj
    c = [0.1 * i, 0.0, 5.0 + i]
    a = {"id": i, "image_id": img, "category_id": cat_id, "category_name": cat_name, "behind_camera": False, "valid3D": True,
         "dimensions": [1.0, 2.0, 3.0], "center_cam": c, "lidar_pts": -1, "segmentation_pts": -1, "depth_error": -1,
         "truncation": 0.0, "visibility": 1.0, "bbox2D_proj": [x1, y1, x2, y2], "bbox2D_tight": [-1, -1, -1, -1],
         "bbox2D_trunc": [x1, y1, x2, y2], "R_cam": np.eye(3).tolist(), "bbox3D_cam": ob.make_box(c, [3.0, 2.0, 1.0], np.eye(3)).tolist()}
    a.update(kw)
    return a


def two_datasets(seed):
    """Two Omni3D annotation dicts (images 1, 2 and 11, 12; categories chair / table) with random boxes, the ground truth over both,
    the detections (dataset ids) and the image ids of the first dataset."""
    from ovmono3d_amd.evaluation import Omni3DGroundTruth, filter_settings_from_cfg
    g = np.random.default_rng(seed)
    cats = [{"id": 18, "name": "chair"}, {"id": 22, "name": "table"}]
    files, dts, i = [], [], 0
    for base in (0, 10):
        annos = []
        for img in (base + 1, base + 2):
            for cid, name in ((18, "chair"), (22, "table")):
                mine = []
                for _ in range(int(g.integers(0, 5))):
                    i += 1
                    x, y = float(g.choice([10, 60, 120])), float(g.choice([10, 60, 120]))
                    w, h = float(g.choice([40, 80])), float(g.choice([40, 80]))
                    mine.append([x, y, w, h])
                    annos.append(_omni_anno(i, img, cid, name, [x, y, x + w, y + h], visibility=float(g.choice([1.0, 1.0, 0.0]))))
                for _ in range(int(g.integers(0, 8))):
                    if mine and g.random() < 0.5:
                        x, y, w, h = mine[int(g.integers(0, len(mine)))]
                        x += float(g.choice([0, 5, -12]))
                    else:
                        x, y = float(g.choice([10, 60, 120, 400])), float(g.choice([10, 60, 120, 400]))
                        w, h = float(g.choice([40, 80])), float(g.choice([40, 80]))
                    dts.append({"image_id": img, "category_id": cid, "bbox": [x, y, w, h], "score": float(g.choice([0.9, 0.7, 0.5, 0.2])),
                                "bbox3D": ob.make_box([x / 50, y / 50, 6.0], [3.0, 2.0, 1.0], np.eye(3)).tolist(), "depth": 6.0})
        files.append({"info": {"name": f"toy{base}"}, "images": [{"id": base + 1, "height": 480, "width": 640}, {"id": base + 2, "height": 480, "width": 640}],
                      "categories": cats, "annotations": annos})
    fs = filter_settings_from_cfg(None)
    fs.update(category_names=["chair", "table"], trunc_2D_boxes=True)
    return files, fs, Omni3DGroundTruth(files, fs), dts, {1, 2}


@pytest.mark.parametrize("mode", ["2D", "3D"])
def test_proximity_by_image_ids_equals_per_dataset_evaluation(mode):
    """The collective pass evaluates the union of the datasets at once with the rule on the images of the proximity datasets: every
    cell comes out as in the evaluation of its own dataset."""
    from ovmono3d_amd.evaluation import Omni3DGroundTruth, Omni3Deval, evaluate_omni3d, ground_truth_records
    files, fs, gt, dts, prox_imgs = two_datasets(3)
    recs = ground_truth_records(gt)
    both = Omni3Deval(recs, dts, mode, fork_compat_2d_iou=True, img_ids=gt.image_ids, cat_ids=gt.category_ids, eval_prox=prox_imgs)
    both.evaluate()
    n_ignored_far = 0
    for f, prox in zip(files, (True, False)):
        one = Omni3DGroundTruth(f, dict(fs))
        mine = [d for d in dts if d["image_id"] in set(one.image_ids)]
        e = Omni3Deval(ground_truth_records(one), mine, mode, fork_compat_2d_iou=True, img_ids=one.image_ids, cat_ids=one.category_ids,
                       eval_prox=prox)
        e.evaluate()
        assert e.per_cell and set(e.per_cell) <= set(both.per_cell)
        for key, r in e.per_cell.items():
            s = both.per_cell[key]
            for field in ("score", "matched", "ignored", "pick", "gt_order"):
                assert np.array_equal(r[field], s[field]), (key, field)
            assert r["n_gt"] == s["n_gt"]
            if prox:
                n_ignored_far += int((r["ignored"] & ~r["matched"]).sum())
    assert n_ignored_far > 0
    r = evaluate_omni3d(gt, dts, only_2d=True, eval_prox=prox_imgs)
    assert set(r) >= {"bbox_2D", "bbox_2D_per_category"}


def _novel_results(ap2, ap3=None, ar2=None, ar3=None):
    return {"bbox_2D_per_category": dict(ap2), "bbox_2D_per_category_AR": dict(ar2 if ar2 is not None else ap2),
            "bbox_3D_per_category": dict(ap3 if ap3 is not None else ap2), "bbox_3D_per_category_AR": dict(ar3 if ar3 is not None else ap2)}


def test_novel_easy_hard_split():
    from ovmono3d_amd.evaluation import OMNI3D_NOVEL, OMNI3D_NOVEL_EASY, collective_summary
    assert len(OMNI3D_NOVEL) == 22 and len(OMNI3D_NOVEL_EASY) == 8 and OMNI3D_NOVEL_EASY <= OMNI3D_NOVEL
    hard = sorted(OMNI3D_NOVEL - OMNI3D_NOVEL_EASY)
    ap2 = {c: 10.0 for c in OMNI3D_NOVEL}
    ap2["board"], ap2["tram"] = 30.0, 50.0                                      # easy: (6 * 10 + 30 + 50) / 8 = 17.5
    ap2["monitor"] = 38.0                                                       # hard: (13 * 10 + 38) / 14 = 12
    ap3 = {c: 4.0 for c in OMNI3D_NOVEL}
    ar2 = {c: 60.0 for c in OMNI3D_NOVEL}
    ar3 = {c: 20.0 for c in OMNI3D_NOVEL}
    ar3["rack"] = 48.0                                                          # hard AR3D: (13 * 20 + 48) / 14 = 22
    c = collective_summary(_novel_results(ap2, ap3, ar2, ar3))
    assert c["Novel_Easy"] == {"AP2D": 17.5, "AP3D": 4.0, "AR2D": 60.0, "AR3D": 20.0}
    assert c["Novel_Hard"] == {"AP2D": 12.0, "AP3D": 4.0, "AR2D": 60.0, "AR3D": 22.0}
    assert set(c) == {"<Concat>", "Omni3D_Out", "Omni3D_In", "Omni3D", "Novel_Easy", "Novel_Hard"}
    # a NaN propagates into its group's mean only
    ap3["tray"] = float("nan")
    c = collective_summary(_novel_results(ap2, ap3, ar2, ar3))
    assert np.isnan(c["Novel_Easy"]["AP3D"]) and c["Novel_Easy"]["AP2D"] == 17.5 and c["Novel_Hard"]["AP3D"] == 4.0
    # a category with any result counts (AP2D NaN, AR2D known); no 3D tables: the 3D means are NaN
    ap2["toys"] = float("nan")
    c = collective_summary({"bbox_2D_per_category": ap2, "bbox_2D_per_category_AR": ar2})
    assert np.isnan(c["Novel_Hard"]["AP2D"]) and c["Novel_Hard"]["AR2D"] == 60.0 and np.isnan(c["Novel_Easy"]["AP3D"])
    # any other category set: no entries (one novel category without any result, or an extra one with results)
    nan = float("nan")
    for tables in (_novel_results({**{k: 10.0 for k in hard}, **{k: 10.0 for k in sorted(OMNI3D_NOVEL_EASY)[1:]},
                                   sorted(OMNI3D_NOVEL_EASY)[0]: nan}),
                   _novel_results({**{k: 10.0 for k in OMNI3D_NOVEL}, "chair": 3.0}),
                   _novel_results({k: 10.0 for k in hard})):
        c = collective_summary(tables)
        assert "Novel_Easy" not in c and "Novel_Hard" not in c
    # still present when an extra category has no result at all
    c = collective_summary(_novel_results({**{k: 10.0 for k in OMNI3D_NOVEL}, "chair": nan}))
    assert c["Novel_Easy"]["AP2D"] == 10.0


def test_device_matcher_has_no_cpu_fallback(monkeypatch):
    import torch
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    with pytest.raises(ValueError):
        Omni3Deval([], [], "2D", matcher="gpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    e = Omni3Deval([_ann(1, 0, [0, 0, 10, 10])], [_ann(1, 0, [0, 0, 10, 10], score=0.5)], "2D", matcher="device")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.evaluate()


def test_eval_cell_layout_matches_the_library():
    from ovmono3d_amd import lib
    from ovmono3d_amd.evaluation.omni3d_eval import _CELL_DTYPE
    L = lib.load()
    assert C.sizeof(lib.OvmEvalCell) == 32 == _CELL_DTYPE.itemsize
    assert L.ovm_abi_sizeof(b"OvmEvalCell") == 32
    assert [f[0] for f in lib.OvmEvalCell._fields_] == list(_CELL_DTYPE.names)
    assert all(getattr(lib.OvmEvalCell, n).offset == _CELL_DTYPE.fields[n][1] for n in _CELL_DTYPE.names)


def test_entry_point_flags():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.train_net import default_argument_parser, uses_proximity
    a = default_argument_parser().parse_args(["--eval-only"])
    assert a.eval_prox is False and a.eval_matcher == "host"
    a = default_argument_parser().parse_args(["--eval-only", "--eval-prox", "--eval-matcher", "device", "MODEL.WEIGHTS", "x.pth"])
    assert a.eval_prox is True and a.eval_matcher == "device" and a.opts == ["MODEL.WEIGHTS", "x.pth"]
    with pytest.raises(SystemExit):
        default_argument_parser().parse_args(["--eval-matcher", "cpu"])
    assert uses_proximity("SUNRGBD_test_novel") and uses_proximity("Objectron_test")
    assert not uses_proximity("KITTI_test_novel") and not uses_proximity("ARKitScenes_test_novel")
