"""CPU: the evaluation sample panels' host layout (ovm_host_panels_layout, ovmono3d_amd/csrc/panels.hip) against the numpy
restatement tests/panels_oracle.py - exactly -, the error summary of visualize_from_instances against a scalar, loop-by-loop
restatement below, the ABI of the new structs, and the --vis-every switch of tools/train_net.py."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import panels_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((96, 128), (250, 334))
COUNTS = ((0, 0), (12, 20), (5, 0), (0, 7), (3, 20), (12, 1))


def _library_panels(K, H, W, gt_all, gt_eval, preds):
    from ovmono3d_amd import vis
    lay, prims, glyphs = vis.panels_layout(K, H, W, gt_all, gt_eval, preds)
    assert (lay.height, lay.width, lay.thickness3d) == (H, W, po.thickness3d(H))
    assert lay.start[0] == 0 and lay.start[6] == lay.n_prims and lay.glyph_bytes == glyphs.size
    out = []
    for p in range(6):
        cur = []
        for i in range(lay.start[p], lay.start[p + 1]):
            q = prims[i]
            a, col = [int(v) for v in q.a], tuple(int(v) for v in q.color[:3])
            if q.kind == 0:
                cur.append(("seg", *a, int(q.thickness), col))
            elif q.kind == 1:
                cur.append(("blend", *a, col))
            else:
                assert q.kind == 2 and 0 <= q.glyph_offset and q.glyph_offset + a[2] * a[3] <= glyphs.size
                cur.append(("glyph", *a, col, glyphs[q.glyph_offset:q.glyph_offset + a[2] * a[3]].reshape(a[3], a[2])))
        out.append(cur)
    return out


def _same(lib, ref, what):
    for p in range(6):
        assert len(lib[p]) == len(ref[p]), f"{what}: panel {p} has {len(lib[p])} primitives, the oracle {len(ref[p])}"
        for k, (a, b) in enumerate(zip(lib[p], ref[p])):
            if a[0] == "glyph":
                assert a[:-1] == b[:-1] and np.array_equal(a[-1], b[-1]), f"{what}: panel {p} primitive {k}: {a[:-1]} != {b[:-1]}"
            else:
                assert a == b, f"{what}: panel {p} primitive {k}: {a} != {b}"


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("n_gt,n_pred", COUNTS)
def test_layout_matches_oracle_on_seeded_scenes(H, W, n_gt, n_pred):
    K, gt_all, gt_eval, preds = po.make_scene(1000 + 31 * n_gt + n_pred + H, n_gt, n_pred, H, W)
    _same(_library_panels(K, H, W, gt_all, gt_eval, preds), po.layout(K, H, W, gt_all, gt_eval, preds), f"{n_gt}+{n_pred} {H}x{W}")


@pytest.mark.parametrize("H,W", SIZES + ((60, 80), (416, 555)))
def test_layout_matches_oracle_on_constructed_cases(H, W):
    for name, (K, gt_all, gt_eval, preds) in po.constructed(H, W).items():
        _same(_library_panels(K, H, W, gt_all, gt_eval, preds), po.layout(K, H, W, gt_all, gt_eval, preds), f"{name} {H}x{W}")


def _kinds(panel):
    return [p[0] for p in panel]


def _eq(a, b):
    """Two primitive lists are the same (glyph masks compared as arrays)."""
    return len(a) == len(b) and all(p[0] == q[0] and (p[:-1] == q[:-1] and np.array_equal(p[-1], q[-1]) if p[0] == "glyph" else p == q)
                                    for p, q in zip(a, b))


def test_constructed_cases_are_what_they_claim():
    H, W = 250, 334
    cases = po.constructed(H, W)
    lib = {k: _library_panels(*((v[0], H, W) + v[1:])) for k, v in cases.items()}
    # a cuboid straddling zplane keeps some edges and loses others; every kept endpoint was cut at or in front of the plane
    n = _kinds(lib["straddle"][3]).count("seg")
    assert 0 < n < 12
    # wholly behind: no edge; the label (drawn from the 2D box) stays, as in the reference
    assert _kinds(lib["behind"][3]) == ["blend", "glyph"] and _kinds(lib["behind"][0]) == ["seg"] * 4 + ["glyph"]
    # boxes partly / wholly off the canvas keep their primitives in the list (the renderer clips), with the int() corners
    assert lib["partly_off"][0][0][:5] == ("seg", -15, -8, 24, -8) and lib["wholly_off"][0][0][:5] == ("seg", W + 20, H + 10, W + 50, H + 10)
    assert _kinds(lib["wholly_off"][3]).count("seg") == 12
    # labels at the border: the rectangle is clipped to the image, and dropped when nothing of it is left
    blends = [p for p in lib["border_label"][3] if p[0] == "blend"]
    assert len(blends) == 2 and blends[0][3] == W and blends[0][2] == 0 and blends[1][1:3] == (0, 0)
    assert all(0 <= p[1] < p[3] <= W and 0 <= p[2] < p[4] <= H for k in lib for q in lib[k] for p in q if p[0] == "blend")
    # an annotation whose class is not prompted is absent from the middle column only
    u = lib["unprompted"]
    assert len(u[0]) == 2 * len(u[1]) == 10 and len(u[3]) == 2 * len(u[4]) and _eq(u[1], u[0][:5]) and _eq(u[4], u[3][:len(u[4])])
    # a prediction below the threshold: 2D panel only
    assert len(lib["pred_2d_only"][2]) == 10 and _eq(lib["pred_2d_only"][5], lib["pred_2d_only"][3])


@pytest.mark.parametrize("H,thickness", ((60, 1), (83, 1), (84, 1), (250, 2), (416, 2), (417, 3), (500, 3)))
def test_thickness_rounds_half_to_even_and_clamps(H, thickness):
    K, gt_all, gt_eval, preds = po.make_scene(7, 2, 2, H, 100)
    from ovmono3d_amd import vis
    lay, prims, _ = vis.panels_layout(K, H, 100, gt_all, gt_eval, preds)
    assert lay.thickness3d == thickness == po.thickness3d(H)
    assert {prims[i].thickness for i in range(lay.start[3], lay.n_prims) if prims[i].kind == 0} == {thickness}
    assert {prims[i].thickness for i in range(0, lay.start[3]) if prims[i].kind == 0} == {2}


def test_oracle_bands_are_small():
    """The GPU test's scenes: the pixels the oracle itself calls ambiguous stay below 0.1 % of the mosaic."""
    import test_gpu_evalvis as tg
    for what, H, W, (K, gt_all, gt_eval, preds) in tg.scenes():
        img = tg.image(H, W)
        _, band = po.render(img, po.layout(K, H, W, gt_all, gt_eval, preds))
        assert band.sum() < 1e-3 * band.size, f"{what}: {int(band.sum())} band pixels of {band.size}"


# ---------------------------------------------------------------------------------------------------------- error summary

CATS = ["chair", "table", "sofa", "bed"]


def _scalar_summary(detections, dataset, dataset_name, iteration, every, fork_compat):
    """visualize_from_instances' error summary, one loop per step (reference :204-254, 285-294)."""
    xy_e, z_e, w_e, h_e, l_e, ry_e = [], [], [], [], [], []
    for imind, im_obj in enumerate(detections):
        sampled = every > 0 and imind % every == 0
        if fork_compat and not sampled:
            continue
        annos = dataset._dataset[imind]["annotations"]
        if len(annos) == 0:
            continue
        data_obj = dataset[imind]
        iid = im_obj.get("image_id")
        if isinstance(iid, str):
            matched = iid.split("/")[-1] == data_obj["file_name"].split("/")[-1]
        else:
            matched = isinstance(iid, int) and isinstance(data_obj.get("image_id"), int) and iid == data_obj["image_id"]
        if not matched:
            continue
        K = im_obj["K"]
        for inst in im_obj["instances"]:
            x1, y1, w, h = inst["bbox"]
            x2, y2 = x1 + w, y1 + h
            best, best_iou = None, -math.inf
            for a in annos:
                if a["category_id"] != inst["category_id"]:
                    continue
                gx1, gy1, gx2, gy2 = a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]
                iw, ih = max(min(x2, gx2) - max(x1, gx1), 0), max(min(y2, gy2) - max(y1, gy1), 0)
                inter = iw * ih
                iou = inter / (((x2 - x1) * (y2 - y1) + (gx2 - gx1) * (gy2 - gy1)) - inter)
                if iou > best_iou:                                   # strict: the first maximum wins
                    best, best_iou = a, iou
            if best is None or not best_iou >= 0.5:
                continue
            gc = best["center_cam"]
            den = (K[2][0] * gc[0] + K[2][1] * gc[1]) + K[2][2] * gc[2]
            dx = inst["center_2D"][0] - ((K[0][0] * gc[0] + K[0][1] * gc[1]) + K[0][2] * gc[2]) / den
            dy = inst["center_2D"][1] - ((K[1][0] * gc[0] + K[1][1] * gc[1]) + K[1][2] * gc[2]) / den
            xy_e.append(math.sqrt(dx * dx + dy * dy))
            z_e.append(abs(inst["center_cam"][2] - gc[2]))
            w_e.append(abs(inst["dimensions"][0] - best["dimensions"][0]))
            h_e.append(abs(inst["dimensions"][1] - best["dimensions"][1]))
            l_e.append(abs(inst["dimensions"][2] - best["dimensions"][2]))
            trace = None
            for i in range(3):
                for j in range(3):
                    t = inst["pose"][i][j] * best["pose"][i][j]
                    trace = t if trace is None else trace + t
            if fork_compat:
                if trace < -1 - 1e-4 or trace > 3 + 1e-4:
                    continue
                ry_e.append(math.pi / 2 - (trace - 1) / 2)
            else:
                ry_e.append(math.acos(min(max((trace - 1) / 2, -1.0), 1.0)))
    lists = (xy_e, z_e, w_e, h_e, l_e, list(ry_e))
    if len(ry_e) == 0:
        ry_e = [1000, 1000]
    mean = lambda v: float(np.mean(v)) if len(v) else float("nan")  # noqa: E731
    return dataset_name + "iter={}, xy({:.2f}), z({:.2f}), whl({:.2f}, {:.2f}, {:.2f}), ry({:.2f})\n".format(
        iteration, mean(xy_e), mean(z_e), mean(w_e), mean(h_e), mean(l_e), mean(ry_e)), lists


def _anno(cat, bbox, center, dims, ang):
    return {"category_id": cat, "bbox": list(bbox), "center_cam": list(center), "dimensions": list(dims), "pose": po.yaw(ang)}


def _inst(cat, bbox, c2d, z, dims, pose, score=0.9):
    return {"category_id": cat, "score": score, "bbox": list(bbox), "center_2D": list(c2d), "center_cam": [0.0, 0.0, z],
            "dimensions": list(dims), "pose": pose}


def _summary_case(n_images=7):
    from ovmono3d_amd import vis
    rng = np.random.default_rng(5)
    K = po.intrinsics(96, 128).tolist()
    records, dets = [], []
    for i in range(n_images):
        annos, insts = [], []
        for _ in range(int(rng.integers(1, 6))):
            b = [float(v) for v in (rng.uniform(0, 80), rng.uniform(0, 50), rng.uniform(8, 40), rng.uniform(8, 40))]
            a = _anno(int(rng.integers(0, 4)), b, (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)), rng.uniform(0.3, 2, 3),
                      rng.uniform(-3, 3))
            annos.append(a)
            for _ in range(int(rng.integers(0, 3))):                 # jittered predictions, some of another class
                jb = [b[0] + rng.uniform(-4, 4), b[1] + rng.uniform(-4, 4), b[2] * rng.uniform(0.7, 1.3), b[3] * rng.uniform(0.7, 1.3)]
                insts.append(_inst(a["category_id"] if rng.uniform() > 0.2 else (a["category_id"] + 1) % 4, jb,
                                   (rng.uniform(0, 128), rng.uniform(0, 96)), rng.uniform(2, 6), rng.uniform(0.3, 2, 3),
                                   po.yaw(rng.uniform(-3, 3))))
        records.append({"file_name": f"/data/img/{i:04d}.jpg", "image_id": i, "annotations": annos})
        dets.append({"image_id": i, "K": K, "height": 96, "width": 128, "instances": insts})
    # by construction
    sq = [10.0, 10.0, 20.0, 20.0]
    records[1]["annotations"] = [_anno(0, [0.0, 10.0, 20.0, 20.0], (0, 0, 3), (1, 1, 1), 0.1),      # a tie in IoU: both 1/3 ...
                                 _anno(0, [20.0, 10.0, 20.0, 20.0], (1, 0, 4), (2, 2, 2), 0.2),
                                 _anno(1, [40.0, 40.0, 30.0, 30.0], (0, 1, 5), (1, 2, 3), 0.3),      # ... IoU exactly 0.5 with the 2nd instance
                                 _anno(1, [40.0, 40.0, 30.0, 30.0], (0, 1, 6), (3, 2, 1), 0.4),      # and a tie at 0.5: the first wins
                                 _anno(2, sq, (0, 0, 3), (1, 1, 1), 0.0)]
    eye = po.yaw(0.0)
    big = [[1.0 + 2e-4 / 3, 0.0, 0.0], [0.0, 1.0 + 2e-4 / 3, 0.0], [0.0, 0.0, 1.0 + 2e-4 / 3]]
    dets[1]["instances"] = [_inst(0, sq, (60, 40), 3.5, (1, 1, 1), eye),                              # IoU 1/3 with both: no match
                            _inst(1, [40.0, 40.0, 30.0, 15.0], (64, 50), 5.5, (1, 1, 1), po.yaw(1.0)),  # IoU exactly 0.5: match
                            _inst(3, sq, (60, 40), 3.0, (1, 1, 1), eye),                              # no ground truth of the class
                            _inst(2, sq, (64, 48), 3.0, (1, 1, 1), big)]                              # trace 3 + 2e-4
    records[2]["annotations"] = []                                                                    # an image without annotations
    dets[3]["image_id"] = 999                                                                         # an id mismatch
    dets[4]["image_id"] = "some/where/0004.jpg"                                                       # matched by file base name
    dets[5]["image_id"] = "some/where/0099.jpg"                                                       # mismatch by base name
    return dets, vis.SampleDataset(records)


@pytest.mark.parametrize("fork_compat", (False, True))
@pytest.mark.parametrize("every", (0, 1, 2, 50))
def test_error_summary_matches_scalar_restatement(tmp_path, fork_compat, every):
    from ovmono3d_amd.vis import panels
    dets, ds = _summary_case()
    want, lists = _scalar_summary(dets, ds, "SUNRGBD_test", "final", every, fork_compat)
    errs = [[] for _ in range(6)]
    for imind, im_obj in enumerate(dets):                            # the vectorised per-image step, image by image
        if fork_compat and not (every > 0 and imind % every == 0):
            continue
        annos = ds._dataset[imind]["annotations"]
        if annos and panels._image_matches(im_obj, ds[imind]):
            for dst, src in zip(errs, panels.match_errors(im_obj, annos, fork_compat)):
                dst += src
    assert errs == [list(v) for v in lists]                          # bit for bit, in order
    # the whole function: sampled images would be drawn on the device, so only the runs that sample none run here
    if every == 0:
        got = panels.visualize_from_instances(dets, ds, "SUNRGBD_test", 512, str(tmp_path), CATS, CATS, "final", every=0,
                                              fork_compat=fork_compat)
        assert got == want
        assert os.listdir(tmp_path / "vis") == []


def test_error_summary_constructed_pairs():
    from ovmono3d_amd.vis import panels
    dets, ds = _summary_case()
    annos = ds._dataset[1]["annotations"]
    xy, z, w, h, l, ry = panels.match_errors(dets[1], annos, False)
    # instance 1 matches the FIRST of the two tied boxes (z 5, dims 1 2 3); instance 3 is clipped to angle 0
    assert z == [0.5, 0.0] and w == [0.0, 0.0] and h == [1.0, 0.0] and l == [2.0, 0.0]
    assert ry[1] == 0.0 and ry[0] == pytest.approx(0.7, abs=1e-12)
    xy_f, *_, ry_f = panels.match_errors(dets[1], annos, True)
    assert len(xy_f) == 2 and len(ry_f) == 1                         # trace 3 + 2e-4: the pair is dropped from ry only
    assert ry_f[0] == pytest.approx(math.pi / 2 - (1 + 2 * math.cos(0.7) - 1) / 2, abs=1e-12)
    assert xy[1] == pytest.approx(0.0, abs=1e-9)                     # centre (0, 0, 3) projects to the principal point (64, 48)


def test_error_summary_empty_and_log_string(tmp_path):
    from ovmono3d_amd import vis
    ds = vis.SampleDataset([{"file_name": "a.jpg", "image_id": 0, "annotations": []}])
    dets = [{"image_id": 0, "K": po.intrinsics(96, 128).tolist(), "height": 96, "width": 128, "instances": []}]
    s = vis.visualize_from_instances(dets, ds, "KITTI_test", 512, str(tmp_path), CATS, CATS, every=0)
    assert s == "KITTI_testiter=, xy(nan), z(nan), whl(nan, nan, nan), ry(1000.00)\n"
    a = _anno(0, [10.0, 10.0, 20.0, 20.0], (0.0, 0.0, 4.0), (1.0, 2.0, 3.0), 0.0)
    ds = vis.SampleDataset([{"file_name": "a.jpg", "image_id": 0, "annotations": [a]}] * 2)
    i = _inst(0, [10.0, 10.0, 20.0, 20.0], (67.0, 52.0), 4.25, (1.5, 2.0, 2.0), po.yaw(0.5))
    dets = [dict(dets[0], instances=[i]), dict(dets[0], instances=[])]
    s = vis.visualize_from_instances(dets, ds, "KITTI_test", 512, str(tmp_path), CATS, CATS, 1234, every=0)
    assert s == "KITTI_testiter=1234, xy(5.00), z(0.25), whl(0.50, 0.00, 1.00), ry(0.50)\n"
    s = vis.visualize_from_instances(dets, ds, "KITTI_test", 512, str(tmp_path), CATS, CATS, 1234, every=0, fork_compat=True)
    assert s == "KITTI_testiter=1234, xy(nan), z(nan), whl(nan, nan, nan), ry(1000.00)\n"     # the fork looks at sampled images only


def test_prediction_at_the_threshold_is_not_drawn():
    from ovmono3d_amd import vis
    thres = float(np.sqrt(1 / len(CATS)) * 1.2)
    K = po.intrinsics(96, 128)
    a = _anno(0, [10.0, 10.0, 20.0, 20.0], (0.0, 0.0, 4.0), (1.0, 2.0, 3.0), 0.0)
    insts = [_inst(0, [10.0, 10.0, 20.0, 20.0], (67.0, 52.0), 4.0, (1.0, 1.0, 1.0), po.yaw(0.5), score=s)
             for s in (thres, float(np.nextafter(thres, 1.0)), 0.1)]
    im_obj = {"image_id": 0, "K": K.tolist(), "height": 96, "width": 128, "instances": insts}
    K2, gt_all, gt_eval, preds = vis.panel_boxes(im_obj, [a], CATS, ["table"])
    assert [p["draw3d"] for p in preds] == [False, True, False] and gt_eval == [False] and gt_all[0]["name"] == "chair"
    c = preds[1]["center_cam"]                                       # K^-1 @ (z * [center_2D, 1])
    assert np.allclose(K @ np.asarray(c) / c[2], [67.0, 52.0, 1.0], atol=1e-9) and c[2] == pytest.approx(4.0)
    lib = _library_panels(K2, 96, 128, gt_all, gt_eval, preds)
    assert len(lib[2]) == 15
    assert _kinds(lib[5]).count("glyph") == 1 and lib[1] == [] and lib[4] == [] and len(lib[0]) == 5


# ------------------------------------------------------------------------------------------------------------------- ABI

def test_abi_sizes_and_error_codes():
    from ovmono3d_amd import lib as L
    lib = L.load()
    for name, mirror in (("OvmPanelBox", L.OvmPanelBox), ("OvmPanelsInput", L.OvmPanelsInput), ("OvmPanelPrim", L.OvmPanelPrim),
                         ("OvmPanelsLayout", L.OvmPanelsLayout)):
        assert lib.ovm_abi_sizeof(name.encode()) == C.sizeof(mirror) > 0, name
    boxes = (L.OvmPanelBox * 2)()
    for b in boxes:
        b.bbox[:] = [10.0, 10.0, 20.0, 20.0]
        b.center[:] = [0.0, 0.0, 4.0]
        b.dims[:] = [1.0, 1.0, 1.0]
        b.R[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
        b.draw3d = b.in_eval = 1
        b.glyph2d[:] = [5, 4]
        b.glyph3d[:] = [3, 2]
    inp = L.OvmPanelsInput()
    inp.height, inp.width, inp.n_gt, inp.n_pred = 96, 128, 2, 0
    inp.K[:] = po.intrinsics(96, 128).reshape(9).tolist()
    inp.gt = C.addressof(boxes)
    lay = L.OvmPanelsLayout()
    prims = (L.OvmPanelPrim * 128)()
    assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay), prims, 128) == 0
    need = lay.n_prims
    assert need == 2 * (2 * 5 + 2 * 14) and lay.glyph_bytes == 2 * (20 + 6)
    # over capacity: the code, and the count needed
    lay2 = L.OvmPanelsLayout()
    assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), prims, need - 1) == -5 and lay2.n_prims == need
    assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), None, 0) == -5 and lay2.n_prims == need
    # non-finite input, one field at a time
    for field, k in (("bbox", 2), ("center", 0), ("dims", 1), ("R", 8)):
        keep = getattr(boxes[1], field)[k]
        for bad in (float("nan"), float("inf")):
            getattr(boxes[1], field)[k] = bad
            assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), prims, 128) == -1, field
        getattr(boxes[1], field)[k] = keep
    inp.K[4] = float("nan")
    assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), prims, 128) == -1
    inp.K[4] = 100.0
    for h, w, ng in ((0, 128, 2), (96, 40000, 2), (96, 128, -1)):
        inp.height, inp.width, inp.n_gt = h, w, ng
        assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), prims, 128) == -1
    inp.height, inp.width, inp.n_gt = 96, 128, 2
    assert lib.ovm_host_panels_layout(C.byref(inp), C.byref(lay2), prims, 128) == 0
    # the renderer refuses inconsistent arguments before any device work (no GPU is needed to be refused)
    ws = C.c_int64()
    assert lib.ovm_render_panels_workspace(C.byref(lay), C.byref(ws)) == 0 and ws.value >= 256
    lay2.start[3] = lay2.start[2] - 1 if lay2.start[2] else -1
    assert lib.ovm_render_panels_workspace(C.byref(lay2), C.byref(ws)) == -1
    glyphs = np.ones(int(lay.glyph_bytes), np.uint8)
    buf = np.zeros(16, np.uint8)
    args = (glyphs.ctypes.data, glyphs.size, buf.ctypes.data, 3 * 128, buf.ctypes.data, 9 * 128, buf.ctypes.data)
    assert lib.ovm_render_panels(C.byref(lay), prims, *args, ws.value - 1, None) == -5
    assert lib.ovm_render_panels(C.byref(lay), prims, glyphs.ctypes.data, glyphs.size - 1, *args[2:], ws.value, None) == -1
    assert lib.ovm_render_panels(C.byref(lay), prims, *args[:3], 3 * 128 - 1, *args[4:], ws.value, None) == -1
    assert lib.ovm_render_panels(C.byref(lay), prims, *args[:5], 9 * 128 - 1, args[6], ws.value, None) == -1


def test_vis_every_defaults_to_off():
    spec = importlib.util.spec_from_file_location("train_net_for_evalvis", os.path.join(ROOT, "tools", "train_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.default_argument_parser()
    a = p.parse_args([])
    assert a.vis_every == 0 and a.vis_fork_compat is False
    a = p.parse_args(["--vis-every", "50", "--vis-fork-compat"])
    assert a.vis_every == 50 and a.vis_fork_compat is True
    assert "50" in [x for x in p._actions if x.dest == "vis_every"][0].help
