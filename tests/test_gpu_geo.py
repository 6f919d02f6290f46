"""OVMono3D-GEO on the device (csrc/geo.hip, ovmono3d_amd/geo) against the numpy restatement tests/geo_oracle.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import geo_oracle as G
from common import ROOT
from test_geo_cpu import write_fixture

pytestmark = pytest.mark.gpu

ULP32 = lambda v: float(np.spacing(np.float32(abs(v))))  # noqa: E731


def _labels_on_device(T, eps, device):
    from ovmono3d_amd.geo import dbscan
    return dbscan(torch.from_numpy(np.ascontiguousarray(T)).to(device), eps, 100).cpu().numpy().astype(np.int64)


def _dbscan_cases():
    for name, kw in G.SCENES.items():
        depth, mask, K = G.make_scene(**kw)
        r = G.lift_points(depth, mask, K)
        eps = 0.01
        for t in range(1, (r["trial"] or 4) + 1):
            yield f"{name}@{eps:g}", r["T"], eps
            eps = 2 * eps
    yield "blobs@0.02", G.make_blobs(), 0.02
    yield "n1", np.array([[0.1, 0.2, -1.0]]), 0.01
    yield "n99", np.random.RandomState(1).randn(99, 3) * 0.001, 0.01
    yield "n100_coincident", np.tile(np.array([[0.3, -0.2, -2.0]]), (100, 1)), 0.01
    yield "n99_coincident", np.tile(np.array([[0.3, -0.2, -2.0]]), (99, 1)), 0.01


def test_dbscan_labels_equal_the_restatement(device):
    """Exact label equality, scikit-learn's numbering. Condition, asserted with the restatement alone: no pair distance within 1e-9
    (relative) of eps, so that no label hangs on the last bits of a distance."""
    from scipy.spatial import cKDTree
    seen_blobs = False
    for name, T, eps in _dbscan_cases():
        assert G.eps_margin_ok(T, eps), f"{name}: a pair distance lies within 1e-9 of eps - take another seed"
        ref = G.dbscan_labels(T, eps, 100)
        if name.startswith("blobs"):
            core = cKDTree(T).query_ball_point(T, eps, return_length=True) >= 100
            assert len(T) == 40000 and ref.max() + 1 >= 5 and int(((ref >= 0) & ~core).sum()) >= 1000
            seen_blobs = True
        if name == "n99":
            assert (ref == -1).all()
        if name == "n100_coincident":
            assert (ref == 0).all()
        got = _labels_on_device(T, eps, device)
        assert got.shape == ref.shape
        bad = np.nonzero(got != ref)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} labels differ, first at {bad[:5]}: {got[bad[:5]]} vs {ref[bad[:5]]}"
    assert seen_blobs


def _lift_composite(device, subset=None, want_labels=False):
    from ovmono3d_amd.geo import lift
    depth, K, inst = G.make_composite()
    if subset is not None:
        inst = [inst[i] for i in subset]
    d = torch.from_numpy(depth).to(device)
    masks = [torch.from_numpy(it["mask"]).to(device) if "mask" in it else None for it in inst]
    boxes = np.array([it.get("box", (0.0, 0.0, 0.0, 0.0)) for it in inst], np.float64)
    res, lab = lift(d, K, boxes_xyxy=boxes, masks=masks, want_labels=want_labels)
    return depth, K, inst, res, lab


def test_lift_against_the_restatement(device):
    """15 instances in one call: the six scenes as mask planes, three of them again as rectangles, a rectangle clipped by the image
    border, and one instance of each refused kind. Counts, trial and status are equal; offset, yaw and extents agree within 1e-7
    (m, rad): an fp64 sum of <= 307,200 terms of <= 100 m is good to about 3e-9, the eigenvector's conditioning is allowed 30 x
    that. Condition: the two eigenvalues of the 2 x 2 covariance are a factor >= 1.5 apart."""
    from ovmono3d_amd.geo import host_box
    depth, K, inst, res, lab = _lift_composite(device, want_labels=True)
    assert len(inst) >= 12
    refs = [G.lift_points(depth, it.get("mask"), K, rect=G.box_to_rect(it["box"]) if "box" in it else None) for it in inst]
    assert {r["trial"] for r in refs if r["status"] == G.OK} == {0, 1, 2, 3, 4}
    assert {r["status"] for r in refs} == {G.OK, G.EMPTY, G.TOO_FEW, G.NONFINITE, G.RECT_OUTSIDE}
    assert any(r["status"] == G.OK and r["n_points"] <= 40000 for r in refs) and sum("mask" in it for it in inst) >= 6 and \
        sum("box" in it for it in inst) >= 4
    worst, worst_box, worst_ulp = 0.0, 0.0, 0.0
    for it, got, ref, gl in zip(inst, res, refs, lab):
        name = it["name"]
        assert got.status == ref["status"], name
        assert got.n_points == ref["n_points"], name
        if ref["status"] != G.OK:
            assert (got.n_used, got.n_kept, got.trial) == (0, 0, 0), name
            continue
        with np.errstate(divide="ignore"):
            assert ref["eig"][1] / ref["eig"][0] >= 1.5, name
        assert (got.n_used, got.n_kept, got.trial) == (ref["n_used"], ref["n_kept"], ref["trial"]), name
        assert got.eps == ref["eps"], name
        assert np.array_equal(gl.astype(np.int64), ref["labels"]), name
        e = max(np.abs(np.array(got.offset) - ref["offset"]).max(), abs(got.yaw - ref["yaw"]),
                np.abs(np.array(got.ext_min) - ref["ext_min"]).max(), np.abs(np.array(got.ext_max) - ref["ext_max"]).max())
        print(f"{name}: n {got.n_points} used {got.n_used} kept {got.n_kept} trial {got.trial}  max |offset, yaw, extents - restatement| {e:.3e}")
        worst = max(worst, float(e))
        assert e <= 1e-7, name
        b, rb = host_box(got, K), G.box_of(ref["offset"], ref["yaw"], ref["ext_min"], ref["ext_max"], K)
        for f in ("center_cam", "dimensions", "pose", "center_2D", "depth"):
            eb = float(np.abs(np.asarray(b[f]) - np.asarray(rb[f])).max())
            worst_box = max(worst_box, eb)
            assert eb <= 1e-6, (name, f)
        d = float(np.abs(np.asarray(b["bbox3D"], np.float64) - rb["bbox3D"].astype(np.float64)).max())
        u = d / ULP32(np.abs(rb["bbox3D"]).max())
        worst_ulp = max(worst_ulp, u)
        assert u <= 4.0, name
    print(f"lift: worst offset / yaw / extent error {worst:.3e}; box fields {worst_box:.3e}; bbox3D {worst_ulp:.2f} float32 ulp")


def test_one_call_of_n_equals_n_calls_of_one(device):
    _, _, inst, res, lab = _lift_composite(device, want_labels=True)
    for i in range(len(inst)):
        _, _, _, r1, l1 = _lift_composite(device, subset=[i], want_labels=True)
        assert bytes(r1[0]) == bytes(res[i]), inst[i]["name"]
        assert np.array_equal(l1[0], lab[i]), inst[i]["name"]


def test_lift_boxes_keys_and_refusals(device):
    from ovmono3d_amd.geo import lift_boxes
    depth, K, inst = G.make_composite()
    d = torch.from_numpy(depth).to(device)
    out = lift_boxes(d, K, boxes_xyxy=[it["box"] for it in inst if "box" in it])
    assert [o is None for o in out] == [False, False, False, True, True, False]
    assert set(out[0]) == {"bbox3D", "depth", "center_cam", "dimensions", "pose", "center_2D"}
    ref = G.lift_boxes(depth, K, boxes_xyxy=[it["box"] for it in inst if "box" in it])
    for a, b in zip(out, ref):
        if a is not None:
            assert np.abs(np.asarray(a["center_cam"]) - np.asarray(b["center_cam"])).max() <= 1e-6
    # more than max_points points and no perm: refused by the library before any device work
    from ovmono3d_amd import lib
    L = lib.load()
    p = lib.OvmGeoParams()
    L.ovm_geo_default_params(C.byref(p))
    one = (lib.OvmGeoInstance * 1)()
    one[0].rect[:] = [0, 0, 300, 300]
    nb = C.c_int64()
    assert L.ovm_geo_lift_workspace(one, 1, d.shape[0], d.shape[1], C.byref(p), C.byref(nb), None) == -6
    with pytest.raises(ValueError):
        lift_boxes(d.double(), K, boxes_xyxy=[[0, 0, 10, 10]])


def _run(cmd):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_through_the_tools(device, tmp_path):
    """tools/ovmono3d_geo.py on a synthetic two-dataset fixture gives the restatement's records, and tools/eval_ovmono3d_geo.py
    gives the same omni_ap.json from either."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tool_geo", os.path.join(ROOT, "tools", "ovmono3d_geo.py"))
    geo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geo)
    from test_geo_cpu import oracle_lift_image
    names = ("SYNA_test_novel", "SUNRGBD_syn_novel")
    preds = {"device": [], "oracle": []}
    for k, name in enumerate(names):
        p = write_fixture(str(tmp_path / name), name, 10 + 100 * k, seed=3 * k)
        # the datasets share one root for the evaluator
        os.makedirs(tmp_path / "Omni3D", exist_ok=True)
        os.replace(p["dataset"], tmp_path / "Omni3D" / (name + ".json"))
        p["dataset"] = str(tmp_path / "Omni3D" / (name + ".json"))
        common = ["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"], "--mask-dir", p["masks"]]
        out_dev = str(tmp_path / f"{name}_device.pth")
        _run([os.path.join("tools", "ovmono3d_geo.py")] + common + ["--output", out_dev])
        out_ref = str(tmp_path / f"{name}_oracle.pth")
        orig = geo.lift_image
        geo.lift_image = oracle_lift_image
        try:
            geo.run(geo.argument_parser().parse_args(common + ["--output", out_ref]))
        finally:
            geo.lift_image = orig
        a, b = torch.load(out_dev, weights_only=False), torch.load(out_ref, weights_only=False)
        assert len(a) == len(b) == 2
        for ra, rb in zip(a, b):
            assert {k: v for k, v in ra.items() if k != "instances"} == {k: v for k, v in rb.items() if k != "instances"}
            assert len(ra["instances"]) == len(rb["instances"]) == 2
            for ia, ib in zip(ra["instances"], rb["instances"]):
                assert set(ia) == set(ib)
                for f in ("category_id", "bbox", "score", "image_id"):
                    assert ia[f] == ib[f]
                for f in ("center_cam", "dimensions", "pose", "center_2D", "depth"):
                    assert np.abs(np.asarray(ia[f]) - np.asarray(ib[f])).max() <= 1e-6, f
                assert np.abs(np.asarray(ia["bbox3D"]) - np.asarray(ib["bbox3D"])).max() <= 4 * ULP32(np.abs(np.asarray(ib["bbox3D"])).max())
        preds["device"].append(f"{name}={out_dev}")
        preds["oracle"].append(f"{name}={out_ref}")
        meta = p["meta"]
    aps = {}
    for which in ("device", "oracle"):
        out_dir = str(tmp_path / ("eval_" + which))
        _run([os.path.join("tools", "eval_ovmono3d_geo.py"), "--predictions"] + preds[which] +
             ["--datasets-root", str(tmp_path / "Omni3D"), "--category-meta", meta, "--output-dir", out_dir, "--eval-prox"])
        aps[which] = {n: json.load(open(os.path.join(out_dir, n, "omni_ap.json"))) for n in names}
        aps[which]["all"] = json.load(open(os.path.join(out_dir, "omni_ap_all.json")))
        assert "collective" in aps[which]["all"]
    assert aps["device"] == aps["oracle"]
    assert aps["device"][names[0]]["bbox_3D"]["AP"] > 0.0


def test_wrong_pixel_count_and_bad_perm_are_refused_per_instance(device):
    """What only the device can see: a mask plane that holds another number of pixels than declared, and a perm entry outside
    0 .. n-1. The instance gets a status, nothing is written out of range, and its neighbour in the call is lifted as ever."""
    from ovmono3d_amd import lib
    from ovmono3d_amd.geo import LiftCall
    depth, K, inst = G.make_composite()
    by = {it["name"]: it for it in inst}
    d = torch.from_numpy(depth).to(device)
    masks = [torch.from_numpy(by[n]["mask"]).to(device) for n in ("small", "trial3", "trial1")]
    call = LiftCall(d, K, masks=masks)
    call.launch()
    good, _ = call.read()
    assert [r.status for r in good] == [0, 0, 0]
    call = LiftCall(d, K, masks=masks)
    assert call.inst[0].n_points == 1200 and call.inst[1].n_points == 58000
    call.inst[0].n_points = 1000
    perm = torch.from_numpy(G.perm_for(58000).astype(np.int32)).to(device)
    perm[5] = 58000
    call.inst[1].perm = perm.data_ptr()
    call.launch()
    res, _ = call.read()
    assert res[0].status == lib.OVM_GEO_COUNT_MISMATCH and res[0].n_points == 1200 and res[0].n_used == 0
    assert res[1].status == lib.OVM_GEO_BAD_PERM and res[1].n_points == 58000 and res[1].n_kept == 0
    assert bytes(res[2]) == bytes(good[2])
