"""OVMono3D-GEO without a GPU: the numpy restatement (tests/geo_oracle.py) against live scikit-learn and a recorded fixture, the
host box function against the restatement, the argument validation of the device calls, and the two tools' file handling."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import geo_oracle as G
from common import GOLDEN, ROOT


def _scene(name):
    depth, mask, K = G.make_scene(**G.SCENES[name])
    return depth, mask, K, G.lift_points(depth, mask, K)


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", list(G.SCENES))
def test_scenes_reach_their_outcomes(name):
    """Every branch of the trial loop is reached by the generator's scenes, and their covariance eigenvalues are well apart."""
    _, _, _, r = _scene(name)
    assert r["status"] == G.OK
    if name in G.SCENE_TRIAL:
        assert r["trial"] == G.SCENE_TRIAL[name]
    assert r["n_used"] == min(r["n_points"], 40000)
    assert (r["n_points"] > 40000) == (name in ("trial2", "trial3", "trial4", "fallback"))
    assert r["n_points"] == {"trial1": 22500, "small": 1200}.get(name, r["n_points"])
    assert r["eig"][1] / r["eig"][0] >= 1.5
    if name == "trial2":                                                  # small clusters exist and the 10 % rule drops them
        sizes = np.bincount(r["labels"][r["labels"] >= 0])
        assert len(sizes) >= 2 and (sizes / r["n_used"] < 0.1).any() and r["n_kept"] == sizes[sizes / r["n_used"] >= 0.1].sum()
    if name == "fallback":
        assert r["n_kept"] == r["n_used"] and (r["labels"] == -1).all()


@pytest.mark.parametrize("name", list(G.SCENES))
def test_restatement_equals_live_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn.cluster import DBSCAN
    from sklearn.decomposition import PCA
    from sklearn.utils import shuffle
    depth, mask, K, r = _scene(name)
    P = G.unproject(depth, mask, K)
    v = PCA(2).fit((P - P.mean(0))[:, [0, 2]]).components_[0]
    assert abs(np.arctan2(v[1], v[0]) - r["yaw"]) <= 1e-12
    n = r["n_points"]
    assert np.array_equal(shuffle(np.arange(n), random_state=42), G.perm_for(n))
    eps = 0.01
    for t in range(1, (r["trial"] or 4) + 1):
        assert np.array_equal(DBSCAN(eps=eps, min_samples=100).fit(r["T"]).labels_, G.dbscan_labels(r["T"], eps, 100)), (name, t)
        eps = 2 * eps


def test_restatement_equals_recorded_sklearn():
    """tests/golden/geo_sklearn.npz (make_geo_golden.py): scikit-learn's labels, yaw and shuffle for two scenes."""
    z = np.load(os.path.join(GOLDEN, "geo_sklearn.npz"))
    for name in ("trial2", "small"):
        _, _, _, r = _scene(name)
        assert abs(float(z[f"{name}_yaw"]) - r["yaw"]) <= 1e-12
        assert np.array_equal(z[f"{name}_perm_head"], G.perm_for(r["n_points"])[:256])
        eps, t = 0.01, 1
        while f"{name}_labels{t}" in z:
            assert np.array_equal(z[f"{name}_labels{t}"].astype(np.int64), G.dbscan_labels(r["T"], eps, 100)), (name, t)
            eps, t = 2 * eps, t + 1
        assert t - 1 == (r["trial"] or 4)


def test_refused_instances_of_the_restatement():
    depth, mask, K = G.make_scene(**G.SCENES["small"])
    assert G.lift_points(depth, np.zeros_like(mask), K)["status"] == G.EMPTY
    one = np.zeros_like(mask)
    one[5, 7] = 1
    assert G.lift_points(depth, one, K)["status"] == G.TOO_FEW
    bad = depth.copy()
    bad[210, 310] = np.inf
    assert G.lift_points(bad, mask, K)["status"] == G.NONFINITE
    assert G.lift_points(depth, None, K, rect=(700, 10, 720, 40))["status"] == G.RECT_OUTSIDE
    assert G.lift_points(depth, None, K, rect=(10, 10, 10, 40))["status"] == G.EMPTY


# ------------------------------------------------------------------------------------------------------------ host function
def _random_result(lib, rng):
    """A lifted instance at 2.5 m or more: |coordinate| <= 8 m keeps a few-ulp difference of a corner (cos / sin of two maths
    libraries) below 1e-14, and fx / Z <= 208 keeps its image in center_2D below 1e-12."""
    r = lib.OvmGeoResult()
    off = rng.uniform(-3, 3, 3)
    off[2] = -rng.uniform(4, 6)
    lo, hi = off - rng.uniform(0.05, 1.5, 3), off + rng.uniform(0.05, 1.5, 3)
    for k in range(3):
        r.offset[k], r.ext_min[k], r.ext_max[k] = off[k], lo[k], hi[k]
    r.yaw = rng.uniform(-np.pi, np.pi)
    return r, off, lo, hi


def test_host_geo_box_against_the_restatement():
    """float64 fields to 1e-12; bbox3D (float32 arithmetic as the reference's torch code) within 2 float32 ulp of the largest
    coordinate. On this set the corners came out bit-equal to torch's CPU matmul; the test does not require it."""
    from ovmono3d_amd import lib
    from ovmono3d_amd.geo import host_box
    rng = np.random.RandomState(7)
    worst, worst_ulp, bit_equal = 0.0, 0.0, True
    for _ in range(100):
        r, off, lo, hi = _random_result(lib, rng)
        got, ref = host_box(r, G.K_SCENE), G.box_of(off, r.yaw, lo, hi, G.K_SCENE)
        for f in ("center_cam", "dimensions", "pose", "center_2D", "depth"):
            worst = max(worst, float(np.abs(np.asarray(got[f]) - np.asarray(ref[f])).max()))
        a, b = np.asarray(got["bbox3D"], np.float32), ref["bbox3D"]
        assert b.dtype == np.float32
        d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        worst_ulp = max(worst_ulp, d / float(np.spacing(np.abs(b).max())))
        bit_equal &= d == 0.0
    print(f"host box: worst float64 difference {worst:.3e}, bbox3D {worst_ulp:.2f} ulp, bit-equal {bit_equal}")
    assert worst <= 1e-12
    assert worst_ulp <= 2.0


def test_pose_is_ry_of_minus_yaw():
    """The reference's Kabsch / SVD pose (get_pose) equals the closed form the host function uses."""
    from ovmono3d_amd import lib
    rng = np.random.RandomState(3)
    for _ in range(50):
        r, off, lo, hi = _random_result(lib, rng)
        pose = G.box_of(off, r.yaw, lo, hi, G.K_SCENE)["pose"]
        c, s = np.cos(r.yaw), np.sin(r.yaw)
        # the SVD sees the float32-rounded identity cuboid, which moves the rotation by a few 1e-8 at most
        assert np.abs(pose - np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])).max() <= 1e-6
        assert abs(np.linalg.det(pose) - 1) <= 1e-12


def test_host_geo_box_refuses_an_unlifted_instance():
    from ovmono3d_amd import lib
    L = lib.load()
    r = lib.OvmGeoResult()
    r.status = lib.OVM_GEO_EMPTY
    K = (C.c_double * 9)(*G.K_SCENE.reshape(9))
    b = lib.OvmGeoBox()
    assert L.ovm_host_geo_box(C.byref(r), K, C.byref(b)) == -1
    assert b"not lifted" in L.ovm_geo_last_error()
    assert L.ovm_host_geo_box(None, K, C.byref(b)) == -1


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_struct_sizes_and_defaults():
    from ovmono3d_amd import lib
    L = lib.load()
    for name, mirror in (("OvmGeoParams", lib.OvmGeoParams), ("OvmGeoInstance", lib.OvmGeoInstance), ("OvmGeoResult", lib.OvmGeoResult),
                         ("OvmGeoBox", lib.OvmGeoBox)):
        assert L.ovm_abi_sizeof(name.encode()) == C.sizeof(mirror), name
    assert C.sizeof(lib.OvmGeoResult) == 11 * 8 + 6 * 4 and C.sizeof(lib.OvmGeoBox) == 18 * 8 + 24 * 4
    p = lib.OvmGeoParams()
    assert L.ovm_geo_default_params(C.byref(p)) == 0
    assert (p.eps0, p.min_samples, p.max_points, p.trials, p.min_cluster, p.min_cluster_frac, p.accept_frac, p.last_stage) == \
        (0.01, 100, 40000, 4, 100, 0.1, 0.5, 0)
    from ovmono3d_amd.geo import GeoParams
    q = GeoParams().to_c()
    assert bytes(p) == bytes(q)


def test_device_calls_validate_before_any_device_work():
    """Every refusal below happens on the host: this test runs without a GPU (bogus device pointers are never touched)."""
    from ovmono3d_amd import lib
    L = lib.load()
    p = lib.OvmGeoParams()
    L.ovm_geo_default_params(C.byref(p))
    K = (C.c_double * 9)(*G.K_SCENE.reshape(9))
    inst = (lib.OvmGeoInstance * 1)()
    inst[0].rect[:] = [0, 0, 300, 300]                                    # 90,000 points, no perm
    nbytes = C.c_int64(-1)
    fake = C.c_void_p(4096)
    assert L.ovm_geo_lift_workspace(inst, 1, 480, 640, C.byref(p), C.byref(nbytes), None) == -6
    assert b"no perm" in L.ovm_geo_last_error()
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(p), fake, None, fake, 1 << 40, None) == -6
    inst[0].rect[:] = [0, 0, 100, 100]
    offs = (C.c_int64 * 2)()
    assert L.ovm_geo_lift_workspace(inst, 1, 480, 640, C.byref(p), C.byref(nbytes), offs) == 0
    assert nbytes.value > 10000 * 24 * 2 and list(offs) == [0, 10000]
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(p), fake, None, fake, 16, None) == -5       # workspace too small
    assert L.ovm_geo_lift(None, 480, 640, K, inst, 1, C.byref(p), fake, None, fake, nbytes.value, None) == -1
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(p), None, None, fake, nbytes.value, None) == -1
    assert L.ovm_geo_lift(fake, 0, 640, K, inst, 1, C.byref(p), fake, None, fake, nbytes.value, None) == -1
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, -1, C.byref(p), fake, None, fake, nbytes.value, None) == -1
    bad = lib.OvmGeoParams.from_buffer_copy(bytes(p))
    bad.trials = 0
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(bad), fake, None, fake, nbytes.value, None) == -1
    bad = lib.OvmGeoParams.from_buffer_copy(bytes(p))
    bad.eps0 = float("nan")
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(bad), fake, None, fake, nbytes.value, None) == -1
    assert b"OvmGeoParams" in L.ovm_geo_last_error()
    K0 = (C.c_double * 9)(*([0.0] * 9))
    assert L.ovm_geo_lift(fake, 480, 640, K0, inst, 1, C.byref(p), fake, None, fake, nbytes.value, None) == -1
    inst[0].mask = 4096
    inst[0].n_points = 480 * 640 + 1
    assert L.ovm_geo_lift(fake, 480, 640, K, inst, 1, C.byref(p), fake, None, fake, nbytes.value, None) == -1
    # the clustering alone
    assert L.ovm_geo_dbscan_workspace(-1, C.byref(nbytes)) == -1
    assert L.ovm_geo_dbscan_workspace(1000, C.byref(nbytes)) == 0 and nbytes.value >= 6 * 4 * 1000
    assert L.ovm_geo_dbscan(fake, -1, 0.01, 100, fake, fake, nbytes.value, None) == -1
    assert L.ovm_geo_dbscan(fake, 1000, 0.0, 100, fake, fake, nbytes.value, None) == -1
    assert L.ovm_geo_dbscan(fake, 1000, 0.01, 0, fake, fake, nbytes.value, None) == -1
    assert L.ovm_geo_dbscan(None, 1000, 0.01, 100, fake, fake, nbytes.value, None) == -1
    assert L.ovm_geo_dbscan(fake, 1000, 0.01, 100, fake, fake, 8, None) == -5


def test_python_layer_refuses_cpu_tensors():
    from ovmono3d_amd.geo import dbscan, lift_boxes
    with pytest.raises(ValueError, match="HIP device"):
        lift_boxes(torch.zeros(480, 640), G.K_SCENE, boxes_xyxy=[[10, 10, 50, 50]])
    with pytest.raises(ValueError, match="HIP device"):
        dbscan(torch.zeros(10, 3, dtype=torch.float64), 0.01, 100)


def test_downsample_perm_is_the_reference_shuffle():
    from ovmono3d_amd.geo import box_to_rect, downsample_perm
    assert np.array_equal(downsample_perm(58000), G.perm_for(58000))
    assert downsample_perm(58000).dtype == np.int32
    assert box_to_rect([10.2, 3.0, 50.0, 40.7]) == (11, 3, 50, 41) == G.box_to_rect([10.2, 3.0, 50.0, 40.7])


# ---------------------------------------------------------------------------------------------------------------- the tools
CATS = [{"id": 7, "name": "monitor"}, {"id": 12, "name": "printer"}, {"id": 30, "name": "chair"}]


def write_fixture(root, name, first_id, seed):
    """A dataset of two 480 x 640 images with ground truth made from the restatement's own boxes, depth and mask files and an
    oracle-2D file. Returns the paths."""
    rng = np.random.RandomState(seed)
    images, annos, oracle = [], [], []
    os.makedirs(os.path.join(root, "depth", "test"), exist_ok=True)
    os.makedirs(os.path.join(root, "masks"), exist_ok=True)
    specs = [dict(z0=2.0, box=(300, 200, 330, 240), seed=seed), dict(z0=1.2, box=(100, 120, 160, 170), noise=0.001, seed=seed + 1),
             dict(z0=3.0, box=(400, 300, 470, 380), noise=0.003, seed=seed + 2)]
    for k in range(2):
        iid = first_id + k
        depth = np.full((G.H, G.W), 5.0, np.float32)
        masks, inst = [], []
        for j, sp in enumerate(specs[k:k + 2]):
            d, m, K = G.make_scene(**sp)
            depth[m > 0] = d[m > 0]
            x0, y0, x1, y1 = sp["box"]
            masks.append(m)
            inst.append({"bbox": [x0 - 0.5, y0 - 0.5, float(x1 - x0), float(y1 - y0)], "category_id": int(j % 2), "score": 0.9 - 0.1 * j,
                         "category_name": CATS[j % 2]["name"]})
        inst.append({"bbox": [5.0, 5.0, 40.0, 40.0], "category_id": 0, "score": 0.1})               # below the threshold
        inst.append({"bbox": [700.0, 10.0, 30.0, 30.0], "category_id": 1, "score": 0.8})            # outside the image / no mask
        images.append({"id": iid, "file_path": f"{name}/img_{iid}.jpg", "height": G.H, "width": G.W, "K": G.K_SCENE.tolist(), "dataset_id": 0})
        np.savez(os.path.join(root, "depth", "test", f"img_{iid}.npz"), depth=depth)
        np.savez(os.path.join(root, "masks", f"{iid}.npz"), masks=np.stack(masks + [np.zeros_like(masks[0])]), index=np.array([0, 1, 3]))
        oracle.append({"image_id": iid, "K": G.K_SCENE.tolist(), "instances": inst})
        # ground truth: the restatement's own box of the first instance, jittered
        b = G.lift_boxes(depth, G.K_SCENE, masks=[masks[0]])[0]
        verts = (np.asarray(b["bbox3D"]) + rng.uniform(-0.004, 0.004, 3)).tolist()
        x0, y0, x1, y1 = specs[k]["box"]
        annos.append({"id": 100 * iid, "image_id": iid, "category_id": 7, "category_name": "monitor", "valid3D": True,
                      "bbox2D_tight": [-1, -1, -1, -1], "bbox2D_trunc": [x0, y0, x1, y1], "bbox2D_proj": [x0, y0, x1, y1],
                      "bbox3D_cam": verts, "center_cam": b["center_cam"], "dimensions": b["dimensions"], "R_cam": b["pose"],
                      "behind_camera": False, "visibility": 1.0, "truncation": 0.0, "segmentation_pts": -1, "lidar_pts": -1, "depth_error": -1})
    ds = {"info": {"name": name}, "images": images, "annotations": annos, "categories": CATS}
    os.makedirs(os.path.join(root, "Omni3D"), exist_ok=True)
    paths = {"dataset": os.path.join(root, "Omni3D", name + ".json"), "oracle2d": os.path.join(root, f"{name}_oracle_2d.json"),
             "depth": os.path.join(root, "depth"), "masks": os.path.join(root, "masks"), "root": os.path.join(root, "Omni3D")}
    with open(paths["dataset"], "w") as f:
        json.dump(ds, f)
    with open(paths["oracle2d"], "w") as f:
        json.dump(oracle, f)
    meta = os.path.join(root, "category_meta.json")
    with open(meta, "w") as f:
        json.dump({"thing_classes": ["monitor", "printer"], "thing_dataset_id_to_contiguous_id": {"7": 0, "12": 1}}, f)
    paths["meta"] = meta
    return paths


def oracle_lift_image(depth, K, boxes_xyxy, masks, params):
    return G.lift_boxes(depth, K, boxes_xyxy=boxes_xyxy, masks=masks)


def test_tools_file_handling(tmp_path, monkeypatch):
    """Both tools end to end on files, the lifter replaced by the restatement: the oracle-2D, depth and mask files are read, the
    score threshold and the skip accounting hold, and a .pth and a .json output give the same evaluation."""
    geo, ev = _tool("ovmono3d_geo"), _tool("eval_ovmono3d_geo")
    monkeypatch.setattr(geo, "lift_image", oracle_lift_image)
    p = write_fixture(str(tmp_path), "SYN_test_novel", 10, 0)
    outs = {}
    for ext in ("pth", "json"):
        out = str(tmp_path / f"pred_mask.{ext}")
        args = geo.argument_parser().parse_args(["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"],
                                                 "--mask-dir", p["masks"], "--output", out])
        stats = geo.run(args)
        # per image: 4 instances, 1 below 0.30, the mask at position 3 is empty -> skipped
        assert stats == {"images": 2, "instances": 8, "below_threshold": 2, "skipped": 2, "lifted": 4}
        outs[ext] = out
    recs = ev.load_predictions(outs["pth"])
    assert recs == ev.load_predictions(outs["json"])
    assert [r["image_id"] for r in recs] == [10, 11] and all("K" in r for r in recs)
    for r in recs:
        for ins in r["instances"]:
            assert set(ins) >= {"category_id", "bbox", "score", "image_id", "bbox3D", "depth", "center_cam", "dimensions", "pose", "center_2D"}
            assert ins["image_id"] == r["image_id"] and ins["depth"] == ins["center_cam"][2] and np.asarray(ins["bbox3D"]).shape == (8, 3)
    assert recs[0]["instances"][0]["category_name"] == "monitor"
    # the box as the mask: position 3 lies outside the image -> skipped
    out = str(tmp_path / "pred_box.json")
    stats = geo.run(geo.argument_parser().parse_args(["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"],
                                                     "--mask", "box", "--output", out]))
    assert stats == {"images": 2, "instances": 8, "below_threshold": 2, "skipped": 2, "lifted": 4}
    # a depth map of another shape is refused
    np.savez(os.path.join(p["depth"], "test", "img_10.npz"), depth=np.zeros((240, 320), np.float32))
    with pytest.raises(SystemExit, match="resolution"):
        geo.run(geo.argument_parser().parse_args(["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"],
                                                  "--mask", "box", "--output", out]))
    # the evaluator on both files (AP2D only: the 3D IoU needs the device)
    res = {}
    for ext in ("pth", "json"):
        w = ev.run(ev.argument_parser().parse_args(["--predictions", "SYN_test_novel=" + outs[ext], "--datasets-root", p["root"],
                                                    "--category-meta", p["meta"], "--output-dir", str(tmp_path / ("ev_" + ext)), "--only-2d"]))
        res[ext] = json.load(open(w["SYN_test_novel"]))
        assert "collective" in json.load(open(w["all"]))
    assert res["pth"] == res["json"]
    assert res["pth"]["bbox_2D"]["AP"] > 50.0
    fs = ev.geo_filter_settings()
    assert len(fs["category_names"]) == 22 and fs["max_height_thres"] == 1.5 and fs["min_height_thres"] == 0.0625
