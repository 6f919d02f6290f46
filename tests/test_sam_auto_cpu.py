"""CPU: the rules of SAM's automatic mask generation as tests/sam_auto_oracle.py restates them (the grid, the two filters, the NMS) on
closed cases and against Hugging Face transformers' helpers where it has one for the same rule; the condition of the fields the GPU
kernel test counts (tests/test_gpu_sam_mask_stats.py); that the count comparison rejects named wrong evaluations; the refusals of
``SamAutomaticMaskGenerator``, of the library without a handle, and of demo/demo_geo.py --everything."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ovmono3d_amd.sam import SamAutomaticMaskGenerator  # noqa: F401  (the feature under test: without it this module does not load)
import sam_auto_oracle as ao
import sam_dp_glue_ref as G
from common import ROOT
from sam_auto_oracle import F32, F64


# ---------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("n", [1, 2, 5, 32])
def test_grid_is_the_formula(n):
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator, build_point_grid
    g = build_point_grid(n)
    off = 1 / (2 * n)
    line = np.linspace(off, 1 - off, n)
    assert g.dtype == np.float64 and g.shape == (n * n, 2)
    for i in range(n):
        for j in range(n):
            assert g[i * n + j, 0] == line[j] and g[i * n + j, 1] == line[i]          # x first, row-major in y
    assert np.array_equal(g, ao.point_grid(n))
    H, W = 70, 100                                                                    # W != H: x scales with W, y with H
    gen = SamAutomaticMaskGenerator(None, points_per_side=n)
    pts = gen.grid_points(H, W)
    assert pts.dtype == np.float32 and np.array_equal(pts, ao.grid_points(n, H, W))
    assert np.array_equal(pts[:, 0], (g[:, 0] * W).astype(F32)) and np.array_equal(pts[:, 1], (g[:, 1] * H).astype(F32))
    if n > 1:
        assert pts[1, 0] > pts[0, 0] and pts[1, 1] == pts[0, 1] and pts[n, 1] > pts[0, 1]


def _hf():
    """transformers' SAM image processor helpers (the PIL flavour imports without torchvision)"""
    import transformers.models.sam.image_processing_pil_sam as m
    return m


@pytest.mark.parametrize("n", [1, 2, 5, 32])
def test_grid_equals_transformers(n):
    assert np.array_equal(ao.point_grid(n), _hf()._build_point_grid(n))


def test_stability_and_box_equal_transformers():
    hf = _hf()
    g = np.random.default_rng(5)
    v = (g.standard_normal((6, 17, 23)) * 2).astype(F32)
    v[4] = -3.0                                                                        # empty: 0 / 0 and the zero box
    v[5] = 3.0
    st = [ao.plane_stats(p) for p in v]
    mine = ao.stability([s[0] for s in st], [s[2] for s in st])
    with np.errstate(invalid="ignore"):
        theirs = hf._compute_stability_score(torch.from_numpy(v), 0.0, 1.0).numpy()
    assert np.array_equal(mine, theirs.astype(F32), equal_nan=True) and np.isnan(mine[4]) and mine[5] == 1.0
    boxes = hf._batched_mask_to_box(torch.from_numpy(v > 0)).numpy()
    assert np.array_equal(np.asarray([s[3] for s in st]), boxes) and st[4][3] == [0, 0, 0, 0] and st[5][3] == [0, 0, 22, 16]


# ---------------------------------------------------------------------------------------------------- filters and NMS, closed cases
FAR = [[0, 0, 10, 10], [100, 100, 110, 110], [200, 0, 210, 10], [0, 200, 10, 210], [300, 300, 310, 310]]


def test_thresholds_at_or_below_zero_disable_their_filter():
    t = ao.table([0.9, -2.0, 0.1], [0.99, 0.1, float("nan")], FAR[:3])
    assert ao.select(t, 0.0, 0.0, 0.7).tolist() == [0, 2, 1]                           # nothing filtered, NaN stability included
    assert ao.select(t, -1.0, -0.5, 0.7).tolist() == [0, 2, 1]
    assert ao.select(t, 0.5, 0.0, 0.7).tolist() == [0]
    assert ao.select(t, 0.0, 0.05, 0.7).tolist() == [0, 1]                             # NaN dropped once filter 2 is on


def test_strict_and_non_strict_comparison_at_equality():
    a, b = F32(0.88), F32(0.95)
    t = ao.table([a, np.nextafter(a, F32(1)), 0.9, 0.9], [0.99, 0.99, b, np.nextafter(b, F32(0))], FAR[:4])
    # iou == thresh fails (strict), stability == thresh passes, the next float below fails
    assert ao.select(t, float(a), float(b), 0.7).tolist() == [2, 1]


def test_nan_stability_is_dropped_and_skipped_rows_stay_out():
    t = ao.table([0.9, 0.95, 0.99], [float("nan"), 0.97, 0.99], FAR[:3], flags=[0, 0, ao.SKIPPED])
    assert ao.select(t, 0.88, 0.95, 0.7).tolist() == [1]
    assert ao.select(t, 0.0, 0.0, 0.7).tolist() == [1, 0]


def test_score_ties_go_to_the_lower_index():
    same = [[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]]
    t = ao.table([0.9, 0.9, 0.9], [1, 1, 1], same)
    assert ao.select(t, 0.5, 0.5, 0.7).tolist() == [0]                                 # identical boxes: IoU 1 > 0.7
    assert ao.select(t, 0.5, 0.5, 1.0).tolist() == [0, 1, 2]                           # IoU 1 is not > 1: nothing suppressed, index order
    t = ao.table([0.7, 0.9, 0.9, 0.8], [1, 1, 1, 1], FAR[:4])
    assert ao.select(t, 0.5, 0.5, 0.7).tolist() == [1, 2, 3, 0]


def test_iou_exactly_at_the_threshold_is_kept():
    # [0,0,10,10] and [0,0,10,5]: inter 50, union 100: IoU 0.5 exactly
    t = ao.table([0.9, 0.8], [1, 1], [[0, 0, 10, 10], [0, 0, 10, 5]])
    assert ao.select(t, 0.5, 0.5, 0.5).tolist() == [0, 1]
    assert ao.select(t, 0.5, 0.5, float(np.nextafter(F32(0.5), F32(0)))).tolist() == [0]
    # inclusive boxes as floats: [2,3,2,3] (one pixel) has area 0
    assert not ao.box_iou_gt([2, 3, 2, 3], [2, 3, 2, 3], 0.0)


def test_empty_mask_boxes_never_suppress():
    t = ao.table([0.9, 0.8, 0.7], [1, 1, 1], [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 5, 5]])
    assert ao.select(t, 0.5, 0.5, 0.0).tolist() == [0, 1, 2]                           # 0 / 0 and 0 / 25 are not > 0


def test_select_is_the_pairwise_rule_written_out():
    """select evaluates box_iou_gt over arrays; here the same greedy pass one pair at a time"""
    g = np.random.default_rng(3)
    m = 120
    x0, y0 = g.integers(0, 50, m), g.integers(0, 50, m)
    t = ao.table((np.round(g.uniform(0.5, 1.0, m) * 16) / 16), g.uniform(0.8, 1.0, m), np.stack([x0, y0, x0 + g.integers(0, 30, m), y0 + g.integers(0, 30, m)], 1))
    for thr in (0.3, 0.5, 0.7):
        order = sorted((i for i in range(m) if ao.valid_rows(t, 0.6, 0.85)[i]), key=lambda i: (-float(t["iou"][i]), i))
        keep = []
        for i in order:
            if not any(ao.box_iou_gt(t["box"][k], t["box"][i], thr) for k in keep):
                keep.append(i)
        assert 3 < len(keep) < len(order) and ao.select(t, 0.6, 0.85, thr).tolist() == keep


def test_more_rows_than_the_nms_takes():
    m = ao.MAX_ROWS + 1
    with pytest.raises(ValueError):
        ao.select(ao.table(np.zeros(m), np.ones(m), np.zeros((m, 4))), 0, 0, 0.7)


def test_pack_is_the_header_layout():
    from ovmono3d_amd import lib
    from ovmono3d_amd.sam import CAND_WORDS, candidate_fields
    assert C.sizeof(lib.OvmSamCandidate) == 64 == 4 * ao.WORDS and CAND_WORDS == ao.WORDS and lib.OVM_SAM_CAND_SKIPPED == ao.SKIPPED
    assert lib.load().ovm_abi_sizeof(b"OvmSamCandidate") == 64
    t = ao.table([0.5, -1.25], [0.75, float("nan")], [[1, 2, 3, 4], [5, 6, 7, 8]], flags=[0, 1], area=[9, 10])
    rows = ao.pack(t)
    c = lib.OvmSamCandidate.from_buffer_copy(rows[1].tobytes())
    assert c.iou == -1.25 and np.isnan(c.stability) and c.area == 10 and list(c.box) == [5, 6, 7, 8] and c.flags == 1
    f = candidate_fields(rows)
    assert np.array_equal(f["iou"], t["iou"]) and np.array_equal(f["box"], t["box"]) and np.array_equal(f["flags"], t["flags"])


# ---------------------------------------------------------------------------------------------------- the kernel test's fields
_STATS = {}


def _stats(case):
    """(planes, fp64 logits, fp32 logits) of one geometry, computed once"""
    key = ao.stats_id(case)
    if key not in _STATS:
        inp = ao.stats_inputs(case)
        planes = np.concatenate([inp["smooth"], inp["crafted"]])
        _STATS[key] = (planes, ao.stats_logits(case, planes, F64), ao.stats_logits(case, planes, F32))
    return _STATS[key]


@pytest.mark.parametrize("case", ao.STATS_GEOMETRIES, ids=ao.stats_id)
def test_fields_meet_the_condition_and_cut_every_threshold(case):
    planes, v64, v32 = _stats(case)
    H, W = case["hw"]
    for i, v in enumerate(v64):
        band = G.band_of(v, v32[i])                                                                         # per plane: the plane's own fp32 error
        assert ao.left_out_share(v, band) <= ao.MAX_LEFT_OUT, (ao.stats_id(case), i)
        ao.check_counts(ao.as_device(v32[i:i + 1])[0][:3], v, band, tag=f"{ao.stats_id(case)} plane {i}")      # the fp32 run passes its own rule
    for v in v64[:ao.STATS_SMOOTH]:                                                                         # all three thresholds cut the smooth fields
        hi, mid, lo, _ = ao.plane_stats(v)
        assert 0 < hi < mid < lo < H * W or H * W < 20
    n = ao.STATS_SMOOTH
    assert ao.plane_stats(v64[n])[:3] == (0, 0, 0) and ao.plane_stats(v64[n])[3] == [0, 0, 0, 0]
    assert ao.plane_stats(v64[n + 1])[:3] == (H * W,) * 3 and ao.plane_stats(v64[n + 1])[3] == [0, 0, W - 1, H - 1]
    assert ao.plane_stats(v64[n + 2])[:3] == (0, H * W, H * W)
    assert 0 < ao.plane_stats(v64[n + 3])[1] < H * W


# (5, 3) has 15 pixels: a wrong evaluation may count the same there, so the rejection is asked of the other geometries
@pytest.mark.parametrize("mut", ao.STATS_MUTATIONS)
@pytest.mark.parametrize("case", [c for c in ao.STATS_GEOMETRIES if c["hw"] != (5, 3)], ids=ao.stats_id)
def test_count_comparison_rejects_wrong_evaluations(case, mut):
    planes, v64, v32 = _stats(case)
    wrong = ao.as_device(ao.stats_logits(case, planes[:ao.STATS_SMOOTH], F32, mut), mut=mut)
    rejected = 0
    for i in range(ao.STATS_SMOOTH):
        try:
            ao.check_counts(wrong[i][:3], v64[i], G.band_of(v64[i], v32[i]))
        except AssertionError:
            rejected += 1
    assert rejected >= 1, f"{mut} passes the comparison on {ao.stats_id(case)}"


# ---------------------------------------------------------------------------------------------------- refusals
class _NoPredictor:
    def __getattr__(self, name):
        raise AssertionError(f"the predictor was asked for {name}")


@pytest.mark.parametrize("kwargs,name", [(dict(crop_n_layers=1), "crop_n_layers"), (dict(min_mask_region_area=10), "min_mask_region_area"),
                                         (dict(output_mode="coco_rle"), "output_mode"), (dict(output_mode="uncompressed_rle"), "output_mode"),
                                         (dict(point_grids=[np.zeros((4, 2))]), "point_grids"), (dict(points_per_side=None), "points_per_side"),
                                         (dict(points_per_side=37), "points_per_side"),
                                         (dict(points_per_side=None, point_grids=[np.zeros((1366, 2))]), "point_grids"),
                                         (dict(points_per_side=0), "points_per_side"), (dict(points_per_batch=0), "points_per_batch")])
def test_generator_refusals_name_their_argument_before_any_device_call(kwargs, name):
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator
    with pytest.raises(ValueError, match=name):
        SamAutomaticMaskGenerator(_NoPredictor(), **kwargs)


def test_generator_accepts_what_the_rules_allow():
    from ovmono3d_amd.sam import MAX_AUTO_POINTS, SamAutomaticMaskGenerator
    assert MAX_AUTO_POINTS == 1365 and 36 * 36 <= MAX_AUTO_POINTS < 37 * 37
    g = SamAutomaticMaskGenerator(_NoPredictor())
    assert (g.point_grid.shape, g.points_per_batch, g.pred_iou_thresh, g.stability_score_thresh, g.stability_score_offset, g.box_nms_thresh) == \
        ((1024, 2), 64, 0.88, 0.95, 1.0, 0.7)
    assert SamAutomaticMaskGenerator(_NoPredictor(), points_per_side=36).point_grid.shape == (1296, 2)
    own = np.random.default_rng(0).random((1365, 2))
    assert np.array_equal(SamAutomaticMaskGenerator(_NoPredictor(), points_per_side=None, point_grids=[own]).point_grid, own)
    with pytest.raises(RuntimeError):
        g.candidates()


def test_library_refusals_without_a_device():
    from ovmono3d_amd import lib
    L = lib.load()
    n = C.c_int64(-7)
    assert L.ovm_sam_auto_candidates_workspace(None, 1, C.byref(n)) == -1 and n.value == -7
    assert L.ovm_sam_auto_candidates(None, None, 1, 0.88, 1.0, None, None, 0, None) == -1
    assert L.ovm_sam_auto_select_workspace(4096, C.byref(n)) == 0 and n.value >= 4096 * 24
    assert L.ovm_sam_auto_select_workspace(-1, C.byref(n)) == -1
    nk = C.c_int32(-5)
    assert L.ovm_sam_auto_select(None, 4097, 0.88, 0.95, 0.7, None, C.byref(nk), None, 0, None) == lib.OVM_ERR_CAPACITY and nk.value == -5
    assert L.ovm_sam_auto_select(None, -1, 0.88, 0.95, 0.7, None, C.byref(nk), None, 0, None) == -1
    buf = (C.c_float * 16)()
    out = (C.c_int32 * 7)(*([-9] * 7))
    S = lib.OVM_ERR_SHAPE
    for geo in ((32, 128, 129, 100, 70, 100), (32, 128, 90, 0, 70, 100), (0, 128, 90, 128, 70, 100), (32, 16, 9, 16, 70, 100), (32, 8192, 4097, 8192, 70, 100),
                (32, 128, 90, 128, 0, 100), (32, 128, 90, 128, 65536, 32768)):
        assert L.ovm_op_sam_mask_stats(buf, 1024, 1, *geo, 1.0, None, out, None) == S, geo
    assert L.ovm_op_sam_mask_stats(buf, 1023, 1, 32, 128, 90, 128, 70, 100, 1.0, None, out, None) == S           # planes would overlap
    assert L.ovm_op_sam_mask_stats(buf, 1024, 65536, 32, 128, 90, 128, 70, 100, 1.0, None, out, None) == S
    assert L.ovm_op_sam_mask_stats(None, 1024, 1, 32, 128, 90, 128, 70, 100, 1.0, None, out, None) == -1
    assert list(out) == [-9] * 7


EVERYTHING = ["--input-folder", "none", "--everything", "--depth", "files", "--depth-dir", "d"]


@pytest.mark.parametrize("extra,msg", [(["--mask", "box"], "needs --mask sam"), (["--sam-weights", "w", "--points-file", "p.json"], "neither --points-file nor --boxes-file"),
                                       (["--sam-weights", "w", "--boxes-file", "b.json"], "neither --points-file nor --boxes-file"),
                                       (["--sam-weights", "w", "--points-per-side", "37"], "--points-per-side"), ([], "--mask sam needs --sam-weights")])
def test_everything_refusals_of_demo_geo(extra, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), *EVERYTHING, *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, r.stderr[-600:]


def test_demo_geo_without_everything_still_asks_for_labels():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--input-folder", "none", "--depth", "files", "--depth-dir", "d"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "the following arguments are required: --labels-file (or --points-file)" in r.stderr
    assert "--everything" in subprocess.run([sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--help"], capture_output=True, text=True, timeout=120).stdout


def test_package_still_does_not_import_transformers():
    code = ("import sys; import ovmono3d_amd.sam as s; s.SamAutomaticMaskGenerator(None, points_per_side=4); "
            "assert 'transformers' not in sys.modules, 'transformers imported'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
