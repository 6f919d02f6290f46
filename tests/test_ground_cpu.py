"""The ground plane without a GPU: the conditions under which tests/test_gpu_ground.py may ask the device for exact counts, stated on
the numpy restatement alone (tests/ground_oracle.py), and the host side of the feature (defaults, config key, refusals, the box turned
back by ovm_host_geo_box_frame)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import geo_oracle as G
import ground_oracle as O

OK_CASES = [n for n in O.GPU_CASES if O.case(n)["expect"] == O.OK]
ROOMS = [n for n in OK_CASES if O.case(n)["scene"]["normal"] is not None]


@pytest.mark.parametrize("name", O.GPU_CASES)
def test_no_point_hangs_on_its_band(name):
    """Zero (point, plane) pairs within 1e-9 m of the band over all valid hypotheses, 1e-7 m for the refined plane (its normal
    differs from the restatement's by rounding, amplified by at most 1 / eigen-gap). Only then may the device counts be asked to be
    exact. A failure here means: take another seed, never a wider band. The tilt and d > 0 tests get the same margin."""
    c, r = O.case(name), O.reference(name)
    assert c["expect"] is None or r["status"] == c["expect"]
    P, p = r["points"], c["params"]
    tol = O.band(P, p)
    pairs = 0
    for pl in r["planes"]:
        if np.isfinite(pl[3]):
            pairs += int((np.abs(np.abs(O.distances(P, pl)) - tol) <= 1e-9).sum())
    assert pairs == 0
    if r["refined"] is not None:
        assert int((np.abs(np.abs(O.distances(P, r["refined"])) - tol) <= 1e-7).sum()) == 0
        assert abs(r["refined"][1] - np.cos(np.deg2rad(p.max_tilt_deg))) > 1e-7 and abs(r["refined"][3]) > 1e-7
    # the tests of step 2 on every candidate plane, recomputed without them: none within 1e-9 of a threshold
    if len(P) >= 3:
        raw = O.hypotheses(P, p, tests=False)[0]
        raw = raw[np.isfinite(raw[:, 3])]
        cos_tilt = np.cos(np.deg2rad(p.max_tilt_deg))
        assert len(raw) == 0 or np.abs(raw[:, 1] - cos_tilt).min() > 1e-9
        flat = raw[raw[:, 1] >= cos_tilt]                                            # a wall is refused whatever its d
        assert len(flat) == 0 or np.abs(flat[:, 3]).min() > 1e-9


@pytest.mark.parametrize("name", ROOMS)
def test_the_restatement_recovers_the_rendered_floor(name):
    """Within 0.5 degrees and 1 cm of the floor the room was rendered with."""
    s, r = O.case(name)["scene"], O.reference(name)
    angle = np.degrees(np.arccos(min(1.0, float(r["normal"] @ s["normal"]))))
    print(f"{name}: angle {angle:.4f} deg, offset error {abs(r['offset'] - s['offset']) * 1e3:.2f} mm, inliers {r['n_inliers']} of {r['n_points']}")
    assert angle <= 0.5 and abs(r["offset"] - s["offset"]) <= 0.01
    U = r["frame"]
    assert np.abs(U @ U.T - np.eye(3)).max() <= 1e-14 and np.abs(U @ r["normal"] - [0.0, 1.0, 0.0]).max() <= 1e-14


@pytest.mark.parametrize("name", OK_CASES)
def test_the_eigenvector_bound_has_its_gap(name):
    """The inlier scatter matrix' two smaller eigenvalues differ by at least 10 % of the largest: with summation errors of about
    n 2^-53 relative, the smallest eigenvector is then good to about 1e-11 rad, and the GPU test's 1e-9 leaves two orders."""
    w = O.reference(name)["eig"]
    assert (w[1] - w[0]) >= 0.1 * w[2], w


def test_the_cases_cover_what_they_are_for():
    r = O.reference("tilted_room")
    s = O.case("tilted_room")["scene"]
    seen = s["surface"].ravel()[r["pixels"]]
    assert (seen == O.WALL).sum() > (seen == O.FLOOR).sum() > 0                      # the wall covers more than the floor
    assert r["n_points"] % 64 != 0 and r["n_points"] % 256 != 0 and r["n_points"] < 47 * 61
    d = s["depth"]
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and (d < 0).any() and (d[np.isfinite(d)] > 6.0).any()
    assert (r["hyp_counts"] == -1).any() and (r["hyp_counts"] >= 0).any()
    assert np.allclose(r["normal"], r["refined"][:3]) and not np.allclose(O.reference("hyp1100")["normal"], O.reference("hyp1100")["refined"][:3])
    # looking up: the ceiling is the largest surface, the floor about 15 %, and no hypothesis of three ceiling points is valid
    r, s = O.reference("ceiling"), O.case("ceiling")["scene"]
    seen = s["surface"].ravel()[r["pixels"]]
    share = (seen == O.FLOOR).mean()
    assert 0.10 <= share <= 0.20 and (seen == O.CEILING).mean() > 0.4
    on_ceiling = (seen[r["indices"]] == O.CEILING).all(1)
    assert on_ceiling.sum() >= 100 and (r["hyp_counts"][on_ceiling] == -1).all()
    assert (seen[O.inliers(r["points"], np.append(r["normal"], r["offset"]), O.case("ceiling")["params"])] == O.FLOOR).mean() > 0.95
    assert O.reference("ceiling_share")["status"] == O.NO_PLANE and O.reference("ceiling_share")["hyp_inliers"] == r["hyp_inliers"]
    assert O.reference("three_points")["n_points"] == 3 and O.reference("two_points")["status"] == O.TOO_FEW
    assert O.reference("collinear")["n_valid_hyp"] == 0 and O.reference("collinear")["status"] == O.NO_PLANE
    assert O.reference("demo_wall")["status"] == O.NO_PLANE and O.reference("demo_room")["status"] == O.OK


def _mix_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_mix_values():
    listed = {0: 0x00000000, 1: 0x688990c0, 0xdeadbeef: 0xe628c683}
    for x, y in listed.items():
        assert int(O.mix(x)) == y == _mix_int(x)
    idx = O.hypothesis_indices(1000, O.Params(seed=7, hypotheses=5))
    assert idx.tolist() == [[_mix_int(7 * 0x9E3779B9 + 3 * h + j) % 1000 for j in range(3)] for h in range(5)]


def test_defaults_agree_everywhere():
    from ovmono3d_amd import lib
    from ovmono3d_amd.geo import GroundParams
    L = lib.load()
    c = lib.OvmGroundParams()
    assert L.ovm_geo_ground_default_params(C.byref(c)) == 0
    fields = [f.name for f in dataclasses.fields(O.Params)]
    assert fields == [f.name for f in dataclasses.fields(GroundParams)]
    for f in fields:
        assert getattr(c, f) == getattr(O.Params(), f) == getattr(GroundParams(), f), f
    assert bytes(GroundParams().to_c()) == bytes(c)
    assert (c.thresh, c.thresh_rel, c.max_tilt_deg, c.min_share, c.max_depth, c.hypotheses, c.stride, c.seed, c.refine) == \
        (0.02, 0.01, 45.0, 0.10, 0.0, 512, 4, 0, 1)
    assert L.ovm_abi_sizeof(b"OvmGroundParams") == C.sizeof(lib.OvmGroundParams) == 5 * 8 + 4 * 4 + 8
    assert L.ovm_abi_sizeof(b"OvmGroundResult") == C.sizeof(lib.OvmGroundResult) == 17 * 8 + 6 * 4
    assert (lib.OVM_GROUND_OK, lib.OVM_GROUND_TOO_FEW, lib.OVM_GROUND_NO_PLANE) == (O.OK, O.TOO_FEW, O.NO_PLANE)


def test_the_config_key_exists_and_is_off():
    from ovmono3d_amd.defaults import make_cfg
    assert make_cfg("", []).MODEL.AMD.GEO_UPRIGHT is False
    assert make_cfg("", ["MODEL.AMD.GEO_UPRIGHT", "True"]).MODEL.AMD.GEO_UPRIGHT is True


def test_refusals_come_before_any_device_work():
    """Null or inconsistent arguments and a short workspace: the lift's codes, with no device call (this test has no device)."""
    from ovmono3d_amd import lib
    L = lib.load()
    p = lib.OvmGroundParams()
    L.ovm_geo_ground_default_params(C.byref(p))
    nb = C.c_int64(-1)
    assert L.ovm_geo_ground_workspace(480, 640, C.byref(p), C.byref(nb)) == 0 and nb.value > 0
    assert L.ovm_geo_ground_workspace(480, 640, C.byref(p), None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_workspace(0, 640, C.byref(p), C.byref(nb)) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_workspace(480, 640, None, C.byref(nb)) == lib.OVM_ERR_INVALID
    for field, bad in (("hypotheses", 0), ("hypotheses", 4097), ("stride", 0), ("refine", 2), ("max_tilt_deg", 90.0), ("max_tilt_deg", 0.0),
                       ("thresh", -1.0), ("thresh", float("nan")), ("thresh_rel", -0.1), ("min_share", 1.5), ("max_depth", -1.0)):
        q = lib.OvmGroundParams.from_buffer_copy(bytes(p))
        setattr(q, field, bad)
        assert L.ovm_geo_ground_workspace(480, 640, C.byref(q), C.byref(nb)) == lib.OVM_ERR_INVALID, (field, bad)
        assert b"ground" in L.ovm_geo_last_error()
    K = (C.c_double * 9)(500.0, 0, 320, 0, 500, 240, 0, 0, 1)
    fake = 0x1000                                                                    # never dereferenced: every call below is refused
    assert L.ovm_geo_ground_plane(None, 480, 640, K, C.byref(p), fake, None, fake, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, 480, 640, None, C.byref(p), fake, None, fake, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, 480, 640, K, None, fake, None, fake, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, 480, 640, K, C.byref(p), None, None, fake, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, 480, 640, K, C.byref(p), fake, None, None, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, -1, 640, K, C.byref(p), fake, None, fake, nb.value, None) == lib.OVM_ERR_INVALID
    assert L.ovm_geo_ground_plane(fake, 480, 640, K, C.byref(p), fake, None, fake, nb.value - 1, None) == lib.OVM_ERR_CAPACITY
    K0 = (C.c_double * 9)(0.0, 0, 320, 0, 500, 240, 0, 0, 1)
    assert L.ovm_geo_ground_plane(fake, 480, 640, K0, C.byref(p), fake, None, fake, nb.value, None) == lib.OVM_ERR_INVALID


def _result(r):
    from ovmono3d_amd import lib
    g = lib.OvmGeoResult()
    g.offset[:], g.ext_min[:], g.ext_max[:] = r["offset"].tolist(), r["ext_min"].tolist(), r["ext_max"].tolist()
    g.yaw, g.eps, g.n_points, g.n_used, g.n_kept, g.trial, g.status = r["yaw"], r["eps"], r["n_points"], r["n_used"], r["n_kept"], r["trial"], 0
    return g


def test_host_box_frame_against_the_restatement():
    """ovm_host_geo_box_frame on the restatement's own upright lift of the tilted room's cuboid: the fields within 1e-9 (the pose is
    a closed form there and Kabsch here, equal to 4e-16; the rest is a handful of fp64 operations), bbox3D within 4 float32 ulp; NULL
    for a frame, and the plain call, give the same bytes."""
    from ovmono3d_amd import lib
    from ovmono3d_amd.geo import height_above_plane, host_box
    L = lib.load()
    s, g = O.case("tilted_room")["scene"], O.reference("tilted_room")
    mask = ((s["surface"] == O.CUBOID) & np.isfinite(s["depth"]) & (s["depth"] > 0)).astype(np.uint8)
    r = O.lift_points_frame(s["depth"], mask, s["K"], g["frame"])
    ref = O.box_of_frame(r, s["K"], g["frame"])
    got = host_box(_result(r), s["K"], g["frame"].reshape(9))
    for f in ("center_cam", "dimensions", "pose", "center_2D", "depth"):
        assert np.abs(np.asarray(got[f]) - np.asarray(ref[f])).max() <= 1e-9, f
    assert np.abs(np.asarray(got["bbox3D"], np.float64) - ref["bbox3D"]).max() <= 4 * np.spacing(np.float32(np.abs(ref["bbox3D"]).max()))
    assert abs(height_above_plane(got, g["normal"], g["offset"]) - O.height_above_ground(ref, g["normal"], g["offset"])) <= 1e-9
    Kd = (C.c_double * 9)(*s["K"].reshape(9).tolist())
    a, b, c = lib.OvmGeoBox(), lib.OvmGeoBox(), lib.OvmGeoBox()
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert L.ovm_host_geo_box(C.byref(_result(r)), Kd, C.byref(a)) == 0
    assert L.ovm_host_geo_box_frame(C.byref(_result(r)), Kd, None, C.byref(b)) == 0
    assert L.ovm_host_geo_box_frame(C.byref(_result(r)), Kd, eye, C.byref(c)) == 0
    assert bytes(a) == bytes(b)
    level = G.box_of(r["offset"], r["yaw"], r["ext_min"], r["ext_max"], s["K"])
    assert np.abs(np.asarray(list(c.center_cam)) - level["center_cam"]).max() <= 1e-12
