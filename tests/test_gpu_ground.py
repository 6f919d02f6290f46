"""The ground plane and the upright lift on the device (csrc/ground.hip, csrc/geo.hip, ovmono3d_amd/geo) against the numpy restatement
tests/ground_oracle.py. The inputs are its named cases; tests/test_ground_cpu.py holds, on the restatement alone, the conditions under
which the integer results below may be asked to be exact (no point within 1e-9 m of a band, no plane within 1e-9 of a test of step 2,
an eigen-gap of 10 %)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ground_oracle as O

pytestmark = pytest.mark.gpu

_DEVICE_RUNS = {}


def _params(p):
    from ovmono3d_amd.geo import GroundParams
    return GroundParams(**{f: getattr(p, f) for f in ("thresh", "thresh_rel", "max_tilt_deg", "min_share", "max_depth", "hypotheses", "stride",
                                                       "seed", "refine")})


def _run(name, device):
    """(OvmGroundResult, hyp_counts, GroundCall) of a case on the device, computed once."""
    from ovmono3d_amd.geo import GroundCall
    if name not in _DEVICE_RUNS:
        c = O.case(name)
        call = GroundCall(torch.from_numpy(c["scene"]["depth"]).to(device), c["scene"]["K"], _params(c["params"]), want_counts=True).launch()
        _DEVICE_RUNS[name] = (call.read(), call.counts.cpu().numpy().astype(np.int64), call)
    return _DEVICE_RUNS[name]


def _angle(a, b):
    return float(np.linalg.norm(np.cross(np.asarray(a, np.float64), np.asarray(b, np.float64))))


def _compare(name, device):
    """Every integer equal; the hypothesis' plane within 1e-12 (a cross product, a square root and a dot product of values below
    10 m: a few ulp of 1e-15); the plane kept within 1e-9 rad and 1e-9 m: the centroid and scatter sums of n <= 3000 terms differ
    from numpy's by about n 2^-53 relative, about 3e-13, which an eigen-gap of at least 0.1 turns into about 1e-11 - the bound
    leaves two orders. The frame: orthonormal and frame . normal = e_y to 1e-12 (closed form, entries below 1)."""
    got, counts, _ = _run(name, device)
    ref, c = O.reference(name), O.case(name)
    assert c["expect"] is None or ref["status"] == c["expect"]
    bad = np.nonzero(counts != ref["hyp_counts"])[0]
    assert len(bad) == 0, f"{name}: {len(bad)} counts differ, first at {bad[:5]}: {counts[bad[:5]]} vs {ref['hyp_counts'][bad[:5]]}"
    for f in ("status", "n_points", "n_valid_hyp", "best_hyp", "hyp_inliers", "n_inliers"):
        assert getattr(got, f) == ref[f], (name, f, getattr(got, f), ref[f])
    assert np.abs(np.array(got.hyp_normal) - ref["hyp_normal"]).max() <= 1e-12 and abs(got.hyp_offset - ref["hyp_offset"]) <= 1e-12, name
    U = np.array(got.frame).reshape(3, 3)
    if ref["status"] != O.OK:
        assert list(got.frame) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and list(got.normal) == [0.0, 0.0, 0.0] and got.offset == 0.0, name
        return got, ref
    e = (_angle(got.normal, ref["normal"]), abs(got.offset - ref["offset"]), float(np.abs(U - ref["frame"]).max()))
    print(f"{name}: n {got.n_points}, {got.n_valid_hyp} valid hypotheses, best {got.best_hyp} with {got.hyp_inliers}, kept {got.n_inliers}; "
          f"normal {e[0]:.2e} rad, offset {e[1]:.2e} m, frame {e[2]:.2e} from the restatement")
    assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 1e-9, name
    assert abs(np.linalg.norm(got.normal) - 1.0) <= 1e-12
    assert np.abs(U @ U.T - np.eye(3)).max() <= 1e-12 and np.abs(U @ np.array(got.normal) - [0.0, 1.0, 0.0]).max() <= 1e-12, name
    return got, ref


def test_tilted_room(device):
    """47 x 61 at stride 1 - n is no multiple of 64 or 256 - and 100 hypotheses, no multiple of 64; pitch 20, roll 5 degrees, more
    wall than floor; NaN, inf, 0, negative and too deep pixels are dropped. The counts are the restatement's, the -1 entries too."""
    got, ref = _compare("tilted_room", device)
    assert got.status == O.OK and got.n_points % 64 != 0 and (ref["hyp_counts"] == -1).any()
    s = O.case("tilted_room")["scene"]
    assert np.degrees(np.arccos(min(1.0, float(np.array(got.normal) @ s["normal"])))) <= 0.5 and abs(got.offset - s["offset"]) <= 0.01


def test_stride_3(device):
    """50 x 70 at stride 3: rows and columns 0, 3, .. - the last sampled row and column are not the map's last. The points are the
    restatement's: their number, every hypothesis built from three of them by index, and every count over all of them are equal."""
    got, _ = _compare("stride3", device)
    assert got.n_points == 17 * 24 and got.status == O.OK


def test_ceiling_dominant(device):
    """Looking up: the ceiling is the largest surface and the floor about 17 % of the points. The floor is found; no hypothesis on
    the ceiling is valid (d <= 0; test_ground_cpu.py shows that the -1 entries cover them). With min_share 0.3 the same best
    hypothesis is refused: NO_PLANE, the identity for a frame. 2048 hypotheses: two LDS chunks of planes."""
    got, _ = _compare("ceiling", device)
    s = O.case("ceiling")["scene"]
    assert got.status == O.OK and np.degrees(np.arccos(min(1.0, float(np.array(got.normal) @ s["normal"])))) <= 0.5
    refused, ref = _compare("ceiling_share", device)
    assert refused.status == O.NO_PLANE and refused.best_hyp == got.best_hyp and refused.hyp_inliers == got.hyp_inliers and refused.n_inliers == 0


@pytest.mark.parametrize("name", ["three_points", "two_points", "collinear", "hyp1", "hyp1100"])
def test_degenerate_inputs(device, name):
    """Exactly 3 points; 2 points (TOO_FEW); a 1 x 64 map of collinear points (NO_PLANE, no valid hypothesis); 1 hypothesis; 1100
    hypotheses, one more LDS chunk than 1024 planes fill."""
    got, ref = _compare(name, device)
    if name == "three_points":
        assert (got.status, got.n_points, got.n_inliers) == (O.OK, 3, 3)
    if name == "two_points":
        assert (got.status, got.n_points, got.n_valid_hyp, got.best_hyp) == (O.TOO_FEW, 2, 0, -1)
    if name == "collinear":
        assert (got.status, got.n_points, got.n_valid_hyp) == (O.NO_PLANE, 64, 0)
    if name == "hyp1100":
        assert got.status == O.OK and got.best_hyp >= 0


def _raw_call(L, lib, depth, K, p, res, counts, ws, nbytes):
    Kd = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9).tolist()) if K is not None else None
    return L.ovm_geo_ground_plane(depth.data_ptr() if depth is not None else None, depth.shape[0] if depth is not None else 47,
                                  depth.shape[1] if depth is not None else 61, Kd, C.byref(p) if p is not None else None, res.data_ptr(),
                                  counts.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)


def test_determinism_bounds_and_refusals(device):
    """Two runs give the same bytes; with the workspace, the result and the counts each followed by a sentinel-filled tail, the
    tails are untouched; a refused call writes nothing at all."""
    from ovmono3d_amd import lib
    L = lib.load()
    c = O.case("hyp1100")
    depth = torch.from_numpy(c["scene"]["depth"]).to(device)
    p = _params(c["params"]).to_c()
    nb = C.c_int64()
    assert L.ovm_geo_ground_workspace(depth.shape[0], depth.shape[1], C.byref(p), C.byref(nb)) == 0
    nbytes, rsize, tail = int(nb.value), C.sizeof(lib.OvmGroundResult), 4096
    runs = []
    for fill in (0xA5, 0x3C):
        ws = torch.full((nbytes + tail,), fill, dtype=torch.uint8, device=device)
        res = torch.full((rsize + tail,), fill, dtype=torch.uint8, device=device)
        counts = torch.full((p.hypotheses + tail // 4,), -7 - fill, dtype=torch.int32, device=device)
        assert _raw_call(L, lib, depth, c["scene"]["K"], p, res, counts, ws, nbytes) == 0
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == fill).all()) and bool((res[rsize:] == fill).all()) and bool((counts[p.hypotheses:] == -7 - fill).all())
        runs.append((res[:rsize].cpu().numpy().tobytes(), counts[:p.hypotheses].cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    assert runs[0][0] == bytes(_run("hyp1100", device)[0])
    # refusals: nothing is written
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=device)
    res = torch.full((rsize,), 0xA5, dtype=torch.uint8, device=device)
    counts = torch.full((p.hypotheses,), -9, dtype=torch.int32, device=device)
    bad = _params(c["params"]).to_c()
    bad.hypotheses = 5000
    assert _raw_call(L, lib, depth, c["scene"]["K"], p, res, counts, ws, nbytes - 1) == lib.OVM_ERR_CAPACITY
    assert _raw_call(L, lib, depth, None, p, res, counts, ws, nbytes) == lib.OVM_ERR_INVALID
    assert _raw_call(L, lib, None, c["scene"]["K"], p, res, counts, ws, nbytes) == lib.OVM_ERR_INVALID
    assert _raw_call(L, lib, depth, c["scene"]["K"], None, res, counts, ws, nbytes) == lib.OVM_ERR_INVALID
    assert _raw_call(L, lib, depth, c["scene"]["K"], bad, res, counts, ws, nbytes) == lib.OVM_ERR_INVALID
    Kbad = c["scene"]["K"].copy()
    Kbad[1, 1] = np.inf
    assert _raw_call(L, lib, depth, Kbad, p, res, counts, ws, nbytes) == lib.OVM_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((res == 0xA5).all()) and bool((counts == -9).all())


def _cuboid_mask(s, max_depth=6.0):
    d = s["depth"]
    with np.errstate(invalid="ignore"):
        return ((s["surface"] == O.CUBOID) & np.isfinite(d) & (d > 0) & (d <= max_depth)).astype(np.uint8)


def test_no_frame_and_the_identity_frame_are_the_level_lift(device):
    """frame=None is ovm_geo_lift itself; a frame that holds the identity gives its bytes (1 p_x + 0 p_y + 0 p_z is p_x)."""
    from ovmono3d_amd import lib
    from ovmono3d_amd.geo import LiftCall
    L = lib.load()
    s = O.case("tilted_room")["scene"]
    depth, mask = torch.from_numpy(np.nan_to_num(s["depth"], nan=3.0, posinf=3.0)).to(device), torch.from_numpy(_cuboid_mask(s)).to(device)
    boxes = np.array([[0.0, 0.0, 0.0, 0.0], [5.2, 20.0, 40.7, 46.0]])
    call = LiftCall(depth, s["K"], boxes_xyxy=boxes, masks=[mask, None], want_labels=True)
    call.launch()
    plain, plain_labels = call.read()
    assert [r.status for r in plain] == [0, 0] and plain[1].n_points > 256
    assert L.ovm_geo_lift(call.depth.data_ptr(), call.H, call.W, call.K, call.inst, call.n, C.byref(call.params), call.res.data_ptr(),
                          call.labels.data_ptr(), call.ws.data_ptr(), call.nbytes, torch.cuda.current_stream().cuda_stream) == 0
    old, old_labels = call.read()
    eye = LiftCall(depth, s["K"], boxes_xyxy=boxes, masks=[mask, None], want_labels=True, frame=torch.eye(3, dtype=torch.float64, device=device).reshape(9))
    eye.launch()
    turned, turned_labels = eye.read()
    for a, b, c_ in zip(plain, old, turned):
        assert bytes(a) == bytes(b) == bytes(c_)
    for a, b, c_ in zip(plain_labels, old_labels, turned_labels):
        assert np.array_equal(a, b) and np.array_equal(a, c_)
    with pytest.raises(ValueError):
        LiftCall(depth, s["K"], boxes_xyxy=boxes, frame=torch.eye(3, device=device).reshape(9))                # float32


def test_upright_lift_on_the_tilted_room(device):
    """The cuboid's mask lifted in the fitted frame, the frame handed over on the device with no read in between. Against the
    restatement in the restatement's own frame: the bounds of tests/test_gpu_geo.py, 1e-7 on the result's fields and 1e-6 on the
    box's (the two frames differ by 1e-9 at most, see _compare). The box's vertical axis is the plane's normal to 1e-9; its
    dimensions are closer to the cuboid's than the level lift's.

    height_above_ground: the box's bottom is its lowest sample on the cuboid. That sample lies above the floor by at most the spacing
    of samples up a vertical face, (r / f) / cos(elevation) with r <= 2.7 m, f = 60 px and an elevation below 40 degrees: 5.9 cm,
    plus 4 sigma of the 3 mm noise: 7.1 cm; and below it by at most those 4 sigma plus the 1 cm the plane's offset may be off."""
    from ovmono3d_amd.geo import host_box, lift, lift_boxes
    c = O.case("tilted_room")
    s, ground_ref = c["scene"], O.reference("tilted_room")
    ground, _, call = _run("tilted_room", device)
    mask = _cuboid_mask(s)
    assert mask.sum() >= 300
    depth = call.depth                                                       # the spoiled pixels lie outside the mask
    planes = [torch.from_numpy(mask).to(device)]
    (got,), _ = lift(depth, s["K"], masks=planes, frame=call)
    ref = O.lift_points_frame(s["depth"], mask, s["K"], ground_ref["frame"])
    assert (got.status, got.n_points, got.n_used, got.n_kept, got.trial) == (0, ref["n_points"], ref["n_used"], ref["n_kept"], ref["trial"])
    assert ref["eig"][1] / ref["eig"][0] >= 1.5
    e = max(np.abs(np.array(got.offset) - ref["offset"]).max(), abs(got.yaw - ref["yaw"]), np.abs(np.array(got.ext_min) - ref["ext_min"]).max(),
            np.abs(np.array(got.ext_max) - ref["ext_max"]).max())
    assert e <= 1e-7, e
    box, rbox = host_box(got, s["K"], list(ground.frame)), O.box_of_frame(ref, s["K"], ground_ref["frame"])
    for f in ("center_cam", "dimensions", "pose", "center_2D", "depth"):
        assert np.abs(np.asarray(box[f]) - np.asarray(rbox[f])).max() <= 1e-6, f
    assert np.abs(np.asarray(box["bbox3D"], np.float64) - rbox["bbox3D"]).max() <= 4 * np.spacing(np.float32(np.abs(rbox["bbox3D"]).max()))
    up_cam = np.array(ground.normal) * [1.0, -1.0, -1.0]
    assert _angle(np.asarray(box["pose"])[:, 1], up_cam) <= 1e-9
    # against the level lift, and against the cuboid that was rendered
    level, upright = lift_boxes(depth, s["K"], masks=planes)[0], lift_boxes(depth, s["K"], masks=planes, frame=call)[0]
    assert "height_above_ground" not in level and upright["dimensions"] == box["dimensions"] and upright["pose"] == box["pose"]
    truth = np.array(s["cuboid"]["dims"])
    err_level, err_upright = np.abs(np.array(level["dimensions"]) - truth), np.abs(np.array(upright["dimensions"]) - truth)
    print(f"dimensions (W, H, L): level {level['dimensions']}, upright {upright['dimensions']}, rendered {truth.tolist()}; "
          f"height above ground {upright['height_above_ground']:.4f} m")
    assert err_upright.sum() < err_level.sum() and err_upright[1] < err_level[1]
    assert abs(upright["height_above_ground"] - O.height_above_ground(rbox, ground_ref["normal"], ground_ref["offset"])) <= 1e-6
    assert -(4 * O.NOISE + 0.01) <= upright["height_above_ground"] <= (2.7 / 60.0) / np.cos(np.deg2rad(40.0)) + 4 * O.NOISE
    # a frame without its plane: upright, but no height; no plane: the level records
    bare = lift_boxes(depth, s["K"], masks=planes, frame=call.frame.clone())[0]
    assert "height_above_ground" not in bare and bare["dimensions"] == upright["dimensions"]
    none = _run("ceiling_share", device)[2]
    s2 = O.case("ceiling_share")["scene"]
    d2 = torch.from_numpy(s2["depth"]).to(device)
    assert lift_boxes(d2, s2["K"], boxes_xyxy=[[4.0, 30.0, 30.0, 60.0]], frame=none) == lift_boxes(d2, s2["K"], boxes_xyxy=[[4.0, 30.0, 30.0, 60.0]])
