"""The 3D IoU kernel `ovm_box3d_iou` against the float64 oracle where fp32 goes wrong: boxes from 3 cm to 12 m at 1 to
100 m from the camera, thin boxes, touching, nested and turned boxes, degenerate ground truth, every launch shape; and AP3D
of the evaluator against the same evaluation on the oracle's IoU. The oracle always gets the fp32-rounded corners the kernel
sees (tests/box3d_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import box3d_cases as bc
from oracle import box3d as ob

pytestmark = pytest.mark.gpu

_GUARD = 256                                                                   # words after each output that must stay untouched


def _kernel(dt, gt, device):
    """(iou [N,M], vol [N,M]) from one ovm_box3d_iou launch with the evaluator's screening thresholds."""
    from ovmono3d_amd import lib
    L = lib.load()
    d = torch.tensor(np.asarray(dt, np.float32).reshape(-1, 24), device=device)
    g = torch.tensor(np.asarray(gt, np.float32).reshape(-1, 24), device=device)
    N, M = d.shape[0], g.shape[0]
    iou = torch.full((N * M + _GUARD,), -7.0, dtype=torch.float32, device=device)
    vol = torch.full((N * M + _GUARD,), -7.0, dtype=torch.float32, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.check(L.ovm_box3d_iou(d.data_ptr(), g.data_ptr(), N, M, 1e-4, 1e-8, iou.data_ptr(), vol.data_ptr(), stream), what="ovm_box3d_iou")
    iou, vol = iou.cpu().numpy(), vol.cpu().numpy()
    assert (iou[N * M:] == -7.0).all() and (vol[N * M:] == -7.0).all(), "write past the N x M outputs"
    return iou[:N * M].reshape(N, M).astype(np.float64), vol[:N * M].reshape(N, M).astype(np.float64)


def _check_pairs(dt, gt, device, what):
    """Kernel vs oracle on pairs dt[k], gt[k]: (oracle IoU, max |IoU error|, failures) with the per-pair gate of
    box3d_cases.gate; every IoU of the N x N launch must lie in [0, 1]."""
    iou, vol = _kernel(dt, gt, device)
    fails = [] if np.isfinite(iou).all() and (iou >= 0).all() and (iou <= 1).all() else [f"{what}: IoU outside [0, 1]: {iou.min()} .. {iou.max()}"]
    got, got_vol = np.diag(iou), np.diag(vol)
    ref = np.array([ob.iou_matrix(d[None], g[None])[0, 0] for d, g in zip(dt, gt)])
    ref_vol = np.array([ob.intersection_volume(d, g) for d, g in zip(dt, gt)])
    gates = np.array([bc.gate(d, g) for d, g in zip(dt, gt)])
    err = np.abs(got - ref)
    if (err > gates).any():
        fails.append(f"{what}: IoU error {err.max():.2e} > {gates[np.argmax(err / gates)]:.1e}")
    # the intersection volume itself (nothing in the evaluator reads it), where it is not a sliver of the smaller box
    small = np.minimum([ob.box_volume(d) for d in dt], [ob.box_volume(g) for g in gt])
    solid = ref_vol > 0.05 * small
    vol_err = np.abs(got_vol[solid] - ref_vol[solid]) / ref_vol[solid]
    if solid.any() and vol_err.max() > 1e-4:
        fails.append(f"{what}: relative volume error {vol_err.max():.2e}")
    return ref, err.max(), fails


def test_distance_size_rotation_sweep(device):
    """Boxes of 3-10 cm, 0.2-0.6 m, 1-3 m, 4-12 m and thin 0.02 x 1 x 2 m slabs, 1 to 100 m out, yaw-only and full 3D
    rotations: |IoU error| <= 2e-5 where the smaller box's smallest side is >= 0.2 m, else <= 2.5e-4; every IoU in [0, 1]."""
    fails, worst = [], []
    for dist, size, rot, dt, gt in bc.sweep_rows():
        ref, err, f = _check_pairs(dt, gt, device, f"{dist:g} m {size} {rot}")
        assert ((ref > 0.05) & (ref < 0.95)).sum() >= 15, f"{dist:g} m {size} {rot}: the row has too few real overlaps"
        fails += f
        worst.append(f"{dist:g} m {size} {rot}: {err:.1e}")
    assert not fails, "\n".join(fails + ["max |IoU error| per row:"] + worst)


@pytest.mark.parametrize("shift", bc.SHIFTS)
def test_translation_invariance(device, shift):
    """The 1 m rows of the sweep moved 0, 10, 50 and 100 m along the optical axis: the same gate against the oracle."""
    fails = []
    for dist, size, rot, dt, gt in bc.sweep_rows(distances=(1.0,)):
        fails += _check_pairs(bc.shifted(dt, shift), bc.shifted(gt, shift), device, f"1 m + {shift:g} m {size} {rot}")[2]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dist", [3.0, 80.0])
def test_closed_forms(device, dist):
    """Identical and relabelled boxes -> 1 (never above), nested -> volume ratio, stacked on a shared face -> 0, half overlap
    -> 1/3, a gap of 1e-3 x size -> 0, a cube against its 45-degree turn -> the octagon value; in both argument orders."""
    fails = []
    for name, a, b, want in bc.closed_forms(dist):
        for order, (d, g) in (("dt, gt", (a, b)), ("gt, dt", (b, a))):
            got = _kernel(d[None], g[None], device)[0][0, 0]
            if not (abs(got - want) <= 2e-5 and got <= 1.0):
                fails.append(f"{name} ({order}) at {dist:g} m: {got!r}, want {want:.6f}")
            if name == "gap" and got != 0.0:
                fails.append(f"gap ({order}) at {dist:g} m: {got!r}, want exactly 0")
    assert not fails, "\n".join(fails)


def test_degenerate_ground_truth_intersects_nothing(device):
    """All -1 (Omni3D's invalid 3D fields), all 0 (NaN corners after the evaluator's nan_to_num), a flat box and a segment
    lying among 200 valid detections: IoU and intersection volume exactly 0 for every pair."""
    dt = bc.detections_around(200, seed=3)
    names, gt = zip(*bc.degenerate_gt())
    iou, vol = _kernel(dt, np.array(gt), device)
    bad = [f"{n}: {int((iou[:, j] != 0).sum())} IoU != 0 (max {iou[:, j].max():.3g}), {int((vol[:, j] != 0).sum())} volumes != 0"
           for j, n in enumerate(names) if (iou[:, j] != 0).any() or (vol[:, j] != 0).any()]
    assert not bad, "\n".join(bad)
    for j in range(len(gt)):                                                   # the oracle agrees
        assert ob.box_volume(gt[j]) == 0.0 and all(ob.intersection_volume(d, gt[j]) == 0.0 for d in dt[:20])


def _tile_sources():
    """40 distinct detections and 30 distinct ground truths, at 2-90 m, many pairs overlapping."""
    g = np.random.default_rng(11)
    rows = bc.sweep_rows(distances=(2.0, 20.0, 90.0), seed=5)
    gt = np.concatenate([r[4][:2] for r in rows])[:30]
    dt = np.concatenate([np.concatenate([r[3][:2] for r in rows])[:30], bc.detections_around(10, seed=12)])
    return dt[g.permutation(40)], gt


@pytest.mark.parametrize("n,m", [(1, 1), (1, 300), (257, 129), (2000, 150)])
def test_launch_shapes(device, n, m):
    """Grids tiled from 40 x 30 distinct boxes: expected[i, j] = ref[i % 40, j % 30]; nothing written past N x M."""
    dt, gt = _tile_sources()
    ref = ob.iou_matrix(dt, gt)
    assert (ref > 0.05).sum() >= 20
    got = _kernel(dt[np.arange(n) % 40], gt[np.arange(m) % 30], device)[0]
    want = ref[np.ix_(np.arange(n) % 40, np.arange(m) % 30)]
    assert np.abs(got - want).max() <= 2.5e-4, np.abs(got - want).max()
    small = _kernel(dt, gt, device)[0]                                         # each pair's value does not depend on where it sits
    assert np.array_equal(got, small[np.ix_(np.arange(n) % 40, np.arange(m) % 30)])


# ---------------------------------------------------------------- AP3D of the evaluator ------------------------------------------
def _scene(kind, seed):
    """Ground truth and detections for 6 images, 2 categories. Objects of a cell sit apart from each other (every detection
    overlaps at most its own ground truth), each true IoU is at least 1e-3 from every threshold 0.05 .. 0.50, and every
    cell holds ignored ground truth with -1 and with NaN corners next to unmatched detections of high score."""
    from scipy.spatial.transform import Rotation
    g = np.random.default_rng(seed)
    thrs = np.linspace(0.05, 0.5, 10)
    gts, dts = [], []

    def rec(img, cat, corners, depth, **kw):
        return {"image_id": img, "category_id": cat, "bbox": [0.0, 0.0, 10.0, 10.0], "bbox3D": np.asarray(corners).tolist(), "depth": float(depth), **kw}

    for img in range(1, 7):
        for cat in (0, 1):
            slots = g.permutation(12)[:7]
            for k, slot in enumerate(slots):
                if kind == "kitti":                                            # pedestrians / cones and cars, 20 - 90 m
                    depth = 20.0 + 5.8 * slot + g.uniform(0, 1)
                    centre = np.array([g.uniform(-0.3, 0.3) * depth, g.uniform(0.01, 0.05) * depth, depth])
                    dims = g.uniform(0.3, 0.8, 3) if cat == 0 else np.array([1.6, 1.5, 4.0]) * g.uniform(0.9, 1.1, 3)
                    R = Rotation.from_euler("y", g.uniform(-np.pi, np.pi)).as_matrix()
                else:                                                          # mugs, remotes, books: 3 - 30 cm at 1 - 8 m
                    depth = 1.0 + 0.58 * slot + g.uniform(0, 0.05)
                    centre = np.array([g.uniform(-0.4, 0.4) * depth, g.uniform(-0.2, 0.2) * depth, depth])
                    dims = g.uniform(0.03, 0.3, 3)
                    R = Rotation.from_rotvec(g.normal(size=3)).as_matrix()
                box = bc.f32(ob.make_box(centre, dims, R))
                gts.append(rec(img, cat, box, depth))
                if k >= 5:                                                     # missed
                    continue
                while True:                                                    # a detection whose IoU is clear of every threshold
                    scale = g.uniform(0.0, 0.45)
                    dbox = bc.f32(ob.make_box(centre + R @ (g.normal(0, scale, 3) * dims), dims * (1 + g.uniform(-scale, scale, 3)),
                                              Rotation.from_euler("y", g.normal(0, scale)).as_matrix() @ R))
                    v = ob.iou_matrix(dbox[None], box[None])[0, 0]
                    if np.abs(v - thrs).min() >= 1e-3:
                        break
                dts.append(rec(img, cat, dbox, depth, score=float(g.uniform(0.05, 0.9))))
            far = np.array([0.0, 0.0, 1.0]) * (150.0 if kind == "kitti" else 12.0)
            for _ in range(3):                                                 # false positives nowhere near any ground truth
                fp = bc.f32(ob.make_box(far + g.normal(0, 0.1 * far[2], 3), dims, Rotation.from_rotvec(g.normal(size=3)).as_matrix()))
                dts.append(rec(img, cat, fp, far[2], score=float(g.uniform(0.9, 1.0))))
            gts.append(rec(img, cat, -np.ones((8, 3)), -1.0, ignore3D=1))
            gts.append(rec(img, cat, np.full((8, 3), np.nan), -1.0, ignore3D=1))
    return gts, dts


@pytest.mark.parametrize("kind", ["kitti", "indoor"])
def test_ap3d_equals_the_oracle_evaluation(device, kind, monkeypatch):
    """Omni3Deval in 3D mode on the kernel vs the same evaluation on the float64 oracle's IoU: precision and recall tables
    equal exactly. Ignored ground truth without volume must not absorb the unmatched detections (a false positive that
    matches it would be ignored and lift AP3D)."""
    from ovmono3d_amd.evaluation import omni3d_eval
    gts, dts = _scene(kind, seed=21 if kind == "kitti" else 22)

    def run():
        e = omni3d_eval.Omni3Deval(gts, dts, "3D", device=device)
        e.evaluate(); e.accumulate()
        return e

    got = run().eval

    def oracle_overlap(bd, bg, eps_coplanar=1e-4, eps_nonzero=1e-8):
        return torch.tensor(ob.iou_matrix(bd.cpu().double().numpy(), bg.cpu().double().numpy()))
    monkeypatch.setattr(omni3d_eval, "box3d_overlap", oracle_overlap)
    e = run()
    want = e.eval
    thrs = e.params.iouThrs
    assert min(np.abs(c.iou[..., None] - thrs).min() for c in e.cells.values() if c.iou.size) >= 1e-3
    assert ((want["precision"] > 0) & (want["precision"] < 1)).sum() > 100    # real curves at several thresholds
    assert len(np.unique(want["recall"][:, :, 0, -1])) > 3
    assert np.array_equal(got["recall"], want["recall"]), np.abs(got["recall"] - want["recall"]).max()
    assert np.array_equal(got["precision"], want["precision"]), np.abs(got["precision"] - want["precision"]).max()
