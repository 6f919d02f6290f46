"""Oriented-box pairs for the 3D IoU tests (tests/test_box3d_oracle.py on the CPU, tests/test_gpu_box3d_iou.py against the
HIP kernel): a distance x size x rotation sweep, closed forms, degenerate ground truth. Every box comes back as the
fp32-rounded corners the kernel sees, widened to float64 for the oracle."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

from oracle import box3d as ob

DISTANCES = (1.0, 3.0, 10.0, 30.0, 60.0, 100.0)
SIZES = {"3-10cm": (0.03, 0.10), "0.2-0.6m": (0.2, 0.6), "1-3m": (1.0, 3.0), "4-12m": (4.0, 12.0), "thin": None}
ROTATIONS = ("yaw", "full")
PAIRS_PER_ROW = 25
SHIFTS = (0.0, 10.0, 50.0, 100.0)


def f32(c) -> np.ndarray:
    """What the kernel sees, as float64."""
    return np.asarray(c, np.float64).astype(np.float32).astype(np.float64)


def gate(a: np.ndarray, b: np.ndarray) -> float:
    """|IoU error| allowed for a pair: 2e-5 when the smaller box's smallest dimension is at least 0.2 m, else 2.5e-4."""
    small = a if ob.box_volume(a) <= ob.box_volume(b) else b
    edges = [np.linalg.norm(small[1] - small[0]), np.linalg.norm(small[3] - small[0]), np.linalg.norm(small[4] - small[0])]
    return 2e-5 if min(edges) >= 0.2 else 2.5e-4


def _rotation(g, kind: str) -> np.ndarray:
    if kind == "yaw":                                                          # camera frame: yaw turns about y
        return Rotation.from_euler("y", g.uniform(-np.pi, np.pi)).as_matrix()
    axis = g.normal(size=3)
    return Rotation.from_rotvec(axis / np.linalg.norm(axis) * g.uniform(0.2, np.pi)).as_matrix()


def _pair(g, dist: float, size: str, rot: str):
    """A box at `dist` metres from the camera, off the optical axis by a lateral offset of either sign, and a perturbed
    copy of it: centre moved by ~12 % of each dimension, dimensions scaled by up to 15 %, turned by a small angle."""
    d = np.array([g.choice([-1.0, 1.0]) * g.uniform(0.05, 0.6), g.choice([-1.0, 1.0]) * g.uniform(0.02, 0.25), 1.0])
    centre = dist * d / np.linalg.norm(d)
    if size == "thin":
        dims = g.permutation([0.02, 1.0, 2.0]) * g.uniform(0.9, 1.1)
    else:
        dims = g.uniform(*SIZES[size], size=3)
    R = _rotation(g, rot)
    centre2 = centre + R @ (g.normal(0.0, 0.12, 3) * dims)
    dims2 = dims * (1.0 + g.uniform(-0.15, 0.15, 3))
    tilt = 0.15 * dims.min() / dims.max()                                    # a thin box turned far would leave its twin
    if rot == "yaw":
        R2 = Rotation.from_euler("y", g.normal(0.0, tilt)).as_matrix() @ R
    else:
        R2 = Rotation.from_rotvec(g.normal(0.0, tilt, 3)).as_matrix() @ R
    return f32(ob.make_box(centre, dims, R)), f32(ob.make_box(centre2, dims2, R2))


def sweep_rows(distances=DISTANCES, seed: int = 0):
    """[(distance, size, rotation, dt [P,8,3], gt [P,8,3])], PAIRS_PER_ROW pairs a row, seeded per row."""
    rows = []
    for di, dist in enumerate(distances):
        for si, size in enumerate(SIZES):
            for ri, rot in enumerate(ROTATIONS):
                g = np.random.default_rng([seed, di, si, ri])
                pairs = [_pair(g, dist, size, rot) for _ in range(PAIRS_PER_ROW)]
                rows.append((dist, size, rot, np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])))
    return rows


def shifted(c: np.ndarray, s: float) -> np.ndarray:
    """The boxes moved `s` metres along the optical axis, rounded to fp32 again."""
    return f32(np.asarray(c, np.float64) + np.array([0.0, 0.0, s]))


def _relabel_90(c: np.ndarray) -> np.ndarray:
    """The same box with its corners relabelled by a quarter turn about its third axis: the same points, another order."""
    unit = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64) - 0.5
    turned = unit @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64).T
    perm = [int(np.argmin(np.abs(unit - t).sum(1))) for t in turned]
    assert sorted(perm) == list(range(8))
    return c[perm]


def closed_forms(dist: float):
    """[(name, dt [8,3], gt [8,3], IoU)] for a box `dist` metres from the camera. The shared-face and gap cases build the
    second box from the first one's rounded corners, so the shared face is the same four points."""
    R = Rotation.from_euler("yx", [25.0, 8.0], degrees=True).as_matrix()
    centre = np.array([0.2, 0.05, 1.0]) * dist
    dims = np.array([1.6, 1.2, 0.8])
    a = f32(ob.make_box(centre, dims, R))
    out = [("identical", a, a.copy(), 1.0), ("relabelled", a, _relabel_90(a), 1.0)]
    inner_dims = np.array([0.5, 0.4, 0.3])
    inner = f32(ob.make_box(centre + R @ [0.3, -0.2, 0.1], inner_dims, R @ Rotation.from_euler("z", 30, degrees=True).as_matrix()))
    out.append(("nested", a, inner, float(np.prod(inner_dims) / np.prod(dims))))
    up = a[4:8] - a[0:4]                                                       # the box's third edge, per corner
    out.append(("stacked", a, f32(np.concatenate([a[4:8], a[4:8] + up])), 0.0))
    out.append(("stacked_below", a, f32(np.concatenate([a[0:4] - up, a[0:4]])), 0.0))
    along = a[1] - a[0]
    out.append(("half_overlap", a, f32(a + 0.5 * along), 1.0 / 3.0))
    out.append(("gap", a, f32(a + (1.0 + 1e-3) * along), 0.0))
    cube = f32(ob.make_box(centre, [1.0, 1.0, 1.0], R))
    turned = f32(ob.make_box(centre, [1.0, 1.0, 1.0], R @ Rotation.from_euler("z", 45, degrees=True).as_matrix()))
    octagon = 2.0 * (2 ** 0.5 - 1)                                             # area of the unit square cut by its 45-degree turn
    out.append(("octagon", cube, turned, octagon / (2.0 - octagon)))
    return out


def degenerate_gt():
    """[(name, gt [8,3])]: ground truth the evaluator keeps as ignored. Omni3D writes -1 into the 3D fields of invalid
    annotations, the evaluator turns NaN corners into 0; the flat box and the segment sit among the detections."""
    centre = np.array([0.5, 0.3, 12.0])
    R = Rotation.from_euler("yx", [30.0, 5.0], degrees=True).as_matrix()
    return [("all_minus_one", -np.ones((8, 3))), ("all_zero", np.zeros((8, 3))),
            ("flat", f32(ob.make_box(centre, [2.0, 1.5, 0.0], R))), ("segment", f32(ob.make_box(centre, [2.0, 0.0, 0.0], R)))]


def detections_around(n: int, seed: int, centre=(0.5, 0.3, 12.0)) -> np.ndarray:
    """`n` valid boxes of 0.3-3 m scattered around `centre`, in every orientation."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append(f32(ob.make_box(np.asarray(centre) + g.normal(0.0, 1.0, 3), g.uniform(0.3, 3.0, 3), _rotation(g, "full"))))
    return np.array(out)
