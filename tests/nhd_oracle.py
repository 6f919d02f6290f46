"""fp64 restatement of the disentangled NHD (ovmono3d_amd/evaluation/nhd.py) and the cuboid pairs the NHD tests share
(tests/test_eval3d_cpu.py without a GPU, tests/test_gpu_eval3d.py against the HIP kernel ``ovm_eval_nhd``).

The oracle rounds the inputs to fp32 exactly where ``nhd.cuboid_corners`` does (centre, dimensions, rotation) and does everything
after that in float64: corners, the 8x8 distances, scipy's assignment, the division by the ground truth's extent. The host path
computes the corners and distances in fp32, so its distance to this oracle is the error the device route is allowed."""
from __future__ import annotations

from itertools import permutations

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.transform import Rotation

COMPONENTS = ("xy", "z", "dimensions", "pose")
KEYS = ("overall",) + COMPONENTS
_SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64)
_PERMS = None


def corners64(xy, z, dimensions, pose) -> np.ndarray:
    w, h, l = (np.float64(np.float32(v)) for v in dimensions)
    half = np.array([l, h, w], dtype=np.float64) / 2.0
    R = np.asarray(pose, dtype=np.float32).reshape(3, 3).astype(np.float64)
    c = np.array([xy[0], xy[1], z], dtype=np.float32).astype(np.float64)
    return (_SIGNS * half) @ R.T + c


def cost64(pred_corners: np.ndarray, gt_corners: np.ndarray) -> np.ndarray:
    return np.linalg.norm(pred_corners[:, None, :] - gt_corners[None, :, :], axis=2)


def extent64(gt_corners: np.ndarray) -> float:
    return float(np.linalg.norm(gt_corners.max(axis=0) - gt_corners.min(axis=0)))


def mixed(pred, gt, comp):
    """``pred`` itself for "overall", else the ground truth with ``comp`` taken from the prediction."""
    if comp == "overall":
        return pred
    return {c: (pred[c] if c == comp else gt[c]) for c in COMPONENTS}


def disentangled_nhd64(pred, gt, solver=None) -> dict:
    gc = corners64(gt["xy"], gt["z"], gt["dimensions"], gt["pose"])
    out = {}
    for key in KEYS:
        m = mixed(pred, gt, key)
        cost = cost64(corners64(m["xy"], m["z"], m["dimensions"], m["pose"]), gc)
        if solver is None:
            rows, cols = linear_sum_assignment(cost)
            total = float(cost[rows, cols].sum())
        else:
            total = solver(cost)
        out[key] = total / extent64(gc)
    return out


def brute_force(cost: np.ndarray) -> float:
    """The minimum over all 8! assignments."""
    global _PERMS
    if _PERMS is None:
        _PERMS = np.array(list(permutations(range(8))), dtype=np.int64)          # [40320, 8]
    return float(cost[np.arange(8)[None, :], _PERMS].sum(axis=1).min())


def subset_dp(cost: np.ndarray) -> float:
    """dp[mask] = min over j in mask of dp[mask without j] + cost[popcount(mask) - 1][j]: the device kernel's recurrence."""
    dp = np.full(256, np.inf)
    dp[0] = 0.0
    for mask in range(1, 256):
        row = bin(mask).count("1") - 1
        dp[mask] = min(dp[mask ^ (1 << j)] + cost[row, j] for j in range(8) if mask >> j & 1)
    return float(dp[255])


def _yaw(a):
    return Rotation.from_euler("y", a).as_matrix()


def random_cuboid(g, depth, lo=0.05, hi=4.0):
    d = np.array([g.choice([-1.0, 1.0]) * g.uniform(0.05, 0.6), g.choice([-1.0, 1.0]) * g.uniform(0.02, 0.25), 1.0])
    c = depth * d / d[2]
    R = _yaw(g.uniform(-np.pi, np.pi)) @ Rotation.from_euler("xz", g.normal(0.0, 0.1, 2)).as_matrix()
    return {"xy": c[:2].tolist(), "z": float(c[2]), "dimensions": g.uniform(lo, hi, 3).tolist(), "pose": R.tolist()}


def perturbed(g, gt):
    """Yaw noise, 3 % depth, 10 % dimensions, and the centre moved sideways by a few percent of the box."""
    dims = np.asarray(gt["dimensions"])
    return {"xy": (np.asarray(gt["xy"]) + g.normal(0.0, 0.05, 2) * dims.mean()).tolist(), "z": float(gt["z"] * (1.0 + g.normal(0.0, 0.03))),
            "dimensions": (dims * (1.0 + g.uniform(-0.1, 0.1, 3))).tolist(),
            "pose": (_yaw(g.normal(0.0, 0.15)) @ np.asarray(gt["pose"])).tolist()}


def pair_set(seed: int = 0):
    """[(pred, gt)]: 180 perturbed pairs at each of 1, 5, 20, 60 and 100 m with extents of 0.05-4 m, then 100 unrelated pairs."""
    g = np.random.default_rng(seed)
    pairs = []
    for depth in (1.0, 5.0, 20.0, 60.0, 100.0):
        for _ in range(180):
            gt = random_cuboid(g, depth)
            pairs.append((perturbed(g, gt), gt))
    for _ in range(100):
        pairs.append((random_cuboid(g, float(g.choice([1.0, 5.0, 20.0, 60.0, 100.0]))), random_cuboid(g, float(g.choice([1.0, 5.0, 20.0, 60.0, 100.0])))))
    return pairs


def as_table(results) -> np.ndarray:
    """[n, 5] in KEYS order from a list of result dicts."""
    return np.array([[r[k] for k in KEYS] for r in results], dtype=np.float64).reshape(-1, 5)


def error_against_oracle(values: np.ndarray, oracle: np.ndarray):
    """(largest absolute, largest relative) difference; the relative one over entries whose oracle value is not 0."""
    diff = np.abs(values - oracle)
    nz = oracle != 0
    return float(diff.max()), float((diff[nz] / np.abs(oracle[nz])).max()) if nz.any() else 0.0
