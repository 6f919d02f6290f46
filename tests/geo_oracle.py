"""Restatement of OVMono3D-GEO's 2D-to-3D lifting (reference tools/ovmono3d_geo.py:127-258) in numpy float64 + scipy. A helper,
not a test: it is what the HIP path (ovmono3d_amd/csrc/geo.hip, ovmono3d_amd/geo) is compared with, and itself pinned against
live scikit-learn and a recorded fixture in tests/test_geo_cpu.py.

The steps, quirks included:
 1. points for the mask pixels (mask > 0.5) in row-major order: z = depth[y, x] (float32 widened),
    p = (z (x - cx) / fx, -(z (y - cy) / fy), -z)
 2. offset = mean(p), X = p - offset
 3. yaw = atan2(v[1], v[0]) for the first principal direction v of X[:, [0, 2]], sign as scikit-learn's svd_flip
 4. T = Ry(-yaw) X + offset (heading2rotmat)
 5. more than 40000 rows: rows perm[:40000], perm = RandomState(42).shuffle(arange(n)) (= sklearn.utils.shuffle(random_state=42))
 6. up to four DBSCAN trials, eps 0.01 doubling, min_samples 100; a cluster is kept unless size / n < 0.1 or size <= 100; a trial
    is accepted when the kept points are more than 0.5 n; else all points
 7. extents of the kept points, eight corners in gen_8corners order (its swapped y / z names make dy, dz negative), rotated back
    with Ry(yaw) about the offset, y and z flipped
 8. center = corner mean, dimensions = (|c0-c4|, |c0-c3|, |c0-c1|), pose = Kabsch / SVD against the identity-pose cuboid,
    bbox3D = get_cuboid_verts_faces in float32.

Instances the reference has no answer for (it divides by zero or raises) get a status and no box, as the library declares.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

OK, EMPTY, TOO_FEW, NONFINITE, RECT_OUTSIDE = 0, 1, 2, 3, 4


@dataclass
class Params:
    eps0: float = 0.01
    min_samples: int = 100
    max_points: int = 40000
    trials: int = 4
    min_cluster_frac: float = 0.1
    min_cluster: int = 100
    accept_frac: float = 0.5


# ------------------------------------------------------------------------------------------------------------------- scenes
H, W = 480, 640
K_SCENE = np.array([[520.0, 0.0, 320.0], [0.0, 520.0, 240.0], [0.0, 0.0, 1.0]])
STRIP = 12


def make_scene(z0, box=(200, 150, 420, 400), noise=0.002, strip=False, seed=5, background=5.0):
    """A 480 x 640 depth map (float32, background 5 m) with a tilted rectangle x0 <= x < x1, y0 <= y < y1 of depth
    z0 + 0.002 (x - x0) + N(0, noise), the noise drawn in the rectangle's row-major order; the mask is the rectangle plus, with
    ``strip``, the 12 columns of background right of it. Returns (depth, mask uint8, K)."""
    x0, y0, x1, y1 = box
    depth = np.full((H, W), background, np.float64)
    r = np.random.RandomState(seed).randn((y1 - y0) * (x1 - x0)).reshape(y1 - y0, x1 - x0)
    depth[y0:y1, x0:x1] = z0 + 0.002 * (np.arange(x0, x1) - x0)[None, :] + noise * r
    mask = np.zeros((H, W), np.uint8)
    mask[y0:y1, x0:min(W, x1 + (STRIP if strip else 0))] = 1
    return depth.astype(np.float32), mask, K_SCENE.copy()


# the six outcomes (name, make_scene arguments, expected accepted trial - 0 is the fallback -, points, points used)
SCENES = {
    "trial1": dict(z0=0.4, box=(250, 170, 400, 320), noise=0.0005, seed=5),
    "trial2": dict(z0=1.0, box=(200, 150, 420, 400), noise=0.004, strip=True, seed=1),
    "trial3": dict(z0=2.0, box=(200, 150, 420, 400), noise=0.002, strip=True, seed=0),
    "trial4": dict(z0=1.5, box=(10, 10, 600, 460), strip=True, seed=3),
    "fallback": dict(z0=30.0, noise=0.05, seed=5),
    "small": dict(z0=2.0, box=(300, 200, 330, 240), seed=5),
}
SCENE_TRIAL = {"trial1": 1, "trial2": 2, "trial3": 3, "trial4": 4, "fallback": 0}


def box_to_rect(box_xyxy):
    """The rectangle mask of an xyxy box: the pixels ceil(x0) <= x < ceil(x1), ceil(y0) <= y < ceil(y1) (clipped by the user)."""
    return tuple(int(np.ceil(v)) for v in box_xyxy)


def rect_mask(rect, shape):
    x0, y0, x1, y1 = rect
    m = np.zeros(shape, np.uint8)
    if x1 > x0 and y1 > y0:
        m[max(y0, 0):max(min(y1, shape[0]), 0), max(x0, 0):max(min(x1, shape[1]), 0)] = 1
    return m


# -------------------------------------------------------------------------------------------------------------------- steps
def unproject(depth, mask, K):
    ys, xs = np.where(mask > 0.5)
    z = depth[ys, xs].astype(np.float64)
    K = np.asarray(K, np.float64)
    x3 = z * (xs - K[0, 2]) / K[0, 0]
    y3 = z * (ys - K[1, 2]) / K[1, 1]
    return np.stack([x3, -y3, -z], 1)


def pca_direction(X2):
    """First principal direction of the [n, 2] array as sklearn.decomposition.PCA(2).components_[0]: the unit eigenvector of the
    covariance for the larger eigenvalue, flipped so that its entry of larger magnitude is positive (the first on a tie)."""
    C = np.cov((X2 - X2.mean(0)).T)
    w, V = np.linalg.eigh(C)
    v = V[:, int(np.argmax(w))]
    k = int(np.argmax(np.abs(v)))
    return v * (1.0 if v[k] >= 0 else -1.0), w


def heading2rotmat(a):
    R = np.zeros((3, 3))
    R[1, 1] = 1
    R[0, 0] = np.cos(a)
    R[0, 2] = -np.sin(a)
    R[2, 0] = np.sin(a)
    R[2, 2] = np.cos(a)
    return R


_PERM = {}


def perm_for(n):
    if n not in _PERM:
        idx = np.arange(n)
        np.random.RandomState(42).shuffle(idx)
        _PERM[n] = idx
    return _PERM[n]


def dbscan_labels(T, eps, min_samples):
    """labels_ of sklearn.cluster.DBSCAN(eps, min_samples).fit(T): clusters numbered in the order of their smallest core index,
    a border point takes the smallest label among its core neighbours' clusters, noise -1."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(T)
    tree = cKDTree(T)
    counts = tree.query_ball_point(T, eps, return_length=True)           # d <= eps, the point itself included
    core = counts >= min_samples
    labels = np.full(n, -1, np.int64)
    if not core.any():
        return labels
    pairs = tree.query_pairs(eps, output_type="ndarray")
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    g = coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    core_idx = np.nonzero(core)[0]
    first = {}
    for i in core_idx:                                                    # ascending: a component's first hit is its smallest index
        first.setdefault(comp[i], len(first))
    labels[core_idx] = [first[c] for c in comp[core_idx]]
    for a, b in ((0, 1), (1, 0)):                                         # border points: min over the core neighbours
        sel = pairs[core[pairs[:, a]] & ~core[pairs[:, b]]]
        if len(sel):
            border = np.full(n, np.iinfo(np.int64).max)
            np.minimum.at(border, sel[:, b], labels[sel[:, a]])
            hit = border != np.iinfo(np.int64).max
            labels[hit] = np.where(labels[hit] < 0, border[hit], np.minimum(labels[hit], border[hit]))
    return labels


def eps_margin_ok(T, eps, rel=1e-9):
    """No pair distance within ``rel`` of eps: the labels do not hang on the last bits of a distance."""
    from scipy.spatial import cKDTree
    tree = cKDTree(T)
    return tree.count_neighbors(tree, eps * (1 - rel)) == tree.count_neighbors(tree, eps * (1 + rel))


def lift_points(depth, mask, K, params=Params(), rect=None):
    """Steps 1-6 and the extents. Returns a dict: status, n_points, n_used, n_kept, trial, eps, offset, yaw, ext_min, ext_max,
    T (the clustered points), labels (of the last trial run), eig (the covariance eigenvalues, ascending)."""
    out = dict(status=OK, n_points=0, n_used=0, n_kept=0, trial=0, eps=0.0, offset=np.zeros(3), yaw=0.0, ext_min=np.zeros(3),
               ext_max=np.zeros(3))
    if rect is not None:
        x0, y0, x1, y1 = rect
        if x1 <= x0 or y1 <= y0:
            out["status"] = EMPTY
            return out
        mask = rect_mask(rect, depth.shape)
        if not mask.any():
            out["status"] = RECT_OUTSIDE
            return out
    n = int((mask > 0.5).sum())
    out["n_points"] = n
    if n < 2:
        out["status"] = EMPTY if n == 0 else TOO_FEW
        return out
    P = unproject(depth, mask, K)
    if not np.isfinite(P).all():
        out["status"] = NONFINITE
        return out
    offset = P.mean(0)
    X = P - offset
    v, eig = pca_direction(X[:, [0, 2]])
    yaw = float(np.arctan2(v[1], v[0]))
    T = (heading2rotmat(-yaw) @ X.T).T + offset
    if n > params.max_points:
        T = T[perm_for(n)[:params.max_points]]
    m = len(T)
    eps, clean, labels, trial = params.eps0, None, None, 0
    for t in range(1, params.trials + 1):
        labels = dbscan_labels(T, eps, params.min_samples)
        keep = np.zeros(m, bool)
        for c in np.unique(labels):
            if c < 0:
                continue
            ind = labels == c
            size = int(ind.sum())
            if size / m < params.min_cluster_frac or size <= params.min_cluster:
                continue
            keep |= ind
        if keep.sum() > params.accept_frac * m:
            clean, trial = T[keep], t
            break
        if t < params.trials:
            eps = 2 * eps
    if clean is None:
        clean = T
    out.update(n_used=m, n_kept=len(clean), trial=trial, eps=eps, offset=offset, yaw=yaw, ext_min=clean.min(0), ext_max=clean.max(0),
               T=T, labels=labels, eig=eig)
    return out


def gen_8corners(x_min, y_min, z_min, cx, cy, cz):
    flags = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]
    return np.array([np.array([x_min, y_min, z_min]) + np.array(f) * np.array([cx, cy, cz]) for f in flags])


def pseudo_corners(offset, yaw, ext_min, ext_max):
    """Step 7 from the extents on: the eight corners in camera coordinates."""
    x_min, x_max = ext_min[0], ext_max[0]
    y_max, y_min = ext_min[1], ext_max[1]
    z_max, z_min = ext_min[2], ext_max[2]
    box = gen_8corners(x_min, y_min, z_min, x_max - x_min, y_max - y_min, z_max - z_min)
    box = box - offset
    box = (heading2rotmat(yaw) @ box.T).T + offset
    return box.dot(np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]]))


def get_dims(b):
    x = np.sqrt(np.sum((b[0] - b[1]) * (b[0] - b[1])))
    y = np.sqrt(np.sum((b[0] - b[3]) * (b[0] - b[3])))
    z = np.sqrt(np.sum((b[0] - b[4]) * (b[0] - b[4])))
    return np.array([z, y, x])


def cuboid_verts_f32(center, dims, R=None):
    """get_cuboid_verts_faces of the reference (cubercnn/util/math_util.py) on float32 CPU tensors: [8, 3]."""
    import torch
    box = torch.as_tensor(np.concatenate([center, dims])[None], dtype=torch.float32)
    w, h, l = box[:, 3:4], box[:, 4:5], box[:, 5:6]
    verts = torch.zeros([1, 3, 8], dtype=torch.float32)
    verts[:, 0, [0, 3, 4, 7]] = -l / 2
    verts[:, 0, [1, 2, 5, 6]] = l / 2
    verts[:, 1, [0, 1, 4, 5]] = -h / 2
    verts[:, 1, [2, 3, 6, 7]] = h / 2
    verts[:, 2, [0, 1, 2, 3]] = -w / 2
    verts[:, 2, [4, 5, 6, 7]] = w / 2
    if R is not None:
        verts = torch.as_tensor(np.asarray(R)[None], dtype=torch.float32) @ verts
    verts[:, 0, :] += box[:, 0:1]
    verts[:, 1, :] += box[:, 1:2]
    verts[:, 2, :] += box[:, 2:3]
    return verts[0].T.contiguous().numpy()


def get_pose(a, b):
    """The reference's get_pose: both corner sets are centred on a's mean in place, so b keeps its dtype (float32 there)."""
    center = np.mean(a, axis=0)
    a -= center
    b -= center
    U, _, Vt = np.linalg.svd(a.T @ b, full_matrices=True)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        U[:, -1] *= -1
        R = U @ Vt
    return R


def box_of(offset, yaw, ext_min, ext_max, K):
    """Step 7's corners and step 8: the reference's record fields (center_cam, dimensions, pose, bbox3D float32, depth, center_2D)."""
    corners = pseudo_corners(np.asarray(offset, np.float64), float(yaw), np.asarray(ext_min, np.float64), np.asarray(ext_max, np.float64))
    dims = get_dims(corners)
    center = np.mean(corners, axis=0)
    infer = cuboid_verts_f32(center, dims, np.eye(3))                      # float32, as the reference's .numpy() of a float tensor
    pose = get_pose(corners.copy(), infer)
    verts = cuboid_verts_f32(center, dims, pose)
    K = np.asarray(K, np.float64)
    x = (K[0, 0] * center[0]) / center[2] + K[0, 2]
    y = (K[1, 1] * center[1]) / center[2] + K[1, 2]
    return dict(center_cam=center, dimensions=dims, pose=pose, bbox3D=verts, depth=float(center[2]), center_2D=np.array([x, y]))


def lift_boxes(depth, K, boxes_xyxy=None, masks=None, params=Params()):
    """The restatement behind the signature of ovmono3d_amd.geo.lift_boxes (numpy / CPU inputs): one dict per instance with the
    reference's keys as lists, or None for an instance that is not lifted."""
    depth = np.asarray(depth.cpu() if hasattr(depth, "cpu") else depth, np.float32)
    K = np.asarray(K, np.float64).reshape(3, 3)
    n = len(masks) if masks is not None else len(boxes_xyxy)
    out = []
    for i in range(n):
        m = masks[i] if masks is not None else None
        if m is not None:
            m = np.asarray(m.cpu() if hasattr(m, "cpu") else m)
            r = lift_points(depth, m, K, params)
        else:
            r = lift_points(depth, None, K, params, rect=box_to_rect(np.asarray(boxes_xyxy[i], np.float64)))
        if r["status"] != OK:
            out.append(None)
            continue
        b = box_of(r["offset"], r["yaw"], r["ext_min"], r["ext_max"], K)
        out.append(dict(bbox3D=b["bbox3D"].tolist(), depth=b["depth"], center_cam=b["center_cam"].tolist(),
                        dimensions=b["dimensions"].tolist(), pose=b["pose"].tolist(), center_2D=b["center_2D"].tolist()))
    return out


# ---------------------------------------------------------------------------------------------------------- one image, many
def make_composite():
    """The six scenes side by side in one 960 x 1920 depth map (a 2 x 3 grid of 480 x 640 tiles, the principal point in the middle
    of the "trial2" tile, which is thereby the scene exactly; the others are seen off-axis and may settle at another trial), so
    that one call can lift them all, plus instances of every refused kind. Returns (depth, K, instances): each instance is a
    dict with ``name`` and either ``mask`` (uint8 plane) or ``box`` (xyxy, the rectangle is the mask)."""
    names = ["trial4", "trial2", "trial3", "small", "trial1", "fallback"]
    Hc, Wc = 2 * H, 3 * W
    depth = np.full((Hc, Wc), 5.0, np.float32)
    K = np.array([[520.0, 0.0, W + W / 2], [0.0, 520.0, H / 2], [0.0, 0.0, 1.0]])
    inst = []
    for k, name in enumerate(names):
        d, m, _ = make_scene(**SCENES[name])
        ty, tx = (k // 3) * H, (k % 3) * W
        depth[ty:ty + H, tx:tx + W] = d
        plane = np.zeros((Hc, Wc), np.uint8)
        plane[ty:ty + H, tx:tx + W] = m
        inst.append(dict(name=name, mask=plane))
        if not SCENES[name].get("strip", False):                         # the mask is the rectangle: also as a box
            x0, y0, x1, y1 = SCENES[name].get("box", (200, 150, 420, 400))
            inst.append(dict(name=name + "_box", box=(tx + x0 - 0.25, ty + y0 - 0.5, tx + x1 - 0.75, ty + y1 - 1.0)))
    depth[3, 1900] = np.inf
    bad = np.zeros((Hc, Wc), np.uint8)
    bad[0:8, 1890:1910] = 1
    one = np.zeros((Hc, Wc), np.uint8)
    one[20, 30] = 1
    inst += [dict(name="empty", mask=np.zeros((Hc, Wc), np.uint8)), dict(name="too_few", mask=one), dict(name="nonfinite", mask=bad),
             dict(name="outside", box=(2000.0, 10.0, 2100.0, 90.0)), dict(name="degenerate", box=(50.0, 60.0, 50.0, 90.0)),
             dict(name="clipped_box", box=(-40.5, 900.2, 60.0, 1000.0))]
    return depth, K, inst


def make_blobs(seed=0, n=40000):
    """40,000 points in seven Gaussian blobs of different sizes (sigma 3 cm, 1 m apart) in shuffled order: at eps 0.02 several
    clusters with wide fringes of border points and noise around them."""
    rng = np.random.RandomState(seed)
    sizes = np.array([11000, 9000, 7000, 5000, 4000, 2500, 1500])
    assert sizes.sum() == n
    pts = np.concatenate([rng.randn(s, 3) * 0.03 + np.array([1.0 * k, 0.3 * (k % 2), -2.0 - 0.1 * k]) for k, s in enumerate(sizes)])
    return pts[rng.permutation(n)]
