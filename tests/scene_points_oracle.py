"""numpy fp64 restatement of the point cloud of ovm_render_scene_points (ovmono3d_amd/csrc/render.hip, rules in include/ovm3d.h).

splat(...)    pass A: per source pixel the same IEEE fp64 operations in the same order as scene_splat, np.float32 for the key's
              depth word, and the lexicographic minimum of (float bits, source index) per target pixel - the [S, S] uint64 buffer
              the device must produce bit for bit - plus counts of the pixels each rule removed, for tests to assert on.
compose(...)  pass B: which novel pixels hold a point and the colour the point gives them.
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def targets(depth, K, Kn, R, center, shift, zplane):
    """Per source pixel: (ok, x, y, key) - ok: the pixel survives the depth and zplane rules; (x, y): float64 floor of its novel
    projection (any value where not ok); key: uint64."""
    K, Kn, R = np.asarray(K, np.float64).reshape(3, 3), np.asarray(Kn, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    c = np.asarray(center, np.float64).reshape(3)
    d32 = np.asarray(depth, np.float32)
    H, W = d32.shape
    i, j = np.mgrid[0:H, 0:W]
    valid = np.isfinite(d32) & (d32 > 0)
    d = d32.astype(np.float64)
    with np.errstate(all="ignore"):
        X = ((j + 0.5) - K[0, 2]) / K[0, 0] * d
        Y = ((i + 0.5) - K[1, 2]) / K[1, 1] * d
        d0, d1, d2 = X - c[0], Y - c[1], d - c[2]
        r0 = R[0, 0] * d0 + R[0, 1] * d1 + R[0, 2] * d2
        r1 = R[1, 0] * d0 + R[1, 1] * d1 + R[1, 2] * d2
        r2 = R[2, 0] * d0 + R[2, 1] * d1 + R[2, 2] * d2
        r2 = r2 + shift
        front = (r2 >= zplane) & (r2 > 0.0)
        u = (Kn[0, 0] * r0 + Kn[0, 1] * r1 + Kn[0, 2] * r2) / r2
        v = (Kn[1, 0] * r0 + Kn[1, 1] * r1 + Kn[1, 2] * r2) / r2
        x, y = np.floor(u), np.floor(v)
        zbits = r2.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (zbits << np.uint64(32)) | (i * W + j).astype(np.uint64)
    return valid, front, x, y, key


def splat(depth, K, Kn, R, center, shift, zplane, S, point_size):
    """-> (zbuf uint64 [S, S], stats). stats: pixels removed by the depth rule, by the zplane rule, landing with no footprint pixel on the
    canvas, and splatted."""
    assert point_size % 2 == 1 and 1 <= point_size <= 9
    half = (point_size - 1) // 2
    valid, front, x, y, key = targets(depth, K, Kn, R, center, shift, zplane)
    alive = valid & front
    with np.errstate(invalid="ignore"):
        on = alive & (x >= -half) & (x <= S - 1 + half) & (y >= -half) & (y <= S - 1 + half)
    stats = {"bad_depth": int((~valid).sum()), "behind": int((valid & ~front).sum()), "off_canvas": int((alive & ~on).sum()), "splatted": int(on.sum())}
    xs, ys, ks = x[on].astype(np.int64), y[on].astype(np.int64), key[on]
    order = np.argsort(ks, kind="stable")[::-1]                     # descending: in a fancy assignment the last write - the minimum - stays
    xs, ys, ks = xs[order], ys[order], ks[order]
    flat = np.full(S * S, EMPTY, np.uint64)
    for dy in range(-half, half + 1):
        for dx in range(-half, half + 1):
            xx, yy = xs + dx, ys + dy
            m = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
            t = yy[m] * S + xx[m]
            flat[t] = np.minimum(flat[t], ks[m])
    return flat.reshape(S, S), stats


def compose(zbuf, image, labels=None, edge_u8=None):
    """-> (hit bool [S, S], colour uint8 [S, S, 3]): where the buffer holds a point, and the image's BGR at the winning source pixel,
    tinted (image + edge_u8[b] + 1) >> 1 where labels[b] >= 0 there. Applies only where the novel pixel has no triangle; edges and
    labels are drawn over it afterwards."""
    H, W = image.shape[:2]
    hit = zbuf != EMPTY
    src = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    src[~hit] = 0
    si, sj = src // W, src % W
    col = image[si, sj].astype(np.int64)
    if labels is not None:
        b = np.asarray(labels)[si, sj].astype(np.int64)
        n = len(edge_u8)
        tinted = (b >= 0) & (b < n)
        tint = np.asarray(edge_u8, np.int64).reshape(-1, 4)[np.where(tinted, b, 0), :3] if n else np.zeros_like(col)
        col = np.where(tinted[..., None], (col + tint + 1) >> 1, col)
    col[~hit] = 0
    return hit, col.astype(np.uint8)
