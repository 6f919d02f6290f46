"""numpy restatement of the evaluation sample panels (reference cubercnn/vis/vis.py:76-296: visualize_from_instances, with
draw_3d_box_from_verts :695-728 and draw_text :755-783), written from the rules listed in include/ovm3d.h.

The reference draws with cv2 (rectangle, line, putText), which is not available; this file states the rules the native compositor
(ovmono3d_amd/csrc/panels.hip) must follow, the declared deviations included: a thick line covers the integer pixel centres within
thickness / 2 of the segment, glyphs are the masks of ovmono3d_amd.vis.text_mask, colours are ovmono3d_amd.vis.get_color, geometry
is fp64 with every product written out term by term, left to right, and the 3D thickness is max(1, round_half_even(3 * H / 500)).

layout(...) -> six lists of primitives in drawing order (panel 0 gt_all_2d, 1 gt_2d, 2 pred_2d, 3 gt_all_3d, 4 gt_3d, 5 pred_3d):
               ("seg", x0, y0, x1, y1, thickness, colour), ("blend", x0, y0, x1, y1, colour) half-open, already clipped to the image,
               ("glyph", x, y, w, h, colour, mask) with (x, y) the mask's top-left.
render(...) -> (mosaic uint8 [2H, 3W, 3], band bool [2H, 3W]). band: pixel centres within 1e-3 px of a line's radius (the rule of
               tests/test_gpu_render.py), where fp64 rounding may legitimately decide differently - except the exact ties: a pixel
               whose squared distance EQUALS the squared radius bit for bit (every pixel beside an axis-aligned line of even
               thickness) is computed without rounding by both sides, so it is held to the bytes. This band is a subset of the
               plain 1e-3 band: it asks more, never less.
"""
import math

import numpy as np

from scene_oracle import _clip_segment, _i64, _seg_dist2

EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (1, 5), (5, 6), (6, 2), (4, 5), (4, 7), (6, 7), (0, 4), (3, 7))
SIGNS = ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1))
ZPLANE, EPS, BAND = 0.05, 1e-4, 1e-3


def color_of(b):
    from ovmono3d_amd.vis import get_color
    return tuple(int(v) for v in (b["color"] if "color" in b else get_color(b["category_id"])))


def masks_of(b, H):
    """(2D mask, 3D mask) of the box's name."""
    from ovmono3d_amd.vis import text_mask
    return text_mask(str(b["name"]), 0.5), text_mask(str(b["name"]), 0.50 * H / 500)


def thickness3d(H):
    return max(1, int(np.round(3 * H / 500)))


def cuboid(center, dims, R):
    """get_cuboid_verts_faces' corners (math_util.py:169-191) of centre, (w, h, l) and pose, fp64."""
    w, h, l = (float(v) for v in dims)
    R = np.asarray(R, np.float64).reshape(3, 3)
    v = np.zeros((8, 3))
    for k, (sx, sy, sz) in enumerate(SIGNS):
        x, y, z = sx * l / 2, sy * h / 2, sz * w / 2
        for d in range(3):
            v[k, d] = (R[d, 0] * x + R[d, 1] * y + R[d, 2] * z) + float(center[d])
    return v


def _proj(K, v, div):
    return ((K[0, 0] * v[0] + K[0, 1] * v[1] + K[0, 2] * v[2]) / div, (K[1, 0] * v[0] + K[1, 1] * v[1] + K[1, 2] * v[2]) / div)


def _prims_2d(b, H):
    x, y, w, h = (float(v) for v in b["bbox"])
    x1, y1, x2, y2 = int(_i64(x)), int(_i64(y)), int(_i64(x + w)), int(_i64(y + h))
    col = color_of(b)
    out = [("seg", *s, 2, col) for s in ((x1, y1, x2, y1), (x2, y1, x2, y2), (x2, y2, x1, y2), (x1, y2, x1, y1))]
    m = masks_of(b, H)[0]
    if m.size:
        out.append(("glyph", x1, y1 - 10 - m.shape[0], m.shape[1], m.shape[0], col, m))
    return out


def _prims_3d(b, K, H, W):
    col = color_of(b)
    v = cuboid(b["center_cam"], b["dimensions"], b["pose"])
    t = thickness3d(H)
    out = []
    for i, j in EDGES:
        v0, v1 = v[i].copy(), v[j].copy()
        z0, z1 = v0[2], v1[2]
        if not (z0 >= ZPLANE or z1 >= ZPLANE):
            continue
        s = (ZPLANE - z0) / max(z1 - z0, EPS)
        nv = v0 + s * (v1 - v0)
        if z0 < ZPLANE and z1 >= ZPLANE:
            v0 = nv
        elif z0 >= ZPLANE and z1 < ZPLANE:
            v1 = nv
        u0, u1 = _proj(K, v0, max(v0[2], EPS)), _proj(K, v1, max(v1[2], EPS))
        out.append(("seg", int(_i64(u0[0])), int(_i64(u0[1])), int(_i64(u1[0])), int(_i64(u1[1])), t, col))
    m = masks_of(b, H)[1]
    if not m.size:
        return out
    gh, gw = m.shape
    p0, p1 = int(_i64(float(b["bbox"][0]))), int(_i64(float(b["bbox"][1])))
    clip = lambda a, hi: min(max(a, 0), hi)  # noqa: E731
    xs = clip(p0, W)
    xe = clip(xs + gw - 1 + 4, W)
    ys, ye = clip(p1 - gh - 2, H), clip(p1 + 1 - 2, H)
    rx1, ry1 = min(xe + 1, W), min(ye + 1, H)
    if rx1 > xs and ry1 > ys:
        out.append(("blend", xs, ys, rx1, ry1, col))
    tc = 0 if (col[0] + col[1] + col[2]) / 3 > 127.5 else 255
    out.append(("glyph", clip(p0 + 2, W), clip(p1 - 2, H) - gh, gw, gh, (tc, tc, tc), m))
    return out


def layout(K, H, W, gt_all, gt_eval, preds):
    K = np.asarray(K, np.float64).reshape(3, 3)
    panels = [[] for _ in range(6)]
    for b, ev in zip(gt_all, gt_eval):
        p2 = _prims_2d(b, H)
        p3 = _prims_3d(b, K, H, W) if b.get("draw3d", True) else []
        panels[0] += p2
        panels[3] += p3
        if ev:
            panels[1] += p2
            panels[4] += p3
    for b in preds:
        panels[2] += _prims_2d(b, H)
        if b.get("draw3d", True):
            panels[5] += _prims_3d(b, K, H, W)
    return panels


def _draw(img, band, prims):
    H, W = img.shape[:2]
    for p in prims:
        if p[0] == "seg":
            r = p[5] / 2.0
            c = _clip_segment(float(p[1]), float(p[2]), float(p[3]), float(p[4]), r, W, H)
            if c is None:
                continue
            x0, x1 = max(int(math.floor(min(c[0], c[2]) - r)), 0), min(int(math.ceil(max(c[0], c[2]) + r)), W - 1)
            y0, y1 = max(int(math.floor(min(c[1], c[3]) - r)), 0), min(int(math.ceil(max(c[1], c[3]) + r)), H - 1)
            if x0 > x1 or y0 > y1:
                continue
            yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
            d2 = _seg_dist2(xx, yy, *c)
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            img[sl][d2 <= r * r] = p[6]
            band[sl] |= (np.abs(np.sqrt(d2) - r) < BAND) & (d2 != r * r)
        elif p[0] == "blend":
            sl = (slice(p[2], p[4]), slice(p[1], p[3]))
            for ch in range(3):
                img[sl + (ch,)] = img[sl + (ch,)].astype(np.float64) * 0.33 + p[5][ch] * (1 - 0.33)     # float64, truncated by the uint8 store
        else:
            _, gx, gy, gw, gh, col, m = p
            x0, y0, x1, y1 = max(gx, 0), max(gy, 0), min(gx + gw, W), min(gy + gh, H)
            if x0 >= x1 or y0 >= y1:
                continue
            sub = m[y0 - gy:y1 - gy, x0 - gx:x1 - gx] > 0
            img[y0:y1, x0:x1][sub] = col


def render(image, panels):
    """image: uint8 BGR [H, W, 3]; panels: layout()'s lists."""
    H, W = image.shape[:2]
    mosaic = np.zeros((2 * H, 3 * W, 3), np.uint8)
    band = np.zeros((2 * H, 3 * W), bool)
    for p in range(6):
        r, c = divmod(p, 3)
        img, b = image.copy(), np.zeros((H, W), bool)
        _draw(img, b, panels[p])
        mosaic[r * H:(r + 1) * H, c * W:(c + 1) * W] = img
        band[r * H:(r + 1) * H, c * W:(c + 1) * W] = b
    return mosaic, band


# ------------------------------------------------------------------------------------------------------------------ scenes

NAMES = ("chair", "table", "sofa", "bed", "lamp", "books", "cup", "bottle", "shoes")


def yaw(a):
    return [[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]


def intrinsics(H, W):
    f = 0.9 * W
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def box(K, cat, center, dims, ang, bbox=None, **kw):
    """A box dict; bbox defaults to the xywh hull of the projected corners that lie in front of the camera."""
    R = yaw(ang)
    if bbox is None:
        v = cuboid(center, dims, R)
        v = v[v[:, 2] > 0.1] if (v[:, 2] > 0.1).any() else np.array([[0.0, 0.0, 1.0]])
        u, w = (K[0, 0] * v[:, 0] + K[0, 2] * v[:, 2]) / v[:, 2], (K[1, 1] * v[:, 1] + K[1, 2] * v[:, 2]) / v[:, 2]
        bbox = [float(u.min()), float(w.min()), float(u.max() - u.min()), float(w.max() - w.min())]
    return dict({"category_id": int(cat), "name": NAMES[int(cat)], "bbox": [float(t) for t in bbox],
                 "center_cam": [float(t) for t in center], "dimensions": [float(t) for t in dims], "pose": R}, **kw)


def make_scene(seed, n_gt, n_pred, H, W):
    """Seeded boxes in front of the camera, some leaving the canvas: (K, gt_all, gt_eval, preds)."""
    rng = np.random.default_rng(seed)
    K = intrinsics(H, W)

    def one(**kw):
        z = rng.uniform(1.5, 8.0)
        c = [rng.uniform(-0.75, 0.75) * z, rng.uniform(-0.5, 0.5) * z, z]
        return box(K, rng.integers(0, len(NAMES)), c, rng.uniform(0.3, 1.6, 3), rng.uniform(-math.pi, math.pi), **kw)

    gt_all = [one() for _ in range(n_gt)]
    gt_eval = [bool(b["category_id"] % 3) for b in gt_all]
    preds = [one(draw3d=bool(rng.uniform() > 0.3)) for _ in range(n_pred)]
    return K, gt_all, gt_eval, preds


def constructed(H, W):
    """Edge cases by construction: name -> (K, gt_all, gt_eval, preds)."""
    K = intrinsics(H, W)
    mid = [0.3 * W, 0.3 * H, 0.3 * W, 0.3 * H]
    plain = box(K, 4, [0.2, 0.1, 4.0], [0.8, 0.9, 1.1], 0.5)
    out = {
        # corners at z in about [-0.3, 0.9]: some edges cross zplane, some lie wholly behind it
        "straddle": ([box(K, 0, [0.1, 0.0, 0.3], [1.0, 0.5, 0.7], 0.4, bbox=mid)], [True], [box(K, 1, [-0.2, 0.1, 0.2], [0.6, 0.4, 0.9], -1.1, bbox=mid)]),
        "behind": ([box(K, 1, [0.0, 0.0, -2.0], [0.5, 0.5, 0.5], 0.3, bbox=[10.0, 20.0, 30.0, 20.0])], [True], []),
        "partly_off": ([box(K, 2, [-3.0, -1.5, 4.0], [1.0, 1.0, 1.0], 0.2, bbox=[-15.5, -8.2, 40.0, 30.0])], [True],
                       [box(K, 5, [3.2, 1.9, 4.0], [1.0, 1.0, 1.0], 0.9, bbox=[W - 20.5, H - 12.25, 60.0, 40.0])]),
        "wholly_off": ([box(K, 3, [60.0, 0.0, 5.0], [1.0, 1.0, 1.0], 0.0, bbox=[W + 20.0, H + 10.0, 30.0, 30.0])], [True],
                       [box(K, 6, [0.0, -70.0, 5.0], [1.0, 1.0, 1.0], 0.0, bbox=[-90.0, -80.0, 30.0, 30.0])]),
        "border_label": ([dict(plain, bbox=[W - 6.0, 3.0, 20.0, 20.0]), dict(plain, bbox=[0.0, 0.0, 12.0, 9.0]),
                          dict(plain, bbox=[W + 0.0, H + 0.0, 5.0, 5.0])], [True, True, True], [dict(plain, bbox=[-3.5, H - 1.0, 9.0, 9.0])]),
        "unprompted": ([plain, box(K, 7, [-0.5, 0.2, 3.0], [0.5, 0.6, 0.7], 1.0)], [True, False], []),
        "pred_2d_only": ([plain], [True], [dict(plain, draw3d=False), dict(plain, draw3d=True)]),
    }
    return {k: (K,) + v for k, v in out.items()}
