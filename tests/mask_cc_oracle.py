"""The checker of connected components and the small-region clean-up (ovmono3d_amd.masks.connected_components /
remove_small_regions, csrc/mask_cc.hip; include/ovm3d.h, "Mask connected components").

Labels are scipy.ndimage.label's (the cross for 4-connectivity, ones((3, 3)) for 8): components numbered in row-major order of
their first pixel. The clean-up is segment_anything's utils/amg.py remove_small_regions restated in numpy on those labels (the
package is not installed; it labels with cv2.connectedComponentsWithStats, whose numbering differs from scipy's only in which of
two equally large regions argmax meets first - the header defines that as label order). postprocess_small_regions restates the
automatic mask generator's method of that name with the NMS of tests/sam_auto_oracle.py.

Everything is integer-exact: no comparison against this file carries a tolerance.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy import ndimage

import sam_auto_oracle as A

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.int32)
FULL = np.ones((3, 3), np.int32)
MODES = ("holes", "islands", "both")

# (H, W), 1 x 1 up to one full-HD plane: below, at and above a wave (64 pixels of a row), a workgroup (4 of them) and several rows of
# them. The kernels' only tile is the 64 pixels of a row that one wave owns: widths 63, 64 and 65 are the tile edge and its two sides.
SHAPES = [(1, 1), (1, 130), (130, 1), (7, 5), (5, 63), (64, 64), (5, 65), (65, 67), (130, 257), (1080, 1920)]
NOISE_DENSITIES = (0.3, 0.5, 0.593, 0.7)


def label(plane, connectivity=8, invert=False):
    """(labels int32 [H, W], count) of one plane: foreground != 0, or == 0 with invert"""
    fg = (np.asarray(plane) != 0) != bool(invert)
    lab, n = ndimage.label(fg, structure=FULL if connectivity == 8 else CROSS)
    return lab.astype(np.int32), int(n)


@functools.lru_cache(maxsize=40)                                         # a mask and its complement for every plane of one shape's set
def _regions(working_bytes, shape):
    lab, n = ndimage.label(np.frombuffer(working_bytes, np.uint8).reshape(shape), structure=FULL)
    return lab, n, np.bincount(lab.ravel(), minlength=n + 1)[1:]


def remove_small_regions_step(mask, area_thresh, mode):
    """segment_anything's remove_small_regions: (bool [H, W], changed). Its lists of labels are a lookup table here (fill[label] =
    the label belongs to the output), which is the same selection."""
    assert mode in ("holes", "islands")
    mask = np.asarray(mask) != 0
    holes = mode == "holes"
    regions, n, sizes = _regions((holes ^ mask).astype(np.uint8).tobytes(), mask.shape)     # the same plane is asked for at several thresholds
    small = sizes < area_thresh
    if not small.any():
        return mask, False
    fill = np.zeros(n + 1, bool)
    if holes:
        fill[0] = True                                                   # [0] + small_regions
        fill[1:] = small
    else:
        fill[1:] = ~small                                                # every label not in [0] + small_regions
        if not fill.any():
            fill[int(np.argmax(sizes)) + 1] = True                       # argmax: the first of equal ones
    return fill[regions], True


def remove_small_regions(mask, area_thresh, mode):
    """(uint8 [H, W] of 0 / 1, changed) for mode "holes", "islands" or "both" (holes, then islands on the result; changed = either)"""
    if mode != "both":
        m, ch = remove_small_regions_step(mask, area_thresh, mode)
        return m.astype(np.uint8), bool(ch)
    m, ch1 = remove_small_regions_step(mask, area_thresh, "holes")
    m, ch2 = remove_small_regions_step(m, area_thresh, "islands")
    return m.astype(np.uint8), bool(ch1 or ch2)


def tight_box(mask):
    """(float32 [4] = (xmin, ymin, xmax + 1, ymax + 1), area): SamPredictor.mask_boxes; zeros for an empty mask"""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return np.zeros(4, np.float32), 0
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32), int(len(ys))


def postprocess_small_regions(out, min_area, nms_thresh):
    """`out`: generate_device's dict as host arrays. Every mask cleaned with mode "both"; NMS (sam_auto_oracle.select: decreasing
    score, ties to the lower index, IoU > nms_thresh on the inclusive boxes as floats) with score 1 for an unchanged and 0 for a
    changed mask; the result in keep order, a changed mask with its cleaned plane, box and area, an unchanged one as it was."""
    masks = np.asarray(out["masks"])
    m = len(masks)
    if m == 0:
        return {k: np.asarray(v) for k, v in out.items()}
    cleaned, changed, boxes, areas, incl = [], [], [], [], []
    for plane in masks:
        c, ch = remove_small_regions(plane, min_area, "both")
        b, a = tight_box(c)
        cleaned.append(c), changed.append(ch), boxes.append(b), areas.append(a)
        incl.append([b[0], b[1], b[2] - 1, b[3] - 1] if a else [0, 0, 0, 0])
    changed = np.asarray(changed)
    t = A.table(iou=(~changed).astype(np.float32), stability_=np.zeros(m, np.float32), boxes=np.asarray(incl, np.int32))
    keep = A.select(t, 0.0, 0.0, nms_thresh)
    res = {k: np.asarray(v)[keep] for k, v in out.items()}
    for j, i in enumerate(keep):
        if changed[i]:
            res["masks"][j], res["boxes"][j], res["areas"][j] = cleaned[i], boxes[i], areas[i]
    res["changed"] = changed[keep]
    return res


# ------------------------------------------------------------------------------------------------ the planes
def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((x + y) % 2 == 0).astype(np.uint8)


def serpentine(H, W):
    """One-pixel-wide path through every row: even rows are full, odd rows hold the one pixel that joins them, at alternating ends"""
    p = np.zeros((H, W), np.uint8)
    p[0::2] = 1
    p[1::4, W - 1] = 1
    p[3::4, 0] = 1
    return p


def comb(H, W):
    """Teeth in every other column that meet only in the last row"""
    p = np.zeros((H, W), np.uint8)
    p[:, 0::2] = 1
    p[H - 1] = 1
    return p


def u_shape(H, W):
    """Two arms at the sides that meet only in the last row"""
    p = np.zeros((H, W), np.uint8)
    p[:, 0] = 1
    p[:, W - 1] = 1
    p[H - 1] = 1
    return p


def rings(H, W):
    """Concentric one-pixel rectangles, every other one"""
    y, x = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d % 2 == 0).astype(np.uint8)


def diagonals(H, W, period=3):
    y, x = np.mgrid[:H, :W]
    return ((x + y) % period == 0).astype(np.uint8)


def anti_diagonals(H, W, period=4):
    y, x = np.mgrid[:H, :W]
    return ((x - y) % period == 0).astype(np.uint8)


def noise(H, W, density, seed=0):
    g = np.random.default_rng(1000 * H + W + int(1000 * density) + seed)
    return (g.random((H, W)) < density).astype(np.uint8)


def edge_planes(H, W):
    """{name: uint8 [H, W]}: the contents the kernels are held to at every shape"""
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8), "checkerboard": checkerboard(H, W),
           "serpentine": serpentine(H, W), "comb": comb(H, W), "u": u_shape(H, W), "rings": rings(H, W), "diagonals": diagonals(H, W),
           "anti_diagonals": anti_diagonals(H, W)}
    for d in NOISE_DENSITIES:
        out[f"noise{d}"] = noise(H, W, d)
    return out


def blobs(H, W, n_blobs=6, specks=40, pinholes=40, seed=0):
    """A mask as SAM returns it: a few ellipses, specks of 1 - 9 pixels away from them and pinholes of 1 - 9 pixels inside them"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    p = np.zeros((H, W), bool)
    for _ in range(n_blobs):
        cy, cx = g.uniform(0, H), g.uniform(0, W)
        ry, rx = g.uniform(H / 16, H / 4), g.uniform(W / 16, W / 4)
        p |= ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
    for k in range(specks + pinholes):
        s = int(g.integers(1, 4))
        y0, x0 = int(g.integers(0, max(H - s, 1))), int(g.integers(0, max(W - s, 1)))
        p[y0:y0 + s, x0:x0 + s] = k < specks
    return p.astype(np.uint8)


def area_thresholds(plane):
    """1, 2, the area of an existing region of the plane or its complement (8-connected; 3 when there is none), H * W + 1"""
    H, W = plane.shape
    existing = 3
    for inv in (False, True):
        lab, n = label(plane, 8, inv)
        if n:
            sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            existing = int(np.sort(sizes)[len(sizes) // 2])
            break
    return [1, 2, existing, H * W + 1]
