"""Scene drawing: the reference's ``cubercnn.vis.draw_scene_view`` (cubercnn/vis/vis.py:309-640) on the device.

The small per-scene geometry runs on the host in the library (``ovm_host_scene_layout``); every pixel - rasterisation, shading,
blending, the ground grid, box edges and label compositing - is made by ``ovm_render_scene`` (ovmono3d_amd/csrc/render.hip).
Label glyphs are coverage masks drawn here with Pillow's built-in font (the reference uses cv2's Hershey font); the rules and
every declared deviation are listed in include/ovm3d.h and restated in numpy by tests/scene_oracle.py.

``visualize_from_instances`` and ``render_panels`` (the evaluation's six-panel samples and 3D error line) live in ``panels.py``;
``scene_ply`` and ``write_scene_ply`` (the scene as a binary PLY file of points and boxes) in ``ply.py``.
"""
from __future__ import annotations

import colorsys
import ctypes as C
import functools
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import lib as _lib

MODES = {"front": _lib.OVM_SCENE_FRONT, "novel": _lib.OVM_SCENE_NOVEL,
         "front_and_novel": _lib.OVM_SCENE_FRONT | _lib.OVM_SCENE_NOVEL}
_GRID_CAPACITY = 1 << 16


def euler2mat(euler: Sequence[float]) -> np.ndarray:
    """R = Rz @ Ry @ Rx (reference cubercnn/util/math_util.py:86-105)."""
    cx, sx = math.cos(euler[0]), math.sin(euler[0])
    cy, sy = math.cos(euler[1]), math.sin(euler[1])
    cz, sz = math.cos(euler[2]), math.sin(euler[2])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.dot(rz, np.dot(ry, rx))


def get_color(idx: int) -> List[int]:
    """Deterministic box colour (0..255 per component) for detection index ``idx``: hues stepped by the golden ratio."""
    h = (int(idx) * 0.6180339887498949) % 1.0
    r, g, b = colorsys.hsv_to_rgb(h, 0.7, 0.95)
    return [int(round(r * 255)), int(round(g * 255)), int(round(b * 255))]


@functools.lru_cache(maxsize=16)
def _font(size: int):
    from PIL import ImageFont
    return ImageFont.load_default(size=size)


def text_mask(text: str, font_scale: float) -> np.ndarray:
    """Glyph coverage mask (uint8 0/1, rows x cols) of ``text`` at the reference's cv2 font scale: Pillow's built-in font at
    size round(21 * font_scale), alpha > 127. Its size is the text size the label rectangle is built from."""
    if not text:
        return np.zeros((0, 0), np.uint8)
    from PIL import Image, ImageDraw
    font = _font(max(1, int(round(21 * font_scale))))
    left, top, right, bottom = font.getbbox(text)
    w, h = max(right, 1), max(bottom - top, 1)
    img = Image.new("L", (w, h), 0)
    ImageDraw.Draw(img).text((0, -top), text, fill=255, font=font)
    return (np.asarray(img) > 127).astype(np.uint8)


def _as_f64(a, shape) -> np.ndarray:
    if torch.is_tensor(a):
        a = a.detach().cpu().double().numpy()
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def scene_layout(K, height: int, width: int, corners, colors, masks=None, scale: int = 1000, R=None, T=None,
                 mode: str = "front_and_novel", blend_weight: float = 0.80, blend_weight_overlay: float = 1.0,
                 ground_bounds=None, zplane: float = 0.05):
    """Host geometry (``ovm_host_scene_layout``). masks: [2 views][n] glyph masks or None. Returns (layout, grid [m, 4] int64)."""
    if mode not in MODES:
        raise ValueError(f"draw_scene_view: mode {mode!r} is not supported (front, novel, front_and_novel)")
    L = _lib.load()
    corners = _as_f64(corners, (-1, 8, 3))
    n = len(corners)
    if n > _lib.OVM_SCENE_MAX_BOXES:
        raise ValueError(f"draw_scene_view: {n} boxes, at most {_lib.OVM_SCENE_MAX_BOXES}")
    colors = np.ascontiguousarray(np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors, np.float32).reshape(n, 3))
    inp = _lib.OvmSceneInput()
    inp.n_boxes, inp.mode, inp.height, inp.width, inp.scale = n, MODES[mode], int(height), int(width), int(scale)
    inp.K[:] = _as_f64(K, (9,)).tolist()
    inp.R[:] = _as_f64(euler2mat([np.pi / 3, 0, 0]) if R is None else R, (9,)).tolist()
    if T is not None:
        inp.has_T = 1
        inp.T[:] = _as_f64(T, (3,)).tolist()
    if ground_bounds is not None:
        inp.has_ground_bounds = 1
        inp.ground_bounds[:] = _as_f64(ground_bounds, (5,)).tolist()
    inp.blend_weight, inp.blend_weight_overlay, inp.zplane = float(blend_weight), float(blend_weight_overlay), float(zplane)
    inp.corners, inp.colors = corners.ctypes.data, colors.ctypes.data
    sizes = np.zeros((2, n, 2), np.int32)
    if masks is not None:
        inp.has_labels = 1
        for v in range(2):
            for b in range(n):
                sizes[v, b] = (masks[v][b].shape[1], masks[v][b].shape[0])
        inp.label_size = sizes.ctypes.data
    lay = _lib.OvmSceneLayout()
    cap = _GRID_CAPACITY
    while True:
        grid = np.zeros((cap, 4), np.int64)
        rc = L.ovm_host_scene_layout(C.byref(inp), C.byref(lay), grid.ctypes.data, cap)
        if rc == -5 and lay.n_grid > cap:                     # OVM_ERR_CAPACITY: n_grid holds the count needed
            cap = int(lay.n_grid)
            continue
        _lib.check(rc, what="ovm_host_scene_layout")
        return lay, grid[:lay.n_grid]


def _check_points(depth, point_size, labels, zbuf_out, hw, scale: int, mode: str) -> None:
    """The argument checks of the point cloud; host only."""
    if mode != "front_and_novel":
        raise ValueError("draw_scene_view: the point cloud is the front image's depth in the novel view: mode must be front_and_novel")
    if isinstance(point_size, bool) or not isinstance(point_size, (int, np.integer)) or not 1 <= point_size <= 9 or point_size % 2 == 0:
        raise ValueError(f"draw_scene_view: point_size must be odd and in 1..9, is {point_size!r}")
    for a, name, tdt, ndt in ((depth, "depth", torch.float32, np.float32), (labels, "point_labels", torch.int32, np.int32)):
        if a is None:
            continue
        if torch.is_tensor(a):
            if not a.is_cuda:
                raise ValueError(f"draw_scene_view: {name} is a CPU tensor; pass a tensor on the HIP device, or a numpy array to upload")
            ok = a.dtype == tdt
        elif isinstance(a, np.ndarray):
            ok = a.dtype == ndt
        else:
            raise ValueError(f"draw_scene_view: {name} must be a device tensor or a numpy array")
        if not ok or tuple(a.shape) != tuple(hw):
            raise ValueError(f"draw_scene_view: {name} must be {ndt.__name__} [{hw[0]}, {hw[1]}], is {a.dtype} {list(a.shape)}")
    if zbuf_out is not None and not (torch.is_tensor(zbuf_out) and zbuf_out.is_cuda and zbuf_out.dtype == torch.int64 and
                                     tuple(zbuf_out.shape) == (scale, scale) and zbuf_out.is_contiguous()):
        raise ValueError(f"draw_scene_view: zbuf_out must be a contiguous device int64 [{scale}, {scale}] tensor")


def _rows_on(a, device) -> torch.Tensor:
    """A checked [H, W] map on the device with unit column stride (rows may be pitched: a column slice of a wider buffer)."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device)
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def labels_from_masks(masks: torch.Tensor) -> torch.Tensor:
    """uint8 (or bool) [n, H, W] device planes, nonzero = inside, to the int32 [H, W] map ``draw_scene_view(point_labels=...)`` takes: the
    lowest plane index that covers the pixel, -1 where none does."""
    if not torch.is_tensor(masks) or masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError("labels_from_masks: masks must be uint8 or bool [n, H, W]")
    n = masks.shape[0]
    if n == 0:
        return torch.full(tuple(masks.shape[1:]), -1, dtype=torch.int32, device=masks.device)
    idx = torch.arange(n, dtype=torch.int32, device=masks.device).view(n, 1, 1)
    first = torch.where(masks != 0, idx, torch.full_like(idx, n)).amin(0)
    return torch.where(first < n, first, torch.full_like(first, -1))


def draw_scene_view(im, K, corners, colors, text: Optional[Sequence[str]] = None, scale: int = 1000, R=None, T=None,
                    mode: str = "front_and_novel", blend_weight: float = 0.80, blend_weight_overlay: float = 1.0,
                    ground_bounds=None, zplane: float = 0.05, device=None, depth=None, point_size: int = 3, point_labels=None,
                    zbuf_out=None):
    """Draw the boxes into the image (front) and a top-down view of them (novel), on the device.

    im: BGR uint8 [H, W, 3], numpy or torch (a device tensor is used in place). corners: [n, 8, 3] camera-space corners in
    pred_bbox3D order. colors: [n, 3] in [0, 1] (component k lands in image channel k, as in the reference). text: one label per
    box or None. Returns device uint8 tensors: (front, novel) for 'front_and_novel' - when scale == H they are the two halves of
    one [H, W + scale, 3] buffer -, front for 'front', novel for 'novel'.

    depth: None (the reference's picture, ``ovm_render_scene``), or the metric depth of ``im``, fp32 [H, W], a device tensor or a numpy
    array to upload: the novel view then shows it as a point cloud under the boxes (``ovm_render_scene_points``; mode
    'front_and_novel' only), each point a ``point_size`` (odd, 1..9) square in the image's colour at its pixel. point_labels: int32
    [H, W] (``labels_from_masks``), the box index per pixel or -1: labelled points are tinted with their box's edge colour.
    zbuf_out: a device int64 [scale, scale] tensor that receives the splat's key buffer (tests). A wrong dtype or shape, or a CPU
    tensor, raises ValueError before any device call.
    """
    if mode not in MODES:
        raise ValueError(f"draw_scene_view: mode {mode!r} is not supported (front, novel, front_and_novel)")
    if depth is None and (point_labels is not None or zbuf_out is not None):
        raise ValueError("draw_scene_view: point_labels and zbuf_out belong to the point cloud: pass depth")
    if depth is not None:
        if not (torch.is_tensor(im) or isinstance(im, np.ndarray)) or im.ndim != 3:
            raise ValueError("draw_scene_view: im must be uint8 [H, W, 3]")
        _check_points(depth, point_size, point_labels, zbuf_out, (int(im.shape[0]), int(im.shape[1])), int(scale), mode)
    if device is None:
        device = im.device if torch.is_tensor(im) and im.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("draw_scene_view renders on the HIP device only (no CPU fallback)")
    img = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("draw_scene_view: im must be uint8 [H, W, 3]")
    H, W = int(img.shape[0]), int(img.shape[1])
    S = int(scale)
    n = len(corners)
    masks = None
    if text is not None:
        if len(text) != n:
            raise ValueError("draw_scene_view: one text per box")
        drawn = (MODES[mode] & _lib.OVM_SCENE_FRONT, MODES[mode] & _lib.OVM_SCENE_NOVEL)
        masks = [[text_mask(str(t), 0.50 * hh / 500) if on else np.zeros((0, 0), np.uint8) for t in text]
                 for hh, on in zip((H, S), drawn)]
    lay, grid = scene_layout(K, H, W, corners, colors, masks, S, R, T, mode, blend_weight, blend_weight_overlay, ground_bounds,
                             zplane)
    glyphs = (np.concatenate([m.reshape(-1) for v in masks for m in v]) if masks is not None and n else np.zeros(0, np.uint8))
    glyphs = np.ascontiguousarray(glyphs, np.uint8)
    L = _lib.load()
    ws_bytes = C.c_int64()
    if depth is not None:
        _lib.check(L.ovm_render_scene_points_workspace(C.byref(lay), glyphs.size, C.byref(ws_bytes)), what="ovm_render_scene_points_workspace")
    else:
        _lib.check(L.ovm_render_scene_workspace(C.byref(lay), glyphs.size, C.byref(ws_bytes)), what="ovm_render_scene_workspace")
    want_f, want_n = bool(MODES[mode] & _lib.OVM_SCENE_FRONT), bool(MODES[mode] & _lib.OVM_SCENE_NOVEL)
    with torch.cuda.device(device):
        img = img.to(device, non_blocking=False).contiguous()
        ws = torch.empty(max(int(ws_bytes.value), 1), dtype=torch.uint8, device=device)
        front = novel = None
        if want_f and want_n and S == H:
            both = torch.empty((H, W + S, 3), dtype=torch.uint8, device=device)
            front, novel = both[:, :W], both[:, W:]
            fp = np_ = both.stride(0)
        else:
            if want_f:
                front = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
            if want_n:
                novel = torch.empty((S, S, 3), dtype=torch.uint8, device=device)
            fp, np_ = 3 * W, 3 * S
        stream = torch.cuda.current_stream(device)
        if depth is not None:
            dep, lab = _rows_on(depth, device), (_rows_on(point_labels, device) if point_labels is not None else None)
            Rn = (C.c_double * 9)(*_as_f64(euler2mat([np.pi / 3, 0, 0]) if R is None else R, (9,)).tolist())
            rc = L.ovm_render_scene_points(C.byref(lay), grid.ctypes.data if len(grid) else None, glyphs.ctypes.data if glyphs.size else None,
                                           glyphs.size, img.data_ptr(), img.stride(0), front.data_ptr(), fp, novel.data_ptr(), np_,
                                           dep.data_ptr(), 4 * dep.stride(0), lab.data_ptr() if lab is not None else None,
                                           4 * lab.stride(0) if lab is not None else 0, C.byref(Rn), int(point_size),
                                           zbuf_out.data_ptr() if zbuf_out is not None else None, ws.data_ptr(), ws.numel(),
                                           C.c_void_p(stream.cuda_stream))
            _lib.check(rc, what="ovm_render_scene_points")
        else:
            rc = L.ovm_render_scene(C.byref(lay), grid.ctypes.data if len(grid) else None, glyphs.ctypes.data if glyphs.size else None,
                                    glyphs.size, img.data_ptr(), img.stride(0), front.data_ptr() if front is not None else None, fp,
                                    novel.data_ptr() if novel is not None else None, np_, ws.data_ptr(), ws.numel(),
                                    C.c_void_p(stream.cuda_stream))
            _lib.check(rc, what="ovm_render_scene")
    if mode == "front":
        return front
    if mode == "novel":
        return novel
    return front, novel


def concat_views(front: torch.Tensor, novel: torch.Tensor) -> torch.Tensor:
    """[H, W + scale, 3]: the buffer the two views were rendered into when they share one, else a concatenation."""
    base = front._base
    if base is not None and base is novel._base and base.shape[1] == front.shape[1] + novel.shape[1]:
        return base
    return torch.cat((front, novel), 1)


from .panels import SampleDataset, match_errors, panel_boxes, panels_layout, render_panels, visualize_from_instances  # noqa: E402,F401
from .ply import scene_ply, write_scene_ply  # noqa: E402,F401
