"""The scene as a 3D file: ``<name>_scene.ply``, binary little-endian PLY 1.0 of the un-projected depth map and the boxes.

The device holds the image, the depth map and the label map; ``ovm_scene_ply_points`` (ovmono3d_amd/csrc/scene_ply.hip) compacts
the valid pixels and packs their 15-byte vertex records, and only the 8-byte count and those 15 P bytes cross PCIe. The header,
the box vertices, the faces and the edges - a few hundred bytes per box - are assembled here on the host. The format and every
rule are stated in include/ovm3d.h ("Scene as a PLY file") and restated in numpy by tests/scene_ply_oracle.py.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import lib as _lib
from . import _rows_on

FRAMES = ("camera", "opengl")
# the renderer's face table (render.hip kQuad: each face split along its first-to-third corner) and the panels' edge order
QUADS = ((0, 1, 2, 3), (1, 5, 6, 2), (4, 0, 3, 7), (5, 4, 7, 6), (4, 5, 1, 0), (3, 2, 6, 7))
TRIS = tuple(t for a, b, c, d in QUADS for t in ((a, b, c), (c, d, a)))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (1, 5), (5, 6), (6, 2), (4, 5), (4, 7), (6, 7), (0, 4), (3, 7))
RECORD = 15

_VERTEX = np.dtype({"names": ["xyz", "rgb"], "formats": [("<f4", 3), ("u1", 3)], "offsets": [0, 12], "itemsize": RECORD})
_FACE = np.dtype({"names": ["n", "v"], "formats": ["u1", ("<i4", 3)], "offsets": [0, 1], "itemsize": 13})
_pinned = None


def ply_header(n_points: int, n_boxes: int, frame: str) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\n"
            f"comment ovmono3d_amd scene, frame {frame}, metres\n"
            f"element vertex {n_points + 8 * n_boxes}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {12 * n_boxes}\nproperty list uchar int vertex_indices\n"
            f"element edge {12 * n_boxes}\nproperty int vertex1\nproperty int vertex2\n"
            "end_header\n").encode("ascii")


def edge_colors(colors, n: int) -> np.ndarray:
    """uint8 [n, 4]: the layout's edge colour of colours in [0, 1], min(255, c * 255 * 1.25) rounded half to even ([3] unused)."""
    c = np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors, np.float32).reshape(n, 3).astype(np.float64)
    out = np.zeros((n, 4), np.uint8)
    out[:, :3] = np.rint(np.minimum(255.0, c * 255 * 1.25)).astype(np.uint8)
    return out


def _box_part(corners: np.ndarray, tint: np.ndarray, n_points: int, flip: bool) -> bytes:
    """Vertices, faces and edges of the boxes, indices offset by the points in front of them."""
    n = len(corners)
    v = np.zeros(8 * n, _VERTEX)
    xyz = corners.reshape(8 * n, 3).astype(np.float32)
    if flip:
        xyz[:, 1:] = -xyz[:, 1:]
    v["xyz"] = xyz
    v["rgb"] = np.repeat(tint[:, 2::-1], 8, axis=0)                       # red, green, blue from the BGR edge colour
    first = (n_points + 8 * np.arange(n, dtype=np.int64))[:, None, None]
    f = np.zeros(12 * n, _FACE)
    f["n"] = 3
    f["v"] = (first + np.asarray(TRIS, np.int64)[None]).reshape(12 * n, 3)
    e = (first + np.asarray(EDGES, np.int64)[None]).reshape(12 * n, 2).astype("<i4")
    return v.tobytes() + f.tobytes() + e.tobytes()


def _check_map(a, name: str, tdt, ndt, hw) -> None:
    if torch.is_tensor(a):
        if not a.is_cuda:
            raise ValueError(f"scene_ply: {name} is a CPU tensor; pass a tensor on the HIP device, or a numpy array to upload")
        ok = a.dtype == tdt
    elif isinstance(a, np.ndarray):
        ok = a.dtype == ndt
    else:
        raise ValueError(f"scene_ply: {name} must be a device tensor or a numpy array")
    if not ok or tuple(a.shape) != tuple(hw):
        raise ValueError(f"scene_ply: {name} must be {np.dtype(ndt).name} {list(hw)}, is {a.dtype} {list(a.shape)}")


def _assemble(head: bytes, src: torch.Tensor, tail: bytes) -> bytes:
    """head + the device bytes ``src`` + tail, put together in the module's pinned buffer (grown on demand, reused): the device
    copies its part straight to its place in the file, and the host copies the whole once."""
    global _pinned
    if src.numel() == 0:
        return head + tail
    h, total = len(head), len(head) + src.numel() + len(tail)
    if _pinned is None or _pinned.numel() < total:
        _pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    _pinned[h:h + src.numel()].copy_(src, non_blocking=True)
    host = _pinned.numpy()
    host[:h] = np.frombuffer(head, np.uint8)
    host[h + src.numel():total] = np.frombuffer(tail, np.uint8)
    torch.cuda.current_stream(src.device).synchronize()
    return host[:total].tobytes()


def scene_ply(im, K, depth=None, corners=None, colors=None, point_labels=None, stride: int = 1, max_depth=None,
              frame: str = "camera") -> bytes:
    """The bytes of ``<name>_scene.ply``: the valid pixels of ``depth`` as coloured points, then the boxes as vertices, faces and edges.

    im: BGR uint8 [H, W, 3]; depth: fp32 [H, W] metric depth of it or None (a boxes-only file); point_labels: int32 [H, W]
    (``labels_from_masks``), the box index per pixel or -1, tints a box's points with its colour. Each is a device tensor - rows may be
    pitched, a column slice of a wider buffer is taken as it is - or a numpy array to upload; a CPU tensor, a wrong dtype or shape is a
    ValueError before any device call. K: 3 x 3. corners: [n, 8, 3] camera-space corners in pred_bbox3D order or None (a points-only
    file); colors: [n, 3] in [0, 1], component k for image channel k as ``draw_scene_view`` takes them - the file shows the picture's
    edge colours. stride: every stride-th row and column (1..16); max_depth: drop points farther than it (metres); frame: 'camera'
    (x right, y down, z forward: the frame of ``<name>_dets.json``) or 'opengl' (y and z negated, the reference's flip_matrix).
    One 8-byte read of the point count, then exactly 15 bytes per point are copied, through a pinned buffer."""
    if frame not in FRAMES:
        raise ValueError(f"scene_ply: frame {frame!r} is not supported ({', '.join(FRAMES)})")
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= 16:
        raise ValueError(f"scene_ply: stride must be an integer in 1..16, is {stride!r}")
    if max_depth is not None and not (isinstance(max_depth, (int, float, np.integer, np.floating)) and math.isfinite(max_depth) and np.float32(max_depth) > 0):
        raise ValueError(f"scene_ply: max_depth must be a positive finite number of metres (as float32) or None, is {max_depth!r}")
    if torch.is_tensor(im):
        if not im.is_cuda:
            raise ValueError("scene_ply: im is a CPU tensor; pass a tensor on the HIP device, or a numpy array to upload")
        ok = im.dtype == torch.uint8
    else:
        ok = isinstance(im, np.ndarray) and im.dtype == np.uint8
    if not ok or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("scene_ply: im must be uint8 [H, W, 3]")
    H, W = int(im.shape[0]), int(im.shape[1])
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"scene_ply: an image of {H} x {W} (H * W <= 2^31 - 1)")
    if depth is None and point_labels is not None:
        raise ValueError("scene_ply: point_labels tint the points: pass depth")
    if depth is not None:
        _check_map(depth, "depth", torch.float32, np.float32, (H, W))
    if point_labels is not None:
        _check_map(point_labels, "point_labels", torch.int32, np.int32, (H, W))
    Kh = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float64)
    if Kh.size != 9 or not np.isfinite(Kh).all() or Kh.reshape(9)[0] == 0 or Kh.reshape(9)[4] == 0:
        raise ValueError("scene_ply: K must be a finite 3 x 3 matrix with non-zero focal lengths")
    Kh = np.ascontiguousarray(Kh.reshape(9))
    if corners is None:
        box = np.zeros((0, 8, 3), np.float64)
    else:
        box = np.asarray(corners.detach().cpu() if torch.is_tensor(corners) else corners, np.float64)
        if box.size % 24 != 0 or (box.size and box.shape[-2:] != (8, 3)) or not np.isfinite(box).all():
            raise ValueError("scene_ply: corners must be finite [n, 8, 3]")
        box = np.ascontiguousarray(box.reshape(-1, 8, 3))
    n = len(box)
    if n > _lib.OVM_SCENE_MAX_BOXES:
        raise ValueError(f"scene_ply: {n} boxes, at most {_lib.OVM_SCENE_MAX_BOXES}")
    if n and (colors is None or np.size(colors.detach().cpu() if torch.is_tensor(colors) else colors) != 3 * n):
        raise ValueError(f"scene_ply: colors must be [{n}, 3] in [0, 1], one per box")
    tint = edge_colors(colors, n) if n else np.zeros((1, 4), np.uint8)
    flip = frame == "opengl"

    P, records = 0, torch.empty(0, dtype=torch.uint8)
    if depth is not None:
        src = next((a for a in (im, depth, point_labels) if torch.is_tensor(a)), None)
        device = src.device if src is not None else torch.device("cuda", torch.cuda.current_device())
        L = _lib.load()
        ws_bytes = C.c_int64()
        _lib.check(L.ovm_scene_ply_points_workspace(H, W, int(stride), n, C.byref(ws_bytes)), what="ovm_scene_ply_points_workspace")
        with torch.cuda.device(device):
            img = (im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))).to(device)
            if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * W:
                img = img.contiguous()
            dep = _rows_on(depth, device)
            lab = _rows_on(point_labels, device) if point_labels is not None else None
            worst = -(-H // stride) * -(-W // stride) * RECORD
            out = torch.empty(worst, dtype=torch.uint8, device=device)
            count = torch.empty(1, dtype=torch.int64, device=device)
            ws = torch.empty(max(int(ws_bytes.value), 1), dtype=torch.uint8, device=device)
            rc = L.ovm_scene_ply_points(img.data_ptr(), img.stride(0), dep.data_ptr(), 4 * dep.stride(0),
                                        lab.data_ptr() if lab is not None else None, 4 * lab.stride(0) if lab is not None else 0,
                                        tint.ctypes.data, n, H, W, Kh.ctypes.data, int(stride), float(max_depth) if max_depth is not None else 0.0,
                                        int(flip), out.data_ptr(), worst, count.data_ptr(), ws.data_ptr(), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
            _lib.check(rc, what="ovm_scene_ply_points")
            P = int(count.item())                                          # the one 8-byte read
            records = out[:RECORD * P]
    return _assemble(ply_header(P, n, frame), records, _box_part(box, tint[:n], P, flip))


def write_scene_ply(path, im, K, **kwargs) -> int:
    """``scene_ply(im, K, **kwargs)`` written to ``path``; returns the number of bytes."""
    data = scene_ply(im, K, **kwargs)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
