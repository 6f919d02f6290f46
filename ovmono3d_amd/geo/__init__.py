"""OVMono3D-GEO: lift 2D boxes to 3D from metric depth and masks (reference tools/ovmono3d_geo.py:127-258) on the device.

``lift_boxes`` runs the whole geometric part - un-projection, PCA yaw, DBSCAN outlier removal, extent fit - for all instances of
one image in one call of ``ovm_geo_lift`` (ovmono3d_amd/csrc/geo.hip), then builds the reference's record fields on the host with
``ovm_host_geo_box``. Of the two networks the reference runs in front of it, SAM is ``ovmono3d_amd.sam`` (its ``predict_boxes``
planes are device tensors ``masks`` takes as they are); Depth Pro is not here: the depth map arrives as an array. Masks may also
come from files, or the 2D box itself is the mask: ``geo.sources`` holds every source of boxes and masks the two front ends
(tools/ovmono3d_geo.py, demo/demo_geo.py) put in front of ``lift_boxes``, and their command-line flags.

``ground_plane`` fits the floor to the depth map (``ovm_geo_ground_plane``, ovmono3d_amd/csrc/ground.hip) and ``lift`` /
``lift_boxes`` take its frame, so that boxes stand upright on the floor under a pitched or rolled camera: a declared deviation
from the reference, which takes the camera for level, and off unless a caller passes ``frame``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import lib as _lib

STATUS_NAMES = ("ok", "empty mask", "fewer than 2 points", "non-finite depth under the mask", "rectangle outside the image",
                "mask pixel count mismatch", "perm entry out of range")


@dataclass
class GeoParams:
    """The reference's settings (tools/ovmono3d_geo.py:154-176)."""
    eps0: float = 0.01
    min_samples: int = 100
    max_points: int = 40000
    trials: int = 4
    min_cluster_frac: float = 0.1
    min_cluster: int = 100
    accept_frac: float = 0.5
    last_stage: int = 0

    def to_c(self) -> "_lib.OvmGeoParams":
        p = _lib.OvmGeoParams()
        p.eps0, p.min_cluster_frac, p.accept_frac = self.eps0, self.min_cluster_frac, self.accept_frac
        p.min_samples, p.max_points, p.trials, p.min_cluster, p.last_stage = (self.min_samples, self.max_points, self.trials,
                                                                             self.min_cluster, self.last_stage)
        return p


GROUND_STATUS_NAMES = ("ok", "fewer than 3 points", "no plane")


@dataclass
class GroundParams:
    """Settings of the ground-plane fit (``OvmGroundParams``). thresh, thresh_rel and min_share are not tuned on real depth maps."""
    thresh: float = 0.02
    thresh_rel: float = 0.01
    max_tilt_deg: float = 45.0
    min_share: float = 0.10
    max_depth: float = 0.0
    hypotheses: int = 512
    stride: int = 4
    seed: int = 0
    refine: int = 1

    def to_c(self) -> "_lib.OvmGroundParams":
        p = _lib.OvmGroundParams()
        p.thresh, p.thresh_rel, p.max_tilt_deg, p.min_share, p.max_depth = self.thresh, self.thresh_rel, self.max_tilt_deg, self.min_share, self.max_depth
        p.hypotheses, p.stride, p.seed, p.refine = self.hypotheses, self.stride, self.seed, int(self.refine)
        return p


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise _lib.OvmError(f"{what} failed with code {rc}: {(_lib.load().ovm_geo_last_error() or b'').decode()}")


def box_to_rect(box_xyxy) -> tuple:
    """The rectangle used when the 2D box is the mask: the pixels ceil(x0) <= x < ceil(x1), ceil(y0) <= y < ceil(y1)."""
    return tuple(int(math.ceil(float(v))) for v in box_xyxy)


_PERM_HOST: Dict[int, np.ndarray] = {}
_PERM_DEV: Dict[tuple, torch.Tensor] = {}


def downsample_perm(n: int) -> np.ndarray:
    """sklearn.utils.shuffle(arange(n), random_state=42) of the reference's auto_downsample, cached per n."""
    if n not in _PERM_HOST:
        idx = np.arange(n)
        np.random.RandomState(42).shuffle(idx)
        _PERM_HOST[n] = idx.astype(np.int32)
    return _PERM_HOST[n]


def _perm_on(n: int, device: torch.device) -> torch.Tensor:
    key = (n, str(device))
    if key not in _PERM_DEV:
        if len(_PERM_DEV) >= 64:
            _PERM_DEV.clear()
        _PERM_DEV[key] = torch.from_numpy(downsample_perm(n)).to(device)
    return _PERM_DEV[key]


def _need_hip(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what} must be a tensor on the HIP device (there is no CPU path)")


class GroundCall:
    """The arguments of one ``ovm_geo_ground_plane`` call, prepared once: ``launch()`` enqueues it on the current stream (no read,
    no synchronisation), ``read()`` fetches the ``OvmGroundResult``. ``frame`` is the result's frame on the device, 9 doubles: what
    ``LiftCall`` / ``lift`` / ``lift_boxes`` take, no read in between."""

    def __init__(self, depth: torch.Tensor, K, params: GroundParams = GroundParams(), want_counts: bool = False):
        self.L = _lib.load()
        _need_hip(depth, "depth")
        if depth.dtype != torch.float32 or depth.dim() != 2:
            raise ValueError("depth must be float32 [H, W]")
        self.depth = depth.contiguous()
        self.H, self.W, self.dev = int(depth.shape[0]), int(depth.shape[1]), depth.device
        self.K = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9).tolist())
        self.params = params.to_c()
        nbytes = C.c_int64()
        _check(self.L.ovm_geo_ground_workspace(self.H, self.W, C.byref(self.params), C.byref(nbytes)), "ovm_geo_ground_workspace")
        self.nbytes = int(nbytes.value)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=self.dev)
        self.res = torch.zeros(C.sizeof(_lib.OvmGroundResult) // 8, dtype=torch.float64, device=self.dev)
        self.counts = torch.empty(params.hypotheses, dtype=torch.int32, device=self.dev) if want_counts else None
        self.launched = False

    @property
    def frame(self) -> torch.Tensor:
        o = _lib.OvmGroundResult.frame.offset // 8
        return self.res[o:o + 9]

    def launch(self) -> "GroundCall":
        _check(self.L.ovm_geo_ground_plane(self.depth.data_ptr(), self.H, self.W, self.K, C.byref(self.params), self.res.data_ptr(),
                                           self.counts.data_ptr() if self.counts is not None else None, self.ws.data_ptr(), self.nbytes,
                                           torch.cuda.current_stream(self.dev).cuda_stream), "ovm_geo_ground_plane")
        self.launched = True
        return self

    def read(self):
        if not self.launched:
            self.launch()
        return _lib.OvmGroundResult.from_buffer_copy(self.res.cpu().numpy().tobytes())


def ground_plane(depth: torch.Tensor, K, params: GroundParams = GroundParams()) -> GroundCall:
    """The floor of a metric depth map (float32 [H, W] on the device): a launched ``GroundCall``. Nothing is read back; hand it to
    ``lift`` / ``lift_boxes`` as ``frame``, and ``read()`` it for the plane."""
    return GroundCall(depth, K, params).launch()


def _frame_tensor(frame, dev) -> Optional[torch.Tensor]:
    if frame is None:
        return None
    if isinstance(frame, GroundCall):
        if not frame.launched:
            frame.launch()
        frame = frame.frame
    _need_hip(frame, "frame")
    if frame.dtype != torch.float64 or frame.numel() != 9 or frame.device != dev:
        raise ValueError("frame must be 9 float64 values on the depth map's device, or a GroundCall")
    return frame.contiguous()


class LiftCall:
    """The arguments of one ``ovm_geo_lift`` call, prepared once: ``launch()`` enqueues it on the current stream (no read, no
    synchronisation), ``read()`` fetches the results (the one device-to-host read of the lift)."""

    def __init__(self, depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams(), want_labels: bool = False,
                 frame=None):
        self.L = _lib.load()
        _need_hip(depth, "depth")
        if depth.dtype != torch.float32 or depth.dim() != 2:
            raise ValueError("depth must be float32 [H, W]")
        self.depth = depth.contiguous()
        H, W = self.depth.shape
        self.H, self.W, self.dev = H, W, depth.device
        self.frame = _frame_tensor(frame, self.dev)                      # device [9] or None: the level camera of the reference
        n = len(masks) if masks is not None else (len(boxes_xyxy) if boxes_xyxy is not None else 0)
        if boxes_xyxy is not None and len(boxes_xyxy) != n:
            raise ValueError("boxes_xyxy and masks differ in length")
        self.n = n
        if n == 0:
            return
        if isinstance(boxes_xyxy, torch.Tensor):
            boxes_xyxy = boxes_xyxy.detach().cpu().numpy()
        self.K = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9).tolist())
        planes: List[Optional[torch.Tensor]] = []
        for i in range(n):
            m = masks[i] if masks is not None else None
            if m is None:
                if boxes_xyxy is None:
                    raise ValueError(f"instance {i}: neither a mask nor a box")
                planes.append(None)
                continue
            _need_hip(m, f"masks[{i}]")
            if tuple(m.shape) != (H, W) or m.dtype not in (torch.uint8, torch.bool):
                raise ValueError(f"masks[{i}] must be uint8 or bool [{H}, {W}]")
            planes.append(m.contiguous().view(torch.uint8))
        counts = {}
        have = [i for i in range(n) if planes[i] is not None]
        if have:                                                         # one read for all mask planes of the image
            counts = dict(zip(have, torch.stack([planes[i].ne(0).sum() for i in have]).tolist()))
        self.inst = (_lib.OvmGeoInstance * n)()
        self.keep = [planes]
        self.params = params.to_c()
        for i in range(n):
            if planes[i] is not None:
                self.inst[i].mask = planes[i].data_ptr()
                npts = int(counts[i])
            else:
                r = box_to_rect(boxes_xyxy[i])
                for k in range(4):
                    self.inst[i].rect[k] = max(-2 ** 31 + 1, min(2 ** 31 - 1, r[k]))
                npts = max(0, min(r[2], W) - max(r[0], 0)) * max(0, min(r[3], H) - max(r[1], 0))
            self.inst[i].n_points = npts
            if npts > params.max_points:
                p = _perm_on(npts, self.dev)
                self.keep.append(p)
                self.inst[i].perm = p.data_ptr()
        nbytes = C.c_int64()
        self.offs = (C.c_int64 * (n + 1))()
        _check(self.L.ovm_geo_lift_workspace(self.inst, n, H, W, C.byref(self.params), C.byref(nbytes), self.offs), "ovm_geo_lift_workspace")
        self.nbytes = int(nbytes.value)
        self.ws = torch.empty(max(self.nbytes, 1), dtype=torch.uint8, device=self.dev)
        self.res = torch.empty(n * C.sizeof(_lib.OvmGeoResult), dtype=torch.uint8, device=self.dev)
        self.labels = torch.empty(max(int(self.offs[n]), 1), dtype=torch.int32, device=self.dev) if want_labels else None

    def launch(self, last_stage: Optional[int] = None) -> None:
        if self.n == 0:
            return
        if last_stage is not None:
            self.params.last_stage = last_stage
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        _check(self.L.ovm_geo_lift_frame(self.depth.data_ptr(), self.H, self.W, self.K, self.inst, self.n, C.byref(self.params),
                                         self.frame.data_ptr() if self.frame is not None else None, self.res.data_ptr(),
                                         self.labels.data_ptr() if self.labels is not None else None, self.ws.data_ptr(), self.nbytes, stream),
               "ovm_geo_lift_frame")

    def read(self):
        if self.n == 0:
            return [], []
        host = self.res.cpu().numpy().tobytes()
        size = C.sizeof(_lib.OvmGeoResult)
        results = [_lib.OvmGeoResult.from_buffer_copy(host, i * size) for i in range(self.n)]
        lab = []
        if self.labels is not None:
            lh = self.labels.cpu().numpy()
            lab = [lh[int(self.offs[i]):int(self.offs[i + 1])].copy() for i in range(self.n)]
        return results, lab


def lift(depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams(), want_labels: bool = False, frame=None):
    """One ``ovm_geo_lift`` call. depth: float32 [H, W] on the device. Instance i is ``masks[i]`` (a [H, W] uint8 / bool device
    tensor, nonzero = inside) when given and not None, else the rectangle of ``boxes_xyxy[i]``. Returns (results, labels):
    a list of ``OvmGeoResult`` and, with ``want_labels``, the per-instance label arrays of the last trial run. ``frame`` (a
    ``GroundCall`` or 9 float64 values on the device): the points are turned by it before the fit (``ovm_geo_lift_frame``)."""
    call = LiftCall(depth, K, boxes_xyxy, masks, params, want_labels, frame)
    call.launch()
    return call.read()


def host_box(result, K, frame=None) -> dict:
    """The reference's record fields of one lifted instance (``ovm_host_geo_box``: host, fp64, no GPU). ``frame`` (9 host values):
    the frame the instance was lifted in; the box is turned back into the camera's (``ovm_host_geo_box_frame``)."""
    L = _lib.load()
    Kd = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9).tolist())
    b = _lib.OvmGeoBox()
    if frame is None:
        _check(L.ovm_host_geo_box(C.byref(result), Kd, C.byref(b)), "ovm_host_geo_box")
    else:
        Fd = (C.c_double * 9)(*np.asarray(frame, np.float64).reshape(9).tolist())
        _check(L.ovm_host_geo_box_frame(C.byref(result), Kd, Fd, C.byref(b)), "ovm_host_geo_box_frame")
    return {"bbox3D": [[float(v) for v in row] for row in b.bbox3D], "depth": float(b.depth), "center_cam": list(b.center_cam),
            "dimensions": list(b.dimensions), "pose": [list(b.pose[3 * r:3 * r + 3]) for r in range(3)], "center_2D": list(b.center_2D)}


def height_above_plane(box: dict, normal, offset: float) -> float:
    """The smallest n . p + d over the 8 corners of a record's box (center_cam, dimensions (W, H, L), pose; camera frame), for a plane
    (n, d) of the lift's frame p = (x, -y, -z): negative when the box sinks below the plane."""
    w, h, l = box["dimensions"]
    c, R = np.asarray(box["center_cam"], np.float64), np.asarray(box["pose"], np.float64)
    n = np.asarray(normal, np.float64) * np.array([1.0, -1.0, -1.0])         # the plane in the camera's frame
    local = np.array([[sx * l / 2, sy * h / 2, sz * w / 2] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    return float(((local @ R.T + c) @ n + float(offset)).min())


def lift_boxes(depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams(), frame=None) -> List[Optional[dict]]:
    """3D boxes for the 2D instances of one image: a dict with the reference's keys ``bbox3D`` (8 corners, float32 values),
    ``depth``, ``center_cam``, ``dimensions`` (W, H, L), ``pose`` and ``center_2D`` per instance, or None for an instance that is
    not lifted (an empty mask, fewer than 2 points, a non-finite depth under the mask, a rectangle outside the image - cases in
    which the reference divides by zero or raises).

    ``frame``: a ``GroundCall`` (or 9 float64 values on the device); the instances are lifted upright in it. With a ``GroundCall``
    that found a plane every record also gets ``"height_above_ground"`` (``height_above_plane`` against that plane, metres); one
    that found none has the identity for a frame, and the records are those of ``frame=None``."""
    results, _ = lift(depth, K, boxes_xyxy, masks, params, frame=frame)
    if frame is None:
        return [host_box(r, K) if r.status == _lib.OVM_GEO_OK else None for r in results]
    ground = frame.read() if isinstance(frame, GroundCall) else None
    if ground is not None and ground.status != _lib.OVM_GROUND_OK:
        return [host_box(r, K) if r.status == _lib.OVM_GEO_OK else None for r in results]
    U = list(ground.frame) if ground is not None else frame.cpu().numpy().reshape(9).tolist()
    out: List[Optional[dict]] = []
    for r in results:
        box = host_box(r, K, U) if r.status == _lib.OVM_GEO_OK else None
        if box is not None and ground is not None:
            box["height_above_ground"] = height_above_plane(box, list(ground.normal), ground.offset)
        out.append(box)
    return out


def dbscan(points: torch.Tensor, eps: float, min_samples: int) -> torch.Tensor:
    """labels_ of sklearn.cluster.DBSCAN(eps, min_samples) for float64 [n, 3] device points (``ovm_geo_dbscan``); int32 on the device."""
    L = _lib.load()
    _need_hip(points, "points")
    if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be float64 [n, 3]")
    points = points.contiguous()
    n = points.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=points.device)
    nbytes = C.c_int64()
    _check(L.ovm_geo_dbscan_workspace(n, C.byref(nbytes)), "ovm_geo_dbscan_workspace")
    ws = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=points.device)
    _check(L.ovm_geo_dbscan(points.data_ptr(), n, float(eps), int(min_samples), labels.data_ptr(), ws.data_ptr(), int(nbytes.value),
                            torch.cuda.current_stream(points.device).cuda_stream), "ovm_geo_dbscan")
    return labels
