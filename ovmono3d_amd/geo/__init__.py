"""OVMono3D-GEO: lift 2D boxes to 3D from metric depth and masks (reference tools/ovmono3d_geo.py:127-258) on the device.

``lift_boxes`` runs the whole geometric part - un-projection, PCA yaw, DBSCAN outlier removal, extent fit - for all instances of
one image in one call of ``ovm_geo_lift`` (ovmono3d_amd/csrc/geo.hip), then builds the reference's record fields on the host with
``ovm_host_geo_box``. Of the two networks the reference runs in front of it, SAM is ``ovmono3d_amd.sam`` (its ``predict_boxes``
planes are device tensors ``masks`` takes as they are); Depth Pro is not here: the depth map arrives as an array. Masks may also
come from files, or the 2D box itself is the mask: ``geo.sources`` holds every source of boxes and masks the two front ends
(tools/ovmono3d_geo.py, demo/demo_geo.py) put in front of ``lift_boxes``, and their command-line flags.
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


class LiftCall:
    """The arguments of one ``ovm_geo_lift`` call, prepared once: ``launch()`` enqueues it on the current stream (no read, no
    synchronisation), ``read()`` fetches the results (the one device-to-host read of the lift)."""

    def __init__(self, depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams(), want_labels: bool = False):
        self.L = _lib.load()
        _need_hip(depth, "depth")
        if depth.dtype != torch.float32 or depth.dim() != 2:
            raise ValueError("depth must be float32 [H, W]")
        self.depth = depth.contiguous()
        H, W = self.depth.shape
        self.H, self.W, self.dev = H, W, depth.device
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
        _check(self.L.ovm_geo_lift(self.depth.data_ptr(), self.H, self.W, self.K, self.inst, self.n, C.byref(self.params), self.res.data_ptr(),
                                   self.labels.data_ptr() if self.labels is not None else None, self.ws.data_ptr(), self.nbytes, stream),
               "ovm_geo_lift")

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


def lift(depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams(), want_labels: bool = False):
    """One ``ovm_geo_lift`` call. depth: float32 [H, W] on the device. Instance i is ``masks[i]`` (a [H, W] uint8 / bool device
    tensor, nonzero = inside) when given and not None, else the rectangle of ``boxes_xyxy[i]``. Returns (results, labels):
    a list of ``OvmGeoResult`` and, with ``want_labels``, the per-instance label arrays of the last trial run."""
    call = LiftCall(depth, K, boxes_xyxy, masks, params, want_labels)
    call.launch()
    return call.read()


def host_box(result, K) -> dict:
    """The reference's record fields of one lifted instance (``ovm_host_geo_box``: host, fp64, no GPU)."""
    L = _lib.load()
    Kd = (C.c_double * 9)(*np.asarray(K, np.float64).reshape(9).tolist())
    b = _lib.OvmGeoBox()
    _check(L.ovm_host_geo_box(C.byref(result), Kd, C.byref(b)), "ovm_host_geo_box")
    return {"bbox3D": [[float(v) for v in row] for row in b.bbox3D], "depth": float(b.depth), "center_cam": list(b.center_cam),
            "dimensions": list(b.dimensions), "pose": [list(b.pose[3 * r:3 * r + 3]) for r in range(3)], "center_2D": list(b.center_2D)}


def lift_boxes(depth: torch.Tensor, K, boxes_xyxy=None, masks=None, params: GeoParams = GeoParams()) -> List[Optional[dict]]:
    """3D boxes for the 2D instances of one image: a dict with the reference's keys ``bbox3D`` (8 corners, float32 values),
    ``depth``, ``center_cam``, ``dimensions`` (W, H, L), ``pose`` and ``center_2D`` per instance, or None for an instance that is
    not lifted (an empty mask, fewer than 2 points, a non-finite depth under the mask, a rectangle outside the image - cases in
    which the reference divides by zero or raises)."""
    results, _ = lift(depth, K, boxes_xyxy, masks, params)
    return [host_box(r, K) if r.status == _lib.OVM_GEO_OK else None for r in results]


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
