"""Evaluation samples: the reference's ``cubercnn.vis.visualize_from_instances`` (cubercnn/vis/vis.py:76-296).

For every ``every``-th image a six-panel mosaic - ground truth of all classes, ground truth of the evaluated classes, predictions;
2D boxes above 3D boxes - composed on the device (``ovm_host_panels_layout`` + ``ovm_render_panels``, ovmono3d_amd/csrc/panels.hip)
and written as JPEG, and one line per dataset with the mean centre, depth, size and rotation errors of the predictions that hit a
ground-truth box of their class (host, fp64). The drawing rules and every declared deviation are listed in include/ovm3d.h and
restated in numpy by tests/panels_oracle.py. Parity with cv2 (lines, Hershey glyphs) and with pytorch3d (``fork_compat``'s rotation
error) is unpinned: neither library is available to compare against.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import lib as _lib

logger = logging.getLogger("cubercnn")

_mask_cache: Dict[Tuple[str, float], np.ndarray] = {}


def _mask(text: str, scale: float) -> np.ndarray:
    from . import text_mask
    key = (text, float(scale))
    if key not in _mask_cache:
        if len(_mask_cache) > 4096:
            _mask_cache.clear()
        _mask_cache[key] = text_mask(text, scale)
    return _mask_cache[key]


class SampleDataset:
    """What ``visualize_from_instances`` reads of a detectron2 test loader's dataset: ``_dataset[i]['annotations']`` (each with
    ``category_id`` indexing ``category_names_official``, ``bbox`` xywh, ``center_cam``, ``dimensions``, ``pose``) and ``self[i]``
    (``file_name``, ``image_id``)."""

    def __init__(self, records: Sequence[Dict]):
        self._dataset = list(records)

    def __len__(self) -> int:
        return len(self._dataset)

    def __getitem__(self, i: int) -> Dict:
        return self._dataset[i]

    @classmethod
    def from_ground_truth(cls, dicts: Sequence[Dict], gt, category_map) -> "SampleDataset":
        """Image records of ``load_omni3d_json`` with the kept annotations of an ``Omni3DGroundTruth``, their category ids mapped to
        the model's class index (datasets.py:404-433). Ignored annotations and those of a class outside the map are left out (the
        reference gives them the id -1, which would index the last class name)."""
        per_image: Dict = {}
        for a in gt.annotations:
            cid = category_map.dataset_id_to_contiguous.get(int(a["category_id"]))
            if cid is None or a.get("ignore", False):
                continue
            per_image.setdefault(a["image_id"], []).append({
                "category_id": cid, "bbox": list(a["bbox"]), "center_cam": a["center_cam"], "dimensions": a["dimensions"],
                "pose": a["R_cam"]})
        return cls([dict(d, annotations=per_image.get(d["image_id"], [])) for d in dicts])


def _pack_boxes(boxes: Sequence[Dict], H: int, flags: Optional[Sequence[bool]] = None):
    from . import get_color
    arr = (_lib.OvmPanelBox * max(len(boxes), 1))()
    masks = []
    for i, b in enumerate(boxes):
        o = arr[i]
        o.bbox[:] = [float(v) for v in b["bbox"]]
        o.center[:] = [float(v) for v in b["center_cam"]]
        o.dims[:] = [float(v) for v in b["dimensions"]]
        o.R[:] = np.asarray(b["pose"], np.float64).reshape(9).tolist()
        o.color[:3] = b["color"] if "color" in b else get_color(b["category_id"])
        o.draw3d = int(bool(b.get("draw3d", True)))
        o.in_eval = int(bool(flags[i])) if flags is not None else 0
        m2, m3 = _mask(str(b["name"]), 0.5), _mask(str(b["name"]), 0.50 * H / 500)
        o.glyph2d[:] = [m2.shape[1], m2.shape[0]]
        o.glyph3d[:] = [m3.shape[1], m3.shape[0]]
        masks += [m2, m3]
    return arr, masks


def panels_layout(K, height: int, width: int, gt_all: Sequence[Dict], gt_eval: Sequence[bool], preds: Sequence[Dict]):
    """Host geometry (``ovm_host_panels_layout``): (layout, prims ctypes array, glyphs uint8 array). No GPU."""
    if len(gt_eval) != len(gt_all):
        raise ValueError("render_panels: gt_eval holds one flag per box of gt_all")
    L = _lib.load()
    gt, gm = _pack_boxes(gt_all, height, gt_eval)
    pr, pm = _pack_boxes(preds, height)
    inp = _lib.OvmPanelsInput()
    inp.height, inp.width, inp.n_gt, inp.n_pred = int(height), int(width), len(gt_all), len(preds)
    inp.K[:] = np.asarray(K, np.float64).reshape(9).tolist()
    inp.gt, inp.pred = C.addressof(gt), C.addressof(pr)
    lay = _lib.OvmPanelsLayout()
    cap = 22 * (2 * len(gt_all) + len(preds)) + 1
    while True:
        prims = (_lib.OvmPanelPrim * cap)()
        rc = L.ovm_host_panels_layout(C.byref(inp), C.byref(lay), prims, cap)
        if rc == -5 and lay.n_prims > cap:                    # OVM_ERR_CAPACITY: n_prims holds the count needed
            cap = int(lay.n_prims)
            continue
        _lib.check(rc, what="ovm_host_panels_layout")
        break
    glyphs = np.concatenate([m.reshape(-1) for m in gm + pm]) if gm or pm else np.zeros(0, np.uint8)
    return lay, prims, np.ascontiguousarray(glyphs, np.uint8)


def render_panels(image_bgr_device: torch.Tensor, K, gt_all: Sequence[Dict], gt_eval: Sequence[bool], preds: Sequence[Dict], *,
                  out: Optional[torch.Tensor] = None, save_path: Optional[str] = None, gpu_jpeg: bool = True) -> torch.Tensor:
    """The six-panel mosaic of one image, device uint8 [2H, 3W, 3] (BGR). save_path: the mosaic is also written there as a JPEG of
    quality 95 (:274); gpu_jpeg: encoded on the device (data/gpu_jpeg.py write_jpeg), else copied to the host and saved with Pillow -
    the same bytes either way.

    image_bgr_device: device uint8 [H, W, 3] (rows may be pitched). gt_all / preds: one dict per box with ``bbox`` (xywh),
    ``center_cam``, ``dimensions`` (w, h, l), ``pose`` (3 x 3), ``category_id`` (its colour, or ``color``), ``name`` and, optionally,
    ``draw3d`` (False: the box appears in the 2D panel only). gt_eval: one flag per box of gt_all - the box also appears in the
    middle column. out: a device uint8 [2H, 3W, 3] view to render into (rows may be pitched).
    """
    img = image_bgr_device
    if not torch.is_tensor(img) or not img.is_cuda:
        raise RuntimeError("render_panels renders on the HIP device only (no CPU fallback)")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("render_panels: image must be uint8 [H, W, 3]")
    if img.stride(2) != 1 or img.stride(1) != 3:
        img = img.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    lay, prims, glyphs = panels_layout(K, H, W, gt_all, gt_eval, preds)
    L = _lib.load()
    ws_bytes = C.c_int64()
    _lib.check(L.ovm_render_panels_workspace(C.byref(lay), C.byref(ws_bytes)), what="ovm_render_panels_workspace")
    with torch.cuda.device(img.device):
        if out is None:
            out = torch.empty((2 * H, 3 * W, 3), dtype=torch.uint8, device=img.device)
        elif (out.device != img.device or out.dtype != torch.uint8 or tuple(out.shape) != (2 * H, 3 * W, 3) or out.stride(2) != 1
              or out.stride(1) != 3):
            raise ValueError("render_panels: out must be a device uint8 [2H, 3W, 3] view with packed pixels")
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=img.device)
        stream = torch.cuda.current_stream(img.device)
        rc = L.ovm_render_panels(C.byref(lay), prims, glyphs.ctypes.data if glyphs.size else None, glyphs.size, img.data_ptr(),
                                 img.stride(0), out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
                                 C.c_void_p(stream.cuda_stream))
        _lib.check(rc, what="ovm_render_panels")
        if save_path is not None:
            from ..data.gpu_jpeg import write_jpeg
            write_jpeg(save_path, out, quality=95, channel_order="BGR", use_device=gpu_jpeg)
    return out


def _image_matches(im_obj: Dict, data_obj: Dict) -> bool:
    """:133-150 - a string id is compared by file base name, two int ids by value; anything else does not match."""
    a, b = im_obj.get("image_id"), data_obj.get("image_id")
    if isinstance(a, str):
        return a.split("/")[-1] == str(data_obj["file_name"]).split("/")[-1]
    if isinstance(a, int) and isinstance(b, int) and not isinstance(a, bool) and not isinstance(b, bool):
        return a == b
    return False


def _sum9(a: np.ndarray) -> np.ndarray:
    s = a[:, 0]
    for k in range(1, 9):
        s = s + a[:, k]
    return s


def match_errors(im_obj: Dict, annos: Sequence[Dict], fork_compat: bool = False):
    """One image's matched-prediction errors (:204-254), vectorised, fp64: lists (xy, z, w, h, l, ry) in instance order."""
    inst = im_obj["instances"]
    if not inst or not annos:
        return [], [], [], [], [], []
    K = np.asarray(im_obj["K"], np.float64).reshape(3, 3)
    g = np.asarray([a["bbox"] for a in annos], np.float64).reshape(-1, 4)
    gx1, gy1, gx2, gy2 = g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    gcat = np.asarray([a["category_id"] for a in annos])
    p = np.asarray([i["bbox"] for i in inst], np.float64).reshape(-1, 4)
    px1, py1, px2, py2 = p[:, 0:1], p[:, 1:2], p[:, 0:1] + p[:, 2:3], p[:, 1:2] + p[:, 3:4]
    pcat = np.asarray([i["category_id"] for i in inst])
    with np.errstate(invalid="ignore", divide="ignore"):
        iw = np.clip(np.minimum(px2, gx2) - np.maximum(px1, gx1), 0, None)
        ih = np.clip(np.minimum(py2, gy2) - np.maximum(py1, gy1), 0, None)
        inter = iw * ih
        iou = inter / (((px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1)) - inter)
    same = pcat[:, None] == gcat[None, :]
    q = np.where(same, iou, -np.inf)
    near = q.argmax(1)                                           # the first maximum among the ground truth of the class
    best = q[np.arange(len(inst)), near]
    hit = np.flatnonzero(same.any(1) & (best >= 0.5))
    if len(hit) == 0:
        return [], [], [], [], [], []
    gi = near[hit]
    gc = np.asarray([annos[j]["center_cam"] for j in gi], np.float64).reshape(-1, 3)
    gd = np.asarray([annos[j]["dimensions"] for j in gi], np.float64).reshape(-1, 3)
    gr = np.asarray([annos[j]["pose"] for j in gi], np.float64).reshape(-1, 9)
    c2 = np.asarray([inst[j]["center_2D"] for j in hit], np.float64).reshape(-1, 2)
    pz = np.asarray([inst[j]["center_cam"][2] for j in hit], np.float64)
    pd = np.asarray([inst[j]["dimensions"] for j in hit], np.float64).reshape(-1, 3)
    pr = np.asarray([inst[j]["pose"] for j in hit], np.float64).reshape(-1, 9)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (K[2, 0] * gc[:, 0] + K[2, 1] * gc[:, 1]) + K[2, 2] * gc[:, 2]
        dx = c2[:, 0] - ((K[0, 0] * gc[:, 0] + K[0, 1] * gc[:, 1]) + K[0, 2] * gc[:, 2]) / w
        dy = c2[:, 1] - ((K[1, 0] * gc[:, 0] + K[1, 1] * gc[:, 1]) + K[1, 2] * gc[:, 2]) / w
        xy = np.sqrt(dx * dx + dy * dy)
    trace = _sum9(pr * gr)                                       # trace(R_pred @ R_gt^T), summed in row-major order
    if fork_compat:
        ok = (trace >= -1 - 1e-4) & (trace <= 3 + 1e-4)          # outside: the ValueError the fork swallows
        ry = (math.pi / 2 - (trace[ok] - 1) / 2).tolist()
    else:
        ry = np.arccos(np.clip((trace - 1) / 2, -1.0, 1.0)).tolist()
    return (xy.tolist(), np.abs(pz - gc[:, 2]).tolist(), np.abs(pd[:, 0] - gd[:, 0]).tolist(), np.abs(pd[:, 1] - gd[:, 1]).tolist(),
            np.abs(pd[:, 2] - gd[:, 2]).tolist(), ry)


def panel_boxes(im_obj: Dict, annos: Sequence[Dict], category_names_official: Sequence[str],
                prompted_category_names: Sequence[str]):
    """One sample's boxes for ``render_panels`` (:172-274): (K, gt_all, gt_eval, preds). A prediction's centre is
    K^-1 @ (z * [center_2D, 1]); its cuboid and label are drawn when score > sqrt(1 / n_classes) * 1.2 (strictly)."""
    thres = np.sqrt(1 / len(category_names_official)) * 1.2
    prompted = set(prompted_category_names)
    K = np.array(im_obj["K"], np.float64).reshape(3, 3)
    K_inv = np.linalg.inv(K)
    gt_all = [dict(a, name=category_names_official[a["category_id"]]) for a in annos]
    gt_eval = [b["name"] in prompted for b in gt_all]
    preds = []
    for inst in im_obj["instances"]:
        z3d = inst["center_cam"][2]
        center = K_inv @ (z3d * np.array(list(inst["center_2D"]) + [1], np.float64))
        preds.append({"category_id": inst["category_id"], "name": category_names_official[inst["category_id"]],
                      "bbox": inst["bbox"], "center_cam": center, "dimensions": inst["dimensions"], "pose": inst["pose"],
                      "draw3d": bool(inst["score"] > thres)})
    return K, gt_all, gt_eval, preds


def _mean(v: Sequence[float]) -> float:
    return float(np.mean(v)) if len(v) else float("nan")


def visualize_from_instances(detections, dataset, dataset_name, min_size_test, output_folder, category_names_official,
                             prompted_category_names, iteration="", *, every: int = 50, fork_compat: bool = False, device=None,
                             gpu_jpeg: bool = True) -> str:
    """Writes ``<output_folder>/vis/<dataset_name>_<imind:06d>.jpg`` for the images with ``imind % every == 0`` and returns the
    reference's log line ``<dataset_name>iter=<iteration>, xy(..), z(..), whl(.., .., ..), ry(..)``.

    The positional arguments are the reference's. ``every=0`` writes nothing. Default: the errors are taken over all images and
    ry is the geodesic angle acos(clip((trace - 1) / 2, -1, 1)) (upstream Cube R-CNN). ``fork_compat=True``: over the sampled images
    only and ry = pi / 2 - (trace - 1) / 2, the pair dropped when the trace is outside [-1 - 1e-4, 3 + 1e-4] (what pytorch3d's
    ``so3_relative_angle(..., cos_bound=1)`` computes, read from its source; parity unpinned). ``device``: where the panels are drawn
    (default: the current HIP device); without sampled images the GPU is not touched. ``gpu_jpeg``: the samples are encoded on the
    device (``write_jpeg``); False: copied to the host and saved with Pillow, as the reference does - the files are the same.
    """
    vis_folder = os.path.join(output_folder, "vis")
    os.makedirs(vis_folder, exist_ok=True)
    errs: Tuple[List[float], ...] = ([], [], [], [], [], [])
    every = int(every)
    for imind, im_obj in enumerate(detections):
        write_sample = every > 0 and imind % every == 0
        if fork_compat and not write_sample:
            continue
        annos = dataset._dataset[imind]["annotations"]
        if len(annos) == 0:
            continue
        data_obj = dataset[imind]
        if not _image_matches(im_obj, data_obj):
            logger.warning("visualize_from_instances: image %d: detections of %r do not belong to %r (%r); skipped", imind,
                           im_obj.get("image_id"), data_obj.get("image_id"), data_obj.get("file_name"))
            continue
        for dst, src in zip(errs, match_errors(im_obj, annos, fork_compat)):
            dst += src
        if not write_sample:
            continue
        from ..data.gpu_jpeg import read_image_device
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        im = read_image_device(data_obj["file_name"], "BGR", dev)
        K, gt_all, gt_eval, preds = panel_boxes(im_obj, annos, category_names_official, prompted_category_names)
        render_panels(im, K, gt_all, gt_eval, preds, save_path=os.path.join(vis_folder, f"{dataset_name}_{imind:06d}.jpg"),
                      gpu_jpeg=gpu_jpeg)
    ry = errs[5] if len(errs[5]) else [1000, 1000]               # :286-287
    return dataset_name + "iter={}, xy({:.2f}), z({:.2f}), whl({:.2f}, {:.2f}, {:.2f}), ry({:.2f})\n".format(
        iteration, _mean(errs[0]), _mean(errs[1]), _mean(errs[2]), _mean(errs[3]), _mean(errs[4]), _mean(ry))
