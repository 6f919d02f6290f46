"""Segment Anything on the device: the mask source of OVMono3D-GEO (reference tools/ovmono3d_geo.py:213-217,270-272,308-309 -
segment_anything's ``SamPredictor.set_image`` then ``predict(box=...)``, plane ``[2]`` of the multimask outputs) and the rest of the
predictor's prompt surface: clicks (foreground, background, padding), a box with clicks, a previous low-resolution mask fed back
as ``mask_input``, and the single-mask output.

``build_sam(arch, checkpoint)`` loads a segment_anything checkpoint by its own key names into libovm3d's ``OvmSam`` handle
(csrc/sam.hip): image encoder (the OVM_TOWER_SAM blocks + neck), prompt encoder, two-way-transformer mask decoder and
``postprocess_masks`` all run there; masks come back as device uint8 planes that ``ovmono3d_amd.geo.lift_boxes`` takes as they
are. There is no CPU or PyTorch path.

Scope: ``vit_b`` and ``vit_l``. ``vit_h`` (the reference's "default") has head dimension 80; the attention kernels take 64, so the
library refuses it (``OVM_ERR_UNSUPPORTED``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from .. import lib as _lib
from ..util.synth_weights import SAM_ARCH

# (width, layers, heads, patch, checkpoint grid, window, global-attention blocks): segment_anything build_sam_vit_h
VIT_H = (1280, 32, 16, 16, 64, 14, (7, 15, 23, 31))
PIXEL_MEAN = (123.675, 116.28, 103.53)
PIXEL_STD = (58.395, 57.12, 57.375)
MAX_POINTS = 8                       # points per prompt (csrc/sam.hip: 5 + 8 + 2 = 15 of the 16 tokens its second attention kernel holds)
CAND_WORDS = C.sizeof(_lib.OvmSamCandidate) // 4          # an OvmSamCandidate as int32 words
MAX_AUTO_POINTS = 4096 // 3          # 3 candidates per point must fit the 4,096 rows the NMS takes: points_per_side <= 36


def candidate_fields(table) -> Dict[str, np.ndarray]:
    """A candidate table (int32 [m, 16], device or host) as named host arrays: the fields of ``OvmSamCandidate``."""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    t = np.ascontiguousarray(t, np.int32).reshape(-1, CAND_WORDS)
    return {"iou": t[:, 0].copy().view(np.float32), "stability": t[:, 1].copy().view(np.float32), "area": t[:, 2].copy(), "box": t[:, 3:7].copy(),
            "cnt_hi": t[:, 7].copy(), "cnt_lo": t[:, 8].copy(), "flags": t[:, 9].copy()}


def check_prompts(point_coords=None, point_labels=None, boxes=None, mask_inputs=None, low_side: Optional[int] = None):
    """The argument rules of ``predict`` / ``predict_prompts``, on the host and before any device call. Returns
    ``(n, P, coords float32 [n, P, 2] | None, labels int32 [n, P] | None, boxes float32 [n, 4] | None)``; ``mask_inputs`` is only
    checked for its shape ([n, L, L], L = ``low_side`` when given). ValueError for: no prompt at all, coordinates without labels (or
    the reverse), more than MAX_POINTS points, a label outside {1, 0, -1}, counts that differ between the arguments."""
    def host(x, dtype):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        return np.asarray(x, dtype)

    if (point_coords is None) != (point_labels is None):
        raise ValueError("point_coords and point_labels come together")
    coords = labels = bx = None
    n = None
    if point_coords is not None:
        coords, lab = host(point_coords, np.float32), host(point_labels, np.float64)
        if coords.ndim != 3 or coords.shape[-1] != 2 or lab.shape != coords.shape[:2]:
            raise ValueError(f"point_coords must be [n, P, 2] and point_labels [n, P], are {coords.shape} and {lab.shape}")
        if coords.shape[1] > MAX_POINTS:
            raise ValueError(f"at most {MAX_POINTS} points per prompt, got {coords.shape[1]}")
        bad = sorted(set(np.unique(lab).tolist()) - {1.0, 0.0, -1.0})
        if bad:
            raise ValueError(f"point labels must be 1 (foreground), 0 (background) or -1 (padding), got {bad}")
        labels = lab.astype(np.int32)
        n = coords.shape[0]
        if coords.shape[1] == 0:
            coords = labels = None
    if boxes is not None:
        bx = host(boxes, np.float32).reshape(-1, 4)
        if n is not None and bx.shape[0] != n:
            raise ValueError(f"{bx.shape[0]} boxes for {n} point prompts")
        n = bx.shape[0]
    if coords is None and bx is None:
        raise ValueError("a prompt needs points or a box")
    if mask_inputs is not None:
        shp = tuple(mask_inputs.shape)
        if len(shp) != 3 or shp[0] != n or shp[1] != shp[2] or (low_side is not None and shp[1] != low_side):
            raise ValueError(f"mask_inputs must be [{n}, L, L] with L = {low_side if low_side is not None else '4 x grid'}, is {shp}")
    return n, (0 if coords is None else coords.shape[1]), coords, labels, bx


def sam_config(arch: str, image_size: Optional[int] = None, precision: int = 3, max_boxes: int = 16) -> "_lib.OvmSamConfig":
    if arch in ("vit_h", "default"):
        D, L, heads, patch, grid, window, glob = VIT_H
    elif arch in SAM_ARCH:
        D, L, heads, patch, grid, window, glob = SAM_ARCH[arch]
    else:
        raise ValueError(f"unknown SAM architecture {arch!r} (known: {sorted(SAM_ARCH) + ['vit_h']})")
    c = _lib.OvmSamConfig()
    c.embed_dim, c.depth, c.heads, c.patch, c.window = D, L, heads, patch, window
    c.image_size = int(image_size) if image_size else grid * patch
    c.pos_grid = c.image_size // patch
    c.global_mask = sum(1 << i for i in glob)
    c.prompt_dim, c.dec_depth, c.dec_heads, c.dec_mlp, c.attn_downsample = 256, 2, 8, 2048, 2
    c.num_mask_tokens, c.iou_depth, c.iou_hidden = 4, 3, 256
    for i in range(3):
        c.pixel_mean[i], c.pixel_std[i] = PIXEL_MEAN[i], PIXEL_STD[i]
    c.precision, c.max_boxes = int(precision), int(max_boxes)
    return c


class SamEngine:
    """Owner of one ``OvmSam`` handle."""

    def __init__(self, cfg: "_lib.OvmSamConfig", state_dict: Dict[str, torch.Tensor], device: Optional[torch.device] = None):
        self.L = _lib.load()
        self.cfg = cfg
        self.dev = device if device is not None else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        host = {k: np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy()) for k, v in state_dict.items()
                if torch.is_tensor(v) and v.dtype.is_floating_point and v.dim() <= 4}
        table, keep = _lib.make_tensor_table(host)
        self._h = C.c_void_p()
        rc = self.L.ovm_sam_create(C.byref(cfg), table, len(host), self.dev.index or 0, C.byref(self._h))
        del keep
        if rc != 0:
            msg = (self.L.ovm_sam_last_error(self._h) or b"").decode() if self._h else ""
            if self._h:
                self.L.ovm_sam_destroy(self._h)
                self._h = None
            raise _lib.OvmError(f"ovm_sam_create failed with code {rc}: {msg}")
        self.grid = cfg.image_size // cfg.patch
        self._ws = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self.L.ovm_sam_destroy(h)
            except Exception:
                pass

    def _chk(self, rc, what):
        if rc != 0:
            raise _lib.OvmError(f"{what} failed with code {rc}: {(self.L.ovm_sam_last_error(self._h) or b'').decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def set_image(self, image_hwc: torch.Tensor, flip: bool) -> None:
        d = _lib.OvmImage()
        d.data = image_hwc.data_ptr()
        d.height, d.width = int(image_hwc.shape[0]), int(image_hwc.shape[1])
        d.stride_h, d.stride_w, d.stride_c = (int(s) for s in image_hwc.stride())
        d.orig_height, d.orig_width = d.height, d.width
        self._chk(self.L.ovm_sam_set_image(self._h, C.byref(d), int(flip), self._stream()), "ovm_sam_set_image")

    def workspace(self, n: int) -> torch.Tensor:
        nbytes = C.c_int64()
        self._chk(self.L.ovm_sam_predict_boxes_workspace(self._h, int(n), C.byref(nbytes)), "ovm_sam_predict_boxes_workspace")
        if self._ws is None or self._ws.numel() < nbytes.value:
            self._ws = None
            self._ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.dev)
        return self._ws

    def predict_boxes(self, boxes: torch.Tensor, H: int, W: int, mask_index: int, want_iou: bool = False, want_lowres: bool = False,
                      workspace: Optional[torch.Tensor] = None):
        n = int(boxes.shape[0])
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=self.dev)
        iou = torch.empty((n, 3), dtype=torch.float32, device=self.dev) if want_iou else None
        low = torch.empty((n, 3, 4 * self.grid, 4 * self.grid), dtype=torch.float32, device=self.dev) if want_lowres else None
        if n:
            ws = workspace if workspace is not None else self.workspace(n)
            self._chk(self.L.ovm_sam_predict_boxes(self._h, boxes.data_ptr(), n, int(mask_index), masks.data_ptr(),
                                                   iou.data_ptr() if iou is not None else None, low.data_ptr() if low is not None else None,
                                                   ws.data_ptr(), ws.numel(), self._stream()), "ovm_sam_predict_boxes")
        return masks, iou, low

    def prompt_workspace(self, n: int, n_points: int, has_box: bool, has_mask: bool) -> torch.Tensor:
        nbytes = C.c_int64()
        self._chk(self.L.ovm_sam_predict_workspace(self._h, int(n), int(n_points), int(has_box), int(has_mask), C.byref(nbytes)),
                  "ovm_sam_predict_workspace")
        if self._ws is None or self._ws.numel() < nbytes.value:
            self._ws = None
            self._ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.dev)
        return self._ws

    def predict_prompts(self, coords: Optional[torch.Tensor], labels: Optional[torch.Tensor], boxes: Optional[torch.Tensor],
                        mask_inputs: Optional[torch.Tensor], H: int, W: int, multimask: bool = True, mask_index: int = 2, want_iou: bool = False,
                        want_lowres: bool = False, workspace: Optional[torch.Tensor] = None):
        """ovm_sam_predict on device tensors already checked (``check_prompts``): coords fp32 [n, P, 2], labels int32 [n, P], boxes
        fp32 [n, 4], mask_inputs fp32 [n, L, L]; any of them None. (masks uint8 [n, H, W], iou [n, K] | None, lowres [n, K, L, L] | None)."""
        n = int(coords.shape[0] if coords is not None else boxes.shape[0])
        P = int(coords.shape[1]) if coords is not None else 0
        K, Ls = (3 if multimask else 1), 4 * self.grid
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=self.dev)
        iou = torch.empty((n, K), dtype=torch.float32, device=self.dev) if want_iou else None
        low = torch.empty((n, K, Ls, Ls), dtype=torch.float32, device=self.dev) if want_lowres else None
        if n:
            ws = workspace if workspace is not None else self.prompt_workspace(n, P, boxes is not None, mask_inputs is not None)
            ptr = lambda t: t.data_ptr() if t is not None else None                                     # noqa: E731
            self._chk(self.L.ovm_sam_predict(self._h, ptr(coords), ptr(labels), P, ptr(boxes), ptr(mask_inputs), n, int(bool(multimask)), int(mask_index),
                                             masks.data_ptr(), ptr(iou), ptr(low), ws.data_ptr(), ws.numel(), self._stream()), "ovm_sam_predict")
        return masks, iou, low

    def mask_boxes(self, masks: torch.Tensor):
        """masks: device uint8 [n, H, W]. (boxes fp32 [n, 4] = (xmin, ymin, xmax + 1, ymax + 1), pixel counts int32 [n]); zeros for an empty mask."""
        n, H, W = (int(v) for v in masks.shape)
        boxes = torch.empty((n, 4), dtype=torch.float32, device=self.dev)
        counts = torch.empty((n,), dtype=torch.int32, device=self.dev)
        if n:
            self._chk(self.L.ovm_sam_mask_boxes(masks.data_ptr(), n, H, W, boxes.data_ptr(), counts.data_ptr(), self._stream()), "ovm_sam_mask_boxes")
        return boxes, counts

    def auto_candidates(self, points: torch.Tensor, pred_iou_thresh: float, offset: float, out: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ovm_sam_auto_candidates: points device fp32 [n, 2] (x, y) -> the candidate table, device int32 [3 n, 16] (the words of
        ``OvmSamCandidate``; ``candidate_fields`` names them). ``out``: a slice of a larger table to fill."""
        n = int(points.shape[0])
        if out is None:
            out = torch.empty((3 * n, CAND_WORDS), dtype=torch.int32, device=self.dev)
        if n:
            ws = workspace
            if ws is None:
                nbytes = C.c_int64()
                self._chk(self.L.ovm_sam_auto_candidates_workspace(self._h, n, C.byref(nbytes)), "ovm_sam_auto_candidates_workspace")
                if self._ws is None or self._ws.numel() < nbytes.value:
                    self._ws = None
                    self._ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.dev)
                ws = self._ws
            self._chk(self.L.ovm_sam_auto_candidates(self._h, points.data_ptr(), n, float(pred_iou_thresh), float(offset), out.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), self._stream()), "ovm_sam_auto_candidates")
        return out

    def auto_select(self, cands: torch.Tensor, pred_iou_thresh: float, stability_score_thresh: float, box_nms_thresh: float):
        """ovm_sam_auto_select on a table of ``auto_candidates``: (keep_idx int32 [m], n_keep int32 [1]), device tensors."""
        m = int(cands.shape[0])
        keep = torch.empty((max(m, 1),), dtype=torch.int32, device=self.dev)
        n_keep = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        nbytes = C.c_int64()
        rc = self.L.ovm_sam_auto_select_workspace(m, C.byref(nbytes))
        ws = torch.empty(int(nbytes.value) if rc == 0 else 256, dtype=torch.uint8, device=self.dev)
        rc = self.L.ovm_sam_auto_select(cands.data_ptr(), m, float(pred_iou_thresh), float(stability_score_thresh), float(box_nms_thresh),
                                        keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        if rc != 0:
            raise _lib.OvmError(f"ovm_sam_auto_select failed with code {rc} (m = {m}; at most 4096 candidates)")
        return keep, n_keep

    def debug(self, name: str, shape) -> torch.Tensor:
        out = torch.empty(shape, dtype=torch.float32, device=self.dev)
        n = self.L.ovm_sam_debug_copy(self._h, name.encode(), out.data_ptr(), out.numel(), self._stream())
        if n < 0:
            self._chk(int(n), f"ovm_sam_debug_copy({name})")
        assert n == out.numel(), (name, n, tuple(shape))
        return out


class SamPredictor:
    """segment_anything's ``SamPredictor``: box, point and mask prompts, multimask or single-mask output."""

    def __init__(self, engine: SamEngine):
        self.engine = engine
        self.original_size = None

    def set_image(self, image, image_format: str = "RGB") -> None:
        """image: uint8 [H, W, 3], a device tensor (any strides) or a numpy array. As in segment_anything, a format other than the
        model's ("RGB") reverses the channels before normalisation."""
        if image_format not in ("RGB", "BGR"):
            raise ValueError(f"image_format must be 'RGB' or 'BGR', is {image_format!r}")
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image)).to(self.engine.dev)
        if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError("image must be uint8 [H, W, 3] on the HIP device (or a numpy array to upload)")
        self._image = image                                       # keeps the buffer alive while the stream reads it
        self.engine.set_image(image, flip=image_format != "RGB")
        self.original_size = (int(image.shape[0]), int(image.shape[1]))

    def _boxes(self, boxes) -> torch.Tensor:
        if self.original_size is None:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        b = torch.as_tensor(np.asarray(boxes, np.float32) if not isinstance(boxes, torch.Tensor) else boxes)
        return b.to(self.engine.dev, torch.float32).reshape(-1, 4).contiguous()

    def predict_boxes(self, boxes, mask_index: int = 2, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """boxes: [n, 4] xyxy in original pixels. Device uint8 [n, H, W]: plane ``mask_index`` of each box's multimask outputs."""
        b = self._boxes(boxes)
        return self.engine.predict_boxes(b, *self.original_size, mask_index, workspace=workspace)[0]

    def predict_prompts(self, point_coords=None, point_labels=None, boxes=None, mask_inputs=None, multimask_output: bool = True,
                        mask_index: int = 2, want_iou: bool = False, want_lowres: bool = False, workspace: Optional[torch.Tensor] = None):
        """n prompts of one shape in one call: point_coords [n, P, 2] (original pixels, P <= 8) with point_labels [n, P] (1 foreground,
        0 background, -1 padding), boxes [n, 4] xyxy, mask_inputs [n, L, L] (low-resolution logits of an earlier call, L = 4 x grid);
        at least points or boxes. (masks uint8 [n, H, W]: plane ``mask_index`` of the three multimask outputs, or the single mask with
        ``multimask_output=False`` (mask_index 0); iou [n, K] | None; low-res logits [n, K, L, L] | None), K = 3 or 1. Device tensors."""
        if self.original_size is None:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        if not multimask_output:
            mask_index = 0
        if not 0 <= int(mask_index) <= 2:
            raise ValueError(f"mask_index must be 0, 1 or 2, is {mask_index}")
        eng = self.engine
        _, _, coords, labels, bx = check_prompts(point_coords, point_labels, boxes, mask_inputs, 4 * eng.grid)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev)      # noqa: E731
        mi = None
        if mask_inputs is not None:
            mi = torch.as_tensor(mask_inputs).to(eng.dev, torch.float32).contiguous()
        return eng.predict_prompts(up(coords), up(labels), up(bx), mi, *self.original_size, multimask=multimask_output, mask_index=int(mask_index),
                                   want_iou=want_iou, want_lowres=want_lowres, workspace=workspace)

    def mask_boxes(self, masks: torch.Tensor):
        """The tight xyxy box (xmin, ymin, xmax + 1, ymax + 1) and the pixel count of each uint8 / bool mask plane [n, H, W], on the device."""
        m = masks.to(torch.uint8) if masks.dtype != torch.uint8 else masks
        return self.engine.mask_boxes(m.contiguous())

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output: bool = True, return_logits: bool = False):
        """segment_anything's call for one prompt: point_coords [P, 2] with point_labels [P], box [4] xyxy, mask_input [1, L, L] ->
        (masks [C, H, W] bool, iou [C], low_res [C, L, L]), C = 3 or 1, device tensors. The reference's call shape is ``predict(box=b)``."""
        if return_logits:
            raise NotImplementedError("return_logits: the masks are thresholded on the device")
        if point_coords is None and point_labels is None and box is None:
            raise ValueError("a prompt needs points or a box")
        if point_coords is None and mask_input is None and multimask_output:                  # the reference's call, as it always ran
            b = self._boxes(box)
            if b.shape[0] != 1:
                raise ValueError("predict takes one box; use predict_boxes for several")
            H, W = self.original_size
            planes = []
            iou = low = None
            for k in range(3):
                m, i, l = self.engine.predict_boxes(b, H, W, k, want_iou=k == 0, want_lowres=k == 0)
                planes.append(m[0])
                if k == 0:
                    iou, low = i[0], l[0]
            return torch.stack(planes).bool(), iou, low
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)      # noqa: E731
        pc = None if point_coords is None else as_np(point_coords).reshape(1, -1, 2)
        pl = None if point_labels is None else as_np(point_labels).reshape(1, -1)
        bx = None if box is None else as_np(box).reshape(-1, 4)
        if bx is not None and bx.shape[0] != 1:
            raise ValueError("predict takes one box; use predict_prompts for several")
        planes = []
        iou = low = None
        for k in range(3 if multimask_output else 1):
            m, i, l = self.predict_prompts(pc, pl, bx, mask_input, multimask_output, k, want_iou=k == 0, want_lowres=k == 0)
            planes.append(m[0])
            if k == 0:
                iou, low = i[0], l[0]
        return torch.stack(planes).bool(), iou, low


def build_point_grid(n_per_side: int) -> np.ndarray:
    """segment_anything's grid: n x n points in [0, 1]^2 at the cell centres, float64 [n * n, 2] as (x, y), row-major in y."""
    n = int(n_per_side)
    offset = 1 / (2 * n)
    g = np.linspace(offset, 1 - offset, n)
    return np.stack([np.tile(g[None, :], (n, 1)), np.tile(g[:, None], (1, n))], axis=-1).reshape(-1, 2)


class SamAutomaticMaskGenerator:
    """segment_anything's ``SamAutomaticMaskGenerator`` for the full image: a grid of foreground clicks, three candidates per click,
    the predicted-IoU filter, the stability filter and box NMS, all on the device (``ovm_sam_auto_candidates`` /
    ``ovm_sam_auto_select``, include/ovm3d.h states the rules). The emitted masks are ``SamPredictor.predict_prompts``'s own planes.

    Not built and refused with ValueError: crops (``crop_n_layers > 0``), ``output_mode`` other than "binary_mask" (RLE records come
    from ``generate_rle``). The small-region clean-up is a keyword of the ``generate*`` calls (``min_mask_region_area=A``:
    :meth:`postprocess_small_regions` on the device); the constructor argument of that name keeps refusing a value above 0, as
    ``output_mode`` does. The crop-edge filter never removes a mask of the full-image crop. Parity with the
    segment_anything package is not pinned by a test (the package is not a dependency); DESIGN.md section 4.4."""

    def __init__(self, predictor: SamPredictor, points_per_side: Optional[int] = 32, points_per_batch: int = 64, pred_iou_thresh: float = 0.88,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, box_nms_thresh: float = 0.7, crop_n_layers: int = 0,
                 crop_nms_thresh: float = 0.7, crop_overlap_ratio: float = 512 / 1500, crop_n_points_downscale_factor: int = 1,
                 point_grids=None, min_mask_region_area: int = 0, output_mode: str = "binary_mask"):
        if crop_n_layers > 0:
            raise ValueError(f"crop_n_layers = {crop_n_layers}: crops are not built (the full image only)")
        if min_mask_region_area > 0:
            raise ValueError(f"min_mask_region_area = {min_mask_region_area}: not a constructor argument here; the small-region clean-up is the "
                             "keyword min_mask_region_area of generate_device / generate / generate_rle")
        if output_mode != "binary_mask":
            raise ValueError(f"output_mode = {output_mode!r}: only 'binary_mask' (RLE modes are not built)")
        if (points_per_side is None) == (point_grids is None):
            raise ValueError("exactly one of points_per_side and point_grids must be given")
        if points_per_side is not None:
            if int(points_per_side) < 1:
                raise ValueError(f"points_per_side must be at least 1, is {points_per_side}")
            grid = build_point_grid(points_per_side) if int(points_per_side) ** 2 <= MAX_AUTO_POINTS else None
            npts = int(points_per_side) ** 2
            what = f"points_per_side = {points_per_side}"
        else:
            grids = point_grids if isinstance(point_grids, (list, tuple)) else [point_grids]
            if len(grids) != 1:
                raise ValueError(f"point_grids must hold one grid (crop_n_layers = 0), holds {len(grids)}")
            grid = np.asarray(grids[0], np.float64).reshape(-1, 2)
            npts = grid.shape[0]
            what = f"point_grids with {npts} points"
        if npts > MAX_AUTO_POINTS:
            raise ValueError(f"{what}: at most {MAX_AUTO_POINTS} points (3 candidates each, 4096 rows in the NMS: points_per_side <= 36)")
        if int(points_per_batch) < 1:
            raise ValueError(f"points_per_batch must be at least 1, is {points_per_batch}")
        self.predictor, self.point_grid = predictor, grid
        self.points_per_batch = int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = float(pred_iou_thresh), float(stability_score_thresh)
        self.stability_score_offset, self.box_nms_thresh = float(stability_score_offset), float(box_nms_thresh)
        self._cands = self._points = None

    def grid_points(self, H: int, W: int) -> np.ndarray:
        """The grid in the pixels of an H x W image: float32 [n, 2] (x, y), scaled in float64 as segment_anything does."""
        return (self.point_grid * np.array([W, H], np.float64)[None]).astype(np.float32)

    def candidates(self):
        """(fields of the last image's candidate table as host arrays (``candidate_fields``), its points float32 [n, 2])."""
        if self._cands is None:
            raise RuntimeError("generate() has not been called")
        return candidate_fields(self._cands), self._points.copy()

    @staticmethod
    @torch.no_grad()
    def postprocess_small_regions(out, min_area: int, nms_thresh: float):
        """segment_anything's method of this name on the dict of :meth:`generate_device`: every mask is cleaned with
        ``masks.remove_small_regions(m, min_area, "both")``; boxes and areas of the cleaned masks are recomputed; NMS by ``ovm_op_nms``'s
        rule runs over the inclusive boxes as floats with score 1.0 for an unchanged mask and 0.0 for a changed one (ties to the lower
        index), so a mask is dropped when cleaning made its box overlap a kept one's above ``nms_thresh``. The result is in keep order:
        a kept changed mask carries its cleaned plane, box and area, an unchanged one what it had; ``scores``, ``stability``,
        ``points`` and ``index`` are carried through. All on the device; the number kept is the one word read back."""
        from ..masks import remove_small_regions
        masks = out["masks"]
        m = int(masks.shape[0])
        if m == 0:
            return dict(out)
        L = _lib.load()
        dev = masks.device
        H, W = int(masks.shape[1]), int(masks.shape[2])
        with torch.cuda.device(dev):
            cleaned, changed = remove_small_regions(masks, int(min_area), "both")
            boxes = torch.empty((m, 4), dtype=torch.float32, device=dev)
            areas = torch.empty((m,), dtype=torch.int32, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(L.ovm_sam_mask_boxes(cleaned.data_ptr(), m, H, W, boxes.data_ptr(), areas.data_ptr(), stream), what="ovm_sam_mask_boxes")
            incl = boxes.clone()
            incl[:, 2:] -= (areas > 0).to(torch.float32)[:, None]          # (xmin, ymin, xmax, ymax); zeros for an empty mask
            scores = (~changed).to(torch.float32).contiguous()
            keep = torch.empty((m,), dtype=torch.int32, device=dev)
            n_keep = torch.zeros((1,), dtype=torch.int32, device=dev)
            rc = L.ovm_op_nms(incl.data_ptr(), scores.data_ptr(), m, float(nms_thresh), keep.data_ptr(), n_keep.data_ptr(), stream)
            if rc != 0:
                raise _lib.OvmError(f"ovm_op_nms failed with code {rc} (m = {m}; at most 4096 masks)")
            keep = keep[:int(n_keep.item())].to(torch.int64)
            ch = changed[keep]
            res = {k: v[keep] for k, v in out.items()}
            res["masks"] = torch.where(ch[:, None, None], cleaned[keep], out["masks"][keep])
            res["boxes"] = torch.where(ch[:, None], boxes[keep], out["boxes"][keep])
            res["areas"] = torch.where(ch, areas[keep], out["areas"][keep])
        return res

    @torch.no_grad()
    def generate_device(self, image, image_format: str = "RGB", min_mask_region_area: int = 0):
        """dict of device tensors for the kept masks, in NMS keep order: masks uint8 [m, H, W], boxes fp32 [m, 4] (xmin, ymin,
        xmax + 1, ymax + 1: ``SamPredictor.mask_boxes``), scores fp32 [m] (predicted IoU), stability fp32 [m], points fp32 [m, 2],
        areas int32 [m]; and ``index`` int64 [m]: the candidate (3 * point + plane) each mask came from.
        ``min_mask_region_area`` > 0: :meth:`postprocess_small_regions` with that area and ``nms_thresh = box_nms_thresh`` is applied to
        the result (segment_anything takes the larger of the box and crop thresholds; there are no crops here). This keyword is the
        route to the clean-up: the constructor argument of the same name keeps refusing a value above 0. 0 is the path without it."""
        if int(min_mask_region_area) < 0:
            raise ValueError(f"min_mask_region_area must not be negative, is {min_mask_region_area}")
        if int(min_mask_region_area) > 0:
            return self.postprocess_small_regions(self.generate_device(image, image_format), int(min_mask_region_area), self.box_nms_thresh)
        pred = self.predictor
        eng = pred.engine
        pred.set_image(image, image_format)
        H, W = pred.original_size
        pts_host = self.grid_points(H, W)
        pts = torch.from_numpy(pts_host).to(eng.dev)
        n = pts.shape[0]
        table = torch.empty((3 * n, CAND_WORDS), dtype=torch.int32, device=eng.dev)
        for b0 in range(0, n, self.points_per_batch):
            b1 = min(n, b0 + self.points_per_batch)
            eng.auto_candidates(pts[b0:b1], self.pred_iou_thresh, self.stability_score_offset, out=table[3 * b0:3 * b1])
        keep, n_keep = eng.auto_select(table, self.pred_iou_thresh, self.stability_score_thresh, self.box_nms_thresh)
        m = int(n_keep.item())                                     # the one read the flow needs before it can size its outputs
        keep = keep[:m].to(torch.int64)
        self._cands, self._points = table, pts_host
        masks = torch.empty((m, H, W), dtype=torch.uint8, device=eng.dev)
        if m:
            idx = keep.cpu().numpy()
            ones = torch.ones((m, 1), dtype=torch.int32, device=eng.dev)
            for k in range(3):                                     # the predictor's own planes, one call per plane
                rows = np.nonzero(idx % 3 == k)[0]
                if len(rows):
                    sel = torch.from_numpy(rows).to(eng.dev)
                    coords = pts[keep[sel] // 3].reshape(-1, 1, 2).contiguous()
                    masks[sel] = eng.predict_prompts(coords, ones[:len(rows)], None, None, H, W, multimask=True, mask_index=k)[0]
        boxes, areas = eng.mask_boxes(masks)
        kept = table[keep]
        return {"masks": masks, "boxes": boxes, "scores": kept[:, 0].contiguous().view(torch.float32), "stability": kept[:, 1].contiguous().view(torch.float32),
                "points": pts[keep // 3], "areas": areas, "index": keep}

    def _records(self, out, segmentations, cleaned: bool = False):
        """cleaned: area and bbox come from the outputs (the cleaned masks' own), not from the candidate table."""
        H, W = self.predictor.original_size
        f, pts = self.candidates()
        records = []
        if cleaned:
            areas, boxes = out["areas"].cpu().numpy(), out["boxes"].cpu().numpy().astype(np.int64)
        for i, c in enumerate(out["index"].cpu().numpy().tolist()):
            x0, y0, x1, y1 = (int(v) for v in f["box"][c])
            area = int(f["area"][c])
            if cleaned:
                area = int(areas[i])
                x0, y0, x1, y1 = (int(boxes[i][0]), int(boxes[i][1]), int(boxes[i][2]) - 1, int(boxes[i][3]) - 1) if area else (0, 0, 0, 0)
            records.append({"segmentation": segmentations[i], "area": area, "bbox": [x0, y0, x1 - x0, y1 - y0], "predicted_iou": float(f["iou"][c]),
                            "point_coords": [[float(pts[c // 3][0]), float(pts[c // 3][1])]], "stability_score": float(f["stability"][c]),
                            "crop_box": [0, 0, W, H]})
        return records

    def generate(self, image, image_format: str = "RGB", min_mask_region_area: int = 0):
        """segment_anything's records, one dict per kept mask in NMS keep order: segmentation (bool [H, W], a device tensor), area,
        bbox (XYWH of the inclusive box: w = xmax - xmin), predicted_iou, point_coords [[x, y]], stability_score, crop_box [0, 0, W, H].
        (The constructor's ``output_mode`` takes "binary_mask" only; RLE records come from :meth:`generate_rle`.)
        ``min_mask_region_area`` > 0: the masks of :meth:`postprocess_small_regions`, with ``area`` and ``bbox`` of the cleaned masks."""
        out = self.generate_device(image, image_format, min_mask_region_area)
        return self._records(out, out["masks"].bool(), cleaned=int(min_mask_region_area) > 0)

    def generate_rle(self, image, image_format: str = "RGB", compressed: bool = True, min_mask_region_area: int = 0):
        """The records of :meth:`generate` with ``segmentation`` as the COCO RLE dict ``{"size": [H, W], "counts": str}`` (segment_anything's
        "coco_rle"; ``compressed=False``: ``counts`` the list of run lengths, its "uncompressed_rle"). The masks are encoded on the
        device (``ovmono3d_amd.masks.encode_rle``): no plane is copied to the host. The constructor's ``output_mode`` argument still
        refuses everything but "binary_mask"; this method is the RLE route. ``min_mask_region_area``: as in :meth:`generate`."""
        from ..masks import encode_rle
        out = self.generate_device(image, image_format, min_mask_region_area)
        return self._records(out, encode_rle(out["masks"], compressed=compressed), cleaned=int(min_mask_region_area) > 0)


def build_sam(arch: str, checkpoint: Union[str, Dict[str, torch.Tensor], None], device: Optional[torch.device] = None,
              image_size: Optional[int] = None, precision: int = 3, max_boxes: int = 16) -> SamPredictor:
    """checkpoint: a segment_anything ``.pth`` (or its state dict)."""
    cfg = sam_config(arch, image_size, precision, max_boxes)
    if isinstance(checkpoint, str):
        checkpoint = torch.load(checkpoint, map_location="cpu")
    return SamPredictor(SamEngine(cfg, checkpoint or {}, device))
