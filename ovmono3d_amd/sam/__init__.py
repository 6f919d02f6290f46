"""Segment Anything with box prompts on the device: the mask source of OVMono3D-GEO (reference tools/ovmono3d_geo.py:213-217,
270-272,308-309 - segment_anything's ``SamPredictor.set_image`` then ``predict(box=...)``, plane ``[2]`` of the multimask outputs).

``build_sam(arch, checkpoint)`` loads a segment_anything checkpoint by its own key names into libovm3d's ``OvmSam`` handle
(csrc/sam.hip): image encoder (the OVM_TOWER_SAM blocks + neck), prompt encoder for boxes, two-way-transformer mask decoder and
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

    def debug(self, name: str, shape) -> torch.Tensor:
        out = torch.empty(shape, dtype=torch.float32, device=self.dev)
        n = self.L.ovm_sam_debug_copy(self._h, name.encode(), out.data_ptr(), out.numel(), self._stream())
        if n < 0:
            self._chk(int(n), f"ovm_sam_debug_copy({name})")
        assert n == out.numel(), (name, n, tuple(shape))
        return out


class SamPredictor:
    """segment_anything's ``SamPredictor`` for box prompts."""

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

    def predict(self, box=None, multimask_output: bool = True):
        """The reference's call shape: one xyxy box -> (masks [3, H, W] bool, iou [3], low_res [3, 4G, 4G]), device tensors."""
        if box is None or not multimask_output:
            raise NotImplementedError("box prompts with multimask_output=True only")
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


def build_sam(arch: str, checkpoint: Union[str, Dict[str, torch.Tensor], None], device: Optional[torch.device] = None,
              image_size: Optional[int] = None, precision: int = 3, max_boxes: int = 16) -> SamPredictor:
    """checkpoint: a segment_anything ``.pth`` (or its state dict). The prompt encoder's mask-input convolutions are loaded by the
    checkpoint reader like every other tensor and not used (box prompts only)."""
    cfg = sam_config(arch, image_size, precision, max_boxes)
    if isinstance(checkpoint, str):
        checkpoint = torch.load(checkpoint, map_location="cpu")
    return SamPredictor(SamEngine(cfg, checkpoint or {}, device))
