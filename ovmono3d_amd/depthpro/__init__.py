"""Depth Pro metric depth on the device: the depth source of OVMono3D-GEO (reference tools/ovmono3d_geo.py:267,290-295 -
``depth_pro.create_model_and_transforms`` then ``model.infer(image, f_px=...)``).

``build_depthpro(checkpoint)`` loads a checkpoint in the key names of Hugging Face's ``apple/DepthPro-hf``
(``depth_pro.encoder.*``, ``depth_pro.neck.*``, ``fusion_stage.*``, ``head.*``, ``fov_model.*``) into libovm3d's ``OvmDepthPro``
handle (csrc/depthpro.hip): preprocessing, the three-level crop pyramid, the three DINOv2 towers, the fusion decoder, both heads and
the conversion to metres run there. There is no CPU or PyTorch path, and this package does not import ``transformers``.

Scope: Hugging Face key names only. Apple's own ``depth_pro.pt`` uses other names; a key map for it is not part of this package.
The focal length comes from the caller (``f_px``) or from the field-of-view head; EXIF is not read. One image per call.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Union

import numpy as np
import torch

from .. import lib as _lib

# apple/DepthPro-hf: ViT-L/16 towers at 384, 1536 x 1536 canvas
DEFAULT_CONFIG = dict(embed_dim=1024, depth=24, heads=16, patch=16, crop=384, hook_ids=(11, 5), fusion_dim=256,
                      scaled_dims=(1024, 1024, 512), inter_dims=(256, 256), ratios=(0.25, 0.5, 1.0), overlaps=(0.0, 0.5, 0.25),
                      merge_padding=3, num_fov_layers=2, ln_eps=1e-6)


def depthpro_config(config: Optional[dict] = None, precision: int = 1, use_fov: bool = True) -> "_lib.OvmDepthProConfig":
    d = dict(DEFAULT_CONFIG)
    d.update(config or {})
    c = _lib.OvmDepthProConfig()
    c.embed_dim, c.depth, c.heads, c.patch, c.crop = (int(d[k]) for k in ("embed_dim", "depth", "heads", "patch", "crop"))
    c.fusion_dim, c.merge_padding, c.num_fov_layers = int(d["fusion_dim"]), int(d["merge_padding"]), int(d["num_fov_layers"])
    for name, n in (("hook_ids", 2), ("scaled_dims", 3), ("inter_dims", 2), ("ratios", 3), ("overlaps", 3)):
        v = tuple(d[name])
        if len(v) != n:
            raise ValueError(f"{name} must have {n} entries, has {len(v)}")
        for i in range(n):
            getattr(c, name)[i] = v[i]
    c.use_fov, c.precision, c.ln_eps = int(bool(use_fov)), int(precision), float(d["ln_eps"])
    return c


def check_config(cfg: "_lib.OvmDepthProConfig") -> None:
    """Raises OvmError with the library's message when the pyramid geometry is outside what is built. Host only."""
    buf = C.create_string_buffer(512)
    rc = _lib.load().ovm_host_depthpro_check(C.byref(cfg), buf, len(buf))
    if rc != 0:
        raise _lib.OvmError(f"ovm_depthpro_create would fail with code {rc}: {buf.value.decode()}")


class DepthPro:
    """Owner of one ``OvmDepthPro`` handle."""

    def __init__(self, cfg: "_lib.OvmDepthProConfig", state_dict: Dict[str, torch.Tensor], device: Optional[torch.device] = None):
        self.L = _lib.load()
        self.cfg = cfg
        check_config(cfg)                                          # before any device call
        self.dev = device if device is not None else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        host = {k: np.ascontiguousarray(v.detach().to(torch.float32).cpu().numpy()) for k, v in state_dict.items()
                if torch.is_tensor(v) and v.dtype.is_floating_point and v.dim() <= 4 and not k.endswith("embeddings.mask_token")}
        table, keep = _lib.make_tensor_table(host)
        self._h = C.c_void_p()
        rc = self.L.ovm_depthpro_create(C.byref(cfg), table, len(host), self.dev.index or 0, C.byref(self._h))
        del keep
        if rc != 0:
            msg = (self.L.ovm_depthpro_last_error(self._h) or b"").decode() if self._h else ""
            if self._h:
                self.L.ovm_depthpro_destroy(self._h)
                self._h = None
            raise _lib.OvmError(f"ovm_depthpro_create failed with code {rc}: {msg}")
        self.canvas = 4 * cfg.crop
        self._ws = None
        self._image = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self.L.ovm_depthpro_destroy(h)
            except Exception:
                pass

    def _chk(self, rc, what):
        if rc != 0:
            raise _lib.OvmError(f"{what} failed with code {rc}: {(self.L.ovm_depthpro_last_error(self._h) or b'').decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def workspace_bytes(self, H: int, W: int) -> int:
        n = C.c_int64()
        self._chk(self.L.ovm_depthpro_workspace(self._h, int(H), int(W), C.byref(n)), "ovm_depthpro_workspace")
        return int(n.value)

    def infer(self, image, f_px: Optional[float] = None, image_format: str = "RGB", workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """image: uint8 [H, W, 3], a device tensor (any strides) or a numpy array; a format other than "RGB" reverses the channels.
        f_px: focal length in pixels, or None to estimate it from the field of view. Returns device tensors: "depth" fp32 [H, W] in
        metres, "focallength_px" and "fov_deg" fp32 scalars."""
        if image_format not in ("RGB", "BGR"):
            raise ValueError(f"image_format must be 'RGB' or 'BGR', is {image_format!r}")
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image)).to(self.dev)
        if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError("image must be uint8 [H, W, 3] on the HIP device (or a numpy array to upload)")
        H, W = int(image.shape[0]), int(image.shape[1])
        if workspace is None:
            need = self.workspace_bytes(H, W)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            workspace = self._ws
        self._image, self._last_ws = image, workspace             # kept alive while the stream reads them / for debug()
        d = _lib.OvmImage()
        d.data = image.data_ptr()
        d.height, d.width = H, W
        d.stride_h, d.stride_w, d.stride_c = (int(s) for s in image.stride())
        d.orig_height, d.orig_width = H, W
        depth = torch.empty((H, W), dtype=torch.float32, device=self.dev)
        scal = torch.zeros(2, dtype=torch.float32, device=self.dev)
        self._chk(self.L.ovm_depthpro_infer(self._h, C.byref(d), int(image_format != "RGB"), float(f_px) if f_px else 0.0, depth.data_ptr(),
                                            scal.data_ptr(), scal.data_ptr() + 4, workspace.data_ptr(), workspace.numel(), self._stream()),
                  "ovm_depthpro_infer")
        return {"depth": depth, "focallength_px": scal[1], "fov_deg": scal[0]}

    STAGES = ("pyramid", "towers", "merge_neck", "fusion", "head", "fov", "output")

    def profile(self, on: bool = True) -> None:
        """Record HIP events at the stage boundaries of every following infer."""
        self._chk(self.L.ovm_depthpro_profile_enable(self._h, int(on)), "ovm_depthpro_profile_enable")

    def stage_ms(self) -> Dict[str, float]:
        """Milliseconds per stage of the last infer (waits for it)."""
        ms = (C.c_float * len(self.STAGES))()
        self._chk(self.L.ovm_depthpro_stage_ms(self._h, ms, len(self.STAGES)), "ovm_depthpro_stage_ms")
        return dict(zip(self.STAGES, (float(x) for x in ms)))

    def debug(self, name: str, shape) -> torch.Tensor:
        out = torch.empty(shape, dtype=torch.float32, device=self.dev)
        n = self.L.ovm_depthpro_debug_copy(self._h, name.encode(), out.data_ptr(), out.numel(), self._stream())
        if n < 0:
            self._chk(int(n), f"ovm_depthpro_debug_copy({name})")
        assert n == out.numel(), (name, n, tuple(shape))
        return out


def load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise RuntimeError(f"{path}: reading a .safetensors checkpoint needs the `safetensors` module, which does not import ({e}); "
                               "convert the checkpoint to a torch file or install safetensors") from e
        return load_file(path)
    sd = torch.load(path, map_location="cpu")
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def build_depthpro(checkpoint: Union[str, Dict[str, torch.Tensor]], device: Optional[torch.device] = None, precision: int = 1,
                   use_fov: bool = True, config: Optional[dict] = None) -> DepthPro:
    """checkpoint: a state dict or a file (torch.load; ``.safetensors`` through the safetensors module) in Hugging Face key names.
    precision 1 (fp16 operands, the reference runs Depth Pro in half precision) or 3 (split fp16 x 3, the parity mode)."""
    if isinstance(checkpoint, str):
        checkpoint = load_checkpoint(checkpoint)
    return DepthPro(depthpro_config(config, precision, use_fov), checkpoint, device)
