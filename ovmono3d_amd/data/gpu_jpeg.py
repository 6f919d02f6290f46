"""JPEG decode with the data-parallel part on the device ("next" row 2 of SURVEY.md 8f).

The reference reads images with ``cv2.imread`` (demo/demo.py:52) and detectron2's ``read_image`` = Pillow
(cubercnn/data/dataset_mapper.py:38) - libjpeg-turbo at its defaults either way. Here the host only undoes the entropy coding
(``ovm_host_jpeg_entropy_decode``: Huffman streams are serial) into pinned coefficient planes; dequantisation, the inverse DCT,
chroma upsampling and the colour transform run in libovm3d on the device (``ovm_jpeg_reconstruct``), bit-identical to Pillow's
``Image.open(f).convert("RGB")``, and the image is born in HBM where the resize kernel and the patch gather read it.

Baseline and progressive files are covered; streams outside the scope (arithmetic-coded, CMYK, 4:4:0, an incomplete progression ...) raise :class:`UnsupportedJpeg`;
:func:`read_image_device` then hands that file, like a PNG, to the host reader and uploads the pixels.

The other direction has no serial step: :func:`encode_jpeg` produces the whole baseline file on the device (``ovm_jpeg_encode``,
csrc/jpeg_enc.hip), byte for byte the one Pillow's ``Image.save(quality=q)`` writes, and :func:`write_jpeg` is what the demo and the
evaluation samples save their pictures with (the reference: demo/demo.py:117-121, cubercnn/vis/vis.py:274)."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np
import torch

from .. import lib as _lib

OVM_ERR_UNSUPPORTED = -6


class UnsupportedJpeg(ValueError):
    """A valid JPEG the device decoder does not cover (see include/ovm3d.h)."""


def jpeg_info(data: bytes) -> "_lib.OvmJpegInfo":
    """Header walk on the host: size, sampling layout, quantisation tables."""
    L = _lib.load()
    info = _lib.OvmJpegInfo()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = L.ovm_host_jpeg_info(C.addressof(buf), len(data), C.byref(info))
    if rc == OVM_ERR_UNSUPPORTED:
        raise UnsupportedJpeg("JPEG outside the device decoder's scope (arithmetic / 12-bit / CMYK / unusual sampling)")
    _lib.check(rc, what="ovm_host_jpeg_info")
    return info


def entropy_decode(data: bytes, pin: bool = False) -> Tuple[torch.Tensor, "_lib.OvmJpegInfo"]:
    """Huffman-decodes every scan on the host: (coefficients int16 [coef_blocks, 64] in natural order, header record)."""
    L = _lib.load()
    info = jpeg_info(data)
    coef = torch.empty((int(info.coef_blocks), 64), dtype=torch.int16, pin_memory=pin)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = L.ovm_host_jpeg_entropy_decode(C.addressof(buf), len(data), coef.data_ptr(), coef.numel(), C.byref(info))
    if rc == OVM_ERR_UNSUPPORTED:
        raise UnsupportedJpeg("JPEG outside the device decoder's scope")
    _lib.check(rc, what="ovm_host_jpeg_entropy_decode")
    return coef, info


def decode_jpeg(data: bytes, device: torch.device) -> torch.Tensor:
    """JPEG bytes -> uint8 RGB [H, W, 3] on the HIP device, bit-identical to Pillow's decode."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_jpeg reconstructs on the HIP device only (no CPU fallback)")
    L = _lib.load()
    coef, info = entropy_decode(data, pin=True)
    with torch.cuda.device(device):
        d_coef = coef.to(device, non_blocking=True)
        planes = torch.empty(int(info.coef_blocks) * 64, dtype=torch.uint8, device=device)
        rgb = torch.empty((int(info.height), int(info.width), 3), dtype=torch.uint8, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        rc = L.ovm_jpeg_reconstruct(d_coef.data_ptr(), C.byref(info), planes.data_ptr(), rgb.data_ptr(), stream)
        _lib.check(rc, what="ovm_jpeg_reconstruct")
        d_coef.record_stream(torch.cuda.current_stream(device))
    return rgb


_SUBSAMPLING = {"4:2:0": 2, "4:4:4": 0, 2: 2, 0: 0}


def _encode_plan(img: torch.Tensor, quality: int, subsampling, channel_order: str, with_header: bool):
    """Argument checks shared by the encode calls: (plan record, header buffer or None, address of the R sample of pixel (0, 0),
    channel stride). BGR is the same memory read with a negative channel stride, not a flipped copy."""
    if not torch.is_tensor(img) or not img.is_cuda:
        raise RuntimeError("the JPEG encoder runs on the HIP device only (no CPU fallback; write_jpeg(use_device=False) is the host path)")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("encode_jpeg: image must be uint8 [H, W, 3]")
    if channel_order not in ("RGB", "BGR"):
        raise ValueError(f"encode_jpeg: channel_order {channel_order!r} (RGB or BGR)")
    if subsampling not in _SUBSAMPLING:
        raise UnsupportedJpeg(f"encode_jpeg: subsampling {subsampling!r} (the device encoder writes 4:2:0 and 4:4:4)")
    L = _lib.load()
    info = _lib.OvmJpegEncInfo()
    header = (C.c_uint8 * 640)() if with_header else None
    rc = L.ovm_host_jpeg_encode_plan(int(img.shape[1]), int(img.shape[0]), int(quality), _SUBSAMPLING[subsampling], C.byref(info),
                                     header, 640 if with_header else 0)
    _lib.check(rc, what="ovm_host_jpeg_encode_plan")
    sc = int(img.stride(2))
    base = img.data_ptr()
    if channel_order == "BGR":
        base, sc = base + 2 * sc, -sc
    return info, header, base, sc


def jpeg_forward(img: torch.Tensor, quality: int = 95, subsampling="4:2:0", channel_order: str = "RGB") -> torch.Tensor:
    """The encoder's first half alone (``ovm_jpeg_forward``): quantised coefficients, device int16 [coef_blocks, 64] in the layout
    :func:`entropy_decode` returns for the file Pillow writes of the same picture."""
    info, _, base, sc = _encode_plan(img, quality, subsampling, channel_order, False)
    L = _lib.load()
    with torch.cuda.device(img.device):
        ws = torch.empty(int(info.coef_blocks) * 64, dtype=torch.uint8, device=img.device)
        coef = torch.empty((int(info.coef_blocks), 64), dtype=torch.int16, device=img.device)
        stream = C.c_void_p(torch.cuda.current_stream(img.device).cuda_stream)
        rc = L.ovm_jpeg_forward(base, img.stride(0), img.stride(1), sc, C.byref(info), ws.data_ptr(), ws.numel(), coef.data_ptr(), stream)
        _lib.check(rc, what="ovm_jpeg_forward")
    return coef


def encode_jpeg(img: torch.Tensor, quality: int = 95, subsampling="4:2:0", channel_order: str = "RGB") -> bytes:
    """Device uint8 [H, W, 3] (any strides) -> the bytes of the baseline JPEG Pillow's ``Image.save(f, "JPEG", quality=quality)``
    writes of the same picture (``subsampling="4:4:4"``: of ``subsampling=0``), encoded entirely on the device
    (``ovm_jpeg_encode``). Two device-to-host reads: the length, then exactly that many bytes."""
    info, header, base, sc = _encode_plan(img, quality, subsampling, channel_order, True)
    L = _lib.load()
    ws_bytes, cap = C.c_int64(), C.c_int64()
    _lib.check(L.ovm_jpeg_encode_workspace(C.byref(info), C.byref(ws_bytes), C.byref(cap)), what="ovm_jpeg_encode_workspace")
    with torch.cuda.device(img.device):
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=img.device)
        out = torch.empty(int(cap.value), dtype=torch.uint8, device=img.device)
        out_len = torch.empty(1, dtype=torch.int64, device=img.device)
        stream = C.c_void_p(torch.cuda.current_stream(img.device).cuda_stream)
        rc = L.ovm_jpeg_encode(base, img.stride(0), img.stride(1), sc, C.byref(info), header, ws.data_ptr(), ws.numel(), out.data_ptr(),
                               out.numel(), out_len.data_ptr(), stream)
        _lib.check(rc, what="ovm_jpeg_encode")
        n = int(out_len.item())
        return out[:n].cpu().numpy().tobytes()


def write_jpeg(path: str, img, quality: int = 95, channel_order: str = "RGB", use_device: bool = True) -> None:
    """Writes ``img`` (uint8 [H, W, 3], tensor or array, in ``channel_order``) as the JPEG ``Image.fromarray(rgb).save(path,
    quality=quality)`` writes. A tensor on the HIP device is encoded there when ``use_device`` is true; otherwise the picture is
    copied to the host and saved with Pillow, as the reference does (demo/demo.py:117-121, cubercnn/vis/vis.py:274). The file is
    the same either way."""
    if use_device and torch.is_tensor(img) and img.is_cuda:
        data = encode_jpeg(img, quality=quality, channel_order=channel_order)
        with open(path, "wb") as f:
            f.write(data)
        return
    if channel_order not in ("RGB", "BGR"):
        raise ValueError(f"write_jpeg: channel_order {channel_order!r} (RGB or BGR)")
    from PIL import Image
    arr = img.cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    rgb = arr[:, :, ::-1] if channel_order == "BGR" else arr
    Image.fromarray(np.ascontiguousarray(rgb)).save(path, format="JPEG", quality=quality)


def read_image_device(path: str, fmt: str, device: torch.device) -> torch.Tensor:
    """uint8 [H, W, 3] on the device in RGB or BGR channel order (``fmt``; BGR = cv2.imread's order, demo/demo.py:52). Baseline JPEGs are
    reconstructed on the device; other formats (PNG, CMYK JPEG ...) are read by the host reader and uploaded."""
    with open(path, "rb") as f:
        data = f.read()
    img = None
    if data[:2] == b"\xff\xd8":
        try:
            img = decode_jpeg(data, device)
        except UnsupportedJpeg:
            img = None
    if img is None:
        from .feeding import read_image
        img = torch.from_numpy(np.array(read_image(path, "RGB"))).to(device)
    return img.flip(-1) if fmt == "BGR" else img
