"""JPEG decode on the device ("next" row 2 of SURVEY.md 8f).

The reference reads images with ``cv2.imread`` (demo/demo.py:52) and detectron2's ``read_image`` = Pillow
(cubercnn/data/dataset_mapper.py:38) - libjpeg-turbo at its defaults either way. Here dequantisation, the inverse DCT, chroma
upsampling and the colour transform run in libovm3d on the device (``ovm_jpeg_reconstruct``), bit-identical to Pillow's
``Image.open(f).convert("RGB")``, and the image is born in HBM where the resize kernel and the patch gather read it. The entropy
stage in front of them has two routes:

- ``entropy="host"`` (the default): ``ovm_host_jpeg_entropy_decode`` Huffman-decodes every scan on the host into pinned
  coefficient planes, which are uploaded (3 B per pixel);
- ``entropy="device"`` (``MODEL.AMD.GPU_JPEG_ENTROPY``): only the file's bytes are uploaded and ``ovm_jpeg_entropy_decode`` produces
  the same planes, bit for bit, with self-synchronising parallel Huffman decoding (csrc/jpeg_dec.hip). It covers 8-bit
  baseline / extended-sequential files with one scan of all components (grey, 4:4:4, 4:2:2, 4:2:0; standard or optimised tables;
  with or without restart markers). The device accepts only what it can prove: progressive files, per-component scans and whatever
  the plan finds odd are not sent at all, and a stream on which any check fails (marker sequence, block counts per restart
  segment, consumed bits, DC range, convergence within the round cap) comes back with a non-zero status. Either way the host
  decoder then runs on the same bytes and accepts or raises as it always did - the device never decides that a file is invalid.

Baseline and progressive files are covered; streams outside the scope (arithmetic-coded, CMYK, 4:4:0, an incomplete progression ...) raise :class:`UnsupportedJpeg`;
:func:`read_image_device` then hands that file, like a PNG, to the host reader and uploads the pixels.

The other direction needs no such synchronisation: :func:`encode_jpeg` produces the whole baseline file on the device (``ovm_jpeg_encode``,
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


class EntropyDeclined(UnsupportedJpeg):
    """The plan of the device entropy route does not take this file: outside its scope (progressive, per-component scans, data
    behind the scan ...) or refused by the header walk, whatever the code - the plan judges no file, so a corrupt header is
    reported here as well and not as an error. The host route decides about the file (and raises on a corrupt one)."""


def _decode_plan(data: bytes, max_rounds):
    L = _lib.load()
    plan = _lib.OvmJpegDecPlan()
    tables = np.empty(_DEC_TABLE_BYTES, dtype=np.uint8)
    rc = L.ovm_host_jpeg_decode_plan(data, len(data), int(max_rounds or 0), C.byref(plan), tables.ctypes.data, tables.size)
    if rc != 0:
        raise EntropyDeclined(f"ovm_host_jpeg_decode_plan declined the file (code {rc})")
    return plan, tables


_DEC_TABLE_BYTES = 11008


def entropy_decode_emulated(data: bytes, max_rounds=None, with_launches: bool = False):
    """The device entropy route run serially on the CPU (``ovm_host_jpeg_entropy_emulate``: the same stages, round schedule and
    core routine as the kernels): (coefficients, header record, status, rounds), with ``with_launches`` also the number of
    synchronisation launches in which anything was decoded (at most 5 of the 6 may be for a file to be accepted). Raises :class:`EntropyDeclined` when the plan
    does not cover the file."""
    L = _lib.load()
    plan, _ = _decode_plan(data, max_rounds)
    info = _lib.OvmJpegInfo()
    coef = torch.empty((int(plan.info.coef_blocks), 64), dtype=torch.int16)
    status, rounds, launches = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = L.ovm_host_jpeg_entropy_emulate(data, len(data), int(max_rounds or 0), coef.data_ptr(), coef.numel(), C.byref(info),
                                         C.byref(status), C.byref(rounds), C.byref(launches))
    _lib.check(rc, what="ovm_host_jpeg_entropy_emulate")
    if with_launches:
        return coef, info, int(status.value), int(rounds.value), int(launches.value)
    return coef, info, int(status.value), int(rounds.value)


def _entropy_enqueue(data: bytes, device: torch.device, max_rounds=None, stream_offset: int = 0):
    """Plan, upload and the stream-ordered call of the device entropy route, without the read back:
    (coefficients, plan, result words on the device)."""
    L = _lib.load()
    plan, tables = _decode_plan(data, max_rounds)
    n, nb = int(plan.ecs_bytes), int(plan.info.coef_blocks)
    ws_bytes = C.c_int64()
    _lib.check(L.ovm_jpeg_entropy_decode_workspace(C.byref(plan), C.byref(ws_bytes)), what="ovm_jpeg_entropy_decode_workspace")
    pad = int(stream_offset)                                            # the table block is a multiple of 16 bytes
    host = torch.empty(_DEC_TABLE_BYTES + pad + n, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[:_DEC_TABLE_BYTES] = tables
    hv[_DEC_TABLE_BYTES + pad:] = np.frombuffer(data, dtype=np.uint8, count=n, offset=int(plan.ecs_offset))
    with torch.cuda.device(device):
        blob = host.to(device, non_blocking=True)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=device)
        coef = torch.empty((nb, 64), dtype=torch.int16, device=device)
        result = torch.empty(3, dtype=torch.int32, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        rc = L.ovm_jpeg_entropy_decode(blob.data_ptr() + _DEC_TABLE_BYTES + pad, blob.data_ptr(), C.byref(plan), ws.data_ptr(), ws.numel(),
                                       coef.data_ptr(), coef.numel(), result.data_ptr(), stream)
        _lib.check(rc, what="ovm_jpeg_entropy_decode")
    return coef, plan, result


def entropy_decode_device(data: bytes, device: torch.device, max_rounds=None, stream_offset: int = 0):
    """Huffman-decodes the file's one scan on the device (``ovm_jpeg_entropy_decode``): only the entropy-coded bytes and 11 KB of
    tables are uploaded. Returns (coefficients device int16 [coef_blocks, 64], header record, status, rounds). ``status`` 0: the
    coefficients are proven equal to :func:`entropy_decode`'s; non-zero (``OVM_JPEG_DEC_*`` bits of include/ovm3d.h): the device
    declined and the coefficients are undefined - the caller asks the host decoder. Raises :class:`EntropyDeclined` when the plan
    does not cover the file. ``stream_offset`` places the bytes at that offset of their device buffer (any alignment works)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("entropy_decode_device runs on the HIP device only (entropy_decode is the host route)")
    coef, plan, result = _entropy_enqueue(data, device, max_rounds, stream_offset)
    status, rounds, _launches = result.tolist()                         # the one read back: the route is decided here
    return coef, plan.info, int(status), int(rounds)


def decode_jpeg(data: bytes, device: torch.device, entropy: str = "host", max_rounds=None) -> torch.Tensor:
    """JPEG bytes -> uint8 RGB [H, W, 3] on the HIP device, bit-identical to Pillow's decode. ``entropy="host"`` Huffman-decodes
    on the host and uploads the coefficient planes; ``entropy="device"`` uploads the file's bytes and decodes them there
    (:func:`entropy_decode_device`), and runs the host decoder on the same bytes whenever the device route declines - so what is
    accepted, refused or raised is the host route's in either mode."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_jpeg reconstructs on the HIP device only (no CPU fallback)")
    if entropy not in ("host", "device"):
        raise ValueError(f"decode_jpeg: entropy {entropy!r} (host or device)")
    L = _lib.load()
    d_coef = None
    if entropy == "device":
        try:
            d_coef, info, status, _ = entropy_decode_device(data, device, max_rounds=max_rounds)
            if status != 0:
                d_coef = None
        except EntropyDeclined:
            d_coef = None
    with torch.cuda.device(device):
        if d_coef is None:
            coef, info = entropy_decode(data, pin=True)
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


def read_image_device(path: str, fmt: str, device: torch.device, entropy: str = "host") -> torch.Tensor:
    """uint8 [H, W, 3] on the device in RGB or BGR channel order (``fmt``; BGR = cv2.imread's order, demo/demo.py:52). Baseline JPEGs are
    reconstructed on the device (``entropy``: where their Huffman decode runs, see :func:`decode_jpeg`; the key
    ``MODEL.AMD.GPU_JPEG_ENTROPY``); other formats (PNG, CMYK JPEG ...) are read by the host reader and uploaded."""
    with open(path, "rb") as f:
        data = f.read()
    img = None
    if data[:2] == b"\xff\xd8":
        try:
            img = decode_jpeg(data, device, entropy=entropy)
        except UnsupportedJpeg:
            img = None
    if img is None:
        from .feeding import read_image
        img = torch.from_numpy(np.array(read_image(path, "RGB"))).to(device)
    return img.flip(-1) if fmt == "BGR" else img
