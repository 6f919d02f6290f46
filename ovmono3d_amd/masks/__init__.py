"""Masks as outputs: COCO run-length encoding, the label map and the mask picture, all computed on the HIP device
(``ovm_mask_rle_encode`` / ``ovm_mask_rle_decode`` / ``ovm_mask_labels`` / ``ovm_render_mask_overlay``; the rules are stated in
include/ovm3d.h). Only the RLE strings cross PCIe; there is no CPU fallback. The one piece of host arithmetic is the string ->
counts conversion of :func:`decode_rle` and :func:`rle_area`, a few bytes per run.

And their topology: :func:`connected_components` (``ovm_mask_cc_label``) and segment_anything's small-region clean-up
:func:`remove_small_regions` (``ovm_mask_remove_small_regions``), also on the device: the planes never leave HBM.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Union

import numpy as np
import torch

from .. import lib as _lib

MAX_CHARS = _lib.OVM_MASK_RLE_MAX_CHARS
_I32_MAX = 2 ** 31 - 1


def _planes(masks, what: str) -> torch.Tensor:
    """A checked uint8 [n, H, W] view with unit column stride (bool is the same bytes; plane and row strides are taken as they are)."""
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise RuntimeError(f"{what} runs on the HIP device only (no CPU fallback): masks must be a device tensor")
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{what}: masks must be uint8 or bool [n, H, W] (8-bit planes only)")
    m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    n, H, W = m.shape
    if n and (m.stride(2) != 1 or m.stride(1) < W or m.stride(0) < 0):
        m = m.contiguous()
    return m


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def string_to_counts(s: Union[str, bytes]) -> List[int]:
    """pycocotools' rleFrString: per count groups of 5 bits, low group first, each one ASCII character - 48, 0x20 = another group
    follows, sign-extended when the last group has 0x10 set; from the fourth count on the value is a difference to the count two
    places back. A string that ends inside a count, holds a character outside '0'..'o' or gives a negative count raises ValueError."""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts: List[int] = []
    p = 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError("RLE string ends inside a count")
            g = data[p] - 48
            if not 0 <= g < 64:
                raise ValueError(f"RLE string holds byte {data[p]} outside '0'..'o'")
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and g & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        if x < 0:
            raise ValueError("RLE string gives a negative count")
        counts.append(x)
    return counts


def _record_counts(record: Dict) -> List[int]:
    c = record["counts"]
    return string_to_counts(c) if isinstance(c, (str, bytes)) else [int(v) for v in c]


def rle_area(record: Dict) -> int:
    """Pixels inside the mask of one RLE record (host): the sum of the odd-numbered counts."""
    return int(sum(_record_counts(record)[1::2]))


def _encode_call(m: torch.Tensor, max_runs: int, compressed: bool):
    """One ovm_mask_rle_encode call: (status list, counts tensor, run offsets, string tensor or None, string offsets or None)."""
    L = _lib.load()
    n, H, W = (int(v) for v in m.shape)
    dev = m.device
    max_bytes = MAX_CHARS * max_runs if compressed else 0
    ws_bytes = C.c_int64()
    _lib.check(L.ovm_mask_rle_encode_workspace(n, H, W, max_runs, max_bytes, C.byref(ws_bytes)), what="ovm_mask_rle_encode_workspace")
    with torch.cuda.device(dev):
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=dev)
        run_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        counts = string = str_off = None
        if compressed:
            string = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
            str_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        else:
            counts = torch.empty(max_runs, dtype=torch.int32, device=dev)
        rc = L.ovm_mask_rle_encode(m.data_ptr(), m.stride(0), m.stride(1), n, H, W, counts.data_ptr() if counts is not None else None, max_runs,
                                   run_off.data_ptr(), string.data_ptr() if compressed else None, max_bytes,
                                   str_off.data_ptr() if compressed else None, status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
        _lib.check(rc, what="ovm_mask_rle_encode")
        return status.cpu().tolist(), counts, run_off, string, str_off           # the one 16-byte read


def _encode_chunk(m: torch.Tensor, compressed: bool, max_runs=None) -> List[Dict]:
    n, H, W = (int(v) for v in m.shape)
    worst = n * (H * W + 1)
    if max_runs is None:
        max_runs = min(worst, max(4096, n * H * W // 64))
    st, counts, run_off, string, str_off = _encode_call(m, int(max_runs), compressed)
    if st[0] == _lib.OVM_ERR_CAPACITY:
        # once more with the stated need (a saturated total is read from the 64-bit offsets); that call fits, there is no loop
        need = int(run_off[n].item()) if st[1] == _I32_MAX else st[1]
        st, counts, run_off, string, str_off = _encode_call(m, need, compressed)
    if st[0] != _lib.OVM_OK:
        raise _lib.OvmError(f"ovm_mask_rle_encode: status {st}")
    if compressed:
        off = str_off.cpu().tolist()
        data = string[: off[n]].cpu().numpy().tobytes()
        return [{"size": [H, W], "counts": data[off[i]:off[i + 1]].decode("ascii")} for i in range(n)]
    off = run_off.cpu().tolist()
    vals = counts[: off[n]].cpu().numpy().view(np.uint32).tolist()
    return [{"size": [H, W], "counts": vals[off[i]:off[i + 1]]} for i in range(n)]


def encode_rle(masks: torch.Tensor, compressed: bool = True, max_runs=None) -> List[Dict]:
    """Device uint8 / bool [n, H, W] (nonzero = inside; any plane and row strides) -> one COCO RLE record per plane:
    ``{"size": [H, W], "counts": str}``, or the uncompressed ``counts: list[int]`` with ``compressed=False``. Encoded on the device;
    what is read back is the 16-byte status, the n + 1 offsets and exactly the strings' bytes. ``max_runs`` sizes the first call's
    buffers (default H * W / 64 runs per plane); when the planes hold more, the call is made once more with the count the device
    stated. Planes are taken in chunks that keep a call's worst-case totals within 32 bits."""
    m = _planes(masks, "encode_rle")
    n, H, W = (int(v) for v in m.shape)
    if n == 0:
        return []
    if H < 1 or W < 1 or H * W > _I32_MAX:
        raise ValueError(f"encode_rle: a plane of {H} x {W} (1 <= H * W <= 2^31 - 1: counts are uint32, as in COCO)")
    per_call = max(1, (_I32_MAX // MAX_CHARS) // (H * W + 1))
    out: List[Dict] = []
    for i in range(0, n, per_call):
        out += _encode_chunk(m[i:i + per_call], bool(compressed), max_runs)
    return out


def decode_rle(records: Sequence[Dict], device) -> torch.Tensor:
    """RLE records of one size (``counts`` a string or a list) -> device uint8 [n, H, W] of 0 / 1. The strings are turned into counts
    on the host (a few bytes per run); the counts are uploaded and the planes are filled on the device. Counts that do not sum to
    H * W raise ValueError (the device reports the plane)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_rle runs on the HIP device only (no CPU fallback)")
    records = list(records)
    if not records:
        raise ValueError("decode_rle: no records (the plane size comes from them)")
    H, W = (int(v) for v in records[0]["size"])
    if any([int(v) for v in r["size"]] != [H, W] for r in records):
        raise ValueError("decode_rle: the records must share one size")
    if H < 1 or W < 1 or H * W > _I32_MAX:
        raise ValueError(f"decode_rle: size {H} x {W}")
    per = [_record_counts(r) for r in records]
    n = len(per)
    flat = np.fromiter((c for p in per for c in p), dtype=np.int64)
    if flat.size == 0 or flat.min() < 0 or flat.max() > 0xffffffff:
        raise ValueError("decode_rle: counts must be a non-empty list of uint32 values")
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in per], out=offsets[1:])
    total = int(offsets[n])
    L = _lib.load()
    ws_bytes = C.c_int64()
    _lib.check(L.ovm_mask_rle_decode_workspace(n, H, W, total, C.byref(ws_bytes)), what="ovm_mask_rle_decode_workspace")
    with torch.cuda.device(device):
        d_counts = torch.from_numpy(flat.astype(np.uint32).view(np.int32)).to(device)
        d_off = torch.from_numpy(offsets).to(device)
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=device)
        out = torch.empty((n, H, W), dtype=torch.uint8, device=device)
        status = torch.empty(4, dtype=torch.int32, device=device)
        rc = L.ovm_mask_rle_decode(d_counts.data_ptr(), d_off.data_ptr(), total, n, H, W, out.data_ptr(), out.stride(0), out.stride(1),
                                   status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(device))
        _lib.check(rc, what="ovm_mask_rle_decode")
        st = status.cpu().tolist()
    if st[0] != _lib.OVM_OK:
        raise ValueError(f"decode_rle: the counts of {st[1]} record(s) do not sum to H * W = {H * W} (first: record {st[2]})")
    return out


def mask_labels(masks: torch.Tensor) -> torch.Tensor:
    """uint8 / bool [n, H, W] device planes -> int32 [H, W]: the lowest plane index covering the pixel, -1 where none does. What
    ``vis.labels_from_masks`` computes, in one kernel and without its n x H x W int32 temporary."""
    m = _planes(masks, "mask_labels")
    n, H, W = (int(v) for v in m.shape)
    with torch.cuda.device(m.device):
        labels = torch.empty((H, W), dtype=torch.int32, device=m.device)
        rc = _lib.load().ovm_mask_labels(m.data_ptr() if n else None, m.stride(0) if n else 0, m.stride(1) if n else 0, n, H, W,
                                         labels.data_ptr(), labels.stride(0), _stream(m.device))
        _lib.check(rc, what="ovm_mask_labels")
    return labels


def overlay_masks(im: torch.Tensor, masks_or_labels: torch.Tensor, colors, alpha: float = 0.5) -> torch.Tensor:
    """The picture of the masks: ``im`` (device uint8 [H, W, 3]) with instance b's pixels blended towards ``colors[b]`` (0..255 per
    component, in the image's channel order) at ``alpha`` and its contour drawn in the full colour. ``masks_or_labels``: the planes
    [n, H, W] (the lowest covering plane wins) or an int32 [H, W] label map. Returns a new device tensor; integer arithmetic, defined
    to the byte (include/ovm3d.h, ovm_render_mask_overlay)."""
    if not torch.is_tensor(im) or not im.is_cuda or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
        raise ValueError("overlay_masks: im must be a device uint8 [H, W, 3] tensor")
    dev = im.device
    H, W = int(im.shape[0]), int(im.shape[1])
    labels = masks_or_labels if masks_or_labels.dim() == 2 else mask_labels(masks_or_labels)
    if labels.dtype != torch.int32 or tuple(labels.shape) != (H, W) or labels.device != dev:
        raise ValueError(f"overlay_masks: labels must be int32 [{H}, {W}] on {dev}")
    if labels.stride(1) != 1 or labels.stride(0) < W:
        labels = labels.contiguous()
    if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * W:
        im = im.contiguous()
    col = torch.as_tensor(np.asarray(colors, dtype=np.uint8).reshape(-1, 3)).to(dev)
    a = int(round(float(alpha) * 255))
    with torch.cuda.device(dev):
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        rc = _lib.load().ovm_render_mask_overlay(im.data_ptr(), im.stride(0), labels.data_ptr(), labels.stride(0),
                                                 col.data_ptr() if col.numel() else None, int(col.shape[0]), a, out.data_ptr(), out.stride(0),
                                                 H, W, _stream(dev))
        _lib.check(rc, what="ovm_render_mask_overlay")
    return out


# ---- connected components and the small-region clean-up (include/ovm3d.h, "Mask connected components") ---------------------------
MAX_CC_WORKSPACE = 1 << 30           # bytes of workspace one call may take: the planes are walked in chunks that stay below it
_CC_MODES = {"holes": 1, "islands": 2, "both": 3}


def _cc_chunks(n: int, H: int, W: int, workspace_fn):
    """(planes per call, workspace bytes of such a call): the largest chunk whose workspace stays within MAX_CC_WORKSPACE and which
    one call takes (one plane when even that is above the constant). The workspace grows with n by at most need(2) - need(1) per plane
    (the offsets are rounded up to 16 bytes), which gives the start; the call's own limit on n is found by halving."""
    def need(k):
        b = C.c_int64()
        return b.value if workspace_fn(k, H, W, C.byref(b)) == _lib.OVM_OK else None

    one = need(1)
    if one is None:
        raise ValueError(f"a plane of {H} x {W} is more than one call takes")
    per = 1
    if n > 1 and need(2) is not None:
        per = max(1, min(n, 1 + (MAX_CC_WORKSPACE - one) // max(need(2) - one, 1)))
    while per > 1:
        got = need(per)
        if got is not None and got <= MAX_CC_WORKSPACE:
            return per, got
        # more segments than a launch takes: halve; over the constant (the 16-byte rounding): scale down, one fewer at the least
        per = per // 2 if got is None else min(per - 1, per * MAX_CC_WORKSPACE // got)
    return 1, one


def _cc_status(status: torch.Tensor, what: str) -> None:
    st = status.cpu().tolist()                                # the one 16-byte read
    if st[0] != _lib.OVM_OK:
        raise _lib.OvmError(f"{what}: status {st} ({st[1]} thread(s) reached the bound of a union-find walk)")


def connected_components(masks: torch.Tensor, connectivity: int = 8, invert: bool = False):
    """Device uint8 / bool [n, H, W] (nonzero = foreground, zero with ``invert``; any plane and row strides) -> (labels int32
    [n, H, W], counts int32 [n]), device tensors. The components of each plane are numbered 1, 2, ... in row-major order of their
    first pixel, background 0: ``scipy.ndimage.label`` with the cross (``connectivity=4``) or ``ones((3, 3))`` (8). Labelled on
    the device (``ovm_mask_cc_label``: union-find, a fixed number of launches); what is read back is the 16-byte status."""
    m = _planes(masks, "connected_components")
    if connectivity not in (4, 8):
        raise ValueError(f"connected_components: connectivity must be 4 or 8, is {connectivity}")
    n, H, W = (int(v) for v in m.shape)
    dev = m.device
    with torch.cuda.device(dev):
        labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:
            return labels, counts
        if H < 1 or W < 1 or H * W > _I32_MAX:
            raise ValueError(f"connected_components: a plane of {H} x {W} (1 <= H * W <= 2^31 - 1)")
        L = _lib.load()
        per, ws_bytes = _cc_chunks(n, H, W, L.ovm_mask_cc_label_workspace)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        for i in range(0, n, per):
            c, lab = m[i:i + per], labels[i:i + per]
            rc = L.ovm_mask_cc_label(c.data_ptr(), c.stride(0), c.stride(1), int(c.shape[0]), H, W, int(connectivity), int(bool(invert)),
                                     lab.data_ptr(), lab.stride(0), lab.stride(1), counts[i:i + per].data_ptr(), status.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _stream(dev))
            _lib.check(rc, what="ovm_mask_cc_label")
            _cc_status(status, "ovm_mask_cc_label")
    return labels, counts


def remove_small_regions(masks: torch.Tensor, area_thresh: int, mode: str):
    """segment_anything's ``remove_small_regions`` on device planes: uint8 / bool [n, H, W] -> (masks uint8 [n, H, W] of 0 / 1,
    changed bool [n]), device tensors. ``mode``: "holes" fills the regions of the complement (8-connected, the outer background
    included) whose area is below ``area_thresh``; "islands" clears such regions of the mask, keeping the largest (the first of equal
    ones) when all are that small; "both" is holes, then islands on the result, as the automatic mask generator applies them.
    ``changed`` is whether the plane had a small region. ``remove_small_regions(m, H * W + 1, "islands")`` is "keep the largest
    component". Runs on the device (``ovm_mask_remove_small_regions``); what is read back is the 16-byte status."""
    m = _planes(masks, "remove_small_regions")
    if mode not in _CC_MODES:
        raise ValueError(f"remove_small_regions: mode must be one of {sorted(_CC_MODES)}, is {mode!r}")
    if int(area_thresh) < 1:
        raise ValueError(f"remove_small_regions: area_thresh must be at least 1, is {area_thresh}")
    n, H, W = (int(v) for v in m.shape)
    dev = m.device
    with torch.cuda.device(dev):
        out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        changed = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:
            return out, changed.bool()
        if H < 1 or W < 1 or H * W > _I32_MAX:
            raise ValueError(f"remove_small_regions: a plane of {H} x {W} (1 <= H * W <= 2^31 - 1)")
        L = _lib.load()
        per, ws_bytes = _cc_chunks(n, H, W, L.ovm_mask_remove_small_regions_workspace)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        for i in range(0, n, per):
            c, o = m[i:i + per], out[i:i + per]
            rc = L.ovm_mask_remove_small_regions(c.data_ptr(), c.stride(0), c.stride(1), int(c.shape[0]), H, W, int(area_thresh), _CC_MODES[mode],
                                                 o.data_ptr(), o.stride(0), o.stride(1), changed[i:i + per].data_ptr(), status.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _stream(dev))
            _lib.check(rc, what="ovm_mask_remove_small_regions")
            _cc_status(status, "ovm_mask_remove_small_regions")
    return out, changed.bool()
