"""JPEG encode, the parts that need no GPU: the host plan (header bytes, quantisation tables, geometry), the numpy restatement
tests/jpeg_enc_ref.py and the host path of ``write_jpeg``, all against Pillow (libjpeg-turbo), live and byte for byte."""
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_enc_ref as R
from ovmono3d_amd import lib as _lib
from ovmono3d_amd.data import gpu_jpeg


def _plan(w, h, q, sub, header=True):
    L = _lib.load()
    info = _lib.OvmJpegEncInfo()
    buf = (C.c_uint8 * 640)() if header else None
    rc = L.ovm_host_jpeg_encode_plan(w, h, q, sub, C.byref(info), buf, 640 if header else 0)
    return rc, info, (bytes(buf[:info.header_len]) if header and rc == 0 else None)


@pytest.mark.parametrize("sub", [2, 0], ids=["420", "444"])
def test_plan_header_equals_pillow_at_every_quality(sub):
    """DQT scaling, SOF sampling bytes, the Huffman tables and the segment order: the first header_len bytes of Pillow's file."""
    rgb = R.picture("noise", 19, 301)
    for q in range(1, 101):
        rc, info, hdr = _plan(301, 19, q, sub)
        assert rc == 0 and info.header_len == len(hdr) == 623
        ref = R.pillow_bytes(rgb, q, sub)
        assert ref[:623] == hdr, f"quality {q}"
        assert R.header(301, 19, q, sub) == hdr
        qt = R.quant_tables(q)
        assert [list(info.qt[0]), list(info.qt[1])] == [t.tolist() for t in qt]
    rc, info, hdr = _plan(65535, 1, 50, sub)                     # both size bytes in use
    assert rc == 0 and hdr[20 + 138 + 5:20 + 138 + 9] == b"\x00\x01\xff\xff"


def test_plan_geometry():
    rc, info, _ = _plan(333, 250, 95, 2, header=False)
    assert rc == 0 and (info.hs, info.vs, info.mcus_x, info.mcus_y) == (2, 2, 21, 16)
    assert list(info.bw) == [42, 21, 21] and list(info.bh) == [32, 16, 16] and info.coef_blocks == 42 * 32 + 2 * 21 * 16
    rc, info, _ = _plan(333, 250, 95, 0, header=False)
    assert rc == 0 and (info.hs, info.vs) == (1, 1) and list(info.bw) == [42] * 3 and list(info.bh) == [32] * 3
    L = _lib.load()
    ws, cap = C.c_int64(), C.c_int64()
    assert L.ovm_jpeg_encode_workspace(C.byref(info), C.byref(ws), C.byref(cap)) == 0
    assert cap.value == 623 + 416 * info.coef_blocks + 16 and ws.value > 208 * info.coef_blocks


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_restatement_equals_pillow(case):
    """The file byte for byte, and the coefficient planes against the project's own entropy decoder on Pillow's file."""
    rgb, ref = R.case(*case)
    assert R.encode(rgb, case[3], case[4]) == ref
    coef, info = gpu_jpeg.entropy_decode(ref)
    assert np.array_equal(R.coefficient_planes(rgb, case[3], case[4]), coef.numpy())


def test_case_conditions_hold():
    """What the case list is there to exercise, asserted on the oracle alone: Pillow's bytes and the restatement's symbol counts."""
    def stats(case):
        st = {}
        rgb, ref = R.case(*case)
        assert R.encode(rgb, case[3], case[4], st) == ref
        return st, ref
    noise100 = [c for c in R.CASES if c[0] == "noise" and c[3] == 100]
    assert noise100
    for c in noise100:
        st, ref = stats(c)
        if c[1] * c[2] >= 37 * 53:                                   # a handful of blocks cannot promise every symbol
            assert b"\xff\x00" in ref[623:] and st["stuffed"] >= 1
            assert st["max_dc_cat"] >= 10 and st["max_ac_size"] == 10, (c, st)
    assert any(stats(c)[0]["zrl"] >= 1 for c in R.CASES if c[0] == "impulse")
    for c in R.CASES:                                                # constant colour: EOB only; white: every DC difference but the first 0
        if c[0] in ("constant", "white"):
            st, _ = stats(c)
            assert st["max_ac_size"] == 0 and st["zrl"] == 0
    # 600 x 800 is more than one workgroup of each prefix sum (2048 items) and of the bit packing (64 blocks)
    rc, info, _ = _plan(800, 600, 100, 2, header=False)
    assert info.coef_blocks == 11400 > 2048


def test_abi_mirror_and_refusals():
    L = _lib.load()
    assert L.ovm_abi_sizeof(b"OvmJpegEncInfo") == C.sizeof(_lib.OvmJpegEncInfo) == 4 * 5 + 4 * 6 + 4 * 4 + 2 * 128
    for w, h, q in ((0, 8, 75), (8, 0, 75), (65536, 8, 75), (8, 65536, 75), (8, 8, 0), (8, 8, 101), (-1, 8, 75)):
        assert _plan(w, h, q, 2)[0] == -1, (w, h, q)                 # OVM_ERR_INVALID
    for sub in (1, 3, -1):
        assert _plan(8, 8, 75, sub)[0] == -6                         # OVM_ERR_UNSUPPORTED: 4:2:2 and the rest
    info = _lib.OvmJpegEncInfo()
    small = (C.c_uint8 * 622)()
    assert L.ovm_host_jpeg_encode_plan(8, 8, 75, 2, C.byref(info), small, 622) == -5      # OVM_ERR_CAPACITY
    assert L.ovm_host_jpeg_encode_plan(8, 8, 75, 2, None, None, 0) == -1
    # the device calls check their arguments before anything is launched (no GPU needed to be refused)
    rc, info, hdr = _plan(8, 8, 75, 2)
    ws, cap = C.c_int64(), C.c_int64()
    assert L.ovm_jpeg_encode_workspace(C.byref(info), C.byref(ws), C.byref(cap)) == 0
    hb = (C.c_uint8 * 640).from_buffer_copy(hdr + bytes(17))
    assert L.ovm_jpeg_encode(4096, 24, 3, 1, C.byref(info), hb, 4096, ws.value - 1, 4096, cap.value, 4096, None) == -5
    assert L.ovm_jpeg_encode(4096, 24, 3, 1, C.byref(info), hb, 4096, ws.value, 4096, cap.value - 1, 4096, None) == -5
    assert L.ovm_jpeg_forward(4096, 24, 3, 1, C.byref(info), 4096, info.coef_blocks * 64 - 1, 4096, None) == -5
    bad = _lib.OvmJpegEncInfo.from_buffer_copy(info)
    bad.coef_blocks += 1                                             # a plan that host_plan did not write
    assert L.ovm_jpeg_encode_workspace(C.byref(bad), C.byref(ws), C.byref(cap)) == -1
    assert L.ovm_jpeg_encode(4096, 24, 3, 1, C.byref(bad), hb, 4096, 1 << 30, 4096, 1 << 30, 4096, None) == -1
    with pytest.raises(RuntimeError):
        gpu_jpeg.encode_jpeg(torch.zeros((8, 8, 3), dtype=torch.uint8))                   # no CPU fallback of the encoder


def test_write_jpeg_host_path_writes_pillows_bytes(tmp_path):
    rgb = R.picture("primaries", 37, 53)
    for order, arr in (("RGB", rgb), ("BGR", np.ascontiguousarray(rgb[:, :, ::-1]))):
        for q in (95, 30):
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, format="JPEG", quality=q)
            p1, p2, p3 = (str(tmp_path / f"{order}{q}{i}.jpg") for i in range(3))
            gpu_jpeg.write_jpeg(p1, torch.from_numpy(arr), quality=q, channel_order=order, use_device=False)
            gpu_jpeg.write_jpeg(p2, torch.from_numpy(arr), quality=q, channel_order=order)       # a CPU tensor: the host path
            gpu_jpeg.write_jpeg(p3, arr, quality=q, channel_order=order)
            for p in (p1, p2, p3):
                assert open(p, "rb").read() == b.getvalue()
    with pytest.raises(ValueError):
        gpu_jpeg.write_jpeg(str(tmp_path / "x.jpg"), rgb, channel_order="GBR")
