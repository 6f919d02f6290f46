"""CPU: the rules of the device mask run-length coder, without a device.

Counts: the numpy restatement (tests/mask_rle_oracle.py) equals transformers' ``_mask_to_rle`` (the SAM image processor's helper, the
one live pin) on seeded planes and on the edge planes the GPU tests use.
String: parity with pycocotools is UNPINNED - the package is not installed. It is held by the round trip
from_string(to_string(c)) == c over seeded count lists that include differences of both signs and the 5-bit group boundaries, by one
hand-worked string, and by the package's own host decoder agreeing with the oracle's.
Also: the library's refusals before any device work, the two command lines' new flags, and the package staying free of transformers."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_rle_oracle as mo
from common import ROOT
from ovmono3d_amd import lib
from ovmono3d_amd import masks as M


def _hf_counts(plane):
    # image_processing_sam needs torchvision to import; image_processing_pil_sam holds the same function and needs none
    try:
        f = importlib.import_module("transformers.models.sam.image_processing_sam")._mask_to_rle
    except ImportError:
        f = importlib.import_module("transformers.models.sam.image_processing_pil_sam")._mask_to_rle
    return f(torch.from_numpy(np.asarray(plane) != 0)[None])[0]


@pytest.mark.parametrize("H,W", [(1, 1)] + mo.SHAPES)
def test_counts_equal_the_sam_image_processors(H, W):
    planes = mo.edge_planes(H, W)
    planes.update({f"seed{s}": mo.blobs(H, W, seed=s) for s in (1, 2, 3)})
    for name, p in planes.items():
        ref = _hf_counts(p)
        assert ref["size"] == [H, W]
        got = mo.counts(p)
        assert got == [int(v) for v in ref["counts"]], name
        assert sum(got) == H * W and np.array_equal(mo.decode(got, H, W), (p != 0).astype(np.uint8)), name
    assert mo.counts(planes["zeros"]) == [H * W] and mo.counts(planes["ones"]) == [0, H * W]
    assert mo.counts(planes["first"])[0] == 0 and len(mo.counts(planes["checker"])) == H * W + 1


BOUNDARY = [15, 16, 511, 512, 2 ** 20, 2 ** 20 - 1, 2 ** 31 - 1]


def _count_lists():
    rng = np.random.RandomState(5)
    out = [[0, 1], [7], [2 ** 31 - 1], [0, 2 ** 31 - 1]]
    # differences d = c[i] - c[i-2] of both signs at the group boundaries: 15 / 16, -16 / -17, 511 / 512, -512 / -513, 2^20
    for d in (15, 16, -16, -17, 511, 512, -512, -513, 2 ** 20, -(2 ** 20), 2 ** 20 - 1, -(2 ** 20) - 1, 2 ** 31 - 2, -(2 ** 31 - 2)):
        base = max(1, 1 - d)
        out.append([3, 1, 4, base, 9, base + d, 2])
    for _ in range(40):
        k = int(rng.randint(1, 60))
        scale = int(rng.choice([4, 40, 600, 20000, 3000000]))
        out.append([int(v) for v in rng.randint(0, scale, size=k)])
    out.append(BOUNDARY + BOUNDARY[::-1])
    return out


def test_string_round_trip_and_group_boundaries():
    for c in _count_lists():
        s = mo.to_string(c)
        assert mo.from_string(s) == c, c
        assert all(48 <= ord(ch) < 48 + 64 for ch in s)
        assert len(s) <= lib.OVM_MASK_RLE_MAX_CHARS * len(c)
        # the package's host decoder is a second, separately written statement of the inverse
        assert M.string_to_counts(s) == c
    # one group holds -16 .. 15, two hold -512 .. 511, and 2^31 - 1 needs the stated maximum
    assert [len(mo.to_string([v])) for v in (15, 16, 511, 512, 2 ** 20, 2 ** 31 - 1)] == [1, 2, 2, 3, 5, 7]
    assert [len(mo.to_string([9, 9, 9, 9 + d])) - 3 for d in (-16, -17, -512, -513)] == [1, 2, 2, 3]
    assert len(mo.to_string([0, 2 ** 31 - 1, 0, 0])) == 1 + 7 + 1 + lib.OVM_MASK_RLE_MAX_CHARS            # the last: -(2^31 - 1)


def test_hand_worked_string():
    """counts [5, 2, 37, 1, 3], worked by hand from the rule (c = x & 31; x >>= 5; more = x != -1 if c & 16 else x != 0; c |= 32 if more;
    emit chr(c + 48)):
      i=0  x = 5              c = 5,  x -> 0,  bit 16 clear, x == 0: stop           chr(53)  '5'
      i=1  x = 2              c = 2,  x -> 0:  stop                                 chr(50)  '2'
      i=2  x = 37 (i > 2 not yet)  c = 5, x -> 1, bit 16 clear, x != 0: more, c = 37    chr(85)  'U'
                              c = 1,  x -> 0:  stop                                 chr(49)  '1'
      i=3  x = 1 - cnts[1] = -1   c = 31, x -> -1, bit 16 set, x == -1: stop           chr(79)  'O'
      i=4  x = 3 - cnts[2] = -34  c = -34 & 31 = 30, x -> -2, bit 16 set, x != -1: more, c = 62   chr(110) 'n'
                              c = -2 & 31 = 30, x -> -1, bit 16 set, x == -1: stop  chr(78)  'N'
    """
    assert mo.to_string([5, 2, 37, 1, 3]) == "52U1OnN"
    assert mo.from_string("52U1OnN") == [5, 2, 37, 1, 3]
    assert M.string_to_counts("52U1OnN") == [5, 2, 37, 1, 3]
    assert M.rle_area({"size": [6, 8], "counts": "52U1OnN"}) == 3 and M.rle_area({"size": [6, 8], "counts": [5, 2, 37, 1, 3]}) == 3


def test_host_string_decoder_refuses_malformed_strings():
    for bad in ("U", "5\x7f", "5 "):                                   # ends inside a count; bytes outside '0'..'o'
        with pytest.raises(ValueError):
            M.string_to_counts(bad)
    with pytest.raises(ValueError):
        M.string_to_counts("O")                                          # a negative first count
    with pytest.raises(RuntimeError, match="HIP device only"):
        M.encode_rle(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device only"):
        M.decode_rle([{"size": [4, 4], "counts": [16]}], "cpu")


def test_library_refusals_without_a_device():
    L = lib.load()
    INV, CAP = lib.OVM_ERR_INVALID, lib.OVM_ERR_CAPACITY
    n = C.c_int64(-7)
    assert L.ovm_mask_rle_encode_workspace(1, 1080, 1920, 4096, 7 * 4096, C.byref(n)) == 0 and n.value >= 4096 * 16
    for bad in ((0, 4, 4, 16, 16), (1, 0, 4, 16, 16), (1, 4, 0, 16, 16), (1, 65536, 32768, 16, 16), (1, 4, 4, 0, 16), (1, 4, 4, 16, -1)):
        n.value = -7
        assert L.ovm_mask_rle_encode_workspace(*bad, C.byref(n)) == INV and n.value == -7, bad
    assert L.ovm_mask_rle_encode_workspace(1, 4, 4, 16, 16, None) == INV
    assert L.ovm_mask_rle_encode_workspace(1, 46340, 46340, 16, 16, C.byref(n)) == 0                     # H * W just below 2^31
    assert L.ovm_mask_rle_encode_workspace(2 ** 24, 4, 4, 16, 16, C.byref(n)) == CAP                      # more workgroups than a launch takes
    buf = (C.c_uint8 * 4096)(*([0xA5] * 4096))
    p = C.addressof(buf)
    p += -p % 16                                                          # the library wants a 16-byte aligned workspace
    ok = dict(masks=p, ps=16, pitch=4, n=1, H=4, W=4, counts=p, max_runs=8, ro=p, string=p, max_bytes=56, so=p, status=p, ws=p, ws_bytes=2048)

    def encode(**kw):
        a = dict(ok, **kw)
        return L.ovm_mask_rle_encode(a["masks"], a["ps"], a["pitch"], a["n"], a["H"], a["W"], a["counts"], a["max_runs"], a["ro"], a["string"],
                                     a["max_bytes"], a["so"], a["status"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(masks=None), dict(ro=None), dict(status=None), dict(ws=None), dict(n=0), dict(H=0), dict(W=0), dict(H=65536, W=32768, pitch=32768),
               dict(pitch=3), dict(max_runs=0), dict(max_bytes=0), dict(so=None), dict(ws=p + 4)):
        assert encode(**kw) == INV, kw
    assert encode(ws_bytes=64) == CAP
    dn = C.c_int64(-7)
    assert L.ovm_mask_rle_decode_workspace(1, 4, 4, 3, C.byref(dn)) == 0 and dn.value >= 32
    assert L.ovm_mask_rle_decode_workspace(1, 4, 4, 0, C.byref(dn)) == INV and L.ovm_mask_rle_decode_workspace(1, 4, 4, 3, None) == INV

    def decode(counts=p, ro=p, total=3, n=1, H=4, W=4, out=p, ps=16, pitch=4, status=p, ws=p, ws_bytes=2048):
        return L.ovm_mask_rle_decode(counts, ro, total, n, H, W, out, ps, pitch, status, ws, ws_bytes, None)
    for kw in (dict(counts=None), dict(ro=None), dict(out=None), dict(status=None), dict(ws=None), dict(total=0), dict(n=0), dict(H=0), dict(W=-1),
               dict(pitch=3), dict(H=65536, W=32768, pitch=32768), dict(counts=p + 4), dict(ws=p + 8)):
        assert decode(**kw) == INV, kw
    assert decode(ws_bytes=16) == CAP
    # the label map and the mask picture
    assert L.ovm_mask_labels(None, 16, 4, 1, 4, 4, p, 4, None) == INV and L.ovm_mask_labels(p, 16, 4, 1, 4, 4, None, 4, None) == INV
    for geo in ((-1, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 0, 4, 4), (1, 4, 4, 3, 4), (1, 4, 4, 4, 3)):
        nn, H, W, pitch, lp = geo
        assert L.ovm_mask_labels(p, 16, pitch, nn, H, W, p, lp, None) == INV, geo
    assert L.ovm_mask_labels(p, 16, 4, 1, 4 * 65535 + 1, 4, p, 4, None) == CAP

    def overlay(image=p, ip=12, labels=p, lp=4, colors=p, n=1, alpha=128, out=p, op=12, H=4, W=4):
        return L.ovm_render_mask_overlay(image, ip, labels, lp, colors, n, alpha, out, op, H, W, None)
    for kw in (dict(image=None), dict(labels=None), dict(out=None), dict(colors=None), dict(n=-1), dict(alpha=-1), dict(alpha=256), dict(ip=11), dict(op=11),
               dict(lp=3), dict(H=0), dict(W=0)):
        assert overlay(**kw) == INV, kw
    assert bytes(buf) == b"\xA5" * 4096                                  # nothing was written


def test_command_lines_know_the_new_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--segmentation" in r.stdout and "--show-masks" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ovmono3d_geo.py"), "--mask-format", "x"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--mask-format" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--segmentation", "polygon"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--segmentation" in r.stderr


def test_the_package_stays_free_of_transformers():
    code = ("import sys; import ovmono3d_amd.masks, ovmono3d_amd.sam, ovmono3d_amd.geo, ovmono3d_amd.vis; "
            "assert 'transformers' not in sys.modules and 'pycocotools' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
