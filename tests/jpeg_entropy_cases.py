"""Files for the device entropy route (tests/test_jpeg_entropy_cpu.py on the CPU emulation, tests/test_gpu_jpeg_entropy.py on
the kernels). Each file is made once per session and never changed; the host decoder's planes of each are computed once too.
What a case is there to break is asserted on the file itself by test_jpeg_entropy_cpu.py::test_cases_have_their_conditions."""
import ctypes as C
import functools
import io

import numpy as np
from PIL import Image

from test_jpeg import CASES, COCO, _case_bytes, _jpeg, _scene

from ovmono3d_amd import lib as _lib
from ovmono3d_amd.data import gpu_jpeg


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def plan_of(data, max_rounds=0):
    """(return code, plan record) of ovm_host_jpeg_decode_plan."""
    L = _lib.load()
    plan = _lib.OvmJpegDecPlan()
    tables = np.empty(11008, dtype=np.uint8)
    rc = L.ovm_host_jpeg_decode_plan(data, len(data), max_rounds, C.byref(plan), tables.ctypes.data, tables.size)
    return rc, plan


def ac_code_lengths(data, th):
    """symbol -> code length of AC table th, read from the file's DHT segments."""
    i = data.find(b"\xff\xc4")
    while i >= 0:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        seg, o = data[i + 4:i + 2 + n], 0
        while o + 17 <= len(seg):
            counts = list(seg[o + 1:o + 17])
            vals = seg[o + 17:o + 17 + sum(counts)]
            if seg[o] == 0x10 + th:
                lens = [l + 1 for l, c in enumerate(counts) for _ in range(c)]
                return dict(zip(vals, lens))
            o += 17 + sum(counts)
        i = data.find(b"\xff\xc4", i + 2 + n)
    raise AssertionError("no such table")


def ac_symbols(block):
    """The (run << 4 | size) symbols of one block's AC coefficients (natural order in, ZRL and EOB included)."""
    zz = [int(block[i]) for i in ZIGZAG]
    out, run = [], 0
    for v in zz[1:]:
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(0xF0)
            run -= 16
        out.append((run << 4) | abs(v).bit_length())
        run = 0
    if run:
        out.append(0)
    return out


def unstuffed_len(data, plan):
    ecs = data[plan.ecs_offset:plan.ecs_offset + plan.ecs_bytes]
    markers = sum(ecs.count(bytes([0xFF, 0xD0 + i])) for i in range(8))
    return len(ecs) - ecs.count(b"\xff\x00") - 2 * markers


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _primaries(h, w):
    """8-pixel stripes of black / white / red / green / blue / black ...: neighbouring blocks differ by the full range."""
    cols = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]], dtype=np.uint8)
    img = np.zeros((h, w, 3), dtype=np.uint8)
    for x in range(w):
        img[:, x] = cols[(x // 8) % len(cols)]
    return img


@functools.lru_cache(maxsize=None)
def _boundary_files():
    """Seeded search over size and quality: the first file whose unstuffed stream is one byte short of a multiple of the
    subsequence size, and the first that is one byte over."""
    found = {}
    g = np.random.default_rng(2024)
    for _ in range(4000):
        h, w, q = int(g.integers(17, 64)), int(g.integers(17, 64)), int(g.integers(40, 96))
        data = _jpeg(_scene(h, w, h + w), quality=q, subsampling=2)
        rc, plan = plan_of(data)
        assert rc == 0
        sub_bytes = plan.sub_bits // 8
        n = unstuffed_len(data, plan)
        if n > 2 * sub_bytes:
            if n % sub_bytes == sub_bytes - 1:
                found.setdefault("one_byte_under_multiple", data)
            elif n % sub_bytes == 1:
                found.setdefault("one_byte_over_multiple", data)
        if len(found) == 2:
            break
    assert len(found) == 2, "the seeded search found no such files"
    return found


@functools.lru_cache(maxsize=None)
def well_formed():
    """name -> bytes: every file the device route must accept (status 0)."""
    out = {}
    for name, hw, kw in CASES:
        if not kw.get("progressive"):
            out[name] = _case_bytes(name, hw, kw)
    out["grey"] = _jpeg(_scene(77, 53, 3)[:, :, 0], quality=80)
    out["coco"] = open(COCO, "rb").read()
    out["scene_300x400_q95"] = _jpeg(_scene(300, 400, 5), quality=95, subsampling=2)
    out["noise_q100"] = _jpeg(_noise(48, 64, 1), quality=100, subsampling=2)
    out["primaries_444_q100"] = _jpeg(_primaries(32, 96), quality=100, subsampling=0)
    out["rgb_no_transform"] = _rgb_file()
    with Image.open(COCO) as im:                    # all components on one table pair, longer than the launches could walk step by step
        b = io.BytesIO()
        im.convert("RGB").save(b, format="JPEG", quality=90, keep_rgb=True)
    out["coco_rgb_one_table_pair"] = b.getvalue()
    out["444_restart_every_mcu"] = _jpeg(_scene(40, 90, 8), quality=50, subsampling=0, restart_marker_blocks=1)
    out.update(_boundary_files())
    return out


def _rgb_file():
    b = io.BytesIO()
    Image.fromarray(_scene(37, 41, 6)).save(b, format="JPEG", quality=85, keep_rgb=True)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def host_planes(name):
    """The judge: ovm_host_jpeg_entropy_decode's planes of a well-formed file (torch int16 [coef_blocks, 64]) and its header."""
    return gpu_jpeg.entropy_decode(well_formed()[name])


@functools.lru_cache(maxsize=None)
def emulated(name):
    """(planes, info, status, rounds) of the CPU emulation at the default round cap."""
    return gpu_jpeg.entropy_decode_emulated(well_formed()[name])


@functools.lru_cache(maxsize=None)
def emulated_launches(name):
    """Synchronisation launches in which the emulation decoded anything (at the default round cap)."""
    return gpu_jpeg.entropy_decode_emulated(well_formed()[name], with_launches=True)[4]


@functools.lru_cache(maxsize=None)
def small_files():
    """The two files whose damaged versions are tried: 4:2:0 without and 4:4:4 with restart markers."""
    return {"baseline_420": _jpeg(_scene(40, 56, 2), quality=80, subsampling=2),
            "restart_444": _jpeg(_scene(33, 47, 3), quality=70, subsampling=0, restart_marker_blocks=2)}


def fixed_mutations(data):
    """The 32 damaged versions of a file that also go to the device: the arithmetic of scratch/fuzz_jpeg_dec.cpp --list."""
    rc, plan = plan_of(data)
    assert rc == 0
    out = []
    for m in range(32):
        d = bytearray(data)
        pos = plan.ecs_offset + ((m * 7919 + 13) * 31) % plan.ecs_bytes
        if m % 4 == 3:
            d[pos] = 0xFF
        else:
            d[pos] ^= 1 << (m & 7)
        out.append(bytes(d))
    return out


def judge_damaged(data, got):
    """The contract on damaged data. got: None when the route declined (plan or status), else its planes. An accepted decode
    equals the host decoder's, which must then have accepted the file. Returns whether the route accepted."""
    import torch
    if got is None:
        return False
    want, _ = gpu_jpeg.entropy_decode(data)          # raises if the host refuses: an accepted file the host refuses is a failure
    assert torch.equal(got.cpu(), want), "accepted, but differs from the host decoder"
    return True
