"""numpy restatement of the baseline JPEG encoder Pillow runs for ``Image.save(f, "JPEG", quality=q)`` (libjpeg-turbo at its
defaults: JDCT_ISLOW, standard Huffman tables, one interleaved scan), and the case list the encoder tests share.

Every rule is restated from the published algorithms (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jccoefct.c, jchuff.c, jcparam.c,
jcmarker.c); the oracle is Pillow itself, live: tests/test_jpeg_encode_cpu.py compares this file's bytes and coefficient planes with
Pillow's on every case, tests/test_gpu_jpeg_encode.py compares the device encoder (ovmono3d_amd/csrc/jpeg_enc.hip) with Pillow's.
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
COCO = os.path.join(HERE, "golden", "coco_000000101762.jpg")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

# Annex K.1 quantisation tables, natural order
QT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                    80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                    95, 98, 112, 100, 103, 99])
QT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                      99, 99] + [99] * 32)

# Annex K.3 Huffman tables: number of codes of each length 1..16, then the symbols in code order
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def _codes(bits, vals):
    """Canonical Huffman codes (Annex C): (code[256], length[256]) by symbol."""
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


DC_CODES = [_codes(DC_LUMA_BITS, DC_VALS), _codes(DC_CHROMA_BITS, DC_VALS)]
AC_CODES = [_codes(AC_LUMA_BITS, AC_LUMA_VALS), _codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]


def quant_tables(quality):
    """jpeg_set_quality with force_baseline: (luma, chroma) in natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (QT_LUMA, QT_CHROMA)]


def header(width, height, quality, subsampling):
    """The bytes in front of the entropy-coded data, as Pillow writes them: SOI, APP0 (JFIF 1.01, density 1 x 1), one DQT per table,
    SOF0, DHT x 4, SOS."""
    hs = {0: 1, 2: 2}[subsampling]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(quant_tables(quality)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in t[ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03"
    out += bytes([1, hs * 16 + hs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                              (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def _fix(x):
    return int(x * 65536 + 0.5)


def color_planes(rgb, hs):
    """jccolor.c rgb_ycc_convert, the edge rules and jcsample.c h2v2_downsample: the three padded planes (whole MCUs) as int64."""
    H, W = rgb.shape[:2]
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.168735892) * r - _fix(.331264108) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.418687589) * g - _fix(.081312411) * b + (128 << 16) + 32767) >> 16
    mx, my = -(-W // (8 * hs)), -(-H // (8 * hs))

    def pad(p, w, h):                                            # columns to the right, then the last row downwards
        p = np.concatenate([p, np.repeat(p[:, -1:], w - p.shape[1], 1)], 1) if w > p.shape[1] else p
        return np.concatenate([p, np.repeat(p[-1:], h - p.shape[0], 0)], 0) if h > p.shape[0] else p

    if hs == 1:
        return [pad(p, mx * 8, my * 8) for p in (y, cb, cr)]
    out = [pad(y, mx * 16, my * 16)]
    for p in (cb, cr):
        p = pad(p, mx * 16, H + (H & 1))                         # rows only to the row group: the rest is replicated AFTER downsampling
        bias = np.tile(np.array([1, 2]), mx * 4)[None, :]
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(pad(d, mx * 8, my * 8))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of jpeg_fdct_islow over the last axis (8 values); first: the row pass."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(plane, q):
    """[bh * 8, bw * 8] samples -> [bh, bw, 64] quantised coefficients in natural order (jfdctint.c, jcdctmgr.c)."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    c = _fdct_1d(blk, True)                                      # rows
    c = _fdct_1d(c.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    c = c.reshape(bh, bw, 64)
    d = 8 * q[None, None, :]
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(rgb, quality, subsampling):
    """Quantised coefficient planes, component after component, with the dummy-block rule of jccoefct.c: list of [bh, bw, 64]."""
    H, W = rgb.shape[:2]
    hs = {0: 1, 2: 2}[subsampling]
    qt = quant_tables(quality)
    planes = color_planes(rgb, hs)
    out = [fdct_quant(planes[0], qt[0]), fdct_quant(planes[1], qt[1]), fdct_quant(planes[2], qt[1])]
    if hs == 2:                                                  # only the luma plane of 4:2:0 can hold dummy blocks
        y = out[0]
        nbx, nby = -(-W // 8), -(-H // 8)
        if nbx < y.shape[1]:                                     # right of a real row: the DC of the block before
            y[:nby, nbx, 1:] = 0
            y[:nby, nbx, 0] = y[:nby, nbx - 1, 0]
        if nby < y.shape[0]:                                     # a dummy row: the DC of the MCU's last block of the row above
            y[nby, :, 1:] = 0
            y[nby, 0::2, 0] = y[nby - 1, 1::2, 0]
            y[nby, 1::2, 0] = y[nby - 1, 1::2, 0]
    return out


def scan_order(planes, hs):
    """Blocks in the order of the interleaved scan: ([n, 64] coefficients, component of each block)."""
    my, mx = planes[1].shape[:2]
    if hs == 2:
        y = planes[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
    else:
        y = planes[0].reshape(my, mx, 1, 64)
    mcu = np.concatenate([y, planes[1][:, :, None], planes[2][:, :, None]], 2)
    comp = np.tile(np.array([0] * (hs * hs) + [1, 2]), my * mx)
    return mcu.reshape(-1, 64), comp


def _nbits(v):
    v = np.abs(v)
    n = np.zeros(v.shape, np.int64)
    for k in range(12):
        n += v >= (1 << k)
    return n


def entropy_code(blocks, comp, stats=None):
    """jchuff.c encode_one_block over the scan, byte stuffing and the final padding: the entropy-coded bytes. Every coefficient
    becomes one token (its ZRL codes, its (run, size) code and its value bits), position 64 is the EOB."""
    n = blocks.shape[0]
    z = blocks[:, ZIGZAG].astype(np.int64)
    tab = (comp > 0).astype(np.int64)
    val = np.zeros((n, 65), np.uint64)
    length = np.zeros((n, 65), np.int64)
    # DC: difference to the previous block of the same component
    diff = z[:, 0].copy()
    for c in range(3):
        i = np.flatnonzero(comp == c)
        diff[i] = np.diff(z[i, 0], prepend=0)
    cat = _nbits(diff)
    low = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    dcode = np.where(tab == 0, DC_CODES[0][0][cat], DC_CODES[1][0][cat])
    dsize = np.where(tab == 0, DC_CODES[0][1][cat], DC_CODES[1][1][cat])
    val[:, 0] = ((dcode << cat) | low).astype(np.uint64)
    length[:, 0] = dsize + cat
    # AC: run = zeros since the previous non-zero coefficient
    nz = z != 0
    nz[:, 0] = True
    pos = np.where(nz, np.arange(64)[None, :], 0)
    prev = np.maximum.accumulate(pos, 1)
    prev = np.concatenate([np.zeros((n, 1), np.int64), prev[:, :-1]], 1)
    run = np.arange(64)[None, :] - prev - 1
    size = _nbits(z)
    bi, ki = np.nonzero(nz[:, 1:])
    ki = ki + 1
    r, s, v, t = run[bi, ki], size[bi, ki], z[bi, ki], tab[bi]
    sym = ((r & 15) << 4) | s
    code = np.where(t == 0, AC_CODES[0][0][sym], AC_CODES[1][0][sym])
    csz = np.where(t == 0, AC_CODES[0][1][sym], AC_CODES[1][1][sym])
    zrl = np.where(t == 0, AC_CODES[0][0][0xf0], AC_CODES[1][0][0xf0])
    zsz = np.where(t == 0, AC_CODES[0][1][0xf0], AC_CODES[1][1][0xf0])
    acc = np.zeros(len(bi), np.int64)
    alen = np.zeros(len(bi), np.int64)
    for k in range(3):
        m = (r >> 4) > k
        acc = np.where(m, (acc << zsz) | zrl, acc)
        alen = alen + np.where(m, zsz, 0)
    acc = (((acc << csz) | code) << s) | (np.where(v < 0, v - 1, v) & ((1 << s) - 1))
    val[bi, ki] = acc.astype(np.uint64)
    length[bi, ki] = alen + csz + s
    last = np.where(nz, np.arange(64)[None, :], 0).max(1)
    eob = last < 63
    val[:, 64] = np.where(eob, np.where(tab == 0, AC_CODES[0][0][0], AC_CODES[1][0][0]), 0).astype(np.uint64)
    length[:, 64] = np.where(eob, np.where(tab == 0, AC_CODES[0][1][0], AC_CODES[1][1][0]), 0)
    if stats is not None:
        stats["zrl"] = int((r >> 4).sum())
        stats["max_dc_cat"] = int(cat.max())
        stats["max_ac_size"] = int(s.max()) if len(s) else 0
        stats["eob"] = int(eob.sum())
    # tokens -> bits
    val, length = val.reshape(-1), length.reshape(-1)
    keep = length > 0
    val, length = val[keep], length[keep]
    total = int(length.sum())
    start = np.cumsum(length) - length
    tok = np.repeat(np.arange(len(length)), length)
    shift = (length[tok] - 1 - (np.arange(total) - start[tok])).astype(np.uint64)
    bits = ((val[tok] >> shift) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    data = np.packbits(bits)
    ff = np.flatnonzero(data == 0xff)
    if stats is not None:
        stats["stuffed"] = int(len(ff))
    return np.insert(data, ff + 1, 0).tobytes()


def encode(rgb, quality=75, subsampling=2, stats=None):
    """The whole file."""
    H, W = rgb.shape[:2]
    planes = coefficients(rgb, quality, subsampling)
    blocks, comp = scan_order(planes, {0: 1, 2: 2}[subsampling])
    return header(W, H, quality, subsampling) + entropy_code(blocks, comp, stats) + b"\xff\xd9"


def coefficient_planes(rgb, quality, subsampling):
    """[coef_blocks, 64] int16 in the decoder's layout (what ``entropy_decode`` returns)."""
    return np.concatenate([p.reshape(-1, 64) for p in coefficients(rgb, quality, subsampling)]).astype(np.int16)


def pillow_bytes(rgb, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, **({"subsampling": 0} if subsampling == 0 else {}))
    return b.getvalue()


# ------------------------------------------------------------------------------------------------
# shared cases
# ------------------------------------------------------------------------------------------------
def picture(kind, h, w, seed=0):
    g = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    if kind == "noise":
        # uniform noise; a seeded third of the 4 x 4 tiles each is pushed to black and to white. Plain uniform noise has block means
        # within a few levels of 127 and no coefficient near 512, so it cannot meet the conditions asked of this picture at quality
        # 100 (a DC category >= 10, an AC size of 10); the tiles give half-block steps and block-to-block jumps of the full range.
        img = g.integers(0, 256, (h, w, 3)).astype(np.int64)
        step = g.integers(-1, 2, ((h + 3) // 4, (w + 3) // 4)) * 255
        img += np.kron(step, np.ones((4, 4), np.int64))[:h, :w, None]
        return np.clip(img, 0, 255).astype(np.uint8)
    if kind == "coco":
        with Image.open(COCO) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:h, :w])
    if kind == "constant":
        return np.broadcast_to(np.array([37, 150, 201], np.uint8), (h, w, 3)).copy()
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "impulse":                                        # a horizontal ramp, isolated +-255 impulses on every 11th row and column
        ramp = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.int64)
        img = np.broadcast_to(ramp[None, :, None], (h, w, 3)).copy()
        yy, xx = np.mgrid[0:h, 0:w]
        m = (yy % 11 == 0) & (xx % 11 == 0)
        img[m] += np.where((yy // 11 + xx // 11) % 2 == 0, 255, -255)[m][:, None]
        return np.clip(img, 0, 255).astype(np.uint8)
    if kind == "primaries":                                      # saturated colours in 5 x 7 patches
        pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]],
                       np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        return pal[(yy // 5 * 3 + xx // 7) % 8]
    raise ValueError(kind)


# (kind, height, width, quality, subsampling): every size, picture, quality and both samplings appear; not their full product
CASES = [
    ("noise", 1, 1, 95, 2), ("noise", 1, 1, 75, 0), ("noise", 8, 8, 75, 2), ("noise", 16, 16, 30, 2), ("noise", 16, 16, 100, 0),
    ("noise", 17, 9, 95, 2), ("noise", 17, 9, 100, 0), ("noise", 37, 53, 30, 2), ("noise", 37, 53, 100, 2), ("noise", 37, 53, 95, 0),
    ("noise", 250, 333, 95, 2), ("noise", 250, 333, 75, 0), ("noise", 64, 64, 100, 2), ("noise", 64, 64, 75, 2),
    ("noise", 600, 800, 100, 2), ("noise", 600, 800, 95, 0),
    ("coco", 480, 640, 95, 2), ("coco", 480, 640, 75, 0), ("coco", 250, 333, 30, 2),
    ("constant", 37, 53, 95, 2), ("constant", 64, 64, 75, 0), ("constant", 250, 333, 30, 2),
    ("white", 17, 9, 95, 2), ("white", 64, 64, 100, 0), ("white", 250, 333, 75, 2),
    ("impulse", 37, 53, 95, 2), ("impulse", 250, 333, 75, 2), ("impulse", 64, 64, 30, 0), ("impulse", 480, 640, 100, 2),
    ("primaries", 37, 53, 100, 2), ("primaries", 250, 333, 95, 0), ("primaries", 64, 64, 75, 2), ("primaries", 17, 9, 30, 2),
]
CASE_IDS = ["%s_%dx%d_q%d_%s" % (k, h, w, q, "420" if s == 2 else "444") for k, h, w, q, s in CASES]

_cache = {}


def case(kind, h, w, quality, subsampling):
    """(picture, Pillow's file) of one case, computed once per process."""
    key = (kind, h, w, quality, subsampling)
    if key not in _cache:
        rgb = picture(kind, h, w)
        rgb.setflags(write=False)
        _cache[key] = (rgb, pillow_bytes(rgb, quality, subsampling))
    return _cache[key]
