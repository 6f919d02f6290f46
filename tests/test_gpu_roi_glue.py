"""The kernels between the GEMMs (csrc/roi_cube.hip, csrc/elementwise.hip), each through its own ovm_op_* entry point, against the
fp64 restatement of tests/roi_glue_ref.py (itself checked on the CPU by tests/test_roi_glue_ref_cpu.py).

Tolerance (roi_glue_ref.bound): max |got - fp64| <= 4 * E32 + one fp32 ulp of the largest |fp64| value, E32 = the fp32 run of the
restatement against fp64; per ROI row, per record field and row, per case elsewhere. Never from the kernel's output. Re-layouts and
split outputs are compared bit for bit. Every destination is pre-filled with a sentinel and must keep it outside the kernel's range.
Each test prints E32 and the measured error; the worst of a run on an MI355X stands next to the case lists.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_glue_ref as R
from roi_glue_ref import F32, F64, SENTINEL

pytestmark = pytest.mark.gpu
OVM_ERR_INVALID, OVM_ERR_SHAPE = -1, -4
S16 = int(np.float16(SENTINEL).view(np.uint16))


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _h16(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.float16, device=device)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _check(name, got, ref64, ref32, worst=None):
    """The tolerance rule for one field; returns (E32, error)."""
    e32, tol = R.bound(ref64, ref32)
    err = float(np.max(np.abs(np.asarray(got, F64) - ref64))) if np.size(ref64) else 0.0
    if worst is not None:
        worst[0], worst[1] = max(worst[0], e32), max(worst[1], err)
    assert err <= tol, f"{name}: |got - fp64| = {err:.3e} > 4 * E32 + ulp = {tol:.3e} (E32 {e32:.3e})"
    return e32, err


# ================================================================================================ ROIAlign
def _roi_call(device, feats, hw, scales, C_, out, min_level, max_level, boxes, idx, with_lo, ldo):
    n = len(boxes)
    d_f = [_dev(f, device) for f in feats]
    fp = (C.c_void_p * len(feats))(*[f.data_ptr() for f in d_f])
    hwa = (C.c_int32 * (2 * len(hw)))(*[v for p in hw for v in p])
    sc = (C.c_float * len(scales))(*scales)
    hi = _h16((n + 1, ldo), device)
    lo = _h16((n + 1, ldo), device) if with_lo else None
    d_b, d_i = _dev(boxes, device), _dev(idx, device)
    rc = _lib().ovm_op_roi_align_ex(fp, len(feats), hwa, sc, C_, out, min_level, max_level, d_b.data_ptr(), d_i.data_ptr(), n,
                                    hi.data_ptr(), _ptr(lo), ldo, _stream())
    return rc, _np(hi), (_np(lo) if with_lo else None)


# Levels read back on an MI355X (4 levels | 3 levels): sides 56 112 224 448 896 -> 0 1 2 3 3 | 0 1 2 2 2; 0.1 % under, over 112, 224,
# 448 -> 0 1, 1 2, 2 3 | 0 1, 1 2, 2 2; 56 x 224 -> 1 | 1: as fp32 torch. Largest |value - (level + 1)|: 0 in both.
@pytest.mark.parametrize("max_level", [5, 4])
def test_roi_level_rule(device, max_level):
    """Level l holds the constant l + 1 and contains every box whole, so each bin reads back the level the kernel chose: it must be
    the one fp32 torch chooses (oracle.assign_boxes_to_levels), also for boxes exactly on 112 / 224 / 448 and 0.1 % either side."""
    from oracle.roi_ops import assign_boxes_to_levels
    nl = max_level - 1
    boxes = R.level_boxes()
    want = assign_boxes_to_levels(torch.from_numpy(boxes), 2, max_level).numpy()
    feats = [np.full((1, h, w, 4), l + 1.0, dtype=F32) for l, (h, w) in enumerate(R.LEVEL_HW[:nl])]
    idx = np.zeros(len(boxes), dtype=np.int32)
    rc, hi, lo = _roi_call(device, feats, R.LEVEL_HW[:nl], R.LEVEL_SCALES[:nl], 4, 2, 2, max_level, boxes, idx, True, 16)
    assert rc == 0
    v = R.join(hi[:-1], lo[:-1])
    got = np.rint(v).astype(np.int64) - 1
    dev = float(np.max(np.abs(v - np.rint(v))))
    print(f"\nroi_level_rule max_level={max_level}: levels {got[:, 0].tolist()} want {want.tolist()} max |v - rint(v)| {dev:.3e}")
    assert np.array_equal(got, np.broadcast_to(want[:, None], got.shape)), (got[:, 0].tolist(), want.tolist())
    # weights of one sample sum to 1 within 2 ulp and a bin averages <= 784 samples: far below the 1 / 784 a lost sample would cost
    assert dev <= 2.0 ** -12
    assert np.all(R.bits(hi[-1]) == S16) and np.all(R.bits(lo[-1]) == S16)


# Worst over the 13 ROI rows (E32 / kernel error), MI355X:
#   C   4: out 1 1.8e-07 / 1.8e-07, out 7 2.3e-06 / 2.3e-06       C  64: out 1 2.2e-07 / 2.2e-07, out 7 3.0e-06 / 3.0e-06
#   C 260: out 1 2.7e-07 / 2.7e-07, out 7 3.4e-06 / 3.4e-06       (the worst row is the 64-pixel box: 100 samples per bin)
@pytest.mark.parametrize("out", [1, 7])
@pytest.mark.parametrize("C_", [4, 64, 260])
def test_roi_align_values(device, C_, out):
    """Random features on three levels of different non-square sizes, images interleaved 1, 0, 1, 0, ...; C = 260 takes the lane
    loop's second trip; ldo is wider than the row; lo NULL (one-pass mode) must leave the same hi."""
    boxes, idx = R.value_boxes()
    feats = R.value_feats(C_, seed=C_ + out)
    lv = R.roi_levels(boxes, 2, 4, F64)
    r64 = R.roi_align(feats, R.VAL_SCALES, boxes, idx, lv, out, F64)
    r32 = R.render(R.roi_align(feats, R.VAL_SCALES, boxes, idx, lv, out, F32), F32)
    n, w = len(boxes), out * out * C_
    ldo = w + 8
    rc, hi, lo = _roi_call(device, feats, R.VAL_HW, R.VAL_SCALES, C_, out, 2, 4, boxes, idx, True, ldo)
    assert rc == 0
    for buf in (hi, lo):
        assert np.all(R.bits(buf[:, w:]) == S16) and np.all(R.bits(buf[-1]) == S16), "wrote outside the ROI rows"
        assert not np.any(R.bits(buf[:n, :w]) == S16), "an output element was not written"
    got = R.join(hi[:n, :w], lo[:n, :w])
    worst = [0.0, 0.0]
    for r in range(n):
        e32, err = _check(f"roi row {r}", got[r], r64[r], r32[r], worst)
        print(f"\nroi_align C={C_} out={out} row {r}: E32 {e32:.3e} err {err:.3e}", end="")
    print(f"\nroi_align C={C_} out={out} worst: E32 {worst[0]:.3e} err {worst[1]:.3e}")
    for r in (0, 8, 11):                                          # zero width, wholly outside, x2 < x1: all zeros
        assert not got[r].any()
    rc, hi1, _ = _roi_call(device, feats, R.VAL_HW, R.VAL_SCALES, C_, out, 2, 4, boxes, idx, False, ldo)
    assert rc == 0 and np.array_equal(R.bits(hi1), R.bits(hi)), "hi differs between one-pass and split mode"


def test_roi_align_refuses_c6(device):
    boxes, idx = R.value_boxes()
    feats = [np.zeros((2, h, w, 6), dtype=F32) for h, w in R.VAL_HW]
    rc, hi, lo = _roi_call(device, feats, R.VAL_HW, R.VAL_SCALES, 6, 1, 2, 4, boxes, idx, True, 16)
    assert rc == OVM_ERR_SHAPE and np.all(R.bits(hi) == S16) and np.all(R.bits(lo) == S16)


# ================================================================================================ cube decode
# Worst per field over all rows of n = 129 (E32 / kernel error), MI355X, ldh 16, postprocess 1:
#   box 1.8e-05 / 1.8e-05, score 6.4e-08 / 4.4e-08, bbox3D 2.0e-04 / 2.0e-04, center_cam 4.1e-07 / 4.1e-07, center_2D 3.1e-05 / 2.8e-05,
#   dimensions 3.1e-06 / 3.1e-06, pose 2.2e-04 / 2.2e-04
# Pose rows, E32 / error: on_pp 6.8e-08 / 2.5e-08 (angle == 0: R is the 6D matrix), off_1e-3 2.2e-06 / 2.2e-06, off_0.1 2.2e-04 / 2.2e-04,
# off_1 2.8e-05 / 2.8e-05 (acos of a number next to 1: the reference formula's own fp32 behaviour), a1_zero 8.1e-08 / 8.1e-08,
# a2_parallel_exact 0 / 0, on_pp_far_pose 3.9e-08 / 3.5e-08
@pytest.mark.parametrize("postprocess", [0, 1])
@pytest.mark.parametrize("ldh", [13, 16])
@pytest.mark.parametrize("n", [1, 129])
def test_cube_decode_rows(device, n, ldh, postprocess):
    from ovmono3d_amd.lib import OvmImage
    d = R.decode_inputs(n, ldh)
    metas = d["metas"]
    r64, k64 = R.cube_decode(d["head"], d["boxes"], d["scores"], d["idx"], metas, 512.0, postprocess, F64)
    r32, k32 = R.cube_decode(d["head"], d["boxes"], d["scores"], d["idx"], metas, 512.0, postprocess, F32)
    assert np.array_equal(k64, k32)
    imgs = (OvmImage * 2)()
    for i, m in enumerate(metas):
        imgs[i].height, imgs[i].width, imgs[i].orig_height, imgs[i].orig_width = m["h"], m["w"], m["oh"], m["ow"]
        for j, v in enumerate(m["K"]):
            imgs[i].K[j] = float(v)
    rec = torch.full((n + 1, 48), SENTINEL, device=device)
    keep = torch.full((n + 1,), -7, dtype=torch.int32, device=device)
    t = [_dev(d[k], device) for k in ("head", "boxes", "scores", "classes", "idx")]
    rc = _lib().ovm_op_cube_decode(t[0].data_ptr(), ldh, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), imgs, 2, n,
                                   512.0, postprocess, rec.data_ptr(), keep.data_ptr(), _stream())
    assert rc == 0
    rec, keep = _np(rec), _np(keep)
    assert np.all(rec[n] == SENTINEL) and keep[n] == -7
    assert np.array_equal(keep[:n], k64)
    assert np.array_equal(np.ascontiguousarray(rec[:n, 5]).view(np.int32), d["classes"])
    assert np.array_equal(np.ascontiguousarray(rec[:n, 47]).view(np.int32), d["idx"])
    worst = {name: [0.0, 0.0] for name, _, _ in R.FIELDS}
    assert np.isfinite(rec[:n, :5]).all() and np.isfinite(rec[:n, 6:47]).all()
    for i in range(n):
        for name, a, b in R.FIELDS:
            if d["names"].get(i) == "a2_parallel" and name in ("pose", "bbox3D"):
                continue                     # b2 = normalize(rounding noise): no arithmetic defines it (roi_glue_ref.decode_inputs)
            e32, err = _check(f"decode row {i} ({d['names'].get(i, 'random')}) {name}", rec[i, a:b], r64[i, a:b], r32[i, a:b], worst[name])
            if i in d["names"] and name in ("pose", "bbox3D"):
                print(f"\ncube_decode n={n} ldh={ldh} pp={postprocess} row {i} {d['names'][i]} {name}: E32 {e32:.3e} err {err:.3e}", end="")
    print(f"\ncube_decode n={n} ldh={ldh} pp={postprocess} worst: " + ", ".join(f"{k} {v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()))


# ================================================================================================ record compaction (exact)
@pytest.mark.parametrize("n", R.COMPACT_N)
def test_compact_records(device, n):
    """1023 / 1024 / 1025 / 2500: either side of one chunk of the kernel's loop, and three chunks with a running base."""
    for pattern in R.COMPACT_KEEP:
        rec, keep = R.compact_inputs(n, pattern)
        want, cnt = R.compact_records(rec, keep, 3)
        out = torch.full((n + 2, 48), 0x5A5A5A5A, dtype=torch.int32, device=device)
        counts = torch.full((4,), -9, dtype=torch.int32, device=device)
        d_r, d_k = _dev(rec.view(np.int32), device), _dev(keep, device)
        rc = _lib().ovm_op_compact_records(d_r.data_ptr(), d_k.data_ptr(), n, 3, out.data_ptr(), counts.data_ptr(), _stream())
        assert rc == 0
        out, counts = _np(out).view(np.uint32), _np(counts)
        assert counts[:3].tolist() == cnt.tolist() and counts[3] == -9, (pattern, counts.tolist(), cnt.tolist())
        assert np.array_equal(out[:len(want)], want), f"n={n} {pattern}: kept records differ"
        assert np.all(out[len(want):] == 0x5A5A5A5A), f"n={n} {pattern}: wrote past the kept records"


# ================================================================================================ LayerNorm rows
# Worst fp32-output E32 / kernel error over M in {1, 5, 7}, the bordered M = 30 and the interleaved M = 5, MI355X:
#   D     ordinary              offset (1000 + 0.01 n)   constant
#   4     3.0e-07 / 2.7e-07     1.6e-02 / 3.1e-07        0 / 0
#   252   8.2e-07 / 6.5e-07     1.2e-02 / 5.5e-07        7.1e-04 / 0
#   256   6.7e-07 / 7.7e-07     9.0e-03 / 5.6e-07        1.4e-03 / 0
#   260   9.7e-07 / 7.0e-07     1.2e-02 / 5.2e-07        1.4e-03 / 0
#   1024  6.4e-07 / 7.6e-07     9.1e-03 / 5.6e-07        1.4e-03 / 0
#   1028  7.6e-07 / 1.2e-06     8.5e-03 / 7.0e-07        1.4e-03 / 0
#   1536  7.0e-07 / 1.1e-06     9.6e-03 / 1.1e-06        1.1e-03 / 0
#   2048  9.4e-07 / 1.0e-06     1.1e-02 / 8.7e-07        2.1e-03 / 0
# Before the kernel shifted each row by its first element the offset rows measured 8.2e-03 .. 1.6e-02 and D = 1536, M = 1 missed the
# bound (E32 4.1e-04, error 9.6e-03); constant rows measured up to 1.4e-03.
@pytest.mark.parametrize("D", R.LN_D)
def test_ln_rows(device, D):
    """D = 1028 .. 2048 run ln_rows_kernel<8>. fp32 output vs fp64; every split output must be split(y) of the kernel's own fp32 y,
    bit for bit, at its place: plain rows (ld = D + 8), the interior of a bordered image, the interleaved image."""
    L = _lib()
    ldx, ldf, ld = D + 8, D + 4, D + 8
    worst = {k: [0.0, 0.0] for k in R.LN_ROWS}

    def run(x, g, b, M, variant, tag):
        xb = np.full((M, ldx), 3.25, dtype=F32)
        xb[:, :D] = x
        d_x, d_g, d_b = _dev(xb, device), _dev(g, device), _dev(b, device)
        y = torch.full((M + 1, ldf), SENTINEL, device=device)
        if variant == "plain":
            hi, lo = _h16((M + 1, ld), device), _h16((M + 1, ld), device)
            rc = L.ovm_op_ln_rows(d_x.data_ptr(), ldx, M, D, d_g.data_ptr(), d_b.data_ptr(), 1e-6, y.data_ptr(), ldf, hi.data_ptr(),
                                  lo.data_ptr(), ld, 0, 0, 0, _stream())
            rows, cols, lo_off = np.arange(M), np.arange(D), None
        elif variant == "bordered":
            hi, lo = _h16((2 * 5 * 7 + 1, ld), device), _h16((2 * 5 * 7 + 1, ld), device)
            rc = L.ovm_op_ln_rows(d_x.data_ptr(), ldx, M, D, d_g.data_ptr(), d_b.data_ptr(), 1e-6, y.data_ptr(), ldf, hi.data_ptr(),
                                  lo.data_ptr(), ld, 3, 5, 0, _stream())
            rows, cols, lo_off = R.bordered_rows(2, 3, 5), np.arange(D), None
        else:
            hi = _h16((M + 1, 2 * D), device)
            lo = None
            rc = L.ovm_op_ln_rows(d_x.data_ptr(), ldx, M, D, d_g.data_ptr(), d_b.data_ptr(), 1e-6, y.data_ptr(), ldf, hi.data_ptr(),
                                  hi.data_ptr() + 64, 2 * D, 0, 0, 1, _stream())
            rows, cols, lo_off = np.arange(M), R.il_col(np.arange(D)), 32
        assert rc == 0, tag
        y, hi = _np(y), _np(hi)
        assert np.all(y[:M, D:] == SENTINEL) and np.all(y[M] == SENTINEL), tag
        e32, err = _check(tag, y[:M, :D], R.layer_norm(x, g, b, 1e-6, F64), R.layer_norm(x, g, b, 1e-6, F32), worst[tag.split()[0]])
        print(f"\nln_rows D={D} M={M} {variant} {tag}: E32 {e32:.3e} err {err:.3e}", end="")
        wh, wl = R.split(y[:M, :D])
        exp_hi = np.full(hi.shape, SENTINEL, dtype=np.float16)
        exp_hi[rows[:, None], cols[None, :]] = wh
        if lo_off is None:
            exp_lo = np.full(hi.shape, SENTINEL, dtype=np.float16)
            exp_lo[rows[:, None], cols[None, :]] = wl
            assert np.array_equal(R.bits(_np(lo)), R.bits(exp_lo)), f"{tag} {variant}: lo is not split(y).lo at its place"
        else:
            exp_hi[rows[:, None], cols[None, :] + lo_off] = wl
        assert np.array_equal(R.bits(hi), R.bits(exp_hi)), f"{tag} {variant}: hi is not split(y).hi at its place (or the border changed)"

    for M in R.LN_M:
        for kind in R.LN_ROWS:
            x, g, b = R.ln_inputs(M, D, kind)
            run(x, g, b, M, "plain", kind)
    for kind in R.LN_ROWS:
        x, g, b = R.ln_inputs(30, D, kind)
        run(x, g, b, 30, "bordered", kind)
        if D % 32 == 0:
            x, g, b = R.ln_inputs(5, D, kind, seed=1)
            run(x, g, b, 5, "interleaved", kind)
    print(f"\nln_rows D={D} worst: " + ", ".join(f"{k} {v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("D", [6, 2052])
def test_ln_rows_refusals(device, D):
    x = torch.zeros(2, D + 8, device=device)
    g = torch.ones(D + 8, device=device)
    y = torch.full((2, D + 8), SENTINEL, device=device)
    rc = _lib().ovm_op_ln_rows(x.data_ptr(), D + 8, 2, D, g.data_ptr(), g.data_ptr(), 1e-6, y.data_ptr(), D + 8, None, None, 0, 0, 0, 0,
                               _stream())
    assert rc == OVM_ERR_SHAPE and bool((_np(y) == SENTINEL).all())


# ================================================================================================ LN + GELU on split rows
# E32 / kernel error, MI355X (M = 1, M = 6); hi only: the error is the fp16 rounding, within half a spacing per element:
#   D     split                                    hi only
#   4     7.2e-08 / 1.7e-07, 2.2e-07 / 2.2e-07     6.5e-08 / 6.7e-04, 3.5e-07 / 7.1e-04
#   128   5.9e-07 / 4.4e-07, 4.4e-07 / 5.0e-07     2.3e-07 / 1.4e-03, 5.4e-07 / 1.7e-03
#   384   3.3e-07 / 3.7e-07, 5.2e-07 / 4.3e-07     4.0e-07 / 9.0e-04, 4.1e-07 / 1.8e-03
#   512   5.5e-07 / 3.4e-07, 9.6e-07 / 9.6e-07     5.3e-07 / 9.5e-04, 7.0e-07 / 1.7e-03
#   1024  8.8e-07 / 6.9e-07, 6.9e-07 / 6.9e-07     7.0e-07 / 1.5e-03, 4.6e-07 / 1.7e-03
@pytest.mark.parametrize("D", [4, 128, 384, 512, 1024])
def test_ln_gelu_split(device, D):
    """In place on [M][D] split rows. With lo the result is compared as hi + lo; without, the value is hi alone and the bound adds
    half the fp16 spacing per element (roi_glue_ref.bound_hi_only)."""
    L = _lib()
    for M in (1, 6):
        g0 = np.random.default_rng(700 + D + M)
        x = (g0.standard_normal((M, D)) * 2 + 0.5).astype(F32)
        g, b = (g0.random(D) + 0.5).astype(F32), g0.standard_normal(D).astype(F32)
        xh, xl = R.split(x)
        d_g, d_b = _dev(g, device), _dev(b, device)
        for with_lo in (True, False):
            hi, lo = _h16((M + 1, D), device), (_h16((M + 1, D), device) if with_lo else None)
            hi[:M] = _dev(xh, device)
            if with_lo:
                lo[:M] = _dev(xl, device)
            rc = L.ovm_op_ln_gelu_split(hi.data_ptr(), _ptr(lo), M, D, d_g.data_ptr(), d_b.data_ptr(), 1e-6, _stream())
            assert rc == 0
            hi = _np(hi)
            assert np.all(R.bits(hi[M]) == S16)
            r64 = R.ln_gelu(xh, xl if with_lo else None, g, b, 1e-6, F64)
            r32 = R.ln_gelu(xh, xl if with_lo else None, g, b, 1e-6, F32)
            if with_lo:
                lo = _np(lo)
                assert np.all(R.bits(lo[M]) == S16)
                e32, err = _check(f"ln_gelu D={D} M={M}", R.join(hi[:M], lo[:M]), r64, R.render(r32, F32))
            else:
                e32, tol = R.bound_hi_only(r64, r32)
                diff = np.abs(R.join(hi[:M]) - r64)
                err = float(diff.max())
                assert np.all(diff <= tol), f"ln_gelu D={D} M={M} hi only: worst excess {float((diff - tol).max()):.3e} (E32 {e32:.3e})"
            print(f"\nln_gelu_split D={D} M={M} lo={'yes' if with_lo else 'NULL'}: E32 {e32:.3e} err {err:.3e}", end="")
    x = _h16((2, 1028), device)
    g = torch.ones(1028, device=device)
    assert L.ovm_op_ln_gelu_split(x.data_ptr(), None, 2, 1028, g.data_ptr(), g.data_ptr(), 1e-6, _stream()) == OVM_ERR_SHAPE
    assert np.all(R.bits(_np(x)) == S16)


# ================================================================================================ patch gather
def _u8_call(device, imgs, G, P, Kpad, with_lo):
    from ovmono3d_amd.lib import OvmImage
    desc = (OvmImage * len(imgs))()
    keepalive = []
    for b, im in enumerate(imgs):
        H, W = im.shape[:2]
        if b % 2 == 0:                                           # CHW
            t = _dev(im.transpose(2, 0, 1), device)
            sc, sh, sw = H * W, W, 1
        else:                                                    # NHWC
            t = _dev(im, device)
            sc, sh, sw = 1, 3 * W, 3
        keepalive.append(t)
        desc[b].data, desc[b].height, desc[b].width = t.data_ptr(), H, W
        desc[b].stride_c, desc[b].stride_h, desc[b].stride_w = sc, sh, sw
    rows = len(imgs) * G * G
    hi = _h16((rows + 1, Kpad), device)
    lo = _h16((rows + 1, Kpad), device) if with_lo else None
    mean, std = (C.c_float * 3)(*R.PIXEL_MEAN), (C.c_float * 3)(*R.PIXEL_STD)
    rc = _lib().ovm_op_patch_gather(desc, len(imgs), G, P, Kpad, mean, std, hi.data_ptr(), _ptr(lo), _stream())
    return rc, _np(hi), (_np(lo) if with_lo else None)


# E32 / kernel error, MI355X:   patch 14 3.5e-07 / 3.5e-07   patch 16 3.5e-07 / 3.5e-07 (both are the split's 2^-22)
@pytest.mark.parametrize("P,G,Kpad", R.PATCH_CASES)
def test_patch_gather_u8(device, P, G, Kpad):
    """Images 30 x 37 (CHW) and 42 x 29 (NHWC) on a 42 (patch 14) / 32 (patch 16) canvas: partial patches at the right and bottom,
    empty canvas beyond; every column 0 .. Kpad - 1 of every row is written, zeros outside the image and in the K padding."""
    imgs = R.patch_images()
    r64 = R.patch_gather(imgs, G, P, Kpad, R.PIXEL_MEAN, R.PIXEL_STD, F64)
    r32 = R.render(R.patch_gather(imgs, G, P, Kpad, R.PIXEL_MEAN, R.PIXEL_STD, F32), F32)
    rows = 2 * G * G
    rc, hi, lo = _u8_call(device, imgs, G, P, Kpad, True)
    assert rc == 0
    for buf in (hi, lo):
        assert np.all(R.bits(buf[rows]) == S16), "wrote past the last row"
        assert not np.any(R.bits(buf[:rows]) == S16), "a column was not written"
    inside = np.zeros((rows, Kpad), dtype=bool)
    for b, im in enumerate(imgs):
        for gy in range(G):
            for gx in range(G):
                for py in range(min(P, max(0, im.shape[0] - gy * P))):
                    inside[(b * G + gy) * G + gx, py * P * 3:(py * P + min(P, max(0, im.shape[1] - gx * P))) * 3] = True
    assert inside.any() and (~inside[:, :3 * P * P]).any()
    assert not np.any(R.bits(hi[:rows])[~inside]) and not np.any(R.bits(lo[:rows])[~inside]), "non-zero bits outside the image"
    e32, err = _check(f"patch {P}", R.join(hi[:rows], lo[:rows]), r64, r32)
    print(f"\npatch_gather_u8 P={P}: E32 {e32:.3e} err {err:.3e}")
    rc, hi1, _ = _u8_call(device, imgs, G, P, Kpad, False)
    assert rc == 0 and np.array_equal(R.bits(hi1), R.bits(hi))


def test_patch_gather_refusals(device):
    imgs = R.patch_images()
    for P, G, Kpad in ((8, 2, 192), (16, 2, 800)):
        rc, hi, lo = _u8_call(device, imgs, G, P, Kpad, True)
        assert rc == OVM_ERR_INVALID and np.all(R.bits(hi) == S16) and np.all(R.bits(lo) == S16)


def test_patch_gather_f32(device):
    """Two overlapping 32 x 32 crops of one CHW plane, read in place through their strides: the rows are split(x), exactly."""
    L = _lib()
    plane = (np.random.default_rng(800).standard_normal((3, 40, 56)) * 3).astype(F32)
    d_p = _dev(plane, device)
    offs = ((0, 0), (8, 16))
    views = (C.c_int64 * 8)(*[v for (y, x) in offs for v in (d_p.data_ptr() + 4 * (y * 56 + x), 40 * 56, 56, 1)])
    want = R.patch_rows_f32([plane[:, y:y + 32, x:x + 32].transpose(1, 2, 0) for y, x in offs], 2)
    wh, wl = R.split(want)
    for with_lo in (True, False):
        hi, lo = _h16((9, 768), device), (_h16((9, 768), device) if with_lo else None)
        assert L.ovm_op_patch_gather_f32(views, 2, 2, 768, hi.data_ptr(), _ptr(lo), _stream()) == 0
        hi = _np(hi)
        assert np.array_equal(R.bits(hi[:8]), R.bits(wh)) and np.all(R.bits(hi[8]) == S16)
        if with_lo:
            lo = _np(lo)
            assert np.array_equal(R.bits(lo[:8]), R.bits(wl)) and np.all(R.bits(lo[8]) == S16)
    hi = _h16((9, 800), device)
    assert L.ovm_op_patch_gather_f32(views, 2, 2, 800, hi.data_ptr(), None, _stream()) == OVM_ERR_INVALID
    assert np.all(R.bits(_np(hi)) == S16)


# ================================================================================================ exact re-layouts
@pytest.mark.parametrize("D,ldo,depth", [(8, 8, False), (64, 128, True), (64, 128, False)])
@pytest.mark.parametrize("lead", [0, 1, 5])
def test_tokens_cast(device, lead, D, ldo, depth):
    B, G2 = 2, 6
    T = lead + G2
    g = np.random.default_rng(900 + lead + D)
    X = (g.standard_normal((B, T, D)) * 3).astype(F32)
    dep = (g.random(B * G2) * 5).astype(F32) if depth else None
    wh, wl = R.split(R.tokens_cast(X, G2, ldo, dep))
    d_x, d_d = _dev(X, device), (_dev(dep, device) if depth else None)
    hi, lo = _h16((B * G2 + 1, ldo), device), _h16((B * G2 + 1, ldo), device)
    rc = _lib().ovm_op_tokens_cast(d_x.data_ptr(), B, T, G2, D, ldo, _ptr(d_d), hi.data_ptr(), lo.data_ptr(), _stream())
    assert rc == 0
    hi, lo = _np(hi), _np(lo)
    assert np.array_equal(R.bits(hi[:-1]), R.bits(wh)) and np.array_equal(R.bits(lo[:-1]), R.bits(wl))
    assert np.all(R.bits(hi[-1]) == S16) and np.all(R.bits(lo[-1]) == S16)
    if ldo > D:
        assert not np.any(R.bits(hi[:-1, D + 1:])) and (np.any(R.bits(hi[:-1, D])) == depth)


@pytest.mark.parametrize("lead", [0, 1, 5])
def test_tokens_writeback(device, lead):
    B, G2, D = 2, 6, 8
    g = np.random.default_rng(950 + lead)
    X = g.standard_normal((B, lead + G2, D)).astype(F32)
    Fm = g.standard_normal((B * G2, D)).astype(F32)
    d_x, d_f = _dev(np.concatenate([X.reshape(-1), np.full(D, SENTINEL, F32)]), device), _dev(Fm, device)
    assert _lib().ovm_op_tokens_writeback(d_x.data_ptr(), d_f.data_ptr(), B, lead + G2, G2, D, _stream()) == 0
    got = _np(d_x)
    assert np.array_equal(R.bits(got[:-D]), R.bits(R.tokens_writeback(X, Fm, G2).reshape(-1))) and np.all(got[-D:] == SENTINEL)


@pytest.mark.parametrize("Rg", [0, 4])
def test_cls_init(device, Rg):
    B, G2, D = 2, 6, 8
    T = 1 + Rg + G2
    g = np.random.default_rng(970 + Rg)
    X = g.standard_normal((B, T, D)).astype(F32)
    cls, pos = g.standard_normal(D).astype(F32), g.standard_normal((1 + G2, D)).astype(F32)
    reg = g.standard_normal((Rg, D)).astype(F32) if Rg else None
    d_x, d_c, d_p = _dev(X, device), _dev(cls, device), _dev(pos, device)
    d_r = _dev(reg, device) if Rg else None
    assert _lib().ovm_op_cls_init(d_x.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), _ptr(d_r), Rg, B, T, D, _stream()) == 0
    assert np.array_equal(R.bits(_np(d_x)), R.bits(R.cls_init(X, cls, pos, reg, Rg)))


@pytest.mark.parametrize("with_lo", [True, False])
@pytest.mark.parametrize("G", [4, 5])
def test_maxpool2(device, G, with_lo):
    """Negatives, exact ties, and values whose hi parts are equal so that lo decides; G = 5 drops the last row and column. The result
    is split(max) of the reconstructed values (split is monotone)."""
    B, D, Go = 2, 8, G // 2
    xh, xl = R.split(R.maxpool_inputs(G))
    m = R.maxpool2(R.join(xh, xl if with_lo else None))
    wh, wl = R.split(m.astype(F32))
    assert np.array_equal(R.join(wh, wl), m)
    d_h, d_l = _dev(xh, device), (_dev(xl, device) if with_lo else None)
    oh, ol = _h16((B * Go * Go + 1, D), device), (_h16((B * Go * Go + 1, D), device) if with_lo else None)
    assert _lib().ovm_op_maxpool2(d_h.data_ptr(), _ptr(d_l), B, G, D, oh.data_ptr(), _ptr(ol), _stream()) == 0
    oh = _np(oh)
    assert np.array_equal(R.bits(oh[:-1]), R.bits(wh.reshape(-1, D))) and np.all(R.bits(oh[-1]) == S16)
    if with_lo:
        ol = _np(ol)
        assert np.array_equal(R.bits(ol[:-1]), R.bits(wl.reshape(-1, D))) and np.all(R.bits(ol[-1]) == S16)
