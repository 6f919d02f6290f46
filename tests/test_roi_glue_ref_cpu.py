"""tests/roi_glue_ref.py against independent code on the CPU (no GPU): the fp64 restatement that tests/test_gpu_roi_glue.py holds the
kernels to must itself agree with torch's own ops, with the oracle (oracle/roi_ops.py, oracle/heads.py, written from the reference)
and with plain loops. Also asserts, with the restatement alone, the conditions the GPU cases rely on: no input of a GPU case sits
where its result jumps (a level boundary, a sample grid size, a sample on the validity edge), and the rows built to be exact are."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_glue_ref as R
from roi_glue_ref import F32, F64


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64))) / max(float(np.max(np.abs(b))), 1e-30))


def test_split_is_the_definition_and_join_is_exact_in_fp32():
    x = (np.random.default_rng(0).standard_normal(4096) * np.logspace(-6, 3, 4096)).astype(F32)
    hi, lo = R.split(x)
    assert np.array_equal(hi, torch.from_numpy(x).half().numpy())
    assert np.array_equal(lo, (torch.from_numpy(x) - torch.from_numpy(x).half().float()).half().numpy())
    j = R.join(hi, lo)
    assert np.array_equal(j.astype(F32).astype(F64), j)                       # hi + lo is an fp32 number
    assert np.all(np.abs(j - x) <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25))   # 22 bits, or half the fp16 subnormal spacing
    assert [R.il_col(k) for k in (0, 31, 32, 63, 64)] == [0, 31, 64, 95, 128]


@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_layer_norm_and_gelu_vs_torch(rows):
    for D in (4, 260, 1536):
        x, g, b = R.ln_inputs(5, D, rows)
        ref = F.layer_norm(torch.from_numpy(x).double(), (D,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-6)
        y = R.layer_norm(x, g, b, 1e-6, F64)
        # eps enters as the fp32 number the kernel receives; for a constant row that is all of the denominator
        assert _rel(y, ref.numpy()) <= 1e-7
        assert R.layer_norm(x, g, b, 1e-6, F32).dtype == F32
    z = np.linspace(-6, 6, 1001)
    assert _rel(R.gelu(z), F.gelu(torch.from_numpy(z)).numpy()) <= 1e-15
    assert R.gelu(z.astype(F32)).dtype == F32
    hi, lo = R.split(x)
    ref = F.gelu(F.layer_norm(torch.from_numpy(R.join(hi, lo)), (D,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-6))
    assert _rel(R.ln_gelu(hi, lo, g, b, 1e-6, F64), ref.numpy()) <= 1e-7


@pytest.mark.parametrize("G", [4, 5])
def test_maxpool_vs_torch_and_its_inputs(G):
    x = R.maxpool_inputs(G)
    hi, lo = R.split(x)
    for v in (R.join(hi, lo), R.join(hi)):
        ref = F.max_pool2d(torch.from_numpy(v).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()
        got = R.maxpool2(v)
        assert got.shape == (2, G // 2, G // 2, 8) and np.array_equal(got, ref)
    # the inputs hold what the GPU test says they hold
    assert np.array_equal(R.bits(hi[0, 0, 0]), R.bits(hi[0, 1, 0])) and np.all(R.join(hi, lo)[0, 1, 0] > R.join(hi, lo)[0, 0, 0])
    assert np.array_equal(R.bits(hi[0, 1, 0]), R.bits(hi[0, 1, 1])) and not np.array_equal(R.bits(lo[0, 1, 0]), R.bits(lo[0, 1, 1]))
    assert np.array_equal(x[0, 0, 0], x[0, 0, 1]) and np.all(x[0, 0:2, 2:4] < 0) and np.all(x[1, 2:4, 0:2] == x[1, 2, 0])


@pytest.mark.parametrize("max_level", [5, 4])
def test_level_rule_vs_oracle_and_margin(max_level):
    from oracle.roi_ops import assign_boxes_to_levels
    boxes = R.level_boxes()
    ref = assign_boxes_to_levels(torch.from_numpy(boxes), 2, max_level).numpy()
    for dt in (F32, F64):
        assert np.array_equal(R.roi_levels(boxes, 2, max_level, dt), ref)
    # 56, 112 (and 56 x 224), 224, 448, 896 -> levels 2, 3, 3, 4, 5, 5 before the clamp
    assert ref[:5].tolist() == [0, 1, 2, min(3, max_level - 2), min(3, max_level - 2)] and ref[-1] == 1
    t = R.roi_level_arg(boxes, F64)
    on = np.abs(t - np.rint(t)) < 1e-7                       # the 1e-8 inside the log moves an exact size by 1e-8 / ln 2
    assert on[:5].all() and on[-1] and not on[5:-1].any()
    assert np.all(np.abs(t - np.rint(t))[~on] >= 1e-4)
    # ... and on the boundary the fp32 evaluation is exact: x + 1e-8 == x and log2 of a power of two
    t32 = R.roi_level_arg(boxes, F32)
    assert np.array_equal(t32[on], np.rint(t32[on]))


def _value_levels(boxes):
    lv = R.roi_levels(boxes, 2, 4, F64)
    assert np.array_equal(lv, R.roi_levels(boxes, 2, 4, F32))
    assert (lv == -1).tolist() == [r == 11 for r in range(len(boxes))]
    t = R.roi_level_arg(boxes, F64)
    ok = ~np.isnan(t) & np.isfinite(t)
    assert np.all(np.abs(t - np.rint(t))[ok] >= 1e-4)
    return lv


@pytest.mark.parametrize("out", [1, 7])
def test_roi_align_vs_oracle_and_margins(out):
    from oracle.roi_ops import roi_align_single
    boxes, idx = R.value_boxes()
    assert idx.tolist()[:4] == [1, 0, 1, 0]
    lv = _value_levels(boxes)
    assert set(lv.tolist()) == {-1, 0, 1, 2}
    feats = R.value_feats(4)
    margins = {}
    r64 = R.roi_align(feats, R.VAL_SCALES, boxes, idx, lv, out, F64, margins)
    r32 = R.roi_align(feats, R.VAL_SCALES, boxes, idx, lv, out, F32)
    # fp32 coordinates (|x| < 100) carry ~1e-5: the cases stay 1e-3 away from every jump, so both runs sample the same grid
    assert margins["grid"] >= 1e-3 and margins["edge"] >= 1e-3, margins
    for r in range(len(boxes)):
        l = max(int(lv[r]), 0)
        ref = roi_align_single(torch.from_numpy(feats[l][idx[r]]).permute(2, 0, 1), torch.from_numpy(boxes[r]), R.VAL_SCALES[l], out)
        ref = ref.permute(1, 2, 0).reshape(-1).numpy()
        scale = max(float(np.abs(r64[r]).max()), 1e-30)
        assert np.max(np.abs(r64[r] - ref)) <= 2e-5 * scale + 1e-30, r
        assert np.max(np.abs(r32[r] - r64[r])) <= 2e-5 * scale + 1e-30, r
    for r in (0, 8, 11):                                     # zero width, wholly outside, x2 < x1
        assert not r64[r].any() and not r32[r].any()
    assert r64[3].any() and r64[1].any()
    g = [int(np.ceil((boxes[3, 2 + a] - boxes[3, a]) / 16 / out)) for a in (0, 1)]
    assert g == ([10, 10] if out == 7 else [65, 65])         # the big box: 10 x 10 samples per bin at out = 7


def test_roi_align_vs_torchvision():
    tv = pytest.importorskip("torchvision")
    boxes, idx = R.value_boxes()
    lv = _value_levels(boxes)
    feats = R.value_feats(4)
    r64 = R.roi_align(feats, R.VAL_SCALES, boxes, idx, lv, 7, F64)
    for r in range(len(boxes)):
        if lv[r] < 0:
            continue
        f = torch.from_numpy(feats[lv[r]][idx[r]]).permute(2, 0, 1)[None].double()
        ref = tv.ops.roi_align(f, [torch.from_numpy(boxes[r:r + 1]).double()], 7, R.VAL_SCALES[lv[r]], 0, True)[0]
        assert _rel(r64[r], ref.permute(1, 2, 0).reshape(-1).numpy()) <= 1e-6 or not r64[r].any()


@pytest.mark.parametrize("postprocess", [0, 1])
def test_cube_decode_vs_oracle_and_exact_rows(postprocess):
    from oracle import heads as OH
    n = 40
    d = R.decode_inputs(n, 16)
    head, boxes, idx, metas = d["head"], d["boxes"], d["idx"], d["metas"]
    r64, k64 = R.cube_decode(head, boxes, d["scores"], idx, metas, 512.0, postprocess, F64)
    r32, k32 = R.cube_decode(head, boxes, d["scores"], idx, metas, 512.0, postprocess, F32)
    assert np.array_equal(k64, k32) and r32.dtype == F32
    names = d["names"]
    inv = {v: k for k, v in names.items()}
    assert len(inv) == 14
    if postprocess:
        assert k64.sum() == n - 2 and k64[inv["empty_x"]] == 0 and k64[inv["empty_y"]] == 0
        bx = r64[inv["empty_x"], 0:4]; by = r64[inv["empty_y"], 0:4]
        assert bx[2] - bx[0] == 0 and bx[3] - bx[1] > 0 and by[3] - by[1] == 0 and by[2] - by[0] > 0
    else:
        assert k64.all() and np.array_equal(r64[:, 0:4], boxes.astype(F64))
    # the oracle, as tests/test_gpu_ops.py::test_cube_decode replays it (fp32 torch)
    th, tb, ti = torch.from_numpy(head), torch.from_numpy(boxes), torch.from_numpy(idx).long()
    Ks = torch.stack([torch.tensor(m["K"], dtype=torch.float32).view(3, 3) for m in metas])
    ratios = torch.tensor([m["oh"] / m["h"] for m in metas], dtype=torch.float32)
    Ks_box = (Ks / ratios[:, None, None])[ti]
    Ks_box[:, -1, -1] = 1
    rat, ims = ratios[ti], torch.tensor([float(m["h"]) for m in metas])[ti]
    v2r = OH.compute_virtual_scale_from_focal_spaces(Ks[ti][:, 1, 1], ims * rat, 512.0, ims)
    sw, sh = tb[:, 2] - tb[:, 0], tb[:, 3] - tb[:, 1]
    cx = tb[:, 0] + 0.5 * sw + sw * th[:, 0]
    cy = tb[:, 1] + 0.5 * sh + sh * th[:, 1]
    dims = torch.exp(th[:, 2:5].clip(max=5))
    pose = OH.R_from_allocentric(Ks_box, OH.rotation_6d_to_matrix(th[:, 5:11]), cx, cy)
    z = th[:, 11] * v2r
    x3 = z * (cx - Ks_box[:, 0, 2]) / Ks_box[:, 0, 0]
    y3 = z * (cy - Ks_box[:, 1, 2]) / Ks_box[:, 1, 1]
    conf = torch.exp(-th[:, 12].clip(0.01))
    verts = OH.get_cuboid_verts(torch.cat([torch.stack([x3, y3, z], 1), dims], 1), pose)
    want = {"score": (torch.from_numpy(d["scores"]) * conf).sqrt()[:, None], "bbox3D": verts.reshape(n, 24),
            "center_cam": torch.stack([x3, y3, z], 1), "center_2D": torch.stack([cx, cy], 1) * rat[:, None], "dimensions": dims,
            "pose": pose.reshape(n, 9)}
    # rows whose pose no fp32 evaluation pins down: a2 parallel to a1 by rounding only, and acos next to 1 (E32 ~ 1e-4, see the GPU test)
    loose = {inv["a2_parallel"], inv["off_1e-3"], inv["off_0.1"], inv["off_1"]}
    for name, a, b in R.FIELDS:
        if name == "box":
            continue
        w = want[name].double().numpy()
        for i in range(n):
            tol = 2e-3 if (i in loose and name in ("pose", "bbox3D")) else 2e-5
            assert np.max(np.abs(r64[i, a:b] - w[i])) <= tol * max(float(np.abs(w[i]).max()), 1.0), (name, i, names.get(i))
    # rows built to be exact: on the principal point the ray is (0, 0, 1) in fp32 and fp64 alike, angle == 0, R is the 6D matrix
    for nm in ("on_pp", "on_pp_far_pose"):
        i = inv[nm]
        for rr, dt in ((r64, F64), (r32, F32)):
            b1 = R._unit(head[i, 5:8].astype(dt), dt)
            b2 = R._unit(head[i, 8:11].astype(dt) - (b1 * head[i, 8:11].astype(dt)).sum() * b1, dt)
            assert np.array_equal(rr[i, 38:47], np.stack([b1, b2, np.cross(b1, b2)]).reshape(-1))
            assert rr[i, 30] == 0 and rr[i, 31] == 0 and rr[i, 33] == 320 and rr[i, 34] == 240
    i = inv["a2_parallel_exact"]
    assert r64[i, 38:47].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0] and r32[i, 38:47].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert np.linalg.matrix_rank(r64[inv["a1_zero"], 38:47].reshape(3, 3)) == 1 and np.isfinite(r64).all() and np.isfinite(r32).all()
    assert r64[inv["uncert_low"], 4] == np.sqrt(F64(d["scores"][inv["uncert_low"]]) * np.exp(-F64(F32(0.01))))
    assert np.allclose(r64[inv["dims_at_5"], 35:38], np.exp(5.0)) and np.allclose(r64[inv["dims_above_5"], 35:38], np.exp(5.0))
    assert r64[inv["neg_z"], 32] < 0


@pytest.mark.parametrize("n", R.COMPACT_N)
def test_compaction_vs_plain_loop(n):
    for pattern in R.COMPACT_KEEP:
        rec, keep = R.compact_inputs(n, pattern)
        out, counts = R.compact_records(rec, keep, 3)
        rows, cnt = [], [0, 0, 0]
        for i in range(n):
            if keep[i]:
                rows.append(rec[i])
                cnt[int(rec[i, 47])] += 1
        assert len(out) == len(rows) and all(np.array_equal(a, b) for a, b in zip(out, rows))
        assert counts.tolist() == cnt and cnt[1] == 0
        assert len(rows) == {"all": n, "none": 0, "last": 1}.get(pattern, len(rows))


def test_patch_rows_and_relayouts_against_torch_indexing():
    imgs = R.patch_images()
    for P, G, Kpad in R.PATCH_CASES:
        rows = R.patch_gather(imgs, G, P, Kpad, R.PIXEL_MEAN, R.PIXEL_STD, F64)
        assert rows.shape == (2 * G * G, Kpad) and not rows[:, 3 * P * P:].any()
        for b, im in enumerate(imgs):
            canvas = torch.zeros(3, G * P, G * P, dtype=torch.float64)
            h, w = min(im.shape[0], G * P), min(im.shape[1], G * P)
            t = (torch.from_numpy(im).permute(2, 0, 1).double() - torch.tensor(R.PIXEL_MEAN, dtype=torch.float32).double()[:, None, None]) \
                / torch.tensor(R.PIXEL_STD, dtype=torch.float32).double()[:, None, None]
            canvas[:, :h, :w] = t[:, :h, :w]
            ref = F.unfold(canvas[None], P, stride=P)[0].T.reshape(G * G, 3, P, P).permute(0, 2, 3, 1).reshape(G * G, -1)
            assert np.array_equal(rows[b * G * G:(b + 1) * G * G, :3 * P * P], ref.numpy())
            assert h < G * P or w < G * P                        # each image leaves part of the canvas empty
    v = np.random.default_rng(1).standard_normal((2, 32, 32, 3)).astype(F32)
    ref = F.unfold(torch.from_numpy(v).permute(0, 3, 1, 2), 16, stride=16).transpose(1, 2).reshape(8, 3, 16, 16).permute(0, 2, 3, 1).reshape(8, -1)
    assert np.array_equal(R.patch_rows_f32(list(v), 2), ref.numpy())
    X = np.random.default_rng(2).standard_normal((2, 11, 8)).astype(F32)
    dep = np.arange(12, dtype=F32) + 1
    tc = R.tokens_cast(X, 6, 16, dep)
    assert np.array_equal(tc[:, :8], X[:, 5:].reshape(12, 8)) and np.array_equal(tc[:, 8], dep) and not tc[:, 9:].any()
    assert not R.tokens_cast(X, 6, 16, None)[:, 8:].any()
    Fm = -X[:, :6].reshape(12, 8)
    wb = R.tokens_writeback(X, Fm, 6)
    assert np.array_equal(wb[:, :5], X[:, :5]) and np.array_equal(wb[:, 5:].reshape(12, 8), Fm)
    cls, pos, reg = (np.random.default_rng(s).standard_normal(sh).astype(F32) for s, sh in ((3, 8), (4, (7, 8)), (5, (4, 8))))
    ci = R.cls_init(X, cls, pos, reg, 4)
    assert np.array_equal(ci[:, 0], np.broadcast_to(cls + pos[0], (2, 8))) and np.array_equal(ci[:, 1:5], np.broadcast_to(reg, (2, 4, 8)))
    assert np.array_equal(ci[:, 5:], X[:, 5:]) and np.array_equal(R.cls_init(X, cls, pos, None, 0)[:, 1:], X[:, 1:])
    assert np.array_equal(R.bordered_rows(2, 3, 5)[[0, 4, 5, 15]], [8, 12, 15, 43])


def test_bound_is_the_rule():
    ref = np.array([1.0, -3.0, 0.5])
    e32, tol = R.bound(ref, ref + np.array([0.0, 1e-7, -2e-7]))
    assert abs(e32 - 2e-7) < 1e-12 and tol == 4 * e32 + float(np.spacing(F32(3.0)))
    e32, tol = R.bound(np.zeros(3), np.zeros(3))
    assert e32 == 0 and 0 < tol < 1e-40
    _, t = R.bound_hi_only(ref, ref)
    assert np.allclose(t - float(np.spacing(F32(3.0))), [2.0 ** -11, 2.0 ** -10, 2.0 ** -12])
