"""The evaluator's 3D stages on the device (csrc/box3d.hip ``ovm_eval_iou3d``, csrc/eval3d.hip ``ovm_eval_nhd``): the per-cell 3D
IoU bit-equal to ``ovm_box3d_iou``, the NHD against the fp64 oracle of tests/nhd_oracle.py within the host path's own error, the
pairing rule, and ``Omni3Deval(stage3d="device")`` against ``stage3d="host"``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import box3d_cases as bc
import nhd_oracle as no
from oracle import box3d as ob


def _cells(nd, ng):
    from ovmono3d_amd.evaluation.omni3d_eval import _CELL_DTYPE
    nd, ng = np.asarray(nd, np.int64), np.asarray(ng, np.int64)
    cells = np.zeros(len(nd), dtype=_CELL_DTYPE)
    cells["n_dt"], cells["n_gt"] = nd, ng
    cells["dt_off"], cells["gt_off"] = np.cumsum(nd) - nd, np.cumsum(ng) - ng
    cells["iou_off"] = np.cumsum(nd * ng) - nd * ng
    return cells


def _dev(device, a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    if a.size == 0:                                                             # keep a real allocation behind every pointer
        return torch.zeros(8, dtype=torch.uint8, device=device)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)


# ---- 1. IoU blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_iou3d_blocks_are_bit_equal_to_box3d_overlap(device):
    from ovmono3d_amd import lib
    from ovmono3d_amd.evaluation.omni3d_eval import box3d_overlap
    L = lib.load()
    sizes = [(5, 7), (0, 3), (4, 0), (1, 1), (70, 90), (33, 2), (12, 150)]
    rows = bc.sweep_rows(distances=(1.0, 3.0, 10.0, 30.0, 60.0, 100.0))
    sweep_dt = np.concatenate([r[3] for r in rows])                             # pairs i <-> i overlap
    sweep_gt = np.concatenate([r[4] for r in rows])
    degenerate = np.array([b for _, b in bc.degenerate_gt()])
    near_dt, near_gt = bc.detections_around(60, seed=1), bc.detections_around(80, seed=2)
    pick = np.random.default_rng(3).permutation(len(sweep_dt))

    def take(n_dt, n_gt, k):
        """``n_dt`` / ``n_gt`` boxes: sweep pairs from position k on (every distance and size comes up), boxes crowded around one
        point, the degenerate ground truth where there is room."""
        idx = pick[k:k + max(n_dt, n_gt)]
        n_near = n_dt // 2
        dt = np.concatenate([near_dt[:n_near], sweep_dt[idx[:n_dt - n_near]]]) if n_dt else np.zeros((0, 8, 3))
        n_deg = 4 if n_gt >= 7 else 0
        g_near = min((n_gt - n_deg) // 2, len(near_gt))
        n_sw = n_gt - n_deg - g_near
        gt = np.concatenate([near_gt[:g_near], sweep_gt[np.resize(idx, n_sw)] if n_sw else np.zeros((0, 8, 3)), degenerate[:n_deg]]) if n_gt \
            else np.zeros((0, 8, 3))
        return dt.copy(), gt.copy()
    dts, gts, k = [], [], 0
    for n_dt, n_gt in sizes:
        d, g = take(n_dt, n_gt, k)
        k += max(n_dt, n_gt)
        dts.append(d); gts.append(g)
    gts[0][1] = dts[0][0]                                                       # identical boxes: IoU 1
    gts[3][0] = dts[3][0]
    gts[4][5] = dts[4][40]
    dts[4][3, 6] += [0.3, -0.2, 0.25]                                           # a non-coplanar detection: its row is 0
    gts[4][7, 2] = np.nan                                                       # NaN corners: 0 after nan_to_num, as in the evaluator
    gts[6][100] = np.nan
    gts = [np.nan_to_num(g.astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0) for g in gts]
    dts = [d.astype(np.float32) for d in dts]
    nd, ng = [s[0] for s in sizes], [s[1] for s in sizes]
    cells = _cells(nd, ng)
    n_dt, n_iou = int(sum(nd)), int(cells["iou_off"][-1] + nd[-1] * ng[-1])
    d_cells, d_cell_of = _dev(device, cells), _dev(device, np.repeat(np.arange(len(sizes)), nd), np.int32)
    d_dt, d_gt = _dev(device, np.concatenate(dts)), _dev(device, np.concatenate(gts))
    iou = torch.full((n_iou,), -7.0, dtype=torch.float64, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.check(L.ovm_eval_iou3d(d_cells.data_ptr(), d_cell_of.data_ptr(), n_dt, d_dt.data_ptr(), d_gt.data_ptr(), 1e-4, 1e-8, iou.data_ptr(), stream),
              what="ovm_eval_iou3d")
    got = iou.cpu().numpy()
    n_mid = n_zero = n_one = 0
    for i, (d, m) in enumerate(sizes):
        ref = torch.nan_to_num(box3d_overlap(torch.from_numpy(dts[i]).to(device), torch.from_numpy(gts[i]).to(device)).double()).cpu().numpy()
        blk = got[cells["iou_off"][i]:cells["iou_off"][i] + d * m].reshape(d, m)
        assert ref.shape == blk.shape
        assert np.array_equal(blk.view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)), i
        n_mid += int(((ref > 0) & (ref < 1)).sum()); n_zero += int((ref == 0).sum()); n_one += int((ref == 1).sum())
        if i == 4:
            assert not blk[3].any() and blk[2].any()
    print(f"IoU values: {n_mid} in (0, 1), {n_zero} zeros, {n_one} ones")
    assert n_mid > 200 and n_zero > 100 and n_one >= 2


# ---- the NHD kernel on a list of single-pair cells, or on hand-made IoU rows ------------------------------------------------------
def _record(c):
    return np.concatenate([np.asarray(c["xy"], np.float32), np.asarray([c["z"]], np.float32), np.asarray(c["dimensions"], np.float32),
                           np.asarray(c["pose"], np.float32).reshape(9)])


def _run_nhd(device, nd, ng, iou, thr, dt_cub, gt_cub, dt_ok=None, gt_ok=None):
    from ovmono3d_amd import lib
    L = lib.load()
    cells = _cells(nd, ng)
    n_dt, n_gt = int(np.sum(nd)), int(np.sum(ng))
    dt_ok = np.ones(n_dt, np.uint8) if dt_ok is None else np.asarray(dt_ok, np.uint8)
    gt_ok = np.ones(n_gt, np.uint8) if gt_ok is None else np.asarray(gt_ok, np.uint8)
    assert len(iou) == int((np.asarray(nd) * np.asarray(ng)).sum()) and dt_cub.shape == (n_dt, 15) and gt_cub.shape == (n_gt, 15)
    keep = [_dev(device, cells), _dev(device, np.repeat(np.arange(len(nd)), nd), np.int32), _dev(device, iou, np.float64), _dev(device, dt_ok),
            _dev(device, gt_ok), _dev(device, dt_cub, np.float32), _dev(device, gt_cub, np.float32)]
    pair = torch.full((n_dt,), -9, dtype=torch.int32, device=device)
    nhd = torch.full((n_dt, 5), -9.0, dtype=torch.float64, device=device)
    status = torch.full((n_dt,), 9, dtype=torch.uint8, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.check(L.ovm_eval_nhd(keep[0].data_ptr(), keep[1].data_ptr(), n_dt, int(max(ng)) if len(ng) else 0, keep[2].data_ptr(), float(thr),
                             keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), keep[6].data_ptr(), pair.data_ptr(), nhd.data_ptr(),
                             status.data_ptr(), stream), what="ovm_eval_nhd")
    return pair.cpu().numpy(), nhd.cpu().numpy(), status.cpu().numpy()


def _nhd_of_pairs(device, pairs):
    """Every (pred, gt) as its own 1 x 1 cell with IoU 1."""
    n = len(pairs)
    pair, nhd, status = _run_nhd(device, [1] * n, [1] * n, np.ones(n), 0.5, np.array([_record(p) for p, _ in pairs]),
                                 np.array([_record(g) for _, g in pairs]))
    return pair, nhd, status


@functools.lru_cache(maxsize=None)
def _pair_set_tables():
    """(pairs, host [n,5], oracle [n,5]) of the shared pair set: computed once."""
    from ovmono3d_amd.evaluation import nhd
    pairs = no.pair_set()
    host = no.as_table([nhd.disentangled_nhd(p, g) for p, g in pairs])
    oracle = no.as_table([no.disentangled_nhd64(p, g) for p, g in pairs])
    return pairs, host, oracle


# ---- 2. NHD kernel against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nhd_kernel_is_at_least_as_close_to_fp64_as_the_host_path(device):
    """Bound = the host path's (nhd.disentangled_nhd, fp32 corners) largest absolute error against the fp64 oracle on the same 1,000
    pairs, measured here; the relative error is held the same way. Measured on the MI355X: host 3.898e-04 absolute and 2.417e-02
    relative (the worst pairs are 5 cm boxes at 100 m), device 1.137e-13 absolute and 6.117e-16 relative."""
    from ovmono3d_amd import lib
    pairs, host, oracle = _pair_set_tables()
    pair, got, status = _nhd_of_pairs(device, pairs)
    assert (status == lib.OVM_NHD_OK).all() and (pair == 0).all()
    h_abs, h_rel = no.error_against_oracle(host, oracle)
    d_abs, d_rel = no.error_against_oracle(got, oracle)
    print(f"NHD against fp64 on {len(pairs)} pairs: host {h_abs:.3e} abs {h_rel:.3e} rel, device {d_abs:.3e} abs {d_rel:.3e} rel")
    assert 0.0 < h_abs < 1e-2
    assert d_abs <= h_abs and d_rel <= h_rel


def _cuboid(xy, z, dims, R):
    return {"xy": list(xy), "z": float(z), "dimensions": list(dims), "pose": np.asarray(R, np.float64).tolist()}


@pytest.mark.gpu
def test_nhd_kernel_exact_cases(device):
    from scipy.spatial.transform import Rotation
    from ovmono3d_amd import lib
    from ovmono3d_amd.evaluation import nhd as host_nhd
    g = np.random.default_rng(8)
    R = Rotation.from_euler("yx", [25.0, 8.0], degrees=True).as_matrix().astype(np.float32).astype(np.float64)
    base = _cuboid([0.7, -0.3], 12.0, [1.6, 1.2, 0.8], R)
    half_turn = _cuboid(base["xy"], base["z"], base["dimensions"], R @ np.diag([-1.0, 1.0, -1.0]))       # pi about the box's y axis
    t = np.array([0.11, -0.07])
    shifted = _cuboid(np.asarray(base["xy"]) + t, base["z"], base["dimensions"], R)
    cube = _cuboid([0.2, 0.1], 6.0, [1.0, 1.0, 1.0], np.eye(3))
    cube_turned = _cuboid(cube["xy"], cube["z"], cube["dimensions"], Rotation.from_euler("y", 90, degrees=True).as_matrix().round())
    bad_pose = _cuboid(base["xy"], base["z"], base["dimensions"], R)
    bad_pose["pose"][1][1] = float("nan")
    flat_gt = _cuboid(base["xy"], base["z"], [0.0, 0.0, 0.0], R)
    rand = [(no.random_cuboid(g, float(g.uniform(1, 50))), no.random_cuboid(g, float(g.uniform(1, 50)))) for _ in range(20)]
    named = [(base, base), (half_turn, base), (shifted, base), (cube_turned, cube), (bad_pose, base), (base, flat_gt), (flat_gt, flat_gt)]
    pair, got, status = _nhd_of_pairs(device, named + rand)
    ok = lib.OVM_NHD_OK
    # identical cuboids
    assert status[0] == ok and np.array_equal(got[0], np.zeros(5))
    # the same set of corners in another order: an identity assignment would give 8 x (a diagonal of the box) / diag
    assert status[1] == ok and got[1][0] == 0.0 and got[1][4] == 0.0 and np.array_equal(got[1][1:4], np.zeros(3))
    # a small shift in xy: every corner goes with its own image
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    t32 = f32(shifted["xy"]) - f32(base["xy"])
    diag = no.extent64(no.corners64(base["xy"], base["z"], base["dimensions"], base["pose"]))
    want = 8.0 * np.linalg.norm(t32) / diag
    assert status[2] == ok and abs(got[2][0] - want) <= 1e-12 * want and abs(got[2][1] - want) <= 1e-12 * want
    assert np.array_equal(got[2][2:], np.zeros(3))
    # a cube turned by a quarter: the same corners again, every distance tied many times over
    assert status[3] == ok and np.array_equal(got[3], np.zeros(5))
    # NaN in the prediction's pose: scipy raises on the host, the pair is skipped
    with pytest.raises(ValueError):
        host_nhd.disentangled_nhd(bad_pose, base)
    assert status[4] == lib.OVM_NHD_SKIPPED and pair[4] == -1
    # zero ground-truth extent divides as IEEE does, as nhd.hungarian_distance
    with np.errstate(all="ignore"):
        h5, h6 = host_nhd.disentangled_nhd(base, flat_gt), host_nhd.disentangled_nhd(flat_gt, flat_gt)
    assert status[5] == ok and np.isinf(got[5][0]) and np.isinf(h5["overall"]) and got[5][0] > 0
    assert status[6] == ok and np.isnan(got[6]).all() and np.isnan(h6["overall"])
    # random cuboids: the assignment against brute force over all 40,320 permutations
    for i, (p, q) in enumerate(rand):
        ref = no.disentangled_nhd64(p, q, solver=no.brute_force)
        r = got[len(named) + i]
        assert status[len(named) + i] == ok
        for k, key in enumerate(no.KEYS):
            assert abs(r[k] - ref[key]) <= 1e-12 * ref[key], (i, key, r[k], ref[key])


# ---- 3. pairing -------------------------------------------------------------------------------------------------------------------
def _host_pairing(iou, thr, dt_ok, gt_ok):
    """Omni3Deval._collect_nhd's rule on one cell's [D, G] block."""
    out = -np.ones(iou.shape[0], np.int64)
    if iou.size == 0:
        return out
    best = np.argmax(iou, axis=1)
    for d, gi in enumerate(best):
        v = iou[d, gi]
        if v > 0 and v >= thr and dt_ok[d] and gt_ok[gi]:
            out[d] = gi
    return out


@pytest.mark.gpu
def test_nhd_pairing_follows_the_host_rule(device):
    from ovmono3d_amd import lib
    g = np.random.default_rng(4)
    thr = 0.5
    blocks = []
    a = g.random((6, 5)) * 0.45
    a[0, [1, 3]] = 0.8                                                          # two identical ground-truth boxes: the first wins
    a[1, 2] = 0.5                                                               # exactly at the threshold
    a[2, 4] = np.nextafter(0.5, 0)                                              # just below it
    a[3, :] = 0.0                                                               # best IoU 0
    a[4, 0] = 0.9                                                               # dt_ok cleared below
    a[5, 3] = 0.9                                                               # gt_ok cleared below
    blocks.append(a)
    blocks.append(np.zeros((3, 0)))                                             # no ground truth
    b = g.random((9, 150)) * 0.49                                               # rows wider than a wave
    b[0, [70, 5]] = 0.7                                                         # tie across lanes: the lower index
    b[1, [67, 3]] = 0.7                                                         # tie within one lane (3 and 3 + 64)
    b[2, [149, 64]] = 0.95
    b[3, 149] = 0.6
    b[4, 0] = 0.6
    b[5, 63] = b[5, 64] = 1.0
    b[6, 128] = 0.5
    b[7, 10] = 0.9                                                              # dt_ok cleared below
    blocks.append(b)
    blocks.append(np.array([[0.0]]))
    blocks.append(np.array([[1.0]]))
    nd, ng = [x.shape[0] for x in blocks], [x.shape[1] for x in blocks]
    dt_ok, gt_ok = np.ones(sum(nd), np.uint8), np.ones(sum(ng), np.uint8)
    dt_ok[4] = 0
    gt_ok[3] = 0
    dt_ok[6 + 3 + 7] = 0                                                        # row 7 of the wide cell
    cub = lambda n: np.array([_record(no.random_cuboid(g, 10.0)) for _ in range(n)]).reshape(n, 15)
    pair, nhd, status = _run_nhd(device, nd, ng, np.concatenate([x.ravel() for x in blocks]), thr, cub(sum(nd)), cub(sum(ng)), dt_ok, gt_ok)
    want, r, q = [], 0, 0
    for x in blocks:
        want.append(_host_pairing(x, thr, dt_ok[r:r + x.shape[0]], gt_ok[q:q + x.shape[1]]))
        r, q = r + x.shape[0], q + x.shape[1]
    want = np.concatenate(want)
    assert np.array_equal(pair, want)
    assert list(want[:6]) == [1, 2, -1, -1, -1, -1] and list(want[9:16]) == [5, 3, 64, 149, 0, 63, 128] and list(want[-2:]) == [-1, 0]
    assert np.array_equal(status, np.where(want >= 0, lib.OVM_NHD_OK, lib.OVM_NHD_NONE))
    assert np.isfinite(nhd[want >= 0]).all() and (nhd[want < 0] == -9.0).all()    # rows without a pair are not written


# ---- 4. the evaluator -----------------------------------------------------------------------------------------------------------
def _project(c3):
    u, v = 500.0 * c3[:, 0] / c3[:, 2] + 640.0, 500.0 * c3[:, 1] / c3[:, 2] + 360.0
    return [float(u.min()), float(v.min()), float(u.max() - u.min()), float(v.max() - v.min())]


def _rec(img, cat, cub, score=None, **kw):
    """A record with every 3D field; ``cub`` as nhd_oracle's cuboids (dimensions W, H, L; L along the box's x axis)."""
    w, h, l = cub["dimensions"]
    centre = [cub["xy"][0], cub["xy"][1], cub["z"]]
    c3 = ob.make_box(centre, [l, h, w], cub["pose"])
    r = {"image_id": img, "category_id": cat, "bbox": _project(c3), "bbox3D": c3.tolist(), "depth": cub["z"], "center_cam": centre,
         "dimensions": [w, h, l], **kw}
    if score is None:
        r["R_cam"] = cub["pose"]
    else:
        r["pose"], r["score"] = cub["pose"], score
    return r


def _scene3d(seed):
    """Images 1-8 x categories 0-2 of 0-5 cuboids at 2-12 m with detections that are perturbed copies or strangers; image 20 / category
    0 holds 150 ground-truth boxes, image 21 / category 1 only ignored ones, image 22 / category 2 only detections, image 23 / category
    0 only ground truth; image 30 and category 3 are evaluated but empty. Eight detections lack ``pose``, eight ground truths ``R_cam``."""
    g = np.random.default_rng(seed)
    gts, dts = [], []

    def fill(img, cat, n_gt, n_dt, ignore=None, depth=None):
        mine = [no.random_cuboid(g, float(g.uniform(2, 12)) if depth is None else depth, 0.4, 3.0) for _ in range(n_gt)]
        for c in mine:
            gts.append(_rec(img, cat, c, ignore2D=int(g.random() < 0.15) if ignore is None else ignore,
                            ignore3D=int(g.random() < 0.15) if ignore is None else ignore))
        for _ in range(n_dt):
            if mine and g.random() < 0.7:
                c = no.perturbed(g, mine[int(g.integers(0, len(mine)))])
            else:
                c = no.random_cuboid(g, float(g.uniform(2, 12)), 0.4, 3.0)
            dts.append(_rec(img, cat, c, score=float(g.choice([0.9, 0.8, 0.8, 0.5, 0.3, 0.3, 0.1]))))
    for img in range(1, 9):
        for cat in range(3):
            if g.random() < 0.1:
                continue
            fill(img, cat, 0 if g.random() < 0.1 else int(g.integers(1, 6)), int(g.integers(0, 16)))
    fill(20, 0, 150, 120, depth=10.0)
    fill(21, 1, 4, 6, ignore=1)
    fill(22, 2, 0, 5)
    fill(23, 0, 3, 0)
    for d in [d for d in dts if d["image_id"] == 20][:8]:
        del d["pose"]
    for t in [t for t in gts if t["image_id"] == 20][:8]:
        del t["R_cam"]
    return gts, dts, list(range(1, 9)) + [20, 21, 22, 23, 30], [0, 1, 2, 3], {2, 3, 20, 21}


def _host_pairs(e, need_fields=True):
    """The (pred, gt) cuboids behind ``e.nhd_pairs``, by the rule of Omni3Deval._collect_nhd."""
    pairs = []
    for key in sorted(e.cells, key=lambda k: (str(k[1]), str(k[0]))):
        c = e.cells[key]
        if not c.dt or not c.gt:
            continue
        for di, gi in enumerate(np.argmax(c.iou, axis=1)):
            v, d, t = c.iou[di, gi], c.dt[di], c.gt[gi]
            if v > 0 and v >= e.nhd_iou_threshold and not need_fields:
                pairs.append((d, t))
            elif v > 0 and v >= e.nhd_iou_threshold and "pose" in d and "R_cam" in t:
                pairs.append(({"xy": d["center_cam"][:2], "z": d["depth"], "dimensions": d["dimensions"], "pose": d["pose"]},
                              {"xy": t["center_cam"][:2], "z": t["depth"], "dimensions": t["dimensions"], "pose": t["R_cam"]}))
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42])
def test_stage3d_device_equals_host(device, seed):
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    gts, dts, img_ids, cat_ids, prox = _scene3d(seed)
    runs = {}
    for name, matcher, stage in (("host", "host", "host"), ("match", "device", "host"), ("dev", "device", "device")):
        e = Omni3Deval(gts, dts, "3D", device=device, img_ids=img_ids, cat_ids=cat_ids, eval_prox=prox, matcher=matcher, stage3d=stage)
        e.evaluate(); e.accumulate()
        runs[name] = e
    h, d = runs["match"], runs["dev"]
    assert max(len(c.gt) for c in h.cells.values()) == 150 and max(len(c.dt) for c in h.cells.values()) == 100
    assert any(c.prox for c in h.cells.values()) and not all(c.prox for c in h.cells.values())
    for ref in (runs["host"], h):
        assert set(ref.per_cell) == set(d.per_cell) and len(d.per_cell) > 0
        for key, r in ref.per_cell.items():
            s = d.per_cell[key]
            for field in ("score", "matched", "ignored", "pick", "gt_order"):
                assert r[field].shape == s[field].shape and np.array_equal(r[field], s[field]), (key, field)
            assert r["n_gt"] == s["n_gt"], key
        for key, c in ref.cells.items():
            other = d.cells[key].iou
            assert c.iou.shape == other.shape and c.iou.dtype == other.dtype == np.float64
            assert np.ascontiguousarray(c.iou).tobytes() == np.ascontiguousarray(other).tobytes(), key
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(ref.eval[k], d.eval[k]), k
    # the NHD: the same pairs in the same order, every value within twice the host path's own error on these pairs (the
    # device is at least as close to fp64 as the host is - test 2 - so the triangle inequality gives 2 x)
    pairs = _host_pairs(h)
    assert len(pairs) == len(h.nhd_pairs) == len(d.nhd_pairs) == len(runs["host"].nhd_pairs)
    host = no.as_table(h.nhd_pairs)
    oracle = no.as_table([no.disentangled_nhd64(p, q) for p, q in pairs])
    got = no.as_table(d.nhd_pairs)
    e_host = float(np.abs(host - oracle).max())
    print(f"seed {seed}: {len(pairs)} pairs, host against fp64 {e_host:.3e}, device against host {np.abs(got - host).max():.3e}, "
          f"device against fp64 {np.abs(got - oracle).max():.3e}")
    assert e_host > 0 and np.isfinite(oracle).all()
    assert [list(p) for p in d.nhd_pairs] == [list(p) for p in h.nhd_pairs]     # the same dict keys
    assert d.nhd_pair_ids == h.nhd_pair_ids == runs["host"].nhd_pair_ids        # the same (detection, ground truth) pairs in the same order
    assert len(set(d.nhd_pair_ids)) == len(pairs)
    assert (np.abs(got - host) <= 2 * e_host).all()
    for k in no.KEYS:
        assert abs(d.eval["average_nhd"][k] - h.eval["average_nhd"][k]) <= 2 * e_host, k
        assert len(d.eval["nhd_accumulators"][k]) == len(pairs)
    assert len(pairs) >= 100                                                    # at least 200 over the two scenes
    assert len(_host_pairs(h, need_fields=False)) > len(pairs)                  # records without their fields did lose pairs
