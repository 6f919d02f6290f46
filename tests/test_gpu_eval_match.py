"""The evaluator's HIP matcher (csrc/eval_match.hip): the 2D IoU kernel bit-equal to the host's IoU, and matcher="device" equal to
matcher="host" exactly - per-cell picks, ignore flags and ground-truth counts, then the precision / recall / score tables."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_eval_novel import _ann, _random_scene, two_datasets


@pytest.mark.gpu
def test_iou2d_kernel_is_bit_equal_to_the_host_iou(device):
    from ovmono3d_amd import lib
    from ovmono3d_amd.evaluation.omni3d_eval import _CELL_DTYPE, iou2d_xywh
    L = lib.load()
    g = np.random.default_rng(0)

    def boxes(n):
        b = np.column_stack([g.uniform(-50, 200, n), g.uniform(-50, 200, n), g.uniform(0, 120, n), g.uniform(0, 120, n)])
        b[g.random(n) < 0.15, 2] = 0.0                                          # zero width
        b[g.random(n) < 0.15, 3] = 0.0                                          # zero height
        if n:
            b[g.random(n) < 0.1] = b[0]                                        # repeated boxes
        return b
    sizes = [(5, 7), (0, 3), (4, 0), (70, 90), (1, 1), (12, 200), (33, 2)]
    dts = [boxes(d) for d, _ in sizes]
    gts = [boxes(m) for _, m in sizes]
    dts[4][:] = [3.0, 4.0, 0.0, 0.0]                                            # zero union: IoU 0
    gts[4][:] = [3.0, 4.0, 0.0, 0.0]
    gts[0][:2] = dts[0][:2] = [[1.5, 2.5, 30.25, 40.125], [7.0, 9.0, 11.0, 13.0]]   # identical boxes: IoU 1
    dts[6][:, 2:] *= 1e-7                                                       # tiny and large magnitudes
    gts[6][:, :2] += 1e6
    nd, ng = np.array([d for d, _ in sizes]), np.array([m for _, m in sizes])
    cells = np.zeros(len(sizes), dtype=_CELL_DTYPE)
    cells["n_dt"], cells["n_gt"] = nd, ng
    cells["dt_off"], cells["gt_off"] = np.cumsum(nd) - nd, np.cumsum(ng) - ng
    cells["iou_off"] = np.cumsum(nd * ng) - nd * ng
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).to(device)
    d_cells = t(cells.view(np.uint8))
    d_cell_of = t(np.repeat(np.arange(len(sizes)), nd), np.int32)
    d_dt, d_gt = t(np.concatenate(dts)), t(np.concatenate(gts))
    iou = torch.full((int((nd * ng).sum()),), -7.0, dtype=torch.float64, device=device)
    prox = torch.full((int(nd.sum()),), 9, dtype=torch.uint8, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.check(L.ovm_eval_iou2d(d_cells.data_ptr(), d_cell_of.data_ptr(), int(nd.sum()), d_dt.data_ptr(), d_gt.data_ptr(), 0.3, iou.data_ptr(),
                               prox.data_ptr(), stream), what="ovm_eval_iou2d")
    got, got_prox = iou.cpu().numpy(), prox.cpu().numpy()
    n_mid = 0
    for i, (d, m) in enumerate(sizes):
        ref = iou2d_xywh(dts[i], gts[i])
        blk = got[cells["iou_off"][i]:cells["iou_off"][i] + d * m].reshape(d, m)
        assert np.array_equal(blk.view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)), i
        assert np.array_equal(got_prox[cells["dt_off"][i]:cells["dt_off"][i] + d], (ref > 0.3).any(axis=1).astype(np.uint8)), i
        n_mid += int(((ref > 0) & (ref < 1)).sum())
    assert n_mid > 500 and (got == 0).sum() > 100 and (got == 1).sum() >= 2


def _scene(seed):
    """The random crowded scene plus a cell with 150 ground-truth boxes (more than one wave's lanes), a cell whose ground truth is
    all ignored, a cell with detections only; image 30 and category 3 are evaluated but empty."""
    gts, dts = _random_scene(seed, n_img=8)
    g = np.random.default_rng(seed + 100)
    big = []
    for i in range(150):
        x, y = float(g.integers(0, 40)) * 15, float(g.integers(0, 30)) * 15
        w, h = float(g.choice([20, 30, 45])), float(g.choice([20, 30, 45]))
        big.append([x, y, w, h])
        gts.append(_ann(20, 0, [x, y, w, h], depth=float(g.choice([5.0, 20.0, 60.0])), ignore2D=int(g.random() < 0.1),
                        ignore3D=int(g.random() < 0.1)))
    for i in range(120):
        x, y, w, h = big[int(g.integers(0, 150))]
        dts.append(_ann(20, 0, [x + float(g.choice([0, 3, -5])), y + float(g.choice([0, 4])), w, h], depth=float(g.choice([5.0, 20.0, 60.0])),
                        score=float(g.choice([0.9, 0.7, 0.7, 0.4]))))
    for i in range(4):
        gts.append(_ann(21, 1, [10.0 + 30 * i, 10.0, 40.0, 40.0], ignore2D=1, ignore3D=1))
        dts.append(_ann(21, 1, [12.0 + 30 * i, 10.0, 40.0, 40.0], score=0.5 + 0.1 * i))
        dts.append(_ann(22, 2, [12.0 + 30 * i, 10.0, 40.0, 40.0], score=0.5))
    img_ids = list(range(1, 10)) + [20, 21, 22, 30]
    return gts, dts, img_ids, [0, 1, 2, 3]


def _same_cells(h, d):
    assert set(h.per_cell) == set(d.per_cell) and len(h.per_cell) > 0
    for key, r in h.per_cell.items():
        s = d.per_cell[key]
        for field in ("score", "matched", "ignored", "pick", "gt_order"):
            assert r[field].shape == s[field].shape and np.array_equal(r[field], s[field]), (key, field)
        assert r["n_gt"] == s["n_gt"], key
    for key, c in h.cells.items():
        assert np.array_equal(c.iou, d.cells[key].iou), key


@pytest.mark.gpu
@pytest.mark.parametrize("mode,fork", [("2D", False), ("3D", False), ("3D", True)])
@pytest.mark.parametrize("prox", [False, True])
@pytest.mark.parametrize("seed", [31, 32])
def test_device_matcher_equals_host(device, mode, fork, prox, seed):
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    gts, dts, img_ids, cat_ids = _scene(seed)
    runs = {}
    for matcher in ("host", "device"):
        e = Omni3Deval(gts, dts, mode, device=device, fork_compat_2d_iou=fork, img_ids=img_ids, cat_ids=cat_ids, eval_prox=prox, matcher=matcher)
        e.evaluate(); e.accumulate()
        runs[matcher] = e
    h, d = runs["host"], runs["device"]
    assert max(len(c.gt) for c in h.cells.values()) == 150 and max(len(c.dt) for c in h.cells.values()) == 100
    _same_cells(h, d)
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(h.eval[k], d.eval[k]), k
    _same_results(h.summarize(), d.summarize())
    n_match = sum(int(r["matched"].sum()) for r in h.per_cell.values())
    n_ign = sum(int(r["ignored"].sum()) for r in h.per_cell.values())
    assert n_match > 1000 and n_ign > 100


def _same_results(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same_results(a[k], b[k])
    else:
        assert (np.isnan(a) and np.isnan(b)) or a == b, (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("fork", [False, True])
def test_evaluate_omni3d_device_equals_host_on_two_datasets(device, fork):
    from ovmono3d_amd.evaluation import evaluate_omni3d
    _, _, gt, dts, prox_imgs = two_datasets(7)
    host = evaluate_omni3d(gt, dts, device=device, fork_compat_2d_iou=fork, eval_prox=prox_imgs)
    dev = evaluate_omni3d(gt, dts, device=device, fork_compat_2d_iou=fork, eval_prox=prox_imgs, matcher="device")
    _same_results(host, dev)
    plain = evaluate_omni3d(gt, dts, device=device, fork_compat_2d_iou=fork, matcher="device")
    assert plain["bbox_2D"] != dev["bbox_2D"]                                   # the proximity rule does act on this sample
