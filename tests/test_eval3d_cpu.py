"""The evaluator's ``stage3d`` keyword and the yardsticks of the device NHD test, without a GPU: the fp64 oracle of
tests/nhd_oracle.py against brute force, the subset recurrence the kernel uses against scipy, and the host path's distance to
the oracle (the bound tests/test_gpu_eval3d.py holds the kernel to)."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import nhd_oracle as no
from test_eval_novel import _ann


def test_stage3d_validation():
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    with pytest.raises(ValueError, match="stage3d"):
        Omni3Deval([], [], "3D", matcher="device", stage3d="gpu")
    with pytest.raises(ValueError, match="stage3d"):
        Omni3Deval([], [], "3D", matcher="host", stage3d="device")
    with pytest.raises(ValueError, match="stage3d"):
        Omni3Deval([], [], "2D", matcher="device", stage3d="device")
    with pytest.raises(ValueError, match="stage3d"):
        Omni3Deval([], [], "3D", matcher="device", fork_compat_2d_iou=True, stage3d="device")
    assert Omni3Deval([], [], "3D").stage3d == "host"
    assert Omni3Deval([], [], "3D", matcher="device", stage3d="device").stage3d == "device"


def test_stage3d_device_has_no_cpu_fallback(monkeypatch):
    import torch
    from ovmono3d_amd.evaluation.omni3d_eval import Omni3Deval
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    e = Omni3Deval([_ann(1, 0, [0, 0, 10, 10])], [_ann(1, 0, [0, 0, 10, 10], score=0.5)], "3D", matcher="device", stage3d="device")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.evaluate()


def test_nhd_call_checks_its_arguments_before_any_device_work():
    from ovmono3d_amd import lib
    L = lib.load()
    none = [None] * 7
    assert L.ovm_eval_nhd(None, None, 1, 4097, None, 0.5, *none, None) == -5    # OVM_ERR_CAPACITY: a cell holds at most 4096 boxes
    assert L.ovm_eval_nhd(None, None, 1, 4096, None, 0.5, *none, None) == -1
    assert L.ovm_eval_nhd(None, None, 0, 0, None, 0.5, *none, None) == 0
    assert L.ovm_eval_iou3d(None, None, 0, None, None, 1e-4, 1e-8, None, None) == 0
    assert L.ovm_eval_iou3d(None, None, 3, None, None, 1e-4, 1e-8, None, None) == -1


def test_entry_points_take_eval_3d():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.eval_ovmono3d_geo import argument_parser
    from tools.train_net import default_argument_parser
    assert default_argument_parser().parse_args(["--eval-only"]).eval_3d == "host"
    assert default_argument_parser().parse_args(["--eval-only", "--eval-3d", "device"]).eval_3d == "device"
    assert argument_parser().parse_args(["--predictions", "A=b.pth"]).eval_3d == "host"
    assert argument_parser().parse_args(["--predictions", "A=b.pth", "--eval-3d", "device"]).eval_3d == "device"
    with pytest.raises(SystemExit):
        default_argument_parser().parse_args(["--eval-3d", "gpu"])


def test_oracle_equals_brute_force_over_permutations():
    pairs = no.pair_set(seed=5)
    for pred, gt in pairs[::100][:10]:
        a, b = no.disentangled_nhd64(pred, gt), no.disentangled_nhd64(pred, gt, solver=no.brute_force)
        for k in no.KEYS:
            assert abs(a[k] - b[k]) <= 1e-13 * max(abs(b[k]), 1e-300), (k, a[k], b[k])


def test_subset_dp_equals_linear_sum_assignment():
    g = np.random.default_rng(11)
    for i in range(50):
        cost = g.random((8, 8)) * g.choice([1e-3, 1.0, 1e3])
        if i % 5 == 0:
            cost = np.round(cost * 4) / 4                                       # many ties
        rows, cols = linear_sum_assignment(cost)
        ref = cost[rows, cols].sum()
        assert abs(no.subset_dp(cost) - ref) <= 4e-16 * 8 * max(ref, cost.max()), i
    cost = g.random((8, 8))
    assert no.subset_dp(cost) == pytest.approx(no.brute_force(cost), rel=1e-15)


def test_host_path_error_against_the_oracle_is_a_usable_bound():
    """The bound of the GPU test is the host path's own error on the same pairs: it must exist and not be 0."""
    from ovmono3d_amd.evaluation import nhd
    pairs = no.pair_set()
    assert len(pairs) == 1000
    host = no.as_table([nhd.disentangled_nhd(p, g) for p, g in pairs])
    oracle = no.as_table([no.disentangled_nhd64(p, g) for p, g in pairs])
    e_abs, e_rel = no.error_against_oracle(host, oracle)
    print(f"host NHD against fp64: {e_abs:.3e} absolute, {e_rel:.3e} relative")
    assert np.isfinite(oracle).all() and np.isfinite(e_abs) and np.isfinite(e_rel)
    assert 0.0 < e_abs < 1e-2 and e_rel > 0.0
