"""The float64 3D IoU oracle (oracle/box3d.py) is the reference of tests/test_gpu_box3d_iou.py: it must not depend on
where a pair sits, it must give the closed forms at any distance, and a box without volume must intersect nothing."""
import numpy as np
import pytest

import box3d_cases as bc
from oracle import box3d as ob


def test_oracle_is_translation_invariant_on_the_sweep():
    """Every row of the sweep (5 pairs a row), moved 10, 50 and 100 m in float64: the IoU changes by less than 1e-9."""
    for dist, size, rot, dt, gt in bc.sweep_rows():
        base = np.array([ob.iou_matrix(d[None], g[None])[0, 0] for d, g in zip(dt[:5], gt[:5])])
        assert ((base > 0.05) & (base < 0.95)).sum() >= 3, (dist, size, rot)
        for s in (10.0, 50.0, 100.0):
            off = np.array([0.3 * s, -0.1 * s, s])
            moved = np.array([ob.iou_matrix((d + off)[None], (g + off)[None])[0, 0] for d, g in zip(dt[:5], gt[:5])])
            assert np.abs(moved - base).max() < 1e-9, (dist, size, rot, s, np.abs(moved - base).max())


@pytest.mark.parametrize("dist", [3.0, 80.0])
def test_oracle_closed_forms_far_from_the_camera(dist):
    for name, a, b, want in bc.closed_forms(dist):
        got = ob.iou_matrix(a[None], b[None])[0, 0]
        assert abs(got - want) < 2e-5, (name, got, want)


def test_oracle_degenerate_boxes_have_no_volume_and_intersect_nothing():
    dt = bc.detections_around(20, seed=3)
    for name, g in bc.degenerate_gt():
        assert ob.box_volume(g) == 0.0, name
        assert all(ob.intersection_volume(d, g) == 0.0 for d in dt), name
        assert all(ob.intersection_volume(g, d) == 0.0 for d in dt), name
        assert (ob.iou_matrix(dt, g[None]) == 0.0).all(), name
        assert (ob.iou_matrix(g[None], g[None]) == 0.0).all(), name            # empty union
    assert ob.box_volume(np.full((8, 3), np.nan)) == 0.0


def test_sweep_cases_are_rounded_to_fp32_and_gated_by_size():
    dist, size, rot, dt, gt = bc.sweep_rows(distances=(100.0,))[0]
    assert np.array_equal(dt, dt.astype(np.float32).astype(np.float64))
    assert size == "3-10cm" and bc.gate(dt[0], gt[0]) == 2.5e-4
    big = bc.sweep_rows(distances=(100.0,))[4]
    assert big[1] == "1-3m" and bc.gate(big[3][0], big[4][0]) == 2e-5
