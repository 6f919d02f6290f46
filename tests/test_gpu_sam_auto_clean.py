"""GPU: the small-region clean-up of the automatic mask generator (SamAutomaticMaskGenerator.postprocess_small_regions and the
``min_mask_region_area`` keyword of generate_device / generate / generate_rle) against tests/mask_cc_oracle.py. On the synthetic
vit_test SAM the oracle is applied to the output of the call without the keyword, so SAM's numerics do not enter: every field is
compared for equality."""
import numpy as np
import pytest
import torch

import mask_cc_oracle as O
import sam_oracle as so
from ovmono3d_amd import masks as M
from ovmono3d_amd.sam import SamAutomaticMaskGenerator

pytestmark = pytest.mark.gpu

H, W = 96, 128
# random weights give large, ragged masks whose boxes nearly coincide: thresholds that keep several of them (tests/
# test_gpu_demo_geo_everything.py's), and the one area that cleans some and leaves others - single stray pixels; from 8 on every mask changes
GRID, PRED_IOU, STABILITY, NMS = 3, 0.25, 0.0, 1.0
AREA = 2
FIELDS = ("masks", "boxes", "scores", "stability", "points", "areas", "index")


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_equal(got, ref, tag):
    assert sorted(got) == sorted(FIELDS), tag
    for k in FIELDS:
        g = got[k].cpu().numpy()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape and np.array_equal(g, ref[k]), (tag, k)


def _dict(masks, scores, device):
    """generate_device's dict for hand-made planes"""
    boxes, areas = zip(*(O.tight_box(m) for m in masks))
    n = len(masks)
    host = dict(masks=np.stack(masks).astype(np.uint8), boxes=np.stack(boxes).astype(np.float32), scores=np.asarray(scores, np.float32),
                stability=np.linspace(0.9, 1.0, n).astype(np.float32), points=np.arange(2 * n, dtype=np.float32).reshape(n, 2),
                areas=np.asarray(areas, np.int32), index=3 * np.arange(n, dtype=np.int64) + 1)
    return host, {k: torch.from_numpy(v).to(device) for k, v in host.items()}


def test_hand_made_planes(device):
    Hh, Ww = 40, 70
    a = np.zeros((Hh, Ww), np.uint8)
    a[5:25, 6:40] = 1
    b = a.copy()
    b[33, 66] = 1                                                        # the same mask with a speck far away: another box until it is cleaned
    c = np.zeros((Hh, Ww), np.uint8)
    c[28:38, 2:20] = 1
    e = c.copy()
    e[30:33, 5:8] = 0                                                    # c with a hole: filled, then box-equal to c
    f = np.zeros((Hh, Ww), np.uint8)
    f[1:4, 60:69] = 1
    f[20, 50] = 1                                                        # a changed mask nothing overlaps: kept, after the unchanged ones
    host, dev = _dict([b, a, e, c, f], [0.99, 0.5, 0.98, 0.6, 0.7], device)
    ref = O.postprocess_small_regions(host, 10, 0.7)
    assert ref["index"].tolist() == [4, 10, 13] and ref["changed"].tolist() == [False, False, True]                # a, c, then cleaned f
    got = SamAutomaticMaskGenerator.postprocess_small_regions(dev, 10, 0.7)
    _assert_equal(got, ref, "hand-made")
    assert got["boxes"][2].tolist() == [60.0, 1.0, 69.0, 4.0] and int(got["areas"][2]) == 27                         # the cleaned mask's own
    assert host["boxes"][4].tolist() == [50.0, 1.0, 69.0, 21.0] and int(host["areas"][4]) == 28
    # a threshold nothing is below: everything is unchanged and NMS works on the boxes as they were (b and a differ, e and c coincide)
    ref1 = O.postprocess_small_regions(host, 1, 0.7)
    assert ref1["index"].tolist() == [1, 4, 7, 13] and not ref1["changed"].any()
    _assert_equal(SamAutomaticMaskGenerator.postprocess_small_regions(dev, 1, 0.7), ref1, "threshold 1")
    empty = {k: v[:0] for k, v in dev.items()}
    got0 = SamAutomaticMaskGenerator.postprocess_small_regions(empty, 10, 0.7)
    assert all(tuple(got0[k].shape) == tuple(empty[k].shape) for k in FIELDS)


@pytest.fixture(scope="module")
def generator(device):
    from ovmono3d_amd.sam import build_sam
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    pred = build_sam("vit_test", synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), device=device, image_size=128)
    return SamAutomaticMaskGenerator(pred, points_per_side=GRID, pred_iou_thresh=PRED_IOU, stability_score_thresh=STABILITY, box_nms_thresh=NMS)


@pytest.fixture(scope="module")
def image(device):
    return torch.from_numpy(so.test_image(H, W, seed=20)).to(device)


@pytest.fixture(scope="module")
def plain(generator, image):
    """The call without the keyword, and the oracle's clean-up of its output"""
    out = generator.generate_device(image, "BGR")
    return out, O.postprocess_small_regions(_host(out), AREA, NMS)


def test_generate_device_with_the_keyword_equals_the_oracle_on_the_plain_output(generator, image, plain):
    out, ref = plain
    flags = [O.remove_small_regions(p, AREA, "both")[1] for p in out["masks"].cpu().numpy()]
    print(f"{len(flags)} masks, changed at area {AREA}: {[int(f) for f in flags]}; kept {ref['index'].tolist()}, of them changed {ref['changed'].tolist()}")
    assert any(flags) and not all(flags)                                 # the input exercises both branches: a cleaned mask and an untouched one
    got = generator.generate_device(image, "BGR", min_mask_region_area=AREA)
    _assert_equal(got, ref, "generate_device")
    assert len(ref["masks"]) == len(flags) and ref["changed"].tolist() == sorted(ref["changed"].tolist())      # nothing dropped at 1.0; unchanged first
    # the method itself at a threshold that matters: the masks' boxes nearly coincide, so the second NMS drops most of them
    ref7 = O.postprocess_small_regions(_host(out), AREA, 0.7)
    assert 1 <= len(ref7["masks"]) < len(flags)
    _assert_equal(SamAutomaticMaskGenerator.postprocess_small_regions(out, AREA, 0.7), ref7, "nms 0.7")
    # the keyword at 0 is the call without it
    zero = generator.generate_device(image, "BGR", min_mask_region_area=0)
    assert sorted(zero) == sorted(out) and all(torch.equal(zero[k], out[k]) for k in out)


def test_records_carry_the_cleaned_masks_with_their_areas_and_boxes(generator, image, plain, device):
    _, ref = plain
    recs = generator.generate(image, "BGR", min_mask_region_area=AREA)
    rles = generator.generate_rle(image, "BGR", min_mask_region_area=AREA)
    assert len(recs) == len(rles) == len(ref["masks"]) >= 2
    dec = M.decode_rle([r["segmentation"] for r in rles], device).cpu().numpy()
    for j, (r, q) in enumerate(zip(recs, rles)):
        plane = ref["masks"][j]
        assert r["segmentation"].dtype == torch.bool and np.array_equal(r["segmentation"].cpu().numpy(), plane != 0)
        assert np.array_equal(dec[j], plane)
        ys, xs = np.nonzero(plane)
        want_box = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())] if len(ys) else [0, 0, 0, 0]
        assert r["area"] == int(plane.sum()) == M.rle_area(q["segmentation"]) and r["bbox"] == want_box
        assert {k: v for k, v in q.items() if k != "segmentation"} == {k: v for k, v in r.items() if k != "segmentation"}
        assert r["predicted_iou"] == float(ref["scores"][j]) and r["stability_score"] == float(ref["stability"][j])
        assert r["point_coords"] == [[float(ref["points"][j][0]), float(ref["points"][j][1])]] and r["crop_box"] == [0, 0, W, H]
    # and without the keyword the records are the candidate table's, as before
    base = generator.generate(image, "BGR")
    assert [b["area"] for b in base] == generator.generate_device(image, "BGR")["areas"].cpu().tolist()
