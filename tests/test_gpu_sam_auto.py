"""SAM's automatic mask generation end to end (ovmono3d_amd.sam.SamAutomaticMaskGenerator: ovm_sam_auto_candidates, ovm_sam_auto_select,
then the predictor's own planes) on vit_test at image size 128: so.TINY (70 x 100, a 6 x 6 grid) and so.PORTRAIT (99 x 71,
max_boxes = 2, a 5 x 5 grid: chunks, and masks at odd byte offsets).

The candidate table against Hugging Face SamModel in fp64 on the grid's points (sam_prompt_oracle.run), the fp32 run of the same model
as the yardstick: the IoU predictions within 4 x the fp32 run's error (scale-relative, as tests/test_gpu_sam_prompts.py); the three
counts inside count64(v > t + band) .. count64(v > t - band) for t in {+1, 0, -1}, band = 4 x the fp32 run's largest low-res error, at
most 1 % of a plane within the band of a threshold; the stability equal to float32(cnt_hi) / float32(cnt_lo) of the device's own
counts, bit for bit.

The selection is exact: generate() equals tests/sam_auto_oracle.select applied to the device's own table, so no float tolerance
enters a discrete decision. Random weights give near-whole-image masks: the settings cover one surviving mask and more than ten.
Every emitted plane is predict_prompts' for its point and plane, byte for byte; area, bbox, crop_box and point_coords follow the
rules; two calls and points_per_batch 1, 7, 64 give equal results.

Measured on an MI355X (tiny | portrait): IoU predictions HF fp32 1.9e-06 | 1.3e-06 against HIP 3.4e-06 | 1.8e-06; bands 1.44e-03 |
1.56e-03 with at most 0.043 % | 0.071 % of a plane within the band of a threshold; IoU predictions span -2.3 .. 3.3, stability
0.54 .. 0.98; kept masks from 1 (box_nms_thresh 0.7, every setting) to 108 | 75 (no filter, box_nms_thresh 1.0).
"""
import numpy as np
import pytest
import torch

from ovmono3d_amd.sam import SamAutomaticMaskGenerator  # noqa: F401  (the feature under test: without it this module does not load)
import sam_auto_oracle as ao
import sam_oracle as so
import sam_prompt_oracle as po
from common import rel_err
from sam_auto_oracle import F32

pytestmark = pytest.mark.gpu

FACTOR = 4.0
CASES = {"tiny": (so.TINY, 6), "portrait": (so.PORTRAIT, 5)}
SETTINGS = [(p, s, n) for p in (0.25, 0.0) for s in (0.85, 0.0) for n in (0.7, 0.95, 1.0)]


@pytest.fixture(scope="module", params=list(CASES))
def setup(request, device):
    """The case, its grid, the fp64 and fp32 HF runs on the grid's points, and one predictor; built once per case"""
    from ovmono3d_amd.sam import build_sam
    base, n = CASES[request.param]
    sd, img = so.case_inputs(base)
    H, W = base["hw"]
    pts = ao.grid_points(n, H, W)
    case = dict(points=pts.reshape(-1, 1, 2).tolist(), labels=[[1]] * len(pts))
    m64 = so.build_model(base["arch"], sd, base["image_size"], torch.float64)
    r64 = po.run(m64, img, case)
    del m64
    r32 = po.run(so.build_model(base["arch"], sd, base["image_size"], torch.float32), img, case)
    pred = build_sam(base["arch"], sd, device=device, image_size=base["image_size"], max_boxes=base.get("max_boxes", 16))
    return dict(name=request.param, base=base, n=n, img=torch.from_numpy(img).to(device), pts=pts, r64=r64, r32=r32, pred=pred)


def _gen(s, pthr=0.88, sthr=0.95, nthr=0.7, batch=64):
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator
    return SamAutomaticMaskGenerator(s["pred"], points_per_side=s["n"], points_per_batch=batch, pred_iou_thresh=pthr, stability_score_thresh=sthr,
                                     box_nms_thresh=nthr)


def test_candidate_table_against_fp64(setup):
    s = setup
    gen = _gen(s, pthr=0.0, sthr=0.0)                                          # pred_iou_thresh <= 0: every row is counted
    gen.generate(s["img"])
    f, pts = gen.candidates()
    r64, r32 = s["r64"], s["r32"]
    H, W = s["base"]["hw"]
    m = 3 * len(s["pts"])
    assert np.array_equal(pts, s["pts"]) and len(f["iou"]) == m and not f["flags"].any()
    e32, e = so.fp32_error(r64, r32, "iou"), rel_err(torch.from_numpy(f["iou"].reshape(-1, 3)), r64["iou"])
    print(f"\n{s['name']} IoU predictions: HF fp32 {e32:.2e} | HIP {e:.2e} | bound {FACTOR * e32:.2e}; span {f['iou'].min():.2f} .. {f['iou'].max():.2f}")
    assert e <= FACTOR * e32
    band = FACTOR * float((r32["low"].double() - r64["low"]).abs().max())
    v64 = r64["logits"].reshape(m, H, W).numpy()
    worst = 0.0
    for i in range(m):
        worst = max(worst, ao.check_counts((f["cnt_hi"][i], f["area"][i], f["cnt_lo"][i]), v64[i], band, tag=f"{s['name']} candidate {i}"))
        _, mid, _, box = ao.plane_stats(v64[i])
        assert abs(int(f["area"][i]) - mid) <= H * W * ao.MAX_LEFT_OUT and 0 <= f["box"][i][0] <= f["box"][i][2] < W and 0 <= f["box"][i][1] <= f["box"][i][3] < H
    st = ao.stability(f["cnt_hi"], f["cnt_lo"])
    assert np.array_equal(f["stability"].view(np.uint32), st.view(np.uint32))
    print(f"{s['name']}: band {band:.2e}, at most {worst:.4%} of a plane within it of a threshold; stability {np.nanmin(st):.2f} .. {np.nanmax(st):.2f}; "
          f"areas {f['area'].min()} .. {f['area'].max()} of {H * W}")


def test_filter_one_skips_on_the_device_and_the_counted_rows_do_not_change(setup):
    s = setup
    full = _gen(s, pthr=0.0, sthr=0.0)
    full.generate(s["img"])
    f0, _ = full.candidates()
    part = _gen(s, pthr=0.25, sthr=0.0)
    part.generate(s["img"])
    f1, _ = part.candidates()
    skipped = ~(f0["iou"] > F32(0.25))
    assert 0 < skipped.sum() < len(skipped) and np.array_equal((f1["flags"] & ao.SKIPPED) != 0, skipped)
    assert np.array_equal(f0["iou"].view(np.uint32), f1["iou"].view(np.uint32))
    for k in ("area", "box", "cnt_hi", "cnt_lo"):
        assert np.array_equal(f1[k][~skipped], f0[k][~skipped]) and not f1[k][skipped].any()
    assert np.array_equal(f1["stability"][~skipped].view(np.uint32), f0["stability"][~skipped].view(np.uint32)) and not f1["stability"][skipped].any()


def test_selection_equals_the_restatement_on_the_devices_own_table(setup):
    s = setup
    counts = {}
    for pthr, sthr, nthr in SETTINGS:
        gen = _gen(s, pthr, sthr, nthr)
        recs = gen.generate(s["img"])
        f, pts = gen.candidates()
        ref = ao.select(f, pthr, sthr, nthr)
        got = gen.generate_device(s["img"])["index"].cpu().numpy()
        assert got.tolist() == ref.tolist() and len(recs) == len(ref), (pthr, sthr, nthr)
        for r, c in zip(recs, ref):
            assert r["predicted_iou"] == float(f["iou"][c]) and r["point_coords"] == [[float(pts[c // 3][0]), float(pts[c // 3][1])]]
        counts[(pthr, sthr, nthr)] = len(ref)
    print(f"\n{s['name']} kept masks per (pred_iou_thresh, stability_score_thresh, box_nms_thresh): {counts}")
    assert max(counts.values()) > 10 and 1 in counts.values()
    assert counts[(0.25, 0.85, 0.7)] <= counts[(0.25, 0.85, 0.95)] <= counts[(0.25, 0.85, 1.0)]


def _by_plane(pred, pts, cands, H, W):
    """predict_prompts' planes for candidates `cands` (3 * point + plane), one call per plane"""
    out = torch.zeros((len(cands), H, W), dtype=torch.uint8, device=pred.engine.dev)
    for k in range(3):
        rows = [i for i, c in enumerate(cands) if c % 3 == k]
        if rows:
            coords = np.asarray([pts[cands[i] // 3] for i in rows], np.float32).reshape(-1, 1, 2)
            out[rows] = pred.predict_prompts(coords, np.ones((len(rows), 1), np.int32), mask_index=k)[0]
    return out


def test_emitted_masks_are_the_predictors_and_records_follow_the_rules(setup):
    s = setup
    H, W = s["base"]["hw"]
    gen = _gen(s, 0.0, 0.0, 1.0)                                               # every candidate is kept: all three planes of every point
    recs = gen.generate(s["img"])
    f, pts = gen.candidates()
    dev = gen.generate_device(s["img"])
    cands = dev["index"].cpu().numpy().tolist()
    assert len(recs) == 3 * len(pts) and sorted(cands) == list(range(3 * len(pts)))
    own = _by_plane(s["pred"], pts, cands, H, W)
    assert torch.equal(dev["masks"], own)
    tight, counts = po.mask_boxes(own.cpu().numpy())
    assert np.array_equal(dev["boxes"].cpu().numpy(), tight) and np.array_equal(dev["areas"].cpu().numpy(), counts)
    assert np.array_equal(dev["scores"].cpu().numpy().view(np.uint32), f["iou"][cands].view(np.uint32))
    assert np.array_equal(dev["stability"].cpu().numpy().view(np.uint32), f["stability"][cands].view(np.uint32))
    assert np.array_equal(dev["points"].cpu().numpy(), pts[np.asarray(cands) // 3])
    for i, (r, c) in enumerate(zip(recs, cands)):
        seg = r["segmentation"]
        assert seg.dtype == torch.bool and tuple(seg.shape) == (H, W) and torch.equal(seg, own[i].bool())
        assert r["area"] == int(counts[i]) == int(f["area"][c])
        x0, y0, x1, y1 = (int(v) for v in tight[i])
        assert r["bbox"] == ([x0, y0, x1 - 1 - x0, y1 - 1 - y0] if counts[i] else [0, 0, 0, 0])
        assert r["crop_box"] == [0, 0, W, H] and r["stability_score"] == float(f["stability"][c])
        assert set(r) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x["segmentation"], y["segmentation"]) and {k: v for k, v in x.items() if k != "segmentation"} == {k: v for k, v in y.items() if k != "segmentation"}


def test_two_calls_and_every_batch_size_give_equal_results(setup):
    s = setup
    for pthr, sthr, nthr in ((0.25, 0.85, 0.95), (0.0, 0.0, 0.7)):
        gen = _gen(s, pthr, sthr, nthr)
        a = gen.generate(s["img"])
        ta = gen._cands.clone()
        _same(a, gen.generate(s["img"]))
        assert torch.equal(ta, gen._cands)
        for batch in (1, 7, 64):
            g2 = _gen(s, pthr, sthr, nthr, batch=batch)
            _same(a, g2.generate(s["img"]))
            assert torch.equal(ta, g2._cands)
