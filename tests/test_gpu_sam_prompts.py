"""SAM's point, box + point and mask-input prompts and its single-mask output on the device (ovm_sam_predict, csrc/sam.hip) against
Hugging Face SamModel in fp64 on the CPU, in the per-prompt batch form (tests/sam_prompt_oracle.py), on TINY's image and weights.

The rules are tests/test_gpu_sam.py's, none chosen here: every float stage (sparse embeddings, dense embedding, decoder tokens,
low-res logits, IoU) within 4 x the error of the SAME HF model in fp32 against its fp64 run on the same inputs, measured in the test
(scale-relative, tests/common.py rel_err); one-pass fp16 (precision 1) within DESIGN.md section 2's 5e-2; masks exact on every pixel
whose fp64 logit lies outside +- band (band = 4 x the fp32 run's largest absolute low-res error), at most 1 % of a mask inside.
The dense embedding without a mask input is no_mask_embed in every cell: HF's fp32 error is 0 and so is the bound. The dense
embedding the device keeps is the last prompt's.

Cases (sam_prompt_oracle.CASES): one click (foreground, on the image border, background); three clicks with labels 1 / 0 / -1 (nine
tokens: the 16-token attention kernel); a box with two clicks; a box with eight clicks (15 tokens); a box refined with its previous
logits; a click refined with its previous logits; the single-mask output. PORTRAIT (99 x 71, max_boxes = 2) runs three click prompts
as two chunks, the second chunk's masks at byte 2 * 99 * 71 = 2 (mod 4).

Measured on an MI355X (HF fp32 vs fp64 | HIP precision 3 vs fp64), the case closest to its bound in each stage:

    sparse embeddings    box_mask          9.71e-07 | 9.80e-07
    dense embedding      points1_mask      3.65e-07 | 3.04e-07      (0 | 0 without a mask input)
    decoder tokens       portrait_points1  6.22e-07 | 1.70e-06
    low-res logits       portrait_points1  2.00e-06 | 4.30e-06
    IoU predictions      points3           9.69e-07 | 2.84e-06

Precision 1: at most 6.7e-04 (tokens), 1.6e-03 (logits), 1.1e-03 (IoU). Masks: bands 1.0e-3 .. 1.4e-3, no disagreement, at most
0.029 % of a mask left out.
"""
import numpy as np
import pytest
import torch

import sam_oracle as so
import sam_prompt_oracle as po
from common import rel_err

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FAST_BAND = 5e-2
MAX_LEFT_OUT = 0.01
STAGES = (("sparse", "sparse embeddings"), ("dense", "dense embedding"), ("tokens", "decoder tokens"), ("low", "low-res logits"), ("iou", "IoU predictions"))
C = 256


@pytest.fixture(scope="module")
def refs():
    return po.reference_set()


@pytest.fixture(scope="module")
def portrait_refs():
    return po.reference_set(so.PORTRAIT, tuple(po.PORTRAIT_CASES))


def _predictor(base, sd, img, device, precision=3, max_boxes=16):
    from ovmono3d_amd.sam import build_sam
    pred = build_sam(base["arch"], sd, device=device, image_size=base["image_size"], precision=precision, max_boxes=max_boxes)
    pred.set_image(torch.from_numpy(img).to(device), "RGB")
    return pred


def _prompts(case, mk, sl=slice(None)):
    a = lambda k, dt: None if k not in case else np.asarray(case[k], dt)[sl]          # noqa: E731
    return dict(point_coords=a("points", np.float32), point_labels=a("labels", np.int32), boxes=a("boxes", np.float32),
                mask_inputs=None if mk is None else torch.from_numpy(mk[sl]), multimask_output=case.get("multimask", True))


def _hip_stages(pred, base, case, mk, mask_index, rows=None):
    """rows: how many prompts the last chunk held (default: all of them)."""
    n, P, hb, ns, nt = po.case_shape(case)
    rows = n if rows is None else rows
    G = base["image_size"] // 16
    masks, iou, low = pred.predict_prompts(mask_index=mask_index, want_iou=True, want_lowres=True, **_prompts(case, mk))
    eng = pred.engine
    out = {"sparse": eng.debug("sparse", (rows, ns, C)), "dense": eng.debug("dense", (G, G, C)), "tokens": eng.debug("tokens_out", (rows, nt, C)),
           "low": low, "iou": iou, "masks": masks}
    torch.cuda.synchronize()
    return out


def _tail(r, rows):
    return {k: (v[-rows:] if k in ("sparse", "tokens") else v[-1] if k == "dense" else v) for k, v in r.items()}


def _check_floats(hip, r64, r32, label, bound=None):
    rows, bad = [], []
    for key, name in STAGES:
        assert tuple(hip[key].shape) == tuple(r64[key].shape), (key, tuple(hip[key].shape), tuple(r64[key].shape))
        e32, e = so.fp32_error(r64, r32, key), rel_err(hip[key], r64[key])
        tol = bound if bound is not None else FACTOR * e32
        rows.append(f"{label} {name:20s} HF fp32 {e32:.2e} | HIP {e:.2e} | bound {tol:.2e}")
        if not e <= tol:
            bad.append(rows[-1])
    print("\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)


def _check_masks(masks_u8, logits64_plane, band, label):
    got = masks_u8.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    got, ref, worst = got.astype(bool), logits64_plane.numpy(), 0.0
    for i in range(ref.shape[0]):
        decided = np.abs(ref[i]) > band
        left_out = 1.0 - decided.mean()
        worst = max(worst, left_out)
        assert left_out <= MAX_LEFT_OUT, f"{label} prompt {i}: {left_out:.3%} of the pixels lie inside the band {band:.2e}"
        wrong = int(((got[i] != (ref[i] > 0)) & decided).sum())
        assert wrong == 0, f"{label} prompt {i}: {wrong} pixels outside the band disagree"
    print(f"{label}: band {band:.3e}, at most {worst:.4%} of a mask left out, no disagreement")


@pytest.mark.parametrize("name", po.GPU_CASES)
def test_prompt_case_stages_and_masks_match_fp64(device, refs, name):
    allrefs, sd, img = refs
    case, (r64, r32, mk) = po.CASES[name], allrefs[name]
    K = 3 if case.get("multimask", True) else 1
    n = po.case_shape(case)[0]
    pred = _predictor(so.TINY, sd, img, device)
    hip = _hip_stages(pred, so.TINY, case, mk, K - 1)
    _check_floats(hip, _tail(r64, n), _tail(r32, n), f"{name} p3")
    band = FACTOR * float((r32["low"].double() - r64["low"]).abs().max())
    H, W = so.TINY["hw"]
    for k in range(K):
        masks = hip["masks"] if k == K - 1 else pred.predict_prompts(mask_index=k, **_prompts(case, mk))[0]
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (n, H, W)
        _check_masks(masks, r64["logits"][:, k], band, f"{name} plane {k}")


@pytest.mark.parametrize("name", ("points3", "box_mask"))
def test_prompt_case_one_pass_fp16(device, refs, name):
    allrefs, sd, img = refs
    case, (r64, r32, mk) = po.CASES[name], allrefs[name]
    n = po.case_shape(case)[0]
    hip = _hip_stages(_predictor(so.TINY, sd, img, device, precision=1), so.TINY, case, mk, 2)
    _check_floats(hip, _tail(r64, n), _tail(r32, n), f"{name} p1", bound=FAST_BAND)


def test_portrait_clicks_in_chunks_second_chunk_off_a_word(device, portrait_refs):
    allrefs, sd, img = portrait_refs
    name = "portrait_points1"
    case, (r64, r32, _) = po.CASES[name], allrefs[name]
    H, W = so.PORTRAIT["hw"]
    n, mb = po.case_shape(case)[0], so.PORTRAIT["max_boxes"]
    assert (mb * H * W) % 4 == 2 and n > mb
    last = n % mb or mb
    pred = _predictor(so.PORTRAIT, sd, img, device, max_boxes=mb)
    hip = _hip_stages(pred, so.PORTRAIT, case, None, 2, rows=last)
    _check_floats(hip, _tail(r64, last), _tail(r32, last), f"{name} p3")
    band = FACTOR * float((r32["low"].double() - r64["low"]).abs().max())
    _check_masks(hip["masks"], r64["logits"][:, 2], band, f"{name} plane 2")


def test_box_alone_through_predict_is_predict_boxes_bit_for_bit(device, refs):
    """ovm_sam_predict with no points, a box, no mask input and multimask outputs takes the launches of ovm_sam_predict_boxes."""
    _, sd, img = refs
    pred = _predictor(so.TINY, sd, img, device)
    boxes = torch.tensor(so.TINY["boxes"], dtype=torch.float32, device=device)
    H, W = so.TINY["hw"]
    for k in range(3):
        a = pred.engine.predict_boxes(boxes, H, W, k, want_iou=True, want_lowres=True)
        b = pred.engine.predict_prompts(None, None, boxes, None, H, W, multimask=True, mask_index=k, want_iou=True, want_lowres=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert torch.equal(pred.engine.predict_boxes(boxes, H, W, k)[0], pred.engine.predict_prompts(None, None, boxes, None, H, W, mask_index=k)[0])
    m, i, l = pred.predict(box=so.TINY["boxes"][0])
    assert torch.equal(m[2].to(torch.uint8), a[0][0]) and torch.equal(i, a[1][0]) and torch.equal(l, a[2][0])


@pytest.mark.parametrize("name", ("points3", "points1_mask", "points3_single"))
def test_two_calls_give_equal_bytes_and_chunks_equal_single_prompts(device, refs, name):
    allrefs, sd, img = refs
    case, (_, _, mk) = po.CASES[name], allrefs[name]
    n = po.case_shape(case)[0]
    mi = 2 if case.get("multimask", True) else 0
    pred = _predictor(so.TINY, sd, img, device)
    a = pred.predict_prompts(mask_index=mi, want_iou=True, want_lowres=True, **_prompts(case, mk))
    b = pred.predict_prompts(mask_index=mi, want_iou=True, want_lowres=True, **_prompts(case, mk))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # one prompt per decoder pass (max_boxes = 1: n chunks), and n calls of one prompt
    one = _predictor(so.TINY, sd, img, device, max_boxes=1)
    c = one.predict_prompts(mask_index=mi, want_iou=True, want_lowres=True, **_prompts(case, mk))
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    for i in range(n):
        d = pred.predict_prompts(mask_index=mi, want_iou=True, want_lowres=True, **_prompts(case, mk, slice(i, i + 1)))
        for x, y in zip(a, d):
            assert torch.equal(x[i:i + 1], y)


def test_predict_keeps_segment_anythings_shapes(device, refs):
    allrefs, sd, img = refs
    pred = _predictor(so.TINY, sd, img, device)
    H, W = so.TINY["hw"]
    L = 4 * (so.TINY["image_size"] // 16)
    case, (r64, r32, _) = po.CASES["points3"], allrefs["points3"]
    m, i, l = pred.predict(point_coords=np.asarray(case["points"][0]), point_labels=np.asarray(case["labels"][0]))
    assert m.dtype == torch.bool and tuple(m.shape) == (3, H, W) and tuple(i.shape) == (3,) and tuple(l.shape) == (3, L, L)
    full = pred.predict_prompts(case["points"], case["labels"], mask_index=1)[0]
    assert torch.equal(m[1].to(torch.uint8), full[0])
    m1, i1, l1 = pred.predict(point_coords=np.asarray(case["points"][0]), point_labels=np.asarray(case["labels"][0]), mask_input=l[2:3],
                              multimask_output=False)
    assert tuple(m1.shape) == (1, H, W) and tuple(i1.shape) == (1,) and tuple(l1.shape) == (1, L, L)
    with pytest.raises(ValueError):
        pred.predict()
    with pytest.raises(NotImplementedError):
        pred.predict(box=so.TINY["boxes"][0], return_logits=True)
    # the library's own refusals: nine points, and a mask_index without a plane
    eng = pred.engine
    pts, lab = torch.zeros((1, 9, 2), device=device), torch.ones((1, 9), dtype=torch.int32, device=device)
    with pytest.raises(Exception, match="at most 8 points"):
        eng.predict_prompts(pts, lab, None, None, H, W, workspace=torch.empty(1 << 20, dtype=torch.uint8, device=device))
    with pytest.raises(Exception, match="mask_index"):
        eng.predict_prompts(pts[:, :1], lab[:, :1], None, None, H, W, multimask=False, mask_index=1)
