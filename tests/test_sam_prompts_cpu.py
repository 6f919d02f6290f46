"""SAM's point, box + point and mask-input prompts, checks that need no GPU: the condition of every mask the GPU tests threshold (on
the reference alone), the token order and padding rule of the restatement against Hugging Face's prompt encoder, the mask-embedding
restatement against HF's, the argument refusals of ``ovmono3d_amd.sam`` and of demo/demo_geo.py, and the tool's grouping rule."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sam_oracle as so
import sam_prompt_oracle as po
from common import ROOT
from roi_glue_ref import F32, F64


@pytest.fixture(scope="module")
def refs():
    return po.reference_set()


@pytest.fixture(scope="module")
def portrait_refs():
    return po.reference_set(so.PORTRAIT, tuple(po.PORTRAIT_CASES))


def _condition(name, r64, r32, hw):
    band = 4.0 * float((r32["low"].double() - r64["low"]).abs().max())
    shares = so.band_share(r64["logits"], band)
    n, _, _, _, _ = po.case_shape(po.CASES[name])
    K = 3 if po.CASES[name].get("multimask", True) else 1
    print(f"{name}: band {band:.3e}, largest share inside {max(shares):.4%}, logit std {float(r64['logits'].std()):.2f}")
    assert len(shares) == n * K and tuple(r64["logits"].shape) == (n, K) + tuple(hw)
    assert max(shares) <= 0.01, shares
    for plane in r64["logits"].reshape(-1, hw[0] * hw[1]):
        assert 0.01 < float((plane > 0).double().mean()) < 0.99


@pytest.mark.parametrize("name", po.TINY_CASES)
def test_masks_of_the_prompt_cases_are_well_conditioned(refs, name):
    """tests/test_sam_cpu.py's condition check for every new case: band = 4 x |HF fp32 - fp64| of the low-res logits; at most 1 % of
    any thresholded mask inside it and pixels on both sides in every plane. Measured: 0.01 - 0.03 %."""
    r64, r32, _ = refs[0][name]
    _condition(name, r64, r32, so.TINY["hw"])


def test_masks_of_the_portrait_prompt_case_are_well_conditioned(portrait_refs):
    H, W = so.PORTRAIT["hw"]
    assert (so.PORTRAIT["max_boxes"] * H * W) % 4 == 2 and po.case_shape(po.CASES["portrait_points1"])[0] > so.PORTRAIT["max_boxes"]
    r64, r32, _ = portrait_refs[0]["portrait_points1"]
    _condition("portrait_points1", r64, r32, (H, W))


def test_mask_input_is_live(refs):
    """Feeding plane 2 back moves the logits by far more than any tolerance: the synthetic mask_downscaling weights are not inert."""
    a, b = refs[0]["box"][0]["low"], refs[0]["box_mask"][0]["low"]
    assert float((a - b).abs().max()) > 10.0


def _prompt_weights(sd):
    P = "prompt_encoder."
    pe = torch.cat([sd[P + f"point_embeddings.{i}.weight"] for i in range(4)]).numpy()
    out = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]]).numpy()
    return dict(out_tokens=out, gauss=sd[P + "pe_layer.positional_encoding_gaussian_matrix"].numpy(), point_emb=pe[:2], corner=pe[2:],
                not_a_point=sd[P + "not_a_point_embed.weight"].numpy()[0])


@pytest.mark.parametrize("name", ("points1", "points3", "box_points2", "box", "box_points8"))
def test_token_order_and_padding_of_the_restatement_match_hf(refs, name):
    """sparse rows = points, then ONE padding row without a box, or the two corners with one; label -1 rows are not_a_point_embed. The
    fp64 restatement against HF's prompt_encoder in fp64: a swapped row or a wrong padding rule is an error of order 1."""
    allrefs, sd, img = refs
    case, (r64, _, _) = po.CASES[name], allrefs[name]
    H, W = img.shape[:2]
    nh, nw = so.preprocess_shape(H, W, so.TINY["image_size"])
    n, P, hb, ns, nt = po.case_shape(case)
    tok, sparse = po.point_tokens(case.get("points"), case.get("labels"), case.get("boxes"), H=H, W=W, newh=nh, neww=nw, S=so.TINY["image_size"],
                                  dtype=F64, **_prompt_weights(sd))
    assert sparse.shape == (n, ns, 256) and tok.shape == (n, nt, 256)
    assert np.abs(sparse - r64["sparse"].numpy()).max() < 1e-12
    assert np.array_equal(tok[:, 5:], sparse) and np.array_equal(tok[0, :5], _prompt_weights(sd)["out_tokens"].astype(F64))
    if not hb:
        assert np.array_equal(sparse[:, -1], np.broadcast_to(_prompt_weights(sd)["not_a_point"].astype(F64), (n, 256)))
    for b, labs in enumerate(case.get("labels", [])):
        for p, l in enumerate(labs):
            assert (l == -1) == bool(np.array_equal(sparse[b, p], _prompt_weights(sd)["not_a_point"].astype(F64)))


def test_mask_embedding_restatement_matches_hf(refs):
    allrefs, sd, _ = refs
    r64, r32, mk = allrefs["box_mask"]
    w = po.mask_weights(sd)
    got = po.mask_embed(mk, w, F64).reshape(r64["dense"].shape)
    assert np.abs(got - r64["dense"].numpy()).max() < 1e-12 * float(r64["dense"].abs().max())
    assert np.abs(po.mask_embed(mk, w, F32).reshape(r64["dense"].shape) - r64["dense"].numpy()).max() < 1e-4


def test_mask_boxes_restatement():
    m = np.zeros((3, 5, 7), np.uint8)
    m[1, 2, 3] = 1
    m[2, 1:4, 2] = 1
    m[2, 3, 2:6] = 7
    boxes, counts = po.mask_boxes(m)
    assert boxes.tolist() == [[0, 0, 0, 0], [3, 2, 4, 3], [2, 1, 6, 4]] and counts.tolist() == [0, 1, 6]


# ---- refusals, before any device work ----------------------------------------------------------------------------------------------
def test_check_prompts_refuses_without_device_work():
    from ovmono3d_amd.sam import MAX_POINTS, check_prompts
    assert MAX_POINTS == 8
    n, P, c, l, b = check_prompts(np.zeros((2, 8, 2)), np.ones((2, 8)), [[0, 0, 5, 5], [1, 1, 2, 2]], None)
    assert (n, P) == (2, 8) and c.dtype == np.float32 and l.dtype == np.int32 and b.shape == (2, 4)
    with pytest.raises(ValueError, match="at most 8 points"):
        check_prompts(np.zeros((1, 9, 2)), np.ones((1, 9)))
    with pytest.raises(ValueError, match="labels must be 1"):
        check_prompts(np.zeros((1, 2, 2)), [[1, 2]])
    with pytest.raises(ValueError, match="needs points or a box"):
        check_prompts()
    with pytest.raises(ValueError, match="needs points or a box"):
        check_prompts(np.zeros((1, 0, 2)), np.zeros((1, 0)))
    with pytest.raises(ValueError, match="come together"):
        check_prompts(np.zeros((1, 1, 2)), None)
    with pytest.raises(ValueError, match="boxes for"):
        check_prompts(np.zeros((2, 1, 2)), np.ones((2, 1)), [[0, 0, 1, 1]])
    with pytest.raises(ValueError, match="mask_inputs"):
        check_prompts(None, None, [[0, 0, 1, 1]], np.zeros((1, 16, 32)), 32)


class _NoEngine:
    """A predictor whose engine must not be reached."""
    grid, dev = 8, torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}")


def test_predict_refusals_come_before_the_engine():
    from ovmono3d_amd.sam import SamPredictor
    p = SamPredictor(_NoEngine())
    p.original_size = (70, 100)
    with pytest.raises(ValueError):
        p.predict()                                                           # no prompt at all
    with pytest.raises(ValueError):
        p.predict(mask_input=np.zeros((1, 32, 32), np.float32))               # a mask input is no prompt
    with pytest.raises(NotImplementedError):
        p.predict(box=[0, 0, 5, 5], return_logits=True)
    with pytest.raises(ValueError, match="at most 8"):
        p.predict(point_coords=np.zeros((9, 2)), point_labels=np.ones(9))
    with pytest.raises(ValueError, match="labels must be"):
        p.predict(point_coords=np.zeros((1, 2)), point_labels=[2])
    with pytest.raises(ValueError):
        p.predict_prompts()
    with pytest.raises(ValueError, match="mask_index"):
        p.predict_prompts(boxes=[[0, 0, 5, 5]], mask_index=3)


def test_library_refuses_bad_prompt_shapes_without_a_handle():
    import ctypes as C
    from ovmono3d_amd import lib
    L = lib.load()
    n = C.c_int64()
    assert L.ovm_sam_predict_workspace(None, 1, 1, 0, 0, C.byref(n)) == -1
    assert L.ovm_sam_predict(None, None, None, 1, None, None, 1, 1, 2, None, None, None, None, 0, None) == -1
    assert L.ovm_sam_mask_boxes(None, 1, 0, 5, None, None, None) == -1
    assert L.ovm_sam_mask_boxes(None, 0, 4, 5, None, None, None) == 0         # no masks: nothing to do


@pytest.mark.parametrize("extra,msg", [(["--mask", "box"], "needs --mask sam"), (["--boxes-file", "b.json", "--sam-weights", "w"], "give one"),
                                       (["--sam-weights", "w", "--sam-refine", "-1"], "--sam-refine")])
def test_points_file_refusals_of_demo_geo(extra, msg):
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--input-folder", "none", "--points-file", "p.json", "--depth", "files",
           "--depth-dir", "d", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, r.stderr[-600:]


def test_points_file_grouping_rule():
    from ovmono3d_amd.geo import sources as g
    entries = [{"points": [[1, 2]], "labels": [1]},
               {"points": [[1, 2], [3, 4]], "labels": [1, 0]},
               {"points": [[5, 6]], "labels": [1], "bbox": [0, 0, 9, 9]},
               {"points": [[7, 8]], "labels": [0]},
               {"points": [[1, 1], [2, 2]], "labels": [1, 1]}]
    groups = g.group_point_prompts(entries)
    assert groups == {(1, False): [0, 3], (2, False): [1, 4], (1, True): [2]} == po.group_reference(entries)
    assert list(groups) == [(1, False), (2, False), (1, True)]                 # first appearance
    assert sorted(i for idx in groups.values() for i in idx) == list(range(len(entries)))
    for (P, _), idx in groups.items():                                         # nobody is padded: each prompt keeps its own point count
        assert all(len(entries[i]["points"]) == P for i in idx)
    with pytest.raises(SystemExit):
        g.group_point_prompts([{"points": [[1, 2]], "labels": [1, 0]}])
