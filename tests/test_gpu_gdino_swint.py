"""The GroundingDINO engine on the Swin-T record (window 7, C = 96 / 192 / 384 / 768, heads 3 / 6 / 12 / 24): against the Hugging Face
port on the CPU at token maps that are no multiples of 7, the 49-token window kernel with the qkv projection inside
(ovm_tune_set gdino_swin_fused) against the two-launch form with the launch counts, graph replay against eager, and ROIHeads3DGDINO
end to end from ``synthetic://gdino?arch=swint``. Helpers, taps and tolerances: test_gpu_gdino_engine.py's."""
from functools import lru_cache

import pytest
import torch

from common import assert_close, rel_err
from test_gpu_gdino_engine import MEAN, SMALL, STD, _engine, _normalised  # noqa: F401

pytestmark = pytest.mark.gpu

SWINT_SMALL = dict(SMALL, swin_embed=96, swin_depths=(2, 2, 2, 2), swin_heads=(3, 6, 12, 24), swin_window=7)
IDS = [101, 500, 1012, 600, 601, 1012, 700, 701, 702, 1012, 102]
HWS = ((264, 328), (300, 268))          # token maps 66 x 82 and 75 x 67; last stage 9 x 11 and 10 x 9: every stage larger than the window


@lru_cache(maxsize=None)
def _small_hf_swint():
    """test_gpu_gdino._small_hf_gdino itself (its BERT, transformer, seeds and perturbation), with the SwinConfig it builds turned into the
    Swin-T-shaped one: the helper takes no argument for the backbone, so the class it imports is wrapped while it runs."""
    from unittest import mock
    import transformers
    from test_gpu_gdino import _small_hf_gdino
    real = transformers.SwinConfig

    def swint_config(**kw):
        kw.update(image_size=224, embed_dim=96, num_heads=[3, 6, 12, 24], window_size=7)
        return real(**kw)
    with mock.patch.object(transformers, "SwinConfig", swint_config):
        hf, cfg = _small_hf_gdino()
    bb = cfg.backbone_config
    assert (bb.embed_dim, list(bb.depths), list(bb.num_heads), bb.window_size) == (96, [2, 2, 2, 2], [3, 6, 12, 24], 7)
    return hf


@lru_cache(maxsize=None)
def _image(hw, seed=2):
    return torch.randint(0, 256, (3,) + tuple(hw), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@lru_cache(maxsize=None)
def _hf_out(hw):
    """HF fp32 on the CPU, computed once per image size"""
    from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map
    hf = _small_hf_swint()
    ids = torch.tensor(IDS)
    x = _normalised(_image(hw))[None]
    torch.set_num_threads(min(8, torch.get_num_threads()))
    with torch.no_grad():
        out = hf(pixel_values=x, input_ids=ids[None], return_dict=True)
        stages = hf.model.backbone.conv_encoder.model(x).feature_maps
    pids = generate_masks_with_special_tokens_and_transfer_map(ids[None])[1][0].tolist()
    return out, [s[0].flatten(1).t().contiguous() for s in stages], pids


@pytest.mark.parametrize("hw", HWS)
def test_swint_engine_matches_hf_small(device, hw):
    """Whatever route the plan picks (by default the fused window kernel) must match HF. Measured: Swin stages 8.7e-07 .. 2.2e-06,
    encoder 4.7e-07 .. 1.7e-06, boxes 1.8e-07, logits 8.6e-07 .. 1.1e-06 against bounds of 1e-4 / 1e-4 / 2e-4 / 2e-4."""
    out, stages, pids = _hf_out(hw)
    eng = _engine(device, _small_hf_swint().state_dict(), SWINT_SMALL, use_graphs=False)
    img = _image(hw).to(device)
    eng.forward(img, IDS, pids)
    T, S = len(IDS), out.encoder_last_hidden_state_vision.shape[1]
    errs = {}
    for i, ref in enumerate(stages):
        got = eng.debug(f"swin_stage{i + 1}", tuple(ref.shape))
        errs[f"swin_stage{i + 1}"] = assert_close(got, ref, 1e-4, f"swin stage {i + 1} at {hw}")
    errs["enc_text"] = assert_close(eng.debug("enc_text", (T, 64)), out.encoder_last_hidden_state_text[0], 1e-4, "encoder text")
    errs["enc_vision"] = assert_close(eng.debug("enc_vision", (S, 64)), out.encoder_last_hidden_state_vision[0], 1e-4, "encoder vision")
    hf_topk = torch.topk(out.enc_outputs_class[0].max(-1)[0], 30)[1]
    assert sorted(eng.debug("topk", (30,), torch.int32).cpu().tolist()) == sorted(hf_topk.tolist())
    eng.set_force_topk(hf_topk)                                  # HF's order of the selected proposals for the decoder comparison
    logits, boxes = eng.forward(img, IDS, pids)
    assert torch.isinf(logits[:, T:]).all() and (logits[:, T:] < 0).all()
    errs["boxes"] = assert_close(boxes, out.pred_boxes[0], 2e-4, "pred_boxes")
    errs["logits"] = assert_close(logits[:, :T], out.logits[0][:, :T], 2e-4, "pred_logits")
    print(f"FIG swint engine vs HF {hw}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def _ab(device, sd, cfgk, hw, ids, seed):
    """one forward per setting of gdino_swin_fused (0, 1) on fresh engines -> [(logits, boxes)], [launches]"""
    from ovmono3d_amd import lib
    L = lib.load()
    img = torch.randint(0, 256, (3,) + hw, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(device)
    outs, launches = [], []
    try:
        for fused in (0, 1):
            assert L.ovm_tune_set(b"gdino_swin_fused", fused) == 0
            eng = _engine(device, sd, cfgk, use_graphs=False)
            logits, boxes = eng.forward(img, ids)
            outs.append((logits[:, :len(ids)].clone(), boxes.clone()))
            launches.append(eng.launches())
            del eng
    finally:
        L.ovm_tune_set(b"gdino_swin_fused", 1)
    return outs, launches


@pytest.mark.parametrize("size", ["small", "full"])
def test_swint_qkv_projection_inside_the_window_kernel(device, size):
    """swin7_qkv_attn_kernel against qkv GEMM + attn_f32_kernel (Tq = Tk = 49): one launch less per Swin block, boxes to 2e-5 and logits
    to 1e-4 of their largest magnitude (test_swin_qkv_projection_inside_the_window_kernel's bounds for the same A/B at window 12).
    Measured: small record boxes 6.0e-08 / logits 3.3e-07, launches 170 -> 162; full Swin-T record at 532 x 532 boxes 1.3e-06 /
    logits 2.6e-05, launches 372 -> 360."""
    if size == "small":
        sd, cfgk, hw, ids, blocks = _small_hf_swint().state_dict(), SWINT_SMALL, HWS[0], IDS, 8
    else:
        from ovmono3d_amd.gdino.config import GDinoConfig
        from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
        sd, cfgk, hw, blocks = synth_gdino_state_dict(3, GDinoConfig.swin_t()), dict(swin_embed=96, swin_depths=(2, 2, 6, 2),
                                                                                     swin_heads=(3, 6, 12, 24), swin_window=7), (532, 532), 12
        ids = [101, 2000 + 17, 1012, 2000 + 29, 2000 + 31, 1012, 2000 + 5, 1012, 102]
    outs, launches = _ab(device, sd, cfgk, hw, ids, 19)
    assert launches[1] == launches[0] - blocks, launches
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    print(f"FIG swint fused vs two launches ({size}): boxes {rel_err(outs[1][1], outs[0][1]):.3e} logits {rel_err(outs[1][0], outs[0][0]):.3e} "
          f"launches {launches}")
    assert_close(outs[1][1], outs[0][1], 2e-5, "pred_boxes (fused 7 x 7 window kernel vs two launches)")
    assert_close(outs[1][0], outs[0][0], 1e-4, "pred_logits (fused 7 x 7 window kernel vs two launches)")


def test_swint_graph_replay_equals_eager(device):
    sd = _small_hf_swint().state_dict()
    eager = _engine(device, sd, SWINT_SMALL, use_graphs=False)
    graphed = _engine(device, sd, SWINT_SMALL, use_graphs=True)
    g = torch.Generator().manual_seed(3)
    ids = [101, 500, 1012, 600, 601, 1012, 102]
    for i, (h, w) in enumerate([HWS[0], HWS[0], HWS[1], HWS[0], HWS[1]]):
        im = torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g).to(device)
        a_l, a_b = eager.forward(im, ids)
        b_l, b_b = graphed.forward(im, ids)
        assert torch.equal(a_b, b_b) and torch.equal(a_l, b_l), (i, h, w)


def test_swint_roi_heads_end_to_end_from_the_synthetic_url(device):
    """MODEL.AMD.GDINO_WEIGHTS synthetic://gdino?arch=swint&seed=3: load_detector builds the Swin-T network without being told the
    architecture; detections come back, and ovm_infer (one call) equals the staged path, as
    test_ovm_infer_one_call_equals_staged_path checks for Swin-B."""
    from common import build_cfg, synth_inputs
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.modeling import build_model
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    sd = synth_state_dict("vittest14", seed=3)
    outs, detector = [], None
    for fused in (True, False):
        cfg = build_cfg("vittest14", 280, "f16x3", max_batch=1, max_rois=1000, roi_heads="ROIHeads3DGDINO",   # 900 queries fit
                        extra=["MODEL.AMD.FUSED_INFER", fused, "MODEL.AMD.GDINO_WEIGHTS", "synthetic://gdino?arch=swint&seed=3"])
        model = build_model(cfg, device=device)
        model.load_state_dict(sd)
        if detector is None:
            model.roi_heads.load_detector()
            detector = model.roi_heads.detector
            assert detector.engine.cfg == GDinoConfig.swin_t()
        else:
            model.roi_heads.detector = detector                  # same weights: packed once
        res = []
        for seed in (5, 6):
            inp = synth_inputs(1, hw=((210, 280),), oracle2d=False, seed=seed)
            inp[0]["category_list"] = ["chair", "dining table", "sofa"]
            inp[0]["image"] = inp[0]["image"].to(device)
            res.append(model(inp)[0]["instances"])
        outs.append(res)
    for a, b in zip(*outs):
        assert len(a) == len(b) and len(a) >= 1
        assert torch.equal(a.pred_classes.cpu(), b.pred_classes.cpu())
        for f in ("scores", "pred_bbox3D", "pred_center_cam", "pred_dimensions", "pred_pose"):
            assert torch.equal(a.get(f), b.get(f)), f
        assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
