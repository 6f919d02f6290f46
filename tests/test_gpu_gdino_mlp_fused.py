"""The fused MLP route of the detector's Swin blocks (ovm_tune_set gdino_mlp_fused; csrc/mlp_fused.hip) through the engine, against
today's two GEMMs per MLP on the same weights and image.

A reduced detector - the SMALL pattern of test_gpu_gdino_engine.py with swin_embed = 64, so the four stages have C = 64 .. 512 and
hidden layers of 256 .. 2048 (one to eight chunks of 256) - on a 120 x 168 image: 1260 / 315 / 88 / 24 tokens per stage, none of
stages 2-4 a multiple of the 64-row tile. Same operands and the same three-pass products; what differs is where the k-sum of the
second layer is cut into partial sums (chunks of 256 against the GEMM's split-K slices, or none), so the outputs agree to the bounds
the project uses for the same kind of A/B (test_swin_qkv_projection_inside_the_window_kernel): boxes 2e-5, logits 1e-4 of their
largest magnitude. The launch count (op wrappers, as the engine counts them) drops by one per fused site.
"""
import pytest
import torch

from common import assert_close
from test_gpu_gdino_engine import SMALL, _engine

pytestmark = pytest.mark.gpu

SMALL64 = dict(SMALL, swin_embed=64, swin_heads=(2, 4, 8, 16))
HW = (120, 168)
IDS = [101, 500, 1012, 600, 601, 1012, 102]


def _state_dict():
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    return synth_gdino_state_dict(5, GDinoConfig(**SMALL64), bert_hidden=64, bert_layers=2, bert_ffn=128, vocab=2000)


def test_fused_mlp_route_matches_two_gemms_and_replays_bit_for_bit(device):
    from ovmono3d_amd import lib
    L = lib.load()
    sd = _state_dict()
    img = torch.randint(0, 256, (3,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(23)).to(device)
    outs, launches, sites = [], [], []
    try:
        for knob in (0, 1):
            assert L.ovm_tune_set(b"gdino_mlp_fused", knob) == 0
            eng = _engine(device, sd, SMALL64, use_graphs=False)
            logits, boxes = eng.forward(img, IDS)
            outs.append((logits[:, :len(IDS)].clone(), boxes.clone()))
            launches.append(eng.launches())
            sites.append(eng.debug_scalar("mlp_fused_sites"))
            del eng
        # second pass with graphs on, knob on: the first call runs eagerly and captures, the second replays
        graphed = _engine(device, sd, SMALL64, use_graphs=True)
        first = [t.clone() for t in graphed.forward(img, IDS)]
        replay = [t.clone() for t in graphed.forward(img, IDS)]
        g_sites = graphed.debug_scalar("mlp_fused_sites")
        del graphed
    finally:
        L.ovm_tune_set(b"gdino_mlp_fused", 1)
    print(f"FIG gdino mlp fused: launches {launches[0]} -> {launches[1]}, fused sites {sites}")
    assert sites[0] == 0 and sites[1] == sum(SMALL64["swin_depths"]), sites        # every Swin block of the four stages
    assert launches[1] == launches[0] - sites[1], (launches, sites)
    assert g_sites == sites[1]
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    d_box = float((outs[0][1] - outs[1][1]).abs().max()); d_log = float((outs[0][0] - outs[1][0]).abs().max())
    print(f"FIG gdino mlp fused vs two GEMMs: max |d boxes| {d_box:.3e}, max |d logits| {d_log:.3e} "
          f"(max |logits| {float(outs[0][0].abs().max()):.3e})")
    assert_close(outs[1][1], outs[0][1], 2e-5, "pred_boxes (fused MLP vs two GEMMs)")
    assert_close(outs[1][0], outs[0][0], 1e-4, "pred_logits (fused MLP vs two GEMMs)")
    assert torch.equal(first[1], outs[1][1]) and torch.equal(first[0][:, :len(IDS)], outs[1][0]), "graph engine's eager pass differs"
    assert torch.equal(replay[0], first[0]) and torch.equal(replay[1], first[1]), "graph replay differs from the eager pass"


def test_encoder_ffn_on_the_fused_route(device):
    """gdino_mlp_fused = 2 adds the encoder's FFN (ReLU, EPI_STORE with the residual R) where the kernel takes its shape: the same
    reduced detector with ffn_dim = 256 (one chunk), d_model = 64. Against knob 1 on the same weights: one op launch less per encoder
    layer, outputs within the bounds of the test above."""
    from ovmono3d_amd import lib
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    L = lib.load()
    cfgk = dict(SMALL64, ffn_dim=256)
    sd = synth_gdino_state_dict(7, GDinoConfig(**cfgk), bert_hidden=64, bert_layers=2, bert_ffn=128, vocab=2000)
    img = torch.randint(0, 256, (3,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(29)).to(device)
    outs, launches, sites = [], [], []
    try:
        for knob in (1, 2):
            assert L.ovm_tune_set(b"gdino_mlp_fused", knob) == 0
            eng = _engine(device, sd, cfgk, use_graphs=False)
            logits, boxes = eng.forward(img, IDS)
            outs.append((logits[:, :len(IDS)].clone(), boxes.clone()))
            launches.append(eng.launches())
            sites.append(eng.debug_scalar("mlp_fused_sites"))
            del eng
    finally:
        L.ovm_tune_set(b"gdino_mlp_fused", 1)
    print(f"FIG gdino mlp fused, encoder: launches {launches[0]} -> {launches[1]}, fused sites {sites}")
    assert sites[1] == sites[0] + cfgk["enc_layers"], sites
    assert launches[1] == launches[0] - cfgk["enc_layers"], (launches, sites)
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    assert_close(outs[1][1], outs[0][1], 2e-5, "pred_boxes (encoder FFN fused vs two GEMMs)")
    assert_close(outs[1][0], outs[0][0], 1e-4, "pred_logits (encoder FFN fused vs two GEMMs)")
