"""The GroundingDINO architecture record comes from the checkpoint: ``GDinoConfig.from_state_dict`` on Swin-B and Swin-T shaped state
dicts (native names and upstream names through ``convert_upstream_state_dict``), its refusals, the ``synthetic://gdino?arch=`` URL,
the Swin-T synthetic weights against the Hugging Face port's parameter tree, and the ABI size of the window-kernel descriptor."""
import ctypes as C
from functools import lru_cache

import pytest
import torch

from ovmono3d_amd.gdino.config import GDinoConfig
from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict

SW = "model.backbone.conv_encoder.model.swin."
BERT_TINY = dict(bert_hidden=768, bert_layers=1, bert_ffn=64, vocab=200, bert_positions=16)     # hidden 768: bert_heads = 12, as the records say


@lru_cache(maxsize=None)
def _sd(arch: str):
    cfg = GDinoConfig.swin_t() if arch == "swint" else GDinoConfig()
    return cfg, synth_gdino_state_dict(1, cfg, **BERT_TINY)


@pytest.mark.parametrize("arch", ["swinb", "swint"])
def test_from_state_dict_recovers_the_record(arch):
    cfg, sd = _sd(arch)
    got = GDinoConfig.from_state_dict(sd)
    assert got == cfg, (got, cfg)
    if arch == "swint":
        assert (got.swin_embed, tuple(got.swin_depths), tuple(got.swin_heads), got.swin_window) == (96, (2, 2, 6, 2), (3, 6, 12, 24), 7)


def test_from_state_dict_reads_the_transformer_fields():
    small = GDinoConfig.swin_t(d_model=64, enc_layers=2, dec_layers=3, heads=4, ffn_dim=128, num_queries=30, swin_depths=(2, 2, 2, 2), n_levels=3)
    sd = synth_gdino_state_dict(2, small, **BERT_TINY)
    assert GDinoConfig.from_state_dict(sd) == small


def test_from_state_dict_after_converting_upstream_names():
    """convert_upstream_state_dict needs no change for Swin-T: an upstream-named copy of the Swin-T dict (inverse rules of
    test_gdino_convert.py, DDP prefix included) converts back to every tensor, and the record read off it is Swin-T's."""
    from test_gdino_convert import _to_upstream
    from ovmono3d_amd.gdino.detector import convert_upstream_state_dict
    cfg, sd = _sd("swint")
    up = _to_upstream(sd)
    assert "module.backbone.0.layers.2.blocks.5.attn.qkv.weight" in up and tuple(up["module.backbone.0.layers.0.blocks.0.attn.qkv.weight"].shape) == (288, 96)
    back = convert_upstream_state_dict(up)
    assert GDinoConfig.from_state_dict(back) == cfg
    skip = ("model.decoder.bbox_embed.", SW + "layernorm.")        # aliases of bbox_embed.* / a norm upstream does not have
    for k, v in sd.items():
        if not k.startswith(skip):
            assert k in back and torch.equal(back[k], v), k


def test_bias_table_whose_rows_are_no_odd_square_is_refused_by_name():
    _, sd = _sd("swint")
    key = SW + "encoder.layers.1.blocks.1.attention.relative_position_bias.relative_position_bias_table"
    bad = dict(sd)
    bad[key] = torch.zeros(170, 6)
    with pytest.raises(ValueError, match="layers.1.blocks.1.*relative_position_bias_table"):
        GDinoConfig.from_state_dict(bad)
    bad[key] = torch.zeros(196, 6)                                  # a square, but of an even side: no (2 w - 1)^2 either
    with pytest.raises(ValueError, match="layers.1.blocks.1.*relative_position_bias_table"):
        GDinoConfig.from_state_dict(bad)


def test_three_swin_stages_are_refused():
    """the engine's record and neck are built for four stages: fewer must not get as far as the library"""
    _, sd = _sd("swint")
    bad = {k: v for k, v in sd.items() if SW + "encoder.layers.3." not in k}
    with pytest.raises(ValueError, match="3 Swin stages"):
        GDinoConfig.from_state_dict(bad)


def test_head_dimension_24_is_refused_by_name():
    _, sd = _sd("swint")
    bad = dict(sd)
    for j in range(2):                                              # stage 0: 96 channels over 4 heads
        bad[SW + f"encoder.layers.0.blocks.{j}.attention.relative_position_bias.relative_position_bias_table"] = torch.zeros(169, 4)
    with pytest.raises(ValueError, match="layers.0.blocks.0.*relative_position_bias_table.*24"):
        GDinoConfig.from_state_dict(bad)


def test_synthetic_url_selects_the_architecture():
    from ovmono3d_amd.gdino.detector import synthetic_spec
    cfg, seed = synthetic_spec("synthetic://gdino?arch=swint&seed=1")
    assert cfg == GDinoConfig.swin_t() and seed == 1
    assert synthetic_spec("synthetic://gdino?seed=4") == (GDinoConfig(), 4)
    assert synthetic_spec("synthetic://gdino?arch=swinb") == (GDinoConfig(), 0)
    assert synthetic_spec("synthetic://gdino") == (GDinoConfig(), 0)
    with pytest.raises(ValueError, match="arch"):
        synthetic_spec("synthetic://gdino?arch=swinl")
    sd = synth_gdino_state_dict(seed, cfg, **BERT_TINY)
    assert tuple(sd[SW + "embeddings.patch_embeddings.projection.weight"].shape) == (96, 3, 4, 4)
    assert tuple(sd[SW + "encoder.layers.3.blocks.1.attention.relative_position_bias.relative_position_bias_table"].shape) == (169, 24)
    assert tuple(sd["model.input_proj_vision.0.0.weight"].shape) == (256, 192, 1, 1)
    assert SW + "encoder.layers.2.blocks.5.mlp.fc1.weight" in sd and SW + "encoder.layers.2.blocks.6.mlp.fc1.weight" not in sd
    # without arch: today's tensors, element for element
    a = synth_gdino_state_dict(synthetic_spec("synthetic://gdino?seed=4")[1], synthetic_spec("synthetic://gdino?seed=4")[0], **BERT_TINY)
    b = synth_gdino_state_dict(4, **BERT_TINY)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # ... and those are the tensors of before the arch parameter existed: two sums recorded from that code (seed 4, this BERT)
    assert float(b["model.level_embed"].double().sum()) == pytest.approx(16.63060193043202, rel=1e-12)
    assert float(b[SW + "encoder.layers.2.blocks.17.mlp.fc2.weight"].double().abs().sum()) == pytest.approx(23336.62149530596, rel=1e-12)


def test_roi_head_builds_what_the_url_names(monkeypatch):
    """load_detector hands the URL's record to the synthetic weights and no record to the detector: the checkpoint decides."""
    from ovmono3d_amd.gdino import detector as det
    from ovmono3d_amd.modeling.roi_heads.roi_heads_gdino import ROIHeads3DGDINO
    from ovmono3d_amd.util import synth_gdino_weights as sw
    seen = {}

    class Fake:
        def __init__(self, device, sd, tok, mean, std, cfg=None, **kw):
            seen.update(cfg=cfg, sd=sd)
    monkeypatch.setattr(det, "NativeGroundingDino", Fake)
    monkeypatch.setattr(sw, "synth_gdino_state_dict", lambda seed=0, cfg=GDinoConfig(): {"seed": seed, "cfg": cfg})
    from ovmono3d_amd.config import get_cfg, get_cfg_defaults
    cfg = get_cfg_defaults(get_cfg())
    cfg.MODEL.AMD.GDINO_WEIGHTS = "synthetic://gdino?arch=swint&seed=3"
    head = ROIHeads3DGDINO.__new__(ROIHeads3DGDINO)
    head._gdino_cfg = cfg
    head.engine = type("E", (), {"device": torch.device("cpu")})()
    head.load_detector()
    assert seen["cfg"] is None and seen["sd"] == {"seed": 3, "cfg": GDinoConfig.swin_t()}


def test_swint_synthetic_weights_load_strictly_into_the_hf_port():
    transformers = pytest.importorskip("transformers")
    from transformers import BertConfig, GroundingDinoConfig, GroundingDinoForObjectDetection, SwinConfig
    cfg, sd = _sd("swint")
    bb = SwinConfig(image_size=224, patch_size=4, embed_dim=cfg.swin_embed, depths=list(cfg.swin_depths), num_heads=list(cfg.swin_heads),
                    window_size=cfg.swin_window, out_indices=[2, 3, 4], layer_norm_eps=1e-5)
    tc = BertConfig(vocab_size=BERT_TINY["vocab"], hidden_size=BERT_TINY["bert_hidden"], num_hidden_layers=BERT_TINY["bert_layers"],
                    num_attention_heads=cfg.bert_heads, intermediate_size=BERT_TINY["bert_ffn"],
                    max_position_embeddings=BERT_TINY["bert_positions"], attn_implementation="eager")
    hc = GroundingDinoConfig(backbone_config=bb, text_config=tc, d_model=cfg.d_model, encoder_layers=cfg.enc_layers, decoder_layers=cfg.dec_layers,
                             encoder_attention_heads=cfg.heads, decoder_attention_heads=cfg.heads, encoder_ffn_dim=cfg.ffn_dim,
                             decoder_ffn_dim=cfg.ffn_dim, num_queries=cfg.num_queries, num_feature_levels=cfg.n_levels, max_text_len=cfg.max_text_len,
                             positional_embedding_temperature=20, two_stage=True, embedding_init_target=True, decoder_bbox_embed_share=True,
                             disable_custom_kernels=True, attn_implementation="eager")
    with torch.device("meta"):
        model = GroundingDinoForObjectDetection(hc)
    want = {k: tuple(v.shape) for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    got = {k: tuple(v.shape) for k, v in sd.items()}
    assert got == want
    missing, unexpected = model.load_state_dict(sd, strict=False, assign=True)
    assert not unexpected and all(not model.state_dict()[k].dtype.is_floating_point for k in missing), (missing[:5], unexpected[:5])


def test_abi_size_of_the_window_kernel_descriptor():
    from ovmono3d_amd import lib
    L = lib.load()
    assert L.ovm_abi_sizeof(b"OvmSwinQkvAttnOp") == C.sizeof(lib.OvmSwinQkvAttnOp) == 8 * 8 + 10 * 4
