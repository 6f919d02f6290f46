"""The checkpoint keys a broken checkpoint is reported by, for every family of the ViT tower's key table (csrc/tower.hip) through every
owner: the detection backbone (ovm_create), the SAM predictor's image encoder and Depth Pro's three encoders.

The oracle tests prove that the keys which are present are read; these pin the spelling on the error path: one key is taken out of a
tiny state dict, the create call must return OVM_ERR_MISSING_WEIGHT (-3), and the handle's error text must be exactly today's, the
owner's prefix ("image encoder: ", ...) included. A create call that fails on a missing key returns before any kernel is launched.
"""
import functools

import pytest
import torch

import depthpro_oracle as do
import sam_oracle as so
from common import build_cfg, build_clip_cfg, build_mae_cfg, build_midas_cfg, build_sam_cfg
from ovmono3d_amd.lib import OvmError

pytestmark = pytest.mark.gpu

# model name -> (config builder, key prefix, patch-embed weight, second MLP linear of block {l})
BACKBONES = {
    "vittest14": (build_cfg, "backbone.net.vit.", "patch_embed.proj.weight", "blocks.{l}.mlp.fc2.weight"),
    "vittest14_reg": (build_cfg, "backbone.net.vit.", "patch_embed.proj.weight", "blocks.{l}.mlp.fc2.bias"),
    "vitgtest14": (build_cfg, "backbone.net.vit.", "patch_embed.proj.weight", "blocks.{l}.mlp.w3.weight"),
    "ViT-test-16": (build_clip_cfg, "backbone.net.visual.", "conv1.weight", "transformer.resblocks.{l}.mlp.c_proj.weight"),
    "test/vit-mae-test": (build_mae_cfg, "backbone.net.vit.", "embeddings.patch_embeddings.projection.weight", "encoder.layer.{l}.output.dense.weight"),
    "DPT_test": (build_midas_cfg, "backbone.net.vit.", "patch_embed.proj.weight", "blocks.{l}.mlp.fc2.weight"),
    "vit_test": (build_sam_cfg, "backbone.net.vit.", "patch_embed.proj.weight", "blocks.{l}.mlp.lin2.bias"),
}
# Depth Pro: key prefix of each encoder -> the name ovm_depthpro_create reports it by
DEPTHPRO_ENCODERS = {
    "depth_pro.encoder.patch_encoder.model.": "patch encoder",
    "depth_pro.encoder.image_encoder.model.": "image encoder",
    "fov_model.fov_encoder.model.": "field-of-view encoder",
}


@functools.lru_cache(maxsize=None)
def _backbone(name):
    """(config, state dict) of one tiny detection model, built once; the tests take keys out of a shallow copy."""
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    cfg = BACKBONES[name][0](name, max_batch=1)
    return cfg, synth_state_dict(name, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=2)


@functools.lru_cache(maxsize=None)
def _sam_sd():
    return so.case_inputs(so.TINY)[0]


@functools.lru_cache(maxsize=None)
def _depthpro_sd():
    return do.case_inputs(do.TINY)[0]


def _without(sd, key):
    assert key in sd, f"the synthetic checkpoint has no {key}"
    out = dict(sd)
    del out[key]
    return out


def _backbone_error(name, sd, device):
    from ovmono3d_amd.native import Engine
    with pytest.raises(OvmError) as e:
        Engine(_backbone(name)[0], device).load_state_dict(sd)
    return str(e.value)


def _sam_error(sd, device):
    from ovmono3d_amd.sam import build_sam
    with pytest.raises(OvmError) as e:
        build_sam(so.TINY["arch"], sd, device=device, image_size=so.TINY["image_size"])
    return str(e.value)


def _depthpro_error(sd, device):
    from ovmono3d_amd.depthpro import build_depthpro
    with pytest.raises(OvmError) as e:
        build_depthpro(sd, device=device, precision=3, config=do.TINY["config"])
    return str(e.value)


@pytest.mark.parametrize("which", ["mlp", "patch_embed"])
@pytest.mark.parametrize("name", list(BACKBONES))
def test_backbone_missing_key(device, name, which):
    from ovmono3d_amd.native import config_to_native
    cfg, sd = _backbone(name)
    _, prefix, pe, mlp = BACKBONES[name]
    last = config_to_native(cfg).depth - 1                 # the last block the tower runs (MAE: one fewer than the checkpoint holds)
    key = prefix + (pe if which == "patch_embed" else mlp.format(l=last))
    assert _backbone_error(name, _without(sd, key), device) == f"ovm_create failed (-3): missing weight: {key}"


@pytest.mark.parametrize("which", ["mlp", "patch_embed"])
def test_sam_predictor_missing_key(device, which):
    from ovmono3d_amd.util.synth_weights import SAM_ARCH
    last = SAM_ARCH[so.TINY["arch"]][1] - 1
    key = "image_encoder." + ("patch_embed.proj.weight" if which == "patch_embed" else f"blocks.{last}.mlp.lin2.weight")
    assert _sam_error(_without(_sam_sd(), key), device) == f"ovm_sam_create failed with code -3: image encoder: missing weight: {key}"


@pytest.mark.parametrize("which", ["mlp", "patch_embed"])
@pytest.mark.parametrize("prefix", list(DEPTHPRO_ENCODERS))
def test_depthpro_missing_key(device, prefix, which):
    last = do.TINY["config"]["depth"] - 1
    key = prefix + ("embeddings.patch_embeddings.projection.weight" if which == "patch_embed" else f"encoder.layer.{last}.mlp.fc2.weight")
    assert _depthpro_error(_without(_depthpro_sd(), key), device) == \
        f"ovm_depthpro_create failed with code -3: {DEPTHPRO_ENCODERS[prefix]}: missing weight: {key}"


def test_sam_relative_position_table_with_a_wrong_second_dimension(device):
    """segment_anything's attn.rel_pos_h is [2 s - 1][head_dim = 64]: another width is refused by name, through both owners."""
    key = "backbone.net.vit.blocks.0.attn.rel_pos_h"
    sd = dict(_backbone("vit_test")[1])
    sd[key] = torch.zeros(sd[key].shape[0], 32)
    assert _backbone_error("vit_test", sd, device) == f"ovm_create failed (-3): missing or mis-shaped weight: {key}"
    key = "image_encoder.blocks.1.attn.rel_pos_h"
    sd = dict(_sam_sd())
    sd[key] = torch.zeros(sd[key].shape[0], 32)
    assert _sam_error(sd, device) == f"ovm_sam_create failed with code -3: image encoder: missing or mis-shaped weight: {key}"
