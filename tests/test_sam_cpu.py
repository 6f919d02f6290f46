"""SAM predictor, checks that need no GPU: the synthetic checkpoint is a segment_anything checkpoint (it loads strictly into Hugging
Face's SamModel through tests/sam_oracle.py's key map), the product package stays free of ``transformers``, vit_h is refused with the
head-dimension message, the ABI mirror of OvmSamConfig, and the condition of the masks the GPU tests threshold."""
import ctypes as C
import subprocess
import sys

import pytest
import torch

from common import ROOT

import sam_oracle as so


@pytest.mark.parametrize("arch,image_size", [("vit_test", 128), ("vit_b", 1024), ("vit_l", 1024)])
def test_synthetic_checkpoint_loads_strictly_into_hf_sam(arch, image_size):
    from transformers import SamModel
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    sd = synth_sam_predictor_state_dict(arch, seed=1, image_size=image_size)
    with torch.device("meta"):
        model = SamModel(so.hf_config(arch, image_size))
    hf = so.convert_state_dict(sd)
    want = dict(model.state_dict())
    # HF stores the shared positional matrix twice; segment_anything once
    assert set(want) - set(hf) == {so.TIED[0]}, sorted(set(want) - set(hf))
    assert not set(hf) - set(want), sorted(set(hf) - set(want))
    for k, v in hf.items():
        assert tuple(v.shape) == tuple(want[k].shape), (k, tuple(v.shape), tuple(want[k].shape))
    if arch == "vit_test":                                     # and an actual strict load where it is cheap
        hf[so.TIED[0]] = hf[so.TIED[1]]
        SamModel(so.hf_config(arch, image_size)).load_state_dict(hf, strict=True)


def test_key_map_examples():
    assert so.sa_to_hf("image_encoder.blocks.3.norm2.bias") == "vision_encoder.layers.3.layer_norm2.bias"
    assert so.sa_to_hf("image_encoder.neck.2.weight") == "vision_encoder.neck.conv2.weight"
    assert so.sa_to_hf("mask_decoder.output_hypernetworks_mlps.2.layers.1.weight") == "mask_decoder.output_hypernetworks_mlps.2.layers.0.weight"
    assert so.sa_to_hf("mask_decoder.iou_prediction_head.layers.2.bias") == "mask_decoder.iou_prediction_head.proj_out.bias"
    assert so.sa_to_hf("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix") == "shared_image_embedding.positional_embedding"


def test_package_does_not_import_transformers():
    code = "import sys; import ovmono3d_amd.sam, ovmono3d_amd.util.synth_sam_weights; assert 'transformers' not in sys.modules, 'transformers imported'"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_vit_h_is_refused_with_the_head_dim_message():
    from ovmono3d_amd import lib
    from ovmono3d_amd.sam import build_sam
    with pytest.raises(lib.OvmError) as e:
        build_sam("vit_h", None)
    msg = str(e.value)
    assert "code -6" in msg and "head dimension 80" in msg and "64" in msg, msg
    with pytest.raises(ValueError):
        build_sam("vit_x", None)


def test_abi_size_of_sam_config():
    from ovmono3d_amd import lib
    L = lib.load()
    assert L.ovm_abi_sizeof(b"OvmSamConfig") == C.sizeof(lib.OvmSamConfig) == 4 * 24
    c = lib.OvmSamConfig()
    c.embed_dim, c.heads = 256, 4                              # everything else zero: refused before any device call
    h = C.c_void_p()
    assert L.ovm_sam_create(C.byref(c), None, 0, 0, C.byref(h)) == -1
    assert b"invalid config" in L.ovm_sam_last_error(h)
    L.ovm_sam_destroy(h)
    assert L.ovm_sam_last_error(None) == b"null handle"


def test_sam_config_tables():
    from ovmono3d_amd.sam import sam_config
    b, l = sam_config("vit_b"), sam_config("vit_l")
    assert (b.embed_dim, b.depth, b.heads, b.global_mask) == (768, 12, 12, sum(1 << i for i in (2, 5, 8, 11)))
    assert (l.embed_dim, l.depth, l.heads, l.global_mask) == (1024, 24, 16, sum(1 << i for i in (5, 11, 17, 23)))
    assert b.image_size == l.image_size == 1024 and b.pos_grid == 64 and l.embed_dim == l.heads * 64


def test_masks_of_the_tiny_case_are_well_conditioned():
    """The condition check of the mask comparison, on the reference alone: the band is 4 x the absolute error of HF's own fp32 run of
    the low-resolution logits against its fp64 run (the tolerance of the float stages); for every mask the GPU test thresholds, at
    most 1 % of the output pixels may have an fp64 logit inside it. A failure means the synthetic weights need fixing, not the cap."""
    r64, r32, _, _ = so.reference_pair(so.TINY)
    band = 4.0 * float((r32["low"].double() - r64["low"]).abs().max())
    shares = so.band_share(r64["logits"], band)
    print(f"tiny case: band {band:.3e}, largest share inside {max(shares):.4%}, logit std {float(r64['logits'].std()):.2f}")
    assert len(shares) == len(so.TINY["boxes"]) * 3
    assert max(shares) <= 0.01, shares
    # and the masks are not degenerate: each plane has pixels on both sides
    for plane in r64["logits"].reshape(-1, r64["logits"].shape[-2] * r64["logits"].shape[-1]):
        assert 0.01 < float((plane > 0).double().mean()) < 0.99


def test_masks_of_the_portrait_case_are_well_conditioned():
    """The same check for the portrait case (99 x 71, three boxes in chunks of two)."""
    r64, r32, _, _ = so.reference_pair(so.PORTRAIT)
    band = 4.0 * float((r32["low"].double() - r64["low"]).abs().max())
    shares = so.band_share(r64["logits"], band)
    print(f"portrait case: band {band:.3e}, largest share inside {max(shares):.4%}, logit std {float(r64['logits'].std()):.2f}")
    H, W = so.PORTRAIT["hw"]
    assert H > W and (so.PORTRAIT["max_boxes"] * H * W) % 4 == 2 and len(so.PORTRAIT["boxes"]) > so.PORTRAIT["max_boxes"]
    assert tuple(r64["logits"].shape) == (3, 3, H, W) and max(shares) <= 0.01, shares
    for plane in r64["logits"].reshape(-1, H * W):
        assert 0.01 < float((plane > 0).double().mean()) < 0.99


def test_masks_of_the_vit_b_case_are_well_conditioned():
    """The same check for the vit_b case at 1024 (two CPU forward passes of ViT-B: about a minute)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    r64, r32, _, _ = so.reference_pair(so.VITB)
    band = 4.0 * float((r32["low"].double() - r64["low"]).abs().max())
    shares = so.band_share(r64["logits"], band)
    print(f"vit_b case: band {band:.3e}, largest share inside {max(shares):.4%}")
    assert max(shares) <= 0.01, shares
