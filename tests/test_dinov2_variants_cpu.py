"""DINOv2 register-token and SwiGLU variants, the parts that need no GPU: tables, synthetic checkpoints against Hugging Face's
models, the checker of tests/dinov2_variants_oracle.py against the same, the host-side position resize, the weight row order of the
SwiGLU epilogue, and the loader's refusals (which happen before the first device call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import build_cfg
from ovmono3d_amd.util.synth_weights import VIT_ARCH, swiglu_hidden, synth_state_dict, vit_variant

import dinov2_variants_oracle as vo

V = "backbone.net.vit."


def _hf_model(name, pos_grid):
    from transformers import Dinov2Config, Dinov2Model, Dinov2WithRegistersConfig, Dinov2WithRegistersModel
    D, L, heads = VIT_ARCH[name]
    n_reg, ffn = vit_variant(name)
    kw = dict(hidden_size=D, num_hidden_layers=L, num_attention_heads=heads, image_size=14 * pos_grid, patch_size=14, mlp_ratio=4,
              layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=(ffn == "swiglu"))
    if n_reg:
        return Dinov2WithRegistersModel(Dinov2WithRegistersConfig(num_register_tokens=n_reg, **kw)).eval()
    return Dinov2Model(Dinov2Config(**kw)).eval()


def test_arch_tables():
    assert all(isinstance(v, tuple) and len(v) == 3 for v in VIT_ARCH.values())
    for n in ("vits14_reg", "vitb14_reg", "vitl14_reg", "vitg14_reg", "vittest14_reg", "vitgtest14", "vitgtest14_reg", "vitg14_d2", "vitl14_reg_d2"):
        assert n in VIT_ARCH
    assert VIT_ARCH["vitb14_reg"] == VIT_ARCH["vitb14"] and VIT_ARCH["vitg14_d2"] == (1536, 2, 24) and VIT_ARCH["vitl14_reg_d2"] == (1024, 2, 16)
    assert vit_variant("vitb14") == (0, "mlp") and vit_variant("vitb14_reg") == (4, "mlp")
    assert vit_variant("vitg14") == (0, "swiglu") and vit_variant("vitg14_reg") == (4, "swiglu") and vit_variant("vitgtest14_reg") == (4, "swiglu")
    assert vit_variant("vitl14_d2") == (0, "mlp") and vit_variant("vitg14_d2") == (0, "swiglu") and vit_variant("vitl14_reg_d2") == (4, "mlp")
    assert (swiglu_hidden(128), swiglu_hidden(384), swiglu_hidden(1536)) == (344, 1024, 4096)


def test_synthetic_key_trees():
    sd = synth_state_dict("vitgtest14_reg", seed=3)
    assert sd[V + "register_tokens"].shape == (1, 4, 128) and float(sd[V + "register_tokens"].abs().min()) > 0
    assert sd[V + "blocks.1.mlp.w12.weight"].shape == (688, 128) and sd[V + "blocks.1.mlp.w12.bias"].shape == (688,)
    assert sd[V + "blocks.1.mlp.w3.weight"].shape == (128, 344) and sd[V + "blocks.1.mlp.w3.bias"].shape == (128,)
    assert not [k for k in sd if ".mlp.fc1." in k or ".mlp.fc2." in k]
    plain, reg = synth_state_dict("vittest14", seed=3), synth_state_dict("vittest14_reg", seed=3)
    assert set(reg) - set(plain) == {V + "register_tokens"}
    assert all(torch.equal(plain[k], reg[k]) for k in plain)          # a register model is its plain twin plus the registers
    assert not [k for k in plain if "w12" in k or "w3" in k]


@pytest.mark.parametrize("name", ["vittest14_reg", "vitgtest14", "vitgtest14_reg"])
def test_synthetic_checkpoint_loads_strictly_into_hf(name):
    sd = synth_state_dict(name, seed=2, pos_grid=16)
    m = _hf_model(name, 16)
    m.load_state_dict(vo.hub_to_hf(sd, VIT_ARCH[name][1]), strict=True)


@pytest.mark.parametrize("name,grid", [("vittest14_reg", 10), ("vitgtest14", 16), ("vitgtest14_reg", 10)])
def test_checker_matches_hf_last_block_tokens(name, grid):
    """vittest14_reg: the 16-grid table resized DOWN to a 10-grid canvas, the only case where antialias changes values. vitgtest14: canvas
    grid = table grid (Hugging Face's plain Dinov2 resizes without the hub's 0.1 offset, so only the no-resize case is comparable)."""
    D, L, heads = VIT_ARCH[name]
    sd = synth_state_dict(name, seed=4, pos_grid=16)
    m = _hf_model(name, 16)
    m.load_state_dict(vo.hub_to_hf(sd, L), strict=True)
    img = torch.randn(2, 3, 14 * grid, 14 * grid, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        y_hf = m(pixel_values=img, output_hidden_states=True, interpolate_pos_encoding=True).hidden_states[-1]
        y = vo.last_block_tokens(sd, img, heads, L)
    assert y.shape == y_hf.shape == (2, 1 + vit_variant(name)[0] + grid * grid, D)
    assert (y - y_hf).abs().max() < 2e-5 * y_hf.abs().max()
    if vit_variant(name)[0]:
        # and the antialias matters at this size: the plain bicubic table differs
        pos = sd[V + "pos_embed"]
        g = pos[:, 1:].reshape(1, 16, 16, D).permute(0, 3, 1, 2)
        plain = F.interpolate(g, size=(grid, grid), mode="bicubic", antialias=False).permute(0, 2, 3, 1).reshape(1, -1, D)
        assert (vo.resize_pos_antialias(pos, grid, grid)[:, 1:] - plain).abs().max() > 1e-3


def test_dense_tap_skips_registers():
    sd = synth_state_dict("vitgtest14_reg", seed=1, pos_grid=16)
    img = torch.randn(1, 3, 140, 140, generator=torch.Generator().manual_seed(1))
    dense = vo.dino_backbone_forward(sd, img, 2, 2, None, True)
    x = vo.last_block_tokens(sd, img, 2, 2)
    assert torch.equal(dense, x[:, 5:].reshape(1, 10, 10, 128).permute(0, 3, 1, 2))
    with pytest.raises(AssertionError):
        vo.dino_backbone_forward(sd, img, 2, 2, torch.rand(1, 1, 30, 40), True)


@pytest.mark.parametrize("M,G", [(16, 10), (37, 16), (16, 16), (6, 9)])
def test_engine_position_table_for_register_models(M, G):
    """The table a register model gets (ovm_host_resize_pos_embed_aa in csrc/api.hip) is F.interpolate(..., antialias=True)."""
    from ovmono3d_amd import lib
    L = lib.load()
    D = 24
    pos = torch.randn(1, 1 + M * M, D, generator=torch.Generator().manual_seed(M * 100 + G))
    src = np.ascontiguousarray(pos[0].numpy())
    out = np.empty((1 + G * G, D), np.float32)
    assert L.ovm_host_resize_pos_embed_aa(src.ctypes.data, M, D, G, out.ctypes.data) == 0
    ref = vo.resize_pos_antialias(pos, G, G)[0]
    assert np.array_equal(out[0], src[0])
    assert float((torch.from_numpy(out) - ref).abs().max()) < 2e-6 * float(ref.abs().max())


@pytest.mark.parametrize("Hs", [1, 16, 344, 4096])
def test_swiglu_row_order(Hs):
    """ovm_host_swiglu_perm: blocks of 16 gate rows | 16 value rows, outputs padded to 32 with zero rows; every source row once."""
    from ovmono3d_amd import lib
    L = lib.load()
    Kp = (Hs + 31) // 32 * 32
    perm = np.full(2 * Kp, -7, np.int32)
    assert L.ovm_host_swiglu_perm(Hs, perm.ctypes.data) == 0
    n = np.arange(2 * Kp)
    j = (n // 32) * 16 + n % 16
    want = np.where(j < Hs, np.where(n % 32 >= 16, Hs + j, j), -1)
    assert np.array_equal(perm, want)
    assert sorted(perm[perm >= 0].tolist()) == list(range(2 * Hs))
    assert L.ovm_host_swiglu_perm(0, perm.ctypes.data) != 0 and L.ovm_host_swiglu_perm(8, None) != 0


def _create_rc(sd):
    from ovmono3d_amd import lib
    from ovmono3d_amd.native import config_to_native
    L = lib.load()
    ncfg = config_to_native(build_cfg("vitgtest14_reg", 224, "f16x3", max_batch=1, max_rois=8))
    arrs = {k: np.ascontiguousarray(v.detach().float().numpy()) for k, v in sd.items() if v.dim() <= 4}
    table, keep = lib.make_tensor_table(arrs)
    h = C.c_void_p()
    rc = L.ovm_create(C.byref(ncfg), table, len(keep), 0, C.byref(h))
    msg = (L.ovm_last_error(h) or b"").decode()
    L.ovm_destroy(h)
    return rc, msg


def test_loader_refusals_name_the_key():
    """Variant detection is host-only and comes before the first device call, so these run without a GPU."""
    base = synth_state_dict("vitgtest14_reg", seed=0)
    B0 = V + "blocks.0.mlp."
    sd = dict(base); sd[B0 + "fc1.weight"] = torch.zeros(512, 128)
    rc, msg = _create_rc(sd)
    assert rc == -1 and "w12.weight" in msg and "fc1.weight" in msg and "both" in msg
    sd = {k: v for k, v in base.items() if not k.startswith(B0 + "w12")}
    rc, msg = _create_rc(sd)
    assert rc == -3 and "w12.weight" in msg and "fc1.weight" in msg
    sd = dict(base); sd[B0 + "w12.weight"] = torch.zeros(687, 128)
    rc, msg = _create_rc(sd)
    assert rc == -4 and B0 + "w12.weight" in msg
    sd = dict(base); sd[B0 + "w12.weight"] = torch.zeros(688, 96)
    rc, msg = _create_rc(sd)
    assert rc == -4 and B0 + "w12.weight" in msg
    sd = dict(base); sd[B0 + "w3.weight"] = torch.zeros(128, 352)
    rc, msg = _create_rc(sd)
    assert rc == -4 and B0 + "w3.weight" in msg
    sd = {k: v for k, v in base.items() if k != B0 + "w3.weight"}
    rc, msg = _create_rc(sd)
    assert rc == -3 and B0 + "w3.weight" in msg
    sd = dict(base); sd[V + "register_tokens"] = torch.ones(1, 17, 128)
    rc, msg = _create_rc(sd)
    assert rc == -5 and "register_tokens" in msg
    sd = dict(base); sd[V + "register_tokens"] = torch.ones(1, 4, 64)
    rc, msg = _create_rc(sd)
    assert rc == -4 and "register_tokens" in msg


def test_config_accepts_the_new_names():
    from ovmono3d_amd.native import config_to_native
    for n, D in (("vitb14_reg", 768), ("vitg14", 1536), ("vitg14_reg", 1536), ("vittest14_reg", 128)):
        c = config_to_native(build_cfg(n, 518, "f16x3", max_batch=1))
        assert (c.embed_dim, c.tower) == (D, 0)
    with pytest.raises(ValueError):
        config_to_native(build_cfg("vitb14_regs", 518, "f16x3", max_batch=1))
