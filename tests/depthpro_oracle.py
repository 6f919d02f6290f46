"""The checker of Depth Pro on the device: Hugging Face ``transformers.DepthProForDepthEstimation`` in fp64 on the CPU, plus a torch
restatement of ``DepthProImageProcessor``'s preprocessing (normalise, then bilinear resize without antialias) and of
``post_process_depth_estimation`` in the model's dtype. The product package never imports ``transformers``; only tests do.

Both cases use towers of width 128 (2 heads, 4 blocks, hooks [3, 1]), fusion width 64, feature dims [128, 128, 64] / [64, 64] and
the field-of-view model. TINY (crop 128, canvas 512, 150 x 200 input) merges to 24 cells where 32 are wanted, so the bilinear resize
of the merged map runs; GEOM (crop 384, canvas 1536, 375 x 1242 input) has the real token geometry: 35 crops of 577 tokens, padding
3 and 6, merged sides equal to the targets.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from sam_oracle import test_image

_BASE = dict(embed_dim=128, depth=4, heads=2, patch=16, hook_ids=(3, 1), fusion_dim=64, scaled_dims=(128, 128, 64), inter_dims=(64, 64),
             ratios=(0.25, 0.5, 1.0), overlaps=(0.0, 0.5, 0.25), merge_padding=3, num_fov_layers=2, ln_eps=1e-6)
TINY = dict(name="tiny", config=dict(_BASE, crop=128), seed=11, hw=(150, 200), image_seed=4, f_given=180.0)
GEOM = dict(name="geom", config=dict(_BASE, crop=384), seed=12, hw=(375, 1242), image_seed=5, f_given=721.5)


def hf_config(config: dict, device_meta: bool = False):
    from transformers import DepthProConfig
    vit = dict(model_type="dinov2", hidden_size=config["embed_dim"], num_hidden_layers=config["depth"], num_attention_heads=config["heads"],
               image_size=config["crop"], patch_size=config["patch"], mlp_ratio=4, layer_norm_eps=config["ln_eps"], use_swiglu_ffn=False,
               qkv_bias=True, hidden_act="gelu")
    return DepthProConfig(fusion_hidden_size=config["fusion_dim"], patch_size=config["crop"], intermediate_hook_ids=list(config["hook_ids"]),
                          intermediate_feature_dims=list(config["inter_dims"]), scaled_images_ratios=list(config["ratios"]),
                          scaled_images_overlap_ratios=list(config["overlaps"]), scaled_images_feature_dims=list(config["scaled_dims"]),
                          merge_padding_value=config["merge_padding"], use_fov_model=True, num_fov_head_layers=config["num_fov_layers"],
                          image_model_config=dict(vit), patch_model_config=dict(vit), fov_model_config=dict(vit), attn_implementation="eager")


def build_model(config: dict, sd: Dict[str, torch.Tensor], dtype=torch.float64):
    """HF DepthProForDepthEstimation with ``sd`` loaded strictly."""
    from transformers import DepthProForDepthEstimation
    model = DepthProForDepthEstimation(hf_config(config)).eval()
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(dtype)


def preprocess(image_u8: np.ndarray, canvas: int, dtype) -> torch.Tensor:
    """DepthProImageProcessor._preprocess: rescale + normalise FIRST ((x / 255 - 0.5) / 0.5), then the bilinear resize to the canvas
    (torch interpolation, antialias off). [1, 3, S, S]."""
    x = torch.from_numpy(image_u8.copy()).permute(2, 0, 1)[None].to(dtype)
    x = (x / 255.0 - 0.5) / 0.5
    return F.interpolate(x, size=(canvas, canvas), mode="bilinear", align_corners=False)


def postprocess(canonical: torch.Tensor, hw, f_px: torch.Tensor):
    """post_process_depth_estimation with the focal length already chosen: (inverse depth before the clamp, depth)."""
    H, W = hw
    inv = canonical * W / f_px
    inv = F.interpolate(inv[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0]
    return inv, 1.0 / torch.clamp(inv, min=1e-4, max=1e4)


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    return x[0].permute(1, 2, 0).contiguous()


@torch.no_grad()
def run(model, image_u8: np.ndarray, f_given: float) -> Dict[str, torch.Tensor]:
    """Every stage the GPU tests compare, in the model's dtype."""
    dtype = next(model.parameters()).dtype
    cfg = model.config
    S = 4 * cfg.patch_size
    H, W = image_u8.shape[:2]
    x = preprocess(image_u8, S, dtype)
    out = {"pyramid0": _nhwc(x)}
    for i, r in ((1, 0.5), (2, 0.25)):
        out[f"pyramid{i}"] = _nhwc(F.interpolate(x, scale_factor=r, mode="bilinear", align_corners=False))
    enc = model.depth_pro.encoder(x)
    for i, f in enumerate(enc.features):
        out[f"features{i}"] = _nhwc(f)
    neck = model.depth_pro.neck(list(enc.features))
    for i, f in enumerate(neck):
        out[f"neck{i}"] = _nhwc(f)
    fused = model.fusion_stage(neck)[-1]
    out["fused"] = _nhwc(fused)
    canonical = model.head(fused)[0]
    out["canonical"] = canonical
    fov = model.fov_model(pixel_values=x, global_features=neck[0])
    out["fov"] = fov.reshape(1)
    f_est = 0.5 * W / torch.tan(0.5 * torch.deg2rad(fov.reshape(())))
    out["f_est"] = f_est.reshape(1)
    out["inv_est"], out["depth_est"] = postprocess(canonical, (H, W), f_est)
    out["inv_given"], out["depth_given"] = postprocess(canonical, (H, W), torch.tensor(f_given, dtype=dtype))
    return out


def case_inputs(case):
    from ovmono3d_amd.util.synth_depthpro_weights import synth_depthpro_state_dict
    return synth_depthpro_state_dict(case["config"], seed=case["seed"]), test_image(*case["hw"], seed=case["image_seed"])


_CACHE: Dict[str, tuple] = {}


def reference_pair(case):
    """(fp64 stages, fp32 stages, state dict, image) of one case, computed once per process: the fp32 run of the same HF model is the
    yardstick of the float tolerances (tests/test_gpu_depthpro.py)."""
    if case["name"] not in _CACHE:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        sd, img = case_inputs(case)
        m64 = build_model(case["config"], sd, torch.float64)
        r64 = run(m64, img, case["f_given"])
        del m64
        m32 = build_model(case["config"], sd, torch.float32)
        r32 = run(m32, img, case["f_given"])
        _CACHE[case["name"]] = (r64, r32, sd, img)
    return _CACHE[case["name"]]


def fp32_error(r64, r32, key: str) -> float:
    """Scale-relative error (tests/common.py rel_err) of the fp32 HF run against the fp64 one."""
    a, b = r32[key].double(), r64[key].double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
