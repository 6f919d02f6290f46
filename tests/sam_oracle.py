"""The checker of the SAM predictor: Hugging Face ``transformers.SamModel`` (a port of segment_anything that loads the official
weights) in fp64 on the CPU, plus an fp64 torch restatement of ``SamPredictor``'s pre- and post-processing (PIL for the resize).
Used as HF GroundingDINO is for the detector: the product package never imports ``transformers``; only tests do.

``sa_to_hf`` maps segment_anything's key names to HF's. HF keeps the prompt encoder's Gaussian matrix twice (the model's
``shared_image_embedding`` and the prompt encoder's ``shared_embedding``); both receive the one tensor.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from ovmono3d_amd.sam import PIXEL_MEAN, PIXEL_STD
from ovmono3d_amd.util.synth_weights import SAM_ARCH

_RULES = [
    (r"^image_encoder\.blocks\.(\d+)\.norm([12])\.", r"vision_encoder.layers.\1.layer_norm\2."),
    (r"^image_encoder\.blocks\.(\d+)\.", r"vision_encoder.layers.\1."),
    (r"^image_encoder\.patch_embed\.proj\.", "vision_encoder.patch_embed.projection."),
    (r"^image_encoder\.neck\.0\.", "vision_encoder.neck.conv1."),
    (r"^image_encoder\.neck\.1\.", "vision_encoder.neck.layer_norm1."),
    (r"^image_encoder\.neck\.2\.", "vision_encoder.neck.conv2."),
    (r"^image_encoder\.neck\.3\.", "vision_encoder.neck.layer_norm2."),
    (r"^image_encoder\.", "vision_encoder."),
    (r"^prompt_encoder\.pe_layer\.positional_encoding_gaussian_matrix$", "shared_image_embedding.positional_embedding"),
    (r"^prompt_encoder\.point_embeddings\.(\d+)\.", r"prompt_encoder.point_embed.\1."),
    (r"^prompt_encoder\.mask_downscaling\.0\.", "prompt_encoder.mask_embed.conv1."),
    (r"^prompt_encoder\.mask_downscaling\.1\.", "prompt_encoder.mask_embed.layer_norm1."),
    (r"^prompt_encoder\.mask_downscaling\.3\.", "prompt_encoder.mask_embed.conv2."),
    (r"^prompt_encoder\.mask_downscaling\.4\.", "prompt_encoder.mask_embed.layer_norm2."),
    (r"^prompt_encoder\.mask_downscaling\.6\.", "prompt_encoder.mask_embed.conv3."),
    (r"^mask_decoder\.transformer\.layers\.(\d+)\.norm([1234])\.", r"mask_decoder.transformer.layers.\1.layer_norm\2."),
    (r"^mask_decoder\.transformer\.norm_final_attn\.", "mask_decoder.transformer.layer_norm_final_attn."),
    (r"^mask_decoder\.output_upscaling\.0\.", "mask_decoder.upscale_conv1."),
    (r"^mask_decoder\.output_upscaling\.1\.", "mask_decoder.upscale_layer_norm."),
    (r"^mask_decoder\.output_upscaling\.3\.", "mask_decoder.upscale_conv2."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.0\.", r"mask_decoder.\1.proj_in."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.1\.", r"mask_decoder.\1.layers.0."),
    (r"^mask_decoder\.(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.2\.", r"mask_decoder.\1.proj_out."),
]
TIED = ("prompt_encoder.shared_embedding.positional_embedding", "shared_image_embedding.positional_embedding")


def sa_to_hf(key: str) -> str:
    for pat, rep in _RULES:
        new, n = re.subn(pat, rep, key)
        if n:
            return new
    return key


def convert_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """segment_anything names -> HF names, without the second copy of the tied matrix."""
    return {sa_to_hf(k): v for k, v in sd.items()}


def hf_config(arch: str, image_size: int):
    from transformers import SamConfig, SamMaskDecoderConfig, SamPromptEncoderConfig, SamVisionConfig
    D, L, heads, patch, _, ws, glob = SAM_ARCH[arch]
    vis = SamVisionConfig(hidden_size=D, output_channels=256, num_hidden_layers=L, num_attention_heads=heads, image_size=image_size,
                          patch_size=patch, window_size=ws, global_attn_indexes=list(glob), layer_norm_eps=1e-6, hidden_act="gelu",
                          mlp_dim=4 * D, num_pos_feats=128)
    prm = SamPromptEncoderConfig(hidden_size=256, image_size=image_size, patch_size=patch)
    # segment_anything's two-way transformer uses nn.LayerNorm's default eps (1e-5) in every norm
    dec = SamMaskDecoderConfig(hidden_size=256, mlp_dim=2048, num_hidden_layers=2, num_attention_heads=8, attention_downsample_rate=2,
                               num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256, layer_norm_eps=1e-5)
    return SamConfig(vision_config=vis, prompt_encoder_config=prm, mask_decoder_config=dec, attn_implementation="eager")


def build_model(arch: str, sd: Dict[str, torch.Tensor], image_size: int, dtype=torch.float64, strict_report: Optional[dict] = None):
    """HF SamModel with the segment_anything-named weights ``sd`` loaded strictly."""
    from transformers import SamModel
    model = SamModel(hf_config(arch, image_size)).eval()
    hf = convert_state_dict(sd)
    hf[TIED[0]] = hf[TIED[1]]
    res = model.load_state_dict(hf, strict=False)
    if strict_report is not None:
        strict_report["missing"], strict_report["unexpected"] = list(res.missing_keys), list(res.unexpected_keys)
    assert not res.missing_keys and not res.unexpected_keys, (res.missing_keys, res.unexpected_keys)
    return model.to(dtype)


def preprocess_shape(h: int, w: int, image_size: int):
    scale = image_size * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def preprocess(image_u8: np.ndarray, image_size: int, flip: bool, dtype=torch.float64) -> torch.Tensor:
    """SamPredictor.set_image up to the encoder: ResizeLongestSide (PIL bilinear on uint8), optional channel flip, (x - mean) / std,
    zero padding bottom / right. image_u8: [H, W, 3]. Returns [1, 3, S, S]."""
    H, W = image_u8.shape[:2]
    nh, nw = preprocess_shape(H, W, image_size)
    img = image_u8[..., ::-1] if flip else image_u8
    r = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((nw, nh), Image.BILINEAR))
    x = torch.from_numpy(r.copy()).permute(2, 0, 1).to(dtype)
    x = (x - torch.tensor(PIXEL_MEAN, dtype=dtype).view(3, 1, 1)) / torch.tensor(PIXEL_STD, dtype=dtype).view(3, 1, 1)
    return F.pad(x, (0, image_size - nw, 0, image_size - nh))[None]


def postprocess(low_res: torch.Tensor, image_size: int, input_hw, original_hw) -> torch.Tensor:
    """Sam.postprocess_masks: [n, k, L, L] logits -> [n, k, H, W] logits."""
    m = F.interpolate(low_res, (image_size, image_size), mode="bilinear", align_corners=False)
    m = m[..., : input_hw[0], : input_hw[1]]
    return F.interpolate(m, tuple(original_hw), mode="bilinear", align_corners=False)


@torch.no_grad()
def run(model, image_u8: np.ndarray, boxes_xyxy: Sequence[Sequence[float]], flip: bool = False) -> Dict[str, torch.Tensor]:
    """Every stage the GPU tests compare, in the model's dtype. boxes in original pixels."""
    dtype = next(model.parameters()).dtype
    S = model.config.vision_config.image_size
    H, W = image_u8.shape[:2]
    nh, nw = preprocess_shape(H, W, S)
    pre = preprocess(image_u8, S, flip, dtype)
    boxes = np.asarray(boxes_xyxy, np.float64).reshape(-1, 2, 2).copy()      # ResizeLongestSide.apply_boxes, fp64 as numpy does it
    boxes[..., 0] *= nw / W
    boxes[..., 1] *= nh / H
    bt = torch.from_numpy(boxes.reshape(1, -1, 4)).to(dtype)
    got = {}
    hook = model.mask_decoder.transformer.register_forward_hook(lambda mod, args, out: got.__setitem__("tokens", out[0]))
    try:
        emb = model.get_image_embeddings(pre)
        out = model(image_embeddings=emb, input_boxes=bt, multimask_output=True)
    finally:
        hook.remove()
    sparse, _ = model.prompt_encoder(None, None, bt, None)
    low = out.pred_masks[0]                                                   # [n, 3, L, L]
    return {"pre": pre[0], "neck": emb[0].permute(1, 2, 0).contiguous(), "sparse": sparse[0], "tokens": got["tokens"][0], "low": low,
            "iou": out.iou_scores[0], "logits": postprocess(low, S, (nh, nw), (H, W))}


def test_image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """A seeded image with structure at several scales (smooth blobs + noise), uint8 [h, w, 3]."""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(6):
            cy, cx, s, a = g.uniform(0, h), g.uniform(0, w), g.uniform(0.05, 0.4) * max(h, w), g.uniform(-90, 90)
            img[..., c] += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img = 128 + img + g.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


test_image.__test__ = False


def band_share(logits: torch.Tensor, band: float) -> List[float]:
    """Per mask plane [.., H, W] -> share of pixels with |logit| <= band."""
    flat = logits.reshape(-1, logits.shape[-2] * logits.shape[-1])
    return [float((row.abs() <= band).double().mean()) for row in flat]


# ---- the cases the GPU tests run (tests/test_gpu_sam.py) and the CPU condition check examines (tests/test_sam_cpu.py) ----------
TINY = dict(arch="vit_test", image_size=128, seed=3, hw=(70, 100), image_seed=1,
            boxes=[[20.0, 15.0, 70.0, 55.0],        # an ordinary box
                   [40.0, 30.0, 41.0, 31.0],        # one pixel
                   [0.0, 0.0, 100.0, 70.0],         # the whole image
                   [-10.0, -5.0, 60.0, 90.0]])      # reaching outside the image
VITB = dict(arch="vit_b", image_size=1024, seed=5, hw=(600, 900), image_seed=2,
            boxes=[[100.0, 80.0, 400.0, 380.0], [0.0, 0.0, 900.0, 600.0], [450.5, 200.25, 452.0, 203.0], [700.0, 300.0, 950.0, 650.0],
                   [30.0, 400.0, 330.0, 590.0], [500.0, 20.0, 880.0, 290.0], [250.0, 250.0, 650.0, 350.0], [10.0, 10.0, 60.0, 50.0]])
# portrait, an odd pixel count, and more boxes than one decoder pass takes (max_boxes = 2): the second chunk's masks start at byte
# 2 * 99 * 71 = 2 (mod 4), where the mask kernel cannot use its 32-bit stores
PORTRAIT = dict(arch="vit_test", image_size=128, seed=3, hw=(99, 71), image_seed=4, max_boxes=2,
                boxes=[[10.0, 20.0, 50.0, 80.0], [30.5, 5.25, 60.0, 40.0], [-8.0, 60.0, 90.0, 120.0]])      # the last reaches outside


def case_inputs(case):
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    sd = synth_sam_predictor_state_dict(case["arch"], seed=case["seed"], image_size=case["image_size"])
    return sd, test_image(*case["hw"], seed=case["image_seed"])


def reference_pair(case):
    """(fp64 stages, fp32 stages, state dict, image) of one case: the fp32 run of the same HF model is the yardstick of the float
    tolerances (tests/test_gpu_sam.py)."""
    sd, img = case_inputs(case)
    m64 = build_model(case["arch"], sd, case["image_size"], torch.float64)
    r64 = run(m64, img, case["boxes"])
    del m64
    m32 = build_model(case["arch"], sd, case["image_size"], torch.float32)
    r32 = run(m32, img, case["boxes"])
    return r64, r32, sd, img


def fp32_error(r64, r32, key: str) -> float:
    """Scale-relative error (tests/common.py rel_err) of the fp32 HF run against the fp64 one."""
    a, b = r32[key].double(), r64[key].double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
