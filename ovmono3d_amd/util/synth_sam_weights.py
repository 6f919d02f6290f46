"""Seeded synthetic checkpoints of the whole Segment Anything model in segment_anything's own key names (``image_encoder.*``,
``prompt_encoder.*``, ``mask_decoder.*``): what ``ovmono3d_amd.sam.build_sam`` loads, for tests and benchmarks without the
published weights.

The image-encoder part follows ``synth_weights.synth_sam_state_dict`` (relative-position tables get real values). The last layers
of the hypernetwork MLPs and of the upscaling are scaled up so that the mask logits spread over several units: with a
library-default initialisation a large share of the logits lies within 1e-3 of zero, and a thresholded comparison of two
implementations then says nothing.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .synth_weights import SAM_ARCH, _lin

PROMPT_DIM = 256


def synth_sam_predictor_state_dict(arch: str = "vit_b", seed: int = 0, image_size: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """``image_size``: the encoder's input side (default: the architecture's checkpoint grid x patch, 1024 for the published ones)."""
    D, L, H, P, M, ws, glob = SAM_ARCH[arch]
    if image_size is not None:
        M = image_size // P
    dh, C = D // H, PROMPT_DIM
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def norm(key, n):
        sd[key + ".weight"] = 0.5 + torch.rand(n, generator=g)
        sd[key + ".bias"] = rn(n, std=0.05)

    V = "image_encoder."
    sd[V + "pos_embed"] = rn(1, M, M, D, std=0.02)
    sd[V + "patch_embed.proj.weight"] = rn(D, 3, P, P, std=1.0 / math.sqrt(3.0 * P * P))
    sd[V + "patch_embed.proj.bias"] = rn(D, std=0.02)
    for i in range(L):
        B = V + f"blocks.{i}."
        norm(B + "norm1", D)
        norm(B + "norm2", D)
        sd[B + "attn.qkv.weight"], sd[B + "attn.qkv.bias"] = _lin(g, 3 * D, D, std=2.0 / math.sqrt(D))
        sd[B + "attn.proj.weight"], sd[B + "attn.proj.bias"] = _lin(g, D, D, std=0.5 / math.sqrt(D))
        side = M if i in glob else ws
        sd[B + "attn.rel_pos_h"] = rn(2 * side - 1, dh, std=0.05)
        sd[B + "attn.rel_pos_w"] = rn(2 * side - 1, dh, std=0.05)
        sd[B + "mlp.lin1.weight"], sd[B + "mlp.lin1.bias"] = _lin(g, 4 * D, D)
        sd[B + "mlp.lin2.weight"], sd[B + "mlp.lin2.bias"] = _lin(g, D, 4 * D, std=0.5 / math.sqrt(4 * D))
    sd[V + "neck.0.weight"] = rn(C, D, 1, 1, std=1.0 / math.sqrt(D))
    norm(V + "neck.1", C)
    sd[V + "neck.2.weight"] = rn(C, C, 3, 3, std=1.0 / math.sqrt(9.0 * C))
    norm(V + "neck.3", C)

    Pk = "prompt_encoder."
    sd[Pk + "pe_layer.positional_encoding_gaussian_matrix"] = rn(2, C // 2)
    for i in range(4):
        sd[Pk + f"point_embeddings.{i}.weight"] = rn(1, C, std=0.5)
    sd[Pk + "not_a_point_embed.weight"] = rn(1, C, std=0.5)
    sd[Pk + "no_mask_embed.weight"] = rn(1, C, std=0.5)
    # the mask-input branch: part of every checkpoint, unused with box prompts
    sd[Pk + "mask_downscaling.0.weight"], sd[Pk + "mask_downscaling.0.bias"] = rn(4, 1, 2, 2, std=0.5), rn(4, std=0.02)
    norm(Pk + "mask_downscaling.1", 4)
    sd[Pk + "mask_downscaling.3.weight"], sd[Pk + "mask_downscaling.3.bias"] = rn(16, 4, 2, 2, std=0.25), rn(16, std=0.02)
    norm(Pk + "mask_downscaling.4", 16)
    sd[Pk + "mask_downscaling.6.weight"], sd[Pk + "mask_downscaling.6.bias"] = rn(C, 16, 1, 1, std=0.25), rn(C, std=0.02)

    Dk = "mask_decoder."
    sd[Dk + "iou_token.weight"] = rn(1, C, std=0.5)
    sd[Dk + "mask_tokens.weight"] = rn(4, C, std=0.5)

    def attn(key, internal):
        for n, (o, i) in (("q_proj", (internal, C)), ("k_proj", (internal, C)), ("v_proj", (internal, C)), ("out_proj", (C, internal))):
            sd[key + f".{n}.weight"], sd[key + f".{n}.bias"] = _lin(g, o, i)

    for i in range(2):
        T = Dk + f"transformer.layers.{i}."
        attn(T + "self_attn", C)
        attn(T + "cross_attn_token_to_image", C // 2)
        attn(T + "cross_attn_image_to_token", C // 2)
        for n in ("norm1", "norm2", "norm3", "norm4"):
            norm(T + n, C)
        sd[T + "mlp.lin1.weight"], sd[T + "mlp.lin1.bias"] = _lin(g, 2048, C)
        sd[T + "mlp.lin2.weight"], sd[T + "mlp.lin2.bias"] = _lin(g, C, 2048, std=0.5 / math.sqrt(2048))
    attn(Dk + "transformer.final_attn_token_to_image", C // 2)
    norm(Dk + "transformer.norm_final_attn", C)
    sd[Dk + "output_upscaling.0.weight"], sd[Dk + "output_upscaling.0.bias"] = rn(C, C // 4, 2, 2, std=1.0 / math.sqrt(C)), rn(C // 4, std=0.02)
    norm(Dk + "output_upscaling.1", C // 4)
    # x4 / x3 on the last upscaling and hypernetwork layers: mask logits with a standard deviation of several units
    sd[Dk + "output_upscaling.3.weight"], sd[Dk + "output_upscaling.3.bias"] = rn(C // 4, C // 8, 2, 2, std=4.0 / math.sqrt(C // 4)), rn(C // 8, std=0.5)
    for i in range(4):
        Hk = Dk + f"output_hypernetworks_mlps.{i}.layers."
        sd[Hk + "0.weight"], sd[Hk + "0.bias"] = _lin(g, C, C, std=math.sqrt(2.0 / C))
        sd[Hk + "1.weight"], sd[Hk + "1.bias"] = _lin(g, C, C, std=math.sqrt(2.0 / C))
        sd[Hk + "2.weight"], sd[Hk + "2.bias"] = _lin(g, C // 8, C, std=3.0 * math.sqrt(2.0 / C), bias_std=0.5)
    Ik = Dk + "iou_prediction_head.layers."
    sd[Ik + "0.weight"], sd[Ik + "0.bias"] = _lin(g, C, C, std=math.sqrt(2.0 / C))
    sd[Ik + "1.weight"], sd[Ik + "1.bias"] = _lin(g, C, C, std=math.sqrt(2.0 / C))
    sd[Ik + "2.weight"], sd[Ik + "2.bias"] = _lin(g, 4, C, std=math.sqrt(2.0 / C))
    return sd
