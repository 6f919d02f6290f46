"""Seeded synthetic Depth Pro checkpoints in Hugging Face key names (``apple/DepthPro-hf``): what
``ovmono3d_amd.depthpro.build_depthpro`` loads, for tests and benchmarks without the published weights.

A library-default initialisation is useless for comparing two implementations: most of the depth head's outputs are exactly 0 behind
its last ReLU and the field of view comes out negative. These weights are shaped instead:
  * ``head.layers.4`` has non-negative weights and a positive bias, so the canonical inverse depth is bounded away from 0;
  * every convolution is scaled by its fan-in, so activations stay O(1) through the decoder and the inverse depth far from the clamp;
  * the field-of-view head's last convolution has a bias of 60 and small weights: the estimate stays within a few degrees of 60.
"""
from __future__ import annotations

import math
from typing import Dict

import torch


def synth_depthpro_state_dict(config: dict, seed: int = 0) -> Dict[str, torch.Tensor]:
    """config: the keys of ``ovmono3d_amd.depthpro.DEFAULT_CONFIG``."""
    D, L, P, crop, F = config["embed_dim"], config["depth"], config["patch"], config["crop"], config["fusion_dim"]
    sdims, idims, nfov = tuple(config["scaled_dims"]), tuple(config["inter_dims"]), config["num_fov_layers"]
    G = crop // P
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def norm(key):
        sd[key + ".weight"] = 0.75 + 0.5 * torch.rand(D, generator=g)
        sd[key + ".bias"] = rn(D, std=0.05)

    def linear(key, n, k, gain=1.0):
        sd[key + ".weight"] = rn(n, k, std=gain / math.sqrt(k))
        sd[key + ".bias"] = rn(n, std=0.02)

    def conv(key, co, ci, k, bias=True, gain=1.0):
        sd[key + ".weight"] = rn(co, ci, k, k, std=gain / math.sqrt(ci * k * k))
        if bias:
            sd[key + ".bias"] = rn(co, std=0.05)

    def convt(key, ci, co, bias=False, gain=1.0):
        sd[key + ".weight"] = rn(ci, co, 2, 2, std=gain / math.sqrt(ci))
        if bias:
            sd[key + ".bias"] = rn(co, std=0.05)

    def tower(V):
        sd[V + "embeddings.cls_token"] = rn(1, 1, D, std=0.02)
        sd[V + "embeddings.mask_token"] = torch.zeros(1, D)
        sd[V + "embeddings.position_embeddings"] = rn(1, 1 + G * G, D, std=0.02)
        conv(V + "embeddings.patch_embeddings.projection", D, 3, P)
        for l in range(L):
            B = f"{V}encoder.layer.{l}."
            norm(B + "norm1"); norm(B + "norm2")
            for n in ("query", "key", "value"):
                linear(B + "attention.attention." + n, D, D)
            linear(B + "attention.output.dense", D, D)
            sd[B + "layer_scale1.lambda1"] = 0.2 + 0.3 * torch.rand(D, generator=g)
            linear(B + "mlp.fc1", 4 * D, D)
            linear(B + "mlp.fc2", D, 4 * D)
            sd[B + "layer_scale2.lambda1"] = 0.2 + 0.3 * torch.rand(D, generator=g)
        norm(V + "layernorm")

    tower("depth_pro.encoder.patch_encoder.model.")
    tower("depth_pro.encoder.image_encoder.model.")
    U = "depth_pro.neck.feature_upsample."
    convt(U + "image_block.layers.0", D, sdims[0], bias=True)
    for i, c in enumerate(sdims):
        conv(f"{U}scaled_images.{i}.layers.0", c, D, 1, bias=False)
        convt(f"{U}scaled_images.{i}.layers.1", c, c)
    for i, c in enumerate(idims):
        mid = F if i == 0 else c
        conv(f"{U}intermediate.{i}.layers.0", mid, D, 1, bias=False)
        for k in range(2 + i):
            convt(f"{U}intermediate.{i}.layers.{1 + k}", mid if k == 0 else c, c)
    conv("depth_pro.neck.fuse_image_with_low_res", sdims[0], 2 * sdims[0], 1)
    dims = sdims + idims
    for i, c in enumerate(dims):
        if i == len(dims) - 1 and c == F:
            continue                                             # nn.Identity
        conv(f"depth_pro.neck.feature_projection.projections.{i}", F, c, 3, bias=False)
    for name, deconv in [(f"fusion_stage.intermediate.{i}", True) for i in range(len(dims) - 1)] + [("fusion_stage.final", False)]:
        for r in ("residual_layer1", "residual_layer2"):
            conv(f"{name}.{r}.convolution1", F, F, 3, gain=1.0)
            conv(f"{name}.{r}.convolution2", F, F, 3, gain=0.5)
        if deconv:
            convt(f"{name}.deconv", F, F)
        conv(f"{name}.projection", F, F, 1, gain=0.7)
    conv("head.layers.0", F // 2, F, 3)
    convt("head.layers.1", F // 2, F // 2, bias=True)
    conv("head.layers.2", 32, F // 2, 3, gain=1.4)
    sd["head.layers.4.weight"] = torch.rand(1, 32, 1, 1, generator=g) * (0.5 / 32 ** 0.5)     # >= 0: the output is >= the bias
    sd["head.layers.4.bias"] = torch.tensor([0.5])
    tower("fov_model.fov_encoder.model.")
    linear("fov_model.fov_encoder.neck", F // 2, D)
    conv("fov_model.conv", F // 2, F, 3)
    for i in range(nfov):
        conv(f"fov_model.head.layers.{2 * i}", F >> (i + 2), F >> (i + 1), 3)
    k = int((G - 1) / 2 ** nfov + 1)
    cf = F >> (nfov + 1)
    sd[f"fov_model.head.layers.{2 * nfov}.weight"] = rn(1, cf, k, k, std=3.0 / math.sqrt(cf * k * k))
    sd[f"fov_model.head.layers.{2 * nfov}.bias"] = torch.tensor([60.0])
    return sd
