"""fp32 restatement of the DINOv2 hub variants the plain oracle (oracle/vit.py) does not cover: register tokens (``vit*14_reg``)
and the fused SwiGLU FFN (``vitg14``). Built from oracle/vit.py's functions; what differs is restated here:

* SwiGLUFFNFused: ``x1, x2 = w12(x).chunk(2, -1); w3(silu(x1) * x2)``, hidden width ``(int(4 D * 2 / 3) + 7) // 8 * 8``.
* register models: ``x = cat(cls, patches) + pos; x = cat(x[:, :1], register_tokens, x[:, 1:])`` - the registers are inserted
  after the position table was added, so they carry no position row; the hub builds these models with
  ``interpolate_offset=0.0, interpolate_antialias=True``, i.e. the table is resized with
  ``F.interpolate(size=(gh, gw), mode="bicubic", antialias=True)`` (Hugging Face's Dinov2WithRegistersEmbeddings does the same).
* the dense tap reads the last gh * gw tokens (reference dino.py:116), which skips class and register tokens alike.

Both variants are detected from the checkpoint's keys, as the engine does.  ``hub_to_hf`` maps the hub key tree to Hugging Face's
Dinov2Model(use_swiglu_ffn=True) / Dinov2WithRegistersModel so the restatement can be pinned to an independent implementation.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import vit

PATCH = vit.PATCH


def resize_pos_antialias(pos_embed: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """pos_embed [1, 1 + M*M, D] -> [1, 1 + gh*gw, D]: class row kept, patch rows resized with antialiased bicubic, no offset."""
    N = pos_embed.shape[1] - 1
    M = int(round(N ** 0.5))
    assert M * M == N
    D = pos_embed.shape[-1]
    if gh == M and gw == M:
        return pos_embed
    grid = pos_embed[:, 1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, D)], dim=1)


def prepare_tokens(sd: Dict[str, torch.Tensor], images: torch.Tensor, prefix: str) -> torch.Tensor:
    """dinov2 ``prepare_tokens_with_masks(x, None)`` for plain and register models."""
    reg = sd.get(prefix + "register_tokens")
    if reg is None:
        return vit.prepare_tokens(sd, images, prefix)
    B = images.shape[0]
    x = F.conv2d(images, sd[prefix + "patch_embed.proj.weight"], sd[prefix + "patch_embed.proj.bias"], stride=PATCH)
    gh, gw = x.shape[-2:]
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([sd[prefix + "cls_token"].expand(B, -1, -1), x], dim=1)
    x = x + resize_pos_antialias(sd[prefix + "pos_embed"], gh, gw)
    return torch.cat([x[:, :1], reg.expand(B, -1, -1), x[:, 1:]], dim=1)


def swiglu_ffn(h: torch.Tensor, sd, p: str) -> torch.Tensor:
    x12 = F.linear(h, sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"])
    x1, x2 = x12.chunk(2, dim=-1)
    return F.linear(F.silu(x1) * x2, sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"])


def block(x: torch.Tensor, sd, p: str, heads: int) -> torch.Tensor:
    """dinov2 ``Block.forward`` (eval) with either FFN."""
    if p + "mlp.w12.weight" not in sd:
        return vit.block(x, sd, p, heads)
    D = x.shape[-1]
    h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
    h = vit.attention(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"], sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"], heads)
    x = x + h * sd[p + "ls1.gamma"]
    h = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
    return x + swiglu_ffn(h, sd, p) * sd[p + "ls2.gamma"]


def last_block_tokens(sd, images: torch.Tensor, heads: int, depth: int, net_prefix: str = "backbone.net.") -> torch.Tensor:
    vp = net_prefix + "vit."
    x = prepare_tokens(sd, images, vp)
    for i in range(depth):
        x = block(x, sd, vp + f"blocks.{i}.", heads)
    return x


def dino_backbone_forward(sd: Dict[str, torch.Tensor], images: torch.Tensor, heads: int, depth: int,
                          prompt_depth: Optional[torch.Tensor] = None, use_depth_fusion: bool = True,
                          net_prefix: str = "backbone.net.") -> torch.Tensor:
    """Drop-in for ``oracle.vit.dino_backbone_forward`` (same signature) that also runs the two variants."""
    vp = net_prefix + "vit."
    if vp + "register_tokens" not in sd and vp + "blocks.0.mlp.w12.weight" not in sd:
        return _PLAIN(sd, images, heads, depth, prompt_depth, use_depth_fusion, net_prefix)
    if vp + "register_tokens" in sd:
        # reference dino.py:91-105 takes x[:, 1:] as the patch tokens: its torch.cat of [B, C, R + HW] with [B, 1, HW] raises
        assert prompt_depth is None, "depth fusion is not defined for a register-token model"
    B = images.shape[0]
    gh, gw = images.shape[-2] // PATCH, images.shape[-1] // PATCH
    x = prepare_tokens(sd, images, vp)
    depth_tokens = None
    if use_depth_fusion and prompt_depth is not None:
        depth_tokens = F.interpolate(prompt_depth, size=(gh, gw), mode="bilinear").flatten(2).permute(0, 2, 1)
    for i in range(depth):
        x = block(x, sd, vp + f"blocks.{i}.", heads)
        if depth_tokens is not None and i == depth - 1:
            cls_tok, patch = x[:, :1], x[:, 1:]
            fused = torch.cat([patch.permute(0, 2, 1), depth_tokens.permute(0, 2, 1)], dim=1).view(B, -1, gh, gw)
            fused = F.conv2d(fused, sd[net_prefix + "depth_fusion.weight"], sd[net_prefix + "depth_fusion.bias"])
            x = torch.cat([cls_tok, fused.flatten(2).permute(0, 2, 1)], dim=1)
    spatial = x[:, -gh * gw:]
    return spatial.reshape(B, gh, gw, -1).permute(0, 3, 1, 2).contiguous()


_PLAIN = vit.dino_backbone_forward      # bound at import: tests monkeypatch oracle.vit.dino_backbone_forward with the function above


def hub_to_hf(sd: Dict[str, torch.Tensor], depth: int, prefix: str = "backbone.net.vit.") -> Dict[str, torch.Tensor]:
    """Hub DINOv2 key tree -> Hugging Face Dinov2Model / Dinov2WithRegistersModel state dict (every key of those models)."""
    hf = {"embeddings.cls_token": sd[prefix + "cls_token"], "embeddings.mask_token": sd[prefix + "mask_token"],
          "embeddings.position_embeddings": sd[prefix + "pos_embed"],
          "embeddings.patch_embeddings.projection.weight": sd[prefix + "patch_embed.proj.weight"],
          "embeddings.patch_embeddings.projection.bias": sd[prefix + "patch_embed.proj.bias"],
          "layernorm.weight": sd[prefix + "norm.weight"], "layernorm.bias": sd[prefix + "norm.bias"]}
    if prefix + "register_tokens" in sd:
        hf["embeddings.register_tokens"] = sd[prefix + "register_tokens"]
    for i in range(depth):
        p, q = prefix + f"blocks.{i}.", f"encoder.layer.{i}."
        wq, wk, wv = sd[p + "attn.qkv.weight"].chunk(3, 0)
        bq, bk, bv = sd[p + "attn.qkv.bias"].chunk(3, 0)
        hf.update({q + "attention.attention.query.weight": wq, q + "attention.attention.query.bias": bq,
                   q + "attention.attention.key.weight": wk, q + "attention.attention.key.bias": bk,
                   q + "attention.attention.value.weight": wv, q + "attention.attention.value.bias": bv,
                   q + "attention.output.dense.weight": sd[p + "attn.proj.weight"], q + "attention.output.dense.bias": sd[p + "attn.proj.bias"],
                   q + "layer_scale1.lambda1": sd[p + "ls1.gamma"], q + "layer_scale2.lambda1": sd[p + "ls2.gamma"]})
        for n in ("norm1", "norm2"):
            hf[q + n + ".weight"], hf[q + n + ".bias"] = sd[p + n + ".weight"], sd[p + n + ".bias"]
        names = (("w12", "weights_in"), ("w3", "weights_out")) if p + "mlp.w12.weight" in sd else (("fc1", "fc1"), ("fc2", "fc2"))
        for a, b in names:
            hf[q + f"mlp.{b}.weight"], hf[q + f"mlp.{b}.bias"] = sd[p + f"mlp.{a}.weight"], sd[p + f"mlp.{a}.bias"]
    return hf
