"""Test-side patches that make the Hugging Face GroundingDINO port (transformers 5.x) compute what upstream
IDEA-Research/GroundingDINO @856dde2 computes, in the three places where the port departs from it. Used by the
GPU parity tests and by bench.py's cpu_baseline / parity leg; never imported by the product package.

The patches follow the model's dtype: an fp32 model computes exactly what it did when they were written for fp32 only; a model
converted with .double() (the float64 reference of the long-caption tests) gets its mask and its sine embedding in float64."""
from __future__ import annotations

import contextlib
import math

import torch


def _sine_embedding(pos: torch.Tensor, num_pos_feats: int = 128, temperature: int = 10000) -> torch.Tensor:
    """encode_sinusoidal_position_embedding of the port, every step in pos.dtype (the port builds its frequency table in fp32)"""
    dim_t = torch.arange(num_pos_feats, dtype=pos.dtype, device=pos.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    emb = [c[..., None] * (2 * math.pi) / dim_t for c in pos.unbind(-1)]
    emb = [torch.stack((e[..., 0::2].sin(), e[..., 1::2].cos()), dim=-1).flatten(-2) for e in emb]
    if len(emb) >= 2:
        emb[0], emb[1] = emb[1], emb[0]
    return torch.cat(emb, dim=-1)


def patch_hf_to_upstream(hf):
    """(1) transformers 5.x's BertModel adds a 4-D bool mask as +1.0 (nothing is masked); upstream builds the additive mask
    (get_extended_attention_mask): feed HF what upstream computes. (3) encode_sinusoidal_position_embedding casts its result
    back to the input dtype, which truncates the text position embedding of int64 position ids to integers; upstream
    (get_sine_pos_embed) keeps floats."""
    import transformers.models.grounding_dino.modeling_grounding_dino as mgd
    tb = hf.model.text_backbone
    if not getattr(tb, "_ovm_patched", False):
        orig = tb.forward

        def patched(input_ids, attention_mask=None, token_type_ids=None, position_ids=None, **kw):
            dtype = next(tb.parameters()).dtype
            mgd._ovm_model_dtype = dtype                        # the text backbone runs first: integer position ids follow it below
            if attention_mask is not None and attention_mask.dtype == torch.bool:
                attention_mask = torch.where(attention_mask, 0.0, torch.finfo(torch.float32).min).to(dtype)
            return orig(input_ids, attention_mask, token_type_ids, position_ids, **kw)
        tb.forward = patched
        tb._ovm_patched = True
    if not getattr(mgd, "_ovm_patched", False):
        orig_enc = mgd.encode_sinusoidal_position_embedding

        def patched_enc(pos, **kw):
            dtype = pos.dtype if pos.dtype.is_floating_point else getattr(mgd, "_ovm_model_dtype", torch.float32)
            if dtype == torch.float32:
                return orig_enc(pos.float(), **kw)
            return _sine_embedding(pos.to(dtype), **kw)
        mgd.encode_sinusoidal_position_embedding = patched_enc
        mgd._ovm_patched = True
    return hf


@contextlib.contextmanager
def upstream_position_ids():
    """(2) HF numbers the text positions its own way (the '.' delimiters get position 0); upstream - which the native path
    follows - numbers them 0..len inside each phrase, delimiter included. Inside this context HF uses upstream's ids."""
    import transformers.models.grounding_dino.modeling_grounding_dino as mgd
    from pyref_gdino.bert import masks_and_position_ids
    orig = mgd.generate_masks_with_special_tokens_and_transfer_map
    mgd.generate_masks_with_special_tokens_and_transfer_map = \
        lambda ids: (orig(ids)[0], masks_and_position_ids(ids[0].cpu())[1][None].to(ids.device))
    try:
        yield
    finally:
        mgd.generate_masks_with_special_tokens_and_transfer_map = orig
