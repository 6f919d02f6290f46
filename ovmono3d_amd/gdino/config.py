"""Architecture record of the GroundingDINO network the engine runs (defaults = reference configs/GroundingDINO_SwinB_cfg.py:
Swin-B, BERT-base, 6 / 6 layers, 900 queries; IDEA-Research/GroundingDINO @856dde2). ``GDinoConfig.swin_t()`` is the record of
upstream's GroundingDINO_SwinT_OGC.py (groundingdino_swint_ogc.pth): the same transformer on a Swin-T backbone. A checkpoint names
its own architecture: ``GDinoConfig.from_state_dict`` reads the record off the tensors' shapes."""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Dict, Sequence


@dataclass
class GDinoConfig:
    d_model: int = 256
    enc_layers: int = 6
    dec_layers: int = 6
    heads: int = 8
    ffn_dim: int = 2048
    n_levels: int = 4
    n_points: int = 4
    num_queries: int = 900
    max_text_len: int = 256
    pe_temperature: float = 20.0
    eps: float = 1e-5
    bert_heads: int = 12
    swin_embed: int = 128
    swin_depths: Sequence[int] = (2, 2, 18, 2)
    swin_heads: Sequence[int] = (4, 8, 16, 32)
    swin_window: int = 12

    @classmethod
    def swin_t(cls, **kw) -> "GDinoConfig":
        """Swin-T backbone (swin_T_224_1k): embed 96, depths 2/2/6/2, heads 3/6/12/24, window 7; everything else as Swin-B's record."""
        return cls(**{**dict(swin_embed=96, swin_depths=(2, 2, 6, 2), swin_heads=(3, 6, 12, 24), swin_window=7), **kw})

    @classmethod
    def from_state_dict(cls, sd: Dict[str, object]) -> "GDinoConfig":
        """The record of a checkpoint in the Hugging Face port's names (after ``convert_upstream_state_dict``), read off its tensors.
        What no tensor carries keeps the published value: 4 sampling points per level, max_text_len, pe_temperature, eps, and a
        head dimension of 64 in BERT (bert_heads = hidden / 64: right for bert-base, the text encoder of both published checkpoints;
        a network with another head dimension needs its record passed). BERT's layer count, hidden size and vocabulary are not
        fields of the record: the loader counts and reads them off the tensors itself (load_bert, gdino_load.hip). Raises ValueError naming the key for a missing tensor or a Swin stage the engine cannot run."""
        sw = "model.backbone.conv_encoder.model.swin."

        def shape(key: str):
            if key not in sd:
                raise ValueError(f"GroundingDINO checkpoint: missing tensor {key!r}")
            return tuple(int(d) for d in sd[key].shape)

        def count(pattern: str) -> int:
            rx = re.compile(pattern)
            found = {int(m.group(1)) for m in (rx.match(k) for k in sd) if m}
            return max(found) + 1 if found else 0

        embed = shape(sw + "embeddings.patch_embeddings.projection.weight")[0]
        n_stages = count(re.escape(sw) + r"encoder\.layers\.(\d+)\.blocks\.0\.layernorm_before\.weight")
        if n_stages != 4:                                       # the engine's record and its neck are built for the four stages
            raise ValueError(f"GroundingDINO checkpoint: {n_stages} Swin stages under {sw + 'encoder.layers'!r}, the engine runs 4")
        depths, heads, window = [], [], None
        for i in range(n_stages):
            depth = count(re.escape(f"{sw}encoder.layers.{i}.blocks.") + r"(\d+)\.layernorm_before\.weight")
            C = embed << i
            for j in range(depth):
                key = f"{sw}encoder.layers.{i}.blocks.{j}.attention.relative_position_bias.relative_position_bias_table"
                rows, nh = shape(key)
                side = math.isqrt(rows)
                if side * side != rows or side % 2 == 0:
                    raise ValueError(f"{key}: {rows} rows are not (2 w - 1)^2 for any window side w")
                w = (side + 1) // 2
                if window is None:
                    window = w
                if w != window:
                    raise ValueError(f"{key}: window side {w}, but {window} in the blocks before it")
                if j == 0:
                    heads.append(nh)
                if nh != heads[i]:
                    raise ValueError(f"{key}: {nh} heads, but {heads[i]} in the stage's first block")
                if nh <= 0 or C % nh or C // nh not in (16, 32, 64):
                    raise ValueError(f"{key}: {nh} heads over {C} channels give head dimension {C / max(nh, 1):g}; the engine runs 16, 32 and 64")
                qk = f"{sw}encoder.layers.{i}.blocks.{j}.attention.q_proj.weight"
                if shape(qk) != (C, C):
                    raise ValueError(f"{qk}: shape {shape(qk)}, expected {(C, C)} in stage {i} of embed {embed}")
            depths.append(depth)
        d_model = shape("model.level_embed")[1]
        n_levels = shape("model.level_embed")[0]
        n_points = cls.n_points
        aw = "model.encoder.layers.0.deformable_layer.self_attn.attention_weights.weight"
        n_samp = shape(aw)[0]
        if n_samp % (n_levels * n_points):
            raise ValueError(f"{aw}: {n_samp} rows are not heads x {n_levels} levels x {n_points} points")
        bert_hidden = shape("model.text_backbone.embeddings.word_embeddings.weight")[1]
        return cls(
            d_model=d_model,
            enc_layers=count(r"model\.encoder\.layers\.(\d+)\.deformable_layer\.fc1\.weight"),
            dec_layers=count(r"model\.decoder\.layers\.(\d+)\.fc1\.weight"),
            heads=n_samp // (n_levels * n_points),
            ffn_dim=shape("model.encoder.layers.0.deformable_layer.fc1.weight")[0],
            n_levels=n_levels, n_points=n_points,
            num_queries=shape("model.query_position_embeddings.weight")[0],
            bert_heads=max(1, bert_hidden // 64),
            swin_embed=embed, swin_depths=tuple(depths), swin_heads=tuple(heads), swin_window=window)
