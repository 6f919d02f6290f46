"""ctypes binding of libovm3d.so (the C ABI declared in include/ovm3d.h).

The library is built in-tree by ``ovmono3d_amd/csrc/build.sh`` (``__graft_entry__.build()``).
There is no CPU or PyTorch fallback: if the shared object is missing or fails to load,
importing the native path raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libovm3d.so")

OVM_REC_FLOATS = 48


class OvmConfig(C.Structure):
    _fields_ = [
        ("embed_dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32),
        ("pos_grid", C.c_int32), ("canvas", C.c_int32), ("fpn_channels", C.c_int32),
        ("use_depth_fusion", C.c_int32),
        ("pixel_mean", C.c_float * 3), ("pixel_std", C.c_float * 3),
        ("num_classes", C.c_int32), ("fc_dim", C.c_int32), ("pooler_res", C.c_int32),
        ("pooler_min_level", C.c_int32), ("pooler_max_level", C.c_int32),
        ("virtual_focal", C.c_float),
        ("anchor_sizes", C.c_float * 4), ("anchor_ratios", C.c_float * 3),
        ("rpn_pre_topk", C.c_int32), ("rpn_post_topk", C.c_int32), ("rpn_nms_thresh", C.c_float),
        ("score_thresh", C.c_float), ("nms_thresh", C.c_float), ("detections_per_image", C.c_int32),
        ("precision", C.c_int32), ("max_batch", C.c_int32), ("max_rois", C.c_int32),
        ("tower", C.c_int32), ("sam_window", C.c_int32), ("sam_global_mask", C.c_uint32),
    ]


OVM_TOWER_DINOV2, OVM_TOWER_CLIP, OVM_TOWER_MAE, OVM_TOWER_MIDAS, OVM_TOWER_SAM = 0, 1, 2, 3, 4


class OvmTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class OvmImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32),
                ("stride_c", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64),
                ("orig_height", C.c_int32), ("orig_width", C.c_int32), ("K", C.c_float * 9)]


class OvmGdinoConfig(C.Structure):
    _fields_ = [
        ("d_model", C.c_int32), ("enc_layers", C.c_int32), ("dec_layers", C.c_int32), ("heads", C.c_int32), ("ffn_dim", C.c_int32),
        ("n_levels", C.c_int32), ("n_points", C.c_int32), ("num_queries", C.c_int32), ("max_text_len", C.c_int32),
        ("pe_temperature", C.c_float), ("eps", C.c_float), ("bert_heads", C.c_int32),
        ("swin_embed", C.c_int32), ("swin_depths", C.c_int32 * 4), ("swin_heads", C.c_int32 * 4), ("swin_window", C.c_int32),
        ("pixel_mean", C.c_float * 3), ("pixel_std", C.c_float * 3), ("flip_channels", C.c_int32), ("precision", C.c_int32),
        ("use_graphs", C.c_int32), ("max_plans", C.c_int32), ("plan_budget_mb", C.c_int32),
    ]


class OvmJpegInfo(C.Structure):
    """Mirror of include/ovm3d.h OvmJpegInfo."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hmax", C.c_int32), ("vmax", C.c_int32),
        ("h", C.c_int32 * 3), ("v", C.c_int32 * 3), ("bw", C.c_int32 * 3), ("bh", C.c_int32 * 3), ("cw", C.c_int32 * 3),
        ("ch", C.c_int32 * 3), ("qidx", C.c_int32 * 3), ("colorspace", C.c_int32), ("coef_blocks", C.c_int32),
        ("qt", (C.c_uint16 * 64) * 4),
    ]


class OvmJpegEncInfo(C.Structure):
    """Mirror of include/ovm3d.h OvmJpegEncInfo."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("quality", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
        ("bw", C.c_int32 * 3), ("bh", C.c_int32 * 3), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("coef_blocks", C.c_int32),
        ("header_len", C.c_int32), ("qt", (C.c_uint16 * 64) * 2),
    ]


class OvmJpegDecPlan(C.Structure):
    """Mirror of include/ovm3d.h OvmJpegDecPlan."""
    _fields_ = [
        ("info", OvmJpegInfo), ("ecs_offset", C.c_int64), ("ecs_bytes", C.c_int64), ("restart_interval", C.c_int32),
        ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("blocks_per_mcu", C.c_int32), ("segments", C.c_int32),
        ("sub_bits", C.c_int32), ("wg_subs", C.c_int32), ("sync_launches", C.c_int32), ("max_rounds", C.c_int32),
        ("tables_bytes", C.c_int32), ("sel_comp", C.c_uint8 * 8), ("sel_sub", C.c_uint8 * 8), ("sel_dc", C.c_uint8 * 8),
        ("sel_ac", C.c_uint8 * 8),
    ]


OVM_SCENE_MAX_BOXES = 1024
OVM_SCENE_FRONT, OVM_SCENE_NOVEL = 1, 2


class OvmSceneInput(C.Structure):
    """Mirror of include/ovm3d.h OvmSceneInput."""
    _fields_ = [
        ("n_boxes", C.c_int32), ("mode", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("scale", C.c_int32),
        ("has_T", C.c_int32), ("has_ground_bounds", C.c_int32), ("has_labels", C.c_int32),
        ("K", C.c_double * 9), ("R", C.c_double * 9), ("T", C.c_double * 3), ("ground_bounds", C.c_double * 5),
        ("blend_weight", C.c_double), ("blend_weight_overlay", C.c_double), ("zplane", C.c_double),
        ("corners", C.c_void_p), ("colors", C.c_void_p), ("label_size", C.c_void_p),
    ]


class OvmSceneBox(C.Structure):
    _fields_ = [
        ("verts", (C.c_double * 3) * 8), ("edge", (C.c_int64 * 4) * 12), ("edge_drawn", C.c_int32 * 12),
        ("rect", C.c_int32 * 4), ("text_org", C.c_int32 * 2), ("label_w", C.c_int32), ("label_h", C.c_int32),
    ]


class OvmSceneView(C.Structure):
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("thickness", C.c_int32), ("drawn", C.c_int32),
        ("K", C.c_double * 9), ("order", C.c_int32 * OVM_SCENE_MAX_BOXES), ("box", OvmSceneBox * OVM_SCENE_MAX_BOXES),
    ]


class OvmSceneLayout(C.Structure):
    """Mirror of include/ovm3d.h OvmSceneLayout."""
    _fields_ = [
        ("n_boxes", C.c_int32), ("mode", C.c_int32), ("early_return", C.c_int32),
        ("grid_thickness", C.c_int32), ("n_grid", C.c_int32), ("reserved", C.c_int32),
        ("zoom_factor", C.c_double), ("zoom_bias", C.c_double), ("center", C.c_double * 3), ("ground", C.c_double * 5),
        ("blend_weight", C.c_double), ("blend_weight_overlay", C.c_double), ("zplane", C.c_double),
        ("edge_color", (C.c_double * 3) * OVM_SCENE_MAX_BOXES), ("edge_u8", (C.c_uint8 * 4) * OVM_SCENE_MAX_BOXES),
        ("color", (C.c_float * 3) * OVM_SCENE_MAX_BOXES), ("view", OvmSceneView * 2),
    ]


class OvmSceneSegment(C.Structure):
    _fields_ = [("x0", C.c_int64), ("y0", C.c_int64), ("x1", C.c_int64), ("y1", C.c_int64)]


OVM_PANELS = 6
OVM_PANEL_SEGMENT, OVM_PANEL_BLEND, OVM_PANEL_GLYPH = 0, 1, 2


class OvmPanelBox(C.Structure):
    """Mirror of include/ovm3d.h OvmPanelBox."""
    _fields_ = [
        ("bbox", C.c_double * 4), ("center", C.c_double * 3), ("dims", C.c_double * 3), ("R", C.c_double * 9),
        ("color", C.c_uint8 * 4), ("draw3d", C.c_int32), ("in_eval", C.c_int32),
        ("glyph2d", C.c_int32 * 2), ("glyph3d", C.c_int32 * 2),
    ]


class OvmPanelsInput(C.Structure):
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("n_gt", C.c_int32), ("n_pred", C.c_int32),
        ("K", C.c_double * 9), ("gt", C.c_void_p), ("pred", C.c_void_p),
    ]


class OvmPanelPrim(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("thickness", C.c_int32), ("a", C.c_int64 * 4), ("glyph_offset", C.c_int64),
        ("color", C.c_uint8 * 4), ("box", C.c_int32),
    ]


class OvmPanelsLayout(C.Structure):
    """Mirror of include/ovm3d.h OvmPanelsLayout."""
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("thickness3d", C.c_int32), ("n_prims", C.c_int32),
        ("start", C.c_int32 * (OVM_PANELS + 1)), ("reserved", C.c_int32), ("glyph_bytes", C.c_int64),
    ]


# include/ovm3d.h OVM_NHD_*: the per-detection status ovm_eval_nhd writes
OVM_NHD_NONE, OVM_NHD_OK, OVM_NHD_SKIPPED = 0, 1, 2


class OvmEvalCell(C.Structure):
    """Mirror of include/ovm3d.h OvmEvalCell."""
    _fields_ = [("iou_off", C.c_int64), ("dt_off", C.c_int32), ("n_dt", C.c_int32), ("gt_off", C.c_int32), ("n_gt", C.c_int32),
                ("prox", C.c_int32), ("reserved", C.c_int32)]


OVM_GEO_OK, OVM_GEO_EMPTY, OVM_GEO_TOO_FEW, OVM_GEO_NONFINITE, OVM_GEO_RECT_OUTSIDE, OVM_GEO_COUNT_MISMATCH, OVM_GEO_BAD_PERM = range(7)


class OvmGeoParams(C.Structure):
    """Mirror of include/ovm3d.h OvmGeoParams."""
    _fields_ = [("eps0", C.c_double), ("min_cluster_frac", C.c_double), ("accept_frac", C.c_double),
                ("min_samples", C.c_int32), ("max_points", C.c_int32), ("trials", C.c_int32), ("min_cluster", C.c_int32),
                ("last_stage", C.c_int32), ("reserved", C.c_int32)]


class OvmGeoInstance(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("perm", C.c_void_p), ("rect", C.c_int32 * 4), ("n_points", C.c_int32), ("reserved", C.c_int32)]


class OvmGeoResult(C.Structure):
    _fields_ = [("offset", C.c_double * 3), ("yaw", C.c_double), ("ext_min", C.c_double * 3), ("ext_max", C.c_double * 3),
                ("eps", C.c_double), ("n_points", C.c_int32), ("n_used", C.c_int32), ("n_kept", C.c_int32), ("trial", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class OvmGeoBox(C.Structure):
    _fields_ = [("center_cam", C.c_double * 3), ("dimensions", C.c_double * 3), ("pose", C.c_double * 9), ("center_2D", C.c_double * 2),
                ("depth", C.c_double), ("bbox3D", (C.c_float * 3) * 8)]


class OvmSamConfig(C.Structure):
    """Mirror of include/ovm3d.h OvmSamConfig."""
    _fields_ = [
        ("embed_dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32), ("patch", C.c_int32), ("pos_grid", C.c_int32),
        ("window", C.c_int32), ("global_mask", C.c_uint32), ("image_size", C.c_int32), ("prompt_dim", C.c_int32),
        ("dec_depth", C.c_int32), ("dec_heads", C.c_int32), ("dec_mlp", C.c_int32), ("attn_downsample", C.c_int32),
        ("num_mask_tokens", C.c_int32), ("iou_depth", C.c_int32), ("iou_hidden", C.c_int32),
        ("pixel_mean", C.c_float * 3), ("pixel_std", C.c_float * 3), ("precision", C.c_int32), ("max_boxes", C.c_int32),
    ]


class OvmDepthProConfig(C.Structure):
    """Mirror of include/ovm3d.h OvmDepthProConfig."""
    _fields_ = [
        ("embed_dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32), ("patch", C.c_int32), ("crop", C.c_int32),
        ("hook_ids", C.c_int32 * 2), ("fusion_dim", C.c_int32), ("scaled_dims", C.c_int32 * 3), ("inter_dims", C.c_int32 * 2),
        ("ratios", C.c_float * 3), ("overlaps", C.c_float * 3), ("merge_padding", C.c_int32), ("num_fov_layers", C.c_int32),
        ("use_fov", C.c_int32), ("precision", C.c_int32), ("ln_eps", C.c_float),
    ]



class OvmGemmEpiOp(C.Structure):
    """Mirror of include/ovm3d.h OvmGemmEpiOp (ovm_op_gemm_epi: one fused GEMM epilogue in isolation, for tests)."""
    _fields_ = [
        ("epi", C.c_int32), ("amode", C.c_int32), ("precision", C.c_int32), ("a_il", C.c_int32), ("route", C.c_int32),
        ("ksplit_hint", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("cH", C.c_int32), ("cW", C.c_int32), ("cC", C.c_int32),
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p),
        ("gamma", C.c_void_p), ("X", C.c_void_p), ("row_map", C.c_void_p), ("ldx", C.c_int32), ("relu", C.c_int32),
        ("C", C.c_void_p), ("ldc", C.c_int32), ("ldo", C.c_int32),
        ("O", C.c_void_p), ("o_elems", C.c_int64), ("o_il", C.c_int32), ("relu_o", C.c_int32),
        ("R", C.c_void_p), ("R2", C.c_void_p), ("ldr", C.c_int32), ("ldr2", C.c_int32), ("padH", C.c_int32), ("padW", C.c_int32),
        ("Q", C.c_void_p), ("Kout", C.c_void_p), ("Vt", C.c_void_p), ("T", C.c_int32), ("Tpad", C.c_int32), ("heads", C.c_int32),
        ("qscale", C.c_float),
        ("pos", C.c_void_p), ("G2", C.c_int32), ("G", C.c_int32), ("Cout", C.c_int32), ("reserved", C.c_int32),
    ]


class OvmAttnF32Op(C.Structure):
    """Mirror of include/ovm3d.h OvmAttnF32Op (ovm_g_attn_f32: attn_f32_kernel in isolation, for tests)."""
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32),
        ("reserved0", C.c_int32),
        ("sq1", C.c_int64), ("sq2", C.c_int64), ("sk1", C.c_int64), ("sk2", C.c_int64), ("sv1", C.c_int64), ("sv2", C.c_int64),
        ("o", C.c_void_p), ("ldo", C.c_int32), ("reserved1", C.c_int32), ("so1", C.c_int64), ("so2", C.c_int64),
        ("ohi", C.c_void_p), ("olo", C.c_void_p), ("ldoh", C.c_int32), ("reserved2", C.c_int32), ("soh1", C.c_int64), ("soh2", C.c_int64),
        ("nb1", C.c_int32), ("nb2", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32), ("DH", C.c_int32), ("scale", C.c_float),
        ("bias_h", C.c_void_p), ("sbh", C.c_int64), ("ldbh", C.c_int32), ("reserved3", C.c_int32),
        ("bias_b", C.c_void_p), ("sbb", C.c_int64), ("ldbb", C.c_int32), ("reserved4", C.c_int32),
        ("rel_h", C.c_void_p), ("rel_w", C.c_void_p), ("rel_gw", C.c_int32), ("ldrel", C.c_int32),
    ]


class OvmMsDeformOp(C.Structure):
    """Mirror of include/ovm3d.h OvmMsDeformOp (ovm_g_msdeform_fused: the fused deformable-attention kernels in isolation, for tests)."""
    _fields_ = [
        ("value", C.c_void_p), ("ow", C.c_void_p), ("ref", C.c_void_p), ("ldv", C.c_int32), ("ldow", C.c_int32), ("ldref", C.c_int32),
        ("mode", C.c_int32),
        ("Q", C.c_int32), ("H", C.c_int32), ("dh", C.c_int32), ("L", C.c_int32), ("P", C.c_int32), ("reserved0", C.c_int32),
        ("lh", C.c_int32 * 8), ("lw", C.c_int32 * 8), ("lstart", C.c_int32 * 8),
        ("out", C.c_void_p), ("ohi", C.c_void_p), ("olo", C.c_void_p), ("ldo", C.c_int32), ("ldoh", C.c_int32),
    ]


class OvmRowOp(C.Structure):
    """Mirror of include/ovm3d.h OvmRowOp (ovm_g_rowop: rowop_kernel in isolation, for tests)."""
    _fields_ = [
        ("x", C.c_void_p), ("idx", C.c_void_p), ("res", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("add", C.c_void_p),
        ("ldx", C.c_int32), ("nidx", C.c_int32), ("seg", C.c_int32), ("ldr", C.c_int32), ("eps", C.c_float),
        ("zero_masked", C.c_int32), ("ld_add", C.c_int32), ("add_rows", C.c_int32),
        ("M", C.c_int32), ("D", C.c_int32),
        ("y", C.c_void_p), ("y2", C.c_void_p), ("hi", C.c_void_p), ("lo", C.c_void_p), ("hi2", C.c_void_p), ("lo2", C.c_void_p),
        ("ldy", C.c_int32), ("ldy2", C.c_int32), ("ldh", C.c_int32), ("il", C.c_int32), ("ldh2", C.c_int32), ("reserved0", C.c_int32),
    ]


class OvmSwinQkvAttnOp(C.Structure):
    """Mirror of include/ovm3d.h OvmSwinQkvAttnOp (ovm_g_swin_qkv_attn: the Swin qkv + window-attention kernels in isolation, for tests)."""
    _fields_ = [
        ("xhi", C.c_void_p), ("xlo", C.c_void_p), ("wfrag", C.c_void_p), ("bias", C.c_void_p), ("relbias", C.c_void_p), ("mask", C.c_void_p),
        ("ohi", C.c_void_p), ("olo", C.c_void_p),
        ("ldx", C.c_int32), ("KS", C.c_int32), ("C", C.c_int32), ("nh", C.c_int32), ("nW", C.c_int32), ("ldo", C.c_int32),
        ("scale", C.c_float), ("ws", C.c_int32), ("wpg", C.c_int32), ("reserved0", C.c_int32),
    ]


class OvmChainLin(C.Structure):
    """Mirror of include/ovm3d.h OvmChainLin: one linear of the decoder row chains (fragment-ordered split image, bias, N, K, Kpad)."""
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32), ("Kpad", C.c_int32), ("reserved0", C.c_int32)]


class OvmChainLn(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p)]


class OvmDecChainOp(C.Structure):
    """Mirror of include/ovm3d.h OvmDecChainOp (ovm_g_dec_chain: the decoder row-chain kernels in isolation, for tests)."""
    LIN = ("ref0", "ref1", "sa_qk", "sa_v", "sa_out", "ca_q", "ca_out", "offw", "msda_out", "fc1", "fc2", "bb0", "bb1", "bb2")
    _fields_ = [
        ("Q", C.c_int32), ("D", C.c_int32), ("T", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32), ("eps", C.c_float),
        ("hs", C.c_void_p), ("ref", C.c_void_p), ("sine_dim_t", C.c_void_p), ("ref_next", C.c_void_p), ("qpos", C.c_void_p),
        ("qk", C.c_void_p), ("v", C.c_void_p), ("ctx", C.c_void_p),
        ("tk", C.c_void_p), ("tv", C.c_void_p), ("val", C.c_void_p), ("ldt", C.c_int32), ("ldv", C.c_int32),
        ("L", C.c_int32), ("P", C.c_int32), ("lh", C.c_int32 * 8), ("lw", C.c_int32 * 8), ("lstart", C.c_int32 * 8),
        ("lin", OvmChainLin * 14), ("ln", OvmChainLn * 4),
        ("ffn_split", C.c_int32), ("reserved0", C.c_int32), ("ffn_x", C.c_void_p), ("ffn_part", C.c_void_p),
    ]


EXPORTS = [
    "ovm_create", "ovm_destroy", "ovm_last_error", "ovm_version", "ovm_abi_sizeof", "ovm_backbone_forward", "ovm_cube_forward",
    "ovm_rpn_box_forward", "ovm_gather_records", "ovm_gather_counts", "ovm_host_interp_pos_embed", "ovm_host_resize_pos_embed_aa", "ovm_host_sincos_pos_embed", "ovm_host_shard_range",
    "ovm_backbone_num_levels", "ovm_backbone_level",
    "ovm_op_split_f16", "ovm_op_interleave", "ovm_op_gemm", "ovm_op_gemm_epi", "ovm_op_mlp_fused", "ovm_op_gemm_swiglu", "ovm_host_swiglu_perm", "ovm_op_layernorm", "ovm_op_attention", "ovm_op_roi_align",
    "ovm_op_roi_align_ex", "ovm_op_compact_records", "ovm_op_ln_rows", "ovm_op_ln_gelu_split", "ovm_op_patch_gather", "ovm_op_patch_gather_f32",
    "ovm_op_cls_init", "ovm_op_tokens_cast", "ovm_op_tokens_writeback", "ovm_op_maxpool2",
    "ovm_op_cube_decode", "ovm_op_nms", "ovm_op_rpn_proposals", "ovm_op_boxhead_post", "ovm_debug_copy", "ovm_set_corun", "ovm_profile_enable", "ovm_profile_read",
    "ovm_comm_unique_id", "ovm_comm_init", "ovm_comm_destroy", "ovm_tune_set", "ovm_gdino_postprocess", "ovm_box3d_iou", "ovm_eval_iou2d", "ovm_eval_match", "ovm_eval_iou3d", "ovm_eval_nhd", "ovm_host_pil_bilinear_coeffs", "ovm_resize_bilinear_u8", "ovm_resize_bilinear_f32",
    "ovm_g_pack_weight", "ovm_host_pack_weight", "ovm_g_linear", "ovm_g_layernorm", "ovm_g_bmm", "ovm_g_bmm2", "ovm_g_softmax", "ovm_g_softmax2", "ovm_g_eltwise", "ovm_g_gather_rows",
    "ovm_g_groupnorm", "ovm_g_biattn", "ovm_g_msdeform", "ovm_g_sine_embed", "ovm_g_normalize_image", "ovm_g_topk", "ovm_g_rowmax",
    "ovm_g_attn_f32", "ovm_g_msdeform_fused", "ovm_g_rowop", "ovm_g_swin_qkv_attn",
    "ovm_host_frag_order", "ovm_g_dec_chain", "ovm_host_dec_chain_supported",
    "ovm_gdino_create", "ovm_gdino_destroy", "ovm_gdino_last_error", "ovm_gdino_forward", "ovm_gdino_detect", "ovm_gdino_set_force_topk",
    "ovm_gdino_debug_copy", "ovm_debug_set_ptr", "ovm_gdino_num_queries", "ovm_gdino_last_outputs", "ovm_infer", "ovm_infer_depth",
    "ovm_host_jpeg_info", "ovm_host_jpeg_entropy_decode", "ovm_jpeg_reconstruct",
    "ovm_host_jpeg_decode_plan", "ovm_jpeg_entropy_decode_workspace", "ovm_jpeg_entropy_decode", "ovm_host_jpeg_entropy_emulate",
    "ovm_host_jpeg_encode_plan", "ovm_jpeg_encode_workspace", "ovm_jpeg_forward", "ovm_jpeg_encode",
    "ovm_host_scene_layout", "ovm_render_scene_workspace", "ovm_render_scene", "ovm_render_scene_points_workspace", "ovm_render_scene_points",
    "ovm_host_panels_layout", "ovm_render_panels_workspace", "ovm_render_panels",
    "ovm_geo_default_params", "ovm_geo_last_error", "ovm_geo_lift_workspace", "ovm_geo_lift", "ovm_geo_dbscan_workspace", "ovm_geo_dbscan",
    "ovm_host_geo_box",
    "ovm_sam_create", "ovm_sam_destroy", "ovm_sam_last_error", "ovm_sam_set_image", "ovm_sam_predict_boxes_workspace", "ovm_sam_predict_boxes",
    "ovm_sam_debug_copy", "ovm_sam_predict_workspace", "ovm_sam_predict", "ovm_sam_mask_boxes",
    "ovm_depthpro_create", "ovm_depthpro_destroy", "ovm_depthpro_last_error", "ovm_depthpro_workspace", "ovm_depthpro_infer",
    "ovm_depthpro_debug_copy", "ovm_host_depthpro_check", "ovm_depthpro_profile_enable", "ovm_depthpro_stage_ms",
    "ovm_op_sam_dense_pe", "ovm_op_sam_box_tokens", "ovm_op_sam_ln_gelu", "ovm_op_sam_i2t_attn", "ovm_op_sam_mask_prod", "ovm_op_sam_mask_out",
    "ovm_op_sam_unpatch", "ovm_op_sam_iou_slice", "ovm_op_sam_add_bcast", "ovm_op_sam_i2t_attn16", "ovm_op_sam_point_tokens", "ovm_op_sam_mask_embed",
    "ovm_op_dp_pyramid", "ovm_op_dp_merge", "ovm_op_dp_unsplit", "ovm_op_dp_conv_s2", "ovm_op_dp_dot", "ovm_op_dp_head_tail",
    "ovm_op_dp_clear_borders", "ovm_op_dp_depth_out",
]
PROF_NAMES = ("attn", "qkv", "proj", "fc1", "fc2", "ln")

_lib = None


def load() -> C.CDLL:
    """Load libovm3d.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with ovmono3d_amd/csrc/build.sh (or __graft_entry__.build()). "
            "The native HIP path has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.ovm_create.argtypes = [C.POINTER(OvmConfig), C.POINTER(OvmTensor), i32, i32, C.POINTER(vp)]
    lib.ovm_destroy.argtypes = [vp]
    lib.ovm_last_error.argtypes = [vp]
    lib.ovm_last_error.restype = C.c_char_p
    lib.ovm_version.restype = C.c_char_p
    lib.ovm_abi_sizeof.argtypes = [C.c_char_p]
    for name, mirror in (("OvmConfig", OvmConfig), ("OvmTensor", OvmTensor), ("OvmImage", OvmImage), ("OvmGdinoConfig", OvmGdinoConfig),
                         ("OvmJpegInfo", OvmJpegInfo), ("OvmJpegEncInfo", OvmJpegEncInfo), ("OvmJpegDecPlan", OvmJpegDecPlan), ("OvmSceneInput", OvmSceneInput), ("OvmSceneLayout", OvmSceneLayout),
                         ("OvmSceneSegment", OvmSceneSegment), ("OvmPanelBox", OvmPanelBox), ("OvmPanelsInput", OvmPanelsInput),
                         ("OvmPanelPrim", OvmPanelPrim), ("OvmPanelsLayout", OvmPanelsLayout), ("OvmEvalCell", OvmEvalCell), ("OvmGeoParams", OvmGeoParams),
                         ("OvmGeoInstance", OvmGeoInstance), ("OvmGeoResult", OvmGeoResult), ("OvmGeoBox", OvmGeoBox),
                         ("OvmSamConfig", OvmSamConfig), ("OvmDepthProConfig", OvmDepthProConfig), ("OvmGemmEpiOp", OvmGemmEpiOp),
                         ("OvmAttnF32Op", OvmAttnF32Op), ("OvmMsDeformOp", OvmMsDeformOp), ("OvmRowOp", OvmRowOp),
                         ("OvmSwinQkvAttnOp", OvmSwinQkvAttnOp), ("OvmDecChainOp", OvmDecChainOp)):
        if lib.ovm_abi_sizeof(name.encode()) != C.sizeof(mirror):
            raise RuntimeError(f"{LIB_PATH}: sizeof({name}) = {lib.ovm_abi_sizeof(name.encode())} but the ctypes mirror has "
                               f"{C.sizeof(mirror)} bytes - rebuild the library (ovmono3d_amd/csrc/build.sh) or update lib.py")
    lib.ovm_host_jpeg_info.argtypes = [vp, C.c_size_t, C.POINTER(OvmJpegInfo)]
    lib.ovm_host_jpeg_entropy_decode.argtypes = [vp, C.c_size_t, vp, i64, C.POINTER(OvmJpegInfo)]
    lib.ovm_jpeg_reconstruct.argtypes = [vp, C.POINTER(OvmJpegInfo), vp, vp, vp]
    lib.ovm_host_jpeg_decode_plan.argtypes = [vp, C.c_size_t, i32, C.POINTER(OvmJpegDecPlan), vp, i64]
    lib.ovm_jpeg_entropy_decode_workspace.argtypes = [C.POINTER(OvmJpegDecPlan), C.POINTER(i64)]
    lib.ovm_jpeg_entropy_decode.argtypes = [vp, vp, C.POINTER(OvmJpegDecPlan), vp, i64, vp, i64, vp, vp]
    lib.ovm_host_jpeg_entropy_emulate.argtypes = [vp, C.c_size_t, i32, vp, i64, C.POINTER(OvmJpegInfo), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.ovm_host_jpeg_encode_plan.argtypes = [i32, i32, i32, i32, C.POINTER(OvmJpegEncInfo), vp, i32]
    lib.ovm_jpeg_encode_workspace.argtypes = [C.POINTER(OvmJpegEncInfo), C.POINTER(i64), C.POINTER(i64)]
    lib.ovm_jpeg_forward.argtypes = [vp, i64, i64, i64, C.POINTER(OvmJpegEncInfo), vp, i64, vp, vp]
    lib.ovm_jpeg_encode.argtypes = [vp, i64, i64, i64, C.POINTER(OvmJpegEncInfo), vp, vp, i64, vp, i64, vp, vp]
    lib.ovm_host_scene_layout.argtypes = [C.POINTER(OvmSceneInput), C.POINTER(OvmSceneLayout), vp, i32]
    lib.ovm_render_scene_workspace.argtypes = [C.POINTER(OvmSceneLayout), i64, C.POINTER(i64)]
    lib.ovm_render_scene.argtypes = [C.POINTER(OvmSceneLayout), vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    lib.ovm_render_scene_points_workspace.argtypes = [C.POINTER(OvmSceneLayout), i64, C.POINTER(i64)]
    lib.ovm_render_scene_points.argtypes = [C.POINTER(OvmSceneLayout), vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64,
                                            C.POINTER(C.c_double * 9), i32, vp, vp, i64, vp]
    lib.ovm_host_panels_layout.argtypes = [C.POINTER(OvmPanelsInput), C.POINTER(OvmPanelsLayout), vp, i32]
    lib.ovm_render_panels_workspace.argtypes = [C.POINTER(OvmPanelsLayout), C.POINTER(i64)]
    lib.ovm_render_panels.argtypes = [C.POINTER(OvmPanelsLayout), vp, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    lib.ovm_backbone_forward.argtypes = [vp, C.POINTER(OvmImage), i32, vp, i32, i32, vp, vp, vp, vp]
    lib.ovm_cube_forward.argtypes = [vp, C.POINTER(OvmImage), i32, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ovm_rpn_box_forward.argtypes = [vp, C.POINTER(OvmImage), i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ovm_gather_records.argtypes = [vp, i32, i32, vp, i32, vp, C.POINTER(i32), vp]
    lib.ovm_gather_counts.argtypes = [vp, i32, i32, i32, C.POINTER(i32), vp]
    lib.ovm_host_interp_pos_embed.argtypes = [vp, i32, i32, i32, vp]
    lib.ovm_host_resize_pos_embed_aa.argtypes = [vp, i32, i32, i32, vp]
    lib.ovm_host_sincos_pos_embed.argtypes = [i32, i32, vp]
    lib.ovm_backbone_num_levels.argtypes = [vp]
    lib.ovm_backbone_level.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(f32)]
    lib.ovm_host_shard_range.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.ovm_op_split_f16.argtypes = [vp, i64, vp, vp, vp]
    lib.ovm_op_interleave.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.ovm_op_gemm.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, vp, i32, vp, i32, i32, vp]
    lib.ovm_op_gemm_epi.argtypes = [C.POINTER(OvmGemmEpiOp), vp]
    lib.ovm_op_mlp_fused.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp]
    lib.ovm_op_gemm_swiglu.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, vp]
    lib.ovm_host_swiglu_perm.argtypes = [i32, vp]
    lib.ovm_op_layernorm.argtypes = [vp, i32, i32, vp, vp, f32, vp, vp]
    lib.ovm_op_attention.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    lib.ovm_op_roi_align.argtypes = [vp, vp, vp, C.POINTER(i32), C.POINTER(f32), i32, i32, i32, i32, vp, vp, i32, vp, vp]
    lib.ovm_op_cube_decode.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(OvmImage), i32, i32, f32, i32, vp, vp, vp]
    lib.ovm_op_roi_align_ex.argtypes = [C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(f32), i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp]
    lib.ovm_op_compact_records.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    lib.ovm_op_ln_rows.argtypes = [vp, i32, i32, i32, vp, vp, f32, vp, i32, vp, vp, i32, i32, i32, i32, vp]
    lib.ovm_op_ln_gelu_split.argtypes = [vp, vp, i32, i32, vp, vp, f32, vp]
    lib.ovm_op_patch_gather.argtypes = [C.POINTER(OvmImage), i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), vp, vp, vp]
    lib.ovm_op_patch_gather_f32.argtypes = [C.POINTER(i64), i32, i32, i32, vp, vp, vp]
    lib.ovm_op_cls_init.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ovm_op_tokens_cast.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ovm_op_tokens_writeback.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.ovm_op_maxpool2.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.ovm_op_nms.argtypes = [vp, vp, i32, f32, vp, vp, vp]
    lib.ovm_op_rpn_proposals.argtypes = [C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32),
                                         C.POINTER(OvmImage), i32, i32, i32, f32, vp, vp, vp, vp]
    lib.ovm_op_boxhead_post.argtypes = [vp, i32, vp, vp, C.POINTER(OvmImage), i32, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ovm_debug_copy.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.ovm_debug_copy.restype = i64
    lib.ovm_profile_enable.argtypes = [vp, i32]
    lib.ovm_set_corun.argtypes = [vp, i32]
    lib.ovm_profile_read.argtypes = [vp, C.POINTER(f32), C.POINTER(i32)]
    lib.ovm_comm_unique_id.argtypes = [vp]
    lib.ovm_comm_init.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.ovm_comm_destroy.argtypes = [vp]
    lib.ovm_tune_set.argtypes = [C.c_char_p, i32]
    lib.ovm_debug_set_ptr.argtypes = [C.c_char_p, vp]
    lib.ovm_host_pil_bilinear_coeffs.argtypes = [i32, i32, vp, vp, i32]
    lib.ovm_resize_bilinear_u8.argtypes = [vp, i32, i32, i32, i64, i64, i64, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.ovm_resize_bilinear_f32.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    lib.ovm_box3d_iou.argtypes = [vp, vp, i32, i32, f32, f32, vp, vp, vp]
    lib.ovm_eval_iou2d.argtypes = [vp, vp, i32, vp, vp, C.c_double, vp, vp, vp]
    lib.ovm_eval_match.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.ovm_eval_iou3d.argtypes = [vp, vp, i32, vp, vp, f32, f32, vp, vp]
    lib.ovm_eval_nhd.argtypes = [vp, vp, i32, i32, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ovm_geo_default_params.argtypes = [C.POINTER(OvmGeoParams)]
    lib.ovm_geo_last_error.argtypes = []
    lib.ovm_geo_last_error.restype = C.c_char_p
    lib.ovm_geo_lift_workspace.argtypes = [C.POINTER(OvmGeoInstance), i32, i32, i32, C.POINTER(OvmGeoParams), C.POINTER(i64), C.POINTER(i64)]
    lib.ovm_geo_lift.argtypes = [vp, i32, i32, C.POINTER(C.c_double), C.POINTER(OvmGeoInstance), i32, C.POINTER(OvmGeoParams), vp, vp, vp, i64, vp]
    lib.ovm_geo_dbscan_workspace.argtypes = [i32, C.POINTER(i64)]
    lib.ovm_geo_dbscan.argtypes = [vp, i32, C.c_double, i32, vp, vp, i64, vp]
    lib.ovm_host_geo_box.argtypes = [C.POINTER(OvmGeoResult), C.POINTER(C.c_double), C.POINTER(OvmGeoBox)]
    lib.ovm_sam_create.argtypes = [C.POINTER(OvmSamConfig), C.POINTER(OvmTensor), i32, i32, C.POINTER(vp)]
    lib.ovm_sam_destroy.argtypes = [vp]
    lib.ovm_sam_last_error.argtypes = [vp]
    lib.ovm_sam_last_error.restype = C.c_char_p
    lib.ovm_sam_set_image.argtypes = [vp, C.POINTER(OvmImage), i32, vp]
    lib.ovm_sam_predict_boxes_workspace.argtypes = [vp, i32, C.POINTER(i64)]
    lib.ovm_sam_predict_boxes.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.ovm_sam_debug_copy.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.ovm_sam_debug_copy.restype = i64
    lib.ovm_sam_predict_workspace.argtypes = [vp, i32, i32, i32, i32, C.POINTER(i64)]
    lib.ovm_sam_predict.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.ovm_sam_mask_boxes.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.ovm_depthpro_create.argtypes = [C.POINTER(OvmDepthProConfig), C.POINTER(OvmTensor), i32, i32, C.POINTER(vp)]
    lib.ovm_depthpro_destroy.argtypes = [vp]
    lib.ovm_depthpro_last_error.argtypes = [vp]
    lib.ovm_depthpro_last_error.restype = C.c_char_p
    lib.ovm_depthpro_workspace.argtypes = [vp, i32, i32, C.POINTER(i64)]
    lib.ovm_depthpro_infer.argtypes = [vp, C.POINTER(OvmImage), i32, f32, vp, vp, vp, vp, i64, vp]
    lib.ovm_depthpro_debug_copy.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.ovm_depthpro_debug_copy.restype = i64
    lib.ovm_depthpro_profile_enable.argtypes = [vp, i32]
    lib.ovm_depthpro_stage_ms.argtypes = [vp, vp, i32]
    lib.ovm_host_depthpro_check.argtypes = [C.POINTER(OvmDepthProConfig), C.c_char_p, i32]
    lib.ovm_op_sam_dense_pe.argtypes = [vp, i32, i32, vp, vp]
    lib.ovm_op_sam_box_tokens.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ovm_op_sam_ln_gelu.argtypes = [vp, i64, i32, vp, vp, f32, vp]
    lib.ovm_op_sam_i2t_attn.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp, i32, vp]
    lib.ovm_op_sam_mask_prod.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, i64, vp]
    lib.ovm_op_sam_mask_out.argtypes = [vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.ovm_op_sam_unpatch.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.ovm_op_sam_iou_slice.argtypes = [vp, i32, i32, vp, vp]
    lib.ovm_op_sam_add_bcast.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.ovm_op_sam_i2t_attn16.argtypes = lib.ovm_op_sam_i2t_attn.argtypes
    lib.ovm_op_sam_point_tokens.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ovm_op_sam_mask_embed.argtypes = [vp, i32, i32, i32] + [vp] * 12
    lib.ovm_op_dp_pyramid.argtypes = [vp, i32, i32, i64, i64, i64, i32, i32, vp, vp, vp, vp]
    lib.ovm_op_dp_merge.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ovm_op_dp_unsplit.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ovm_op_dp_conv_s2.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.ovm_op_dp_dot.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.ovm_op_dp_head_tail.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    lib.ovm_op_dp_clear_borders.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32, vp]
    lib.ovm_op_dp_depth_out.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp, vp, vp]
    lib.ovm_g_pack_weight.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.ovm_host_pack_weight.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.ovm_g_linear.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, vp]
    lib.ovm_g_layernorm.argtypes = [vp, vp, i32, i32, vp, vp, f32, vp, vp]
    lib.ovm_g_bmm.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i32, f32, vp]
    lib.ovm_g_bmm2.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i64, i32, f32, vp]
    lib.ovm_g_softmax2.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, i32, vp]
    lib.ovm_g_softmax.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32, vp]
    lib.ovm_g_eltwise.argtypes = [i32, vp, vp, vp, i64, i64, f32, f32, vp]
    lib.ovm_g_gather_rows.argtypes = [vp, i32, vp, i64, i32, i32, vp, vp]
    lib.ovm_g_groupnorm.argtypes = [vp, i32, i32, i32, i32, vp, vp, f32, vp, vp]
    lib.ovm_g_msdeform.argtypes = [vp, C.POINTER(i32), i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ovm_g_biattn.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, i32, vp, i32, vp]
    lib.ovm_g_sine_embed.argtypes = [vp, i64, i32, i32, f32, vp, vp]
    lib.ovm_g_normalize_image.argtypes = [C.POINTER(OvmImage), C.POINTER(f32), C.POINTER(f32), i32, vp, vp]
    lib.ovm_g_topk.argtypes = [vp, i32, i32, vp, vp]
    lib.ovm_g_rowmax.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.ovm_g_attn_f32.argtypes = [C.POINTER(OvmAttnF32Op), vp]
    lib.ovm_g_msdeform_fused.argtypes = [C.POINTER(OvmMsDeformOp), vp]
    lib.ovm_g_rowop.argtypes = [C.POINTER(OvmRowOp), vp]
    lib.ovm_g_swin_qkv_attn.argtypes = [C.POINTER(OvmSwinQkvAttnOp), vp]
    lib.ovm_host_frag_order.argtypes = [vp, i32, i32, vp]
    lib.ovm_g_dec_chain.argtypes = [C.POINTER(OvmDecChainOp), i32, vp]
    lib.ovm_host_dec_chain_supported.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    lib.ovm_gdino_postprocess.argtypes = [vp, i32, i32, vp, C.POINTER(i32), i32, i32, i32, f32, f32, vp, vp, vp, vp, vp]
    lib.ovm_gdino_create.argtypes = [C.POINTER(OvmGdinoConfig), C.POINTER(OvmTensor), i32, i32, C.POINTER(vp)]
    lib.ovm_gdino_destroy.argtypes = [vp]
    lib.ovm_gdino_last_error.argtypes = [vp]
    lib.ovm_gdino_last_error.restype = C.c_char_p
    lib.ovm_gdino_forward.argtypes = [vp, C.POINTER(OvmImage), C.POINTER(i32), i32, C.POINTER(i32), vp, vp, vp]
    lib.ovm_gdino_detect.argtypes = [vp, C.POINTER(OvmImage), C.POINTER(i32), i32, C.POINTER(i32), i32, f32, f32, vp, vp, vp, vp, vp]
    lib.ovm_gdino_set_force_topk.argtypes = [vp, vp]
    lib.ovm_gdino_debug_copy.argtypes = [vp, C.c_char_p, vp, i64, vp]
    lib.ovm_gdino_debug_copy.restype = i64
    lib.ovm_gdino_num_queries.argtypes = [vp]
    lib.ovm_gdino_last_outputs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
    lib.ovm_infer.argtypes = [vp, vp, C.POINTER(OvmImage), C.POINTER(i32), i32, C.POINTER(i32), i32, f32, f32, vp, i32, C.POINTER(i32), vp]
    lib.ovm_infer_depth.argtypes = [vp, vp, C.POINTER(OvmImage), vp, i32, i32, C.POINTER(i32), i32, C.POINTER(i32), i32, f32, f32, vp, i32,
                                    C.POINTER(i32), vp]
    for name in EXPORTS:
        if name not in ("ovm_last_error", "ovm_version", "ovm_debug_copy", "ovm_gdino_last_error", "ovm_gdino_debug_copy", "ovm_geo_last_error",
                        "ovm_sam_last_error", "ovm_sam_debug_copy", "ovm_depthpro_last_error", "ovm_depthpro_debug_copy"):
            getattr(lib, name).restype = i32
    # experiment knobs, e.g. OVM_TUNE="gemm_bm=256,attn_tail=0"
    for kv in filter(None, os.environ.get("OVM_TUNE", "").split(",")):
        k, _, v = kv.partition("=")
        lib.ovm_tune_set(k.strip().encode(), int(v))
    _lib = lib
    return lib


class OvmError(RuntimeError):
    pass


def check(rc: int, handle=None, what: str = "") -> None:
    if rc == 0:
        return
    msg = ""
    if handle:
        msg = (load().ovm_last_error(handle) or b"").decode()
    raise OvmError(f"{what} failed with code {rc}: {msg}")


def make_tensor_table(state_dict: Dict[str, "np.ndarray"]):
    """state_dict values: contiguous float32 numpy arrays (host). Returns (ctypes array, keepalive)."""
    items = list(state_dict.items())
    arr = (OvmTensor * len(items))()
    keep = []
    for i, (k, v) in enumerate(items):
        v = np.ascontiguousarray(v, dtype=np.float32)
        if v.ndim > 4:
            raise ValueError(f"{k}: more than 4 dims")
        kb = k.encode()
        keep.append((kb, v))
        arr[i].name = kb
        arr[i].data = v.ctypes.data
        arr[i].ndim = v.ndim
        for d in range(v.ndim):
            arr[i].shape[d] = v.shape[d]
    return arr, keep


def shard_range(n: int, rank: int, world: int):
    b, e = C.c_int64(), C.c_int64()
    check(load().ovm_host_shard_range(n, rank, world, C.byref(b), C.byref(e)), what="ovm_host_shard_range")
    return b.value, e.value


def interp_pos_embed(pos: "np.ndarray", G: int) -> "np.ndarray":
    """pos [1+M*M, D] float32 -> [1+G*G, D] (host, no GPU needed)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    M = int(round((pos.shape[0] - 1) ** 0.5))
    out = np.empty((1 + G * G, pos.shape[1]), dtype=np.float32)
    check(load().ovm_host_interp_pos_embed(pos.ctypes.data, M, pos.shape[1], G, out.ctypes.data),
          what="ovm_host_interp_pos_embed")
    return out
