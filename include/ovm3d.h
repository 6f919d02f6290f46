/*
 * libovm3d - C ABI of the MI355X-native OVMono3D-LIFT inference path.
 *
 * The reference (nightgoodl/ovmono3d) is pure Python and has no FFI; the entry points below are the
 * native equivalents of the Python plugin surface it exposes for this path. Each one cites the
 * reference interface it replaces. All pointers are plain pointers, all sizes plain integers; no
 * torch / C++ types cross the boundary. Device pointers are HIP device memory of the device the
 * handle was created on. Functions return 0 on success and a negative OVM_ERR_* code otherwise and
 * never throw; ovm_last_error() returns a message for the last failure on a handle.
 *
 * Threading: a handle is not thread-safe; use one handle per (device, stream). All work is
 * stream-ordered on the caller's stream; functions do not synchronise unless documented.
 * Ownership: the caller owns every input/output buffer; the handle owns packed weights + workspace
 * (sized at create for max_batch / max_rois) and allocates nothing on the hot path.
 */
#ifndef OVM3D_H
#define OVM3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVM_OK 0
#define OVM_ERR_INVALID (-1)
#define OVM_ERR_HIP (-2)
#define OVM_ERR_MISSING_WEIGHT (-3)
#define OVM_ERR_SHAPE (-4)
#define OVM_ERR_CAPACITY (-5)
#define OVM_ERR_UNSUPPORTED (-6) /* a valid input outside the documented scope of the call (e.g. a CMYK JPEG) */

#define OVM_REC_FLOATS 48 /* detection record width, see OvmDet3D */

typedef struct OvmHandle OvmHandle;
typedef void* ovm_stream_t; /* hipStream_t */

/* Model / path configuration: the inference-relevant keys of the reference config tree
 * (cubercnn/config/config.py:80-92,118-239; configs/Base.yaml; configs/OVMono3D_dinov2_SFP.yaml). */
typedef struct OvmConfig {
  /* MODEL.DINO.MODEL_NAME table, reference cubercnn/modeling/backbone/dino.py:17-24 */
  int32_t embed_dim, depth, heads;
  int32_t pos_grid;         /* sqrt(#pretrained position embeddings) (37 for the 518px hub models) */
  int32_t canvas;           /* MODEL.FPN.SQUARE_PAD (OVMono3D_dinov2_SFP.yaml:37), multiple of 14 */
  int32_t fpn_channels;     /* MODEL.FPN.OUT_CHANNELS */
  int32_t use_depth_fusion; /* MODEL.DINO.USE_DEPTH_FUSION (config.py:92) */
  float pixel_mean[3];      /* MODEL.PIXEL_MEAN in tensor channel order */
  float pixel_std[3];
  /* ROI heads */
  int32_t num_classes;      /* MODEL.ROI_HEADS.NUM_CLASSES */
  int32_t fc_dim;           /* ROI_BOX_HEAD.FC_DIM / ROI_CUBE_HEAD.FC_DIM */
  int32_t pooler_res;       /* 7 */
  int32_t pooler_min_level, pooler_max_level; /* ROIPooler level clamp */
  float virtual_focal;      /* ROI_CUBE_HEAD.VIRTUAL_FOCAL */
  /* RPN + box head (reference configs/Base.yaml:45-66) */
  float anchor_sizes[4];    /* one size per pyramid level (3 levels: the 4th is unused) */
  float anchor_ratios[3];
  int32_t rpn_pre_topk, rpn_post_topk;
  float rpn_nms_thresh;
  float score_thresh, nms_thresh;
  int32_t detections_per_image;
  /* build-specific */
  int32_t precision;        /* 1 = fp16 operands, one MFMA pass; 3 = split fp16 (hi+lo), three passes */
  int32_t max_batch, max_rois;
  /* Which ViT feeds the simple feature pyramid (MODEL.BACKBONE.NAME):
   *   OVM_TOWER_DINOV2 (0)  build_dino_backbone, reference cubercnn/modeling/backbone/dino.py:17-153: hub DINOv2, patch 14,
   *                         LayerScale, erf-GELU, LN eps 1e-6, pos-embed bicubic with the +0.1 offset; pyramid scales (2, 1, 0.5)
   *                         -> p2..p4 at strides 7 / 14 / 28; checkpoint keys backbone.net.vit.*
   *                         Two variants of the hub's model table are selected by the checkpoint, not by this struct:
   *                         - register tokens (vit*14_reg): key backbone.net.vit.register_tokens [1][R][D], R <= 16. Sequence = class,
   *                           R registers, patches (T = 1 + R + G^2); the registers get no position row; the position table is
   *                           resized with antialiased bicubic and no offset (the hub builds these models with
   *                           interpolate_offset = 0, interpolate_antialias = True); prompt_depth is refused (the reference's
   *                           fusion takes x[:, 1:] as the patch tokens, dino.py:91-105)
   *                         - SwiGLU FFN (vitg14): keys blocks.N.mlp.w12.{weight [2 Hs][D], bias}, mlp.w3.{weight [D][Hs], bias}
   *                           instead of mlp.fc1 / mlp.fc2; Hs = w12 rows / 2 (4096 for ViT-g), at most 4 D after padding to 32.
   *                           y = w3(silu(h[:Hs]) * h[Hs:]), h = w12(LN2(x)). Both or neither of w12 / fc1 present: refused
   *   OVM_TOWER_CLIP   (1)  build_clip_backbone, reference cubercnn/modeling/backbone/clip.py:17-166: open_clip VisionTransformer
   *                         image tower (conv1 without bias, class_embedding, ln_pre, QuickGELU, LN eps 1e-5, no ln_post / proj),
   *                         patch 16, pos-embed resized with antialiased bicubic (:98-133); pyramid scales (4, 2, 1, 0.5)
   *                         -> p2..p5 at strides 4 / 8 / 16 / 32; checkpoint keys backbone.net.visual.*; prompt_depth refused
   *                         (detectron2's SimpleFeaturePyramid.forward takes no depth: SURVEY.md 0.4).
   *   OVM_TOWER_MAE    (2)  build_mae_backbone, reference cubercnn/modeling/backbone/mae.py:20-150: Hugging Face ViTMAE encoder
   *                         (patch 16 with bias, separate query / key / value linears, erf-GELU, LN eps 1e-12, no LayerScale),
   *                         position embeddings = fixed 2-D sin-cos table rebuilt for the canvas grid (:62-78,152-180), class token
   *                         + its (zero) position row, tap = hidden_states[depth] i.e. `depth` blocks are run - the reference taps
   *                         hidden_states[num_layers - 1], the state BEFORE the last block (:43-55,110-116), so depth = 11 for
   *                         vit-mae-base; same 4-level pyramid and prompt_depth rule as CLIP; keys backbone.net.vit.embeddings.*,
   *                         backbone.net.vit.encoder.layer.N.*
   *   OVM_TOWER_MIDAS  (3)  build_midas_backbone, reference cubercnn/modeling/backbone/midas_final.py:19-95: the ViT-L/16 of MiDaS
   *                         DPT_Large (timm vit_large_patch16_384: patch 16 with bias, class token, plain pre-norm blocks without
   *                         LayerScale, erf-GELU, LN eps 1e-6, norm_pre = identity, no final norm), position table of the 24 x 24
   *                         grid resized with the CLIP tower's antialiased bicubic (:64-66); checkpoint keys backbone.net.vit.*
   *                         in timm's naming (cls_token, pos_embed, patch_embed.proj, blocks.N.{norm1,attn.qkv,attn.proj,norm2,
   *                         mlp.fc1,mlp.fc2}); same 4-level pyramid and prompt_depth rule as CLIP
   *   OVM_TOWER_SAM    (4)  build_sam_backbone, reference cubercnn/modeling/backbone/sam.py:19-112: segment_anything's ImageEncoderViT
   *                         blocks (no class token; patch 16 with bias; absolute position table [grid][grid][D], bicubic-resized when
   *                         the canvas grid differs, :73-86; blocks with 14 x 14 windowed attention over the zero-padded grid except
   *                         the global ones; decomposed relative-position bias from the query content; erf-GELU, LN eps 1e-6), dense
   *                         output of the last block, the neck unused; keys backbone.net.vit.{pos_embed, patch_embed.proj,
   *                         blocks.N.{norm1, attn.qkv, attn.proj, attn.rel_pos_h, attn.rel_pos_w, norm2, mlp.lin1, mlp.lin2}};
   *                         pos_grid = the checkpoint's grid (64); sam_window / sam_global_mask below */
  int32_t tower;
  int32_t sam_window;        /* OVM_TOWER_SAM: window side of the windowed blocks (14) */
  uint32_t sam_global_mask;  /* OVM_TOWER_SAM: bit i set = block i attends globally (vit_b: blocks 2, 5, 8, 11) */
} OvmConfig;

enum { OVM_TOWER_DINOV2 = 0, OVM_TOWER_CLIP = 1, OVM_TOWER_MAE = 2, OVM_TOWER_MIDAS = 3, OVM_TOWER_SAM = 4 };

/* One host-resident fp32 tensor of a checkpoint, named with the reference state_dict key
 * (module tree printed at reference nohup.out:563-684; loaded at reference demo/demo.py:148). */
typedef struct OvmTensor {
  const char* name;
  const float* data;
  int32_t ndim;
  int64_t shape[4];
} OvmTensor;

/* One input image: the per-image dict of the reference (demo/demo.py:82-85, dataset_mapper.py:72):
 * 'image' uint8 at network resolution (any C/H/W element strides: CHW dict tensors and native NHWC both
 * work without a copy), 'height'/'width' (original), 'K'. */
typedef struct OvmImage {
  const uint8_t* data;      /* device pointer */
  int32_t height, width;    /* network resolution */
  int64_t stride_c, stride_h, stride_w;
  int32_t orig_height, orig_width;
  float K[9];
} OvmImage;

/* Detection record, 48 x 4 bytes (fields of detectron2 Instances as filled at reference
 * cubercnn/modeling/roi_heads/roi_heads.py:823-843 and consumed at omni3d_evaluation.py:1219-1249). */
typedef struct OvmDet3D {
  float box[4];        /* pred_boxes xyxy, original resolution (after detector_postprocess) */
  float score;         /* sqrt(score2d * exp(-uncertainty)) */
  int32_t category;    /* pred_classes */
  float bbox3D[24];    /* 8 corners x (x,y,z), camera space */
  float center_cam[3];
  float center_2D[2];  /* original-resolution pixels */
  float dimensions[3]; /* W, H, L */
  float pose[9];       /* row-major 3x3, egocentric */
  int32_t image;       /* index into the call's image array */
} OvmDet3D;

/* --- lifecycle ---------------------------------------------------------------------------------
 * Replaces build_model(cfg) + DetectionCheckpointer.resume_or_load (reference rcnn3d.py:252-276,
 * demo/demo.py:144-150): packs the named fp32 tensors into device-resident fp16(-split) GEMM layouts. */
int ovm_create(const OvmConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmHandle** out);
int ovm_destroy(OvmHandle* h);
const char* ovm_last_error(const OvmHandle* h);
const char* ovm_version(void);
/* sizeof() of a struct of this header as the library was compiled: every `typedef struct X { ... } X;` here answers to "X", the
 * nested ones (OvmSceneBox, OvmChainLin, ...) included; -1 for an unknown name. Lets a binding check its view of the layout before
 * the first call. */
int ovm_abi_sizeof(const char* struct_name);

/* --- backbone: build_dino_backbone(...).forward(x, prompt_depth) -> {p2,p3,p4}
 * (reference dino.py:70-120,123-153,208-224; preprocess_image folded in, rcnn3d.py:88).
 * images: host array of B descriptors. prompt_depth: device fp32 [B][1][depth_h][depth_w] or NULL.
 * p2/p3/p4: device fp32 NHWC outputs [B][S/7][S/7][C], [B][S/14]..., [B][S/28]... or NULL to keep
 * the features only inside the handle (ovm_cube_forward / ovm_rpn_box_forward read them there). */
int ovm_backbone_forward(OvmHandle* h, const OvmImage* images, int32_t B, const float* prompt_depth,
                         int32_t depth_h, int32_t depth_w, float* p2, float* p3, float* p4, ovm_stream_t stream);

/* The pyramid the handle holds after ovm_backbone_forward, level by level (0 = finest, "p2"): number of levels (3 or 4 by
 * tower), and for one level its device pointer (fp32 NHWC [max_batch][side][side][fpn_channels], valid until the next forward
 * or ovm_destroy), side and stride in pixels. The 4-level towers' p5 is read this way. */
int ovm_backbone_num_levels(const OvmHandle* h);
int ovm_backbone_level(const OvmHandle* h, int32_t level, const float** data, int32_t* side, float* stride);

/* --- ROIHeads3D._forward_cube, eval branch (reference roi_heads.py:329-549,798-848) followed by
 * GeneralizedRCNN._postprocess (rcnn3d.py:115). Uses the features of the last ovm_backbone_forward.
 * boxes [n][4] xyxy at network resolution, scores [n], classes [n] int32, image_idx [n] int32 (sorted by
 * image), all device. out: device [n] records; out_counts: device int32 [B] kept detections per image
 * (records of empty post-processed boxes are dropped, order preserved). postprocess = 0 keeps every record
 * with its network-resolution box (RCNN3D.inference(do_postprocess=False), rcnn3d.py:113-117). */
int ovm_cube_forward(OvmHandle* h, const OvmImage* images, int32_t B, const float* boxes, const float* scores,
                     const int32_t* classes, const int32_t* image_idx, int32_t n, int32_t postprocess, OvmDet3D* out,
                     int32_t* out_counts, ovm_stream_t stream);

/* --- RPN inference + ROIHeads3D._forward_box + FastRCNNOutputs.inference
 * (reference rcnn3d.py:106, rpn.py:19-39 -> detectron2 RPN; roi_heads.py:252-296; fast_rcnn.py:57-143).
 * Outputs up to detections_per_image rows per image, image-major: boxes [B*topk][4] network res,
 * scores, classes, image_idx, and scores_full [B*topk][num_classes] (may be NULL); out_counts int32 [B]. */
int ovm_rpn_box_forward(OvmHandle* h, const OvmImage* images, int32_t B, float* boxes, float* scores,
                        int32_t* classes, int32_t* image_idx, float* scores_full, int32_t* out_counts,
                        ovm_stream_t stream);

/* --- detection gather over RCCL: replaces comm.gather(inference_json, dst=0)
 * (reference omni3d_evaluation.py:717-720). comm is an ncclComm_t. counts_all (host, world ints) is
 * filled on every rank; recv (device) must hold sum(counts_all) records on rank 0. */
int ovm_gather_records(void* comm, int32_t rank, int32_t world, const OvmDet3D* send, int32_t n_send,
                       OvmDet3D* recv, int32_t* counts_all, ovm_stream_t stream);

/* The counts exchange alone, so that rank 0 can size `recv` first: every rank calls it, then every rank calls
 * ovm_gather_records (which repeats the 4-byte exchange). counts_all: host, world ints, filled on every rank. */
int ovm_gather_counts(void* comm, int32_t rank, int32_t world, int32_t n_send, int32_t* counts_all, ovm_stream_t stream);

int ovm_comm_unique_id(uint8_t* id128);                                     /* ncclGetUniqueId */
int ovm_comm_init(const uint8_t* id128, int32_t rank, int32_t world, int32_t device, void** comm);
int ovm_comm_destroy(void* comm);

/* --- per-kernel timing with HIP events recorded on the stream the kernels are launched on (what
 * bench.py's roofline figure is computed from). Categories index the ms/launches arrays. */
#define OVM_PROF_ATTN 0
#define OVM_PROF_QKV 1
#define OVM_PROF_PROJ 2
#define OVM_PROF_FC1 3
#define OVM_PROF_FC2 4
#define OVM_PROF_LN 5
#define OVM_PROF_NCAT 6
/* Co-run mode: tells the handle that the caller runs other work on a second stream while ovm_backbone_forward executes (the
 * GroundingDINO detector of ROIHeads3DGDINO). The attention launches then keep to one workgroup per CU so that the other stream's
 * short kernels find free wave slots. Scheduling only: results are unchanged. */
int ovm_set_corun(OvmHandle* handle, int32_t on);

int ovm_profile_enable(OvmHandle* h, int32_t on); /* 0 off, 1 every category, else bit (c + 1) selects category c (attn, qkv, proj, fc1, fc2, ln) */
int ovm_profile_read(OvmHandle* h, float* ms /* [OVM_PROF_NCAT] */, int32_t* launches /* [OVM_PROF_NCAT] */);

/* --- host-side helpers (no GPU needed) -------------------------------------------------------- */
/* dinov2 interpolate_pos_encoding (hub: offset 0.1, bicubic, no antialias): pos [1+M*M][D] -> out [1+G*G][D] */
int ovm_host_interp_pos_embed(const float* pos, int32_t M, int32_t D, int32_t G, float* out);
/* resize_pos_embed of the CLIP tower (reference cubercnn/modeling/backbone/clip.py:98-133): F.interpolate(size=(G,G), bicubic,
 * align_corners=False, antialias=True) of the patch rows, class row kept: pos [1+M*M][D] -> out [1+G*G][D] */
int ovm_host_resize_pos_embed_aa(const float* pos, int32_t M, int32_t D, int32_t G, float* out);
/* get_2d_sincos_pos_embed(D, (G, G), add_cls_token=True) of the MAE tower (reference cubercnn/modeling/backbone/mae.py:152-180 over
 * transformers' get_2d_sincos_pos_embed_from_grid): out [1+G*G][D], row 0 zero; first D/2 columns encode the x coordinate, the
 * rest y, each as [sin | cos] over D/4 frequencies 10000^(-i/(D/4)); computed in double, stored fp32 */
int ovm_host_sincos_pos_embed(int32_t D, int32_t G, float* out);
/* Row order of the w12 image ovm_op_gemm_swiglu / the engine stream: perm[n], n < 2 * ceil32(Hs), is the row of the checkpoint's
 * w12 [2 Hs][K] (gates [0, Hs), values [Hs, 2 Hs)) that packed row n holds, or -1 for a zero row. Packed rows [32 q, 32 q + 16) are the
 * gates of outputs 16 q .. 16 q + 15, rows [32 q + 16, 32 q + 32) their values. */
int ovm_host_swiglu_perm(int32_t Hs, int32_t* perm /* [2 * ceil32(Hs)] */);
/* InferenceSampler contiguous shard [begin,end) of rank (reference cubercnn/data/build.py:320) */
int ovm_host_shard_range(int64_t n_items, int32_t rank, int32_t world, int64_t* begin, int64_t* end);

/* --- kernel-level entry points (parity tests and micro-benchmarks call the same kernels the model
 * path launches). All pointers device; "split" fp16 tensors are a hi array and an optional lo array
 * (x ~= hi + lo). */
int ovm_op_split_f16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, ovm_stream_t stream);
int ovm_op_gemm(const uint16_t* a_hi, const uint16_t* a_lo, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo,
                int32_t M, int32_t N, int32_t K, const float* bias, int32_t relu, float* c, int32_t ldc,
                int32_t precision, ovm_stream_t stream);
/* The fused first linear of a SwiGLU FFN (dinov2 SwiGLUFFNFused.w12) with the activation in the GEMM epilogue:
 *   out[m][j] = silu(a[m] . Wg[j] + bg[j]) * (a[m] . Wu[j] + bu[j]),  j < Hs, computed in fp32 and stored as a split fp16 image
 * of Kp = ceil32(Hs) columns whose columns [Hs, Kp) are written as zeros (the K padding of the next linear).
 * The weight image holds 2 Kp rows in the order of ovm_host_swiglu_perm (blocks of 16 gate rows | 16 value rows, so one lane of the
 * MFMA epilogue owns gate j and value j), padded with zero rows to a multiple of 128 rows (256 when the op_gemm256 tune key forces the
 * 256 x 256 kernel; its split-K hint is ignored: this epilogue never runs split over K); bias [2 Kp] in the same order or null.
 * Operand layouts as ovm_op_gemm. out_lo = out_hi + 32 selects the interleaved image (ldo >= 2 Kp), otherwise plain arrays (ldo >= Kp). */
int ovm_op_gemm_swiglu(const uint16_t* a_hi, const uint16_t* a_lo, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo,
                       int32_t M, int32_t Hs, int32_t K, const float* bias, uint16_t* out_hi, uint16_t* out_lo, int32_t ldo,
                       int32_t precision, ovm_stream_t stream);
/* One fused GEMM epilogue in isolation (test-only): out = epilogue(A W^T), launched exactly as the model path launches it. All
 * pointers are fp32 device tensors; the adapter pads W to 256 rows, converts A and W to the (split, interleaved) fp16 operand
 * images, and for amode 1 builds the zero-bordered image of the un-bordered NHWC input A [B][cH][cW][cC] (M = B cH cW, K = 9 cC,
 * W columns ordered (dy*3 + dx)*cC + c). Outputs are fp32 buffers in the kernel's own layout, which the caller pre-fills (a value
 * that is exact in fp16 survives wherever the kernel does not write): fp16 destinations are split from the caller's buffer before
 * the launch and joined back after it.
 *   epi 0 store : C [M][ldc] and / or O with row stride ldo; relu 0 none | 1 ReLU | 2 GELU(erf); + R [M][ldr] + R2 [M][ldr2] after the
 *                 activation; relu_o: O receives relu(value); padH > 0: row (b, y, x) of O goes to the interior of a bordered
 *                 [B][padH+2][padW+2] image
 *   epi 1 resid : X[row_map ? row_map[m] : m][n] += (gamma ? gamma[n] : 1) * (acc + bias[n]), negative rows dropped
 *   epi 2 gelu  : O = gelu(acc + bias) (relu 3: QuickGELU); o_il: O is the interleaved image [M][ldo = 2N] of hi and lo halves,
 *                 returned element by element (hi at column il(n) = (n/32)*64 + n%32, lo 32 further)
 *   epi 3 qkv   : N = 3 heads 64; Q (scaled by qscale), Kout [B][heads][T][64], Vt [B][heads][64][Tpad] with the token order of the
 *                 attention kernel (bits 2 and 3 of the token index swapped inside each group of 16)
 *   epi 4 patch : X[b*T + (T - G2) + p][n] = acc + bias[n] + pos[((T > G2) + p)*N + n], m = b*G2 + p
 *   epi 5 convt : 2x2 stride-2 scatter, n = (a*2 + bb)*Cout + co -> O pixel (2i + a, 2j + bb) of [B][2G][2G], pixel stride ldo
 *                 (0: Cout), padH > 0: the interior of a [B][2G+2][2G+2] image
 * precision 1 | 3 (3: split operands; a_il: A as an interleaved image as well). route 0: launch_gemm; 1: the 256 x 256 kernel with
 * split-K hint ksplit_hint. Routes inside launch_gemm follow the gemm_* tune keys. Invalid combinations return the launcher's code. */
typedef struct OvmGemmEpiOp {
  int32_t epi, amode, precision, a_il, route, ksplit_hint;
  int32_t M, N, K, cH, cW, cC;
  const float* A; const float* W; const float* bias;
  const float* gamma; float* X; const int32_t* row_map; int32_t ldx, relu;
  float* C; int32_t ldc, ldo;
  float* O; int64_t o_elems; int32_t o_il, relu_o;
  const float* R; const float* R2; int32_t ldr, ldr2, padH, padW;
  float* Q; float* Kout; float* Vt; int32_t T, Tpad, heads; float qscale;
  const float* pos; int32_t G2, G, Cout, reserved;
} OvmGemmEpiOp;
int ovm_op_gemm_epi(const OvmGemmEpiOp* op, ovm_stream_t stream);
/* The fused two-layer MLP of the detector's image branch in isolation (test-only): the two launches of that route - fc1 + activation +
 * fc2's k-slices in one kernel, then the split-K reduce - on the caller's own device buffers; nothing is converted or allocated.
 * x_il: interleaved split rows [M][C/32][hi 32 | lo 32] (ovm_op_interleave), row stride ldx >= 2 C halves; w1_il: the same image of
 * W1 [hidden][C], w2_il of W2 [C][hidden]; b1 [hidden], b2 [C] or null; act: 1 ReLU, 2 GELU(erf). ws: fp32 workspace of at least
 * (hidden / 256) * M * C * 4 bytes, written as slabs [hidden / 256][M][C]. X != null: X [M][C] += result + b2 in place (a Swin block's
 * residual); X == null: Y [M][C] = result + b2 (+ R [M][C] when given) (the encoder's FFN). All pointers 16-byte aligned.
 * OVM_ERR_INVALID, and nothing launched, for a shape the kernel does not take (C % 32, hidden % 256, act, f16x3 only);
 * OVM_ERR_CAPACITY, and nothing launched, when ws_bytes is too small. */
int ovm_op_mlp_fused(const uint16_t* x_il, int32_t ldx, const uint16_t* w1_il, const float* b1, const uint16_t* w2_il, const float* b2,
                     int32_t M, int32_t C, int32_t hidden, int32_t act, float* ws, int64_t ws_bytes, float* X, const float* R, float* Y,
                     ovm_stream_t stream);
/* hi, lo [rows][K] (K % 32 == 0) -> out [rows][K/32][hi 32 | lo 32]: the interleaved operand image of the split-precision GEMM.
 * In split mode ovm_op_gemm takes w_hi = such an image and w_lo = w_hi + 32; activations may be plain arrays or an image
 * (a_lo = a_hi + 32, lda = 2K). */
int ovm_op_interleave(const uint16_t* hi, const uint16_t* lo, int64_t rows, int32_t K, uint16_t* out, ovm_stream_t stream);
int ovm_op_layernorm(const float* x, int32_t M, int32_t D, const float* gamma, const float* beta, float eps,
                     float* y, ovm_stream_t stream);
int ovm_op_attention(const float* qkv, int32_t B, int32_t T, int32_t heads, float* out, int32_t precision,
                     ovm_stream_t stream);
int ovm_op_roi_align(const float* p2, const float* p3, const float* p4, const int32_t* hw /* [3][2] */,
                     const float* scales /* [3] */, int32_t C, int32_t out_res, int32_t min_level, int32_t max_level,
                     const float* boxes, const int32_t* image_idx, int32_t n, float* out /* [n][res*res*C] (ph,pw,c) */,
                     ovm_stream_t stream);
int ovm_op_cube_decode(const float* head13, int32_t ld, const float* boxes, const float* scores, const int32_t* classes,
                       const int32_t* image_idx, const OvmImage* images, int32_t B, int32_t n, float virtual_focal,
                       int32_t postprocess, OvmDet3D* rec, int32_t* keep, ovm_stream_t stream);
/* torchvision.ops.nms: keep_idx [n] in decreasing-score order (ties: lower index first), *n_keep their number. n <= 4096;
 * a larger n returns OVM_ERR_CAPACITY before any device work and leaves keep_idx and *n_keep untouched. Synchronises. */
int ovm_op_nms(const float* boxes, const float* scores, int32_t n, float thresh, int32_t* keep_idx, int32_t* n_keep,
               ovm_stream_t stream);
/* The post-processing stages of ovm_rpn_box_forward on their own, with inputs the caller chooses. Both allocate their scratch,
 * free it on every exit path and synchronise the stream. Of `images` only height / width are read (the clip size).
 *
 * RPN.predict_proposals + find_top_rpn_proposals. levels_o: host array of nlev (1 .. 4) device pointers, level l fp32
 * [B * sides[l]^2][16] = 3 objectness logits then 3 x 4 anchor deltas per cell (cell = y * side + x, image-major); sides, strides,
 * anchor_sizes [nlev] and anchor_ratios [3] host arrays. Outputs (device): prop_boxes [B][post_topk][4] and prop_scores
 * [B][post_topk] in decreasing-score order, rows past prop_count [B] zero. pre_topk, post_topk <= 1024, else OVM_ERR_CAPACITY. */
int ovm_op_rpn_proposals(const float* const* levels_o, int32_t nlev, const int32_t* sides, const float* strides,
                         const float* anchor_sizes, const float* anchor_ratios, const OvmImage* images, int32_t B,
                         int32_t pre_topk, int32_t post_topk, float nms_thresh, float* prop_boxes, float* prop_scores,
                         int32_t* prop_count, ovm_stream_t stream);
/* FastRCNNOutputLayers.inference. HO (device) fp32 [B*R][ldh]: K+1 class logits, then K x 4 box deltas (weights 10, 10, 5, 5);
 * prop_boxes [B][R][4] and prop_count [B] (device): rows r >= prop_count[b] are ignored. Outputs (device, capacity B*topk rows,
 * image-major and compact, nothing is written past the sum of out_counts): boxes [.][4], scores, classes, image_idx,
 * scores_full [.][K] (may be NULL), out_counts [B]. R, topk <= 1024 and K <= 63, else OVM_ERR_CAPACITY. */
int ovm_op_boxhead_post(const float* HO, int32_t ldh, const float* prop_boxes, const int32_t* prop_count, const OvmImage* images,
                        int32_t B, int32_t R, int32_t K, float score_thresh, float nms_thresh, int32_t topk, float* boxes,
                        float* scores, int32_t* classes, int32_t* image_idx, float* scores_full, int32_t* out_counts,
                        ovm_stream_t stream);
/* The kernels between the GEMMs, each on its own (test-only): thin adapters over the launchers the model path calls. Device pointers
 * unless marked host; fp16 buffers are passed as uint16_t and written in the kernel's own layout, so the caller sees exactly which
 * elements a kernel touches. A lo pointer may be NULL (one-pass mode). None synchronises unless it says so.
 *
 * ROIAlign with the pooler's level rule over nlevels <= 4 NHWC fp32 levels: feats (host array of device pointers), hw (host, [nlevels][2] =
 * fh, fw) and scales (host). Row r of hi / lo (row stride ldo >= out*out*C, (ph, pw, c) order) receives box r. C % 4 != 0: OVM_ERR_SHAPE. */
int ovm_op_roi_align_ex(const float* const* feats, int32_t nlevels, const int32_t* hw, const float* scales, int32_t C, int32_t out_res,
                        int32_t min_level, int32_t max_level, const float* boxes, const int32_t* image_idx, int32_t n,
                        uint16_t* hi, uint16_t* lo, int32_t ldo, ovm_stream_t stream);
/* Stable compaction of the records (OvmDet3D rows) with keep != 0 into out, and counts [B] = kept records per image (field `image`). */
int ovm_op_compact_records(const OvmDet3D* rec, const int32_t* keep, int32_t n, int32_t B, OvmDet3D* out, int32_t* counts,
                           ovm_stream_t stream);
/* LayerNorm of rows x [M][ldx] (D % 4 == 0, D <= 2048, else OVM_ERR_SHAPE) into any of: y fp32 [M][ldf]; hi / lo fp16 split rows of
 * stride ld. padH > 0: row (b, yy, xx) of M = B padH padW goes to pixel (yy + 1, xx + 1) of a [B][padH + 2][padW + 2] image. il: hi / lo
 * form an interleaved image (lo = hi + 32, ld = 2 D; column k at (k / 32) * 64 + k % 32). */
int ovm_op_ln_rows(const float* x, int32_t ldx, int32_t M, int32_t D, const float* gamma, const float* beta, float eps, float* y,
                   int32_t ldf, uint16_t* hi, uint16_t* lo, int32_t ld, int32_t padH, int32_t padW, int32_t il, ovm_stream_t stream);
/* hi + lo [M][D] <- split(gelu_erf(LayerNorm(hi + lo))), in place (D % 4 == 0, D <= 1024, else OVM_ERR_SHAPE) */
int ovm_op_ln_gelu_split(uint16_t* hi, uint16_t* lo, int32_t M, int32_t D, const float* gamma, const float* beta, float eps,
                         ovm_stream_t stream);
/* Patch rows of B uint8 images (host array; data, height, width and the three strides are read) on a G x G grid of patch x patch
 * patches: hi / lo [B G^2][Kpad], column (py * patch + px) * 3 + c = (u8 - mean[c]) / std[c], zero outside the image and from column
 * 3 patch^2 on. patch 14, or patch 16 with Kpad 768, else OVM_ERR_INVALID. mean, std: host [3]. Synchronises. */
int ovm_op_patch_gather(const OvmImage* images, int32_t B, int32_t G, int32_t patch, int32_t Kpad, const float* mean, const float* std,
                        uint16_t* hi, uint16_t* lo, ovm_stream_t stream);
/* The same rows (patch 16, Kpad 768, else OVM_ERR_INVALID) from B <= 36 strided fp32 views, split as they are. views: host
 * [B][4] = device address of the view's first pixel, then its channel, row and column strides in elements. */
int ovm_op_patch_gather_f32(const int64_t* views, int32_t B, int32_t G, int32_t Kpad, uint16_t* hi, uint16_t* lo, ovm_stream_t stream);
/* X [B][T][D]: token 0 <- cls + pos[0 .. D), tokens 1 .. R <- reg [R][D] */
int ovm_op_cls_init(float* X, const float* cls, const float* pos, const float* reg, int32_t R, int32_t B, int32_t T, int32_t D,
                    ovm_stream_t stream);
/* The last G2 tokens of each image of X [B][T][D] as split rows hi / lo [B G2][ldo]; ldo > D: column D holds depth_tok [B G2] (zero
 * when NULL) and the columns after it zero */
int ovm_op_tokens_cast(const float* X, int32_t B, int32_t T, int32_t G2, int32_t D, int32_t ldo, const float* depth_tok, uint16_t* hi,
                       uint16_t* lo, ovm_stream_t stream);
/* The last G2 tokens of each image of X [B][T][D] <- F [B G2][D] */
int ovm_op_tokens_writeback(float* X, const float* F, int32_t B, int32_t T, int32_t G2, int32_t D, ovm_stream_t stream);
/* 2 x 2 / 2 max-pool of split NHWC rows [B][G][G][D] -> [B][G/2][G/2][D] (an odd last row and column are dropped) */
int ovm_op_maxpool2(const uint16_t* in_hi, const uint16_t* in_lo, int32_t B, int32_t G, int32_t D, uint16_t* out_hi, uint16_t* out_lo,
                    ovm_stream_t stream);

/* --- GroundingDINO output glue of ROIHeads3DGDINO (reference roi_heads_gdino.py:186-202,236-263,266-294):
 * pred_logits [nq][ld] (pre-sigmoid token logits, ld = 256), pred_boxes [nq][4] cxcywh in [0,1] (device);
 * spans: host int32 [n_phrases][2] = [begin, end) token positions of each category phrase (walked from id 1,
 * +1 per separator, :277-291). Sigmoid, per-phrase SUM, max / first-argmax, strict `> box_threshold`, * [w,h,w,h],
 * cxcywh->xyxy, class-agnostic NMS. Outputs (device, capacity nq) in decreasing-score order; n_out device int32.
 * Synchronises the stream. */
int ovm_gdino_postprocess(const float* pred_logits, int32_t nq, int32_t ld, const float* pred_boxes, const int32_t* spans,
                          int32_t n_phrases, int32_t img_h, int32_t img_w, float box_threshold, float nms_threshold,
                          float* out_boxes, float* out_scores, int32_t* out_classes, int32_t* n_out, ovm_stream_t stream);

/* --- GroundingDINO network of ROIHeads3DGDINO as ONE call (ovm_gdino_forward). Replaces
 * `load_model("./configs/GroundingDINO_SwinB_cfg.py", "./checkpoints/groundingdino_swinb_cogcoor.pth")` and
 * `model(image[None], captions=[caption])` of reference cubercnn/modeling/roi_heads/roi_heads_gdino.py:16-23,186 (network:
 * IDEA-Research/GroundingDINO @856dde2, configs/GroundingDINO_SwinB_cfg.py:1-43). The handle owns the packed weights; per
 * (image size, caption) it builds a plan (index maps, masks, position tables, activation arena) once and replays the forward
 * as a single HIP graph afterwards. Weights are named as in the Hugging Face port (upstream checkpoints are renamed by the host,
 * ovmono3d_amd/gdino/detector.py:convert_upstream_state_dict). */
typedef struct OvmGdino OvmGdino;
typedef struct OvmGdinoConfig {
  int32_t d_model, enc_layers, dec_layers, heads, ffn_dim;        /* cfg:9-15: 256, 6, 6, 8, 2048 */
  int32_t n_levels, n_points, num_queries, max_text_len;          /* cfg:19-21,16,33: 4, 4, 900, 256 */
  float pe_temperature, eps;                                      /* cfg:4-6: 20; LayerNorm eps 1e-5 */
  int32_t bert_heads;                                             /* bert-base-uncased: 12 */
  int32_t swin_embed, swin_depths[4], swin_heads[4], swin_window; /* swin_B_384_22k (cfg:3): 128, 2/2/18/2, 4/8/16/32, 12;
                                                                     swin_T_224_1k (GroundingDINO_SwinT_OGC.py, groundingdino_swint_ogc.pth):
                                                                     96, 2/2/6/2, 3/6/12/24, 7. Head dimension 16, 32 or 64 */
  float pixel_mean[3], pixel_std[3];                              /* MODEL.PIXEL_MEAN / STD in tensor channel order */
  int32_t flip_channels;                                          /* 1: the reference's images[0][[2,1,0]] (roi_heads_gdino.py:146) */
  int32_t precision;                                              /* 1 = fp16 operands, 3 = split fp16 (default) */
  int32_t use_graphs;                                             /* capture each plan's forward into a HIP graph */
  int32_t max_plans;                                              /* plans kept (LRU); 0 = 128 */
  int32_t plan_budget_mb;                                         /* device memory the kept plans may hold together (arenas, tables,
                                                                     split-K workspaces), MiB; least recently used plans go first;
                                                                     0 = 32768. A dataset has more aspect ratios than any fixed
                                                                     count: the bound that matters is bytes */
} OvmGdinoConfig;
int ovm_gdino_create(const OvmGdinoConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmGdino** out);
int ovm_gdino_destroy(OvmGdino* g);
const char* ovm_gdino_last_error(const OvmGdino* g);
/* image: uint8 at network resolution (device). token_ids: host int32 [ntok] = tokenizer(caption) incl. [CLS] / [SEP];
 * position_ids: host int32 [ntok] or NULL (upstream numbering: restart per phrase, delimiter included).
 * pred_logits: device fp32 [num_queries][max_text_len], pre-sigmoid, -inf beyond the caption; pred_boxes: device fp32
 * [num_queries][4] (cx, cy, w, h in [0, 1]). Either output may be NULL (results stay in the handle for ovm_gdino_detect).
 * ntok > max_text_len is OVM_ERR_INVALID. The row-chain decoder (tune key gdino_dec_chain) applies while heads * ntok <= 516 (64
 * tokens at 8 heads); longer captions run the launch-per-op decoder. */
int ovm_gdino_forward(OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* position_ids,
                      float* pred_logits, float* pred_boxes, ovm_stream_t stream);
/* forward + the reference-owned output glue (ovm_gdino_postprocess below; roi_heads_gdino.py:186-202,236-263): outputs as there. */
int ovm_gdino_detect(OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* spans, int32_t n_phrases,
                     float box_threshold, float nms_threshold, float* out_boxes, float* out_scores, int32_t* out_classes, int32_t* n_out,
                     ovm_stream_t stream);
int32_t ovm_gdino_num_queries(const OvmGdino* g);
/* device pointers of the last forward's raw outputs (owned by the handle; valid until its next forward); logits_ld = max_text_len */
int ovm_gdino_last_outputs(OvmGdino* g, const float** pred_logits, const float** pred_boxes, int32_t* logits_ld);
/* tests: pin the two-stage top-k selection to the given device int32 [num_queries] (NULL: the network's own) */
int ovm_gdino_set_force_topk(OvmGdino* g, const int32_t* idx_device);
/* tests: copy an intermediate of the last forward ("bert_out", "text_features", "swin_stage1..3", "enc_vision", "enc_text",
 * "topk" (int32), "init_ref") into dst; returns the element count. name "launches": returns the kernel launches per forward
 * (per image: with the caption cache, tune key gdino_text_cache, the caption's encoding is not among them); "text_launches": the
 * launches the last forward call spent on encoding its caption, 0 when it was held; "text_entries": captions the handle holds. */
int64_t ovm_gdino_debug_copy(OvmGdino* g, const char* name, void* dst, int64_t capacity_elems, ovm_stream_t stream);

/* --- the whole path for one image as ONE call (SURVEY.md 8b `ovm_infer`): RCNN3D.inference with the text-prompted head, reference
 * cubercnn/modeling/meta_arch/rcnn3d.py:79-117 (batched_inputs = [{image, height, width, K, category_list}]) ->
 * roi_heads_gdino.py:93-171 -> roi_heads.py:329-549,798-848 -> detector_postprocess. `image` as for ovm_backbone_forward (orig
 * size and K filled); token_ids / spans as for ovm_gdino_detect (spans[k] = [begin, end) token positions of category k's phrase,
 * so the record's `category` is the index into the category list, roi_heads_gdino.py:162). out: device records, capacity
 * out_capacity (<= the detector's num_queries are produced); n_out: host. Synchronises the stream. */
int ovm_infer(OvmHandle* h, OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* spans,
              int32_t n_phrases, float box_threshold, float nms_threshold, OvmDet3D* out, int32_t out_capacity, int32_t* n_out,
              ovm_stream_t stream);

/* ovm_infer with a depth prompt: RCNN3D.forward(batched_inputs, prompt_depth) of the reference (rcnn3d.py:41,97: the backbone call
 * becomes self.backbone(images.tensor, prompt_depth), dino.py:82-105 - the metric depth map, resized to the patch grid, concatenated
 * to the last block's patch tokens and run through depth_fusion). prompt_depth: device fp32 [1][1][depth_h][depth_w] as for
 * ovm_backbone_forward, read on the caller's stream, or NULL, which is ovm_infer. The refusals of ovm_backbone_forward for a prompt
 * (a tower other than DINOv2, a register-token model, absent depth_fusion weights: OVM_ERR_INVALID with a message) are returned
 * before anything is launched or forked; the handle stays usable. Every other argument, the kernels and their order as ovm_infer. */
int ovm_infer_depth(OvmHandle* h, OvmGdino* g, const OvmImage* image, const float* prompt_depth, int32_t depth_h, int32_t depth_w,
                    const int32_t* token_ids, int32_t ntok, const int32_t* spans, int32_t n_phrases, float box_threshold,
                    float nms_threshold, OvmDet3D* out, int32_t out_capacity, int32_t* n_out, ovm_stream_t stream);

/* --- generic device ops the GroundingDINO branch (ROIHeads3DGDINO's network, reference roi_heads_gdino.py:186) is
 * was sequenced from in round 1 (still exported: unit tests and the Python-sequenced cross-check path use them): fp32
 * row-major tensors in HBM, one call per op, all arithmetic on the device. */
int ovm_g_pack_weight(const float* w, int32_t N, int32_t K, int32_t Kpad, uint16_t* hi, uint16_t* lo, ovm_stream_t stream);
/* The same image written on the host (no device call; what every model handle packs its weights with). w: host [N][K] fp32;
 * out: host, ceil128(N) * Kpad halves for precision 1 ([Npad][Kpad]) or twice that for precision 3 (the interleaved split image
 * [Npad][Kpad/32][hi 32 | lo 32], hi = fp16(x), lo = fp16(x - hi), round to nearest even, subnormals kept), padding rows and columns
 * zero. OVM_ERR_INVALID for a null pointer, N < 1, K < 1, Kpad < K or a precision other than 1 and 3; OVM_ERR_SHAPE for precision 3
 * with Kpad % 32 != 0; out is left untouched then. */
int ovm_host_pack_weight(const float* w, int32_t N, int32_t K, int32_t Kpad, int32_t precision, uint16_t* out);
int ovm_g_linear(const float* x, int32_t ldx, int32_t M, int32_t K, const uint16_t* w_hi, const uint16_t* w_lo, int32_t N, int32_t Kpad,
                 const float* bias, int32_t act /* 0 none, 1 relu, 2 gelu */, const float* residual, int32_t ldr, float* y, int32_t ldy,
                 int32_t precision, ovm_stream_t stream);
int ovm_g_layernorm(const float* x, const float* residual, int32_t M, int32_t D, const float* gamma, const float* beta, float eps, float* y,
                    ovm_stream_t stream);
int ovm_g_bmm(const float* a, const float* b, float* c, int32_t batch, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc,
              int64_t sA, int64_t sB, int64_t sC, int32_t transB, float alpha, ovm_stream_t stream);
int ovm_g_bmm2(const float* a, const float* b, float* c, int32_t nb1, int32_t nb2, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
               int32_t ldc, int64_t sA1, int64_t sB1, int64_t sC1, int64_t sA2, int64_t sB2, int64_t sC2, int32_t transB, float alpha,
               ovm_stream_t stream);
int ovm_g_softmax2(float* x, int32_t rows, int32_t cols, int32_t ld, const float* bias, int32_t bias_rows, int32_t bias_div, int32_t bias_ld,
                   const float* bias2, int32_t d2, int32_t m2, ovm_stream_t stream);
int ovm_g_softmax(float* x, int32_t rows, int32_t cols, int32_t ld, const float* bias, int32_t bias_rows, int32_t bias_div, int32_t bias_ld,
                  ovm_stream_t stream);
int ovm_g_eltwise(int32_t op, const float* a, const float* b, float* out, int64_t n, int64_t bmod, float alpha, float beta, ovm_stream_t stream);
int ovm_g_gather_rows(const float* src, int32_t ld_src, const int32_t* idx, int64_t n_out, int32_t nidx, int32_t cols, float* dst,
                      ovm_stream_t stream);
int ovm_g_groupnorm(const float* x, int32_t B, int32_t HW, int32_t C, int32_t groups, const float* gamma, const float* beta, float eps, float* y,
                    ovm_stream_t stream);
int ovm_g_msdeform(const float* value, const int32_t* shapes_hw, int32_t L, int32_t B, int32_t S, int32_t Q, int32_t H, int32_t dh, int32_t P,
                   const float* loc, const float* w, float* out, ovm_stream_t stream);
/* GroundingDINO BiMultiHeadAttention.forward (groundingdino/models/GroundingDINO/fuse_modules.py) as reached from
 * roi_heads_gdino.py:186, after its four input projections: with A = scale * Q K_text^T per head (head h = columns h*dh ..),
 * ctx_img = softmax over the T text tokens of A, times V_text; ctx_text = softmax over the S image tokens of A^T, times V_img.
 * q, v_img: device fp32 [S][H*dh] (row strides ldq, ldvi); k_text, v_text: [T][H*dh] (ldk, ldvt); row strides multiples of 4 floats,
 * rows 16-byte aligned. Outputs (device): ctx_img fp32 [S][ldc] and / or its split-fp16 image ctx_img_hi / ctx_img_lo [S][ldc]
 * halves (either may be NULL, not both ctx_img and ctx_img_hi); ctx_text fp32 [T][H*dh]. dh = 256 and T <= 256 run the one-pass
 * matrix-core kernel, anything else (dh % 4 == 0, dh <= 512) or generic != 0 the four generic kernels. Owns its scratch and
 * synchronises the stream. OVM_ERR_INVALID (nothing launched) for a null pointer or a non-positive dimension. */
int ovm_g_biattn(const float* q, int32_t ldq, const float* k_text, int32_t ldk, const float* v_img, int32_t ldvi, const float* v_text,
                 int32_t ldvt, int32_t S, int32_t T, int32_t H, int32_t dh, float scale, float* ctx_img, uint16_t* ctx_img_hi,
                 uint16_t* ctx_img_lo, int32_t ldc, float* ctx_text, int32_t generic, ovm_stream_t stream);
int ovm_g_sine_embed(const float* pos, int64_t n, int32_t nc, int32_t F, float temperature, float* out, ovm_stream_t stream);
int ovm_g_normalize_image(const OvmImage* image, const float* mean, const float* stdv, int32_t flip_channels, float* out_nhwc,
                          ovm_stream_t stream);
int ovm_g_rowmax(const float* x, int32_t rows, int32_t cols, int32_t ld, float* out, ovm_stream_t stream);
int ovm_g_topk(const float* scores, int32_t n, int32_t k, int32_t* out_idx, ovm_stream_t stream);

/* --- the fused kernels of ovm_gdino_forward (and, for the attention, of the SAM tower) one at a time, for tests: each descriptor
 * mirrors the engine's own parameter block (csrc/gdino.hpp) field for field and the call is that kernel's launcher, nothing else -
 * no conversion, no scratch, no synchronisation; all pointers are device memory the caller owns, the result is the launcher's code.
 * OVM_ERR_INVALID for a null descriptor.
 *
 * attn_f32_kernel: o[b1][b2][q][0:DH] = softmax_k(scale q.k + bias_h[b2][q][k] + bias_b[b1][q][k] + rel_h[kh] + rel_w[kw]) v, exact
 * fp32 products on the matrix cores, keys walked in chunks of 144. DH in {16, 32, 64}; sq1 .. so2 are the element strides of the two
 * batch levels (b1 outer, b2 = head); o (fp32) and / or ohi, olo (split fp16: hi = fp16(y), lo = fp16(y - hi)) with their own strides;
 * bias_h [nb2][Tq][ldbh] (stride sbh), bias_b [nb1][Tq][ldbb] (stride sbb, 0: shared by all b1), either may be NULL; rel_h, rel_w:
 * [b1][q][b2][ldrel], key = kh * rel_gw + kw (NULL: none). k, v and o rows must be 16-byte aligned with strides that are multiples
 * of 4 floats, else OVM_ERR_SHAPE (also for another DH); nothing is launched then. */
typedef struct OvmAttnF32Op {
  const float* q; const float* k; const float* v; int32_t ldq, ldk, ldv, reserved0;
  int64_t sq1, sq2, sk1, sk2, sv1, sv2;
  float* o; int32_t ldo, reserved1; int64_t so1, so2;
  uint16_t* ohi; uint16_t* olo; int32_t ldoh, reserved2; int64_t soh1, soh2;
  int32_t nb1, nb2, Tq, Tk, DH; float scale;
  const float* bias_h; int64_t sbh; int32_t ldbh, reserved3;
  const float* bias_b; int64_t sbb; int32_t ldbb, reserved4;
  const float* rel_h; const float* rel_w; int32_t rel_gw, ldrel;
} OvmAttnF32Op;
int ovm_g_attn_f32(const OvmAttnF32Op* op, ovm_stream_t stream);
/* msdeform_fused_kernel / msdeform_fused4_kernel (the latter where L * P = 16, dh % 4 == 0 and everything is 16-byte aligned, unless
 * ovm_tune_set msdeform_vec = 0). value [S][ldv] (H * dh columns), level l = rows lstart[l] .. of an lh[l] x lw[l] map; ow [Q][ldow] =
 * H*L*P (x, y) offsets then H*L*P logits; mode 0 (encoder): ref [Q][ldref >= 2] point, loc = ref + off / (W_l, H_l); mode 1
 * (decoder): ref [Q][ldref >= 4] box (cx, cy, w, h), loc = c + off * wh * 0.5 / P. Bilinear taps as F.grid_sample (align_corners =
 * False, zero padding), weights = softmax over the L*P logits of a head. out fp32 [Q][ldo] and / or split ohi, olo [Q][ldoh].
 * L <= 8, else OVM_ERR_CAPACITY. */
typedef struct OvmMsDeformOp {
  const float* value; const float* ow; const float* ref; int32_t ldv, ldow, ldref, mode;
  int32_t Q, H, dh, L, P, reserved0;
  int32_t lh[8], lw[8], lstart[8];
  float* out; uint16_t* ohi; uint16_t* olo; int32_t ldo, ldoh;
} OvmMsDeformOp;
int ovm_g_msdeform_fused(const OvmMsDeformOp* op, ovm_stream_t stream);
/* rowop_kernel, one wave per row r < M: row = concat_j x[idx[r * nidx + j]][0:seg] (idx NULL: x[r][0:D]; idx < 0: zeros; D = nidx *
 * seg) + res[r] -> LayerNorm(gamma, beta, eps) over D (gamma NULL: none) -> zero_masked: rows whose first index is negative are
 * zero after the norm -> y; y2 = y + add[r % add_rows]. Outputs, each optional: y [M][ldy], y2 [M][ldy2], hi / lo = split fp16 of y
 * [M][ldh] with columns D .. ldh written as zero, or with il = 1 ONE interleaved image (lo = hi + 32, ldh = 2 D, column n at
 * (n / 32) * 64 + n % 32; anything else is OVM_ERR_INVALID), hi2 / lo2 = split of y2 [M][ldh2]. With a LayerNorm D <= 4096 on the
 * float4 route (D, seg, ldx, ldr % 4 == 0 and 16-byte aligned x, res) and D <= 1024 otherwise, else OVM_ERR_SHAPE. */
typedef struct OvmRowOp {
  const float* x; const int32_t* idx; const float* res; const float* gamma; const float* beta; const float* add;
  int32_t ldx, nidx, seg, ldr; float eps; int32_t zero_masked, ld_add, add_rows;
  int32_t M, D;
  float* y; float* y2; uint16_t* hi; uint16_t* lo; uint16_t* hi2; uint16_t* lo2;
  int32_t ldy, ldy2, ldh, il, ldh2, reserved0;
} OvmRowOp;
int ovm_g_rowop(const OvmRowOp* op, ovm_stream_t stream);
/* swin_qkv_attn_kernel (ws = 12) / swin7_qkv_attn_kernel (ws = 7): a Swin block's qkv projection and window attention in one launch, head
 * dimension 32, C = 32 nh channels. xhi / xlo: window-partitioned rows [nW * ws^2][ldx] as planar split fp16 (hi = fp16(x), lo = fp16(x -
 * hi)), columns C .. 32 KS zero; wfrag: the [3 C][C] weight (q | k | v rows) packed by ovm_host_pack_weight (precision 3, Kpad = 32 KS),
 * then re-ordered [tile of 16 rows][k-step of 32][hi | lo][lane 0..63][8 halves] with lane l = row l % 16, halves 8 (l / 16) .. of the
 * k-step; bias fp32 [3 C]; relbias fp32 [nh][ws^2][ws^2]; mask fp32 [nW][ws^2][ws^2] or NULL. Output: ohi / olo [nW * ws^2][ldo], head h
 * at columns 32 h ..: softmax_k(scale q.k + relbias + mask) v, as split fp16. Three-pass split-fp16 products for the projection, exact
 * fp32 products for the attention. ws = 12 needs C % 128 == 0 and KS % 4 == 0; ws = 7 takes any C = 32 nh with KS >= C / 32 and wpg =
 * windows per workgroup (1, 2 or 4; 0 = the default). ldx % 8 == 0, ldo % 4 == 0, 16-byte aligned x, wfrag and bias (ws = 12: relbias
 * and mask too), 8-byte aligned ohi and olo. Any other geometry: OVM_ERR_SHAPE, nothing launched. */
typedef struct OvmSwinQkvAttnOp {
  const uint16_t* xhi; const uint16_t* xlo; const uint16_t* wfrag; const float* bias; const float* relbias; const float* mask;
  uint16_t* ohi; uint16_t* olo;
  int32_t ldx, KS, C, nh, nW, ldo; float scale; int32_t ws, wpg, reserved0;
} OvmSwinQkvAttnOp;
int ovm_g_swin_qkv_attn(const OvmSwinQkvAttnOp* op, ovm_stream_t stream);
/* The split image of ovm_host_pack_weight (precision 3, [ceil128(N)][Kpad/32][hi 32 | lo 32]) re-ordered for the kernels that feed
 * weight fragments from global memory straight into the matrix cores (the decoder row chains, the Swin window kernels): [tile of 16
 * rows][k-step of 32][hi | lo][lane 0..63][8 halves], lane l = row l % 16, halves 8 (l / 16) .. of the k-step. Host only; out holds
 * as many halves as the image and must not alias it. This is the function the GroundingDINO loader cuts its fragment copies with.
 * OVM_ERR_INVALID for a null pointer, out == image, N < 1 or Kpad < 32; OVM_ERR_SHAPE for Kpad % 32 != 0; out untouched then. */
int ovm_host_frag_order(const uint16_t* image, int32_t N, int32_t Kpad, uint16_t* out);
/* dec_chain_a_kernel / dec_chain_b_kernel / dec_chain_c_kernel (csrc/dec_chain.hip): a GroundingDINO decoder layer around its query
 * self-attention, 16 query rows per workgroup. part 0 (chain A): qpos = ref_point_head(sine(ref)), qk = (hs + qpos) W_qk ([Q][2 D]),
 * v = hs W_v. part 1 (chain B): hs <- LN1(hs + ctx W_o); text cross-attention over the T rows of tk / tv (row stride ldt) + LN2;
 * deformable sampling of val ([S][ldv], level l = rows lstart[l] .. of an lh[l] x lw[l] map, box mode of OvmMsDeformOp) + LN3; FFN +
 * LN4 -> hs (in place); ref_next = sigmoid(bbox MLP(hs) + logit(clamp(ref, 1e-5, 1 - 1e-5))) unless ref_next is NULL. With ffn_split > 1
 * (= ffn / 512) part 1 runs on a (row blocks x 512-column chunks) grid and ends at the partial products in ffn_x [Q][D] and ffn_part
 * [ffn_split][Q][D]; part 2 (chain C) adds them up and finishes the layer, bit-identical to ffn_split <= 1.
 * lin[]: ref_point_head 0, 1 (2 D -> D -> D), self-attention q | k (N = 2 D), v, out, text-attention q, out, sampling offsets | logits
 * (N = 3 heads L P), deformable out, fc1, fc2, bbox MLP 0, 1, 2 (N = 4); w: ovm_host_pack_weight (precision 3) then ovm_host_frag_order,
 * 16-byte aligned; bias [N]. ln[]: LN1 .. LN4. sine_dim_t [D / 4]: 10000^(2 i / (D / 2)). The call is the engine's launcher
 * (launch_dec_chain) behind a check of the descriptor: OVM_ERR_INVALID for a null descriptor, part outside 0..2, part 2 with
 * ffn_split <= 1 or a null pointer (ref_next may be NULL and lin[11..13] then too; ffn_x / ffn_part only count with ffn_split > 1);
 * OVM_ERR_SHAPE for a geometry ovm_host_dec_chain_supported refuses, a non-positive size, a lin[] entry whose N, K, Kpad are not the
 * geometry's, ldt or ldv below D or not a multiple of 4, or a row pointer that is not 16-byte aligned. Nothing is launched then. */
typedef struct OvmChainLin { const uint16_t* w; const float* bias; int32_t N, K, Kpad, reserved0; } OvmChainLin;
typedef struct OvmChainLn { const float* gamma; const float* beta; } OvmChainLn;
typedef struct OvmDecChainOp {
  int32_t Q, D, T, heads, ffn; float eps;
  float* hs; const float* ref; const float* sine_dim_t; float* ref_next; float* qpos; float* qk; float* v; const float* ctx;
  const float* tk; const float* tv; const float* val; int32_t ldt, ldv;
  int32_t L, P; int32_t lh[8], lw[8], lstart[8];
  OvmChainLin lin[14];
  OvmChainLn ln[4];
  int32_t ffn_split, reserved0; float* ffn_x; float* ffn_part;
} OvmDecChainOp;
int ovm_g_dec_chain(const OvmDecChainOp* op, int32_t part, ovm_stream_t stream);
/* 1 when the decoder row chains take this geometry (what the engine asks before it picks that route; split-fp16 weights, i.e.
 * precision 3, only), else 0. Host only. */
int ovm_host_dec_chain_supported(int32_t D, int32_t heads, int32_t ffn, int32_t L, int32_t P, int32_t T, int32_t precision);
/* The small kernels between the fused ones, one at a time (tests): each call checks for null pointers and non-positive sizes
 * (OVM_ERR_INVALID, nothing launched) and is then the launcher the engine calls (csrc/gdino.hpp), nothing else - no scratch, no
 * synchronisation; all pointers are device memory the caller owns.
 *
 * launch_topk_keys (single_keys_kernel, the bitonic sort, topk_emit_kernel): out_idx[0:k] = the indices of the k largest of scores[0:n]
 * by decreasing score, the lower index first among equal scores, -0.0 equal to +0.0; NaN scores are outside the contract. keys: N
 * 64-bit words of caller-owned workspace, N >= max(2048, the next power of two >= n); only the first max(2048, pow2 >= n) words are
 * written (every real key, then the padding keys, which sort after all of them). n <= 2^24. k > n or N too small: OVM_ERR_INVALID. */
int ovm_g_topk_keys(const float* scores, int32_t n, int32_t k, int32_t* out_idx, uint64_t* keys, int32_t N, ovm_stream_t stream);
/* select_ref_kernel: out[i][c] = sigmoid(coord[idx[i]][c] + prop_logit[idx[i]][c]), c < 4, i < n; coord rows have stride ldc,
 * prop_logit is [rows][4] dense, out [n][4] dense. An infinite proposal logit (an invalid proposal) gives
 * exactly 1. The indices are trusted. */
int ovm_g_select_ref(const float* coord, int32_t ldc, const float* prop_logit, const int32_t* idx, int32_t n, float* out,
                     ovm_stream_t stream);
/* box_refine_kernel: out[i][c] = sigmoid(delta[i][c] + logit(clamp(ref[i][c], eps, 1 - eps))), c < 4, i < n (torch.special.logit(ref,
 * eps)); delta rows have stride ldd, ref and out are [n][4] dense. */
int ovm_g_box_refine(const float* delta, int32_t ldd, const float* ref, float eps, float* out, int32_t n, ovm_stream_t stream);
/* pad_logits_kernel: out[q][0:T] = x[q][0:T] (row stride ldx >= T), out[q][T:ld] = -inf, q < Q; out rows have stride ld >= T and are
 * written whole (T = ld: no -inf). */
int ovm_g_pad_logits(const float* x, int32_t ldx, int32_t Q, int32_t T, float* out, int32_t ld, ovm_stream_t stream);
/* bert_embed_kernel: out[t][0:D] = LayerNorm((word[ids[t]] + pos[pids[t]]) + type[0:D]; gamma, beta, eps) over D, two-pass variance,
 * one wave per row t < T; word / pos [rows][D] dense, type the one row of token type 0, out [T][D] dense. The ids are trusted. */
int ovm_g_bert_embed(const float* word, const float* pos, const float* type, const int32_t* ids, const int32_t* pids, int32_t T, int32_t D,
                     const float* gamma, const float* beta, float eps, float* out, ovm_stream_t stream);
/* relpos_tables_kernel (the SAM tower's decomposed relative positions, the rel_h / rel_w operands of OvmAttnF32Op): for the rows m < M
 * of q (row stride ldq, head h at columns h * DH ..), whose position on the gh x gw attention grid is (qh, qw) = divmod(m mod (gh gw),
 * gw): rel_h[(m * H + h) * ldrel + kh] = q[m][h] . Rh[qh - kh + gh - 1], kh < gh; rel_w[(m * H + h) * ldrel + kw] = q[m][h] .
 * Rw[qw - kw + gw - 1], kw < gw. Rh [2 gh - 1][DH], Rw [2 gw - 1][DH] dense; columns past gh (gw) of a table row are not written.
 * DH % 4, ldq % 4 (the rows are read 16 bytes at a time; q, Rh, Rw 16-byte aligned) or ldrel < max(gh, gw): OVM_ERR_SHAPE, nothing
 * launched. M = 0: OVM_OK, nothing launched. */
int ovm_g_relpos_tables(const float* q, int32_t ldq, int32_t M, int32_t H, int32_t DH, int32_t gh, int32_t gw, const float* Rh,
                        const float* Rw, float* rel_h, float* rel_w, int32_t ldrel, ovm_stream_t stream);

/* Process-global tuning knobs for experiments and tests (also settable as OVM_TUNE="key=value,..." when the host loads the
 * library). Defaults are the measured best; none changes results beyond fp32 summation order.
 *   gemm_bm 0|128|256, gemm_stages 0 (auto: wave-specialised kernel up to 512 tiles, symmetric 2-slot kernel above) |2|3|5|6,
 *   gemm_splitk 0|1, gemm_tail 0|1 (leftover rows as dot-product workgroups), attn_waves 0 (auto)|4|8, attn_lds_pad bytes,
 *   gemm256 0|1 (256 x 256 two-wave-group kernel for qkv / fc1), op_gemm256 n (ovm_op_gemm on that kernel, n = split-K hint),
 *   attn_tail 0|1, glin_small_max_tiles (-1 = heuristic), glin_target_blocks, glin_max_ksplit, glin_stages 1|2, gbmm_tiled 0|1,
 *   gemm256_n192 0|1 (qkv on 256 x 192 tiles where they fill the chip better; default 1), attn_q64 0|1 (the 4-wave x 64-query attention
 *   kernel; default 0: measured slower), attn_pp 0|1 (two-wave-group attention kernel), msdeform_vec 0|1 (vectorised deformable sampling;
 *   default 1), gdino_dec_chain 0|1 (GroundingDINO decoder layers as row-chain kernels; default 1; read when a plan is built),
 *   gdino_ffn_split 0|1 (decoder row chains: the FFN's 512-column chunks on separate workgroups + a finishing kernel; bit-identical, faster for the detector alone, not beside the ViT; default 0; read when a plan is built),
 *   gdino_swin_fused 0|1 (Swin blocks: qkv projection inside the window-attention kernel, windows of 12 x 12 and of 7 x 7; default 1; read
 *   when a plan is built), gdino_swin_tap n (tests: plans built afterwards keep copies of their n-th Swin block's window rows and context
 *   rows and offer them, with that block's qkv fragment image, bias, relative-position bias and shift mask, to ovm_gdino_debug_copy as
 *   "swin_tap_xhi|xlo|ohi|olo|wfrag|bias|relbias|mask", counted in 4-byte elements; default 0),
 *   gdino_gemm256 0|1 (the detector's wide K <= 256 contractions on the 256 x 256 kernel; default 1; read when a plan is built),
 *   gdino_mlp_fused 0|1|2 (the image branch's two-layer MLPs as one kernel + the split-K reduce: 0 off, 1 the Swin blocks whose fc2 is
 *   split over K today, 2 those and the encoder's FFN where its slabs fit the workspace; default 1; read when a plan is built),
 *   gdino_enc_fold 0|1|2|3 (encoder: 1 = the position term of the sampling-offsets projection as a per-plan table, value and offsets projections as one GEMM, split rows written by their producers; 2 = the fold alone, 3 = the producers' split rows of the neck and the decoder inputs alone; default 0; read when a plan is built),
 *   gdino_enc_tap 0|1 (tests: plans built afterwards keep copies of encoder layer 0's out-projection rows, their split and the value |
 *   offsets projections' outputs for ovm_gdino_debug_copy "enc_pos|enc_vis0|enc_vis0_hi|enc_vis0_lo|enc_voff0|enc_P0", with gdino_enc_fold 0
 *   "enc_val0|enc_ow0" for the last two; default 0),
 *   gdino_text_cache n (the detector's caption cache: what depends on the caption and the weights alone - BERT, the text projection and
 *   encoder layer 0's text norm and text projection - is computed once per (token ids, position ids), outside the per-image graph, and the
 *   handle keeps the n most recently used captions' results, which all plans of a caption share; every ovm_tune_set call retires the
 *   results made before it; 0 = inside every forward as before, the same bits; default 16; read when a plan is built),
 *   attn_tail_split 0|1 (attention's leftover queries split over 16 key slices + combine kernel; default 1), attn_prio n (experiment:
 *   s_setprio inside the two-wave-group attention kernel; default 0), gemm256_ksplit n (experiment: split-K hint of the 256 x 256 kernel for
 *   proj / fc2; default 0 = off, measured slower), glin_wpe 2|4 (experiment: workgroups per CU the small fp32-A GEMM is compiled for; default 2),
 *   gdino_branches 0|1. Values that select timing-only ablations with wrong results exist in -DOVM_DIAG builds only. */
int ovm_tune_set(const char* key, int32_t value);
/* diagnostic hooks: device pointer for a named debug hook ("gemm256_stamps": u64 [8 waves][128] s_memtime stamps of workgroup 0;
 * "attn_stamps": -DOVM_DIAG builds only, OVM_ERR_UNSUPPORTED otherwise) */
int ovm_debug_set_ptr(const char* key, void* ptr);

/* --- introspection for tests: copy a named intermediate of the last forward into dst (device).
 * names: "tokens" [B*T][D] fp32, "p2" / "p3" / "p4" (/ "p5"); "rpn_boxes" [B][R][4], "rpn_scores" [B][R], "rpn_counts" [B] (int32 bits) =
 * the RPN's proposals after top-k / NMS of the last ovm_rpn_box_forward; "cube_head" [n][16] = the cube head's raw outputs of the
 * last ovm_cube_forward (deltas 2, dims 3, pose 6-D, depth 1, uncertainty 1). Returns the element count or a negative error. */
int64_t ovm_debug_copy(OvmHandle* h, const char* name, float* dst, int64_t capacity, ovm_stream_t stream);

/* ---- evaluation ("next" row 1 of SURVEY.md 8f) ---------------------------------------------------------------------------
 * Exact IoU of oriented 3D boxes, iou[i*M + j] for detection i and ground truth j; boxes are 8 corners x 3 floats in
 * pytorch3d's corner order. Replaces `box3d_overlap` -> pytorch3d `_C.iou_box3d` (cubercnn/evaluation/omni3d_evaluation.py:109-169)
 * including the screening of the detections: rows of non-coplanar (:68-87) or zero-area (:90-107) detections are 0.
 * A box without volume (a face without a normal, or volume <= 0: all -1 or all 0 corners, flat boxes) intersects nothing:
 * IoU and volume 0. `vol` (optional) receives the intersection volumes. */
int ovm_box3d_iou(const float* boxes_dt, const float* boxes_gt, int32_t N, int32_t M, float eps_coplanar, float eps_nonzero, float* iou,
                  float* vol, ovm_stream_t stream);

/* One (image, category) cell of the COCO-style evaluation, packed CSR-style: its detections are rows dt_off .. dt_off+n_dt-1
 * of the detection arrays (descending score, cut to the largest maxDets), its ground truth rows gt_off .. gt_off+n_gt-1 of the
 * ground-truth arrays (file order), its IoU the row-major [n_dt][n_gt] block at iou_off. prox != 0: the proximity rules of
 * upstream Omni3D's evaluateImg apply to the cell (reference Omni3Deval(eval_prox=...) :1472-1485, threshold :1459-1461). */
typedef struct OvmEvalCell {
  int64_t iou_off;
  int32_t dt_off, n_dt;
  int32_t gt_off, n_gt;
  int32_t prox;
  int32_t reserved;
} OvmEvalCell;

/* fp64 xywh box IoU of every cell, bit-equal to pycocotools maskUtils.iou without crowd regions (the IoU of COCOeval.computeIoU
 * that Omni3Deval inherits, reference :1467). dt_cell [n_dt_total]: the cell of each detection row. dt_box / gt_box [.][4] xywh.
 * iou (optional) receives each cell's block; in_prox (optional, uint8 [n_dt_total]) = any IoU of the row > prox_thresh. All device. */
int ovm_eval_iou2d(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, const double* dt_box, const double* gt_box,
                   double prox_thresh, double* iou, uint8_t* in_prox, ovm_stream_t stream);

/* Greedy COCO matching of every cell x range x IoU threshold in one launch: COCOeval.evaluateImg as Omni3Deval runs it (reference
 * :1467-1545 on pycocotools), with upstream Omni3D's proximity rules for cells with prox set. Per range the ground truth is ordered
 * not-ignored first (stable); per threshold the detections pick in score order the free ground truth of highest IoU >= floor (the
 * later one on equal IoU), among the ignored ones only when no not-ignored one qualifies; crowd ground truth is never taken; a NaN
 * IoU counts as 0. iou: the [n_dt][n_gt] blocks (fp64). dt_rng / gt_rng: area (2D) or depth (3D); gt_flag / gt_crowd uint8;
 * in_prox: uint8 per detection (read for prox cells only, may be NULL when none is). ranges [n_rng][2] = lo, hi; floors [n_thr]
 * = min(threshold, 1 - 1e-10). Outputs, cell c at detection offset o = dt_off * n_rng * n_thr: pick int32 [o + (r*n_thr + t)*n_dt + d]
 * (index into the ORDERED ground truth, -1 = none), ignored uint8 (same index), n_gt int32 [c*n_rng + r]. All device. max_gt: the
 * largest n_gt of any cell; a cell holds at most 4096 ground-truth boxes (OVM_ERR_CAPACITY otherwise). */
int ovm_eval_match(const OvmEvalCell* cells, int32_t n_cells, int32_t max_gt, const double* iou, const double* dt_rng, const double* gt_rng,
                   const uint8_t* gt_flag, const uint8_t* gt_crowd, const uint8_t* in_prox, const double* ranges, int32_t n_rng,
                   const double* floors, int32_t n_thr, int32_t* pick, uint8_t* ignored, int32_t* n_gt, ovm_stream_t stream);

/* The exact 3D IoU of every cell's [n_dt][n_gt] block, written as fp64 straight into the CSR IoU buffer ovm_eval_match reads
 * (`box3d_overlap` per cell, reference cubercnn/evaluation/omni3d_evaluation.py:109-169). dt_cell as for ovm_eval_iou2d;
 * dt_corners [n_dt_total][8][3] / gt_corners [n_gt_total][8][3] fp32, the ground truth already through nan_to_num. Every value is
 * (double) of what ovm_box3d_iou gives for the pair (the same per-pair code), a NaN written as 0. One wave per detection row, one
 * lane per ground-truth box. All device. */
int ovm_eval_iou3d(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, const float* dt_corners, const float* gt_corners,
                   float eps_coplanar, float eps_nonzero, double* iou, ovm_stream_t stream);

#define OVM_NHD_NONE 0    /* the detection has no pair */
#define OVM_NHD_OK 1      /* paired and scored */
#define OVM_NHD_SKIPPED 2 /* paired, but a corner distance is not finite: no score (scipy's linear_sum_assignment raises there) */

/* Pairing and disentangled Normalised Hungarian Distance of Omni3DevalWithNHD (reference :2342-2484 with calculate_nhd /
 * disentangled_nhd :2227-2290), one wave per detection row. Pairing: the first maximum of the row's IoU block (iou: the fp64 CSR
 * blocks), accepted when it is > 0 and >= iou_thr and dt_ok[d] and gt_ok[g] (uint8: the record carries its fields); pair_gt [n_dt_total]
 * receives the cell-local ground-truth index in file order, or -1. Cuboid records dt_cuboid [n_dt_total][15] / gt_cuboid
 * [n_gt_total][15] fp32: xy (2), z, dimensions W H L (3), rotation row-major (9); rows without their fields are not read. Everything
 * after the load is fp64: corners = signs * (L, H, W)/2 @ R^T + c for the prediction and for the prediction with only xy / z /
 * dimensions / pose kept (the rest the ground truth's), the five 8x8 Euclidean cost matrices, each assignment solved exactly by
 * dynamic programming over the 256 subsets, divided by the norm of the ground truth's axis-aligned extent (0 divides as IEEE
 * does). nhd [n_dt_total][5] = overall, xy, z, dimensions, pose (written for OVM_NHD_OK rows only); status uint8 [n_dt_total] one of
 * OVM_NHD_*; a skipped row gets pair_gt -1. max_gt: the largest n_gt of any cell, at most 4096 (OVM_ERR_CAPACITY otherwise). All device. */
int ovm_eval_nhd(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, int32_t max_gt, const double* iou, double iou_thr,
                 const uint8_t* dt_ok, const uint8_t* gt_ok, const float* dt_cuboid, const float* gt_cuboid, int32_t* pair_gt, double* nhd,
                 uint8_t* status, ovm_stream_t stream);

/* ---- data feeding ("next" row 2 of SURVEY.md 8f) ---------------------------------------------------------------------------
 * uint8 bilinear resize bit-identical to Pillow's Image.resize(size, BILINEAR), i.e. to detectron2's ResizeShortestEdge on
 * uint8 images (reference demo/demo.py:79-83, cubercnn/data/dataset_mapper.py:62-72). ovm_host_pil_bilinear_coeffs builds one
 * axis' window bounds and 22-bit integer weights on the host (call with null tables to get ksize); ovm_resize_bilinear_u8 runs
 * the horizontal then the vertical pass on the device. src strides are in elements over [H][W][C]. */
int ovm_host_pil_bilinear_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs, int32_t coefs_capacity);
int ovm_resize_bilinear_u8(const uint8_t* src, int32_t H, int32_t W, int32_t C, int64_t sy, int64_t sx, int64_t sc, int32_t outH, int32_t outW,
                           const int32_t* xbounds, const int32_t* xcoefs, int32_t xksize, const int32_t* ybounds, const int32_t* ycoefs,
                           int32_t yksize, uint8_t* tmp, uint8_t* dst, ovm_stream_t stream);

/* fp32 bilinear resize, align_corners=False, no antialias: torch.nn.functional.interpolate(mode="bilinear") as the reference's
 * mapper applies it to a depth prompt (cubercnn/data/dataset_mapper.py:45-52 to the image size, :70-72 through ResizeShortestEdge
 * - detectron2's ResizeTransform takes this route for non-uint8 arrays). src [B][H][W] dense, dst [B][outH][outW], device. */
int ovm_resize_bilinear_f32(const float* src, int32_t B, int32_t H, int32_t W, int32_t outH, int32_t outW, float* dst, ovm_stream_t stream);

/* JPEG decode split behind its entropy stage. The reference reads images with cv2.imread (demo/demo.py:52) and detectron2's
 * read_image = Pillow (cubercnn/data/dataset_mapper.py:38), both libjpeg-turbo at its defaults (JDCT_ISLOW, fancy upsampling,
 * integer YCbCr -> RGB). ovm_host_jpeg_info walks the headers; ovm_host_jpeg_entropy_decode Huffman-decodes every scan on the
 * host into coefficient planes (int16 [coef_blocks][64] in natural order, component after component, each plane bw x bh blocks =
 * whole MCUs); ovm_jpeg_reconstruct dequantises, runs the 8 x 8 inverse DCT, upsamples the chroma and converts the colours on the
 * device into rgb [height][width][3] (planes: device scratch of coef_blocks * 64 bytes). Bit-identical to libjpeg-turbo / Pillow
 * `Image.open(f).convert("RGB")`. Scope: 8-bit Huffman JPEGs - baseline, extended-sequential and progressive (every scan of the
 * progression present) -, grey or 3 components with luma sampling 1x1 / 2x1 / 2x2; anything else (arithmetic coding, 12-bit, CMYK,
 * 4:4:0, an incomplete progression) -> OVM_ERR_UNSUPPORTED from the two host
 * calls, a corrupt stream -> OVM_ERR_INVALID. */
typedef struct OvmJpegInfo {
  int32_t width, height, ncomp;   /* ncomp 1 or 3 */
  int32_t hmax, vmax;             /* luma sampling factors (chroma is 1 x 1) */
  int32_t h[3], v[3];
  int32_t bw[3], bh[3];           /* coefficient plane of each component, in blocks */
  int32_t cw[3], ch[3];           /* component size in samples (ceil(width * h / hmax), ...) */
  int32_t qidx[3];
  int32_t colorspace;             /* 0 grey, 1 YCbCr, 2 RGB (no transform) */
  int32_t coef_blocks;            /* sum of bw * bh */
  uint16_t qt[4][64];             /* quantisation tables, natural order */
} OvmJpegInfo;
int ovm_host_jpeg_info(const uint8_t* data, size_t n, OvmJpegInfo* info);
int ovm_host_jpeg_entropy_decode(const uint8_t* data, size_t n, int16_t* coef, int64_t coef_capacity, OvmJpegInfo* info);
int ovm_jpeg_reconstruct(const int16_t* coef, const OvmJpegInfo* info, uint8_t* planes, uint8_t* rgb, ovm_stream_t stream);

/* The entropy stage on the device: a second route to the coefficient planes, for which only the file's bytes cross PCIe. Huffman
 * streams resynchronise: a decoder started at a wrong bit falls in step with the true one after a few symbols, so the unstuffed
 * stream is cut into subsequences of sub_bits bits, one thread each, whose entry states (bit, block of the MCU, zig-zag index) are
 * relaxed - entry of i + 1 := exit of i - until none changes (csrc/jpeg_dec.hip; the decoding rules are jpeg_dec_core.hpp, shared
 * with the host). The result is int16 [coef_blocks][64], bit for bit what ovm_host_jpeg_entropy_decode writes, for
 * ovm_jpeg_reconstruct to read.
 * Scope: 8-bit Huffman SOF0 / SOF1 with exactly one scan that carries all components in frame order (grey; YCbCr or RGB at 4:4:4,
 * 4:2:2, 4:2:0), standard or optimised tables, with or without restart intervals, EOI right behind the scan. For anything else
 * ovm_host_jpeg_decode_plan returns what ovm_host_jpeg_info returns, or OVM_ERR_UNSUPPORTED: the file takes the host route.
 * The device accepts only what it can prove: result[0] (status, a device word) is 0 only when the marker sequence was the frame's,
 * the entry states reached their fixed point within the rounds allowed, every restart segment completed exactly its blocks inside
 * its own bits (which covers invalid codes, coefficients past index 63 and cut data) and every DC predictor stayed within the
 * host's [-65536, 65535]; the bits are OVM_JPEG_DEC_*. On a non-zero status the planes are undefined and the caller runs the host
 * decoder on the same bytes, which accepts or refuses as it always did: the device never calls a file invalid, it only declines.
 * result[1] = relaxation rounds used: the sum over the sync_launches launches of the largest step count of any workgroup;
 * result[2] = launches in which any thread decoded (at most sync_launches - 1 for an accepted file: a clean launch must follow the
 * last productive one). result is three device words.
 * ovm_host_jpeg_decode_plan: geometry, the scan's byte range ecs_offset / ecs_bytes within the file, table selectors per block of
 * the MCU, and the Huffman tables in the kernels' form into tables (tables_capacity >= tables_bytes = 11008, else
 * OVM_ERR_CAPACITY). max_rounds <= 0: the default (256 = wg_subs, at which a workgroup is certainly consistent).
 * ovm_jpeg_entropy_decode: stream = the ecs_bytes bytes (device, any alignment), tables = the plan's table block (device, 16-byte
 * aligned), ws (16-byte aligned, size from ovm_jpeg_entropy_decode_workspace), coef (16-byte aligned, coef_capacity >=
 * coef_blocks * 64 elements). Stream-ordered, no read back inside; too small a buffer -> OVM_ERR_CAPACITY, nothing launched.
 * ovm_host_jpeg_entropy_emulate: the same stages, rounds schedule and core routine run serially on the CPU (status, rounds and - launches may be null - productive launches as
 * the device reports them): the algorithm's test bed on a machine without a GPU. Returns the plan's code when the plan declines. */
#define OVM_JPEG_DEC_MARKER 1    /* an 0xFF followed by neither 0x00 nor the RSTn that is due */
#define OVM_JPEG_DEC_SEGMENTS 2  /* restart-segment count differs from the frame's, or an empty segment */
#define OVM_JPEG_DEC_NOSYNC 4    /* synchronisation did not converge within the rounds allowed */
#define OVM_JPEG_DEC_COUNT 8     /* a segment completed another number of blocks than the frame needs */
#define OVM_JPEG_DEC_BADCODE 16  /* invalid Huffman code or DC category > 11 */
#define OVM_JPEG_DEC_ZIGZAG 32   /* coefficient at zig-zag index > 63 */
#define OVM_JPEG_DEC_DCRANGE 64  /* DC predictor outside [-65536, 65535] */
typedef struct OvmJpegDecPlan {
  OvmJpegInfo info;
  int64_t ecs_offset, ecs_bytes;            /* the entropy-coded segment within the file (stuffed, with its RSTn markers) */
  int32_t restart_interval;                 /* MCUs per restart segment as the file's DRI states it, 0 = none */
  int32_t mcus_x, mcus_y, blocks_per_mcu, segments;
  int32_t sub_bits, wg_subs, sync_launches, max_rounds;
  int32_t tables_bytes;
  uint8_t sel_comp[8], sel_sub[8], sel_dc[8], sel_ac[8];   /* per block of the MCU: component, index in its h x v, DC / AC table */
} OvmJpegDecPlan;
int ovm_host_jpeg_decode_plan(const uint8_t* data, size_t n, int32_t max_rounds, OvmJpegDecPlan* plan, uint8_t* tables, int64_t tables_capacity);
int ovm_jpeg_entropy_decode_workspace(const OvmJpegDecPlan* plan, int64_t* ws_bytes);
int ovm_jpeg_entropy_decode(const uint8_t* stream, const uint8_t* tables, const OvmJpegDecPlan* plan, uint8_t* ws, int64_t ws_bytes,
                            int16_t* coef, int64_t coef_capacity, int32_t* result, ovm_stream_t stream_handle);
int ovm_host_jpeg_entropy_emulate(const uint8_t* data, size_t n, int32_t max_rounds, int16_t* coef, int64_t coef_capacity,
                                  OvmJpegInfo* info, int32_t* status, int32_t* rounds, int32_t* launches);

/* JPEG encode, entirely on the device: the last step of the two picture paths. The reference hands the finished picture to
 * cv2.imwrite (demo/demo.py:117-121, <name>_combine.jpg / <name>_boxes.jpg) and to Pillow's Image.save (cubercnn/vis/vis.py:274, the
 * evaluation samples) - libjpeg-turbo at its defaults either way. Here the uint8 picture stays in HBM and only the compressed file
 * crosses PCIe; the file is byte for byte the one Pillow's Image.save(f, "JPEG", quality=q[, subsampling=0]) writes.
 *
 * ovm_host_jpeg_encode_plan (host, replaces jpeg_set_quality + the marker writer): geometry, the quality-scaled Annex K quantisation
 * tables and, when header is not null, the header_len bytes in front of the entropy-coded data (SOI, APP0 JFIF 1.01, one DQT per
 * table, SOF0, DHT x 4, SOS; header_capacity >= 623). subsampling uses Pillow's numbering: 0 = 4:4:4, 2 = 4:2:0.
 * ovm_jpeg_encode_workspace: the device scratch ovm_jpeg_encode needs and the output capacity header_len + 416 * coef_blocks + 16
 * (a block emits at most 22 + 63 * 26 = 1660 bits < 208 bytes, at most doubled by byte stuffing).
 * ovm_jpeg_forward (replaces libjpeg's colour conversion, downsampling, forward DCT and quantisation): img is device uint8 [H][W][3]
 * in R, G, B order addressed by element strides (sy, sx, sc) - sc may be negative, so a BGR picture is passed as (base + 2, sc = -1);
 * coef receives int16 [coef_blocks][64] in the layout ovm_jpeg_reconstruct reads; ws needs coef_blocks * 64 bytes here.
 * ovm_jpeg_encode (replaces Image.save / cv2.imwrite's encoder): the whole file into out, its length into *out_len (both device
 * memory; header is the host buffer the plan filled). Stream-ordered, no read back inside the call. ws and coef of the two device
 * calls are 16-byte aligned (else OVM_ERR_INVALID).
 * Scope: 8-bit baseline, three components YCbCr, luma sampling 2x2 or 1x1, standard Huffman tables, one interleaved scan, no restart
 * markers. Quality outside 1..100 or a size outside 1..65535 -> OVM_ERR_INVALID; another subsampling -> OVM_ERR_UNSUPPORTED; too small
 * a workspace or output -> OVM_ERR_CAPACITY (nothing is launched). Not offered: greyscale, 4:2:2 / 4:4:0, progressive and
 * optimised-Huffman files, custom tables, dpi / EXIF / ICC / comment segments, 12-bit samples. */
typedef struct OvmJpegEncInfo {
  int32_t width, height, quality, hs, vs;   /* hs, vs: luma sampling, 2,2 or 1,1 */
  int32_t bw[3], bh[3];                     /* coefficient plane of each component, in blocks (whole MCUs) */
  int32_t mcus_x, mcus_y, coef_blocks, header_len;
  uint16_t qt[2][64];                       /* natural order */
} OvmJpegEncInfo;
int ovm_host_jpeg_encode_plan(int32_t width, int32_t height, int32_t quality, int32_t subsampling, OvmJpegEncInfo* info, uint8_t* header,
                              int32_t header_capacity);
int ovm_jpeg_encode_workspace(const OvmJpegEncInfo* info, int64_t* ws_bytes, int64_t* out_capacity);
int ovm_jpeg_forward(const uint8_t* img, int64_t sy, int64_t sx, int64_t sc, const OvmJpegEncInfo* info, uint8_t* ws, int64_t ws_bytes,
                     int16_t* coef, ovm_stream_t stream);
int ovm_jpeg_encode(const uint8_t* img, int64_t sy, int64_t sx, int64_t sc, const OvmJpegEncInfo* info, const uint8_t* header, uint8_t* ws,
                    int64_t ws_bytes, uint8_t* out, int64_t out_capacity, int64_t* out_len, ovm_stream_t stream);

/* ---- Visualisation ----------------------------------------------------------------------------------------------------------
 * draw_scene_view(mode in {front, novel, front_and_novel}) of the reference (cubercnn/vis/vis.py:309-640, edges :673-748, labels
 * :755-784): the input image with the boxes rendered, blended and outlined, and a top-down "novel" view of the same boxes over a
 * ground grid. The reference draws with pytorch3d (MeshRasterizer + SoftPhongShader) and cv2; the rules below restate those calls
 * and are pinned by the numpy restatement tests/scene_oracle.py, not by the two libraries (neither is available to compare).
 *
 * ovm_host_scene_layout (host, fp64, no GPU): per-view box frames, depth order, the zoom search (:442-478), the ground bounds
 * (:488-533, with the reference's quirks), the deduplicated grid segment set (:557-579), edge endpoints after zplane clipping and
 * the label rectangles. ovm_render_scene (device, one stream-ordered call): triangle setup, per-tile culling, rasterisation,
 * Phong shading, softmax blend, grid, edges, labels and the overlay, written once as BGR uint8.
 *
 * Declared deviations from the reference:
 *  - triangles are clipped against z = zplane before projection (pytorch3d does not clip); a clipped triangle becomes up to two;
 *  - a pixel (row i, col j) samples the image point (j + 0.5, i + 0.5) under K; covered = edge functions all >= 0 or all <= 0;
 *  - thick lines: a pixel is covered when its integer centre lies within thickness / 2 of the segment (cv2 draws a polygon with
 *    round caps); the segment is clipped to the canvas grown by that radius, which leaves the covered set unchanged;
 *  - label glyphs are a coverage mask made by the caller (Pillow's built-in font, not cv2's Hershey font); the text size used
 *    for the background rectangle is that mask's size;
 *  - box colours come from the caller (the reference jitters them with an unseeded RNG);
 *  - the depth order is a stable sort of the mean corner y (the reference's default argsort is not stable for > 16 boxes);
 *  - host geometry is fp64 throughout (the reference's torch part is fp32); shading is fp32 as in pytorch3d. */
#define OVM_SCENE_MAX_BOXES 1024
#define OVM_SCENE_FRONT 1   /* mode bits */
#define OVM_SCENE_NOVEL 2

typedef struct OvmSceneInput {
  int32_t n_boxes, mode;            /* 0..OVM_SCENE_MAX_BOXES; OVM_SCENE_FRONT | OVM_SCENE_NOVEL */
  int32_t height, width, scale;     /* front image height x width; novel canvas scale x scale */
  int32_t has_T, has_ground_bounds, has_labels;
  double K[9], R[9], T[3];          /* row-major K; novel view rotation R (euler2mat([pi/3, 0, 0]) in the reference); T */
  double ground_bounds[5];          /* max_y3d, x3d_start, x3d_end, z3d_start, z3d_end */
  double blend_weight, blend_weight_overlay, zplane;
  const double* corners;            /* [n_boxes][8][3] camera-space corners, pred_bbox3D order */
  const float* colors;              /* [n_boxes][3] in [0, 1]; component k lands in image channel k */
  const int32_t* label_size;        /* [2 views][n_boxes][2] glyph mask (width, height); read when has_labels */
} OvmSceneInput;

typedef struct OvmSceneBox {        /* one box in one view */
  double verts[8][3];               /* corners in the view's camera frame */
  int64_t edge[12][4];              /* int() of the projected endpoints after zplane clipping: u0, v0, u1, v1 */
  int32_t edge_drawn[12];           /* 0 when both endpoints are behind zplane */
  int32_t rect[4];                  /* label background, half-open x0, y0, x1, y1 on the canvas (empty when x1 <= x0 or y1 <= y0) */
  int32_t text_org[2];              /* bottom-left corner of the glyph mask: the mask covers rows [y - h, y), cols [x, x + w) */
  int32_t label_w, label_h;         /* glyph mask size (0 x 0: no label) */
} OvmSceneBox;

typedef struct OvmSceneView {
  int32_t height, width, thickness, drawn;    /* drawn = 0: the view is not produced */
  double K[9];
  int32_t order[OVM_SCENE_MAX_BOXES];         /* draw order: reversed stable argsort of the mean corner y */
  OvmSceneBox box[OVM_SCENE_MAX_BOXES];
} OvmSceneView;

typedef struct OvmSceneLayout {
  int32_t n_boxes, mode, early_return;        /* early_return: empty grid mask (:522-526) - front = the input, novel = the bare render */
  int32_t grid_thickness, n_grid, reserved;
  double zoom_factor, zoom_bias, center[3];
  double ground[5];                           /* max_y3d, x3d_start, x3d_end, z3d_start, z3d_end of the drawn grid */
  double blend_weight, blend_weight_overlay, zplane;
  double edge_color[OVM_SCENE_MAX_BOXES][3];  /* min(255, c * 255 * 1.25): the label background */
  uint8_t edge_u8[OVM_SCENE_MAX_BOXES][4];    /* [0..2] edge colour rounded half to even, [3] text colour (0 or 255) */
  float color[OVM_SCENE_MAX_BOXES][3];        /* texel colour c */
  OvmSceneView view[2];                       /* 0 front, 1 novel */
} OvmSceneLayout;

typedef struct OvmSceneSegment { int64_t x0, y0, x1, y1; } OvmSceneSegment;

/* Fills *out and grid[0 .. out->n_grid) (sorted ascending). OVM_ERR_CAPACITY, with out->n_grid set to the count needed, when
 * grid_capacity is too small; OVM_ERR_INVALID for null, non-finite or out-of-range arguments. */
int ovm_host_scene_layout(const OvmSceneInput* in, OvmSceneLayout* out, OvmSceneSegment* grid, int32_t grid_capacity);
/* Device workspace bytes ovm_render_scene needs for this layout and glyph buffer. */
int ovm_render_scene_workspace(const OvmSceneLayout* layout, int64_t glyph_bytes, int64_t* bytes);
/* layout, grid, glyphs: host. glyphs: the masks of view 0 boxes 0..n-1, then view 1 boxes 0..n-1, each label_h x label_w bytes
 * row-major, nonzero = ink; glyph_bytes must equal their total. image: device BGR uint8 [height][width][3] with a row pitch in
 * bytes; front / novel: device outputs of the views the layout draws (null otherwise), row pitches in bytes - front and novel may
 * be the two halves of one height x (width + scale) x 3 buffer. Too small a workspace -> OVM_ERR_CAPACITY; null or inconsistent
 * arguments -> OVM_ERR_INVALID, both before any device work. */
int ovm_render_scene(const OvmSceneLayout* layout, const OvmSceneSegment* grid, const uint8_t* glyphs, int64_t glyph_bytes,
                     const uint8_t* image, int64_t image_pitch, uint8_t* front, int64_t front_pitch, uint8_t* novel, int64_t novel_pitch,
                     void* workspace, int64_t workspace_bytes, ovm_stream_t stream);

/* ovm_render_scene with the scene's geometry under the boxes of the novel view: a metric depth map of the front image, splatted
 * as a z-buffered point cloud. A layer of this project (declared deviation: the reference draws the boxes over the bare grid);
 * the rules are restated in numpy by tests/scene_points_oracle.py.
 *
 * Pass A (scene_splat, one thread per front pixel (i, j), fp64 with contraction off): d = depth[i][j]; the pixel is skipped unless
 * d is finite and > 0. Camera point under the renderer's sampling convention, X = ((j + 0.5) - K[2]) / K[0] * d,
 * Y = ((i + 0.5) - K[5]) / K[4] * d, Z = d with the front view's K; novel frame as the layout moves box corners,
 * r = R (p - center) summed left to right, r[2] += zoom_bias * zoom_factor; skipped unless r[2] >= zplane and r[2] > 0;
 * (x, y) = floor of K_novel r / r[2]. Key = float bits of (float)r[2] in the high word, i * width + j in the low word: the nearest
 * point wins, the lower source index on a tie. The key goes, by 64-bit atomicMin, to every canvas pixel of the point_size x
 * point_size square centred on (x, y); the buffer starts as all ones (no point), and its final state does not depend on the
 * execution order.
 * Pass B (inside scene_tiles): only where a novel-view pixel has no triangle - the pixel that is otherwise the canvas (225) or
 * grid (175) grey. With a key there the base colour is the image's BGR at the winning source pixel, and with labels given and
 * 0 <= labels[i][j] < n_boxes there it is tinted, (image[ch] + edge_u8[b][ch] + 1) >> 1 (any other label value: no tint). Box
 * faces stay on top, edges and labels are drawn after as before, the front view is ovm_render_scene's. With early_return set
 * nothing is splatted: both views are ovm_render_scene's and the key buffer stays all ones.
 *
 * depth: device fp32 [height][width] of the front view; labels: device int32 of the same shape or null; both with a row pitch in
 * bytes (a multiple of 4, at least one row). R: host, the rotation given to ovm_host_scene_layout (the layout does not keep it).
 * point_size: odd, 1..9. zbuf_out: null, or device uint64 [scale][scale] that receives the key buffer. The layout must draw both
 * views. A null depth or R, a bad pitch or point_size, a layout without both views -> OVM_ERR_INVALID, before any device work.
 * The workspace is ovm_render_scene's plus the key buffer: ovm_render_scene_points_workspace. */
int ovm_render_scene_points_workspace(const OvmSceneLayout* layout, int64_t glyph_bytes, int64_t* bytes);
int ovm_render_scene_points(const OvmSceneLayout* layout, const OvmSceneSegment* grid, const uint8_t* glyphs, int64_t glyph_bytes,
                            const uint8_t* image, int64_t image_pitch, uint8_t* front, int64_t front_pitch, uint8_t* novel,
                            int64_t novel_pitch, const float* depth, int64_t depth_pitch, const int32_t* labels, int64_t labels_pitch,
                            const double* R, int32_t point_size, uint64_t* zbuf_out, void* workspace, int64_t workspace_bytes,
                            ovm_stream_t stream);

/* ---- Visualisation: evaluation sample panels -------------------------------------------------------------------------------
 * visualize_from_instances of the reference (cubercnn/vis/vis.py:76-296): per sampled image a 2H x 3W mosaic of six copies of
 * the image - columns: ground truth of all classes, ground truth of the evaluated classes, predictions; top row the 2D boxes,
 * bottom row the 3D boxes (draw_3d_box_from_verts :695-728, draw_text :755-783). The rules are pinned by the numpy restatement
 * tests/panels_oracle.py; parity with cv2 is unpinned (cv2 is not available to compare).
 *
 * ovm_host_panels_layout (host, fp64, no GPU) turns the boxes into the ordered primitive list of each panel; ovm_render_panels
 * (device, one stream-ordered call) applies each panel's list, strictly in order, to a copy of the image and writes the mosaic.
 * Primitives, in the reference's drawing order (a later primitive overwrites an earlier one):
 *  - 2D panels, per box: the outline (int() of x, y, x + w, y + h) as four segments of thickness 2 - top, right, bottom, left -
 *    in the class colour, then the class name's glyphs in the class colour, the mask's bottom-left at (int(x), int(y) - 10);
 *  - 3D panels, per box with draw3d: the cuboid's corners (get_cuboid_verts_faces order) are R @ (+-l/2, +-h/2, +-w/2) +
 *    center; its 12 edges in the order 0-1 1-2 2-3 3-0 1-5 5-6 6-2 4-5 4-7 6-7 0-4 3-7, each dropped when both ends lie behind
 *    zplane = 0.05 and else cut at it (eps 1e-4) and projected, int() of the endpoints; then the label: the background
 *    rectangle of draw_text at int() of the 2D box's x, y, clipped to the image, blended px * 0.33 + bg * (1 - 0.33) in fp64
 *    (two products, one sum, truncated), then the glyphs in black or white by the mean of bg (> 127.5: black);
 *  - the middle column holds only the ground-truth boxes with in_eval set.
 * Declared deviations from the reference (the first four are the scene view's, above):
 *  - thick lines: a pixel is covered when its integer centre lies within thickness / 2 of the segment;
 *  - glyphs are a coverage mask made by the caller (Pillow's built-in font); putText's stroke thickness is ignored; the text size
 *    of the label rectangle is the mask's size, and a box with an empty 0 x 0 mask gets no glyphs and no label rectangle;
 *  - colours come from the caller (a deterministic colour per category_id);
 *  - host geometry is fp64 (the reference's get_cuboid_verts is fp32);
 *  - the 3D line thickness is max(1, int(round_half_even(3 * H / 500))): cv2 refuses thickness 0, which the reference's formula
 *    gives below H = 84. */
#define OVM_PANELS 6              /* 0 gt_all_2d, 1 gt_2d, 2 pred_2d, 3 gt_all_3d, 4 gt_3d, 5 pred_3d: row-major in the mosaic */
#define OVM_PANEL_SEGMENT 0
#define OVM_PANEL_BLEND 1
#define OVM_PANEL_GLYPH 2

typedef struct OvmPanelBox {
  double bbox[4];                 /* x, y, w, h */
  double center[3], dims[3];      /* camera-space centre; w, h, l */
  double R[9];                    /* row-major pose */
  uint8_t color[4];               /* class colour; component k lands in image channel k ([3] unused) */
  int32_t draw3d;                 /* the cuboid and its label are drawn (a prediction: score > threshold) */
  int32_t in_eval;                /* ground truth: also drawn in the middle column (ignored for predictions) */
  int32_t glyph2d[2], glyph3d[2]; /* (width, height) of the name's mask at scale 0.5, and at scale 0.5 * H / 500 */
} OvmPanelBox;

typedef struct OvmPanelsInput {
  int32_t height, width, n_gt, n_pred;
  double K[9];
  const OvmPanelBox* gt;          /* [n_gt] */
  const OvmPanelBox* pred;        /* [n_pred] */
} OvmPanelsInput;

typedef struct OvmPanelPrim {
  int32_t kind, thickness;        /* OVM_PANEL_*; thickness of a segment */
  int64_t a[4];                   /* segment: x0, y0, x1, y1; blend: half-open x0, y0, x1, y1; glyph: top-left x, y, then w, h */
  int64_t glyph_offset;           /* glyph: byte offset of its h x w mask in the glyph buffer */
  uint8_t color[4];               /* segment and glyph colour, blend background ([3] unused) */
  int32_t box;                    /* source: index into gt (panels 0, 1, 3, 4) or pred (panels 2, 5) */
} OvmPanelPrim;

typedef struct OvmPanelsLayout {
  int32_t height, width, thickness3d, n_prims;   /* n_prims: the count needed, also on OVM_ERR_CAPACITY */
  int32_t start[OVM_PANELS + 1];                 /* panel p owns prims[start[p] .. start[p + 1]) */
  int32_t reserved;
  int64_t glyph_bytes;                           /* size of the glyph buffer the offsets index */
} OvmPanelsLayout;

/* Glyph buffer order: per ground-truth box its 2D mask then its 3D mask, then the same per prediction, each h x w bytes
 * row-major, nonzero = ink. Fills *out and prims[0 .. out->n_prims). OVM_ERR_CAPACITY, with out->n_prims set to the count
 * needed, when prim_capacity is too small; OVM_ERR_INVALID for null, non-finite or out-of-range arguments. */
int ovm_host_panels_layout(const OvmPanelsInput* in, OvmPanelsLayout* out, OvmPanelPrim* prims, int32_t prim_capacity);
/* Device workspace bytes ovm_render_panels needs for this layout. */
int ovm_render_panels_workspace(const OvmPanelsLayout* layout, int64_t* bytes);
/* layout, prims, glyphs: host. image: device BGR uint8 [height][width][3], row pitch in bytes; mosaic: device
 * [2 * height][3 * width][3], row pitch in bytes, must not overlap image. One pinned upload, one kernel, stream-ordered, no
 * allocation once the pinned buffer has grown to size. Too small a workspace -> OVM_ERR_CAPACITY; null, inconsistent or
 * out-of-range arguments (a glyph whose mask leaves the buffer, a start[] that is not ascending) -> OVM_ERR_INVALID, both before
 * any device work. */
int ovm_render_panels(const OvmPanelsLayout* layout, const OvmPanelPrim* prims, const uint8_t* glyphs, int64_t glyph_bytes,
                      const uint8_t* image, int64_t image_pitch, uint8_t* mosaic, int64_t mosaic_pitch, void* workspace,
                      int64_t workspace_bytes, ovm_stream_t stream);

/* ---- Mask run-length encoding -----------------------------------------------------------------------------------------------
 * COCO's RLE of binary masks, produced and consumed in HBM: only the strings cross PCIe. The rules are restated from pycocotools'
 * maskApi.c (rleEncode, rleToString, rleFrString); pycocotools is not a dependency, the numpy restatement is
 * tests/mask_rle_oracle.py.
 *
 * Counts. A plane is uint8 [H][W], row-major, nonzero = inside, and is scanned column-major: position p = x * H + y. counts are
 * the lengths of the alternating runs along p, the first one a run of zeros: a plane whose first pixel is set starts with count
 * 0, an all-zero plane is [H * W], an all-one plane [0, H * W]. A run continues across a column boundary (pixel (H - 1, x) and
 * pixel (0, x + 1) are neighbours). A plane with T value changes along p (the change from the implied 0 in front of p = 0
 * included) has T + 1 counts.
 * String. For count i: x = cnts[i], x -= cnts[i - 2] when i > 2 (signed 64-bit); then repeat { c = x & 0x1f; x >>= 5
 * (arithmetic); more = (c & 0x10) ? x != -1 : x != 0; if (more) c |= 0x20; emit the byte c + 48 } while more.
 * The inverse (rleFrString) reads groups of 5 bits until one without 0x20, sign-extends when that last group has 0x10 set, and
 * adds cnts[m - 2] when m > 2; it is host code of the Python layer (ovmono3d_amd.masks), the device takes and gives counts.
 * H * W <= 2^31 - 1 (counts are uint32, as in COCO), so a difference of two counts lies within +-(2^31 - 1), which is 32 bits with
 * its sign: OVM_MASK_RLE_MAX_CHARS = ceil(32 / 5) = 7 bytes per count at the most. max_bytes = 7 * max_runs always suffices.
 *
 * ovm_mask_rle_encode: masks device uint8, plane i at masks + i * plane_stride, row y at + y * row_pitch (bytes; any alignment,
 * so a crop of a larger tensor is taken as it is). run_offsets / str_offsets: device int64 [n + 1], the first run / first string
 * byte of each plane in counts_out (device uint32 [max_runs]) / string_out (device uint8 [max_bytes]); entry n is the total.
 * counts_out may be null (no counts wanted), string_out and str_offsets may be null (no strings wanted; string_out without
 * str_offsets is OVM_ERR_INVALID). status: device int32 [4] = code, total runs, total bytes, reserved (totals saturate at
 * 2^31 - 1; run_offsets[n] and str_offsets[n] hold them in 64 bits).
 * The runs and (when strings are wanted) the string bytes of every plane are always counted exactly, and run_offsets and
 * str_offsets are always written. Runs and bytes are written only if the totals fit: total runs <= max_runs, else code =
 * OVM_ERR_CAPACITY and nothing is written to counts_out or string_out (the string lengths then come from two more walks over the
 * planes instead of the stored runs); total bytes <= max_bytes, else code = OVM_ERR_CAPACITY, counts_out written and string_out
 * untouched. A caller reads status once and on OVM_ERR_CAPACITY calls once more with the stated totals: that call fits.
 * Launches go on the caller's stream only; no read back, no allocation, no synchronisation. Workgroups of 64 columns x 4 bands
 * of 64 rows read a plane coalesced in its own order (the value in front of pixel (y, x) is (y - 1, x), or (H - 1, x - 1) for
 * y = 0: no transpose): pass 1 counts the value changes per (plane, column, band), one exclusive scan in column-major order ranks
 * them, pass 2 stores the positions at their ranks; then per count its length, one 64-bit scan, the scatter. Integer arithmetic
 * throughout: the output does not depend on scheduling.
 *
 * ovm_mask_rle_decode: counts device uint32 [total_runs] (16-byte aligned), run_offsets device int64 [n + 1] as above; plane i is
 * written as 0 / 1 bytes into masks_out (same addressing as the encoder's input). A prefix sum of the counts, then each (column,
 * band) finds the run of its first pixel by bisection and walks on; the value is run & 1. status: device int32 [4] = code, number
 * of bad planes, index of the first bad plane or -1, reserved. A plane is bad when its counts do not sum to H * W or its offsets
 * are not within 0 <= run_offsets[i] <= run_offsets[i + 1] <= total_runs (they are clamped to that before use): code =
 * OVM_ERR_INVALID; pixels past the sum of a short plane are 0. Like ovm_jpeg_encode's out_len the word is device memory and the
 * call does not wait for it.
 *
 * Refused before any device work: a null pointer (other than the optional ones), n < 1, H < 1, W < 1, H * W > 2^31 - 1,
 * row_pitch < W, max_runs < 1, max_bytes < 1 with a string wanted, total_runs < 1, a workspace that is not 16-byte aligned
 * (OVM_ERR_INVALID); a workspace below what the _workspace call states, or more than 2^24 - 1 workgroups of 64 columns x 256 rows (OVM_ERR_CAPACITY: split
 * the planes over several calls).
 * Scope: 8-bit planes. Not built: toBbox, merge and iou on RLEs (ovm_sam_mask_boxes and the evaluator cover boxes and IoU),
 * polygons. */
#define OVM_MASK_RLE_MAX_CHARS 7
int ovm_mask_rle_encode_workspace(int32_t n, int32_t H, int32_t W, int64_t max_runs, int64_t max_bytes, int64_t* bytes);
int ovm_mask_rle_encode(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W,
                        uint32_t* counts_out, int64_t max_runs, int64_t* run_offsets, uint8_t* string_out, int64_t max_bytes,
                        int64_t* str_offsets, int32_t* status, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
int ovm_mask_rle_decode_workspace(int32_t n, int32_t H, int32_t W, int64_t total_runs, int64_t* bytes);
int ovm_mask_rle_decode(const uint32_t* counts, const int64_t* run_offsets, int64_t total_runs, int32_t n, int32_t H, int32_t W,
                        uint8_t* masks_out, int64_t plane_stride, int64_t row_pitch, int32_t* status, void* workspace,
                        int64_t workspace_bytes, ovm_stream_t stream);

/* ---- Mask label map and mask picture ----------------------------------------------------------------------------------------
 * A layer of this project (declared deviation: the reference draws no masks). Integer arithmetic only: the output is defined to
 * the byte; the numpy restatement is tests/mask_overlay_oracle.py.
 *
 * ovm_mask_labels: labels_out[y][x] (device int32, row pitch label_pitch in elements) = the lowest plane index i with
 * masks[i][y][x] != 0, or -1: what vis.labels_from_masks computes, without an n x H x W temporary (a lane stops at its first
 * covering plane). masks as ovm_mask_rle_encode takes them; n = 0 (masks may then be null) gives -1 everywhere.
 * ovm_render_mask_overlay: image and out are device uint8 [H][W][3] with row pitches in bytes (out may be image itself), colors
 * device uint8 [n][3] in the image's channel order, alpha 0..255. With b = labels[y][x]:
 *   b < 0 or b >= n                       out = image
 *   contour: one of the 4-neighbours that lie inside the image has a label other than b (-1 included): out = colors[b]
 *   otherwise                             out = (image * (255 - alpha) + colors[b] * alpha + 127) / 255 per channel, integer division
 * The image border is not contour by itself. OVM_ERR_INVALID, nothing launched: a null pointer (colors may be null when n = 0),
 * n < 0, H < 1, W < 1, a pitch below one row, alpha outside 0..255; OVM_ERR_CAPACITY: H > 262140. Stream-ordered. */
int ovm_mask_labels(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W,
                    int32_t* labels_out, int64_t label_pitch, ovm_stream_t stream);
int ovm_render_mask_overlay(const uint8_t* image, int64_t image_pitch, const int32_t* labels, int64_t label_pitch,
                            const uint8_t* colors, int32_t n, int32_t alpha, uint8_t* out, int64_t out_pitch, int32_t H, int32_t W,
                            ovm_stream_t stream);

/* ---- Mask connected components ----------------------------------------------------------------------------------------------
 * Connected-component labelling of binary planes in HBM, and segment_anything's small-region clean-up (utils/amg.py
 * remove_small_regions, restated) on top of it. Everything is integer arithmetic and defined exactly; the reference for the labels is
 * scipy.ndimage.label, the numpy restatement of the clean-up is tests/mask_cc_oracle.py.
 *
 * Planes are addressed as ovm_mask_rle_encode takes them (plane i at masks + i * plane_stride, row y at + y * row_pitch, bytes, any
 * alignment). Foreground is a byte != 0, or == 0 with invert != 0. connectivity is 4 (edge neighbours) or 8 (edge and corner).
 *
 * ovm_mask_cc_label: labels_out device int32, pixel (y, x) of plane i at labels_out + i * label_plane_stride + y * label_pitch + x
 * (elements); background is 0. counts_out device int32 [n]: the number of components of each plane.
 * Label rule. The components of a plane are numbered 1, 2, ... in row-major order of their first pixel: scipy.ndimage.label's
 * numbering (structure: the cross for 4, ones((3, 3)) for 8). The unions always hook the larger root under the smaller, so a
 * component's root is its first pixel, and its label is the rank of that root among the plane's roots (one prefix sum).
 *
 * ovm_mask_remove_small_regions: mode 1 = holes, 2 = islands, 3 = holes, then islands on the result. masks_out device uint8 planes of
 * 0 / 1 (out_plane_stride, out_row_pitch in bytes) that must overlap neither the input nor each other (n > 1:
 * |out_plane_stride| >= (H - 1) * out_row_pitch + W); changed_out device int32 [n].
 * Clean-up rule, per plane and step. The working plane is the mask for islands and its complement for holes; connectivity is 8 in
 * both; the outer background is a region like any other. A region is small when area < min_area (strict). No small region: the
 * plane is copied (as 0 / 1) and changed = 0. Otherwise changed = 1 and: holes - the small regions of the complement are filled;
 * islands - the small regions are cleared, and when every region is small the largest one is kept, on a tie the one that comes first
 * in label order (argmax's first). Mode 3: changed is the OR of the two steps.
 *
 * status: device int32 [4] = code, number of threads that gave up, reserved, reserved. Every walk through the union-find forest
 * counts its steps against a bound derived from H * W (a walk only ever moves to smaller indices, so the bound cannot be reached);
 * a thread that reaches it, or meets an index that cannot be a parent, sets code = OVM_ERR_HIP and ends: a defect comes back as a
 * code, not as a hang. The outputs are then undefined. Like ovm_mask_rle_encode's status it is device memory and the call does
 * not wait for it.
 * Launches go on the caller's stream only: no read back, no allocation, no synchronisation. Their number is fixed (7 for labels, 5
 * per clean-up step) and does not depend on what the planes hold. One wave owns 64 consecutive pixels of a row; the unions
 * within those cost a ballot, the others are atomicMin hooks on roots in global memory, made only where a contact between two rows
 * begins. No decision relies on a plain load seeing what another workgroup wrote in the same launch: a union takes its decisions
 * from the atomics' return values and treats a plain read of a parent as a hint (parents only move to smaller indices of the same
 * component, so an old parent is still an ancestor). Region areas are summed within the wave first: one atomicAdd per distinct
 * root among its lanes. Outputs do not depend on scheduling; two calls give equal bytes.
 *
 * Refused before any device work: a null pointer, n < 1, H < 1, W < 1, H * W > 2^31 - 1, row_pitch, label_pitch or out_row_pitch
 * below W, connectivity outside {4, 8}, mode outside 1..3, min_area < 1, masks_out overlapping masks or its own planes, a workspace that is not
 * 16-byte aligned (OVM_ERR_INVALID); a workspace below what the _workspace call states, or more than 2^24 - 1 workgroups of 4
 * row segments of 64 pixels (OVM_ERR_CAPACITY: split the planes over several calls).
 * Scope: 8-bit planes. Not built: component statistics tables (boxes, centroids). */
int ovm_mask_cc_label_workspace(int32_t n, int32_t H, int32_t W, int64_t* bytes);
int ovm_mask_cc_label(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W, int32_t connectivity,
                      int32_t invert, int32_t* labels_out, int64_t label_plane_stride, int64_t label_pitch, int32_t* counts_out, int32_t* status,
                      void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
int ovm_mask_remove_small_regions_workspace(int32_t n, int32_t H, int32_t W, int64_t* bytes);
int ovm_mask_remove_small_regions(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W, int64_t min_area,
                                  int32_t mode, uint8_t* masks_out, int64_t out_plane_stride, int64_t out_row_pitch, int32_t* changed_out,
                                  int32_t* status, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);

/* ---- Scene as a PLY file ----------------------------------------------------------------------------------------------------
 * <name>_scene.ply: the un-projected depth map and the boxes as one binary little-endian PLY 1.0 file, the 3D counterpart of the
 * novel view (a layer of this project; the reference's GEO script shows Open3D line sets over the cloud, tools/ovmono3d_geo.py:
 * 89-104, 209). The device packs the point records; the header, the box part and the file are host work of the Python layer
 * (ovmono3d_amd.vis.scene_ply). The numpy restatement is tests/scene_ply_oracle.py; the file is defined to the byte.
 *
 *   ply / format binary_little_endian 1.0 / comment ovmono3d_amd scene, frame <camera|opengl>, metres
 *   element vertex <P + 8 n>   property float x, y, z; property uchar red, green, blue          15 bytes per vertex
 *   element face <12 n>        property list uchar int vertex_indices                           13 bytes per face (3, a, b, c)
 *   element edge <12 n>        property int vertex1; property int vertex2                       8 bytes per edge
 *   end_header
 *
 * Points, P records in row-major pixel order. Pixel (i, j) with i % stride == 0 and j % stride == 0 is kept when d = depth[i][j]
 * is finite, d > 0 and, with max_depth > 0, d <= max_depth (compared as floats). Its position is Pass A's camera point above, in
 * fp64 with contraction off, X = ((j + 0.5) - K[2]) / K[0] * d, Y = ((i + 0.5) - K[5]) / K[4] * d, Z = d, each rounded once to
 * float32: the file and the picture show the same points. Its colour is Pass B's base colour: the image's BGR there, with labels
 * given and 0 <= labels[i][j] < n_boxes each channel tinted (c + tint[b][ch] + 1) >> 1; written red = channel 2, green = channel
 * 1, blue = channel 0.
 * Boxes (host): 8 vertices per box, the fp64 corners in pred_bbox3D order rounded to float32, in the box's edge_u8 colour with the
 * same channel swap; the 12 triangles of the renderer's face table (per face (a, b, c, d) of front 0 1 2 3, right 1 5 6 2, left
 * 4 0 3 7, back 5 4 7 6, top 4 5 1 0, bottom 3 2 6 7: a b c, then c d a); the 12 edges in the panels' order above; indices
 * offset by P + 8 b.
 * flip = 1 (frame "opengl") negates y and z of every vertex, the reference's flip_matrix: exact. flip = 0 ("camera") agrees with
 * <name>_dets.json.
 *
 * ovm_scene_ply_points: image device BGR uint8 [H][W][3], depth device fp32 [H][W], labels device int32 [H][W] or null, row pitches
 * in bytes (depth and labels: multiples of 4; each at least one row). tint: host uint8 [n_boxes][4] ([3] unused), required with
 * labels. K: host, row-major [9]. out: device, out_bytes >= ceil(H / stride) * ceil(W / stride) * 15 (the worst case), receives
 * exactly 15 P bytes; no byte at or past 15 P is written. count: device uint64, receives P. Launches go on the caller's stream only:
 * no allocation, no read back, no synchronisation (the tint rows are copied to the workspace stream-ordered). One workgroup per
 * tile of 2,048 kept pixels counts its valid ones, ovm_scan ranks the tiles, and the same workgroup packs its records in LDS and
 * stores its own byte range [15 r0, 15 r1) - bytes up to the first 16-byte boundary, 16-byte stores, bytes - so no store covers a
 * byte of another workgroup's range. Integer ranks: the bytes do not depend on scheduling.
 * OVM_ERR_INVALID: a null pointer (labels and tint may be null), H < 1, W < 1, H * W > 2^31 - 1, stride outside 1..16, n_boxes
 * outside 0..OVM_SCENE_MAX_BOXES, a pitch below one row or (depth, labels) not a multiple of 4, labels without tint, flip other than
 * 0 / 1, a NaN max_depth, a non-finite K or a zero focal length, a workspace not 16-byte or a count not 8-byte aligned.
 * OVM_ERR_CAPACITY: out_bytes below the worst case or a workspace below ovm_scene_ply_points_workspace. Both before any device
 * work; nothing is written then. */
int ovm_scene_ply_points_workspace(int32_t H, int32_t W, int32_t stride, int32_t n_boxes, int64_t* bytes);
int ovm_scene_ply_points(const uint8_t* image, int64_t image_pitch, const float* depth, int64_t depth_pitch, const int32_t* labels,
                         int64_t labels_pitch, const uint8_t* tint, int32_t n_boxes, int32_t H, int32_t W, const double* K,
                         int32_t stride, float max_depth, int32_t flip, uint8_t* out, int64_t out_bytes, uint64_t* count,
                         void* workspace, int64_t workspace_bytes, ovm_stream_t stream);

/* ---- OVMono3D-GEO -----------------------------------------------------------------------------------------------------------
 * The training-free baseline of the reference (tools/ovmono3d_geo.py:127-258): a 2D box's mask pixels are un-projected with a
 * metric depth map, the cloud is yaw-aligned by the first principal direction of its (x, z) columns, outliers are removed with
 * DBSCAN (up to `trials` runs, eps doubling), and the box is the extent of the kept points. Of the two networks in front of it,
 * SAM and Depth Pro are in this library (OvmSam, OvmDepthPro below: their planes and depth maps are what `mask` and `depth` take).
 *
 * Steps, all in fp64 as the reference (the numpy restatement is tests/geo_oracle.py):
 *  1. points, row-major over the mask pixels: z = depth[y][x]; p = (z (x - cx) / fx, -(z (y - cy) / fy), -z)
 *  2. offset = mean(p), X = p - offset
 *  3. yaw = atan2(v[1], v[0]), v the unit eigenvector of the larger eigenvalue of the 2 x 2 covariance of X's (x, z) columns, its
 *     sign scikit-learn's (the entry of larger magnitude is positive; on equal magnitudes the first)
 *  4. T = Ry(-yaw) X + offset, Ry(a) = [[cos a, 0, -sin a], [0, 1, 0], [sin a, 0, cos a]]
 *  5. more than max_points rows: keep rows perm[0 .. max_points) (perm: the caller's permutation of 0 .. n-1; the reference's is
 *     numpy.random.RandomState(42).shuffle(arange(n)))
 *  6. trial t = 1 .. trials at eps = eps0 * 2^(t-1): DBSCAN(eps, min_samples), Euclidean, a point counts itself, d <= eps; a
 *     cluster is kept unless size / n < min_cluster_frac or size <= min_cluster; the trial is accepted when kept > accept_frac * n;
 *     no trial accepted: every point is kept (trial 0)
 *  7. the extents are the kept points' min / max per axis of the rotated frame.
 * ovm_host_geo_box turns the result into the reference's box (its gen_8corners order, rotation back, y / z flip, center, (W, H, L),
 * pose, float32 corners).
 *
 * Cluster numbering is scikit-learn's: clusters in the order of their smallest core-point index, a border point takes the smallest
 * label among the clusters of its core neighbours, noise is -1.
 *
 * Declared deviations from the reference:
 *  - instances for which the reference divides by zero or raises are not lifted; they get a status and no box: an empty mask
 *    (OVM_GEO_EMPTY), fewer than 2 points (OVM_GEO_TOO_FEW), a non-finite depth under the mask (OVM_GEO_NONFINITE), a rectangle
 *    that misses the image (OVM_GEO_RECT_OUTSIDE);
 *  - "the box is the mask" (mask == NULL) is ours, the reference always runs SAM: the pixels x0 <= x < x1, y0 <= y < y1 of `rect`
 *    clipped to the image; the tools derive rect from an xyxy box as (ceil(x0), ceil(y0), ceil(x1), ceil(y1));
 *  - pose is the closed form Ry(-yaw) = [[cos yaw, 0, sin yaw], [0, 1, 0], [-sin yaw, 0, cos yaw]]; the reference's Kabsch / SVD
 *    (get_pose) gives the same matrix to 4e-16. */
enum { OVM_GEO_OK = 0, OVM_GEO_EMPTY = 1, OVM_GEO_TOO_FEW = 2, OVM_GEO_NONFINITE = 3, OVM_GEO_RECT_OUTSIDE = 4,
       OVM_GEO_COUNT_MISMATCH = 5, /* a mask plane holds another number of pixels than n_points declares */
       OVM_GEO_BAD_PERM = 6 };     /* a perm entry outside 0 .. n_points-1 */

typedef struct OvmGeoParams {       /* reference defaults: 0.01, 0.1, 0.5, 100, 40000, 4, 100 */
  double eps0;                      /* eps of the first trial, metres; doubled per trial */
  double min_cluster_frac;          /* a cluster with size / n below this is dropped */
  double accept_frac;               /* a trial is accepted when kept > accept_frac * n */
  int32_t min_samples;              /* DBSCAN core threshold, the point itself included */
  int32_t max_points;               /* down-sampling cap */
  int32_t trials;                   /* 1 .. 8 */
  int32_t min_cluster;              /* a cluster with size <= this is dropped */
  int32_t last_stage;               /* 0: everything. Timing aid: stop after 1 points, 2 mean + yaw, 3 rotate + gather, 3 + t trial t */
  int32_t reserved;
} OvmGeoParams;

typedef struct OvmGeoInstance {
  const uint8_t* mask;              /* device [H][W] plane, nonzero = inside; NULL: the rectangle is the mask */
  const int32_t* perm;              /* device [n_points] or NULL; required when n_points > max_points */
  int32_t rect[4];                  /* x0, y0, x1, y1, half-open, read when mask == NULL */
  int32_t n_points;                 /* mask: the number of nonzero pixels (the caller counts them); rectangle: ignored */
  int32_t reserved;
} OvmGeoInstance;

typedef struct OvmGeoResult {
  double offset[3];                 /* mean of the un-projected points */
  double yaw;
  double ext_min[3], ext_max[3];    /* kept points' min / max in the rotated frame */
  double eps;                       /* eps of the accepted trial (of the last one run when none was) */
  int32_t n_points, n_used, n_kept; /* points, points after down-sampling, points the extents cover */
  int32_t trial;                    /* accepted trial 1 .. trials, 0 = fallback to all points */
  int32_t status;                   /* OVM_GEO_*; anything but OVM_GEO_OK: the other fields except n_points are zero */
  int32_t reserved;
} OvmGeoResult;

typedef struct OvmGeoBox {
  double center_cam[3], dimensions[3], pose[9], center_2D[2], depth;
  float bbox3D[8][3];
} OvmGeoBox;

/* The reference's parameters. */
int ovm_geo_default_params(OvmGeoParams* params);
/* Message of the last OVM_ERR_* a GEO call returned on this thread (these calls take no handle). */
const char* ovm_geo_last_error(void);
/* Workspace bytes for ovm_geo_lift on these instances; label_offsets (host, [n_inst + 1], may be NULL) receives where each
 * instance's n_used labels start in the `labels` array. inst is host memory; nothing touches the device. */
int ovm_geo_lift_workspace(const OvmGeoInstance* inst, int32_t n_inst, int32_t H, int32_t W, const OvmGeoParams* params, int64_t* bytes,
                           int64_t* label_offsets);
/* Lifts all instances of one image: one stream-ordered launch sequence, no device-to-host read and no wait for the device
 * other than for the previous call's descriptor upload, whose pinned staging buffer is reused (a per-instance flag on the device ends
 * the later trials of an accepted instance early). depth: device fp32 [H][W]; K: host,
 * row-major 3 x 3; inst: host; results: device [n_inst]; labels: device int32, the last trial's labels per instance at
 * label_offsets (all -1 for an instance that is not lifted), or NULL. OVM_ERR_INVALID for null / inconsistent arguments, OVM_ERR_UNSUPPORTED when an instance has more than
 * max_points points and no perm, OVM_ERR_CAPACITY for too small a workspace - all before any device work. */
int ovm_geo_lift(const float* depth, int32_t H, int32_t W, const double* K, const OvmGeoInstance* inst, int32_t n_inst,
                 const OvmGeoParams* params, OvmGeoResult* results, int32_t* labels, void* workspace, int64_t workspace_bytes,
                 ovm_stream_t stream);
/* The clustering alone: labels of sklearn.cluster.DBSCAN(eps, min_samples).fit(points).labels_ for device fp64 points [n][3]. */
int ovm_geo_dbscan_workspace(int32_t n, int64_t* bytes);
int ovm_geo_dbscan(const double* points, int32_t n, double eps, int32_t min_samples, int32_t* labels, void* workspace,
                   int64_t workspace_bytes, ovm_stream_t stream);
/* Host, fp64, no GPU: steps 7's corners and the box of a lifted instance (status OVM_GEO_OK, else OVM_ERR_INVALID). bbox3D is
 * get_cuboid_verts_faces of the float32-rounded center, dimensions and pose, computed in float32 as the reference does. */
int ovm_host_geo_box(const OvmGeoResult* result, const double* K, OvmGeoBox* box);

/* ---- OVMono3D-GEO: the ground plane, and boxes upright to it (ours; off by default everywhere) ------------------------------------
 * The lift above takes the camera for level: yaw is fitted in the camera's (x, z) plane and the box's vertical axis is the camera's
 * y axis, so under a pitched or rolled camera the boxes lean with it. The reference has the same defect. A declared deviation,
 * used only where a caller asks for it: the floor is fitted to the depth map (RANSAC over plane hypotheses, then a least-squares
 * refinement), and the lift runs in the frame in which the floor's normal is +y.
 *
 * All arithmetic is fp64 (no fused multiply-adds); all points are in the lift's frame, step 1 above:
 * p = (z (x - cx) / fx, -(z (y - cy) / fy), -z), in which "up" is +y. A plane is (n, d), |n| = 1: the points with n . p + d = 0;
 * the camera, at the origin, is d above it. The numpy restatement is tests/ground_oracle.py.
 *
 * Steps:
 *  1. points: the pixels (y, x) with y % stride == 0 and x % stride == 0 in row-major order whose depth is finite, > 0 and, with
 *     max_depth > 0, <= max_depth, compacted in that order and un-projected; n_points = n is their number. n < 3: OVM_GROUND_TOO_FEW.
 *  2. hypothesis h = 0 .. hypotheses-1: the points i_j = mix(seed * 0x9E3779B9 + 3 h + j) % n, j = 0, 1, 2, in 32-bit unsigned
 *     arithmetic, mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *     c = (p1 - p0) x (p2 - p0); invalid when two indices coincide or |c|^2 <= 1e-12 |p1 - p0|^2 |p2 - p0|^2.
 *     n = c / |c|, negated when n_y < 0; d = -n . p0. Invalid too when n_y < cos(max_tilt_deg) (a wall) or d <= 0 (the camera is
 *     not above the plane: a ceiling).
 *  3. count[h] = the number of points with |n . p + d| <= thresh + thresh_rel * |p_z|, n . p = (n_x p_x + n_y p_y) + n_z p_z;
 *     -1 for an invalid hypothesis. Integer sums: the counts do not depend on any order.
 *  4. best_hyp = the largest count, the lowest h on ties; hyp_inliers its count. No valid hypothesis, or
 *     hyp_inliers < min_share * n: OVM_GROUND_NO_PLANE.
 *  5. with refine: centroid and 3 x 3 scatter matrix of the best hypothesis' inliers (two passes, partial sums over 1024 points
 *     added in a fixed tree: the same bits run to run), the eigenvector of its smallest eigenvalue (cyclic Jacobi, 12 sweeps),
 *     negated when n_y < 0, d = -n . centroid; its inliers are counted as in step 3. It replaces the hypothesis when it passes the
 *     tilt and d > 0 tests of step 2 and its count is >= hyp_inliers; n_inliers is the count of the plane kept.
 *  6. frame = U, the shortest-arc rotation with U n = (0, 1, 0), row-major: U = I + [a]x + [a]x^2 / (1 + n_y), a = n x e_y.
 * status != OVM_GROUND_OK: frame is the identity, normal / offset / n_inliers are zero; best_hyp is -1 and the hyp_ fields zero when
 * no hypothesis was valid, else they describe the best one (which min_share then refused).
 *
 * Not measured: the defaults of thresh, thresh_rel and min_share are settings chosen from the noise model of the synthetic scenes
 * of the tests; nobody has tuned them on real Depth Pro maps. */
enum { OVM_GROUND_OK = 0, OVM_GROUND_TOO_FEW = 1, OVM_GROUND_NO_PLANE = 2 };

typedef struct OvmGroundParams {    /* defaults: 0.02, 0.01, 45, 0.10, 0, 512, 4, 0, 1 */
  double thresh;                    /* inlier band, metres ... */
  double thresh_rel;                /* ... plus this per metre of |p_z| (depth noise grows with depth) */
  double max_tilt_deg;              /* largest angle between the plane's normal and the camera's up axis; in (0, 90) */
  double min_share;                 /* the best hypothesis needs this share of the points; in [0, 1] */
  double max_depth;                 /* points beyond it are not taken; 0: no cut */
  int32_t hypotheses;               /* 1 .. 4096 */
  int32_t stride;                   /* >= 1: every stride-th pixel of every stride-th row */
  uint32_t seed;
  int32_t refine;                   /* 0 / 1: step 5 */
  int32_t reserved[2];
} OvmGroundParams;

typedef struct OvmGroundResult {
  double normal[3], offset;         /* the plane kept: n and d */
  double frame[9];                  /* U, row-major */
  double hyp_normal[3], hyp_offset; /* the best hypothesis */
  int32_t n_points, n_valid_hyp, best_hyp, hyp_inliers, n_inliers;
  int32_t status;                   /* OVM_GROUND_* */
} OvmGroundResult;

int ovm_geo_ground_default_params(OvmGroundParams* params);
/* Workspace bytes of ovm_geo_ground_plane for an H x W map; nothing touches the device. */
int ovm_geo_ground_workspace(int32_t H, int32_t W, const OvmGroundParams* params, int64_t* bytes);
/* Steps 1 to 6: one stream-ordered launch sequence, no device-to-host read, no wait for the device. depth: device fp32 [H][W]; K:
 * host, row-major 3 x 3; result: device, one OvmGroundResult; hyp_counts: device int32 [hypotheses] (step 3's counts) or NULL.
 * OVM_ERR_INVALID for null / inconsistent arguments, OVM_ERR_CAPACITY for too small a workspace - before any device work, with
 * nothing written; the message is ovm_geo_last_error's. */
int ovm_geo_ground_plane(const float* depth, int32_t H, int32_t W, const double* K, const OvmGroundParams* params,
                         OvmGroundResult* result, int32_t* hyp_counts, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
/* ovm_geo_lift in a turned frame: step 1 writes U p instead of p, U = frame (device, 9 doubles, row-major; e.g. the frame field of a
 * device OvmGroundResult), steps 2 to 7 run unchanged on those points. frame == NULL is ovm_geo_lift, which is this call. */
int ovm_geo_lift_frame(const float* depth, int32_t H, int32_t W, const double* K, const OvmGeoInstance* inst, int32_t n_inst,
                       const OvmGeoParams* params, const double* frame, OvmGeoResult* results, int32_t* labels, void* workspace,
                       int64_t workspace_bytes, ovm_stream_t stream);
/* Host, fp64: ovm_host_geo_box for a result of ovm_geo_lift_frame. frame: host, 9 doubles (NULL: ovm_host_geo_box). The box is
 * built as for a level camera and turned back into the camera's frame by V = F U^T F, F = diag(1, -1, -1): center_cam = V c',
 * pose = V P', dimensions unchanged, bbox3D the float32 cuboid of the float32-rounded center, dimensions and pose, depth the
 * center's z, center_2D its projection with K. */
int ovm_host_geo_box_frame(const OvmGeoResult* result, const double* K, const double* frame, OvmGeoBox* box);

/* ---- Segment Anything, box-prompted ------------------------------------------------------------------------------------------
 * The mask source of OVMono3D-GEO (reference tools/ovmono3d_geo.py:213-217,270-272,308-309): segment_anything's
 * SamPredictor.set_image(image) once, then predict(box=xyxy) per instance, of which the reference keeps plane [2] of the three
 * multimask outputs. Weights carry segment_anything's own key names (image_encoder.*, prompt_encoder.*, mask_decoder.*).
 *
 * The image encoder's blocks are the OVM_TOWER_SAM code of ovm_create (same packing, same kernels); the neck, the prompt encoder
 * for boxes, the two-way transformer, the upscaling / hypernetwork heads and postprocess_masks are sequenced here. GEMMs follow
 * `precision` (1: fp16 operands, 3: split fp16 x 3); softmax, LayerNorm, sin / cos and the resampling are fp32.
 *
 * Scope: head dimension 64 in the image encoder (vit_b, vit_l). vit_h (1280 wide, 16 heads: head dimension 80) is refused with
 * OVM_ERR_UNSUPPORTED. ovm_sam_predict_boxes is the reference's call (a box, multimask outputs); ovm_sam_predict below takes
 * points, a box, a mask input and the single-mask output as well. */
typedef struct OvmSam OvmSam;
typedef struct OvmSamConfig {
  int32_t embed_dim, depth, heads, patch;   /* image encoder: vit_b 768 / 12 / 12 / 16, vit_l 1024 / 24 / 16 / 16 */
  int32_t pos_grid;                         /* side of the checkpoint's position table (64) */
  int32_t window;                           /* window side of the windowed blocks (14) */
  uint32_t global_mask;                     /* bit i set = block i attends globally */
  int32_t image_size;                       /* ResizeLongestSide target and encoder input side (1024) */
  int32_t prompt_dim;                       /* prompt / decoder width (256) */
  int32_t dec_depth, dec_heads, dec_mlp;    /* two-way transformer: 2, 8, 2048 */
  int32_t attn_downsample;                  /* internal width of the cross attentions = prompt_dim / this (2) */
  int32_t num_mask_tokens;                  /* 4 (multimask outputs + 1) */
  int32_t iou_depth, iou_hidden;            /* IoU head: 3 layers, 256 wide */
  float pixel_mean[3], pixel_std[3];        /* in the network's channel order (segment_anything: 123.675 116.28 103.53 / 58.395 57.12 57.375) */
  int32_t precision;                        /* 1 or 3 */
  int32_t max_boxes;                        /* most boxes one decoder pass takes; a call with more runs in chunks */
} OvmSamConfig;
int ovm_sam_create(const OvmSamConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmSam** out);
int ovm_sam_destroy(OvmSam* sam);
const char* ovm_sam_last_error(const OvmSam* sam);
/* SamPredictor.set_image: image = uint8 device image at its own resolution (height x width; any element strides). ResizeLongestSide
 * (target sides int(side * image_size / max(h, w) + 0.5), Pillow-exact bilinear), flip_bgr != 0: channels reversed first (the
 * predictor's image_format != "RGB" branch), (x - mean) / std, zero padding to the square, encoder, neck. The [G][G][prompt_dim]
 * embedding and the dense positional encoding stay in the handle. */
int ovm_sam_set_image(OvmSam* sam, const OvmImage* image, int32_t flip_bgr, ovm_stream_t stream);
/* Device workspace bytes of ovm_sam_predict_boxes for n boxes (chunks of min(n, max_boxes) boxes); a smaller workspace that still
 * holds one box is accepted and means smaller chunks. */
int ovm_sam_predict_boxes_workspace(const OvmSam* sam, int32_t n, int64_t* bytes);
/* SamPredictor.predict(box=..., multimask_output=True) for n boxes of the image of the last ovm_sam_set_image. boxes_xyxy: device
 * fp32 [n][4] in original pixels. mask_index 0..2: which multimask plane masks_u8 (device uint8 [n][H][W], 1 = logit > 0 after
 * postprocess_masks) receives. iou: device fp32 [n][3] or NULL. lowres: device fp32 [n][3][4G][4G] low-resolution logits or NULL
 * (NULL: only the requested mask token's product is computed). Stream-ordered, no synchronisation. */
int ovm_sam_predict_boxes(OvmSam* sam, const float* boxes_xyxy, int32_t n, int32_t mask_index, uint8_t* masks_u8, float* iou,
                          float* lowres, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
/* tests: copy an intermediate into dst (device fp32); returns the element count or a negative error. names: "preprocessed"
 * [3][S][S] (the encoder's input as its patch rows hold it), "neck" [G][G][C], "dense_pe" [G][G][C]; of the last chunk of the
 * last predict call: "sparse" [n][ns][C], "tokens_out" [n][nt][C] (ovm_sam_predict_boxes: ns = 2, nt = 3 + num_mask_tokens;
 * ovm_sam_predict: ns and nt as described there); "dense" [G][G][C]: the dense prompt embedding of the last prompt of that chunk
 * (its mask embedding, or no_mask_embed in every cell). */
int64_t ovm_sam_debug_copy(OvmSam* sam, const char* name, float* dst, int64_t capacity, ovm_stream_t stream);

/* SamPredictor.predict with every prompt kind, for n prompts of one shape on the image of the last ovm_sam_set_image.
 *   points_xy   device fp32 [n][n_points][2], original pixels (x, y); labels device int32 [n][n_points]: 1 foreground, 0 background,
 *               -1 padding (not_a_point_embed alone, no positional part). 0 <= n_points <= 8, else OVM_ERR_SHAPE. The labels live on
 *               the device and are not read back: a value outside {1, 0, -1} is the caller's to refuse (ovmono3d_amd.sam does), the
 *               kernel gives it the padding token. Both may be NULL when n_points == 0.
 *   boxes_xyxy  device fp32 [n][4] or NULL. Without a box segment_anything appends one padding token, with a box it does not: the
 *               sparse embeddings are [n][ns][C], ns = n_points + (box ? 2 : 1), ordered points, (padding), (corner 0, corner 1),
 *               and the decoder runs nt = 1 + num_mask_tokens + ns <= 15 tokens per prompt. Neither points nor box: OVM_ERR_INVALID.
 *   mask_inputs device fp32 [n][4G][4G] low-resolution logits of an earlier call, or NULL (no_mask_embed). Run through
 *               mask_downscaling (conv 2x2 s2 1 -> 4, LayerNorm2d, GELU, conv 2x2 s2 4 -> 16, LayerNorm2d, GELU, conv 1x1 16 -> C, fp32).
 *   multimask   != 0: K = 3 planes (mask tokens 1..3), masks_u8 receives plane mask_index 0..2; 0: K = 1 (mask token 0, IoU column
 *               0), mask_index must be 0.
 *   masks_u8 device uint8 [n][H][W]; iou device fp32 [n][K] or NULL; lowres device fp32 [n][K][4G][4G] or NULL.
 * Chunks of max_boxes prompts as ovm_sam_predict_boxes; a call with n_points == 0, a box, no mask input and multimask != 0 IS
 * ovm_sam_predict_boxes (same launches, same bytes). Stream-ordered, no synchronisation. */
int ovm_sam_predict_workspace(const OvmSam* sam, int32_t n, int32_t n_points, int32_t has_box, int32_t has_mask, int64_t* bytes);
int ovm_sam_predict(OvmSam* sam, const float* points_xy, const int32_t* labels, int32_t n_points, const float* boxes_xyxy,
                    const float* mask_inputs, int32_t n, int32_t multimask, int32_t mask_index, uint8_t* masks_u8, float* iou, float* lowres,
                    void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
/* The tight box and the pixel count of n masks (device uint8 [n][H][W], nonzero = inside): boxes_xyxy_out device fp32 [n][4] =
 * (xmin, ymin, xmax + 1, ymax + 1), counts_out device int32 [n]; an empty mask gives zeros. Integer reductions (wave, then
 * atomicMin / atomicMax / atomicAdd into the outputs): exact. boxes_xyxy_out 16-byte aligned. Stream-ordered. */
int ovm_sam_mask_boxes(const uint8_t* masks_u8, int32_t n, int32_t H, int32_t W, float* boxes_xyxy_out, int32_t* counts_out, ovm_stream_t stream);

/* ---- Segment Anything, automatic mask generation -----------------------------------------------------------------------------
 * segment_anything's SamAutomaticMaskGenerator for the full-image crop (crop_n_layers = 0), "binary_mask" output, no small-region
 * clean-up: one foreground click per grid point, multimask outputs, 3 candidates per point in point-major order (candidate
 * 3 p + k = plane k of point p). The rules (restated from segment_anything's automatic_mask_generator.py / utils/amg.py; the
 * package is not a dependency, parity with it is not pinned by a test):
 *   filter 1    only when pred_iou_thresh > 0: keep iou > pred_iou_thresh (strict)
 *   stability   over the postprocess_masks logits v at H x W: float32(count(v > +offset)) / float32(count(v > -offset)); 0 / 0 = NaN
 *   filter 2    only when stability_thresh > 0: keep stability >= stability_thresh (NaN fails)
 *   mask        v > 0; box = inclusive (xmin, ymin, xmax, ymax) of the mask, (0, 0, 0, 0) for an empty one; area = its pixel count
 *   NMS         torchvision.ops.nms on the inclusive boxes as floats (area (xmax - xmin) (ymax - ymin)), score = iou, suppression at
 *               IoU > nms_thresh (strict): the rule of ovm_op_nms (decreasing score, ties to the lower index); output in keep order
 * The crop-edge filter of the generator never removes a mask of the full-image crop and is not built.
 *
 * One candidate. flags bit 0 (OVM_SAM_CAND_SKIPPED): the row failed filter 1 inside ovm_sam_auto_candidates and its mask was never
 * counted: stability 0, area 0, box and counts 0. 64 bytes. */
#define OVM_SAM_CAND_SKIPPED 1
typedef struct OvmSamCandidate {
  float iou;                 /* the decoder's IoU prediction of the plane */
  float stability;           /* float32(cnt_hi) / float32(cnt_lo) */
  int32_t area;              /* count(v > 0) */
  int32_t box[4];            /* inclusive xmin, ymin, xmax, ymax of v > 0; zeros for an empty mask */
  int32_t cnt_hi, cnt_lo;    /* count(v > +offset), count(v > -offset) */
  int32_t flags;
  int32_t reserved[6];
} OvmSamCandidate;
/* The candidates of n foreground clicks on the image of the last ovm_sam_set_image. points_xy: device fp32 [n][2], original pixels
 * (x, y). out: device OvmSamCandidate [3 n]. Per chunk of at most max_boxes points: ovm_sam_predict's own launches for one point of
 * label 1, multimask, low-resolution logits into the workspace and no mask written; then the mask statistics of the chunk's planes
 * (ovm_op_sam_mask_stats: nothing of image size is written); then the rows. With pred_iou_thresh > 0 the planes with
 * !(iou > pred_iou_thresh) are not counted (decided on the device; OVM_SAM_CAND_SKIPPED); with pred_iou_thresh <= 0 every plane is.
 * The workspace (256-byte aligned) may be smaller than ovm_sam_auto_candidates_workspace says as long as it holds one point: smaller
 * chunks. Stream-ordered, no synchronisation, no allocation. */
int ovm_sam_auto_candidates_workspace(const OvmSam* sam, int32_t n, int64_t* bytes);
int ovm_sam_auto_candidates(OvmSam* sam, const float* points_xy, int32_t n, float pred_iou_thresh, float offset, OvmSamCandidate* out,
                            void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
/* Filters 1 and 2 and the NMS over m candidates (device). A row is valid when it was not skipped, its iou is a number, and it
 * passes the filters that are switched on; pred_iou_thresh here must not be lower than the one the table was computed with (a
 * skipped row stays out). keep_idx: device int32 [m], the kept candidate indices in NMS keep order; n_keep: one device word.
 * m > 4096: OVM_ERR_CAPACITY before any device work (points_per_side <= 36). workspace: ovm_sam_auto_select_workspace bytes,
 * 16-byte aligned. Stream-ordered; the NMS is ovm_op_nms's and, as there, allocates its scratch and waits for the stream. */
int ovm_sam_auto_select_workspace(int32_t m, int64_t* bytes);
int ovm_sam_auto_select(const OvmSamCandidate* cands, int32_t m, float pred_iou_thresh, float stability_thresh, float nms_thresh,
                        int32_t* keep_idx, int32_t* n_keep, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);

/* ---- Depth Pro, metric depth ------------------------------------------------------------------------------------------------
 * The depth source of OVMono3D-GEO (reference tools/ovmono3d_geo.py:267,290-295: depth_pro's model.infer(image, f_px)). The
 * arithmetic is Hugging Face transformers' DepthProForDepthEstimation + DepthProImageProcessor (preprocess and
 * post_process_depth_estimation), and the weights carry the key names of the apple/DepthPro-hf checkpoint.
 *
 * The three encoders (patch, image, field of view) are DINOv2 towers of ovm_create's block code with HF key names; the 35 crops of
 * the three-level pyramid run as one batch. Pyramid, token merge, neck, DPT fusion, the depth head, the field-of-view head and the
 * conversion to metres are sequenced here. GEMMs and convolutions follow `precision` (1: fp16 operands, 3: split fp16 x 3);
 * LayerNorm, softmax and every resampling are fp32.
 *
 * Scope: one image per call; ratios 0.25 / 0.5 / 1 with overlaps 0 / 0.5 / 0.25 on a canvas of 4 * crop (anything else:
 * OVM_ERR_UNSUPPORTED); the three encoders share one architecture; no batch norm in the fusion units. */
typedef struct OvmDepthPro OvmDepthPro;
typedef struct OvmDepthProConfig {
  int32_t embed_dim, depth, heads;          /* the towers: ViT-L 1024 / 24 / 16 (head dimension 64) */
  int32_t patch, crop;                      /* ViT patch (16) and crop side = the towers' image size (384); canvas = 4 * crop */
  int32_t hook_ids[2];                      /* blocks of the patch tower whose output feeds the two finest decoder levels (11, 5) */
  int32_t fusion_dim;                       /* decoder width (256) */
  int32_t scaled_dims[3];                   /* scaled_images_feature_dims (1024, 1024, 512) */
  int32_t inter_dims[2];                    /* intermediate_feature_dims (256, 256) */
  float ratios[3], overlaps[3];             /* scaled_images_ratios (0.25, 0.5, 1) and _overlap_ratios (0, 0.5, 0.25) */
  int32_t merge_padding;                    /* 3 */
  int32_t num_fov_layers;                   /* stride-2 convolutions of the field-of-view head (2) */
  int32_t use_fov;                          /* 0: no field-of-view model is loaded and every call must give f_px */
  int32_t precision;                        /* 1 or 3 */
  float ln_eps;                             /* LayerNorm eps of the towers (1e-6) */
} OvmDepthProConfig;
int ovm_depthpro_create(const OvmDepthProConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmDepthPro** out);
int ovm_depthpro_destroy(OvmDepthPro* dp);
const char* ovm_depthpro_last_error(const OvmDepthPro* dp);
/* Device workspace bytes of ovm_depthpro_infer for an H x W image (256-byte aligned by the caller). */
int ovm_depthpro_workspace(const OvmDepthPro* dp, int32_t H, int32_t W, int64_t* bytes);
/* image: uint8 device image [H][W][3] with any element strides; flip_bgr != 0 reverses the channels first. f_px > 0: the focal
 * length in pixels of the original image; f_px <= 0: estimated by the field-of-view head, f = 0.5 W / tan(0.5 fov). depth_out:
 * device fp32 [H][W] in metres, 1 / clamp(canonical * W / f resized to H x W, 1e-4, 1e4). fov_deg_out, f_px_out: device fp32
 * scalars (fov_deg_out receives the head's estimate, or 0 without a field-of-view model); either may be NULL. Stream-ordered: the
 * focal length is read from device memory, nothing is synchronised. The intermediates stay in the workspace for
 * ovm_depthpro_debug_copy until the next call. */
int ovm_depthpro_infer(OvmDepthPro* dp, const OvmImage* image, int32_t flip_bgr, float f_px, float* depth_out, float* fov_deg_out,
                       float* f_px_out, void* workspace, int64_t workspace_bytes, ovm_stream_t stream);
/* tests: copy a stage of the last infer into dst (device fp32); returns the element count or a negative error. NHWC throughout:
 * "pyramid0/1/2" [s][s][3] (s = canvas, / 2, / 4), "tokens_patch" [35][T][D], "features0..5" (image, low, medium, high, hook 0,
 * hook 1: [side][side][D]), "neck0..4" [side][side][fusion_dim], "fused", "canonical" [S][S], "fov" [1]. */
int64_t ovm_depthpro_debug_copy(OvmDepthPro* dp, const char* name, float* dst, int64_t capacity, ovm_stream_t stream);
/* Per-stage timing: after ovm_depthpro_profile_enable(dp, 1) every infer records HIP events at its stage boundaries on its stream;
 * ovm_depthpro_stage_ms waits for the last infer and writes 7 durations in milliseconds (n >= 7): pyramid (with the border clear),
 * towers, merge + neck, fusion, head, field of view, output. */
int ovm_depthpro_profile_enable(OvmDepthPro* dp, int32_t on);
int ovm_depthpro_stage_ms(OvmDepthPro* dp, float* ms, int32_t n);
/* Host only (no device call): OVM_OK when the geometry of cfg is supported, else the error ovm_depthpro_create would give, with its
 * message in msg (capacity bytes). */
int ovm_host_depthpro_check(const OvmDepthProConfig* cfg, char* msg, int32_t capacity);

/* ---- the kernels of the SAM and Depth Pro engines one at a time (tests) ---------------------------------------------------------
 * Each call is the launcher the engine itself uses (csrc/sam.hip, csrc/depthpro.hip), nothing else. Device pointers unless marked
 * host; fp32 row-major; fp16 buffers are passed as uint16_t. None synchronises. An argument outside a kernel's contract is refused
 * before anything is launched: OVM_ERR_INVALID for a null pointer or a non-positive count, OVM_ERR_SHAPE for the limits named below.
 *
 * get_dense_pe: pe [G*G][2 F] = [sin | cos](2 pi (2 c - 1) . gauss), c = ((j + 0.5) / G, (i + 0.5) / G) for row i * G + j; gauss [2][F]. */
int ovm_op_sam_dense_pe(const float* gauss, int32_t G, int32_t F, float* pe, ovm_stream_t stream);
/* Tokens of nb boxes: tok [nb][nout + 2][C] = out_tokens [nout][C], then the two box corners: boxes [nb][4] xyxy in the pixels of the
 * H x W image, scaled by neww / W and newh / H (fp64), + 0.5, / S, encoded with gauss [2][C/2], + corner [2][C]. sparse [nb][2][C]
 * receives the two corner rows as well. C % 2 != 0: OVM_ERR_SHAPE. */
int ovm_op_sam_box_tokens(const float* boxes, int32_t nb, int32_t nout, int32_t C, const float* out_tokens, const float* gauss, const float* corner,
                          int32_t H, int32_t W, int32_t newh, int32_t neww, int32_t S, float* tok, float* sparse, ovm_stream_t stream);
/* x [M][D] <- gelu_erf(LayerNorm(x)), in place. D > 256: OVM_ERR_SHAPE. */
int ovm_op_sam_ln_gelu(float* x, int64_t M, int32_t D, const float* gamma, const float* beta, float eps, ovm_stream_t stream);
/* Image -> token attention, head dimension 16: q [nb * G2][ldq] and o [nb * G2][ldo] hold heads x 16 columns, k / v [nb * nt][ld];
 * o = softmax_t(scale q . k_t) v over the nt tokens of the row's own box. OVM_ERR_SHAPE unless 1 <= nt <= 8, heads <= 16,
 * 256 % heads == 0, G2 % (256 / heads) == 0, ldq, ld, ldo >= 16 heads and ldq % 4 == ldo % 4 == 0; q and o 16-byte aligned. */
int ovm_op_sam_i2t_attn(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, int32_t nt, int32_t heads, int32_t G2, int32_t nb,
                        float scale, float* o, int32_t ldo, ovm_stream_t stream);
/* The same kernel instantiated for up to 16 tokens (32 KB of LDS): 1 <= nt <= 16, every other limit as above; for nt <= 8 the bytes
 * of ovm_op_sam_i2t_attn. */
int ovm_op_sam_i2t_attn16(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, int32_t nt, int32_t heads, int32_t G2, int32_t nb,
                          float scale, float* o, int32_t ldo, ovm_stream_t stream);
/* Tokens of nb prompts with P points each (and a box each when boxes != NULL): tok [nb][nout + ns][C] = out_tokens [nout][C], then
 * the ns = P + (boxes ? 2 : 1) sparse rows, which sparse [nb][ns][C] receives as well: point p = PE of points [nb][P][2] (x, y;
 * scaled, + 0.5, / S and encoded as the corners of ovm_op_sam_box_tokens) + point_emb [2][C] row 1 for label 1, row 0 for label 0;
 * any other label: not_a_point [C] alone. Without boxes one more not_a_point row follows; with boxes [nb][4] the two corner rows of
 * ovm_op_sam_box_tokens. labels int32 [nb][P]; points and labels may be NULL when P == 0. P > 8 or C % 2 != 0: OVM_ERR_SHAPE. */
int ovm_op_sam_point_tokens(const float* points, const int32_t* labels, const float* boxes, int32_t nb, int32_t P, int32_t nout, int32_t C,
                            const float* out_tokens, const float* gauss, const float* point_emb, const float* not_a_point, const float* corner,
                            int32_t H, int32_t W, int32_t newh, int32_t neww, int32_t S, float* tok, float* sparse, ovm_stream_t stream);
/* mask_downscaling of the prompt encoder, fused, fp32: mask [n][4G][4G] -> out [n][G*G][C], row i * G + j = conv1x1(GELU(LN2d(conv
 * 2x2 s2(GELU(LN2d(conv 2x2 s2(mask patch 4i.., 4j..))))))). w0 [4][1][2][2], b0 [4], g1 / be1 [4] (LayerNorm2d, eps 1e-6, biased
 * variance over the channels), w3 [16][4][2][2], b3 [16], g4 / be4 [16], w6 [C][16], b6 [C]. C outside 1 .. 256: OVM_ERR_SHAPE. */
int ovm_op_sam_mask_embed(const float* mask, int32_t n, int32_t G, int32_t C, const float* w0, const float* b0, const float* g1, const float* be1,
                          const float* w3, const float* b3, const float* g4, const float* be4, const float* w6, const float* b6, float* out,
                          ovm_stream_t stream);
/* Hypernetwork product over the blocked upscaled map up [nb * G*G * 4][4 * C8]: pixel (4 i + 2 a + a2, 4 j + 2 b + b2) of box n is
 * row (n * G*G + i * G + j) * 4 + a * 2 + b, columns (a2 * 2 + b2) * C8 .. + C8. out[n * out_box_stride + t * L*L + Y * L + X] =
 * hyper[n * ld_hyper + (t0 + t) * C8 ..] . up[n][Y][X][:], t < ntk, L = 4 G. OVM_ERR_SHAPE unless C8 % 4 == 0, ld_hyper % 4 == 0,
 * ld_hyper >= (t0 + ntk) * C8 and out_box_stride >= ntk * L*L. */
int ovm_op_sam_mask_prod(const float* up, const float* hyper, int32_t ld_hyper, int32_t t0, int32_t ntk, int32_t C8, int32_t G, int32_t nb, float* out,
                         int64_t out_box_stride, ovm_stream_t stream);
/* postprocess_masks + threshold: out uint8 [nb][H][W] (any byte alignment) = bilinear(bilinear(logits L x L -> S x S)[:newh, :neww]
 * -> H x W) > 0, plane n at logits + n * box_stride. newh or neww outside 1 .. S: OVM_ERR_SHAPE. */
int ovm_op_sam_mask_out(const float* logits, int64_t box_stride, int32_t L, int32_t S, int32_t newh, int32_t neww, int32_t H, int32_t W, int32_t nb,
                        uint8_t* out, ovm_stream_t stream);
/* The statistics of the same value v = bilinear(bilinear(logits L x L -> S x S)[:newh, :neww] -> H x W) without writing it: per plane
 * n (logits + n * plane_stride) seven int32 words out[n][7] = count(v > +offset), count(v > 0), count(v > -offset), then the inclusive
 * xmin, ymin, xmax, ymax of v > 0 (zeros for an empty plane). v is the value ovm_op_sam_mask_out thresholds, by the same device
 * functions: the middle count is that mask's byte sum and the box its tight box, to the bit. skip: device int32 [planes] or NULL; a
 * plane whose word is nonzero is not evaluated and its seven words stay as the caller left them. Integer reductions (thread, wave,
 * one atomic per wave and value): independent of execution order. OVM_ERR_SHAPE, before any device work, for L < 1, S < L, newh or
 * neww outside 1 .. S, neww > 4096 (two rows of the S-plane must fit the kernel's 32 KiB of LDS), H, W < 1, H * W >= 2^31,
 * plane_stride < L * L or planes > 65535. */
int ovm_op_sam_mask_stats(const float* logits, int64_t plane_stride, int32_t planes, int32_t L, int32_t S, int32_t newh, int32_t neww, int32_t H,
                          int32_t W, float offset, const int32_t* skip, int32_t* out, ovm_stream_t stream);
/* Patch rows hi (+ lo, may be NULL) [G*G][ld], column (py * P + px) * 3 + c -> out fp32 [3][G P][G P]. ld < 3 P^2: OVM_ERR_SHAPE. */
int ovm_op_sam_unpatch(const uint16_t* hi, const uint16_t* lo, int32_t ld, int32_t G, int32_t P, float* out, ovm_stream_t stream);
/* iou [n][3] = head [n][ldh] columns 1 .. 3. ldh < 4: OVM_ERR_SHAPE. */
int ovm_op_sam_iou_slice(const float* head, int32_t ldh, int32_t n, float* iou, ovm_stream_t stream);
/* out[i] = a[i] + b[i % bmod], i < n; b == NULL: out[i] = a[i % bmod]. n % 4 != 0 or bmod % 4 != 0: OVM_ERR_SHAPE. 16-byte aligned. */
int ovm_op_sam_add_bcast(const float* a, const float* b, float* out, int64_t n, int64_t bmod, ovm_stream_t stream);

/* uint8 image (H x W, 3 channels, element strides; flip: channel 2 - c) -> (x / 255 - 0.5) / 0.5 -> bilinear S x S = P0 [S][S][3], and
 * F.interpolate(scale_factor 0.5 / 0.25) of it: P1 [S/2][S/2][3], P2 [S/4][S/4][3]. S % 4 != 0: OVM_ERR_SHAPE. */
int ovm_op_dp_pyramid(const uint8_t* img, int32_t H, int32_t W, int64_t stride_h, int64_t stride_w, int64_t stride_c, int32_t flip, int32_t S, float* P0,
                      float* P1, float* P2, ovm_stream_t stream);
/* merge_patches: tok [crops][T][D], the n x n crops from crop0 on, each T = 1 + g*g tokens (token 0 skipped); the first crop of an
 * axis keeps cells [0, g - pad), inner ones [pad, g - pad), the last [pad, g): a map of side Ms = n g - 2 (n - 1) pad, bilinearly
 * resized to out x out when out != Ms, as split rows hi / lo (lo may be NULL) [out*out][D]. OVM_ERR_SHAPE unless D % 4 == 0,
 * T >= 1 + g*g, 2 pad < g, pad == 0 for n == 1 and Ms as above. */
int ovm_op_dp_merge(const float* tok, int32_t T, int32_t D, int32_t crop0, int32_t n, int32_t g, int32_t pad, int32_t Ms, int32_t out, uint16_t* hi,
                    uint16_t* lo, ovm_stream_t stream);
/* Split pixels hi + lo (lo may be NULL), pixel stride ld, [side*side] or (pad_in) the interior of [side + 2][side + 2] -> out fp32
 * [side*side][C] and / or split(relu(value)) into the interior of p_hi / p_lo [side + 2][side + 2][C] (any may be NULL, not both out
 * and p_hi). OVM_ERR_SHAPE unless C % 4 == 0, ld % 4 == 0 and ld >= C. */
int ovm_op_dp_unsplit(const uint16_t* hi, const uint16_t* lo, int32_t side, int32_t C, int32_t ld, int32_t pad_in, float* out, uint16_t* p_hi,
                      uint16_t* p_lo, ovm_stream_t stream);
/* out [So][So][Cout] = relu(conv3x3 stride 2 pad 1 of in [Si][Si][Cin] + bias) + add[(oy * So + ox) * ld_add + co] (add may be NULL),
 * So = (Si - 1) / 2 + 1, w [Cout][3][3][Cin]. Cin % 4 != 0, or ld_add < Cout: OVM_ERR_SHAPE. */
int ovm_op_dp_conv_s2(const float* in, int32_t Si, int32_t Cin, const float* w, const float* bias, int32_t Cout, const float* add, int32_t ld_add,
                      float* out, ovm_stream_t stream);
/* out[0] = bias[0] + sum_i in[i] w[i], i < n */
int ovm_op_dp_dot(const float* in, const float* w, const float* bias, int32_t n, float* out, ovm_stream_t stream);
/* The depth head's tail on the matrix cores: out [S][S] = relu(b2 + w2 . relu(b1 + conv3x3(in))) with in = hi (+ lo at precision 3)
 * zero-bordered [S + 2][S + 2][C] and w_hi (+ w_lo) fp16 [32][9 C], k = (ky * 3 + kx) * C + c. S % 16 != 0 or C % 32 != 0: OVM_ERR_SHAPE. */
int ovm_op_dp_head_tail(const uint16_t* hi, const uint16_t* lo, int32_t S, int32_t C, const uint16_t* w_hi, const uint16_t* w_lo, const float* b1,
                        const float* w2, const float* b2, int32_t precision, float* out, ovm_stream_t stream);
/* Zeroes the one-pixel frame of n <= 24 images hi[i] (+ lo[i]; lo or lo[i] may be NULL) [side[i] + 2][side[i] + 2][C[i]]; hi, lo, side, C: host
 * arrays. C[i] % 8 != 0 or n > 24: OVM_ERR_SHAPE. */
int ovm_op_dp_clear_borders(uint16_t* const* hi, uint16_t* const* lo, const int32_t* side, const int32_t* C, int32_t n, ovm_stream_t stream);
/* post_process_depth_estimation: f = f_px when > 0, else 0.5 W / tan(0.5 deg2rad(fov_deg[0])); depth [H][W] = 1 / clamp(bilinear S x S
 * -> H x W of canon * W / f, 1e-4, 1e4). fov_out / f_out (may be NULL) receive fov_deg[0] (0 when fov_deg is NULL) and f. f_px <= 0
 * with fov_deg NULL: OVM_ERR_INVALID. */
int ovm_op_dp_depth_out(const float* canon, int32_t S, int32_t H, int32_t W, float f_px, const float* fov_deg, float* depth, float* fov_out, float* f_out,
                        ovm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OVM3D_H */
