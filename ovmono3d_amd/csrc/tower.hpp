// The ViT tower: patch embed, class / register tokens, position table and the blocks, with the weights, workspace and geometry they need
// and nothing else. Owners: the detection backbone (OvmHandle, api.hip), the SAM predictor's image encoder (sam.hip), Depth Pro's three
// encoders (depthpro.hip). Defined in tower.hip, with the GEMM dispatcher the tower shares with the pyramid and heads of api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/ovm3d.h"
#include "kernels.hpp"
#include "loader.hpp"

namespace ovm {

// checkpoint families, one row of kFamilies each (tower.hip): hub DINOv2 (*_reg and the SwiGLU ViT-g are read off the checkpoint), Hugging
// Face Dinov2Model (Depth Pro's encoders), open_clip, Hugging Face ViTMAE, timm as MiDaS loads it, segment_anything's ImageEncoderViT
enum TowerFamily { FAM_DINOV2_HUB, FAM_DINOV2_HF, FAM_OPEN_CLIP, FAM_HF_VITMAE, FAM_TIMM, FAM_SAM, FAM_COUNT };
enum QkvKind { QKV_FUSED /* one nn.Linear */, QKV_BARE /* nn.MultiheadAttention in_proj_weight / in_proj_bias */, QKV_TRIPLE /* query, key, value */ };
// position table: dinov2's bicubic with the +0.1 offset (register models: POS_AA, as the hub builds them) | antialiased bicubic | plain
// bicubic on a [grid][grid][D] table | no key, sin-cos table built on the host | as stored (the checkpoint's grid must be the canvas grid)
enum PosRule { POS_HUB, POS_AA, POS_GRID, POS_SINCOS, POS_STORED };
struct FamilyRow {
  int patch, Kpe;                       // patch side and the K of the patch rows (3 P^2 padded to the k-step)
  float ln_eps; int mlp_act; bool cls_token;   // LayerNorm eps of the blocks; fc1 activation: 0 erf-GELU, 3 QuickGELU
  const char *prefix, *block;           // default key prefix; block l lives under prefix + block + "l."
  const char *norm1, *norm2, *ls1, *ls2;          // under the block; ls1 / ls2: full parameter names, null = no LayerScale
  QkvKind qkv_kind; const char* qkv;    // FUSED: the linear; BARE: "<qkv>weight" / "<qkv>bias"; TRIPLE: "<qkv>query" / "key" / "value"
  const char *proj, *fc1, *fc2;
  const char *pe_w, *pe_b, *cls;        // patch-embed weight, bias (null: none), class token
  const char* pos; PosRule pos_rule;
  const char *ln_pre, *ln_final;        // null: the family has none
  bool rel_pos, variants;               // segment_anything's window map and relative-position tables; hub DINOv2's checkpoint probe
};
extern const FamilyRow kFamilies[FAM_COUNT];
constexpr int kMaxTowerViews = 36, kMaxTowerTaps = 4;
struct TowerView { const float* data; int64_t sC, sH, sW; };   // one canvas x canvas crop of a normalised fp32 image: pointer to its first pixel, element strides
struct TowerViews { int n; TowerView v[kMaxTowerViews]; };
// what an owner fills from its own config (OvmConfig, OvmSamConfig, OvmDepthProConfig)
struct TowerConfig {
  int family /* TowerFamily */, embed_dim, depth, heads, pos_grid, canvas, precision, max_batch;
  float pixel_mean[3], pixel_std[3];    // the uint8 patch gather's normalisation (tower_forward; the fp32 views are taken as they are)
  int sam_window; uint32_t sam_global_mask;
  float ln_eps;                         // > 0: replaces the family's
  const char* prefix;                   // key prefix of the tower's tensors; null: the family's
};

// ---- the GEMM dispatcher's context: what gemm() and ProfScope read of their caller
struct Prof {                           // optional per-kernel-category timing with HIP events on the caller's stream
  bool on = false; unsigned mask = ~0u; // mask: categories that are bracketed while on
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[OVM_PROF_NCAT];
  size_t used[OVM_PROF_NCAT] = {0};
};
struct GemmCtx {
  int precision = 3; float* splitk_ws = nullptr; size_t splitk_cap = 0;   // split-K partials of this owner's thin GEMMs (not the launcher's process-global one)
  Prof* prof = nullptr;                 // null: nothing is bracketed
};
struct ProfScope {
  hipStream_t s; hipEvent_t stop = nullptr;
  ProfScope(const GemmCtx& c, int cat, hipStream_t s_);
  ~ProfScope() { if (stop) (void)hipEventRecord(stop, s); }
};
// 256 x 256 tiles for the large block contractions, 128 x 128 otherwise; cat: OVM_PROF_* category to bracket, -1 none
int gemm(const GemmCtx& c, const GemmParams& p_in, int epi, int amode, hipStream_t s, int cat = -1);
GemmParams gp_base(const SplitImg& A, int lda, const PackedLin& W, int M);
// fp16 split activation image of a loader's precision: two planes, or (il) one interleaved image [rows][K/32][hi 32 | lo 32], lo = hi + 32
int salloc(Loader* L, SplitImg* s, size_t count, bool zero = false, bool il = false);

constexpr const char* kErrTowerGeometry = "invalid config (canvas % patch, embed_dim = heads*64 and %128 (%256 for 4-level towers), precision in {1,3}, fpn_channels %64)";
constexpr const char* kErrOffsets = "max_batch / max_rois too large: an activation image would exceed the GEMM kernels' 32-bit element offsets";

struct TowerLayer {
  float *ln1g, *ln1b, *ln2g, *ln2b, *ls1, *ls2;
  PackedLin qkv, proj, fc1, fc2;
  // SAM: window side of the block (0 = global) and its relative-position tables [2 s - 1][64] (s = window side or canvas grid), resized at load
  int ws = 0; float *relh = nullptr, *relw = nullptr;
};
struct Tower : Loader {                 // err: the first error of the current call, for the owner to report (with its own prefix)
  TowerConfig cfg;
  const FamilyRow* fam = nullptr;
  int device = 0;
  int G = 0, G2 = 0, T = 0, Tpad = 0, D = 0, Kpe = 0, patch = 0;
  // hub DINOv2 variants, read off the checkpoint: register tokens between the class token and the patches (T = 1 + nreg + G^2), and the
  // fused SwiGLU FFN (ffn_hs = hidden width Hs, 0 = GELU MLP; ffn_k = Hs padded to the k-step, the K of w3 / width of its input image)
  int nreg = 0, ffn_hs = 0, ffn_k = 0;
  float ln_eps = 1e-6f; int mlp_act = 0; bool corun = false;    // corun: ovm_set_corun
  PackedLin pe; float *cls = nullptr, *pos = nullptr, *reg = nullptr;
  float *lnpre_g = nullptr, *lnpre_b = nullptr, *fin_g = nullptr, *fin_b = nullptr;
  std::vector<TowerLayer> layers;
  float* X = nullptr;                   // the residual stream [B * T][D] fp32: after a forward, the last block's tokens
  SplitImg PA, HN, AO, F1, Q, Kx, Vt;
  GemmCtx ctx;                          // precision, split-K workspace, the owner's profiling state
  float* attn_tail_ws = nullptr; int* attn_tail_cnt = nullptr;     // attention's leftover-query partials / arrival counters (attn_tail.hpp)
  // SAM (windowed blocks run on window-partitioned rows like the Swin backbone of the detector)
  int sam_ws = 0, sam_nw = 0, sam_rows = 0;                     // window side, windows per image, rows per image of the partitioned layout
  int* sam_map = nullptr;                                       // [max_batch][sam_rows]: token row of X, -1 = padding
  SplitImg XW, CTX; float *QKVF = nullptr, *RELH = nullptr, *RELW = nullptr; int ldrel = 0;
  ImageDesc *d_imgs = nullptr, *h_imgs = nullptr;               // device / pinned staging of the uint8 inputs

  int configure(const TowerConfig& c);                               // host only: the family's row, validation of cfg, geometry
  int load(const OvmTensor* weights, int n_weights, int device_);    // the checkpoint's variants and their refusals (host only), then the
  void destroy();                                                    // device: offset check, weights, workspace
  int stage_images(const OvmImage* images, int B, hipStream_t s);    // h_imgs[b] <- images[b] and its upload on s
  // every launch of patch embed (+ preprocess of the staged uint8 images) and the blocks on B images
  int launches(int B, hipStream_t s, const struct TowerRun* run = nullptr);
};

// one uint8 image: preprocess ((x - mean) / std, zero padding to the canvas), patch embed, blocks; stream-ordered
int tower_forward(Tower* t, const OvmImage* image, hipStream_t s);
// the blocks on views.n crops as one batch (no pixel is copied: the patch gather reads the views; patch-16 families without windows).
// tap_out[i]: fp32 [n * T][D] copy of the residual stream after block tap_blocks[i]; final_out: the final LayerNorm of the last block's
// tokens, fp32 [n * T][D], or null. Stream-ordered, no synchronisation.
int tower_forward_f32(Tower* t, const TowerViews& views, int n_taps, const int* tap_blocks, float* const* tap_out, float* final_out, hipStream_t s);
// fp32 [T][D] tokens of the last block (device; valid until the next forward)
inline const float* tower_tokens(const Tower* t) { return t->X; }
// the patch rows the encoder read: fp16 [G * G][ld], column (py * P + px) * 3 + c; lo = null in one-pass mode (value = hi + lo)
inline void tower_patches(const Tower* t, const half_t** hi, const half_t** lo, int* ld) { *hi = t->PA.hi; *lo = t->PA.lo; *ld = t->Kpe; }

}  // namespace ovm
