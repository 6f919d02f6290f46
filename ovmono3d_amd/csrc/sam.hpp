// The ViT blocks of ovm_create as a stand-alone image encoder: what the SAM predictor (sam.hip) runs in front of its neck.
// Defined in api.hip beside ovm_create / ovm_backbone_forward, whose weight packing and block loop they share.
#pragma once
#include "../../include/ovm3d.h"
#include "common.hpp"

namespace ovm {

// ovm_create restricted to patch embed + blocks: no pyramid, no heads, keys under vit_prefix (e.g. "image_encoder.")
int tower_create(const OvmConfig* cfg, const OvmTensor* weights, int n_weights, int device, const char* vit_prefix, OvmHandle** out);
// preprocess ((x - mean) / std, zero padding to the canvas), patch embed, blocks; stream-ordered
int tower_forward(OvmHandle* h, const OvmImage* image, hipStream_t s);

// ---- additions for Depth Pro's encoders (depthpro.hip); an encoder created with tower_create is untouched by them ----
constexpr int kMaxTowerViews = 36, kMaxTowerTaps = 4;
struct TowerOpts {
  int hf_dinov2;       // Hugging Face Dinov2Model key names under vit_prefix (embeddings.*, encoder.layer.N.*, layernorm.*), patch 16, position
                       // table at the canvas grid; q / k / v are packed into the fused QKV
  float ln_eps;        // LayerNorm eps of the blocks and of the final norm (> 0)
};
struct TowerView { const float* data; int64_t sC, sH, sW; };   // one canvas x canvas crop of a normalised fp32 image: pointer to its first pixel, element strides
struct TowerViews { int n; TowerView v[kMaxTowerViews]; };
int tower_create_ex(const OvmConfig* cfg, const OvmTensor* weights, int n_weights, int device, const char* vit_prefix, const TowerOpts* opts,
                    OvmHandle** out);
// the blocks on views.n crops as one batch (no pixel is copied: the patch gather reads the views). tap_out[i]: fp32 [n * T][D] copy of
// the residual stream after block tap_blocks[i]; final_out: the final LayerNorm of the last block's tokens, fp32 [n * T][D], or null.
// Stream-ordered, no synchronisation.
int tower_forward_f32(OvmHandle* h, const TowerViews& views, int n_taps, const int* tap_blocks, float* const* tap_out, float* final_out,
                      hipStream_t s);
// fp32 [T][D] tokens of the last block (device; valid until the next forward)
const float* tower_tokens(const OvmHandle* h);
// the patch rows the encoder read: fp16 [G * G][ld], column (py * P + px) * 3 + c; lo = null in one-pass mode (value = hi + lo)
void tower_patches(const OvmHandle* h, const half_t** hi, const half_t** lo, int* ld);

}  // namespace ovm
