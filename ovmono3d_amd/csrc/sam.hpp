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
// fp32 [T][D] tokens of the last block (device; valid until the next forward)
const float* tower_tokens(const OvmHandle* h);
// the patch rows the encoder read: fp16 [G * G][ld], column (py * P + px) * 3 + c; lo = null in one-pass mode (value = hi + lo)
void tower_patches(const OvmHandle* h, const half_t** hi, const half_t** lo, int* ld);

}  // namespace ovm
