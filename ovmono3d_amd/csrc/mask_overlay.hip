// The label map of a stack of mask planes and the mask picture drawn from it (ovm_mask_labels, ovm_render_mask_overlay; the rules
// are in include/ovm3d.h, "Mask label map and mask picture"). One lane per pixel, lanes along x: plane rows, label rows and picture
// rows are read and written coalesced. Integer arithmetic only.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/ovm3d.h"

namespace {

constexpr int kMaxRows = 4 * 65535;      // 4 rows per workgroup, 65535 workgroups along y

__global__ __launch_bounds__(256) void mask_labels_kernel(const uint8_t* __restrict__ masks, int64_t plane_stride, int64_t pitch, int n, int H, int W,
                                                          int32_t* __restrict__ labels, int64_t label_pitch) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const uint8_t* p = masks + (int64_t)y * pitch + x;
  int label = -1;
  for (int i = 0; i < n; ++i) {
    if (p[(int64_t)i * plane_stride] != 0) { label = i; break; }
  }
  labels[(int64_t)y * label_pitch + x] = label;
}

__global__ __launch_bounds__(256) void mask_overlay_kernel(const uint8_t* __restrict__ image, int64_t image_pitch, const int32_t* __restrict__ labels,
                                                           int64_t label_pitch, const uint8_t* __restrict__ colors, int n, int alpha, uint8_t* out,
                                                           int64_t out_pitch, int H, int W) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int32_t* L = labels + (int64_t)y * label_pitch + x;
  const uint8_t* src = image + (int64_t)y * image_pitch + 3 * (int64_t)x;
  uint8_t* dst = out + (int64_t)y * out_pitch + 3 * (int64_t)x;
  const int b = *L;
  int v[3] = {src[0], src[1], src[2]};
  if (b >= 0 && b < n) {
    const bool contour = (x > 0 && L[-1] != b) || (x + 1 < W && L[1] != b) || (y > 0 && L[-label_pitch] != b) || (y + 1 < H && L[label_pitch] != b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int col = colors[3 * b + c];
      v[c] = contour ? col : (v[c] * (255 - alpha) + col * alpha + 127) / 255;
    }
  }
  dst[0] = (uint8_t)v[0]; dst[1] = (uint8_t)v[1]; dst[2] = (uint8_t)v[2];
}

}  // namespace

extern "C" {

int ovm_mask_labels(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W,
                    int32_t* labels_out, int64_t label_pitch, ovm_stream_t stream) {
  if ((!masks && n > 0) || !labels_out || n < 0 || H < 1 || W < 1 || (n > 0 && row_pitch < W) || label_pitch < W) return OVM_ERR_INVALID;
  if (H > kMaxRows) return OVM_ERR_CAPACITY;
  hipLaunchKernelGGL(mask_labels_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, (hipStream_t)stream, masks, plane_stride, row_pitch, (int)n,
                     (int)H, (int)W, labels_out, label_pitch);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

int ovm_render_mask_overlay(const uint8_t* image, int64_t image_pitch, const int32_t* labels, int64_t label_pitch,
                            const uint8_t* colors, int32_t n, int32_t alpha, uint8_t* out, int64_t out_pitch, int32_t H, int32_t W,
                            ovm_stream_t stream) {
  if (!image || !labels || !out || (!colors && n > 0) || n < 0 || H < 1 || W < 1 || alpha < 0 || alpha > 255) return OVM_ERR_INVALID;
  if (image_pitch < 3 * (int64_t)W || out_pitch < 3 * (int64_t)W || label_pitch < W) return OVM_ERR_INVALID;
  if (H > kMaxRows) return OVM_ERR_CAPACITY;
  hipLaunchKernelGGL(mask_overlay_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, (hipStream_t)stream, image, image_pitch, labels,
                     label_pitch, colors, (int)n, (int)alpha, out, out_pitch, (int)H, (int)W);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
