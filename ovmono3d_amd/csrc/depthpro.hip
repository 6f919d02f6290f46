// Depth Pro (include/ovm3d.h, "Depth Pro, metric depth"): Hugging Face DepthProForDepthEstimation + DepthProImageProcessor as
// OVMono3D-GEO calls depth_pro's model.infer (reference tools/ovmono3d_geo.py:267,290-295).
//
// The three encoders are Towers of the Hugging Face Dinov2Model family (tower.hpp: float input as strided views, taps, final
// LayerNorm). Neck, fusion and the first two head layers go through launch_gemm (1x1: row-major, 3x3: A_CONV3X3, transposed
// convolutions: EPI_CONVT). The kernels of this file:
//   dp_pyramid_kernel     uint8 image -> (x / 255 - 0.5) / 0.5 -> bilinear S x S -> the 0.5 and 0.25 levels, one pass; a thread owns a
//                         4 x 4 block of level 0, which holds every tap of its 2 x 2 level-1 cells and of its level-2 cell
//   dp_merge_kernel       [crops][T][D] tokens -> one map: class token dropped, inner crop borders cut, bilinear resize when the merged
//                         side is not the target; written as the split fp16 rows the next GEMM reads
//   dp_unsplit_kernel     split fp16 -> fp32 (+ relu'd zero-bordered copy): the one decoder level whose projection is the identity
//   dp_conv_s2_kernel     3x3 stride-2 convolution + ReLU (+ add) on maps of <= 2 g cells: the field-of-view head (direct, fp32)
//   dp_dot_kernel         its final k x k valid convolution to one number
//   dp_head_tail_kernel   conv3x3 C -> 32, ReLU, 1x1 32 -> 1, ReLU at S x S on the matrix cores: the 32 channels of a pixel stay in the
//                         MFMA accumulators, only the scalar is stored
//   dp_clear_borders_kernel  zeroes the one-pixel frames of the zero-bordered images (their interiors are overwritten by every call)
//   dp_depth_out_kernel   focal length (given or from the field of view, read on the device), canonical * W / f, bilinear resize to
//                         H x W, 1 / clamp
// Layouts: maps are NHWC. GEMM inputs are split fp16 (hi, lo; lo absent at precision 1): row-major [pixels][C] for 1x1 / transposed
// convolutions, zero-bordered [side + 2][side + 2][C] for 3x3. Skip connections and debug stages are fp32 [pixels][C].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ovm3d.h"
#include "kernels.hpp"
#include "tower.hpp"
#include "depthpro.hpp"
#include "loader.hpp"

using namespace ovm;

namespace {

struct ResUnit { PackedLin c1, c2; };
struct FusionLayer { ResUnit r1, r2; PackedLin deconv, proj; bool has_r1 = false, has_deconv = false; };
struct DirectConv { float* w = nullptr; float* b = nullptr; int Cin = 0, Cout = 0; };   // fp32 [Cout][ky][kx][Cin]

constexpr int kTailCo = 32;      // channels of the depth head's last 3x3 convolution (fixed by the architecture)
constexpr int kMaxBordered = 24; // zero-bordered images of one infer
constexpr int kStages = 7;       // ovm_depthpro_stage_ms: pyramid, towers, merge + neck, fusion, head, field of view, output
struct Bordered { half_t* hi; half_t* lo; int side, C; };
struct BorderList { int n; Bordered b[kMaxBordered]; };

struct Plan {                    // one infer's buffers, carved from the caller's workspace
  float *P0, *P1, *P2;                       // pyramid, NHWC fp32
  float *TOK, *TAP[2], *TOKI, *TOKF;         // patch tower: final tokens + two taps [35][T][D]; image / fov tower tokens [T][D]
  SplitImg FEAT[6];                               // image, low, medium, high, hook0, hook1: [side^2][D]
  SplitImg UA, UB;                                // upsample chain ping-pong (unpadded rows)
  SplitImg CAT;                                   // [ (2g)^2 ][2 * sd0]: low-res | image halves of the concatenation
  SplitImg UP[5];                                 // inputs of the five projections, zero-bordered (UP[4] unpadded when the projection is the identity)
  float* NECK[5]; SplitImg NECKP[5];              // projected features fp32 + relu'd zero-bordered copy
  SplitImg T1[5], HSP[5]; float* HS[5];           // per fusion level: relu(conv1) image, fused sum fp32 + relu'd image
  SplitImg Y[5], DEC[4]; float* HID[4];           // residual-unit output rows, deconvolution output rows, projected hidden state fp32 (next level's side)
  float* FUSED; SplitImg FUSEDP; SplitImg H1, H2;      // head
  float *CANON, *FOVF, *FV[6], *FOV;
  BorderList borders;                        // the zero-bordered images: their frames are cleared at the start of every infer
};

}  // namespace

struct OvmDepthPro : ovm::Loader {
  OvmDepthProConfig cfg;
  int device = 0;
  DepthProGeom geo;
  Tower patch, image, fov;
  int D = 0, T = 0, F = 0;
  bool ident4 = false;                       // the last projection is nn.Identity (inter_dims[1] == fusion_dim)
  int side[5] = {0}, upc[5] = {0};           // decoder level sides (2 g .. 32 g) and the channel counts entering the projections
  PackedLin up_img, up_proj[5], up_ct[5][3], fuse, projc[5];
  FusionLayer fl[5];
  PackedLin head0, head1; half_t *tail_whi = nullptr, *tail_wlo = nullptr; float *tail_b = nullptr, *tail_w2 = nullptr, *tail_b2 = nullptr;
  PackedLin fov_neck; DirectConv fov_conv, fov_head[4]; float *fov_fw = nullptr, *fov_fb = nullptr; int fov_k = 0, fov_fc = 0, fov_side[6] = {0};
  float* splitk = nullptr; size_t splitk_cap = 0;
  Plan last; bool has_last = false;
  bool prof = false; hipEvent_t ev[kStages + 1] = {nullptr}; bool ev_valid = false;      // ovm_depthpro_profile_enable
};

namespace {

// Conv2d k x k; the bias is taken when the checkpoint has one
int pack_conv(OvmDepthPro* m, const WeightMap& wm, const std::string& prefix, int Cout, int Cin, int k, bool need_bias, PackedLin* out) {
  int r = ovm::pack_conv(m, wm, prefix, Cout, Cin, k, BIAS_IF_PRESENT, out); if (r) return r;
  if (need_bias && !out->bias) { m->err = "missing weight: " + prefix + ".bias"; return OVM_ERR_MISSING_WEIGHT; }
  return OVM_OK;
}

// ConvTranspose2d k2 s2; bias [Cout] (EPI_CONVT adds it per co), taken when the checkpoint has one
int pack_convt(OvmDepthPro* m, const WeightMap& wm, const std::string& prefix, int Cin, int Cout, PackedLin* out) {
  return ovm::pack_convt(m, wm, prefix, Cin, Cout, BIAS_IF_PRESENT, false, out);
}

int load_direct(OvmDepthPro* m, const WeightMap& wm, const std::string& prefix, int Cout, int Cin, DirectConv* d) {
  const float *w, *b;
  int r = find_weight(m, wm, prefix + ".weight", (int64_t)Cout * Cin * 9, &w); if (r) return r;
  r = find_weight(m, wm, prefix + ".bias", Cout, &b); if (r) return r;
  const std::vector<float> v = reorder_conv(w, Cout, Cin, 3, 3);
  d->Cin = Cin; d->Cout = Cout;
  r = upload_f32(m, v.data(), v.size(), &d->w); if (r) return r;
  return upload_f32(m, b, (size_t)Cout, &d->b);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------

// torch's bilinear source index, align_corners = False: src = max(scale * (dst + 0.5) - 0.5, 0)
__device__ __forceinline__ void bil_tap(int dst, float scale, int in, int* i0, int* i1, float* l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  int a = (int)src; if (a > in - 1) a = in - 1;
  *i0 = a; *i1 = a + (a < in - 1 ? 1 : 0);
  const float l = src - (float)a;
  *l1 = l > 1.f ? 1.f : l;
}
__device__ __forceinline__ float bil_mix(float a, float b, float c, float d, float ly, float lx) {
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}

// One thread per (4 x 4 block of level 0, channel). Level 1 is F.interpolate(scale_factor = 0.5): src = 2 d + 0.5, the mean of
// level-0 pixels (2 d, 2 d + 1) in each direction; level 2 (scale_factor = 0.25, also the resize to the crop side): src = 4 d + 1.5,
// the mean of pixels (4 d + 1, 4 d + 2). Both lie inside the thread's block.
__global__ void dp_pyramid_kernel(const uint8_t* __restrict__ img, int H, int W, int64_t sH, int64_t sW, int64_t sC, int flip, int S,
                                  float* __restrict__ P0, float* __restrict__ P1, float* __restrict__ P2) {
  const int S4 = S >> 2, S2 = S >> 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)S4 * S4 * 3) return;
  const int c = (int)(idx % 3); const int cell = (int)(idx / 3); const int bx = cell % S4, by = cell / S4;
  const uint8_t* src = img + (int64_t)(flip ? 2 - c : c) * sC;
  const float scy = (float)H / (float)S, scx = (float)W / (float)S;
  float v[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int y0, y1; float ly; bil_tap(4 * by + j, scy, H, &y0, &y1, &ly);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int x0, x1; float lx; bil_tap(4 * bx + i, scx, W, &x0, &x1, &lx);
      const float a = ((float)src[y0 * sH + x0 * sW] / 255.f - 0.5f) / 0.5f, b = ((float)src[y0 * sH + x1 * sW] / 255.f - 0.5f) / 0.5f;
      const float cc = ((float)src[y1 * sH + x0 * sW] / 255.f - 0.5f) / 0.5f, d = ((float)src[y1 * sH + x1 * sW] / 255.f - 0.5f) / 0.5f;
      v[j][i] = bil_mix(a, b, cc, d, ly, lx);
      P0[((size_t)(4 * by + j) * S + 4 * bx + i) * 3 + c] = v[j][i];
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      P1[((size_t)(2 * by + j) * S2 + 2 * bx + i) * 3 + c] = bil_mix(v[2 * j][2 * i], v[2 * j][2 * i + 1], v[2 * j + 1][2 * i], v[2 * j + 1][2 * i + 1], 0.5f, 0.5f);
  P2[((size_t)by * S4 + bx) * 3 + c] = bil_mix(v[1][1], v[1][2], v[2][1], v[2][2], 0.5f, 0.5f);
}

// merged-map coordinate -> (crop index along the axis, cell inside the crop): the first crop keeps cells [0, g - pad), inner crops
// [pad, g - pad), the last [pad, g) (merge_patches)
__device__ __forceinline__ void merged_cell(int mcoord, int n, int g, int pad, int* crop, int* cell) {
  if (n == 1 || mcoord < g - pad) { *crop = 0; *cell = mcoord; return; }
  const int r = mcoord - (g - pad), w = g - 2 * pad;
  int i = 1 + r / w;
  if (i > n - 1) i = n - 1;
  *crop = i; *cell = pad + r - (i - 1) * w;
}

// tok: [crops][T][D] fp32 (crop0 = first crop of this level, n x n crops, T = 1 + g * g). One thread per (output cell, 4 channels).
__global__ void dp_merge_kernel(const float* __restrict__ tok, int T, int D, int crop0, int n, int g, int pad, int Ms, int out,
                                half_t* __restrict__ Ohi, half_t* __restrict__ Olo) {
  const int D4 = D >> 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)out * out * D4) return;
  const int d4 = (int)(idx % D4); const int pix = (int)(idx / D4); const int x = pix % out, y = pix / out;
  auto row = [&](int my, int mx) -> const f32x4* {
    int cy, ly, cx, lx;
    merged_cell(my, n, g, pad, &cy, &ly); merged_cell(mx, n, g, pad, &cx, &lx);
    return (const f32x4*)(tok + ((size_t)(crop0 + cy * n + cx) * T + 1 + ly * g + lx) * D) + d4;
  };
  f32x4 v;
  if (Ms == out) {
    v = *row(y, x);
  } else {                                              // F.interpolate(size = out, bilinear, align_corners = False) of the merged map
    const float sc = (float)Ms / (float)out;
    int y0, y1, x0, x1; float ly, lx;
    bil_tap(y, sc, Ms, &y0, &y1, &ly); bil_tap(x, sc, Ms, &x0, &x1, &lx);
    const f32x4 a = *row(y0, x0), b = *row(y0, x1), c = *row(y1, x0), d = *row(y1, x1);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = bil_mix(a[r], b[r], c[r], d[r], ly, lx);
  }
  half4 h, l;
#pragma unroll
  for (int r = 0; r < 4; ++r) { half_t hh, ll; split_f16_nt(v[r], hh, ll); h[r] = hh; l[r] = ll; }
  const size_t o = (size_t)pix * D + d4 * 4;
  *(half4*)(Ohi + o) = h;
  if (Olo) *(half4*)(Olo + o) = l;
}

// split rows [side^2][C] (pad_in: zero-bordered source) -> fp32 rows; Phi: also relu(value) into a zero-bordered split image
__global__ void dp_unsplit_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, int side, int C, int ld, int pad_in,
                                  float* __restrict__ out, half_t* __restrict__ Phi, half_t* __restrict__ Plo) {
  const int C4 = C >> 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)side * side * C4) return;
  const int c4 = (int)(idx % C4); const long pix = idx / C4; const int x = (int)(pix % side), y = (int)(pix / side);
  const size_t prow = (size_t)(y + 1) * (side + 2) + x + 1;
  const size_t s = (pad_in ? prow : (size_t)pix) * ld + c4 * 4;
  const half4 h = *(const half4*)(hi + s);
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (float)h[r];
  if (lo) { const half4 l = *(const half4*)(lo + s);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += (float)l[r]; }
  if (out) *(f32x4*)(out + (size_t)pix * C + c4 * 4) = v;
  if (Phi) {
    half4 ph, pl;
#pragma unroll
    for (int r = 0; r < 4; ++r) { half_t hh, ll; split_f16_nt(fmaxf(v[r], 0.f), hh, ll); ph[r] = hh; pl[r] = ll; }
    *(half4*)(Phi + prow * C + c4 * 4) = ph;
    if (Plo) *(half4*)(Plo + prow * C + c4 * 4) = pl;
  }
}

// out[oy][ox][co] = relu(bias[co] + sum in[2 oy - 1 + ky][2 ox - 1 + kx][:] . w[co][ky][kx][:]) (+ add[(oy * So + ox) * ld_add + co])
__global__ void dp_conv_s2_kernel(const float* __restrict__ in, int Si, int Cin, const float* __restrict__ w, const float* __restrict__ bias, int So, int Cout,
                                  const float* __restrict__ add, int ld_add, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= So * So * Cout) return;
  const int co = idx % Cout; const int pix = idx / Cout; const int ox = pix % So, oy = pix / So;
  float acc = bias[co];
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky; if (iy < 0 || iy >= Si) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx; if (ix < 0 || ix >= Si) continue;
      const f32x4* a = (const f32x4*)(in + ((size_t)iy * Si + ix) * Cin);
      const f32x4* b = (const f32x4*)(w + ((size_t)co * 9 + ky * 3 + kx) * Cin);
      for (int c = 0; c < Cin / 4; ++c) { const f32x4 p = a[c], q = b[c]; acc = fmaf(p[0], q[0], acc); acc = fmaf(p[1], q[1], acc); acc = fmaf(p[2], q[2], acc); acc = fmaf(p[3], q[3], acc); }
    }
  }
  acc = fmaxf(acc, 0.f);
  if (add) acc += add[(size_t)pix * ld_add + co];
  out[idx] = acc;
}

// out[0] = bias[0] + sum_i in[i] * w[i]; one workgroup
__global__ __launch_bounds__(256) void dp_dot_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias, int n, float* __restrict__ out) {
  __shared__ float part[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a = fmaf(in[i], w[i], a);
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (part[0] + part[1]) + (part[2] + part[3]) + bias[0];
}

// The depth head's tail at S x S: conv3x3 C -> 32 (+ bias), ReLU, 1x1 32 -> 1 (+ bias), ReLU, as an implicit GEMM on the matrix cores
// (M = pixels, N = 32, K = 9 C). in: zero-bordered split image [S + 2][S + 2][C] (the transposed convolution's output); w: [32][9 C]
// fp16 (hi, lo), k = tap * C + c. A workgroup owns 16 x 16 pixels, a wave 4 rows of 16: per 32-wide k-step it loads the two weight
// fragments (MFMA "A" side, as gemm.hpp: a lane's 4 accumulators run along n) once and one pixel fragment per row, 8 contiguous
// channels of one pixel straight from the NHWC image (neighbouring taps and rows re-read it from L1 / L2; nothing passes through
// LDS). A lane ends with 8 of its pixel's 32 channels; bias, ReLU and the 1x1 are applied to the accumulators and the four lane
// groups are summed with two shuffles. C % 32 == 0.
template <int NPASS>
__global__ __launch_bounds__(256) void dp_head_tail_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, int S, int C,
                                                           const half_t* __restrict__ whi, const half_t* __restrict__ wlo, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16 + wave * 4, P = S + 2, K = 9 * C;
  f32x4 acc[4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r) { acc[r][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[r][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap - dy * 3;
    for (int c0 = 0; c0 < C; c0 += 32) {
      const size_t wk = (size_t)tap * C + c0 + 8 * fq;
      half8 ah[2], al[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        ah[t] = *(const half8*)(whi + (size_t)(t * 16 + fr) * K + wk);
        if (NPASS == 3) al[t] = *(const half8*)(wlo + (size_t)(t * 16 + fr) * K + wk);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t o = ((size_t)(y0 + r + dy) * P + x0 + fr + dx) * C + c0 + 8 * fq;
        const half8 bh = *(const half8*)(hi + o);
        half8 bl;
        if (NPASS == 3) bl = *(const half8*)(lo + o);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (NPASS == 3) {
            acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh, acc[r][t], 0, 0, 0);
            acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl, acc[r][t], 0, 0, 0);
          }
          acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh, acc[r][t], 0, 0, 0);
        }
      }
    }
  }
  // lane holds, for pixel (y0 + r, x0 + fr), channels n = t * 16 + fq * 4 .. + 3
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int n = t * 16 + fq * 4 + i; sum = fmaf(fmaxf(acc[r][t][i] + b1[n], 0.f), w2[n], sum); }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (fq == 0) out[(size_t)(y0 + r) * S + x0 + fr] = fmaxf(sum + b2[0], 0.f);
  }
}

// the one-pixel frame of zero-bordered split images [side + 2][side + 2][C]: blockIdx.y = image, one thread per (frame pixel, 8 channels)
__global__ void dp_clear_borders_kernel(const BorderList bl) {
  const Bordered b = bl.b[blockIdx.y];
  const int P = b.side + 2, C8 = b.C >> 3, nf = 4 * (b.side + 1);
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)nf * C8) return;
  const int c8 = (int)(idx % C8), f = (int)(idx / C8), e = f / (b.side + 1), k = f - e * (b.side + 1);
  // four runs of side + 1 pixels: top row from the left, right column from the top, bottom row from the right, left column from the bottom
  const int y = e == 0 ? 0 : (e == 1 ? k : (e == 2 ? P - 1 : P - 1 - k)), x = e == 0 ? k : (e == 1 ? P - 1 : (e == 2 ? P - 1 - k : 0));
  const size_t o = ((size_t)y * P + x) * b.C + c8 * 8;
  const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  *(half8*)(b.hi + o) = z;
  if (b.lo) *(half8*)(b.lo + o) = z;
}

// post_process_depth_estimation: f = given, or 0.5 W / tan(0.5 deg2rad(fov)); inv = canonical * W / f; bilinear resize S x S -> H x W;
// depth = 1 / clamp(inv, 1e-4, 1e4). The focal length is read here, on the device.
__global__ void dp_depth_out_kernel(const float* __restrict__ canon, int S, int H, int W, float f_given, const float* __restrict__ fov,
                                    float* __restrict__ depth, float* __restrict__ fov_out, float* __restrict__ f_out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const float fv = fov ? fov[0] : 0.f;
  const float f = f_given > 0.f ? f_given : 0.5f * (float)W / tanf(0.5f * (fv * 0.017453292519943295f));
  if (idx == 0) { if (fov_out) fov_out[0] = fv; if (f_out) f_out[0] = f; }
  if (idx >= (long)H * W) return;
  const int x = (int)(idx % W), y = (int)(idx / W);
  int y0, y1, x0, x1; float ly, lx;
  bil_tap(y, (float)S / (float)H, S, &y0, &y1, &ly); bil_tap(x, (float)S / (float)W, S, &x0, &x1, &lx);
  const float wf = (float)W;
  const float a = canon[(size_t)y0 * S + x0] * wf / f, b = canon[(size_t)y0 * S + x1] * wf / f;
  const float c = canon[(size_t)y1 * S + x0] * wf / f, d = canon[(size_t)y1 * S + x1] * wf / f;
  const float inv = bil_mix(a, b, c, d, ly, lx);
  depth[idx] = 1.0f / fminf(fmaxf(inv, 1e-4f), 1e4f);
}

// ---- GEMM wrappers ---------------------------------------------------------------------------------------------------------------

GemmParams gp(OvmDepthPro* m, const SplitImg& A, const PackedLin& w, long M) {
  GemmParams p; memset(&p, 0, sizeof(p));
  p.Ahi = A.hi; p.Alo = A.lo; p.Whi = w.hi; p.Wlo = w.lo; p.M = (int)M; p.N = w.N; p.K = w.Kpad; p.bias = w.bias;
  p.part_ws = m->splitk; p.part_cap = m->splitk_cap;
  return p;
}

// 1x1 convolution / linear on rows [M][lda]: C fp32 and / or split rows O (ldo; pad_side > 0: into a zero-bordered image)
int lin(OvmDepthPro* m, const SplitImg& A, int lda, long M, const PackedLin& w, float* C, const SplitImg& O, int ldo, int pad_side, hipStream_t s) {
  GemmParams p = gp(m, A, w, M);
  p.lda = lda; p.C = C; p.ldc = w.N; p.Ohi = O.hi; p.Olo = O.lo; p.ldo = ldo; p.padH = p.padW = pad_side;
  return launch_gemm(p, m->cfg.precision, EPI_STORE, A_ROWMAJOR, s);
}

// 3x3 convolution, pad 1, over a zero-bordered image: value = act(conv + bias) + R + R2; C fp32, O split (pad_o: zero-bordered, relu_o: relu'd)
int conv3(OvmDepthPro* m, const SplitImg& A, int side, int Cin, const PackedLin& w, int relu, const float* R, const float* R2, float* C, const SplitImg& O, int ldo,
          bool pad_o, bool relu_o, hipStream_t s) {
  GemmParams p = gp(m, A, w, (long)side * side);
  p.cH = p.cW = side; p.cC = Cin; p.K = 9 * Cin; p.relu = relu; p.R = R; p.ldr = w.N; p.R2 = R2; p.ldr2 = w.N;
  p.C = C; p.ldc = w.N; p.Ohi = O.hi; p.Olo = O.lo; p.ldo = ldo; p.padH = p.padW = pad_o ? side : 0; p.relu_o = relu_o ? 1 : 0;
  return launch_gemm(p, m->cfg.precision, EPI_STORE, A_CONV3X3, s);
}

// ConvTranspose2d k2 s2: rows [side^2][lda] -> [2 side][2 side][Cout] (ldo: pixel stride of O; pad_o: zero-bordered)
int convt(OvmDepthPro* m, const SplitImg& A, int lda, int side, const PackedLin& w, const SplitImg& O, int ldo, bool pad_o, hipStream_t s) {
  GemmParams p = gp(m, A, w, (long)side * side);
  p.lda = lda; p.Ohi = O.hi; p.Olo = O.lo; p.G = side; p.Cout = w.N / 4; p.ldo = ldo; p.padH = p.padW = pad_o ? 2 * side : 0;
  return launch_gemm(p, m->cfg.precision, EPI_CONVT, A_ROWMAJOR, s);
}

// ---- launchers of the kernels above: the engine and the per-kernel entry points at the end of the file fill every launch here. A
// precondition the engine guarantees by its configuration is checked again, before the launch.

int unsplit(const SplitImg& A, int side, int C, int ld, bool pad_in, float* out, const SplitImg& P, hipStream_t s) {
  if (C < 4 || C % 4 != 0 || ld % 4 != 0 || ld < C) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(dp_unsplit_kernel, g1((long)side * side * (C / 4)), dim3(256), 0, s, A.hi, A.lo, side, C, ld, pad_in ? 1 : 0, out, P.hi, P.lo);
  return last_launch();
}

// a thread owns a 4 x 4 block of level 0
int launch_pyramid(const uint8_t* img, int H, int W, int64_t sH, int64_t sW, int64_t sC, int flip, int S, float* P0, float* P1, float* P2, hipStream_t s) {
  if (S < 4 || S % 4 != 0) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(dp_pyramid_kernel, g1((long)(S / 4) * (S / 4) * 3), dim3(256), 0, s, img, H, W, sH, sW, sC, flip, S, P0, P1, P2);
  return last_launch();
}

int launch_merge(const float* tok, int T, int D, int crop0, int n, int g, int pad, int Ms, int out, half_t* Ohi, half_t* Olo, hipStream_t s) {
  if (D < 4 || D % 4 != 0) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(dp_merge_kernel, g1((long)out * out * (D / 4)), dim3(256), 0, s, tok, T, D, crop0, n, g, pad, Ms, out, Ohi, Olo);
  return last_launch();
}

// So = the side a 3x3 stride-2 pad-1 convolution leaves of Si
int launch_conv_s2(const float* in, int Si, int Cin, const float* w, const float* bias, int So, int Cout, const float* add, int ld_add, float* out, hipStream_t s) {
  if (Cin < 4 || Cin % 4 != 0 || So != (Si - 1) / 2 + 1) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(dp_conv_s2_kernel, g1((long)So * So * Cout), dim3(256), 0, s, in, Si, Cin, w, bias, So, Cout, add, ld_add, out);
  return last_launch();
}

int launch_dot(const float* in, const float* w, const float* bias, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(dp_dot_kernel, dim3(1), dim3(256), 0, s, in, w, bias, n, out);
  return last_launch();
}

// a workgroup owns 16 x 16 pixels, a k-step 32 channels
int launch_head_tail(const SplitImg& in, int S, int C, const half_t* whi, const half_t* wlo, const float* b1, const float* w2, const float* b2, int precision,
                     float* out, hipStream_t s) {
  if (S < 16 || S % 16 != 0 || C < 32 || C % 32 != 0) return OVM_ERR_SHAPE;
  if (precision == 3)
    hipLaunchKernelGGL(dp_head_tail_kernel<3>, dim3(S / 16, S / 16), dim3(256), 0, s, in.hi, in.lo, S, C, whi, wlo, b1, w2, b2, out);
  else
    hipLaunchKernelGGL(dp_head_tail_kernel<1>, dim3(S / 16, S / 16), dim3(256), 0, s, in.hi, in.lo, S, C, whi, wlo, b1, w2, b2, out);
  return last_launch();
}

// a thread clears 8 channels of one frame pixel
int launch_clear_borders(const BorderList& bl, hipStream_t s) {
  if (bl.n < 1 || bl.n > kMaxBordered) return OVM_ERR_SHAPE;
  int mx = 0;
  for (int i = 0; i < bl.n; ++i) {
    if (bl.b[i].side < 1 || bl.b[i].C < 8 || bl.b[i].C % 8 != 0) return OVM_ERR_SHAPE;
    const int n = 4 * (bl.b[i].side + 1) * (bl.b[i].C / 8);
    if (n > mx) mx = n;
  }
  hipLaunchKernelGGL(dp_clear_borders_kernel, dim3((mx + 255) / 256, bl.n), dim3(256), 0, s, bl);
  return last_launch();
}

int launch_depth_out(const float* canon, int S, int H, int W, float f_given, const float* fov, float* depth, float* fov_out, float* f_out, hipStream_t s) {
  hipLaunchKernelGGL(dp_depth_out_kernel, g1((long)H * W), dim3(256), 0, s, canon, S, H, W, f_given, fov, depth, fov_out, f_out);
  return last_launch();
}

int k64(int c) { return (c + 63) / 64 * 64; }

// the workspace layout; base null: size only
size_t plan(const OvmDepthPro* m, char* base, Plan* pl) {
  const DepthProGeom& q = m->geo;
  const size_t D = m->D, F = m->F, T = m->T, S = q.S, g = q.g;
  const bool split = m->cfg.precision == 3;
  size_t off = 0;
  auto takef = [&](float** p, size_t n) { *p = (float*)(base + off); off += (n * 4 + 255) / 256 * 256; };
  auto takei = [&](SplitImg* p, size_t n) {
    p->hi = (half_t*)(base + off); off += (n * 2 + 255) / 256 * 256;
    p->lo = nullptr;
    if (split) { p->lo = (half_t*)(base + off); off += (n * 2 + 255) / 256 * 256; }
  };
  takef(&pl->P0, S * S * 3); takef(&pl->P1, S * S * 3 / 4); takef(&pl->P2, S * S * 3 / 16);
  takef(&pl->TOK, q.total * T * D); takef(&pl->TAP[0], q.total * T * D); takef(&pl->TAP[1], q.total * T * D);
  takef(&pl->TOKI, T * D); takef(&pl->TOKF, T * D);
  const size_t fside[6] = {g, g, 2 * g, 4 * g, 4 * g, 4 * g};
  for (int i = 0; i < 6; ++i) takei(&pl->FEAT[i], fside[i] * fside[i] * D);
  size_t umax = 0;                                        // largest unpadded intermediate of the upsample chains
  for (int i = 0; i < 5; ++i) { const size_t sd = (size_t)m->side[i] * m->side[i] * m->upc[i]; if (sd > umax) umax = sd; }
  takei(&pl->UA, umax); takei(&pl->UB, umax);
  takei(&pl->CAT, 4 * g * g * 2 * m->cfg.scaled_dims[0]);
  for (int i = 0; i < 5; ++i) {
    const size_t px = (size_t)m->side[i] * m->side[i];
    takef(&pl->NECK[i], px * F); takef(&pl->HS[i], px * F); takei(&pl->Y[i], px * F);
    if (i < 4) { takei(&pl->DEC[i], 4 * px * F); takef(&pl->HID[i], 4 * px * F); }
  }
  if (m->ident4) takei(&pl->UP[4], (size_t)m->side[4] * m->side[4] * m->upc[4]);
  takef(&pl->FUSED, (size_t)m->side[4] * m->side[4] * F);
  takef(&pl->CANON, S * S);
  takef(&pl->FOVF, T * (F / 2));
  for (int i = 0; i < 6; ++i) takef(&pl->FV[i], g * g * F);
  takef(&pl->FOV, 64);
  // zero-bordered images: only their frames are cleared (dp_clear_borders_kernel), the interiors are overwritten by every call
  pl->borders.n = 0;
  auto takeb = [&](SplitImg* p, int side, int C) {
    takei(p, (size_t)(side + 2) * (side + 2) * C);
    pl->borders.b[pl->borders.n++] = Bordered{p->hi, p->lo, side, C};
  };
  for (int i = 0; i < 5; ++i) {
    if (!(i == 4 && m->ident4)) takeb(&pl->UP[i], m->side[i], m->upc[i]);
    takeb(&pl->NECKP[i], m->side[i], (int)F); takeb(&pl->T1[i], m->side[i], (int)F); takeb(&pl->HSP[i], m->side[i], (int)F);
  }
  takeb(&pl->FUSEDP, m->side[4], (int)F);
  takeb(&pl->H2, (int)S, (int)F / 2);
  takei(&pl->H1, (size_t)m->side[4] * m->side[4] * k64((int)F / 2));      // its pad columns (F / 2 < 64 only) are cleared with the rows
  return off;
}

int run_tower(OvmDepthPro* m, Tower* t, const TowerViews& v, int ntap, const int* blk, float* const* taps, float* fin, const char* what, hipStream_t s) {
  const int r = tower_forward_f32(t, v, ntap, blk, taps, fin, s);
  if (r) m->err = std::string(what) + ": " + t->err;
  return r;
}

}  // namespace

namespace ovm {

int depthpro_geometry(const OvmDepthProConfig& c, DepthProGeom* geo, std::string* err) {
  const float want_r[3] = {0.25f, 0.5f, 1.0f}, want_o[3] = {0.0f, 0.5f, 0.25f};
  for (int i = 0; i < 3; ++i)
    if (c.ratios[i] != want_r[i] || c.overlaps[i] != want_o[i]) {
      char b[320];
      snprintf(b, sizeof(b), "unsupported pyramid: scaled_images_ratios (%g, %g, %g) with overlap ratios (%g, %g, %g); only the ratios 0.25 / 0.5 / 1 "
               "with the overlaps 0 / 0.5 / 0.25 on a canvas of 4 * crop are built", c.ratios[0], c.ratios[1], c.ratios[2], c.overlaps[0], c.overlaps[1], c.overlaps[2]);
      if (err) *err = b;
      return OVM_ERR_UNSUPPORTED;
    }
  if (c.patch != 16 || c.crop < 64 || c.crop % 64 != 0 || c.merge_padding < 0) {
    if (err) *err = "invalid config (patch 16, crop a multiple of 64, merge_padding >= 0)";
    return OVM_ERR_INVALID;
  }
  DepthProGeom q;
  q.crop = c.crop; q.g = c.crop / 16; q.S = 4 * c.crop;
  const int lev[3] = {q.S, q.S / 2, q.S / 4};            // level sides at ratio 1, 0.5, 0.25
  const float ov[3] = {0.25f, 0.5f, 0.0f}; const float ra[3] = {1.0f, 0.5f, 0.25f};
  q.total = 0;
  for (int i = 0; i < 3; ++i) {
    q.stride[i] = (int)((float)c.crop * (1.0f - ov[i]));
    q.ncrop[i] = lev[i] == c.crop ? 1 : (lev[i] - c.crop) / q.stride[i] + 1;
    int pad = (int)((float)c.merge_padding * (1.0f / ra[i]));
    if (q.ncrop[i] * q.ncrop[i] < 4) pad = 0;
    if (pad > q.g / 4) pad = q.g / 4;
    q.pad[i] = pad;
    q.merged[i] = q.ncrop[i] == 1 ? q.g : q.ncrop[i] * q.g - 2 * (q.ncrop[i] - 1) * pad;
    q.out[i] = q.g << (2 - i);
    q.total += q.ncrop[i] * q.ncrop[i];
  }
  if (q.total > kMaxTowerViews) { if (err) *err = "too many crops"; return OVM_ERR_CAPACITY; }
  if (geo) *geo = q;
  return OVM_OK;
}

}  // namespace ovm

extern "C" {

int ovm_host_depthpro_check(const OvmDepthProConfig* cfg, char* msg, int32_t capacity) {
  if (!cfg) return OVM_ERR_INVALID;
  std::string e;
  const int r = depthpro_geometry(*cfg, nullptr, &e);
  if (msg && capacity > 0) { strncpy(msg, e.c_str(), (size_t)capacity - 1); msg[capacity - 1] = 0; }
  return r;
}

const char* ovm_depthpro_last_error(const OvmDepthPro* m) { return m ? m->err.c_str() : "null handle"; }

int ovm_depthpro_destroy(OvmDepthPro* m) {
  if (!m) return OVM_OK;
  (void)hipSetDevice(m->device);
  m->patch.destroy(); m->image.destroy(); m->fov.destroy();
  m->free_all();
  for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
  delete m;
  return OVM_OK;
}

int ovm_depthpro_create(const OvmDepthProConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmDepthPro** out) {
  if (!cfg || !out) return OVM_ERR_INVALID;
  OvmDepthPro* m = new OvmDepthPro();
  *out = m;
  m->cfg = *cfg; m->device = device; m->precision = cfg->precision; m->k_align = 64;
  const OvmDepthProConfig& c = m->cfg;
  int r;
  if ((r = depthpro_geometry(c, &m->geo, &m->err))) return r;           // host only: before any device call
  const DepthProGeom& q = m->geo;
  const int D = c.embed_dim, F = c.fusion_dim, g = q.g;
  if (c.heads < 1 || D != c.heads * 64) {
    m->err = "unsupported towers: head dimension " + std::to_string(c.heads > 0 ? D / c.heads : 0) + "; the attention kernels take head dimension 64 only";
    return OVM_ERR_UNSUPPORTED;
  }
  bool ok = D % 128 == 0 && c.depth >= 1 && F >= 64 && F % 64 == 0 && (c.precision == 1 || c.precision == 3) && c.num_fov_layers >= 1 && c.num_fov_layers <= 4 &&
            (F >> (c.num_fov_layers + 1)) >= 4 && (F >> (c.num_fov_layers + 1)) % 4 == 0 && (F / 2) % 32 == 0;
  for (int i = 0; i < 3; ++i) ok = ok && c.scaled_dims[i] >= 64 && c.scaled_dims[i] % 64 == 0;
  for (int i = 0; i < 2; ++i) ok = ok && c.inter_dims[i] >= 64 && c.inter_dims[i] % 64 == 0 && c.hook_ids[i] >= 0 && c.hook_ids[i] < c.depth;
  if (!ok) { m->err = "invalid config (embed_dim % 128, fusion / feature dims multiples of 64, hook ids inside the tower, precision in {1,3}, 1..4 FOV head layers)"; return OVM_ERR_INVALID; }
  m->D = D; m->F = F; m->T = 1 + g * g;
  m->ident4 = c.inter_dims[1] == F;
  for (int i = 0; i < 5; ++i) m->side[i] = (2 * g) << i;
  m->upc[0] = c.scaled_dims[0]; m->upc[1] = c.scaled_dims[1]; m->upc[2] = c.scaled_dims[2]; m->upc[3] = c.inter_dims[0]; m->upc[4] = c.inter_dims[1];
  OVM_HIP(m, hipSetDevice(device));
  const WeightMap wm(weights, n_weights);
  if (wm.get("fusion_stage.final.residual_layer1.batch_norm1.weight")) { m->err = "unsupported: batch norm in the fusion residual units"; return OVM_ERR_UNSUPPORTED; }
  // ---- the three towers
  {
    TowerConfig t; memset(&t, 0, sizeof(t));
    t.family = FAM_DINOV2_HF; t.ln_eps = c.ln_eps;
    t.embed_dim = D; t.depth = c.depth; t.heads = c.heads; t.pos_grid = g; t.canvas = c.crop; t.precision = c.precision;
    for (int i = 0; i < 3; ++i) t.pixel_std[i] = 1.f;
    struct { const char* prefix; Tower* t; int batch; const char* what; bool on; } tw[3] = {
        {"depth_pro.encoder.patch_encoder.model.", &m->patch, q.total, "patch encoder", true},
        {"depth_pro.encoder.image_encoder.model.", &m->image, 1, "image encoder", true},
        {"fov_model.fov_encoder.model.", &m->fov, 1, "field-of-view encoder", c.use_fov != 0}};
    for (auto& x : tw) {
      if (!x.on) continue;
      t.max_batch = x.batch; t.prefix = x.prefix;
      if (!(r = x.t->configure(t))) r = x.t->load(weights, n_weights, device);
      if (r) { m->err = std::string(x.what) + ": " + x.t->err; return r; }
    }
  }
  // ---- neck: feature_upsample, fuse_image_with_low_res, feature_projection
  const std::string U = "depth_pro.neck.feature_upsample.";
  if ((r = pack_convt(m, wm, U + "image_block.layers.0", D, c.scaled_dims[0], &m->up_img))) return r;
  for (int i = 0; i < 3; ++i) {
    const std::string P = U + "scaled_images." + std::to_string(i) + ".layers.";
    if ((r = pack_conv(m, wm, P + "0", c.scaled_dims[i], D, 1, false, &m->up_proj[i]))) return r;
    if ((r = pack_convt(m, wm, P + "1", c.scaled_dims[i], c.scaled_dims[i], &m->up_ct[i][0]))) return r;
  }
  for (int i = 0; i < 2; ++i) {
    const std::string P = U + "intermediate." + std::to_string(i) + ".layers.";
    const int mid = i == 0 ? F : c.inter_dims[i];
    if ((r = pack_conv(m, wm, P + "0", mid, D, 1, false, &m->up_proj[3 + i]))) return r;
    for (int k = 0; k < 2 + i; ++k)
      if ((r = pack_convt(m, wm, P + std::to_string(1 + k), k == 0 ? mid : c.inter_dims[i], c.inter_dims[i], &m->up_ct[3 + i][k]))) return r;
  }
  if ((r = pack_conv(m, wm, "depth_pro.neck.fuse_image_with_low_res", c.scaled_dims[0], 2 * c.scaled_dims[0], 1, true, &m->fuse))) return r;
  for (int i = 0; i < 5; ++i) {
    if (i == 4 && m->ident4) break;
    if ((r = pack_conv(m, wm, "depth_pro.neck.feature_projection.projections." + std::to_string(i), F, m->upc[i], 3, false, &m->projc[i]))) return r;
  }
  // ---- fusion stage
  for (int i = 0; i < 5; ++i) {
    FusionLayer& y = m->fl[i];
    const std::string P = i < 4 ? "fusion_stage.intermediate." + std::to_string(i) + "." : std::string("fusion_stage.final.");
    y.has_r1 = i > 0; y.has_deconv = i < 4;
    if (y.has_r1) {
      if ((r = pack_conv(m, wm, P + "residual_layer1.convolution1", F, F, 3, false, &y.r1.c1))) return r;
      if ((r = pack_conv(m, wm, P + "residual_layer1.convolution2", F, F, 3, false, &y.r1.c2))) return r;
    }
    if ((r = pack_conv(m, wm, P + "residual_layer2.convolution1", F, F, 3, false, &y.r2.c1))) return r;
    if ((r = pack_conv(m, wm, P + "residual_layer2.convolution2", F, F, 3, false, &y.r2.c2))) return r;
    if (y.has_deconv && (r = pack_convt(m, wm, P + "deconv", F, F, &y.deconv))) return r;
    if ((r = pack_conv(m, wm, P + "projection", F, F, 1, true, &y.proj))) return r;
  }
  // ---- depth head
  if ((r = pack_conv(m, wm, "head.layers.0", F / 2, F, 3, true, &m->head0))) return r;
  if ((r = pack_convt(m, wm, "head.layers.1", F / 2, F / 2, &m->head1))) return r;
  {
    const int C = F / 2;
    const float *w, *b, *w2, *b2;
    if ((r = find_weight(m, wm, "head.layers.2.weight", (int64_t)kTailCo * C * 9, &w))) return r;
    if ((r = find_weight(m, wm, "head.layers.2.bias", kTailCo, &b))) return r;
    if ((r = find_weight(m, wm, "head.layers.4.weight", kTailCo, &w2))) return r;
    if ((r = find_weight(m, wm, "head.layers.4.bias", 1, &b2))) return r;
    const std::vector<float> v = reorder_conv(w, kTailCo, C, 3, 3);
    std::vector<half_t> vh(v.size()), vl(v.size());                         // [32][tap * C + c], split
    for (size_t i = 0; i < v.size(); ++i) { vh[i] = (half_t)v[i]; vl[i] = (half_t)(v[i] - (float)vh[i]); }
    if ((r = m->alloc(&m->tail_whi, vh.size()))) return r;
    if ((r = m->alloc(&m->tail_wlo, vl.size()))) return r;
    OVM_HIP(m, hipMemcpy(m->tail_whi, vh.data(), vh.size() * 2, hipMemcpyHostToDevice));
    OVM_HIP(m, hipMemcpy(m->tail_wlo, vl.data(), vl.size() * 2, hipMemcpyHostToDevice));
    if ((r = upload_f32(m, b, kTailCo, &m->tail_b))) return r;
    if ((r = upload_f32(m, w2, kTailCo, &m->tail_w2))) return r;
    if ((r = upload_f32(m, b2, 1, &m->tail_b2))) return r;
  }
  // ---- field of view
  if (c.use_fov) {
    if ((r = pack_linear(m, wm, "fov_model.fov_encoder.neck", F / 2, D, &m->fov_neck))) return r;
    if ((r = load_direct(m, wm, "fov_model.conv", F / 2, F, &m->fov_conv))) return r;
    int sd = g; m->fov_side[0] = g;
    for (int i = 0; i < c.num_fov_layers; ++i) {
      if ((r = load_direct(m, wm, "fov_model.head.layers." + std::to_string(2 * i), F >> (i + 2), F >> (i + 1), &m->fov_head[i]))) return r;
      sd = (sd - 1) / 2 + 1; m->fov_side[i + 1] = sd;
    }
    m->fov_k = (int)((float)(g - 1) / (float)(1 << c.num_fov_layers) + 1.f); m->fov_fc = F >> (c.num_fov_layers + 1);
    if (m->fov_k != sd) { m->err = "unsupported field-of-view head: its last convolution does not reduce the map to one number"; return OVM_ERR_UNSUPPORTED; }
    const std::string P = "fov_model.head.layers." + std::to_string(2 * c.num_fov_layers);
    const int k = m->fov_k, C = m->fov_fc;
    const float *w, *b;
    if ((r = find_weight(m, wm, P + ".weight", (int64_t)C * k * k, &w))) return r;
    if ((r = find_weight(m, wm, P + ".bias", 1, &b))) return r;
    const std::vector<float> v = reorder_conv(w, 1, C, k, k);     // [1][C][k][k] -> [ky][kx][C]
    if ((r = upload_f32(m, v.data(), v.size(), &m->fov_fw))) return r;
    if ((r = upload_f32(m, b, 1, &m->fov_fb))) return r;
  }
  m->splitk_cap = (size_t)112 << 20;                      // split-K: <= 96 tiles of 128 x 128, <= 16 slices of fp32 partials
  { char* p = nullptr; if ((r = m->alloc(&p, m->splitk_cap))) return r; m->splitk = (float*)p; }
  OVM_HIP(m, hipDeviceSynchronize());
  return OVM_OK;
}

int ovm_depthpro_workspace(const OvmDepthPro* m, int32_t H, int32_t W, int64_t* bytes) {
  if (!m || !bytes || H < 1 || W < 1 || !m->patch.fam) return OVM_ERR_INVALID;
  Plan pl;
  *bytes = (int64_t)plan(m, nullptr, &pl);
  return OVM_OK;
}

int ovm_depthpro_infer(OvmDepthPro* m, const OvmImage* image, int32_t flip_bgr, float f_px, float* depth_out, float* fov_deg_out, float* f_px_out,
                       void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  if (!m) return OVM_ERR_INVALID;
  m->err.clear();
  if (!m->patch.fam) { m->err = "handle was not created"; return OVM_ERR_INVALID; }
  if (!image || !image->data || image->height < 1 || image->width < 1) { m->err = "null or empty image"; return OVM_ERR_INVALID; }
  if (!depth_out || !workspace) { m->err = "null depth_out or workspace"; return OVM_ERR_INVALID; }
  if ((uintptr_t)workspace & 255) { m->err = "the workspace must be 256-byte aligned"; return OVM_ERR_INVALID; }
  const OvmDepthProConfig& c = m->cfg;
  if (!(f_px > 0.f) && !c.use_fov) { m->err = "f_px must be given: the handle was created without the field-of-view model"; return OVM_ERR_INVALID; }
  Plan pl;
  const size_t need = plan(m, (char*)workspace, &pl);
  if ((int64_t)need > workspace_bytes) {
    m->err = "workspace too small: " + std::to_string(workspace_bytes) + " bytes given, " + std::to_string(need) + " needed (ovm_depthpro_workspace)";
    return OVM_ERR_CAPACITY;
  }
  OVM_HIP(m, hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const DepthProGeom& q = m->geo;
  const int H = image->height, W = image->width, S = q.S, g = q.g, D = m->D, F = m->F, T = m->T;
  m->has_last = false;
  auto stamp = [&](int i) -> int {                      // stage boundaries, only when profiling is on
    if (!m->prof) return OVM_OK;
    return hipEventRecord(m->ev[i], s) == hipSuccess ? OVM_OK : OVM_ERR_HIP;
  };
  m->ev_valid = false;
  OVM_TRY(m, stamp(0));
  {
    OVM_TRY(m, launch_clear_borders(pl.borders, s));
    if (k64(F / 2) != F / 2) {                            // F / 2 = 32: H1's rows carry 32 pad columns, which the next GEMM reads
      const size_t hb = (size_t)m->side[4] * m->side[4] * k64(F / 2) * 2;
      OVM_HIP(m, hipMemsetAsync(pl.H1.hi, 0, hb, s));
      if (pl.H1.lo) OVM_HIP(m, hipMemsetAsync(pl.H1.lo, 0, hb, s));
    }
  }
  // ---- 1. preprocess + pyramid
  OVM_TRY(m, launch_pyramid((const uint8_t*)image->data, H, W, image->stride_h, image->stride_w, image->stride_c, flip_bgr ? 1 : 0, S, pl.P0, pl.P1, pl.P2, s));
  OVM_TRY(m, stamp(1));
  // ---- 2. towers: 35 crops as one batch (high resolution first), the whole image at the crop side for the other two
  {
    TowerViews v; memset(&v, 0, sizeof(v));
    float* lev[3] = {pl.P0, pl.P1, pl.P2}; const int ls[3] = {S, S / 2, S / 4};
    int n = 0;
    for (int l = 0; l < 3; ++l)
      for (int i = 0; i < q.ncrop[l]; ++i)
        for (int j = 0; j < q.ncrop[l]; ++j)
          v.v[n++] = TowerView{lev[l] + ((size_t)i * q.stride[l] * ls[l] + (size_t)j * q.stride[l]) * 3, 1, (int64_t)3 * ls[l], 3};
    v.n = n;
    float* taps[2] = {pl.TAP[0], pl.TAP[1]};
    OVM_TRY(m, run_tower(m, &m->patch, v, 2, c.hook_ids, taps, pl.TOK, "patch encoder", s));
    TowerViews w1; memset(&w1, 0, sizeof(w1));
    w1.n = 1; w1.v[0] = TowerView{pl.P2, 1, (int64_t)3 * (S / 4), 3};
    OVM_TRY(m, run_tower(m, &m->image, w1, 0, nullptr, nullptr, pl.TOKI, "image encoder", s));
    if (c.use_fov) OVM_TRY(m, run_tower(m, &m->fov, w1, 0, nullptr, nullptr, pl.TOKF, "field-of-view encoder", s));
  }
  OVM_TRY(m, stamp(2));
  // ---- 3. token merge: features 0..5 = image, low, medium, high, hook 0, hook 1
  {
    const int c_hi = 0, c_med = q.ncrop[0] * q.ncrop[0], c_low = c_med + q.ncrop[1] * q.ncrop[1];
    struct { const float* tok; int crop0, lvl; } src[6] = {{pl.TOKI, 0, 2}, {pl.TOK, c_low, 2}, {pl.TOK, c_med, 1}, {pl.TOK, c_hi, 0}, {pl.TAP[0], c_hi, 0}, {pl.TAP[1], c_hi, 0}};
    for (int i = 0; i < 6; ++i) {
      const int l = src[i].lvl, out = q.out[l];
      OVM_TRY(m, launch_merge(src[i].tok, T, D, src[i].crop0, q.ncrop[l], g, q.pad[l], q.merged[l], out, pl.FEAT[i].hi, pl.FEAT[i].lo, s));
    }
  }
  // ---- 4. neck
  const int sd0 = c.scaled_dims[0];
  const SplitImg none;
  {
    SplitImg cat_img{pl.CAT.hi + sd0, pl.CAT.lo ? pl.CAT.lo + sd0 : nullptr};
    OVM_TRY(m, convt(m, pl.FEAT[0], D, g, m->up_img, cat_img, 2 * sd0, false, s));                        // image features -> second half
    OVM_TRY(m, lin(m, pl.FEAT[1], D, (long)g * g, m->up_proj[0], nullptr, pl.UA, sd0, 0, s));
    OVM_TRY(m, convt(m, pl.UA, sd0, g, m->up_ct[0][0], pl.CAT, 2 * sd0, false, s));                       // low resolution -> first half
    OVM_TRY(m, lin(m, pl.CAT, 2 * sd0, (long)4 * g * g, m->fuse, nullptr, pl.UP[0], sd0, 2 * g, s));
    for (int i = 1; i < 5; ++i) {                                                                    // medium, high, hook 0, hook 1
      const int side_in = i == 1 ? 2 * g : 4 * g, nct = i < 3 ? 1 : i - 1, Cm = m->up_proj[i].N;
      OVM_TRY(m, lin(m, pl.FEAT[i + 1], D, (long)side_in * side_in, m->up_proj[i], nullptr, pl.UA, Cm, 0, s));
      SplitImg cur = pl.UA, nxt = pl.UB; int sd = side_in, Cc = Cm;
      for (int k = 0; k < nct; ++k) {
        const bool last = k + 1 == nct, pad = last && !(i == 4 && m->ident4);
        const SplitImg& dst = last ? pl.UP[i] : nxt;
        OVM_TRY(m, convt(m, cur, Cc, sd, m->up_ct[i][k], dst, m->upc[i], pad, s));
        sd *= 2; Cc = m->upc[i];
        if (!last) { SplitImg t = cur; cur = nxt; nxt = t; }
      }
    }
    for (int i = 0; i < 5; ++i) {
      if (i == 4 && m->ident4) { OVM_TRY(m, unsplit(pl.UP[4], m->side[4], F, F, false, pl.NECK[4], pl.NECKP[4], s)); break; }
      OVM_TRY(m, conv3(m, pl.UP[i], m->side[i], m->upc[i], m->projc[i], 0, nullptr, nullptr, pl.NECK[i], pl.NECKP[i], F, true, true, s));
    }
  }
  OVM_TRY(m, stamp(3));
  // ---- 5. fusion: y = x + conv2(relu(conv1(relu(x)))) with the relu'd images written by the producing epilogues
  for (int i = 0; i < 5; ++i) {
    const FusionLayer& y = m->fl[i];
    const int sd = m->side[i];
    const float* hs = pl.NECK[i]; SplitImg hsp = pl.NECKP[i];
    if (y.has_r1) {
      OVM_TRY(m, conv3(m, pl.NECKP[i], sd, F, y.r1.c1, 1, nullptr, nullptr, nullptr, pl.T1[i], F, true, false, s));
      OVM_TRY(m, conv3(m, pl.T1[i], sd, F, y.r1.c2, 0, pl.NECK[i], pl.HID[i - 1], pl.HS[i], pl.HSP[i], F, true, true, s));
      hs = pl.HS[i]; hsp = pl.HSP[i];
    }
    OVM_TRY(m, conv3(m, hsp, sd, F, y.r2.c1, 1, nullptr, nullptr, nullptr, pl.T1[i], F, true, false, s));
    OVM_TRY(m, conv3(m, pl.T1[i], sd, F, y.r2.c2, 0, hs, nullptr, nullptr, pl.Y[i], F, false, false, s));
    if (y.has_deconv) {
      OVM_TRY(m, convt(m, pl.Y[i], F, sd, y.deconv, pl.DEC[i], F, false, s));
      OVM_TRY(m, lin(m, pl.DEC[i], F, (long)4 * sd * sd, y.proj, pl.HID[i], none, 0, 0, s));
    } else {
      OVM_TRY(m, lin(m, pl.Y[i], F, (long)sd * sd, y.proj, pl.FUSED, pl.FUSEDP, F, sd, s));
    }
  }
  OVM_TRY(m, stamp(4));
  // ---- 6. depth head
  {
    const int sd = m->side[4], C = F / 2;
    OVM_TRY(m, conv3(m, pl.FUSEDP, sd, F, m->head0, 0, nullptr, nullptr, nullptr, pl.H1, k64(C), false, false, s));
    OVM_TRY(m, convt(m, pl.H1, k64(C), sd, m->head1, pl.H2, C, true, s));
    OVM_TRY(m, launch_head_tail(pl.H2, S, C, m->tail_whi, m->tail_wlo, m->tail_b, m->tail_w2, m->tail_b2, c.precision, pl.CANON, s));
  }
  OVM_TRY(m, stamp(5));
  // ---- 7. field of view
  if (c.use_fov) {
    const PackedLin& nk = m->fov_neck;
    OVM_TRY(m, ovm_g_linear(pl.TOKF, D, T, D, (const uint16_t*)nk.hi, (const uint16_t*)nk.lo, nk.N, nk.Kpad, nk.bias, 0, nullptr, 0, pl.FOVF, F / 2, c.precision, s));
    OVM_TRY(m, launch_conv_s2(pl.NECK[0], 2 * g, F, m->fov_conv.w, m->fov_conv.b, g, F / 2, pl.FOVF + F / 2 /* the class token's row is dropped */, F / 2,
                              pl.FV[0], s));
    for (int i = 0; i < c.num_fov_layers; ++i) {
      const DirectConv& d = m->fov_head[i];
      OVM_TRY(m, launch_conv_s2(pl.FV[i], m->fov_side[i], d.Cin, d.w, d.b, m->fov_side[i + 1], d.Cout, nullptr, 0, pl.FV[i + 1], s));
    }
    OVM_TRY(m, launch_dot(pl.FV[c.num_fov_layers], m->fov_fw, m->fov_fb, m->fov_k * m->fov_k * m->fov_fc, pl.FOV, s));
  }
  OVM_TRY(m, stamp(6));
  // ---- 8. metres
  OVM_TRY(m, launch_depth_out(pl.CANON, S, H, W, f_px > 0.f ? f_px : 0.f, c.use_fov ? pl.FOV : (const float*)nullptr, depth_out, fov_deg_out, f_px_out, s));
  OVM_TRY(m, stamp(7));
  m->ev_valid = m->prof;
  m->last = pl; m->has_last = true;
  return OVM_OK;
}

int ovm_depthpro_profile_enable(OvmDepthPro* m, int32_t on) {
  if (!m || !m->patch.fam) return OVM_ERR_INVALID;
  if (on && !m->ev[0]) {
    OVM_HIP(m, hipSetDevice(m->device));
    for (int i = 0; i <= kStages; ++i) OVM_HIP(m, hipEventCreate(&m->ev[i]));
  }
  m->prof = on != 0; m->ev_valid = false;
  return OVM_OK;
}

int ovm_depthpro_stage_ms(OvmDepthPro* m, float* ms, int32_t n) {
  if (!m || !ms || n < kStages) return OVM_ERR_INVALID;
  if (!m->ev_valid) { m->err = "no profiled infer to read (ovm_depthpro_profile_enable, then ovm_depthpro_infer)"; return OVM_ERR_INVALID; }
  OVM_HIP(m, hipEventSynchronize(m->ev[kStages]));
  for (int i = 0; i < kStages; ++i) OVM_HIP(m, hipEventElapsedTime(&ms[i], m->ev[i], m->ev[i + 1]));
  return OVM_OK;
}

int64_t ovm_depthpro_debug_copy(OvmDepthPro* m, const char* name, float* dst, int64_t capacity, ovm_stream_t stream) {
  if (!m || !name || !dst || !m->patch.fam || !m->has_last) return OVM_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  const Plan& pl = m->last; const DepthProGeom& q = m->geo;
  const int64_t S = q.S, g = q.g, D = m->D, F = m->F;
  const float* src = nullptr; int64_t cnt = 0;
  if (n.size() == 8 && n.compare(0, 7, "pyramid") == 0 && n[7] >= '0' && n[7] <= '2') {
    const int l = n[7] - '0'; src = l == 0 ? pl.P0 : (l == 1 ? pl.P1 : pl.P2); cnt = 3 * (S >> l) * (S >> l);
  } else if (n == "tokens_patch") { src = pl.TOK; cnt = (int64_t)q.total * m->T * D; }
  else if (n.size() == 9 && n.compare(0, 8, "features") == 0 && n[8] >= '0' && n[8] <= '5') {
    const int i = n[8] - '0'; const int64_t sd = i < 2 ? g : (i == 2 ? 2 * g : 4 * g);
    cnt = sd * sd * D;
    if (cnt > capacity) return OVM_ERR_CAPACITY;
    return unsplit(pl.FEAT[i], (int)sd, (int)D, (int)D, false, dst, SplitImg(), s) ? OVM_ERR_HIP : cnt;
  } else if (n.size() == 5 && n.compare(0, 4, "neck") == 0 && n[4] >= '0' && n[4] <= '4') {
    const int i = n[4] - '0'; src = pl.NECK[i]; cnt = (int64_t)m->side[i] * m->side[i] * F;
  } else if (n == "fused") { src = pl.FUSED; cnt = (int64_t)m->side[4] * m->side[4] * F; }
  else if (n == "canonical") { src = pl.CANON; cnt = S * S; }
  else if (n == "fov") { if (!m->cfg.use_fov) return OVM_ERR_INVALID; src = pl.FOV; cnt = 1; }
  else return OVM_ERR_INVALID;
  if (cnt > capacity) return OVM_ERR_CAPACITY;
  if (hipMemcpyAsync(dst, src, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  return cnt;
}

// The kernels of this file one at a time (tests): the arguments are checked, then the engine's own launcher is called. None synchronises.
int ovm_op_dp_pyramid(const uint8_t* img, int32_t H, int32_t W, int64_t stride_h, int64_t stride_w, int64_t stride_c, int32_t flip, int32_t S, float* P0,
                      float* P1, float* P2, ovm_stream_t stream) {
  if (!img || !P0 || !P1 || !P2 || H < 1 || W < 1) return OVM_ERR_INVALID;
  return launch_pyramid(img, H, W, stride_h, stride_w, stride_c, flip ? 1 : 0, S, P0, P1, P2, (hipStream_t)stream);
}

int ovm_op_dp_merge(const float* tok, int32_t T, int32_t D, int32_t crop0, int32_t n, int32_t g, int32_t pad, int32_t Ms, int32_t out, uint16_t* hi,
                    uint16_t* lo, ovm_stream_t stream) {
  if (!tok || !hi || crop0 < 0 || n < 1 || g < 1 || pad < 0 || out < 1) return OVM_ERR_INVALID;
  if (n == 1 && pad != 0) return OVM_ERR_SHAPE;
  if (T < 1 + g * g || 2 * pad >= g || Ms != n * g - 2 * (n - 1) * pad) return OVM_ERR_SHAPE;
  return launch_merge(tok, T, D, crop0, n, g, pad, Ms, out, (half_t*)hi, (half_t*)lo, (hipStream_t)stream);
}

int ovm_op_dp_unsplit(const uint16_t* hi, const uint16_t* lo, int32_t side, int32_t C, int32_t ld, int32_t pad_in, float* out, uint16_t* p_hi,
                      uint16_t* p_lo, ovm_stream_t stream) {
  if (!hi || side < 1 || (!out && !p_hi) || (p_lo && !p_hi)) return OVM_ERR_INVALID;
  return unsplit(SplitImg{(half_t*)hi, (half_t*)lo}, side, C, ld, pad_in != 0, out, SplitImg{(half_t*)p_hi, (half_t*)p_lo}, (hipStream_t)stream);
}

int ovm_op_dp_conv_s2(const float* in, int32_t Si, int32_t Cin, const float* w, const float* bias, int32_t Cout, const float* add, int32_t ld_add,
                      float* out, ovm_stream_t stream) {
  if (!in || !w || !bias || !out || Si < 1 || Cout < 1) return OVM_ERR_INVALID;
  if (add && ld_add < Cout) return OVM_ERR_SHAPE;
  return launch_conv_s2(in, Si, Cin, w, bias, (Si - 1) / 2 + 1, Cout, add, ld_add, out, (hipStream_t)stream);
}

int ovm_op_dp_dot(const float* in, const float* w, const float* bias, int32_t n, float* out, ovm_stream_t stream) {
  if (!in || !w || !bias || !out || n < 1) return OVM_ERR_INVALID;
  return launch_dot(in, w, bias, n, out, (hipStream_t)stream);
}

int ovm_op_dp_head_tail(const uint16_t* hi, const uint16_t* lo, int32_t S, int32_t C, const uint16_t* w_hi, const uint16_t* w_lo, const float* b1,
                        const float* w2, const float* b2, int32_t precision, float* out, ovm_stream_t stream) {
  if (!hi || !w_hi || !b1 || !w2 || !b2 || !out || (precision != 1 && precision != 3) || (precision == 3 && (!lo || !w_lo))) return OVM_ERR_INVALID;
  return launch_head_tail(SplitImg{(half_t*)hi, (half_t*)lo}, S, C, (const half_t*)w_hi, (const half_t*)w_lo, b1, w2, b2, precision, out, (hipStream_t)stream);
}

int ovm_op_dp_clear_borders(uint16_t* const* hi, uint16_t* const* lo, const int32_t* side, const int32_t* C, int32_t n, ovm_stream_t stream) {
  if (!hi || !side || !C || n < 1) return OVM_ERR_INVALID;
  if (n > kMaxBordered) return OVM_ERR_SHAPE;
  BorderList bl; memset(&bl, 0, sizeof(bl));
  bl.n = n;
  for (int i = 0; i < n; ++i) {
    if (!hi[i]) return OVM_ERR_INVALID;
    bl.b[i] = Bordered{(half_t*)hi[i], lo ? (half_t*)lo[i] : nullptr, side[i], C[i]};
  }
  return launch_clear_borders(bl, (hipStream_t)stream);
}

int ovm_op_dp_depth_out(const float* canon, int32_t S, int32_t H, int32_t W, float f_px, const float* fov_deg, float* depth, float* fov_out, float* f_out,
                        ovm_stream_t stream) {
  if (!canon || !depth || S < 1 || H < 1 || W < 1 || (!(f_px > 0.f) && !fov_deg)) return OVM_ERR_INVALID;
  return launch_depth_out(canon, S, H, W, f_px > 0.f ? f_px : 0.f, fov_deg, depth, fov_out, f_out, (hipStream_t)stream);
}

}  // extern "C"
