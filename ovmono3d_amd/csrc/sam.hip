// Segment Anything (include/ovm3d.h, "Segment Anything, box-prompted"): SamPredictor.set_image / predict of segment_anything as
// OVMono3D-GEO calls them (reference tools/ovmono3d_geo.py:213-217,270-272,308-309: a box, multimask outputs), and the predictor's
// other prompts (points, a box with points, a mask input, the single-mask output: ovm_sam_predict).
//
// The image encoder's blocks are a Tower of the segment_anything family (tower.hpp: configure / load / tower_forward). Everything behind them is
// sequenced here from the generic fp32 device ops (ovm_g_linear / ovm_g_layernorm / ovm_g_bmm2 / ovm_g_softmax) plus the kernels
// of this file:
//   sam_i2t_attn_kernel   image -> token cross attention: G*G queries against <= 8 (box prompts) or <= 16 token keys per prompt,
//                         score + softmax + value sum in registers (a tiled attention kernel would spend its key tile on 7 keys)
//   sam_point_tokens_kernel / sam_mask_embed_kernel   the prompt encoder for points and for a mask input (mask_downscaling, fused)
//   sam_mask_boxes_kernel tight box and pixel count of a mask plane
//   sam_mask_out_kernel   postprocess_masks + threshold: both bilinear resamplings (4G -> S, crop, -> H x W) evaluated per output
//                         pixel from the low-resolution logits, uint8 written at (H, W); the S x S plane never exists in HBM
//   sam_mask_stats_kernel the same value counted instead of written (automatic mask generation): per plane the pixel counts above
//                         +offset, 0 and -offset and the tight box, S-plane rows cached in LDS; nothing of image size is written
//   sam_mask_prod_kernel  hypernetwork product over the requested mask tokens
//   small element-wise ones (box embedding, dense positional encoding, LayerNorm + GELU of the upscaling, broadcast add)
// Layouts: every activation is fp32 row-major [rows][channels]; image-side rows are (box, y * G + x). The two transposed
// convolutions of the upscaling are GEMMs over source pixels whose output columns are (a * 2 + b) * Cout + co, so the upscaled map is
// kept blocked: pixel (4 i + 2 a + a2, 4 j + 2 b + b2) of box n lives at row ((n * G*G + i * G + j) * 4 + a * 2 + b), columns
// (a2 * 2 + b2) * C8 .. + C8.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ovm3d.h"
#include "det2d.hpp"
#include "kernels.hpp"
#include "tower.hpp"

using namespace ovm;

namespace {

struct Attn { PackedLin q, k, v, o; };
struct Norm { float* g = nullptr; float* b = nullptr; };
struct DecLayer { Attn self, t2i, i2t; PackedLin lin1, lin2; Norm n1, n2, n3, n4; };

constexpr int kMaxTok = 8;           // tokens per box the image -> token kernel holds (1 IoU + mask tokens + 2 corners)
constexpr int kMaxTok16 = 16;        // its second instantiation: point prompts
constexpr int kMaxPoints = 8;        // points per prompt: 5 + 8 + 2 = 15 tokens
constexpr float kDecEps = 1e-5f;     // nn.LayerNorm default of the two-way transformer
constexpr float kLn2dEps = 1e-6f;    // LayerNorm2d of the neck and the upscaling

}  // namespace

struct OvmSam : ovm::Loader {
  OvmSamConfig cfg;
  int device = 0;
  Tower tower;                               // the image encoder (tower.fam is set once ovm_sam_create has come as far as configuring it)
  int G = 0, G2 = 0, C = 0, S = 0, L = 0, nt = 0, I = 0;      // grid, prompt width, image size, low-res side 4G, tokens per box, cross-attention width
  // neck
  PackedLin neck1, neck3; Norm nn1, nn3;
  half_t *pad_hi = nullptr, *pad_lo = nullptr; float *T1 = nullptr, *T2 = nullptr, *emb = nullptr, *src0 = nullptr, *pe = nullptr;
  // prompt encoder
  float *gauss = nullptr, *corner = nullptr /* point_embeddings 2, 3: [2][C] */, *no_mask = nullptr;
  float *point_emb = nullptr /* point_embeddings 0, 1: [2][C] */, *not_a_point = nullptr;
  float *md_w0 = nullptr, *md_b0 = nullptr, *md_g1 = nullptr, *md_be1 = nullptr, *md_w3 = nullptr, *md_b3 = nullptr, *md_g4 = nullptr, *md_be4 = nullptr,
        *md_w6 = nullptr, *md_b6 = nullptr;                                                       // mask_downscaling 0, 1, 3, 4, 6
  // decoder
  float* out_tokens = nullptr;          // [1 + num_mask_tokens][C]: iou_token, mask_tokens
  std::vector<DecLayer> layers; Attn fin; Norm nfin;
  PackedLin up1, up2; Norm upn; std::vector<PackedLin> hyper; PackedLin iou[8]; int n_iou = 0;
  // image state
  bool has_image = false; int H = 0, W = 0, newh = 0, neww = 0;
  uint8_t *rs_tmp = nullptr, *rs_dst = nullptr; size_t rs_tmp_cap = 0;
  int *tab = nullptr; size_t tab_cap = 0; int tabH = -1, tabW = -1, xk = 0, yk = 0; size_t off_xc = 0, off_yb = 0, off_yc = 0;
  std::vector<int> tab_host;
  // debug copies of the last chunk
  float *dbg_sparse = nullptr, *dbg_tokens = nullptr, *dbg_dense = nullptr; int dbg_n = 0, dbg_ns = 2, dbg_nt = 0; bool dbg_dense_mask = false;
};

namespace {

int pack_attn(OvmSam* m, const WeightMap& wm, const std::string& prefix, int C, int I, Attn* a) {
  int r = pack_linear(m, wm, prefix + ".q_proj", I, C, &a->q); if (r) return r;
  r = pack_linear(m, wm, prefix + ".k_proj", I, C, &a->k); if (r) return r;
  r = pack_linear(m, wm, prefix + ".v_proj", I, C, &a->v); if (r) return r;
  return pack_linear(m, wm, prefix + ".out_proj", C, I, &a->o);
}

int load_norm(OvmSam* m, const WeightMap& wm, const std::string& prefix, int D, Norm* n) {
  int r = upload_weight(m, wm, prefix + ".weight", D, &n->g); if (r) return r;
  return upload_weight(m, wm, prefix + ".bias", D, &n->b);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------

// out[i] = a[i] + b[i % bmod]
__global__ void sam_add_bcast_kernel(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ out, long n4, long bmod4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 x = a[i], y = b[i % bmod4];
  out[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

// out[i] = b[i % bmod]
__global__ void sam_bcast_kernel(const float4* __restrict__ b, float4* __restrict__ out, long n4, long bmod4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  out[i] = b[i % bmod4];
}

// PositionEmbeddingRandom._pe_encoding of a point in [0, 1]^2: [sin | cos](2 pi ((2 c - 1) . gauss)), F = C / 2 frequencies
__device__ __forceinline__ void pe_encode(float cx, float cy, const float* __restrict__ gauss, int F, int f, float* s, float* c) {
  const float x = 2.f * cx - 1.f, y = 2.f * cy - 1.f;
  const float v = 6.283185307179586f * (x * gauss[f] + y * gauss[F + f]);
  *s = sinf(v); *c = cosf(v);
}

// get_dense_pe: pe[(i * G + j)][:] for the cell centres ((j + 0.5) / G, (i + 0.5) / G)
__global__ void sam_dense_pe_kernel(const float* __restrict__ gauss, int G, int F, float* __restrict__ pe) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G * G * F) return;
  const int f = idx % F, p = idx / F, i = p / G, j = p - i * G;
  float s, c;
  pe_encode(((float)(j + 1) - 0.5f) / (float)G, ((float)(i + 1) - 0.5f) / (float)G, gauss, F, f, &s, &c);
  pe[(size_t)p * 2 * F + f] = s; pe[(size_t)p * 2 * F + F + f] = c;
}

// tokens of one chunk: tok[b] = [iou_token, mask_tokens, corner 0, corner 1] with corner k = PE of the box corner (original pixels
// -> ResizeLongestSide's frame: * new / old in fp64 as apply_coords, then + 0.5 and / S in fp32 as _embed_boxes) + point_embeddings[2 + k]
__global__ void sam_box_tokens_kernel(const float* __restrict__ boxes, int nb, int nout, int C, const float* __restrict__ out_tokens,
                                      const float* __restrict__ gauss, const float* __restrict__ corner, double sx, double sy, float S,
                                      float* __restrict__ tok, float* __restrict__ sparse) {
  const int nt = nout + 2, F = C / 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)nb * nt * F) return;
  const int f = (int)(idx % F), t = (int)((idx / F) % nt), b = (int)(idx / ((long)F * nt));
  float* o = tok + ((size_t)b * nt + t) * C;
  if (t < nout) { o[f] = out_tokens[(size_t)t * C + f]; o[F + f] = out_tokens[(size_t)t * C + F + f]; return; }
  const int k = t - nout;
  const float px = (float)((double)boxes[b * 4 + 2 * k] * sx), py = (float)((double)boxes[b * 4 + 2 * k + 1] * sy);
  float s, c;
  pe_encode((px + 0.5f) / S, (py + 0.5f) / S, gauss, F, f, &s, &c);
  s += corner[(size_t)k * C + f]; c += corner[(size_t)k * C + F + f];
  o[f] = s; o[F + f] = c;
  float* sp = sparse + ((size_t)b * 2 + k) * C;
  sp[f] = s; sp[F + f] = c;
}

// tokens of one chunk with P points per prompt: tok[b] = [iou_token, mask_tokens, points, then one padding token (no boxes) or the two
// corners]; the sparse rows go to `sparse` [nb][ns][C] as well. A point is treated as a corner is (apply_coords in fp64, + 0.5, / S in
// fp32) and gets point_embeddings[label] for label 0 / 1; any other label is PromptEncoder's -1: not_a_point_embed alone.
__global__ void sam_point_tokens_kernel(const float* __restrict__ points, const int* __restrict__ labels, const float* __restrict__ boxes, int nb, int P,
                                        int nout, int C, const float* __restrict__ out_tokens, const float* __restrict__ gauss,
                                        const float* __restrict__ point_emb, const float* __restrict__ not_a_point, const float* __restrict__ corner,
                                        double sx, double sy, float S, float* __restrict__ tok, float* __restrict__ sparse) {
  const int ns = P + (boxes ? 2 : 1), nt = nout + ns, F = C / 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)nb * nt * F) return;
  const int f = (int)(idx % F), t = (int)((idx / F) % nt), b = (int)(idx / ((long)F * nt));
  float* o = tok + ((size_t)b * nt + t) * C;
  if (t < nout) { o[f] = out_tokens[(size_t)t * C + f]; o[F + f] = out_tokens[(size_t)t * C + F + f]; return; }
  const int k = t - nout;
  const int lab = k < P ? labels[(size_t)b * P + k] : -1;
  float s, c;
  if (k < P && (lab == 0 || lab == 1)) {
    const float* pt = points + ((size_t)b * P + k) * 2;
    const float px = (float)((double)pt[0] * sx), py = (float)((double)pt[1] * sy);
    pe_encode((px + 0.5f) / S, (py + 0.5f) / S, gauss, F, f, &s, &c);
    s += point_emb[(size_t)lab * C + f]; c += point_emb[(size_t)lab * C + F + f];
  } else if (k < P || !boxes) {
    s = not_a_point[f]; c = not_a_point[F + f];
  } else {
    const int j = k - P;
    const float px = (float)((double)boxes[b * 4 + 2 * j] * sx), py = (float)((double)boxes[b * 4 + 2 * j + 1] * sy);
    pe_encode((px + 0.5f) / S, (py + 0.5f) / S, gauss, F, f, &s, &c);
    s += corner[(size_t)j * C + f]; c += corner[(size_t)j * C + F + f];
  }
  o[f] = s; o[F + f] = c;
  float* sp = sparse + ((size_t)b * ns + k) * C;
  sp[f] = s; sp[F + f] = c;
}

__device__ __forceinline__ float gelu_erf(float y) { return 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f)); }

// PromptEncoder.mask_downscaling, fused: one workgroup per embedding cell (prompt b, cell i * G + j). The cell's 4 x 4 patch of the
// mask goes to LDS; 16 threads run conv 2x2 s2 (1 -> 4) . LayerNorm2d . GELU . conv 2x2 s2 (4 -> 16) . LayerNorm2d . GELU on it (four
// positions x four channels, then sixteen channels), every thread c < C the 1x1 convolution's channel c. out [b][cell][C].
__global__ __launch_bounds__(256) void sam_mask_embed_kernel(const float* __restrict__ mask, int G, int C, const float* __restrict__ w0,
                                                             const float* __restrict__ b0, const float* __restrict__ g1, const float* __restrict__ be1,
                                                             const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ g4,
                                                             const float* __restrict__ be4, const float* __restrict__ w6, const float* __restrict__ b6,
                                                             float eps, float* __restrict__ out) {
  __shared__ float patch[16], s1[16], a1[16], s2[16], a2[16];
  const int cell = blockIdx.x, b = blockIdx.y, i = cell / G, j = cell - i * G, L = 4 * G, t = threadIdx.x;
  if (t < 16) patch[t] = mask[(size_t)b * L * L + (size_t)(4 * i + (t >> 2)) * L + 4 * j + (t & 3)];
  __syncthreads();
  if (t < 16) {                                                  // conv 1: position p = (py, px) of the 2 x 2 map, channel c
    const int p = t >> 2, c = t & 3, py = p >> 1, px = p & 1;
    float v = b0[c];
    for (int ky = 0; ky < 2; ++ky)
      for (int kx = 0; kx < 2; ++kx) v = fmaf(w0[c * 4 + ky * 2 + kx], patch[(2 * py + ky) * 4 + 2 * px + kx], v);
    s1[t] = v;
  }
  __syncthreads();
  if (t < 16) {                                                  // LayerNorm2d over the 4 channels of the position, GELU
    const int p = t >> 2, c = t & 3;
    const float mean = (s1[p * 4] + s1[p * 4 + 1] + s1[p * 4 + 2] + s1[p * 4 + 3]) * 0.25f;
    float q = 0.f;
    for (int k = 0; k < 4; ++k) { const float d = s1[p * 4 + k] - mean; q = fmaf(d, d, q); }
    a1[t] = gelu_erf((s1[t] - mean) / sqrtf(q * 0.25f + eps) * g1[c] + be1[c]);
  }
  __syncthreads();
  if (t < 16) {                                                  // conv 2: channel t from [ci][ky][kx]; position (ky, kx) is a1's p
    float v = b3[t];
    for (int ci = 0; ci < 4; ++ci)
      for (int p = 0; p < 4; ++p) v = fmaf(w3[t * 16 + ci * 4 + p], a1[p * 4 + ci], v);
    s2[t] = v;
  }
  __syncthreads();
  if (t < 16) {
    float mean = 0.f;
    for (int k = 0; k < 16; ++k) mean += s2[k];
    mean *= 0.0625f;
    float q = 0.f;
    for (int k = 0; k < 16; ++k) { const float d = s2[k] - mean; q = fmaf(d, d, q); }
    a2[t] = gelu_erf((s2[t] - mean) / sqrtf(q * 0.0625f + eps) * g4[t] + be4[t]);
  }
  __syncthreads();
  if (t < C) {
    float v = b6[t];
    for (int k = 0; k < 16; ++k) v = fmaf(w6[t * 16 + k], a2[k], v);
    out[((size_t)b * G * G + cell) * C + t] = v;
  }
}

// rows of D channels: x = GELU(LayerNorm(x)), in place; one wave per row (D <= 256)
__global__ __launch_bounds__(256) void sam_ln_gelu_kernel(float* __restrict__ x, long M, int D, const float* __restrict__ g,
                                                          const float* __restrict__ b, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  float* xr = x + (size_t)row * D;
  float v[4]; float s = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) { const int j = lane + 64 * t; v[t] = j < D ? xr[j] : 0.f; s += v[t]; }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) { const int j = lane + 64 * t; const float d = j < D ? v[t] - mean : 0.f; q += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    if (j < D) { const float y = (v[t] - mean) * rstd * g[j] + b[j]; xr[j] = 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f)); }
  }
}

// Image -> token cross attention. q [nb * G2][ldq] (heads x DH columns), k / v [nb * nt][ld] -> o [nb * G2][ldo]. One thread per
// (pixel, head): its DH query values in registers, the box's nt <= MAXT keys and values in LDS, softmax over nt in registers. A workgroup
// of 256 threads covers 256 / heads consecutive pixels of ONE box (G2 % (256 / heads) == 0 is checked by the launcher).
template <int DH, int MAXT>                                     // MAXT: the token bound (LDS: 2 KB per token)
__global__ __launch_bounds__(256) void sam_i2t_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, const float* __restrict__ v,
                                                           int ld, int nt, int heads, int G2, long rows, float scale, float* __restrict__ o, int ldo) {
  __shared__ float ks[MAXT * 256], vs[MAXT * 256];
  const int ppb = 256 / heads;                                  // pixels per workgroup
  const long row0 = (long)blockIdx.x * ppb;
  const int box = (int)(row0 / G2), width = heads * DH;
  for (int i = threadIdx.x; i < nt * width; i += 256) {
    const int t = i / width, c = i - t * width;
    ks[i] = k[((size_t)box * nt + t) * ld + c]; vs[i] = v[((size_t)box * nt + t) * ld + c];
  }
  __syncthreads();
  const int h = threadIdx.x % heads;
  const long row = row0 + threadIdx.x / heads;
  if (row >= rows) return;
  float qr[DH];
  const float4* qp = reinterpret_cast<const float4*>(q + (size_t)row * ldq + h * DH);
#pragma unroll
  for (int d = 0; d < DH / 4; ++d) { const float4 t4 = qp[d]; qr[4 * d] = t4.x; qr[4 * d + 1] = t4.y; qr[4 * d + 2] = t4.z; qr[4 * d + 3] = t4.w; }
  float sc[MAXT]; float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    float a = 0.f;
    if (t < nt) {
      const float* kr = ks + t * width + h * DH;
#pragma unroll
      for (int d = 0; d < DH; ++d) a = fmaf(qr[d], kr[d], a);
      a *= scale; mx = fmaxf(mx, a);
    }
    sc[t] = a;
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) { sc[t] = t < nt ? expf(sc[t] - mx) : 0.f; sum += sc[t]; }
  const float inv = 1.0f / sum;
  float acc[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
    if (t < nt) {
      const float p = sc[t] * inv; const float* vr = vs + t * width + h * DH;
#pragma unroll
      for (int d = 0; d < DH; ++d) acc[d] = fmaf(p, vr[d], acc[d]);
    }
  float4* op = reinterpret_cast<float4*>(o + (size_t)row * ldo + h * DH);
#pragma unroll
  for (int d = 0; d < DH / 4; ++d) op[d] = make_float4(acc[4 * d], acc[4 * d + 1], acc[4 * d + 2], acc[4 * d + 3]);
}

// masks[b][t][Y][X] = hyper[b][t0 + t][:] . up[b][Y][X][:] over the blocked upscaled map (layout: file header). One thread per
// (up-row r, tap q2): 128 contiguous bytes of `up` for C8 = 32.
__global__ void sam_mask_prod_kernel(const float* __restrict__ up, const float* __restrict__ hyper, int ld_hyper /* floats per box */, int t0, int ntk,
                                     int C8, int G, long total, float* __restrict__ out, long out_box_stride) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int q2 = (int)(idx & 3); const long r = idx >> 2;            // r = (box * G2 + i * G + j) * 4 + q1
  const int q1 = (int)(r & 3); const long pix = r >> 2;
  const int G2 = G * G; const int box = (int)(pix / G2), p = (int)(pix - (long)box * G2), i = p / G, j = p - i * G;
  const int Y = 4 * i + 2 * (q1 >> 1) + (q2 >> 1), X = 4 * j + 2 * (q1 & 1) + (q2 & 1), L = 4 * G;
  const float4* u = reinterpret_cast<const float4*>(up + (size_t)idx * C8);
  for (int t = 0; t < ntk; ++t) {
    const float4* hy = reinterpret_cast<const float4*>(hyper + (size_t)box * ld_hyper + (size_t)(t0 + t) * C8);
    float a = 0.f;
    for (int c = 0; c < C8 / 4; ++c) { const float4 x = u[c], w = hy[c]; a = fmaf(x.x, w.x, a); a = fmaf(x.y, w.y, a); a = fmaf(x.z, w.z, a); a = fmaf(x.w, w.w, a); }
    out[(size_t)box * out_box_stride + (size_t)t * L * L + (size_t)Y * L + X] = a;
  }
}

// torch's bilinear source index, align_corners = False: scale = in / out (fp32), src = max(scale * (dst + 0.5) - 0.5, 0)
__device__ __forceinline__ void bil_tap(int dst, float scale, int in, int* i0, int* i1, float* l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  const int a = (int)src;
  *i0 = a; *i1 = a + (a < in - 1 ? 1 : 0); *l1 = src - (float)a;
}

// the S x S plane of postprocess_masks at (Y, X), from the L x L logits
__device__ __forceinline__ float up_sample(const float* __restrict__ lg, int L, float sc1, int Y, int X) {
  int y0, y1, x0, x1; float ly, lx;
  bil_tap(Y, sc1, L, &y0, &y1, &ly); bil_tap(X, sc1, L, &x0, &x1, &lx);
  const float a = lg[y0 * L + x0], b = lg[y0 * L + x1], c = lg[y1 * L + x0], d = lg[y1 * L + x1];
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}

// the second resampling's blend of four S-plane samples: the value of postprocess_masks at an output pixel. sam_mask_out_kernel
// thresholds it, sam_mask_stats_kernel counts it; both go through this one function (and through up_sample for a, b, c, d)
__device__ __forceinline__ float mask_blend(float a, float b, float c, float d, float ly, float lx) {
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
}

__device__ __forceinline__ uint8_t mask_pixel(const float* __restrict__ lg, int L, float sc1, int newh, int neww, float sch, float scw, int y, int x) {
  int y0, y1, x0, x1; float ly, lx;
  bil_tap(y, sch, newh, &y0, &y1, &ly); bil_tap(x, scw, neww, &x0, &x1, &lx);
  const float a = up_sample(lg, L, sc1, y0, x0), b = up_sample(lg, L, sc1, y0, x1), c = up_sample(lg, L, sc1, y1, x0), d = up_sample(lg, L, sc1, y1, x1);
  const float vv = mask_blend(a, b, c, d, ly, lx);
  return vv > 0.f ? 1 : 0;
}

// postprocess_masks + `> mask_threshold (0)`: F.interpolate(L -> S) . [:newh, :neww] . F.interpolate(-> H x W), per output pixel.
// Four consecutive output bytes per thread, one 32-bit store where the address allows it.
__global__ void sam_mask_out_kernel(const float* __restrict__ logits, long box_stride, int L, int S, int newh, int neww, int H, int W, long total,
                                    uint8_t* __restrict__ out) {
  const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= total) return;
  const float sc1 = (float)L / (float)S, sch = (float)newh / (float)H, scw = (float)neww / (float)W;
  const long HW = (long)H * W;
  uint32_t packed = 0; uint8_t px[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long i = i4 + e;
    px[e] = 0;
    if (i < total) {
      const int b = (int)(i / HW); const long r = i - (long)b * HW; const int y = (int)(r / W), x = (int)(r - (long)y * W);
      px[e] = mask_pixel(logits + (size_t)b * box_stride, L, sc1, newh, neww, sch, scw, y, x);
    }
    packed |= (uint32_t)px[e] << (8 * e);
  }
  if (i4 + 3 < total && (((uintptr_t)(out + i4)) & 3) == 0) *reinterpret_cast<uint32_t*>(out + i4) = packed;
  else for (int e = 0; e < 4 && i4 + e < total; ++e) out[i4 + e] = px[e];
}

// the encoder's input image back from its patch rows: out[c][y][x], S = G * P
__global__ void sam_unpatch_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, int ld, int G, int P, float* __restrict__ out) {
  const int S = G * P; const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)3 * S * S) return;
  const int x = (int)(idx % S), y = (int)((idx / S) % S), c = (int)(idx / ((long)S * S));
  const size_t o = (size_t)((y / P) * G + x / P) * ld + (size_t)((y % P) * P + x % P) * 3 + c;
  out[idx] = (float)hi[o] + (lo ? (float)lo[o] : 0.f);
}

// iou[b][0:nc] = head[b][c0 : c0 + nc] (multimask: columns 1 .. 3; single mask: column 0)
__global__ void sam_iou_slice_kernel(const float* __restrict__ head, int ldh, int n, int c0, int nc, float* __restrict__ iou) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * nc) return;
  iou[i] = head[(size_t)(i / nc) * ldh + c0 + i % nc];
}

// Tight box and pixel count of mask plane blockIdx.y: per-thread extremes over a grid-stride walk, a wave reduction, then one integer
// atomic per wave and value into box [n][4] (xmin, ymin, xmax, ymax as int32, preset to INT_MAX / -1) and cnt [n].
__global__ void sam_mask_boxes_init_kernel(int* __restrict__ box, int* __restrict__ cnt, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  box[4 * i] = 0x7fffffff; box[4 * i + 1] = 0x7fffffff; box[4 * i + 2] = -1; box[4 * i + 3] = -1; cnt[i] = 0;
}

__global__ __launch_bounds__(256) void sam_mask_boxes_kernel(const uint8_t* __restrict__ masks, int H, int W, int* __restrict__ box, int* __restrict__ cnt) {
  const int b = blockIdx.y; const long HW = (long)H * W;
  const uint8_t* mk = masks + (size_t)b * HW;
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1, c = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256)
    if (mk[i]) {
      const int y = (int)(i / W), x = (int)(i - (long)y * W);
      x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y); ++c;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
    x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64)); c += __shfl_xor(c, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && c > 0) {
    atomicMin(&box[4 * b], x0); atomicMin(&box[4 * b + 1], y0); atomicMax(&box[4 * b + 2], x1); atomicMax(&box[4 * b + 3], y1); atomicAdd(&cnt[b], c);
  }
}

// int32 (xmin, ymin, xmax, ymax) -> fp32 (xmin, ymin, xmax + 1, ymax + 1) in place; zeros for an empty mask
__global__ void sam_mask_boxes_final_kernel(int* __restrict__ box, const int* __restrict__ cnt, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 v = reinterpret_cast<const int4*>(box)[i];
  const bool any = cnt[i] > 0;
  reinterpret_cast<float4*>(box)[i] = any ? make_float4((float)v.x, (float)v.y, (float)(v.z + 1), (float)(v.w + 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- automatic mask generation: the statistics of a mask plane without the plane -------------------------------------------------
// stats [n][7] int32: count(v > +off), count(v > 0), count(v > -off), xmin, ymin, xmax, ymax of v > 0; v = the value mask_pixel
// thresholds. A plane whose skip word is set is left alone by all three kernels.
constexpr int kStatsWords = 7;
constexpr int kStatsLdsFloats = 8192;   // 32 KiB of S-plane samples per workgroup: five workgroups share a CU's 160 KiB
constexpr int kStatsMaxRows = 16;       // S-plane rows a workgroup caches at most
constexpr int kStatsMaxBand = 64;       // output rows per workgroup at most

__global__ void sam_mask_stats_init_kernel(int* __restrict__ st, const int* __restrict__ skip, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (skip && skip[i])) return;
  int* o = st + (size_t)i * kStatsWords;
  o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0x7fffffff; o[4] = 0x7fffffff; o[5] = -1; o[6] = -1;      // sam_mask_boxes_init_kernel's sentinels
}

// Workgroup (band, plane): output rows [band * R, band * R + R) of one plane. The S-plane rows those rows blend (from the first
// row's upper tap to the last row's lower tap, at most NR of them) are evaluated once, by up_sample, into LDS [row][neww]; each
// output pixel is then mask_blend of four cached samples - the arithmetic of mask_pixel, value for value - or of up_sample itself for
// a row beyond the cache. A thread owns columns (x taps once per column) and walks the band's rows; counts and extremes go per
// thread, then per wave (shuffles), then one atomic per wave and value.
__global__ __launch_bounds__(256) void sam_mask_stats_kernel(const float* __restrict__ logits, long plane_stride, const int* __restrict__ skip, int L, int S,
                                                             int newh, int neww, int H, int W, int R, int NR, int txw_log2, float off,
                                                             int* __restrict__ st) {
  extern __shared__ float smp[];
  const int p = blockIdx.y;
  if (skip && skip[p]) return;
  const float* lg = logits + (size_t)p * plane_stride;
  const float sc1 = (float)L / (float)S, sch = (float)newh / (float)H, scw = (float)neww / (float)W;
  const int ya = blockIdx.x * R, yb = min(H, ya + R);
  int Ylo, Yhi, ti; float tl;
  bil_tap(ya, sch, newh, &Ylo, &ti, &tl); bil_tap(yb - 1, sch, newh, &ti, &Yhi, &tl);
  const int nrows = min(Yhi - Ylo + 1, NR);
  for (int i = threadIdx.x; i < nrows * neww; i += 256) {
    const int r = i / neww, X = i - r * neww;
    smp[i] = up_sample(lg, L, sc1, Ylo + r, X);
  }
  __syncthreads();
  auto sample = [&](int Y, int X) -> float { const int r = Y - Ylo; return r < nrows ? smp[r * neww + X] : up_sample(lg, L, sc1, Y, X); };
  const int txw = 1 << txw_log2, tx = threadIdx.x & (txw - 1), ty = threadIdx.x >> txw_log2, nty = 256 >> txw_log2;
  int chi = 0, cmid = 0, clo = 0, bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -1, by1 = -1;
  for (int x = tx; x < W; x += txw) {
    int x0, x1; float lx;
    bil_tap(x, scw, neww, &x0, &x1, &lx);
    bool any = false;
    for (int y = ya + ty; y < yb; y += nty) {
      int y0, y1; float ly;
      bil_tap(y, sch, newh, &y0, &y1, &ly);
      const float v = mask_blend(sample(y0, x0), sample(y0, x1), sample(y1, x0), sample(y1, x1), ly, lx);
      chi += v > off ? 1 : 0; clo += v > -off ? 1 : 0;
      if (v > 0.f) { ++cmid; any = true; by0 = min(by0, y); by1 = max(by1, y); }
    }
    if (any) { bx0 = min(bx0, x); bx1 = max(bx1, x); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    chi += __shfl_xor(chi, o, 64); cmid += __shfl_xor(cmid, o, 64); clo += __shfl_xor(clo, o, 64);
    bx0 = min(bx0, __shfl_xor(bx0, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64));
    bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    int* o = st + (size_t)p * kStatsWords;
    if (chi > 0) atomicAdd(&o[0], chi);
    if (clo > 0) atomicAdd(&o[2], clo);
    if (cmid > 0) { atomicAdd(&o[1], cmid); atomicMin(&o[3], bx0); atomicMin(&o[4], by0); atomicMax(&o[5], bx1); atomicMax(&o[6], by1); }
  }
}

// an empty plane's box: the sentinels -> zeros
__global__ void sam_mask_stats_final_kernel(int* __restrict__ st, const int* __restrict__ skip, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (skip && skip[i])) return;
  int* o = st + (size_t)i * kStatsWords;
  if (o[1] == 0) { o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; }
}

__global__ void sam_fill_int_kernel(int* __restrict__ x, int v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

// filter 1 ahead of the statistics: skip[i] = the plane fails iou > thr (thr > 0; a NaN fails)
__global__ void sam_auto_skip_kernel(const float* __restrict__ iou, float thr, int n, int* __restrict__ skip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) skip[i] = (thr > 0.f && !(iou[i] > thr)) ? 1 : 0;
}

__global__ void sam_auto_rows_kernel(const float* __restrict__ iou, const int* __restrict__ st, const int* __restrict__ skip, int n,
                                     OvmSamCandidate* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  OvmSamCandidate c; memset(&c, 0, sizeof(c));
  c.iou = iou[i];
  if (skip[i]) c.flags = OVM_SAM_CAND_SKIPPED;
  else {
    const int* o = st + (size_t)i * kStatsWords;
    c.cnt_hi = o[0]; c.area = o[1]; c.cnt_lo = o[2];
    c.stability = (float)o[0] / (float)o[2];                       // 0 / 0: NaN, which fails filter 2
    c.box[0] = o[3]; c.box[1] = o[4]; c.box[2] = o[5]; c.box[3] = o[6];
  }
  out[i] = c;
}

// the valid mask of filters 1 and 2 and the NMS operands: the inclusive box as floats, the IoU prediction as the score
__global__ void sam_auto_valid_kernel(const OvmSamCandidate* __restrict__ cands, int m, float pthr, float sthr, float* __restrict__ boxes,
                                      float* __restrict__ scores, int* __restrict__ valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const OvmSamCandidate c = cands[i];
  bool ok = !(c.flags & OVM_SAM_CAND_SKIPPED) && c.iou == c.iou;
  if (pthr > 0.f) ok = ok && c.iou > pthr;
  if (sthr > 0.f) ok = ok && c.stability >= sthr;
  valid[i] = ok ? 1 : 0; scores[i] = c.iou;
#pragma unroll
  for (int k = 0; k < 4; ++k) boxes[4 * i + k] = (float)c.box[k];
}

int lin(OvmSam* m, const PackedLin& w, const float* x, int ldx, long M, int act, const float* res, int ldr, float* y, int ldy, hipStream_t s) {
  return ovm_g_linear(x, ldx, (int)M, w.K, (const uint16_t*)w.hi, (const uint16_t*)w.lo, w.N, w.Kpad, w.bias, act, res, ldr, y, ldy, m->cfg.precision, s);
}

// ---- launchers: the engine and the per-kernel entry points at the end of the file fill every launch here. A precondition the engine
// guarantees by its configuration is checked again, before the launch, so that a call outside it is an error and not a partial result.

// out[i] = a[i] + b[i % bmod]; the kernels move float4s: n and bmod are multiples of 4
int add_bcast(const float* a, const float* b, float* out, long n, long bmod, hipStream_t s) {
  if (n < 0 || bmod < 4 || n % 4 != 0 || bmod % 4 != 0) return OVM_ERR_SHAPE;
  if (n == 0) return OVM_OK;
  hipLaunchKernelGGL(sam_add_bcast_kernel, g1(n / 4), dim3(256), 0, s, (const float4*)a, (const float4*)b, (float4*)out, n / 4, bmod / 4);
  return last_launch();
}

// out[i] = b[i % bmod]
int bcast(const float* b, float* out, long n, long bmod, hipStream_t s) {
  if (n < 0 || bmod < 4 || n % 4 != 0 || bmod % 4 != 0) return OVM_ERR_SHAPE;
  if (n == 0) return OVM_OK;
  hipLaunchKernelGGL(sam_bcast_kernel, g1(n / 4), dim3(256), 0, s, (const float4*)b, (float4*)out, n / 4, bmod / 4);
  return last_launch();
}

int launch_dense_pe(const float* gauss, int G, int F, float* pe, hipStream_t s) {
  hipLaunchKernelGGL(sam_dense_pe_kernel, g1((long)G * G * F), dim3(256), 0, s, gauss, G, F, pe);
  return last_launch();
}

// boxes in the pixels of the H x W image; ResizeLongestSide's frame is newh x neww inside S x S
int launch_box_tokens(const float* boxes, int nb, int nout, int C, const float* out_tokens, const float* gauss, const float* corner, int H, int W, int newh,
                      int neww, int S, float* tok, float* sparse, hipStream_t s) {
  hipLaunchKernelGGL(sam_box_tokens_kernel, g1((long)nb * (nout + 2) * (C / 2)), dim3(256), 0, s, boxes, nb, nout, C, out_tokens, gauss, corner,
                     (double)neww / (double)W, (double)newh / (double)H, (float)S, tok, sparse);
  return last_launch();
}

// points and a box or the padding token per prompt (the kernel's comment); P <= kMaxPoints
int launch_point_tokens(const float* points, const int* labels, const float* boxes, int nb, int P, int nout, int C, const float* out_tokens, const float* gauss,
                        const float* point_emb, const float* not_a_point, const float* corner, int H, int W, int newh, int neww, int S, float* tok,
                        float* sparse, hipStream_t s) {
  if (P < 0 || P > kMaxPoints || (P == 0 && !boxes) || (P > 0 && (!points || !labels))) return OVM_ERR_SHAPE;
  const int nt = nout + P + (boxes ? 2 : 1);
  hipLaunchKernelGGL(sam_point_tokens_kernel, g1((long)nb * nt * (C / 2)), dim3(256), 0, s, points, labels, boxes, nb, P, nout, C, out_tokens, gauss, point_emb,
                     not_a_point, corner, (double)neww / (double)W, (double)newh / (double)H, (float)S, tok, sparse);
  return last_launch();
}

// one workgroup of 256 threads per cell: C <= 256; grid.y = prompts
int launch_mask_embed(const float* mask, int n, int G, int C, const float* w0, const float* b0, const float* g1_, const float* be1, const float* w3,
                      const float* b3, const float* g4, const float* be4, const float* w6, const float* b6, float* out, hipStream_t s) {
  if (C < 1 || C > 256 || G < 1 || n < 1 || n > 65535) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(sam_mask_embed_kernel, dim3((unsigned)(G * G), (unsigned)n), dim3(256), 0, s, mask, G, C, w0, b0, g1_, be1, w3, b3, g4, be4, w6, b6,
                     kLn2dEps, out);
  return last_launch();
}

// one wave holds a row in four registers per lane: D <= 256
int launch_ln_gelu(float* x, long M, int D, const float* g, const float* b, float eps, hipStream_t s) {
  if (D < 1 || D > 256) return OVM_ERR_SHAPE;
  hipLaunchKernelGGL(sam_ln_gelu_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, M, D, g, b, eps);
  return last_launch();
}

// head dimension 16; a workgroup's 256 / heads pixels belong to one box and its LDS holds MAXT tokens of 256 columns
template <int MAXT>
int launch_i2t_attn(const float* q, int ldq, const float* k, const float* v, int ld, int nt, int heads, int G2, int nb, float scale, float* o, int ldo,
                    hipStream_t s) {
  if (nt < 1 || nt > MAXT || heads < 1 || heads > 16 || 256 % heads != 0 || G2 < 1 || G2 % (256 / heads) != 0) return OVM_ERR_SHAPE;
  if (ldq < heads * 16 || ld < heads * 16 || ldo < heads * 16 || ldq % 4 != 0 || ldo % 4 != 0) return OVM_ERR_SHAPE;
  const long rows = (long)nb * G2;
  hipLaunchKernelGGL((sam_i2t_attn_kernel<16, MAXT>), dim3((unsigned)(rows / (256 / heads))), dim3(256), 0, s, q, ldq, k, v, ld, nt, heads, G2, rows, scale, o, ldo);
  return last_launch();
}

int launch_mask_prod(const float* up, const float* hyper, int ld_hyper, int t0, int ntk, int C8, int G, int nb, float* out, long out_box_stride, hipStream_t s) {
  if (C8 < 4 || C8 % 4 != 0 || ld_hyper % 4 != 0) return OVM_ERR_SHAPE;
  const long total = (long)nb * G * G * 16;
  hipLaunchKernelGGL(sam_mask_prod_kernel, g1(total), dim3(256), 0, s, up, hyper, ld_hyper, t0, ntk, C8, G, total, out, out_box_stride);
  return last_launch();
}

int launch_mask_out(const float* logits, long box_stride, int L, int S, int newh, int neww, int H, int W, int nb, uint8_t* out, hipStream_t s) {
  const long total = (long)nb * H * W;
  hipLaunchKernelGGL(sam_mask_out_kernel, g1((total + 3) / 4), dim3(256), 0, s, logits, box_stride, L, S, newh, neww, H, W, total, out);
  return last_launch();
}

int launch_unpatch(const half_t* hi, const half_t* lo, int ld, int G, int P, float* out, hipStream_t s) {
  hipLaunchKernelGGL(sam_unpatch_kernel, g1((long)3 * G * P * G * P), dim3(256), 0, s, hi, lo, ld, G, P, out);
  return last_launch();
}

int launch_iou_slice(const float* head, int ldh, int n, int c0, int nc, float* iou, hipStream_t s) {
  hipLaunchKernelGGL(sam_iou_slice_kernel, g1((long)n * nc), dim3(256), 0, s, head, ldh, n, c0, nc, iou);
  return last_launch();
}

// box: fp32 [n][4] used as int32 until the last kernel; every plane gets up to 256 workgroups, each thread at least 8 pixels
int launch_mask_boxes(const uint8_t* masks, int n, int H, int W, float* box, int* cnt, hipStream_t s) {
  if (n > 65535) return OVM_ERR_SHAPE;
  const long HW = (long)H * W;
  long gx = (HW + 2047) / 2048; if (gx > 256) gx = 256;
  hipLaunchKernelGGL(sam_mask_boxes_init_kernel, g1(n), dim3(256), 0, s, (int*)box, cnt, n);
  hipLaunchKernelGGL(sam_mask_boxes_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, masks, H, W, (int*)box, cnt);
  hipLaunchKernelGGL(sam_mask_boxes_final_kernel, g1(n), dim3(256), 0, s, (int*)box, (const int*)cnt, n);
  return last_launch();
}

// The geometry rules of ovm_op_sam_mask_stats, without a launch (the engine checks them before its first chunk)
int mask_stats_geometry(long plane_stride, int planes, int L, int S, int newh, int neww, int H, int W) {
  if (L < 1 || S < L || newh < 1 || neww < 1 || newh > S || neww > S || 2 * neww > kStatsLdsFloats || H < 1 || W < 1) return OVM_ERR_SHAPE;
  if ((long)H * W >= (1L << 31) || plane_stride < (long)L * L || planes > 65535) return OVM_ERR_SHAPE;
  return OVM_OK;
}

// st int32 [planes][7]. NR = the S-plane rows the LDS budget holds (>= 2: an output row blends two); a band of R output rows spans
// about R * newh / H + 2 of them, so R = (NR - 2) * H / newh keeps a band inside the cache (the kernel evaluates a row beyond it directly).
int launch_mask_stats(const float* logits, long plane_stride, int planes, int L, int S, int newh, int neww, int H, int W, float off, const int* skip, int* st,
                      hipStream_t s) {
  const int g = mask_stats_geometry(plane_stride, planes, L, S, newh, neww, H, W);
  if (g) return g;
  int NR = kStatsLdsFloats / neww; if (NR > kStatsMaxRows) NR = kStatsMaxRows;
  long R = (long)((double)(NR - 2) * (double)H / (double)newh);
  if (R < 1) R = 1;
  if (R > kStatsMaxBand) R = kStatsMaxBand;
  if (R > H) R = H;
  const int bands = (int)((H + R - 1) / R), txw_log2 = W > 128 ? 8 : W > 32 ? 6 : 4;
  hipLaunchKernelGGL(sam_mask_stats_init_kernel, g1(planes), dim3(256), 0, s, st, skip, planes);
  hipLaunchKernelGGL(sam_mask_stats_kernel, dim3((unsigned)bands, (unsigned)planes), dim3(256), (size_t)NR * neww * sizeof(float), s, logits, plane_stride, skip, L, S,
                     newh, neww, H, W, (int)R, NR, txw_log2, off, st);
  hipLaunchKernelGGL(sam_mask_stats_final_kernel, g1(planes), dim3(256), 0, s, st, skip, planes);
  return last_launch();
}

// token queries [nb * nt][I] against Tk keys per box: scores (bmm) -> softmax -> context (bmm); heads x dh = I
int token_attention(OvmSam* m, const float* Q, const float* K, const float* V, int nb, int nt, int Tk, int I, float* scores, float* ctx, hipStream_t s) {
  const int hd = m->cfg.dec_heads, dh = I / hd;
  OVM_TRY(m, ovm_g_bmm2(Q, K, scores, nb, hd, nt, Tk, dh, I, I, Tk, (int64_t)nt * I, (int64_t)Tk * I, (int64_t)hd * nt * Tk, dh, dh, (int64_t)nt * Tk, 1,
                   1.0f / sqrtf((float)dh), s));
  OVM_TRY(m, ovm_g_softmax(scores, nb * hd * nt, Tk, Tk, nullptr, 0, 0, 0, s));
  OVM_TRY(m, ovm_g_bmm2(scores, V, ctx, nb, hd, nt, dh, Tk, Tk, I, I, (int64_t)hd * nt * Tk, (int64_t)Tk * I, (int64_t)nt * I, (int64_t)nt * Tk, dh, dh, 0, 1.0f, s));
  return OVM_OK;
}

struct Work {                       // one chunk's buffers, carved from the caller's workspace
  float *tok0, *q, *qpe, *tq, *tk, *tv, *tctx, *tout, *mlp, *keys, *kpe, *tmp, *iA, *iB, *scores, *up2, *hyp, *h1, *h2, *iouh, *low, *dense;
};

// nt: tokens per prompt of the call; has_mask: the mask-input route's dense embeddings [nb * G2][C] follow everything else
size_t carve(Work* w, char* base, const OvmSam* m, long nb, int nt_call, bool has_mask) {
  const size_t C = m->C, nt = (size_t)nt_call, G2 = m->G2, I = m->I, Mt = (size_t)nb * nt, Mi = (size_t)nb * G2;
  const size_t hid = m->cfg.iou_hidden > m->C ? m->cfg.iou_hidden : m->C;
  size_t off = 0;
  auto take = [&](float** p, size_t floats) { if (w) *p = (float*)(base + off); off += (floats * 4 + 255) / 256 * 256; };
  Work dummy; Work* x = w ? w : &dummy;
  take(&x->tok0, Mt * C); take(&x->q, Mt * C); take(&x->qpe, Mt * C); take(&x->tq, Mt * C); take(&x->tk, Mt * C); take(&x->tv, Mt * C);
  take(&x->tctx, Mt * C); take(&x->tout, Mt * C); take(&x->mlp, Mt * m->cfg.dec_mlp);
  take(&x->keys, Mi * C); take(&x->kpe, Mi * C); take(&x->tmp, Mi * C); take(&x->iA, Mi * I); take(&x->iB, Mi * I);
  take(&x->scores, (size_t)nb * m->cfg.dec_heads * nt * G2);
  take(&x->up2, Mi * 2 * C);                                        // [nb * G2 * 4][4 * C / 8]
  take(&x->hyp, (size_t)nb * m->cfg.num_mask_tokens * (C / 8)); take(&x->h1, (size_t)nb * hid); take(&x->h2, (size_t)nb * hid);
  take(&x->iouh, (size_t)nb * 128); take(&x->low, (size_t)nb * m->L * m->L);
  x->dense = nullptr;
  if (has_mask) take(&x->dense, Mi * C);
  return off;
}

// the prompts of one call (device pointers, advanced per chunk by decode's caller)
struct Prompt {
  const float* points = nullptr; const int* labels = nullptr; int P = 0;       // [n][P][2], [n][P]
  const float* boxes = nullptr;                                                 // [n][4] or null
  const float* mask_in = nullptr;                                               // [n][L][L] or null
  bool multimask = true;
  int ns() const { return P + (boxes ? 2 : 1); }
};

int decode_chunk(OvmSam* m, const Prompt& pr, int nb, int mask_index, uint8_t* masks, float* iou, float* lowres, const Work& w, hipStream_t s) {
  const OvmSamConfig& c = m->cfg;
  const int C = m->C, G2 = m->G2, I = m->I, nout = 1 + c.num_mask_tokens, nt = nout + pr.ns();
  const long Mt = (long)nb * nt, Mi = (long)nb * G2;
  // 1. tokens + sparse embeddings (a box alone: the box kernel, as ever); src = embedding + (no_mask_embed | mask embedding) per prompt
  if (pr.P == 0 && pr.boxes)
    OVM_TRY(m, launch_box_tokens(pr.boxes, nb, nout, C, m->out_tokens, m->gauss, m->corner, m->H, m->W, m->newh, m->neww, m->S, w.tok0, m->dbg_sparse, s));
  else
    OVM_TRY(m, launch_point_tokens(pr.points, pr.labels, pr.boxes, nb, pr.P, nout, C, m->out_tokens, m->gauss, m->point_emb, m->not_a_point, m->corner, m->H,
                                   m->W, m->newh, m->neww, m->S, w.tok0, m->dbg_sparse, s));
  OVM_HIP(m, hipMemcpyAsync(w.q, w.tok0, (size_t)Mt * C * 4, hipMemcpyDeviceToDevice, s));
  if (pr.mask_in) {
    OVM_TRY(m, launch_mask_embed(pr.mask_in, nb, m->G, C, m->md_w0, m->md_b0, m->md_g1, m->md_be1, m->md_w3, m->md_b3, m->md_g4, m->md_be4, m->md_w6, m->md_b6,
                                 w.dense, s));
    OVM_TRY(m, add_bcast(w.dense, m->emb, w.keys, Mi * C, (long)G2 * C, s));
    OVM_HIP(m, hipMemcpyAsync(m->dbg_dense, w.dense + (size_t)(nb - 1) * G2 * C, (size_t)G2 * C * 4, hipMemcpyDeviceToDevice, s));
  } else {
    OVM_TRY(m, bcast(m->src0, w.keys, Mi * C, (long)G2 * C, s));
  }
  m->dbg_dense_mask = pr.mask_in != nullptr; m->dbg_ns = pr.ns(); m->dbg_nt = nt;
  auto norm = [&](const Norm& n, const float* x, long M, float* y) { return ovm_g_layernorm(x, nullptr, (int)M, C, n.g, n.b, kDecEps, y, s); };
  // token -> image attention of one block (also the final one): q += out_proj(attn(q + pe_q, keys + pe_k, keys)), then the norm
  auto tok_to_img = [&](const Attn& a, const Norm& n) -> int {
    OVM_TRY(m, add_bcast(w.q, w.tok0, w.qpe, Mt * C, Mt * C, s));
    OVM_TRY(m, add_bcast(w.keys, m->pe, w.kpe, Mi * C, (long)G2 * C, s));
    OVM_TRY(m, lin(m, a.q, w.qpe, C, Mt, 0, nullptr, 0, w.tq, I, s));
    OVM_TRY(m, lin(m, a.k, w.kpe, C, Mi, 0, nullptr, 0, w.iA, I, s));
    OVM_TRY(m, lin(m, a.v, w.keys, C, Mi, 0, nullptr, 0, w.iB, I, s));
    OVM_TRY(m, token_attention(m, w.tq, w.iA, w.iB, nb, nt, G2, I, w.scores, w.tctx, s));
    OVM_TRY(m, lin(m, a.o, w.tctx, I, Mt, 0, w.q, C, w.tout, C, s));
    return norm(n, w.tout, Mt, w.q);
  };
  for (int l = 0; l < c.dec_depth; ++l) {
    const DecLayer& y = m->layers[l];
    // self attention (layer 0: no positional encoding, and the output REPLACES the tokens)
    const float* qin = w.q;
    if (l > 0) { OVM_TRY(m, add_bcast(w.q, w.tok0, w.qpe, Mt * C, Mt * C, s)); qin = w.qpe; }
    OVM_TRY(m, lin(m, y.self.q, qin, C, Mt, 0, nullptr, 0, w.tq, C, s));
    OVM_TRY(m, lin(m, y.self.k, qin, C, Mt, 0, nullptr, 0, w.tk, C, s));
    OVM_TRY(m, lin(m, y.self.v, w.q, C, Mt, 0, nullptr, 0, w.tv, C, s));
    OVM_TRY(m, token_attention(m, w.tq, w.tk, w.tv, nb, nt, nt, C, w.scores, w.tctx, s));
    OVM_TRY(m, lin(m, y.self.o, w.tctx, C, Mt, 0, l > 0 ? w.q : nullptr, C, w.tout, C, s));
    OVM_TRY(m, norm(y.n1, w.tout, Mt, w.q));
    OVM_TRY(m, tok_to_img(y.t2i, y.n2));
    // MLP
    OVM_TRY(m, lin(m, y.lin1, w.q, C, Mt, 1, nullptr, 0, w.mlp, c.dec_mlp, s));
    OVM_TRY(m, lin(m, y.lin2, w.mlp, c.dec_mlp, Mt, 0, w.q, C, w.tout, C, s));
    OVM_TRY(m, norm(y.n3, w.tout, Mt, w.q));
    // image -> token: the image rows (keys + pe, unchanged since tok_to_img) are the queries
    OVM_TRY(m, add_bcast(w.q, w.tok0, w.qpe, Mt * C, Mt * C, s));
    OVM_TRY(m, lin(m, y.i2t.q, w.kpe, C, Mi, 0, nullptr, 0, w.iA, I, s));
    OVM_TRY(m, lin(m, y.i2t.k, w.qpe, C, Mt, 0, nullptr, 0, w.tk, I, s));
    OVM_TRY(m, lin(m, y.i2t.v, w.q, C, Mt, 0, nullptr, 0, w.tv, I, s));
    if (nt <= kMaxTok) OVM_TRY(m, launch_i2t_attn<kMaxTok>(w.iA, I, w.tk, w.tv, I, nt, c.dec_heads, G2, nb, 0.25f, w.iB, I, s));
    else OVM_TRY(m, launch_i2t_attn<kMaxTok16>(w.iA, I, w.tk, w.tv, I, nt, c.dec_heads, G2, nb, 0.25f, w.iB, I, s));
    OVM_TRY(m, lin(m, y.i2t.o, w.iB, I, Mi, 0, w.keys, C, w.tmp, C, s));
    OVM_TRY(m, norm(y.n4, w.tmp, Mi, w.keys));
  }
  OVM_TRY(m, tok_to_img(m->fin, m->nfin));
  OVM_HIP(m, hipMemcpyAsync(m->dbg_tokens, w.q, (size_t)Mt * C * 4, hipMemcpyDeviceToDevice, s));
  m->dbg_n = nb;
  // 4. upscaling: ConvT . LayerNorm2d . GELU . ConvT . GELU as GEMMs over source pixels (blocked layout: file header)
  const int C4 = C / 4, C8 = C / 8;
  OVM_TRY(m, lin(m, m->up1, w.keys, C, Mi, 0, nullptr, 0, w.tmp, C, s));
  OVM_TRY(m, launch_ln_gelu(w.tmp, Mi * 4, C4, m->upn.g, m->upn.b, kLn2dEps, s));
  OVM_TRY(m, lin(m, m->up2, w.tmp, C4, Mi * 4, 2, nullptr, 0, w.up2, 4 * C8, s));
  // hypernetwork MLPs (every mask token when the low-resolution logits are asked for, else the requested one) and the IoU head.
  // multimask: the planes are mask tokens 1 .. 3 and IoU columns 1 .. 3; single mask: token 0, column 0
  const int K = pr.multimask ? 3 : 1, tk0 = pr.multimask ? 1 : 0;
  const int t_first = lowres ? 0 : tk0 + mask_index, t_last = lowres ? (pr.multimask ? c.num_mask_tokens : 1) : tk0 + mask_index + 1;
  for (int t = t_first; t < t_last; ++t) {
    const PackedLin* hl = &m->hyper[(size_t)t * 3];
    OVM_TRY(m, lin(m, hl[0], w.q + (size_t)(1 + t) * C, nt * C, nb, 1, nullptr, 0, w.h1, C, s));
    OVM_TRY(m, lin(m, hl[1], w.h1, C, nb, 1, nullptr, 0, w.h2, C, s));
    OVM_TRY(m, lin(m, hl[2], w.h2, C, nb, 0, nullptr, 0, w.hyp + (size_t)t * C8, c.num_mask_tokens * C8, s));
  }
  {
    const float* x = w.q; int ldx = nt * C; float* bufs[2] = {w.h1, w.h2};
    for (int i = 0; i < m->n_iou; ++i) {
      const bool last = i + 1 == m->n_iou;
      float* y = last ? w.iouh : bufs[i & 1]; const int ldy = last ? 128 : c.iou_hidden;
      OVM_TRY(m, lin(m, m->iou[i], x, ldx, nb, last ? 0 : 1, nullptr, 0, y, ldy, s));
      x = y; ldx = ldy;
    }
    if (iou) OVM_TRY(m, launch_iou_slice(w.iouh, 128, nb, tk0, K, iou, s));
  }
  // mask product: multimask slice 1:4 into `lowres`, or the requested token alone into the workspace
  const long LL = (long)m->L * m->L;
  float* planes = lowres ? lowres : w.low; const long stride = lowres ? K * LL : LL;
  OVM_TRY(m, launch_mask_prod(w.up2, w.hyp, c.num_mask_tokens * C8, lowres ? tk0 : tk0 + mask_index, lowres ? K : 1, C8, m->G, nb, planes, stride, s));
  // 5. postprocess_masks + threshold (not for the candidates of the automatic generator: they are counted, not written)
  if (!masks) return OVM_OK;
  return launch_mask_out(planes + (lowres ? (size_t)mask_index * LL : 0), stride, m->L, m->S, m->newh, m->neww, m->H, m->W, nb, masks, s);
}

}  // namespace

extern "C" {

const char* ovm_sam_last_error(const OvmSam* m) { return m ? m->err.c_str() : "null handle"; }

int ovm_sam_destroy(OvmSam* m) {
  if (!m) return OVM_OK;
  (void)hipSetDevice(m->device);
  m->tower.destroy();
  m->free_all();
  if (m->rs_tmp) (void)hipFree(m->rs_tmp);
  if (m->tab) (void)hipFree(m->tab);
  delete m;
  return OVM_OK;
}

int ovm_sam_create(const OvmSamConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmSam** out) {
  if (!cfg || !out) return OVM_ERR_INVALID;
  OvmSam* m = new OvmSam();
  *out = m;
  m->cfg = *cfg; m->device = device; m->precision = cfg->precision; m->k_align = 64;
  const OvmSamConfig& c = m->cfg;
  if (c.heads > 0 && c.embed_dim != c.heads * 64) {
    m->err = "unsupported image encoder: head dimension " + std::to_string(c.embed_dim / c.heads) + " (embed_dim " + std::to_string(c.embed_dim) +
             " / " + std::to_string(c.heads) + " heads); the attention kernels take head dimension 64 only (vit_b, vit_l; vit_h has 80)";
    return OVM_ERR_UNSUPPORTED;
  }
  m->C = c.prompt_dim; m->S = c.image_size; m->nt = 1 + c.num_mask_tokens + 2;       // the box route's token count
  if (c.heads < 1 || c.patch != 16 || c.image_size < 16 || c.image_size % 16 != 0 || c.prompt_dim < 64 || c.prompt_dim % 64 != 0 || c.prompt_dim > 256 ||
      c.dec_depth < 1 || c.dec_heads < 1 || c.attn_downsample < 1 || c.prompt_dim % (c.attn_downsample * c.dec_heads) != 0 ||
      c.prompt_dim / c.attn_downsample / c.dec_heads != 16 || 256 % c.dec_heads != 0 || c.num_mask_tokens != 4 || m->nt > kMaxTok || c.iou_depth < 2 ||
      c.iou_depth > 8 || c.iou_hidden < 4 || c.iou_hidden % 4 != 0 || c.dec_mlp % 64 != 0 || (c.precision != 1 && c.precision != 3) || c.max_boxes < 1) {
    m->err = "invalid config (patch 16, image_size % 16, prompt_dim % 64 and <= 256, cross-attention head dimension 16, 4 mask tokens, precision in {1,3}, max_boxes >= 1)";
    return OVM_ERR_INVALID;
  }
  m->G = c.image_size / c.patch; m->G2 = m->G * m->G; m->L = 4 * m->G; m->I = c.prompt_dim / c.attn_downsample;
  if (m->G2 % (256 / c.dec_heads) != 0) { m->err = "invalid config (grid cells must fill whole workgroups of the image -> token kernel)"; return OVM_ERR_INVALID; }
  OVM_HIP(m, hipSetDevice(device));
  {
    TowerConfig t; memset(&t, 0, sizeof(t));
    t.family = FAM_SAM; t.prefix = "image_encoder."; t.precision = c.precision; t.max_batch = 1; t.sam_window = c.window; t.sam_global_mask = c.global_mask;
    t.embed_dim = c.embed_dim; t.depth = c.depth; t.heads = c.heads; t.pos_grid = c.pos_grid; t.canvas = c.image_size;
    for (int i = 0; i < 3; ++i) { t.pixel_mean[i] = c.pixel_mean[i]; t.pixel_std[i] = c.pixel_std[i]; }
    int r = m->tower.configure(t);
    if (!r) r = m->tower.load(weights, n_weights, device);
    if (r) { m->err = std::string("image encoder: ") + m->tower.err; return r; }
  }
  const WeightMap wm(weights, n_weights);
  const int C = m->C, D = c.embed_dim, G = m->G, G2 = m->G2, I = m->I;
  int r;
  // ---- neck: conv1x1 (no bias) . LayerNorm2d . conv3x3 (no bias, pad 1) . LayerNorm2d
  {
    if ((r = pack_conv(m, wm, "image_encoder.neck.0", C, D, 1, BIAS_NONE, &m->neck1))) return r;
    if ((r = load_norm(m, wm, "image_encoder.neck.1", C, &m->nn1))) return r;
    if ((r = pack_conv(m, wm, "image_encoder.neck.2", C, C, 3, BIAS_NONE, &m->neck3))) return r;
    if ((r = load_norm(m, wm, "image_encoder.neck.3", C, &m->nn3))) return r;
    const size_t pp = (size_t)(G + 2) * (G + 2) * C;
    if ((r = m->alloc(&m->pad_hi, pp, true))) return r;
    if (c.precision == 3 && (r = m->alloc(&m->pad_lo, pp, true))) return r;
    if ((r = m->alloc(&m->T1, (size_t)G2 * C))) return r;
    if ((r = m->alloc(&m->T2, (size_t)G2 * C))) return r;
    if ((r = m->alloc(&m->emb, (size_t)G2 * C))) return r;
    if ((r = m->alloc(&m->src0, (size_t)G2 * C))) return r;
    if ((r = m->alloc(&m->pe, (size_t)G2 * C))) return r;
  }
  // ---- prompt encoder (boxes): the Gaussian matrix, the two corner embeddings, no_mask_embed
  {
    if ((r = upload_weight(m, wm, "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (int64_t)2 * (C / 2), &m->gauss))) return r;
    const float *p2, *p3;
    if ((r = find_weight(m, wm, "prompt_encoder.point_embeddings.2.weight", C, &p2))) return r;
    if ((r = find_weight(m, wm, "prompt_encoder.point_embeddings.3.weight", C, &p3))) return r;
    std::vector<float> cr((size_t)2 * C);
    memcpy(cr.data(), p2, (size_t)C * 4); memcpy(cr.data() + C, p3, (size_t)C * 4);
    if ((r = upload_f32(m, cr.data(), cr.size(), &m->corner))) return r;
    if ((r = upload_weight(m, wm, "prompt_encoder.no_mask_embed.weight", C, &m->no_mask))) return r;
    // points and the mask input
    const float *p0, *p1;
    if ((r = find_weight(m, wm, "prompt_encoder.point_embeddings.0.weight", C, &p0))) return r;
    if ((r = find_weight(m, wm, "prompt_encoder.point_embeddings.1.weight", C, &p1))) return r;
    memcpy(cr.data(), p0, (size_t)C * 4); memcpy(cr.data() + C, p1, (size_t)C * 4);
    if ((r = upload_f32(m, cr.data(), cr.size(), &m->point_emb))) return r;
    if ((r = upload_weight(m, wm, "prompt_encoder.not_a_point_embed.weight", C, &m->not_a_point))) return r;
    const std::string Md = "prompt_encoder.mask_downscaling.";
    if ((r = upload_weight(m, wm, Md + "0.weight", 4 * 4, &m->md_w0))) return r;
    if ((r = upload_weight(m, wm, Md + "0.bias", 4, &m->md_b0))) return r;
    if ((r = upload_weight(m, wm, Md + "1.weight", 4, &m->md_g1))) return r;
    if ((r = upload_weight(m, wm, Md + "1.bias", 4, &m->md_be1))) return r;
    if ((r = upload_weight(m, wm, Md + "3.weight", 16 * 16, &m->md_w3))) return r;
    if ((r = upload_weight(m, wm, Md + "3.bias", 16, &m->md_b3))) return r;
    if ((r = upload_weight(m, wm, Md + "4.weight", 16, &m->md_g4))) return r;
    if ((r = upload_weight(m, wm, Md + "4.bias", 16, &m->md_be4))) return r;
    if ((r = upload_weight(m, wm, Md + "6.weight", (int64_t)C * 16, &m->md_w6))) return r;
    if ((r = upload_weight(m, wm, Md + "6.bias", C, &m->md_b6))) return r;
    if ((r = launch_dense_pe(m->gauss, G, C / 2, m->pe, nullptr))) { m->err = "dense positional encoding launch failed"; return r; }
  }
  // ---- mask decoder
  {
    const std::string Dp = "mask_decoder.";
    const float *it, *mt;
    if ((r = find_weight(m, wm, Dp + "iou_token.weight", C, &it))) return r;
    if ((r = find_weight(m, wm, Dp + "mask_tokens.weight", (int64_t)c.num_mask_tokens * C, &mt))) return r;
    std::vector<float> ot((size_t)(1 + c.num_mask_tokens) * C);
    memcpy(ot.data(), it, (size_t)C * 4); memcpy(ot.data() + C, mt, (size_t)c.num_mask_tokens * C * 4);
    if ((r = upload_f32(m, ot.data(), ot.size(), &m->out_tokens))) return r;
    m->layers.resize(c.dec_depth);
    for (int l = 0; l < c.dec_depth; ++l) {
      DecLayer& y = m->layers[l];
      const std::string P = Dp + "transformer.layers." + std::to_string(l) + ".";
      if ((r = pack_attn(m, wm, P + "self_attn", C, C, &y.self))) return r;
      if ((r = pack_attn(m, wm, P + "cross_attn_token_to_image", C, I, &y.t2i))) return r;
      if ((r = pack_attn(m, wm, P + "cross_attn_image_to_token", C, I, &y.i2t))) return r;
      if ((r = pack_linear(m, wm, P + "mlp.lin1", c.dec_mlp, C, &y.lin1))) return r;
      if ((r = pack_linear(m, wm, P + "mlp.lin2", C, c.dec_mlp, &y.lin2))) return r;
      if ((r = load_norm(m, wm, P + "norm1", C, &y.n1))) return r;
      if ((r = load_norm(m, wm, P + "norm2", C, &y.n2))) return r;
      if ((r = load_norm(m, wm, P + "norm3", C, &y.n3))) return r;
      if ((r = load_norm(m, wm, P + "norm4", C, &y.n4))) return r;
    }
    if ((r = pack_attn(m, wm, Dp + "transformer.final_attn_token_to_image", C, I, &m->fin))) return r;
    if ((r = load_norm(m, wm, Dp + "transformer.norm_final_attn", C, &m->nfin))) return r;
    // the upscaling runs as plain linears over the (tap, co) columns (file header): bias tiled over the four taps
    if ((r = pack_convt(m, wm, Dp + "output_upscaling.0", C, C / 4, BIAS_REQUIRED, true, &m->up1))) return r;
    if ((r = load_norm(m, wm, Dp + "output_upscaling.1", C / 4, &m->upn))) return r;
    if ((r = pack_convt(m, wm, Dp + "output_upscaling.3", C / 4, C / 8, BIAS_REQUIRED, true, &m->up2))) return r;
    m->hyper.resize((size_t)c.num_mask_tokens * 3);
    for (int t = 0; t < c.num_mask_tokens; ++t) {
      const std::string P = Dp + "output_hypernetworks_mlps." + std::to_string(t) + ".layers.";
      if ((r = pack_linear(m, wm, P + "0", C, C, &m->hyper[(size_t)t * 3]))) return r;
      if ((r = pack_linear(m, wm, P + "1", C, C, &m->hyper[(size_t)t * 3 + 1]))) return r;
      if ((r = pack_linear(m, wm, P + "2", C / 8, C, &m->hyper[(size_t)t * 3 + 2]))) return r;
    }
    m->n_iou = c.iou_depth;
    for (int i = 0; i < c.iou_depth; ++i) {
      const int in = i == 0 ? C : c.iou_hidden, on = i + 1 == c.iou_depth ? c.num_mask_tokens : c.iou_hidden;
      if ((r = pack_linear(m, wm, Dp + "iou_prediction_head.layers." + std::to_string(i), on, in, &m->iou[i]))) return r;
    }
  }
  if ((r = m->alloc(&m->rs_dst, (size_t)c.image_size * c.image_size * 3))) return r;
  const int ns_max = kMaxPoints + 2, nt_max = 1 + c.num_mask_tokens + ns_max;
  if ((r = m->alloc(&m->dbg_sparse, (size_t)c.max_boxes * ns_max * C, true))) return r;
  if ((r = m->alloc(&m->dbg_tokens, (size_t)c.max_boxes * nt_max * C, true))) return r;
  if ((r = m->alloc(&m->dbg_dense, (size_t)G2 * C, true))) return r;
  m->dbg_nt = m->nt;
  OVM_HIP(m, hipDeviceSynchronize());
  return OVM_OK;
}

int ovm_sam_set_image(OvmSam* m, const OvmImage* image, int32_t flip_bgr, ovm_stream_t stream) {
  if (!m) return OVM_ERR_INVALID;
  m->err.clear();
  if (!m->tower.fam) { m->err = "handle was not created"; return OVM_ERR_INVALID; }
  if (!image || !image->data || image->height < 1 || image->width < 1) { m->err = "null or empty image"; return OVM_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  OVM_HIP(m, hipSetDevice(m->device));
  const OvmSamConfig& c = m->cfg;
  const int H = image->height, W = image->width, S = m->S, G = m->G, G2 = m->G2, C = m->C;
  // ResizeLongestSide.get_preprocess_shape
  const double scale = (double)S / (double)(H > W ? H : W);
  const int newh = (int)((double)H * scale + 0.5), neww = (int)((double)W * scale + 0.5);
  if (newh < 1 || neww < 1 || newh > S || neww > S) { m->err = "image too elongated for ResizeLongestSide"; return OVM_ERR_SHAPE; }
  m->has_image = false;
  const bool need_h = neww != W, need_v = newh != H;
  if (m->tabH != H || m->tabW != W) {
    OVM_HIP(m, hipStreamSynchronize(s));                  // the previous tables may still be in use / in flight
    const int xk = ovm_host_pil_bilinear_coeffs(W, neww, nullptr, nullptr, 0), yk = ovm_host_pil_bilinear_coeffs(H, newh, nullptr, nullptr, 0);
    if (xk < 1 || yk < 1) { m->err = "resize coefficient size query failed"; return OVM_ERR_INVALID; }
    m->xk = xk; m->yk = yk;
    m->off_xc = (size_t)2 * neww; m->off_yb = m->off_xc + (size_t)neww * xk; m->off_yc = m->off_yb + (size_t)2 * newh;
    const size_t n = m->off_yc + (size_t)newh * yk;
    m->tab_host.assign(n, 0);
    if (ovm_host_pil_bilinear_coeffs(W, neww, m->tab_host.data(), m->tab_host.data() + m->off_xc, neww * xk) < 0 ||
        ovm_host_pil_bilinear_coeffs(H, newh, m->tab_host.data() + m->off_yb, m->tab_host.data() + m->off_yc, newh * yk) < 0) {
      m->err = "resize coefficients failed"; return OVM_ERR_INVALID;
    }
    if (n > m->tab_cap) {
      if (m->tab) (void)hipFree(m->tab);
      m->tab = nullptr; m->tab_cap = 0;
      OVM_HIP(m, hipMalloc((void**)&m->tab, n * sizeof(int)));
      m->tab_cap = n;
    }
    OVM_HIP(m, hipMemcpy(m->tab, m->tab_host.data(), n * sizeof(int), hipMemcpyHostToDevice));
    const size_t tmp_need = (size_t)H * neww * 3;
    if (tmp_need > m->rs_tmp_cap) {
      if (m->rs_tmp) (void)hipFree(m->rs_tmp);
      m->rs_tmp = nullptr; m->rs_tmp_cap = 0;
      OVM_HIP(m, hipMalloc((void**)&m->rs_tmp, tmp_need));
      m->rs_tmp_cap = tmp_need;
    }
    m->tabH = H; m->tabW = W;
  }
  {
    const int r = ovm_resize_bilinear_u8(image->data, H, W, 3, image->stride_h, image->stride_w, image->stride_c, newh, neww, need_h ? m->tab : nullptr,
                                         need_h ? m->tab + m->off_xc : nullptr, m->xk, need_v ? m->tab + m->off_yb : nullptr,
                                         need_v ? m->tab + m->off_yc : nullptr, m->yk, m->rs_tmp, m->rs_dst, s);
    if (r) { m->err = "resize failed (an image whose width is not resized must be dense [H][W][3])"; return r; }
  }
  // encoder: (x - mean) / std and the zero padding to S x S happen in the tower's patch gather; a channel flip is a negative stride
  OvmImage net; memset(&net, 0, sizeof(net));
  net.data = m->rs_dst + (flip_bgr ? 2 : 0); net.height = newh; net.width = neww;
  net.stride_c = flip_bgr ? -1 : 1; net.stride_h = (int64_t)3 * neww; net.stride_w = 3;
  net.orig_height = H; net.orig_width = W;
  {
    const int r = tower_forward(&m->tower, &net, s);
    if (r) { m->err = std::string("image encoder: ") + m->tower.err; return r; }
  }
  // neck
  OVM_TRY(m, lin(m, m->neck1, tower_tokens(&m->tower), c.embed_dim, G2, 0, nullptr, 0, m->T1, C, s));
  {
    LnOut o; memset(&o, 0, sizeof(o));
    o.hi = m->pad_hi; o.lo = m->pad_lo; o.ld = C; o.padH = G; o.padW = G;
    OVM_TRY(m, launch_ln_rows(m->T1, C, G2, C, m->nn1.g, m->nn1.b, kLn2dEps, o, s));
    GemmParams q; memset(&q, 0, sizeof(q));
    q.Ahi = m->pad_hi; q.Alo = m->pad_lo; q.Whi = m->neck3.hi; q.Wlo = m->neck3.lo;
    q.M = G2; q.N = C; q.K = 9 * C; q.cH = G; q.cW = G; q.cC = C; q.C = m->T2; q.ldc = C; q.ws_slot = 1;
    OVM_TRY(m, launch_gemm(q, c.precision, EPI_STORE, A_CONV3X3, s));
  }
  OVM_TRY(m, ovm_g_layernorm(m->T2, nullptr, G2, C, m->nn3.g, m->nn3.b, kLn2dEps, m->emb, s));
  OVM_TRY(m, add_bcast(m->emb, m->no_mask, m->src0, (long)G2 * C, C, s));
  m->H = H; m->W = W; m->newh = newh; m->neww = neww; m->has_image = true;
  return OVM_OK;
}

int ovm_sam_predict_boxes_workspace(const OvmSam* m, int32_t n, int64_t* bytes) {
  if (!m || !bytes || n < 0 || !m->tower.fam) return OVM_ERR_INVALID;
  const int nb = n < m->cfg.max_boxes ? n : m->cfg.max_boxes;
  *bytes = (int64_t)carve(nullptr, nullptr, m, nb < 1 ? 1 : nb, m->nt, false);
  return OVM_OK;
}

int ovm_sam_predict_workspace(const OvmSam* m, int32_t n, int32_t n_points, int32_t has_box, int32_t has_mask, int64_t* bytes) {
  if (!m || !bytes || n < 0 || !m->tower.fam) return OVM_ERR_INVALID;
  if (n_points < 0 || n_points > kMaxPoints) return OVM_ERR_SHAPE;
  if (n_points == 0 && !has_box) return OVM_ERR_INVALID;
  const int nb = n < m->cfg.max_boxes ? n : m->cfg.max_boxes;
  *bytes = (int64_t)carve(nullptr, nullptr, m, nb < 1 ? 1 : nb, 1 + m->cfg.num_mask_tokens + n_points + (has_box ? 2 : 1), has_mask != 0);
  return OVM_OK;
}

// the chunk loop of both predict calls; the arguments were checked by the caller
static int run_prompts(OvmSam* m, const Prompt& all, int n, int mask_index, uint8_t* masks, float* iou, float* lowres, void* workspace, int64_t workspace_bytes,
                       hipStream_t s) {
  const int nt = 1 + m->cfg.num_mask_tokens + all.ns(); const bool hm = all.mask_in != nullptr;
  // the largest chunk the workspace holds (the carve is linear in the box count up to the 256-byte rounding of each buffer)
  int nb = n < m->cfg.max_boxes ? n : m->cfg.max_boxes;
  while (nb > 1 && (int64_t)carve(nullptr, nullptr, m, nb, nt, hm) > workspace_bytes) nb = (nb + 1) / 2;
  if ((int64_t)carve(nullptr, nullptr, m, nb, nt, hm) > workspace_bytes) { m->err = "workspace too small for one box (ovm_sam_predict_boxes_workspace)"; return OVM_ERR_CAPACITY; }
  OVM_HIP(m, hipSetDevice(m->device));
  Work w; carve(&w, (char*)workspace, m, nb, nt, hm);
  const size_t HW = (size_t)m->H * m->W, LL = (size_t)m->L * m->L, K = all.multimask ? 3 : 1;
  for (int b0 = 0; b0 < n; b0 += nb) {
    const int cnt = n - b0 < nb ? n - b0 : nb;
    Prompt pr = all;
    if (all.P) { pr.points = all.points + (size_t)b0 * all.P * 2; pr.labels = all.labels + (size_t)b0 * all.P; }
    if (all.boxes) pr.boxes = all.boxes + (size_t)b0 * 4;
    if (all.mask_in) pr.mask_in = all.mask_in + (size_t)b0 * LL;
    const int r = decode_chunk(m, pr, cnt, mask_index, masks + (size_t)b0 * HW, iou ? iou + (size_t)b0 * K : nullptr,
                               lowres ? lowres + (size_t)b0 * K * LL : nullptr, w, s);
    if (r) return r;
  }
  return OVM_OK;
}

int ovm_sam_predict_boxes(OvmSam* m, const float* boxes, int32_t n, int32_t mask_index, uint8_t* masks, float* iou, float* lowres, void* workspace,
                          int64_t workspace_bytes, ovm_stream_t stream) {
  if (!m) return OVM_ERR_INVALID;
  m->err.clear();
  if (!m->tower.fam) { m->err = "handle was not created"; return OVM_ERR_INVALID; }
  if (!m->has_image) { m->err = "ovm_sam_set_image has not been called"; return OVM_ERR_INVALID; }
  if (n < 0 || mask_index < 0 || mask_index > 2) { m->err = "invalid arguments (n >= 0, mask_index 0..2)"; return OVM_ERR_INVALID; }
  if (n == 0) return OVM_OK;
  if (!boxes || !masks || !workspace) { m->err = "null boxes, masks or workspace"; return OVM_ERR_INVALID; }
  if ((uintptr_t)workspace & 255) { m->err = "the workspace must be 256-byte aligned"; return OVM_ERR_INVALID; }
  Prompt pr; pr.boxes = boxes;
  return run_prompts(m, pr, n, mask_index, masks, iou, lowres, workspace, workspace_bytes, (hipStream_t)stream);
}

int ovm_sam_predict(OvmSam* m, const float* points_xy, const int32_t* labels, int32_t n_points, const float* boxes, const float* mask_inputs, int32_t n,
                    int32_t multimask, int32_t mask_index, uint8_t* masks, float* iou, float* lowres, void* workspace, int64_t workspace_bytes,
                    ovm_stream_t stream) {
  if (!m) return OVM_ERR_INVALID;
  m->err.clear();
  if (!m->tower.fam) { m->err = "handle was not created"; return OVM_ERR_INVALID; }
  if (!m->has_image) { m->err = "ovm_sam_set_image has not been called"; return OVM_ERR_INVALID; }
  if (n_points < 0 || n_points > kMaxPoints) { m->err = "at most 8 points per prompt"; return OVM_ERR_SHAPE; }
  if (n_points == 0 && !boxes) { m->err = "a prompt needs points or a box"; return OVM_ERR_INVALID; }
  if (n < 0 || mask_index < 0 || mask_index > (multimask ? 2 : 0)) { m->err = "invalid arguments (n >= 0, mask_index 0..2, 0 without multimask)"; return OVM_ERR_INVALID; }
  if (n == 0) return OVM_OK;
  if ((n_points > 0 && (!points_xy || !labels)) || !masks || !workspace) { m->err = "null points, labels, masks or workspace"; return OVM_ERR_INVALID; }
  if ((uintptr_t)workspace & 255) { m->err = "the workspace must be 256-byte aligned"; return OVM_ERR_INVALID; }
  Prompt pr; pr.points = n_points ? points_xy : nullptr; pr.labels = n_points ? labels : nullptr; pr.P = n_points; pr.boxes = boxes; pr.mask_in = mask_inputs;
  pr.multimask = multimask != 0;
  return run_prompts(m, pr, n, mask_index, masks, iou, lowres, workspace, workspace_bytes, (hipStream_t)stream);
}

int ovm_sam_mask_boxes(const uint8_t* masks, int32_t n, int32_t H, int32_t W, float* boxes_out, int32_t* counts_out, ovm_stream_t stream) {
  if (n < 0 || H < 1 || W < 1) return OVM_ERR_INVALID;
  if (n == 0) return OVM_OK;
  if (!masks || !boxes_out || !counts_out || ((uintptr_t)boxes_out & 15)) return OVM_ERR_INVALID;
  return launch_mask_boxes(masks, n, H, W, boxes_out, counts_out, (hipStream_t)stream);
}

// ---- automatic mask generation (include/ovm3d.h, "Segment Anything, automatic mask generation")
namespace {
struct AutoWork { float* low; float* iou; int* labels; int* stats; int* skip; };

// the prompt workspace of a chunk of nb one-point prompts, then the chunk's low-res logits, IoU rows, labels, statistics, skip words
size_t carve_auto(Work* w, AutoWork* a, char* base, const OvmSam* m, long nb) {
  size_t off = carve(w, base, m, nb, 1 + m->cfg.num_mask_tokens + 2, false);
  auto take = [&](void** p, size_t bytes) { if (a) *p = base + off; off += (bytes + 255) / 256 * 256; };
  AutoWork dummy; AutoWork* x = a ? a : &dummy;
  take((void**)&x->low, (size_t)nb * 3 * m->L * m->L * 4); take((void**)&x->iou, (size_t)nb * 3 * 4); take((void**)&x->labels, (size_t)nb * 4);
  take((void**)&x->stats, (size_t)nb * 3 * kStatsWords * 4); take((void**)&x->skip, (size_t)nb * 3 * 4);
  return off;
}
}  // namespace

int ovm_sam_auto_candidates_workspace(const OvmSam* m, int32_t n, int64_t* bytes) {
  if (!m || !bytes || n < 0 || !m->tower.fam) return OVM_ERR_INVALID;
  const int nb = n < m->cfg.max_boxes ? n : m->cfg.max_boxes;
  *bytes = (int64_t)carve_auto(nullptr, nullptr, nullptr, m, nb < 1 ? 1 : nb);
  return OVM_OK;
}

int ovm_sam_auto_candidates(OvmSam* m, const float* points_xy, int32_t n, float pred_iou_thresh, float offset, OvmSamCandidate* out, void* workspace,
                            int64_t workspace_bytes, ovm_stream_t stream) {
  if (!m) return OVM_ERR_INVALID;
  m->err.clear();
  if (!m->tower.fam) { m->err = "handle was not created"; return OVM_ERR_INVALID; }
  if (!m->has_image) { m->err = "ovm_sam_set_image has not been called"; return OVM_ERR_INVALID; }
  if (n < 0) { m->err = "invalid arguments (n >= 0)"; return OVM_ERR_INVALID; }
  if (n == 0) return OVM_OK;
  if (!points_xy || !out || !workspace) { m->err = "null points, candidates or workspace"; return OVM_ERR_INVALID; }
  if ((uintptr_t)workspace & 255) { m->err = "the workspace must be 256-byte aligned"; return OVM_ERR_INVALID; }
  const long LL = (long)m->L * m->L;
  if (mask_stats_geometry(LL, 3, m->L, m->S, m->newh, m->neww, m->H, m->W)) { m->err = "image or model size outside the mask statistics kernel's range (ovm_op_sam_mask_stats)"; return OVM_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  int nb = n < m->cfg.max_boxes ? n : m->cfg.max_boxes;
  while (nb > 1 && (int64_t)carve_auto(nullptr, nullptr, nullptr, m, nb) > workspace_bytes) nb = (nb + 1) / 2;
  if ((int64_t)carve_auto(nullptr, nullptr, nullptr, m, nb) > workspace_bytes) { m->err = "workspace too small for one point (ovm_sam_auto_candidates_workspace)"; return OVM_ERR_CAPACITY; }
  OVM_HIP(m, hipSetDevice(m->device));
  Work w; AutoWork a; carve_auto(&w, &a, (char*)workspace, m, nb);
  hipLaunchKernelGGL(sam_fill_int_kernel, g1(nb), dim3(256), 0, s, a.labels, 1, nb);
  OVM_TRY(m, last_launch());
  for (int b0 = 0; b0 < n; b0 += nb) {
    const int cnt = n - b0 < nb ? n - b0 : nb, planes = 3 * cnt;
    Prompt pr; pr.points = points_xy + (size_t)b0 * 2; pr.labels = a.labels; pr.P = 1; pr.multimask = true;
    OVM_TRY(m, decode_chunk(m, pr, cnt, 0, nullptr, a.iou, a.low, w, s));
    hipLaunchKernelGGL(sam_auto_skip_kernel, g1(planes), dim3(256), 0, s, (const float*)a.iou, pred_iou_thresh, planes, a.skip);
    OVM_TRY(m, launch_mask_stats(a.low, LL, planes, m->L, m->S, m->newh, m->neww, m->H, m->W, offset, a.skip, a.stats, s));
    hipLaunchKernelGGL(sam_auto_rows_kernel, g1(planes), dim3(256), 0, s, (const float*)a.iou, (const int*)a.stats, (const int*)a.skip, planes, out + (size_t)b0 * 3);
    OVM_TRY(m, last_launch());
  }
  return OVM_OK;
}

int ovm_sam_auto_select_workspace(int32_t m, int64_t* bytes) {
  if (!bytes || m < 0) return OVM_ERR_INVALID;
  const size_t rows = m < 1 ? 1 : (size_t)m;
  *bytes = (int64_t)((rows * 16 + 255) / 256 * 256 + 2 * ((rows * 4 + 255) / 256 * 256));
  return OVM_OK;
}

int ovm_sam_auto_select(const OvmSamCandidate* cands, int32_t m, float pred_iou_thresh, float stability_thresh, float nms_thresh, int32_t* keep_idx,
                        int32_t* n_keep, void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  if (m < 0 || !n_keep) return OVM_ERR_INVALID;
  if (m > 4096) return OVM_ERR_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  if (m == 0) return hipMemsetAsync(n_keep, 0, sizeof(int), s) == hipSuccess ? OVM_OK : OVM_ERR_HIP;
  int64_t need = 0;
  ovm_sam_auto_select_workspace(m, &need);
  if (!cands || !keep_idx || !workspace || ((uintptr_t)workspace & 15)) return OVM_ERR_INVALID;
  if (workspace_bytes < need) return OVM_ERR_CAPACITY;
  char* base = (char*)workspace;
  float* boxes = (float*)base; base += ((size_t)m * 16 + 255) / 256 * 256;
  float* scores = (float*)base; base += ((size_t)m * 4 + 255) / 256 * 256;
  int* valid = (int*)base;
  hipLaunchKernelGGL(sam_auto_valid_kernel, g1(m), dim3(256), 0, s, cands, m, pred_iou_thresh, stability_thresh, boxes, scores, valid);
  if (last_launch()) return OVM_ERR_HIP;
  return launch_nms_single(boxes, scores, valid, m, nms_thresh, keep_idx, n_keep, s);
}

int64_t ovm_sam_debug_copy(OvmSam* m, const char* name, float* dst, int64_t capacity, ovm_stream_t stream) {
  if (!m || !name || !dst || !m->tower.fam) return OVM_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  const int C = m->C, G2 = m->G2;
  const float* src = nullptr; int64_t cnt = 0;
  if (n == "preprocessed") {
    cnt = (int64_t)3 * m->S * m->S;
    if (cnt > capacity) return OVM_ERR_CAPACITY;
    const half_t *hi, *lo; int ld;
    tower_patches(&m->tower, &hi, &lo, &ld);
    return launch_unpatch(hi, lo, ld, m->G, m->cfg.patch, dst, s) ? OVM_ERR_HIP : cnt;
  }
  if (n == "neck") { src = m->emb; cnt = (int64_t)G2 * C; }
  else if (n == "dense_pe") { src = m->pe; cnt = (int64_t)G2 * C; }
  else if (n == "sparse") { src = m->dbg_sparse; cnt = (int64_t)m->dbg_n * m->dbg_ns * C; }
  else if (n == "tokens_out") { src = m->dbg_tokens; cnt = (int64_t)m->dbg_n * m->dbg_nt * C; }
  else if (n == "dense") {
    cnt = (int64_t)G2 * C;
    if (cnt > capacity) return OVM_ERR_CAPACITY;
    if (m->dbg_dense_mask) src = m->dbg_dense;
    else return bcast(m->no_mask, dst, cnt, C, s) ? OVM_ERR_HIP : cnt;
  }
  else return OVM_ERR_INVALID;
  if (cnt > capacity) return OVM_ERR_CAPACITY;
  if (cnt && hipMemcpyAsync(dst, src, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  return cnt;
}

// The kernels of this file one at a time (tests): the arguments are checked, then the engine's own launcher is called. None synchronises.
int ovm_op_sam_dense_pe(const float* gauss, int32_t G, int32_t F, float* pe, ovm_stream_t stream) {
  if (!gauss || !pe || G < 1 || F < 1) return OVM_ERR_INVALID;
  return launch_dense_pe(gauss, G, F, pe, (hipStream_t)stream);
}

int ovm_op_sam_box_tokens(const float* boxes, int32_t nb, int32_t nout, int32_t C, const float* out_tokens, const float* gauss, const float* corner,
                          int32_t H, int32_t W, int32_t newh, int32_t neww, int32_t S, float* tok, float* sparse, ovm_stream_t stream) {
  if (!boxes || !out_tokens || !gauss || !corner || !tok || !sparse || nb < 1 || nout < 0 || H < 1 || W < 1 || newh < 1 || neww < 1 || S < 1) return OVM_ERR_INVALID;
  if (C < 2 || C % 2 != 0) return OVM_ERR_SHAPE;
  return launch_box_tokens(boxes, nb, nout, C, out_tokens, gauss, corner, H, W, newh, neww, S, tok, sparse, (hipStream_t)stream);
}

int ovm_op_sam_ln_gelu(float* x, int64_t M, int32_t D, const float* gamma, const float* beta, float eps, ovm_stream_t stream) {
  if (!x || !gamma || !beta || M < 1) return OVM_ERR_INVALID;
  return launch_ln_gelu(x, (long)M, D, gamma, beta, eps, (hipStream_t)stream);
}

int ovm_op_sam_i2t_attn(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, int32_t nt, int32_t heads, int32_t G2, int32_t nb,
                        float scale, float* o, int32_t ldo, ovm_stream_t stream) {
  if (!q || !k || !v || !o || nb < 1) return OVM_ERR_INVALID;
  if ((((uintptr_t)q) | ((uintptr_t)o)) & 15) return OVM_ERR_INVALID;
  return launch_i2t_attn<kMaxTok>(q, ldq, k, v, ld, nt, heads, G2, nb, scale, o, ldo, (hipStream_t)stream);
}

int ovm_op_sam_i2t_attn16(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, int32_t nt, int32_t heads, int32_t G2, int32_t nb,
                          float scale, float* o, int32_t ldo, ovm_stream_t stream) {
  if (!q || !k || !v || !o || nb < 1) return OVM_ERR_INVALID;
  if ((((uintptr_t)q) | ((uintptr_t)o)) & 15) return OVM_ERR_INVALID;
  return launch_i2t_attn<kMaxTok16>(q, ldq, k, v, ld, nt, heads, G2, nb, scale, o, ldo, (hipStream_t)stream);
}

int ovm_op_sam_point_tokens(const float* points, const int32_t* labels, const float* boxes, int32_t nb, int32_t P, int32_t nout, int32_t C,
                            const float* out_tokens, const float* gauss, const float* point_emb, const float* not_a_point, const float* corner, int32_t H,
                            int32_t W, int32_t newh, int32_t neww, int32_t S, float* tok, float* sparse, ovm_stream_t stream) {
  if (!out_tokens || !gauss || !point_emb || !not_a_point || !corner || !tok || !sparse || nb < 1 || nout < 0 || H < 1 || W < 1 || newh < 1 || neww < 1 || S < 1)
    return OVM_ERR_INVALID;
  if (P < 0 || (P > 0 && (!points || !labels)) || (P == 0 && !boxes)) return OVM_ERR_INVALID;
  if (C < 2 || C % 2 != 0 || P > kMaxPoints) return OVM_ERR_SHAPE;
  return launch_point_tokens(points, labels, boxes, nb, P, nout, C, out_tokens, gauss, point_emb, not_a_point, corner, H, W, newh, neww, S, tok, sparse,
                             (hipStream_t)stream);
}

int ovm_op_sam_mask_embed(const float* mask, int32_t n, int32_t G, int32_t C, const float* w0, const float* b0, const float* g1_, const float* be1,
                          const float* w3, const float* b3, const float* g4, const float* be4, const float* w6, const float* b6, float* out,
                          ovm_stream_t stream) {
  if (!mask || !w0 || !b0 || !g1_ || !be1 || !w3 || !b3 || !g4 || !be4 || !w6 || !b6 || !out || n < 1 || G < 1) return OVM_ERR_INVALID;
  return launch_mask_embed(mask, n, G, C, w0, b0, g1_, be1, w3, b3, g4, be4, w6, b6, out, (hipStream_t)stream);
}

int ovm_op_sam_mask_prod(const float* up, const float* hyper, int32_t ld_hyper, int32_t t0, int32_t ntk, int32_t C8, int32_t G, int32_t nb, float* out,
                         int64_t out_box_stride, ovm_stream_t stream) {
  if (!up || !hyper || !out || G < 1 || nb < 1 || t0 < 0 || ntk < 1) return OVM_ERR_INVALID;
  if (C8 > 0 && ld_hyper < (t0 + ntk) * C8) return OVM_ERR_SHAPE;
  if (out_box_stride < (int64_t)ntk * 16 * G * G) return OVM_ERR_SHAPE;
  return launch_mask_prod(up, hyper, ld_hyper, t0, ntk, C8, G, nb, out, (long)out_box_stride, (hipStream_t)stream);
}

int ovm_op_sam_mask_out(const float* logits, int64_t box_stride, int32_t L, int32_t S, int32_t newh, int32_t neww, int32_t H, int32_t W, int32_t nb,
                        uint8_t* out, ovm_stream_t stream) {
  if (!logits || !out || nb < 1 || L < 1 || H < 1 || W < 1) return OVM_ERR_INVALID;
  if (newh < 1 || neww < 1 || newh > S || neww > S) return OVM_ERR_SHAPE;
  return launch_mask_out(logits, (long)box_stride, L, S, newh, neww, H, W, nb, out, (hipStream_t)stream);
}

int ovm_op_sam_mask_stats(const float* logits, int64_t plane_stride, int32_t planes, int32_t L, int32_t S, int32_t newh, int32_t neww, int32_t H, int32_t W,
                          float offset, const int32_t* skip, int32_t* out, ovm_stream_t stream) {
  if (!logits || !out || planes < 1) return OVM_ERR_INVALID;
  return launch_mask_stats(logits, (long)plane_stride, planes, L, S, newh, neww, H, W, offset, skip, out, (hipStream_t)stream);
}

int ovm_op_sam_unpatch(const uint16_t* hi, const uint16_t* lo, int32_t ld, int32_t G, int32_t P, float* out, ovm_stream_t stream) {
  if (!hi || !out || G < 1 || P < 1) return OVM_ERR_INVALID;
  if (ld < 3 * P * P) return OVM_ERR_SHAPE;
  return launch_unpatch((const half_t*)hi, (const half_t*)lo, ld, G, P, out, (hipStream_t)stream);
}

int ovm_op_sam_iou_slice(const float* head, int32_t ldh, int32_t n, float* iou, ovm_stream_t stream) {
  if (!head || !iou || n < 1) return OVM_ERR_INVALID;
  if (ldh < 4) return OVM_ERR_SHAPE;
  return launch_iou_slice(head, ldh, n, 1, 3, iou, (hipStream_t)stream);
}

int ovm_op_sam_add_bcast(const float* a, const float* b, float* out, int64_t n, int64_t bmod, ovm_stream_t stream) {
  if (!a || !out || n < 1 || bmod < 1) return OVM_ERR_INVALID;
  return b ? add_bcast(a, b, out, (long)n, (long)bmod, (hipStream_t)stream) : bcast(a, out, (long)n, (long)bmod, (hipStream_t)stream);
}

}  // extern "C"
