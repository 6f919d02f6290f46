// Kernel-level C entry points (parity tests / micro-benchmarks): thin adapters that convert fp32 test
// tensors to the split-fp16 layouts and launch the same kernels the model path uses.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/ovm3d.h"
#include "kernels.hpp"
#include "det2d.hpp"
#include "gdino.hpp"
#include "tower.hpp"

using namespace ovm;

namespace {
__global__ void split_kernel(const float* __restrict__ x, int64_t n, half_t* __restrict__ hi, half_t* __restrict__ lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  half_t h, l; split_f16(x[i], h, l);
  hi[i] = h;
  if (lo) lo[i] = l;
}
// qkv [B*T][3D] fp32 (as nn.Linear emits it) -> Q (pre-scaled), K, V^T split layouts of the attention kernel
__global__ void qkv_layout_kernel(const float* __restrict__ qkv, int B, int T, int Tpad, int heads,
                                  half_t* Qh, half_t* Ql, half_t* Kh, half_t* Kl, half_t* Vh, half_t* Vl) {
  const int D = heads * 64;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * T * 3 * D;
  if (i >= total) return;
  const int n = (int)(i % (3 * D)); const int64_t m = i / (3 * D);
  const int b = (int)(m / T), t = (int)(m - (int64_t)b * T);
  const int which = n / D, f = n - which * D, head = f >> 6, d = f & 63;
  float v = qkv[i]; if (which == 0) v *= kQScale;
  half_t h, l; split_f16(v, h, l);
  if (which < 2) {
    const size_t o = ((size_t)(b * heads + head) * T + t) * 64 + d;
    if (which == 0) { Qh[o] = h; if (Ql) Ql[o] = l; } else { Kh[o] = h; if (Kl) Kl[o] = l; }
  } else {
    const int tp = (t & ~15) | (t & 3) | ((t & 4) << 1) | ((t & 8) >> 1);
    const size_t o = ((size_t)(b * heads + head) * 64 + d) * Tpad + tp;
    Vh[o] = h; if (Vl) Vl[o] = l;
  }
}
__global__ void join_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, int64_t n, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = (float)hi[i] + (lo ? (float)lo[i] : 0.f);
}
struct Tmp {
  std::vector<void*> p;
  template <typename Tp> Tp* get(size_t n, bool zero = false) {
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(Tp) + 16) != hipSuccess) return nullptr;
    if (zero) hipMemset(q, 0, n * sizeof(Tp) + 16);
    p.push_back(q);
    return (Tp*)q;
  }
  ~Tmp() { for (void* q : p) hipFree(q); }
};
}  // namespace

namespace ovm { void set_use_gemm256(int v); void set_gdino_branches(int v); void msdeform_set_vec(int v); void set_gdino_dec_chain(int v); void set_gdino_gemm256(int v); void set_gdino_swin_fused(int v); void set_gdino_swin_tap(int v); void set_gdino_ffn_split(int v); void set_gdino_mlp_fused(int v); void set_gdino_enc_fold(int v); void set_gdino_enc_tap(int v); void set_gdino_text_cache(int v); void bump_tune_generation(); void gemm256_set_n192(int v); void set_gemm256_ksplit(int v); }

extern "C" {

int ovm_op_split_f16(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, ovm_stream_t stream) {
  if (n <= 0) return OVM_OK;
  hipLaunchKernelGGL(split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, (half_t*)hi, (half_t*)lo);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

// C[M][N] = A[M][K] W[N][K]^T (+bias)(+relu). W must be padded to a multiple of 128 rows by the caller.
static int g_op_gemm256 = 0;
static unsigned long long* g_gemm256_stamps = nullptr;   // diagnostic: device buffer [8][128] set through ovm_debug_set_ptr

int ovm_op_gemm(const uint16_t* a_hi, const uint16_t* a_lo, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo,
                int32_t M, int32_t N, int32_t K, const float* bias, int32_t relu, float* c, int32_t ldc,
                int32_t precision, ovm_stream_t stream) {
  GemmParams p; memset(&p, 0, sizeof(p));
  p.Ahi = (const half_t*)a_hi; p.Alo = (const half_t*)a_lo; p.lda = lda;
  p.Whi = (const half_t*)w_hi; p.Wlo = (const half_t*)w_lo;
  if (precision == 3) {
    if (w_lo != w_hi + 32) return OVM_ERR_INVALID;            // split weights are an interleaved image (ovm_op_interleave)
    p.a_il = (a_lo == a_hi + 32);                             // activations: either layout
  }
  p.M = M; p.N = N; p.K = K; p.bias = bias; p.relu = relu; p.C = c; p.ldc = ldc;
  if (g_op_gemm256 > 0) {                                     // tests / micro-benchmarks: force the 256 x 256 kernel (value = split-K hint)
    if (!gemm256_supported(p, precision)) return OVM_ERR_INVALID;
    p.stamps = g_gemm256_stamps;
    return launch_gemm256(p, EPI_STORE, g_op_gemm256, (hipStream_t)stream);
  }
  return launch_gemm(p, precision, EPI_STORE, A_ROWMAJOR, (hipStream_t)stream);
}

// w12 of a SwiGLU FFN with silu(gate) * value in the epilogue: out[M][Hs] = silu(A Wg^T + bg) * (A Wu^T + bu) as a split fp16 image
// (see include/ovm3d.h for the row order of the weight image)
int ovm_op_gemm_swiglu(const uint16_t* a_hi, const uint16_t* a_lo, int32_t lda, const uint16_t* w_hi, const uint16_t* w_lo,
                       int32_t M, int32_t Hs, int32_t K, const float* bias, uint16_t* out_hi, uint16_t* out_lo, int32_t ldo,
                       int32_t precision, ovm_stream_t stream) {
  if (!a_hi || !w_hi || !out_hi || Hs < 1 || (precision != 1 && precision != 3)) return OVM_ERR_INVALID;
  const int Kp = (Hs + 31) / 32 * 32;
  GemmParams p; memset(&p, 0, sizeof(p));
  p.Ahi = (const half_t*)a_hi; p.Alo = (const half_t*)a_lo; p.lda = lda;
  p.Whi = (const half_t*)w_hi; p.Wlo = (const half_t*)w_lo;
  if (precision == 3) {
    if (w_lo != w_hi + 32 || !out_lo) return OVM_ERR_INVALID;
    p.a_il = (a_lo == a_hi + 32);
  }
  p.o_il = (out_lo == out_hi + 32);
  if (ldo < (p.o_il ? 2 : 1) * Kp) return OVM_ERR_SHAPE;
  p.M = M; p.N = 2 * Kp; p.K = K; p.bias = bias;
  p.Ohi = (half_t*)out_hi; p.Olo = (half_t*)out_lo; p.ldo = ldo;
  if (g_op_gemm256 > 0) {                                     // forced onto the 256 x 256 kernel (no split-K with this epilogue)
    if (!gemm256_supported(p, precision)) return OVM_ERR_INVALID;
    return launch_gemm256(p, EPI_SWIGLU, 1, (hipStream_t)stream);
  }
  return launch_gemm(p, precision, EPI_SWIGLU, A_ROWMAJOR, (hipStream_t)stream);
}

namespace {
__global__ void interleave_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, long rows, int K, half_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * K) return;
  const long r = i / K; const int k = (int)(i - r * K);
  const size_t o = (size_t)r * 2 * K + (size_t)(k >> 5) * 64 + (k & 31);
  out[o] = hi[i];
  out[o + 32] = lo[i];
}
}  // namespace

namespace {
// un-bordered NHWC fp32 [B][H][W][Cc] -> the interior of a zero-bordered split fp16 image [B][H+2][W+2][Cc] (border: the caller's memset)
__global__ void pad_nhwc_split_kernel(const float* __restrict__ x, int64_t n, int H, int W, int Cc, half_t* __restrict__ hi,
                                      half_t* __restrict__ lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % Cc); const int64_t px = i / Cc;
  const int xx = (int)(px % W); const int64_t t = px / W; const int y = (int)(t % H); const int64_t b = t / H;
  const size_t o = (size_t)(((b * (H + 2) + y + 1) * (W + 2) + xx + 1) * Cc + c);
  half_t h, l; split_f16(x[i], h, l);
  hi[o] = h;
  if (lo) lo[o] = l;
}
inline dim3 grid1d(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
}  // namespace

// Any fused epilogue of gemm.hpp in isolation (tests): fp32 operands in, the kernel's own output layouts out. Converts the operands with
// the kernels above, fills GemmParams and calls the launcher the model path calls; checks nothing the launchers check themselves.
int ovm_op_gemm_epi(const OvmGemmEpiOp* d, ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!d || !d->A || !d->W) return OVM_ERR_INVALID;
  if ((d->precision != 1 && d->precision != 3) || d->M < 1 || d->N < 1 || d->K < 1) return OVM_ERR_INVALID;   // the conversions below need them
  const bool split = d->precision == 3, conv = d->amode == A_CONV3X3, a_il = split && d->a_il;
  if (conv && (d->cH < 1 || d->cW < 1 || d->cC < 1)) return OVM_ERR_INVALID;
  if (d->epi == EPI_QKV && (!d->Q || !d->Kout || !d->Vt || d->T < 1 || d->heads < 1)) return OVM_ERR_INVALID;
  if ((d->epi == EPI_RESID || d->epi == EPI_PATCH) && !d->X) return OVM_ERR_INVALID;
  if (d->epi == EPI_PATCH && !d->pos) return OVM_ERR_INVALID;
  if ((d->epi == EPI_GELU || d->epi == EPI_CONVT) && !d->O) return OVM_ERR_INVALID;
  if (d->O && d->o_elems < 1) return OVM_ERR_INVALID;
  Tmp tmp;
  // ---- A: [M][K] rows, or the zero-bordered image of the un-bordered NHWC input
  const int64_t a_rows = conv ? (int64_t)((d->M + d->cH * d->cW - 1) / (d->cH * d->cW)) * (d->cH + 2) * (d->cW + 2) : d->M;
  const int a_k = conv ? d->cC : d->K;
  if (split && (a_k % 32 != 0 || d->K % 32 != 0)) return OVM_ERR_SHAPE;          // no interleaved image exists (the launchers' K % BK)
  const size_t na = (size_t)a_rows * a_k;
  half_t* ah = tmp.get<half_t>(na, conv);
  half_t* al = split ? tmp.get<half_t>(na, conv) : nullptr;
  if (!ah || (split && !al)) return OVM_ERR_HIP;
  if (conv) {
    const int64_t n = (int64_t)(a_rows / ((d->cH + 2) * (d->cW + 2))) * d->cH * d->cW * d->cC;
    hipLaunchKernelGGL(pad_nhwc_split_kernel, grid1d(n), dim3(256), 0, s, d->A, n, d->cH, d->cW, d->cC, ah, al);
  } else {
    hipLaunchKernelGGL(split_kernel, grid1d((int64_t)na), dim3(256), 0, s, d->A, (int64_t)na, ah, al);
  }
  GemmParams p; memset(&p, 0, sizeof(p));
  p.Ahi = ah; p.Alo = al; p.lda = d->K;
  if (a_il) {
    half_t* ai = tmp.get<half_t>(2 * na);
    if (!ai) return OVM_ERR_HIP;
    hipLaunchKernelGGL(interleave_kernel, grid1d((int64_t)na), dim3(256), 0, s, ah, al, (long)a_rows, a_k, ai);
    p.Ahi = ai; p.Alo = ai + 32; p.lda = 2 * d->K; p.a_il = 1;
  }
  // ---- W: zero rows up to a multiple of 256 (whole tiles of either kernel); split mode: the interleaved image
  const size_t n_pad = ((size_t)d->N + 255) / 256 * 256, nw = n_pad * d->K;
  float* wf = tmp.get<float>(nw, true);
  half_t* wh = tmp.get<half_t>(nw);
  half_t* wl = split ? tmp.get<half_t>(nw) : nullptr;
  if (!wf || !wh || (split && !wl)) return OVM_ERR_HIP;
  if (hipMemcpyAsync(wf, d->W, (size_t)d->N * d->K * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  hipLaunchKernelGGL(split_kernel, grid1d((int64_t)nw), dim3(256), 0, s, wf, (int64_t)nw, wh, wl);
  p.Whi = wh;
  if (split) {
    half_t* wi = tmp.get<half_t>(2 * nw);
    if (!wi) return OVM_ERR_HIP;
    hipLaunchKernelGGL(interleave_kernel, grid1d((int64_t)nw), dim3(256), 0, s, wh, wl, (long)n_pad, d->K, wi);
    p.Whi = wi; p.Wlo = wi + 32;
  }
  p.M = d->M; p.N = d->N; p.K = d->K; p.cH = d->cH; p.cW = d->cW; p.cC = d->cC;
  p.bias = d->bias; p.gamma = d->gamma; p.X = d->X; p.ldx = d->ldx; p.row_map = d->row_map;
  p.C = d->C; p.ldc = d->ldc; p.relu = d->relu; p.R = d->R; p.ldr = d->ldr; p.R2 = d->R2; p.ldr2 = d->ldr2; p.relu_o = d->relu_o;
  p.padH = d->padH; p.padW = d->padW; p.ldo = d->ldo; p.o_il = d->o_il;
  p.T = d->T; p.Tpad = d->Tpad; p.heads = d->heads; p.qscale = d->qscale; p.pos = d->pos; p.G2 = d->G2; p.G = d->G; p.Cout = d->Cout;
  // ---- fp16 outputs: the caller's fp32 buffer (sentinels included) is split before the launch and joined back after it. An
  // interleaved O is converted element by element (its hi and lo columns are separate elements of the caller's image).
  struct Out { float* f; half_t* hi; half_t* lo; int64_t n; } outs[4]; int n_out = 0;
  auto add_out = [&](float* f, int64_t n, bool with_lo) -> Out* {
    Out& o = outs[n_out]; o.f = f; o.n = n;
    o.hi = tmp.get<half_t>((size_t)n); o.lo = with_lo ? tmp.get<half_t>((size_t)n) : nullptr;
    if (!o.hi || (with_lo && !o.lo)) return nullptr;
    hipLaunchKernelGGL(split_kernel, grid1d(n), dim3(256), 0, s, f, n, o.hi, o.lo);
    ++n_out;
    return &o;
  };
  if (d->O) {
    Out* o = add_out(d->O, d->o_elems, split && !d->o_il);
    if (!o) return OVM_ERR_HIP;
    p.Ohi = o->hi; p.Olo = d->o_il ? o->hi + 32 : o->lo;
  }
  if (d->epi == EPI_QKV) {
    const int64_t bh = (int64_t)((d->M + d->T - 1) / d->T) * d->heads, nqk = bh * d->T * 64, nv = bh * 64 * d->Tpad;
    if (nv < 1) return OVM_ERR_INVALID;
    Out* q = add_out(d->Q, nqk, split); Out* k = add_out(d->Kout, nqk, split); Out* v = add_out(d->Vt, nv, split);
    if (!q || !k || !v) return OVM_ERR_HIP;
    p.Qhi = q->hi; p.Qlo = q->lo; p.Khi = k->hi; p.Klo = k->lo; p.Vhi = v->hi; p.Vlo = v->lo;
  }
  const int rc = d->route == 1 ? launch_gemm256(p, d->epi, d->ksplit_hint, s) : launch_gemm(p, d->precision, d->epi, d->amode, s);
  if (rc == OVM_OK)
    for (int i = 0; i < n_out; ++i)
      hipLaunchKernelGGL(join_kernel, grid1d(outs[i].n), dim3(256), 0, s, outs[i].hi, outs[i].lo, outs[i].n, outs[i].f);
  if (hipStreamSynchronize(s) != hipSuccess) return OVM_ERR_HIP;          // the scratch is freed on return
  return rc;
}

// The two launches of the fused MLP route (mlp_fused.hip) on the caller's own buffers (tests): nothing is converted or allocated.
// X != null: the residual stream, updated in place (EPI_RESID, as a Swin block); else Y = sum + b2 (+ R) (EPI_STORE, as the encoder's FFN).
int ovm_op_mlp_fused(const uint16_t* x_il, int32_t ldx, const uint16_t* w1_il, const float* b1, const uint16_t* w2_il, const float* b2,
                     int32_t M, int32_t C, int32_t hidden, int32_t act, float* ws, int64_t ws_bytes, float* X, const float* R, float* Y,
                     ovm_stream_t stream) {
  if (!mlp_fused_supported(M, C, hidden, act, 3) || ws_bytes < 0 || (!X && !Y)) return OVM_ERR_INVALID;
  MlpFusedParams p; memset(&p, 0, sizeof(p));
  p.X = (const half_t*)x_il; p.ldx = ldx; p.W1 = (const half_t*)w1_il; p.b1 = b1; p.W2 = (const half_t*)w2_il;
  p.M = M; p.C = C; p.hidden = hidden; p.act = act; p.part = ws; p.part_cap = (size_t)ws_bytes;
  GemmParams q; memset(&q, 0, sizeof(q));
  q.bias = b2;
  if (X) { q.X = X; q.ldx = C; return launch_mlp_fused(p, q, EPI_RESID, (hipStream_t)stream); }
  q.C = Y; q.ldc = C; q.R = R; q.ldr = C;
  return launch_mlp_fused(p, q, EPI_STORE, (hipStream_t)stream);
}

// hi, lo [rows][K] (K % 32 == 0) -> out [rows][K/32][hi 32 | lo 32], the operand image of the split-mode GEMM
int ovm_op_interleave(const uint16_t* hi, const uint16_t* lo, int64_t rows, int32_t K, uint16_t* out, ovm_stream_t stream) {
  if (rows <= 0) return OVM_OK;
  if (!hi || !lo || !out || K % 32 != 0) return OVM_ERR_INVALID;
  const long n = (long)rows * K;
  hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)hi, (const half_t*)lo,
                     (long)rows, K, (half_t*)out);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

int ovm_op_layernorm(const float* x, int32_t M, int32_t D, const float* gamma, const float* beta, float eps, float* y,
                     ovm_stream_t stream) {
  LnOut o; memset(&o, 0, sizeof(o)); o.f32 = y; o.ldf = D;
  return launch_ln_rows(x, D, M, D, gamma, beta, eps, o, (hipStream_t)stream);
}

// qkv [B*T][3*heads*64] fp32 -> out [B*T][heads*64] fp32 (synchronous helper: allocates scratch)
int ovm_op_attention(const float* qkv, int32_t B, int32_t T, int32_t heads, float* out, int32_t precision, ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int D = heads * 64, Tpad = (T + 63) / 64 * 64;
  const size_t nqk = (size_t)B * T * D, nv = (size_t)B * D * Tpad;
  Tmp tmp;
  half_t *Qh = tmp.get<half_t>(nqk), *Kh = tmp.get<half_t>(nqk), *Vh = tmp.get<half_t>(nv, true), *Oh = tmp.get<half_t>(nqk);
  half_t *Ql = nullptr, *Kl = nullptr, *Vl = nullptr, *Ol = nullptr;
  if (precision == 3) { Ql = tmp.get<half_t>(nqk); Kl = tmp.get<half_t>(nqk); Vl = tmp.get<half_t>(nv, true); Ol = tmp.get<half_t>(nqk); }
  if (!Qh || !Kh || !Vh || !Oh) return OVM_ERR_HIP;
  const int64_t total = (int64_t)B * T * 3 * D;
  hipLaunchKernelGGL(qkv_layout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qkv, B, T, Tpad, heads, Qh, Ql, Kh, Kl, Vh, Vl);
  AttnParams a; memset(&a, 0, sizeof(a));
  a.Qhi = Qh; a.Qlo = Ql; a.Khi = Kh; a.Klo = Kl; a.Vhi = Vh; a.Vlo = Vl; a.Ohi = Oh; a.Olo = Ol; a.ldo = D;
  a.B = B; a.heads = heads; a.T = T; a.Tpad = Tpad;
  a.tail_ws = tmp.get<float>(attn_tail_ws_floats(B, heads)); a.tail_cnt = tmp.get<int>((size_t)B * heads * 8, true);
  if (!a.tail_ws || !a.tail_cnt) return OVM_ERR_HIP;
  int r = launch_attention(a, precision, s);
  if (r) return r;
  hipLaunchKernelGGL(join_kernel, dim3((unsigned)((nqk + 255) / 256)), dim3(256), 0, s, Oh, Ol, (int64_t)nqk, out);
  if (hipStreamSynchronize(s) != hipSuccess) return OVM_ERR_HIP;
  return OVM_OK;
}

int ovm_op_roi_align(const float* p2, const float* p3, const float* p4, const int32_t* hw, const float* scales, int32_t C,
                     int32_t out_res, int32_t min_level, int32_t max_level, const float* boxes, const int32_t* image_idx,
                     int32_t n, float* out, ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return OVM_OK;
  Tmp tmp;
  const size_t ne = (size_t)n * out_res * out_res * C;
  half_t *hi = tmp.get<half_t>(ne), *lo = tmp.get<half_t>(ne);
  if (!hi || !lo) return OVM_ERR_HIP;
  RoiParams rp; memset(&rp, 0, sizeof(rp));
  const float* f[3] = {p2, p3, p4};
  int nl = 0;
  for (int i = 0; i < 3; ++i) if (f[i]) { rp.feat[nl] = f[i]; rp.fh[nl] = hw[2 * i]; rp.fw[nl] = hw[2 * i + 1]; rp.scale[nl] = scales[i]; ++nl; }
  rp.C = C; rp.nlevels = nl; rp.min_level = min_level; rp.max_level = max_level; rp.out = out_res;
  rp.boxes = boxes; rp.batch_idx = image_idx; rp.n = n; rp.Ohi = hi; rp.Olo = lo; rp.ldo = out_res * out_res * C;
  int r = launch_roi_align(rp, s);
  if (r) return r;
  hipLaunchKernelGGL(join_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, hi, lo, (int64_t)ne, out);
  if (hipStreamSynchronize(s) != hipSuccess) return OVM_ERR_HIP;
  return OVM_OK;
}

int ovm_op_cube_decode(const float* head13, int32_t ld, const float* boxes, const float* scores, const int32_t* classes,
                       const int32_t* image_idx, const OvmImage* images, int32_t B, int32_t n, float virtual_focal,
                       int32_t postprocess, OvmDet3D* rec, int32_t* keep, ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n <= 0) return OVM_OK;
  std::vector<ImageMeta> hm(B);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < 9; ++i) hm[b].K[i] = images[b].K[i];
    hm[b].ratio = (float)((double)images[b].orig_height / (double)images[b].height);
    hm[b].net_h = images[b].height; hm[b].net_w = images[b].width;
    hm[b].orig_h = images[b].orig_height; hm[b].orig_w = images[b].orig_width;
  }
  Tmp tmp;
  ImageMeta* dm = tmp.get<ImageMeta>(B);
  if (!dm) return OVM_ERR_HIP;
  if (hipMemcpy(dm, hm.data(), sizeof(ImageMeta) * B, hipMemcpyHostToDevice) != hipSuccess) return OVM_ERR_HIP;
  CubeDecodeParams cp; memset(&cp, 0, sizeof(cp));
  cp.head = head13; cp.ldh = ld; cp.boxes = boxes; cp.scores = scores; cp.classes = classes; cp.batch_idx = image_idx;
  cp.meta = dm; cp.n = n; cp.virtual_focal = virtual_focal; cp.rec = (float*)rec; cp.keep = keep; cp.postprocess = postprocess;
  int r = launch_cube_decode(cp, s);
  if (r) return r;
  if (hipStreamSynchronize(s) != hipSuccess) return OVM_ERR_HIP;
  return OVM_OK;
}

// ---- the kernels between the GEMMs, one launcher each (tests): the caller's buffers are the kernel's own, nothing is converted
int ovm_op_roi_align_ex(const float* const* feats, int32_t nlevels, const int32_t* hw, const float* scales, int32_t C, int32_t out_res,
                        int32_t min_level, int32_t max_level, const float* boxes, const int32_t* image_idx, int32_t n,
                        uint16_t* hi, uint16_t* lo, int32_t ldo, ovm_stream_t stream) {
  if (!feats || !hw || !scales || nlevels < 1 || nlevels > kMaxLevels) return OVM_ERR_INVALID;
  RoiParams rp; memset(&rp, 0, sizeof(rp));
  for (int l = 0; l < nlevels; ++l) { rp.feat[l] = feats[l]; rp.fh[l] = hw[2 * l]; rp.fw[l] = hw[2 * l + 1]; rp.scale[l] = scales[l]; }
  rp.C = C; rp.nlevels = nlevels; rp.min_level = min_level; rp.max_level = max_level; rp.out = out_res;
  rp.boxes = boxes; rp.batch_idx = image_idx; rp.n = n; rp.Ohi = (half_t*)hi; rp.Olo = (half_t*)lo; rp.ldo = ldo;
  return launch_roi_align(rp, (hipStream_t)stream);
}

int ovm_op_compact_records(const OvmDet3D* rec, const int32_t* keep, int32_t n, int32_t B, OvmDet3D* out, int32_t* counts,
                           ovm_stream_t stream) {
  return launch_compact_records((const float*)rec, keep, n, B, (float*)out, counts, (hipStream_t)stream);
}

int ovm_op_ln_rows(const float* x, int32_t ldx, int32_t M, int32_t D, const float* gamma, const float* beta, float eps, float* y,
                   int32_t ldf, uint16_t* hi, uint16_t* lo, int32_t ld, int32_t padH, int32_t padW, int32_t il, ovm_stream_t stream) {
  LnOut o; memset(&o, 0, sizeof(o));
  o.hi = (half_t*)hi; o.lo = (half_t*)lo; o.ld = ld; o.f32 = y; o.ldf = ldf; o.padH = padH; o.padW = padW; o.il = il;
  return launch_ln_rows(x, ldx, M, D, gamma, beta, eps, o, (hipStream_t)stream);
}

int ovm_op_ln_gelu_split(uint16_t* hi, uint16_t* lo, int32_t M, int32_t D, const float* gamma, const float* beta, float eps,
                         ovm_stream_t stream) {
  return launch_ln_gelu_split((half_t*)hi, (half_t*)lo, M, D, gamma, beta, eps, (hipStream_t)stream);
}

int ovm_op_patch_gather(const OvmImage* images, int32_t B, int32_t G, int32_t patch, int32_t Kpad, const float* mean, const float* std,
                        uint16_t* hi, uint16_t* lo, ovm_stream_t stream) {
  if (!images || !mean || !std || B < 1) return OVM_ERR_INVALID;
  std::vector<ImageDesc> hd(B);
  for (int b = 0; b < B; ++b)
    hd[b] = ImageDesc{images[b].data, images[b].height, images[b].width, images[b].stride_c, images[b].stride_h, images[b].stride_w};
  Tmp tmp;
  ImageDesc* dd = tmp.get<ImageDesc>(B);
  if (!dd || hipMemcpy(dd, hd.data(), sizeof(ImageDesc) * B, hipMemcpyHostToDevice) != hipSuccess) return OVM_ERR_HIP;
  const int r = launch_patch_gather(dd, B, G, patch, Kpad, mean, std, (half_t*)hi, (half_t*)lo, (hipStream_t)stream);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && !r) return OVM_ERR_HIP;      // the descriptors are freed on return
  return r;
}

int ovm_op_patch_gather_f32(const int64_t* views, int32_t B, int32_t G, int32_t Kpad, uint16_t* hi, uint16_t* lo, ovm_stream_t stream) {
  if (!views || B < 1 || B > kMaxTowerViews) return OVM_ERR_INVALID;
  TowerViews v; memset(&v, 0, sizeof(v));
  v.n = B;
  for (int b = 0; b < B; ++b) v.v[b] = TowerView{(const float*)(uintptr_t)views[4 * b], views[4 * b + 1], views[4 * b + 2], views[4 * b + 3]};
  return launch_patch_gather_f32(v, B, G, Kpad, (half_t*)hi, (half_t*)lo, (hipStream_t)stream);
}

int ovm_op_cls_init(float* X, const float* cls, const float* pos, const float* reg, int32_t R, int32_t B, int32_t T, int32_t D,
                    ovm_stream_t stream) {
  return launch_cls_init(X, cls, pos, reg, R, B, T, D, (hipStream_t)stream);
}

int ovm_op_tokens_cast(const float* X, int32_t B, int32_t T, int32_t G2, int32_t D, int32_t ldo, const float* depth_tok, uint16_t* hi,
                       uint16_t* lo, ovm_stream_t stream) {
  return launch_tokens_cast(X, B, T, G2, D, ldo, depth_tok, (half_t*)hi, (half_t*)lo, (hipStream_t)stream);
}

int ovm_op_tokens_writeback(float* X, const float* F, int32_t B, int32_t T, int32_t G2, int32_t D, ovm_stream_t stream) {
  return launch_tokens_writeback(X, F, B, T, G2, D, (hipStream_t)stream);
}

int ovm_op_maxpool2(const uint16_t* in_hi, const uint16_t* in_lo, int32_t B, int32_t G, int32_t D, uint16_t* out_hi, uint16_t* out_lo,
                    ovm_stream_t stream) {
  return launch_maxpool2((const half_t*)in_hi, (const half_t*)in_lo, B, G, D, (half_t*)out_hi, (half_t*)out_lo, (hipStream_t)stream);
}

// Tuning knobs for experiments (not part of the stable surface): "gemm_bm" = 0 (heuristic) | 128 | 256.
int ovm_tune_set(const char* key, int32_t value) {
  if (!key) return OVM_ERR_INVALID;
  ovm::bump_tune_generation();                    // caption entries of the detector made so far serve no forward issued from here on (gdino_model.hpp)
  if (!strcmp(key, "gemm_bm")) { gemm_set_force_bm(value); return OVM_OK; }
  if (!strcmp(key, "gemm_stages")) { gemm_set_stages(value); return OVM_OK; }
  if (!strcmp(key, "gemm_splitk")) { gemm_set_splitk(value); return OVM_OK; }
  if (!strcmp(key, "gemm_tail")) { gemm_set_tail_rows(value); return OVM_OK; }
  if (!strcmp(key, "attn_waves")) { attn_set_waves(value); return OVM_OK; }
  if (!strcmp(key, "attn_pp")) {
#ifndef OVM_DIAG
    if (value < 0 || value > 1) return OVM_ERR_INVALID;    // 2 / 3 select timing-only ablations with wrong results: -DOVM_DIAG builds only
#endif
    attn_set_pp(value); return OVM_OK;
  }
  // the gdino_* keys below are copied into a detector plan when it is built (GdinoTune, gdino_model.hpp): a plan keeps its values
  if (!strcmp(key, "gdino_mlp_fused")) { ovm::set_gdino_mlp_fused(value); return OVM_OK; }   // plans built afterwards: 0 = fc1 and fc2 as two GEMMs, 1 = Swin blocks fused, 2 = and the encoder's FFN
  if (!strcmp(key, "gdino_enc_fold")) { ovm::set_gdino_enc_fold(value); return OVM_OK; }     // plans built afterwards: 0 = off, 1 = offsets term folded + no split passes, 2 / 3 = either half
  if (!strcmp(key, "gdino_enc_tap")) { ovm::set_gdino_enc_tap(value); return OVM_OK; }        // tests; plans built afterwards
  if (!strcmp(key, "gdino_text_cache")) { ovm::set_gdino_text_cache(value); return OVM_OK; }  // plans built afterwards: n > 0 = captions encoded once, the handle keeps n; 0 = inside every forward
  if (!strcmp(key, "gdino_ffn_split")) { ovm::set_gdino_ffn_split(value); return OVM_OK; }   // plans built afterwards: 0 = one workgroup per row block runs the whole FFN
  if (!strcmp(key, "gdino_swin_tap")) { ovm::set_gdino_swin_tap(value); return OVM_OK; }      // tests; plans built afterwards
  if (!strcmp(key, "gdino_swin_fused")) { ovm::set_gdino_swin_fused(value); return OVM_OK; }  // plans built afterwards: 0 = qkv GEMM + window attention as two launches
  if (!strcmp(key, "gdino_gemm256")) { ovm::set_gdino_gemm256(value); return OVM_OK; }       // plans built afterwards: 0 = planar rows, 128 x 128 tiles
  if (!strcmp(key, "gdino_dec_chain")) { ovm::set_gdino_dec_chain(value); return OVM_OK; }   // plans built afterwards: 0 = one launch per decoder op
  if (!strcmp(key, "msdeform_vec")) { msdeform_set_vec(value); return OVM_OK; }
  if (!strcmp(key, "attn_q64")) { attn_set_q64(value); return OVM_OK; }      // 0: the 8-wave x 32-query attention kernel of rounds 1-2
  if (!strcmp(key, "attn_prio")) { attn_set_prio(value); return OVM_OK; }
  if (!strcmp(key, "attn_lds_pad")) { attn_set_lds_pad(value); return OVM_OK; }
  if (!strcmp(key, "attn_tail")) { attn_set_tail_rows(value); return OVM_OK; }
  if (!strcmp(key, "attn_tail_split")) { attn_set_tail_split(value); return OVM_OK; }
  if (!strcmp(key, "glin_small_max_tiles")) { glinear_set_small_max_tiles(value); return OVM_OK; }
  if (!strcmp(key, "glin_target_blocks")) { gemm_small_set(value, -1); return OVM_OK; }
  if (!strcmp(key, "gbmm_tiled")) { gbmm_set_tiled(value); return OVM_OK; }
  if (!strcmp(key, "glin_stages")) { gemm_small_set_stages(value); return OVM_OK; }
  if (!strcmp(key, "glin_wpe")) { gemm_small_set_wpe(value); return OVM_OK; }
  if (!strcmp(key, "glin_max_ksplit")) { gemm_small_set(-1, value); return OVM_OK; }
  if (!strcmp(key, "gemm256_ksplit")) { ovm::set_gemm256_ksplit(value); return OVM_OK; }
  if (!strcmp(key, "gemm256_n192")) { ovm::gemm256_set_n192(value); return OVM_OK; }     // qkv: 256 x 192 tiles when they fill the chip better (default 1)
  if (!strcmp(key, "gemm256")) { ovm::set_use_gemm256(value); return OVM_OK; }          // engine: 256 x 256 kernel for qkv / fc1 (default 1)
  if (!strcmp(key, "op_gemm256")) { g_op_gemm256 = value; return OVM_OK; }              // ovm_op_gemm: force it, value = split-K hint
  if (!strcmp(key, "gdino_branches")) { ovm::set_gdino_branches(value); return OVM_OK; }  // engines created afterwards: text branch on its own stream (default 1)
  return OVM_ERR_INVALID;
}

/* diagnostics: hands a device pointer to a named debug hook ("gemm256_stamps": u64 [8][128], NULL switches it off) */
int ovm_debug_set_ptr(const char* key, void* ptr) {
  if (key && !strcmp(key, "gemm256_stamps")) { g_gemm256_stamps = (unsigned long long*)ptr; return OVM_OK; }
#ifdef OVM_DIAG
  if (key && !strcmp(key, "attn_stamps")) { attn_set_stamps((unsigned long long*)ptr); return OVM_OK; }
#else
  if (key && !strcmp(key, "attn_stamps")) return OVM_ERR_UNSUPPORTED;      // stamp / ablation kernels exist in -DOVM_DIAG builds only (OVM_DIAG=1 csrc/build.sh)
#endif
  return OVM_ERR_INVALID;
}

int ovm_op_nms(const float* boxes, const float* scores, int32_t n, float thresh, int32_t* keep_idx, int32_t* n_keep,
               ovm_stream_t stream) {
  return launch_nms_single(boxes, scores, nullptr, n, thresh, keep_idx, n_keep, (hipStream_t)stream);
}

namespace {
// the clip sizes of `images` as a device-resident ImageMeta array (only net_h / net_w are read by the detection stages)
ImageMeta* upload_clip_meta(Tmp& tmp, const OvmImage* images, int B) {
  std::vector<ImageMeta> hm(B);
  memset(hm.data(), 0, sizeof(ImageMeta) * B);
  for (int b = 0; b < B; ++b) { hm[b].net_h = images[b].height; hm[b].net_w = images[b].width; }
  ImageMeta* dm = tmp.get<ImageMeta>(B);
  if (dm && hipMemcpy(dm, hm.data(), sizeof(ImageMeta) * B, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return dm;
}
}  // namespace

int ovm_op_rpn_proposals(const float* const* levels_o, int32_t nlev, const int32_t* sides, const float* strides,
                         const float* anchor_sizes, const float* anchor_ratios, const OvmImage* images, int32_t B,
                         int32_t pre_topk, int32_t post_topk, float nms_thresh, float* prop_boxes, float* prop_scores,
                         int32_t* prop_count, ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!levels_o || !sides || !strides || !anchor_sizes || !anchor_ratios || !images || !prop_boxes || !prop_scores || !prop_count ||
      B < 1 || pre_topk < 1 || post_topk < 1)
    return OVM_ERR_INVALID;
  if (nlev < 1 || nlev > kMaxLevels) return OVM_ERR_INVALID;
  for (int l = 0; l < nlev; ++l) if (!levels_o[l] || sides[l] < 1) return OVM_ERR_INVALID;
  Tmp tmp;                                       // frees the scratch on every exit path
  Det2dWorkspace w;
  int r = det2d_alloc(&w, B, nlev, sides, 0, 1, post_topk, pre_topk, post_topk, 1, &tmp.p);
  if (r) return r;
  Det2dModel m; memset(&m, 0, sizeof(m));
  m.B = B; m.nlev = nlev; m.num_classes = 1; m.pre_topk = pre_topk; m.post_topk = post_topk; m.rpn_nms = nms_thresh;
  for (int l = 0; l < nlev; ++l) { m.stride[l] = strides[l]; m.anchor_sizes[l] = anchor_sizes[l]; w.rpn_o[l] = const_cast<float*>(levels_o[l]); }
  for (int a = 0; a < 3; ++a) m.anchor_ratios[a] = anchor_ratios[a];
  if (!(m.meta = upload_clip_meta(tmp, images, B))) return OVM_ERR_HIP;
  w.prop_boxes = prop_boxes; w.prop_scores = prop_scores; w.prop_count = prop_count;
  r = det2d_rpn_proposals(m, w, s);
  if (hipStreamSynchronize(s) != hipSuccess && !r) r = OVM_ERR_HIP;
  return r;
}

int ovm_op_boxhead_post(const float* HO, int32_t ldh, const float* prop_boxes, const int32_t* prop_count, const OvmImage* images,
                        int32_t B, int32_t R, int32_t K, float score_thresh, float nms_thresh, int32_t topk, float* boxes,
                        float* scores, int32_t* classes, int32_t* image_idx, float* scores_full, int32_t* out_counts,
                        ovm_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!HO || !prop_boxes || !prop_count || !images || !boxes || !scores || !classes || !image_idx || !out_counts || B < 1 || R < 1 ||
      K < 1 || topk < 1 || ldh < 5 * (int64_t)K + 1)
    return OVM_ERR_INVALID;
  Tmp tmp;
  Det2dWorkspace w;
  const int side = 1;
  int r = det2d_alloc(&w, B, 1, &side, 0, K, R, 1, R, topk, &tmp.p);
  if (r) return r;
  Det2dModel m; memset(&m, 0, sizeof(m));
  m.B = B; m.nlev = 1; m.num_classes = K; m.pre_topk = 1; m.score_thresh = score_thresh; m.nms_thresh = nms_thresh; m.topk = topk;
  if (!(m.meta = upload_clip_meta(tmp, images, B))) return OVM_ERR_HIP;
  w.prop_boxes = const_cast<float*>(prop_boxes); w.prop_count = const_cast<int*>(prop_count);
  r = det2d_boxhead_post(m, w, HO, ldh, boxes, scores, classes, image_idx, scores_full, out_counts, s);
  if (hipStreamSynchronize(s) != hipSuccess && !r) r = OVM_ERR_HIP;
  return r;
}

int ovm_gdino_postprocess(const float* pred_logits, int32_t nq, int32_t ld, const float* pred_boxes, const int32_t* spans, int32_t n_phrases,
                          int32_t img_h, int32_t img_w, float box_threshold, float nms_threshold, float* out_boxes, float* out_scores,
                          int32_t* out_classes, int32_t* n_out, ovm_stream_t stream) {
  return launch_gdino_post(pred_logits, nq, ld, pred_boxes, spans, n_phrases, img_h, img_w, box_threshold, nms_threshold, out_boxes,
                           out_scores, out_classes, n_out, (hipStream_t)stream);
}

}  // extern "C"
