// The ViT tower (tower.hpp): the checkpoint-family table, loading, workspace, the block launches, and the GEMM dispatcher it shares with
// the pyramid and heads of api.hip.
#include "tower.hpp"

#include <cmath>
#include <cstring>
#include <string>

#include "gdino.hpp"

namespace ovm {

// One row per checkpoint dialect; Tower::load reads the row, nothing else names a family's keys.
const FamilyRow kFamilies[FAM_COUNT] = {
    // FAM_DINOV2_HUB
    {14, 640, 1e-6f, 0, true, "backbone.net.vit.", "blocks.", "norm1", "norm2", "ls1.gamma", "ls2.gamma", QKV_FUSED, "attn.qkv", "attn.proj", "mlp.fc1",
     "mlp.fc2", "patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed", POS_HUB, nullptr, nullptr, false, true},
    // FAM_DINOV2_HF: Dinov2Embeddings, Dinov2Layer, the model's final layernorm; patch 16, table at the canvas grid
    {16, 768, 1e-6f, 0, true, "", "encoder.layer.", "norm1", "norm2", "layer_scale1.lambda1", "layer_scale2.lambda1", QKV_TRIPLE, "attention.attention.",
     "attention.output.dense", "mlp.fc1", "mlp.fc2", "embeddings.patch_embeddings.projection.weight", "embeddings.patch_embeddings.projection.bias",
     "embeddings.cls_token", "embeddings.position_embeddings", POS_STORED, nullptr, "layernorm", false, false},
    // FAM_OPEN_CLIP: ResidualAttentionBlock (ln_1, nn.MultiheadAttention, ln_2, mlp with QuickGELU); conv1 has no bias; x = ln_pre(x + pos)
    {16, 768, 1e-5f, 3, true, "backbone.net.visual.", "transformer.resblocks.", "ln_1", "ln_2", nullptr, nullptr, QKV_BARE, "attn.in_proj_", "attn.out_proj",
     "mlp.c_fc", "mlp.c_proj", "conv1.weight", nullptr, "class_embedding", "positional_embedding", POS_AA, "ln_pre", nullptr, false, false},
    // FAM_HF_VITMAE: ViTLayer (layernorm_before, attention, layernorm_after, intermediate / output); position table rebuilt for the grid (mae.py:62-78)
    {16, 768, 1e-12f, 0, true, "backbone.net.vit.", "encoder.layer.", "layernorm_before", "layernorm_after", nullptr, nullptr, QKV_TRIPLE, "attention.attention.",
     "attention.output.dense", "intermediate.dense", "output.dense", "embeddings.patch_embeddings.projection.weight",
     "embeddings.patch_embeddings.projection.bias", "embeddings.cls_token", nullptr, POS_SINCOS, nullptr, nullptr, false, false},
    // FAM_TIMM: Block with init_values=None (no LayerScale); table resized with the CLIP tower's antialiased bicubic (midas_final.py:64-66)
    {16, 768, 1e-6f, 0, true, "backbone.net.vit.", "blocks.", "norm1", "norm2", nullptr, nullptr, QKV_FUSED, "attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2",
     "patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed", POS_AA, nullptr, nullptr, false, false},
    // FAM_SAM: Block (norm1, attn with rel_pos_h / _w, norm2, mlp lin1 / lin2); no class token, table [grid][grid][D], plain bicubic (sam.py:73-86)
    {16, 768, 1e-6f, 0, false, "backbone.net.vit.", "blocks.", "norm1", "norm2", nullptr, nullptr, QKV_FUSED, "attn.qkv", "attn.proj", "mlp.lin1", "mlp.lin2",
     "patch_embed.proj.weight", "patch_embed.proj.bias", nullptr, "pos_embed", POS_GRID, nullptr, nullptr, true, false},
};

// ---- GEMM dispatcher -------------------------------------------------------------------------------------------------------------
static int g_use_gemm256 = 1;     // ovm_tune_set("gemm256", 0 | 1)
static int g_gemm256_ksplit = 0;  // ovm_tune_set("gemm256_ksplit", n)
void set_use_gemm256(int v) { g_use_gemm256 = v; }
void set_gemm256_ksplit(int v) { g_gemm256_ksplit = v; }

ProfScope::ProfScope(const GemmCtx& c, int cat, hipStream_t s_) : s(s_) {
  Prof* p = c.prof;
  if (!p || !p->on || cat < 0 || !((p->mask >> cat) & 1u)) return;
  auto& pool = p->ev[cat];
  if (p->used[cat] == pool.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    pool.push_back({a, b});
  }
  auto& pr = pool[p->used[cat]++];
  (void)hipEventRecord(pr.first, s);
  stop = pr.second;
}

int gemm(const GemmCtx& c, const GemmParams& p_in, int epi, int amode, hipStream_t s, int cat) {
  ProfScope ps(c, cat, s);
  GemmParams p = p_in;
  if (!p.part_ws && c.splitk_ws) { p.part_ws = c.splitk_ws; p.part_cap = c.splitk_cap; }
  // the large block contractions (qkv, fc1: >= 2048 rows and >= 3072 columns -> at least 192 tiles of 256 x 256) go to the
  // two-wave-group 256 x 256 kernel; everything else keeps the 128 x 128 kernels
  // (at batch >= 4 the N = D contractions - proj, fc2 - reach that tile count too: 128 x 128 tiles fetch twice the operand bytes
  // per MFMA from L2, which is what bounds them at batch 1, where only 128-wide tiles fill the chip)
  if (g_use_gemm256 && amode == A_ROWMAJOR && gemm256_supported(p, c.precision) &&
      (long)((p.M + 255) / 256) * (p.N / 256) >= 192 &&
      (epi == EPI_STORE || epi == EPI_RESID || epi == EPI_GELU || epi == EPI_QKV || epi == EPI_SWIGLU))   // w12 of ViT-g: N = 8192, 192 tiles from T = 1281
    return launch_gemm256(p, epi, 1, s);
  // experiment knob (ovm_tune_set "gemm256_ksplit"): the long-K contractions with too few 256-wide tiles (fc2 at batch 1: 64 tiles,
  // K = 4096) as k-slices of 256 x 256 tiles + a reduce pass - half the operand fetch of 128 x 128 tiles
  if (g_gemm256_ksplit > 1 && amode == A_ROWMAJOR && gemm256_supported(p, c.precision) && epi == EPI_RESID && p.K >= 2048 && !p.row_map)
    return launch_gemm256(p, epi, g_gemm256_ksplit, s);
  return launch_gemm(p, c.precision, epi, amode, s);
}

GemmParams gp_base(const SplitImg& A, int lda, const PackedLin& W, int M) {
  GemmParams p; memset(&p, 0, sizeof(p));
  p.Ahi = A.hi; p.Alo = A.lo; p.lda = lda;
  p.Whi = W.hi; p.Wlo = W.lo;
  p.M = M; p.N = W.N; p.K = W.Kpad; p.bias = W.bias;
  return p;
}

// il: interleaved split image [rows][K/32][hi 32 | lo 32] (f16x3 mode; plain fp16 rows in one-pass mode): the A-operand layout of the
// 256 x 256 GEMM (one 128-byte LDS-DMA line per row and k-group holds both parts)
int salloc(Loader* L, SplitImg* s, size_t count, bool zero, bool il) {
  const bool split = L->precision == 3;
  s->lo = nullptr;
  const int r = L->alloc(&s->hi, il && split ? 2 * count : count, zero);
  if (r || !split) return r;
  if (il) { s->lo = s->hi + 32; return OVM_OK; }
  return L->alloc(&s->lo, count, zero);
}

// ---- host position-table helpers -------------------------------------------------------------------------------------------------
// F.interpolate(src[1,D,M,M], size=(G,G), mode="bicubic", align_corners=False) on a channels-last table [M*M][D] -> [G*G][D]
// (A = -0.75, border indices clamped, x pass then y as upsample_bicubic2d evaluates it); scale = the source step per output pixel
static int host_bicubic_grid(const float* src, int M, int D, int G, float scale, float* dst) {
  if (M <= 0 || D <= 0 || G <= 0) return OVM_ERR_INVALID;
  if (G == M) { memcpy(dst, src, (size_t)M * M * D * 4); return OVM_OK; }
  auto coef = [](float t, float* w) {
    const float A = -0.75f;
    auto c1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
    auto c2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
    w[0] = c2(t + 1.f); w[1] = c1(t); w[2] = c1(1.f - t); w[3] = c2(2.f - t);
  };
  for (int oy = 0; oy < G; ++oy) {
    const float ry = scale * ((float)oy + 0.5f) - 0.5f;
    const int iy = (int)floorf(ry);
    float wy[4]; coef(ry - (float)iy, wy);
    for (int ox = 0; ox < G; ++ox) {
      const float rx = scale * ((float)ox + 0.5f) - 0.5f;
      const int ix = (int)floorf(rx);
      float wx[4]; coef(rx - (float)ix, wx);
      float* o = dst + ((size_t)oy * G + ox) * D;
      for (int d = 0; d < D; ++d) o[d] = 0.f;
      for (int a = 0; a < 4; ++a) {
        int yy = iy - 1 + a; yy = yy < 0 ? 0 : (yy > M - 1 ? M - 1 : yy);
        for (int d = 0; d < D; ++d) {
          float acc = 0.f;
          for (int b = 0; b < 4; ++b) {
            int xx = ix - 1 + b; xx = xx < 0 ? 0 : (xx > M - 1 ? M - 1 : xx);
            acc += src[((size_t)yy * M + xx) * D + d] * wx[b];
          }
          o[d] += acc * wy[a];
        }
      }
    }
  }
  return OVM_OK;
}

// F.interpolate(src[1,C,L], size=Lo, mode="linear", align_corners=False) on rows [L][C] -> [Lo][C]
static void host_linear_rows(const float* src, int L, int C, int Lo, float* dst) {
  if (L == Lo) { memcpy(dst, src, (size_t)L * C * 4); return; }
  const float scale = (float)L / (float)Lo;
  for (int o = 0; o < Lo; ++o) {
    float f = scale * ((float)o + 0.5f) - 0.5f; if (f < 0.f) f = 0.f;
    int i0 = (int)f; if (i0 > L - 1) i0 = L - 1;
    const int i1 = i0 + (i0 < L - 1 ? 1 : 0);
    const float l1 = f - (float)i0, l0 = 1.f - l1;
    for (int c = 0; c < C; ++c) dst[(size_t)o * C + c] = l0 * src[(size_t)i0 * C + c] + l1 * src[(size_t)i1 * C + c];
  }
}

}  // namespace ovm

extern "C" {

// F.interpolate(pos[1,D,M,M], size=(G,G), mode="bicubic", align_corners=False, antialias=True) of the patch part of an
// open_clip positional embedding [1 + M*M][D], class row kept (reference clip.py:98-133). PyTorch's antialiased path is a
// separable, NORMALISED filter (not the clamped 4-tap one above): per output index, taps j in [xmin, xmin + xsize) with
// xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), M) - xmin, center = scale (i + 0.5),
// scale = M / G, support = 2 max(scale, 1), weight = cubic_{a = -0.5}((j - center + 0.5) / max(scale, 1)) / sum; all in fp32,
// width pass first, then height (ATen UpSampleKernel.cpp, _compute_indices_min_size_weights_aa). Returns pos unchanged when
// G == M (:117-118).
int ovm_host_resize_pos_embed_aa(const float* pos, int32_t M, int32_t D, int32_t G, float* out) {
  if (M <= 0 || D <= 0 || G <= 0) return OVM_ERR_INVALID;
  memcpy(out, pos, (size_t)D * 4);
  if (G == M) { memcpy(out + D, pos + D, (size_t)M * M * D * 4); return OVM_OK; }
  const float scale = (float)M / (float)G;
  const float support = scale >= 1.f ? 2.f * scale : 2.f;
  const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
  const int max_taps = (int)ceilf(support) * 2 + 1;
  auto filt = [](float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
    if (x < 2.f) return ((a * x - 5.f * a) * x + 8.f * a) * x - 4.f * a;
    return 0.f;
  };
  std::vector<int> xmin(G), xsize(G);
  std::vector<float> wt((size_t)G * max_taps, 0.f);
  for (int i = 0; i < G; ++i) {
    const float center = scale * ((float)i + 0.5f);
    int lo = (int)(center - support + 0.5f); if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5f); if (hi > M) hi = M;
    int n = hi - lo; if (n < 0) n = 0; if (n > max_taps) n = max_taps;
    xmin[i] = lo; xsize[i] = n;
    float total = 0.f;
    for (int j = 0; j < n; ++j) { const float w = filt(((float)(j + lo) - center + 0.5f) * invscale); wt[(size_t)i * max_taps + j] = w; total += w; }
    const float inv = total != 0.f ? 1.f / total : 0.f;
    for (int j = 0; j < n; ++j) wt[(size_t)i * max_taps + j] *= inv;
  }
  const float* src = pos + D;                              // [M][M][D]
  std::vector<float> tmp((size_t)M * G * D);               // width pass: [M][G][D]
  for (int y = 0; y < M; ++y)
    for (int ox = 0; ox < G; ++ox) {
      float* o = &tmp[((size_t)y * G + ox) * D];
      const float* w = &wt[(size_t)ox * max_taps];
      for (int d = 0; d < D; ++d) {
        float t = xsize[ox] > 0 ? src[((size_t)y * M + xmin[ox]) * D + d] * w[0] : 0.f;
        for (int j = 1; j < xsize[ox]; ++j) t += src[((size_t)y * M + xmin[ox] + j) * D + d] * w[j];
        o[d] = t;
      }
    }
  float* dst = out + D;
  for (int oy = 0; oy < G; ++oy) {
    const float* w = &wt[(size_t)oy * max_taps];
    for (int ox = 0; ox < G; ++ox) {
      float* o = dst + ((size_t)oy * G + ox) * D;
      for (int d = 0; d < D; ++d) {
        float t = xsize[oy] > 0 ? tmp[((size_t)xmin[oy] * G + ox) * D + d] * w[0] : 0.f;
        for (int j = 1; j < xsize[oy]; ++j) t += tmp[((size_t)(xmin[oy] + j) * G + ox) * D + d] * w[j];
        o[d] = t;
      }
    }
  }
  return OVM_OK;
}

// dinov2 interpolate_pos_encoding of a table [1 + M*M][D], class row kept: PyTorch upsample_bicubic2d, align_corners=False,
// scale_factor given (so the source scale is 1/scale_factor, which is what dinov2's +0.1 offset relies on).
int ovm_host_interp_pos_embed(const float* pos, int32_t M, int32_t D, int32_t G, float* out) {
  if (M <= 0 || D <= 0 || G <= 0) return OVM_ERR_INVALID;
  memcpy(out, pos, (size_t)D * 4);
  const double sf = ((double)G + 0.1) / (double)M;                  // python: float(w0 + 0.1) / M (double)
  return ovm::host_bicubic_grid(pos + D, M, D, G, (float)(1.0 / sf), out + D);
}

int ovm_host_swiglu_perm(int32_t Hs, int32_t* perm) {
  if (Hs < 1 || !perm) return OVM_ERR_INVALID;
  const int Kp = (Hs + 31) / 32 * 32;
  for (int n = 0; n < 2 * Kp; ++n) {
    const int j = ((n >> 5) << 4) | (n & 15);                   // output of packed row n (inverse of swiglu_row)
    perm[n] = j < Hs ? ((n & 16) ? Hs + j : j) : -1;
  }
  return OVM_OK;
}

int ovm_host_sincos_pos_embed(int32_t D, int32_t G, float* out) {
  if (D <= 0 || D % 4 != 0 || G <= 0) return OVM_ERR_INVALID;
  const int Q = D / 4;                                       // frequencies per (coordinate, sin / cos)
  std::vector<double> omega(Q);
  for (int i = 0; i < Q; ++i) omega[i] = 1.0 / pow(10000.0, (double)i / (double)Q);
  for (int d = 0; d < D; ++d) out[d] = 0.f;
  for (int y = 0; y < G; ++y)
    for (int x = 0; x < G; ++x) {
      float* o = out + (size_t)(1 + y * G + x) * D;
      // meshgrid(grid_w, grid_h): "grid[0]" is the x coordinate and feeds the FIRST half (named emb_h upstream)
      for (int i = 0; i < Q; ++i) {
        const double ax = (double)x * omega[i], ay = (double)y * omega[i];
        o[i] = (float)sin(ax); o[Q + i] = (float)cos(ax);
        o[2 * Q + i] = (float)sin(ay); o[3 * Q + i] = (float)cos(ay);
      }
    }
  return OVM_OK;
}

}  // extern "C"

namespace ovm {
namespace {

// dinov2 SwiGLUFFNFused.w12 [2 Hs][K] (rows [0, Hs) gates, [Hs, 2 Hs) values) -> the row order EPI_SWIGLU pairs (gemm.hpp): blocks of
// 16 gates | 16 values, outputs padded to Kp (a multiple of 32, >= Hs) with zero rows and zero bias (silu(0) * 0 = 0 fills the pad columns)
int pack_swiglu_w12(Loader* L, const WeightMap& wm, const std::string& prefix, int Hs, int Kp, int K, PackedLin* out) {
  const float *w, *b;
  int r = find_weight(L, wm, prefix + ".weight", (int64_t)2 * Hs * K, &w); if (r) return r;
  r = find_weight(L, wm, prefix + ".bias", (int64_t)2 * Hs, &b); if (r) return r;
  const int K32 = (Hs + 31) / 32 * 32;
  if (Kp % 32 != 0 || Kp < K32) return OVM_ERR_INVALID;
  std::vector<int32_t> perm((size_t)2 * K32);
  if (ovm_host_swiglu_perm(Hs, perm.data()) != OVM_OK) return OVM_ERR_INVALID;
  std::vector<float> v((size_t)2 * Kp * K, 0.f), bv((size_t)2 * Kp, 0.f);
  for (int n = 0; n < 2 * K32; ++n)                        // rows beyond 2 ceil32(Hs) are all padding
    if (perm[n] >= 0) { memcpy(&v[(size_t)n * K], w + (size_t)perm[n] * K, (size_t)K * 4); bv[n] = b[perm[n]]; }
  return upload_packed(L, v.data(), 2 * Kp, K, K, bv.data(), 2 * Kp, out);
}

// Hub DINOv2 variants: no config field names them, the checkpoint does. Host-only checks, before any device call.
int probe_variants(Tower* t, const WeightMap& wm, const std::string& V) {
  const int D = t->cfg.embed_dim;
  if (const OvmTensor* r = wm.get(V + "register_tokens")) {      // hub *_reg models: [1][R][D]
    if (r->ndim != 3 || r->shape[0] != 1 || r->shape[2] != D) { t->err = "bad shape for " + V + "register_tokens (expected [1][R][embed_dim])"; return OVM_ERR_SHAPE; }
    if (r->shape[1] > 16) { t->err = V + "register_tokens: more than 16 register tokens"; return OVM_ERR_CAPACITY; }
    t->nreg = (int)r->shape[1];
  }
  const std::string M0 = V + t->fam->block + "0.mlp.";
  const OvmTensor *w12 = wm.get(M0 + "w12.weight"), *fc1 = wm.get(M0 + "fc1.weight");
  if (w12 && fc1) { t->err = "checkpoint has both " + M0 + "w12.weight and " + M0 + "fc1.weight"; return OVM_ERR_INVALID; }
  if (!w12 && !fc1) { t->err = "missing weight: " + M0 + "fc1.weight or " + M0 + "w12.weight"; return OVM_ERR_MISSING_WEIGHT; }
  if (!w12) return OVM_OK;
  // hub vitg14: SwiGLUFFNFused, w12 [2 Hs][D], w3 [D][Hs]
  if (w12->ndim != 2 || w12->shape[0] < 2 || w12->shape[0] % 2 != 0 || w12->shape[1] != D) {
    t->err = "bad shape for " + M0 + "w12.weight (expected [2 Hs][embed_dim])"; return OVM_ERR_SHAPE;
  }
  const int64_t Hs = w12->shape[0] / 2;
  const OvmTensor* w3 = wm.get(M0 + "w3.weight");
  if (!w3) { t->err = "missing weight: " + M0 + "w3.weight"; return OVM_ERR_MISSING_WEIGHT; }
  if (w3->ndim != 2 || w3->shape[0] != D || w3->shape[1] != Hs) {
    t->err = "bad shape for " + M0 + "w3.weight (expected [embed_dim][" + std::to_string(Hs) + "] after " + M0 + "w12.weight)"; return OVM_ERR_SHAPE;
  }
  // the activation image lives in F1, sized for the 4 D wide GELU MLP; its width is the K of w3: whole 32-wide k-groups of the
  // split image, whole 64-wide k-steps in one-pass mode
  const int64_t kq = t->cfg.precision == 3 ? 32 : 64, Kp = (Hs + kq - 1) / kq * kq;
  if (Kp > 4 * (int64_t)D) { t->err = M0 + "w12.weight: hidden width exceeds 4 * embed_dim"; return OVM_ERR_CAPACITY; }
  t->ffn_hs = (int)Hs; t->ffn_k = (int)Kp;
  return OVM_OK;
}

int load_norm(Tower* t, const WeightMap& wm, const std::string& name, float** g, float** b) {
  int r = upload_weight(t, wm, name + ".weight", t->D, g); if (r) return r;
  return upload_weight(t, wm, name + ".bias", t->D, b);
}

// patch embed [D][3][P][P] -> [D][(py*P+px)*3 + c] (P = 14: K padded 588 -> 640), class / register tokens, the position table at the
// canvas grid (one row per patch (+ class row): register tokens have none), ln_pre and the final LayerNorm where the family has them
int load_embeddings(Tower* t, const WeightMap& wm, const std::string& V) {
  const FamilyRow& f = *t->fam;
  const int D = t->D, G = t->G, G2 = t->G2, PP = t->patch * t->patch, M = t->cfg.pos_grid, ncls = f.cls_token ? 1 : 0;
  int r;
  const float* w; r = find_weight(t, wm, V + f.pe_w, (int64_t)D * 3 * PP, &w); if (r) return r;
  std::vector<float> v((size_t)D * 3 * PP);
  for (int o = 0; o < D; ++o)
    for (int ch = 0; ch < 3; ++ch)
      for (int k = 0; k < PP; ++k) v[(size_t)o * 3 * PP + k * 3 + ch] = w[((size_t)o * 3 + ch) * PP + k];
  r = upload_packed(t, v.data(), D, 3 * PP, t->Kpe, nullptr, 0, &t->pe); if (r) return r;
  if (f.pe_b && (r = upload_weight(t, wm, V + f.pe_b, D, &t->pe.bias))) return r;
  if (f.cls && (r = upload_weight(t, wm, V + f.cls, D, &t->cls))) return r;
  std::vector<float> pi((size_t)(G2 + ncls) * D);
  const float* pos = nullptr;
  if (f.pos_rule == POS_STORED && M != G) { t->err = "HF DINOv2 tower: the position table must have the canvas grid (no interpolation)"; return OVM_ERR_UNSUPPORTED; }
  if (f.pos && (r = find_weight(t, wm, V + f.pos, (int64_t)(ncls + M * M) * D, &pos))) return r;
  switch (t->nreg ? POS_AA : f.pos_rule) {       // the hub's *_reg models are built with interpolate_offset = 0, interpolate_antialias = True
    case POS_HUB: r = ovm_host_interp_pos_embed(pos, M, D, G, pi.data()); break;
    case POS_AA: r = ovm_host_resize_pos_embed_aa(pos, M, D, G, pi.data()); break;
    case POS_GRID: r = host_bicubic_grid(pos, M, D, G, (float)M / (float)G, pi.data()); break;
    case POS_SINCOS: r = ovm_host_sincos_pos_embed(D, G, pi.data()); break;
    case POS_STORED: memcpy(pi.data(), pos, pi.size() * 4); break;
  }
  if (r) return r;
  if ((r = upload_f32(t, pi.data(), pi.size(), &t->pos))) return r;
  if (f.ln_pre && (r = load_norm(t, wm, V + f.ln_pre, &t->lnpre_g, &t->lnpre_b))) return r;
  if (f.ln_final && (r = load_norm(t, wm, V + f.ln_final, &t->fin_g, &t->fin_b))) return r;
  if (t->nreg && (r = upload_weight(t, wm, V + "register_tokens", (int64_t)t->nreg * D, &t->reg))) return r;
  return OVM_OK;
}

// segment_anything: the block's window side and its two relative-position tables at the block's attention grid
int load_rel_pos(Tower* t, const WeightMap& wm, const std::string& P, int l, TowerLayer* y) {
  y->ws = ((t->cfg.sam_global_mask >> l) & 1u) ? 0 : t->cfg.sam_window;
  const int side = y->ws ? y->ws : t->G;
  for (int hw = 0; hw < 2; ++hw) {
    const std::string key = P + (hw ? "attn.rel_pos_w" : "attn.rel_pos_h");
    const OvmTensor* tab = wm.get(key);
    if (!tab || tab->ndim != 2 || tab->shape[1] != 64) { t->err = "missing or mis-shaped weight: " + key; return OVM_ERR_MISSING_WEIGHT; }
    std::vector<float> out((size_t)(2 * side - 1) * 64);
    host_linear_rows(tab->data, (int)tab->shape[0], 64, 2 * side - 1, out.data());     // get_rel_pos: F.interpolate(mode="linear") when lengths differ
    const int r = upload_f32(t, out.data(), out.size(), hw ? &y->relw : &y->relh);
    if (r) return r;
  }
  return OVM_OK;
}

int load_block(Tower* t, const WeightMap& wm, const std::string& P, int l, TowerLayer* y) {
  const FamilyRow& f = *t->fam;
  const int D = t->D;
  int r;
  if ((r = load_norm(t, wm, P + f.norm1, &y->ln1g, &y->ln1b))) return r;
  if ((r = load_norm(t, wm, P + f.norm2, &y->ln2g, &y->ln2b))) return r;
  y->ls1 = y->ls2 = nullptr;
  if (f.ls1 && ((r = upload_weight(t, wm, P + f.ls1, D, &y->ls1)) || (r = upload_weight(t, wm, P + f.ls2, D, &y->ls2)))) return r;
  const std::string A = P + f.qkv;
  switch (f.qkv_kind) {
    case QKV_FUSED: r = pack_linear(t, wm, A, 3 * D, D, &y->qkv); break;
    case QKV_BARE: r = pack_linear_named(t, wm, A + "weight", A + "bias", 3 * D, D, &y->qkv); break;
    case QKV_TRIPLE: r = pack_concat(t, wm, {{A + "query", D}, {A + "key", D}, {A + "value", D}}, D, &y->qkv); break;
  }
  if (r) return r;
  if ((r = pack_linear(t, wm, P + f.proj, D, D, &y->proj))) return r;
  if (t->ffn_hs) {                                       // SwiGLUFFNFused: w12 row-permuted for EPI_SWIGLU, w3 with K padded to the image width
    if ((r = pack_swiglu_w12(t, wm, P + "mlp.w12", t->ffn_hs, t->ffn_k, D, &y->fc1))) return r;
    if ((r = pack_linear(t, wm, P + "mlp.w3", D, t->ffn_hs, &y->fc2, true, t->ffn_k))) return r;
  } else {
    if ((r = pack_linear(t, wm, P + f.fc1, 4 * D, D, &y->fc1))) return r;
    if ((r = pack_linear(t, wm, P + f.fc2, D, 4 * D, &y->fc2))) return r;
  }
  return f.rel_pos ? load_rel_pos(t, wm, P, l, y) : OVM_OK;
}

int alloc_workspace(Tower* t) {
  const int D = t->D, G = t->G, T = t->T, B = t->cfg.max_batch, heads = t->cfg.heads;
  const size_t MT = (size_t)B * T, MP = (size_t)B * t->G2;
  int r;
  if ((r = t->alloc(&t->X, MT * D))) return r;
  if ((r = salloc(t, &t->PA, MP * t->Kpe))) return r;
  if ((r = salloc(t, &t->HN, MT * D, false, true))) return r;
  if ((r = salloc(t, &t->AO, MT * D, false, true))) return r;
  if ((r = salloc(t, &t->F1, MT * 4 * D, false, true))) return r;
  if ((r = salloc(t, &t->Q, MT * D))) return r;
  if ((r = salloc(t, &t->Kx, MT * D))) return r;
  if ((r = salloc(t, &t->Vt, (size_t)B * D * t->Tpad, true))) return r;
  t->ctx.splitk_cap = (size_t)112 << 20;     // split-K is only taken for <= 96 tiles of 128 x 128 with <= 16 slices: <= 100.7 MB of fp32 partials
  { char* q = nullptr; if ((r = t->alloc(&q, t->ctx.splitk_cap))) return r; t->ctx.splitk_ws = (float*)q; }
  if ((r = t->alloc(&t->attn_tail_ws, attn_tail_ws_floats(B, heads)))) return r;
  if ((r = t->alloc(&t->attn_tail_cnt, (size_t)B * heads * 8, true))) return r;
  if (t->fam->rel_pos) {
    const int ws = t->cfg.sam_window, gp = (G + ws - 1) / ws * ws, nw1 = gp / ws;
    t->sam_ws = ws; t->sam_nw = nw1 * nw1; t->sam_rows = t->sam_nw * ws * ws;
    std::vector<int> map((size_t)B * t->sam_rows);
    for (int b = 0; b < B; ++b)
      for (int wy = 0; wy < nw1; ++wy)
        for (int wx = 0; wx < nw1; ++wx)
          for (int iy = 0; iy < ws; ++iy)
            for (int ix = 0; ix < ws; ++ix) {
              const int y = wy * ws + iy, x = wx * ws + ix;          // window_partition pads bottom / right (segment_anything)
              map[(size_t)b * t->sam_rows + ((size_t)(wy * nw1 + wx) * ws + iy) * ws + ix] = (y < G && x < G) ? b * T + y * G + x : -1;
            }
    if ((r = t->alloc(&t->sam_map, map.size()))) return r;
    OVM_HIP(t, hipMemcpy(t->sam_map, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
    const size_t MW = (size_t)B * (t->sam_rows > T ? t->sam_rows : T);
    t->ldrel = ((ws > G ? ws : G) + 3) / 4 * 4;
    if ((r = salloc(t, &t->XW, MW * D))) return r;
    if ((r = salloc(t, &t->CTX, MW * D))) return r;
    if ((r = t->alloc(&t->QKVF, MW * 3 * D))) return r;
    if ((r = t->alloc(&t->RELH, MW * heads * t->ldrel))) return r;
    if ((r = t->alloc(&t->RELW, MW * heads * t->ldrel))) return r;
  }
  if ((r = t->alloc(&t->d_imgs, (size_t)B))) return r;
  OVM_HIP(t, hipHostMalloc((void**)&t->h_imgs, sizeof(ImageDesc) * B));
  return OVM_OK;
}

}  // namespace

int Tower::configure(const TowerConfig& c) {
  cfg = c;
  if (c.family < 0 || c.family >= FAM_COUNT) { err = "invalid config (tower)"; return OVM_ERR_INVALID; }
  fam = &kFamilies[c.family];
  if (fam->rel_pos && (c.sam_window < 1 || c.depth > 32 || c.pos_grid < 1)) { err = "invalid config (sam_window, depth <= 32, pos_grid)"; return OVM_ERR_INVALID; }
  patch = fam->patch; Kpe = fam->Kpe; mlp_act = fam->mlp_act;
  ln_eps = c.ln_eps > 0.f ? c.ln_eps : fam->ln_eps;
  if (c.canvas % patch != 0 || c.embed_dim % 128 != 0 || c.embed_dim != c.heads * 64 || (c.precision != 1 && c.precision != 3) || c.max_batch < 1) {
    err = kErrTowerGeometry; return OVM_ERR_INVALID;
  }
  precision = ctx.precision = c.precision;
  D = c.embed_dim; G = c.canvas / patch; G2 = G * G;
  return OVM_OK;
}

int Tower::load(const OvmTensor* weights, int n_weights, int device_) {
  const WeightMap wm(weights, n_weights); device = device_;
  const std::string V = cfg.prefix ? cfg.prefix : fam->prefix;
  int r;
  if (fam->variants && weights && (r = probe_variants(this, wm, V))) return r;
  OVM_HIP(this, hipSetDevice(device));
  T = G2 + (fam->cls_token ? 1 : 0) + nreg; Tpad = (T + 63) / 64 * 64;
  // The GEMM kernels address operands with 32-bit element offsets (gemm.hip: gemm_offsets_fit): refuse a max_batch whose largest
  // activation image would not fit, here, before anything is allocated - not at the first oversized launch.
  const uint64_t B = cfg.max_batch, il = precision == 3 ? 2 : 1;         // interleaved split rows are 2K halves long
  if (B * T * 4 * D * il > (1ull << 32) /* fc2's input (GELU output), the longest activation rows */ || B * G2 * Kpe > (1ull << 32) /* patch rows */) {
    err = kErrOffsets; return OVM_ERR_CAPACITY;
  }
  if ((r = load_embeddings(this, wm, V))) return r;
  layers.resize(cfg.depth);
  for (int l = 0; l < cfg.depth; ++l)
    if ((r = load_block(this, wm, V + fam->block + std::to_string(l) + ".", l, &layers[l]))) return r;
  if ((r = alloc_workspace(this))) return r;
  OVM_HIP(this, hipDeviceSynchronize());
  return OVM_OK;
}

void Tower::destroy() { free_all(); if (h_imgs) (void)hipHostFree(h_imgs); h_imgs = nullptr; }

int Tower::stage_images(const OvmImage* im, int B, hipStream_t s) {
  for (int b = 0; b < B; ++b) h_imgs[b] = ImageDesc{im[b].data, im[b].height, im[b].width, im[b].stride_c, im[b].stride_h, im[b].stride_w};
  OVM_HIP(this, hipMemcpyAsync(d_imgs, h_imgs, sizeof(ImageDesc) * B, hipMemcpyHostToDevice, s));
  return OVM_OK;
}

struct TowerRun { const TowerViews* views; int ntap; const int* tap_blk; float* const* tap_dst; };   // tower_forward_f32's per-call arguments

// patch embed (+ preprocess) and the ViT blocks: the residual stream X [B * T][D] fp32 afterwards holds the last block's tokens
int Tower::launches(int B, hipStream_t s, const TowerRun* run) {
  const int heads = cfg.heads, L = cfg.depth;
  // ---- patch embed (+ preprocess) ----
  if (run) OVM_TRY(this, launch_patch_gather_f32(*run->views, B, G, Kpe, PA.hi, PA.lo, s));
  else OVM_TRY(this, launch_patch_gather(d_imgs, B, G, patch, Kpe, cfg.pixel_mean, cfg.pixel_std, PA.hi, PA.lo, s));
  if (fam->cls_token) OVM_TRY(this, launch_cls_init(X, cls, pos, reg, nreg, B, T, D, s));       // SAM: no class token (T = G^2)
  {
    GemmParams p = gp_base(PA, Kpe, pe, B * G2);
    p.X = X; p.ldx = D; p.pos = pos; p.G2 = G2; p.T = T;
    OVM_TRY(this, gemm(ctx, p, EPI_PATCH, A_ROWMAJOR, s));
  }
  const int M = B * T;
  const float eps = ln_eps;
  if (lnpre_g) {                                        // open_clip: x = ln_pre(x + pos) (reference clip.py:78-79), in place
    LnOut o; memset(&o, 0, sizeof(o)); o.f32 = X; o.ldf = D;
    ProfScope ps(ctx, OVM_PROF_LN, s); OVM_TRY(this, launch_ln_rows(X, D, M, D, lnpre_g, lnpre_b, eps, o, s));
  }
  for (int l = 0; l < L; ++l) {
    const TowerLayer& y = layers[l];
    const int il = precision == 3 ? 1 : 0, am = il ? 2 : 1;    // activations of the blocks: interleaved split images in f16x3 mode
    LnOut o; memset(&o, 0, sizeof(o)); o.hi = HN.hi; o.lo = HN.lo; o.ld = am * D; o.il = il;
    if (fam->rel_pos) {
      // segment_anything Block (reference sam.py:100-106 runs vit.blocks as they are): norm1 -> [zero-padded 14 x 14 windows] ->
      // attention with the decomposed relative-position bias -> [un-partition] -> + shortcut. Same organisation as a Swin block of
      // the detector: the norm writes window-partitioned rows (padding rows zero AFTER the norm), the projection's epilogue
      // scatters back through the same map and adds the shortcut. Scores are exact fp32 products on the matrix cores (attn_f32).
      const int ws = y.ws, rows = ws ? sam_rows : T, Mw = B * rows, side = ws ? ws : G, Tq = side * side, nseq = Mw / Tq;
      {
        RowOpParams rp; memset(&rp, 0, sizeof(rp));
        rp.x = X; rp.ldx = D; rp.gamma = y.ln1g; rp.beta = y.ln1b; rp.eps = eps; rp.M = Mw; rp.D = D;
        if (ws) { rp.idx = sam_map; rp.nidx = 1; rp.seg = D; rp.zero_masked = 1; }
        rp.hi = XW.hi; rp.lo = XW.lo; rp.ldh = D;
        ProfScope ps(ctx, OVM_PROF_LN, s); OVM_TRY(this, launch_rowop(rp, s));
      }
      {
        GemmParams p = gp_base(XW, D, y.qkv, Mw);
        p.C = QKVF; p.ldc = 3 * D;
        OVM_TRY(this, gemm(ctx, p, EPI_STORE, A_ROWMAJOR, s, OVM_PROF_QKV));
      }
      {
        ProfScope ps(ctx, OVM_PROF_ATTN, s);
        // the bias tables use the UNSCALED query (add_decomposed_rel_pos is given q, the scores use q * scale)
        OVM_TRY(this, launch_relpos_tables(QKVF, 3 * D, Mw, heads, 64, side, side, y.relh, y.relw, RELH, RELW, ldrel, s));
        AttnF32Params a; memset(&a, 0, sizeof(a));
        a.q = QKVF; a.k = QKVF + D; a.v = QKVF + 2 * D; a.ldq = a.ldk = a.ldv = 3 * D;
        a.sq1 = a.sk1 = a.sv1 = (long)Tq * 3 * D; a.sq2 = a.sk2 = a.sv2 = 64;
        a.ohi = CTX.hi; a.olo = CTX.lo; a.ldoh = D; a.soh1 = (long)Tq * D; a.soh2 = 64;
        a.nb1 = nseq; a.nb2 = heads; a.Tq = Tq; a.Tk = Tq; a.DH = 64; a.scale = 0.125f;
        a.rel_h = RELH; a.rel_w = RELW; a.rel_gw = side; a.ldrel = ldrel;
        OVM_TRY(this, launch_attn_f32(a, s));
      }
      {
        GemmParams p = gp_base(CTX, D, y.proj, Mw);
        p.X = X; p.ldx = D; p.row_map = ws ? sam_map : nullptr;
        OVM_TRY(this, gemm(ctx, p, EPI_RESID, A_ROWMAJOR, s, OVM_PROF_PROJ));
      }
    } else {
      { ProfScope ps(ctx, OVM_PROF_LN, s); OVM_TRY(this, launch_ln_rows(X, D, M, D, y.ln1g, y.ln1b, eps, o, s)); }
      {
        GemmParams p = gp_base(HN, am * D, y.qkv, M); p.a_il = il;
        p.Qhi = Q.hi; p.Qlo = Q.lo; p.Khi = Kx.hi; p.Klo = Kx.lo; p.Vhi = Vt.hi; p.Vlo = Vt.lo;
        p.T = T; p.Tpad = Tpad; p.heads = heads; p.qscale = kQScale;
        OVM_TRY(this, gemm(ctx, p, EPI_QKV, A_ROWMAJOR, s, OVM_PROF_QKV));
      }
      {
        AttnParams a; memset(&a, 0, sizeof(a));
        a.Qhi = Q.hi; a.Qlo = Q.lo; a.Khi = Kx.hi; a.Klo = Kx.lo; a.Vhi = Vt.hi; a.Vlo = Vt.lo;
        a.Ohi = AO.hi; a.Olo = AO.lo; a.ldo = am * D; a.o_il = il; a.B = B; a.heads = heads; a.T = T; a.Tpad = Tpad;
        a.corun = corun ? 1 : 0;
        a.tail_ws = attn_tail_ws; a.tail_cnt = attn_tail_cnt;     // leftover queries (T = 4097: one per head) split over the keys
        { ProfScope ps(ctx, OVM_PROF_ATTN, s); OVM_TRY(this, launch_attention(a, precision, s)); }
      }
      {
        GemmParams p = gp_base(AO, am * D, y.proj, M); p.a_il = il;
        p.gamma = y.ls1; p.X = X; p.ldx = D;
        OVM_TRY(this, gemm(ctx, p, EPI_RESID, A_ROWMAJOR, s, OVM_PROF_PROJ));
      }
    }
    { ProfScope ps(ctx, OVM_PROF_LN, s); OVM_TRY(this, launch_ln_rows(X, D, M, D, y.ln2g, y.ln2b, eps, o, s)); }
    const int Kf = ffn_hs ? ffn_k : 4 * D;                    // width of the FFN's activation image = K of its second linear
    if (ffn_hs) {                                             // w12 with silu(gate) * value in the epilogue
      GemmParams p = gp_base(HN, am * D, y.fc1, M); p.a_il = il;
      p.Ohi = F1.hi; p.Olo = F1.lo; p.ldo = am * Kf; p.o_il = il;
      OVM_TRY(this, gemm(ctx, p, EPI_SWIGLU, A_ROWMAJOR, s, OVM_PROF_FC1));
    } else {
      GemmParams p = gp_base(HN, am * D, y.fc1, M); p.a_il = il;
      p.Ohi = F1.hi; p.Olo = F1.lo; p.ldo = am * 4 * D; p.o_il = il; p.relu = mlp_act;
      OVM_TRY(this, gemm(ctx, p, EPI_GELU, A_ROWMAJOR, s, OVM_PROF_FC1));
    }
    {
      GemmParams p = gp_base(F1, am * Kf, y.fc2, M); p.a_il = il;
      p.gamma = y.ls2; p.X = X; p.ldx = D;
      OVM_TRY(this, gemm(ctx, p, EPI_RESID, A_ROWMAJOR, s, OVM_PROF_FC2));
    }
    for (int k = 0; run && k < run->ntap; ++k)                // the residual stream after block l (HF hidden_states[l + 1])
      if (run->tap_blk[k] == l) OVM_HIP(this, hipMemcpyAsync(run->tap_dst[k], X, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
  }
  return OVM_OK;
}

int tower_forward(Tower* t, const OvmImage* image, hipStream_t s) {
  if (!t || !image) return OVM_ERR_INVALID;
  t->err.clear();
  const int canvas = t->cfg.canvas;
  if (image->height > canvas || image->width > canvas || image->height < 1 || image->width < 1) {
    t->err = "image larger than the encoder's canvas"; return OVM_ERR_SHAPE;
  }
  OVM_HIP(t, hipSetDevice(t->device));
  OVM_HIP(t, hipStreamSynchronize(s));                    // the pinned descriptor below may still be read by the previous call's upload
  const int r = t->stage_images(image, 1, s);
  return r ? r : t->launches(1, s);
}

int tower_forward_f32(Tower* t, const TowerViews& views, int n_taps, const int* tap_blocks, float* const* tap_out, float* final_out, hipStream_t s) {
  if (!t || t->patch != 16 || t->fam->rel_pos) return OVM_ERR_INVALID;
  t->err.clear();
  const int B = views.n;
  if (B < 1 || B > t->cfg.max_batch || B > kMaxTowerViews) { t->err = "crop count exceeds max_batch"; return OVM_ERR_CAPACITY; }
  if (n_taps < 0 || n_taps > kMaxTowerTaps) { t->err = "too many taps"; return OVM_ERR_CAPACITY; }
  for (int k = 0; k < n_taps; ++k)
    if (tap_blocks[k] < 0 || tap_blocks[k] >= t->cfg.depth || !tap_out[k]) { t->err = "tap block out of range"; return OVM_ERR_INVALID; }
  if (final_out && !t->fin_g) { t->err = "the tower has no final LayerNorm"; return OVM_ERR_INVALID; }
  OVM_HIP(t, hipSetDevice(t->device));
  const TowerRun run{&views, n_taps, tap_blocks, tap_out};
  if (const int r = t->launches(B, s, &run)) return r;
  if (final_out) {
    LnOut o; memset(&o, 0, sizeof(o)); o.f32 = final_out; o.ldf = t->D;
    OVM_TRY(t, launch_ln_rows(t->X, t->D, B * t->T, t->D, t->fin_g, t->fin_b, t->ln_eps, o, s));
  }
  return OVM_OK;
}

}  // namespace ovm
