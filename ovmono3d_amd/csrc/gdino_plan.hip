// GroundingDINO engine: plans. Everything that depends only on (image size, caption) - index maps of the window partition / shift /
// patch merging, shift masks, sine position embeddings, reference grids, text masks - is built on the host once per plan and uploaded
// (build_plan), with the scratch a forward needs and the tune knobs it will run under. The handle keeps its plans in a least recently
// used cache (find_plan, evict_plans); a plan's forward is captured into one HIP graph after its first run (capture_plan).
// What depends on the caption and the weights alone - the text encoder's output - is not a plan's but a TextEntry's, shared by
// all plans of that caption (find_text, keep_text).
#include <cmath>
#include <memory>
#include <set>
#include "gdino_model.hpp"

namespace ovm {
namespace gdino {
namespace {

// device buffer owned by the plan: count elements, filled from src when given
template <typename T>
int pal(OvmGdino* g, Plan* pl, T** out, size_t count, const T* src = nullptr) {
  void* q = nullptr;
  size_t bytes = count * sizeof(T); if (bytes == 0) bytes = 16;
  OVM_HIP(g, hipMalloc(&q, bytes));
  pl->allocs.push_back(q); pl->bytes += bytes;
  if (src && count) OVM_HIP(g, hipMemcpy(q, src, count * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)q;
  return OVM_OK;
}
template <typename T>
int pup(OvmGdino* g, Plan* pl, const std::vector<T>& v, T** out) { return pal(g, pl, out, v.size(), v.data()); }

// GroundingDINO generate_masks_with_special_tokens_and_transfer_map: tokens attend inside their own sub-sentence (delimited by
// [CLS] [SEP] . ?); position ids restart per phrase, the closing delimiter included (upstream numbering)
void text_masks(const std::vector<int>& ids, std::vector<char>* mask, std::vector<int>* pos) {
  const int T = (int)ids.size();
  mask->assign((size_t)T * T, 0);
  pos->assign(T, 0);
  for (int i = 0; i < T; ++i) (*mask)[(size_t)i * T + i] = 1;
  int prev = 0;
  for (int col = 0; col < T; ++col) {
    const int t = ids[col];
    if (!(t == 101 || t == 102 || t == 1012 || t == 1029)) continue;
    if (col == 0 || col == T - 1) {
      (*mask)[(size_t)col * T + col] = 1; (*pos)[col] = 0;
    } else {
      for (int a = prev + 1; a <= col; ++a) {
        for (int b = prev + 1; b <= col; ++b) (*mask)[(size_t)a * T + b] = 1;
        (*pos)[a] = a - prev - 1;
      }
    }
    prev = col;
  }
}

void window_maps(int H, int W, int ws, int shift, std::vector<int>* win, std::vector<float>* mask, int* nW) {
  const int Hp = (H + ws - 1) / ws * ws, Wp = (W + ws - 1) / ws * ws, nwh = Hp / ws, nww = Wp / ws, ws2 = ws * ws;
  win->assign((size_t)nwh * nww * ws2, -1);
  for (int y = 0; y < Hp; ++y)
    for (int x = 0; x < Wp; ++x) {
      const int sy = (y + shift) % Hp, sx = (x + shift) % Wp;      // source (padded) coordinates of shifted-map position (y, x)
      const int src = (sy < H && sx < W) ? sy * W + sx : -1;
      (*win)[((size_t)(y / ws) * nww + x / ws) * ws2 + (y % ws) * ws + x % ws] = src;
    }
  *nW = nwh * nww;
  mask->clear();
  if (shift > 0) {
    std::vector<int> img((size_t)Hp * Wp);
    for (int y = 0; y < Hp; ++y)
      for (int x = 0; x < Wp; ++x) {
        const int hr = (y >= Hp - ws) + (y >= Hp - shift), wr = (x >= Wp - ws) + (x >= Wp - shift);
        img[(size_t)y * Wp + x] = hr * 3 + wr;
      }
    mask->assign((size_t)nwh * nww * ws2 * ws2, 0.f);
    for (int wy = 0; wy < nwh; ++wy)
      for (int wx = 0; wx < nww; ++wx) {
        const size_t base = ((size_t)wy * nww + wx) * ws2 * ws2;
        for (int a = 0; a < ws2; ++a) {
          const int ia = img[(size_t)(wy * ws + a / ws) * Wp + wx * ws + a % ws];
          for (int b = 0; b < ws2; ++b) {
            const int ib = img[(size_t)(wy * ws + b / ws) * Wp + wx * ws + b % ws];
            (*mask)[base + (size_t)a * ws2 + b] = (ia != ib) ? -100.0f : 0.f;
          }
        }
      }
  }
}

// GroundingDINO PositionEmbeddingSineHW with an all-valid mask, [h*w][2*dhalf] = (pos_y | pos_x); float32 arithmetic as torch
void sine_pos(int h, int w, int dhalf, float temperature, std::vector<float>* out) {
  out->assign((size_t)h * w * 2 * dhalf, 0.f);
  const float eps = 1e-6f, scale = 2.0f * 3.14159265358979323846f;
  std::vector<float> dim_t(dhalf);
  for (int i = 0; i < dhalf; ++i) dim_t[i] = powf(temperature, 2.0f * (float)(i / 2) / (float)dhalf);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const float ye = (float)(y + 1) / ((float)h + eps) * scale, xe = (float)(x + 1) / ((float)w + eps) * scale;
      float* o = out->data() + ((size_t)y * w + x) * 2 * dhalf;
      for (int i = 0; i < dhalf; ++i) {
        const float py = ye / dim_t[i], px = xe / dim_t[i];
        o[i] = (i & 1) ? cosf(py) : sinf(py);
        o[dhalf + i] = (i & 1) ? cosf(px) : sinf(px);
      }
    }
}

// token / position ids, the sub-sentence attention bias and the text enhancers' sine position embedding
int plan_text(OvmGdino* g, Plan* pl, const std::vector<int>& pids_in) {
  const int T = pl->T, D = g->cfg.d_model;
  std::vector<char> mask; std::vector<int> pids;
  text_masks(pl->ids, &mask, &pids);
  if (!pids_in.empty()) pids = pids_in;
  pl->pids = pids_in;
  for (int t = 0; t < T; ++t) {
    if (pl->ids[t] < 0 || pl->ids[t] >= g->vocab) { g->err = "token id out of the vocabulary"; return OVM_ERR_INVALID; }
    if (pids[t] < 0 || pids[t] >= g->n_pos) { g->err = "position id out of range"; return OVM_ERR_INVALID; }
  }
  OVM_TRY(g, pup(g, pl, pl->ids, &pl->d_ids));
  OVM_TRY(g, pup(g, pl, pids, &pl->d_pids));
  std::vector<float> bias((size_t)T * T);
  for (size_t i = 0; i < bias.size(); ++i) bias[i] = mask[i] ? 0.f : -3.4028234663852886e38f;     // torch.finfo(float32).min
  OVM_TRY(g, pup(g, pl, bias, &pl->text_bias));
  std::vector<float> pf(T); for (int t = 0; t < T; ++t) pf[t] = (float)pids[t];
  float* d_pf; OVM_TRY(g, pup(g, pl, pf, &d_pf));
  OVM_TRY(g, pal(g, pl, &pl->text_pos, (size_t)T * D));
  OVM_TRY(g, ovm_g_sine_embed(d_pf, T, 1, D, 10000.0f, pl->text_pos, nullptr));
  OVM_HIP(g, hipDeviceSynchronize());
  return OVM_OK;
}

// patch-embedding gather, per stage the two window maps (plain, shifted) and the patch-merging gather; feat_hw: the output stages' sizes
int plan_swin(OvmGdino* g, Plan* pl, std::vector<std::pair<int, int>>* feat_hw) {
  const int P = 4, ws = g->cfg.swin_window, H = pl->H, W = pl->W;
  pl->Hp = (H + P - 1) / P; pl->Wp = (W + P - 1) / P;
  {
    std::vector<int> pm((size_t)pl->Hp * pl->Wp * P * P);
    for (int oy = 0; oy < pl->Hp; ++oy)
      for (int ox = 0; ox < pl->Wp; ++ox)
        for (int py = 0; py < P; ++py)
          for (int px = 0; px < P; ++px) {
            const int y = oy * P + py, x = ox * P + px;
            pm[((size_t)oy * pl->Wp + ox) * P * P + py * P + px] = (y < H && x < W) ? y * W + x : -1;
          }
    OVM_TRY(g, pup(g, pl, pm, &pl->pe_map));
  }
  int h = pl->Hp, w = pl->Wp;
  pl->geo.resize(g->stages.size());
  for (size_t s = 0; s < g->stages.size(); ++s) {
    StageGeo& ge = pl->geo[s];
    ge.h = h; ge.w = w;
    for (int sh = 0; sh < 2; ++sh) {
      std::vector<int> win; std::vector<float> mk; int nW;
      window_maps(h, w, ws, sh ? ws / 2 : 0, &win, &mk, &nW);
      ge.wm[sh].nW = nW;
      OVM_TRY(g, pup(g, pl, win, &ge.wm[sh].win));
      if (!mk.empty()) OVM_TRY(g, pup(g, pl, mk, &ge.wm[sh].mask));
    }
    if (g->stages[s].has_out) feat_hw->push_back({h, w});
    if (g->stages[s].has_red) {
      const int h2 = (h + 1) / 2, w2 = (w + 1) / 2;
      std::vector<int> mm((size_t)h2 * w2 * 4, -1);
      for (int oy = 0; oy < h2; ++oy)
        for (int ox = 0; ox < w2; ++ox) {
          int k = 0;
          for (int col = 0; col < 2; ++col)                       // HF order: for col in 2: for row in 2
            for (int row = 0; row < 2; ++row) {
              const int y = 2 * oy + row, x = 2 * ox + col;
              mm[((size_t)oy * w2 + ox) * 4 + k++] = (y < h && x < w) ? y * w + x : -1;
            }
        }
      OVM_TRY(g, pup(g, pl, mm, &ge.merge));
      ge.h2 = h2; ge.w2 = w2;
      h = h2; w = w2;
    }
  }
  return OVM_OK;
}

// sizes and offsets of the feature levels; the extra level's 3x3 stride-2 convolution gets its im2col map
int plan_levels(OvmGdino* g, Plan* pl, const std::vector<std::pair<int, int>>& feat_hw) {
  const OvmGdinoConfig& c = g->cfg;
  pl->nlev = c.n_levels;
  const int nfeat = (int)feat_hw.size();
  if (nfeat > c.n_levels || c.n_levels > 8) { g->err = "level count"; return OVM_ERR_SHAPE; }
  int st = 0, lh = 0, lw = 0;
  for (int l = 0; l < c.n_levels; ++l) {
    if (l < nfeat) { lh = feat_hw[l].first; lw = feat_hw[l].second; }
    else {
      const int h2 = (lh + 2 - 3) / 2 + 1, w2 = (lw + 2 - 3) / 2 + 1;
      if (l == nfeat) {                                            // 3x3 stride-2 pad-1 conv on the last backbone stage: im2col map
        std::vector<int> cm((size_t)h2 * w2 * 9, -1);
        for (int oy = 0; oy < h2; ++oy)
          for (int ox = 0; ox < w2; ++ox)
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) {
                const int y = 2 * oy + ky - 1, x = 2 * ox + kx - 1;
                cm[((size_t)oy * w2 + ox) * 9 + ky * 3 + kx] = (y >= 0 && y < lh && x >= 0 && x < lw) ? y * lw + x : -1;
              }
        OVM_TRY(g, pup(g, pl, cm, &pl->conv_map));
        pl->conv_h = lh; pl->conv_w = lw;
      } else { g->err = "more than one extra feature level is not supported"; return OVM_ERR_SHAPE; }
      lh = h2; lw = w2;
    }
    pl->lh[l] = lh; pl->lw[l] = lw; pl->lstart[l] = st; st += lh * lw;
  }
  pl->S = st;
  return OVM_OK;
}

// per encoder token: position embedding (+ level embedding), reference point, proposal logits and the valid-proposal gather
int plan_encoder_tables(OvmGdino* g, Plan* pl) {
  const OvmGdinoConfig& c = g->cfg;
  const int S = pl->S, D = c.d_model;
  std::vector<float> pos((size_t)S * D), ref((size_t)S * 2), prop((size_t)S * 4);
  std::vector<int> valid(S);
  for (int l = 0; l < c.n_levels; ++l) {
    const int hh = pl->lh[l], ww = pl->lw[l];
    std::vector<float> sp; sine_pos(hh, ww, D / 2, c.pe_temperature, &sp);
    for (int i = 0; i < hh * ww; ++i) {
      float* o = pos.data() + (size_t)(pl->lstart[l] + i) * D;
      for (int d = 0; d < D; ++d) o[d] = sp[(size_t)i * D + d] + g->level_embed[(size_t)l * D + d];
      const int y = i / ww, x = i % ww;
      // reference points: linspace(0.5, n - 0.5, n) / n (valid ratios are 1: no padding)
      const float rx = ((float)x + 0.5f) / (float)ww, ry = ((float)y + 0.5f) / (float)hh;
      ref[(size_t)(pl->lstart[l] + i) * 2] = rx; ref[(size_t)(pl->lstart[l] + i) * 2 + 1] = ry;
      // proposals: ((grid + 0.5) / (w, h), 0.05 * 2^l)
      const float gx = ((float)x + 0.5f) / (float)ww, gy = ((float)y + 0.5f) / (float)hh, wh = 0.05f * (float)(1 << l);
      const float pr[4] = {gx, gy, wh, wh};
      bool ok = true;
      for (int k = 0; k < 4; ++k) ok = ok && (pr[k] > 0.01f) && (pr[k] < 0.99f);
      for (int k = 0; k < 4; ++k) prop[(size_t)(pl->lstart[l] + i) * 4 + k] = ok ? logf(pr[k] / (1.0f - pr[k])) : INFINITY;
      valid[pl->lstart[l] + i] = ok ? pl->lstart[l] + i : -1;
    }
  }
  OVM_TRY(g, pup(g, pl, pos, &pl->pos));
  OVM_TRY(g, pup(g, pl, ref, &pl->ref));
  OVM_TRY(g, pup(g, pl, prop, &pl->prop_logit));
  OVM_TRY(g, pup(g, pl, valid, &pl->valid_idx));
  if (S < c.num_queries) {       // torch.topk in the upstream two-stage selection raises the same way
    g->err = "selected index k out of range: " + std::to_string(S) + " encoder tokens < " + std::to_string(c.num_queries) + " queries (image too small)";
    return OVM_ERR_SHAPE;
  }
  return OVM_OK;
}

// what a forward writes outside the arena: the normalised image, sort keys, outputs, split-K workspace
int plan_scratch(OvmGdino* g, Plan* pl) {
  const OvmGdinoConfig& c = g->cfg;
  OVM_TRY(g, pal(g, pl, &pl->img, (size_t)pl->H * pl->W * 3));
  pl->topk_N = 2048; while (pl->topk_N < pl->S) pl->topk_N <<= 1;      // the bitonic sort's minimum length is one 2048-key tile
  OVM_TRY(g, pal(g, pl, &pl->topk_keys, (size_t)pl->topk_N));
  OVM_TRY(g, pal(g, pl, &pl->out_logits, (size_t)c.num_queries * c.max_text_len));
  OVM_TRY(g, pal(g, pl, &pl->out_boxes, (size_t)c.num_queries * 4));
  pl->gemm_ws_cap = (size_t)64 << 20;
  return pal(g, pl, (char**)&pl->gemm_ws, pl->gemm_ws_cap);
}

// tune.fold(): per encoder layer P [S][NOW] = pos W_off^T + b_off, the position term of the sampling-offsets | attention-weights
// projection ((vis + pos) W^T + b = vis W^T + P; pos depends on the image shape and level_embed alone). Computed once, here, with the
// engine's fp32-A GEMM on the null stream and finished before the plan is handed out; the forward's merged GEMM adds it in its epilogue.
int plan_offset_tables(OvmGdino* g, Plan* pl) {
  const OvmGdinoConfig& c = g->cfg;
  const int S = pl->S, D = c.d_model, NOW = c.heads * c.n_levels * c.n_points * 3;
  if (!gemm_small_supported(pl->pos, D, D)) { g->err = "offsets tables: d_model must be a multiple of 4"; return OVM_ERR_SHAPE; }
  pl->enc_P.assign(g->enc.size(), nullptr);
  for (size_t i = 0; i < g->enc.size(); ++i) {
    const Lin& w = g->enc[i].msda.offw;
    if (w.N != NOW || w.K != D) { g->err = "offsets tables: sampling-offsets weight shape"; return OVM_ERR_SHAPE; }
    OVM_TRY(g, pal(g, pl, &pl->enc_P[i], (size_t)S * NOW));
    OVM_TRY(g, launch_gemm_small_ex(pl->pos, nullptr, D, S, D, w.hi, w.lo, NOW, w.Kpad, w.bias, 0, nullptr, 0, pl->enc_P[i], NOW, g->precision,
                                    pl->gemm_ws, pl->gemm_ws_cap, nullptr));
  }
  OVM_HIP(g, hipDeviceSynchronize());
  return OVM_OK;
}

}  // namespace

int build_plan(OvmGdino* g, int H, int W, const std::vector<int>& ids, const std::vector<int>& pids, Plan** out) {
  std::unique_ptr<Plan> pl(new Plan());
  pl->H = H; pl->W = W; pl->T = (int)ids.size(); pl->ids = ids;
  pl->tune = g_gdino_tune; pl->tune.branches = g->branches;
  std::vector<std::pair<int, int>> feat_hw;
  OVM_TRY(g, plan_text(g, pl.get(), pids));
  OVM_TRY(g, plan_swin(g, pl.get(), &feat_hw));
  OVM_TRY(g, plan_levels(g, pl.get(), feat_hw));
  OVM_TRY(g, plan_encoder_tables(g, pl.get()));
  OVM_TRY(g, plan_scratch(g, pl.get()));
  if (pl->tune.fold()) OVM_TRY(g, plan_offset_tables(g, pl.get()));      // after the scratch: the GEMM may split K through the plan's workspace
  *out = pl.release();
  return OVM_OK;
}

Plan* find_plan(OvmGdino* g, int H, int W, const std::vector<int>& ids, const std::vector<int>& pids) {
  for (auto it = g->plans.begin(); it != g->plans.end(); ++it) {
    Plan* p = *it;
    if (p->H == H && p->W == W && p->ids == ids && p->pids == pids) { g->plans.erase(it); return p; }
  }
  return nullptr;
}

std::shared_ptr<TextEntry> find_text(OvmGdino* g, const std::vector<int>& ids, const std::vector<int>& pids, unsigned long gen) {
  for (auto it = g->texts.begin(); it != g->texts.end(); ++it) {
    if ((*it)->gen == gen && (*it)->ids == ids && (*it)->pids == pids) {
      std::shared_ptr<TextEntry> e = *it;
      g->texts.erase(it); g->texts.push_front(e);
      return e;
    }
  }
  return nullptr;
}

// Entries that leave the list live on while a plan holds them; the last owner's release frees the buffers (hipFree waits for the device).
void keep_text(OvmGdino* g, const std::shared_ptr<TextEntry>& e, int cap) {
  g->texts.push_front(e);
  while ((int)g->texts.size() > (cap > 1 ? cap : 1)) g->texts.pop_back();
}

size_t text_bytes(const OvmGdino* g, const Plan* incoming) {
  std::set<const TextEntry*> seen;
  size_t b = 0;
  auto add = [&](const std::shared_ptr<TextEntry>& e) { if (e && seen.insert(e.get()).second) b += e->bytes; };
  for (const auto& e : g->texts) add(e);
  for (const Plan* q : g->plans) add(q->text);
  if (incoming) add(incoming->text);
  return b;
}

// Least recently used plans go when the count or - what matters on a dataset with many aspect ratios - the bytes they hold
// together with the incoming plan exceed the configured bounds (defaults: 128 plans, 32 GiB of the 288 GB).
void evict_plans(OvmGdino* g, const Plan* incoming) {
  const int maxp = g->cfg.max_plans > 0 ? g->cfg.max_plans : 128;
  const size_t budget = (size_t)(g->cfg.plan_budget_mb > 0 ? g->cfg.plan_budget_mb : 32768) << 20;
  size_t held = incoming->bytes + text_bytes(g, incoming);      // caption entries once (they are small; an evicted plan's may stay held by the handle)
  for (Plan* q : g->plans) held += q->bytes;
  while (!g->plans.empty() && ((int)g->plans.size() >= maxp || held > budget)) {
    (void)hipDeviceSynchronize();
    held -= g->plans.back()->bytes;
    delete g->plans.back(); g->plans.pop_back();
  }
}

// Captured right after the first (eager) run of a plan, so every later call of this shape replays; a failed capture leaves the
// eager path in place (same results).
void capture_plan(OvmGdino* g, Plan* pl, hipStream_t s) {
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    Run cap{g, pl, s, false};
    const int r = forward_impl(cap);
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (r == OVM_OK && e == hipSuccess && graph) {
      hipGraphExec_t ex = nullptr;
      if (hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) == hipSuccess) { pl->graph = graph; pl->exec = ex; }
      else (void)hipGraphDestroy(graph);
    } else if (graph) {
      (void)hipGraphDestroy(graph);
    }
    g->err.clear();
  }
  (void)hipGetLastError();
}

}  // namespace gdino
}  // namespace ovm
