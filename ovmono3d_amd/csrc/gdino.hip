// Native GroundingDINO engine: the network `ROIHeads3DGDINO` calls at reference cubercnn/modeling/roi_heads/roi_heads_gdino.py:186
// (built at :16-23 from configs/GroundingDINO_SwinB_cfg.py; IDEA-Research/GroundingDINO @856dde2, source not in the reference
// tree), sequenced in C++ behind ovm_gdino_create / ovm_gdino_forward / ovm_gdino_detect / ovm_infer.
//
// BERT text encoder -> Swin backbone -> input projections -> 6 x (image<->text fusion, text enhancer, multi-scale deformable
// self-attention) -> two-stage query selection -> 6 x decoder -> contrastive class logits + boxes. Module structure and parameter
// names follow the Hugging Face port (the independent implementation the parity tests compare against).
//
// Execution model. Everything that depends only on (image size, caption) - index maps of the window partition / shift / patch
// merging, shift masks, sine position embeddings, reference grids, text masks - is built on the host once per *plan* and uploaded
// (gdino_plan.hip). A plan also owns the activation arena (sized by a dry pass over the same code) and every scratch buffer, so nothing
// is allocated, freed or re-sized on the hot path, and the whole forward is captured into ONE HIP graph per plan, replayed afterwards.
// What depends on the caption and the weights alone - BERT, the text projection, encoder layer 0's text norm and text projection - is
// computed once per caption, outside the graph (encode_caption -> a TextEntry the handle keeps and the caption's plans co-own,
// gdino_model.hpp); the per-image forward starts at the Swin backbone and reads the entry. ovm_tune_set gdino_text_cache 0 puts
// these ops back into every forward (text_encoder, fusion_layer), the same kernels on the same operands in the same order.
// This file: forward_impl, one stage function per part of the network, and the extern "C" entry points (types: gdino_model.hpp;
// weights: gdino_load.hip).
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "det2d.hpp"
#include "dec_chain.hpp"
#include "gdino_model.hpp"

using namespace ovm;
using namespace ovm::gdino;

namespace ovm {
GdinoTune g_gdino_tune = {1, 1, 0, 1, 1, 1, 0, 0, 0, 16}; // branches, dec_chain, ffn_split, swin_fused, gemm256, mlp_fused, swin_tap, enc_fold, enc_tap, text_cache
namespace { std::atomic<unsigned long> g_tune_generation{0}; }
unsigned long tune_generation() { return g_tune_generation.load(); }
void bump_tune_generation() { ++g_tune_generation; }
void set_gdino_branches(int v) { g_gdino_tune.branches = v ? 1 : 0; }       // engines created afterwards
void set_gdino_dec_chain(int v) { g_gdino_tune.dec_chain = v ? 1 : 0; }     // this and the ones below: plans built afterwards
void set_gdino_ffn_split(int v) { g_gdino_tune.ffn_split = v ? 1 : 0; }
void set_gdino_swin_fused(int v) { g_gdino_tune.swin_fused = v ? 1 : 0; }
void set_gdino_swin_tap(int v) { g_gdino_tune.swin_tap = v > 0 ? v : 0; }
void set_gdino_gemm256(int v) { g_gdino_tune.gemm256 = v ? 1 : 0; }
void set_gdino_mlp_fused(int v) { g_gdino_tune.mlp_fused = v < 0 ? 0 : (v > 2 ? 2 : v); }
void set_gdino_enc_fold(int v) { g_gdino_tune.enc_fold = (v < 0 || v > 3) ? 0 : v; }
void set_gdino_enc_tap(int v) { g_gdino_tune.enc_tap = v ? 1 : 0; }
void set_gdino_text_cache(int v) { g_gdino_tune.text_cache = v < 0 ? 0 : (v > 4096 ? 4096 : v); }
}  // namespace ovm

namespace ovm {
namespace gdino {
namespace {

// ---- buffers that cross stages (arena pointers; the order they are allocated in is the arena's layout)
struct Feat { float* f; int h, w, C; SplitBuf sp; };     // sp: the rows as the neck's projection takes them (tune.prod_split())
struct DecScratch {                                        // shared by the decoder layers and the heads
  float *tkv_all, *val_all;                                // all layers' text keys | values [T][NL 2 D], deformable values of the memory [S][NL D]
  float *sine, *qh, *qpos, *qk, *vq, *ctx, *pre, *ow, *ffb, *b1, *b2, *delta;
  float* refs[2];                                          // reference boxes, ping-pong over the layers
  bool chain; int ffn_chunks;                              // row-chain form; > 0: with the FFN split into that many chunks
  float *ffn_x, *ffn_part;
};
struct State {
  float *tx, *text0, *text;                                // BERT output, projected text features (kept intact for the debug tap), encoder text output
  std::vector<Feat> feats;                                 // Swin output stages
  float *vis0, *vis;                                       // projected image features, encoder state / output
  SplitBuf dec_vsp;                                        // tune.prod_split(): the encoder output as dec_value's A operand
  float* ref; int* topk;                                   // two-stage selection
  float *hs, *last_ref, *hn;                               // decoder state, the last layer's reference boxes, normalised state
  DecScratch d;
};

inline int now_cols(const OvmGdinoConfig& c) { return c.heads * c.n_levels * c.n_points * 3; }      // [offsets x, y | logits] per (head, level, point)

// multi-head attention over fp32 rows: q [Tq][D] (at qp, stride ldq), k / v likewise
void mha_core(Run& r, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int Tq, int Tk, int heads, int D, const float* bias,
              int ldb, float* out, int ldo) {
  AttnF32Params a; memset(&a, 0, sizeof(a));
  const int dh = D / heads;
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.sq2 = dh; a.sk2 = dh; a.sv2 = dh; a.o = out; a.ldo = ldo; a.so2 = dh;
  a.nb1 = 1; a.nb2 = heads; a.Tq = Tq; a.Tk = Tk; a.DH = dh; a.scale = 1.0f / sqrtf((float)dh);
  a.bias_b = bias; a.sbb = 0; a.ldbb = ldb;
  r.attn(a);
}

void deform(Run& r, const float* value, int ldv, const float* ow, int ldow, const float* ref, int ldref, int mode, int Q, float* out,
            const SplitBuf* osp) {
  if (!r.go()) return;
  const OvmGdinoConfig& c = r.g->cfg;
  MsDeformParams p; memset(&p, 0, sizeof(p));
  p.value = value; p.ldv = ldv; p.ow = ow; p.ldow = ldow; p.ref = ref; p.ldref = ldref; p.mode = mode;
  p.Q = Q; p.H = c.heads; p.dh = c.d_model / c.heads; p.L = c.n_levels; p.P = c.n_points;
  for (int l = 0; l < c.n_levels; ++l) { p.lh[l] = r.pl->lh[l]; p.lw[l] = r.pl->lw[l]; p.lstart[l] = r.pl->lstart[l]; }
  p.out = out; p.ldo = c.d_model;
  if (osp) { p.ohi = osp->hi; p.olo = osp->lo; p.ldoh = osp->ld; }
  r.chk(launch_msdeform_fused(p, r.s), "msdeform");
}

// =============================== text: BERT + projection ===============================
// BERT over the caption into tx [T][bertD], then the text projection into text0 [T][d_model] (null: taken from the arena, after
// BERT's scratch); returns text0. Scratch comes from the run's arena and stays allocated.
float* bert_chain(Run& r, float* tx, float* text0) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const int T = pl->T, D = g->cfg.d_model, BD = g->bertD, BH = g->cfg.bert_heads;
  if (r.go()) r.chk(launch_bert_embed(g->word, g->posemb, g->typemb, pl->d_ids, pl->d_pids, T, BD, g->emb_ln.g, g->emb_ln.b, 1e-12f, tx, r.s), "bert_embed");
  float* qkv = r.f32((size_t)T * 3 * BD);
  float* ctx = r.f32((size_t)T * BD);
  float* a = r.f32((size_t)T * BD);
  float* hbuf = r.f32((size_t)T * 4 * BD);
  for (auto& ly : g->bert) {
    r.lin(tx, nullptr, BD, T, ly.qkv, 0, nullptr, 0, qkv, 3 * BD);
    mha_core(r, qkv, 3 * BD, qkv + BD, 3 * BD, qkv + 2 * BD, 3 * BD, T, T, BH, BD, pl->text_bias, T, ctx, BD);
    r.lin(ctx, nullptr, BD, T, ly.ao, 0, nullptr, 0, a, BD);
    r.ln(a, T, BD, ly.aln, 1e-12f, tx, tx);
    r.lin(tx, nullptr, BD, T, ly.fi, 2, nullptr, 0, hbuf, ly.fi.N);
    r.lin(hbuf, nullptr, ly.fi.N, T, ly.fo, 0, nullptr, 0, a, BD);
    r.ln(a, T, BD, ly.oln, 1e-12f, tx, tx);
  }
  if (!text0) text0 = r.f32((size_t)T * D);
  r.lin(tx, nullptr, BD, T, g->text_proj, 0, nullptr, 0, text0, D);
  return text0;
}

// With a caption entry (tune.text_cache): nothing is launched, the forward reads the entry. Otherwise the text branch: BERT and the
// projection run beside the Swin backbone and the neck, joined before the encoder.
void text_encoder(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const int T = pl->T, D = g->cfg.d_model, BD = g->bertD;
  if (pl->tune.text_cache) {
    if (!pl->text && !r.dry) { r.fail(OVM_ERR_INVALID, "text_encoder: the plan has no caption entry"); return; }
    st.tx = pl->text ? pl->text->tx : nullptr; st.text0 = pl->text ? pl->text->text0 : nullptr;
  } else {
    st.tx = r.f32((size_t)T * BD);
    r.fork(); r.on_text();
    st.text0 = bert_chain(r, st.tx, nullptr);
  }
  r.tap("bert_out", st.tx, (int64_t)T * BD);
  r.tap("text_features", st.text0, (int64_t)T * D);
  st.text = r.f32((size_t)T * D);                         // encoder output (the input above stays intact for the debug tap)
  r.on_image();
}

// =============================== image: Swin backbone ===============================
// one block on the residual stream x [ntok][C]: (shifted) window attention, then the FFN
void swin_block(Run& r, const SwinBlock& blk, const WinMaps& wmaps, float* x, int C, int nh, int ntok, int ordinal) {
  const OvmGdinoConfig& c = r.g->cfg;
  const int ws = c.swin_window, ws2 = ws * ws, dh = C / nh, nW = wmaps.nW, M = nW * ws2, precision = r.g->precision;
  const float eps = c.eps;
  // tests (ovm_tune_set gdino_swin_tap): copies of this block's window rows and context rows that outlive the block's scratch
  half_t* snap[4] = {nullptr, nullptr, nullptr, nullptr};
  const size_t snap_bytes = (size_t)M * ((C + 63) / 64 * 64) * sizeof(half_t);
  if (r.pl->tune.swin_tap == ordinal && precision == 3) for (half_t*& q : snap) q = (half_t*)r.alloc(snap_bytes);
  const size_t mk = r.mark();
  // LN1 + pad + cyclic shift + window partition -> split fp16 rows (padding rows are zero AFTER the norm)
  SplitBuf xw = r.split((size_t)M, C);
  {
    RowOpParams p = Run::rows(x, C, M, C); Run::into(p, xw);
    p.idx = wmaps.win; p.nidx = 1; p.seg = C; p.gamma = blk.ln1.g; p.beta = blk.ln1.b; p.eps = eps; p.zero_masked = 1;
    r.rowop(p);
  }
  SplitBuf ctx = r.split((size_t)M, C);
  if (r.pl->tune.swin_fused && blk.qkv.frag && dh == 32 && swin_qkv_attn_supported(C, nh, ws, precision) && xw.ld % 8 == 0) {
    // qkv projection inside the window kernel (one workgroup per (window, head); per (windows, head) at ws = 7): no [M][3 C] fp32 round
    // trip, one launch less
    SwinQkvAttnParams a; memset(&a, 0, sizeof(a));
    a.xhi = xw.hi; a.xlo = xw.lo; a.ldx = xw.ld; a.wfrag = blk.qkv.frag; a.KS = blk.qkv.Kpad / 32; a.bias = blk.qkv.bias;
    a.C = C; a.nh = nh; a.nW = nW; a.relbias = blk.relbias; a.mask = wmaps.mask; a.ohi = ctx.hi; a.olo = ctx.lo; a.ldo = ctx.ld;
    a.scale = 1.0f / sqrtf((float)dh); a.ws = ws;
    if (r.go()) r.chk(launch_swin_qkv_attn(a, r.s_main), "swin_qkv_attn");
    if (snap[0]) {
      r.copy(snap[0], xw.hi, snap_bytes, r.s_main); r.copy(snap[1], xw.lo, snap_bytes, r.s_main);
      r.copy(snap[2], ctx.hi, snap_bytes, r.s_main); r.copy(snap[3], ctx.lo, snap_bytes, r.s_main);
      const int64_t nrow = (int64_t)(snap_bytes / 4);                     // debug copies count 4-byte elements
      r.tap("swin_tap_xhi", snap[0], nrow); r.tap("swin_tap_xlo", snap[1], nrow);
      r.tap("swin_tap_ohi", snap[2], nrow); r.tap("swin_tap_olo", snap[3], nrow);
      r.tap("swin_tap_wfrag", blk.qkv.frag, (int64_t)npad128(blk.qkv.N) * 2 * blk.qkv.Kpad / 2);
      r.tap("swin_tap_bias", blk.qkv.bias, 3 * C);
      r.tap("swin_tap_relbias", blk.relbias, (int64_t)nh * ws2 * ws2);
      if (wmaps.mask) r.tap("swin_tap_mask", wmaps.mask, (int64_t)nW * ws2 * ws2);
    }
  } else {
    float* qkv = r.f32((size_t)M * 3 * C);
    { GemmParams q = r.gp(xw, M, blk.qkv); q.C = qkv; q.ldc = 3 * C; r.gemm(q, EPI_STORE); }
    // window attention: QK^T + relative-position bias + shift mask + softmax + PV, one workgroup per (window, head)
    AttnF32Params a; memset(&a, 0, sizeof(a));
    a.q = qkv; a.k = qkv + C; a.v = qkv + 2 * C; a.ldq = a.ldk = a.ldv = 3 * C;
    a.sq1 = a.sk1 = a.sv1 = (long)ws2 * 3 * C; a.sq2 = a.sk2 = a.sv2 = dh;
    a.ohi = ctx.hi; a.olo = ctx.lo; a.ldoh = ctx.ld; a.soh1 = (long)ws2 * ctx.ld; a.soh2 = dh;
    a.nb1 = nW; a.nb2 = nh; a.Tq = ws2; a.Tk = ws2; a.DH = dh; a.scale = 1.0f / sqrtf((float)dh);
    a.bias_h = blk.relbias; a.sbh = (long)ws2 * ws2; a.ldbh = ws2;
    a.bias_b = wmaps.mask; a.sbb = (long)ws2 * ws2; a.ldbb = ws2;
    r.attn(a);
  }
  // output projection; the epilogue un-partitions / un-shifts / crops through the same index map and adds the shortcut
  { GemmParams q = r.gp(ctx, M, blk.proj); q.X = x; q.ldx = C; q.row_map = wmaps.win; r.gemm(q, EPI_RESID); }
  if (r.mlp_fused_ok(1, ntok, blk.fc1, blk.fc2, 2)) {
    // fc1, GELU and fc2's k-slices in one kernel, then the reduce fc2 ends in anyway: no f1 image, one launch of fat workgroups less
    SplitBuf hn = r.split_il((size_t)ntok, C);
    r.ln(x, ntok, C, blk.ln2, eps, nullptr, nullptr, &hn);
    GemmParams q = r.gp(hn, ntok, blk.fc2); q.X = x; q.ldx = C;
    r.mlp_fused(hn, ntok, blk.fc1, blk.fc2, 2, q, EPI_RESID);
    r.release(mk);
    return;
  }
  // stage 1 (17,689 tokens x 512 outputs over K = 128: 556 tiles of 128 x 128, or 140 of 256 x 256 in one round): interleaved rows
  const bool wide = ((ntok + 127) / 128) * ((4 * C + 127) / 128) > 512 && (4 * C) % 256 == 0;
  SplitBuf hn = wide ? r.split_for256((size_t)ntok, C) : r.split((size_t)ntok, C);
  r.ln(x, ntok, C, blk.ln2, eps, nullptr, nullptr, &hn);
  SplitBuf f1 = r.split((size_t)ntok, 4 * C);
  { GemmParams q = r.gp(hn, ntok, blk.fc1); q.Ohi = f1.hi; q.Olo = f1.lo; q.ldo = f1.ld; r.gemm(q, EPI_GELU); }
  { GemmParams q = r.gp(f1, ntok, blk.fc2); q.X = x; q.ldx = C; r.gemm(q, EPI_RESID); }
  r.release(mk);
}

// 2 x 2 neighbourhoods -> LayerNorm -> reduction to 2 C: the next stage's residual stream
float* patch_merge(Run& r, const SwinStage& stg, const StageGeo& ge, const float* x, int C) {
  const int h2 = ge.h2, w2 = ge.w2;
  float* xn = r.f32((size_t)h2 * w2 * 2 * C);
  const size_t mk = r.mark();
  SplitBuf xm = r.split((size_t)h2 * w2, 4 * C);
  RowOpParams p = Run::rows(x, C, h2 * w2, 4 * C); Run::into(p, xm);
  p.idx = ge.merge; p.nidx = 4; p.seg = C; p.gamma = stg.dn.g; p.beta = stg.dn.b; p.eps = r.g->cfg.eps;
  r.rowop(p);
  GemmParams q = r.gp(xm, h2 * w2, stg.red); q.C = xn; q.ldc = 2 * C;
  r.gemm(q, EPI_STORE);
  r.release(mk);
  return xn;
}

void swin_backbone(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const float eps = g->cfg.eps;
  int h = pl->Hp, w = pl->Wp, C = g->stages[0].C;
  // residual streams of the stages live for the whole backbone (the output norms read them at the end of each stage)
  float* x = r.f32((size_t)h * w * C);
  {
    const size_t mk = r.mark();
    SplitBuf pa = r.split((size_t)h * w, 48);
    RowOpParams p = Run::rows(pl->img, 3, h * w, 48); Run::into(p, pa);
    p.idx = pl->pe_map; p.nidx = 16; p.seg = 3;
    r.rowop(p);
    float* y = r.f32((size_t)h * w * C);
    GemmParams q = r.gp(pa, h * w, g->pe); q.C = y; q.ldc = C;
    r.gemm(q, EPI_STORE);
    r.ln(y, h * w, C, g->pe_ln, eps, nullptr, x);
    r.release(mk);
  }
  int ordinal = 0;                                          // Swin blocks so far, 1-based inside swin_block
  for (size_t si = 0; si < g->stages.size(); ++si) {
    const SwinStage& stg = g->stages[si];
    const StageGeo& ge = pl->geo[si];
    const int ntok = h * w;
    for (size_t b = 0; b < stg.blocks.size(); ++b) swin_block(r, stg.blocks[b], ge.wm[b & 1], x, C, stg.nh, ntok, ++ordinal);
    if (stg.has_out) {
      float* f = r.f32((size_t)ntok * C);
      // the neck projects the level straight from these rows: the norm writes them split as well (they live until the neck, like f,
      // which stays for the tap and for the extra level's 3 x 3 gather)
      SplitBuf sp;
      if (pl->tune.prod_split() && (int)st.feats.size() < g->cfg.n_levels) sp = r.split((size_t)ntok, C);
      r.ln(x, ntok, C, stg.on, eps, nullptr, f, sp.hi ? &sp : nullptr);
      st.feats.push_back({f, h, w, C, sp});
      r.tap("swin_stage" + std::to_string(st.feats.size()), f, (int64_t)ntok * C);
    }
    if (stg.has_red) { x = patch_merge(r, stg, ge, x, C); h = ge.h2; w = ge.w2; C = 2 * C; }
  }
}

// =============================== neck: input projections + GroupNorm ===============================
void neck(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, S = pl->S;
  st.vis0 = r.f32((size_t)S * D);
  st.vis = r.f32((size_t)S * D);                          // encoder state / output
  const size_t mk = r.mark();
  for (int l = 0; l < c.n_levels; ++l) {
    const int n = pl->lh[l] * pl->lw[l];
    float* y = r.f32((size_t)n * D);
    const bool conv = l >= (int)st.feats.size();          // the extra level: 3x3 stride-2 convolution of the last stage, rows gathered through the im2col map
    const Feat& f = conv ? st.feats.back() : st.feats[l];
    const int K = conv ? 9 * f.C : f.C;
    SplitBuf a = f.sp;
    if (conv || !a.hi) {
      a = r.split((size_t)n, K);
      RowOpParams p = Run::rows(f.f, f.C, n, K); Run::into(p, a);
      if (conv) { p.idx = pl->conv_map; p.nidx = 9; p.seg = f.C; }
      r.rowop(p);
    }
    GemmParams q = r.gp(a, n, g->inproj[l].w); q.C = y; q.ldc = D;
    r.gemm(q, EPI_STORE);
    if (r.go()) r.chk(ovm_g_groupnorm(y, 1, n, D, 32, g->inproj[l].gn.g, g->inproj[l].gn.b, 1e-5f, st.vis0 + (size_t)pl->lstart[l] * D, r.s_main), "groupnorm");
  }
  r.release(mk);
}

// =============================== encoder ===============================
struct EncBufs {
  float* v; SplitBuf vsp; float *t, *qvv, *tkv; SplitBuf cv; float* ct;
  BiAttnWs bw; float *sc, *stat, *part, *bml;
  float *text2, *tqk, *tv, *tctx, *tff;
  SplitBuf vis_sp, visp_sp; float *val, *ow; SplitBuf dsp; float* pre; SplitBuf ff;
  float* voff;                                             // tune.fold(): [value | offsets | logits] rows [S][D + NOW] in place of visp_sp, val, ow
  float *tap_vis = nullptr, *tap_voff = nullptr; half_t *tap_hi = nullptr, *tap_lo = nullptr;   // tune.enc_tap: layer 0's copies
  bool ffn_fused;                                          // the layers' FFN on the fused route (ff is not allocated then)
};

// bi-directional image <-> text attention; leaves the two contexts (cv, ct) and the normalised inputs (v, t) for the halves below.
// `te`: layer 0 with a caption entry - its normalised text rows and their projection are the entry's (text_in is text0), not computed here
void fusion_layer(Run& r, const EncLayer& ly, EncBufs& b, const float* vis_in, const float* text_in, const TextEntry* te) {
  const OvmGdinoConfig& c = r.g->cfg;
  const int D = c.d_model, T = r.pl->T, S = r.pl->S, HF = c.heads / 2, E = c.ffn_dim / 2, dhf = E / HF;
  r.ln(vis_in, S, D, ly.lnv, c.eps, nullptr, b.v, &b.vsp);
  if (!te) r.ln(text_in, T, D, ly.lnt, c.eps, nullptr, b.t);
  { GemmParams q = r.gp(b.vsp, S, ly.vqv); q.C = b.qvv; q.ldc = 2 * E; r.gemm(q, EPI_STORE); }
  if (!te) r.lin(b.t, nullptr, D, T, ly.tkv, 0, nullptr, 0, b.tkv, 2 * E);
  if (!r.go()) return;
  const float* tkv = te ? te->tkv0 : b.tkv;
  BiAttnParams a; memset(&a, 0, sizeof(a));
  a.qv = b.qvv; a.ldq = 2 * E; a.kt = tkv; a.ldk = 2 * E; a.vv = b.qvv + E; a.ldvv = 2 * E; a.vt = tkv + E; a.ldvt = 2 * E;
  a.S = S; a.T = T; a.H = HF; a.dh = dhf; a.scale = 1.0f / sqrtf((float)dhf);
  a.cv_hi = b.cv.hi; a.cv_lo = b.cv.lo; a.ldcv = b.cv.ld; a.ct = b.ct; a.sc = b.sc; a.stat = b.stat; a.part = b.part; a.chunk = b.bw.chunk; a.nchunk = b.bw.nchunk;
  if (b.bml) { a.bm = b.bml; a.bl = b.bml + b.bw.ml; }
  r.chk(launch_biattn(a, r.s_main), "biattn"); r.launches += b.bw.mfma ? 1 : 3;
}

// text half of a layer, on the text branch: the fusion's gated text output, then the text enhancer -> text
// `t_in`: the layer's normalised text input, the shortcut of the gated output (b.t, or the caption entry's rows for layer 0; b.t is
// rewritten further down, the entry never is)
void text_enhancer(Run& r, const EncLayer& ly, EncBufs& b, float* text, const float* t_in) {
  const OvmGdinoConfig& c = r.g->cfg;
  const int D = c.d_model, T = r.pl->T, E = c.ffn_dim / 2;
  r.fork(); r.on_text();
  r.lin(b.ct, nullptr, E, T, ly.ot, 0, t_in, D, b.text2, D);
  r.lin(b.text2, r.pl->text_pos, D, T, ly.te.qk, 0, nullptr, 0, b.tqk, 2 * D);
  r.lin(b.text2, nullptr, D, T, ly.te.v, 0, nullptr, 0, b.tv, D);
  mha_core(r, b.tqk, 2 * D, b.tqk + D, 2 * D, b.tv, D, T, T, ly.te.heads, D, r.pl->text_bias, T, b.tctx, D);
  r.lin(b.tctx, nullptr, D, T, ly.te.out, 0, b.text2, D, b.t, D);
  r.ln(b.t, T, D, ly.te_ln1, c.eps, nullptr, b.text2);
  r.lin(b.text2, nullptr, D, T, ly.te_fc1, 1, nullptr, 0, b.tff, ly.te_fc1.N);
  r.lin(b.tff, nullptr, ly.te_fc1.N, T, ly.te_fc2, 0, b.text2, D, b.t, D);
  r.ln(b.t, T, D, ly.te_ln2, c.eps, nullptr, text);
  r.on_image();
}

// image half, on the main stream: the fusion's gated image output, deformable self-attention over the image tokens, FFN -> vis
// `li`: the layer's index; `out_sp`: split rows the final norm writes beside vis (the last layer's, for the decoder's value projection)
void deformable_layer(Run& r, const EncLayer& ly, EncBufs& b, float* vis, int li, const SplitBuf* out_sp) {
  const OvmGdinoConfig& c = r.g->cfg; Plan* pl = r.pl;
  const int D = c.d_model, S = pl->S, NOW = now_cols(c);
  if (pl->tune.fold()) {
    // the out-projection writes vis and its split rows; value and offsets projections read those rows as ONE GEMM over [value | offw],
    // whose epilogue adds the layer's table P = pos W_off^T + b_off to the offsets columns (n >= D): no row pass, no vis + pos image
    { GemmParams q = r.gp(b.cv, S, ly.ov); q.C = vis; q.ldc = D; q.R = b.v; q.ldr = D; q.Ohi = b.vis_sp.hi; q.Olo = b.vis_sp.lo; q.ldo = b.vis_sp.ld; r.gemm(q, EPI_STORE); }
    { GemmParams q = r.gp(b.vis_sp, S, ly.msda.voff); q.C = b.voff; q.ldc = D + NOW; q.R = pl->enc_P[li]; q.ldr = NOW; q.r_n0 = D; r.gemm(q, EPI_STORE); }
    deform(r, b.voff, D + NOW, b.voff + D, D + NOW, pl->ref, 2, 0, S, nullptr, &b.dsp);
  } else {
    { GemmParams q = r.gp(b.cv, S, ly.ov); q.C = vis; q.ldc = D; q.R = b.v; q.ldr = D; r.gemm(q, EPI_STORE); }
    {
      RowOpParams p = Run::rows(vis, D, S, D); Run::into(p, b.vis_sp);
      p.add = pl->pos; p.ld_add = D; p.add_rows = S; p.hi2 = b.visp_sp.hi; p.lo2 = b.visp_sp.lo; p.ldh2 = b.visp_sp.ld;
      r.rowop(p);
    }
    { GemmParams q = r.gp(b.vis_sp, S, ly.msda.value); q.C = b.val; q.ldc = D; r.gemm(q, EPI_STORE); }
    { GemmParams q = r.gp(b.visp_sp, S, ly.msda.offw); q.C = b.ow; q.ldc = NOW; r.gemm(q, EPI_STORE); }
    deform(r, b.val, D, b.ow, NOW, pl->ref, 2, 0, S, nullptr, &b.dsp);
  }
  if (li == 0 && b.tap_vis) {
    // tests (ovm_tune_set gdino_enc_tap): layer 0's out-projection rows, their split and the projections' outputs, copied before the later
    // layers reuse the buffers; debug copies count 4-byte elements
    const size_t nsp = (size_t)S * b.vis_sp.ld * sizeof(half_t);
    r.tap("enc_pos", pl->pos, (int64_t)S * D);
    r.copy(b.tap_vis, vis, sizeof(float) * (size_t)S * D, r.s_main); r.tap("enc_vis0", b.tap_vis, (int64_t)S * D);
    r.copy(b.tap_hi, b.vis_sp.hi, nsp, r.s_main); r.tap("enc_vis0_hi", b.tap_hi, (int64_t)(nsp / 4));
    if (b.vis_sp.lo) { r.copy(b.tap_lo, b.vis_sp.lo, nsp, r.s_main); r.tap("enc_vis0_lo", b.tap_lo, (int64_t)(nsp / 4)); }
    if (pl->tune.fold()) {
      r.copy(b.tap_voff, b.voff, sizeof(float) * (size_t)S * (D + NOW), r.s_main); r.tap("enc_voff0", b.tap_voff, (int64_t)S * (D + NOW));
      r.tap("enc_P0", pl->enc_P[0], (int64_t)S * NOW);
    } else {
      r.copy(b.tap_voff, b.val, sizeof(float) * (size_t)S * D, r.s_main); r.tap("enc_val0", b.tap_voff, (int64_t)S * D);
      r.copy(b.tap_voff + (size_t)S * D, b.ow, sizeof(float) * (size_t)S * NOW, r.s_main); r.tap("enc_ow0", b.tap_voff + (size_t)S * D, (int64_t)S * NOW);
    }
  }
  { GemmParams q = r.gp(b.dsp, S, ly.msda.out); q.C = b.pre; q.ldc = D; q.R = vis; q.ldr = D; r.gemm(q, EPI_STORE); }
  r.ln(b.pre, S, D, ly.de_ln1, c.eps, nullptr, b.v, &b.vsp);
  if (b.ffn_fused) {
    GemmParams q = r.gp(b.vsp, S, ly.de_fc2); q.C = b.pre; q.ldc = D; q.R = b.v; q.ldr = D;
    r.mlp_fused(b.vsp, S, ly.de_fc1, ly.de_fc2, 1, q, EPI_STORE);
  } else {
    { GemmParams q = r.gp(b.vsp, S, ly.de_fc1); q.Ohi = b.ff.hi; q.Olo = b.ff.lo; q.ldo = b.ff.ld; q.relu = 1; r.gemm(q, EPI_STORE); }
    { GemmParams q = r.gp(b.ff, S, ly.de_fc2); q.C = b.pre; q.ldc = D; q.R = b.v; q.ldr = D; r.gemm(q, EPI_STORE); }
  }
  r.ln(b.pre, S, D, ly.de_ln2, c.eps, nullptr, vis, out_sp);
}

void encoder(Run& r, State& st) {
  const OvmGdinoConfig& c = r.g->cfg;
  const int D = c.d_model, T = r.pl->T, S = r.pl->S, HF = c.heads / 2, E = c.ffn_dim / 2, dhf = E / HF;
  const int NOW = now_cols(c), NE = (int)r.g->enc.size();
  if (!r.pl->tune.text_cache) r.join();                   // text features and image features meet in the fusion layers (a caption entry: no text branch was forked so far)
  EncBufs b;
  // what outlives the encoder's scratch: the rows the last layer's final norm writes for the decoder's value projection, test copies
  if (r.pl->tune.prod_split() && NE > 0) st.dec_vsp = r.split_for256((size_t)S, D);
  if (r.pl->tune.enc_tap && NE > 0) {
    const size_t nsp = (size_t)S * ((D + 63) / 64 * 64) * sizeof(half_t);
    b.tap_vis = r.f32((size_t)S * D); b.tap_voff = r.f32((size_t)S * (D + NOW));
    b.tap_hi = (half_t*)r.alloc(nsp); b.tap_lo = (half_t*)r.alloc(nsp);
  }
  const size_t mk = r.mark();
  b.v = r.f32((size_t)S * D); b.vsp = r.split_for256((size_t)S, D);      // A of vqv / de_fc1: S x 2048 outputs over K = 256
  b.t = r.f32((size_t)T * D);
  b.qvv = r.f32((size_t)S * 2 * E);              // [vision_proj | values_vision_proj]
  b.tkv = r.f32((size_t)T * 2 * E);              // [text_proj | values_text_proj]
  b.cv = r.split((size_t)S, E);
  b.ct = r.f32((size_t)T * E);
  b.bw = biattn_workspace(S, T, HF, dhf, false);         // the matrix-core path needs neither sc nor stat
  b.sc = b.bw.sc ? r.f32(b.bw.sc) : nullptr;
  b.stat = b.bw.stat ? r.f32(b.bw.stat) : nullptr;
  b.part = r.f32(b.bw.part);
  b.bml = b.bw.ml ? r.f32(2 * b.bw.ml) : nullptr;
  b.text2 = r.f32((size_t)T * D);
  b.tqk = r.f32((size_t)T * 2 * D); b.tv = r.f32((size_t)T * D); b.tctx = r.f32((size_t)T * D);
  b.tff = r.f32((size_t)T * c.ffn_dim);
  b.vis_sp = r.split((size_t)S, D);
  b.val = b.ow = b.voff = nullptr;
  if (r.pl->tune.fold()) {
    if ((int)r.pl->enc_P.size() != NE || D % 4) { r.fail(OVM_ERR_INVALID, "encoder: the plan has no offsets tables"); return; }
    b.voff = r.f32((size_t)S * (D + NOW));                // value at column 0, offsets | logits at column D: both 16-byte aligned rows (D % 4 == 0)
  } else {
    b.visp_sp = r.split((size_t)S, D);
    b.val = r.f32((size_t)S * D);
    b.ow = r.f32((size_t)S * NOW);
  }
  b.dsp = r.split((size_t)S, D);
  b.pre = r.f32((size_t)S * D);
  b.ffn_fused = b.vsp.il;
  for (auto& ly : r.g->enc) b.ffn_fused = b.ffn_fused && r.mlp_fused_ok(2, S, ly.de_fc1, ly.de_fc2, 1);
  if (!b.ffn_fused) b.ff = r.split((size_t)S, c.ffn_dim);
  const float* vis_in = st.vis0; const float* text_in = st.text0;
  for (int li = 0; li < NE; ++li) {
    const EncLayer& ly = r.g->enc[li];
    const TextEntry* te = (li == 0 && r.pl->tune.text_cache) ? r.pl->text.get() : nullptr;
    if (li == 0 && r.pl->tune.text_cache && !te && !r.dry) { r.fail(OVM_ERR_INVALID, "encoder: the plan has no caption entry"); return; }
    fusion_layer(r, ly, b, vis_in, text_in, te);
    vis_in = st.vis; text_in = st.text;
    // the two halves of the layer from here on touch disjoint buffers: text side (ot, text enhancer -> text) on the text
    // branch, image side (ov, deformable self-attention, FFN -> vis) on the main one; joined at the end of the layer
    text_enhancer(r, ly, b, st.text, te ? te->t0 : b.t);
    deformable_layer(r, ly, b, st.vis, li, (li == NE - 1 && st.dec_vsp.hi) ? &st.dec_vsp : nullptr);
    r.join();
  }
  r.release(mk);
  r.tap("source_flatten", st.vis0, (int64_t)S * D);
  r.tap("enc_vision", st.vis, (int64_t)S * D);
  r.tap("enc_text", st.text, (int64_t)T * D);
}

// =============================== two-stage query selection ===============================
void select_queries(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, T = pl->T, S = pl->S, Q = c.num_queries;
  const hipStream_t s = r.s_main;
  float* ref = st.ref = r.f32((size_t)Q * 4);
  int* topk = st.topk = r.i32((size_t)Q);
  const size_t mk = r.mark();
  SplitBuf oqs = r.split((size_t)S, D);
  {
    RowOpParams p = Run::rows(st.vis, D, S, D); Run::into(p, oqs);
    p.idx = pl->valid_idx; p.nidx = 1; p.seg = D;
    r.rowop(p);                                                               // invalid proposals -> zero rows
  }
  float* oq0 = r.f32((size_t)S * D);
  { GemmParams q = r.gp(oqs, S, g->enc_output); q.C = oq0; q.ldc = D; r.gemm(q, EPI_STORE); }
  float* oq = r.f32((size_t)S * D);
  r.ln(oq0, S, D, g->enc_output_ln, c.eps, nullptr, oq, &oqs);
  float* cls = r.f32((size_t)S * T);
  if (r.go()) r.chk(ovm_g_bmm(oq, st.text, cls, 1, S, T, D, D, D, T, 0, 0, 0, 1, 1.0f, s), "bmm cls");
  float* mx = r.f32((size_t)S);
  if (r.go()) r.chk(ovm_g_rowmax(cls, S, T, T, mx, s), "rowmax");
  const int* sel = topk;
  if (g->force_topk) sel = g->force_topk;
  else if (r.go()) r.chk(launch_topk_keys(mx, S, Q, topk, pl->topk_keys, pl->topk_N, s), "topk");
  SplitBuf h1 = r.split((size_t)S, D), h2 = r.split((size_t)S, D);
  { GemmParams q = r.gp(oqs, S, g->enc_bbox[0]); q.Ohi = h1.hi; q.Olo = h1.lo; q.ldo = h1.ld; q.relu = 1; r.gemm(q, EPI_STORE); }
  { GemmParams q = r.gp(h1, S, g->enc_bbox[1]); q.Ohi = h2.hi; q.Olo = h2.lo; q.ldo = h2.ld; q.relu = 1; r.gemm(q, EPI_STORE); }
  float* coord = r.f32((size_t)S * 4);
  { GemmParams q = r.gp(h2, S, g->enc_bbox[2]); q.C = coord; q.ldc = 4; r.gemm(q, EPI_STORE); }
  if (r.go()) r.chk(launch_select_ref(coord, 4, pl->prop_logit, sel, Q, ref, s), "select_ref");
  if (g->force_topk) r.copy(topk, g->force_topk, sizeof(int) * Q, s);
  r.release(mk);
  r.tap("topk", topk, Q);
  r.tap("init_ref", ref, (int64_t)Q * 4);
}

// =============================== decoder ===============================
// State, the projections that do not depend on it (all layers at once: text keys | values, deformable values of the memory) and the
// scratch the layers and the heads share. Returns the arena mark the caller releases after the heads.
size_t decoder_inputs(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, T = pl->T, S = pl->S, Q = c.num_queries, NL = (int)g->dec.size();
  DecScratch& d = st.d;
  st.hs = r.f32((size_t)Q * D);
  st.last_ref = r.f32((size_t)Q * 4);
  st.hn = r.f32((size_t)Q * D);
  const size_t mk = r.mark();
  d.tkv_all = r.f32((size_t)T * NL * 2 * D);
  r.lin(st.text, nullptr, D, T, g->dec_kv_text, 0, nullptr, 0, d.tkv_all, NL * 2 * D);
  SplitBuf vsp = st.dec_vsp;                                // written by the encoder's last norm (tune.prod_split())
  if (!vsp.hi) {
    vsp = r.split_for256((size_t)S, D);
    RowOpParams p = Run::rows(st.vis, D, S, D); Run::into(p, vsp); r.rowop(p);
  }
  d.val_all = r.f32((size_t)S * NL * D);
  { GemmParams q = r.gp(vsp, S, g->dec_value); q.C = d.val_all; q.ldc = NL * D; r.gemm(q, EPI_STORE); }
  r.copy(st.hs, g->tgt, sizeof(float) * (size_t)Q * D, r.s_main);
  d.sine = r.f32((size_t)Q * 2 * D);
  d.qh = r.f32((size_t)Q * D); d.qpos = r.f32((size_t)Q * D);
  d.qk = r.f32((size_t)Q * 2 * D); d.vq = r.f32((size_t)Q * D); d.ctx = r.f32((size_t)Q * D);
  d.pre = r.f32((size_t)Q * D);
  d.ow = r.f32((size_t)Q * now_cols(c));
  d.ffb = r.f32((size_t)Q * c.ffn_dim);
  d.b1 = r.f32((size_t)Q * D); d.b2 = r.f32((size_t)Q * D); d.delta = r.f32((size_t)Q * 4);
  d.refs[0] = st.ref; d.refs[1] = r.f32((size_t)Q * 4);
  // Row-chain form of a layer (dec_chain.hip): everything but the query self-attention is local to a query row, so a workgroup
  // walks 16 rows through the whole layer in LDS - 3 launches per layer instead of ~35 (ovm_tune_set "gdino_dec_chain" 0: the
  // launch-per-op sequence, kept as the cross-check).
  d.chain = pl->tune.dec_chain && dec_chain_supported(D, c.heads, c.ffn_dim, c.n_levels, c.n_points, T, g->precision);
  const int chunks = c.ffn_dim > 512 ? c.ffn_dim / 512 : 1;
  d.ffn_chunks = (d.chain && pl->tune.ffn_split && chunks > 1) ? chunks : 0;
  d.ffn_x = d.ffn_chunks ? r.f32((size_t)Q * D) : nullptr;
  d.ffn_part = d.ffn_chunks ? r.f32((size_t)d.ffn_chunks * Q * D) : nullptr;
  return mk;
}

#ifdef OVM_DIAG
// diagnostic builds: timing ablations (env OVM_DEC_CHAIN_SKIP) and the in-kernel stamps of the first layer's chain A (OVM_DEC_CHAIN_STAMPS)
void diag_arm(Run& r, DecChainParams& dp, int layer) {
  if (const char* e = getenv("OVM_DEC_CHAIN_SKIP")) dp.dbg_skip = atoi(e);
  static unsigned long long* d_st = nullptr;
  if (getenv("OVM_DEC_CHAIN_STAMPS") && layer == 0 && !r.dry) {
    if (!d_st) { (void)hipMalloc((void**)&d_st, 96 * 8); }
    (void)hipMemsetAsync(d_st, 0, 96 * 8, r.s_main);
    dp.dbg_stamps = d_st;
  }
}
void diag_report(Run& r, const DecChainParams& dp) {
  if (!dp.dbg_stamps || !r.go()) return;
  unsigned long long hst[96];
  (void)hipStreamSynchronize(r.s_main);
  (void)hipMemcpy(hst, dp.dbg_stamps, sizeof(hst), hipMemcpyDeviceToHost);
  fprintf(stderr, "[dec_chain_a stamps, cycles since entry]");
  for (int k = 1; k < 32 && hst[k]; ++k) fprintf(stderr, " %llu", hst[k] - hst[0]);
  fprintf(stderr, "\n");
}
#else
inline void diag_arm(Run&, DecChainParams&, int) {}
inline void diag_report(Run&, const DecChainParams&) {}
#endif

DecChainParams chain_params(Run& r, const State& st, int i, const float* rf, float* rf_next) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, NL = (int)g->dec.size();
  const DecScratch& d = st.d;
  const DecLayer& ly = g->dec[i];
  auto cl = [](const Lin& w) { return ChainLin{w.frag, w.bias, w.N, w.K, w.Kpad}; };
  auto cn = [](const Ln& w) { return ChainLn{w.g, w.b}; };
  DecChainParams dp; memset(&dp, 0, sizeof(dp));
  if (d.ffn_chunks) { dp.ffn_split = d.ffn_chunks; dp.ffn_x = d.ffn_x; dp.ffn_part = d.ffn_part; }
  dp.Q = c.num_queries; dp.D = D; dp.T = pl->T; dp.heads = c.heads; dp.ffn = c.ffn_dim; dp.eps = c.eps;
  dp.sine_dim_t = g->sine_dim_t;
  dp.hs = st.hs; dp.ref = rf; dp.ref_next = rf_next;
  dp.qpos = d.qpos; dp.qk = d.qk; dp.v = d.vq; dp.ctx = d.ctx;
  dp.tk = d.tkv_all + (size_t)i * 2 * D; dp.tv = dp.tk + D; dp.ldt = NL * 2 * D;
  dp.val = d.val_all + (size_t)i * D; dp.ldv = NL * D;
  dp.L = c.n_levels; dp.P = c.n_points;
  for (int l = 0; l < c.n_levels; ++l) { dp.lh[l] = pl->lh[l]; dp.lw[l] = pl->lw[l]; dp.lstart[l] = pl->lstart[l]; }
  dp.ref0 = cl(g->ref_head[0]); dp.ref1 = cl(g->ref_head[1]); dp.sa_qk = cl(ly.sa.qk); dp.sa_v = cl(ly.sa.v); dp.sa_out = cl(ly.sa.out);
  dp.ca_q = cl(ly.ca.q); dp.ca_out = cl(ly.ca.out); dp.offw = cl(ly.msda.offw); dp.msda_out = cl(ly.msda.out);
  dp.fc1 = cl(ly.fc1); dp.fc2 = cl(ly.fc2);
  if (i + 1 < NL) { dp.bb0 = cl(g->bbox[i][0]); dp.bb1 = cl(g->bbox[i][1]); dp.bb2 = cl(g->bbox[i][2]); }
  dp.ln1 = cn(ly.ln1); dp.ln2 = cn(ly.ln2); dp.ln3 = cn(ly.ln3); dp.ln4 = cn(ly.ln4);
  return dp;
}

// the last layer's reference boxes (the heads refine them) and the layer's debug tap
void layer_done(Run& r, State& st, int i, int NL, const float* rf) {
  const int Q = r.g->cfg.num_queries;
  if (i == NL - 1) r.copy(st.last_ref, rf, sizeof(float) * (size_t)Q * 4, r.s_main);
  r.tap("dec_hs" + std::to_string(i), st.hs, (int64_t)Q * r.g->cfg.d_model);
}

void decoder_chain(Run& r, State& st) {
  const int D = r.g->cfg.d_model, Q = r.g->cfg.num_queries, NL = (int)r.g->dec.size();
  const hipStream_t s = r.s_main;
  DecScratch& d = st.d;
  int cur = 0;
  for (int i = 0; i < NL; ++i) {
    float* rf = d.refs[cur];
    DecChainParams dp = chain_params(r, st, i, rf, (i + 1 < NL) ? d.refs[cur ^ 1] : nullptr);
    diag_arm(r, dp, i);
    if (r.go()) r.chk(launch_dec_chain(dp, 0, s), "dec_chain_a");
    diag_report(r, dp);
    mha_core(r, d.qk, 2 * D, d.qk + D, 2 * D, d.vq, D, Q, Q, r.g->dec[i].sa.heads, D, nullptr, 0, d.ctx, D);
    if (r.go()) r.chk(launch_dec_chain(dp, 1, s), "dec_chain_b");
    if (d.ffn_chunks && r.go()) r.chk(launch_dec_chain(dp, 2, s), "dec_chain_c");
    layer_done(r, st, i, NL, rf);
    if (i + 1 < NL) cur ^= 1;
  }
}

void decoder_per_op(Run& r, State& st) {
  OvmGdino* g = r.g;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, T = r.pl->T, Q = c.num_queries, NL = (int)g->dec.size(), NOW = now_cols(c);
  const float eps = c.eps;
  const hipStream_t s = r.s_main;
  DecScratch& d = st.d;
  float* hs = st.hs;
  int cur = 0;
  for (int i = 0; i < NL; ++i) {
    const DecLayer& ly = g->dec[i];
    float* rf = d.refs[cur];
    const float* tk = d.tkv_all + (size_t)i * 2 * D;
    if (r.go()) r.chk(ovm_g_sine_embed(rf, Q, 4, D / 2, 10000.0f, d.sine, s), "sine_embed");
    r.lin(d.sine, nullptr, 2 * D, Q, g->ref_head[0], 1, nullptr, 0, d.qh, D);
    r.lin(d.qh, nullptr, D, Q, g->ref_head[1], 0, nullptr, 0, d.qpos, D);
    // self-attention
    r.lin(hs, d.qpos, D, Q, ly.sa.qk, 0, nullptr, 0, d.qk, 2 * D);
    r.lin(hs, nullptr, D, Q, ly.sa.v, 0, nullptr, 0, d.vq, D);
    mha_core(r, d.qk, 2 * D, d.qk + D, 2 * D, d.vq, D, Q, Q, ly.sa.heads, D, nullptr, 0, d.ctx, D);
    r.lin(d.ctx, nullptr, D, Q, ly.sa.out, 0, hs, D, d.pre, D);
    r.ln(d.pre, Q, D, ly.ln1, eps, nullptr, hs);
    // text cross-attention
    r.lin(hs, d.qpos, D, Q, ly.ca.q, 0, nullptr, 0, d.qk, D);
    mha_core(r, d.qk, D, tk, NL * 2 * D, tk + D, NL * 2 * D, Q, T, ly.ca.heads, D, nullptr, 0, d.ctx, D);
    r.lin(d.ctx, nullptr, D, Q, ly.ca.out, 0, hs, D, d.pre, D);
    r.ln(d.pre, Q, D, ly.ln2, eps, nullptr, hs);
    // deformable cross-attention on the encoder memory
    r.lin(hs, d.qpos, D, Q, ly.msda.offw, 0, nullptr, 0, d.ow, NOW);
    deform(r, d.val_all + (size_t)i * D, NL * D, d.ow, NOW, rf, 4, 1, Q, d.ctx, nullptr);
    r.lin(d.ctx, nullptr, D, Q, ly.msda.out, 0, hs, D, d.pre, D);
    r.ln(d.pre, Q, D, ly.ln3, eps, nullptr, hs);
    // FFN
    r.lin(hs, nullptr, D, Q, ly.fc1, 1, nullptr, 0, d.ffb, c.ffn_dim);
    r.lin(d.ffb, nullptr, c.ffn_dim, Q, ly.fc2, 0, hs, D, d.pre, D);
    r.ln(d.pre, Q, D, ly.ln4, eps, nullptr, hs);
    layer_done(r, st, i, NL, rf);
    // iterative box refinement (the update after the last layer is unused)
    if (i + 1 < NL) {
      r.lin(hs, nullptr, D, Q, g->bbox[i][0], 1, nullptr, 0, d.b1, D);
      r.lin(d.b1, nullptr, D, Q, g->bbox[i][1], 1, nullptr, 0, d.b2, D);
      r.lin(d.b2, nullptr, D, Q, g->bbox[i][2], 0, nullptr, 0, d.delta, 4);
      if (r.go()) r.chk(launch_box_refine(d.delta, 4, rf, 1e-5f, d.refs[cur ^ 1], Q, s), "box_refine");
      cur ^= 1;
    }
  }
}

// ---- heads on the normalised last hidden state
void heads(Run& r, State& st) {
  OvmGdino* g = r.g; Plan* pl = r.pl;
  const OvmGdinoConfig& c = g->cfg;
  const int D = c.d_model, T = pl->T, Q = c.num_queries, NL = (int)g->dec.size();
  const hipStream_t s = r.s_main;
  DecScratch& d = st.d;
  r.ln(st.hs, Q, D, g->dec_ln, c.eps, nullptr, st.hn);
  float* lt = r.f32((size_t)Q * T);
  if (r.go()) {
    r.chk(ovm_g_bmm(st.hn, st.text, lt, 1, Q, T, D, D, D, T, 0, 0, 0, 1, 1.0f, s), "bmm logits");
    r.chk(launch_pad_logits(lt, T, Q, T, pl->out_logits, c.max_text_len, s), "pad_logits");
  }
  r.lin(st.hn, nullptr, D, Q, g->bbox[NL - 1][0], 1, nullptr, 0, d.b1, D);
  r.lin(d.b1, nullptr, D, Q, g->bbox[NL - 1][1], 1, nullptr, 0, d.b2, D);
  r.lin(d.b2, nullptr, D, Q, g->bbox[NL - 1][2], 0, nullptr, 0, d.delta, 4);
  if (r.go()) r.chk(launch_box_refine(d.delta, 4, st.last_ref, 1e-5f, pl->out_boxes, Q, s), "box_refine");
}

// what a caption entry holds, into its buffers: the text branch's BERT and projection, then layer 0's text norm and projection of
// the main branch - the kernels, operands, order and workspace slices they have inside a forward without the cache
void caption_ops(Run& r, TextEntry& e) {
  OvmGdino* g = r.g;
  const OvmGdinoConfig& c = g->cfg;
  r.ws_text();
  bert_chain(r, e.tx, e.text0);
  r.ws_image();
  if (g->enc.empty()) return;
  const EncLayer& ly = g->enc[0];
  r.ln(e.text0, e.T, c.d_model, ly.lnt, c.eps, nullptr, e.t0);
  r.lin(e.t0, nullptr, c.d_model, e.T, ly.tkv, 0, nullptr, 0, e.tkv0, ly.tkv.N);
}

// Encodes the plan's caption into a new entry: eagerly on `s`, outside any graph, scratch in a temporary arena. The stream is drained
// before the entry is returned, so every later forward, on whichever stream, reads finished buffers (a plan build synchronises the
// device several times already: once more per new caption costs nothing that matters).
int encode_caption(OvmGdino* g, Plan* pl, hipStream_t s, std::shared_ptr<TextEntry>* out) {
  const OvmGdinoConfig& c = g->cfg;
  auto e = std::make_shared<TextEntry>();
  e->ids = pl->ids; e->pids = pl->pids; e->gen = tune_generation(); e->T = pl->T;
  const size_t T = (size_t)pl->T;
  const size_t n[4] = {T * g->bertD, T * c.d_model, T * c.d_model, T * c.ffn_dim};
  float** dst[4] = {&e->tx, &e->text0, &e->t0, &e->tkv0};
  for (int i = 0; i < 4; ++i) {
    OVM_HIP(g, hipMalloc((void**)dst[i], n[i] * sizeof(float)));
    e->bytes += n[i] * sizeof(float);
  }
  Run dry{g, pl, s, true};
  dry.init_streams();
  caption_ops(dry, *e);
  if (dry.rc) return dry.rc;
  void* tmp = nullptr;
  OVM_HIP(g, hipMalloc(&tmp, dry.peak + 4096));
  Run run{g, pl, s, false};
  run.abase = (char*)tmp; run.acap = dry.peak + 4096;
  run.s_main = s;                                        // one stream: no init_streams(), no fork
  caption_ops(run, *e);
  const hipError_t he = hipStreamSynchronize(s);
  (void)hipFree(tmp);
  if (run.rc) return run.rc;
  OVM_HIP(g, he);
  e->launches = run.launches;
  *out = e;
  return OVM_OK;
}

}  // namespace

int acquire_text(OvmGdino* g, Plan* pl, hipStream_t s, long* launches) {
  *launches = 0;
  if (!pl->tune.text_cache) return OVM_OK;
  const unsigned long gen = tune_generation();
  if (pl->text && pl->text->gen == gen) return OVM_OK;
  std::shared_ptr<TextEntry> e = find_text(g, pl->ids, pl->pids, gen);
  if (!e) {
    OVM_TRY(g, encode_caption(g, pl, s, &e));
    *launches = e->launches;
    keep_text(g, e, pl->tune.text_cache);
  }
  pl->text = e;
  return OVM_OK;
}

// One pass over a plan, run three ways over the same code: dry (sizes the arena), eager, under stream capture. Which kernels a pass
// launches and what it allocates depends on the handle, the plan and the plan's tune knobs alone.
int forward_impl(Run& r) {
  r.init_streams();
  State st;
  text_encoder(r, st);                  // on the text branch, beside the next two stages
  swin_backbone(r, st);
  neck(r, st);
  encoder(r, st);                       // joins the branches first
  select_queries(r, st);
  const size_t mk = decoder_inputs(r, st);
  if (st.d.chain) decoder_chain(r, st);
  else decoder_per_op(r, st);
  heads(r, st);
  r.release(mk);
  return r.rc;
}

}  // namespace gdino
}  // namespace ovm

extern "C" {

int ovm_gdino_create(const OvmGdinoConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmGdino** out) {
  if (!cfg || !weights || !out) return OVM_ERR_INVALID;
  OvmGdino* g = new OvmGdino();
  *out = g;                                      // returned even on failure so that ovm_gdino_last_error can be read; destroy it
  g->cfg = *cfg; g->device = device; g->precision = cfg->precision == 1 ? 1 : 3;
  // Weights and tables live in a few large slabs, not in one hipMalloc each: ~700 separate allocations scatter the checkpoint over as
  // many small VM mappings, and the latency-bound kernels of this branch (every workgroup touches every page of a weight matrix once)
  // then pay an address-translation miss per 4-KiB page; a slab is mapped with large fragments.
  g->policy = ALLOC_SLAB; g->k_align = 64;
  g->graphs_enabled = cfg->use_graphs;
  g->branches = g_gdino_tune.branches;
  {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);         // hi = numerically lowest = highest priority
    if (hipStreamCreateWithPriority(&g->aux, hipStreamNonBlocking, hi) != hipSuccess || hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_join, hipEventDisableTiming) != hipSuccess) {
      g->err = "could not create the text-branch stream"; return OVM_ERR_HIP;
    }
  }
  const OvmGdinoConfig& c = g->cfg;
  if (c.d_model % c.heads || c.n_levels > 8 || c.n_levels < 1 || c.swin_window <= 0) { g->err = "bad GroundingDINO config"; return OVM_ERR_INVALID; }
  OVM_HIP(g, hipSetDevice(device));
  const WeightMap wm(weights, n_weights);
  OVM_TRY(g, load_bert(g, wm));
  OVM_TRY(g, load_swin(g, wm));
  OVM_TRY(g, load_neck(g, wm));
  OVM_TRY(g, load_encoder(g, wm));
  OVM_TRY(g, load_decoder(g, wm));
  OVM_TRY(g, load_encoder_merged(g, wm));
  OVM_HIP(g, hipDeviceSynchronize());
  return OVM_OK;
}

int ovm_gdino_destroy(OvmGdino* g) {
  if (!g) return OVM_OK;
  (void)hipSetDevice(g->device);
  (void)hipDeviceSynchronize();
  for (Plan* p : g->plans) delete p;
  g->texts.clear();
  g->free_all();
  if (g->aux) (void)hipStreamDestroy(g->aux);
  if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
  if (g->ev_join) (void)hipEventDestroy(g->ev_join);
  delete g;
  return OVM_OK;
}

const char* ovm_gdino_last_error(const OvmGdino* g) { return g ? g->err.c_str() : "null handle"; }

int ovm_gdino_set_force_topk(OvmGdino* g, const int32_t* idx_device) {
  if (!g) return OVM_ERR_INVALID;
  g->force_topk = idx_device;
  for (Plan* p : g->plans) p->drop_graph();       // captured graphs bake the selection source in
  return OVM_OK;
}

// The network: image (uint8, any C/H/W strides; normalised here with the reference's images[0][[2,1,0]] convention when
// flip_channels is set, roi_heads_gdino.py:146) + caption token ids -> pred_logits [num_queries][max_text_len] (pre-sigmoid,
// -inf beyond the caption) and pred_boxes [num_queries][4] (cx, cy, w, h in [0, 1]). position_ids: null = upstream numbering.
int ovm_gdino_forward(OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* position_ids,
                      float* pred_logits, float* pred_boxes, ovm_stream_t stream) {
  if (!g || !image || !token_ids || ntok <= 0 || ntok > g->cfg.max_text_len) return OVM_ERR_INVALID;
  g->err.clear();
  hipStream_t s = (hipStream_t)stream;
  const int H = image->height, W = image->width;
  if (H <= 0 || W <= 0) return OVM_ERR_INVALID;
  std::vector<int> ids(token_ids, token_ids + ntok), pids;
  if (position_ids) pids.assign(position_ids, position_ids + ntok);
  Plan* pl = find_plan(g, H, W, ids, pids);
  long text_launches = 0;
  if (!pl) {
    OVM_TRY(g, build_plan(g, H, W, ids, pids, &pl));
    int r = acquire_text(g, pl, s, &text_launches);       // the caption's entry: held already, or encoded here (its scratch is not the arena's)
    if (r) { delete pl; return r; }
    Run dry{g, pl, s, true};
    r = forward_impl(dry);
    if (r) { delete pl; return r; }
    pl->arena_cap = dry.peak + 4096;
    void* q = nullptr;
    if (hipMalloc(&q, pl->arena_cap) != hipSuccess) { delete pl; g->err = "arena allocation failed"; return OVM_ERR_HIP; }
    pl->allocs.push_back(q); pl->arena = (char*)q; pl->bytes += pl->arena_cap;
    evict_plans(g, pl);
  }
  g->plans.push_front(pl);
  g->last = pl;
  // input normalisation reads the caller's buffer: outside the graph
  OVM_TRY(g, ovm_g_normalize_image(image, g->cfg.pixel_mean, g->cfg.pixel_std, g->cfg.flip_channels, pl->img, s));
  if (pl->exec) {
    OVM_HIP(g, hipGraphLaunch(pl->exec, s));
  } else {
    // an eager pass launches under the tune settings of now: so must the caption entry it reads have been (a graph keeps both as captured)
    long again = 0;
    OVM_TRY(g, acquire_text(g, pl, s, &again));
    text_launches += again;
    Run run{g, pl, s, false};
    OVM_TRY(g, forward_impl(run));
    pl->launches = run.launches; pl->mlp_fused_sites = run.mlp_sites;
    if (g->graphs_enabled) capture_plan(g, pl, s);
  }
  g->launches_last = pl->launches;
  g->text_launches_last = text_launches;
  const size_t nl = (size_t)g->cfg.num_queries * g->cfg.max_text_len;
  if (pred_logits) OVM_HIP(g, hipMemcpyAsync(pred_logits, pl->out_logits, nl * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (pred_boxes) OVM_HIP(g, hipMemcpyAsync(pred_boxes, pl->out_boxes, (size_t)g->cfg.num_queries * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return OVM_OK;
}

// network + the reference-owned output glue (ovm_gdino_postprocess): boxes / scores / class indices of the kept queries
int ovm_gdino_detect(OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* spans, int32_t n_phrases,
                     float box_threshold, float nms_threshold, float* out_boxes, float* out_scores, int32_t* out_classes, int32_t* n_out,
                     ovm_stream_t stream) {
  int r = ovm_gdino_forward(g, image, token_ids, ntok, nullptr, nullptr, nullptr, stream);
  if (r) return r;
  Plan* pl = g->last;
  return ovm_gdino_postprocess(pl->out_logits, g->cfg.num_queries, g->cfg.max_text_len, pl->out_boxes, spans, n_phrases, image->height,
                               image->width, box_threshold, nms_threshold, out_boxes, out_scores, out_classes, n_out, stream);
}

int32_t ovm_gdino_num_queries(const OvmGdino* g) { return g ? g->cfg.num_queries : 0; }

// device pointers of the last forward's raw outputs (owned by the handle's current plan; valid until the next forward)
int ovm_gdino_last_outputs(OvmGdino* g, const float** pred_logits, const float** pred_boxes, int32_t* logits_ld) {
  if (!g || !g->last) return OVM_ERR_INVALID;
  if (pred_logits) *pred_logits = g->last->out_logits;
  if (pred_boxes) *pred_boxes = g->last->out_boxes;
  if (logits_ld) *logits_ld = g->cfg.max_text_len;
  return OVM_OK;
}

int64_t ovm_gdino_debug_copy(OvmGdino* g, const char* name, void* dst, int64_t capacity_elems, ovm_stream_t stream) {
  if (!g || !g->last || !name) return OVM_ERR_INVALID;
  if (std::string(name) == "launches") return g->launches_last;
  if (std::string(name) == "mlp_fused_sites") return g->last->mlp_fused_sites;            // MLPs of the last plan's forward on the fused route
  if (std::string(name) == "plans") return (int64_t)g->plans.size();                      // plan-cache occupancy (tests, bench)
  if (std::string(name) == "plan_bytes") { int64_t b = (int64_t)text_bytes(g, nullptr); for (Plan* q : g->plans) b += (int64_t)q->bytes; return b; }   // caption entries once, not per plan
  if (std::string(name) == "text_launches") return g->text_launches_last;                 // op launches the last forward call spent encoding its caption (0: held)
  if (std::string(name) == "text_entries") return (int64_t)g->texts.size();               // caption-cache occupancy
  auto it = g->last->taps.find(name);
  if (it == g->last->taps.end()) { g->err = std::string("unknown debug tensor ") + name; return OVM_ERR_INVALID; }
  if (it->second.second > capacity_elems) return OVM_ERR_CAPACITY;
  if (hipMemcpyAsync(dst, it->second.first, (size_t)it->second.second * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return OVM_ERR_HIP;
  return it->second.second;
}

}  // extern "C"
