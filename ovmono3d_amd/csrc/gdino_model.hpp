// The GroundingDINO engine's own types, shared by its three translation units and by nothing else (not part of the C ABI):
//   gdino_load.hip   checkpoint -> packed weights of the handle (load_bert ... load_decoder)
//   gdino_plan.hip   (image size, caption) -> Plan: host-built tables, scratch, the plan cache and the graph capture
//   gdino.hip        one forward over a plan (forward_impl and its stages) and the extern "C" entry points
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/ovm3d.h"
#include "gdino.hpp"
#include "kernels.hpp"
#include "loader.hpp"
#include "tower.hpp"

namespace ovm {

// ovm_tune_set's detector keys, process wide. `branches` is copied into a handle when it is created, the others into a Plan when it
// is built; the forward reads the plan's copy alone, so every pass over a plan (sizing, eager, capture, later eager calls) walks the
// same allocation and launch sequence whatever is set in between.
struct GdinoTune {
  int branches;        // text side on a stream of its own
  int dec_chain;       // decoder layers as row-chain kernels (dec_chain.hip); 0: one launch per op, kept as the cross-check
  int ffn_split;       // decoder chain B over (row blocks) x (FFN chunks) + chain C. Bit-identical; 8.61 -> 8.34 ms for the detector ALONE,
                       // but 51.14 -> 50.97 images/s beside the ViT (four times the workgroups on the chip): off
  int swin_fused;      // Swin blocks: qkv projection inside the window-attention kernel (windows of 12 x 12 and 7 x 7)
  int gemm256;         // the wide K <= 256 contractions on the 256 x 256 GEMM (interleaved activations)
  int mlp_fused;       // two-layer MLPs of the image branch in one kernel + the split-K reduce (mlp_fused.hip): 0 off, 1 Swin blocks,
                       // 2 Swin blocks and the encoder's FFN
  int swin_tap;        // tests: n > 0 keeps copies of the n-th Swin block's window rows and context rows (fused route) for
                       // ovm_gdino_debug_copy "swin_tap_*"; costs arena and four copies per forward, so 0 outside tests
  int enc_fold;        // encoder, image half: 1 = both halves below, 2 = the fold alone, 3 = the producers' split rows alone, 0 = neither.
                       // Fold: (vis + pos) W_off^T + b_off = vis W_off^T + P with P = pos W_off^T + b_off a per-plan, per-layer table
                       // (Plan::enc_P), so value and offsets projections are ONE GEMM over [value | offw] (MsdaW::voff) whose epilogue adds P
                       // to the offsets columns, and the out-projection writes the split rows that GEMM reads (no row pass).
                       // Producers' split rows: the Swin stages' out-norms write the rows the neck's projections read, the last
                       // layer's final norm those of the decoder's value projection (no row pass at either site).
  int enc_tap;         // tests: keeps copies of encoder layer 0's out-projection rows, their split and the value | offsets projections'
                       // outputs for ovm_gdino_debug_copy "enc_pos|enc_vis0|enc_vis0_hi|enc_vis0_lo|enc_voff0|enc_P0" (enc_fold 0: "enc_val0|enc_ow0"
                       // for the last two); costs arena and four copies per forward, so 0 outside tests
  int text_cache;      // caption cache (TextEntry below): n > 0 = the handle keeps the n most recently used captions' encodings and a plan's
                       // forward reads them; 0 = BERT, the text projection and layer 0's text norm / projection inside every forward
  bool fold() const { return enc_fold == 1 || enc_fold == 2; }
  bool prod_split() const { return enc_fold == 1 || enc_fold == 3; }
};
extern GdinoTune g_gdino_tune;
// Advanced by every ovm_tune_set call. The glin_* and split-K knobs change the summation order of the small GEMMs, so what was
// computed under one setting (a TextEntry) never serves a forward issued under another.
unsigned long tune_generation();
void bump_tune_generation();

namespace gdino {

struct Lin : PackedLin {
  half_t* frag = nullptr;          // decoder weights only: the same image in MFMA-fragment order (make_frag), for the row-chain kernels
  std::vector<half_t> img;         // host copy of the image, kept from packing until make_frag has cut the fragment copy from it
};
struct Ln { float* g = nullptr; float* b = nullptr; };
struct SplitBuf { half_t* hi = nullptr; half_t* lo = nullptr; int ld = 0; bool il = false; };   // il: one interleaved image [row][k/32][hi 32 | lo 32], lo = hi + 32, ld = 2 K

struct SwinBlock { Ln ln1, ln2; Lin qkv, proj, fc1, fc2; float* relbias = nullptr; };
struct SwinStage { std::vector<SwinBlock> blocks; int nh = 0, C = 0; bool has_red = false; Lin red; Ln dn; bool has_out = false; Ln on; };
struct BertLayer { Lin qkv, ao, fi, fo; Ln aln, oln; };
struct Mha { Lin qk, v, out; Lin q, kv; int heads = 0; };       // qk: [query | key] rows; kv: [key | value]; q alone for cross attention
struct MsdaW { Lin offw, value, out; Lin voff; };   // voff (encoder layers): [value | offw] rows, bias on the value columns alone (GdinoTune::enc_fold)
struct EncLayer {
  Ln lnv, lnt; Lin vqv, tkv, ov, ot;            // fusion: [vision_proj | values_vision_proj], [text_proj | values_text_proj], gated output projections
  Mha te; Ln te_ln1, te_ln2; Lin te_fc1, te_fc2;
  MsdaW msda; Ln de_ln1, de_ln2; Lin de_fc1, de_fc2;
};
struct DecLayer { Mha sa, ca; MsdaW msda; Ln ln1, ln2, ln3, ln4; Lin fc1, fc2; };

struct Plan;

// Everything of a forward that depends on the caption and the weights alone, computed once (encode_caption, gdino.hip) and read by
// every plan of that caption: BERT's output, the projected text features, and encoder layer 0's normalised text rows and their
// [text_proj | values_text_proj] projection. Key: (token ids, position ids as the caller gave them, tune generation).
// Lifetime: the handle's list (Model::texts, most recently used first, at most GdinoTune::text_cache entries) and every plan whose
// forward - and captured graph - points into the buffers hold a shared_ptr each, so eviction from the list or of a plan never frees
// memory a live graph reads. Written by encode_caption alone, which drains its stream before the entry is handed out: read-only
// afterwards, on any stream.
struct TextEntry {
  std::vector<int> ids, pids;
  unsigned long gen = 0;
  int T = 0;
  float *tx = nullptr, *text0 = nullptr, *t0 = nullptr, *tkv0 = nullptr;   // [T][bertD], [T][d_model], [T][d_model], [T][ffn_dim]
  size_t bytes = 0;
  long launches = 0;                          // op launches the encoding took (ovm_gdino_debug_copy "text_launches" of the call that encoded)
  ~TextEntry() {
    for (float* p : {tx, text0, t0, tkv0}) if (p) (void)hipFree(p);
  }
};

struct Model : Loader {
  OvmGdinoConfig cfg;
  int device = 0;
  float* sine_dim_t = nullptr;                                 // [d_model / 4] frequency table of the decoder's sine embedding (dec_chain.hip)
  // ---- weights
  float *word = nullptr, *posemb = nullptr, *typemb = nullptr; Ln emb_ln; int bertD = 0, n_pos = 0, vocab = 0;
  std::vector<BertLayer> bert;
  Lin text_proj;
  Lin pe; Ln pe_ln;
  std::vector<SwinStage> stages;
  struct InProj { Lin w; int k = 1; Ln gn; } inproj[8];
  std::vector<float> level_embed;             // host [L][D]
  std::vector<EncLayer> enc;
  Lin enc_output; Ln enc_output_ln; Lin enc_bbox[3];
  float* tgt = nullptr;
  std::vector<DecLayer> dec;
  Lin dec_kv_text, dec_value;                 // all decoder layers' text key|value and deformable value projections, concatenated
  Ln dec_ln; Lin ref_head[2]; std::vector<std::array<Lin, 3>> bbox;
  // ---- plans
  std::list<Plan*> plans;
  Plan* last = nullptr;
  const int* force_topk = nullptr;            // device int32 [num_queries] (tests: pin the two-stage selection)
  int graphs_enabled = 1;
  long launches_last = 0;
  // ---- caption cache
  std::list<std::shared_ptr<TextEntry>> texts;  // most recently used first
  long text_launches_last = 0;                // op launches the last forward call spent on encoding its caption (0: it was held)
  // ---- second branch of the forward: the text side (BERT, the text enhancers) has no data dependence on the image side (Swin,
  // deformable attention) between their joins, so it runs on a stream of its own - in a captured plan two branches of the graph
  int branches = 1;                           // GdinoTune::branches when the handle was created
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

}  // namespace gdino
}  // namespace ovm

struct OvmGdino : ovm::gdino::Model {};       // the C ABI's name for the handle

namespace ovm {
namespace gdino {

// ---- gdino_load.hip: key names, packing order and slab allocation order are the checkpoint's contract with the handle
int load_bert(OvmGdino* g, const WeightMap& wm);
int load_swin(OvmGdino* g, const WeightMap& wm);
int load_neck(OvmGdino* g, const WeightMap& wm);
int load_encoder(OvmGdino* g, const WeightMap& wm);
int load_decoder(OvmGdino* g, const WeightMap& wm);      // with the heads and the fragment-ordered copies (make_frag)
int load_encoder_merged(OvmGdino* g, const WeightMap& wm);   // MsdaW::voff of every encoder layer; last, so that no other weight moves

// ------------------------------------------------------------------------------------------------------------------------------
// Plan: everything derived from (H, W, token ids, position ids)
// ------------------------------------------------------------------------------------------------------------------------------
struct WinMaps { int* win = nullptr; float* mask = nullptr; int nW = 0; };
struct StageGeo { int h = 0, w = 0; WinMaps wm[2]; int* merge = nullptr; int h2 = 0, w2 = 0; };

struct Plan {
  int H = 0, W = 0, T = 0;
  std::vector<int> ids, pids;
  GdinoTune tune = {};                              // g_gdino_tune when the plan was built (branches: the handle's)
  std::vector<void*> allocs; size_t bytes = 0;      // device memory this plan holds (the plan cache's budget counts it)
  // text
  int* d_ids = nullptr; int* d_pids = nullptr; float* text_bias = nullptr; float* text_pos = nullptr;
  std::shared_ptr<TextEntry> text;                  // tune.text_cache > 0: the caption's encoding this plan's forward and graph read (co-owned)
  // swin
  int Hp = 0, Wp = 0; int* pe_map = nullptr;
  std::vector<StageGeo> geo;
  // neck / encoder tables
  int nlev = 0; int lh[8] = {0}, lw[8] = {0}, lstart[8] = {0}; int S = 0;
  int* conv_map = nullptr; int conv_h = 0, conv_w = 0;
  float* pos = nullptr; float* ref = nullptr; float* prop_logit = nullptr; int* valid_idx = nullptr;
  std::vector<float*> enc_P;                     // tune.fold(): per encoder layer [S][NOW] = pos W_off^T + b_off (plan_offset_tables)
  // scratch owned by the plan
  float* img = nullptr;                          // normalised input image [H*W][3]
  char* arena = nullptr; size_t arena_cap = 0;
  float* gemm_ws = nullptr; size_t gemm_ws_cap = 0;     // split-K partials (both GEMM kernels)
  unsigned long long* topk_keys = nullptr; int topk_N = 0;
  float* out_logits = nullptr; float* out_boxes = nullptr;
  // debug taps (pointers into the arena, valid after a forward)
  std::map<std::string, std::pair<const void*, int64_t>> taps;
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
  long launches = 0;
  int mlp_fused_sites = 0;                       // MLPs of one forward that took the fused route (ovm_gdino_debug_copy "mlp_fused_sites")
  void drop_graph() {
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
  }
  ~Plan() {
    drop_graph();
    for (void* p : allocs) (void)hipFree(p);
  }
};

// ---- gdino_plan.hip
int build_plan(OvmGdino* g, int H, int W, const std::vector<int>& ids, const std::vector<int>& pids, Plan** out);
Plan* find_plan(OvmGdino* g, int H, int W, const std::vector<int>& ids, const std::vector<int>& pids);   // taken out of the cache, or null
void evict_plans(OvmGdino* g, const Plan* incoming);
// caption cache: the held entry of this key (moved to the front of the handle's list) or null; keep_text puts a freshly encoded one
// in front and drops the least recently used ones beyond `cap`; text_bytes = device memory of every live entry, each counted once
std::shared_ptr<TextEntry> find_text(OvmGdino* g, const std::vector<int>& ids, const std::vector<int>& pids, unsigned long gen);
void keep_text(OvmGdino* g, const std::shared_ptr<TextEntry>& e, int cap);
size_t text_bytes(const OvmGdino* g, const Plan* incoming);
void capture_plan(OvmGdino* g, Plan* pl, hipStream_t s);

// split-K workspace of the text branch (tail of the plan's workspace): its largest user is BERT's output projection at the
// maximum caption length, 12 slices x 256 tokens x 768 columns of fp32 partials = 9.4 MB
constexpr size_t kAuxWs = (size_t)16 << 20;

// ------------------------------------------------------------------------------------------------------------------------------
// One forward over a plan. `dry` = size the arena only (no launches).
// ------------------------------------------------------------------------------------------------------------------------------
struct Run {
  OvmGdino* g; Plan* pl; hipStream_t s; bool dry;
  size_t off = 0, peak = 0;
  char* abase = nullptr; size_t acap = 0;        // an arena of the caller's in place of the plan's (encode_caption's temporary)
  long launches = 0;
  int mlp_sites = 0;                             // MLPs on the fused route so far
  int rc = OVM_OK;
  // the two branches (see Model::aux). `s` is the stream the op wrappers launch on; fork() lets the text branch start from
  // the current point of the main stream, join() makes the main stream wait for it. Each branch has its own slice of the split-K
  // workspace. With branches off (or in the sizing pass) everything stays on the caller's stream.
  hipStream_t s_main = nullptr;
  float* ws = nullptr; size_t ws_cap = 0;
  bool two() const { return g->branches && g->aux && !dry; }
  void init_streams() { s_main = s; ws = pl->gemm_ws; ws_cap = two() ? pl->gemm_ws_cap - kAuxWs : pl->gemm_ws_cap; }
  void fork() {
    if (!two() || rc != OVM_OK) return;
    if (hipEventRecord(g->ev_fork, s_main) != hipSuccess || hipStreamWaitEvent(g->aux, g->ev_fork, 0) != hipSuccess) fail(OVM_ERR_HIP, "fork");
  }
  void on_text() { if (two()) { s = g->aux; ws = (float*)((char*)pl->gemm_ws + (pl->gemm_ws_cap - kAuxWs)); ws_cap = kAuxWs; } }
  void on_image() { if (two()) { s = s_main; ws = pl->gemm_ws; ws_cap = pl->gemm_ws_cap - kAuxWs; } }
  // the branches' workspace slices without their streams: encode_caption issues both branches' caption ops on one stream and gives
  // each the slice - hence the split-K choice - it has inside a forward
  bool sliced() const { return g->branches && g->aux; }
  void ws_text() {
    if (sliced()) { ws = (float*)((char*)pl->gemm_ws + (pl->gemm_ws_cap - kAuxWs)); ws_cap = kAuxWs; }
    else ws_image();
  }
  void ws_image() { ws = pl->gemm_ws; ws_cap = sliced() ? pl->gemm_ws_cap - kAuxWs : pl->gemm_ws_cap; }
  void join() {
    if (!two()) return;
    on_image();
    if (rc != OVM_OK) return;
    if (hipEventRecord(g->ev_join, g->aux) != hipSuccess || hipStreamWaitEvent(s_main, g->ev_join, 0) != hipSuccess) fail(OVM_ERR_HIP, "join");
  }

  void* alloc(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    char* base = abase ? abase : pl->arena;
    void* p = dry ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base + off);
    off += bytes;
    if (off > peak) peak = off;
    if (!dry && off > (abase ? acap : pl->arena_cap)) { fail(OVM_ERR_CAPACITY, "arena overflow"); return base; }
    return p;
  }
  float* f32(size_t n) { return (float*)alloc(n * sizeof(float)); }
  int* i32(size_t n) { return (int*)alloc(n * sizeof(int)); }
  // split-fp16 rows of logical width K; the row stride is K rounded up to the GEMM's k-step (64). Producers write columns
  // [0, K) only, so when a pad exists (K = 32 or 48: test-size models, the 4x4x3 patch rows) the buffer is cleared first -
  // arena memory is recycled and NaN bit patterns in the pad would survive the multiplication by the zero weight columns.
  SplitBuf split(size_t rows, int K) {
    SplitBuf b; b.ld = (K + 63) / 64 * 64;
    const size_t bytes = rows * b.ld * sizeof(half_t);
    b.hi = (half_t*)alloc(bytes);
    b.lo = g->precision == 3 ? (half_t*)alloc(bytes) : nullptr;
    if (b.ld != K && go()) {
      if (hipMemsetAsync(b.hi, 0, bytes, s) != hipSuccess) fail(OVM_ERR_HIP, "memset");
      if (b.lo && hipMemsetAsync(b.lo, 0, bytes, s) != hipSuccess) fail(OVM_ERR_HIP, "memset");
    }
    return b;
  }
  // Interleaved split rows for the operands of the 256 x 256 GEMM (gemm256.hip): the encoder's and Swin stage 1's wide contractions
  // over K <= 256 (752 / 564 / 556 tiles of 128 x 128, i.e. 2-3 rounds of a kernel whose per-round cost hardly depends on K) are one
  // round of 256 x 256 tiles there. Falls back to planar rows when the kernel cannot take the shape (one-pass precision, K % 32).
  SplitBuf split_for256(size_t rows, int K) {
    if (g->precision != 3 || K % 32 || !pl->tune.gemm256) return split(rows, K);
    SplitBuf b; b.il = true; b.ld = 2 * K;
    b.hi = (half_t*)alloc(rows * b.ld * sizeof(half_t)); b.lo = b.hi ? b.hi + 32 : nullptr;
    return b;
  }
  // interleaved split rows whatever the gemm256 knob says: the A operand of the fused MLP
  SplitBuf split_il(size_t rows, int K) {
    SplitBuf b; b.il = true; b.ld = 2 * K;
    b.hi = (half_t*)alloc(rows * b.ld * sizeof(half_t)); b.lo = b.hi + 32;
    return b;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
  void fail(int r, const char* what) { if (rc == OVM_OK) { rc = r; if (g->err.empty()) g->err = what; } }
  void chk(int r, const char* what) { ++launches; if (r != OVM_OK) fail(r, what); }
  void tap(const std::string& name, const void* p, int64_t n) { if (!dry) pl->taps[name] = {p, n}; }

  // ---- op wrappers (all skip the launch in a dry pass) ----
  bool go() const { return !dry && rc == OVM_OK; }      // after a failure nothing further is launched (later kernels would read its garbage)
  void copy(void* dst, const void* src, size_t bytes, hipStream_t st) {      // device to device, not counted as a launch
    if (go() && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) fail(OVM_ERR_HIP, "hipMemcpyAsync");
  }
  // row operator over fp32 rows x [M][ldx] of width D; into(): its split-fp16 output
  static RowOpParams rows(const float* x, int ldx, int M, int D) {
    RowOpParams p; memset(&p, 0, sizeof(p));
    p.x = x; p.ldx = ldx; p.M = M; p.D = D;
    return p;
  }
  static void into(RowOpParams& p, const SplitBuf& b) { p.hi = b.hi; p.lo = b.lo; p.ldh = b.ld; p.il = b.il ? 1 : 0; }
  void rowop(const RowOpParams& p) { if (go()) chk(launch_rowop(p, s), "rowop"); }

  // big GEMM on the LDS-DMA kernels of gemm.hpp: A split fp16 [M][lda]
  GemmParams gp(const SplitBuf& A, int M, const Lin& W) {
    GemmParams p = gp_base(SplitImg{A.hi, A.lo}, A.ld, W, M);
    p.a_il = A.il ? 1 : 0; p.ws_slot = 1; p.part_ws = ws; p.part_cap = ws_cap;
    return p;
  }
  // (not the tower's ovm::gemm: that one routes by a tile-count threshold, this one by the layout of A)
  void gemm(const GemmParams& p, int epi) {
    if (!go()) return;
    if (p.a_il && gemm256_supported(p, g->precision)) chk(launch_gemm256(p, epi, 1, s), "gemm256");
    else chk(launch_gemm(p, g->precision, epi, A_ROWMAJOR, s), "gemm");
  }

  // Two-layer MLP fc2(act(fc1(x))) of the image branch: does this site take the fused route (mlp_fused.hip)? `site`: the knob value that
  // enables it (1 Swin, 2 encoder). Yes when the kernel takes the shape, fc2 is one of the thin grids that end in the split-K reduce
  // today (launch_ws: up to 96 tiles of 128 x 128 - elsewhere the fused route would ADD that launch: Swin stage 1) and the slabs fit
  // the image branch's slice of the workspace; otherwise the caller issues the two GEMMs. The same answer in every pass over a plan.
  bool mlp_fused_ok(int site, int M, const Lin& fc1, const Lin& fc2, int act) const {
    const int C = fc2.N, hidden = fc1.N;
    if (pl->tune.mlp_fused < site || g->precision != 3 || fc1.K != C || fc1.Kpad != C || fc2.K != hidden || fc2.Kpad != hidden) return false;
    if (!mlp_fused_supported(M, C, hidden, act, g->precision)) return false;
    if ((long)((M + 127) / 128) * ((C + 127) / 128) > 96) return false;
    const size_t cap = (g->branches && g->aux) ? pl->gemm_ws_cap - kAuxWs : pl->gemm_ws_cap;
    return mlp_fused_ws_bytes(M, C, hidden) <= cap;
  }
  // A: interleaved rows [M][2 C]; out: fc2's GemmParams with the epilogue operands set (its A side is not read)
  void mlp_fused(const SplitBuf& A, int M, const Lin& fc1, const Lin& fc2, int act, const GemmParams& out, int epi) {
    ++mlp_sites;
    if (!go()) return;
    MlpFusedParams p; memset(&p, 0, sizeof(p));
    p.X = A.hi; p.ldx = A.ld; p.W1 = fc1.hi; p.b1 = fc1.bias; p.W2 = fc2.hi; p.M = M; p.C = fc2.N; p.hidden = fc1.N; p.act = act;
    p.part = ws; p.part_cap = ws_cap;
    chk(launch_mlp_fused(p, out, epi, s), "mlp_fused");
  }

  // small / mid GEMM reading fp32 activations directly (gemm_small.hip): y = act((A + A2) W^T + b) (+ R)
  void lin(const float* A, const float* A2, int lda, int M, const Lin& W, int act, const float* R, int ldr, float* C, int ldc) {
    if (!go() || M <= 0) return;
    if (!gemm_small_supported(A, lda, W.K) || (A2 && (((uintptr_t)A2) & 15))) { fail(OVM_ERR_SHAPE, "lin: unaligned fp32 operand"); return; }
    chk(launch_gemm_small_ex(A, A2, lda, M, W.K, W.hi, W.lo, W.N, W.Kpad, W.bias, act, R, ldr, C, ldc, g->precision, ws, ws_cap, s),
        "lin");
  }
  void ln(const float* x, int M, int D, const Ln& w, float eps, const float* res, float* y, const SplitBuf* sp = nullptr) {
    RowOpParams p = rows(x, D, M, D);
    p.res = res; p.ldr = D; p.gamma = w.g; p.beta = w.b; p.eps = eps; p.y = y; p.ldy = D;
    if (sp) into(p, *sp);
    rowop(p);
  }
  void attn(const AttnF32Params& p) { if (go()) chk(launch_attn_f32(p, s), "attn_f32"); }
};

// gdino.hip
int forward_impl(Run& r);
// tune.text_cache > 0: gives the plan the entry of its caption under the current tune generation - the held one, or a new one encoded
// here, eagerly on `s` (drained before it returns) and outside any graph. *launches: what this call spent on encoding (0: held).
int acquire_text(OvmGdino* g, Plan* pl, hipStream_t s, long* launches);

}  // namespace gdino
}  // namespace ovm
