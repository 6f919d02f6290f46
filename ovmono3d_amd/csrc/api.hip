// C ABI of libovm3d (see include/ovm3d.h): the detection handle - a Tower (tower.hpp) with the pyramid, the heads, det2d, ovm_infer,
// profiling and the RCCL gather around it.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <string>
#include <vector>

#include "det2d.hpp"
#include "gdino.hpp"
#include "tower.hpp"

using namespace ovm;

static_assert(sizeof(OvmDet3D) == kRecFloats * 4, "record layout");

namespace {

struct SfpStage {              // 1x1 conv + LN, 3x3 conv + LN
  PackedLin c1, c3; float *n1g, *n1b, *n3g, *n3b;
};

struct FpnLevel {              // one output level of the simple feature pyramid, finest first ("p2", "p3", ...)
  int side = 0; float stride = 0.f;
  SfpStage st;
  float* T1 = nullptr;         // fp32 conv output (1x1, then reused by the 3x3)
  SplitImg pad;                   // zero-bordered LN(1x1) image: the implicit-GEMM input of the 3x3
  float* p = nullptr;          // the level's feature map, NHWC fp32
  SplitImg rpad;                  // zero-bordered fp16 copy of p (RPN conv input), when the checkpoint has an RPN
};

}  // namespace

struct OvmHandle : ovm::Loader {
  OvmConfig cfg;
  int device = 0;
  ovm::Tower tw;                    // patch embed + blocks (tower.hpp); the pyramid reads tw.X, every GEMM below dispatches through tw.ctx
  int C = 0;
  int nlev = 3;                     // by tower: 3 levels (DINOv2, patch 14, scales 2 1 0.5) or 4 levels (the patch-16 towers, scales 4 2 1 0.5)
  int roiK = 0;
  PackedLin dfuse; bool has_dfuse = false;
  PackedLin convt;                                           // ConvT D -> D/2 (first layer of the scale-2 and scale-4 stages... per stage)
  PackedLin convt4a, convt4b; float *up_ln_g = nullptr, *up_ln_b = nullptr;   // scale-4 stage: ConvT D -> D/2, LN, GELU, ConvT D/2 -> D/4
  FpnLevel lv[kMaxLevels];
  PackedLin cube_fc1, cube_fc2, cube_out;
  PackedLin box_fc1, box_fc2, box_out; bool has_box = false;
  PackedLin rpn_conv, rpn_out; bool has_rpn = false;
  SplitImg DT, DT4, DF, CT, CT4a, CT4b;
  float *dtok = nullptr, *FUS = nullptr;
  SplitImg RF, H1, H2; float* HO = nullptr; int lastN = 0;
  float* rec = nullptr; int* keep = nullptr;
  int *d_bidx = nullptr;
  ImageMeta *d_meta = nullptr, *h_meta = nullptr;               // device / pinned staging
  Det2dWorkspace det;
  int lastB = 0;
  ovm::Prof prof;                   // ovm_profile_enable / _read: the brackets around the ViT's launches (tw.ctx.prof points here)
  // ovm_infer: side stream of the text-prompted detector + 2D detection buffers (capacity = the detector's query count)
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  float *inf_boxes = nullptr, *inf_scores = nullptr; int *inf_classes = nullptr, *inf_n = nullptr, *inf_idx = nullptr, *inf_counts = nullptr;
  int inf_cap = 0;
  void* inf_ws = nullptr; size_t inf_ws_bytes = 0;      // scratch of the GroundingDINO output glue (launch_gdino_post_ws)
  int* inf_host = nullptr;                              // pinned: kept 2D count, record count
};

namespace {

// FC over pooled RoI features: reference flatten order is (c, ph, pw); ROIAlign here emits (ph, pw, c)
int pack_roi_fc(OvmHandle* h, const WeightMap& wm, const std::string& prefix, int N, int C, int res, PackedLin* out) {
  const int K = C * res * res;
  const float *w, *b;
  int r = find_weight(h, wm, prefix + ".weight", (int64_t)N * K, &w); if (r) return r;
  r = find_weight(h, wm, prefix + ".bias", N, &b); if (r) return r;
  std::vector<float> v((size_t)N * K);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int s = 0; s < res * res; ++s) v[(size_t)n * K + (size_t)s * C + c] = w[(size_t)n * K + (size_t)c * res * res + s];
  return upload_packed(h, v.data(), N, K, K, b, N, out);
}

int pack_sfp_stage(OvmHandle* h, const WeightMap& wm, const std::string& p1, const std::string& p3, int Cin, SfpStage* s) {
  const int C = h->C;
  int r = pack_conv(h, wm, p1, C, Cin, 1, BIAS_NONE, &s->c1); if (r) return r;
  r = upload_weight(h, wm, p1 + ".norm.weight", C, &s->n1g); if (r) return r;
  r = upload_weight(h, wm, p1 + ".norm.bias", C, &s->n1b); if (r) return r;
  r = pack_conv(h, wm, p3, C, C, 3, BIAS_NONE, &s->c3); if (r) return r;
  r = upload_weight(h, wm, p3 + ".norm.weight", C, &s->n3g); if (r) return r;
  return upload_weight(h, wm, p3 + ".norm.bias", C, &s->n3b);
}

void fill_meta(OvmHandle* h, const OvmImage* images, int B) {
  for (int b = 0; b < B; ++b) {
    const OvmImage& im = images[b];
    ImageMeta m;
    for (int i = 0; i < 9; ++i) m.K[i] = im.K[i];
    m.ratio = (float)((double)im.orig_height / (double)im.height);     // rcnn3d.py:92 (python float -> fp32 tensor)
    m.net_h = im.height; m.net_w = im.width; m.orig_h = im.orig_height; m.orig_w = im.orig_width;
    h->h_meta[b] = m;
  }
}

int from_tower(OvmHandle* h, int r) { if (r) h->err = h->tw.err; return r; }      // a tower call's result: its message becomes the handle's

}  // namespace

static int backbone_launches(OvmHandle* h, int B, const float* prompt_depth, int depth_h, int depth_w, hipStream_t s);

extern "C" {

const char* ovm_version(void) { return "libovm3d 0.2 (gfx950)"; }

// every struct include/ovm3d.h defines, in its order (the host binding asks for each of them by name when it loads the library)
#define OVM_ABI_STRUCTS(X)                                                                                                         \
  X(OvmConfig) X(OvmTensor) X(OvmImage) X(OvmDet3D) X(OvmGemmEpiOp) X(OvmGdinoConfig) X(OvmAttnF32Op) X(OvmMsDeformOp) X(OvmRowOp) \
  X(OvmSwinQkvAttnOp) X(OvmChainLin) X(OvmChainLn) X(OvmDecChainOp) X(OvmEvalCell) X(OvmJpegInfo) X(OvmJpegDecPlan)               \
  X(OvmJpegEncInfo) X(OvmSceneInput) X(OvmSceneBox) X(OvmSceneView) X(OvmSceneLayout) X(OvmSceneSegment) X(OvmPanelBox)            \
  X(OvmPanelsInput) X(OvmPanelPrim) X(OvmPanelsLayout) X(OvmGeoParams) X(OvmGeoInstance) X(OvmGeoResult) X(OvmGeoBox)              \
  X(OvmGroundParams) X(OvmGroundResult) X(OvmSamConfig) X(OvmSamCandidate) X(OvmDepthProConfig)

int ovm_abi_sizeof(const char* name) {
  if (!name) return -1;
  const std::string n(name);
#define OVM_ABI_SIZEOF(T) if (n == #T) return (int)sizeof(T);
  OVM_ABI_STRUCTS(OVM_ABI_SIZEOF)
#undef OVM_ABI_SIZEOF
  return -1;
}

const char* ovm_last_error(const OvmHandle* h) { return h ? h->err.c_str() : "null handle"; }

int ovm_destroy(OvmHandle* h) {
  if (!h) return OVM_OK;
  hipSetDevice(h->device);
  h->tw.destroy();
  h->free_all();
  if (h->h_meta) hipHostFree(h->h_meta);
  if (h->inf_host) hipHostFree(h->inf_host);
  for (int c = 0; c < OVM_PROF_NCAT; ++c)
    for (auto& pr : h->prof.ev[c]) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  if (h->ev_fork) hipEventDestroy(h->ev_fork);
  if (h->ev_join) hipEventDestroy(h->ev_join);
  if (h->side) hipStreamDestroy(h->side);
  delete h;
  return OVM_OK;
}

int ovm_host_shard_range(int64_t n, int32_t rank, int32_t world, int64_t* begin, int64_t* end) {
  if (world <= 0 || rank < 0 || rank >= world || n < 0) return OVM_ERR_INVALID;
  // InferenceSampler._get_local_indices: shard sizes n//W + (r < n%W), contiguous
  const int64_t q = n / world, r = n % world;
  const int64_t b = rank * q + (rank < r ? rank : r);
  *begin = b;
  *end = b + q + (rank < r ? 1 : 0);
  return OVM_OK;
}

int ovm_create(const OvmConfig* cfg, const OvmTensor* weights, int32_t n_weights, int32_t device, OvmHandle** out) {
  if (!cfg || !out) return OVM_ERR_INVALID;
  OvmHandle* h = new OvmHandle();
  *out = h;
  h->cfg = *cfg; h->device = device;
  const OvmConfig& c = h->cfg;
  Tower& t = h->tw; t.ctx.prof = &h->prof;
  static const int family_of[] = {FAM_DINOV2_HUB, FAM_OPEN_CLIP, FAM_HF_VITMAE, FAM_TIMM, FAM_SAM};      // by OVM_TOWER_*
  if (c.tower < 0 || c.tower > OVM_TOWER_SAM) { h->err = "invalid config (tower)"; return OVM_ERR_INVALID; }
  TowerConfig tc; memset(&tc, 0, sizeof(tc));
  tc.embed_dim = c.embed_dim; tc.depth = c.depth; tc.heads = c.heads; tc.pos_grid = c.pos_grid; tc.canvas = c.canvas; tc.precision = c.precision;
  tc.max_batch = c.max_batch; tc.sam_window = c.sam_window; tc.sam_global_mask = c.sam_global_mask; tc.family = family_of[c.tower];
  for (int i = 0; i < 3; ++i) { tc.pixel_mean[i] = c.pixel_mean[i]; tc.pixel_std[i] = c.pixel_std[i]; }
  int r;
  if ((r = from_tower(h, t.configure(tc)))) return r;
  const bool p16 = t.patch == 16; h->nlev = p16 ? 4 : 3;   // the patch-16 towers sit behind the 4-level pyramid
  // the scale-4 stage needs D/4 channels in 64-wide k-steps
  if (c.fpn_channels % 64 != 0 || c.max_rois < 1 || (p16 && c.embed_dim % 256 != 0)) { h->err = kErrTowerGeometry; return OVM_ERR_INVALID; }
  h->precision = c.precision; h->C = c.fpn_channels;
  const int D = t.D, C = h->C, G = t.G, G2 = t.G2, B = c.max_batch, R = c.max_rois;
  {
    // 32-bit element offsets of the GEMM kernels, as Tower::load checks its own images: the pyramid's and the heads' largest, before anything is allocated
    const uint64_t side0 = (uint64_t)(p16 ? 4 : 2) * G + 2;          // finest pyramid level, zero-bordered
    const uint64_t worst[] = {(uint64_t)B * side0 * side0 * C * 2,   // 3x3 implicit-GEMM image (int offsets, doubled: limit 2^31 elements)
                              (uint64_t)B * R * C * c.pooler_res * c.pooler_res};   // RoI features, fc1's input
    for (uint64_t w : worst)
      if (w > (1ull << 32)) { h->err = kErrOffsets; return OVM_ERR_CAPACITY; }
  }
  if ((r = from_tower(h, t.load(weights, n_weights, device)))) return r;      // its host-only refusals come before its first device call
  const WeightMap wm(weights, n_weights);
  const int P = t.patch, res = c.pooler_res, F = c.fc_dim;
  h->has_dfuse = !p16 && c.use_depth_fusion && wm.get("backbone.net.depth_fusion.weight");
  if (h->has_dfuse) {
    if ((r = pack_linear(h, wm, "backbone.net.depth_fusion", D, D + 1, &h->dfuse, true, D + 64))) return r;
  }
  // ---- SFP (detectron2 SimpleFeaturePyramid; module names simfp_{log2 stride}.{index in the stage's Sequential}):
  //   scale 4   : ConvT(D, D/2) . LN . GELU . ConvT(D/2, D/4) . conv1x1+LN . conv3x3+LN        (4-level towers only)
  //   scale 2   : ConvT(D, D/2) . conv1x1+LN . conv3x3+LN
  //   scale 1   : conv1x1+LN . conv3x3+LN
  //   scale 0.5 : MaxPool2 . conv1x1+LN . conv3x3+LN
  {
    const int first = 2;                                                // int(log2(7)) = int(log2(4)) = 2
    int li = 0;
    auto sname = [&](int lvl, int idx) { return "backbone.simfp_" + std::to_string(first + lvl) + "." + std::to_string(idx); };
    if (p16) {
      if ((r = pack_convt(h, wm, sname(li, 0), D, D / 2, BIAS_REQUIRED, false, &h->convt4a))) return r;
      if ((r = upload_weight(h, wm, sname(li, 1) + ".weight", D / 2, &h->up_ln_g))) return r;
      if ((r = upload_weight(h, wm, sname(li, 1) + ".bias", D / 2, &h->up_ln_b))) return r;
      if ((r = pack_convt(h, wm, sname(li, 3), D / 2, D / 4, BIAS_REQUIRED, false, &h->convt4b))) return r;
      if ((r = pack_sfp_stage(h, wm, sname(li, 4), sname(li, 5), D / 4, &h->lv[li].st))) return r;
      h->lv[li].side = 4 * G; h->lv[li].stride = (float)P / 4.f; ++li;
    }
    if ((r = pack_convt(h, wm, sname(li, 0), D, D / 2, BIAS_REQUIRED, false, &h->convt))) return r;
    if ((r = pack_sfp_stage(h, wm, sname(li, 1), sname(li, 2), D / 2, &h->lv[li].st))) return r;
    h->lv[li].side = 2 * G; h->lv[li].stride = (float)P / 2.f; ++li;
    if ((r = pack_sfp_stage(h, wm, sname(li, 0), sname(li, 1), D, &h->lv[li].st))) return r;
    h->lv[li].side = G; h->lv[li].stride = (float)P; ++li;
    if ((r = pack_sfp_stage(h, wm, sname(li, 1), sname(li, 2), D, &h->lv[li].st))) return r;
    h->lv[li].side = G / 2; h->lv[li].stride = (float)P * 2.f; ++li;
  }
  // ---- heads
  h->roiK = C * res * res;
  const std::string Q = "roi_heads.cube_head.";
  if ((r = pack_roi_fc(h, wm, Q + "feature_generator.fc1", F, C, res, &h->cube_fc1))) return r;
  if ((r = pack_linear(h, wm, Q + "feature_generator.fc2", F, F, &h->cube_fc2))) return r;
  if ((r = pack_concat(h, wm, {{Q + "bbox_3D_center_deltas", 2}, {Q + "bbox_3D_dims", 3}, {Q + "bbox_3D_pose", 6},
                               {Q + "bbox_3D_center_depth", 1}, {Q + "bbox_3D_uncertainty", 1}}, F, &h->cube_out))) return r;
  h->has_box = wm.get("roi_heads.box_head.fc1.weight") && wm.get("roi_heads.box_predictor.cls_score.weight");
  if (h->has_box) {
    if ((r = pack_roi_fc(h, wm, "roi_heads.box_head.fc1", F, C, res, &h->box_fc1))) return r;
    if ((r = pack_linear(h, wm, "roi_heads.box_head.fc2", F, F, &h->box_fc2))) return r;
    if ((r = pack_concat(h, wm, {{"roi_heads.box_predictor.cls_score", c.num_classes + 1},
                                 {"roi_heads.box_predictor.bbox_pred", c.num_classes * 4}}, F, &h->box_out))) return r;
  }
  h->has_rpn = wm.get("proposal_generator.rpn_head.conv.weight") != nullptr;
  if (h->has_rpn) {
    const std::string P = "proposal_generator.rpn_head.";
    if ((r = pack_conv(h, wm, P + "conv", C, C, 3, BIAS_REQUIRED, &h->rpn_conv))) return r;
    // 1x1 convs: objectness [A][C] then deltas [4A][C]
    if ((r = pack_concat(h, wm, {{P + "objectness_logits", 3}, {P + "anchor_deltas", 12}}, C, &h->rpn_out))) return r;
  }
  // ---- workspace
  const size_t MP = (size_t)B * G2;
  if ((r = salloc(h, &h->DT, MP * D))) return r;
  if ((r = salloc(h, &h->DT4, (size_t)B * (G / 2) * (G / 2) * D))) return r;
  if (h->has_dfuse) {
    if ((r = salloc(h, &h->DF, MP * (D + 64)))) return r;
    if ((r = h->alloc(&h->dtok, MP))) return r;
    if ((r = h->alloc(&h->FUS, MP * D))) return r;
  }
  if ((r = h->alloc(&h->d_meta, (size_t)B))) return r;
  OVM_HIP(h, hipHostMalloc((void**)&h->h_meta, sizeof(ImageMeta) * B));
  const int G2x = 2 * G;
  if ((r = salloc(h, &h->CT, (size_t)B * G2x * G2x * (D / 2)))) return r;
  if (p16) {
    if ((r = salloc(h, &h->CT4a, (size_t)B * G2x * G2x * (D / 2)))) return r;
    if ((r = salloc(h, &h->CT4b, (size_t)B * 4 * G2x * G2x * (D / 4)))) return r;
  }
  for (int l = 0; l < h->nlev; ++l) {
    FpnLevel& f = h->lv[l];
    const size_t px = (size_t)B * f.side * f.side, pxp = (size_t)B * (f.side + 2) * (f.side + 2);
    if ((r = h->alloc(&f.T1, px * C))) return r;
    if ((r = salloc(h, &f.pad, pxp * C, true))) return r;
    if ((r = h->alloc(&f.p, px * C))) return r;
    if (h->has_rpn && (r = salloc(h, &f.rpad, pxp * C, true))) return r;
  }
  const size_t RR = (size_t)R * B;
  if ((r = salloc(h, &h->RF, RR * h->roiK))) return r;
  if ((r = salloc(h, &h->H1, RR * F))) return r;
  if ((r = salloc(h, &h->H2, RR * F))) return r;
  if ((r = h->alloc(&h->HO, RR * 256))) return r;
  if ((r = h->alloc(&h->rec, RR * kRecFloats))) return r;
  if ((r = h->alloc(&h->keep, RR))) return r;
  if ((r = h->alloc(&h->d_bidx, RR))) return r;
  if (h->has_rpn && h->has_box) {
    std::vector<void*> extra;
    int sides[kMaxLevels];
    for (int l = 0; l < h->nlev; ++l) sides[l] = h->lv[l].side;
    r = det2d_alloc(&h->det, B, h->nlev, sides, C, c.num_classes, R, c.rpn_pre_topk, c.rpn_post_topk, c.detections_per_image, &extra);
    for (void* p : extra) h->allocs.push_back(p);
    if (r) { h->err = "det2d workspace allocation failed"; return r; }
  }
  OVM_HIP(h, hipDeviceSynchronize());
  return OVM_OK;
}

static int sfp_branch(OvmHandle* h, const SplitImg& in, int lda, int Bn, const FpnLevel& f, hipStream_t s) {
  const int C = h->C, Hs = f.side, M = Bn * Hs * Hs;
  const SfpStage& st = f.st;
  GemmParams p = gp_base(in, lda, st.c1, M);
  p.C = f.T1; p.ldc = C;
  OVM_TRY(h, gemm(h->tw.ctx, p, EPI_STORE, A_ROWMAJOR, s));
  LnOut o; memset(&o, 0, sizeof(o));
  o.hi = f.pad.hi; o.lo = f.pad.lo; o.ld = C; o.padH = Hs; o.padW = Hs;
  OVM_TRY(h, launch_ln_rows(f.T1, C, M, C, st.n1g, st.n1b, 1e-6f, o, s));
  GemmParams q; memset(&q, 0, sizeof(q));
  q.Ahi = f.pad.hi; q.Alo = f.pad.lo; q.Whi = st.c3.hi; q.Wlo = st.c3.lo;
  q.M = M; q.N = C; q.K = 9 * C; q.cH = Hs; q.cW = Hs; q.cC = C;
  q.C = f.T1; q.ldc = C;                                 // 1x1 output already consumed by the LN above
  OVM_TRY(h, gemm(h->tw.ctx, q, EPI_STORE, A_CONV3X3, s));
  LnOut o2; memset(&o2, 0, sizeof(o2));
  o2.f32 = f.p; o2.ldf = C;
  if (f.rpad.hi) { o2.hi = f.rpad.hi; o2.lo = f.rpad.lo; o2.ld = C; o2.padH = Hs; o2.padW = Hs; }
  OVM_TRY(h, launch_ln_rows(f.T1, C, M, C, st.n3g, st.n3b, 1e-6f, o2, s));
  return OVM_OK;
}

// ConvTranspose2d k2 s2 as a GEMM over the source pixels (EPI_CONVT scatters the 2x2 outputs): [Bn][Gs][Gs][Cin] -> [Bn][2Gs][2Gs][Cout]
static int convt_up(OvmHandle* h, const SplitImg& in, int Cin, int Bn, int Gs, const PackedLin& w, const SplitImg& out, hipStream_t s) {
  GemmParams p = gp_base(in, Cin, w, Bn * Gs * Gs);
  p.Ohi = out.hi; p.Olo = out.lo; p.G = Gs; p.Cout = w.N / 4;
  OVM_TRY(h, gemm(h->tw.ctx, p, EPI_CONVT, A_ROWMAJOR, s));
  return OVM_OK;
}

// The depth prompts a handle cannot take (ovm_backbone_forward, ovm_infer_depth): sets the message, launches nothing.
static int depth_prompt_refusal(OvmHandle* h, const float* prompt_depth, int depth_h, int depth_w) {
  if (!prompt_depth) return OVM_OK;
  if (h->cfg.tower != OVM_TOWER_DINOV2) {
    // detectron2's SimpleFeaturePyramid.forward(x) takes no depth; the fork's RCNN3D passes one to every backbone and
    // would raise a TypeError here: refuse rather than silently drop it
    h->err = "prompt_depth is only defined for the DINOv2 tower (depth_fusion, dino.py:91-105)"; return OVM_ERR_INVALID;
  }
  if (h->tw.nreg) {
    // the reference's fusion takes x[:, 1:] as the patch tokens (dino.py:91-105): with register tokens its torch.cat of [B, C, R + HW]
    // with the [B, 1, HW] depth raises
    h->err = "prompt_depth is not defined for a register-token model (depth fusion takes x[:, 1:] as the patch tokens, dino.py:91-105)"; return OVM_ERR_INVALID;
  }
  if (!h->has_dfuse) { h->err = "prompt_depth given but depth_fusion weights absent / disabled"; return OVM_ERR_INVALID; }
  if (depth_h < 1 || depth_w < 1) { h->err = "prompt_depth needs depth_h >= 1 and depth_w >= 1"; return OVM_ERR_INVALID; }
  return OVM_OK;
}

int ovm_backbone_forward(OvmHandle* h, const OvmImage* images, int32_t B, const float* prompt_depth, int32_t depth_h,
                         int32_t depth_w, float* p2, float* p3, float* p4, ovm_stream_t stream) {
  if (!h) return OVM_ERR_INVALID;
  h->err.clear();
  hipStream_t s = (hipStream_t)stream;
  const OvmConfig& c = h->cfg;
  if (B < 1 || B > c.max_batch) { h->err = "batch exceeds max_batch"; return OVM_ERR_CAPACITY; }
  for (int b = 0; b < B; ++b)
    if (images[b].height > c.canvas || images[b].width > c.canvas || images[b].height < 1 || images[b].width < 1) {
      h->err = "image larger than SQUARE_PAD canvas"; return OVM_ERR_SHAPE;
    }
  OVM_HIP(h, hipSetDevice(h->device));
  fill_meta(h, images, B);
  if (const int r = from_tower(h, h->tw.stage_images(images, B, s))) return r;
  OVM_HIP(h, hipMemcpyAsync(h->d_meta, h->h_meta, sizeof(ImageMeta) * B, hipMemcpyHostToDevice, s));
  h->lastB = B;
  if (const int r = depth_prompt_refusal(h, prompt_depth, depth_h, depth_w)) return r;
  const int rr = backbone_launches(h, B, prompt_depth, depth_h, depth_w, s);
  if (rr) return rr;
  const int C = h->C;
  float* outs[3] = {p2, p3, p4};
  for (int l = 0; l < 3; ++l)
    if (outs[l]) OVM_HIP(h, hipMemcpyAsync(outs[l], h->lv[l].p, (size_t)B * h->lv[l].side * h->lv[l].side * C * 4, hipMemcpyDeviceToDevice, s));
  return OVM_OK;
}

// every kernel launch of the backbone (patch embed .. pyramid), on stream s, shapes fixed by (B, canvas)
static int backbone_launches(OvmHandle* h, int B, const float* prompt_depth, int depth_h, int depth_w, hipStream_t s) {
  const Tower& t = h->tw;
  const int D = t.D, G = t.G, G2 = t.G2, T = t.T;
  if (const int r = from_tower(h, h->tw.launches(B, s))) return r;
  // ---- depth fusion at the last block output (reference dino.py:91-105) ----
  if (prompt_depth) {
    OVM_TRY(h, launch_depth_resize(prompt_depth, B, depth_h, depth_w, G, h->dtok, s));
    OVM_TRY(h, launch_tokens_cast(t.X, B, T, G2, D, D + 64, h->dtok, h->DF.hi, h->DF.lo, s));
    GemmParams p = gp_base(h->DF, D + 64, h->dfuse, B * G2);
    p.C = h->FUS; p.ldc = D;
    OVM_TRY(h, gemm(h->tw.ctx, p, EPI_STORE, A_ROWMAJOR, s));
    OVM_TRY(h, launch_tokens_writeback(t.X, h->FUS, B, T, G2, D, s));
  }
  // ---- dense tokens (no final LayerNorm: reference dino.py:88-110) ----
  OVM_TRY(h, launch_tokens_cast(t.X, B, T, G2, D, D, nullptr, h->DT.hi, h->DT.lo, s));
  // ---- SFP (reference dino.py:143-152,208-224; stages nohup.out:565-596; 4-level form clip.py:155-166) ----
  {
    int li = 0;
    if (h->nlev == 4) {                                    // scale 4: ConvT . LN . GELU . ConvT
      OVM_TRY(h, convt_up(h, h->DT, D, B, G, h->convt4a, h->CT4a, s));
      OVM_TRY(h, launch_ln_gelu_split(h->CT4a.hi, h->CT4a.lo, B * 4 * G2, D / 2, h->up_ln_g, h->up_ln_b, 1e-6f, s));
      OVM_TRY(h, convt_up(h, h->CT4a, D / 2, B, 2 * G, h->convt4b, h->CT4b, s));
      OVM_TRY(h, sfp_branch(h, h->CT4b, D / 4, B, h->lv[li++], s));
    }
    OVM_TRY(h, convt_up(h, h->DT, D, B, G, h->convt, h->CT, s));
    OVM_TRY(h, sfp_branch(h, h->CT, D / 2, B, h->lv[li++], s));
    OVM_TRY(h, sfp_branch(h, h->DT, D, B, h->lv[li++], s));
    OVM_TRY(h, launch_maxpool2(h->DT.hi, h->DT.lo, B, G, D, h->DT4.hi, h->DT4.lo, s));
    OVM_TRY(h, sfp_branch(h, h->DT4, D, B, h->lv[li++], s));
  }
  return OVM_OK;
}

int ovm_backbone_num_levels(const OvmHandle* h) { return h ? h->nlev : OVM_ERR_INVALID; }

int ovm_backbone_level(const OvmHandle* h, int32_t level, const float** data, int32_t* side, float* stride) {
  if (!h || level < 0 || level >= h->nlev) return OVM_ERR_INVALID;
  if (data) *data = h->lv[level].p;
  if (side) *side = h->lv[level].side;
  if (stride) *stride = h->lv[level].stride;
  return OVM_OK;
}

static void roi_params(OvmHandle* h, RoiParams* rp) {
  memset(rp, 0, sizeof(*rp));
  for (int l = 0; l < h->nlev; ++l) {
    rp->feat[l] = h->lv[l].p; rp->fh[l] = rp->fw[l] = h->lv[l].side; rp->scale[l] = 1.0f / h->lv[l].stride;
  }
  rp->C = h->C; rp->nlevels = h->nlev; rp->min_level = h->cfg.pooler_min_level; rp->max_level = h->cfg.pooler_max_level;
  rp->out = h->cfg.pooler_res;
}

int ovm_cube_forward(OvmHandle* h, const OvmImage* images, int32_t B, const float* boxes, const float* scores,
                     const int32_t* classes, const int32_t* image_idx, int32_t n, int32_t postprocess, OvmDet3D* out,
                     int32_t* out_counts, ovm_stream_t stream) {
  if (!h) return OVM_ERR_INVALID;
  h->err.clear();
  hipStream_t s = (hipStream_t)stream;
  if (B < 1 || B > h->cfg.max_batch) { h->err = "batch exceeds max_batch"; return OVM_ERR_CAPACITY; }
  if (n > h->cfg.max_rois * h->cfg.max_batch) { h->err = "n exceeds max_rois*max_batch"; return OVM_ERR_CAPACITY; }
  OVM_HIP(h, hipSetDevice(h->device));
  if (n <= 0) {                                       // roi_heads.py:371-372: nothing to do
    OVM_HIP(h, hipMemsetAsync(out_counts, 0, sizeof(int) * B, s));
    return OVM_OK;
  }
  fill_meta(h, images, B);
  OVM_HIP(h, hipMemcpyAsync(h->d_meta, h->h_meta, sizeof(ImageMeta) * B, hipMemcpyHostToDevice, s));
  h->lastN = n;
  const int F = h->cfg.fc_dim;
  RoiParams rp; roi_params(h, &rp);
  rp.boxes = boxes; rp.batch_idx = image_idx; rp.n = n; rp.Ohi = h->RF.hi; rp.Olo = h->RF.lo; rp.ldo = h->roiK;
  OVM_TRY(h, launch_roi_align(rp, s));
  {
    GemmParams p = gp_base(h->RF, h->roiK, h->cube_fc1, n);
    p.Ohi = h->H1.hi; p.Olo = h->H1.lo; p.ldo = F; p.relu = 1;
    OVM_TRY(h, gemm(h->tw.ctx, p, EPI_STORE, A_ROWMAJOR, s));
  }
  {
    GemmParams p = gp_base(h->H1, F, h->cube_fc2, n);
    p.Ohi = h->H2.hi; p.Olo = h->H2.lo; p.ldo = F; p.relu = 1;
    OVM_TRY(h, gemm(h->tw.ctx, p, EPI_STORE, A_ROWMAJOR, s));
  }
  {
    GemmParams p = gp_base(h->H2, F, h->cube_out, n);
    p.C = h->HO; p.ldc = 16;
    OVM_TRY(h, gemm(h->tw.ctx, p, EPI_STORE, A_ROWMAJOR, s));
  }
  CubeDecodeParams cp; memset(&cp, 0, sizeof(cp));
  cp.head = h->HO; cp.ldh = 16; cp.boxes = boxes; cp.scores = scores; cp.classes = classes; cp.batch_idx = image_idx;
  cp.meta = h->d_meta; cp.n = n; cp.virtual_focal = h->cfg.virtual_focal; cp.rec = h->rec; cp.keep = h->keep;
  cp.postprocess = postprocess;
  OVM_TRY(h, launch_cube_decode(cp, s));
  OVM_TRY(h, launch_compact_records(h->rec, h->keep, n, B, (float*)out, out_counts, s));
  return OVM_OK;
}

int ovm_rpn_box_forward(OvmHandle* h, const OvmImage* images, int32_t B, float* boxes, float* scores, int32_t* classes,
                        int32_t* image_idx, float* scores_full, int32_t* out_counts, ovm_stream_t stream) {
  if (!h) return OVM_ERR_INVALID;
  h->err.clear();
  if (!h->has_rpn || !h->has_box) { h->err = "checkpoint has no RPN / box-head weights"; return OVM_ERR_MISSING_WEIGHT; }
  if (B < 1 || B > h->cfg.max_batch) { h->err = "batch exceeds max_batch"; return OVM_ERR_CAPACITY; }
  hipStream_t s = (hipStream_t)stream;
  OVM_HIP(h, hipSetDevice(h->device));
  fill_meta(h, images, B);
  OVM_HIP(h, hipMemcpyAsync(h->d_meta, h->h_meta, sizeof(ImageMeta) * B, hipMemcpyHostToDevice, s));
  Det2dModel m; memset(&m, 0, sizeof(m));
  m.npass = h->precision; m.B = B; m.C = h->C; m.F = h->cfg.fc_dim; m.roiK = h->roiK;
  m.num_classes = h->cfg.num_classes;
  m.nlev = h->nlev;
  for (int l = 0; l < h->nlev; ++l) { m.rpad[l] = {h->lv[l].rpad.hi, h->lv[l].rpad.lo}; m.stride[l] = h->lv[l].stride; }
  m.rpn_conv_hi = h->rpn_conv.hi; m.rpn_conv_lo = h->rpn_conv.lo; m.rpn_conv_bias = h->rpn_conv.bias;
  m.rpn_out_hi = h->rpn_out.hi; m.rpn_out_lo = h->rpn_out.lo; m.rpn_out_bias = h->rpn_out.bias;
  m.fc1_hi = h->box_fc1.hi; m.fc1_lo = h->box_fc1.lo; m.fc1_bias = h->box_fc1.bias;
  m.fc2_hi = h->box_fc2.hi; m.fc2_lo = h->box_fc2.lo; m.fc2_bias = h->box_fc2.bias;
  m.out_hi = h->box_out.hi; m.out_lo = h->box_out.lo; m.out_bias = h->box_out.bias;
  for (int i = 0; i < kMaxLevels; ++i) m.anchor_sizes[i] = h->cfg.anchor_sizes[i];
  for (int i = 0; i < 3; ++i) m.anchor_ratios[i] = h->cfg.anchor_ratios[i];
  m.pre_topk = h->cfg.rpn_pre_topk; m.post_topk = h->cfg.rpn_post_topk; m.rpn_nms = h->cfg.rpn_nms_thresh;
  m.score_thresh = h->cfg.score_thresh; m.nms_thresh = h->cfg.nms_thresh; m.topk = h->cfg.detections_per_image;
  m.meta = h->d_meta;
  RoiParams rp; roi_params(h, &rp);
  m.roi = rp; m.RF = {h->RF.hi, h->RF.lo}; m.H1 = {h->H1.hi, h->H1.lo}; m.H2 = {h->H2.hi, h->H2.lo}; m.HO = h->HO;
  int r = det2d_forward(m, h->det, boxes, scores, classes, image_idx, scores_full, out_counts, s);
  if (r) { h->err = "det2d_forward failed (" + std::to_string(r) + ")"; return r; }
  return OVM_OK;
}

// RCNN3D.inference for ONE image with the text-prompted head, as one call (SURVEY.md 8b `ovm_infer`; reference
// cubercnn/modeling/meta_arch/rcnn3d.py:79-117 with `category_list`: preprocess -> DINOv2 + SFP -> ROIHeads3DGDINO (GroundingDINO
// network, phrase scores, threshold, NMS, class index: roi_heads_gdino.py:93-171) -> _forward_cube -> detector_postprocess).
// The detector runs on an internal side stream beside the backbone (it reads only the input image); the caller's stream joins it
// before the output glue. One host synchronisation (the number of kept 2D boxes sizes the cube-head launch).
// Everything of ovm_infer behind its argument checks: fork, the two networks, join, glue, cube head. Split off so that EVERY error exit
// (a failed detector or backbone launch, an allocation, the capacity check) passes through one place that drains both streams.
static int infer_forked(OvmHandle* h, OvmGdino* g, const OvmImage* image, const float* prompt_depth, int32_t depth_h, int32_t depth_w,
                        const int32_t* token_ids, int32_t ntok, const int32_t* spans, int32_t n_phrases, float box_threshold,
                        float nms_threshold, OvmDet3D* out, int32_t out_capacity, int32_t* n_out, ovm_stream_t stream, int nq) {
  hipStream_t s = (hipStream_t)stream;
  // fork: detector on the side stream
  OVM_HIP(h, hipEventRecord(h->ev_fork, s));
  OVM_HIP(h, hipStreamWaitEvent(h->side, h->ev_fork, 0));
  int r = ovm_gdino_forward(g, image, token_ids, ntok, nullptr, nullptr, nullptr, (ovm_stream_t)h->side);
  if (r) { h->err = std::string("ovm_gdino_forward: ") + ovm_gdino_last_error(g); return r; }
  OVM_HIP(h, hipEventRecord(h->ev_join, h->side));
  // backbone on the caller's stream
  r = ovm_backbone_forward(h, image, 1, prompt_depth, depth_h, depth_w, nullptr, nullptr, nullptr, stream);
  if (r) return r;
  // join, output glue (three launches on the handle's scratch), kept count to the host (the one synchronisation in front of the
  // cube head, whose grid it sizes), cube head
  OVM_HIP(h, hipStreamWaitEvent(s, h->ev_join, 0));
  const float *logits = nullptr, *gboxes = nullptr; int ld = 0;
  r = ovm_gdino_last_outputs(g, &logits, &gboxes, &ld);
  if (r) { h->err = "detector outputs unavailable"; return r; }
  if (nq <= 2048) {
    const size_t need = gdino_post_ws_bytes(nq, n_phrases);
    if (h->inf_ws_bytes < need) {
      char* q = nullptr;
      if ((r = h->alloc(&q, need + need / 4))) return r;        // (the previous block stays in h->allocs until ovm_destroy)
      h->inf_ws = q; h->inf_ws_bytes = need + need / 4;
    }
    r = launch_gdino_post_ws(logits, nq, ld, gboxes, spans, n_phrases, image->height, image->width, box_threshold, nms_threshold, h->inf_ws,
                             h->inf_ws_bytes, h->inf_boxes, h->inf_scores, h->inf_classes, h->inf_n, s);
  } else {
    r = ovm_gdino_postprocess(logits, nq, ld, gboxes, spans, n_phrases, image->height, image->width, box_threshold, nms_threshold,
                              h->inf_boxes, h->inf_scores, h->inf_classes, h->inf_n, stream);
  }
  if (r) { h->err = "GroundingDINO output glue failed (" + std::to_string(r) + ")"; return r; }
  if (!h->inf_host) OVM_HIP(h, hipHostMalloc((void**)&h->inf_host, 2 * sizeof(int), hipHostMallocDefault));
  OVM_HIP(h, hipMemcpyAsync(&h->inf_host[0], h->inf_n, sizeof(int), hipMemcpyDeviceToHost, s));
  OVM_HIP(h, hipStreamSynchronize(s));
  const int n2d = h->inf_host[0];
  if (n2d > out_capacity) { h->err = "output capacity too small"; return OVM_ERR_CAPACITY; }
  r = ovm_cube_forward(h, image, 1, h->inf_boxes, h->inf_scores, h->inf_classes, h->inf_idx, n2d, 1, out, h->inf_counts, stream);
  if (r) return r;
  OVM_HIP(h, hipMemcpyAsync(&h->inf_host[1], h->inf_counts, sizeof(int), hipMemcpyDeviceToHost, s));
  OVM_HIP(h, hipStreamSynchronize(s));
  *n_out = h->inf_host[1];
  return OVM_OK;
}

// ovm_infer with a depth prompt (reference rcnn3d.py:97: self.backbone(images.tensor, prompt_depth)); a null prompt_depth IS ovm_infer.
int ovm_infer_depth(OvmHandle* h, OvmGdino* g, const OvmImage* image, const float* prompt_depth, int32_t depth_h, int32_t depth_w,
                    const int32_t* token_ids, int32_t ntok, const int32_t* spans, int32_t n_phrases, float box_threshold,
                    float nms_threshold, OvmDet3D* out, int32_t out_capacity, int32_t* n_out, ovm_stream_t stream) {
  if (!h || !g || !image || !token_ids || !out || !n_out) return OVM_ERR_INVALID;
  h->err.clear();
  // the refusals of ovm_backbone_forward, in front of the fork: nothing is launched for a prompt the tower cannot take
  if (const int r = depth_prompt_refusal(h, prompt_depth, depth_h, depth_w)) return r;
  hipStream_t s = (hipStream_t)stream;
  OVM_HIP(h, hipSetDevice(h->device));
  if (!h->side) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    OVM_HIP(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi));      // short kernels: let them jump the ViT's queue
    OVM_HIP(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    OVM_HIP(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  }
  const int nq = ovm_gdino_num_queries(g);
  if (nq <= 0) { h->err = "bad detector handle"; return OVM_ERR_INVALID; }
  if (nq > h->cfg.max_rois * h->cfg.max_batch) { h->err = "detector queries exceed max_rois"; return OVM_ERR_CAPACITY; }
  if (h->inf_cap < nq) {
    int r;
    if ((r = h->alloc(&h->inf_boxes, (size_t)nq * 4)) || (r = h->alloc(&h->inf_scores, (size_t)nq)) || (r = h->alloc(&h->inf_classes, (size_t)nq)) ||
        (r = h->alloc(&h->inf_idx, (size_t)nq, true)) || (r = h->alloc(&h->inf_n, 1)) || (r = h->alloc(&h->inf_counts, 1))) return r;
    h->inf_cap = nq;
  }
  const int r_all = infer_forked(h, g, image, prompt_depth, depth_h, depth_w, token_ids, ntok, spans, n_phrases, box_threshold, nms_threshold, out,
                                 out_capacity, n_out, stream, nq);
  if (r_all != OVM_OK) {
    // The detector may still be running on the side stream, reading the caller's image and the plan arena: the caller is entitled to
    // free or reuse the image once this call has returned, and the next call's fork must not race with leftover work on h->inf_*.
    (void)hipStreamSynchronize(h->side);
    (void)hipStreamSynchronize(s);
  }
  return r_all;
}

int ovm_infer(OvmHandle* h, OvmGdino* g, const OvmImage* image, const int32_t* token_ids, int32_t ntok, const int32_t* spans,
              int32_t n_phrases, float box_threshold, float nms_threshold, OvmDet3D* out, int32_t out_capacity, int32_t* n_out,
              ovm_stream_t stream) {
  return ovm_infer_depth(h, g, image, nullptr, 0, 0, token_ids, ntok, spans, n_phrases, box_threshold, nms_threshold, out, out_capacity, n_out,
                         stream);
}

// Co-run mode: the caller runs other work (the GroundingDINO detector) on a second stream while ovm_backbone_forward executes. The
// attention launches then keep to one 4-wave workgroup per CU (slower alone: 6.8 -> 9.3 ms per ViT-L image) so that the other stream's
// short kernels find free wave slots instead of queueing behind 270-us workgroups; measured end to end 28.3 -> 26.7 ms per image.
int ovm_set_corun(OvmHandle* h, int32_t on) {
  if (!h) return OVM_ERR_INVALID;
  h->tw.corun = on != 0;
  return OVM_OK;
}

int ovm_profile_enable(OvmHandle* h, int32_t on) {
  if (!h) return OVM_ERR_INVALID;
  h->prof.on = on != 0;
  h->prof.mask = (on == 0 || on == 1) ? ~0u : ((unsigned)on >> 1);       // 1 = every category; else bit (c + 1) selects category c
  for (int c = 0; c < OVM_PROF_NCAT; ++c) h->prof.used[c] = 0;
  return OVM_OK;
}

// Sums the elapsed time of every bracketed launch since ovm_profile_enable(h, 1) per category and
// resets the counters. Synchronises the device.
int ovm_profile_read(OvmHandle* h, float* ms, int32_t* launches) {
  if (!h) return OVM_ERR_INVALID;
  OVM_HIP(h, hipSetDevice(h->device));
  OVM_HIP(h, hipDeviceSynchronize());
  for (int c = 0; c < OVM_PROF_NCAT; ++c) {
    double tot = 0.0;
    for (size_t i = 0; i < h->prof.used[c]; ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, h->prof.ev[c][i].first, h->prof.ev[c][i].second) == hipSuccess) tot += t;
    }
    ms[c] = (float)tot; launches[c] = (int32_t)h->prof.used[c];
    h->prof.used[c] = 0;
  }
  return OVM_OK;
}

// RCCL communicator bootstrap for ovm_gather_records (the unique id travels over the host's own
// rendezvous, e.g. torch.distributed's store).
int ovm_comm_unique_id(uint8_t* id128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return OVM_ERR_HIP;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(id128, &id, 128);
  return OVM_OK;
}
int ovm_comm_init(const uint8_t* id128, int32_t rank, int32_t world, int32_t device, void** comm) {
  ncclUniqueId id; memcpy(&id, id128, 128);
  if (hipSetDevice(device) != hipSuccess) return OVM_ERR_HIP;
  ncclComm_t c;
  if (ncclCommInitRank(&c, world, id, rank) != ncclSuccess) return OVM_ERR_HIP;
  *comm = (void*)c;
  return OVM_OK;
}
int ovm_comm_destroy(void* comm) {
  if (comm) ncclCommDestroy((ncclComm_t)comm);
  return OVM_OK;
}

int64_t ovm_debug_copy(OvmHandle* h, const char* name, float* dst, int64_t capacity, ovm_stream_t stream) {
  if (!h || !name) return OVM_ERR_INVALID;
  const int B = h->lastB, C = h->C;
  const float* src = nullptr; int64_t n = 0;
  const std::string k(name);
  if (k == "tokens") { src = h->tw.X; n = (int64_t)B * h->tw.T * h->tw.D; }
  else if (k.size() == 2 && k[0] == 'p' && k[1] >= '2' && k[1] < '2' + h->nlev) {
    const FpnLevel& f = h->lv[k[1] - '2'];
    src = f.p; n = (int64_t)B * f.side * f.side * C;
  }
  // the RPN's per-image proposals after top-k / NMS (boxes [B][R][4], objectness logits [B][R], counts [B] as int32 bits) and the
  // cube head's raw outputs of the last ovm_cube_forward ([n][16]: deltas 2, dims 3, pose 6, depth 1, uncertainty 1) - parity tests
  else if (k == "rpn_boxes" && h->has_rpn && h->has_box) { src = h->det.prop_boxes; n = (int64_t)B * h->det.R * 4; }
  else if (k == "rpn_scores" && h->has_rpn && h->has_box) { src = h->det.prop_scores; n = (int64_t)B * h->det.R; }
  else if (k == "rpn_counts" && h->has_rpn && h->has_box) { src = (const float*)h->det.prop_count; n = B; }
  else if (k == "cube_head") { src = h->HO; n = (int64_t)h->lastN * 16; }
  else { h->err = "unknown debug tensor"; return OVM_ERR_INVALID; }
  if (n > capacity) { h->err = "debug copy capacity too small"; return OVM_ERR_CAPACITY; }
  if (hipMemcpyAsync(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return OVM_ERR_HIP;
  return n;
}

// Counts exchange alone (every rank calls it): lets rank 0 size its receive buffer before ovm_gather_records.
int ovm_gather_counts(void* comm, int32_t rank, int32_t world, int32_t n_send, int32_t* counts_all, ovm_stream_t stream) {
  if (!comm || world < 1 || rank < 0 || rank >= world || !counts_all || n_send < 0) return OVM_ERR_INVALID;
  ncclComm_t cm = (ncclComm_t)comm;
  hipStream_t s = (hipStream_t)stream;
  int* d_counts = nullptr;
  if (hipMalloc((void**)&d_counts, sizeof(int) * (world + 1)) != hipSuccess) return OVM_ERR_HIP;
  int rc = OVM_OK;
  if (hipMemcpyAsync(d_counts + world, &n_send, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) rc = OVM_ERR_HIP;
  else if (ncclAllGather(d_counts + world, d_counts, 1, ncclInt32, cm, s) != ncclSuccess) rc = OVM_ERR_HIP;
  else if (hipMemcpyAsync(counts_all, d_counts, sizeof(int) * world, hipMemcpyDeviceToHost, s) != hipSuccess) rc = OVM_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) rc = OVM_ERR_HIP;
  hipFree(d_counts);
  return rc;
}

// One gather of fixed-width records to rank 0: counts all-gather, then grouped send/recv (a gatherv).
// Every peer uses its own xGMI link to rank 0's GPU; the payload is ~200 B per detection.
int ovm_gather_records(void* comm, int32_t rank, int32_t world, const OvmDet3D* send, int32_t n_send, OvmDet3D* recv,
                       int32_t* counts_all, ovm_stream_t stream) {
  if (!comm || world < 1 || rank < 0 || rank >= world) return OVM_ERR_INVALID;
  ncclComm_t cm = (ncclComm_t)comm;
  hipStream_t s = (hipStream_t)stream;
  int* d_counts = nullptr;
  if (hipMalloc((void**)&d_counts, sizeof(int) * (world + 1)) != hipSuccess) return OVM_ERR_HIP;
  int rc = OVM_OK;
  do {
    if (hipMemcpyAsync(d_counts + world, &n_send, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) { rc = OVM_ERR_HIP; break; }
    if (ncclAllGather(d_counts + world, d_counts, 1, ncclInt32, cm, s) != ncclSuccess) { rc = OVM_ERR_HIP; break; }
    if (hipMemcpyAsync(counts_all, d_counts, sizeof(int) * world, hipMemcpyDeviceToHost, s) != hipSuccess) { rc = OVM_ERR_HIP; break; }
    if (hipStreamSynchronize(s) != hipSuccess) { rc = OVM_ERR_HIP; break; }
    const size_t rb = sizeof(OvmDet3D);
    if (ncclGroupStart() != ncclSuccess) { rc = OVM_ERR_HIP; break; }
    if (rank == 0) {
      size_t off = 0;
      for (int r = 0; r < world; ++r) {
        if (r == 0) {
          if (n_send > 0) hipMemcpyAsync(recv, send, rb * n_send, hipMemcpyDeviceToDevice, s);
        } else if (counts_all[r] > 0) {
          ncclRecv((char*)recv + off * rb, rb * counts_all[r], ncclUint8, r, cm, s);
        }
        off += counts_all[r];
      }
    } else if (n_send > 0) {
      ncclSend(send, rb * n_send, ncclUint8, 0, cm, s);
    }
    if (ncclGroupEnd() != ncclSuccess) { rc = OVM_ERR_HIP; break; }
  } while (0);
  hipStreamSynchronize(s);
  hipFree(d_counts);
  return rc;
}

}  // extern "C"
