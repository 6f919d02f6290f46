// Visualisation: the six-panel evaluation sample of the reference's visualize_from_instances (cubercnn/vis/vis.py:76-296) -
// ground truth of all classes, ground truth of the evaluated classes and predictions, 2D boxes above 3D boxes - composed on the
// device. The rules and the declared deviations are listed in include/ovm3d.h; tests/panels_oracle.py restates them in numpy.
//
// Host (ovm_host_panels_layout, fp64, no GPU): per panel the ordered primitive list - outline segments and name glyphs of the 2D
// boxes; the zplane-clipped, projected cuboid edges, the label rectangle and the label glyphs of the 3D boxes.
//
// Device (ovm_render_panels): one pinned upload of the packed lists and glyph masks, then
//   panels_tiles  one 256-thread workgroup per 16 x 16 tile of one panel. The workgroup streams its panel's primitives through
//                 LDS, 256 at a time: each thread tests one primitive's pixel box against the tile, a ballot and a prefix sum
//                 compact the survivors in list order, and every pixel applies them in that order (segment: overwrite inside the
//                 radius; blend: px * 0.33 + bg * (1 - 0.33), truncated; glyph: overwrite where the mask has ink). One BGR write per
//                 pixel. No list in global memory and no atomics: the order makes the picture.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "../../include/ovm3d.h"
#include "draw.hpp"

#pragma clang fp contract(off)

namespace {

using ovm_draw::iround;
using ovm_draw::project;
using ovm_draw::seg_dist2;
using ovm_draw::to_i64;

// The 12 edges in the order draw_3d_box_from_verts draws them, directed as it clips them (:695).
constexpr int kEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {1, 5}, {5, 6}, {6, 2}, {4, 5}, {4, 7}, {6, 7}, {0, 4}, {3, 7}};
// Corner signs of (l, h, w) along (x, y, z) in get_cuboid_verts_faces' order (math_util.py:172-181).
constexpr int kSign[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}};

constexpr int kTile = 16;
constexpr int kThreads = kTile * kTile;
constexpr int kMaxBoxes = 1 << 16;
constexpr int kMaxGlyph = 4096;
constexpr double kZplane = 0.05, kEps = 1e-4;

struct DPrim {              // one primitive as uploaded
  double a[4];              // segment: clipped x0, y0, x1, y1; blend: background colour (3)
  double r2;                // segment: (thickness / 2)^2
  int64_t goff;             // glyph: offset of the mask
  int32_t bx0, by0, bx1, by1;  // inclusive pixel box on the panel: the cull box, and the blend rectangle itself
  int32_t kind, col;        // col: b0 | b1 << 8 | b2 << 16
  int32_t gx, gy, gw, pad;  // glyph mask top-left and width
};

struct PanelArgs {
  int32_t H, W, tiles_x, tiles;   // tiles: per panel
  int32_t start[OVM_PANELS + 1];
  const DPrim* prims;
  const uint8_t* glyphs;
  const uint8_t* image;
  int64_t image_pitch;
  uint8_t* out;
  int64_t out_pitch;
};

// ------------------------------------------------------------------------------------------------------------------ device

__global__ void __launch_bounds__(kThreads) panels_tiles(PanelArgs A) {
  __shared__ DPrim sh[kThreads];
  __shared__ int wave_cnt[kThreads / 64];
  const int panel = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int tx0 = (tile % A.tiles_x) * kTile, ty0 = (tile / A.tiles_x) * kTile;
  const int x = tx0 + (threadIdx.x % kTile), y = ty0 + (threadIdx.x / kTile);
  const bool live = x < A.W && y < A.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c[3] = {0, 0, 0};
  if (live) {
    const uint8_t* ip = A.image + (int64_t)y * A.image_pitch + 3 * x;
    c[0] = ip[0]; c[1] = ip[1]; c[2] = ip[2];
  }
  const int end = A.start[panel + 1];
  for (int base = A.start[panel]; base < end; base += kThreads) {
    const int i = base + threadIdx.x;
    bool f = false;
    if (i < end) {
      const DPrim& P = A.prims[i];
      f = P.bx0 < tx0 + kTile && P.bx1 >= tx0 && P.by0 < ty0 + kTile && P.by1 >= ty0;
    }
    // order-preserving compaction of the chunk's survivors into LDS
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kThreads / 64; ++w) { off += w < wave ? wave_cnt[w] : 0; tot += wave_cnt[w]; }
    if (f) sh[off + pre] = A.prims[i];
    __syncthreads();
    if (live) {
      for (int k = 0; k < tot; ++k) {
        const DPrim& I = sh[k];
        if (x < I.bx0 || x > I.bx1 || y < I.by0 || y > I.by1) continue;
        if (I.kind == OVM_PANEL_SEGMENT) {
          if (seg_dist2((double)x, (double)y, I.a[0], I.a[1], I.a[2], I.a[3]) <= I.r2) {
            c[0] = I.col & 255; c[1] = (I.col >> 8) & 255; c[2] = (I.col >> 16) & 255;
          }
        } else if (I.kind == OVM_PANEL_BLEND) {
          for (int ch = 0; ch < 3; ++ch) c[ch] = (int)((double)c[ch] * 0.33 + I.a[ch] * (1.0 - 0.33));
        } else if (A.glyphs[I.goff + (int64_t)(y - I.gy) * I.gw + (x - I.gx)]) {
          c[0] = I.col & 255; c[1] = (I.col >> 8) & 255; c[2] = (I.col >> 16) & 255;
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  const int prow = panel / 3, pcol = panel % 3;
  uint8_t* op = A.out + ((int64_t)prow * A.H + y) * A.out_pitch + 3 * ((int64_t)pcol * A.W + x);
  op[0] = (uint8_t)c[0]; op[1] = (uint8_t)c[1]; op[2] = (uint8_t)c[2];
}

// -------------------------------------------------------------------------------------------------------------------- host

bool finite_all(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

bool box_ok(const OvmPanelBox& b) {
  if (!finite_all(b.bbox, 4) || !finite_all(b.center, 3) || !finite_all(b.dims, 3) || !finite_all(b.R, 9)) return false;
  for (int k = 0; k < 2; ++k)
    if (b.glyph2d[k] < 0 || b.glyph2d[k] > kMaxGlyph || b.glyph3d[k] < 0 || b.glyph3d[k] > kMaxGlyph) return false;
  return true;
}

struct Emit {
  OvmPanelPrim* out;
  int64_t cap, n;
  void push(const OvmPanelPrim& p) {
    if (n < cap) out[n] = p;
    ++n;
  }
};

OvmPanelPrim prim(int kind, int box, const uint8_t* col, int64_t a0, int64_t a1, int64_t a2, int64_t a3) {
  OvmPanelPrim p{};
  p.kind = kind; p.box = box;
  p.a[0] = a0; p.a[1] = a1; p.a[2] = a2; p.a[3] = a3;
  p.color[0] = col[0]; p.color[1] = col[1]; p.color[2] = col[2];
  return p;
}

// The outline and the class name of one 2D box (:175-179).
void emit_2d(const OvmPanelBox& b, int idx, int64_t goff, Emit* e) {
  const int64_t x1 = to_i64(b.bbox[0]), y1 = to_i64(b.bbox[1]);
  const int64_t x2 = to_i64(b.bbox[0] + b.bbox[2]), y2 = to_i64(b.bbox[1] + b.bbox[3]);
  const int64_t seg[4][4] = {{x1, y1, x2, y1}, {x2, y1, x2, y2}, {x2, y2, x1, y2}, {x1, y2, x1, y1}};
  for (int k = 0; k < 4; ++k) {
    OvmPanelPrim p = prim(OVM_PANEL_SEGMENT, idx, b.color, seg[k][0], seg[k][1], seg[k][2], seg[k][3]);
    p.thickness = 2;
    e->push(p);
  }
  const int gw = b.glyph2d[0], gh = b.glyph2d[1];
  if (gw > 0 && gh > 0) {
    OvmPanelPrim p = prim(OVM_PANEL_GLYPH, idx, b.color, x1, y1 - 10 - gh, gw, gh);
    p.glyph_offset = goff;
    e->push(p);
  }
}

// The cuboid's edges (:695-728) and its label (:755-783).
void emit_3d(const OvmPanelBox& b, int idx, int64_t goff, const double* K, int H, int W, int thickness, Emit* e) {
  double v[8][3];
  for (int k = 0; k < 8; ++k) {
    const double lx = kSign[k][0] * b.dims[2] / 2, ly = kSign[k][1] * b.dims[1] / 2, lz = kSign[k][2] * b.dims[0] / 2;
    for (int d = 0; d < 3; ++d) v[k][d] = (b.R[3 * d] * lx + b.R[3 * d + 1] * ly + b.R[3 * d + 2] * lz) + b.center[d];
  }
  for (int ed = 0; ed < 12; ++ed) {
    double v0[3], v1[3];
    for (int d = 0; d < 3; ++d) { v0[d] = v[kEdge[ed][0]][d]; v1[d] = v[kEdge[ed][1]][d]; }
    const double z0 = v0[2], z1 = v1[2];
    if (!(z0 >= kZplane || z1 >= kZplane)) continue;
    const double den = (z1 - z0) > kEps ? (z1 - z0) : kEps;
    const double s = (kZplane - z0) / den;
    double nv[3];
    for (int d = 0; d < 3; ++d) nv[d] = v0[d] + s * (v1[d] - v0[d]);
    if (z0 < kZplane && z1 >= kZplane) std::memcpy(v0, nv, sizeof nv);
    else if (z0 >= kZplane && z1 < kZplane) std::memcpy(v1, nv, sizeof nv);
    double u0[2], u1[2];
    project(K, v0, v0[2] > kEps ? v0[2] : kEps, u0);
    project(K, v1, v1[2] > kEps ? v1[2] : kEps, u1);
    OvmPanelPrim p = prim(OVM_PANEL_SEGMENT, idx, b.color, to_i64(u0[0]), to_i64(u0[1]), to_i64(u1[0]), to_i64(u1[1]));
    p.thickness = thickness;
    e->push(p);
  }
  const int gw = b.glyph3d[0], gh = b.glyph3d[1];
  if (gw <= 0 || gh <= 0) return;
  const int64_t p0 = to_i64(b.bbox[0]), p1 = to_i64(b.bbox[1]);
  auto clip = [](int64_t a, int64_t hi) { return a < 0 ? (int64_t)0 : (a > hi ? hi : a); };
  const int64_t xs = clip(p0, W), xe = clip(xs + gw - 1 + 4, W), ys = clip(p1 - gh - 2, H), ye = clip(p1 + 1 - 2, H);
  const int64_t rx1 = std::min<int64_t>(xe + 1, W), ry1 = std::min<int64_t>(ye + 1, H);
  if (rx1 > xs && ry1 > ys) e->push(prim(OVM_PANEL_BLEND, idx, b.color, xs, ys, rx1, ry1));
  const double mean = (((double)b.color[0] + (double)b.color[1]) + (double)b.color[2]) / 3;
  const uint8_t t = mean > 127.5 ? 0 : 255;
  const uint8_t tc[3] = {t, t, t};
  OvmPanelPrim g = prim(OVM_PANEL_GLYPH, idx, tc, clip(p0 + 2, W), clip(p1 - 2, H) - gh, gw, gh);
  g.glyph_offset = goff;
  e->push(g);
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool layout_ok(const OvmPanelsLayout* L) {
  if (!L || L->height <= 0 || L->width <= 0 || L->height > 32768 || L->width > 32768 || L->n_prims < 0 || L->glyph_bytes < 0)
    return false;
  if (L->start[0] != 0 || L->start[OVM_PANELS] != L->n_prims) return false;
  for (int p = 0; p < OVM_PANELS; ++p)
    if (L->start[p + 1] < L->start[p]) return false;
  return true;
}

size_t prim_bytes(const OvmPanelsLayout* L) { return align256(sizeof(DPrim) * (size_t)L->n_prims); }
size_t total_bytes(const OvmPanelsLayout* L) { return prim_bytes(L) + align256((size_t)L->glyph_bytes) + 256; }

// One primitive packed for the device; 0: nothing of it is on the panel, -1: out of range.
int pack(const OvmPanelPrim& p, int H, int W, int64_t glyph_bytes, DPrim* d) {
  std::memset(d, 0, sizeof *d);
  d->kind = p.kind;
  d->col = p.color[0] | (p.color[1] << 8) | (p.color[2] << 16);
  if (p.kind == OVM_PANEL_SEGMENT) {
    if (p.thickness < 1 || p.thickness > kMaxGlyph) return -1;
    const double r = p.thickness / 2.0;
    int32_t bb[4];
    if (!ovm_draw::clip_segment((double)p.a[0], (double)p.a[1], (double)p.a[2], (double)p.a[3], r, W, H, d->a, bb)) return 0;
    d->r2 = r * r;
    d->bx0 = bb[0]; d->by0 = bb[1]; d->bx1 = bb[2]; d->by1 = bb[3];
    return 1;
  }
  if (p.kind == OVM_PANEL_BLEND) {
    if (p.a[0] < 0 || p.a[1] < 0 || p.a[2] > W || p.a[3] > H) return -1;
    if (p.a[2] <= p.a[0] || p.a[3] <= p.a[1]) return 0;
    for (int k = 0; k < 3; ++k) d->a[k] = (double)p.color[k];
    d->bx0 = (int32_t)p.a[0]; d->by0 = (int32_t)p.a[1]; d->bx1 = (int32_t)p.a[2] - 1; d->by1 = (int32_t)p.a[3] - 1;
    return 1;
  }
  if (p.kind == OVM_PANEL_GLYPH) {
    const int64_t gw = p.a[2], gh = p.a[3];
    if (gw < 1 || gh < 1 || gw > kMaxGlyph || gh > kMaxGlyph || p.glyph_offset < 0 || p.glyph_offset + gw * gh > glyph_bytes) return -1;
    if (p.a[0] >= W || p.a[1] >= H || p.a[0] <= -gw || p.a[1] <= -gh) return 0;   // also keeps gx, gy in int32
    d->gx = (int32_t)p.a[0]; d->gy = (int32_t)p.a[1]; d->gw = (int32_t)gw;
    d->goff = p.glyph_offset;
    d->bx0 = std::max(d->gx, 0); d->by0 = std::max(d->gy, 0);
    d->bx1 = (int32_t)std::min<int64_t>(p.a[0] + gw, W) - 1; d->by1 = (int32_t)std::min<int64_t>(p.a[1] + gh, H) - 1;
    return 1;
  }
  return -1;
}

std::mutex g_stage_mu;
uint8_t* g_stage = nullptr;      // pinned upload buffer, reused once the previous upload has left it
size_t g_stage_cap = 0;
hipEvent_t g_stage_ev = nullptr;

}  // namespace

extern "C" {

int ovm_host_panels_layout(const OvmPanelsInput* in, OvmPanelsLayout* L, OvmPanelPrim* prims, int32_t prim_capacity) {
  if (!in || !L || prim_capacity < 0 || (prim_capacity > 0 && !prims)) return OVM_ERR_INVALID;
  const int H = in->height, W = in->width, ng = in->n_gt, np = in->n_pred;
  if (H <= 0 || W <= 0 || H > 32768 || W > 32768 || ng < 0 || np < 0 || ng > kMaxBoxes || np > kMaxBoxes) return OVM_ERR_INVALID;
  if ((ng > 0 && !in->gt) || (np > 0 && !in->pred) || !finite_all(in->K, 9)) return OVM_ERR_INVALID;
  for (int i = 0; i < ng; ++i)
    if (!box_ok(in->gt[i])) return OVM_ERR_INVALID;
  for (int i = 0; i < np; ++i)
    if (!box_ok(in->pred[i])) return OVM_ERR_INVALID;

  std::memset(L, 0, sizeof *L);
  L->height = H; L->width = W;
  L->thickness3d = std::max(1, iround(3.0 * H / 500));
  // glyph buffer: per box its 2D mask, then its 3D mask; ground truth first
  int64_t cur = 0;
  auto offsets = [&](const OvmPanelBox& b, int64_t* o2, int64_t* o3) {
    *o2 = cur; cur += (int64_t)b.glyph2d[0] * b.glyph2d[1];
    *o3 = cur; cur += (int64_t)b.glyph3d[0] * b.glyph3d[1];
  };
  Emit e{prims, prim_capacity, 0};
  for (int panel = 0; panel < OVM_PANELS; ++panel) {
    L->start[panel] = (int32_t)e.n;
    const bool is_pred = panel % 3 == 2, eval_only = panel % 3 == 1, is_3d = panel >= 3;
    const OvmPanelBox* boxes = is_pred ? in->pred : in->gt;
    const int n = is_pred ? np : ng;
    cur = 0;
    if (is_pred)
      for (int i = 0; i < ng; ++i) { int64_t a, b; offsets(in->gt[i], &a, &b); }
    for (int i = 0; i < n; ++i) {
      int64_t o2, o3;
      offsets(boxes[i], &o2, &o3);
      if (eval_only && !boxes[i].in_eval) continue;
      if (!is_3d) emit_2d(boxes[i], i, o2, &e);
      else if (boxes[i].draw3d) emit_3d(boxes[i], i, o3, in->K, H, W, L->thickness3d, &e);
    }
    if (e.n > INT32_MAX) return OVM_ERR_INVALID;
  }
  cur = 0;
  for (int i = 0; i < ng; ++i) { int64_t a, b; offsets(in->gt[i], &a, &b); }
  for (int i = 0; i < np; ++i) { int64_t a, b; offsets(in->pred[i], &a, &b); }
  L->glyph_bytes = cur;
  L->start[OVM_PANELS] = (int32_t)e.n;
  L->n_prims = (int32_t)e.n;
  return e.n > prim_capacity ? OVM_ERR_CAPACITY : OVM_OK;
}

int ovm_render_panels_workspace(const OvmPanelsLayout* layout, int64_t* bytes) {
  if (!layout_ok(layout) || !bytes) return OVM_ERR_INVALID;
  *bytes = (int64_t)total_bytes(layout);
  return OVM_OK;
}

int ovm_render_panels(const OvmPanelsLayout* L, const OvmPanelPrim* prims, const uint8_t* glyphs, int64_t glyph_bytes,
                      const uint8_t* image, int64_t image_pitch, uint8_t* mosaic, int64_t mosaic_pitch, void* workspace,
                      int64_t workspace_bytes, ovm_stream_t stream) {
  if (!layout_ok(L) || glyph_bytes != L->glyph_bytes || (glyph_bytes > 0 && !glyphs) || (L->n_prims > 0 && !prims) || !image ||
      !mosaic || !workspace)
    return OVM_ERR_INVALID;
  const int H = L->height, W = L->width;
  if (image_pitch < 3 * (int64_t)W || mosaic_pitch < 9 * (int64_t)W) return OVM_ERR_INVALID;
  if (workspace_bytes < (int64_t)total_bytes(L)) return OVM_ERR_CAPACITY;
  const size_t pb = prim_bytes(L), staged = pb + align256((size_t)glyph_bytes);

  std::lock_guard<std::mutex> lock(g_stage_mu);
  if (g_stage_ev) {
    if (hipEventSynchronize(g_stage_ev) != hipSuccess) return OVM_ERR_HIP;
  } else if (hipEventCreateWithFlags(&g_stage_ev, hipEventDisableTiming) != hipSuccess) {
    return OVM_ERR_HIP;
  }
  if (g_stage_cap < staged) {
    if (g_stage) (void)hipHostFree(g_stage);
    g_stage = nullptr; g_stage_cap = 0;
    if (hipHostMalloc((void**)&g_stage, staged, hipHostMallocPortable) != hipSuccess) { g_stage = nullptr; return OVM_ERR_HIP; }
    g_stage_cap = staged;
  }
  PanelArgs A{};
  DPrim* dp = reinterpret_cast<DPrim*>(g_stage);
  int n = 0;
  for (int p = 0; p < OVM_PANELS; ++p) {
    A.start[p] = n;
    for (int i = L->start[p]; i < L->start[p + 1]; ++i) {
      const int rc = pack(prims[i], H, W, glyph_bytes, &dp[n]);
      if (rc < 0) return OVM_ERR_INVALID;
      n += rc;
    }
  }
  A.start[OVM_PANELS] = n;
  if (glyph_bytes > 0) std::memcpy(g_stage + pb, glyphs, (size_t)glyph_bytes);

  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  if (staged > 0) {
    if (hipMemcpyAsync(ws, g_stage, staged, hipMemcpyHostToDevice, s) != hipSuccess) return OVM_ERR_HIP;
    if (hipEventRecord(g_stage_ev, s) != hipSuccess) return OVM_ERR_HIP;
  }
  A.H = H; A.W = W;
  A.tiles_x = (W + kTile - 1) / kTile;
  A.tiles = A.tiles_x * ((H + kTile - 1) / kTile);
  A.prims = reinterpret_cast<const DPrim*>(ws);
  A.glyphs = ws + pb;
  A.image = image; A.image_pitch = image_pitch;
  A.out = mosaic; A.out_pitch = mosaic_pitch;
  panels_tiles<<<OVM_PANELS * A.tiles, kThreads, 0, s>>>(A);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
