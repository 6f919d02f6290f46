// Visualisation: draw_scene_view of the reference (cubercnn/vis/vis.py:309-640) - the front view (boxes rendered, blended and
// outlined over the image) and the top-down novel view (the same boxes over a ground grid) - with every pixel made on the device.
//
// Host (ovm_host_scene_layout, fp64, no GPU): the small per-scene geometry, in the reference's operation order - per-view box
// frames, the depth order, the zoom search (:442-478), the two passes of the ground bounds (:488-533), the deduplicated integer
// grid segments (:557-579), edge endpoints after the zplane clip (:696-716) and the label rectangles (:762-784).
//
// Device (ovm_render_scene): one pinned upload of the packed scene, then
//   scene_setup   one thread per (view, triangle): vertex normals (pytorch3d: normalised sum of the incident faces' cross
//                 products), Sutherland-Hodgman clip against z >= zplane (declared deviation), projection under K, pixel bbox;
//   scene_tiles   one 256-thread workgroup per 16 x 16 tile of either view. The workgroup culls, chunk by chunk and in order, the
//                 triangles, the grid segments and the (edge, label) items against its tile into an LDS list (ballot + prefix
//                 sum keeps the draw order); every pixel then runs the z-test (nearest camera z, lower triangle index on a tie),
//                 Phong shading and softmax_rgb_blend of the winner, the silhouette blend or canvas, then the edges and labels
//                 strictly in draw order (a label background blends over earlier boxes' edges), the overlay, and one BGR write.
// Coverage and depth are fp64 with contraction off, as in the numpy restatement; shading is fp32 as in pytorch3d.
//
// Point cloud (ovm_render_scene_points; a layer of this project, the reference has none): between the upload and the two kernels
//   scene_splat   one thread per pixel of the front image: the pixel's metric depth un-projected under the front K, moved into the
//                 novel frame as the layout moves box corners, projected under the novel K, and its key (float bits of the novel z,
//                 source index) written with a 64-bit atomicMin into a scale x scale buffer over a point_size square. The minimum
//                 does not depend on the execution order (nor does the read that, for point_size > 1, skips an atomic that could not
//                 lower the stored key). All fp64, contraction off (tests/scene_points_oracle.py restates it).
//   scene_tiles   reads that buffer where a novel-view pixel has no triangle: the winner's image colour, tinted by its box, takes
//                 the place of the canvas / grid grey. With the buffer pointer null the kernel is ovm_render_scene's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/ovm3d.h"
#include "draw.hpp"

#pragma clang fp contract(off)

namespace {

using ovm_draw::clampd;
using ovm_draw::iround;
using ovm_draw::project;
using ovm_draw::seg_dist2;
using ovm_draw::to_i64;

// Each face of the cuboid as its four corners in the reference's (inward) winding, the first-to-third corner being the split
// diagonal (get_cuboid_verts_faces, math_util.py:190-209): front 0-2, right 1-6, left 4-3, back 5-7, top 4-1, bottom 3-6.
// Triangle 2f is (a, b, c), triangle 2f+1 is (c, d, a); the front face's (v1 - v0) x (v2 - v0) points +z.
constexpr int kQuad[6][4] = {{0, 1, 2, 3}, {1, 5, 6, 2}, {4, 0, 3, 7}, {5, 4, 7, 6}, {4, 5, 1, 0}, {3, 2, 6, 7}};
// The 12 edges, directed as the reference clips them (the clip formula is not symmetric in the endpoints).
constexpr int kEdge[12][2] = {{0, 1}, {0, 4}, {1, 2}, {1, 5}, {2, 3}, {3, 0}, {3, 7}, {4, 5}, {4, 7}, {5, 6}, {6, 2}, {6, 7}};

__host__ __device__ inline int tri_vert(int t, int k) {
  const int f = t >> 1;
  return (t & 1) ? kQuad[f][(k + 2) & 3] : kQuad[f][k];
}

constexpr int kTile = 16;
constexpr int kThreads = kTile * kTile;

struct DBox {            // one box in one view, as uploaded
  double v[8][3];
  float c[3];
  int32_t pad;
};

struct DTri {            // one (possibly clipped) triangle
  double x[3], y[3], z[3];  // image point (u, v) and camera z per vertex
  float p[9], n[9];         // camera-space point and vertex normal per vertex
  float c[3];
  int32_t key;              // (box * 12 + tri) * 2 + sub: ascending = pytorch3d's face index order
  int32_t bx0, by0, bx1, by1;  // inclusive pixel bbox, empty when bx0 > bx1
};

struct DItem {           // edge segment (kind 0) or label (kind 1), in draw order; grid segments use kind 0
  double a[4];              // segment: x0, y0, x1, y1 (integer pixel centres); label: background colour (3)
  double r2;                // segment: (thickness / 2)^2
  int32_t bx0, by0, bx1, by1;  // inclusive cull bbox
  int32_t kind, col;        // col: segment colour b0 | b1 << 8 | b2 << 16; label: text colour
  int32_t rx0, ry0, rx1, ry1;  // label background, half-open
  int32_t gx, gy, gw, gh;   // label glyph mask top-left and size
  int64_t goff;
};

struct ViewArgs {
  int32_t H, W, tiles_x, tiles;   // tiles: tile count of this view (0: not drawn)
  int32_t ntri, nitem, ngrid;     // counts (ntri = triangle slots)
  int32_t front;                  // 1 front, 0 novel
  const DTri* tri;
  const DItem* item;
  const DItem* grid;
  uint8_t* out;
  int64_t out_pitch;
};

struct SceneArgs {
  ViewArgs v[2];
  const uint8_t* image;
  int64_t image_pitch;
  const uint8_t* glyphs;
  int32_t early_return, render_front;   // render_front: blend_weight > 0
  double bw, one_minus_bw, bwo, one_minus_bwo;
  int32_t overlay;
  // point cloud under the boxes of the novel view (ovm_render_scene_points); zbuf null: none
  const unsigned long long* zbuf;       // [novel H][novel W] keys, all ones = no point
  const int32_t* labels;                // box index per front pixel or null
  int64_t labels_pitch;
  const uint8_t* tint;                  // [n_boxes][4] edge colours
  int32_t img_w, n_boxes;
};

struct SplatArgs {
  const float* depth;
  int64_t depth_pitch;
  unsigned long long* zbuf;
  int32_t H, W, S, half;                // front image size, novel canvas, (point_size - 1) / 2
  double fx, cx, fy, cy;                // front K[0], K[2], K[4], K[5]
  double R[9], c[3], shift, zplane, Kn[9];
};

inline __host__ __device__ void rotate(const double* R, const double* c, const double* p, double* r) {
  const double d0 = p[0] - c[0], d1 = p[1] - c[1], d2 = p[2] - c[2];
  r[0] = R[0] * d0 + R[1] * d1 + R[2] * d2;
  r[1] = R[3] * d0 + R[4] * d1 + R[5] * d2;
  r[2] = R[6] * d0 + R[7] * d1 + R[8] * d2;
}

// ------------------------------------------------------------------------------------------------------------------ device

__global__ void __launch_bounds__(64) scene_setup(const DBox* __restrict__ boxes, int n, double zplane, ViewArgs v0, ViewArgs v1,
                                                   const double* __restrict__ Kv, DTri* __restrict__ tri0, DTri* __restrict__ tri1,
                                                   int nviews_mask) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * n * 12) return;
  const int view = gid / (n * 12);
  const int t = gid % (n * 12);
  const int b = t / 12, tt = t % 12;
  DTri* out = (view == 0 ? tri0 : tri1) + 2 * t;
  const ViewArgs& va = view == 0 ? v0 : v1;
  if (!((nviews_mask >> view) & 1)) return;
  const DBox& bx = boxes[view * n + b];
  const double* K = Kv + 9 * view;
  // vertex normals of this triangle's corners: sum over the box's 12 triangles that use the corner
  double P[3][3], N[3][3];
  for (int k = 0; k < 3; ++k) {
    const int vi = tri_vert(tt, k);
    for (int d = 0; d < 3; ++d) P[k][d] = bx.v[vi][d];
    double s[3] = {0.0, 0.0, 0.0};
    for (int f = 0; f < 12; ++f) {
      const int a0 = tri_vert(f, 0), a1 = tri_vert(f, 1), a2 = tri_vert(f, 2);
      if (a0 != vi && a1 != vi && a2 != vi) continue;
      const double e1[3] = {bx.v[a1][0] - bx.v[a0][0], bx.v[a1][1] - bx.v[a0][1], bx.v[a1][2] - bx.v[a0][2]};
      const double e2[3] = {bx.v[a2][0] - bx.v[a0][0], bx.v[a2][1] - bx.v[a0][1], bx.v[a2][2] - bx.v[a0][2]};
      s[0] += e1[1] * e2[2] - e1[2] * e2[1];
      s[1] += e1[2] * e2[0] - e1[0] * e2[2];
      s[2] += e1[0] * e2[1] - e1[1] * e2[0];
    }
    const double len = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double inv = 1.0 / (len > 1e-6 ? len : 1e-6);
    for (int d = 0; d < 3; ++d) N[k][d] = s[d] * inv;
  }
  // clip the polygon against z >= zplane (point and normal interpolated along the cut edge)
  double Q[4][6];
  int nq = 0;
  for (int k = 0; k < 3; ++k) {
    const int k2 = (k + 1) % 3;
    const bool in1 = P[k][2] >= zplane, in2 = P[k2][2] >= zplane;
    if (in1) {
      for (int d = 0; d < 3; ++d) { Q[nq][d] = P[k][d]; Q[nq][3 + d] = N[k][d]; }
      ++nq;
    }
    if (in1 != in2) {
      const double s = (zplane - P[k][2]) / (P[k2][2] - P[k][2]);
      for (int d = 0; d < 3; ++d) {
        Q[nq][d] = P[k][d] + s * (P[k2][d] - P[k][d]);
        Q[nq][3 + d] = N[k][d] + s * (N[k2][d] - N[k][d]);
      }
      Q[nq][2] = zplane;
      ++nq;
    }
  }
  for (int sub = 0; sub < 2; ++sub) {
    DTri r;
    r.key = 2 * t + sub;
    r.bx0 = 1; r.bx1 = 0; r.by0 = 1; r.by1 = 0;
    r.c[0] = bx.c[0]; r.c[1] = bx.c[1]; r.c[2] = bx.c[2];
    if (sub + 3 <= nq) {
      const int idx[3] = {0, sub + 1, sub + 2};
      double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
      for (int k = 0; k < 3; ++k) {
        const double* q = Q[idx[k]];
        const double z = q[2];
        r.x[k] = (K[0] * q[0] + K[1] * q[1] + K[2] * q[2]) / z;
        r.y[k] = (K[3] * q[0] + K[4] * q[1] + K[5] * q[2]) / z;
        r.z[k] = z;
        for (int d = 0; d < 3; ++d) { r.p[3 * k + d] = (float)q[d]; r.n[3 * k + d] = (float)q[3 + d]; }
        mnx = fmin(mnx, r.x[k]); mxx = fmax(mxx, r.x[k]); mny = fmin(mny, r.y[k]); mxy = fmax(mxy, r.y[k]);
      }
      const double area = (r.x[1] - r.x[0]) * (r.y[2] - r.y[0]) - (r.y[1] - r.y[0]) * (r.x[2] - r.x[0]);
      // pixel j samples u = j + 0.5: j in [ceil(min - 0.5), floor(max - 0.5)], clamped to the canvas
      const double jx0 = fmax(ceil(mnx - 0.5), 0.0), jx1 = fmin(floor(mxx - 0.5), (double)(va.W - 1));
      const double jy0 = fmax(ceil(mny - 0.5), 0.0), jy1 = fmin(floor(mxy - 0.5), (double)(va.H - 1));
      if (area != 0.0 && jx0 <= jx1 && jy0 <= jy1) {
        r.bx0 = (int)jx0; r.bx1 = (int)jx1; r.by0 = (int)jy0; r.by1 = (int)jy1;
      }
    }
    out[sub] = r;
  }
}

// Pass A of the point cloud: one thread per front pixel (row blockIdx.y). Every write lands inside the S x S key buffer.
__global__ void __launch_bounds__(kThreads) scene_splat(SplatArgs P) {
  const int j = blockIdx.x * kThreads + threadIdx.x, i = blockIdx.y;
  if (j >= P.W || i >= P.H) return;
  const float df = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(P.depth) + (int64_t)i * P.depth_pitch + 4 * (int64_t)j);
  if (!(isfinite(df) && df > 0.0f)) return;
  const double d = (double)df;
  const double p[3] = {((j + 0.5) - P.cx) / P.fx * d, ((i + 0.5) - P.cy) / P.fy * d, d};
  double r[3], u[2];
  rotate(P.R, P.c, p, r);
  r[2] = r[2] + P.shift;
  if (!(r[2] >= P.zplane && r[2] > 0.0)) return;
  project(P.Kn, r, r[2], u);
  const double tx = floor(u[0]), ty = floor(u[1]);
  const double lo = -(double)P.half, hi = (double)(P.S - 1 + P.half);
  if (!(tx >= lo && tx <= hi && ty >= lo && ty <= hi)) return;           // NaN, infinite or no pixel of the footprint on the canvas
  const int x = (int)tx, y = (int)ty;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)r[2]) << 32) | (unsigned int)(i * P.W + j);
  const int x0 = x - P.half > 0 ? x - P.half : 0, x1 = x + P.half < P.S - 1 ? x + P.half : P.S - 1;
  const int y0 = y - P.half > 0 ? y - P.half : 0, y1 = y + P.half < P.S - 1 ? y + P.half : P.S - 1;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      // keys only ever fall, so a (possibly stale) read at or below this key proves the atomic would change nothing. Footprints of
      // neighbouring points overlap, single pixels hardly: at point_size 1 the read costs more than it saves (profiles/scene_points)
      unsigned long long* z = P.zbuf + (int64_t)yy * P.S + xx;
      if (P.half == 0 || *z > key) atomicMin(z, key);
    }
}

// Order-preserving compaction of the chunk [base, base + kThreads) into list[]; returns the count.
__device__ inline int cull(bool flag, int idx, int* list, int* wave_cnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < kThreads / 64; ++w) { off += w < wave ? wave_cnt[w] : 0; tot += wave_cnt[w]; }
  if (flag) list[off + pre] = idx;
  __syncthreads();
  return tot;
}

__device__ inline bool overlaps(int bx0, int by0, int bx1, int by1, int tx0, int ty0) {
  return bx0 <= bx1 && by0 <= by1 && bx0 < tx0 + kTile && bx1 >= tx0 && by0 < ty0 + kTile && by1 >= ty0;
}

__device__ inline float3 nrm(float x, float y, float z) {
  const float l = sqrtf(x * x + y * y + z * z);
  const float inv = 1.0f / (l > 1e-6f ? l : 1e-6f);
  return make_float3(x * inv, y * inv, z * inv);
}

// Phong shading (SoftPhongShader, PointLights at the origin, default Materials) + softmax_rgb_blend for one face per pixel.
__device__ inline void shade(const DTri& T, double px, double py, double b0, double b1, double b2, double z, float ndc_per_px,
                             int out[3]) {
  const float w0 = (float)b0, w1 = (float)b1, w2 = (float)b2;
  const float p0 = w0 * T.p[0] + w1 * T.p[3] + w2 * T.p[6];
  const float p1 = w0 * T.p[1] + w1 * T.p[4] + w2 * T.p[7];
  const float p2 = w0 * T.p[2] + w1 * T.p[5] + w2 * T.p[8];
  const float3 n = nrm(w0 * T.n[0] + w1 * T.n[3] + w2 * T.n[6], w0 * T.n[1] + w1 * T.n[4] + w2 * T.n[7],
                       w0 * T.n[2] + w1 * T.n[5] + w2 * T.n[8]);
  const float3 l = nrm(-p0, -p1, -p2);   // light and camera both at the origin: l = v
  const float nl = n.x * l.x + n.y * l.y + n.z * l.z;
  const float rx = -l.x + 2.0f * nl * n.x, ry = -l.y + 2.0f * nl * n.y, rz = -l.z + 2.0f * nl * n.z;
  float sp = l.x * rx + l.y * ry + l.z * rz;
  sp = (sp > 0.0f && nl > 0.0f) ? sp : 0.0f;
  float s2 = sp * sp, s4 = s2 * s2, s8 = s4 * s4, s16 = s8 * s8, s32 = s16 * s16;
  const float spec = 0.2f * (s32 * s32);
  const float diff = 0.5f + 0.3f * (nl > 0.0f ? nl : 0.0f);
  // distance to the nearest edge of the face, in NDC units
  double d2 = seg_dist2(px, py, T.x[0], T.y[0], T.x[1], T.y[1]);
  d2 = fmin(d2, seg_dist2(px, py, T.x[1], T.y[1], T.x[2], T.y[2]));
  d2 = fmin(d2, seg_dist2(px, py, T.x[2], T.y[2], T.x[0], T.y[0]));
  const float d = (float)sqrt(d2) * ndc_per_px;
  const float prob = 1.0f / (1.0f + expf(-(d * d) / 1e-4f));
  const float zinv = (100.0f - (float)z) / 99.0f;
  const float zmax = zinv > 1e-10f ? zinv : 1e-10f;
  const float w = prob * expf((zinv - zmax) / 1e-4f);
  float delta = expf((1e-10f - zmax) / 1e-4f);
  delta = delta > 1e-10f ? delta : 1e-10f;
  for (int ch = 0; ch < 3; ++ch) {
    const float col = diff * T.c[ch] + spec;
    const float rgb = (w * col + delta) / (w + delta);
    out[ch] = (int)(rgb * 255.0f);
  }
}

__global__ void __launch_bounds__(kThreads) scene_tiles(SceneArgs A) {
  __shared__ int list[kThreads];
  __shared__ int wave_cnt[kThreads / 64];
  int tile = blockIdx.x;
  const int view = tile < A.v[0].tiles ? 0 : 1;
  if (view == 1) tile -= A.v[0].tiles;
  const ViewArgs& V = A.v[view];
  const int tx0 = (tile % V.tiles_x) * kTile, ty0 = (tile / V.tiles_x) * kTile;
  const int x = tx0 + (threadIdx.x % kTile), y = ty0 + (threadIdx.x / kTile);
  const bool live = x < V.W && y < V.H;
  const double px = x + 0.5, py = y + 0.5;
  const float ndc_per_px = 2.0f / (float)(V.H < V.W ? V.H : V.W);

  // 1. z-buffer over the triangles
  double best_z = INFINITY, bb0 = 0, bb1 = 0, bb2 = 0;
  int best_key = 0x7fffffff, best_i = -1;
  const bool raster = V.front ? (A.render_front && !A.early_return) : true;
  if (raster) {
    for (int base = 0; base < V.ntri; base += kThreads) {
      const int i = base + threadIdx.x;
      bool f = false;
      if (i < V.ntri) { const DTri& T = V.tri[i]; f = overlaps(T.bx0, T.by0, T.bx1, T.by1, tx0, ty0); }
      const int cnt = cull(f, i, list, wave_cnt);
      for (int k = 0; k < cnt && live; ++k) {
        const DTri& T = V.tri[list[k]];
        if (x < T.bx0 || x > T.bx1 || y < T.by0 || y > T.by1) continue;
        const double e0 = (T.x[2] - T.x[1]) * (py - T.y[1]) - (T.y[2] - T.y[1]) * (px - T.x[1]);
        const double e1 = (T.x[0] - T.x[2]) * (py - T.y[2]) - (T.y[0] - T.y[2]) * (px - T.x[2]);
        const double e2 = (T.x[1] - T.x[0]) * (py - T.y[0]) - (T.y[1] - T.y[0]) * (px - T.x[0]);
        if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) continue;
        const double area = (T.x[1] - T.x[0]) * (T.y[2] - T.y[0]) - (T.y[1] - T.y[0]) * (T.x[2] - T.x[0]);
        const double b0 = e0 / area, b1 = e1 / area, b2 = e2 / area;
        const double z = b0 * T.z[0] + b1 * T.z[1] + b2 * T.z[2];
        if (z < best_z || (z == best_z && T.key < best_key)) { best_z = z; best_key = T.key; best_i = list[k]; bb0 = b0; bb1 = b1; bb2 = b2; }
      }
      __syncthreads();
    }
  }
  // 2. grid coverage (novel view)
  bool on_grid = false;
  if (!V.front && !A.early_return) {
    for (int base = 0; base < V.ngrid; base += kThreads) {
      const int i = base + threadIdx.x;
      bool f = false;
      if (i < V.ngrid) { const DItem& G = V.grid[i]; f = overlaps(G.bx0, G.by0, G.bx1, G.by1, tx0, ty0); }
      const int cnt = cull(f, i, list, wave_cnt);
      for (int k = 0; k < cnt && live && !on_grid; ++k) {
        const DItem& G = V.grid[list[k]];
        on_grid = seg_dist2((double)x, (double)y, G.a[0], G.a[1], G.a[2], G.a[3]) <= G.r2;
      }
      __syncthreads();
    }
  }
  // 3. base colour
  int c[3] = {0, 0, 0}, orig[3] = {0, 0, 0};
  if (live && V.front) {
    const uint8_t* ip = A.image + (int64_t)y * A.image_pitch + 3 * x;
    orig[0] = ip[0]; orig[1] = ip[1]; orig[2] = ip[2];
    c[0] = orig[0]; c[1] = orig[1]; c[2] = orig[2];
  }
  if (live && best_i >= 0) {
    int r[3];
    shade(V.tri[best_i], px, py, bb0, bb1, bb2, best_z, ndc_per_px, r);
    for (int ch = 0; ch < 3; ++ch)
      c[ch] = V.front ? (int)((double)r[ch] * A.bw + (double)c[ch] * A.one_minus_bw) : r[ch];
  } else if (live && !V.front) {
    c[0] = c[1] = c[2] = A.early_return ? 255 : (on_grid ? 175 : 225);
    if (A.zbuf) {                        // pass B of the point cloud: the nearest point's image colour, tinted by its box
      const unsigned long long key = A.zbuf[(int64_t)y * V.W + x];
      if (key != ~0ull) {
        const unsigned int src = (unsigned int)key;
        const int si = (int)(src / (unsigned int)A.img_w), sj = (int)(src % (unsigned int)A.img_w);
        const uint8_t* ip = A.image + (int64_t)si * A.image_pitch + 3 * sj;
        int b = -1;
        if (A.labels) b = *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(A.labels) + (int64_t)si * A.labels_pitch + 4 * (int64_t)sj);
        const bool tinted = b >= 0 && b < A.n_boxes;
        for (int ch = 0; ch < 3; ++ch) c[ch] = tinted ? ((int)ip[ch] + (int)A.tint[4 * b + ch] + 1) >> 1 : (int)ip[ch];
      }
    }
  }
  // 4. edges and labels in draw order
  if (!A.early_return) {
    for (int base = 0; base < V.nitem; base += kThreads) {
      const int i = base + threadIdx.x;
      bool f = false;
      if (i < V.nitem) { const DItem& I = V.item[i]; f = overlaps(I.bx0, I.by0, I.bx1, I.by1, tx0, ty0); }
      const int cnt = cull(f, i, list, wave_cnt);
      for (int k = 0; k < cnt && live; ++k) {
        const DItem& I = V.item[list[k]];
        if (I.kind == 0) {
          if (seg_dist2((double)x, (double)y, I.a[0], I.a[1], I.a[2], I.a[3]) <= I.r2) {
            c[0] = I.col & 255; c[1] = (I.col >> 8) & 255; c[2] = (I.col >> 16) & 255;
          }
        } else {
          if (x >= I.rx0 && x < I.rx1 && y >= I.ry0 && y < I.ry1)
            for (int ch = 0; ch < 3; ++ch) c[ch] = (int)((double)c[ch] * 0.33 + I.a[ch] * (1.0 - 0.33));
          const int gx = x - I.gx, gy = y - I.gy;
          if (gx >= 0 && gx < I.gw && gy >= 0 && gy < I.gh && A.glyphs[I.goff + (int64_t)gy * I.gw + gx])
            c[0] = c[1] = c[2] = I.col;
        }
      }
      __syncthreads();
    }
  }
  if (!live) return;
  // 5. overlay with the input image (front view), rounded half to even as cv2's saturate_cast
  if (V.front && A.overlay && !A.early_return)
    for (int ch = 0; ch < 3; ++ch) {
      const double v = rint((double)c[ch] * A.bwo + (double)orig[ch] * A.one_minus_bwo);
      c[ch] = v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v);
    }
  uint8_t* op = V.out + (int64_t)y * V.out_pitch + 3 * x;
  op[0] = (uint8_t)c[0]; op[1] = (uint8_t)c[1]; op[2] = (uint8_t)c[2];
}

// -------------------------------------------------------------------------------------------------------------------- host

// np.arange(start, stop) for floats: n = ceil(stop - start), values start + i * ((start + 1) - start)
inline int64_t arange_len(double a, double b) {
  const double n = std::ceil(b - a);
  return n > 0 ? (int64_t)n : 0;
}

void box_view(const double* K, int H, int W, const double (*v)[3], double zplane, int lw, int lh, OvmSceneBox* o) {
  const double eps = 1e-4;
  for (int k = 0; k < 8; ++k)
    for (int d = 0; d < 3; ++d) o->verts[k][d] = v[k][d];
  for (int e = 0; e < 12; ++e) {
    double v0[3], v1[3];
    for (int d = 0; d < 3; ++d) { v0[d] = v[kEdge[e][0]][d]; v1[d] = v[kEdge[e][1]][d]; }
    const double z0 = v0[2], z1 = v1[2];
    o->edge_drawn[e] = (z0 >= zplane || z1 >= zplane) ? 1 : 0;
    if (!o->edge_drawn[e]) { for (int d = 0; d < 4; ++d) o->edge[e][d] = 0; continue; }
    const double den = (z1 - z0) > eps ? (z1 - z0) : eps;
    const double s = (zplane - z0) / den;
    double nv[3];
    for (int d = 0; d < 3; ++d) nv[d] = v0[d] + s * (v1[d] - v0[d]);
    if (z0 < zplane && z1 >= zplane) std::memcpy(v0, nv, sizeof nv);
    else if (z0 >= zplane && z1 < zplane) std::memcpy(v1, nv, sizeof nv);
    double u0[2], u1[2];
    project(K, v0, v0[2] > eps ? v0[2] : eps, u0);
    project(K, v1, v1[2] > eps ? v1[2] : eps, u1);
    o->edge[e][0] = to_i64(u0[0]); o->edge[e][1] = to_i64(u0[1]);
    o->edge[e][2] = to_i64(u1[0]); o->edge[e][3] = to_i64(u1[1]);
  }
  // label anchor: min of the unclipped projections (:728-733), then draw_text's rectangle and text origin
  double x1 = INFINITY, y1 = INFINITY;
  for (int k = 0; k < 8; ++k) {
    double u[2];
    project(K, v[k], v[k][2], u);
    if (std::isnan(u[0]) || std::isnan(u[1])) { x1 = y1 = 0.0; break; }   // 0/0: corner at the camera centre
    x1 = std::fmin(x1, u[0]); y1 = std::fmin(y1, u[1]);
  }
  const int64_t p0 = (int64_t)std::trunc(clampd(x1, -1e12, 1e12)), p1 = (int64_t)std::trunc(clampd(y1, -1e12, 1e12));
  auto clip = [](int64_t a, int64_t hi) { return a < 0 ? (int64_t)0 : (a > hi ? hi : a); };
  o->label_w = lw; o->label_h = lh;
  if (lw > 0 && lh > 0) {
    const int64_t xs = clip(p0, W), xe = clip(xs + lw - 1 + 4, W), ys = clip(p1 - lh - 2, H), ye = clip(p1 + 1 - 2, H);
    o->rect[0] = (int32_t)xs; o->rect[1] = (int32_t)ys;
    o->rect[2] = (int32_t)std::min<int64_t>(xe + 1, W); o->rect[3] = (int32_t)std::min<int64_t>(ye + 1, H);
    o->text_org[0] = (int32_t)clip(p0 + 2, W); o->text_org[1] = (int32_t)clip(p1 - 2, H);
  } else {
    for (int d = 0; d < 4; ++d) o->rect[d] = 0;
    o->text_org[0] = o->text_org[1] = 0;
  }
}

void depth_order(const OvmSceneView& V, int n, int32_t* order) {
  std::vector<std::pair<double, int>> m((size_t)n);
  for (int b = 0; b < n; ++b) {
    double s = 0.0;
    for (int k = 0; k < 8; ++k) s += V.box[b].verts[k][1];
    m[b] = {s / 8.0, b};
  }
  std::stable_sort(m.begin(), m.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
  for (int i = 0; i < n; ++i) order[i] = m[n - 1 - i].second;
}

bool finite_all(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// grid point (x, max_y, z) in the novel camera: rotated, shifted by bias * zoom, z clipped at 0.25; projected to (u, v)
struct GridCam {
  const double* R; const double* c; const double* K; double shift;
  void operator()(double x, double y, double z, double* r, double* u) const {
    const double p[3] = {x, y, z};
    rotate(R, c, p, r);
    r[2] = r[2] + shift;
    if (r[2] < 0.25) r[2] = 0.25;
    project(K, r, r[2], u);
  }
};

// -------------------------------------------------------------------------------------------------------------------- packing

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Packing {
  size_t boxes, kv, items[2], grid, glyphs, tint, staged, tris[2], zbuf, total;
  int nitem_cap[2];
};

Packing plan(const OvmSceneLayout* L, int64_t glyph_bytes, bool points = false) {
  Packing p{};
  const int n = L->n_boxes;
  size_t o = 0;
  p.boxes = o; o = align256(o + sizeof(DBox) * 2 * (size_t)n);
  p.kv = o; o = align256(o + sizeof(double) * 18);
  for (int v = 0; v < 2; ++v) { p.nitem_cap[v] = 13 * n; p.items[v] = o; o = align256(o + sizeof(DItem) * (size_t)(13 * n)); }
  p.grid = o; o = align256(o + sizeof(DItem) * (size_t)L->n_grid);
  p.glyphs = o; o = align256(o + (size_t)glyph_bytes);
  if (points) { p.tint = o; o = align256(o + 4 * (size_t)n); }
  p.staged = o;
  for (int v = 0; v < 2; ++v) { p.tris[v] = o; o = align256(o + sizeof(DTri) * 24 * (size_t)n); }
  if (points) { p.zbuf = o; o = align256(o + sizeof(unsigned long long) * (size_t)L->view[1].height * (size_t)L->view[1].width); }
  p.total = o;
  return p;
}

// ovm_draw::clip_segment into an edge item: no pixel of the canvas within r of the segment is lost. False when nothing is left.
bool clip_segment(double x0, double y0, double x1, double y1, double r, int W, int H, DItem* it) {
  int32_t bb[4];
  if (!ovm_draw::clip_segment(x0, y0, x1, y1, r, W, H, it->a, bb)) return false;
  it->r2 = r * r;
  it->bx0 = bb[0]; it->by0 = bb[1]; it->bx1 = bb[2]; it->by1 = bb[3];
  it->kind = 0;
  return true;
}

bool layout_ok(const OvmSceneLayout* L) {
  if (!L || L->n_boxes < 0 || L->n_boxes > OVM_SCENE_MAX_BOXES || L->n_grid < 0 || (L->mode & ~3) || !L->mode) return false;
  for (int v = 0; v < 2; ++v) {
    const OvmSceneView& V = L->view[v];
    if (!V.drawn) continue;
    if (V.height <= 0 || V.width <= 0 || V.height > 32768 || V.width > 32768 || V.thickness < 1) return false;
    for (int i = 0; i < L->n_boxes; ++i)
      if (V.order[i] < 0 || V.order[i] >= L->n_boxes || V.box[i].label_w < 0 || V.box[i].label_h < 0) return false;
  }
  return L->view[0].drawn == ((L->mode & OVM_SCENE_FRONT) ? 1 : 0) && L->view[1].drawn == ((L->mode & OVM_SCENE_NOVEL) ? 1 : 0);
}

int64_t glyph_total(const OvmSceneLayout* L) {
  int64_t s = 0;
  for (int v = 0; v < 2; ++v)
    for (int i = 0; i < L->n_boxes; ++i) s += (int64_t)L->view[v].box[i].label_w * L->view[v].box[i].label_h;
  return s;
}

std::mutex g_stage_mu;
uint8_t* g_stage = nullptr;      // pinned upload buffer, reused once the previous upload has left it
size_t g_stage_cap = 0;
hipEvent_t g_stage_ev = nullptr;

}  // namespace

extern "C" {

int ovm_host_scene_layout(const OvmSceneInput* in, OvmSceneLayout* L, OvmSceneSegment* grid, int32_t grid_capacity) {
  if (!in || !L || grid_capacity < 0 || (grid_capacity > 0 && !grid)) return OVM_ERR_INVALID;
  const int n = in->n_boxes;
  if (n < 0 || n > OVM_SCENE_MAX_BOXES || (n > 0 && (!in->corners || !in->colors)) || (in->has_labels && n > 0 && !in->label_size))
    return OVM_ERR_INVALID;
  if ((in->mode & ~3) || !in->mode || in->height <= 0 || in->width <= 0 || in->height > 32768 || in->width > 32768) return OVM_ERR_INVALID;
  if ((in->mode & OVM_SCENE_NOVEL) && (in->scale <= 0 || in->scale > 32768)) return OVM_ERR_INVALID;
  if (!finite_all(in->K, 9) || !finite_all(in->R, 9) || !finite_all(in->T, 3) || !finite_all(in->ground_bounds, 5) ||
      !std::isfinite(in->blend_weight) || !std::isfinite(in->blend_weight_overlay) || !std::isfinite(in->zplane) ||
      (n > 0 && !finite_all(in->corners, n * 24)))
    return OVM_ERR_INVALID;
  for (int i = 0; i < 3 * n; ++i)
    if (!(in->colors[i] >= 0.0f && in->colors[i] <= 1.0f)) return OVM_ERR_INVALID;
  if (in->has_labels)
    for (int i = 0; i < 4 * n; ++i)
      if (in->label_size[i] < 0 || in->label_size[i] > 4096) return OVM_ERR_INVALID;

  std::memset(L, 0, sizeof(*L));
  L->n_boxes = n; L->mode = in->mode;
  L->blend_weight = in->blend_weight; L->blend_weight_overlay = in->blend_weight_overlay; L->zplane = in->zplane;
  const double (*C)[8][3] = reinterpret_cast<const double (*)[8][3]>(in->corners);
  for (int b = 0; b < n; ++b) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) {
      L->color[b][k] = in->colors[3 * b + k];
      const double e = (double)in->colors[3 * b + k] * 255 * 1.25;
      L->edge_color[b][k] = e < 255.0 ? e : 255.0;
      L->edge_u8[b][k] = (uint8_t)iround(L->edge_color[b][k]);
    }
    s = (L->edge_color[b][0] + L->edge_color[b][1]) + L->edge_color[b][2];
    L->edge_u8[b][3] = s / 3 > 127.5 ? 0 : 255;
  }
  auto lsize = [&](int view, int b, int k) { return in->has_labels ? in->label_size[(view * n + b) * 2 + k] : 0; };

  // front view
  const int H = in->height, W = in->width;
  if (in->mode & OVM_SCENE_FRONT) {
    OvmSceneView& V = L->view[0];
    V.drawn = 1; V.height = H; V.width = W; V.thickness = std::max(2, iround(3.0 * H / 1250));
    std::memcpy(V.K, in->K, sizeof V.K);
    for (int b = 0; b < n; ++b) box_view(V.K, H, W, C[b], in->zplane, lsize(0, b, 0), lsize(0, b, 1), &V.box[b]);
    depth_order(V, n, V.order);
  }
  L->n_grid = 0;
  if (!(in->mode & OVM_SCENE_NOVEL)) return OVM_OK;

  // novel view: center, rotation, zoom (:430-484)
  const int S = in->scale;
  const double* R = in->R;
  double center[3], mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = 0; b < n; ++b)
    for (int k = 0; k < 8; ++k)
      for (int d = 0; d < 3; ++d) { mn[d] = std::fmin(mn[d], C[b][k][d]); mx[d] = std::fmax(mx[d], C[b][k][d]); }
  if (in->has_T) std::memcpy(center, in->T, sizeof center);
  else for (int d = 0; d < 3; ++d) center[d] = n > 0 ? (mn[d] + mx[d]) / 2 : 0.0;
  std::memcpy(L->center, center, sizeof center);
  double Kn[9];
  std::memcpy(Kn, in->K, sizeof Kn);
  Kn[2] *= (double)S / W;
  Kn[5] *= (double)S / H;
  std::vector<double> rot((size_t)n * 24);
  for (int b = 0; b < n; ++b)
    for (int k = 0; k < 8; ++k) rotate(R, center, C[b][k], &rot[(b * 8 + k) * 3]);
  const double margin = 0.01;
  double zoom = 1.0, bias = 1.0;
  if (!in->has_T) {
    int trials = 10000;
    zoom = 100.0;
    double zin = zoom;
    while (trials) {
      zin = zin * 0.95;
      bool stop = false;
      for (int i = 0; i < 8 * n && !stop; ++i) if (rot[3 * i + 2] + center[2] * zin < 0.25) stop = true;
      for (int i = 0; i < 8 * n && !stop; ++i) {
        const double v[3] = {rot[3 * i], rot[3 * i + 1], rot[3 * i + 2] + center[2] * zin};
        double u[2];
        project(Kn, v, v[2], u);
        if (u[0] < S * margin || u[1] < S * margin || u[0] > S * (1 - margin) || u[1] > S * (1 - margin)) stop = true;
      }
      if (stop) break;
      zoom = zin;
      trials -= 1;
    }
    bias = center[2];
  }
  L->zoom_factor = zoom; L->zoom_bias = bias;
  const double shift = bias * zoom;
  {
    OvmSceneView& V = L->view[1];
    V.drawn = 1; V.height = S; V.width = S; V.thickness = std::max(2, iround(3.0 * S / 1250));
    std::memcpy(V.K, Kn, sizeof Kn);
    double nv[8][3];
    for (int b = 0; b < n; ++b) {
      for (int k = 0; k < 8; ++k) {
        nv[k][0] = rot[(b * 8 + k) * 3]; nv[k][1] = rot[(b * 8 + k) * 3 + 1]; nv[k][2] = rot[(b * 8 + k) * 3 + 2] + shift;
      }
      box_view(Kn, S, S, nv, in->zplane, lsize(1, b, 0), lsize(1, b, 1), &V.box[b]);
    }
    depth_order(V, n, V.order);
  }
  L->grid_thickness = std::max(1, iround(3.0 * S / 1250));

  // ground bounds (:488-533)
  const GridCam cam{R, center, Kn, shift};
  double gb[5];
  if (in->has_ground_bounds) {
    std::memcpy(gb, in->ground_bounds, sizeof gb);
  } else {
    if (n == 0) { L->early_return = 1; return OVM_OK; }
    const double max_y = mx[1];
    const double xs = std::nearbyint(mn[0] - (mx[0] - mn[0]) * 50), xe = std::nearbyint(mx[0] + (mx[0] - mn[0]) * 50);
    const double zs = std::nearbyint(mn[2] - (mx[2] - mn[2]) * 50), ze = std::nearbyint(mx[2] + (mx[2] - mn[2]) * 50);
    const int64_t nx = arange_len(xs, xe), nz = arange_len(zs, ze);
    if (nx * nz > ((int64_t)1 << 31)) return OVM_ERR_INVALID;   // boxes thousands of metres apart: not a scene
    const double dxs = (xs + 1.0) - xs, dzs = (zs + 1.0) - zs;
    double rx_min = INFINITY, rx_max = -INFINITY, oz_min = INFINITY, oz_max = -INFINITY;
    bool anyx = false, anyz = false;
    for (int64_t iz = 0; iz < nz; ++iz) {
      const double z = zs + iz * dzs;
      for (int64_t ix = 0; ix < nx; ++ix) {
        const double x = xs + ix * dxs;
        double r[3], u[2];
        cam(x, max_y, z, r, u);
        if (u[0] >= -50 && u[0] < S + 50 && r[2] > 0) { anyx = true; rx_min = std::fmin(rx_min, r[0]); rx_max = std::fmax(rx_max, r[0]); }
        if (u[1] >= -50 && u[1] < S + 50 && r[2] > 0) { anyz = true; oz_min = std::fmin(oz_min, z); oz_max = std::fmax(oz_max, z); }
      }
    }
    if (!anyz || !anyx) { L->early_return = 1; return OVM_OK; }
    gb[0] = max_y;
    gb[1] = std::nearbyint(rx_min - 10); gb[2] = std::nearbyint(rx_max + 10);
    gb[3] = std::nearbyint(oz_min - 10); gb[4] = std::nearbyint(oz_max + 10);
  }
  std::memcpy(L->ground, gb, sizeof gb);

  // grid segments (:536-579): horizontal (r-1, c-1)-(r-1, c) and vertical (r-1, c-1)-(r, c-1) for r, c >= 1
  const int64_t nx = arange_len(gb[1], gb[2]), nz = arange_len(gb[3], gb[4]);
  if (nx * nz > ((int64_t)1 << 26)) return OVM_ERR_INVALID;   // a ground grid of > 67M points is not a scene
  const double dxs = (gb[1] + 1.0) - gb[1], dzs = (gb[3] + 1.0) - gb[3];
  std::vector<int64_t> pts((size_t)(nx * nz) * 2);
  for (int64_t iz = 0; iz < nz; ++iz)
    for (int64_t ix = 0; ix < nx; ++ix) {
      double r[3], u[2];
      cam(gb[1] + ix * dxs, gb[0], gb[3] + iz * dzs, r, u);
      pts[(iz * nx + ix) * 2] = to_i64(u[0]);
      pts[(iz * nx + ix) * 2 + 1] = to_i64(u[1]);
    }
  std::vector<OvmSceneSegment> segs;
  segs.reserve((size_t)std::max<int64_t>(0, 2 * (nx - 1) * (nz - 1)));
  auto P = [&](int64_t iz, int64_t ix) { return &pts[(iz * nx + ix) * 2]; };
  for (int64_t r = 1; r < nz; ++r)
    for (int64_t c = 1; c < nx; ++c) {
      const int64_t* a = P(r - 1, c - 1);
      const int64_t* h = P(r - 1, c);
      const int64_t* v = P(r, c - 1);
      segs.push_back({a[0], a[1], h[0], h[1]});
      segs.push_back({a[0], a[1], v[0], v[1]});
    }
  auto key = [](const OvmSceneSegment& s) { return std::make_tuple(s.x0, s.y0, s.x1, s.y1); };
  std::sort(segs.begin(), segs.end(), [&](const OvmSceneSegment& a, const OvmSceneSegment& b) { return key(a) < key(b); });
  segs.erase(std::unique(segs.begin(), segs.end(), [&](const OvmSceneSegment& a, const OvmSceneSegment& b) { return key(a) == key(b); }),
             segs.end());
  L->n_grid = (int32_t)segs.size();
  if ((int64_t)segs.size() > grid_capacity) return OVM_ERR_CAPACITY;
  if (!segs.empty()) std::memcpy(grid, segs.data(), segs.size() * sizeof(OvmSceneSegment));
  return OVM_OK;
}

int ovm_render_scene_workspace(const OvmSceneLayout* layout, int64_t glyph_bytes, int64_t* bytes) {
  if (!layout_ok(layout) || glyph_bytes < 0 || !bytes) return OVM_ERR_INVALID;
  *bytes = (int64_t)plan(layout, glyph_bytes).total;
  return OVM_OK;
}

}  // extern "C"

namespace {

struct Points {          // the extra arguments of ovm_render_scene_points
  const float* depth;
  int64_t depth_pitch;
  const int32_t* labels;
  int64_t labels_pitch;
  const double* R;
  int32_t point_size;
  uint64_t* zbuf_out;
};

// ovm_render_scene (pts null) and ovm_render_scene_points: every refusal comes before any device work.
int render(const OvmSceneLayout* L, const OvmSceneSegment* grid, const uint8_t* glyphs, int64_t glyph_bytes, const uint8_t* image,
           int64_t image_pitch, uint8_t* front, int64_t front_pitch, uint8_t* novel, int64_t novel_pitch, const Points* pts,
           void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  if (!layout_ok(L) || glyph_bytes < 0 || glyph_bytes != glyph_total(L) || (glyph_bytes > 0 && !glyphs) ||
      (L->n_grid > 0 && !grid) || !workspace)
    return OVM_ERR_INVALID;
  const OvmSceneView& F = L->view[0];
  const OvmSceneView& N = L->view[1];
  if (F.drawn && (!image || !front || image_pitch < 3 * (int64_t)F.width || front_pitch < 3 * (int64_t)F.width)) return OVM_ERR_INVALID;
  if (N.drawn && (!novel || novel_pitch < 3 * (int64_t)N.width)) return OVM_ERR_INVALID;
  if (pts) {
    if (!F.drawn || !N.drawn || !pts->depth || !pts->R || !finite_all(pts->R, 9)) return OVM_ERR_INVALID;
    if (pts->depth_pitch < 4 * (int64_t)F.width || (pts->depth_pitch & 3)) return OVM_ERR_INVALID;
    if (pts->labels && (pts->labels_pitch < 4 * (int64_t)F.width || (pts->labels_pitch & 3))) return OVM_ERR_INVALID;
    if (pts->point_size < 1 || pts->point_size > 9 || !(pts->point_size & 1)) return OVM_ERR_INVALID;
  }
  const Packing pk = plan(L, glyph_bytes, pts != nullptr);
  if (workspace_bytes < (int64_t)pk.total) return OVM_ERR_CAPACITY;
  const int n = L->n_boxes;

  std::lock_guard<std::mutex> lock(g_stage_mu);
  if (g_stage_ev) {
    if (hipEventSynchronize(g_stage_ev) != hipSuccess) return OVM_ERR_HIP;
  } else if (hipEventCreateWithFlags(&g_stage_ev, hipEventDisableTiming) != hipSuccess) {
    return OVM_ERR_HIP;
  }
  if (g_stage_cap < pk.staged) {
    if (g_stage) (void)hipHostFree(g_stage);
    g_stage = nullptr; g_stage_cap = 0;
    if (hipHostMalloc((void**)&g_stage, pk.staged, hipHostMallocPortable) != hipSuccess) { g_stage = nullptr; return OVM_ERR_HIP; }
    g_stage_cap = pk.staged;
  }
  uint8_t* st = g_stage;
  std::memset(st, 0, pk.staged);
  DBox* boxes = reinterpret_cast<DBox*>(st + pk.boxes);
  for (int v = 0; v < 2; ++v)
    for (int b = 0; b < n; ++b) {
      std::memcpy(boxes[v * n + b].v, L->view[v].box[b].verts, sizeof(double) * 24);
      for (int k = 0; k < 3; ++k) boxes[v * n + b].c[k] = L->color[b][k];
    }
  std::memcpy(st + pk.kv, F.K, sizeof(double) * 9);
  std::memcpy(st + pk.kv + sizeof(double) * 9, N.K, sizeof(double) * 9);
  int nitem[2] = {0, 0};
  int64_t goff = 0;
  for (int v = 0; v < 2; ++v) {
    const OvmSceneView& V = L->view[v];
    DItem* items = reinterpret_cast<DItem*>(st + pk.items[v]);
    if (V.drawn) {
      const double r = V.thickness / 2.0;
      for (int i = 0; i < n; ++i) {
        const int b = V.order[i];
        const OvmSceneBox& B = V.box[b];
        const int col = L->edge_u8[b][0] | (L->edge_u8[b][1] << 8) | (L->edge_u8[b][2] << 16);
        for (int e = 0; e < 12; ++e) {
          if (!B.edge_drawn[e]) continue;
          DItem it{};
          if (!clip_segment((double)B.edge[e][0], (double)B.edge[e][1], (double)B.edge[e][2], (double)B.edge[e][3], r, V.width, V.height, &it))
            continue;
          it.col = col;
          items[nitem[v]++] = it;
        }
        if (B.label_w > 0 && B.label_h > 0) {
          DItem it{};
          it.kind = 1;
          for (int k = 0; k < 3; ++k) it.a[k] = L->edge_color[b][k];
          it.col = L->edge_u8[b][3];
          it.rx0 = B.rect[0]; it.ry0 = B.rect[1]; it.rx1 = B.rect[2]; it.ry1 = B.rect[3];
          it.gx = B.text_org[0]; it.gy = B.text_org[1] - B.label_h; it.gw = B.label_w; it.gh = B.label_h;
          int64_t o = goff;
          for (int bb = 0; bb < b; ++bb) o += (int64_t)V.box[bb].label_w * V.box[bb].label_h;
          it.goff = o;
          int x0 = std::min(it.rx0, it.gx), y0 = std::min(it.ry0, it.gy);
          int x1 = std::max(it.rx1, it.gx + it.gw) - 1, y1 = std::max(it.ry1, it.gy + it.gh) - 1;
          it.bx0 = std::max(x0, 0); it.by0 = std::max(y0, 0); it.bx1 = std::min(x1, V.width - 1); it.by1 = std::min(y1, V.height - 1);
          items[nitem[v]++] = it;
        }
      }
    }
    for (int b = 0; b < n; ++b) goff += (int64_t)V.box[b].label_w * V.box[b].label_h;
  }
  int ngrid = 0;
  if (N.drawn && !L->early_return) {
    DItem* g = reinterpret_cast<DItem*>(st + pk.grid);
    const double r = L->grid_thickness / 2.0;
    for (int i = 0; i < L->n_grid; ++i) {
      DItem it{};
      if (!clip_segment((double)grid[i].x0, (double)grid[i].y0, (double)grid[i].x1, (double)grid[i].y1, r, N.width, N.height, &it)) continue;
      it.col = 175 | (175 << 8) | (175 << 16);
      g[ngrid++] = it;
    }
  }
  if (glyph_bytes > 0) std::memcpy(st + pk.glyphs, glyphs, (size_t)glyph_bytes);
  if (pts)
    for (int b = 0; b < n; ++b) std::memcpy(st + pk.tint + 4 * (size_t)b, L->edge_u8[b], 4);

  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  if (hipMemcpyAsync(ws, st, pk.staged, hipMemcpyHostToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  if (hipEventRecord(g_stage_ev, s) != hipSuccess) return OVM_ERR_HIP;

  SceneArgs A{};
  uint8_t* outs[2] = {front, novel};
  const int64_t pitches[2] = {front_pitch, novel_pitch};
  for (int v = 0; v < 2; ++v) {
    ViewArgs& va = A.v[v];
    const OvmSceneView& V = L->view[v];
    va.front = v == 0;
    if (!V.drawn) continue;
    va.H = V.height; va.W = V.width;
    va.tiles_x = (V.width + kTile - 1) / kTile;
    va.tiles = va.tiles_x * ((V.height + kTile - 1) / kTile);
    va.ntri = 24 * n;
    va.nitem = nitem[v];
    va.ngrid = v == 1 ? ngrid : 0;
    va.tri = reinterpret_cast<const DTri*>(ws + pk.tris[v]);
    va.item = reinterpret_cast<const DItem*>(ws + pk.items[v]);
    va.grid = reinterpret_cast<const DItem*>(ws + pk.grid);
    va.out = outs[v];
    va.out_pitch = pitches[v];
  }
  A.image = image; A.image_pitch = image_pitch;
  A.glyphs = ws + pk.glyphs;
  A.early_return = L->early_return;
  A.render_front = L->blend_weight > 0;
  A.bw = L->blend_weight; A.one_minus_bw = 1 - L->blend_weight;
  A.bwo = L->blend_weight_overlay; A.one_minus_bwo = 1 - L->blend_weight_overlay;
  A.overlay = L->blend_weight_overlay < 1.0 && L->blend_weight_overlay > 0.0;
  const int mask = (F.drawn ? 1 : 0) | (N.drawn ? 2 : 0);
  if (n > 0) {
    const int threads = 2 * n * 12;
    scene_setup<<<(threads + 63) / 64, 64, 0, s>>>(reinterpret_cast<const DBox*>(ws + pk.boxes), n, L->zplane, A.v[0], A.v[1],
                                                   reinterpret_cast<const double*>(ws + pk.kv), reinterpret_cast<DTri*>(ws + pk.tris[0]),
                                                   reinterpret_cast<DTri*>(ws + pk.tris[1]), mask);
  }
  if (pts) {
    unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(ws + pk.zbuf);
    const size_t zbytes = sizeof(unsigned long long) * (size_t)N.height * (size_t)N.width;
    if (hipMemsetAsync(zbuf, 0xff, zbytes, s) != hipSuccess) return OVM_ERR_HIP;
    if (!L->early_return) {              // an empty grid draws the bare render: nothing is splatted
      SplatArgs P{};
      P.depth = pts->depth; P.depth_pitch = pts->depth_pitch; P.zbuf = zbuf;
      P.H = F.height; P.W = F.width; P.S = N.width; P.half = (pts->point_size - 1) / 2;
      P.fx = F.K[0]; P.cx = F.K[2]; P.fy = F.K[4]; P.cy = F.K[5];
      std::memcpy(P.R, pts->R, sizeof P.R);
      std::memcpy(P.c, L->center, sizeof P.c);
      P.shift = L->zoom_bias * L->zoom_factor;
      P.zplane = L->zplane;
      std::memcpy(P.Kn, N.K, sizeof P.Kn);
      scene_splat<<<dim3((unsigned)((F.width + kThreads - 1) / kThreads), (unsigned)F.height), kThreads, 0, s>>>(P);
      A.zbuf = zbuf; A.labels = pts->labels; A.labels_pitch = pts->labels_pitch;
      A.tint = ws + pk.tint; A.img_w = F.width; A.n_boxes = n;
    }
    if (pts->zbuf_out && hipMemcpyAsync(pts->zbuf_out, zbuf, zbytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  }
  const int tiles = A.v[0].tiles + A.v[1].tiles;
  if (tiles > 0) scene_tiles<<<tiles, kThreads, 0, s>>>(A);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // namespace

extern "C" {

int ovm_render_scene(const OvmSceneLayout* L, const OvmSceneSegment* grid, const uint8_t* glyphs, int64_t glyph_bytes,
                     const uint8_t* image, int64_t image_pitch, uint8_t* front, int64_t front_pitch, uint8_t* novel, int64_t novel_pitch,
                     void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  return render(L, grid, glyphs, glyph_bytes, image, image_pitch, front, front_pitch, novel, novel_pitch, nullptr, workspace,
                workspace_bytes, stream);
}

int ovm_render_scene_points_workspace(const OvmSceneLayout* layout, int64_t glyph_bytes, int64_t* bytes) {
  if (!layout_ok(layout) || glyph_bytes < 0 || !bytes || !layout->view[0].drawn || !layout->view[1].drawn) return OVM_ERR_INVALID;
  *bytes = (int64_t)plan(layout, glyph_bytes, true).total;
  return OVM_OK;
}

int ovm_render_scene_points(const OvmSceneLayout* L, const OvmSceneSegment* grid, const uint8_t* glyphs, int64_t glyph_bytes,
                            const uint8_t* image, int64_t image_pitch, uint8_t* front, int64_t front_pitch, uint8_t* novel,
                            int64_t novel_pitch, const float* depth, int64_t depth_pitch, const int32_t* labels, int64_t labels_pitch,
                            const double* R, int32_t point_size, uint64_t* zbuf_out, void* workspace, int64_t workspace_bytes,
                            ovm_stream_t stream) {
  const Points pts{depth, depth_pitch, labels, labels_pitch, R, point_size, zbuf_out};
  return render(L, grid, glyphs, glyph_bytes, image, image_pitch, front, front_pitch, novel, novel_pitch, &pts, workspace,
                workspace_bytes, stream);
}

}  // extern "C"
