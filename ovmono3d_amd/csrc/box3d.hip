// Exact intersection volume / IoU of oriented 3D boxes given by their 8 corners (pytorch3d corner order). Replaces
// pytorch3d's `_C.iou_box3d` behind the reference's `box3d_overlap` (cubercnn/evaluation/omni3d_evaluation.py:109-169),
// including its validity screening of the detections (`_check_coplanar` :68-87, `_check_nonzero` :90-107).
//
// Two entry points, one per-pair routine (pair_iou):
//   ovm_box3d_iou   the N x M matrix of N detections and M ground-truth boxes, fp32, one thread per pair;
//   ovm_eval_iou3d  the [n_dt][n_gt] block of every (image, category) cell of the evaluator, fp64, written straight into the
//                   CSR IoU buffer ovm_eval_match reads; one wave per detection row, one lane per ground-truth box of its cell.
//
// Method: the intersection of two convex boxes is a convex polyhedron whose faces lie on faces of A or of B. By the
// divergence theorem  V = 1/3 * sum_f (p_f . n_f) * area(f),  so
//     V = 1/3 * sum_{faces f of A} (p_f . n_f) * area(f clipped to B)  +  1/3 * sum_{faces g of B} (p_g . n_g) * area(g clipped to A)
// with outward unit normals n and any point p on the face. Each quad face is clipped against the other box's six
// half-spaces (Sutherland-Hodgman, at most 10 vertices). A's faces are clipped against B's CLOSED half-spaces and B's faces
// against A's OPEN ones, so a coincident face pair is counted once (IoU of a box with itself is exactly 1). A face of A
// lying in a plane of B whose outward normal points the other way (two boxes touching face to face) bounds no volume
// of the intersection, so that plane is open for A's faces too.
//
// The pair is handled in a frame centred on the detection's corner centroid. In camera coordinates every face term
// p_f . n_f is about distance x area and the terms cancel down to the volume, which loses most of the fp32 precision of
// a small box far from the camera; in the local frame they are of the box's own size, and so is the snapping tolerance.
// A box without volume (a flat box, a segment, a point: ground truth the evaluator keeps as ignored) intersects
// nothing: such a pair gets volume 0 and IoU 0. The intersection is clamped to the smaller volume, so IoU <= 1.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "common.hpp"
#include "../../include/ovm3d.h"

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }

// pytorch3d `_box_planes`: corner indices of the six quad faces, each in cyclic order
__constant__ int kFace[6][4] = {{0, 1, 2, 3}, {3, 2, 6, 7}, {0, 1, 5, 4}, {0, 3, 7, 4}, {1, 2, 6, 5}, {4, 5, 6, 7}};
// pytorch3d `_box_triangles`
__constant__ int kTri[12][3] = {{0, 1, 2}, {0, 3, 2}, {4, 5, 6}, {4, 6, 7}, {1, 5, 6}, {1, 6, 2}, {0, 4, 7}, {0, 7, 3}, {3, 2, 6}, {3, 6, 7}, {0, 1, 5}, {0, 4, 5}};

struct Box {
  V3 c[8];
  V3 n[6];        // outward unit normals
  float d[6];     // plane offsets: inside <=> n . x <= d
  float vol;
  float scale;    // largest |coordinate|: sets the snapping tolerance of the plane tests
  bool solid;     // every face has a normal and the volume is positive
};

__device__ void load_box(const float* p, Box& b) {
  V3 ctr = {0.f, 0.f, 0.f};
  b.scale = 0.f;
  for (int i = 0; i < 8; ++i) {
    b.c[i] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; ctr = ctr + b.c[i];
    b.scale = fmaxf(b.scale, fmaxf(fabsf(b.c[i].x), fmaxf(fabsf(b.c[i].y), fabsf(b.c[i].z))));
  }
  ctr = ctr * 0.125f;
  b.solid = true;
  for (int f = 0; f < 6; ++f) {
    const V3 v0 = b.c[kFace[f][0]], v1 = b.c[kFace[f][1]], v2 = b.c[kFace[f][2]], v3 = b.c[kFace[f][3]];
    V3 n = cross(v1 - v0, v3 - v0);
    const float l = norm(n);
    if (!(l > 0.f)) b.solid = false;
    n = l > 0.f ? n * (1.f / l) : V3{0.f, 0.f, 0.f};
    const V3 fc = (v0 + v1 + v2 + v3) * 0.25f;
    if (dot(n, fc - ctr) < 0.f) n = n * -1.f;
    b.n[f] = n; b.d[f] = dot(n, fc);
  }
  // Corners rounded to fp32 far from the camera are off their face planes by up to half an ulp of the distance; clipped
  // as given, faces of A and of B then do not close up into one surface, which costs an IoU error of several times that
  // rounding on a small box. Every corner is therefore moved to where its three face planes meet: the box becomes the
  // intersection of its six half-spaces, as the plane tests already take it.
  if (b.solid) {
    for (int k = 0; k < 8; ++k) {
      const int fx = (k == 0 || k == 3 || k == 4 || k == 7) ? 3 : 4, fy = (k == 0 || k == 1 || k == 4 || k == 5) ? 2 : 1, fz = k < 4 ? 0 : 5;
      const V3 c23 = cross(b.n[fy], b.n[fz]), c31 = cross(b.n[fz], b.n[fx]), c12 = cross(b.n[fx], b.n[fy]);
      const float det = dot(b.n[fx], c23);
      if (fabsf(det) > 1e-3f) b.c[k] = (c23 * b.d[fx] + c31 * b.d[fy] + c12 * b.d[fz]) * (1.f / det);
    }
  }
  // volume of the hexahedron: the same face sum with unclipped faces
  float v = 0.f;
  for (int f = 0; f < 6; ++f) {
    const V3 v0 = b.c[kFace[f][0]], v1 = b.c[kFace[f][1]], v2 = b.c[kFace[f][2]], v3 = b.c[kFace[f][3]];
    const float area = 0.5f * (norm(cross(v1 - v0, v2 - v0)) + norm(cross(v2 - v0, v3 - v0)));
    v += b.d[f] * area;
  }
  b.vol = v * (1.f / 3.f);
  if (!(b.vol > 0.f)) b.solid = false;
}

// area of face `f` of `a` inside box `o`; closed = keep points on those planes of o that face the same way as the face
__device__ float clipped_face_area(const Box& a, int f, const Box& o, bool closed) {
  V3 poly[12], tmp[12];
  int n = 4;
  for (int i = 0; i < 4; ++i) poly[i] = a.c[kFace[f][i]];
  for (int pl = 0; pl < 6 && n > 0; ++pl) {
    const V3 pn = o.n[pl]; const float pd = o.d[pl];
    const bool keep_on = closed && dot(pn, a.n[f]) > 0.f;
    // Signed distances within rounding noise of the plane are snapped to "on the plane" (a few fp32 ulps of the coordinate
    // magnitude in the local frame, i.e. of the boxes' size and separation): a face of `a` lying in a plane of `o` is then
    // inside for the closed test and outside for the open one, whichever way the noise fell.
    const float eps = 4e-6f * (fmaxf(a.scale, o.scale) + fabsf(pd));
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const V3 cur = poly[i], nxt = poly[(i + 1 == n) ? 0 : i + 1];
      float sc = dot(pn, cur) - pd, sn = dot(pn, nxt) - pd;
      if (fabsf(sc) <= eps) sc = 0.f;
      if (fabsf(sn) <= eps) sn = 0.f;
      const bool in_c = keep_on ? (sc <= 0.f) : (sc < 0.f);
      const bool in_n = keep_on ? (sn <= 0.f) : (sn < 0.f);
      if (in_c) tmp[m++] = cur;
      if (in_c != in_n) {
        const float t = sc / (sc - sn);
        tmp[m++] = cur + (nxt - cur) * t;
      }
    }
    n = m < 12 ? m : 12;
    for (int i = 0; i < n; ++i) poly[i] = tmp[i];
  }
  if (n < 3) return 0.f;
  V3 acc = {0.f, 0.f, 0.f};
  for (int i = 1; i + 1 < n; ++i) acc = acc + cross(poly[i] - poly[0], poly[i + 1] - poly[0]);
  return 0.5f * fabsf(dot(acc, a.n[f]));
}

__device__ __forceinline__ V3 corner(const float* p, int k) { return {p[3 * k], p[3 * k + 1], p[3 * k + 2]}; }

// on the detection's corners as given (camera coordinates), as the reference screens them
__device__ bool box_valid(const float* p, float eps_coplanar, float eps_nonzero) {
  // reference _check_coplanar: |(v3 - v0) . normalize(cross(normalize(v1 - v0), normalize(v2 - v0)))| summed over the 6 planes < eps
  float s = 0.f;
  for (int f = 0; f < 6; ++f) {
    const V3 v0 = corner(p, kFace[f][0]), v1 = corner(p, kFace[f][1]), v2 = corner(p, kFace[f][2]), v3 = corner(p, kFace[f][3]);
    V3 e0 = v1 - v0, e1 = v2 - v0;
    const float l0 = fmaxf(norm(e0), 1e-12f), l1 = fmaxf(norm(e1), 1e-12f);
    e0 = e0 * (1.f / l0); e1 = e1 * (1.f / l1);
    V3 nn = cross(e0, e1);
    const float ln = fmaxf(norm(nn), 1e-12f);
    nn = nn * (1.f / ln);
    s += dot(v3 - v0, nn);
  }
  if (!(fabsf(s) < eps_coplanar)) return false;
  // reference _check_nonzero: every triangle area > eps
  for (int t = 0; t < 12; ++t) {
    const V3 v0 = corner(p, kTri[t][0]), v1 = corner(p, kTri[t][1]), v2 = corner(p, kTri[t][2]);
    if (!(0.5f * norm(cross(v1 - v0, v2 - v0)) > eps_nonzero)) return false;
  }
  return true;
}

// IoU (and the clamped intersection volume) of detection corners `pa` and ground-truth corners `pb`, both [8][3] in camera
// coordinates: the local frame, face clipping, clamp and detection screening described above. The one per-pair routine of
// ovm_box3d_iou and ovm_eval_iou3d. Not inlined on purpose: inlined into two kernels the compiler contracts multiply-adds differently
// in each (measured: 1 % of 2.6 M pairs differed in the last bits), and the evaluator's two routes must give the same IoU bit for bit.
__device__ __noinline__ float pair_iou(const float* pa, const float* pb, float eps_coplanar, float eps_nonzero, float& vol) {
  // the local frame: both boxes minus the detection's corner centroid
  V3 o = {0.f, 0.f, 0.f};
  for (int k = 0; k < 8; ++k) o = o + corner(pa, k);
  o = o * 0.125f;
  float la[24], lb[24];
  for (int k = 0; k < 8; ++k) {
    la[3 * k] = pa[3 * k] - o.x; la[3 * k + 1] = pa[3 * k + 1] - o.y; la[3 * k + 2] = pa[3 * k + 2] - o.z;
    lb[3 * k] = pb[3 * k] - o.x; lb[3 * k + 1] = pb[3 * k + 1] - o.y; lb[3 * k + 2] = pb[3 * k + 2] - o.z;
  }
  Box a, b;
  load_box(la, a);
  load_box(lb, b);
  float v = 0.f, r = 0.f;
  if (a.solid && b.solid) {
    for (int f = 0; f < 6; ++f) v += a.d[f] * clipped_face_area(a, f, b, true);
    for (int f = 0; f < 6; ++f) v += b.d[f] * clipped_face_area(b, f, a, false);
    v = fminf(fmaxf(v * (1.f / 3.f), 0.f), fminf(a.vol, b.vol));
    const float u = a.vol + b.vol - v;
    r = (u > 0.f) ? fminf(v / u, 1.f) : 0.f;
  }
  if (!box_valid(pa, eps_coplanar, eps_nonzero)) { r = 0.f; }            // offending detections get IoU 0 (:160-167)
  vol = v;
  return r;
}

__global__ __launch_bounds__(128) void box3d_iou_kernel(const float* __restrict__ dt, const float* __restrict__ gt, int N, int M, float eps_coplanar,
                                                        float eps_nonzero, float* __restrict__ iou, float* __restrict__ vol) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * M) return;
  const int i = (int)(idx / M), j = (int)(idx % M);
  float v;
  const float r = pair_iou(dt + (size_t)i * 24, gt + (size_t)j * 24, eps_coplanar, eps_nonzero, v);
  iou[idx] = r;
  if (vol) vol[idx] = v;
}

// One wave per detection row of the evaluator's CSR layout, lane l on the ground-truth boxes l, l + 64, ... of the row's cell: the
// per-pair work is long and register-heavy, so a thread never owns more than its share of one row.
__global__ __launch_bounds__(64) void eval_iou3d_kernel(const OvmEvalCell* __restrict__ cells, const int32_t* __restrict__ dt_cell, int32_t n_dt_total,
                                                        const float* __restrict__ dt, const float* __restrict__ gt, float eps_coplanar,
                                                        float eps_nonzero, double* __restrict__ iou) {
  const int d = blockIdx.x;
  if (d >= n_dt_total) return;
  const OvmEvalCell c = cells[dt_cell[d]];
  const long row = d - c.dt_off;
  const float* pa = dt + (size_t)d * 24;
  for (int g = threadIdx.x; g < c.n_gt; g += 64) {
    float v;
    const float r = pair_iou(pa, gt + (size_t)(c.gt_off + g) * 24, eps_coplanar, eps_nonzero, v);
    iou[c.iou_off + row * c.n_gt + g] = (r != r) ? 0.0 : (double)r;
  }
}

}  // namespace

extern "C" int ovm_box3d_iou(const float* boxes_dt, const float* boxes_gt, int32_t N, int32_t M, float eps_coplanar, float eps_nonzero, float* iou,
                             float* vol, ovm_stream_t stream) {
  if (N <= 0 || M <= 0) return OVM_OK;
  if (!boxes_dt || !boxes_gt || !iou) return OVM_ERR_INVALID;
  const long n = (long)N * M;
  hipLaunchKernelGGL(box3d_iou_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, (hipStream_t)stream, boxes_dt, boxes_gt, N, M, eps_coplanar,
                     eps_nonzero, iou, vol);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

extern "C" int ovm_eval_iou3d(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, const float* dt_corners, const float* gt_corners,
                              float eps_coplanar, float eps_nonzero, double* iou, ovm_stream_t stream) {
  if (n_dt_total < 0) return OVM_ERR_INVALID;
  if (n_dt_total == 0) return OVM_OK;
  if (!cells || !dt_cell || !dt_corners || !gt_corners || !iou) return OVM_ERR_INVALID;
  hipLaunchKernelGGL(eval_iou3d_kernel, dim3((unsigned)n_dt_total), dim3(64), 0, (hipStream_t)stream, cells, dt_cell, n_dt_total, dt_corners, gt_corners,
                     eps_coplanar, eps_nonzero, iou);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}
