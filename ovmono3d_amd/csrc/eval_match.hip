// COCO-style matching of the Omni3D evaluator on the device: the 2D box IoU of pycocotools (maskUtils.iou, iscrowd 0) and the
// greedy per-threshold matching of COCOeval.evaluateImg, both as Omni3Deval runs them (reference
// cubercnn/evaluation/omni3d_evaluation.py:1467-1545 on pycocotools), plus upstream Omni3D's proximity rules (eval_prox,
// :1472-1485, threshold :1459-1461). The host restatement is Omni3Deval._match / _evaluate_cell in
// ovmono3d_amd/evaluation/omni3d_eval.py; the outputs here equal it exactly.
//
// Mapping of the matcher: one wave64 per (cell, range, IoU threshold). Lane l owns the ground-truth boxes l, l+64, l+128, ...
// of the cell and keeps one bit per owned box for "ignored in this range", "crowd" and "taken" (64 bits: up to 4096 boxes per
// cell). The detections are walked in score order; per detection every lane scans its free boxes for the best IoU >= the floor in
// each of the two groups (not ignored / ignored), a shuffle arg-max across the wave picks the winner (the later index on equal
// IoU), and the owner lane marks it taken. Lane d % 64 keeps detection d's result and the wave writes 64 results at a time.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ovm3d.h"

// The IoU must round exactly as numpy's does: no fused multiply-adds anywhere in this file.
#pragma clang fp contract(off)

namespace {

constexpr int kMaxChunks = 64;   // ground-truth boxes per lane: 64 x 64 = 4096 per cell

// numpy's element-wise semantics (NaN from either side propagates; on equal values the second operand)
__device__ __forceinline__ double np_minimum(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double np_maximum(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double np_clip0(double x) { return (x > 0.0 || x != x) ? x : 0.0; }

__global__ __launch_bounds__(256) void eval_iou2d_kernel(const OvmEvalCell* __restrict__ cells, const int32_t* __restrict__ dt_cell, int32_t n,
                                                         const double* __restrict__ dt_box, const double* __restrict__ gt_box, double prox_thresh,
                                                         double* __restrict__ iou, uint8_t* __restrict__ in_prox) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const OvmEvalCell c = cells[dt_cell[i]];
  const long row = i - c.dt_off;
  const double dx = dt_box[4L * i], dy = dt_box[4L * i + 1], dw = dt_box[4L * i + 2], dh = dt_box[4L * i + 3];
  bool prox = false;
  for (int g = 0; g < c.n_gt; ++g) {
    const double* q = gt_box + 4L * (c.gt_off + g);
    const double gx = q[0], gy = q[1], gw = q[2], gh = q[3];
    const double iw = np_clip0(np_minimum(dx + dw, gx + gw) - np_maximum(dx, gx));
    const double ih = np_clip0(np_minimum(dy + dh, gy + gh) - np_maximum(dy, gy));
    const double inter = iw * ih;
    const double uni = (dw * dh + gw * gh) - inter;
    const double v = uni > 0.0 ? inter / uni : 0.0;
    if (iou) iou[c.iou_off + row * c.n_gt + g] = v;
    prox = prox || v > prox_thresh;
  }
  if (in_prox) in_prox[i] = prox ? 1 : 0;
}

__global__ __launch_bounds__(256) void eval_match_kernel(const OvmEvalCell* __restrict__ cells, int32_t n_cells, const double* __restrict__ iou,
                                                         const double* __restrict__ dt_rng, const double* __restrict__ gt_rng,
                                                         const uint8_t* __restrict__ gt_flag, const uint8_t* __restrict__ gt_crowd,
                                                         const uint8_t* __restrict__ in_prox, const double* __restrict__ ranges, int32_t n_rng,
                                                         const double* __restrict__ floors, int32_t n_thr, int32_t* __restrict__ pick,
                                                         uint8_t* __restrict__ ignored, int32_t* __restrict__ n_gt_out) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave >= (long)n_cells * n_rng * n_thr) return;                     // uniform over the wave
  const int t = (int)(wave % n_thr);
  const int r = (int)((wave / n_thr) % n_rng);
  const int ci = (int)(wave / ((long)n_thr * n_rng));
  const OvmEvalCell c = cells[ci];
  const int G = c.n_gt, D = c.n_dt, nch = (G + 63) >> 6;
  if (nch > kMaxChunks) return;                                          // refused on the host side
  const double lo = ranges[2 * r], hi = ranges[2 * r + 1], floor_t = floors[t];

  // ground truth of this range: ignore flag or outside the range; boxes past G count as taken so that they are never picked
  uint64_t ign = 0, crowd = 0, taken = 0;
  int n_keep = 0;
  for (int k = 0; k < nch; ++k) {
    const int g = lane + 64 * k;
    bool keep = false;
    if (g < G) {
      const double v = gt_rng[c.gt_off + g];
      const bool ig = gt_flag[c.gt_off + g] != 0 || v < lo || v > hi;
      if (ig) ign |= 1ull << k;
      if (gt_crowd[c.gt_off + g]) crowd |= 1ull << k;
      keep = !ig;
    } else {
      taken |= 1ull << k;
    }
    n_keep += __popcll(__ballot(keep));
  }
  if (t == 0 && lane == 0) n_gt_out[(long)ci * n_rng + r] = n_keep;
  // proximity: every ground truth ignored in this range (or none at all) ignores the whole cell
  const bool prox = c.prox != 0;
  const bool all_ignored = n_keep == 0;

  const long obase = (long)c.dt_off * n_rng * n_thr + (long)(r * n_thr + t) * D;
  int my_pick = -1;
  uint8_t my_ign = 0;
  for (int d = 0; d < D; ++d) {
    const double* row = iou + c.iou_off + (long)d * G;
    double bv0 = -1.0, bv1 = -1.0;                                       // best IoU among the not-ignored / the ignored boxes
    int bg0 = -1, bg1 = -1;
    for (int k = 0; k < nch; ++k) {
      if ((taken >> k) & 1) continue;
      const int g = lane + 64 * k;
      double v = row[g];
      if (v != v) v = 0.0;
      if (v >= floor_t) {
        if ((ign >> k) & 1) {
          if (v >= bv1) { bv1 = v; bg1 = g; }                            // g grows with k: the later box wins a tie
        } else {
          if (v >= bv0) { bv0 = v; bg0 = g; }
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double ov0 = __shfl_xor(bv0, off), ov1 = __shfl_xor(bv1, off);
      const int og0 = __shfl_xor(bg0, off), og1 = __shfl_xor(bg1, off);
      if (ov0 > bv0 || (ov0 == bv0 && og0 > bg0)) { bv0 = ov0; bg0 = og0; }
      if (ov1 > bv1 || (ov1 == bv1 && og1 > bg1)) { bv1 = ov1; bg1 = og1; }
    }
    const int chosen = bg0 >= 0 ? bg0 : bg1;                             // uniform over the wave
    const bool on_ign = bg0 < 0 && bg1 >= 0;
    int pos = -1;
    bool ig;
    if (chosen >= 0) {
      const int kc = chosen >> 6;
      if (lane == (chosen & 63) && !((crowd >> kc) & 1)) taken |= 1ull << kc;
      // index in the ordered ground truth: not-ignored first, file order within each group
      pos = on_ign ? n_keep : 0;
      for (int k = 0; k <= kc; ++k) {
        const int g = lane + 64 * k;
        pos += __popcll(__ballot(g < chosen && (((ign >> k) & 1) != 0) == on_ign));
      }
      ig = on_ign;
    } else {
      const double v = dt_rng[c.dt_off + d];
      ig = v < lo || v > hi;                                             // unmatched and outside the range
    }
    if (prox && (all_ignored || !in_prox[c.dt_off + d])) ig = true;
    if (lane == (d & 63)) { my_pick = pos; my_ign = ig ? 1 : 0; }
    if ((d & 63) == 63 || d == D - 1) {
      const int d0 = d & ~63;
      if (d0 + lane <= d) {
        pick[obase + d0 + lane] = my_pick;
        ignored[obase + d0 + lane] = my_ign;
      }
    }
  }
}

}  // namespace

extern "C" int ovm_eval_iou2d(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, const double* dt_box, const double* gt_box,
                              double prox_thresh, double* iou, uint8_t* in_prox, ovm_stream_t stream) {
  if (n_dt_total < 0) return OVM_ERR_INVALID;
  if (n_dt_total == 0 || (!iou && !in_prox)) return OVM_OK;
  if (!cells || !dt_cell || !dt_box || !gt_box) return OVM_ERR_INVALID;
  hipLaunchKernelGGL(eval_iou2d_kernel, dim3((unsigned)((n_dt_total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cells, dt_cell, n_dt_total,
                     dt_box, gt_box, prox_thresh, iou, in_prox);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

extern "C" int ovm_eval_match(const OvmEvalCell* cells, int32_t n_cells, int32_t max_gt, const double* iou, const double* dt_rng, const double* gt_rng,
                              const uint8_t* gt_flag, const uint8_t* gt_crowd, const uint8_t* in_prox, const double* ranges, int32_t n_rng,
                              const double* floors, int32_t n_thr, int32_t* pick, uint8_t* ignored, int32_t* n_gt, ovm_stream_t stream) {
  if (n_cells < 0 || n_rng <= 0 || n_thr <= 0 || max_gt < 0) return OVM_ERR_INVALID;
  if (max_gt > 64 * kMaxChunks) return OVM_ERR_CAPACITY;
  if (n_cells == 0) return OVM_OK;
  if (!cells || !dt_rng || !ranges || !floors || !pick || !ignored || !n_gt) return OVM_ERR_INVALID;
  if (max_gt > 0 && (!iou || !gt_rng || !gt_flag || !gt_crowd)) return OVM_ERR_INVALID;
  const long waves = (long)n_cells * n_rng * n_thr;
  const long blocks = (waves + 3) / 4;
  if (blocks > 0x7fffffffL) return OVM_ERR_CAPACITY;
  hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cells, n_cells, iou, dt_rng, gt_rng, gt_flag,
                     gt_crowd, in_prox, ranges, n_rng, floors, n_thr, pick, ignored, n_gt);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}
