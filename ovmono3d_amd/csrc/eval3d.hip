// The NHD stage of the Omni3D evaluator on the device: which ground truth a detection is scored against, and the disentangled
// Normalised Hungarian Distance of the pair (reference cubercnn/evaluation/omni3d_evaluation.py: calculate_nhd / disentangled_nhd
// :2227-2290, Omni3DevalWithNHD :2342-2484). The host restatement is Omni3Deval._collect_nhd with evaluation/nhd.py. (The 3D IoU of
// the cells, ovm_eval_iou3d, lives with the per-pair routine it shares with ovm_box3d_iou in box3d.hip.)
//
// One wave64 per detection row. Pairing: the lanes scan the row's IoU block (lane l the boxes l, l + 64, ...), a shuffle arg-max
// picks the first maximum. Scoring: lane l = 8 i + j owns entry (prediction corner i, ground-truth corner j) of each of the five
// 8x8 cost matrices (whole prediction; prediction with only xy / z / dimensions / pose kept). The assignment is solved exactly by
// dynamic programming over subsets of ground-truth corners,
//     dp[mask] = min_{j in mask} dp[mask \ j] + cost[popcount(mask) - 1][j],     dp[0] = 0,
// 256 states per matrix, walked by popcount so that a layer only reads the layer before it: 5 x C(8, k) independent states in layer
// k, 25 passes of the wave in all. Costs (2.5 KB) and tables (10 KB) stay in LDS. The inputs are the fp32 numbers nhd.py rounds to;
// everything after the load is fp64.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cstdint>
#include "../../include/ovm3d.h"

// Equal inputs must give equal corners whichever of the five sets they are built for (identical cuboids score exactly 0):
// no fused multiply-adds in this file.
#pragma clang fp contract(off)

namespace {

constexpr int kMaxGt = 4096;     // as ovm_eval_match

// the 256 subsets of 8 corners ordered by popcount, and where each popcount starts
struct MaskTable { uint8_t mask[256]; int32_t start[10]; };
constexpr MaskTable make_mask_table() {
  MaskTable t{};
  int n = 0;
  for (int k = 0; k <= 8; ++k) {
    t.start[k] = n;
    for (int m = 0; m < 256; ++m) {
      int c = 0;
      for (int b = 0; b < 8; ++b) c += (m >> b) & 1;
      if (c == k) t.mask[n++] = (uint8_t)m;
    }
  }
  t.start[9] = n;
  return t;
}
__constant__ MaskTable kMasks = make_mask_table();

struct Cuboid { double xy[2], z, dim[3], R[9]; };

__device__ __forceinline__ void load_cuboid(const float* __restrict__ p, Cuboid& c) {
  c.xy[0] = p[0]; c.xy[1] = p[1]; c.z = p[2];
  for (int i = 0; i < 3; ++i) c.dim[i] = p[3 + i];
  for (int i = 0; i < 9; ++i) c.R[i] = p[6 + i];
}

// corner k of nhd.cuboid_corners: signs (sx, sy, sz) = bits 0, 1, 2 of k, half extents (L, H, W) / 2 along x, y, z,
// corner = (signs * half) @ R^T + centre
__device__ __forceinline__ void cuboid_corner(int k, const double* xy, double z, const double* dim, const double* R, double out[3]) {
  const double lx = ((k & 1) ? 1.0 : -1.0) * (dim[2] / 2.0), ly = ((k & 2) ? 1.0 : -1.0) * (dim[1] / 2.0), lz = ((k & 4) ? 1.0 : -1.0) * (dim[0] / 2.0);
  out[0] = ((lx * R[0] + ly * R[1]) + lz * R[2]) + xy[0];
  out[1] = ((lx * R[3] + ly * R[4]) + lz * R[5]) + xy[1];
  out[2] = ((lx * R[6] + ly * R[7]) + lz * R[8]) + z;
}

__global__ __launch_bounds__(64) void eval_nhd_kernel(const OvmEvalCell* __restrict__ cells, const int32_t* __restrict__ dt_cell, int32_t n_dt_total,
                                                      const double* __restrict__ iou, double iou_thr, const uint8_t* __restrict__ dt_ok,
                                                      const uint8_t* __restrict__ gt_ok, const float* __restrict__ dt_cuboid,
                                                      const float* __restrict__ gt_cuboid, int32_t* __restrict__ pair_gt, double* __restrict__ nhd,
                                                      uint8_t* __restrict__ status) {
  __shared__ double cost[5][64];
  __shared__ double dp[5][256];
  const int d = blockIdx.x, lane = threadIdx.x;
  if (d >= n_dt_total) return;
  const OvmEvalCell c = cells[dt_cell[d]];
  const int G = c.n_gt;

  // (a) the first maximum of the row
  const double* row = iou + c.iou_off + (long)(d - c.dt_off) * G;
  double bv = -1.0;
  int bg = INT_MAX;
  for (int g = lane; g < G; g += 64) {
    const double v = row[g];
    if (v > bv) { bv = v; bg = g; }                                        // g grows: the earlier box keeps a tie
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off);
    const int og = __shfl_xor(bg, off);
    if (ov > bv || (ov == bv && og < bg)) { bv = ov; bg = og; }
  }
  const bool paired = bg < G && bv > 0.0 && bv >= iou_thr && dt_ok[d] != 0 && gt_ok[c.gt_off + bg] != 0;     // uniform over the wave
  if (!paired) {
    if (lane == 0) { pair_gt[d] = -1; status[d] = OVM_NHD_NONE; }
    return;
  }

  // (b) the five cost matrices
  Cuboid p, q;
  load_cuboid(dt_cuboid + 15L * d, p);
  load_cuboid(gt_cuboid + 15L * (c.gt_off + bg), q);
  const int ci = lane >> 3, cj = lane & 7;
  double gc[3];
  cuboid_corner(cj, q.xy, q.z, q.dim, q.R, gc);
  bool bad = false;
  for (int m = 0; m < 5; ++m) {
    double pc[3];
    cuboid_corner(ci, (m == 0 || m == 1) ? p.xy : q.xy, (m == 0 || m == 2) ? p.z : q.z, (m == 0 || m == 3) ? p.dim : q.dim,
                  (m == 0 || m == 4) ? p.R : q.R, pc);
    const double dx = pc[0] - gc[0], dy = pc[1] - gc[1], dz = pc[2] - gc[2];
    const double v = sqrt((dx * dx + dy * dy) + dz * dz);
    bad = bad || !(fabs(v) <= DBL_MAX);
    cost[m][lane] = v;
  }
  if (__ballot(bad) != 0) {                                                // scipy refuses such a matrix, the evaluator drops the pair
    if (lane == 0) { pair_gt[d] = -1; status[d] = OVM_NHD_SKIPPED; }
    return;
  }
  if (lane < 5) dp[lane][0] = 0.0;
  __syncthreads();

  // the assignments, one popcount layer at a time
  for (int k = 1; k <= 8; ++k) {
    const int start = kMasks.start[k], cnt = kMasks.start[k + 1] - start;
    for (int t = lane; t < 5 * cnt; t += 64) {
      const int m = t / cnt, mask = kMasks.mask[start + t % cnt];
      double best = DBL_MAX;
      for (int j = 0; j < 8; ++j) {
        if ((mask >> j) & 1) {
          const double v = dp[m][mask ^ (1 << j)] + cost[m][(k - 1) * 8 + j];
          best = v < best ? v : best;
        }
      }
      dp[m][mask] = best;
    }
    __syncthreads();
  }

  // the ground truth's axis-aligned extent
  double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (int k = 0; k < 8; ++k) {
    double g3[3];
    cuboid_corner(k, q.xy, q.z, q.dim, q.R, g3);
    for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], g3[a]); hi[a] = fmax(hi[a], g3[a]); }
  }
  const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  const double diag = sqrt((ex * ex + ey * ey) + ez * ez);
  if (lane < 5) nhd[5L * d + lane] = dp[lane][255] / diag;
  if (lane == 0) { pair_gt[d] = bg; status[d] = OVM_NHD_OK; }
}

}  // namespace

extern "C" int ovm_eval_nhd(const OvmEvalCell* cells, const int32_t* dt_cell, int32_t n_dt_total, int32_t max_gt, const double* iou, double iou_thr,
                            const uint8_t* dt_ok, const uint8_t* gt_ok, const float* dt_cuboid, const float* gt_cuboid, int32_t* pair_gt, double* nhd,
                            uint8_t* status, ovm_stream_t stream) {
  if (n_dt_total < 0 || max_gt < 0) return OVM_ERR_INVALID;
  if (max_gt > kMaxGt) return OVM_ERR_CAPACITY;
  if (n_dt_total == 0) return OVM_OK;
  if (!cells || !dt_cell || !dt_ok || !dt_cuboid || !pair_gt || !nhd || !status) return OVM_ERR_INVALID;
  if (max_gt > 0 && (!iou || !gt_ok || !gt_cuboid)) return OVM_ERR_INVALID;
  hipLaunchKernelGGL(eval_nhd_kernel, dim3((unsigned)n_dt_total), dim3(64), 0, (hipStream_t)stream, cells, dt_cell, n_dt_total, iou, iou_thr, dt_ok,
                     gt_ok, dt_cuboid, gt_cuboid, pair_gt, nhd, status);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}
