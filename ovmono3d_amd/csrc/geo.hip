// OVMono3D-GEO on the device: mask -> points -> yaw -> DBSCAN -> extents for all instances of one image in one launch sequence
// (reference tools/ovmono3d_geo.py:127-258; the steps are listed in include/ovm3d.h, the numpy restatement is tests/geo_oracle.py).
//
// Everything that decides a result is fp64. Sums are two-level with a fixed shape (1024 points per partial, partials added in a
// fixed tree), so an instance's numbers do not depend on what else is in the batch; every cross-block accumulation is an integer
// atomic or a min / max, which do not depend on arrival order either.
//
// DBSCAN, the simple form: LDS-tiled all-pairs sweeps over an instance's points (24 B each, at most max_points of them: L2
// resident). A block owns 512 rows (256 threads x 2 rows in registers) and a chunk of 4096 columns, staged 256 at a time in LDS
// as three fp64 arrays that every lane reads at the same address (a broadcast, no bank conflict). Three sweeps per trial:
//   COUNT   neighbours within eps of every point (itself included)  -> core flags
//   UNION   union-find over core-core pairs j > i: 32-bit parents, the larger root hooked under the smaller with atomicCAS, so
//           every root is its component's smallest core index; a snapshot of the column tile's parents skips the pairs already
//           known to share the row's root
//   BORDER  a non-core point takes the min over its core neighbours' roots
// Labels are the rank of the root among the roots in ascending order, which is scikit-learn's numbering.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>
#include "../../include/ovm3d.h"
#include "geo_point.hpp"

// The restatement is numpy: no fused multiply-adds except where a function opts in.
#pragma clang fp contract(off)

namespace {

constexpr int kChunk = 1024;        // points per partial sum
constexpr int kRows = 512;          // rows per sweep block
constexpr int kTile = 256;          // columns per LDS tile
constexpr int kColChunk = 4096;     // columns per sweep block
constexpr int kNoRoot = 0x7fffffff;
constexpr int kFlagMismatch = 1, kFlagNonFinite = 2, kFlagBadPerm = 4;
enum { SWEEP_COUNT = 0, SWEEP_UNION = 1, SWEEP_BORDER = 2 };

struct GeoDesc {                    // one instance, built on the host
  const uint8_t* mask;
  const int32_t* perm;
  int32_t x0, y0, x1, y1;           // pixel range scanned (rectangle: clipped; mask plane: the image)
  int32_t n_decl, n_used, status0, pad;
  int64_t pts_off, clu_off;         // first point in the raw / the clustering buffer
};

struct GeoState {                   // one instance, device only
  double mean[3];
  double yaw;
  int32_t n_actual, flags, active, n_kept;
};

struct DbArgs {
  const GeoDesc* desc;
  GeoState* state;
  const double* pts;                // [total_used][3]
  int32_t *cnt, *parent, *root, *broot, *csize, *rank;
  int32_t* labels;                  // may be null
};

thread_local char g_err[256] = "";
int fail(int code, const char* msg) {
  std::snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

__device__ __forceinline__ int ld_relaxed(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Exclusive prefix sum of v over a block of 1024 threads; *total receives the block's sum. scratch: 17 ints of LDS.
__device__ int block_excl_scan_1024(int v, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  __syncthreads();
  if (lane == 63) scratch[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < 16; ++k) { const int t = scratch[k]; scratch[k] = run; run += t; }
    scratch[16] = run;
  }
  __syncthreads();
  *total = scratch[16];
  return scratch[w] + inc - v;
}

__device__ __forceinline__ bool inst_ok(const GeoDesc& d, const GeoState& s) { return d.status0 == 0 && s.flags == 0; }

__global__ void k_init(const GeoDesc* desc, GeoState* state, OvmGeoResult* res, int n_inst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inst) return;
  OvmGeoResult r;
  memset(&r, 0, sizeof(r));
  r.n_points = desc[i].n_decl;
  r.status = desc[i].status0;
  res[i] = r;
  GeoState s;
  memset(&s, 0, sizeof(s));
  state[i] = s;
}

__device__ __forceinline__ bool in_mask(const GeoDesc& d, int W, int y, int x) { return d.mask ? d.mask[(long)y * W + x] != 0 : true; }

// points per image row of every instance
__global__ __launch_bounds__(256) void k_row_count(const GeoDesc* desc, int H, int W, int32_t* rowcnt) {
  const int inst = blockIdx.y, y = blockIdx.x;
  const GeoDesc d = desc[inst];
  if (d.status0 != 0) return;
  __shared__ int wsum[4];
  int c = 0;
  if (y >= d.y0 && y < d.y1) {
    if (!d.mask) {
      c = threadIdx.x == 0 ? d.x1 - d.x0 : 0;
    } else {
      for (int x = d.x0 + threadIdx.x; x < d.x1; x += 256) c += d.mask[(long)y * W + x] != 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) rowcnt[(long)inst * H + y] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void k_row_scan(const GeoDesc* desc, GeoState* state, OvmGeoResult* res, int H, const int32_t* rowcnt,
                                                   int32_t* rowoff) {
  const int inst = blockIdx.x;
  const GeoDesc d = desc[inst];
  if (d.status0 != 0) return;
  __shared__ int scratch[17];
  int base = 0;
  for (int h0 = 0; h0 < H; h0 += 1024) {
    const int h = h0 + threadIdx.x;
    const int v = h < H ? rowcnt[(long)inst * H + h] : 0;
    int total;
    const int ex = block_excl_scan_1024(v, scratch, &total);
    if (h < H) rowoff[(long)inst * H + h] = base + ex;
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state[inst].n_actual = base;
    res[inst].n_points = base;
    if (base != d.n_decl) state[inst].flags = kFlagMismatch;
  }
}

// row-major compaction of the mask pixels and un-projection in one pass
__global__ __launch_bounds__(256) void k_scatter(const GeoDesc* desc, GeoState* state, const float* __restrict__ depth, int H, int W, double fx,
                                                 double fy, double cx, double cy, const double* __restrict__ frame, const int32_t* rowoff, double* pts) {
  const int inst = blockIdx.y, y = blockIdx.x;
  const GeoDesc d = desc[inst];
  if (d.status0 != 0 || y < d.y0 || y >= d.y1) return;
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long run = rowoff[(long)inst * H + y];
  double* out = pts + 3 * d.pts_off;
  bool bad = false;
  for (int xb = d.x0; xb < d.x1; xb += 256) {
    const int x = xb + threadIdx.x;
    const bool in = x < d.x1 && in_mask(d, W, y, x);
    const unsigned long long b = __ballot(in);
    if (lane == 0) wcnt[w] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) before += wcnt[k];
    const int all = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    const long idx = run + before;
    if (in && idx < d.n_decl) {
      const float zf = depth[(long)y * W + x];
      if (!isfinite(zf)) bad = true;
      geo_unproject(zf, x, y, fx, fy, cx, cy, frame, out + 3 * idx);
    }
    run += all;
    __syncthreads();
  }
  if (bad) atomicOr(&state[inst].flags, kFlagNonFinite);
}

// Partial sums over 1024 points. MODE 0: the points; MODE 1: the centred second moments of (x, z): xx, xz, zz.
template <int MODE>
__global__ __launch_bounds__(256) void k_partial(const GeoDesc* desc, const GeoState* state, const double* pts, int max_chunks, double* partial) {
  const int inst = blockIdx.y, c = blockIdx.x;
  const GeoDesc d = desc[inst];
  const GeoState s = state[inst];
  if (!inst_ok(d, s)) return;
  const int n = d.n_decl;
  if ((long)c * kChunk >= n) return;
  const double* p = pts + 3 * d.pts_off;
  __shared__ double red[3][256];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int k = 0; k < kChunk / 256; ++k) {
    const long i = (long)c * kChunk + k * 256 + threadIdx.x;
    if (i < n) {
      if (MODE == 0) {
        a0 += p[3 * i]; a1 += p[3 * i + 1]; a2 += p[3 * i + 2];
      } else {
        const double x = p[3 * i] - s.mean[0], z = p[3 * i + 2] - s.mean[2];
        a0 += x * x; a1 += x * z; a2 += z * z;
      }
    }
  }
  red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1; red[2][threadIdx.x] = a2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 3) partial[((long)inst * max_chunks + c) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

template <int MODE>
__global__ __launch_bounds__(256) void k_final(const GeoDesc* desc, GeoState* state, OvmGeoResult* res, int max_chunks, const double* partial) {
  const int inst = blockIdx.x;
  const GeoDesc d = desc[inst];
  const GeoState s = state[inst];
  if (d.status0 != 0) return;
  if (s.flags != 0) {
    if (MODE == 0 && threadIdx.x == 0) res[inst].status = (s.flags & kFlagMismatch) ? OVM_GEO_COUNT_MISMATCH : OVM_GEO_NONFINITE;
    return;
  }
  const int n = d.n_decl, nch = (n + kChunk - 1) / kChunk;
  __shared__ double red[3][256];
  double a[3] = {0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < nch; c += 256)
    for (int k = 0; k < 3; ++k) a[k] += partial[((long)inst * max_chunks + c) * 3 + k];
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (MODE == 0) {
    for (int k = 0; k < 3; ++k) {
      const double m = red[k][0] / (double)n;
      state[inst].mean[k] = m;
      res[inst].offset[k] = m;
    }
  } else {
    // unit eigenvector of [[a, b], [b, c]] for the larger eigenvalue l = (a + c) / 2 + r: (l - c, b) or (b, l - a), whichever
    // has no cancellation; sign as scikit-learn's svd_flip (the entry of larger magnitude positive, the first on a tie)
    const double va = red[0][0], vb = red[1][0], vc = red[2][0];
    const double h = (va - vc) / 2.0, r = hypot(h, vb);
    double v0, v1;
    if (va >= vc) { v0 = h + r; v1 = vb; } else { v0 = vb; v1 = r - h; }
    if (v0 == 0.0 && v1 == 0.0) v0 = 1.0;
    const bool neg = fabs(v1) > fabs(v0) ? v1 < 0.0 : v0 < 0.0;
    if (neg) { v0 = -v0; v1 = -v1; }
    const double yaw = atan2(v1, v0);
    state[inst].yaw = yaw;
    res[inst].yaw = yaw;
    res[inst].n_used = d.n_used;
  }
}

// T = Ry(-yaw) (p - offset) + offset for the rows the down-sampling keeps
__global__ __launch_bounds__(256) void k_rotate_gather(const GeoDesc* desc, GeoState* state, const double* pts, double* clu) {
  const int inst = blockIdx.y;
  const GeoDesc d = desc[inst];
  const GeoState s = state[inst];
  if (!inst_ok(d, s)) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d.n_used) return;
  int src = j;
  if (d.n_decl > d.n_used) {
    src = d.perm[j];
    if (src < 0 || src >= d.n_decl) { atomicOr(&state[inst].flags, kFlagBadPerm); return; }
  }
  const double* p = pts + 3 * (d.pts_off + src);
  const double x = p[0] - s.mean[0], y = p[1] - s.mean[1], z = p[2] - s.mean[2];
  const double c = cos(-s.yaw), sn = sin(-s.yaw);
  double* o = clu + 3 * (d.clu_off + j);
  o[0] = (c * x + -sn * z) + s.mean[0];
  o[1] = y + s.mean[1];
  o[2] = (sn * x + c * z) + s.mean[2];
}

__global__ void k_activate(const GeoDesc* desc, GeoState* state, OvmGeoResult* res, int n_inst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inst) return;
  if (desc[i].status0 != 0) return;
  const int f = state[i].flags;
  if (f & kFlagBadPerm) {
    if (!(f & (kFlagMismatch | kFlagNonFinite))) res[i].status = OVM_GEO_BAD_PERM;
  }
  if (f != 0) {
    OvmGeoResult r;
    memset(&r, 0, sizeof(r));
    r.n_points = res[i].n_points;
    r.status = res[i].status;
    res[i] = r;
  }
  state[i].active = f == 0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ DBSCAN
__global__ __launch_bounds__(256) void k_db_reset(DbArgs a) {
  const int inst = blockIdx.y;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.state[inst].n_kept = 0;
  if (i >= d.n_used) return;
  const long g = d.clu_off + i;
  a.cnt[g] = 0;
  a.csize[g] = 0;
  a.parent[g] = i;
  a.broot[g] = kNoRoot;
}

__device__ int uf_find(int32_t* par, int x) {
  for (;;) {
    const int p = ld_relaxed(par + x);
    if (p == x) return x;
    const int gp = ld_relaxed(par + p);
    if (gp == p) return p;
    atomicMin(par + x, gp);          // path halving: every value ever stored in par[x] is an ancestor of x, the smallest is the highest
    x = gp;
  }
}

// joins the components of a and b; returns their root (the smaller index) as of the join
__device__ int uf_unite(int32_t* par, int a, int b) {
  a = uf_find(par, a);
  b = uf_find(par, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(par + hi, hi, lo);
    if (old == hi) return lo;
    a = uf_find(par, old);           // hi was hooked by someone else meanwhile
    b = uf_find(par, lo);
  }
  return a;
}

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(fast)
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return dx * dx + dy * dy + dz * dz;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_db_sweep(DbArgs a, double eps2, int min_samples) {
  const int inst = blockIdx.z;
  if (!a.state[inst].active) return;                                     // uniform over the block
  const GeoDesc d = a.desc[inst];
  const int n = d.n_used, row0 = blockIdx.y * kRows, c0 = blockIdx.x * kColChunk;
  if (row0 >= n || c0 >= n) return;
  const int c1 = min(n, c0 + kColChunk);
  if (MODE == SWEEP_UNION && c1 - 1 <= row0) return;                     // only pairs j > i
  const double* P = a.pts + 3 * d.clu_off;
  int32_t* cnt = a.cnt + d.clu_off;
  int32_t* par = a.parent + d.clu_off;
  const int32_t* root = a.root + d.clu_off;
  __shared__ double sx[kTile], sy[kTile], sz[kTile];
  __shared__ int sa[kTile];
  const int tid = threadIdx.x;
  int ri[2];
  double px[2], py[2], pz[2];
  bool act[2];
  int acc[2];
  for (int r = 0; r < 2; ++r) {
    const int i = row0 + r * 256 + tid;
    ri[r] = i;
    act[r] = i < n;
    px[r] = py[r] = pz[r] = 0.0;
    if (act[r]) {
      px[r] = P[3 * (long)i]; py[r] = P[3 * (long)i + 1]; pz[r] = P[3 * (long)i + 2];
      if (MODE == SWEEP_UNION) act[r] = cnt[i] >= min_samples;
      if (MODE == SWEEP_BORDER) act[r] = cnt[i] < min_samples;
    }
    acc[r] = MODE == SWEEP_BORDER ? kNoRoot : 0;
  }
  for (int t0 = c0; t0 < c1; t0 += kTile) {
    if (MODE == SWEEP_UNION && t0 + kTile - 1 <= row0) continue;         // uniform: every column of the tile is <= every row
    __syncthreads();
    {
      const int j = t0 + tid;
      if (j < n) {
        sx[tid] = P[3 * (long)j]; sy[tid] = P[3 * (long)j + 1]; sz[tid] = P[3 * (long)j + 2];
        if (MODE == SWEEP_UNION) sa[tid] = cnt[j] >= min_samples ? ld_relaxed(par + j) : -1;
        if (MODE == SWEEP_BORDER) sa[tid] = root[j];
      } else {
        sx[tid] = sy[tid] = sz[tid] = 1e300;                             // squares to +inf: never within eps
        sa[tid] = MODE == SWEEP_UNION ? -1 : kNoRoot;
      }
    }
    __syncthreads();
    const int lim = min(kTile, c1 - t0);
    for (int jj = 0; jj < lim; ++jj) {
      const double x = sx[jj], y = sy[jj], z = sz[jj];
      for (int r = 0; r < 2; ++r) {
        const bool hit = dist2(px[r], py[r], pz[r], x, y, z) <= eps2;
        if (MODE == SWEEP_COUNT) {
          acc[r] += hit ? 1 : 0;
        } else if (MODE == SWEEP_UNION) {
          const int pj = sa[jj];
          if (hit && act[r] && pj >= 0 && pj != ri[r] && t0 + jj > row0 + r * 256 + tid) ri[r] = uf_unite(par, ri[r], t0 + jj);
        } else {
          if (hit && act[r]) acc[r] = min(acc[r], sa[jj]);
        }
      }
    }
  }
  for (int r = 0; r < 2; ++r) {
    const int i = row0 + r * 256 + tid;
    if (MODE == SWEEP_COUNT && i < n) atomicAdd(cnt + i, acc[r]);
    if (MODE == SWEEP_BORDER && act[r] && acc[r] != kNoRoot) atomicMin(a.broot + d.clu_off + i, acc[r]);
  }
}

// root[i] = the component's smallest core index for a core point, none for the others
__global__ __launch_bounds__(256) void k_db_flatten(DbArgs a, int min_samples) {
  const int inst = blockIdx.y;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n_used) return;
  const long g = d.clu_off + i;
  a.root[g] = a.cnt[g] >= min_samples ? uf_find(a.parent + d.clu_off, i) : kNoRoot;
}

// rank[i] = the number of roots below i (read for roots only)
__global__ __launch_bounds__(1024) void k_db_rank(DbArgs a) {
  const int inst = blockIdx.x;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  __shared__ int scratch[17];
  int base = 0;
  for (int i0 = 0; i0 < d.n_used; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const int v = (i < d.n_used && a.root[d.clu_off + i] == i) ? 1 : 0;
    int total;
    const int ex = block_excl_scan_1024(v, scratch, &total);
    if (i < d.n_used) a.rank[d.clu_off + i] = base + ex;
    base += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_db_label(DbArgs a) {
  const int inst = blockIdx.y;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n_used) return;
  const long g = d.clu_off + i;
  const int r = a.root[g];
  const int lr = r != kNoRoot ? r : a.broot[g];
  a.broot[g] = lr;
  if (lr != kNoRoot) atomicAdd(a.csize + d.clu_off + lr, 1);
  if (a.labels) a.labels[g] = lr != kNoRoot ? a.rank[d.clu_off + lr] : -1;
}

// kept flag per point (left in cnt) and their number
__global__ __launch_bounds__(256) void k_db_keep(DbArgs a, double min_cluster_frac, int min_cluster) {
  const int inst = blockIdx.y;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool kept = false;
  if (i < d.n_used) {
    const long g = d.clu_off + i;
    const int lr = a.broot[g];
    if (lr != kNoRoot) {
      const int size = a.csize[d.clu_off + lr];
      kept = !((double)size / (double)d.n_used < min_cluster_frac || size <= min_cluster);
    }
    a.cnt[g] = kept ? 1 : 0;
  }
  const int c = __popcll(__ballot(kept));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&a.state[inst].n_kept, c);
}

// acceptance, and the extents once the instance is settled
__global__ __launch_bounds__(1024) void k_db_decide(DbArgs a, OvmGeoResult* res, int trial, int is_last, double eps, double accept_frac) {
  const int inst = blockIdx.x;
  if (!a.state[inst].active) return;
  const GeoDesc d = a.desc[inst];
  const int n = d.n_used, n_kept = a.state[inst].n_kept;
  const bool accepted = (double)n_kept > accept_frac * (double)n;
  if (!accepted && !is_last) return;
  const double* P = a.pts + 3 * d.clu_off;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < n; i += 1024) {
    if (accepted && !a.cnt[d.clu_off + i]) continue;
    for (int k = 0; k < 3; ++k) {
      const double v = P[3 * (long)i + k];
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
  __shared__ double slo[3][16], shi[3][16];
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
    if ((threadIdx.x & 63) == 0) { slo[k][threadIdx.x >> 6] = lo[k]; shi[k][threadIdx.x >> 6] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    OvmGeoResult* r = res + inst;
    for (int k = 0; k < 3; ++k) {
      double l = slo[k][0], h = shi[k][0];
      for (int w = 1; w < 16; ++w) { l = fmin(l, slo[k][w]); h = fmax(h, shi[k][w]); }
      r->ext_min[k] = l;
      r->ext_max[k] = h;
    }
    r->n_kept = accepted ? n_kept : n;
    r->trial = accepted ? trial : 0;
    r->eps = eps;
    a.state[inst].active = 0;
  }
}

__global__ void k_db_single(GeoDesc* desc, GeoState* state, int n) {
  GeoDesc d;
  memset(&d, 0, sizeof(d));
  d.n_decl = d.n_used = n;
  desc[0] = d;
  GeoState s;
  memset(&s, 0, sizeof(s));
  s.active = 1;
  state[0] = s;
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

struct DbLayout { int64_t cnt, parent, root, broot, csize, rank, total; };
DbLayout db_layout(int64_t base, int64_t n) {
  DbLayout L;
  int64_t o = base;
  const int64_t sz = align256(4 * std::max<int64_t>(n, 1));
  L.cnt = o; o += sz; L.parent = o; o += sz; L.root = o; o += sz; L.broot = o; o += sz; L.csize = o; o += sz; L.rank = o; o += sz;
  L.total = o;
  return L;
}

DbArgs db_args(uint8_t* ws, const DbLayout& L) {
  DbArgs a{};
  a.cnt = (int32_t*)(ws + L.cnt); a.parent = (int32_t*)(ws + L.parent); a.root = (int32_t*)(ws + L.root);
  a.broot = (int32_t*)(ws + L.broot); a.csize = (int32_t*)(ws + L.csize); a.rank = (int32_t*)(ws + L.rank);
  return a;
}

// one DBSCAN run over every active instance: reset .. labels
void db_launch(const DbArgs& a, int n_inst, int max_used, double eps, int min_samples, hipStream_t s) {
  const dim3 pg((unsigned)((max_used + 255) / 256), (unsigned)n_inst);
  const dim3 sg((unsigned)((max_used + kColChunk - 1) / kColChunk), (unsigned)((max_used + kRows - 1) / kRows), (unsigned)n_inst);
  const double eps2 = eps * eps;
  hipLaunchKernelGGL(k_db_reset, pg, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_db_sweep<SWEEP_COUNT>, sg, dim3(256), 0, s, a, eps2, min_samples);
  hipLaunchKernelGGL(k_db_sweep<SWEEP_UNION>, sg, dim3(256), 0, s, a, eps2, min_samples);
  hipLaunchKernelGGL(k_db_flatten, pg, dim3(256), 0, s, a, min_samples);
  hipLaunchKernelGGL(k_db_sweep<SWEEP_BORDER>, sg, dim3(256), 0, s, a, eps2, min_samples);
  hipLaunchKernelGGL(k_db_rank, dim3((unsigned)n_inst), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(k_db_label, pg, dim3(256), 0, s, a);
}

bool params_ok(const OvmGeoParams* p) {
  return p && std::isfinite(p->eps0) && p->eps0 > 0.0 && std::isfinite(p->min_cluster_frac) && std::isfinite(p->accept_frac) &&
         p->min_samples >= 1 && p->max_points >= 1 && p->trials >= 1 && p->trials <= 8 && p->min_cluster >= 0 && p->last_stage >= 0;
}

struct Plan {
  std::vector<GeoDesc> desc;
  int64_t total_pts = 0, total_used = 0;
  int max_n = 0, max_used = 0, max_chunks = 1;
  int64_t o_desc = 0, o_state = 0, o_rowcnt = 0, o_rowoff = 0, o_pts = 0, o_partial = 0, o_clu = 0, total = 0;
  DbLayout db{};
};

int make_plan(const OvmGeoInstance* inst, int32_t n_inst, int32_t H, int32_t W, const OvmGeoParams* p, Plan* P) {
  if (n_inst < 0 || n_inst > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL || H > 65535) return fail(OVM_ERR_INVALID, "geo: bad n_inst / H / W");
  if (!params_ok(p)) return fail(OVM_ERR_INVALID, "geo: invalid OvmGeoParams");
  if (n_inst > 0 && !inst) return fail(OVM_ERR_INVALID, "geo: null instance array");
  P->desc.resize((size_t)n_inst);
  for (int i = 0; i < n_inst; ++i) {
    const OvmGeoInstance& in = inst[i];
    GeoDesc d{};
    d.mask = in.mask;
    d.perm = in.perm;
    int64_t n;
    if (in.mask) {
      if (in.n_points < 0 || (int64_t)in.n_points > (int64_t)H * W) return fail(OVM_ERR_INVALID, "geo: n_points of a mask instance outside 0 .. H*W");
      d.x0 = 0; d.y0 = 0; d.x1 = W; d.y1 = H;
      n = in.n_points;
      if (n == 0) d.status0 = OVM_GEO_EMPTY;
    } else {
      const int32_t* r = in.rect;
      d.x0 = std::max(r[0], 0); d.y0 = std::max(r[1], 0); d.x1 = std::min(r[2], W); d.y1 = std::min(r[3], H);
      if (r[2] <= r[0] || r[3] <= r[1]) { d.status0 = OVM_GEO_EMPTY; n = 0; }
      else if (d.x1 <= d.x0 || d.y1 <= d.y0) { d.status0 = OVM_GEO_RECT_OUTSIDE; n = 0; }
      else n = (int64_t)(d.x1 - d.x0) * (d.y1 - d.y0);
      if (n == 0) { d.x0 = d.y0 = d.x1 = d.y1 = 0; }
    }
    if (d.status0 == 0 && n < 2) d.status0 = OVM_GEO_TOO_FEW;
    if (d.status0 == 0 && n > p->max_points && !in.perm) {
      char msg[200];
      std::snprintf(msg, sizeof(msg), "geo: instance %d has %lld points (more than max_points = %d) and no perm", i, (long long)n, p->max_points);
      return fail(OVM_ERR_UNSUPPORTED, msg);
    }
    d.n_decl = (int32_t)n;
    const int64_t stored = d.status0 == 0 ? n : 0;
    d.n_used = (int32_t)std::min<int64_t>(stored, p->max_points);
    d.pts_off = P->total_pts;
    d.clu_off = P->total_used;
    P->total_pts += stored;
    P->total_used += d.n_used;
    P->max_n = std::max<int>(P->max_n, (int)stored);
    P->max_used = std::max(P->max_used, d.n_used);
    P->desc[(size_t)i] = d;
  }
  if (P->total_pts > 0x7fffffffLL / 4) return fail(OVM_ERR_CAPACITY, "geo: too many points in one call");
  P->max_chunks = std::max(1, (P->max_n + kChunk - 1) / kChunk);
  int64_t o = 0;
  const int64_t ni = std::max(n_inst, 1);
  P->o_desc = o; o += align256(ni * (int64_t)sizeof(GeoDesc));
  P->o_state = o; o += align256(ni * (int64_t)sizeof(GeoState));
  P->o_rowcnt = o; o += align256(ni * H * 4);
  P->o_rowoff = o; o += align256(ni * H * 4);
  P->o_pts = o; o += align256(std::max<int64_t>(P->total_pts, 1) * 24);
  P->o_partial = o; o += align256(ni * P->max_chunks * 24);
  P->o_clu = o; o += align256(std::max<int64_t>(P->total_used, 1) * 24);
  P->db = db_layout(o, P->total_used);
  P->total = P->db.total;
  return OVM_OK;
}

std::mutex g_stage_mu;
uint8_t* g_stage = nullptr;
size_t g_stage_cap = 0;
hipEvent_t g_stage_ev = nullptr;

}  // namespace

int geo_fail(int code, const char* msg) { return fail(code, msg); }

extern "C" {

const char* ovm_geo_last_error(void) { return g_err; }

int ovm_geo_default_params(OvmGeoParams* p) {
  if (!p) return fail(OVM_ERR_INVALID, "geo: null params");
  std::memset(p, 0, sizeof(*p));
  p->eps0 = 0.01; p->min_cluster_frac = 0.1; p->accept_frac = 0.5;
  p->min_samples = 100; p->max_points = 40000; p->trials = 4; p->min_cluster = 100;
  return OVM_OK;
}

int ovm_geo_lift_workspace(const OvmGeoInstance* inst, int32_t n_inst, int32_t H, int32_t W, const OvmGeoParams* params, int64_t* bytes,
                           int64_t* label_offsets) {
  if (!bytes) return fail(OVM_ERR_INVALID, "geo: null bytes");
  Plan P;
  const int rc = make_plan(inst, n_inst, H, W, params, &P);
  if (rc != OVM_OK) return rc;
  *bytes = P.total;
  if (label_offsets) {
    for (int i = 0; i < n_inst; ++i) label_offsets[i] = P.desc[(size_t)i].clu_off;
    label_offsets[n_inst] = P.total_used;
  }
  return OVM_OK;
}

int ovm_geo_lift(const float* depth, int32_t H, int32_t W, const double* K, const OvmGeoInstance* inst, int32_t n_inst,
                 const OvmGeoParams* params, OvmGeoResult* results, int32_t* labels, void* workspace, int64_t workspace_bytes,
                 ovm_stream_t stream) {
  return ovm_geo_lift_frame(depth, H, W, K, inst, n_inst, params, nullptr, results, labels, workspace, workspace_bytes, stream);
}

int ovm_geo_lift_frame(const float* depth, int32_t H, int32_t W, const double* K, const OvmGeoInstance* inst, int32_t n_inst,
                       const OvmGeoParams* params, const double* frame, OvmGeoResult* results, int32_t* labels, void* workspace,
                       int64_t workspace_bytes, ovm_stream_t stream) {
  if (!depth || !K || !results || !workspace) return fail(OVM_ERR_INVALID, "geo: null depth / K / results / workspace");
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.0 || fy == 0.0)
    return fail(OVM_ERR_INVALID, "geo: K needs finite, nonzero focal lengths and a finite principal point");
  Plan P;
  const int rc = make_plan(inst, n_inst, H, W, params, &P);
  if (rc != OVM_OK) return rc;
  if (workspace_bytes < P.total) return fail(OVM_ERR_CAPACITY, "geo: workspace too small (ask ovm_geo_lift_workspace)");
  if (n_inst == 0) return OVM_OK;

  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  const size_t dbytes = (size_t)n_inst * sizeof(GeoDesc);
  {
    std::lock_guard<std::mutex> lock(g_stage_mu);
    if (g_stage_ev) {
      if (hipEventSynchronize(g_stage_ev) != hipSuccess) return fail(OVM_ERR_HIP, "geo: staging event");
    } else if (hipEventCreateWithFlags(&g_stage_ev, hipEventDisableTiming) != hipSuccess) {
      return fail(OVM_ERR_HIP, "geo: staging event");
    }
    if (g_stage_cap < dbytes) {
      if (g_stage) (void)hipHostFree(g_stage);
      g_stage = nullptr; g_stage_cap = 0;
      if (hipHostMalloc((void**)&g_stage, dbytes, hipHostMallocPortable) != hipSuccess) { g_stage = nullptr; return fail(OVM_ERR_HIP, "geo: staging buffer"); }
      g_stage_cap = dbytes;
    }
    std::memcpy(g_stage, P.desc.data(), dbytes);
    if (hipMemcpyAsync(ws + P.o_desc, g_stage, dbytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail(OVM_ERR_HIP, "geo: upload");
    if (hipEventRecord(g_stage_ev, s) != hipSuccess) return fail(OVM_ERR_HIP, "geo: staging event");
  }

  const GeoDesc* desc = (const GeoDesc*)(ws + P.o_desc);
  GeoState* state = (GeoState*)(ws + P.o_state);
  int32_t* rowcnt = (int32_t*)(ws + P.o_rowcnt);
  int32_t* rowoff = (int32_t*)(ws + P.o_rowoff);
  double* pts = (double*)(ws + P.o_pts);
  double* partial = (double*)(ws + P.o_partial);
  double* clu = (double*)(ws + P.o_clu);
  const OvmGeoParams& p = *params;
  const int stage = p.last_stage == 0 ? 1 << 30 : p.last_stage;
  const dim3 ig((unsigned)((n_inst + 63) / 64));
  const dim3 rg((unsigned)H, (unsigned)n_inst);

  // an instance that is refused on the device (or stopped early by last_stage) keeps -1 everywhere
  if (labels && P.total_used > 0 && hipMemsetAsync(labels, 0xff, (size_t)P.total_used * 4, s) != hipSuccess) return fail(OVM_ERR_HIP, "geo: memset");
  hipLaunchKernelGGL(k_init, ig, dim3(64), 0, s, desc, state, results, n_inst);
  hipLaunchKernelGGL(k_row_count, rg, dim3(256), 0, s, desc, H, W, rowcnt);
  hipLaunchKernelGGL(k_row_scan, dim3((unsigned)n_inst), dim3(1024), 0, s, desc, state, results, H, rowcnt, rowoff);
  hipLaunchKernelGGL(k_scatter, rg, dim3(256), 0, s, desc, state, depth, H, W, fx, fy, cx, cy, frame, rowoff, pts);
  if (stage >= 2) {
    const dim3 cg((unsigned)P.max_chunks, (unsigned)n_inst);
    hipLaunchKernelGGL(k_partial<0>, cg, dim3(256), 0, s, desc, state, pts, P.max_chunks, partial);
    hipLaunchKernelGGL(k_final<0>, dim3((unsigned)n_inst), dim3(256), 0, s, desc, state, results, P.max_chunks, partial);
    hipLaunchKernelGGL(k_partial<1>, cg, dim3(256), 0, s, desc, state, pts, P.max_chunks, partial);
    hipLaunchKernelGGL(k_final<1>, dim3((unsigned)n_inst), dim3(256), 0, s, desc, state, results, P.max_chunks, partial);
  }
  if (stage >= 3 && P.max_used > 0) {
    hipLaunchKernelGGL(k_rotate_gather, dim3((unsigned)((P.max_used + 255) / 256), (unsigned)n_inst), dim3(256), 0, s, desc, state, pts, clu);
    hipLaunchKernelGGL(k_activate, ig, dim3(64), 0, s, desc, state, results, n_inst);
  }
  if (stage >= 4 && P.max_used > 0) {
    DbArgs a = db_args(ws, P.db);
    a.desc = desc; a.state = state; a.pts = clu; a.labels = labels;
    const dim3 pg((unsigned)((P.max_used + 255) / 256), (unsigned)n_inst);
    double eps = p.eps0;
    for (int t = 1; t <= p.trials && 3 + t <= stage; ++t) {
      db_launch(a, n_inst, P.max_used, eps, p.min_samples, s);
      hipLaunchKernelGGL(k_db_keep, pg, dim3(256), 0, s, a, p.min_cluster_frac, p.min_cluster);
      hipLaunchKernelGGL(k_db_decide, dim3((unsigned)n_inst), dim3(1024), 0, s, a, results, t, t == p.trials ? 1 : 0, eps, p.accept_frac);
      eps = 2 * eps;
    }
  }
  return hipGetLastError() == hipSuccess ? OVM_OK : fail(OVM_ERR_HIP, "geo: kernel launch failed");
}

int ovm_geo_dbscan_workspace(int32_t n, int64_t* bytes) {
  if (n < 0 || !bytes) return fail(OVM_ERR_INVALID, "geo: dbscan workspace needs n >= 0 and a bytes pointer");
  *bytes = db_layout(512, n).total;
  return OVM_OK;
}

int ovm_geo_dbscan(const double* points, int32_t n, double eps, int32_t min_samples, int32_t* labels, void* workspace,
                   int64_t workspace_bytes, ovm_stream_t stream) {
  if (n < 0 || !std::isfinite(eps) || eps <= 0.0 || min_samples < 1) return fail(OVM_ERR_INVALID, "geo: dbscan needs n >= 0, eps > 0, min_samples >= 1");
  if (n == 0) return OVM_OK;
  if (!points || !labels || !workspace) return fail(OVM_ERR_INVALID, "geo: dbscan got a null pointer");
  const DbLayout L = db_layout(512, n);
  if (workspace_bytes < L.total) return fail(OVM_ERR_CAPACITY, "geo: dbscan workspace too small");
  static_assert(sizeof(GeoDesc) <= 256 && sizeof(GeoState) <= 256, "the single-instance header fits 512 bytes");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  GeoDesc* desc = (GeoDesc*)ws;
  GeoState* state = (GeoState*)(ws + 256);
  hipLaunchKernelGGL(k_db_single, dim3(1), dim3(1), 0, s, desc, state, n);
  DbArgs a = db_args(ws, L);
  a.desc = desc; a.state = state; a.pts = points; a.labels = labels;
  db_launch(a, 1, n, eps, min_samples, s);
  return hipGetLastError() == hipSuccess ? OVM_OK : fail(OVM_ERR_HIP, "geo: kernel launch failed");
}

int ovm_host_geo_box(const OvmGeoResult* r, const double* K, OvmGeoBox* box) { return ovm_host_geo_box_frame(r, K, nullptr, box); }

int ovm_host_geo_box_frame(const OvmGeoResult* r, const double* K, const double* frame, OvmGeoBox* box) {
  if (!r || !K || !box) return fail(OVM_ERR_INVALID, "geo: null argument");
  if (r->status != OVM_GEO_OK) return fail(OVM_ERR_INVALID, "geo: the instance was not lifted (status != OVM_GEO_OK)");
  // gen_8corners with the reference's swapped names: y_min = max y, z_min = max z, so dy and dz are negative
  const double x_min = r->ext_min[0], y_min = r->ext_max[1], z_min = r->ext_max[2];
  const double dx = r->ext_max[0] - x_min, dy = r->ext_min[1] - y_min, dz = r->ext_min[2] - z_min;
  static const int flag[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
  const double c = std::cos(r->yaw), s = std::sin(r->yaw);
  double v[8][3];
  for (int k = 0; k < 8; ++k) {
    const double px = (x_min + flag[k][0] * dx) - r->offset[0];
    const double py = (y_min + flag[k][1] * dy) - r->offset[1];
    const double pz = (z_min + flag[k][2] * dz) - r->offset[2];
    // Ry(yaw) about the offset, then (x, -y, -z)
    v[k][0] = (c * px + -s * pz) + r->offset[0];
    v[k][1] = -(py + r->offset[1]);
    v[k][2] = -((s * px + c * pz) + r->offset[2]);
  }
  for (int a = 0; a < 3; ++a) {
    double sum = v[0][a];
    for (int k = 1; k < 8; ++k) sum += v[k][a];
    box->center_cam[a] = sum / 8.0;
  }
  auto dist = [&](int i, int j) {
    double q = 0.0;
    for (int a = 0; a < 3; ++a) q += (v[i][a] - v[j][a]) * (v[i][a] - v[j][a]);
    return std::sqrt(q);
  };
  box->dimensions[0] = dist(0, 4);
  box->dimensions[1] = dist(0, 3);
  box->dimensions[2] = dist(0, 1);
  double R[9] = {c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c};
  if (frame) {
    // back into the camera's frame: V = F U^T F, F = diag(1, -1, -1), so V[i][j] = f_i f_j U[j][i]
    static const double f[3] = {1.0, -1.0, -1.0};
    double V[9], cc[3], P[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) V[3 * i + j] = f[i] * f[j] * frame[3 * j + i];
    for (int i = 0; i < 3; ++i) {
      cc[i] = (V[3 * i] * box->center_cam[0] + V[3 * i + 1] * box->center_cam[1]) + V[3 * i + 2] * box->center_cam[2];
      for (int j = 0; j < 3; ++j) P[3 * i + j] = (V[3 * i] * R[j] + V[3 * i + 1] * R[3 + j]) + V[3 * i + 2] * R[6 + j];
    }
    std::memcpy(box->center_cam, cc, sizeof(cc));
    std::memcpy(R, P, sizeof(P));
  }
  std::memcpy(box->pose, R, sizeof(R));
  box->depth = box->center_cam[2];
  box->center_2D[0] = (K[0] * box->center_cam[0]) / box->center_cam[2] + K[2];
  box->center_2D[1] = (K[4] * box->center_cam[1]) / box->center_cam[2] + K[5];
  // get_cuboid_verts_faces on float32 tensors: verts = R @ (+-l/2, +-h/2, +-w/2), then + center
  const float cf[3] = {(float)box->center_cam[0], (float)box->center_cam[1], (float)box->center_cam[2]};
  const float w = (float)box->dimensions[0], h = (float)box->dimensions[1], l = (float)box->dimensions[2];
  float Rf[9];
  for (int k = 0; k < 9; ++k) Rf[k] = (float)R[k];
  static const int sx[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sy[8] = {-1, -1, 1, 1, -1, -1, 1, 1}, sz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
  for (int k = 0; k < 8; ++k) {
    const float x = sx[k] < 0 ? -l / 2 : l / 2, y = sy[k] < 0 ? -h / 2 : h / 2, z = sz[k] < 0 ? -w / 2 : w / 2;
    for (int a = 0; a < 3; ++a) {
      float t = Rf[3 * a] * x;
      t += Rf[3 * a + 1] * y;
      t += Rf[3 * a + 2] * z;
      box->bbox3D[k][a] = t + cf[a];
    }
  }
  return OVM_OK;
}

}  // extern "C"
