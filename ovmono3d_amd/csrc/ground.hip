// The ground plane of a depth map on the device, and the frame that stands boxes upright on it (steps 1 to 6 of "the ground
// plane" in include/ovm3d.h; the numpy restatement is tests/ground_oracle.py). One stream-ordered launch sequence; the number of
// points is known on the device only, so every grid is sized by the sampled pixel count and every kernel reads n itself.
//
// Everything is fp64 without fused multiply-adds. What crosses workgroups is an integer atomic (the inlier counts) or a partial
// sum over 1024 points added in a fixed tree (centroid and scatter matrix), so a run gives the same bytes every time.
//
// The hot kernel is k_count: n points against up to 4096 planes. A workgroup of 256 threads keeps 4 points per thread in
// registers (x, y, z and the point's band: 32 VGPRs) and walks a chunk of up to 1024 planes held in LDS (32 KiB; every lane reads
// the same plane: a broadcast, no bank conflict). Per plane the hits of a wave are a ballot and a popcount per point, one LDS
// atomic per wave into the workgroup's count array (4 KiB), and at the end of the chunk one global integer atomic per plane and
// workgroup. 36 KiB of LDS and under 64 VGPRs leave four workgroups (16 waves) per CU; at most 1024 workgroups stride over the
// point tiles, which bounds the global atomics at 1024 per plane.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "../../include/ovm3d.h"
#include "geo_point.hpp"
#include "scan.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = 1024;          // points per count tile and per partial sum
constexpr int kPts = kChunk / 256;    // points per thread
constexpr int kPlaneChunk = 1024;     // planes per LDS chunk
constexpr int kMaxCountBlocks = 1024;
constexpr int kSweeps = 12;           // cyclic Jacobi sweeps: a 3 x 3 symmetric matrix is diagonal to the last bit after 5 or 6

struct GroundState {                  // device only
  double plane[4];                    // the best hypothesis
  double refined[4];
  double centroid[3];
  int32_t n, best, best_count, n_valid, status, refined_count, pad[2];
};

struct GroundArgs {
  double thresh, thresh_rel, cos_tilt, min_share, max_depth;
  int32_t hyp, stride, refine;
  uint32_t seed;
};

struct Layout { int64_t state, planes, counts, flags, offs, scan, px, py, pz, partial, total; int64_t ns; int32_t hs, ws, chunks; };

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

bool params_ok(const OvmGroundParams* p) {
  return p && std::isfinite(p->thresh) && p->thresh >= 0.0 && std::isfinite(p->thresh_rel) && p->thresh_rel >= 0.0 &&
         std::isfinite(p->max_tilt_deg) && p->max_tilt_deg > 0.0 && p->max_tilt_deg < 90.0 && p->min_share >= 0.0 && p->min_share <= 1.0 &&
         std::isfinite(p->max_depth) && p->max_depth >= 0.0 && p->hypotheses >= 1 && p->hypotheses <= 4096 && p->stride >= 1 &&
         (p->refine == 0 || p->refine == 1);
}

int make_layout(int32_t H, int32_t W, const OvmGroundParams* p, Layout* L) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL) return geo_fail(OVM_ERR_INVALID, "ground: bad H / W");
  if (!params_ok(p)) return geo_fail(OVM_ERR_INVALID, "ground: invalid OvmGroundParams");
  L->hs = (H + p->stride - 1) / p->stride;
  L->ws = (W + p->stride - 1) / p->stride;
  L->ns = (int64_t)L->hs * L->ws;
  L->chunks = (int32_t)((L->ns + kChunk - 1) / kChunk);
  int64_t o = 0;
  L->state = o; o += align256(sizeof(GroundState));
  L->planes = o; o += align256((int64_t)p->hypotheses * 32);
  L->counts = o; o += align256((int64_t)p->hypotheses * 4);
  L->flags = o; o += align256(L->ns * 4);
  L->offs = o; o += align256((L->ns + 1) * 8);
  L->scan = o; o += align256(ovm_scan::scan_partial_bytes(L->ns));
  L->px = o; o += align256(L->ns * 8);
  L->py = o; o += align256(L->ns * 8);
  L->pz = o; o += align256(L->ns * 8);
  L->partial = o; o += align256((int64_t)L->chunks * 6 * 8);
  L->total = o;
  return OVM_OK;
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// step 1: which sampled pixels give a point
__global__ __launch_bounds__(256) void k_flags(const float* __restrict__ depth, int W, int ws, int64_t ns, int stride, double max_depth,
                                               uint32_t* __restrict__ flags, GroundState* state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    GroundState s;
    memset(&s, 0, sizeof(s));
    *state = s;
  }
  if (i >= ns) return;
  const int64_t y = (i / ws) * stride, x = (i % ws) * stride;
  const float z = depth[y * W + x];
  flags[i] = (isfinite(z) && z > 0.0f && (max_depth == 0.0 || (double)z <= max_depth)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_points(const float* __restrict__ depth, int W, int ws, int64_t ns, int stride, double fx, double fy, double cx,
                                                double cy, const uint32_t* __restrict__ flags, const uint64_t* __restrict__ offs,
                                                double* __restrict__ px, double* __restrict__ py, double* __restrict__ pz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns || !flags[i]) return;
  const int64_t y = (i / ws) * stride, x = (i % ws) * stride;
  double p[3];
  geo_unproject(depth[y * W + x], (int)x, (int)y, fx, fy, cx, cy, nullptr, p);
  const int64_t k = (int64_t)offs[i];                                      // < the number of flags set <= ns
  px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
}

// step 2: one thread per hypothesis; an invalid one gets a NaN plane (never within any band) and the count -1
__global__ __launch_bounds__(256) void k_hyp(GroundState* state, const uint64_t* __restrict__ total, const double* __restrict__ px,
                                             const double* __restrict__ py, const double* __restrict__ pz, GroundArgs a, double* __restrict__ planes,
                                             int32_t* __restrict__ counts) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  const int n = (int)*total;
  if (h == 0) state->n = n;
  if (h >= a.hyp) return;
  double nx = NAN, ny = NAN, nz = NAN, d = NAN;
  bool ok = false;
  if (n >= 3) {
    uint32_t idx[3];
    for (int j = 0; j < 3; ++j) idx[j] = mix32(a.seed * 0x9E3779B9u + 3u * (uint32_t)h + (uint32_t)j) % (uint32_t)n;
    if (idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2]) {
      const double x0 = px[idx[0]], y0 = py[idx[0]], z0 = pz[idx[0]];
      const double ax = px[idx[1]] - x0, ay = py[idx[1]] - y0, az = pz[idx[1]] - z0;
      const double bx = px[idx[2]] - x0, by = py[idx[2]] - y0, bz = pz[idx[2]] - z0;
      const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      const double cc = (cx * cx + cy * cy) + cz * cz, aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz;
      if (!(cc <= 1e-12 * aa * bb)) {
        const double len = sqrt(cc);
        nx = cx / len; ny = cy / len; nz = cz / len;
        if (ny < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        d = -((nx * x0 + ny * y0) + nz * z0);
        ok = !(ny < a.cos_tilt) && !(d <= 0.0) && isfinite(d);
      }
    }
  }
  if (!ok) nx = ny = nz = d = NAN;
  planes[4 * h] = nx; planes[4 * h + 1] = ny; planes[4 * h + 2] = nz; planes[4 * h + 3] = d;
  counts[h] = ok ? 0 : -1;
}

__device__ __forceinline__ bool in_band(double nx, double ny, double nz, double d, double x, double y, double z, double tol) {
  return fabs(((nx * x + ny * y) + nz * z) + d) <= tol;
}

// step 3 (and step 5's recount, with one plane): counts[h] += the points within plane h's band. status: when given and not OK,
// nothing is counted.
__global__ __launch_bounds__(256) void k_count(const uint64_t* __restrict__ total, const double* __restrict__ px, const double* __restrict__ py,
                                               const double* __restrict__ pz, const double* __restrict__ planes, int np, int32_t* counts,
                                               double thresh, double thresh_rel, const int32_t* status) {
  if (status && *status != OVM_GROUND_OK) return;
  const int64_t n = (int64_t)*total;
  if ((int64_t)blockIdx.x * kChunk >= n) return;                             // uniform over the workgroup
  __shared__ __attribute__((aligned(16))) double sp[kPlaneChunk][4];
  __shared__ int scount[kPlaneChunk];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int h0 = 0; h0 < np; h0 += kPlaneChunk) {
    const int nh = min(kPlaneChunk, np - h0);
    __syncthreads();
    for (int k = tid; k < nh; k += 256) {
      for (int c = 0; c < 4; ++c) sp[k][c] = planes[4 * (int64_t)(h0 + k) + c];
      scount[k] = 0;
    }
    __syncthreads();
    for (int64_t t0 = (int64_t)blockIdx.x * kChunk; t0 < n; t0 += (int64_t)gridDim.x * kChunk) {
      double x[kPts], y[kPts], z[kPts], tol[kPts];
#pragma unroll
      for (int r = 0; r < kPts; ++r) {
        const int64_t i = t0 + r * 256 + tid;
        x[r] = y[r] = z[r] = 0.0;
        tol[r] = -1.0;                                                       // past the end: inside no band
        if (i < n) {
          x[r] = px[i]; y[r] = py[i]; z[r] = pz[i];
          tol[r] = thresh + thresh_rel * fabs(z[r]);
        }
      }
      for (int k = 0; k < nh; ++k) {
        const double nx = sp[k][0], ny = sp[k][1], nz = sp[k][2], d = sp[k][3];
        int c = 0;
#pragma unroll
        for (int r = 0; r < kPts; ++r) c += __popcll(__ballot(in_band(nx, ny, nz, d, x[r], y[r], z[r], tol[r])));
        if (lane == 0 && c) atomicAdd(&scount[k], c);
      }
    }
    __syncthreads();
    for (int k = tid; k < nh; k += 256)
      if (scount[k]) atomicAdd(&counts[h0 + k], scount[k]);
  }
}

// step 4
__global__ __launch_bounds__(256) void k_best(GroundState* state, const double* __restrict__ planes, const int32_t* __restrict__ counts, GroundArgs a) {
  __shared__ int sc[256], sh[256], sv[256];
  int bc = -1, bh = 0x7fffffff, valid = 0;
  for (int h = threadIdx.x; h < a.hyp; h += 256) {
    const int c = counts[h];
    if (c >= 0) {
      ++valid;
      if (c > bc) { bc = c; bh = h; }                                        // ascending h: the first of equal counts stays
    }
  }
  sc[threadIdx.x] = bc; sh[threadIdx.x] = bh; sv[threadIdx.x] = valid;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      const int oc = sc[threadIdx.x + off], oh = sh[threadIdx.x + off];
      if (oc > sc[threadIdx.x] || (oc == sc[threadIdx.x] && oh < sh[threadIdx.x])) { sc[threadIdx.x] = oc; sh[threadIdx.x] = oh; }
      sv[threadIdx.x] += sv[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const int n = state->n;
  state->n_valid = sv[0];
  state->best = sv[0] > 0 ? sh[0] : -1;
  state->best_count = sv[0] > 0 ? sc[0] : 0;
  if (sv[0] > 0)
    for (int k = 0; k < 4; ++k) state->plane[k] = planes[4 * sh[0] + k];
  int status = OVM_GROUND_OK;
  if (n < 3) status = OVM_GROUND_TOO_FEW;
  else if (sv[0] == 0 || (double)sc[0] < a.min_share * (double)n) status = OVM_GROUND_NO_PLANE;
  state->status = status;
}

// step 5: partial sums over 1024 points of the best hypothesis' inliers. MODE 0: x, y, z; MODE 1: the centred products xx, xy, xz,
// yy, yz, zz.
template <int MODE>
__global__ __launch_bounds__(256) void k_partial(const GroundState* __restrict__ state, const double* __restrict__ px, const double* __restrict__ py,
                                                 const double* __restrict__ pz, double thresh, double thresh_rel, double* __restrict__ partial) {
  if (state->status != OVM_GROUND_OK) return;
  const int64_t n = state->n, c = blockIdx.x;
  if (c * kChunk >= n) return;
  constexpr int NV = MODE == 0 ? 3 : 6;
  __shared__ double red[NV][256];
  const double nx = state->plane[0], ny = state->plane[1], nz = state->plane[2], d = state->plane[3];
  const double mx = state->centroid[0], my = state->centroid[1], mz = state->centroid[2];
  double acc[NV];
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  for (int r = 0; r < kPts; ++r) {
    const int64_t i = c * kChunk + r * 256 + threadIdx.x;
    if (i >= n) continue;
    const double x = px[i], y = py[i], z = pz[i];
    if (!in_band(nx, ny, nz, d, x, y, z, thresh + thresh_rel * fabs(z))) continue;
    if constexpr (MODE == 0) {
      acc[0] += x; acc[1] += y; acc[2] += z;
    } else {
      const double ux = x - mx, uy = y - my, uz = z - mz;
      acc[0] += ux * ux; acc[1] += ux * uy; acc[2] += ux * uz; acc[3] += uy * uy; acc[4] += uy * uz; acc[5] += uz * uz;
    }
  }
  for (int k = 0; k < NV; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < NV; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < NV) partial[c * 6 + threadIdx.x] = red[threadIdx.x][0];
}

// eigenvector of the smallest eigenvalue of the symmetric matrix [[m0, m1, m2], [m1, m3, m4], [m2, m4, m5]]: cyclic Jacobi
__device__ void smallest_eigenvector(const double* m, double* v) {
  double A[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      for (int k = 0; k < 3; ++k) {                                          // A <- A J
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; ++k) {                                          // A <- J^T A
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
      }
      for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
      }
    }
  }
  int k = 0;
  if (A[1][1] < A[k][k]) k = 1;
  if (A[2][2] < A[k][k]) k = 2;
  const double len = sqrt((V[0][k] * V[0][k] + V[1][k] * V[1][k]) + V[2][k] * V[2][k]);
  for (int r = 0; r < 3; ++r) v[r] = V[r][k] / len;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_final(GroundState* state, const double* __restrict__ partial) {
  if (state->status != OVM_GROUND_OK) return;
  constexpr int NV = MODE == 0 ? 3 : 6;
  const int nch = (state->n + kChunk - 1) / kChunk;
  __shared__ double red[NV][256];
  double acc[NV];
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  for (int c = threadIdx.x; c < nch; c += 256)
    for (int k = 0; k < NV; ++k) acc[k] += partial[(int64_t)c * 6 + k];
  for (int k = 0; k < NV; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < NV; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if constexpr (MODE == 0) {
    for (int k = 0; k < 3; ++k) state->centroid[k] = red[k][0] / (double)state->best_count;
  } else {
    double m[6], v[3];
    for (int k = 0; k < 6; ++k) m[k] = red[k][0];
    smallest_eigenvector(m, v);
    if (v[1] < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    for (int k = 0; k < 3; ++k) state->refined[k] = v[k];
    state->refined[3] = -((v[0] * state->centroid[0] + v[1] * state->centroid[1]) + v[2] * state->centroid[2]);
  }
}

// the plane kept, step 6 and the whole result
__global__ void k_finish(const GroundState* __restrict__ state, GroundArgs a, OvmGroundResult* result) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const GroundState s = *state;
  OvmGroundResult r;
  memset(&r, 0, sizeof(r));
  r.n_points = s.n;
  r.n_valid_hyp = s.n_valid;
  r.best_hyp = s.best;
  r.hyp_inliers = s.best_count;
  r.status = s.status;
  if (s.best >= 0) {
    for (int k = 0; k < 3; ++k) r.hyp_normal[k] = s.plane[k];
    r.hyp_offset = s.plane[3];
  }
  r.frame[0] = r.frame[4] = r.frame[8] = 1.0;
  if (s.status == OVM_GROUND_OK) {
    const double* pl = s.plane;
    r.n_inliers = s.best_count;
    if (a.refine && isfinite(s.refined[3]) && !(s.refined[1] < a.cos_tilt) && !(s.refined[3] <= 0.0) && s.refined_count >= s.best_count) {
      pl = s.refined;
      r.n_inliers = s.refined_count;
    }
    for (int k = 0; k < 3; ++k) r.normal[k] = pl[k];
    r.offset = pl[3];
    // U = I + [a]x + [a]x^2 / (1 + n_y), a = n x e_y = (-n_z, 0, n_x)
    const double ax = -pl[2], ay = 0.0, az = pl[0];
    const double X[3][3] = {{0.0, -az, ay}, {az, 0.0, -ax}, {-ay, ax, 0.0}};
    const double f = 1.0 / (1.0 + pl[1]);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double x2 = (X[i][0] * X[0][j] + X[i][1] * X[1][j]) + X[i][2] * X[2][j];
        r.frame[3 * i + j] = ((i == j ? 1.0 : 0.0) + X[i][j]) + x2 * f;
      }
  }
  *result = r;
}

}  // namespace

extern "C" {

int ovm_geo_ground_default_params(OvmGroundParams* p) {
  if (!p) return geo_fail(OVM_ERR_INVALID, "ground: null params");
  std::memset(p, 0, sizeof(*p));
  p->thresh = 0.02; p->thresh_rel = 0.01; p->max_tilt_deg = 45.0; p->min_share = 0.10; p->max_depth = 0.0;
  p->hypotheses = 512; p->stride = 4; p->seed = 0; p->refine = 1;
  return OVM_OK;
}

int ovm_geo_ground_workspace(int32_t H, int32_t W, const OvmGroundParams* params, int64_t* bytes) {
  if (!bytes) return geo_fail(OVM_ERR_INVALID, "ground: null bytes");
  Layout L;
  const int rc = make_layout(H, W, params, &L);
  if (rc != OVM_OK) return rc;
  *bytes = L.total;
  return OVM_OK;
}

int ovm_geo_ground_plane(const float* depth, int32_t H, int32_t W, const double* K, const OvmGroundParams* params, OvmGroundResult* result,
                         int32_t* hyp_counts, void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  if (!depth || !K || !result || !workspace) return geo_fail(OVM_ERR_INVALID, "ground: null depth / K / result / workspace");
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.0 || fy == 0.0)
    return geo_fail(OVM_ERR_INVALID, "ground: K needs finite, nonzero focal lengths and a finite principal point");
  Layout L;
  const int rc = make_layout(H, W, params, &L);
  if (rc != OVM_OK) return rc;
  if (workspace_bytes < L.total) return geo_fail(OVM_ERR_CAPACITY, "ground: workspace too small (ask ovm_geo_ground_workspace)");

  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  GroundState* state = (GroundState*)(ws + L.state);
  double* planes = (double*)(ws + L.planes);
  int32_t* counts = hyp_counts ? hyp_counts : (int32_t*)(ws + L.counts);
  uint32_t* flags = (uint32_t*)(ws + L.flags);
  uint64_t* offs = (uint64_t*)(ws + L.offs);
  const uint64_t* total = offs + L.ns;
  double *px = (double*)(ws + L.px), *py = (double*)(ws + L.py), *pz = (double*)(ws + L.pz), *partial = (double*)(ws + L.partial);
  GroundArgs a{};
  a.thresh = params->thresh; a.thresh_rel = params->thresh_rel; a.cos_tilt = std::cos(params->max_tilt_deg * 3.14159265358979323846 / 180.0);
  a.min_share = params->min_share; a.max_depth = params->max_depth;
  a.hyp = params->hypotheses; a.stride = params->stride; a.refine = params->refine; a.seed = params->seed;

  const dim3 pg((unsigned)((L.ns + 255) / 256)), cg((unsigned)std::min(L.chunks, kMaxCountBlocks)), rg((unsigned)L.chunks);
  hipLaunchKernelGGL(k_flags, pg, dim3(256), 0, s, depth, W, L.ws, L.ns, a.stride, a.max_depth, flags, state);
  ovm_scan::launch_scan(flags, L.ns, (uint64_t*)(ws + L.scan), offs, s);
  hipLaunchKernelGGL(k_points, pg, dim3(256), 0, s, depth, W, L.ws, L.ns, a.stride, fx, fy, cx, cy, flags, offs, px, py, pz);
  hipLaunchKernelGGL(k_hyp, dim3((unsigned)((a.hyp + 255) / 256)), dim3(256), 0, s, state, total, px, py, pz, a, planes, counts);
  hipLaunchKernelGGL(k_count, cg, dim3(256), 0, s, total, px, py, pz, planes, a.hyp, counts, a.thresh, a.thresh_rel, (const int32_t*)nullptr);
  hipLaunchKernelGGL(k_best, dim3(1), dim3(256), 0, s, state, planes, counts, a);
  if (a.refine) {
    hipLaunchKernelGGL(k_partial<0>, rg, dim3(256), 0, s, state, px, py, pz, a.thresh, a.thresh_rel, partial);
    hipLaunchKernelGGL(k_final<0>, dim3(1), dim3(256), 0, s, state, partial);
    hipLaunchKernelGGL(k_partial<1>, rg, dim3(256), 0, s, state, px, py, pz, a.thresh, a.thresh_rel, partial);
    hipLaunchKernelGGL(k_final<1>, dim3(1), dim3(256), 0, s, state, partial);
    hipLaunchKernelGGL(k_count, cg, dim3(256), 0, s, total, px, py, pz, state->refined, 1, &state->refined_count, a.thresh, a.thresh_rel,
                       (const int32_t*)&state->status);
  }
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, state, a, result);
  return hipGetLastError() == hipSuccess ? OVM_OK : geo_fail(OVM_ERR_HIP, "ground: kernel launch failed");
}

}  // extern "C"
