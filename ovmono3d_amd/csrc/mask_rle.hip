// COCO run-length encoding of binary masks on the device (ovm_mask_rle_encode / ovm_mask_rle_decode; the rules, restated from
// pycocotools' maskApi.c, are in include/ovm3d.h, "Mask run-length encoding").
//
// A plane is scanned column-major (p = x * H + y) but read in its own row-major order: a workgroup is 4 waves, wave w owns band
// 4 * block + w (kBand rows), lane l column 64 * block + l, so every row of a band is one coalesced wave load. The value in front of
// pixel (y, x) is (y - 1, x), or (H - 1, x - 1) when y = 0, so a lane needs no neighbour's data.
// Encode, all on the caller's stream, nothing read back:
//   1 rle_count_kernel    value changes per segment = (plane, column, band), stored in column-major order, planes outermost
//     scan.hpp            exclusive prefix sum over all segments: the rank of a segment's first change among all planes' changes
//   2 rle_offsets_kernel  run_offsets[i] = rank of plane i's first segment + i (a plane with T changes has T + 1 counts)
//   3 rle_positions_kernel the walk of 1 again: position p of each change at its rank; H * W behind the last change of a plane
//   4 rle_counts_kernel   one lane per count: count = difference of neighbouring positions; its string length from cnts[i], cnts[i-2]
//     scan.hpp            64-bit offsets of the strings
//   5 rle_string_kernel   one lane per count: its bytes at its offset
//   6 rle_finish_kernel   str_offsets, status
// 3 to 5 do nothing when the runs do not fit max_runs, 5 nothing when the bytes do not fit max_bytes; 1, 2 and 6 always run.
// Only when the runs do not fit (else they return at once), so that the byte total is exact all the same:
//   rle_last3_kernel          the walk again: every segment's last three change positions
//   rle_overflow_bytes_kernel the walk again: each count's string length from its own changes and the three in front of the
//                             segment (found by bisection over the ranks), summed per plane with integer atomics
// Decode: scan.hpp over the counts, rle_check_kernel (sums against H * W, offsets in range -> status), rle_fill_kernel (each
// (column, band) finds the run of its first pixel by bisection over the scanned counts and walks on).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/ovm3d.h"
#include "scan.hpp"

namespace {

using ovm_scan::launch_scan;
using ovm_scan::scan_partial_bytes;

constexpr int kBand = 64;            // rows per band
constexpr int kWgCols = 64, kWgBands = 4;
constexpr int64_t kMaxWorkgroups = (1 << 24) - 1;      // 256 lanes each: a launch stays below 2^32 lanes

struct Geom {
  int n, H, W, NB, cb, bb;           // NB bands per column; cb, bb: workgroups per plane along x and along the bands
  int64_t plane_stride, pitch;
};

// workgroup -> (plane, column, band); false for the lanes beyond the plane
__device__ __forceinline__ bool segment_of(const Geom& G, int* plane, int* x, int* band) {
  const unsigned per_plane = (unsigned)G.cb * (unsigned)G.bb;
  *plane = (int)(blockIdx.x / per_plane);
  const unsigned r = blockIdx.x % per_plane;
  *x = (int)(r % (unsigned)G.cb) * kWgCols + (int)(threadIdx.x & 63);
  *band = (int)(r / (unsigned)G.cb) * kWgBands + (int)(threadIdx.x >> 6);
  return *x < G.W && *band < G.NB;
}

// the value in front of pixel (y0, x) in column-major order; 0 in front of the first pixel
__device__ __forceinline__ unsigned value_before(const uint8_t* __restrict__ P, const Geom& G, int y0, int x) {
  if (y0 > 0) return P[(int64_t)(y0 - 1) * G.pitch + x] != 0;
  if (x > 0) return P[(int64_t)(G.H - 1) * G.pitch + (x - 1)] != 0;
  return 0u;
}

// the walk of one segment: on_change(p) for every pixel of (column x, rows y0 .. y1) whose value differs from the one in front
template <class F>
__device__ __forceinline__ void walk_segment(const uint8_t* __restrict__ P, const Geom& G, int band, int x, F&& on_change) {
  const int y0 = band * kBand, y1 = min(y0 + kBand, G.H);
  unsigned prev = value_before(P, G, y0, x);
  const uint32_t p0 = (uint32_t)x * (uint32_t)G.H;
  for (int y = y0; y < y1; ++y) {
    const unsigned v = P[(int64_t)y * G.pitch + x] != 0;
    if (v != prev) on_change(p0 + (uint32_t)y);
    prev = v;
  }
}

__global__ __launch_bounds__(256) void rle_count_kernel(const uint8_t* __restrict__ masks, Geom G, uint32_t* __restrict__ seg) {
  int i, x, band;
  if (!segment_of(G, &i, &x, &band)) return;
  unsigned c = 0;
  walk_segment(masks + (int64_t)i * G.plane_stride, G, band, x, [&](uint32_t) { ++c; });
  seg[((int64_t)i * G.W + x) * G.NB + band] = c;
}

// also zeroes the per-plane byte sums the overflow path adds into
__global__ void rle_offsets_kernel(const uint64_t* __restrict__ rank, Geom G, int64_t* __restrict__ run_offsets, unsigned long long* __restrict__ plane_bytes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= G.n) run_offsets[i] = (int64_t)rank[(int64_t)i * G.W * G.NB] + i;
  if (i < G.n) plane_bytes[i] = 0ull;
}

__global__ __launch_bounds__(256) void rle_positions_kernel(const uint8_t* __restrict__ masks, Geom G, const uint64_t* __restrict__ rank,
                                                            int64_t nseg, int64_t max_runs, uint32_t* __restrict__ tpos) {
  int i, x, band;
  if (!segment_of(G, &i, &x, &band)) return;
  if ((int64_t)rank[nseg] + G.n > max_runs) return;
  int64_t r = (int64_t)rank[((int64_t)i * G.W + x) * G.NB + band] + i;
  walk_segment(masks + (int64_t)i * G.plane_stride, G, band, x, [&](uint32_t p) { tpos[r++] = p; });
  if (x == G.W - 1 && band == G.NB - 1) tpos[r] = (uint32_t)G.H * (uint32_t)G.W;      // the end of the plane's last run
}

// the string of one difference: its length; the bytes too when out is not null
__device__ __forceinline__ int rle_chars(int64_t x, uint8_t* out) {
  int m = 0;
  bool more;
  do {
    int c = (int)(x & 0x1f);
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (out) out[m] = (uint8_t)(c + 48);
    ++m;
  } while (more);
  return m;
}

// ---- the runs do not fit max_runs: the exact string length without the positions stored --------------------------------------
// The string of count k needs the positions of changes k, k - 1, k - 2 and k - 3. A segment's walk has its own changes; the three
// in front of it are each among the last three changes of the segment that holds them, so pass A leaves every segment's last
// three positions and pass B finds the holder of change q by bisection over the ranks (first segment with rank > q, minus one).
__global__ __launch_bounds__(256) void rle_last3_kernel(const uint8_t* __restrict__ masks, Geom G, const uint64_t* __restrict__ rank, int64_t nseg,
                                                        int64_t max_runs, uint32_t* __restrict__ last3) {
  int i, x, band;
  if (!segment_of(G, &i, &x, &band)) return;
  if ((int64_t)rank[nseg] + G.n <= max_runs) return;
  uint32_t t1 = 0, t2 = 0, t3 = 0;                     // most recent first
  walk_segment(masks + (int64_t)i * G.plane_stride, G, band, x, [&](uint32_t p) { t3 = t2; t2 = t1; t1 = p; });
  uint32_t* o = last3 + 3 * (((int64_t)i * G.W + x) * G.NB + band);
  o[0] = t1; o[1] = t2; o[2] = t3;
}

// position of change q (global rank) of the plane whose segments are [s0, s1), q in front of segment s1
__device__ __forceinline__ uint32_t change_position(const uint64_t* __restrict__ rank, const uint32_t* __restrict__ last3, int64_t s0, int64_t s1,
                                                    uint64_t q) {
  int64_t a = s0, b = s1;                              // the first segment index in (s0, s1] with rank > q
  while (a < b) {
    const int64_t mid = (a + b + 1) >> 1;
    if (rank[mid] > q) b = mid - 1; else a = mid;
  }
  // a: the last index with rank[a] <= q, so segment a holds change q; it is change rank[a + 1] - 1 - q from the segment's end
  return last3[3 * a + (int64_t)(rank[a + 1] - 1 - q)];
}

__global__ __launch_bounds__(256) void rle_overflow_bytes_kernel(const uint8_t* __restrict__ masks, Geom G, const uint64_t* __restrict__ rank,
                                                                 int64_t nseg, int64_t max_runs, const uint32_t* __restrict__ last3,
                                                                 unsigned long long* __restrict__ plane_bytes) {
  int i, x, band;
  if (!segment_of(G, &i, &x, &band)) return;
  if ((int64_t)rank[nseg] + G.n <= max_runs) return;
  const int64_t s0 = (int64_t)i * G.W * G.NB, s = ((int64_t)i * G.W + x) * G.NB + band;
  const uint64_t base = rank[s0], first = rank[s];
  int64_t k = (int64_t)(first - base);                 // the plane's count index of this segment's first change
  uint32_t t1 = 0, t2 = 0, t3 = 0;                     // positions of changes k - 1, k - 2, k - 3 (unused where they do not exist)
  if (k > 0) t1 = change_position(rank, last3, s0, s, first - 1);
  if (k > 1) t2 = change_position(rank, last3, s0, s, first - 2);
  if (k > 2) t3 = change_position(rank, last3, s0, s, first - 3);
  unsigned long long bytes = 0;
  auto count_ends_at = [&](uint32_t p) {
    int64_t d = (int64_t)(p - (k > 0 ? t1 : 0u));
    if (k > 2) d -= (int64_t)(t2 - t3);
    bytes += (unsigned)rle_chars(d, nullptr);
    t3 = t2; t2 = t1; t1 = p; ++k;
  };
  walk_segment(masks + (int64_t)i * G.plane_stride, G, band, x, count_ends_at);
  if (x == G.W - 1 && band == G.NB - 1) count_ends_at((uint32_t)G.H * (uint32_t)G.W);
  if (bytes) atomicAdd(&plane_bytes[i], bytes);
}

// count j (global index, plane found by bisection over run_offsets) and the difference its string encodes
__device__ __forceinline__ uint32_t count_of(const uint32_t* __restrict__ tpos, const int64_t* __restrict__ ro, int n, int64_t j, int64_t* delta) {
  int lo = 0, hi = n;                                  // the last plane with ro[plane] <= j
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ro[mid] <= j) lo = mid; else hi = mid;
  }
  const int64_t k = j - ro[lo];
  const uint32_t c = tpos[j] - (k > 0 ? tpos[j - 1] : 0u);
  int64_t d = (int64_t)c;
  if (k > 2) d -= (int64_t)(tpos[j - 2] - tpos[j - 3]);
  *delta = d;
  return c;
}

__global__ __launch_bounds__(256) void rle_counts_kernel(const uint32_t* __restrict__ tpos, const int64_t* __restrict__ ro, int n, int64_t max_runs,
                                                         uint32_t* __restrict__ counts_out, uint32_t* __restrict__ len) {
  const int64_t R = ro[n];
  const bool fits = R <= max_runs;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < max_runs; j += (int64_t)gridDim.x * blockDim.x) {
    uint32_t l = 0;
    if (fits && j < R) {
      int64_t d;
      const uint32_t c = count_of(tpos, ro, n, j, &d);
      if (counts_out) counts_out[j] = c;
      l = (uint32_t)rle_chars(d, nullptr);
    }
    if (len) len[j] = l;
  }
}

__global__ __launch_bounds__(256) void rle_string_kernel(const uint32_t* __restrict__ tpos, const int64_t* __restrict__ ro, int n, int64_t max_runs,
                                                         const uint64_t* __restrict__ soff, int64_t max_bytes, uint8_t* __restrict__ string_out) {
  const int64_t R = ro[n];
  if (R > max_runs || (int64_t)soff[max_runs] > max_bytes) return;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t d;
    count_of(tpos, ro, n, j, &d);
    rle_chars(d, string_out + soff[j]);
  }
}

__device__ __forceinline__ int32_t saturate_i32(int64_t v) { return v > 0x7fffffffLL ? 0x7fffffff : (int32_t)v; }

// soff null: no strings were asked for. When the runs do not fit, the byte sums are the overflow path's, per plane.
__global__ void rle_finish_kernel(const int64_t* __restrict__ ro, int n, int64_t max_runs, const uint64_t* __restrict__ soff, int64_t max_bytes,
                                  const unsigned long long* __restrict__ plane_bytes, int64_t* __restrict__ str_offsets, int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const int64_t R = ro[n];
  const bool fits = R <= max_runs;
  int64_t off = 0;                                     // the first string byte of plane i; for i = n the total
  if (soff) {
    if (fits) off = (int64_t)soff[i < n ? ro[i] : max_runs];
    else for (int j = 0; j < i; ++j) off += (int64_t)plane_bytes[j];
    str_offsets[i] = off;
  }
  if (i == n) {
    status[0] = fits && (!soff || off <= max_bytes) ? OVM_OK : OVM_ERR_CAPACITY;
    status[1] = saturate_i32(R);
    status[2] = saturate_i32(off);
    status[3] = 0;
  }
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void plane_runs(const int64_t* __restrict__ ro, int i, int64_t total_runs, int64_t* lo, int64_t* hi, bool* in_range) {
  const int64_t a = ro[i], b = ro[i + 1];
  *in_range = a >= 0 && a <= b && b <= total_runs;
  *lo = a < 0 ? 0 : a > total_runs ? total_runs : a;
  *hi = b < *lo ? *lo : b > total_runs ? total_runs : b;
}

__global__ __launch_bounds__(256) void rle_check_kernel(const uint64_t* __restrict__ cum, const int64_t* __restrict__ ro, int64_t total_runs, int n,
                                                        uint64_t hw, int32_t* __restrict__ status) {
  __shared__ int bad, first;
  if (threadIdx.x == 0) { bad = 0; first = 0x7fffffff; }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int64_t lo, hi;
    bool ok;
    plane_runs(ro, i, total_runs, &lo, &hi, &ok);
    if (!ok || cum[hi] - cum[lo] != hw) { atomicAdd(&bad, 1); atomicMin(&first, i); }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    status[0] = bad ? OVM_ERR_INVALID : OVM_OK;
    status[1] = bad;
    status[2] = bad ? first : -1;
    status[3] = 0;
  }
}

__global__ __launch_bounds__(256) void rle_fill_kernel(const uint64_t* __restrict__ cum, const int64_t* __restrict__ ro, int64_t total_runs, Geom G,
                                                       uint8_t* __restrict__ masks_out) {
  int i, x, band;
  if (!segment_of(G, &i, &x, &band)) return;
  int64_t lo, hi;
  bool ok;
  plane_runs(ro, i, total_runs, &lo, &hi, &ok);
  const uint64_t* E = cum + lo + 1;                    // E[k] - base: the position behind run k
  const uint64_t base = cum[lo];
  const int64_t nruns = hi - lo;
  const int y0 = band * kBand, y1 = min(y0 + kBand, G.H);
  uint64_t p = (uint64_t)x * (uint64_t)G.H + (uint64_t)y0;
  int64_t a = 0, b = nruns;                            // the first run k with E[k] - base > p
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (E[mid] - base <= p) a = mid + 1; else b = mid;
  }
  int64_t k = a;
  uint64_t end = k < nruns ? E[k] - base : ~0ull;
  uint8_t* P = masks_out + (int64_t)i * G.plane_stride;
  for (int y = y0; y < y1; ++y, ++p) {
    while (p >= end) {
      ++k;
      end = k < nruns ? E[k] - base : ~0ull;
    }
    P[(int64_t)y * G.pitch + x] = k < nruns ? (uint8_t)(k & 1) : (uint8_t)0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// false: arguments no call takes
bool make_geom(int32_t n, int32_t H, int32_t W, int64_t plane_stride, int64_t pitch, Geom* G) {
  if (n < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL || pitch < W) return false;
  G->n = n; G->H = H; G->W = W;
  G->NB = (H + kBand - 1) / kBand;
  G->cb = (W + kWgCols - 1) / kWgCols;
  G->bb = (G->NB + kWgBands - 1) / kWgBands;
  G->plane_stride = plane_stride; G->pitch = pitch;
  return true;
}

int64_t workgroups(const Geom& G) { return (int64_t)G.n * G.cb * G.bb; }
int64_t segments(const Geom& G) { return (int64_t)G.n * G.W * G.NB; }

struct EncodeLayout { int64_t seg, rank, partial, tpos, len, soff, last3, plane_bytes, total; };

EncodeLayout encode_layout(const Geom& G, int64_t max_runs) {
  EncodeLayout L;
  const int64_t nseg = segments(G);
  int64_t o = 0;
  L.seg = o; o += align16(nseg * 4);
  L.rank = o; o += align16((nseg + 1) * 8);
  L.partial = o; o += align16(scan_partial_bytes(nseg > max_runs ? nseg : max_runs));
  L.tpos = o; o += align16(max_runs * 4);
  L.len = o; o += align16(max_runs * 4);
  L.soff = o; o += align16((max_runs + 1) * 8);
  L.last3 = o; o += align16(nseg * 12);
  L.plane_bytes = o; o += align16((int64_t)G.n * 8);
  L.total = o;
  return L;
}

struct DecodeLayout { int64_t cum, partial, total; };

DecodeLayout decode_layout(int64_t total_runs) {
  DecodeLayout L;
  int64_t o = 0;
  L.cum = o; o += align16((total_runs + 1) * 8);
  L.partial = o; o += align16(scan_partial_bytes(total_runs));
  L.total = o;
  return L;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned stride_grid(int64_t items) {
  const int64_t g = (items + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

}  // namespace

extern "C" {

int ovm_mask_rle_encode_workspace(int32_t n, int32_t H, int32_t W, int64_t max_runs, int64_t max_bytes, int64_t* bytes) {
  Geom G;
  if (!bytes || !make_geom(n, H, W, 0, W, &G) || max_runs < 1 || max_bytes < 0) return OVM_ERR_INVALID;
  if (workgroups(G) > kMaxWorkgroups) return OVM_ERR_CAPACITY;
  *bytes = encode_layout(G, max_runs).total;
  return OVM_OK;
}

int ovm_mask_rle_encode(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W,
                        uint32_t* counts_out, int64_t max_runs, int64_t* run_offsets, uint8_t* string_out, int64_t max_bytes,
                        int64_t* str_offsets, int32_t* status, void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  Geom G;
  if (!masks || !run_offsets || !status || !workspace || !make_geom(n, H, W, plane_stride, row_pitch, &G) || max_runs < 1) return OVM_ERR_INVALID;
  if ((string_out && !str_offsets) || (str_offsets && max_bytes < 1) || !aligned16(workspace)) return OVM_ERR_INVALID;
  if (workgroups(G) > kMaxWorkgroups) return OVM_ERR_CAPACITY;
  const EncodeLayout L = encode_layout(G, max_runs);
  if (workspace_bytes < L.total) return OVM_ERR_CAPACITY;
  uint8_t* ws = (uint8_t*)workspace;
  uint32_t* seg = (uint32_t*)(ws + L.seg);
  uint64_t* rank = (uint64_t*)(ws + L.rank);
  uint64_t* partial = (uint64_t*)(ws + L.partial);
  uint32_t* tpos = (uint32_t*)(ws + L.tpos);
  uint32_t* len = str_offsets ? (uint32_t*)(ws + L.len) : nullptr;
  uint64_t* soff = str_offsets ? (uint64_t*)(ws + L.soff) : nullptr;
  uint32_t* last3 = (uint32_t*)(ws + L.last3);
  unsigned long long* plane_bytes = (unsigned long long*)(ws + L.plane_bytes);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nseg = segments(G);
  const unsigned wgs = (unsigned)workgroups(G), per_plane = (unsigned)((n + 1 + 255) / 256);
  hipLaunchKernelGGL(rle_count_kernel, dim3(wgs), dim3(256), 0, s, masks, G, seg);
  launch_scan(seg, nseg, partial, rank, s);
  hipLaunchKernelGGL(rle_offsets_kernel, dim3(per_plane), dim3(256), 0, s, (const uint64_t*)rank, G, run_offsets, plane_bytes);
  hipLaunchKernelGGL(rle_positions_kernel, dim3(wgs), dim3(256), 0, s, masks, G, (const uint64_t*)rank, nseg, max_runs, tpos);
  if (counts_out || str_offsets)
    hipLaunchKernelGGL(rle_counts_kernel, dim3(stride_grid(max_runs)), dim3(256), 0, s, (const uint32_t*)tpos, (const int64_t*)run_offsets, (int)n,
                       max_runs, counts_out, len);
  if (str_offsets) {
    launch_scan(len, max_runs, partial, soff, s);
    // both return at once unless the runs do not fit
    hipLaunchKernelGGL(rle_last3_kernel, dim3(wgs), dim3(256), 0, s, masks, G, (const uint64_t*)rank, nseg, max_runs, last3);
    hipLaunchKernelGGL(rle_overflow_bytes_kernel, dim3(wgs), dim3(256), 0, s, masks, G, (const uint64_t*)rank, nseg, max_runs, (const uint32_t*)last3,
                       plane_bytes);
  }
  if (string_out)
    hipLaunchKernelGGL(rle_string_kernel, dim3(stride_grid(max_runs)), dim3(256), 0, s, (const uint32_t*)tpos, (const int64_t*)run_offsets, (int)n,
                       max_runs, (const uint64_t*)soff, max_bytes, string_out);
  hipLaunchKernelGGL(rle_finish_kernel, dim3(per_plane), dim3(256), 0, s, (const int64_t*)run_offsets, (int)n, max_runs, (const uint64_t*)soff,
                     max_bytes, (const unsigned long long*)plane_bytes, str_offsets, status);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

int ovm_mask_rle_decode_workspace(int32_t n, int32_t H, int32_t W, int64_t total_runs, int64_t* bytes) {
  Geom G;
  if (!bytes || !make_geom(n, H, W, 0, W, &G) || total_runs < 1) return OVM_ERR_INVALID;
  if (workgroups(G) > kMaxWorkgroups) return OVM_ERR_CAPACITY;
  *bytes = decode_layout(total_runs).total;
  return OVM_OK;
}

int ovm_mask_rle_decode(const uint32_t* counts, const int64_t* run_offsets, int64_t total_runs, int32_t n, int32_t H, int32_t W,
                        uint8_t* masks_out, int64_t plane_stride, int64_t row_pitch, int32_t* status, void* workspace,
                        int64_t workspace_bytes, ovm_stream_t stream) {
  Geom G;
  if (!counts || !run_offsets || !masks_out || !status || !workspace || !make_geom(n, H, W, plane_stride, row_pitch, &G) || total_runs < 1)
    return OVM_ERR_INVALID;
  if (!aligned16(counts) || !aligned16(workspace)) return OVM_ERR_INVALID;
  if (workgroups(G) > kMaxWorkgroups) return OVM_ERR_CAPACITY;
  const DecodeLayout L = decode_layout(total_runs);
  if (workspace_bytes < L.total) return OVM_ERR_CAPACITY;
  uint8_t* ws = (uint8_t*)workspace;
  uint64_t* cum = (uint64_t*)(ws + L.cum);
  hipStream_t s = (hipStream_t)stream;
  launch_scan(counts, total_runs, (uint64_t*)(ws + L.partial), cum, s);
  hipLaunchKernelGGL(rle_check_kernel, dim3(1), dim3(256), 0, s, (const uint64_t*)cum, run_offsets, total_runs, (int)n,
                     (uint64_t)H * (uint64_t)W, status);
  hipLaunchKernelGGL(rle_fill_kernel, dim3((unsigned)workgroups(G)), dim3(256), 0, s, (const uint64_t*)cum, run_offsets, total_runs, G, masks_out);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
