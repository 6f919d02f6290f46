// Connected components of binary planes on the device (ovm_mask_cc_label) and segment_anything's small-region clean-up on top of
// them (ovm_mask_remove_small_regions); the rules are in include/ovm3d.h, "Mask connected components".
//
// One wave owns a segment: 64 consecutive pixels of one row of one plane (a workgroup is 4 segments), so every access of a
// pass is one coalesced wave load or store and ballots describe the row runs. parent[] is int32 per pixel, an index within the
// plane, -1 on background. Union-find in global memory, the larger root always hooked under the smaller, so the root of a
// component is its first pixel in row-major order:
//   1 cc_init_kernel     parent = the start of the pixel's run within its segment (the horizontal unions inside a wave cost a ballot)
//   2 cc_union_kernel    the unions left: a segment's first pixel with the pixel to its left; with the row above only where the
//                        contact begins (up, unless left and up-left are both set; under 8-connectivity up-left / up-right when
//                        up is clear and the pixel to the left / right does not make the same contact)
//   3 cc_flatten_kernel  the first lane of every run walks to the root and hands it to its run: parent = root for every pixel;
//                        label call: the root lanes of the segment as a bit mask and their number; clean-up call: area[root] +=
//                        lanes per distinct root of the wave (one atomicAdd each)
//   label call           scan.hpp over the segments' root counts, then 4 cc_label_kernel: label = rank of the root among its
//                        plane's roots = scanned count of the root's segment + roots below it in that segment's bit mask + 1
//   clean-up call        4 cc_stats_kernel: per plane "a region is small", "a region is not small", max of (area, ~root);
//                        5 cc_apply_kernel writes the plane. Mode 3 runs 1 .. 5 twice, the second time on the output plane.
// Seven launches for labels, five per clean-up step, whatever the planes hold; nothing is read back.
//
// Across workgroups nothing relies on a plain load seeing another workgroup's write of the same launch. Every decision of a
// union is the return value of an atomicMin on a root; a plain read of parent[] is a hint: parents only ever move to smaller
// indices of the same component, so an old parent is still an ancestor and the walk goes on from it. Passes 3 to 5 read what
// earlier launches wrote. Every walk counts its steps against a bound derived from H * W; running out (or meeting an index
// that cannot be a parent) sets the status word and ends the thread.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/ovm3d.h"
#include "scan.hpp"

namespace {

using ovm_scan::launch_scan;
using ovm_scan::scan_partial_bytes;

constexpr int kSeg = 64;                                // pixels per segment = lanes per wave
constexpr int kWgSegs = 4;
constexpr int64_t kMaxWorkgroups = (1 << 24) - 1;       // 4 segments each: a segment index stays below 2^26

struct Geom {
  int n, H, W, SW;                   // SW segments per row
  unsigned per_plane, total;         // segments per plane, segments in all
  int64_t npix;                      // H * W
};

struct Lane {
  int i, y, x, lane;                 // plane, row, column
  unsigned s;                        // segment index over all planes
  bool valid;                        // x < W
  int p;                             // y * W + x (valid lanes)
};

// false for a wave past the last segment (wave-uniform)
__device__ __forceinline__ bool lane_of(const Geom& G, Lane* L) {
  const unsigned s = blockIdx.x * kWgSegs + (threadIdx.x >> 6);
  if (s >= G.total) return false;
  L->s = s;
  L->lane = (int)(threadIdx.x & 63);
  L->i = (int)(s / G.per_plane);
  const unsigned r = s % G.per_plane;
  L->y = (int)(r / (unsigned)G.SW);
  L->x = (int)(r % (unsigned)G.SW) * kSeg + L->lane;
  L->valid = L->x < G.W;
  L->p = (int)((unsigned)L->y * (unsigned)G.W + (unsigned)L->x);     // meaningful on valid lanes
  return true;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the first lane of the run of set bits that holds `lane` (its bit is set)
__device__ __forceinline__ int run_start(uint64_t set, int lane) {
  const uint64_t z = ~set & lanes_below(lane);
  return z ? 64 - __clzll((long long)z) : 0;
}

__device__ __forceinline__ void fail(int32_t* status) {
  atomicExch(&status[0], OVM_ERR_HIP);
  atomicAdd(&status[1], 1);
}

// Walk from x to a root as plain loads show it (a hint: the caller's atomicMin decides). -1: the budget ran out or a value no
// parent can have was met. compress: a walk of more than one step leaves the root it found as the start's parent (atomicMin,
// so the parent still only moves down to an ancestor).
__device__ __forceinline__ int find_root(int* __restrict__ P, int x, int64_t* budget, bool compress) {
  const int start = x;
  int steps = 0;
  for (;;) {
    const int q = P[x];
    if (q == x) break;
    if (q < 0 || q > x || --*budget < 0) return -1;
    x = q;
    ++steps;
  }
  if (compress && steps > 1) atomicMin(&P[start], x);
  return x;
}

__device__ __forceinline__ bool unite(int* __restrict__ P, int a, int b, int64_t budget) {
  for (;;) {
    a = find_root(P, a, &budget, true);
    b = find_root(P, b, &budget, true);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[a], b);                // hook the larger root under the smaller
    if (old == a) return true;                          // a was a root: done
    // a had been hooked under old < a meanwhile, and now hangs under min(old, b): old and b are still to be joined
    if (old < 0 || old > a || --budget < 0) return false;
    a = old;
  }
}

__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* __restrict__ masks, int64_t plane_stride, int64_t pitch, int invert, Geom G,
                                                      int* __restrict__ parent, int* __restrict__ area, unsigned long long* __restrict__ keys,
                                                      int* __restrict__ flags, int32_t* __restrict__ status) {
  Lane L;
  if (!lane_of(G, &L)) return;
  if (status && L.s == 0 && L.lane == 0) { status[0] = OVM_OK; status[1] = 0; status[2] = 0; status[3] = 0; }
  if (keys && L.s % G.per_plane == 0 && L.lane == 0) { keys[L.i] = 0ull; flags[L.i] = 0; }
  const bool fg = L.valid && ((masks[(int64_t)L.i * plane_stride + (int64_t)L.y * pitch + L.x] != 0) != (invert != 0));
  const uint64_t set = __ballot(fg);
  if (!L.valid) return;
  const int64_t g = (int64_t)L.i * G.npix + L.p;
  parent[g] = fg ? L.p - L.lane + run_start(set, L.lane) : -1;
  if (area) area[g] = 0;
}

__global__ __launch_bounds__(256) void cc_union_kernel(Geom G, int conn8, int* __restrict__ parent, int32_t* __restrict__ status) {
  Lane L;
  if (!lane_of(G, &L) || !L.valid) return;
  int* P = parent + (int64_t)L.i * G.npix;
  const int p = L.p, W = G.W;
  if (P[p] < 0) return;
  const int64_t budget = 2 * G.npix + 64;
  const bool left = L.x > 0 && P[p - 1] >= 0;
  bool ok = true;
  if (L.lane == 0 && left) ok = unite(P, p, p - 1, budget);
  if (L.y > 0) {
    const bool up = P[p - W] >= 0;
    const bool ul = L.x > 0 && P[p - W - 1] >= 0;
    if (up) {
      if (!(left && ul)) ok = unite(P, p, p - W, budget) && ok;       // else the pixel to the left carries this contact
    } else if (conn8) {
      const bool ur = L.x < W - 1 && P[p - W + 1] >= 0;
      const bool right = L.x < W - 1 && P[p + 1] >= 0;
      if (ul && !left) ok = unite(P, p, p - W - 1, budget) && ok;
      if (ur && !right) ok = unite(P, p, p - W + 1, budget) && ok;
    }
  }
  if (!ok) fail(status);
}

// rootmask, segcnt: the label call; area: the clean-up call
__global__ __launch_bounds__(256) void cc_flatten_kernel(Geom G, int* __restrict__ parent, uint64_t* __restrict__ rootmask, uint32_t* __restrict__ segcnt,
                                                         int* __restrict__ area, int32_t* __restrict__ status) {
  Lane L;
  if (!lane_of(G, &L)) return;
  int* P = parent + (int64_t)L.i * G.npix;
  const bool fg = L.valid && P[L.p] >= 0;
  const uint64_t set = __ballot(fg);
  const int rs = fg ? run_start(set, L.lane) : L.lane;
  int root = -1;
  if (fg && rs == L.lane) {
    int64_t budget = G.npix + 1;
    root = find_root(P, L.p, &budget, false);
    if (root < 0) fail(status);
  }
  root = __shfl(root, rs);
  if (fg && root >= 0) P[L.p] = root;
  const bool is_root = fg && root == L.p;
  if (rootmask) {
    const uint64_t roots = __ballot(is_root);
    if (L.lane == 0) { rootmask[L.s] = roots; segcnt[L.s] = (uint32_t)__popcll(roots); }
  }
  if (area) {
    uint64_t todo = __ballot(fg && root >= 0);
    while (todo) {                                      // one add per distinct root among the lanes
      const int r = __shfl(root, __ffsll((long long)todo) - 1);
      const uint64_t same = __ballot(fg && root == r);
      if (L.lane == 0) atomicAdd(&area[(int64_t)L.i * G.npix + r], (int)__popcll(same));
      todo &= ~same;
    }
  }
}

__global__ __launch_bounds__(256) void cc_label_kernel(Geom G, const int* __restrict__ parent, const uint64_t* __restrict__ rootmask,
                                                       const uint64_t* __restrict__ segscan, int32_t* __restrict__ labels, int64_t label_plane_stride,
                                                       int64_t label_pitch, int32_t* __restrict__ counts) {
  Lane L;
  if (!lane_of(G, &L)) return;
  const unsigned s0 = (unsigned)L.i * G.per_plane;
  const uint64_t base = segscan[s0];
  if (L.s == s0 && L.lane == 0) counts[L.i] = (int32_t)(segscan[s0 + G.per_plane] - base);
  if (!L.valid) return;
  const int r = parent[(int64_t)L.i * G.npix + L.p];
  int32_t label = 0;
  if (r >= 0) {
    const int ry = r / G.W, rx = r - ry * G.W;
    const unsigned sr = s0 + (unsigned)ry * (unsigned)G.SW + (unsigned)(rx / kSeg);
    label = (int32_t)(segscan[sr] - base) + (int32_t)__popcll(rootmask[sr] & lanes_below(rx % kSeg)) + 1;
  }
  labels[(int64_t)L.i * label_plane_stride + (int64_t)L.y * label_pitch + L.x] = label;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  for (int d = 32; d; d >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), d), lo = __shfl_xor((unsigned)v, d);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// flags: 1 = a region is small, 2 = a region is not small; keys: max of (area << 32 | ~root): the largest region, on a tie the first
__global__ __launch_bounds__(256) void cc_stats_kernel(Geom G, const int* __restrict__ parent, const int* __restrict__ area, int64_t min_area,
                                                       unsigned long long* __restrict__ keys, int* __restrict__ flags) {
  Lane L;
  if (!lane_of(G, &L)) return;
  const int64_t g = (int64_t)L.i * G.npix + L.p;
  const bool is_root = L.valid && parent[g] == L.p;
  const uint64_t roots = __ballot(is_root);
  if (!roots) return;
  const int a = is_root ? area[g] : 0;
  const bool small = is_root && (int64_t)a < min_area;
  const int f = (__ballot(small) ? 1 : 0) | (__ballot(is_root && !small) ? 2 : 0);
  const unsigned long long key = wave_max_u64(is_root ? ((unsigned long long)(unsigned)a << 32) | (unsigned)~(unsigned)L.p : 0ull);
  if (L.lane == 0) {
    atomicOr(&flags[L.i], f);
    atomicMax(&keys[L.i], key);
  }
}

// in: the plane the step works on (the caller's for the first step, the output for the second of mode 3: a lane reads and writes
// its own pixel only). holes: the working plane is the complement.
__global__ __launch_bounds__(256) void cc_apply_kernel(const uint8_t* in, int64_t in_plane_stride, int64_t in_pitch, Geom G, int holes,
                                                       const int* __restrict__ parent, const int* __restrict__ area, int64_t min_area,
                                                       const unsigned long long* __restrict__ keys, const int* __restrict__ flags, uint8_t* out,
                                                       int64_t out_plane_stride, int64_t out_pitch, int32_t* __restrict__ changed, int second) {
  Lane L;
  if (!lane_of(G, &L)) return;
  const int f = flags[L.i];
  if (L.s % G.per_plane == 0 && L.lane == 0) changed[L.i] = (second ? changed[L.i] : 0) | (f & 1);
  if (!L.valid) return;
  const bool inside = in[(int64_t)L.i * in_plane_stride + (int64_t)L.y * in_pitch + L.x] != 0;
  bool o = inside;
  if (f & 1) {
    const int64_t g0 = (int64_t)L.i * G.npix;
    const int r = parent[g0 + L.p];                     // >= 0 on the working plane
    const bool small = r >= 0 && (int64_t)area[g0 + r] < min_area;
    if (holes) o = inside || small;
    else if (f & 2) o = inside && !small;
    else o = inside && r == (int)~(unsigned)keys[L.i];  // every region is small: the largest stays
  }
  out[(int64_t)L.i * out_plane_stride + (int64_t)L.y * out_pitch + L.x] = o ? 1 : 0;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// OVM_ERR_INVALID for arguments no call takes, OVM_ERR_CAPACITY for more segments than one call launches
int make_geom(int32_t n, int32_t H, int32_t W, Geom* G) {
  if (n < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL) return OVM_ERR_INVALID;
  G->n = n; G->H = H; G->W = W;
  G->SW = (W + kSeg - 1) / kSeg;
  G->npix = (int64_t)H * W;
  const int64_t per_plane = (int64_t)H * G->SW, total = per_plane * n;
  if ((total + kWgSegs - 1) / kWgSegs > kMaxWorkgroups) return OVM_ERR_CAPACITY;
  G->per_plane = (unsigned)per_plane;
  G->total = (unsigned)total;
  return OVM_OK;
}

unsigned workgroups(const Geom& G) { return (G.total + kWgSegs - 1) / kWgSegs; }

struct LabelLayout { int64_t parent, rootmask, segcnt, segscan, partial, total; };

LabelLayout label_layout(const Geom& G) {
  LabelLayout L;
  int64_t o = 0;
  L.parent = o; o += align16(G.npix * G.n * 4);
  L.rootmask = o; o += align16((int64_t)G.total * 8);
  L.segcnt = o; o += align16((int64_t)G.total * 4);
  L.segscan = o; o += align16(((int64_t)G.total + 1) * 8);
  L.partial = o; o += align16(scan_partial_bytes(G.total));
  L.total = o;
  return L;
}

struct CleanLayout { int64_t parent, area, keys, flags, total; };

CleanLayout clean_layout(const Geom& G) {
  CleanLayout L;
  int64_t o = 0;
  L.parent = o; o += align16(G.npix * G.n * 4);
  L.area = o; o += align16(G.npix * G.n * 4);
  L.keys = o; o += align16((int64_t)G.n * 8);
  L.flags = o; o += align16((int64_t)G.n * 4);
  L.total = o;
  return L;
}

// the bytes [lo, hi) that n planes of H rows of W bytes touch
void span(const uint8_t* base, int64_t plane_stride, int64_t pitch, const Geom& G, uintptr_t* lo, uintptr_t* hi) {
  const int64_t last = (int64_t)(G.n - 1) * plane_stride;
  *lo = (uintptr_t)base + (uintptr_t)(last < 0 ? last : 0);
  *hi = (uintptr_t)base + (uintptr_t)(last > 0 ? last : 0) + (uintptr_t)((int64_t)(G.H - 1) * pitch + G.W);
}

}  // namespace

extern "C" {

int ovm_mask_cc_label_workspace(int32_t n, int32_t H, int32_t W, int64_t* bytes) {
  Geom G;
  if (!bytes) return OVM_ERR_INVALID;
  if (const int rc = make_geom(n, H, W, &G)) return rc;
  *bytes = label_layout(G).total;
  return OVM_OK;
}

int ovm_mask_cc_label(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W, int32_t connectivity,
                      int32_t invert, int32_t* labels_out, int64_t label_plane_stride, int64_t label_pitch, int32_t* counts_out, int32_t* status,
                      void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  Geom G;
  if (!masks || !labels_out || !counts_out || !status || !workspace) return OVM_ERR_INVALID;
  const int rc = make_geom(n, H, W, &G);
  if (rc == OVM_ERR_INVALID) return rc;
  if (row_pitch < W || label_pitch < W || (connectivity != 4 && connectivity != 8) || !aligned16(workspace)) return OVM_ERR_INVALID;
  if (rc) return rc;
  const LabelLayout L = label_layout(G);
  if (workspace_bytes < L.total) return OVM_ERR_CAPACITY;
  uint8_t* ws = (uint8_t*)workspace;
  int* parent = (int*)(ws + L.parent);
  uint64_t* rootmask = (uint64_t*)(ws + L.rootmask);
  uint32_t* segcnt = (uint32_t*)(ws + L.segcnt);
  uint64_t* segscan = (uint64_t*)(ws + L.segscan);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(workgroups(G)), block(256);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, s, masks, plane_stride, row_pitch, (int)(invert != 0), G, parent, (int*)nullptr,
                     (unsigned long long*)nullptr, (int*)nullptr, status);
  hipLaunchKernelGGL(cc_union_kernel, grid, block, 0, s, G, (int)(connectivity == 8), parent, status);
  hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, G, parent, rootmask, segcnt, (int*)nullptr, status);
  launch_scan(segcnt, G.total, (uint64_t*)(ws + L.partial), segscan, s);
  hipLaunchKernelGGL(cc_label_kernel, grid, block, 0, s, G, (const int*)parent, (const uint64_t*)rootmask, (const uint64_t*)segscan, labels_out,
                     label_plane_stride, label_pitch, counts_out);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

int ovm_mask_remove_small_regions_workspace(int32_t n, int32_t H, int32_t W, int64_t* bytes) {
  Geom G;
  if (!bytes) return OVM_ERR_INVALID;
  if (const int rc = make_geom(n, H, W, &G)) return rc;
  *bytes = clean_layout(G).total;
  return OVM_OK;
}

int ovm_mask_remove_small_regions(const uint8_t* masks, int64_t plane_stride, int64_t row_pitch, int32_t n, int32_t H, int32_t W, int64_t min_area,
                                  int32_t mode, uint8_t* masks_out, int64_t out_plane_stride, int64_t out_row_pitch, int32_t* changed_out,
                                  int32_t* status, void* workspace, int64_t workspace_bytes, ovm_stream_t stream) {
  Geom G;
  if (!masks || !masks_out || !changed_out || !status || !workspace) return OVM_ERR_INVALID;
  const int rc = make_geom(n, H, W, &G);
  if (rc == OVM_ERR_INVALID) return rc;
  if (row_pitch < W || out_row_pitch < W || min_area < 1 || mode < 1 || mode > 3 || !aligned16(workspace)) return OVM_ERR_INVALID;
  uintptr_t a0, a1, b0, b1;
  span(masks, plane_stride, row_pitch, G, &a0, &a1);
  span(masks_out, out_plane_stride, out_row_pitch, G, &b0, &b1);
  if (a0 < b1 && b0 < a1) return OVM_ERR_INVALID;
  // the output planes must not overlap each other either: every plane is written, and mode 3 reads it back
  const int64_t out_plane_bytes = (int64_t)(H - 1) * out_row_pitch + W;
  if (n > 1 && (out_plane_stride < 0 ? -out_plane_stride : out_plane_stride) < out_plane_bytes) return OVM_ERR_INVALID;
  if (rc) return rc;
  const CleanLayout L = clean_layout(G);
  if (workspace_bytes < L.total) return OVM_ERR_CAPACITY;
  uint8_t* ws = (uint8_t*)workspace;
  int* parent = (int*)(ws + L.parent);
  int* area = (int*)(ws + L.area);
  unsigned long long* keys = (unsigned long long*)(ws + L.keys);
  int* flags = (int*)(ws + L.flags);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(workgroups(G)), block(256);
  int second = 0;
  for (int holes = 1; holes >= 0; --holes) {
    if (!(mode & (holes ? 1 : 2))) continue;
    const uint8_t* in = second ? masks_out : masks;
    const int64_t ips = second ? out_plane_stride : plane_stride, ipitch = second ? out_row_pitch : row_pitch;
    hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, s, in, ips, ipitch, holes, G, parent, area, keys, flags, second ? (int32_t*)nullptr : status);
    hipLaunchKernelGGL(cc_union_kernel, grid, block, 0, s, G, 1, parent, status);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, G, parent, (uint64_t*)nullptr, (uint32_t*)nullptr, area, status);
    hipLaunchKernelGGL(cc_stats_kernel, grid, block, 0, s, G, (const int*)parent, (const int*)area, min_area, keys, flags);
    hipLaunchKernelGGL(cc_apply_kernel, grid, block, 0, s, in, ips, ipitch, G, holes, (const int*)parent, (const int*)area, min_area,
                       (const unsigned long long*)keys, (const int*)flags, masks_out, out_plane_stride, out_row_pitch, changed_out, second);
    second = 1;
  }
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
