// The point part of <name>_scene.ply (ovm_scene_ply_points; the rules are in include/ovm3d.h, "Scene as a PLY file"): the depth map's
// valid pixels, un-projected as scene_splat does (render.hip, Pass A) and coloured as Pass B colours them, packed as 15-byte vertex
// records in row-major pixel order. Only those bytes and the 8-byte count cross PCIe; the header, the box vertices, faces and
// edges are host work of the Python layer.
//
// The kept grid (every stride-th row and column) is cut into tiles of 2,048 pixels in row-major order, one 256-thread workgroup
// per tile, lane t taking pixels t, t + 256, ... of the tile (coalesced reads):
//   ply_count   the tile's number of valid pixels (ballots, no atomics);
//   launch_scan the exclusive prefix sum of the tile counts (scan.hpp): tile k owns records [r0, r1) and the total is P;
//   ply_pack    validity again, the rank of each point inside the tile from the ballots, the records laid into LDS at 15 * rank
//               (30 KiB), then the tile's byte range [15 r0, 15 r1) of the output: byte stores up to the first 16-byte boundary,
//               16-byte stores for the interior - each assembled from five LDS words, since the range starts at any alignment -
//               and byte stores for the rest. No store touches a byte outside the tile's own range, so neighbouring workgroups
//               never write the same word and nothing at or past 15 P is written.
// fp64 with contraction off and one rounding to float32, as tests/scene_ply_oracle.py restates it; integer colour arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ovm3d.h"
#include "scan.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = ovm_scan::kScanThreads, kRounds = 8, kTile = kThreads * kRounds;     // 2,048 kept pixels per workgroup
constexpr int kRecord = 15, kWaves = kThreads / 64;
static_assert(kTile * kRecord == 30 * 1024, "the records of one tile fill 30 KiB of LDS");

struct PlyArgs {
  const uint8_t* image; int64_t image_pitch;
  const float* depth; int64_t depth_pitch;
  const int32_t* labels; int64_t labels_pitch;
  const uint8_t* tint;                  // device [n_boxes][4]
  int n_boxes, Ws, stride, flip;
  int64_t G;                            // kept pixels: ceil(H / stride) * ceil(W / stride)
  double fx, cx, fy, cy;
  float max_depth;                      // <= 0: none
};

struct Workspace { size_t counts, partial, offsets, tint, total; };

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

Workspace plan(int64_t tiles, int n_boxes) {
  Workspace w{};
  size_t o = 0;
  w.counts = o; o = align256(o + 4 * (size_t)tiles);
  w.partial = o; o = align256(o + (size_t)ovm_scan::scan_partial_bytes(tiles));
  w.offsets = o; o = align256(o + 8 * (size_t)(tiles + 1));
  w.tint = o; o = align256(o + 4 * (size_t)(n_boxes > 0 ? n_boxes : 1));
  w.total = o;
  return w;
}

// kept pixel g of the grid -> its depth and whether it becomes a point; (i, j) = the pixel
__device__ __forceinline__ bool ply_valid(const PlyArgs& A, int64_t g, int* i, int* j, float* d) {
  if (g >= A.G) return false;
  const int gi = (int)(g / A.Ws);
  *i = gi * A.stride;
  *j = (int)(g - (int64_t)gi * A.Ws) * A.stride;
  const float df = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(A.depth) + (int64_t)*i * A.depth_pitch + 4 * (int64_t)*j);
  *d = df;
  return isfinite(df) && df > 0.0f && !(A.max_depth > 0.0f && df > A.max_depth);
}

__global__ __launch_bounds__(kThreads) void ply_count(PlyArgs A, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kWaves];
  const int64_t g0 = (int64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t c = 0;                        // wave-uniform
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    int i, j;
    float d;
    c += (uint32_t)__popcll(__ballot(ply_valid(A, g0 + k * kThreads, &i, &j, &d)));
  }
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kWaves; ++w) s += wave_cnt[w];
    counts[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kThreads) void ply_pack(PlyArgs A, const uint64_t* __restrict__ offsets, int64_t tiles, uint8_t* __restrict__ out,
                                                     uint64_t* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) uint32_t rec[kTile * kRecord / 4];
  __shared__ uint32_t wave_cnt[kRounds][kWaves];
  uint8_t* rb = reinterpret_cast<uint8_t*>(rec);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t g0 = (int64_t)blockIdx.x * kTile + t;
  if (blockIdx.x == 0 && t == 0) *count = offsets[tiles];

  int pi[kRounds], pj[kRounds], below[kRounds];
  float pd[kRounds];
  bool ok[kRounds];
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    ok[k] = ply_valid(A, g0 + k * kThreads, &pi[k], &pj[k], &pd[k]);
    const unsigned long long b = __ballot(ok[k]);
    below[k] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[k][wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  // pixel order inside the tile is (round, wave, lane): the points in front of this lane's point of round k
  int base[kRounds] = {}, run = 0;
#pragma unroll
  for (int k = 0; k < kRounds; ++k)
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) base[k] = run;
      run += (int)wave_cnt[k][w];
    }
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    if (!ok[k]) continue;
    const int i = pi[k], j = pj[k];
    const double d = (double)pd[k];
    float p[3] = {(float)(((j + 0.5) - A.cx) / A.fx * d), (float)(((i + 0.5) - A.cy) / A.fy * d), pd[k]};
    if (A.flip) { p[1] = -p[1]; p[2] = -p[2]; }
    const uint8_t* ip = A.image + (int64_t)i * A.image_pitch + 3 * (int64_t)j;
    int c[3] = {ip[0], ip[1], ip[2]};
    if (A.labels) {
      const int b = *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(A.labels) + (int64_t)i * A.labels_pitch + 4 * (int64_t)j);
      if (b >= 0 && b < A.n_boxes) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = (c[ch] + (int)A.tint[4 * b + ch] + 1) >> 1;
      }
    }
    uint8_t* r = rb + kRecord * (base[k] + below[k]);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint32_t u = __float_as_uint(p[q]);
      r[4 * q] = (uint8_t)u; r[4 * q + 1] = (uint8_t)(u >> 8); r[4 * q + 2] = (uint8_t)(u >> 16); r[4 * q + 3] = (uint8_t)(u >> 24);
    }
    r[12] = (uint8_t)c[2]; r[13] = (uint8_t)c[1]; r[14] = (uint8_t)c[0];            // red, green, blue from BGR
  }
  __syncthreads();

  const uint64_t r0 = offsets[blockIdx.x], r1 = offsets[blockIdx.x + 1];
  const int nbytes = kRecord * (int)(r1 - r0);                                     // <= 30,720
  uint8_t* dst = out + (int64_t)kRecord * (int64_t)r0;
  int head = (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
  if (head > nbytes) head = nbytes;
  const int nquad = (nbytes - head) >> 4, tail = head + 16 * nquad;
  if (t < head) dst[t] = rb[t];
  // quad q = LDS bytes [head + 16 q, head + 16 q + 16): words w .. w + 3 shifted down by (head & 3) bytes, topped up from word w + 4,
  // which lies inside the records whenever the shift is not zero
  const int sh = 8 * (head & 3);
  for (int q = t; q < nquad; q += kThreads) {
    const int w = (head >> 2) + 4 * q;
    uint32_t v[5] = {rec[w], rec[w + 1], rec[w + 2], rec[w + 3], 0u};
    if (sh) {
      v[4] = rec[w + 4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] >> sh) | (v[e + 1] << (32 - sh));
    }
    *reinterpret_cast<uint4*>(dst + head + 16 * q) = make_uint4(v[0], v[1], v[2], v[3]);
  }
  if (tail + t < nbytes) dst[tail + t] = rb[tail + t];                              // fewer than 16 bytes
}

int check_shape(int32_t H, int32_t W, int32_t stride, int32_t n_boxes) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647ll || stride < 1 || stride > 16 || n_boxes < 0 || n_boxes > OVM_SCENE_MAX_BOXES)
    return OVM_ERR_INVALID;
  return OVM_OK;
}

int64_t kept(int32_t n, int32_t stride) { return ((int64_t)n + stride - 1) / stride; }

}  // namespace

extern "C" {

int ovm_scene_ply_points_workspace(int32_t H, int32_t W, int32_t stride, int32_t n_boxes, int64_t* bytes) {
  if (!bytes || check_shape(H, W, stride, n_boxes) != OVM_OK) return OVM_ERR_INVALID;
  const int64_t G = kept(H, stride) * kept(W, stride);
  *bytes = (int64_t)plan((G + kTile - 1) / kTile, n_boxes).total;
  return OVM_OK;
}

int ovm_scene_ply_points(const uint8_t* image, int64_t image_pitch, const float* depth, int64_t depth_pitch, const int32_t* labels,
                         int64_t labels_pitch, const uint8_t* tint, int32_t n_boxes, int32_t H, int32_t W, const double* K, int32_t stride,
                         float max_depth, int32_t flip, uint8_t* out, int64_t out_bytes, uint64_t* count, void* workspace,
                         int64_t workspace_bytes, ovm_stream_t stream) {
  if (!image || !depth || !K || !out || !count || !workspace || check_shape(H, W, stride, n_boxes) != OVM_OK) return OVM_ERR_INVALID;
  if (image_pitch < 3 * (int64_t)W || depth_pitch < 4 * (int64_t)W || depth_pitch % 4 != 0) return OVM_ERR_INVALID;
  if (labels && (!tint || labels_pitch < 4 * (int64_t)W || labels_pitch % 4 != 0)) return OVM_ERR_INVALID;
  if ((flip != 0 && flip != 1) || std::isnan(max_depth) || reinterpret_cast<uintptr_t>(workspace) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(count) % 8 != 0)
    return OVM_ERR_INVALID;
  if (!std::isfinite(K[0]) || !std::isfinite(K[2]) || !std::isfinite(K[4]) || !std::isfinite(K[5]) || K[0] == 0.0 || K[4] == 0.0)
    return OVM_ERR_INVALID;
  const int64_t Ws = kept(W, stride), G = kept(H, stride) * Ws, tiles = (G + kTile - 1) / kTile;
  const Workspace pk = plan(tiles, n_boxes);
  if (out_bytes < kRecord * G || workspace_bytes < (int64_t)pk.total) return OVM_ERR_CAPACITY;

  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  const bool tinted = labels && n_boxes > 0;
  if (tinted && hipMemcpyAsync(ws + pk.tint, tint, 4 * (size_t)n_boxes, hipMemcpyHostToDevice, s) != hipSuccess) return OVM_ERR_HIP;
  PlyArgs A{};
  A.image = image; A.image_pitch = image_pitch;
  A.depth = depth; A.depth_pitch = depth_pitch;
  A.labels = tinted ? labels : nullptr; A.labels_pitch = labels_pitch;             // no box: no label tints
  A.tint = ws + pk.tint;
  A.n_boxes = n_boxes; A.Ws = (int)Ws; A.stride = stride; A.flip = flip; A.G = G;
  A.fx = K[0]; A.cx = K[2]; A.fy = K[4]; A.cy = K[5];
  A.max_depth = max_depth;
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + pk.counts);
  uint64_t* offsets = reinterpret_cast<uint64_t*>(ws + pk.offsets);
  hipLaunchKernelGGL(ply_count, dim3((unsigned)tiles), dim3(kThreads), 0, s, A, counts);
  ovm_scan::launch_scan(counts, tiles, reinterpret_cast<uint64_t*>(ws + pk.partial), offsets, s);
  hipLaunchKernelGGL(ply_pack, dim3((unsigned)tiles), dim3(kThreads), 0, s, A, (const uint64_t*)offsets, tiles, out, count);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
