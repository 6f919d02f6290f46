// Exclusive prefix sum on the device: uint32 in[n] -> uint64 out[n + 1] (out[n] = the total), 2048 items per workgroup, three
// launches on the caller's stream (reduce per tile, scan the tile sums in one workgroup, apply). Integer sums: exact and
// order-independent. Shared by the JPEG encoder (bit and stuffed-byte offsets), the mask run-length coder (run ranks, string
// offsets) and the scene PLY packer (the first record of each tile); each translation unit gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ovm_scan {

constexpr int kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;

// bytes of the `partial` scratch launch_scan needs for n items
inline int64_t scan_partial_bytes(int64_t n) { return ((n + kScanTile - 1) / kScanTile + 1) * 8; }

// exclusive scan of one value per lane over the workgroup; *total = the sum
__device__ __forceinline__ uint64_t wg_exclusive_scan(uint64_t v, uint64_t* total) {
  __shared__ __attribute__((aligned(16))) uint64_t sh[kScanThreads];
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const uint64_t incl = sh[t];
  *total = sh[kScanThreads - 1];
  return incl - v;
}

__device__ __forceinline__ void scan_load(const uint32_t* __restrict__ in, int64_t n, int64_t i0, unsigned* v) {
  if (i0 + kScanItems <= n) {
    const uint4 a = *(const uint4*)(in + i0), b = *(const uint4*)(in + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) v[j] = i0 + j < n ? in[i0 + j] : 0u;
  }
}

static __global__ __launch_bounds__(kScanThreads) void scan_reduce_kernel(const uint32_t* __restrict__ in, int64_t n, uint64_t* __restrict__ partial) {
  const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
  unsigned v[kScanItems];
  scan_load(in, n, i0, v);
  uint64_t sum = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) sum += v[j];
  uint64_t total;
  wg_exclusive_scan(sum, &total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: the partial sums become exclusive offsets in place; out_total = the grand total
static __global__ __launch_bounds__(kScanThreads) void scan_partials_kernel(uint64_t* __restrict__ partial, int np, uint64_t* __restrict__ out_total) {
  uint64_t carry = 0;
  for (int base = 0; base < np; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const uint64_t v = i < np ? partial[i] : 0;
    uint64_t total;
    const uint64_t ex = wg_exclusive_scan(v, &total);
    if (i < np) partial[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *out_total = carry;
}

static __global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(const uint32_t* __restrict__ in, int64_t n, const uint64_t* __restrict__ partial,
                                                                         uint64_t* __restrict__ out) {
  const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
  unsigned v[kScanItems];
  scan_load(in, n, i0, v);
  uint64_t sum = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) sum += v[j];
  uint64_t total;
  uint64_t run = partial[blockIdx.x] + wg_exclusive_scan(sum, &total);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (i0 + j < n) out[i0 + j] = run;
    run += v[j];
  }
}

// in: 16-byte aligned, n >= 1; partial: scan_partial_bytes(n) of scratch; out: n + 1 words
static inline void launch_scan(const uint32_t* in, int64_t n, uint64_t* partial, uint64_t* out, hipStream_t s) {
  const int np = (int)((n + kScanTile - 1) / kScanTile);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(np), dim3(kScanThreads), 0, s, in, n, partial);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, s, partial, np, out + n);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(np), dim3(kScanThreads), 0, s, in, n, (const uint64_t*)partial, out);
}

}  // namespace ovm_scan
