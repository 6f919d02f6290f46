// The entropy stage of the JPEG decode on the device: the file's bytes in, the coefficient planes of ovm_host_jpeg_entropy_decode out,
// bit for bit, for ovm_jpeg_reconstruct (jpeg.hip) to read. The mirror of jpeg_enc.hip's bit packing.
//
// A Huffman stream is not inherently serial: a decoder started at a wrong bit position falls in step with the true one after a few
// symbols (self-synchronisation; Klein & Wiseman 2003, used for JPEG on GPUs by Weissenberger & Schmidt 2018). The unstuffed stream is
// cut into subsequences of kSubBits bits, one thread each. Every thread decodes its subsequence from a guessed state "start of an MCU";
// then the entry state of subsequence i + 1 is set to the exit state of i and whoever's entry changed decodes again, until nothing
// changes. The first subsequence starts from the true state, and so does every restart segment's first bit, so the fixed point is
// the sequential decode. The decoding rules live in jpeg_dec_core.hpp, shared with the host emulation (jpeg_dec_host.hpp).
//
// Kernels, all on the caller's stream, no read back in between (status and rounds end as two device words):
//   1 jdec_count_kernel / jdec_scan_* / jdec_unstuff_kernel: per 32-byte chunk the bytes that stay (an 0x00 behind 0xFF and the RSTn
//     markers go) and the markers; exclusive prefix sum of both; scatter into the zero-padded stream; each marker checks its number
//     and records where its restart segment starts
//   2 jdec_sync_kernel x kSyncLaunches: a workgroup relaxes its kWgSubs subsequences in LDS (__syncthreads loop, at most max_rounds
//     steps, only threads whose entry changed decode); across workgroups the first thread takes the exit state that the workgroup
//     before it published in the PREVIOUS launch (double-buffered: no workgroup ever waits for, or reads, a word another workgroup
//     writes in the same launch). A launch in which no thread decoded proves the fixed point; later launches return at once.
//   3 jdec_scan_* over the blocks each subsequence completed, then jdec_write_kernel: the same decode once more, now storing each
//     coefficient de-zigzagged at its MCU-order -> plane-order address (a block split by a boundary is written by two threads) and
//     each DC difference; at every restart-segment crossing the block count is checked against the frame's
//   4 jdec_scan_* over the DC differences in component-major scan order, jdec_dc_kernel: predictor = difference of two prefix sums
//     (the restart segments have fixed lengths), range check, int16 store as the host's cast; jdec_finish_kernel: status and rounds
// Only LDS, global vector atomics (atomicOr / atomicMax on the control words) and plain stores.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/ovm3d.h"
#include "jpeg_dec_host.hpp"

namespace {

using namespace ovm_jpeg_dec;

static_assert(sizeof(Tables) == 11008, "include/ovm3d.h states the size of the table block");

// ------------------------------------------------------------------------------------------------
// exclusive prefix sum: uint64 in[n] -> uint64 out[n + 1] (out[n] = the total), kScanTile items per workgroup
// ------------------------------------------------------------------------------------------------
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

// decided on words that stage 1 and the synchronisation launches wrote: the same answer for every thread of a later launch
__device__ __forceinline__ bool declined(const uint32_t* __restrict__ ctl) {
  return ctl[kCtlStatus] != 0 || ctl[kCtlChanged + kSyncLaunches - 1] != 0;
}

__global__ __launch_bounds__(kScanThreads) void jdec_scan_reduce_kernel(const uint64_t* __restrict__ in, int64_t n, uint64_t* __restrict__ partial) {
  const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
  uint64_t sum = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) sum += i0 + j < n ? in[i0 + j] : 0;
  uint64_t total;
  wg_exclusive_scan(sum, &total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void jdec_scan_partials_kernel(uint64_t* __restrict__ partial, int np, uint64_t* __restrict__ out_total) {
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

__global__ __launch_bounds__(kScanThreads) void jdec_scan_apply_kernel(const uint64_t* __restrict__ in, int64_t n, const uint64_t* __restrict__ partial,
                                                                       uint64_t* __restrict__ out) {
  const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
  uint64_t v[kScanItems], sum = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) { v[j] = i0 + j < n ? in[i0 + j] : 0; sum += v[j]; }
  uint64_t total;
  uint64_t run = partial[blockIdx.x] + wg_exclusive_scan(sum, &total);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (i0 + j < n) out[i0 + j] = run;
    run += v[j];
  }
}

void launch_scan(const uint64_t* in, int64_t n, uint64_t* partial, uint64_t* out, hipStream_t s) {
  const int np = (int)((n + kScanTile - 1) / kScanTile);
  hipLaunchKernelGGL(jdec_scan_reduce_kernel, dim3(np), dim3(kScanThreads), 0, s, in, n, partial);
  hipLaunchKernelGGL(jdec_scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, s, partial, np, out + n);
  hipLaunchKernelGGL(jdec_scan_apply_kernel, dim3(np), dim3(kScanThreads), 0, s, in, n, (const uint64_t*)partial, out);
}

// ------------------------------------------------------------------------------------------------
// 1: unstuffing and the restart-segment table
// ------------------------------------------------------------------------------------------------
// counts of a chunk: bytes kept in the low word, markers in the high word
__global__ void jdec_count_kernel(const uint8_t* __restrict__ s, int64_t n, int64_t nchunks, uint64_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nchunks) return;
  const int64_t j0 = i * kChunkBytes;
  int prev = j0 > 0 ? s[j0 - 1] : -1, cur = s[j0];
  uint32_t kept = 0, markers = 0;
  for (int jj = 0; jj < kChunkBytes; ++jj) {
    const int64_t j = j0 + jj;
    if (j >= n) break;
    const int next = j + 1 < n ? s[j + 1] : -1;
    const uint32_t cl = classify_byte(prev, cur, next);
    kept += cl & kByteKeep; markers += (cl & kByteMarker) ? 1u : 0u;
    prev = cur; cur = next;
  }
  cnt[i] = (uint64_t)kept | ((uint64_t)markers << 32);
}

__global__ void jdec_unstuff_kernel(const uint8_t* __restrict__ s, int64_t n, int64_t nchunks, const uint64_t* __restrict__ off, int nseg,
                                    uint8_t* __restrict__ U, uint32_t* __restrict__ seg_off, uint32_t* __restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nchunks) return;
  uint32_t status = 0;
  if (i == 0) {
    const uint64_t tot = off[nchunks];
    ctl[kCtlTotalBytes] = (uint32_t)tot;
    seg_off[0] = 0;
    if ((uint32_t)(tot >> 32) != (uint32_t)nseg - 1u) status |= kStSegments;
  }
  const int64_t j0 = i * kChunkBytes;
  uint32_t kept = (uint32_t)off[i], ord = (uint32_t)(off[i] >> 32);
  int prev2 = j0 > 1 ? s[j0 - 2] : -1, prev = j0 > 0 ? s[j0 - 1] : -1, cur = s[j0];
  for (int jj = 0; jj < kChunkBytes; ++jj) {
    const int64_t j = j0 + jj;
    if (j >= n) break;
    const int next = j + 1 < n ? s[j + 1] : -1;
    const uint32_t cl = classify_byte(prev, cur, next);
    if (cl & kByteAnomaly) status |= kStMarker;
    if (cl & kByteKeep) {
      if ((int64_t)kept < n) U[kept] = (uint8_t)cur;
      ++kept;
    }
    if (cl & kByteMarker) {
      if (next != (int)(0xD0 + (ord & 7))) status |= kStMarker;
      if (ord + 1 < (uint32_t)nseg) seg_off[ord + 1] = kept; else status |= kStSegments;
      const bool empty_before = j == 0 || (j >= 2 && prev2 == 0xFF && prev >= 0xD0 && prev <= 0xD7), empty_behind = j + 2 >= n;
      if (empty_before || empty_behind) status |= kStSegments;
      ++ord;
    }
    prev2 = prev; prev = cur; cur = next;
  }
  if (status) atomicOr(&ctl[kCtlStatus], status);
}

// ------------------------------------------------------------------------------------------------
// 2: synchronisation
// ------------------------------------------------------------------------------------------------
struct DevStream {
  const uint32_t* words; uint32_t nwords;
  const uint32_t* seg_off;
  const Tables* tab;
};

// A workgroup's share of the stream and the Huffman tables, staged in LDS: a symbol costs two dependent reads (bits, table), and
// from global memory their latency is what the whole decode takes. The share: the words its kWgSubs subsequences start in plus what
// the last one may read past its end (a symbol of up to 31 bits started before the end, and the window's second word).
constexpr int kWgWords = kWgSubs * kSubBits / 32 + 4;
struct WgStage {
  uint32_t words[kWgWords];
  uint32_t tab[sizeof(Tables) / 4];
  Geom geom;
};

__device__ __forceinline__ Ctx stage_ctx(const DevStream& D, const Geom& G, const uint32_t* __restrict__ ctl, WgStage& S) {
  const uint32_t base = blockIdx.x * (uint32_t)(kWgSubs * kSubBits / 32), last = D.nwords - 1;
  for (uint32_t w = threadIdx.x; w < (uint32_t)kWgWords; w += kWgSubs) {
    const uint32_t gi = base + w;
    S.words[w] = D.words[gi < last ? gi : last];                     // the clamp of window(): behind the stream stands its zero last word
  }
  const uint32_t* tsrc = (const uint32_t*)D.tab;
  for (uint32_t w = threadIdx.x; w < (uint32_t)(sizeof(Tables) / 4); w += kWgSubs) S.tab[w] = tsrc[w];
  if (threadIdx.x == 0) S.geom = G;
  __syncthreads();
  Ctx C;
  C.words = S.words; C.word_base = base; C.nlocal = kWgWords; C.nwords = D.nwords;
  C.total_bits = ctl[kCtlTotalBytes] * 8u; C.seg_off = D.seg_off; C.tab = (const Tables*)S.tab; C.g = &S.geom;
  return C;
}

__device__ __forceinline__ uint32_t sub_end_of(int64_t i, uint32_t total_bits) {
  const uint64_t e = (uint64_t)(i + 1) * kSubBits;
  return (uint32_t)(e < total_bits ? e : total_bits);
}

__global__ __launch_bounds__(kWgSubs) void jdec_sync_kernel(DevStream D, Geom G, uint64_t* __restrict__ entry, uint64_t* __restrict__ exits,
                                                            uint64_t* __restrict__ cnt, uint64_t* __restrict__ bx, int nwg,
                                                            uint32_t* __restrict__ ctl, int launch, int cap) {
  if (ctl[kCtlStatus] != 0) return;
  if (launch > 0 && ctl[kCtlChanged + launch - 1] == 0) return;      // the launch before proved the fixed point
  __shared__ uint64_t sx[kWgSubs];
  __shared__ WgStage stage;
  const int t = threadIdx.x, j = blockIdx.x;
  const int64_t i = (int64_t)j * kWgSubs + t;
  const Ctx C = stage_ctx(D, G, ctl, stage);
  const uint32_t sub_end = sub_end_of(i, C.total_bits);
  uint64_t e, x = 0, c = 0;
  const bool active = (uint64_t)i * kSubBits < C.total_bits;        // a subsequence behind the data takes no part
  bool dirty = launch == 0;
  if (launch == 0) e = pack_state((uint32_t)(i * kSubBits), 0, 0);
  else { e = entry[i]; x = exits[i]; c = cnt[i]; }
  sx[t] = x;
  __syncthreads();
  int steps = 0;
  for (int step = 0; step < cap; ++step) {
    if (launch > 0 || step > 0) {
      uint64_t ne = e;
      if (t > 0) ne = sx[t - 1];
      else if (step == 0 && j > 0) ne = bx[(size_t)((launch - 1) & 1) * nwg + j - 1];
      if (active && ne != e) { e = ne; dirty = true; }
    }
    if (!__syncthreads_or(dirty ? 1 : 0)) break;
    if (dirty) {
      NullSink sink; uint32_t nbk = 0;
      x = decode_sub(C, e, sub_end, 0u, sink, &nbk);
      c = nbk; dirty = false;
      sx[t] = x;
    }
    __syncthreads();
    ++steps;
  }
  entry[i] = e; exits[i] = x; cnt[i] = c;
  if (t == kWgSubs - 1) bx[(size_t)(launch & 1) * nwg + j] = x;
  if (t == 0 && steps) { atomicOr(&ctl[kCtlChanged + launch], 1u); atomicMax(&ctl[kCtlRounds + launch], (uint32_t)steps); }
}

// ------------------------------------------------------------------------------------------------
// 3: the write pass
// ------------------------------------------------------------------------------------------------
struct DevSink {
  int16_t* coef; int64_t* dcd; uint32_t* status; uint32_t coef_blocks;
  uint32_t cached_g, pb, item;
  __device__ __forceinline__ void place(const Geom& G, uint32_t g) {
    if (g != cached_g) { block_place(G, g, &pb, &item); cached_g = g; }
  }
  __device__ __forceinline__ void dc(const Geom& G, uint32_t g, uint32_t, int diff) {
    place(G, g);
    if (item < coef_blocks) dcd[item] = diff;
  }
  __device__ __forceinline__ void ac(const Geom& G, uint32_t g, uint32_t k, int val) {
    place(G, g);
    if (pb < coef_blocks && k < 64) coef[(size_t)pb * 64 + dezigzag(k)] = (int16_t)val;
  }
  __device__ __forceinline__ void flag(uint32_t bits) { atomicOr(status, bits); }
};

__global__ __launch_bounds__(kWgSubs) void jdec_write_kernel(DevStream D, Geom G, const uint64_t* __restrict__ entry, const uint64_t* __restrict__ before,
                                                             int64_t nthreads, int16_t* __restrict__ coef, int64_t* __restrict__ dcd,
                                                             uint32_t* __restrict__ ctl) {
  if (declined(ctl)) return;
  __shared__ WgStage stage;
  const int64_t i = (int64_t)blockIdx.x * kWgSubs + threadIdx.x;
  const Ctx C = stage_ctx(D, G, ctl, stage);
  if (i >= nthreads) return;
  DevSink sink{coef, dcd, &ctl[kCtlLate], (uint32_t)G.coef_blocks, 0xffffffffu, 0u, 0u};
  uint32_t nbk = 0;
  decode_sub(C, entry[i], sub_end_of(i, C.total_bits), (uint32_t)before[i], sink, &nbk);
}

// ------------------------------------------------------------------------------------------------
// 4: DC predictors, result words
// ------------------------------------------------------------------------------------------------
__global__ void jdec_dc_kernel(Geom G, const uint64_t* __restrict__ pre, int16_t* __restrict__ coef, uint32_t* __restrict__ ctl) {
  if (declined(ctl)) return;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, nb = (uint32_t)G.coef_blocks;
  if (j >= nb) return;
  uint32_t pb, first;
  dc_item_place(G, j, &pb, &first);
  const int64_t pred = (int64_t)(pre[j + 1] - pre[first < nb ? first : 0]);
  if (pred < -65536 || pred > 65535) atomicOr(&ctl[kCtlLate], (uint32_t)kStDcRange);
  if (pb < nb) coef[(size_t)pb * 64] = (int16_t)pred;
}

__global__ void jdec_finish_kernel(const uint32_t* __restrict__ ctl, int32_t* __restrict__ result) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t status = ctl[kCtlStatus] | ctl[kCtlLate], rounds = 0, launches = 0;
  if (ctl[kCtlChanged + kSyncLaunches - 1] != 0) status |= kStNoSync;
  for (int l = 0; l < kSyncLaunches; ++l) { rounds += ctl[kCtlRounds + l]; launches += ctl[kCtlChanged + l] ? 1u : 0u; }
  result[2] = (int32_t)launches;
  result[0] = (int32_t)status;
  result[1] = (int32_t)rounds;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ovm_host_jpeg_decode_plan(const uint8_t* data, size_t n, int32_t max_rounds, OvmJpegDecPlan* plan, uint8_t* tables, int64_t tables_capacity) {
  return ovm_jpeg_dec::host_plan(data, n, max_rounds, plan, tables, tables_capacity);
}

int ovm_host_jpeg_entropy_emulate(const uint8_t* data, size_t n, int32_t max_rounds, int16_t* coef, int64_t coef_capacity, OvmJpegInfo* info,
                                  int32_t* status, int32_t* rounds, int32_t* launches) {
  return ovm_jpeg_dec::host_emulate(data, n, max_rounds, coef, coef_capacity, info, status, rounds, launches);
}

int ovm_jpeg_entropy_decode_workspace(const OvmJpegDecPlan* plan, int64_t* ws_bytes) {
  if (!plan || !ws_bytes || !plan_consistent(*plan)) return OVM_ERR_INVALID;
  *ws_bytes = layout(*plan).total;
  return OVM_OK;
}

int ovm_jpeg_entropy_decode(const uint8_t* stream, const uint8_t* tables, const OvmJpegDecPlan* plan, uint8_t* ws, int64_t ws_bytes,
                            int16_t* coef, int64_t coef_capacity, int32_t* result, ovm_stream_t stream_handle) {
  if (!stream || !tables || !plan || !ws || !coef || !result || !plan_consistent(*plan)) return OVM_ERR_INVALID;
  if (!aligned16(tables) || !aligned16(ws) || !aligned16(coef)) return OVM_ERR_INVALID;
  const OvmJpegDecPlan& P = *plan;
  const Layout L = layout(P);
  const int64_t nb = P.info.coef_blocks, n = P.ecs_bytes;
  if (ws_bytes < L.total || coef_capacity < nb * 64) return OVM_ERR_CAPACITY;
  const Geom G = geom(P);
  hipStream_t s = (hipStream_t)stream_handle;
  uint32_t* ctl = (uint32_t*)(ws + L.ctl);
  uint8_t* U = ws + L.stream;
  int64_t* dcd = (int64_t*)(ws + L.dcd);
  uint32_t* seg_off = (uint32_t*)(ws + L.seg_off);
  uint64_t* chunk_cnt = (uint64_t*)(ws + L.chunk_cnt);
  uint64_t* sub_cnt = (uint64_t*)(ws + L.sub_cnt);
  uint64_t* scan_out = (uint64_t*)(ws + L.scan_out);
  uint64_t* partial = (uint64_t*)(ws + L.partial);
  uint64_t* entry = (uint64_t*)(ws + L.entry);
  uint64_t* exits = (uint64_t*)(ws + L.exits);
  uint64_t* bx = (uint64_t*)(ws + L.boundary);
  if (hipMemsetAsync(ws + L.ctl, 0, (size_t)L.zero_bytes, s) != hipSuccess) return OVM_ERR_HIP;
  if (hipMemsetAsync(coef, 0, (size_t)nb * 128, s) != hipSuccess) return OVM_ERR_HIP;
  const unsigned cgrid = (unsigned)((L.nchunks + 255) / 256);
  hipLaunchKernelGGL(jdec_count_kernel, dim3(cgrid), dim3(256), 0, s, stream, n, L.nchunks, chunk_cnt);
  launch_scan(chunk_cnt, L.nchunks, partial, scan_out, s);
  hipLaunchKernelGGL(jdec_unstuff_kernel, dim3(cgrid), dim3(256), 0, s, stream, n, L.nchunks, (const uint64_t*)scan_out, (int)P.segments, U,
                     seg_off, ctl);
  DevStream D;
  D.words = (const uint32_t*)U; D.nwords = (uint32_t)L.nwords; D.seg_off = seg_off; D.tab = (const Tables*)tables;
  const int nwg = (int)L.nwg;
  for (int l = 0; l < kSyncLaunches; ++l)
    hipLaunchKernelGGL(jdec_sync_kernel, dim3(nwg), dim3(kWgSubs), 0, s, D, G, entry, exits, sub_cnt, bx, nwg, ctl, l, (int)P.max_rounds);
  const int64_t nthreads = L.nwg * kWgSubs;
  launch_scan(sub_cnt, nthreads, partial, scan_out, s);
  hipLaunchKernelGGL(jdec_write_kernel, dim3(nwg), dim3(kWgSubs), 0, s, D, G, (const uint64_t*)entry, (const uint64_t*)scan_out, nthreads, coef,
                     dcd, ctl);
  launch_scan((const uint64_t*)dcd, nb, partial, scan_out, s);
  hipLaunchKernelGGL(jdec_dc_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, G, (const uint64_t*)scan_out, coef, ctl);
  hipLaunchKernelGGL(jdec_finish_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)ctl, result);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
