// Picture writing on the device ("next" row 2 of SURVEY.md 8f, the encode half): a baseline JPEG produced in HBM.
//
// The reference writes its pictures with cv2.imwrite / Pillow's Image.save (demo/demo.py:117 <name>_combine.jpg, cubercnn/vis/vis.py:274
// the evaluation samples), i.e. with libjpeg-turbo at its defaults: JDCT_ISLOW, the Annex K tables scaled by the quality, 4:2:0, the
// standard Huffman tables, one interleaved scan. The encode needs no synchronisation of guessed states as the decode's entropy stage does (jpeg_dec.hip): colour transform, chroma
// downsampling, forward DCT and quantisation are integer arithmetic per 8 x 8 block, and Huffman coding becomes parallel once every
// block's bit length is known - an exclusive prefix sum gives each block its bit offset. So the finished uint8 picture never leaves
// the device; what crosses PCIe is the compressed file. The file is byte for byte the one Pillow writes (the live oracle of
// tests/test_gpu_jpeg_encode.py; tests/jpeg_enc_ref.py restates the same rules in numpy).
//
// The arithmetic is restated from the published algorithms of libjpeg-turbo 3.x, as jpeg.hip does for the inverse direction:
//   jccolor.c   rgb_ycc_convert  - Y / Cb / Cr from 16-bit fixed-point weights F(x) = (int)(x * 65536 + 0.5); Cb and Cr carry
//               (128 << 16) + 32767, Y carries 32768
//   jcprepct.c  edges - columns replicated to the right; input rows replicated down to a whole row group (2 rows at 4:2:0) only, the
//               picture downsampled, THEN the last downsampled row of each component replicated down to the iMCU height
//   jcsample.c  h2v2_downsample  - sum of the 2 x 2 cell plus a bias alternating 1, 2 along the output row, >> 2
//   jfdctint.c  jpeg_fdct_islow  - LL&M 13-bit fixed point on samples - 128: rows first (outputs 0 and 4 << 2, the others descaled by
//               11), then columns (0 and 4 descaled by 2, the others by 15)
//   jcdctmgr.c  quantisation     - sign(c) * ((|c| + (8 q >> 1)) / (8 q)), exact integer division
//   jccoefct.c  dummy blocks     - a block of an MCU beyond the component's ceil(samples / 8) blocks has zero AC and the DC of the
//               block before it in the MCU's block order
//   jchuff.c    encode_one_block - DC difference category + low bits (v - 1 for a negative v), (run, size) symbols, ZRL per 16 zeros,
//               EOB, 1-padding of the last byte, a 0x00 behind every 0xFF
// Kernels, all on the caller's stream, no read back to the host in between:
//   1 jenc_color_kernel   colour, padding and downsampling: the three padded planes (16 / 8 byte stores per lane)
//   2 jenc_fdct_kernel    one lane per block: FDCT, quantisation, dummy-block rule -> int16 planes in the decoder's layout
//   3 jenc_bitlen_kernel  one lane per block in scan order: its bit length; scan.hpp: exclusive prefix sum (64-bit offsets)
//   4 jenc_pack_kernel    one lane per block: its codes at its bit offset. A lane owns every word strictly inside its bit range and
//                         stores it; the first and the last word it shares with its neighbours, so those (zeroed by
//                         jenc_zero_edges_kernel) are merged with atomicOr - integer OR is order-independent: deterministic.
//                         (No LDS staging of a workgroup's run of blocks: the whole call is 0.10 ms of device time on a 1080 x 3000
//                         picture, bound by its thirteen launches - profiles/jpeg_encode/README.md.)
//   5 jenc_ffcount_kernel / scan.hpp / jenc_stuff_kernel: 0xFF bytes per 16-byte chunk, prefix sum, scatter with the stuffed
//                         zeros behind the header; padding bits, EOI and the file length (a device word)
// Scope: 8-bit baseline (SOF0), three components YCbCr, luma sampling 2x2 or 1x1, quality 1..100, sizes 1..65535. Out of scope
// (OVM_ERR_UNSUPPORTED / not offered): greyscale, 4:2:2 and 4:4:0, progressive and optimised-Huffman files, restart markers, custom
// tables, dpi / EXIF / ICC / comment segments, 12-bit samples.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/ovm3d.h"
#include "jpeg_enc_host.hpp"
#include "scan.hpp"

namespace {

using ovm_scan::kScanTile;
using ovm_scan::launch_scan;

struct EncDev {
  int width, height, hs;            // hs: luma sampling on both axes (1 or 2)
  int bw[3], bh[3], boff[3];
  int nbx, nby;                     // luma blocks that hold picture samples: ceil(width / 8), ceil(height / 8)
  int mcus_x, mcus_y, bpm;          // bpm: blocks per MCU (6 or 3)
  int nblocks;
  uint16_t qt[2][64];
};

struct EncHeader { uint8_t b[ovm_jpeg_enc::kHeaderLen + 1]; };

__constant__ ovm_jpeg_enc::EncTables d_enc_tables = ovm_jpeg_enc::build_tables();

#define OVM_FIX_0_298631336 2446
#define OVM_FIX_0_390180644 3196
#define OVM_FIX_0_541196100 4433
#define OVM_FIX_0_765366865 6270
#define OVM_FIX_0_899976223 7373
#define OVM_FIX_1_175875602 9633
#define OVM_FIX_1_501321110 12299
#define OVM_FIX_1_847759065 15137
#define OVM_FIX_1_961570560 16069
#define OVM_FIX_2_053119869 16819
#define OVM_FIX_2_562915447 20995
#define OVM_FIX_3_072711026 25172

// ------------------------------------------------------------------------------------------------
// 1: colour, padding, downsampling
// ------------------------------------------------------------------------------------------------
struct Ycc { int y, cb, cr; };

__device__ __forceinline__ Ycc rgb_ycc(const uint8_t* __restrict__ p, int64_t sc) {
  const int r = p[0], g = p[sc], b = p[2 * sc];
  Ycc o;
  o.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  o.cb = (-11058 * r - 21710 * g + 32768 * b + (128 << 16) + 32767) >> 16;   // the negative weights are -F(.168735892), -F(.331264108)
  o.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;     // -F(.418687589), -F(.081312411)
  return o;
}

// one lane per 8 chroma samples of one chroma row (at 4:4:4: 8 pixels of one row); grid (ceil(mcus_x / 64), mcus_y * 8)
__global__ __launch_bounds__(64) void jenc_color_kernel(const uint8_t* __restrict__ img, int64_t sy, int64_t sx, int64_t sc, EncDev J,
                                                        uint8_t* __restrict__ planes) {
  const int mx = blockIdx.x * blockDim.x + threadIdx.x, cy = blockIdx.y;
  if (mx >= J.mcus_x) return;
  const int W = J.width, H = J.height;
  uint8_t* p0 = planes;
  uint8_t* p1 = planes + (size_t)J.boff[1] * 64 + ((size_t)cy * J.bw[1] + mx) * 8;
  uint8_t* p2 = planes + (size_t)J.boff[2] * 64 + ((size_t)cy * J.bw[2] + mx) * 8;
  unsigned cbw[2] = {0, 0}, crw[2] = {0, 0};
  if (J.hs == 1) {
    const uint8_t* row = img + (int64_t)(cy < H ? cy : H - 1) * sy;
    unsigned yw[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int x = mx * 8 + j;
      const Ycc v = rgb_ycc(row + (int64_t)(x < W ? x : W - 1) * sx, sc);
      yw[j >> 2] |= (unsigned)v.y << (8 * (j & 3));
      cbw[j >> 2] |= (unsigned)v.cb << (8 * (j & 3));
      crw[j >> 2] |= (unsigned)v.cr << (8 * (j & 3));
    }
    *(uint2*)(p0 + ((size_t)cy * J.bw[0] + mx) * 8) = make_uint2(yw[0], yw[1]);
  } else {
    const int crows = (H + 1) >> 1;                                   // downsampled rows that exist; the last one is replicated below
    const int cyr = cy < crows ? cy : crows - 1;
    int cb[8], cr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cb[j] = cr[j] = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ly = 2 * cy + r, csy = 2 * cyr + r;
      const int ysrc = ly < H ? ly : H - 1, csrc = csy < H ? csy : H - 1;
      const uint8_t* yrow = img + (int64_t)ysrc * sy;
      const uint8_t* crow = img + (int64_t)csrc * sy;
      unsigned yw[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int x = mx * 16 + j;
        const int64_t xo = (int64_t)(x < W ? x : W - 1) * sx;
        Ycc v = rgb_ycc(yrow + xo, sc);
        yw[j >> 2] |= (unsigned)v.y << (8 * (j & 3));
        if (csrc != ysrc) v = rgb_ycc(crow + xo, sc);
        cb[j >> 1] += v.cb; cr[j >> 1] += v.cr;
      }
      *(uint4*)(p0 + ((size_t)ly * J.bw[0] + (size_t)mx * 2) * 8) = make_uint4(yw[0], yw[1], yw[2], yw[3]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int bias = 1 + (j & 1);                                  // mx * 8 is even: the bias alternates from 1 at the row's start
      cbw[j >> 2] |= (unsigned)((cb[j] + bias) >> 2) << (8 * (j & 3));
      crw[j >> 2] |= (unsigned)((cr[j] + bias) >> 2) << (8 * (j & 3));
    }
  }
  *(uint2*)p1 = make_uint2(cbw[0], cbw[1]);
  *(uint2*)p2 = make_uint2(crw[0], crw[1]);
}

// ------------------------------------------------------------------------------------------------
// 2: forward DCT, quantisation, dummy blocks
// ------------------------------------------------------------------------------------------------
// one 1-D pass of jpeg_fdct_islow; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int* d, int* o) {
  int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
  if (FIRST) { o[0] = (tmp10 + tmp11) << 2; o[4] = (tmp10 - tmp11) << 2; }
  else { o[0] = (tmp10 + tmp11 + 2) >> 2; o[4] = (tmp10 - tmp11 + 2) >> 2; }
  int z1 = (tmp12 + tmp13) * OVM_FIX_0_541196100;
  o[2] = (z1 + tmp13 * OVM_FIX_0_765366865 + R) >> N;
  o[6] = (z1 + tmp12 * (-OVM_FIX_1_847759065) + R) >> N;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * OVM_FIX_1_175875602;
  tmp4 *= OVM_FIX_0_298631336; tmp5 *= OVM_FIX_2_053119869; tmp6 *= OVM_FIX_3_072711026; tmp7 *= OVM_FIX_1_501321110;
  z1 *= -OVM_FIX_0_899976223; z2 *= -OVM_FIX_2_562915447; z3 *= -OVM_FIX_1_961570560; z4 *= -OVM_FIX_0_390180644;
  z3 += z5; z4 += z5;
  o[7] = (tmp4 + z1 + z3 + R) >> N;
  o[5] = (tmp5 + z2 + z4 + R) >> N;
  o[3] = (tmp6 + z2 + z3 + R) >> N;
  o[1] = (tmp7 + z1 + z4 + R) >> N;
}

// one lane per block of the coefficient planes. A dummy block transforms the block whose DC it repeats and drops the AC part.
__global__ __launch_bounds__(64) void jenc_fdct_kernel(const uint8_t* __restrict__ planes, EncDev J, int16_t* __restrict__ coef) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= J.nblocks) return;
  const int c = b >= J.boff[2] ? 2 : (b >= J.boff[1] ? 1 : 0);
  const int lb = b - J.boff[c];
  const int by = lb / J.bw[c], bx = lb - by * J.bw[c];
  int sby = by, sbx = bx;
  bool dummy = false;
  if (c == 0) {                                                     // only the luma plane of 4:2:0 can hold dummy blocks
    if (by >= J.nby) { dummy = true; sby = by - 1; sbx = bx | 1; }  // a dummy row: the DC of the MCU's last block of the row above
    else if (bx >= J.nbx) { dummy = true; }
    if (sbx >= J.nbx) sbx -= 1;                                      // right of a real row: the DC of the block before
  }
  const uint16_t* q = J.qt[c ? 1 : 0];
  const size_t stride = (size_t)J.bw[c] * 8;
  const uint8_t* src = planes + (size_t)J.boff[c] * 64 + (size_t)sby * 8 * stride + (size_t)sbx * 8;
  int ws[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 v = *(const uint2*)(src + (size_t)r * stride);
    int d[8], o[8];
#pragma unroll
    for (int x = 0; x < 4; ++x) { d[x] = (int)((v.x >> (8 * x)) & 255) - 128; d[4 + x] = (int)((v.y >> (8 * x)) & 255) - 128; }
    fdct_1d<true>(d, o);
#pragma unroll
    for (int x = 0; x < 8; ++x) ws[r * 8 + x] = o[x];
  }
  int out[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[r * 8 + col];
    fdct_1d<false>(d, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = r * 8 + col;
      const unsigned div = 8u * q[i];
      const int v = o[r];
      const unsigned a = ((unsigned)(v < 0 ? -v : v) + (div >> 1)) / div;
      out[i] = v < 0 ? -(int)a : (int)a;
    }
  }
  uint4* dst = (uint4*)(coef + (size_t)b * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lo = (dummy && (i | j)) ? 0 : out[i * 8 + 2 * j], hi = dummy ? 0 : out[i * 8 + 2 * j + 1];
      w[j] = ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16);
    }
    dst[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ------------------------------------------------------------------------------------------------
// 3 / 4: Huffman coding of one block, into a bit counter or into the bit stream
// ------------------------------------------------------------------------------------------------
// block s of the interleaved scan: its place in the coefficient planes, its table, and the block that holds its DC predictor
__device__ __forceinline__ void scan_block(const EncDev& J, int s, int* pb, int* tab, int* prev_pb) {
  const int m = s / J.bpm, k = s - m * J.bpm;
  if (J.hs == 2 && k < 4) {
    const int my = m / J.mcus_x, mx = m - my * J.mcus_x;
    const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
    *pb = by * J.bw[0] + bx; *tab = 0;
    if (k == 0) *prev_pb = m > 0 ? (mx > 0 ? (by + 1) * J.bw[0] + bx - 1 : (by - 1) * J.bw[0] + J.bw[0] - 1) : -1;   // Y11 of the MCU before
    else *prev_pb = k == 2 ? (by - 1) * J.bw[0] + bx + 1 : *pb - 1;                                                  // Y10 follows Y01
    return;
  }
  const int c = J.hs == 2 ? k - 3 : k;
  *pb = J.boff[c] + m; *tab = c ? 1 : 0;
  *prev_pb = m > 0 ? *pb - 1 : -1;
}

struct LenSink {
  unsigned n = 0;
  __device__ __forceinline__ void put(unsigned, int len) { n += (unsigned)len; }
};

// bits arrive most significant first; a word leaves byte-swapped so that the stream is big-endian in memory
struct BitSink {
  uint32_t* w;
  uint64_t acc;
  int n;
  bool first;
  __device__ __forceinline__ void put(unsigned code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t v = __builtin_bswap32((uint32_t)(acc >> n));
      if (first) { atomicOr(w, v); first = false; } else *w = v;
      ++w;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - n))));
  }
};

template <class Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ blk, int prev_dc, int tab, Sink& out) {
  int in[64];
  const uint4* src = (const uint4*)blk;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = src[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { in[i * 8 + 2 * j] = (int)(int16_t)(w[j] & 0xffff); in[i * 8 + 2 * j + 1] = (int)(int16_t)(w[j] >> 16); }
  }
  {
    const int diff = in[0] - prev_dc;
    const int a = diff < 0 ? -diff : diff;
    const int cat = 32 - __clz(a);                                   // __clz(0) = 32
    const unsigned e = d_enc_tables.dc[tab][cat];
    const unsigned low = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
    out.put(((e >> 8) << cat) | low, (int)(e & 255) + cat);
  }
  const unsigned zrl = d_enc_tables.ac[tab][0xf0], eob = d_enc_tables.ac[tab][0];
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const int v = in[zz[k]];
    if (v == 0) { ++run; continue; }
    while (run > 15) { out.put(zrl >> 8, (int)(zrl & 255)); run -= 16; }
    const int a = v < 0 ? -v : v;
    const int size = 32 - __clz(a);
    const unsigned e = d_enc_tables.ac[tab][(run << 4) | size];
    const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    out.put(((e >> 8) << size) | low, (int)(e & 255) + size);
    run = 0;
  }
  if (run > 0) out.put(eob >> 8, (int)(eob & 255));
}

__global__ __launch_bounds__(64) void jenc_bitlen_kernel(const int16_t* __restrict__ coef, EncDev J, uint32_t* __restrict__ blen) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= J.nblocks) return;
  int pb, tab, prev;
  scan_block(J, s, &pb, &tab, &prev);
  const int prev_dc = prev >= 0 ? (int)coef[(size_t)prev * 64] : 0;
  LenSink sink;
  encode_block(coef + (size_t)pb * 64, prev_dc, tab, sink);
  blen[s] = sink.n;
}

// the words two blocks share start out as zero (n + 1 offsets: the last one is the end of the stream)
__global__ void jenc_zero_edges_kernel(const uint64_t* __restrict__ boff, int n, uint32_t* __restrict__ words) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n) words[boff[s] >> 5] = 0;
}

__global__ __launch_bounds__(64) void jenc_pack_kernel(const int16_t* __restrict__ coef, EncDev J, const uint64_t* __restrict__ boff,
                                                       uint32_t* __restrict__ words) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= J.nblocks) return;
  int pb, tab, prev;
  scan_block(J, s, &pb, &tab, &prev);
  const int prev_dc = prev >= 0 ? (int)coef[(size_t)prev * 64] : 0;
  const uint64_t off = boff[s];
  BitSink sink;
  sink.w = words + (off >> 5); sink.acc = 0; sink.n = (int)(off & 31); sink.first = true;
  encode_block(coef + (size_t)pb * 64, prev_dc, tab, sink);
  sink.finish();
}

// ------------------------------------------------------------------------------------------------
// 5: byte stuffing, header, EOI, length
// ------------------------------------------------------------------------------------------------
// chunk i of the unstuffed stream (16 bytes) with the 1-padding of the last byte applied; returns how many of its bytes exist
__device__ __forceinline__ int load_chunk(const uint8_t* __restrict__ bits, uint64_t total_bits, int64_t i, uint8_t* b) {
  const uint64_t nbytes = (total_bits + 7) >> 3;
  const uint64_t base = (uint64_t)i * 16;
  if (base >= nbytes) return 0;
  const uint4 v = *(const uint4*)(bits + base);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  const int n = nbytes - base < 16 ? (int)(nbytes - base) : 16;
  const int tail = (int)(total_bits & 7);
  if (tail && base + 16 >= nbytes) {
    const uint8_t pad = (uint8_t)((1u << (8 - tail)) - 1u);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j == n - 1) b[j] |= pad;
  }
  return n;
}

__global__ void jenc_ffcount_kernel(const uint8_t* __restrict__ bits, const uint64_t* __restrict__ total_bits, int64_t nchunks,
                                    uint32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nchunks) return;
  uint8_t b[16];
  const int n = load_chunk(bits, *total_bits, i, b);
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) c += (j < n && b[j] == 0xff) ? 1u : 0u;
  cnt[i] = c;
}

__global__ void jenc_stuff_kernel(const uint8_t* __restrict__ bits, const uint64_t* __restrict__ total_bits, int64_t nchunks,
                                  const uint64_t* __restrict__ ffoff, EncHeader hdr, int header_len, uint8_t* __restrict__ out,
                                  int64_t* __restrict__ out_len) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t k = i; k < header_len; k += (int64_t)gridDim.x * blockDim.x) out[k] = hdr.b[k];
  if (i >= nchunks) return;
  const uint64_t tb = *total_bits;
  if (i == 0) {
    const uint64_t end = (uint64_t)header_len + ((tb + 7) >> 3) + ffoff[nchunks];
    out[end] = 0xff; out[end + 1] = 0xd9;
    *out_len = (int64_t)(end + 2);
  }
  uint8_t b[16];
  const int n = load_chunk(bits, tb, i, b);
  if (n == 0) return;
  uint8_t* o = out + header_len + (uint64_t)i * 16 + ffoff[i];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < n) {
      *o++ = b[j];
      if (b[j] == 0xff) *o++ = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct EncLayout {
  int64_t planes, coef, blen, boff, partial, bits, ffcnt, ffoff, total;   // byte offsets into the workspace; total = its size
  int64_t nchunks, bits_bytes;
};

EncLayout enc_layout(const OvmJpegEncInfo& I) {
  EncLayout L;
  const int64_t nb = I.coef_blocks;
  L.bits_bytes = align16(208 * nb + 16);                       // a block emits at most 1660 bits < 208 bytes; + the end-of-stream word
  L.nchunks = L.bits_bytes / 16;
  int64_t o = 0;
  L.planes = o; o += align16(nb * 64);
  L.coef = o; o += align16(nb * 128);
  L.blen = o; o += align16(nb * 4);
  L.boff = o; o += align16((nb + 1) * 8);
  L.partial = o; o += align16(((L.nchunks + kScanTile - 1) / kScanTile + 1) * 8);
  L.bits = o; o += L.bits_bytes;
  L.ffcnt = o; o += align16(L.nchunks * 4);
  L.ffoff = o; o += align16((L.nchunks + 1) * 8);
  L.total = o;
  return L;
}

void fill_dev(const OvmJpegEncInfo& I, EncDev* J) {
  memset(J, 0, sizeof(*J));
  J->width = I.width; J->height = I.height; J->hs = I.hs;
  int off = 0;
  for (int c = 0; c < 3; ++c) { J->bw[c] = I.bw[c]; J->bh[c] = I.bh[c]; J->boff[c] = off; off += I.bw[c] * I.bh[c]; }
  J->nbx = (I.width + 7) / 8; J->nby = (I.height + 7) / 8;
  J->mcus_x = I.mcus_x; J->mcus_y = I.mcus_y; J->bpm = I.hs * I.vs + 2;
  J->nblocks = off;
  memcpy(J->qt, I.qt, sizeof(J->qt));
}

void launch_forward(const uint8_t* img, int64_t sy, int64_t sx, int64_t sc, const EncDev& J, uint8_t* planes, int16_t* coef, hipStream_t s) {
  hipLaunchKernelGGL(jenc_color_kernel, dim3((J.mcus_x + 63) / 64, J.mcus_y * 8), dim3(64), 0, s, img, sy, sx, sc, J, planes);
  hipLaunchKernelGGL(jenc_fdct_kernel, dim3((J.nblocks + 63) / 64), dim3(64), 0, s, (const uint8_t*)planes, J, coef);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ovm_host_jpeg_encode_plan(int32_t width, int32_t height, int32_t quality, int32_t subsampling, OvmJpegEncInfo* info, uint8_t* header,
                              int32_t header_capacity) {
  return ovm_jpeg_enc::host_plan(width, height, quality, subsampling, info, header, header_capacity);
}

int ovm_jpeg_encode_workspace(const OvmJpegEncInfo* info, int64_t* ws_bytes, int64_t* out_capacity) {
  if (!info || !ovm_jpeg_enc::info_consistent(*info)) return OVM_ERR_INVALID;
  if (ws_bytes) *ws_bytes = enc_layout(*info).total;
  if (out_capacity) *out_capacity = (int64_t)info->header_len + 416 * (int64_t)info->coef_blocks + 16;
  return OVM_OK;
}

int ovm_jpeg_forward(const uint8_t* img, int64_t sy, int64_t sx, int64_t sc, const OvmJpegEncInfo* info, uint8_t* ws, int64_t ws_bytes,
                     int16_t* coef, ovm_stream_t stream) {
  if (!img || !info || !ws || !coef || !ovm_jpeg_enc::info_consistent(*info) || !aligned16(ws) || !aligned16(coef)) return OVM_ERR_INVALID;
  if (ws_bytes < (int64_t)info->coef_blocks * 64) return OVM_ERR_CAPACITY;
  EncDev J;
  fill_dev(*info, &J);
  launch_forward(img, sy, sx, sc, J, ws, coef, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

int ovm_jpeg_encode(const uint8_t* img, int64_t sy, int64_t sx, int64_t sc, const OvmJpegEncInfo* info, const uint8_t* header, uint8_t* ws,
                    int64_t ws_bytes, uint8_t* out, int64_t out_capacity, int64_t* out_len, ovm_stream_t stream) {
  if (!img || !info || !header || !ws || !out || !out_len || !ovm_jpeg_enc::info_consistent(*info) || !aligned16(ws)) return OVM_ERR_INVALID;
  const OvmJpegEncInfo& I = *info;
  const EncLayout L = enc_layout(I);
  if (ws_bytes < L.total || out_capacity < (int64_t)I.header_len + 416 * (int64_t)I.coef_blocks + 16) return OVM_ERR_CAPACITY;
  EncDev J;
  fill_dev(I, &J);
  EncHeader hdr;
  memset(&hdr, 0, sizeof(hdr));
  memcpy(hdr.b, header, (size_t)I.header_len);
  hipStream_t s = (hipStream_t)stream;
  int16_t* coef = (int16_t*)(ws + L.coef);
  uint32_t* blen = (uint32_t*)(ws + L.blen);
  uint64_t* boff = (uint64_t*)(ws + L.boff);
  uint64_t* partial = (uint64_t*)(ws + L.partial);
  uint8_t* bits = ws + L.bits;
  uint32_t* ffcnt = (uint32_t*)(ws + L.ffcnt);
  uint64_t* ffoff = (uint64_t*)(ws + L.ffoff);
  const int nb = J.nblocks;
  launch_forward(img, sy, sx, sc, J, ws + L.planes, coef, s);
  hipLaunchKernelGGL(jenc_bitlen_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, (const int16_t*)coef, J, blen);
  launch_scan(blen, nb, partial, boff, s);
  hipLaunchKernelGGL(jenc_zero_edges_kernel, dim3((nb + 256) / 256), dim3(256), 0, s, (const uint64_t*)boff, nb, (uint32_t*)bits);
  hipLaunchKernelGGL(jenc_pack_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, (const int16_t*)coef, J, (const uint64_t*)boff, (uint32_t*)bits);
  const unsigned cgrid = (unsigned)((L.nchunks + 255) / 256);
  hipLaunchKernelGGL(jenc_ffcount_kernel, dim3(cgrid), dim3(256), 0, s, (const uint8_t*)bits, (const uint64_t*)(boff + nb), L.nchunks, ffcnt);
  launch_scan(ffcnt, L.nchunks, partial, ffoff, s);
  hipLaunchKernelGGL(jenc_stuff_kernel, dim3(cgrid), dim3(256), 0, s, (const uint8_t*)bits, (const uint64_t*)(boff + nb), L.nchunks,
                     (const uint64_t*)ffoff, hdr, (int)I.header_len, out, out_len);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // extern "C"
