// Core of the parallel JPEG Huffman decode (jpeg_dec.hip on the device, jpeg_dec_host.hpp as its serial emulation): one
// subsequence of the unstuffed entropy-coded stream decoded from a state, with or without writing. __host__ __device__, no HIP
// runtime, so that the CPU emulation and the sanitizer fuzz (scratch/fuzz_jpeg_dec.cpp) run exactly the code the kernels run.
//
// The stream is the scan's entropy-coded segment with the stuffed zeros and the RSTn markers taken out (stage 1), zero-padded, as
// big-endian bits; seg_off[s] is the byte at which restart segment s starts in it. A state is (bit position, block within the
// MCU, zig-zag index k; k = 0: the DC symbol is next). Decoding rules are the host decoder's (jpeg_host.hpp), symbol for symbol:
// the 9-bit fast table, then the canonical search over 10..16 bits; DC category <= 11; ZRL may run past 63 and ends the block,
// a coefficient at k > 63 is an error. What the host calls an error makes this routine ABANDON the block: it moves on to the next
// segment's first bit, or to the end of its subsequence if that comes first, in the state "start of an MCU" and without counting
// the block. A block counts as completed only if its last bit lies inside
// its segment (the host's BitReader::exhausted rule). So a segment that the host refuses completes fewer blocks than the frame
// needs, and the one check "every segment completed exactly its blocks" (the write pass, at every segment crossing) covers
// invalid codes, k > 63 and cut data at once; what follows a segment's last block (padding bits) cannot reach the planes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OVM_JD_HD __host__ __device__ __forceinline__
#else
#define OVM_JD_HD inline
#endif

namespace ovm_jpeg_dec {

constexpr int kSubBits = 512;          // bits per subsequence (one thread)
constexpr int kWgSubs = 256;           // subsequences per workgroup
constexpr int kSyncLaunches = 6;       // synchronisation launches enqueued per call (the last productive one must be followed by a clean one)
constexpr int kDefaultMaxRounds = 256; // relaxation steps per workgroup per launch: = kWgSubs, the count at which a workgroup is certainly consistent
constexpr int64_t kMaxStreamBytes = (int64_t)1 << 26;

// status word (0 = the planes are proven equal to the host decoder's)
enum : uint32_t {
  kStMarker = 1,      // an 0xFF followed by neither 0x00 nor the RSTn that is due; a marker beyond the expected count
  kStSegments = 2,    // number of restart segments differs from the frame's, or an empty segment
  kStNoSync = 4,      // the entry states were still changing when the launches / rounds ran out
  kStCount = 8,       // a segment completed another number of blocks than the frame needs (cut data, trailing data, a refused block)
  kStBadCode = 16,    // an invalid Huffman code or a DC category > 11 inside the blocks the frame needs
  kStZigzag = 32,     // a coefficient at zig-zag index > 63 inside the blocks the frame needs
  kStDcRange = 64,    // a DC predictor outside [-65536, 65535]
};

struct HuffLut {
  uint16_t fast[512];                  // (length << 8) | symbol for codes of <= 9 bits, 0 = longer
  // codes of 10..16 bits, index l - 10 (index 7 unused). limit[l - 10] = max over l' <= l of (maxcode[l'] + 1) << (16 - l'): the
  // host's search "first l with (code >> (16 - l)) <= maxcode[l]" finds the first l whose own bound exceeds the 16-bit window,
  // which is the first l whose running maximum does - so the length is 10 + the number of limits the window has reached, seven
  // comparisons on two 16-byte reads instead of a loop of dependent ones.
  uint32_t limit[8];
  int32_t mincode[8], valptr[8];
  uint8_t vals[256];
};
struct Tables { HuffLut dc[4], ac[4]; };

struct Geom {
  int32_t ncomp, bpm, mcus_x, mcus, restart, nseg, coef_blocks;    // restart: MCUs per segment (= mcus when the file has no DRI)
  // The state's block index runs modulo bperiod, the period of the (DC, AC) table pairs along the MCU's blocks: all it is for is
  // choosing tables (the write pass places a block by its count g). Where every component uses one pair (RGB files) it is 1, and
  // guessed states fall in step on (bit, k) alone; with the index modulo bpm they never would, the tables telling them nothing.
  int32_t bperiod;
  int32_t h[3], v[3], bw[3], plane_off[3];
  uint8_t sel_comp[8], sel_sub[8], sel_dc[8], sel_ac[8];           // per block of the MCU: component, index within the component's h x v, tables
};

struct Ctx {
  const uint32_t* words;               // the unstuffed stream, as stored (big-endian bit order within bytes), zero behind total_bits:
  uint32_t word_base, nlocal;          // words[0 .. nlocal) hold words word_base .. of the stream (the kernels stage their share in LDS)
  uint32_t nwords;                     // words of the whole zero-padded stream
  uint32_t total_bits;
  const uint32_t* seg_off;             // [nseg] byte offsets of the segments' first bytes; segment nseg - 1 ends at total_bits
  const Tables* tab;
  const Geom* g;                       // (the kernels keep it in LDS: indexed by the block of the MCU at every symbol)
};

// Stage 1, per byte of the entropy-coded segment (prev / next: -1 outside it): what becomes of it in the unstuffed stream.
// An 0xFF is data when a stuffed 0x00 follows and the first byte of a restart marker when 0xD0..0xD7 follows; the byte behind an
// 0xFF is dropped either way. Anything else behind an 0xFF is not for this route.
enum : uint32_t { kByteKeep = 1, kByteMarker = 2, kByteAnomaly = 4 };
OVM_JD_HD uint32_t classify_byte(int prev, int cur, int next) {
  if (prev == 0xFF) return 0;
  if (cur != 0xFF) return kByteKeep;
  if (next == 0x00) return kByteKeep;
  if (next >= 0xD0 && next <= 0xD7) return kByteMarker;
  return kByteKeep | kByteAnomaly;
}
constexpr int kChunkBytes = 32;        // stage 1: bytes per thread

// control words in front of the workspace
// kCtlStatus is written by stage 1 only and kCtlChanged[l] by synchronisation launch l only, so every later launch that decides on
// them reads words no workgroup of its own launch writes; what the write pass and the DC kernel find goes to kCtlLate, which only
// the finish kernel reads.
enum : int { kCtlStatus = 0, kCtlChanged = 1, kCtlRounds = 1 + kSyncLaunches, kCtlTotalBytes = 1 + 2 * kSyncLaunches, kCtlLate = 2 + 2 * kSyncLaunches,
             kCtlWords = 16 };
static_assert(kCtlLate < kCtlWords, "control block");

OVM_JD_HD uint64_t pack_state(uint32_t p, uint32_t b, uint32_t k) { return ((uint64_t)p << 16) | ((uint64_t)(b & 7) << 8) | (k & 63); }
OVM_JD_HD uint32_t state_pos(uint64_t s) { return (uint32_t)(s >> 16); }

OVM_JD_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// the 32 bits that start at bit p; reads are clamped to the (zero) last word of the stream, and to the words held
OVM_JD_HD uint32_t window(const Ctx& C, uint32_t p) {
  const uint32_t last = C.nwords - 1, llast = C.nlocal - 1;
  const uint32_t wi = p >> 5;
  uint32_t i0 = (wi < last ? wi : last) - C.word_base, i1 = (wi + 1 < last ? wi + 1 : last) - C.word_base;
  i0 = i0 < llast ? i0 : llast; i1 = i1 < llast ? i1 : llast;
  const uint64_t v = ((uint64_t)bswap32(C.words[i0]) << 32) | bswap32(C.words[i1]);
  return (uint32_t)((v << (p & 31)) >> 32);
}

OVM_JD_HD uint32_t seg_end_bits(const Ctx& C, uint32_t seg) {
  return seg + 1 < (uint32_t)C.g->nseg ? C.seg_off[seg + 1] * 8u : C.total_bits;
}

// how many blocks segment seg must have completed when it ends, counted from the start of the scan
OVM_JD_HD uint32_t seg_block_limit(const Geom& g, uint32_t seg) {
  const uint64_t m = (uint64_t)(seg + 1) * (uint32_t)g.restart;
  return (uint32_t)(m < (uint64_t)g.mcus ? m : (uint64_t)g.mcus) * (uint32_t)g.bpm;
}

// the segment that holds bit p (p < total_bits): the last one that starts at or before it
OVM_JD_HD uint32_t find_segment(const Ctx& C, uint32_t p) {
  uint32_t lo = 0, hi = (uint32_t)C.g->nseg;            // seg_off[lo] * 8 <= p < seg_off[hi] * 8
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (C.seg_off[mid] * 8u <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// returns length << 8 | symbol, 0 for no code (the host's decode_symbol)
OVM_JD_HD uint32_t lookup(const HuffLut& h, uint32_t w) {
  const uint32_t f = h.fast[w >> 23];
  if (f) return f;
  const uint32_t code = w >> 16;
  uint32_t n = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 7; ++i) n += code >= h.limit[i] ? 1u : 0u;
  if (n >= 7) return 0;
  const uint32_t l = 10 + n;
  const int c = (int)(code >> (16 - l));
  if (c < h.mincode[n]) return 0;
  return (l << 8) | h.vals[(h.valptr[n] + c - h.mincode[n]) & 255];
}

OVM_JD_HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// A sink receives what a subsequence decodes. g: blocks completed since the start of the scan (meaningful in the write pass only).
struct NullSink {
  OVM_JD_HD void dc(const Geom&, uint32_t, uint32_t, int) {}
  OVM_JD_HD void ac(const Geom&, uint32_t, uint32_t, int) {}
  OVM_JD_HD void flag(uint32_t) {}
};

// Decodes from `entry` until the position reaches sub_end (<= total_bits). gbase: blocks completed before this subsequence.
// Returns the exit state; *nblocks = blocks completed here. Every iteration consumes at least one bit or leaves a segment, and a
// segment that is left has at least 8 bits (empty ones are refused in stage 1), hence the iteration bound.
template <class Sink>
OVM_JD_HD uint64_t decode_sub(const Ctx& C, uint64_t entry, uint32_t sub_end, uint32_t gbase, Sink& sink, uint32_t* nblocks) {
  const Geom& G = *C.g;
  uint32_t p = state_pos(entry), b = (uint32_t)(entry >> 8) & 7, k = (uint32_t)entry & 63;
  uint32_t g = gbase;
  if (b >= (uint32_t)G.bperiod) b = 0;
  if (p >= C.total_bits || p >= sub_end) { *nblocks = 0; return entry; }
  uint32_t seg = find_segment(C, p), seg_end = seg_end_bits(C, seg), lim = seg_block_limit(G, seg);
  const HuffLut* hd = &C.tab->dc[G.sel_dc[b] & 3];      // the tables of block b: looked up when b changes, not at every symbol
  const HuffLut* ha = &C.tab->ac[G.sel_ac[b] & 3];
  constexpr int kMaxIter = kSubBits + kSubBits / 8 + 8;
  int it = 0;
  for (; it < kMaxIter && p < sub_end; ++it) {
    bool leave = p >= seg_end, done = false;
    uint32_t bad = 0;
    if (!leave) {
      // one path for the DC symbol (k = 0: run 0, size = the category) and the AC symbols
      const uint32_t w = window(C, p);
      const bool isdc = k == 0;
      const uint32_t f = lookup(isdc ? *hd : *ha, w);
      const uint32_t len = f >> 8, sym = f & 255, r = isdc ? 0u : sym >> 4, sz = isdc ? sym : (sym & 15);
      if (!f || (isdc && sym > 11)) bad = kStBadCode;
      else if (!isdc && sz == 0) {
        p += len;
        if (r == 15) { k += 16; done = k > 63; } else done = true;
      } else if (k + r > 63) bad = kStZigzag;
      else {
        k += r;
        const int val = sz ? extend((int)((w << len) >> (32 - sz)), (int)sz) : 0;
        p += len + sz;
        if (g < lim) {
          if (isdc) sink.dc(G, g, b, val); else sink.ac(G, g, k, val);
        }
        ++k;
        done = k > 63;
      }
      if (bad) {
        if (g < lim) sink.flag(bad);
        // a guessed entry state often ends here; leaving with the next subsequence's own guess keeps what was decoded behind it
        if (seg_end > sub_end) { p = sub_end; b = 0; k = 0; break; }
        leave = true;
      } else {
        if (done) {
          if (p <= seg_end) {
            ++g; b = b + 1 >= (uint32_t)G.bperiod ? 0 : b + 1;
            hd = &C.tab->dc[G.sel_dc[b] & 3]; ha = &C.tab->ac[G.sel_ac[b] & 3];
          }
          k = 0;
        }
        leave = p >= seg_end;
      }
    }
    if (leave) {
      if (g != lim) sink.flag(kStCount);
      p = seg_end; b = 0; k = 0;
      hd = &C.tab->dc[G.sel_dc[0] & 3]; ha = &C.tab->ac[G.sel_ac[0] & 3];
      ++seg;
      if (seg >= (uint32_t)G.nseg) break;                  // p = total_bits >= sub_end
      seg_end = seg_end_bits(C, seg); lim = seg_block_limit(G, seg);
    }
  }
  if (it >= kMaxIter && p < sub_end) { p = sub_end; b = 0; k = 0; }   // only behind empty segments, which stage 1 refuses
  *nblocks = g - gbase;
  return pack_state(p, b, k);
}

// where block g of the scan lives: its block in the coefficient planes, and its place in the component-major list of DC differences
OVM_JD_HD void block_place(const Geom& G, uint32_t g, uint32_t* plane_block, uint32_t* dc_item) {
  const uint32_t m = g / (uint32_t)G.bpm, bb = (g - m * (uint32_t)G.bpm) & 7;
  const uint32_t c = G.sel_comp[bb] < 3 ? G.sel_comp[bb] : 0, sub = G.sel_sub[bb];
  const uint32_t my = m / (uint32_t)G.mcus_x, mx = m - my * (uint32_t)G.mcus_x;
  const uint32_t hc = (uint32_t)G.h[c], vc = (uint32_t)G.v[c];
  const uint32_t by = my * vc + sub / hc, bx = mx * hc + sub % hc;
  *plane_block = (uint32_t)G.plane_off[c] + by * (uint32_t)G.bw[c] + bx;
  *dc_item = (uint32_t)G.plane_off[c] + m * hc * vc + sub;
}

// item j of the component-major DC list: its plane block and the item at which its restart segment starts
OVM_JD_HD void dc_item_place(const Geom& G, uint32_t j, uint32_t* plane_block, uint32_t* seg_first) {
  const uint32_t c = (G.ncomp == 3 && j >= (uint32_t)G.plane_off[2]) ? 2 : ((G.ncomp == 3 && j >= (uint32_t)G.plane_off[1]) ? 1 : 0);
  const uint32_t hc = (uint32_t)G.h[c], vc = (uint32_t)G.v[c], hv = hc * vc;
  const uint32_t t = j - (uint32_t)G.plane_off[c], m = t / hv, sub = t - m * hv;
  const uint32_t my = m / (uint32_t)G.mcus_x, mx = m - my * (uint32_t)G.mcus_x;
  *plane_block = (uint32_t)G.plane_off[c] + (my * vc + sub / hc) * (uint32_t)G.bw[c] + mx * hc + sub % hc;
  *seg_first = (uint32_t)G.plane_off[c] + (m / (uint32_t)G.restart) * (uint32_t)G.restart * hv;
}

// natural-order index of zig-zag index k
OVM_JD_HD uint32_t dezigzag(uint32_t k) {
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

}  // namespace ovm_jpeg_dec
