// Host side of the device entropy decode (jpeg_dec.hip): the plan, the workspace layout, and the serial emulation of the kernels.
// Plain C++ (no HIP) like jpeg_host.hpp, whose parser it reuses, so that scratch/fuzz_jpeg_dec.cpp can run it under
// AddressSanitizer.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_dec_core.hpp"
#include "jpeg_host.hpp"

namespace ovm_jpeg_dec {

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

constexpr int kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;

struct Layout {
  int64_t nchunks, nsub, nwg, nwords, scan_items;
  int64_t ctl, stream, dcd, zero_bytes;          // [ctl, ctl + zero_bytes) is cleared at the start of a call
  int64_t seg_off, chunk_cnt, sub_cnt, scan_out, partial, entry, exits, boundary, total;
};

inline Layout layout(const OvmJpegDecPlan& P) {
  Layout L;
  const int64_t n = P.ecs_bytes, nb = P.info.coef_blocks;
  L.nchunks = (n + kChunkBytes - 1) / kChunkBytes;
  L.nsub = (n * 8 + kSubBits - 1) / kSubBits;
  L.nwg = (L.nsub + kWgSubs - 1) / kWgSubs;
  L.nwords = (n + 16 + 3) / 4;                   // at least 16 zero bytes behind the stream
  L.scan_items = L.nchunks > nb ? L.nchunks : nb;
  if (L.nwg * kWgSubs > L.scan_items) L.scan_items = L.nwg * kWgSubs;     // the scan over subsequences covers whole workgroups
  int64_t o = 0;
  L.ctl = o; o += align16(kCtlWords * 4);
  L.stream = o; o += align16(L.nwords * 4);
  L.dcd = o; o += align16(nb * 8);
  L.zero_bytes = o;
  L.seg_off = o; o += align16((int64_t)P.segments * 4);
  L.chunk_cnt = o; o += align16(L.nchunks * 8);
  L.sub_cnt = o; o += align16(L.nwg * kWgSubs * 8);
  L.scan_out = o; o += align16((L.scan_items + 1) * 8);
  L.partial = o; o += align16(((L.scan_items + kScanTile - 1) / kScanTile + 1) * 8);
  L.entry = o; o += align16(L.nwg * kWgSubs * 8);
  L.exits = o; o += align16(L.nwg * kWgSubs * 8);
  L.boundary = o; o += align16(2 * L.nwg * 8);
  L.total = o;
  return L;
}

// what the plan call itself fills in; the device entry points refuse a record that does not pass
inline bool plan_consistent(const OvmJpegDecPlan& P) {
  const OvmJpegInfo& I = P.info;
  if (I.ncomp != 1 && I.ncomp != 3) return false;
  if (I.coef_blocks < 1 || I.coef_blocks > (1 << 22)) return false;
  if (P.ecs_bytes < 1 || P.ecs_bytes > kMaxStreamBytes || P.ecs_offset < 0) return false;
  if (P.sub_bits != kSubBits || P.wg_subs != kWgSubs || P.sync_launches != kSyncLaunches || P.tables_bytes != (int32_t)sizeof(Tables)) return false;
  if (P.max_rounds < 1 || P.max_rounds > kWgSubs) return false;
  if (P.mcus_x < 1 || P.mcus_y < 1 || (int64_t)P.mcus_x * P.mcus_y > (1 << 22)) return false;
  int bpm = 0; int64_t blocks = 0;
  for (int c = 0; c < I.ncomp; ++c) {
    if (I.h[c] < 1 || I.h[c] > 2 || I.v[c] < 1 || I.v[c] > 2) return false;
    if (I.bw[c] != P.mcus_x * I.h[c] || I.bh[c] != P.mcus_y * I.v[c]) return false;
    bpm += I.h[c] * I.v[c]; blocks += (int64_t)I.bw[c] * I.bh[c];
  }
  if (bpm != P.blocks_per_mcu || bpm > 6 || blocks != I.coef_blocks) return false;
  const int mcus = P.mcus_x * P.mcus_y;
  if (P.restart_interval < 0 || P.restart_interval > 65535) return false;
  const int R = P.restart_interval ? P.restart_interval : mcus;
  if (P.segments != (mcus + R - 1) / R) return false;
  for (int b = 0; b < bpm; ++b) {
    const int c = P.sel_comp[b];
    if (c >= I.ncomp || P.sel_sub[b] >= I.h[c] * I.v[c] || P.sel_dc[b] > 3 || P.sel_ac[b] > 3) return false;
  }
  return true;
}

inline Geom geom(const OvmJpegDecPlan& P) {
  Geom G;
  memset(&G, 0, sizeof(G));
  const OvmJpegInfo& I = P.info;
  G.ncomp = I.ncomp; G.bpm = P.blocks_per_mcu; G.mcus_x = P.mcus_x; G.mcus = P.mcus_x * P.mcus_y;
  G.restart = P.restart_interval ? P.restart_interval : G.mcus;
  G.nseg = P.segments; G.coef_blocks = I.coef_blocks;
  int off = 0;
  for (int c = 0; c < 3; ++c) {
    G.h[c] = c < I.ncomp ? I.h[c] : 1; G.v[c] = c < I.ncomp ? I.v[c] : 1; G.bw[c] = c < I.ncomp ? I.bw[c] : 0;
    G.plane_off[c] = off;
    if (c < I.ncomp) off += I.bw[c] * I.bh[c];
  }
  memcpy(G.sel_comp, P.sel_comp, 8); memcpy(G.sel_sub, P.sel_sub, 8); memcpy(G.sel_dc, P.sel_dc, 8); memcpy(G.sel_ac, P.sel_ac, 8);
  G.bperiod = G.bpm;                              // the smallest divisor q of bpm with table pairs of period q
  for (int q = 1; q < G.bpm; ++q) {
    if (G.bpm % q) continue;
    bool periodic = true;
    for (int b = q; b < G.bpm && b < 8; ++b) periodic = periodic && P.sel_dc[b] == P.sel_dc[b - q] && P.sel_ac[b] == P.sel_ac[b - q];
    if (periodic) { G.bperiod = q; break; }
  }
  return G;
}

inline void fill_lut(const ovm_jpeg::Huff& h, HuffLut* t) {
  memset(t, 0, sizeof(*t));
  if (!h.present) return;                          // all limits 0 and no fast entry: no code matches, every symbol is refused
  memcpy(t->fast, h.fast, sizeof(t->fast));
  uint32_t run = 0;
  for (int l = 10; l <= 16; ++l) {
    const uint32_t own = (uint32_t)(h.maxcode[l] + 1) << (16 - l);       // maxcode -1 (no code of this length): 0, never exceeded
    if (own > run) run = own;
    t->limit[l - 10] = run; t->mincode[l - 10] = h.mincode[l]; t->valptr[l - 10] = h.valptr[l];
  }
  memcpy(t->vals, h.vals, 256);
}

// The file must be one the host decoder would read as: headers, ONE scan with all components in frame order, EOI. Whatever is
// odd is declined (OVM_ERR_UNSUPPORTED or the parser's own code), never judged: the host route stays the arbiter.
inline int host_plan(const uint8_t* d, size_t n, int32_t max_rounds, OvmJpegDecPlan* plan, uint8_t* tables, int64_t tables_capacity) {
  if (!d || !plan) return OVM_ERR_INVALID;
  if (tables && tables_capacity < (int64_t)sizeof(Tables)) return OVM_ERR_CAPACITY;
  ovm_jpeg::Frame f;
  const int rc = ovm_jpeg::parse(d, n, f, nullptr);     // stops at the first SOS; refuses what the host route refuses up to there
  if (rc) return rc;
  if (f.progressive) return OVM_ERR_UNSUPPORTED;
  // the same walk again, for the position of that SOS (every length below was checked by parse)
  size_t pos = 2, sos = 0;
  while (pos + 2 <= n) {
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return OVM_ERR_UNSUPPORTED;
    const int m = d[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || pos + 2 > n) return OVM_ERR_UNSUPPORTED;
    const size_t len = (size_t)ovm_jpeg::be16(d + pos);
    if (len < 2 || pos + len > n) return OVM_ERR_UNSUPPORTED;
    if (m == 0xDA) { sos = pos; break; }
    pos += len;
  }
  if (!sos) return OVM_ERR_UNSUPPORTED;
  const OvmJpegInfo& I = f.info;
  const uint8_t* s = d + sos + 2;
  const int sl = ovm_jpeg::be16(d + sos) - 2;
  if (sl < 1 || s[0] != I.ncomp || sl < 1 + 2 * I.ncomp + 3) return OVM_ERR_UNSUPPORTED;
  memset(plan, 0, sizeof(*plan));
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  for (int i = 0; i < I.ncomp; ++i) {
    for (int q = 0; q < I.ncomp; ++q)
      if (q != i && f.cid[q] == f.cid[i]) return OVM_ERR_UNSUPPORTED;       // ambiguous component ids
    if (s[1 + 2 * i] != f.cid[i]) return OVM_ERR_UNSUPPORTED;
    td[i] = s[2 + 2 * i] >> 4; ta[i] = s[2 + 2 * i] & 15;
    if (td[i] > 3 || ta[i] > 3 || !f.dc[td[i]].present || !f.ac[ta[i]].present) return OVM_ERR_UNSUPPORTED;
  }
  const uint8_t* e = s + 1 + 2 * I.ncomp;
  if (e[0] != 0 || e[1] != 63 || e[2] != 0) return OVM_ERR_UNSUPPORTED;
  // the entropy-coded segment ends in front of the first 0xFF that is followed by neither 0x00 nor RSTn; EOI must stand there
  const size_t start = sos + (size_t)sl + 2;
  size_t end = start;
  while (end < n) {
    const uint8_t* q = (const uint8_t*)memchr(d + end, 0xFF, n - end);
    if (!q) { end = n; break; }
    end = (size_t)(q - d);
    if (end + 1 < n && (d[end + 1] == 0x00 || (d[end + 1] >= 0xD0 && d[end + 1] <= 0xD7))) { end += 2; continue; }
    break;
  }
  if (end + 2 > n || d[end] != 0xFF || d[end + 1] != 0xD9) return OVM_ERR_UNSUPPORTED;
  if (end <= start || (int64_t)(end - start) > kMaxStreamBytes) return OVM_ERR_UNSUPPORTED;
  plan->info = I;
  plan->ecs_offset = (int64_t)start; plan->ecs_bytes = (int64_t)(end - start);
  plan->restart_interval = f.restart;
  plan->mcus_x = I.bw[0] / I.h[0]; plan->mcus_y = I.bh[0] / I.v[0];
  const int mcus = plan->mcus_x * plan->mcus_y, R = f.restart ? f.restart : mcus;
  plan->segments = (mcus + R - 1) / R;
  plan->sub_bits = kSubBits; plan->wg_subs = kWgSubs; plan->sync_launches = kSyncLaunches;
  plan->max_rounds = max_rounds <= 0 ? kDefaultMaxRounds : (max_rounds > kWgSubs ? kWgSubs : max_rounds);
  plan->tables_bytes = (int32_t)sizeof(Tables);
  int b = 0;
  for (int c = 0; c < I.ncomp; ++c)
    for (int sub = 0; sub < I.h[c] * I.v[c]; ++sub, ++b) {
      if (b >= 8) return OVM_ERR_UNSUPPORTED;
      plan->sel_comp[b] = (uint8_t)c; plan->sel_sub[b] = (uint8_t)sub; plan->sel_dc[b] = (uint8_t)td[c]; plan->sel_ac[b] = (uint8_t)ta[c];
    }
  plan->blocks_per_mcu = b;
  if (!plan_consistent(*plan)) return OVM_ERR_UNSUPPORTED;
  if (tables) {
    Tables* T = (Tables*)tables;
    for (int t = 0; t < 4; ++t) { fill_lut(f.dc[t], &T->dc[t]); fill_lut(f.ac[t], &T->ac[t]); }
  }
  return OVM_OK;
}

// ---- the emulation: every kernel of jpeg_dec.hip as a loop ----
struct HostSink {
  int16_t* coef; int64_t* dcd; uint32_t* status; uint32_t coef_blocks;
  inline void dc(const Geom& G, uint32_t g, uint32_t, int diff) {
    uint32_t pb, item; block_place(G, g, &pb, &item);
    if (item < coef_blocks) dcd[item] = diff;
  }
  inline void ac(const Geom& G, uint32_t g, uint32_t k, int val) {
    uint32_t pb, item; block_place(G, g, &pb, &item);
    if (pb < coef_blocks && k < 64) coef[(size_t)pb * 64 + dezigzag(k)] = (int16_t)val;
  }
  inline void flag(uint32_t bits) { *status |= bits; }
};

inline int host_emulate(const uint8_t* data, size_t n, int32_t max_rounds, int16_t* coef, int64_t coef_capacity, OvmJpegInfo* info,
                        int32_t* status_out, int32_t* rounds_out, int32_t* launches_out = nullptr) {
  if (!data || !coef || !info || !status_out || !rounds_out) return OVM_ERR_INVALID;
  OvmJpegDecPlan P;
  std::vector<uint8_t> tables(sizeof(Tables));
  const int rc = host_plan(data, n, max_rounds, &P, tables.data(), (int64_t)tables.size());
  if (rc) return rc;
  const int64_t nb = P.info.coef_blocks;
  if (coef_capacity < nb * 64) return OVM_ERR_CAPACITY;
  *info = P.info;
  const Layout L = layout(P);
  const Geom G = geom(P);
  const uint8_t* s = data + P.ecs_offset;
  const int64_t ns = P.ecs_bytes;
  uint32_t ctl[kCtlWords] = {0};
  memset(coef, 0, sizeof(int16_t) * 64 * (size_t)nb);
  // stage 1: unstuff, segment table
  std::vector<uint32_t> words((size_t)L.nwords, 0u), seg_off((size_t)G.nseg, 0u);
  uint8_t* U = (uint8_t*)words.data();
  uint32_t kept = 0, ord = 0;
  for (int64_t j = 0; j < ns; ++j) {
    const int prev = j > 0 ? s[j - 1] : -1, next = j + 1 < ns ? s[j + 1] : -1;
    const uint32_t cl = classify_byte(prev, s[j], next);
    if (cl & kByteAnomaly) ctl[kCtlStatus] |= kStMarker;
    if (cl & kByteKeep) U[kept++] = s[j];
    if (cl & kByteMarker) {
      if (next != (int)(0xD0 + (ord & 7))) ctl[kCtlStatus] |= kStMarker;
      if (ord + 1 < (uint32_t)G.nseg) seg_off[ord + 1] = kept; else ctl[kCtlStatus] |= kStSegments;
      const bool empty_before = j == 0 || (j >= 2 && s[j - 2] == 0xFF && s[j - 1] >= 0xD0 && s[j - 1] <= 0xD7), empty_behind = j + 2 >= ns;
      if (empty_before || empty_behind) ctl[kCtlStatus] |= kStSegments;
      ++ord;
    }
  }
  if (ord != (uint32_t)G.nseg - 1) ctl[kCtlStatus] |= kStSegments;
  ctl[kCtlTotalBytes] = kept;
  Ctx C;
  C.words = words.data(); C.word_base = 0; C.nlocal = (uint32_t)L.nwords; C.nwords = (uint32_t)L.nwords; C.total_bits = kept * 8u; C.seg_off = seg_off.data();
  C.tab = (const Tables*)tables.data(); C.g = &G;
  const int64_t nthreads = L.nwg * kWgSubs;
  std::vector<uint64_t> entry((size_t)nthreads, 0), exits((size_t)nthreads, 0), cnt((size_t)nthreads, 0), bx((size_t)(2 * L.nwg), 0);
  const int cap = P.max_rounds;
  auto sub_end = [&](int64_t i) { const uint64_t e = (uint64_t)(i + 1) * kSubBits; return (uint32_t)(e < C.total_bits ? e : C.total_bits); };
  // stage 2: synchronisation, launch by launch, workgroup by workgroup (a launch reads only what earlier launches wrote)
  for (int l = 0; l < kSyncLaunches; ++l) {
    if (ctl[kCtlStatus]) break;
    if (l > 0 && !ctl[kCtlChanged + l - 1]) break;
    for (int64_t j = 0; j < L.nwg; ++j) {
      uint64_t* e = entry.data() + j * kWgSubs; uint64_t* x = exits.data() + j * kWgSubs; uint64_t* c = cnt.data() + j * kWgSubs;
      bool dirty[kWgSubs];
      for (int t = 0; t < kWgSubs; ++t) {
        dirty[t] = l == 0;
        if (l == 0) e[t] = pack_state((uint32_t)((j * kWgSubs + t) * kSubBits), 0, 0);
      }
      int steps = 0;
      for (int step = 0; step < cap; ++step) {
        if (l > 0 || step > 0) {
          uint64_t prev_x[kWgSubs];
          memcpy(prev_x, x, sizeof(prev_x));
          for (int t = 0; t < kWgSubs; ++t) {
            uint64_t ne = e[t];
            if (t > 0) ne = prev_x[t - 1];
            else if (step == 0 && j > 0) ne = bx[(size_t)(((l - 1) & 1) * L.nwg + j - 1)];
            const bool active = (uint64_t)(j * kWgSubs + t) * kSubBits < C.total_bits;    // a subsequence behind the data takes no part
            if (active && ne != e[t]) { e[t] = ne; dirty[t] = true; }
          }
        }
        bool any = false;
        for (int t = 0; t < kWgSubs; ++t) any = any || dirty[t];
        if (!any) break;
        for (int t = 0; t < kWgSubs; ++t)
          if (dirty[t]) {
            NullSink sink; uint32_t nbk = 0;
            x[t] = decode_sub(C, e[t], sub_end(j * kWgSubs + t), 0, sink, &nbk);
            c[t] = nbk; dirty[t] = false;
          }
        ++steps;
      }
      bx[(size_t)((l & 1) * L.nwg + j)] = x[kWgSubs - 1];
      if (steps) ctl[kCtlChanged + l] = 1;
      if ((uint32_t)steps > ctl[kCtlRounds + l]) ctl[kCtlRounds + l] = (uint32_t)steps;
    }
  }
  if (ctl[kCtlChanged + kSyncLaunches - 1]) ctl[kCtlStatus] |= kStNoSync;
  if (!ctl[kCtlStatus]) {
    // stage 3: blocks completed before each subsequence, then the write pass
    std::vector<int64_t> dcd((size_t)nb, 0);
    HostSink sink{coef, dcd.data(), &ctl[kCtlLate], (uint32_t)nb};
    uint64_t before = 0;
    for (int64_t i = 0; i < nthreads; ++i) {
      uint32_t nbk = 0;
      decode_sub(C, entry[(size_t)i], sub_end(i), (uint32_t)before, sink, &nbk);
      before += cnt[(size_t)i];
    }
    // stage 4: DC predictors per component and restart segment
    std::vector<int64_t> pre((size_t)nb + 1, 0);
    for (int64_t j = 0; j < nb; ++j) pre[(size_t)j + 1] = pre[(size_t)j] + dcd[(size_t)j];
    for (int64_t j = 0; j < nb; ++j) {
      uint32_t pb, first; dc_item_place(G, (uint32_t)j, &pb, &first);
      const int64_t pred = pre[(size_t)j + 1] - pre[first < (uint32_t)nb ? first : 0];
      if (pred < -65536 || pred > 65535) ctl[kCtlLate] |= kStDcRange;
      if (pb < (uint32_t)nb) coef[(size_t)pb * 64] = (int16_t)pred;
    }
  }
  uint32_t rounds = 0;
  uint32_t launches = 0;
  for (int l = 0; l < kSyncLaunches; ++l) { rounds += ctl[kCtlRounds + l]; launches += ctl[kCtlChanged + l] ? 1u : 0u; }
  *status_out = (int32_t)(ctl[kCtlStatus] | ctl[kCtlLate]); *rounds_out = (int32_t)rounds;
  if (launches_out) *launches_out = (int32_t)launches;
  return OVM_OK;
}

}  // namespace ovm_jpeg_dec
