// Host half of the JPEG encoder (see jpeg_enc.hip): the quality-scaled quantisation tables, the plane geometry and the header bytes in
// front of the entropy-coded data, exactly as Pillow 12 (libjpeg-turbo's jcparam.c jpeg_set_quality / jcmarker.c) writes them, and the
// Annex K.3 Huffman tables with their canonical codes (built at compile time; the device kernels read the same tables).
// Plain C++ (no HIP), like jpeg_host.hpp, so that a CPU build can be checked under a sanitizer.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/ovm3d.h"
#include "jpeg_host.hpp"

namespace ovm_jpeg_enc {

// Annex K.1, natural order
static const uint8_t kQtLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                    69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                    81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
static const uint8_t kQtChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: codes per length 1..16, then the symbols in code order. Index 0 luminance, 1 chrominance.
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Canonical codes (Annex C) by symbol, packed (code << 8) | length; 0 = the symbol has no code.
struct EncTables {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
};

constexpr EncTables build_tables() {
  EncTables t{};
  for (int k = 0; k < 2; ++k) {
    uint32_t code = 0;
    int n = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < kDcBits[k][l - 1]; ++i, ++n, ++code) t.dc[k][kDcVals[n]] = (code << 8) | (uint32_t)l;
      code <<= 1;
    }
    code = 0; n = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < kAcBits[k][l - 1]; ++i, ++n, ++code) t.ac[k][kAcVals[k][n]] = (code << 8) | (uint32_t)l;
      code <<= 1;
    }
  }
  return t;
}

static const int kHeaderLen = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14;     // 623

// jpeg_set_quality(quality, force_baseline = TRUE)
inline void quant_tables(int quality, uint16_t qt[2][64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int a = ((int)kQtLuma[i] * scale + 50) / 100, b = ((int)kQtChroma[i] * scale + 50) / 100;
    qt[0][i] = (uint16_t)(a < 1 ? 1 : (a > 255 ? 255 : a));
    qt[1][i] = (uint16_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
  }
}

// Geometry, tables and (header != null) the header bytes. subsampling: Pillow's numbering, 0 = 4:4:4, 2 = 4:2:0.
inline int host_plan(int32_t width, int32_t height, int32_t quality, int32_t subsampling, OvmJpegEncInfo* info, uint8_t* header,
                     int32_t header_capacity) {
  if (!info) return OVM_ERR_INVALID;
  if (quality < 1 || quality > 100 || width < 1 || width > 65535 || height < 1 || height > 65535) return OVM_ERR_INVALID;
  if (subsampling != 0 && subsampling != 2) return OVM_ERR_UNSUPPORTED;
  if (header && header_capacity < kHeaderLen) return OVM_ERR_CAPACITY;
  OvmJpegEncInfo& I = *info;
  memset(&I, 0, sizeof(I));
  I.width = width; I.height = height; I.quality = quality;
  I.hs = I.vs = subsampling == 2 ? 2 : 1;
  I.mcus_x = (width + 8 * I.hs - 1) / (8 * I.hs);
  I.mcus_y = (height + 8 * I.vs - 1) / (8 * I.vs);
  I.bw[0] = I.mcus_x * I.hs; I.bh[0] = I.mcus_y * I.vs;
  I.bw[1] = I.bw[2] = I.mcus_x; I.bh[1] = I.bh[2] = I.mcus_y;
  I.coef_blocks = I.bw[0] * I.bh[0] + 2 * I.mcus_x * I.mcus_y;
  I.header_len = kHeaderLen;
  quant_tables(quality, I.qt);
  if (!header) return OVM_OK;
  uint8_t* p = header;
  static const uint8_t app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  memcpy(p, app0, 20); p += 20;
  for (int t = 0; t < 2; ++t) {
    *p++ = 0xff; *p++ = 0xdb; *p++ = 0; *p++ = 67; *p++ = (uint8_t)t;
    for (int k = 0; k < 64; ++k) *p++ = (uint8_t)I.qt[t][ovm_jpeg::kZigzag[k]];
  }
  const uint8_t sof[19] = {0xff, 0xc0, 0, 17, 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3,
                           1, (uint8_t)(I.hs * 16 + I.vs), 0, 2, 0x11, 1, 3, 0x11, 1};
  memcpy(p, sof, 19); p += 19;
  for (int t = 0; t < 2; ++t) {
    *p++ = 0xff; *p++ = 0xc4; *p++ = 0; *p++ = 31; *p++ = (uint8_t)t;
    memcpy(p, kDcBits[t], 16); p += 16;
    memcpy(p, kDcVals, 12); p += 12;
    *p++ = 0xff; *p++ = 0xc4; *p++ = 0; *p++ = 181; *p++ = (uint8_t)(0x10 | t);
    memcpy(p, kAcBits[t], 16); p += 16;
    memcpy(p, kAcVals[t], 162); p += 162;
  }
  static const uint8_t sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  memcpy(p, sos, 14); p += 14;
  return (int)(p - header) == kHeaderLen ? OVM_OK : OVM_ERR_INVALID;
}

// The plan's derived fields must be the ones host_plan writes: the device calls size their launches and buffers from them.
inline bool info_consistent(const OvmJpegEncInfo& I) {
  if (I.width < 1 || I.width > 65535 || I.height < 1 || I.height > 65535 || I.quality < 1 || I.quality > 100) return false;
  if (!((I.hs == 1 && I.vs == 1) || (I.hs == 2 && I.vs == 2))) return false;
  const int mx = (I.width + 8 * I.hs - 1) / (8 * I.hs), my = (I.height + 8 * I.vs - 1) / (8 * I.vs);
  if (I.mcus_x != mx || I.mcus_y != my || I.bw[0] != mx * I.hs || I.bh[0] != my * I.vs) return false;
  if (I.bw[1] != mx || I.bw[2] != mx || I.bh[1] != my || I.bh[2] != my) return false;
  if (I.coef_blocks != I.bw[0] * I.bh[0] + 2 * mx * my || I.header_len != kHeaderLen) return false;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i)
      if (I.qt[t][i] < 1 || I.qt[t][i] > 255) return false;
  return true;
}

}  // namespace ovm_jpeg_enc
