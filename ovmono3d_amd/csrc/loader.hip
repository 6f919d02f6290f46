// Host-side model loading shared by the four handles (loader.hpp).
#include "loader.hpp"

#include <cstring>

namespace ovm {

constexpr size_t kSlabBytes = (size_t)256 << 20;

// ALLOC_SLAB: 256-byte aligned pieces of 256-MiB slabs (ovm_gdino_create says why that handle wants them)
int Loader::alloc_bytes(void** p, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 16;
  void* q = nullptr;
  if (policy == ALLOC_EACH) {
    OVM_HIP(this, hipMalloc(&q, bytes));
    allocs.push_back(q);
  } else {
    bytes = (bytes + 255) & ~(size_t)255;
    if (slab_off + bytes > slab_cap) {
      const size_t cap = bytes > kSlabBytes ? bytes : kSlabBytes;
      OVM_HIP(this, hipMalloc(&q, cap));
      allocs.push_back(q);
      slab = (char*)q; slab_cap = cap; slab_off = 0;
    }
    q = slab + slab_off;
    slab_off += bytes;
  }
  if (zero) OVM_HIP(this, hipMemset(q, 0, bytes));
  *p = q;
  return OVM_OK;
}

void Loader::free_all() {
  for (void* p : allocs) (void)hipFree(p);
  allocs.clear();
  slab = nullptr; slab_off = slab_cap = 0;
}

int find_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect, const OvmTensor** out) {
  const OvmTensor* t = wm.get(key);
  if (!t) { L->err = "missing weight: " + key; return OVM_ERR_MISSING_WEIGHT; }
  if (expect >= 0 && numel(t) != expect) {
    L->err = "bad shape for " + key + " (expected " + std::to_string(expect) + " elements)";
    return OVM_ERR_SHAPE;
  }
  *out = t;
  return OVM_OK;
}

int find_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect, const float** data) {
  const OvmTensor* t;
  const int r = find_weight(L, wm, key, expect, &t);
  if (!r) *data = t->data;
  return r;
}

int upload_f32(Loader* L, const float* src, size_t n, float** out) {
  OVM_TRY(L, L->alloc(out, n));
  OVM_HIP(L, hipMemcpy(*out, src, n * sizeof(float), hipMemcpyHostToDevice));
  return OVM_OK;
}

int upload_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect, float** out) {
  const OvmTensor* t;
  OVM_TRY(L, find_weight(L, wm, key, expect, &t));
  return upload_f32(L, t->data, (size_t)numel(t), out);
}

int host_pack_weight(const float* w, int N, int K, int Kpad, int precision, half_t* out) {
  if (!w || !out || N < 1 || K < 1 || Kpad < K || (precision != 1 && precision != 3)) return OVM_ERR_INVALID;
  const bool il = precision == 3;
  if (il && Kpad % 32 != 0) return OVM_ERR_SHAPE;
  const size_t ld = il ? (size_t)2 * Kpad : (size_t)Kpad;
  memset(out, 0, packed_halves(N, Kpad, precision) * sizeof(half_t));
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      const float x = w[(size_t)n * K + k];
      const half_t hh = (half_t)x;
      if (il) {
        const size_t o = (size_t)n * ld + (size_t)(k >> 5) * 64 + (k & 31);
        out[o] = hh;
        out[o + 32] = (half_t)(x - (float)hh);
      } else {
        out[(size_t)n * ld + k] = hh;
      }
    }
  return OVM_OK;
}

int host_frag_order(const half_t* image, int N, int Kpad, half_t* out) {
  if (!image || !out || image == out || N < 1 || Kpad < 32) return OVM_ERR_INVALID;
  if (Kpad % 32 != 0) return OVM_ERR_SHAPE;
  const int Npad = npad128(N), KS = Kpad / 32;
  for (int tile = 0; tile < Npad / 16; ++tile)
    for (int ks = 0; ks < KS; ++ks)
      for (int part = 0; part < 2; ++part)
        for (int lane = 0; lane < 64; ++lane) {
          const size_t so = (size_t)(tile * 16 + (lane & 15)) * 2 * Kpad + (size_t)ks * 64 + part * 32 + (lane >> 4) * 8;
          const size_t dof = ((((size_t)tile * KS + ks) * 2 + part) * 64 + lane) * 8;
          for (int e = 0; e < 8; ++e) out[dof + e] = image[so + e];
        }
  return OVM_OK;
}

int upload_packed(Loader* L, const float* w, int N, int K, int Kpad, const float* bias, int nbias, PackedLin* out,
                  std::vector<half_t>* image) {
  std::vector<half_t> local;
  std::vector<half_t>& buf = image ? *image : local;
  buf.resize(packed_halves(N, Kpad, L->precision));
  const int r = host_pack_weight(w, N, K, Kpad, L->precision, buf.data());
  if (r) { if (L->err.empty()) L->err = r == OVM_ERR_SHAPE ? "packed K must be a multiple of 32" : "invalid packed weight shape"; return r; }
  OVM_TRY(L, L->alloc(&out->hi, buf.size()));
  OVM_HIP(L, hipMemcpy(out->hi, buf.data(), buf.size() * sizeof(half_t), hipMemcpyHostToDevice));
  out->lo = L->precision == 3 ? out->hi + 32 : nullptr;
  out->N = N; out->K = K; out->Kpad = Kpad;
  out->bias = nullptr;
  if (bias) return upload_f32(L, bias, (size_t)nbias, &out->bias);
  return OVM_OK;
}

std::vector<float> reorder_conv(const float* w, int Cout, int Cin, int kh, int kw) {
  const int kk = kh * kw;
  std::vector<float> v((size_t)Cout * Cin * kk);
  for (int o = 0; o < Cout; ++o)
    for (int c = 0; c < Cin; ++c)
      for (int t = 0; t < kk; ++t) v[((size_t)o * kk + t) * Cin + c] = w[((size_t)o * Cin + c) * kk + t];
  return v;
}

std::vector<float> reorder_convt(const float* w, int Cin, int Cout) {
  std::vector<float> v((size_t)4 * Cout * Cin);
  for (int ci = 0; ci < Cin; ++ci)
    for (int co = 0; co < Cout; ++co)
      for (int q = 0; q < 4; ++q) v[((size_t)q * Cout + co) * Cin + ci] = w[((size_t)ci * Cout + co) * 4 + q];
  return v;
}

int pack_concat(Loader* L, const WeightMap& wm, const std::vector<std::pair<std::string, int>>& parts, int K, PackedLin* out, bool bias,
                const float* row_scale, std::vector<half_t>* image, int Kpad) {
  std::vector<float> w, b;
  int N = 0;
  for (auto& p : parts) {
    const OvmTensor* t;
    OVM_TRY(L, find_weight(L, wm, p.first + ".weight", -1, &t));
    const int n = p.second < 0 ? (int)t->shape[0] : p.second;
    if (K < 0 && n > 0) K = (int)(numel(t) / n);
    OVM_TRY(L, find_weight(L, wm, p.first + ".weight", (int64_t)n * K, &t));
    w.insert(w.end(), t->data, t->data + (size_t)n * K);
    if (bias) {
      const float* bb;
      OVM_TRY(L, find_weight(L, wm, p.first + ".bias", n, &bb));
      b.insert(b.end(), bb, bb + n);
    }
    N += n;
  }
  if (row_scale)
    for (int n = 0; n < N; ++n) {
      for (int k = 0; k < K; ++k) w[(size_t)n * K + k] *= row_scale[n];
      if (bias) b[n] *= row_scale[n];
    }
  return upload_packed(L, w.data(), N, K, Kpad < 0 ? L->kpad(K) : Kpad, bias ? b.data() : nullptr, N, out, image);
}

int pack_linear_named(Loader* L, const WeightMap& wm, const std::string& wkey, const std::string& bkey, int N, int K, PackedLin* out, int Kpad) {
  const float *w, *b = nullptr;
  OVM_TRY(L, find_weight(L, wm, wkey, (int64_t)N * K, &w));
  if (!bkey.empty()) OVM_TRY(L, find_weight(L, wm, bkey, N, &b));
  return upload_packed(L, w, N, K, Kpad < 0 ? L->kpad(K) : Kpad, b, N, out);
}

// the bias of a convolution under `mode`: *b stays null when there is none to take
static int conv_bias(Loader* L, const WeightMap& wm, const std::string& key, int Cout, BiasMode mode, const float** b) {
  *b = nullptr;
  if (mode == BIAS_REQUIRED) return find_weight(L, wm, key, Cout, b);
  const OvmTensor* t = mode == BIAS_IF_PRESENT ? wm.get(key) : nullptr;
  if (t && numel(t) == Cout) *b = t->data;
  return OVM_OK;
}

int pack_conv(Loader* L, const WeightMap& wm, const std::string& prefix, int Cout, int Cin, int k, BiasMode bias, PackedLin* out) {
  const float *w, *b;
  OVM_TRY(L, find_weight(L, wm, prefix + ".weight", (int64_t)Cout * Cin * k * k, &w));
  OVM_TRY(L, conv_bias(L, wm, prefix + ".bias", Cout, bias, &b));
  const std::vector<float> v = reorder_conv(w, Cout, Cin, k, k);
  return upload_packed(L, v.data(), Cout, Cin * k * k, L->kpad(Cin * k * k), b, Cout, out);
}

int pack_convt(Loader* L, const WeightMap& wm, const std::string& prefix, int Cin, int Cout, BiasMode bias, bool tile_bias, PackedLin* out) {
  const float *w, *b;
  OVM_TRY(L, find_weight(L, wm, prefix + ".weight", (int64_t)Cin * Cout * 4, &w));
  OVM_TRY(L, conv_bias(L, wm, prefix + ".bias", Cout, bias, &b));
  const std::vector<float> v = reorder_convt(w, Cin, Cout);
  std::vector<float> bb;
  if (b && tile_bias) {
    bb.resize((size_t)4 * Cout);
    for (int q = 0; q < 4; ++q) memcpy(&bb[(size_t)q * Cout], b, (size_t)Cout * sizeof(float));
    b = bb.data();
  }
  return upload_packed(L, v.data(), 4 * Cout, Cin, L->kpad(Cin), b, tile_bias ? 4 * Cout : Cout, out);
}

}  // namespace ovm

extern "C" int ovm_host_pack_weight(const float* w, int32_t N, int32_t K, int32_t Kpad, int32_t precision, uint16_t* out) {
  return ovm::host_pack_weight(w, N, K, Kpad, precision, (ovm::half_t*)out);
}

extern "C" int ovm_host_frag_order(const uint16_t* image, int32_t N, int32_t Kpad, uint16_t* out) {
  return ovm::host_frag_order((const ovm::half_t*)image, N, Kpad, (ovm::half_t*)out);
}
