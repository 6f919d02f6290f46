// Host-side model loading shared by the four handles (OvmHandle, OvmGdino, OvmSam, OvmDepthPro) and the ViT tower they hold
// (tower.hpp: a Tower is a Loader of its own): the state a handle embeds (error
// text, recorded device allocations, precision), the checkpoint map, fp32 uploads, the packed fp16 weight image of gemm.hpp and the
// weight reorders that feed it. The image format is written here and nowhere else on the host (the device writer is
// pack_weight_kernel in gops.hip; tests pin the two to each other).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ovm3d.h"
#include "common.hpp"

namespace ovm {

// device fp16 split tensor (one-pass mode: hi alone, lo null)
struct SplitImg { half_t* hi = nullptr; half_t* lo = nullptr; };

// packed nn.Linear: weight image of gemm.hpp / gemm_small.hip (rows padded to 128; split mode [Npad][Kpad/32][hi 32 | lo 32] with
// lo = hi + 32, one-pass mode [Npad][Kpad]) + fp32 bias. K = the logical contraction length, Kpad = the image's (what GemmParams::K takes)
struct PackedLin { half_t* hi = nullptr; half_t* lo = nullptr; float* bias = nullptr; int N = 0, K = 0, Kpad = 0; };

enum AllocPolicy {
  ALLOC_EACH,      // one hipMalloc per buffer
  ALLOC_SLAB,      // 256-byte aligned pieces of 256-MiB slabs
};

// What a handle embeds (as its base): the first error of the current call, every device allocation to free at destroy, the precision
// (1 = one-pass fp16, 3 = f16x3 split) and how weights are allocated and padded.
struct Loader {
  std::string err;
  std::vector<void*> allocs;
  int precision = 3;
  AllocPolicy policy = ALLOC_EACH;
  int k_align = 1;                                     // Kpad of a packed weight when the caller names none: K rounded up to this
  char* slab = nullptr; size_t slab_off = 0, slab_cap = 0;      // ALLOC_SLAB: the current slab

  int kpad(int K) const { return (K + k_align - 1) / k_align * k_align; }
  int alloc_bytes(void** p, size_t bytes, bool zero);
  template <typename T>
  int alloc(T** p, size_t count, bool zero = false) { return alloc_bytes((void**)p, count * sizeof(T), zero); }
  void free_all();
};

// The first recorded message wins: an inner function's text ("missing weight: ...") is not replaced on the way out.
#define OVM_HIP(s, call)                                                                                       \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) {                                                                                    \
      if ((s)->err.empty()) (s)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
      return OVM_ERR_HIP;                                                                                      \
    }                                                                                                          \
  } while (0)

#define OVM_TRY(s, call)                                                                                       \
  do {                                                                                                         \
    int r_ = (call);                                                                                           \
    if (r_ != OVM_OK) {                                                                                        \
      if ((s)->err.empty()) (s)->err = std::string(#call) + " failed (" + std::to_string(r_) + ")";            \
      return r_;                                                                                               \
    }                                                                                                          \
  } while (0)

inline dim3 g1(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
inline int last_launch() { return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP; }
inline int64_t numel(const OvmTensor* t) { int64_t n = 1; for (int i = 0; i < t->ndim; ++i) n *= t->shape[i]; return n; }

// checkpoint: name -> tensor (a later duplicate replaces an earlier one)
struct WeightMap {
  std::unordered_map<std::string, const OvmTensor*> m;
  WeightMap(const OvmTensor* weights, int n) { for (int i = 0; i < n; ++i) m[weights[i].name] = &weights[i]; }
  const OvmTensor* get(const std::string& k) const { auto it = m.find(k); return it == m.end() ? nullptr : it->second; }
};

// "missing weight: KEY" (OVM_ERR_MISSING_WEIGHT); with expect >= 0 also "bad shape for KEY (expected N elements)" (OVM_ERR_SHAPE)
int find_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect, const OvmTensor** out);
int find_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect, const float** data);

int upload_f32(Loader* L, const float* src, size_t n, float** out);
int upload_weight(Loader* L, const WeightMap& wm, const std::string& key, int64_t expect /* < 0: as stored */, float** out);

// ---- the packed weight image
inline int npad128(int N) { return (N + 127) / 128 * 128; }
inline size_t packed_halves(int N, int Kpad, int precision) { return (size_t)npad128(N) * Kpad * (precision == 3 ? 2 : 1); }
// host [N][K] fp32 (GEMM k-order) -> the whole image, padding included, packed_halves(N, Kpad, precision) halves at out. No HIP calls.
// OVM_ERR_INVALID: null pointers, N < 1, K < 1, Kpad < K, precision not 1 or 3; OVM_ERR_SHAPE: split mode with Kpad % 32 != 0
// (out is not written then).
int host_pack_weight(const float* w, int N, int K, int Kpad, int precision, half_t* out);
// the split (precision 3) image of host_pack_weight -> the same halves in MFMA-fragment order [tile of 16 rows][k-step of 32][hi | lo]
// [lane 0..63][8 halves], lane l = row l % 16, halves 8 (l / 16) .. of the k-step: what the row-chain and Swin window kernels load.
// OVM_ERR_INVALID: null pointers, image == out, N < 1, Kpad < 32; OVM_ERR_SHAPE: Kpad % 32 != 0 (out is not written then). No HIP calls.
int host_frag_order(const half_t* image, int N, int Kpad, half_t* out);
// packs and uploads; bias: nbias floats or null. image: when given, receives the host image (gdino's fragment copies are cut from it)
int upload_packed(Loader* L, const float* w, int N, int K, int Kpad, const float* bias, int nbias, PackedLin* out,
                  std::vector<half_t>* image = nullptr);

// ---- reorders into GEMM k-order
// conv weight [Cout][Cin][kh][kw] -> [Cout][(ky * kw + kx) * Cin + c]
std::vector<float> reorder_conv(const float* w, int Cout, int Cin, int kh, int kw);
// ConvTranspose2d k2 s2 weight [Cin][Cout][2][2] -> GEMM rows [(a * 2 + b) * Cout + co][ci]
std::vector<float> reorder_convt(const float* w, int Cin, int Cout);

enum BiasMode { BIAS_NONE, BIAS_IF_PRESENT /* taken when the checkpoint has one of the right length */, BIAS_REQUIRED };

// several nn.Linear sharing one input, concatenated along N: parts = (prefix, rows; rows < 0: the tensor's shape[0]), K < 0: read
// off the first part. row_scale [N]: every row (and its bias) times its factor. image: see upload_packed. Kpad < 0: L->kpad(K)
int pack_concat(Loader* L, const WeightMap& wm, const std::vector<std::pair<std::string, int>>& parts, int K, PackedLin* out,
                bool bias = true, const float* row_scale = nullptr, std::vector<half_t>* image = nullptr, int Kpad = -1);
// nn.Linear stored as bare parameters (nn.MultiheadAttention in_proj_weight / in_proj_bias); bkey empty: no bias
int pack_linear_named(Loader* L, const WeightMap& wm, const std::string& wkey, const std::string& bkey, int N, int K, PackedLin* out,
                      int Kpad = -1);
// nn.Linear weight [N][K] (+ bias)
inline int pack_linear(Loader* L, const WeightMap& wm, const std::string& prefix, int N, int K, PackedLin* out, bool bias = true,
                       int Kpad = -1) {
  return pack_linear_named(L, wm, prefix + ".weight", bias ? prefix + ".bias" : std::string(), N, K, out, Kpad);
}
int pack_conv(Loader* L, const WeightMap& wm, const std::string& prefix, int Cout, int Cin, int k, BiasMode bias, PackedLin* out);
// tile_bias false: bias [Cout], for EPI_CONVT, which adds it per co; true: bias tiled over the four taps [4 Cout], for callers that
// run the transposed convolution as a plain linear over the (tap, co) columns
int pack_convt(Loader* L, const WeightMap& wm, const std::string& prefix, int Cin, int Cout, BiasMode bias, bool tile_bias, PackedLin* out);

}  // namespace ovm
