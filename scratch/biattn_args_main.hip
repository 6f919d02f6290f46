// Host-side checks of the bi-attention launcher under a sanitizer; needs no device (every call below returns before any HIP call):
//   cd ovmono3d_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       ../../scratch/biattn_args_main.hip gdino_kernels.hip -I. -o /tmp/biattn_args && /tmp/biattn_args
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "gdino.hpp"

using namespace ovm;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
  // workspace sizing: the chunks cover S, the sizes follow the path, nothing overflows at the largest geometry the engine accepts
  const int Ss[] = {1, 63, 64, 65, 6015, 10000, 1 << 20}, Ts[] = {1, 22, 32, 33, 256, 257}, dhs[] = {64, 128, 256, 512};
  for (int S : Ss) for (int T : Ts) for (int dh : dhs) for (int gen = 0; gen < 2; ++gen) {
    const BiAttnWs w = biattn_workspace(S, T, 4, dh, gen != 0);
    CHECK(w.mfma == (!gen && biattn_mfma_supported(4, dh, T)));
    CHECK(w.mfma == (!gen && dh == 256 && T <= 256));
    CHECK(w.chunk > 0 && (long)w.nchunk * w.chunk >= S && (long)(w.nchunk - 1) * w.chunk < S);
    CHECK(w.part == (size_t)w.nchunk * T * 4 * dh);
    if (w.mfma) CHECK(w.ml == (size_t)w.nchunk * 4 * T && w.sc == 0 && w.stat == 0);
    else CHECK(w.ml == 0 && w.sc == (size_t)4 * T * S && w.stat == (size_t)8 * T);
  }
  { const BiAttnWs w = biattn_workspace(0, 4, 4, 256, false); CHECK(w.nchunk == 0 && w.part == 0 && w.ml == 0); }
  { const BiAttnWs w = biattn_workspace(4, 4, -1, 256, false); CHECK(w.nchunk == 0 && w.part == 0); }
  CHECK(!biattn_mfma_supported(4, 128, 20) && !biattn_mfma_supported(0, 256, 20) && !biattn_mfma_supported(4, 256, 0));
  CHECK(biattn_mfma_supported(4, 256, 1) && biattn_mfma_supported(4, 256, 256));

  // the launcher refuses a null pointer or a non-positive dimension before it launches anything
  float dummy[4]; half_t hd[4];
  BiAttnParams ok; std::memset(&ok, 0, sizeof(ok));
  ok.qv = ok.kt = ok.vv = ok.vt = dummy; ok.ldq = ok.ldk = ok.ldvv = ok.ldvt = 2048; ok.S = 100; ok.T = 22; ok.H = 4; ok.dh = 256; ok.scale = 0.0625f;
  ok.cv_hi = hd; ok.cv_lo = hd; ok.ldcv = 1024; ok.ct = dummy; ok.part = dummy; ok.bm = dummy; ok.bl = dummy; ok.sc = dummy; ok.stat = dummy;
  ok.chunk = 64; ok.nchunk = 2;
  { BiAttnParams p = ok; p.qv = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.kt = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.vv = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.vt = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.ct = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.part = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.cv_hi = nullptr; p.cv = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.bm = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.bl = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.generic = 1; p.sc = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.dh = 128; p.stat = nullptr; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.S = 0; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.T = -3; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.H = 0; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  { BiAttnParams p = ok; p.dh = 0; CHECK(launch_biattn(p, nullptr) == OVM_ERR_INVALID); }
  // a chunking that is not biattn_workspace's, or a row stride the 16-byte loads cannot take, is a shape error - also before any launch
  { BiAttnParams p = ok; p.chunk = 128; p.nchunk = 1; CHECK(launch_biattn(p, nullptr) == OVM_ERR_SHAPE); }
  { BiAttnParams p = ok; p.ldq = 2049; CHECK(launch_biattn(p, nullptr) == OVM_ERR_SHAPE); }
  std::printf(fails ? "%d check(s) failed\n" : "biattn host checks ok\n", fails);
  return fails != 0;
}
