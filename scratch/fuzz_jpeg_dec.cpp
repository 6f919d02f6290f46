// AddressSanitizer fuzz of the device entropy route's CPU emulation (CPU build only; sanitizers do not run on the GPU pool):
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 scratch/fuzz_jpeg_dec.cpp -o /tmp/fuzz_jpeg_dec && /tmp/fuzz_jpeg_dec a.jpg b.jpg ...
// The emulation (ovmono3d_amd/csrc/jpeg_dec_host.hpp) runs the kernels' own core routine (jpeg_dec_core.hpp) with the kernels' own
// indexing, so an out-of-range table index, stream read or coefficient store of the device code shows here. 20,000 mutated streams
// (byte flips inside the entropy-coded segment, flips anywhere, truncations, insertions, deletions) from the given seeds, each in an
// exact-size heap block, coefficients in an exact-size heap block. Besides memory safety it checks the route's contract: status 0
// only with the host decoder accepting the same bytes and the planes equal bit for bit.
// `--list` as the first argument replays instead the fixed list of 32 mutations per file that tests/test_gpu_jpeg_entropy.py sends
// to the device (tests/jpeg_entropy_cases.py fixed_mutations: the same arithmetic), so that list passes here before it runs there.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../ovmono3d_amd/csrc/jpeg_dec_host.hpp"

static long ok = 0, declined_plan = 0, declined_status = 0, wrong = 0;

static void run_one(const std::vector<unsigned char>& d, int max_rounds) {
  unsigned char* buf = (unsigned char*)malloc(d.size() ? d.size() : 1);
  memcpy(buf, d.data(), d.size());
  OvmJpegInfo info, hinfo;
  if (ovm_jpeg::host_info(buf, d.size(), &info) == 0 && info.coef_blocks <= (1 << 18)) {
    const size_t ne = (size_t)info.coef_blocks * 64;
    int16_t* coef = (int16_t*)malloc(ne * 2);
    int32_t status = -1, rounds = -1;
    const int rc = ovm_jpeg_dec::host_emulate(buf, d.size(), max_rounds, coef, (int64_t)ne, &info, &status, &rounds);
    if (rc != 0) ++declined_plan;
    else if (status != 0) ++declined_status;
    else {
      int16_t* ref = (int16_t*)malloc(ne * 2);
      const int hrc = ovm_jpeg::host_entropy_decode(buf, d.size(), ref, (int64_t)ne, &hinfo);
      if (hrc != 0 || memcmp(ref, coef, ne * 2) != 0) {
        ++wrong;
        fprintf(stderr, "ACCEPTED BUT WRONG: host rc %d, %zu bytes\n", hrc, d.size());
      } else ++ok;
      free(ref);
    }
    free(coef);
  } else ++declined_plan;
  free(buf);
}

int main(int argc, char** argv) {
  std::vector<std::vector<unsigned char>> seeds;
  const bool list = argc > 1 && !strcmp(argv[1], "--list");
  for (int i = list ? 2 : 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    std::vector<unsigned char> b; int c;
    while ((c = fgetc(f)) != EOF) b.push_back((unsigned char)c);
    fclose(f); seeds.push_back(b);
  }
  if (seeds.empty()) { fprintf(stderr, "usage: fuzz_jpeg_dec seed.jpg ...\n"); return 2; }
  const long N = getenv("FUZZ_N") ? atol(getenv("FUZZ_N")) : 20000;      // FUZZ_N / FUZZ_SEED: longer runs with other streams
  std::mt19937 g(getenv("FUZZ_SEED") ? (unsigned)atol(getenv("FUZZ_SEED")) : 1u);
  for (const auto& sd : seeds) run_one(sd, 0);                           // the seeds themselves must pass
  const long seeds_ok = ok;
  if (list) {
    for (const auto& sd : seeds) {
      OvmJpegDecPlan P;
      if (ovm_jpeg_dec::host_plan(sd.data(), sd.size(), 0, &P, nullptr, 0) != 0) { fprintf(stderr, "seed declined by the plan\n"); return 2; }
      for (int m = 0; m < 32; ++m) {
        std::vector<unsigned char> d = sd;
        const size_t pos = (size_t)P.ecs_offset + (size_t)(((long long)m * 7919 + 13) * 31 % P.ecs_bytes);
        if (m % 4 == 3) d[pos] = 0xFF; else d[pos] ^= (unsigned char)(1u << (m & 7));
        run_one(d, 0);
      }
    }
    printf("seeds accepted %ld of %zu; listed mutations %zu: accepted and equal to the host decoder %ld, declined by the plan %ld, declined by status %ld, accepted but wrong %ld\n",
           seeds_ok, seeds.size(), 32 * seeds.size(), ok - seeds_ok, declined_plan, declined_status, wrong);
    return wrong ? 1 : 0;
  }
  for (long it = 0; it < N; ++it) {
    std::vector<unsigned char> d = seeds[it % seeds.size()];
    if (d.size() > 20000) { d.resize(20000); d[d.size() - 2] = 0xFF; d[d.size() - 1] = 0xD9; }
    // where the scan's data starts (0 if the plan declines the seed): most mutations go there, where the new code reads
    OvmJpegDecPlan P;
    size_t ecs = 2;
    if (ovm_jpeg_dec::host_plan(d.data(), d.size(), 0, &P, nullptr, 0) == 0) ecs = (size_t)P.ecs_offset;
    const int kind = g() % 6;
    if (kind <= 1) { int k = 1 + g() % 4; for (int j = 0; j < k; ++j) d[ecs + g() % (d.size() - ecs)] = (unsigned char)g(); }
    else if (kind == 2) { int k = 1 + g() % 6; for (int j = 0; j < k; ++j) d[2 + g() % (d.size() - 2)] = (unsigned char)g(); }
    else if (kind == 3) { d.resize(ecs + g() % (d.size() - ecs)); if (g() & 1) { d.push_back(0xFF); d.push_back(0xD9); } }
    else if (kind == 4) { size_t i = ecs + g() % (d.size() - ecs); int k = 1 + g() % 40; std::vector<unsigned char> ins(k); for (auto& x : ins) x = (g() % 4) ? (unsigned char)g() : (unsigned char)0xFF; d.insert(d.begin() + i, ins.begin(), ins.end()); }
    else { size_t i = 2 + g() % (d.size() - 10); d.erase(d.begin() + i, d.begin() + i + 1 + g() % 8); }
    run_one(d, (it % 7 == 0) ? 1 + (int)(g() % 4) : 0);
  }
  printf("seeds accepted %ld of %zu; mutated streams %ld: accepted and equal to the host decoder %ld, declined by the plan %ld, declined by status %ld, accepted but wrong %ld\n",
         seeds_ok, seeds.size(), N, ok - seeds_ok, declined_plan, declined_status, wrong);
  return wrong ? 1 : 0;
}
