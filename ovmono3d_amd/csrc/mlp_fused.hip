// Two-layer MLP of the detector's image branch in one kernel (f16x3 mode only):
//   P[chunk][m][n] = sum_{j in chunk} act(X[m][:] . W1[j][:] + b1[j]) * W2[n][j]          (fc1, activation and fc2's k-slice)
// followed by the split-K reduce that fc2 ends in anyway (splitk_epilogue_kernel: sums the slabs, adds b2, applies the residual).
// The hidden layer never leaves the chip: today's route writes it to memory as a split fp16 image and reads it back (19 MB per
// Swin stage-3 block) and pays a launch of 96-KB-LDS workgroups for fc1 alone.
//
// Grid: (row tile of 64) x (hidden chunk of 256), chunk fastest, so the workgroups of one XCD (id % 8) share one or two chunks'
// weights (512 KB of W1 + 512 KB of W2 at C = 512) in that XCD's L2.
//
// Workgroup: 8 waves as 2 (rows) x 4 (columns), 32 x 64 outputs each in both phases (32 accumulator registers, reused).
//   phase 1  H[64][256] = act(X[64][0..C) W1[chunk][0..C)^T + b1[chunk]), k-steps of 32 over all of C, per step the three passes
//            lo.hi, hi.lo, hi.hi into one fp32 accumulator in the order of every other GEMM here; H is split with split_f16 (the
//            EPI_GELU / EPI_STORE epilogues' routine), so it holds the values today's f1 image holds.
//   phase 2  for each block of 256 output columns: P = H W2[block][chunk]^T over the chunk's 8 k-groups, stored as fp32 to slab
//            `chunk` of the workspace [chunk][M][N] (what splitk_epilogue_kernel reads).
//
// LDS map (147,456 B of dynamic LDS, one workgroup per CU; every offset a multiple of 16):
//   [0, 81920)       two operand slots of 40 KB: A rows (64 x 128 B, phase 1 only) then W rows (256 x 128 B): one k-group of 32,
//                    each row [hi 32 | lo 32], 16-byte chunk c of row r at slot c ^ ((r >> 1) & 7) (gemm256.hip's frag_off: the
//                    LDS-DMA writes lane-linear 1-KB pieces, the swizzle is applied to the per-lane SOURCE address)
//   [81920, 147456)  H: 8 k-groups x (64 rows x 128 B) in the same row layout, so phase 2 reads its A fragments with the offsets
//                    phase 1 used for X (conflict-free ds_read_b128)
// Why 64 x 256: H costs rows x chunk x 4 B of LDS. 128 x 256 (128 KB) leaves no room for a second operand slot; 64 x 512 likewise;
// 128 x 128 fits a deeper ring but doubles the slabs (16 x M x N fp32 at stage 3: more traffic than the hidden layer it saves) and
// the workgroups. 64 x 256 gives 152 / 284 / 80 workgroups at Swin stages 3 / 2 / 4 of the headline shape and 8 / 4 / 16 slabs.
//
// Operand pipeline: one sequence of C / 32 + 8 ceil(N / 256) steps through the two slots; step s + 1 (the first W2 group included)
// is in flight while step s is multiplied. With one tile in flight the counted wait is vmcnt(0): every wave waits for its own pieces,
// then a barrier, and a slot is read only in the step after that barrier (RAW); it is restaged in the step after its last read,
// whose fragment reads have been waited for (lgkmcnt(0)) before that step's barrier (WAR). H is written after the last phase-1
// step's MFMAs and first read after the barrier that ends that step.
// Rows past M: the load row is clamped and the store skipped (no dot-product tail workgroups). Columns past N (N % 256 != 0):
// the W2 row is clamped and the store skipped.
#include <hip/hip_runtime.h>
#include "gemm.hpp"
#include "gdino.hpp"

namespace ovm {

namespace {

constexpr int kBM = 64;                        // rows per workgroup
constexpr int kHC = 256;                       // hidden columns per workgroup
constexpr int kKG = kHC / 32;                  // k-groups of phase 2
constexpr int kBN = 256;                       // output columns per phase-2 block
constexpr int kSlot = (kBM + 256) * 128;       // one operand slot
constexpr int kOffW = kBM * 128;               // W rows inside a slot
constexpr int kOffH = 2 * kSlot;
constexpr int kHGroup = kBM * 128;             // one k-group of H
constexpr int kSmem = kOffH + kKG * kHGroup;
static_assert(kSmem <= 160 * 1024 && kSlot % 16 == 0 && kOffH % 16 == 0, "LDS map");

__device__ __forceinline__ int frag_off(int row, int chunk) { return row * 128 + (chunk ^ ((row >> 1) & 7)) * 16; }

// ACT: 1 = ReLU, 2 = GELU(erf)  (GemmParams::relu's codes)
template <int ACT>
__global__ __launch_bounds__(512) void mlp_fused_kernel(const MlpFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunks = p.hidden / kHC;
  const int chunk = (int)blockIdx.x % chunks, m0 = ((int)blockIdx.x / chunks) * kBM;
  const int N = p.C;
  const int S1 = p.C / 32;                                   // phase-1 steps
  const int S = S1 + ((N + kBN - 1) / kBN) * kKG;
  const size_t ldw1 = 2 * (size_t)p.C, ldw2 = 2 * (size_t)p.hidden;

  // ---- staging: a wave-instruction moves 8 rows x 128 B; wave w moves piece w of A and pieces w, w + 8, w + 16, w + 24 of W
  const int srow = lane >> 3, sslot = lane & 7;
  size_t aoff, w1off[4];
  int w2row[4], w2col[4];
  {
    const int row = wave * 8 + srow;
    int m = m0 + row; if (m > p.M - 1) m = p.M - 1;
    aoff = (size_t)m * p.ldx + (sslot ^ ((row >> 1) & 7)) * 8;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (wave + 8 * q) * 8 + srow;
    const int ch = sslot ^ ((row >> 1) & 7);
    w1off[q] = (size_t)(chunk * kHC + row) * ldw1 + ch * 8;
    w2row[q] = row;
    w2col[q] = chunk * kKG * 64 + ch * 8;
  }
  auto stage = [&](int s) {
    char* base = smem + (s & 1) * kSlot;
    if (s < S1) {
      glds16(p.X + aoff + (size_t)s * 64, base + wave * 1024);
#pragma unroll
      for (int q = 0; q < 4; ++q) glds16(p.W1 + w1off[q] + (size_t)s * 64, base + kOffW + (wave + 8 * q) * 1024);
    } else {
      const int s2 = s - S1, nb = s2 / kKG, g = s2 % kKG;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int n = nb * kBN + w2row[q]; if (n > N - 1) n = N - 1;
        glds16(p.W2 + (size_t)n * ldw2 + w2col[q] + g * 64, base + kOffW + (wave + 8 * q) * 1024);
      }
    }
  };

  // ---- fragments (16x16x32 operands: lane (fr, fq) holds k = 8 fq .. 8 fq + 7 of row fr; hi chunk fq, lo chunk 4 + fq)
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave >> 2, wn = wave & 3;
  int oa_hi[2], oa_lo[2], ow_hi[4], ow_lo[4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int row = wm * 32 + mi * 16 + fr;
    oa_hi[mi] = frag_off(row, fq); oa_lo[mi] = frag_off(row, 4 + fq);
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int row = wn * 64 + ni * 16 + fr;
    ow_hi[ni] = kOffW + frag_off(row, fq); ow_lo[ni] = kOffW + frag_off(row, 4 + fq);
  }
  f32x4 acc[2][4];
  auto zero = [&]() {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  // W rows on the MFMA "A" side, activation rows on the "B" side: a lane's 4 accumulator registers run along n
  auto mma = [&](const char* abase, const char* wbase) {
    half8 ah[2], al[2], wh[4], wl[4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) { ah[mi] = *(const half8*)(abase + oa_hi[mi]); al[mi] = *(const half8*)(abase + oa_lo[mi]); }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) { wh[ni] = *(const half8*)(wbase + ow_hi[ni]); wl[ni] = *(const half8*)(wbase + ow_lo[ni]); }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        f32x4 c = acc[mi][ni];
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ni], ah[mi], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ni], al[mi], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ni], ah[mi], c, 0, 0, 0);
        acc[mi][ni] = c;
      }
  };

  zero();
  stage(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    if (s + 1 < S) stage(s + 1);
    const char* slot = smem + (s & 1) * kSlot;
    if (s < S1) {
      mma(slot, slot);
      if (s == S1 - 1) {
        // H = act(acc + b1), split: the lane's 4 columns are 8 bytes of one 16-byte chunk of k-group (column / 32)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int hc = wn * 64 + ni * 16 + fq * 4;
          const f32x4 b = p.b1 ? *(const f32x4*)(p.b1 + chunk * kHC + hc) : (f32x4){0.f, 0.f, 0.f, 0.f};
          char* hg = smem + kOffH + (hc >> 5) * kHGroup + (fq & 1) * 8;
          const int c = (ni & 1) * 2 + (fq >> 1);
#pragma unroll
          for (int mi = 0; mi < 2; ++mi) {
            const int row = wm * 32 + mi * 16 + fr;
            half4 h, l;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float z = acc[mi][ni][r] + b[r];
              half_t hh, ll; split_f16(ACT == 2 ? gelu_erf(z) : fmaxf(z, 0.f), hh, ll); h[r] = hh; l[r] = ll;
            }
            *(half4*)(hg + frag_off(row, c)) = h;
            *(half4*)(hg + frag_off(row, 4 + c)) = l;
          }
        }
        zero();
      }
    } else {
      const int s2 = s - S1, nb = s2 / kKG, g = s2 % kKG;
      mma(smem + kOffH + g * kHGroup, slot);
      if (g == kKG - 1) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const int m = m0 + wm * 32 + mi * 16 + fr;
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const int n = nb * kBN + wn * 64 + ni * 16 + fq * 4;
            if (m < p.M && n < N) *(f32x4*)(p.part + ((size_t)chunk * p.M + m) * N + n) = acc[mi][ni];
          }
        }
        zero();
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

}  // namespace

bool mlp_fused_supported(int M, int C, int hidden, int act, int npass) {
  return npass == 3 && M >= 1 && C >= 32 && C % 32 == 0 && hidden >= kHC && hidden % kHC == 0 && (act == 1 || act == 2) &&
         ((long)(M + kBM - 1) / kBM) * (hidden / kHC) <= 0x7fffffffL;
}

size_t mlp_fused_ws_bytes(int M, int C, int hidden) { return (size_t)(hidden / kHC) * M * C * sizeof(float); }

int launch_mlp_fused(const MlpFusedParams& p, const GemmParams& out, int epi, hipStream_t s) {
  if (!mlp_fused_supported(p.M, p.C, p.hidden, p.act, 3) || (epi != EPI_RESID && epi != EPI_STORE)) return OVM_ERR_INVALID;
  if (!p.X || !p.W1 || !p.W2 || !p.part || p.ldx < 2 * p.C || p.ldx % 8 != 0) return OVM_ERR_INVALID;
  if ((((uintptr_t)p.X) | ((uintptr_t)p.W1) | ((uintptr_t)p.W2) | ((uintptr_t)p.part) | ((uintptr_t)p.b1)) & 15) return OVM_ERR_INVALID;
  if (epi == EPI_RESID ? !out.X : (!out.C && !out.Ohi)) return OVM_ERR_INVALID;
  if (p.part_cap < mlp_fused_ws_bytes(p.M, p.C, p.hidden)) return OVM_ERR_CAPACITY;
  const int chunks = p.hidden / kHC, tiles = (p.M + kBM - 1) / kBM;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)mlp_fused_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) != hipSuccess ||
        hipFuncSetAttribute((const void*)mlp_fused_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) != hipSuccess)
      return OVM_ERR_HIP;
    attr_set = true;
  }
  if (p.act == 2) hipLaunchKernelGGL((mlp_fused_kernel<2>), dim3(tiles * chunks), dim3(512), kSmem, s, p);
  else hipLaunchKernelGGL((mlp_fused_kernel<1>), dim3(tiles * chunks), dim3(512), kSmem, s, p);
  // second launch: today's reduce over the slabs, with fc2's bias, residual and output forms
  GemmParams q = out;
  q.M = p.M; q.N = p.C; q.K = p.hidden; q.ksplit = chunks; q.kchunk = kKG; q.part = p.part;
  const long n = (long)p.M * (p.C / 4);
  if (epi == EPI_RESID) hipLaunchKernelGGL((splitk_epilogue_kernel<EPI_RESID>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q);
  else hipLaunchKernelGGL((splitk_epilogue_kernel<EPI_STORE>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q);
  return hipGetLastError() == hipSuccess ? OVM_OK : OVM_ERR_HIP;
}

}  // namespace ovm
