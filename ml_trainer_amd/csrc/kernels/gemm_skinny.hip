// Weight-streaming bf16 GEMM for the few rows of a decode step (1 <= M <= kSkinnyMaxRows):
//   Y[M, N] = epilogue(X[M, K] . W[N, K]^T),  W k-contiguous as a linear layer stores it, N % 16 == 0, K % 32 == 0.
// Every linear of a decode step is bounded by how fast one launch gets its weights moving, not by FLOPs; the
// tile kernels (gemm.hip, gemm_tile.hip, gemm_w4.hip) stage 128 / 256-row tiles of BOTH operands through LDS
// and leave most CUs idle at these shapes.
//
// Arithmetic: v_mfma_f32_16x16x32_bf16 with the operands swapped (as gemm_w4.hip). W is the A operand: lane l
// holds W[n0 + (l & 15)][k0 + 8 (l >> 4) .. + 7], which is ONE 16-byte global load -- the load is the operand, no
// LDS staging, no global_load_lds. X is the B operand (the tokens are the MFMA columns), loaded in the same
// shape from L2, where every workgroup finds it again (X is at most 64 x K bf16). The accumulator of lane l is
// token l & 15, output columns n0 + 4 (l >> 4) .. + 3: four consecutive columns of one row, which is what
// epilogue_store4 (mlt_gemm.h) takes -- bias, GELU with the saved pre-activation, residual and the bf16 / fp32
// store have the bits of every other GEMM here. M = 1 and M = 16 cost the same MFMAs and no VALU work.
//
// Rows: a 16-row group's tokens m >= M are SELECTED to zero (never loaded) and never stored. An MFMA column
// does not mix into another column, so this is memory safety, not arithmetic. M in 17 .. 64 runs MG = 2 or 4
// accumulator sets against the same W fragments.
//
// Partition -- a function of (N, K) only, never of M, so a token's result does not depend on its batch:
//   * one workgroup per 16 output columns (grid N / 16), kSkWaves waves;
//   * 32-k step s belongs to wave (s >> 1) % kSkWaves: a wave takes PAIRS of adjacent steps, so the loads it has
//     in flight for one weight row cover whole 128-byte lines, and the workgroup's waves together stream
//     kSkWaves x 128 contiguous bytes of each row;
//   * a wave accumulates its steps in increasing order, kSkBatch steps' loads in flight before the first wait
//     (a batch's surplus slots re-load the wave's last step and skip the MFMA: no arithmetic effect);
//   * the waves' partials are summed through LDS in wave order 0, 1, 2, ..., then the epilogue.
// No float atomics, no arrival counters, no workspace: the launch allocates nothing and does not synchronise.
// Cross-workgroup split-K is not done: N = 768 occupies 48 CUs (profiles/generate/README.md has the figure).
//
// X straight from L2, no LDS copy: with one column group per workgroup the waves own disjoint k steps, so every
// X element a workgroup needs is used by exactly one wave, once. An LDS copy would move the same bytes out of
// L2, add a barrier in front of the first MFMA and share nothing. (It pays once a workgroup owns several column
// groups; that is also what the M = 64 rows of the table in profiles/generate/README.md ask for.)
//
// Registers (-Rpass-analysis=kernel-resource-usage, bf16 and fp32 output alike), scratch 0 everywhere:
//   MG = 1:  60 VGPRs +  4 AGPRs,  4 KB LDS, 8 waves per SIMD
//   MG = 2:  94 VGPRs +  8 AGPRs,  8 KB LDS, 4 waves per SIMD
//   MG = 4: 150 VGPRs + 20 AGPRs, 16 KB LDS, 2 waves per SIMD
// The registers are the kSkBatch x (1 + MG) fragments in flight. Waves per SIMD decide little here: the layer
// shapes launch 48 - 192 workgroups on 256 CUs (one 4-wave workgroup per CU, one wave per SIMD, whatever the
// limit), and what hides the latency is the 12 - 30 loads each wave has outstanding. Only the vocabulary decoder
// (1,920 workgroups, 7.5 per CU) fills a CU: with MG = 1 all of them are resident at once.
#include "mlt_common.h"
#include "mlt_gemm.h"
#include "mlt_kernels.h"

namespace mlt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSkWaves = 4;  // waves of a workgroup: they split the 32-k steps
constexpr int kSkBatch = 6;  // steps (3 pairs) a wave loads before its first wait: K = 768 is one batch per wave

template <typename OutT, int MG>
__global__ __launch_bounds__(kSkWaves * 64) void gemm_skinny_kernel(const uint16_t* __restrict__ X,
                                                                     const uint16_t* __restrict__ W,
                                                                     OutT* __restrict__ Y, int M, int N, int K,
                                                                     int64_t ldx, int64_t ldw, int64_t ldy,
                                                                     GemmEpi epi) {
  __shared__ f32x4 red[kSkWaves][MG][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 16;

  // this wave's steps: its j-th is step 2 (w + (j >> 1) kSkWaves) + (j & 1); nj of them lie below K / 32
  const int nsteps = K >> 5, npairs = nsteps >> 1;
  int nj = npairs > w ? 2 * ((npairs - w + kSkWaves - 1) / kSkWaves) : 0;
  if ((nsteps & 1) && npairs % kSkWaves == w) ++nj;  // the odd last step: after every full pair of its wave
  auto step_of = [&](int j) { return 2 * (w + (j >> 1) * kSkWaves) + (j & 1); };

  const uint16_t* wp = W + (int64_t)(n0 + r) * ldw + 8 * kq;
  const uint16_t* xp[MG];
  bool live[MG];
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    live[g] = 16 * g + r < M;
    xp[g] = X + (int64_t)(16 * g + r) * ldx + 8 * kq;
  }

  f32x4 acc[MG];
#pragma unroll
  for (int g = 0; g < MG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < nj; j0 += kSkBatch) {
    bf16x8 wf[kSkBatch], xf[MG][kSkBatch];
    int koff[kSkBatch];
#pragma unroll
    for (int u = 0; u < kSkBatch; ++u) {
      koff[u] = 32 * step_of(min(j0 + u, nj - 1));
      wf[u] = *reinterpret_cast<const bf16x8*>(wp + koff[u]);
    }
#pragma unroll
    for (int g = 0; g < MG; ++g) {
#pragma unroll
      for (int u = 0; u < kSkBatch; ++u) xf[g][u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live[g]) {
#pragma unroll
        for (int u = 0; u < kSkBatch; ++u) xf[g][u] = *reinterpret_cast<const bf16x8*>(xp[g] + koff[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kSkBatch; ++u) {
      if (j0 + u < nj) {  // wave-uniform
#pragma unroll
        for (int g = 0; g < MG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], xf[g][u], acc[g], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int g = 0; g < MG; ++g) red[w][g][lane] = acc[g];
  __syncthreads();
  if (w >= MG) return;
  // wave g finishes row group g: the partials in wave order, then the shared epilogue
  f32x4 s = red[0][w][lane];
#pragma unroll
  for (int i = 1; i < kSkWaves; ++i) s += red[i][w][lane];
  const int gm = 16 * w + r, gn = n0 + 4 * kq;
  if (gm >= M) return;
  float vv[4] = {s[0], s[1], s[2], s[3]};
  if (epi.bias) {
#pragma unroll
    for (int q = 0; q < 4; ++q) vv[q] += epi.bias[gn + q];
  }
  epilogue_store4<OutT>(Y, ldy, epi, gm, gn, N, vv);
}

void launch_gemm_skinny(const uint16_t* X, const uint16_t* W, void* Y, bool out_f32, int M, int N, int K, int64_t ldx,
                        int64_t ldw, int64_t ldy, const float* bias, const uint16_t* aux, int64_t ldaux,
                        const uint16_t* res, int64_t ldres, int mode, hipStream_t st) {
  GemmEpi e{};
  e.bias = bias;
  e.aux = aux;
  e.ldaux = ldaux;
  e.res = res;
  e.ldres = ldres;
  e.alpha = 1.f;
  e.mode = mode;
  const int mg = M <= 16 ? 1 : M <= 32 ? 2 : M <= kSkinnyMaxRows ? 4 : 0;
  const bool hit = dispatch_int<1, 2, 4>(mg, [&](auto g) {
    dispatch_bools(
        [&](auto f32) {
          using OutT = std::conditional_t<decltype(f32)::value, float, uint16_t>;
          auto kern = gemm_skinny_kernel<OutT, decltype(g)::value>;
          hipLaunchKernelGGL(kern, dim3(N / 16), dim3(kSkWaves * 64), 0, st, X, W, reinterpret_cast<OutT*>(Y), M, N, K,
                             ldx, ldw, ldy, e);
        },
        out_f32);
  });
  if (!hit) throw_no_kernel("launch_gemm_skinny", "row groups", mg);
}

}  // namespace mlt
