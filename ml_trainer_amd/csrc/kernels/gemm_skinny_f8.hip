// Weight-streaming GEMM for the few rows of a decode step with fp8 WEIGHTS (weight-only quantisation):
//   Y[M, N] = epilogue((X[M, K] . value(W8[N, K])^T) * d[N]),  1 <= M <= kSkinnyMaxRows, N % 16 == 0, K % 32 == 0.
// W8 holds OCP e4m3 codes, k-contiguous, rows 16-byte aligned; d is one fp32 power-of-two scale per output row
// (ops/decode.py: weight_quantize_reference). X stays bf16 and the accumulation fp32. gemm_skinny.hip is the bf16
// form: its header says why a decode linear is bounded by how fast its weights arrive; here they are half the bytes.
//
// Exactness. value(code) has 3 mantissa bits and lies in bf16's range, so the conversion to the MFMA operand is
// exact, and d is a power of two, so multiplying the finished fp32 accumulator by it is exact (outside the
// subnormal range). The kernel therefore computes the bf16 layer whose weight is dequant(W8, d): with operands
// whose partial sums are exact it has gemm_skinny's bits on that weight (tests/test_gemm_skinny_f8_gpu.py).
//
// Weight fragment. v_mfma_f32_16x16x32_bf16 with W as the A operand, as gemm_skinny.hip. The unit of work is a
// DOUBLE step of 64 k: lane l holds row n0 + (l & 15) and loads the 16 codes of k = 64 s + 16 (l >> 4) .. + 15 in ONE
// 16-byte load. Codes 0 .. 7 become the A fragment of a first MFMA and codes 8 .. 15 of a second, each through four
// v_cvt_scalef32_pk_bf16_fp8 (two codes -> two packed bf16, scale operand 1.0: the row scale waits for the epilogue).
// X is loaded with the matching k: 32 contiguous bytes per lane, two B fragments. Inside one MFMA the lanes'
// k ranges are 16 apart, not 8; both operands agree on them and the sum is over the same 32 products.
// K % 64 == 32 leaves one 32-k TAIL step: an 8-byte weight load, 16 bytes of X, one MFMA.
//
// Partition -- a function of (N, K) only, never of M, so a token's result does not depend on its batch:
//   * one workgroup per 16 output columns (grid N / 16), kF8Waves waves;
//   * double step s belongs to wave (s >> 1) % kF8Waves: a wave takes PAIRS of adjacent double steps, so the loads it
//     has in flight on one weight row cover whole 128-byte lines; the tail step belongs to the wave after the one
//     that took the last double step;
//   * a wave accumulates its steps in increasing k (the tail last), kF8Batch double steps' loads in flight before
//     the first wait (surplus slots re-load the wave's last double step and skip the MFMAs);
//   * the waves' partials are summed through LDS in wave order 0, 1, 2, ..., then scale, bias, epilogue_store4.
// No atomics, no workspace. Tokens m >= M are selected to zero, never loaded and never stored.
//
// Loads in flight: kF8Batch = 4 double steps = 4 weight + 8 X loads per wave and row group, the count gemm_skinny
// keeps (6 + 6) over 256 k instead of 192; K = 768 is one batch for every wave. Measured against 6
// (profiles/skinny_f8/README.md): 6 is 3 - 8 % faster at K = 3072 and 13 - 15 % slower on the gated form at K = 768,
// whose waves own at most 4 double steps and would re-load surplus slots.
//
// Registers (-Rpass-analysis=kernel-resource-usage), scratch 0 everywhere; the table stands at each kernel.
#include "mlt_common.h"
#include "mlt_gemm.h"
#include "mlt_kernels.h"
#include "mlt_swiglu.h"

namespace mlt {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kF8Waves = 4;  // waves of a workgroup: they split the double steps
constexpr int kF8Batch = 4;  // double steps (2 pairs) whose loads a wave issues before its first wait

// eight e4m3 codes (k ascending from byte 0 of lo) -> the bf16x8 MFMA fragment; exact
__device__ __forceinline__ bf16x8 f8x8_to_bf16(uint32_t lo, uint32_t hi) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  const bf16x4 ab = __builtin_shufflevector(a, b, 0, 1, 2, 3);
  const bf16x4 cd = __builtin_shufflevector(c, d, 0, 1, 2, 3);
  return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The k loop of both kernels: acc[s][g] += X (row group g) . value(W8 rows n0 + r + s * wrows)^T over this wave's
// steps. NW weight streams (1; 2 = gate | up) share every X fragment. Builtins only: it inlines into the gated
// kernel, which has target features of its own.
template <int NW, int MG>
__device__ __forceinline__ void skinny_f8_accumulate(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                     int M, int wrows, int K, int64_t ldx, int64_t ldw, int n0,
                                                     int lane, int w, f32x4 (&acc)[NW][MG]) {
  const int r = lane & 15, kq = lane >> 4;
  // this wave's double steps: its j-th is 2 (w + (j >> 1) kF8Waves) + (j & 1); nj of them lie below K / 64
  const int nd = K >> 6, npairs = nd >> 1;
  int nj = npairs > w ? 2 * ((npairs - w + kF8Waves - 1) / kF8Waves) : 0;
  if ((nd & 1) && npairs % kF8Waves == w) ++nj;  // the odd last double step: after every full pair of its wave

  const uint8_t* wp[NW];
#pragma unroll
  for (int s = 0; s < NW; ++s) wp[s] = W + (int64_t)(n0 + r + s * wrows) * ldw;
  const uint16_t* xp[MG];
  bool live[MG];
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    live[g] = 16 * g + r < M;
    xp[g] = X + (int64_t)(16 * g + r) * ldx;
  }
#pragma unroll
  for (int s = 0; s < NW; ++s) {
#pragma unroll
    for (int g = 0; g < MG; ++g) acc[s][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int j0 = 0; j0 < nj; j0 += kF8Batch) {
    uint4 wf[NW][kF8Batch];
    bf16x8 xf[MG][kF8Batch][2];
    int koff[kF8Batch];
#pragma unroll
    for (int u = 0; u < kF8Batch; ++u) {
      const int j = j0 + u < nj ? j0 + u : nj - 1;  // surplus slots re-load the wave's last double step
      koff[u] = 64 * (2 * (w + (j >> 1) * kF8Waves) + (j & 1)) + 16 * kq;
#pragma unroll
      for (int s = 0; s < NW; ++s) wf[s][u] = *reinterpret_cast<const uint4*>(wp[s] + koff[u]);
    }
#pragma unroll
    for (int g = 0; g < MG; ++g) {
#pragma unroll
      for (int u = 0; u < kF8Batch; ++u) xf[g][u][0] = xf[g][u][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live[g]) {
#pragma unroll
        for (int u = 0; u < kF8Batch; ++u) {
          xf[g][u][0] = *reinterpret_cast<const bf16x8*>(xp[g] + koff[u]);
          xf[g][u][1] = *reinterpret_cast<const bf16x8*>(xp[g] + koff[u] + 8);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kF8Batch; ++u) {
      if (j0 + u < nj) {  // wave-uniform
#pragma unroll
        for (int s = 0; s < NW; ++s) {
          const bf16x8 a0 = f8x8_to_bf16(wf[s][u].x, wf[s][u].y), a1 = f8x8_to_bf16(wf[s][u].z, wf[s][u].w);
#pragma unroll
          for (int g = 0; g < MG; ++g) {
            acc[s][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf[g][u][0], acc[s][g], 0, 0, 0);
            acc[s][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf[g][u][1], acc[s][g], 0, 0, 0);
          }
        }
      }
    }
  }

  // the 32-k tail step of K % 64 == 32: lane l holds k = 64 nd + 8 (l >> 4) .. + 7, gemm_skinny's own mapping
  if ((K & 32) && (npairs + (nd & 1)) % kF8Waves == w) {  // wave-uniform
    const int kt = 64 * nd + 8 * kq;
    uint2 wt[NW];
#pragma unroll
    for (int s = 0; s < NW; ++s) wt[s] = *reinterpret_cast<const uint2*>(wp[s] + kt);
    bf16x8 xt[MG];
#pragma unroll
    for (int g = 0; g < MG; ++g) {
      xt[g] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (live[g]) xt[g] = *reinterpret_cast<const bf16x8*>(xp[g] + kt);
    }
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const bf16x8 a = f8x8_to_bf16(wt[s].x, wt[s].y);
#pragma unroll
      for (int g = 0; g < MG; ++g) acc[s][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xt[g], acc[s][g], 0, 0, 0);
    }
  }
}

// Registers, bf16 and fp32 output alike:
//   MG = 1:  64 VGPRs +  4 AGPRs,  4 KB LDS, 7 waves per SIMD
//   MG = 2:  98 VGPRs + 16 AGPRs,  8 KB LDS, 4 waves per SIMD
//   MG = 4: 166 VGPRs + 32 AGPRs, 16 KB LDS, 2 waves per SIMD
template <typename OutT, int MG>
__global__ __launch_bounds__(kF8Waves * 64) void gemm_skinny_f8_kernel(const uint16_t* __restrict__ X,
                                                                       const uint8_t* __restrict__ W,
                                                                       const float* __restrict__ wscale,
                                                                       OutT* __restrict__ Y, int M, int N, int K,
                                                                       int64_t ldx, int64_t ldw, int64_t ldy,
                                                                       GemmEpi epi) {
  __shared__ f32x4 red[kF8Waves][MG][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * 16;

  f32x4 acc[1][MG];
  skinny_f8_accumulate<1, MG>(X, W, M, 0, K, ldx, ldw, n0, lane, w, acc);

#pragma unroll
  for (int g = 0; g < MG; ++g) red[w][g][lane] = acc[0][g];
  __syncthreads();
  if (w >= MG) return;
  // wave g finishes row group g: the partials in wave order, the row scales, then the shared epilogue
  f32x4 s = red[0][w][lane];
#pragma unroll
  for (int i = 1; i < kF8Waves; ++i) s += red[i][w][lane];
  const int gm = 16 * w + (lane & 15), gn = n0 + 4 * (lane >> 4);
  if (gm >= M) return;
  float vv[4];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) vv[q] = s[q] * wscale[gn + q];
    if (epi.bias) {
#pragma unroll
      for (int q = 0; q < 4; ++q) vv[q] += epi.bias[gn + q];
    }
  }
  epilogue_store4<OutT>(Y, ldy, epi, gm, gn, N, vv);
}

void launch_gemm_skinny_f8(const uint16_t* X, const uint8_t* W8, const float* wscale, void* Y, bool out_f32, int M,
                           int N, int K, int64_t ldx, int64_t ldw, int64_t ldy, const float* bias, const uint16_t* aux,
                           int64_t ldaux, const uint16_t* res, int64_t ldres, int mode, hipStream_t st) {
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
          auto kern = gemm_skinny_f8_kernel<OutT, decltype(g)::value>;
          hipLaunchKernelGGL(kern, dim3(N / 16), dim3(kF8Waves * 64), 0, st, X, W8, wscale, reinterpret_cast<OutT*>(Y),
                             M, N, K, ldx, ldw, ldy, e);
        },
        out_f32);
  });
  if (!hit) throw_no_kernel("launch_gemm_skinny_f8", "row groups", mg);
}

// The gated FFN1 of a decode step on fp8 weights: Y[M, F] = swiglu(bf16(g), bf16(u)) with
// g = (X . value(W8[0:F])^T) * d[0:F] + bias[0:F] and u the same over rows F .. 2F - 1 of the layer's one [2F, K]
// weight. The partition is gemm_skinny_f8_kernel's with N = F; each double step loads TWO weight fragments and one
// X fragment pair. Epilogue: both sets in wave order, the two scale slices, the two bias slices, g and u each
// rounded to bf16, the shared device function of mlt_swiglu.h: the rounding and activation sequence of
// gemm_skinny_glu_kernel. The output EQUALS, bit for bit, gemm_skinny_f8 with N = 2F followed by swiglu_fwd.
//
// no-packed-fp32-ops as gemm_skinny_glu_kernel, so the body uses builtins and __forceinline__ helpers only.
//
// Registers:
//   MG = 1:  82 VGPRs + 16 AGPRs,  8 KB LDS, 4 waves per SIMD
//   MG = 2: 116 VGPRs + 20 AGPRs, 16 KB LDS, 3 waves per SIMD
//   MG = 4: 184 VGPRs + 36 AGPRs, 32 KB LDS, 2 waves per SIMD
template <int MG>
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kF8Waves * 64) void gemm_skinny_glu_f8_kernel(const uint16_t* __restrict__ X,
                                                                const uint8_t* __restrict__ W,
                                                                const float* __restrict__ wscale,
                                                                uint16_t* __restrict__ Y, int M, int F, int K,
                                                                int64_t ldx, int64_t ldw, int64_t ldy,
                                                                const float* __restrict__ bias) {
  __shared__ f32x4 red[kF8Waves][2][MG][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * 16;

  f32x4 acc[2][MG];
  skinny_f8_accumulate<2, MG>(X, W, M, F, K, ldx, ldw, n0, lane, w, acc);

#pragma unroll
  for (int g = 0; g < MG; ++g) {
    red[w][0][g][lane] = acc[0][g];
    red[w][1][g][lane] = acc[1][g];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (w >= MG) return;
  f32x4 sg = red[0][0][w][lane], su = red[0][1][w][lane];
#pragma unroll
  for (int i = 1; i < kF8Waves; ++i) {
    sg += red[i][0][w][lane];
    su += red[i][1][w][lane];
  }
  const int gm = 16 * w + (lane & 15), gn = n0 + 4 * (lane >> 4);
  if (gm >= M) return;
  float vg[4], vu[4];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vg[q] = sg[q] * wscale[gn + q];
      vu[q] = su[q] * wscale[F + gn + q];
    }
    if (bias) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        vg[q] += bias[gn + q];
        vu[q] += bias[F + gn + q];
      }
    }
  }
  uint16_t o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    o[q] = glu_bf16(swiglu_act(bf16_to_f32(glu_bf16(vg[q])), bf16_to_f32(glu_bf16(vu[q]))));
  uint2 st;
  st.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
  st.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
  *reinterpret_cast<uint2*>(Y + (int64_t)gm * ldy + gn) = st;
}

void launch_gemm_skinny_glu_f8(const uint16_t* X, const uint8_t* W8, const float* wscale, uint16_t* Y, int M, int F,
                               int K, int64_t ldx, int64_t ldw, int64_t ldy, const float* bias, hipStream_t st) {
  const int mg = M <= 16 ? 1 : M <= 32 ? 2 : M <= kSkinnyMaxRows ? 4 : 0;
  const bool hit = dispatch_int<1, 2, 4>(mg, [&](auto g) {
    hipLaunchKernelGGL(gemm_skinny_glu_f8_kernel<decltype(g)::value>, dim3(F / 16), dim3(kF8Waves * 64), 0, st, X, W8,
                       wscale, Y, M, F, K, ldx, ldw, ldy, bias);
  });
  if (!hit) throw_no_kernel("launch_gemm_skinny_glu_f8", "row groups", mg);
}

}  // namespace mlt
