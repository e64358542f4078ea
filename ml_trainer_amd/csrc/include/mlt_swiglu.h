// SwiGLU: the one device definition every kernel of the gated feed-forward calls (swiglu.hip, the gated decode
// GEMM of gemm_skinny.hip). ops/swiglu.py is the same function in plain torch.
//
//   s = 1 / (1 + exp(-g))            a  = bf16_rn((g * s) * u)
//   du = bf16_rn(da * (g * s))       dg = bf16_rn((da * u) * (s * (1 + g * (1 - s))))
//
// g, u, da are bf16 values widened to fp32 (exact). exp is v_exp_f32 on g * -log2(e) and the reciprocal v_rcp_f32
// (1 ulp each in the ISA manual); every product and sum rounds to fp32 on its own (contraction off, as rope.hip),
// so two kernels that call these cannot differ by an fma. The ends of the range need no branch: below g ~ -88.7
// exp2 returns +inf, 1 + inf = inf and rcp(inf) = 0, so s = 0, a = +-0 and dg = +-0; for large g exp2 returns 0
// (v_exp_f32 flushes a denormal result) and s = 1, a = g * u, dg = da * u. A reciprocal below 2^-126 is flushed to
// 0 as well: s carries an absolute error below 2^-126 there.
#pragma once
#include "mlt_common.h"

namespace mlt {

// round to nearest even on the hardware convert; a builtin, so it inlines into kernels with target features of their own
__device__ __forceinline__ uint16_t glu_bf16(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }

__device__ __forceinline__ float glu_sigmoid(float g) {
#pragma clang fp contract(off)
  const float e = __builtin_amdgcn_exp2f(g * -1.4426950408889634f);
  return __builtin_amdgcn_rcpf(1.0f + e);
}

// (g * s) * u in fp32, not yet rounded to bf16
__device__ __forceinline__ float swiglu_act(float g, float u) {
#pragma clang fp contract(off)
  const float s = glu_sigmoid(g);
  return (g * s) * u;
}

__device__ __forceinline__ void swiglu_grad(float da, float g, float u, float& dg, float& du) {
#pragma clang fp contract(off)
  const float s = glu_sigmoid(g);
  du = da * (g * s);
  dg = (da * u) * (s * (1.0f + g * (1.0f - s)));
}

// 8 bf16 of a 16-byte chunk <-> 8 fp32 (widening is exact)
__device__ __forceinline__ void glu_unpack(const uint4& r, float* f) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 glu_pack(const uint16_t* h) {
  uint4 r;
  r.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
  r.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
  r.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
  r.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
  return r;
}

}  // namespace mlt
