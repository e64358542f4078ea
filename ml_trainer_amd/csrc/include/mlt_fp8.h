// OCP fp8 (e4m3 = 0 / e5m2 = 1) device helpers shared by the quantisation kernels (fp8.hip) and
// the GEMM epilogues that quantise their own output (gemm_tile.hip, "q8" epilogue).
#pragma once
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

template <int FMT>
__device__ __forceinline__ float fp8_max() {
  return FMT == 0 ? 448.f : 57344.f;
}

// Saturate to the format's finite range, +-inf included; a NaN stays a NaN. One v_med3_f32 would not keep it:
// with a NaN operand it returns min3 of the others, so NaN came out as -max, a finite value that neither the
// GEMM consuming the operand nor the amax (fmaxf drops NaN too) would ever notice. The IEEE-754-2019 maximum /
// minimum propagate NaN: v_maximum3_f32 + v_minimum3_f32, one instruction more than the med3 (a compare and a
// select around the med3 would be two more).
template <int FMT>
__device__ __forceinline__ float fp8_saturate(float x) {
  const float m = fp8_max<FMT>();
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(x, -m), m);
}

// 4 floats -> 4 saturated fp8 bytes (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32), byte i = value i; NaN -> the format's NaN
template <int FMT>
__device__ __forceinline__ uint32_t pack4_fp8(float a, float b, float c, float d) {
  a = fp8_saturate<FMT>(a);
  b = fp8_saturate<FMT>(b);
  c = fp8_saturate<FMT>(c);
  d = fp8_saturate<FMT>(d);
  int r;
  if constexpr (FMT == 0) {
    r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  } else {
    r = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, r, true);
  }
  return (uint32_t)r;
}

// amax is recorded into kAmaxSlots sub-slots (block b -> slot b % kAmaxSlots) so that thousands
// of blocks do not serialise on one device-scope atomic; update_scale reduces the slots.
// Slots sit kAmaxStride floats apart (one 128-B line each), and a block only issues the
// atomic when its maximum beats the slot's current value -- after the first few blocks almost
// none do, so the tail of thousands of same-line device-scope atomics disappears.
__device__ __forceinline__ void atomic_max_pos(float* slots, float v) {
  // |x| >= 0: IEEE ordering of non-negative floats equals their integer ordering
  unsigned* a = reinterpret_cast<unsigned*>(slots + ((blockIdx.x + blockIdx.y * gridDim.x) % kAmaxSlots) * kAmaxStride);
  const unsigned u = __float_as_uint(v);
  if (__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < u) atomicMax(a, u);
}

}  // namespace mlt
