// Device helpers of the fp8 key/value cache (attn_decode_f8.hip): the row quantiser that the append of a decode
// step and the prefill fill share, and the hardware fp8 -> fp32 unpack of a cached fragment.
//
// The format (its one definition is kv_quantize_reference in ops/decode.py): a cached row of 64 values is 64 OCP
// e4m3 codes plus ONE fp32 scale d = 2^e kept in a tensor of its own, e = max(E - 7, -126) with E the unbiased fp32
// exponent of amax = max |x|, and d = 1 where amax is 0 or not finite. code = e4m3(x * 2^-e) with pack4_fp8<0>'s
// rounding and saturation. A power of two makes the product before the cast and value(code) * d exact, puts the
// scaled amax into [128, 256) (nothing saturates), and lets the kernel apply the scale to a finished dot product.
//
// A row lies over a QUAD of lanes, 16 dims = 16 code bytes = one 16-byte load per lane: lane c = lane & 3 owns dims
// 16 c .. 16 c + 15. Everything that crosses lanes is a quad_perm DPP.
#pragma once
#include "mlt_attn_decode.h"
#include "mlt_fp8.h"

namespace mlt {

constexpr int kF8Lanes = 4;                              // lanes per key (a quad)
constexpr int kF8Dims = kDecHead / kF8Lanes;             // dims per lane: 16 code bytes
constexpr int kF8Groups = 64 / kF8Lanes;                 // keys per wave load: 16 rows, 1 KiB contiguous
constexpr int kF8WaveKeys = kF8Groups * kDecUnroll;      // 64 keys per wave per step
constexpr int kF8BlockKeys = kDecWaves * kF8WaveKeys;    // 256 keys per workgroup per step
static_assert(kDecSplitKeys % kF8BlockKeys == 0, "a split is whole steps of the fp8 key loop");

// quad exchanges on integers (the amax of a row) and the sum over a quad: lane i ^ 2, then lane i ^ 1
__device__ __forceinline__ uint32_t f8_quad_umax(uint32_t a) {
  uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
  a = a > o ? a : o;
  o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
  return a > o ? a : o;
}
__device__ __forceinline__ float f8_quad_sum(float s) {
  s += dec_dpp<0x4E, 0xF>(0.f, s);
  s += dec_dpp<0xB1, 0xF>(0.f, s);
  return s;
}

// 16 e4m3 codes -> their 16 values in fp32 (exact): v_cvt_pk_f32_fp8, two codes per instruction
__device__ __forceinline__ void f8_unpack16(const uint4& r, float* f) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0], f[4 * i + 1] = lo[1], f[4 * i + 2] = hi[0], f[4 * i + 3] = hi[1];
  }
}

// The quantiser of one row, called by all 4 lanes of its quad: (lo, hi) are this lane's 16 bf16 dims. Returns the
// lane's 16 codes and the row's scale d (the same in the 4 lanes). amax is taken on the magnitude BITS with an
// integer maximum: a NaN (above the infinity pattern) wins it as it wins torch's amax, so a row that holds one
// gets d = 1 like a row that holds an infinity. E - 7 of a subnormal amax (exponent field 0) is below the clamp.
__device__ __forceinline__ void f8_quantize_row(const uint4& lo, const uint4& hi, uint4& codes, float& d) {
  float x[kF8Dims];
  dec_unpack(lo, x);
  dec_unpack(hi, x + 8);
  uint32_t a = 0;
#pragma unroll
  for (int i = 0; i < kF8Dims; ++i) {
    const uint32_t u = __float_as_uint(x[i]) & 0x7fffffffu;
    a = a > u ? a : u;
  }
  a = f8_quad_umax(a);
  int e = (int)(a >> 23) - 127 - 7;
  e = e < -126 ? -126 : e;
  e = (a != 0 && a < 0x7f800000u) ? e : 0;
  d = __uint_as_float((uint32_t)(e + 127) << 23);
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e: e in [-126, 120]
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    c[i] = pack4_fp8<0>(x[4 * i] * inv, x[4 * i + 1] * inv, x[4 * i + 2] * inv, x[4 * i + 3] * inv);
  codes = dec_u4(c[0], c[1], c[2], c[3]);
}

// q . code over the 64 dims of a quad: the query still packed (bf16), the key fragment already unpacked; a 16-term
// fma chain from 0 (every bf16 x e4m3 product is exact in fp32), then the two quad levels. The caller multiplies by
// the key's scale.
__device__ __forceinline__ float f8_dot(const uint4& qlo, const uint4& qhi, const float* k) {
  float q[kF8Dims];
  dec_unpack(qlo, q);
  dec_unpack(qhi, q + 8);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kF8Dims; ++i) s = fmaf(q[i], k[i], s);
  return f8_quad_sum(s);
}

// The sum over the 16 lane groups of a wave, every lane of a quad for its own dims: rotations by 4 and by 8 inside
// a row of 16 lanes (DPP row_ror), then xor 16 and 32 through ds_bpermute. A fixed order; four levels where the
// 8-group kernels have three.
__device__ __forceinline__ float f8_groups_sum(float v, int lane) {
  v += dec_dpp<0x124, 0xF>(0.f, v);
  v += dec_dpp<0x128, 0xF>(0.f, v);
  v += dec_xor(v, lane, 16);
  v += dec_xor(v, lane, 32);
  return v;
}
__device__ __forceinline__ float f8_groups_max(float v, int lane) {
  v = fmaxf(v, dec_dpp<0x124, 0xF>(0.f, v));
  v = fmaxf(v, dec_dpp<0x128, 0xF>(0.f, v));
  v = fmaxf(v, dec_xor(v, lane, 16));
  return fmaxf(v, dec_xor(v, lane, 32));
}

}  // namespace mlt
