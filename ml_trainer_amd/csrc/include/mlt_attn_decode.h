// Device helpers shared by the decode attention kernels (attn_decode.hip: one workgroup per head over the whole
// cache; attn_decode_split.hip: the keys of a long cache split over workgroups, and the merge of their partial
// states). Everything the bitwise equalities between those kernels rest on is written once, here.
#pragma once
#include "mlt_common.h"

namespace mlt {

constexpr int kDecHead = 64;                             // head dim
constexpr int kDecWaves = 4;                             // waves per workgroup
constexpr int kDecUnroll = 4;                            // K (and V) loads in flight per lane
constexpr int kDecWaveKeys = 8 * kDecUnroll;             // keys per wave per step (8 lane groups)
constexpr int kDecBlockKeys = kDecWaves * kDecWaveKeys;  // keys per workgroup per step

__device__ __forceinline__ float dec_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // raw v_exp_f32

__device__ __forceinline__ void dec_unpack(const uint4& r, float* f) {  // 8 bf16 -> 8 fp32 (exact)
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

// q . k over the 64 dims of a lane group: an 8-term fma chain, then xor 1, 2, 4 (the sum in all 8 lanes)
__device__ __forceinline__ float dec_dot(const float* q, const uint4& kr) {
  float k[8];
  dec_unpack(kr, k);
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 8; ++d) s = fmaf(q[d], k[d], s);
  return group_sum<8>(s);
}

// the 8 bf16 of r (four interleaved pairs) rotated by the four (c, s) table entries at t, rounded back to bf16:
// the arithmetic of rope.hip (uncontracted fp32 products, then one fp32 sum), so that a cached key and a
// query carry the bits the training path stores in its rotated QKV buffer
__device__ __forceinline__ uint4 dec_rotate(const uint4& r, const float* t) {
#pragma clang fp contract(off)  // plain operators, no fma: see rope_rotate8 in rope.hip
  float f[8];
  dec_unpack(r, f);
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = f[2 * i], b = f[2 * i + 1], c = t[2 * i], s = t[2 * i + 1];
    const float ac = a * c, bs = b * s, as = a * s, bc = b * c;
    const float ya = ac - bs;
    const float yb = as + bc;
    o[i] = (uint32_t)f32_to_bf16(ya) | ((uint32_t)f32_to_bf16(yb) << 16);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// group_sum<8> (xor 4, 2, 1 over the 8 lanes of a group) on DPP operand modifiers instead of three dependent
// ds_bpermute round trips (about 100 cycles each, GC x 4 x 3 of them per step of the key loop: with GC heads per
// workgroup they, not the loads, set the kernel's time). Lane i adds the value of lane i ^ 4 (row_shl:4 into
// lanes 0-3, row_shr:4 into lanes 4-7 of every 8, selected by the bank mask), then i ^ 2 and i ^ 1 (quad_perm):
// the same operand pairs in the same three levels, and an fp32 add commutes, so the sum has group_sum<8>'s bits
// in all 8 lanes.
template <int CTRL, int BANKS>
__device__ __forceinline__ float dec_dpp(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xF, BANKS, false));
}
__device__ __forceinline__ float dec_group_sum8(float s) {
  s += dec_dpp<0x114, 0xA>(dec_dpp<0x104, 0x5>(0.f, s), s);  // lane i ^ 4
  s += dec_dpp<0x4E, 0xF>(0.f, s);                            // quad_perm [2,3,0,1]: lane i ^ 2
  s += dec_dpp<0xB1, 0xF>(0.f, s);                            // quad_perm [1,0,3,2]: lane i ^ 1
  return s;
}

// attn_decode_gqa_kernel carries target features of its own (below), and a device function that is not
// always_inline is then not inlined into it but CALLED (s_swappc_b64): the HIP header's make_uint4, __syncthreads
// and __shfl_xor (33 calls per head in the merge alone). So these three are written here on the builtins; the
// generated code of every instantiation holds no call.
__device__ __forceinline__ uint4 dec_u4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  uint4 r;
  r.x = x, r.y = y, r.z = z, r.w = w;
  return r;
}
__device__ __forceinline__ void dec_barrier() {  // __syncthreads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// The exchanges of the merge over the 8 lane groups of a wave. xor 8 is a rotation by 8 inside a row of 16
// lanes (DPP row_ror:8); xor 16 and 32 cross rows and go through ds_bpermute. Same operand pairs as the xor
// butterfly of attn_decode_kernel, hence the same bits.
__device__ __forceinline__ float dec_xor_row8(float v) { return dec_dpp<0x128, 0xF>(0.f, v); }
__device__ __forceinline__ float dec_xor(float v, int lane, int mask) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, __float_as_int(v)));
}
__device__ __forceinline__ float dec_groups_sum(float v, int lane) {  // v + xor 8, then 16, then 32
  v += dec_xor_row8(v);
  v += dec_xor(v, lane, 16);
  v += dec_xor(v, lane, 32);
  return v;
}

// the dot product of dec_dot with the query still packed and the key already unpacked: the same 8-term fma chain
// from 0 over this lane's dims, the same three-level sum over the group
__device__ __forceinline__ float dec_dot_packed(const uint4& qr, const float* k) {
  float q[8];
  dec_unpack(qr, q);
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 8; ++d) s = fmaf(q[d], k[d], s);
  return dec_group_sum8(s);
}

// ---- the split form (attn_decode_split.hip) ----
// Keys per split. A compile-time constant and a multiple of kDecBlockKeys: which keys meet in which partial sum is
// a function of the key index alone, and the key -> (wave, load, lane group) mapping inside a split is the unsplit
// kernels' (j - z C and j agree modulo 128). 256 / 512 / 1024 were measured (profiles/decode_split/README.md).
// MLT_DEC_SPLIT_KEYS: a build of another candidate for benchmarks/attn_decode_split_bench.py, never set in tree.
#ifndef MLT_DEC_SPLIT_KEYS
#define MLT_DEC_SPLIT_KEYS 256
#endif
constexpr int kDecSplitKeys = MLT_DEC_SPLIT_KEYS;
static_assert(kDecSplitKeys % kDecBlockKeys == 0, "a split is whole steps of the key loop");
// One workspace slot: M, L, two pad words, O[64], all fp32: 272 bytes, so every slot and its O are 16-byte aligned.
constexpr int kDecSlotFloats = 4 + kDecHead;

// The merge of the splits' states, the expressions of attn_decode_merge_kernel. Split 0 starts the sums, the others
// are added in ascending z with one fma each; a = exp2(M_z - M*) through v_exp_f32. With one active split a = 1
// exactly and both return x unchanged: the row then has the unsplit kernels' bits.
__device__ __forceinline__ float dec_merge_first(float a, float x) { return a * x; }
__device__ __forceinline__ float dec_merge_add(float a, float x, float acc) { return fmaf(a, x, acc); }

}  // namespace mlt
