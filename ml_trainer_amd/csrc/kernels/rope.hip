// Rotary position embedding of the q and k columns of a QKV buffer, in place, for gfx950.
//
// Operands: qkv [rows][ld >= 3 * 64 H] bf16 (q | k | v per row, row stride ld elements, ld % 8 == 0, 16-byte
// aligned); table [P][32][2] fp32 (ops/rope.py: (cos, sin) of position p, pair i, each computed in float64
// and rounded once); pos int32 [rows] on the device, or nullptr: the position of a row is row % S.
//
// Within a head's 64 dims pair i is dims (2i, 2i + 1) (interleaved). For a bf16 pair (a, b) widened to fp32,
// the table entry (c, s) of the row's position and ss = sign * s (sign = +1 forward, -1 backward):
//   a' = bf16_rn(a * c - b * ss),   b' = bf16_rn(a * ss + b * c)
// with every product rounded to fp32, then the sum or difference rounded to fp32 (contraction is switched off
// where the rotation is written, see rope_rotate8), so the fp32 torch expression of ops/rope.py is a bitwise
// oracle. The backward of the rotation is the rotation by the negative angle, applied to dq and dk.
//
// One lane owns dims 8c .. 8c + 7 of one head of one row, in q AND in k: four whole pairs, whose table entries
// are 32 contiguous bytes read once and used for both. Per lane: two 16-byte table loads, one 16-byte load and
// one 16-byte store for q and for k. Bytes: 2 x rows x 2D x 2 (the table rows stay in cache). The grid is
// flat over rows x H x 8 lanes (rows = 1 and rows = 65,536 alike); no LDS, no atomics, vector stores only.
// The v columns, the columns past 3D and rows past `rows` are never touched.
// Explicit positions cannot be checked without a read: debug builds check them (MLT_DCHECK), every build
// clamps them into the table.
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

// rotate the 8 bf16 of r (four pairs) by the four (c, s) entries in t0 | t1; sg = +1 or -1
__device__ __forceinline__ uint4 rope_rotate8(const uint4& r, const float4& t0, const float4& t1, float sg) {
  // Plain operators with contraction off: every product and the sum round to fp32 on their own. (__fmul_rn /
  // __fsub_rn do not guarantee that under hipcc: they are inline `x * y` / `x - y` compiled with the default
  // -ffp-contract=fast, and a * c - b * ss written with them still came out as v_pk_mul_f32 + v_pk_fma_f32.)
#pragma clang fp contract(off)
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  const float cs[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = __uint_as_float(w[i] << 16), b = __uint_as_float(w[i] & 0xffff0000u);
    const float c = cs[2 * i], ss = cs[2 * i + 1] * sg;  // exact
    const float ac = a * c, bs = b * ss, as = a * ss, bc = b * c;
    const float ya = ac - bs;
    const float yb = as + bc;
    o[i] = (uint32_t)f32_to_bf16(ya) | ((uint32_t)f32_to_bf16(yb) << 16);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void rope_qk_kernel(uint16_t* __restrict__ qkv, int64_t ld, int64_t rows, int H,
                                                      const float* __restrict__ table, int P, int S,
                                                      const int* __restrict__ posv, float sg) {
  // (row, head, c), c fastest; rows * H * 8 < 2^31 (checked by the caller): 32-bit index arithmetic
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, per_row = (uint32_t)H * 8u;
  const int64_t row = i / per_row;
  if (row >= rows) return;
  const int hc = (int)(i - (uint32_t)row * per_row);  // h * 8 + c: this lane's dims start at hc * 8 inside q (and k)
  int p = posv ? posv[row] : (int)(row % S);
  MLT_DCHECK(p >= 0 && p < P);
  p = min(max(p, 0), P - 1);
  const float4* t = reinterpret_cast<const float4*>(table + (int64_t)p * 64 + (hc & 7) * 8);
  const float4 t0 = t[0], t1 = t[1];
  uint16_t* q = qkv + row * ld + hc * 8;
  uint16_t* k = q + H * 64;
  const uint4 qr = *reinterpret_cast<const uint4*>(q);
  const uint4 kr = *reinterpret_cast<const uint4*>(k);
  *reinterpret_cast<uint4*>(q) = rope_rotate8(qr, t0, t1, sg);
  *reinterpret_cast<uint4*>(k) = rope_rotate8(kr, t0, t1, sg);
}

void launch_rope_qk(uint16_t* qkv, int64_t ld, int64_t rows, int H, const float* table, int P, int S, const int* pos,
                    int sign, hipStream_t st) {
  if (rows <= 0) return;
  const int64_t lanes = rows * H * 8;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  hipLaunchKernelGGL(rope_qk_kernel, grid, block, 0, st, qkv, ld, rows, H, table, P, S, pos, sign < 0 ? -1.f : 1.f);
}

}  // namespace mlt
