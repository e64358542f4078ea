// Single-token ("decode") attention over a key/value cache for gfx950, with the append fused in.
//
// Operands: qkv_new [B, 3 * H * 64] bf16 (the QKV projection of the B new tokens, q | k | v per row, row stride
// ldq elements); kv [2, B, H, Smax, 64] bf16 (kv[0] keys, kv[1] values, head-major: the key stream of one
// (b, h) is contiguous); pos [B] int32 on the device (the row the new token takes = the number of tokens
// already cached); out [B, H * 64] bf16.
//
// One 256-thread workgroup per (head, batch). Per (b, h):
//   * rows pos[b] of kv[0] and kv[1] become the new token's k / v (8 lanes x 16 bytes each, vector stores);
//   * out = sum_{j <= pos[b]} softmax_j(scale q.k_j) v_j. Keys j < pos[b] stream from the cache; key pos[b] is
//     the new token and is taken from the registers that hold qkv_new, never read back from the cache.
// The problem is memory bound (two bytes of cache per multiply-add), so K and V go straight from global
// memory to VGPRs: no LDS staging, no MFMA. A cache row is 128 bytes = 8 lanes x 16 bytes: lane group
// g = lane >> 3 owns a key, lane c = lane & 7 owns dims 8c .. 8c + 7 of it. One wave instruction loads 8 rows
// (1 KiB contiguous); kDecUnroll = 4 of them for K and 4 for V are issued before the first use (8 x 16 bytes in
// flight per lane), so a wave takes 32 keys and the workgroup 128 keys per step:
//   key j -> wave (j % 128) / 32, load (j % 32) / 8, lane group j % 8.
// q.k is an 8-term fp32 fma chain per lane plus a 3-step xor butterfly inside the group. Every lane group
// keeps its OWN online-softmax state (m, l, O[8 dims per lane]) in base 2 (sl2 = scale * log2 e,
// p = exp2(fma(s, sl2, -m)) as in attention.hip), so the key loop has no exchange beyond that butterfly. P
// stays fp32: it never re-enters an MFMA, so it is never rounded to bf16.
// Every state starts at m = the new token's scaled score (finite), with l = 0 and O = 0 except the state of
// wave 0 / group 0, which starts with the new token itself: no state ever holds m = -inf, so no exp2(-inf + inf).
// Rows j > pos[b] are stale memory. Their lanes do not load (the load is predicated on j < pos[b]), their
// score is selected to -inf and their p to 0: nothing of them enters the arithmetic, NaNs included.
// Merge of the 32 states of one (b, h), in a fixed order (no atomics; bitwise reproducible): the maximum M of
// the m's (wave butterfly, then the 4 waves through LDS in wave order), each state scaled by exp2(m - M), an
// xor butterfly over the 8 groups of a wave, then the 4 waves summed through LDS in wave order; out = O / l.
// pos is read from the device and the launch needs nothing from the host: a decode step is capturable.
// pos[b] < Smax cannot be checked without a read: debug builds check it (MLT_DCHECK); every build clamps it
// into the cache, so that a bad value cannot write outside the allocation.
// With a rotary table (the ROPE instantiation) q and the new k are rotated by pos[b] first; see dec_rotate.
#include "mlt_common.h"
#include "mlt_kernels.h"

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

// ROPE: q and the new k are rotated by position pos[b] (rope [>= Smax][32][2] fp32, the table of ops/rope.py) in
// registers and rounded to bf16 BEFORE the dot product and the append; the cache holds rotated keys.
template <bool ROPE>
__global__ __launch_bounds__(kDecWaves * 64) void attn_decode_kernel(const uint16_t* __restrict__ qkv_new,
                                                                     int64_t ldq, uint16_t* __restrict__ kv,
                                                                     const int* __restrict__ pos,
                                                                     uint16_t* __restrict__ out, int H, int Smax,
                                                                     float scale, const float* __restrict__ rope) {
  __shared__ float s_m[kDecWaves];
  __shared__ float s_l[kDecWaves];
  __shared__ float s_o[kDecWaves][kDecHead];
  const int h = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, c = lane & 7;
  const int D = H * kDecHead;
  int n = pos[b];  // cached keys = the new token's row
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const float sl2 = scale * 1.4426950408889634f;  // exponents in base 2

  const uint16_t* row = qkv_new + (int64_t)b * ldq + h * kDecHead + c * 8;
  uint4 qr = *reinterpret_cast<const uint4*>(row);
  uint4 kn = *reinterpret_cast<const uint4*>(row + D);
  if constexpr (ROPE) {  // this lane's dims 8c .. 8c + 7 are four whole pairs: 32 contiguous bytes of the table
    const float4* tp = reinterpret_cast<const float4*>(rope + (int64_t)n * kDecHead + c * 8);
    const float4 t0 = tp[0], t1 = tp[1];
    const float t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    qr = dec_rotate(qr, t);
    kn = dec_rotate(kn, t);
  }
  const uint4 vn = *reinterpret_cast<const uint4*>(row + 2 * D);
  uint16_t* kc = kv + ((int64_t)b * H + h) * Smax * kDecHead + c * 8;  // this lane's dims of key row 0
  uint16_t* vc = kc + (int64_t)B * H * Smax * kDecHead;
  if (w == 0 && g == 0) {  // the append: 8 lanes x 16 bytes per row
    *reinterpret_cast<uint4*>(kc + (int64_t)n * kDecHead) = kn;
    *reinterpret_cast<uint4*>(vc + (int64_t)n * kDecHead) = vn;
  }

  float q[8];
  dec_unpack(qr, q);
  // the new token, from registers: its scaled score is every state's first m
  const float sn = dec_dot(q, kn);
  float m = sn * sl2, l = 0.f, o[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] = 0.f;
  if (w == 0 && g == 0) {
    float v[8];
    dec_unpack(vn, v);
    const float p = dec_exp2(fmaf(sn, sl2, -m));
    l = p;
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] = p * v[d];
  }

  for (int base = w * kDecWaveKeys; base < n; base += kDecBlockKeys) {
    uint4 kr[kDecUnroll], vr[kDecUnroll];
    bool ok[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // all loads first: 8 x 16 bytes in flight per lane
      const int j = base + u * 8 + g;
      ok[u] = j < n;  // rows >= n are stale (row n itself was just written: the new token comes from registers)
      kr[u] = ok[u] ? *reinterpret_cast<const uint4*>(kc + (int64_t)j * kDecHead) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int j = base + u * 8 + g;
      vr[u] = ok[u] ? *reinterpret_cast<const uint4*>(vc + (int64_t)j * kDecHead) : make_uint4(0, 0, 0, 0);
    }
    float s[kDecUnroll], mx = m;
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      s[u] = dec_dot(q, kr[u]);
      mx = fmaxf(mx, ok[u] ? s[u] * sl2 : -INFINITY);
    }
    const float alpha = dec_exp2(m - mx);  // m is finite from the start
    m = mx;
    l *= alpha;
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] *= alpha;
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const float p = ok[u] ? dec_exp2(fmaf(s[u], sl2, -m)) : 0.f;
      float v[8];
      dec_unpack(vr[u], v);
      l += p;
#pragma unroll
      for (int d = 0; d < 8; ++d) o[d] = fmaf(p, v[d], o[d]);
    }
  }

  // merge, fixed order. M over the wave's 8 groups, then over the waves.
  const float mw = wave_max(m);
  if (lane == 0) s_m[w] = mw;
  __syncthreads();
  float M = s_m[0];
#pragma unroll
  for (int i = 1; i < kDecWaves; ++i) M = fmaxf(M, s_m[i]);
  const float a = dec_exp2(m - M);
  l *= a;
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] *= a;
#pragma unroll
  for (int x = 8; x < 64; x <<= 1) {  // the 8 groups of the wave: xor 8, 16, 32
    l += __shfl_xor(l, x, 64);
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] += __shfl_xor(o[d], x, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) s_o[w][c * 8 + d] = o[d];
    if (c == 0) s_l[w] = l;
  }
  __syncthreads();
  if (w == 0 && g == 0) {
    float L = s_l[0];
#pragma unroll
    for (int i = 1; i < kDecWaves; ++i) L += s_l[i];
    const float inv = 1.0f / L;  // L >= the new token's p > 0
    uint32_t pk[4];
#pragma unroll
    for (int d = 0; d < 8; d += 2) {
      float t0 = s_o[0][c * 8 + d], t1 = s_o[0][c * 8 + d + 1];
#pragma unroll
      for (int i = 1; i < kDecWaves; ++i) {
        t0 += s_o[i][c * 8 + d];
        t1 += s_o[i][c * 8 + d + 1];
      }
      pk[d >> 1] = (uint32_t)f32_to_bf16(t0 * inv) | ((uint32_t)f32_to_bf16(t1 * inv) << 16);
    }
    *reinterpret_cast<uint4*>(out + (int64_t)b * D + h * kDecHead + c * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  }
}

void launch_attn_decode(const uint16_t* qkv_new, int64_t ldq, uint16_t* kv, const int* pos, uint16_t* out, int B,
                        int H, int Smax, float scale, hipStream_t st, const float* rope) {
  const dim3 grid(H, B), block(kDecWaves * 64);
  if (rope)
    attn_decode_kernel<true><<<grid, block, 0, st>>>(qkv_new, ldq, kv, pos, out, H, Smax, scale, rope);
  else
    attn_decode_kernel<false><<<grid, block, 0, st>>>(qkv_new, ldq, kv, pos, out, H, Smax, scale, nullptr);
}

}  // namespace mlt
