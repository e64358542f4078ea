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
#include "mlt_attn_decode.h"
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

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

// ---------------------------------------------------------------------------------------------------------
// Grouped-query attention: Hkv < H key/value heads, query head h reads KV head h / G (G = H / Hkv).
//
// Operands: qkv_new [B, ldq >= (H + 2 Hkv) * 64] bf16 in the compact layout q (H heads) | k (Hkv) | v (Hkv);
// kv [2, B, Hkv, Smax, 64]; pos, out and rope as above.
//
// One 256-thread workgroup per (KV head, head chunk, batch): grid (Hkv * chunks, B), chunks = G / GC. A workgroup
// serves the GC query heads hkv * G + chunk * GC .. + GC - 1 from ONE pass over the KV head's rows: the key ->
// (wave, load, lane group) mapping, the 4 + 4 loads in flight and the predication of stale rows are those of
// attn_decode_kernel (they do not depend on GC), and every loaded K fragment is dotted against the GC queries the
// lane holds, every V fragment feeds GC accumulators. The queries stay packed (bf16 pairs, GC x 4 VGPRs) and are
// unpacked at use, which is exact. Every (lane group, head) keeps its own (m, l, O[8]) started at THAT head's
// new-token score, so the arithmetic of one head and its order are attn_decode_kernel's on a cache whose KV heads
// are repeated G times: the output is bitwise that kernel's (tests/test_gqa_gpu.py), and batch invariant like it.
// Merge: the same fixed order per head, the LDS arrays with a GC dimension; the final sum of head i is done by
// lane group i of wave 0 (GC <= 8 groups). The append is done once per (b, KV head): chunk 0 / wave 0 / group 0.
// Why VALU: an MFMA over the group's heads would need V with keys along the contraction (a transposed cache or
// an LDS round trip) and P rounded to bf16, which would break the bitwise property.
// ---------------------------------------------------------------------------------------------------------

// no-packed-fp32-ops: GC heads of independent fp32 work are what the SLP vectoriser packs into v_pk_mul_f32 /
// v_pk_fma_f32 pairs (2,300 of them over the instantiations); the kernel is built without the packed forms, two
// scalar VALU ops each, so that its bits never depend on them.
template <int GC, bool ROPE>
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kDecWaves * 64) void attn_decode_gqa_kernel(const uint16_t* __restrict__ qkv_new,
                                                                         int64_t ldq, uint16_t* __restrict__ kv,
                                                                         const int* __restrict__ pos,
                                                                         uint16_t* __restrict__ out, int H, int Hkv,
                                                                         int chunks, int Smax, float scale,
                                                                         const float* __restrict__ rope) {
  static_assert(GC >= 1 && GC <= 8, "the final sum of head i is lane group i of wave 0");
  __shared__ float s_m[GC][kDecWaves];
  __shared__ float s_l[GC][kDecWaves];
  __shared__ float s_o[GC][kDecWaves][kDecHead];
  const int hkv = blockIdx.x / chunks, ch = blockIdx.x - hkv * chunks, b = blockIdx.y, B = gridDim.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, c = lane & 7;
  const int h0 = (hkv * chunks + ch) * GC;  // the first query head of this workgroup (G = chunks * GC)
  const int D = H * kDecHead;
  int n = pos[b];  // cached keys = the new token's row
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const float sl2 = scale * 1.4426950408889634f;  // exponents in base 2

  const uint16_t* row = qkv_new + (int64_t)b * ldq + c * 8;
  uint4 qr[GC];
#pragma unroll
  for (int i = 0; i < GC; ++i) qr[i] = *reinterpret_cast<const uint4*>(row + (h0 + i) * kDecHead);
  uint4 kn = *reinterpret_cast<const uint4*>(row + D + hkv * kDecHead);
  if constexpr (ROPE) {  // one table row for every head: the position is the token's
    const float4* tp = reinterpret_cast<const float4*>(rope + (int64_t)n * kDecHead + c * 8);
    const float4 t0 = tp[0], t1 = tp[1];
    const float t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int i = 0; i < GC; ++i) qr[i] = dec_rotate(qr[i], t);
    kn = dec_rotate(kn, t);
  }
  const uint4 vn = *reinterpret_cast<const uint4*>(row + D + (Hkv + hkv) * kDecHead);
  uint16_t* kc = kv + ((int64_t)b * Hkv + hkv) * Smax * kDecHead + c * 8;  // this lane's dims of key row 0
  uint16_t* vc = kc + (int64_t)B * Hkv * Smax * kDecHead;
  if (ch == 0 && w == 0 && g == 0) {  // the append, once per (b, KV head)
    *reinterpret_cast<uint4*>(kc + (int64_t)n * kDecHead) = kn;
    *reinterpret_cast<uint4*>(vc + (int64_t)n * kDecHead) = vn;
  }

  // the new token, from registers: head i's scaled score is the first m of every state of head i
  float m[GC], l[GC], o[GC][8];
  {
    float k[8], v[8];
    dec_unpack(kn, k);
    dec_unpack(vn, v);
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const float sn = dec_dot_packed(qr[i], k);
      m[i] = sn * sl2;
      l[i] = 0.f;
#pragma unroll
      for (int d = 0; d < 8; ++d) o[i][d] = 0.f;
      if (w == 0 && g == 0) {
        const float p = dec_exp2(fmaf(sn, sl2, -m[i]));
        l[i] = p;
#pragma unroll
        for (int d = 0; d < 8; ++d) o[i][d] = p * v[d];
      }
    }
  }

  for (int base = w * kDecWaveKeys; base < n; base += kDecBlockKeys) {
    uint4 kr[kDecUnroll], vr[kDecUnroll];
    bool ok[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // all loads first: 8 x 16 bytes in flight per lane, whatever GC
      const int j = base + u * 8 + g;
      ok[u] = j < n;
      kr[u] = ok[u] ? *reinterpret_cast<const uint4*>(kc + (int64_t)j * kDecHead) : dec_u4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int j = base + u * 8 + g;
      vr[u] = ok[u] ? *reinterpret_cast<const uint4*>(vc + (int64_t)j * kDecHead) : dec_u4(0, 0, 0, 0);
    }
    float s[GC][kDecUnroll], mx[GC];
#pragma unroll
    for (int i = 0; i < GC; ++i) mx[i] = m[i];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // one unpack of a K fragment, GC dot products
      float k[8];
      dec_unpack(kr[u], k);
#pragma unroll
      for (int i = 0; i < GC; ++i) {
        s[i][u] = dec_dot_packed(qr[i], k);
        mx[i] = fmaxf(mx[i], ok[u] ? s[i][u] * sl2 : -INFINITY);
      }
    }
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const float alpha = dec_exp2(m[i] - mx[i]);  // m is finite from the start
      m[i] = mx[i];
      l[i] *= alpha;
#pragma unroll
      for (int d = 0; d < 8; ++d) o[i][d] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // one unpack of a V fragment, GC accumulators
      float v[8];
      dec_unpack(vr[u], v);
#pragma unroll
      for (int i = 0; i < GC; ++i) {
        const float p = ok[u] ? dec_exp2(fmaf(s[i][u], sl2, -m[i])) : 0.f;
        l[i] += p;
#pragma unroll
        for (int d = 0; d < 8; ++d) o[i][d] = fmaf(p, v[d], o[i][d]);
      }
    }
  }

  // merge, per head in attn_decode_kernel's fixed order
#pragma unroll
  for (int i = 0; i < GC; ++i) {
    float mw = m[i];  // uniform inside a lane group: the maximum over the 8 groups (exact in any order)
    mw = fmaxf(mw, dec_xor_row8(mw));
    mw = fmaxf(mw, dec_xor(mw, lane, 16));
    mw = fmaxf(mw, dec_xor(mw, lane, 32));
    if (lane == 0) s_m[i][w] = mw;
  }
  dec_barrier();
#pragma unroll
  for (int i = 0; i < GC; ++i) {
    float M = s_m[i][0];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) M = fmaxf(M, s_m[i][x]);
    const float a = dec_exp2(m[i] - M);
    l[i] *= a;
#pragma unroll
    for (int d = 0; d < 8; ++d) o[i][d] *= a;
    l[i] = dec_groups_sum(l[i], lane);  // the 8 groups of the wave: xor 8, 16, 32
#pragma unroll
    for (int d = 0; d < 8; ++d) o[i][d] = dec_groups_sum(o[i][d], lane);
    if (g == 0) {
#pragma unroll
      for (int d = 0; d < 8; ++d) s_o[i][w][c * 8 + d] = o[i][d];
      if (c == 0) s_l[i][w] = l[i];
    }
  }
  dec_barrier();
  if (w == 0 && g < GC) {  // lane group g sums head h0 + g over the waves, in wave order
    float L = s_l[g][0];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) L += s_l[g][x];
    const float inv = 1.0f / L;  // L >= the new token's p > 0
    uint32_t pk[4];
#pragma unroll
    for (int d = 0; d < 8; d += 2) {
      float t0 = s_o[g][0][c * 8 + d], t1 = s_o[g][0][c * 8 + d + 1];
#pragma unroll
      for (int x = 1; x < kDecWaves; ++x) {
        t0 += s_o[g][x][c * 8 + d];
        t1 += s_o[g][x][c * 8 + d + 1];
      }
      pk[d >> 1] = (uint32_t)f32_to_bf16(t0 * inv) | ((uint32_t)f32_to_bf16(t1 * inv) << 16);
    }
    *reinterpret_cast<uint4*>(out + (int64_t)b * D + (h0 + g) * kDecHead + c * 8) =
        dec_u4(pk[0], pk[1], pk[2], pk[3]);
  }
}

// The query heads one workgroup serves: the largest of 4, 3, 2 that divides G and still leaves the grid one
// workgroup per CU (256), else 1. Measured (profiles/gqa/README.md): a workgroup's time grows with GC (its VALU
// work per loaded key does), so a larger GC pays only while the machine stays full; 6 and 8 lost to 2 x 3 and
// 2 x 4 at every batch and pos and are reached through an explicit gc only. The choice cannot change a bit of the
// output (the arithmetic of a head does not depend on GC), so it may depend on the batch.
constexpr int kDecFillWorkgroups = 256;
int attn_decode_gqa_chunk(int G, int Hkv, int B) {
  for (int gc : {4, 3, 2})
    if (G % gc == 0 && (long long)Hkv * (G / gc) * B >= kDecFillWorkgroups) return gc;
  return 1;
}

void launch_attn_decode_gqa(const uint16_t* qkv_new, int64_t ldq, uint16_t* kv, const int* pos, uint16_t* out, int B,
                            int H, int Hkv, int Smax, float scale, hipStream_t st, const float* rope, int gc) {
  const int G = H / Hkv;
  if (gc <= 0) gc = attn_decode_gqa_chunk(G, Hkv, B);
  if (G * Hkv != H || G % gc != 0) throw_no_kernel("launch_attn_decode_gqa", "heads per KV head", G);
  const int chunks = G / gc;
  const dim3 grid(Hkv * chunks, B), block(kDecWaves * 64);
  const bool hit = dispatch_int<1, 2, 3, 4, 6, 8>(gc, [&](auto c) {
    constexpr int GC = decltype(c)::value;
    if (rope)
      attn_decode_gqa_kernel<GC, true><<<grid, block, 0, st>>>(qkv_new, ldq, kv, pos, out, H, Hkv, chunks, Smax, scale,
                                                               rope);
    else
      attn_decode_gqa_kernel<GC, false><<<grid, block, 0, st>>>(qkv_new, ldq, kv, pos, out, H, Hkv, chunks, Smax,
                                                                scale, nullptr);
  });
  if (!hit) throw_no_kernel("launch_attn_decode_gqa", "GC", gc);
}

}  // namespace mlt
