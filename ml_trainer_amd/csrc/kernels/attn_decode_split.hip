// Decode attention over a LONG key/value cache for gfx950: the keys of one (batch, KV head) split over
// workgroups, and a second launch that merges their partial softmax states.
//
// attn_decode.hip gives one workgroup per (head, batch) the whole cache of its head: at batch 1 that is H
// workgroups on 256 CUs, and each pulls its whole K and V stream through one CU. Here the grid grows with the
// cache instead, so a long cache is fetched by the whole machine.
//
// Operands: those of attn_decode_gqa_kernel (qkv_new compact q (H) | k (Hkv) | v (Hkv), kv [2, B, Hkv, Smax, 64],
// pos int32 [B] on the device, out [B, H * 64], rope or nullptr) plus the workspace ws. Multi-head attention is
// Hkv = H, G = 1, GC = 1: the compact row is then the [B, 3 * H * 64] row, so one kernel serves both.
//
// attn_decode_split_kernel<GC, ROPE>, grid (Hkv * G / GC, Z, B) with Z = ceil(Smax / C), C = kDecSplitKeys:
//   * split z of a (batch, KV head, head chunk) owns the cached keys [z C, min((z + 1) C, n)), n = clamp(pos[b]).
//     C is a compile-time constant, so WHICH keys meet in which partial sum depends on the key index alone, not on
//     B, H, Smax or pos; and C is a multiple of 128, so key j keeps the (wave, load, lane group) it has in the
//     unsplit kernels: wave (j % 128) / 32, load (j % 32) / 8, lane group j % 8.
//   * split 0 always runs. It holds the new token (wave 0 / group 0 seeds its state from the registers that hold
//     qkv_new) and does the append, once per (b, KV head), from head chunk 0.
//   * a split z > 0 with z C >= n has no key: the workgroup returns before any other load and before any barrier
//     (the condition is uniform over the workgroup). Its workspace slot keeps whatever an earlier step left there.
//   * inside a workgroup everything is attn_decode_gqa_kernel: 4 + 4 sixteen-byte loads in flight per lane straight
//     to VGPRs, stale rows predicated off and selected out, one (m, l, O[8]) state per (lane group, head) in base
//     2 started at that head's new-token score (every workgroup recomputes it from qkv_new, rotated under ROPE, so
//     no state ever holds m = -inf), the 32 states merged in the same fixed order.
//   * instead of O / L the workgroup writes the merged state (M, L, O[64]) of each of its heads in fp32 to the
//     workspace slot (b, h, z).
// Workspace: ws fp32 [B, H, Z, kDecSlotFloats = 68]; a slot is M, L, two unused words, O[64]: 272 bytes, so every
// slot and its O row are 16-byte aligned and are written with 16-byte stores.
//
// attn_decode_merge_kernel, the second launch: the kernel boundary carries the dependency (no counter, flag or
// atomic). One wave per (b, h), lane d owns dim d, 4 (b, h) per workgroup. Za = max(1, ceil(n / C)) active splits
// from pos on the device; slots z >= Za are never read. M* = max_z M_z, a_z = exp2(M_z - M*) (v_exp_f32),
//   L = a_0 L_0, O_d = a_0 O_0d, then for z = 1 .. Za - 1 in ascending order L = fma(a_z, L_z, L),
//   O_d = fma(a_z, O_zd, O_d)   (dec_merge_first / dec_merge_add in mlt_attn_decode.h);  out = bf16(O_d * (1 / L)).
// The slots are loaded kDecMergeBatch at a time, all loads of a batch before their first use.
//
// What follows bit for bit (tests/test_attn_decode_split_gpu.py):
//   * while pos[b] <= C there is one active split, a_0 = exp2(0) = 1 exactly, and the row of out has the bits of
//     attn_decode_kernel / attn_decode_gqa_kernel on the same inputs;
//   * GC changes no bit (the arithmetic of a head does not depend on it), so the launcher picks it from the grid;
//   * a row depends on its own qkv_new, cache rows and pos[b] only: not on B, not on Smax.
// pos[b] < Smax: debug builds check it (MLT_DCHECK), every build clamps it into the cache.
#include "mlt_attn_decode.h"
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

constexpr int kDecMergeBatch = 8;  // slots whose loads are in flight together in the merge kernel

__device__ __forceinline__ float4 dec_f4(float x, float y, float z, float w) {  // make_float4 without a call
  float4 r;
  r.x = x, r.y = y, r.z = z, r.w = w;
  return r;
}

// no-packed-fp32-ops: as attn_decode_gqa_kernel, whose bits this kernel must reproduce.
template <int GC, bool ROPE>
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kDecWaves * 64) void attn_decode_split_kernel(const uint16_t* __restrict__ qkv_new,
                                                                           int64_t ldq, uint16_t* __restrict__ kv,
                                                                           const int* __restrict__ pos,
                                                                           float* __restrict__ ws, int H, int Hkv,
                                                                           int chunks, int Smax, float scale,
                                                                           const float* __restrict__ rope) {
  static_assert(GC >= 1 && GC <= 8, "the final sum of head i is lane group i of wave 0");
  __shared__ float s_m[GC][kDecWaves];
  __shared__ float s_l[GC][kDecWaves];
  __shared__ float s_o[GC][kDecWaves][kDecHead];
  const int z = blockIdx.y, Z = gridDim.y, b = blockIdx.z, B = gridDim.z;
  int n = pos[b];  // cached keys = the new token's row
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const int first = z * kDecSplitKeys;
  if (z > 0 && first >= n) return;  // no key of this split is cached: uniform, before any load or barrier
  const int end = min(first + kDecSplitKeys, n);  // this split's keys: [first, end)

  const int hkv = blockIdx.x / chunks, ch = blockIdx.x - hkv * chunks;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, c = lane & 7;
  const int h0 = (hkv * chunks + ch) * GC;  // the first query head of this workgroup (G = chunks * GC)
  const int D = H * kDecHead;
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
  const bool seed = z == 0 && w == 0 && g == 0;  // the one state that starts with the new token
  if (ch == 0 && seed) {                         // the append, once per (b, KV head)
    *reinterpret_cast<uint4*>(kc + (int64_t)n * kDecHead) = kn;
    *reinterpret_cast<uint4*>(vc + (int64_t)n * kDecHead) = vn;
  }

  // head i's scaled new-token score is the first m of every state of head i, in every split
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
      if (seed) {
        const float p = dec_exp2(fmaf(sn, sl2, -m[i]));
        l[i] = p;
#pragma unroll
        for (int d = 0; d < 8; ++d) o[i][d] = p * v[d];
      }
    }
  }

  for (int base = first + w * kDecWaveKeys; base < end; base += kDecBlockKeys) {
    uint4 kr[kDecUnroll], vr[kDecUnroll];
    bool ok[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // all loads first: 8 x 16 bytes in flight per lane, whatever GC
      const int j = base + u * 8 + g;
      ok[u] = j < end;  // end <= n: rows >= n are stale; rows >= (z + 1) C are the next split's
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

  // merge of the 32 states, per head in attn_decode_kernel's fixed order
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
  if (w == 0 && g < GC) {  // lane group g sums head h0 + g over the waves, in wave order, and writes its slot
    float M = s_m[g][0], L = s_l[g][0];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) {
      M = fmaxf(M, s_m[g][x]);
      L += s_l[g][x];
    }
    float t[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      t[d] = s_o[g][0][c * 8 + d];
#pragma unroll
      for (int x = 1; x < kDecWaves; ++x) t[d] += s_o[g][x][c * 8 + d];
    }
    float* slot = ws + (((int64_t)b * H + h0 + g) * Z + z) * kDecSlotFloats;
    if (c == 0) *reinterpret_cast<float4*>(slot) = dec_f4(M, L, 0.f, 0.f);
    float4* od = reinterpret_cast<float4*>(slot + 4 + c * 8);
    od[0] = dec_f4(t[0], t[1], t[2], t[3]);
    od[1] = dec_f4(t[4], t[5], t[6], t[7]);
  }
}

// One wave per (b, h) = bh, lane d = dim d. No barrier, no LDS: waves past the last (b, h) just leave.
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kDecWaves * 64) void attn_decode_merge_kernel(const float* __restrict__ ws,
                                                                           const int* __restrict__ pos,
                                                                           uint16_t* __restrict__ out, int BH, int H,
                                                                           int Z, int Smax) {
  const int lane = threadIdx.x & 63, bh = blockIdx.x * kDecWaves + (threadIdx.x >> 6);
  if (bh >= BH) return;
  int n = pos[bh / H];
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const int Za = max(1, (n + kDecSplitKeys - 1) / kDecSplitKeys);  // <= Z; slots z >= Za hold stale states
  const float* slots = ws + (int64_t)bh * Z * kDecSlotFloats;

  float M = -INFINITY;  // M* = max over the active splits (exact in any order): lane-strided, then the wave
  for (int z = lane; z < Za; z += 64) M = fmaxf(M, slots[(int64_t)z * kDecSlotFloats]);
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) M = fmaxf(M, dec_xor(M, lane, x));

  const float a0 = dec_exp2(slots[0] - M);
  float L = dec_merge_first(a0, slots[1]);
  float O = dec_merge_first(a0, slots[4 + lane]);
  for (int z0 = 1; z0 < Za; z0 += kDecMergeBatch) {
    float mz[kDecMergeBatch], lz[kDecMergeBatch], oz[kDecMergeBatch];
#pragma unroll
    for (int u = 0; u < kDecMergeBatch; ++u) {  // the loads of the batch, all before the first use
      const bool ok = z0 + u < Za;
      const float* s = slots + (int64_t)(z0 + u) * kDecSlotFloats;
      mz[u] = ok ? s[0] : 0.f;
      lz[u] = ok ? s[1] : 0.f;
      oz[u] = ok ? s[4 + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kDecMergeBatch; ++u) {
      if (z0 + u < Za) {  // uniform over the wave; ascending z
        const float a = dec_exp2(mz[u] - M);
        L = dec_merge_add(a, lz[u], L);
        O = dec_merge_add(a, oz[u], O);
      }
    }
  }
  const float inv = 1.0f / L;  // L >= a_z L_z > 0 of the split that holds M*
  out[(int64_t)bh * kDecHead + lane] = f32_to_bf16(O * inv);
}

int attn_decode_split_keys() { return kDecSplitKeys; }

void launch_attn_decode_split(const uint16_t* qkv_new, int64_t ldq, uint16_t* kv, const int* pos, uint16_t* out,
                              float* ws, int B, int H, int Hkv, int Smax, float scale, hipStream_t st,
                              const float* rope, int gc) {
  const int G = H / Hkv, Z = (Smax + kDecSplitKeys - 1) / kDecSplitKeys;
  // the unsplit launcher's rule with B * Z workgroups per (KV head, chunk) in place of B: no bit depends on it
  if (gc <= 0) gc = attn_decode_gqa_chunk(G, Hkv, (int)std::min<long long>((long long)B * Z, 1 << 30));
  if (G * Hkv != H || G % gc != 0) throw_no_kernel("launch_attn_decode_split", "heads per KV head", G);
  if (Z > 65535 || B > 65535) throw_no_kernel("launch_attn_decode_split", "splits", Z);
  const int chunks = G / gc;
  const dim3 grid(Hkv * chunks, Z, B), block(kDecWaves * 64);
  // every GC of attn_decode_gqa_kernel is built: none spills (docs/ARCHITECTURE.md has the register table)
  const bool hit = dispatch_int<1, 2, 3, 4, 6, 8>(gc, [&](auto c) {
    constexpr int GC = decltype(c)::value;
    dispatch_bools(
        [&](auto r) {
          attn_decode_split_kernel<GC, decltype(r)::value><<<grid, block, 0, st>>>(qkv_new, ldq, kv, pos, ws, H, Hkv,
                                                                                    chunks, Smax, scale, rope);
        },
        rope != nullptr);
  });
  if (!hit) throw_no_kernel("launch_attn_decode_split", "GC", gc);
  launch_attn_decode_merge(ws, pos, out, B, H, Smax, st);
}

void launch_attn_decode_merge(const float* ws, const int* pos, uint16_t* out, int B, int H, int Smax, hipStream_t st) {
  const int BH = B * H, Z = (Smax + kDecSplitKeys - 1) / kDecSplitKeys;
  attn_decode_merge_kernel<<<dim3((BH + kDecWaves - 1) / kDecWaves), dim3(kDecWaves * 64), 0, st>>>(ws, pos, out, BH,
                                                                                                  H, Z, Smax);
}

}  // namespace mlt
