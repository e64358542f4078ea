// Decode attention over an fp8 (OCP e4m3) key/value cache with one power-of-two scale per cached row, for gfx950:
// half the bytes of the bf16 cache per cached row, in the one bandwidth-bound kernel of a decode step. The format
// and the quantiser are in mlt_kv_f8.h; their definition is kv_quantize_reference in ops/decode.py.
//
// Operands: qkv_new [B, ldq >= (H + 2 Hkv) * 64] bf16, compact q (H heads) | k (Hkv) | v (Hkv) (Hkv == H: the plain
// q | k | v row); kv8 [2, B, Hkv, Smax, 64] uint8 codes (keys, values; head-major); kv_scale [2, B, Hkv, Smax] fp32;
// pos int32 [B] on the device; out [B, H * 64] bf16; rope (or nullptr) the rotary table [>= Smax][32][2] fp32.
//
// attn_decode_f8_kernel<GC, ROPE, SPLIT>: one 256-thread workgroup per (KV head, chunk of GC query heads, batch),
// and with SPLIT per split of kDecSplitKeys cached keys (grid (Hkv * G / GC, Z, B), Z = ceil(Smax / C)).
//   * A cached row is 64 bytes = 4 lanes x 16 bytes: lane group g = lane >> 2 (16 per wave) owns a key, lane
//     c = lane & 3 its dims 16 c .. 16 c + 15. One wave instruction loads 16 rows (1 KiB contiguous), straight from
//     global memory to VGPRs; 4 K + 4 V loads and the 4 + 4 scale words of their rows are issued before the first
//     use. A wave takes 64 keys, the workgroup 256 keys per step:
//       key j -> wave (j % 256) / 64, load (j % 64) / 16, lane group j % 16.
//   * Codes become fp32 through v_cvt_pk_f32_fp8 (two per instruction). q . k_j is a 16-term fma chain over the code
//     values, two quad_perm DPP additions, and ONE multiply by the row's scale (exact: a power of two); p_j is
//     multiplied by the value row's scale once, before its 16 fmas into O. l sums the unscaled p_j.
//   * One online-softmax state (m, l, O[16]) in base 2 per (lane group, head), started at that head's new-token
//     score: no state ever holds m = -inf. Rows j >= n are stale: their loads (codes and scales) are predicated
//     off, their score is selected to -inf and their p to 0.
//   * The new token: its k (rotated under ROPE) and v are QUANTISED FIRST (f8_quantize_row, redundantly in every
//     quad) and enter the step as the dequantised values, from registers; chunk 0 / split 0 / wave 0 / group 0
//     stores the 4 x 16 code bytes and the scale of each row. A token thus contributes the same k / v to its own
//     step and to every later one, and the function computed is attention over the dequantised rows j <= pos[b].
//   * Merge of the 64 states of a head in a fixed order, no atomics: M over the wave (DPP rotations inside a row of
//     16 lanes, ds_bpermute across rows), over the waves through LDS, every state scaled by exp2(m - M), the 16
//     groups of a wave summed by the same four levels, the 4 waves summed through LDS in wave order by lane group i
//     of wave 0 for head i. P stays fp32 throughout.
//   * SPLIT: the workgroup of split z owns the keys [z C, min((z + 1) C, n)) (one step of the loop at C = 256),
//     returns before any load when it has none (z > 0), and writes (M, L, O[64]) to the fp32 workspace slot
//     (b, h, z) of attn_decode_split.hip; attn_decode_merge_kernel (launch_attn_decode_merge) finishes.
// No bit of a row depends on GC, B or Smax: the key -> (wave, load, group) map and every order above depend on the
// key index alone. Every GC carries no-packed-fp32-ops and calls force-inlined helpers only (see attn_decode.hip).
//
// kv_fill_f8_kernel: the prefill fill. One quad per (tensor, b, KV head, row s < S): 16-byte loads from the padded,
// already rotated QKV buffer, f8_quantize_row, 16-byte code stores and one scale. The same device function as the
// append, so a row quantised at prefill and one quantised at a step agree bit for bit.
#include "mlt_attn_decode.h"
#include "mlt_common.h"
#include "mlt_kernels.h"
#include "mlt_kv_f8.h"

namespace mlt {

__device__ __forceinline__ float4 f8_f4(float x, float y, float z, float w) {
  float4 r;
  r.x = x, r.y = y, r.z = z, r.w = w;
  return r;
}

template <int GC, bool ROPE, bool SPLIT>
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kDecWaves * 64) void attn_decode_f8_kernel(const uint16_t* __restrict__ qkv_new, int64_t ldq,
                                                                        uint8_t* __restrict__ kv8,
                                                                        float* __restrict__ kv_scale,
                                                                        const int* __restrict__ pos,
                                                                        uint16_t* __restrict__ out,
                                                                        float* __restrict__ ws, int H, int Hkv,
                                                                        int chunks, int Smax, float scale,
                                                                        const float* __restrict__ rope) {
  static_assert(GC >= 1 && GC <= kF8Groups, "the final sum of head i is lane group i of wave 0");
  __shared__ float s_m[GC][kDecWaves];
  __shared__ float s_l[GC][kDecWaves];
  __shared__ __attribute__((aligned(16))) float s_o[GC][kDecWaves][kDecHead];
  const int z = SPLIT ? blockIdx.y : 0, Z = SPLIT ? gridDim.y : 1;
  const int b = SPLIT ? blockIdx.z : blockIdx.y, B = SPLIT ? gridDim.z : gridDim.y;
  int n = pos[b];  // cached keys = the new token's row
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const int first = z * kDecSplitKeys;
  if (SPLIT && z > 0 && first >= n) return;  // no key of this split is cached: uniform, before any load or barrier
  const int end = SPLIT ? min(first + kDecSplitKeys, n) : n;  // this workgroup's keys: [first, end)

  const int hkv = blockIdx.x / chunks, ch = blockIdx.x - hkv * chunks;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 2, c = lane & 3;
  const int h0 = (hkv * chunks + ch) * GC;  // the first query head of this workgroup (G = chunks * GC)
  const int D = H * kDecHead;
  const float sl2 = scale * 1.4426950408889634f;  // exponents in base 2

  const uint16_t* row = qkv_new + (int64_t)b * ldq + c * kF8Dims;
  uint4 qr[GC][2];
#pragma unroll
  for (int i = 0; i < GC; ++i) {
    const uint4* p = reinterpret_cast<const uint4*>(row + (h0 + i) * kDecHead);
    qr[i][0] = p[0], qr[i][1] = p[1];
  }
  uint4 kn[2], vn[2];
  {
    const uint4* pk = reinterpret_cast<const uint4*>(row + D + hkv * kDecHead);
    const uint4* pv = reinterpret_cast<const uint4*>(row + D + (Hkv + hkv) * kDecHead);
    kn[0] = pk[0], kn[1] = pk[1], vn[0] = pv[0], vn[1] = pv[1];
  }
  if constexpr (ROPE) {  // this lane's 16 dims are eight whole pairs: 64 contiguous bytes of the table row
    const float4* tp = reinterpret_cast<const float4*>(rope + (int64_t)n * kDecHead + c * kF8Dims);
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const float4 t0 = tp[2 * x], t1 = tp[2 * x + 1];
      const float t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
      for (int i = 0; i < GC; ++i) qr[i][x] = dec_rotate(qr[i][x], t);
      kn[x] = dec_rotate(kn[x], t);
    }
  }
  uint8_t* kc = kv8 + ((int64_t)b * Hkv + hkv) * Smax * kDecHead + c * kF8Dims;  // this lane's bytes of key row 0
  uint8_t* vc = kc + (int64_t)B * Hkv * Smax * kDecHead;
  float* ksc = kv_scale + ((int64_t)b * Hkv + hkv) * Smax;  // the scale of key row 0
  float* vsc = ksc + (int64_t)B * Hkv * Smax;
  uint4 knq, vnq;  // the new token as the cache will hold it
  float dkn, dvn;
  f8_quantize_row(kn[0], kn[1], knq, dkn);
  f8_quantize_row(vn[0], vn[1], vnq, dvn);
  const bool seed = z == 0 && w == 0 && g == 0;  // the one state that starts with the new token
  if (ch == 0 && seed) {                         // the append, once per (b, KV head)
    *reinterpret_cast<uint4*>(kc + (int64_t)n * kDecHead) = knq;
    *reinterpret_cast<uint4*>(vc + (int64_t)n * kDecHead) = vnq;
    if (c == 0) ksc[n] = dkn, vsc[n] = dvn;
  }

  // head i's scaled new-token score is the first m of every state of head i, in every split
  float m[GC], l[GC], o[GC][kF8Dims];
  {
    float k[kF8Dims], v[kF8Dims];
    f8_unpack16(knq, k);
    f8_unpack16(vnq, v);
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const float sn = f8_dot(qr[i][0], qr[i][1], k) * dkn;
      m[i] = sn * sl2;
      l[i] = 0.f;
#pragma unroll
      for (int d = 0; d < kF8Dims; ++d) o[i][d] = 0.f;
      if (seed) {
        const float p = dec_exp2(fmaf(sn, sl2, -m[i]));
        const float pd = p * dvn;
        l[i] = p;
#pragma unroll
        for (int d = 0; d < kF8Dims; ++d) o[i][d] = pd * v[d];
      }
    }
  }

  for (int base = first + w * kF8WaveKeys; base < end; base += kF8BlockKeys) {
    uint4 kr[kDecUnroll], vr[kDecUnroll];
    float dk[kDecUnroll], dv[kDecUnroll];
    bool ok[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // all loads first: 8 x 16 bytes and 8 scale words in flight per lane
      const int j = base + u * kF8Groups + g;
      ok[u] = j < end;  // end <= n: rows >= n are stale; rows >= (z + 1) C are the next split's
      kr[u] = ok[u] ? *reinterpret_cast<const uint4*>(kc + (int64_t)j * kDecHead) : dec_u4(0, 0, 0, 0);
      dk[u] = ok[u] ? ksc[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int j = base + u * kF8Groups + g;
      vr[u] = ok[u] ? *reinterpret_cast<const uint4*>(vc + (int64_t)j * kDecHead) : dec_u4(0, 0, 0, 0);
      dv[u] = ok[u] ? vsc[j] : 0.f;
    }
    float s[GC][kDecUnroll], mx[GC];
#pragma unroll
    for (int i = 0; i < GC; ++i) mx[i] = m[i];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // one conversion of a K fragment, GC dot products
      float k[kF8Dims];
      f8_unpack16(kr[u], k);
#pragma unroll
      for (int i = 0; i < GC; ++i) {
        s[i][u] = f8_dot(qr[i][0], qr[i][1], k) * dk[u];
        mx[i] = fmaxf(mx[i], ok[u] ? s[i][u] * sl2 : -INFINITY);
      }
    }
#pragma unroll
    for (int i = 0; i < GC; ++i) {
      const float alpha = dec_exp2(m[i] - mx[i]);  // m is finite from the start
      m[i] = mx[i];
      l[i] *= alpha;
#pragma unroll
      for (int d = 0; d < kF8Dims; ++d) o[i][d] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // one conversion of a V fragment, GC accumulators
      float v[kF8Dims];
      f8_unpack16(vr[u], v);
#pragma unroll
      for (int i = 0; i < GC; ++i) {
        const float p = ok[u] ? dec_exp2(fmaf(s[i][u], sl2, -m[i])) : 0.f;
        const float pd = p * dv[u];  // the value row's scale, once per key
        l[i] += p;
#pragma unroll
        for (int d = 0; d < kF8Dims; ++d) o[i][d] = fmaf(pd, v[d], o[i][d]);
      }
    }
  }

  // merge of the 64 states, per head in a fixed order
#pragma unroll
  for (int i = 0; i < GC; ++i) {
    const float mw = f8_groups_max(m[i], lane);  // uniform inside a quad: the maximum over the 16 groups (exact)
    if (lane == 0) s_m[i][w] = mw;
  }
  dec_barrier();
#pragma unroll
  for (int i = 0; i < GC; ++i) {
    float M = s_m[i][0];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) M = fmaxf(M, s_m[i][x]);
    const float a = dec_exp2(m[i] - M);
    l[i] = f8_groups_sum(l[i] * a, lane);
#pragma unroll
    for (int d = 0; d < kF8Dims; ++d) o[i][d] = f8_groups_sum(o[i][d] * a, lane);
    if (g == 0) {
      float4* so = reinterpret_cast<float4*>(&s_o[i][w][c * kF8Dims]);
#pragma unroll
      for (int d = 0; d < kF8Dims; d += 4) so[d >> 2] = f8_f4(o[i][d], o[i][d + 1], o[i][d + 2], o[i][d + 3]);
      if (c == 0) s_l[i][w] = l[i];
    }
  }
  dec_barrier();
  if (w == 0 && g < GC) {  // lane group g sums head h0 + g over the waves, in wave order
    float M = s_m[g][0], L = s_l[g][0];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) {
      M = fmaxf(M, s_m[g][x]);
      L += s_l[g][x];
    }
    float t[kF8Dims];
#pragma unroll
    for (int d = 0; d < kF8Dims; ++d) {
      t[d] = s_o[g][0][c * kF8Dims + d];
#pragma unroll
      for (int x = 1; x < kDecWaves; ++x) t[d] += s_o[g][x][c * kF8Dims + d];
    }
    if constexpr (SPLIT) {  // the slot format of attn_decode_split.hip: M, L, two pad words, O[64]
      float* slot = ws + (((int64_t)b * H + h0 + g) * Z + z) * kDecSlotFloats;
      if (c == 0) *reinterpret_cast<float4*>(slot) = f8_f4(M, L, 0.f, 0.f);
      float4* od = reinterpret_cast<float4*>(slot + 4 + c * kF8Dims);
#pragma unroll
      for (int d = 0; d < kF8Dims; d += 4) od[d >> 2] = f8_f4(t[d], t[d + 1], t[d + 2], t[d + 3]);
    } else {
      const float inv = 1.0f / L;  // L >= the new token's p > 0
      uint32_t pk[kF8Dims / 2];
#pragma unroll
      for (int d = 0; d < kF8Dims; d += 2)
        pk[d >> 1] = (uint32_t)f32_to_bf16(t[d] * inv) | ((uint32_t)f32_to_bf16(t[d + 1] * inv) << 16);
      uint4* po = reinterpret_cast<uint4*>(out + (int64_t)b * D + (h0 + g) * kDecHead + c * kF8Dims);
      po[0] = dec_u4(pk[0], pk[1], pk[2], pk[3]);
      po[1] = dec_u4(pk[4], pk[5], pk[6], pk[7]);
    }
  }
}

void launch_attn_decode_f8(const uint16_t* qkv_new, int64_t ldq, uint8_t* kv8, float* kv_scale, const int* pos,
                           uint16_t* out, float* ws, int B, int H, int Hkv, int Smax, float scale, hipStream_t st,
                           const float* rope, int gc) {
  const bool split = ws != nullptr;
  const int G = H / Hkv, Z = split ? (Smax + kDecSplitKeys - 1) / kDecSplitKeys : 1;
  // the bf16 launchers' rule (B * Z workgroups per (KV head, chunk) in the split form): no bit depends on it
  if (gc <= 0) gc = attn_decode_gqa_chunk(G, Hkv, (int)std::min<long long>((long long)B * Z, 1 << 30));
  if (G * Hkv != H || G % gc != 0) throw_no_kernel("launch_attn_decode_f8", "heads per KV head", G);
  if (Z > 65535 || B > 65535) throw_no_kernel("launch_attn_decode_f8", "splits", Z);
  const int chunks = G / gc;
  const dim3 grid = split ? dim3(Hkv * chunks, Z, B) : dim3(Hkv * chunks, B), block(kDecWaves * 64);
  const bool hit = dispatch_int<1, 2, 3, 4, 6, 8>(gc, [&](auto c) {
    constexpr int GC = decltype(c)::value;
    dispatch_bools(
        [&](auto r, auto s) {
          attn_decode_f8_kernel<GC, decltype(r)::value, decltype(s)::value><<<grid, block, 0, st>>>(
              qkv_new, ldq, kv8, kv_scale, pos, out, ws, H, Hkv, chunks, Smax, scale, rope);
        },
        rope != nullptr, split);
  });
  if (!hit) throw_no_kernel("launch_attn_decode_f8", "GC", gc);
  if (split) launch_attn_decode_merge(ws, pos, out, B, H, Smax, st);
}

// One quad per cache row: r -> (tensor t, b, KV head, s), s fastest, so a wave stores 16 consecutive code rows.
__global__ __launch_bounds__(256) void kv_fill_f8_kernel(const uint16_t* __restrict__ qkv, int64_t ldq,
                                                         uint8_t* __restrict__ kv8, float* __restrict__ kv_scale,
                                                         int B, int S, int Hkv, int Smax, int koff, int voff,
                                                         int hstride, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * (256 / kF8Lanes) + (threadIdx.x >> 2);
  if (r >= rows) return;  // whole quads leave together
  const int c = threadIdx.x & 3;
  const int s = (int)(r % S);
  const int64_t bh = r / S;  // (t * B + b) * Hkv + hkv
  const int hkv = (int)(bh % Hkv);
  const int64_t tb = bh / Hkv;
  const int t = (int)(tb / B), b = (int)(tb - (int64_t)t * B);
  const uint4* src = reinterpret_cast<const uint4*>(qkv + ((int64_t)b * S + s) * ldq + (t ? voff : koff) +
                                                    hkv * hstride + c * kF8Dims);
  uint4 codes;
  float d;
  f8_quantize_row(src[0], src[1], codes, d);
  const int64_t dst = bh * Smax + s;
  *reinterpret_cast<uint4*>(kv8 + dst * kDecHead + c * kF8Dims) = codes;
  if (c == 0) kv_scale[dst] = d;
}

void launch_kv_fill_f8(const uint16_t* qkv, int64_t ldq, bool compact, uint8_t* kv8, float* kv_scale, int B, int S,
                       int H, int Hkv, int Smax, hipStream_t st) {
  if (Hkv < 1 || H % Hkv != 0) throw_no_kernel("launch_kv_fill_f8", "KV heads", Hkv);
  // wide [.., 3 H 64]: k / v heads equal within a group, every (H / Hkv)-th is taken; compact [.., (H + 2 Hkv) 64]
  const int koff = H * kDecHead, voff = (compact ? H + Hkv : 2 * H) * kDecHead;
  const int hstride = (compact ? 1 : H / Hkv) * kDecHead;
  const int64_t rows = 2ll * B * Hkv * S, per = 256 / kF8Lanes;
  if (rows <= 0) return;
  if ((rows + per - 1) / per > 0x7fffffffll) throw_no_kernel("launch_kv_fill_f8", "rows", rows);
  kv_fill_f8_kernel<<<dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, st>>>(qkv, ldq, kv8, kv_scale, B, S, Hkv,
                                                                                 Smax, koff, voff, hstride, rows);
}

}  // namespace mlt
