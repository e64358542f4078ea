// Decode attention over a PAGED key/value cache for gfx950, and the prefill fill of its pages.
//
// The contiguous kernels (attn_decode.hip, attn_decode_split.hip) find key j of a (batch, KV head) at base + j * 64:
// every sequence owns Smax rows from the start. Here the rows live in a pool of pages shared by all sequences,
//   pool [2, P, Hkv, kPageRows = 64, 64] bf16   (keys / values, page, KV head, row in page, dim),
// so the 64 rows of one (page, head) are 8 KiB contiguous, and a sequence names its pages in a row of
//   block_table int32 [B, max_pages]            (entry i = the page of rows 64 i .. 64 i + 63).
// Page 0 is the null page: the host never hands it out and every unowned table entry is 0, so a clamped or stale
// position lands there and nowhere else. The host owns the table and keeps every entry in [0, P); the kernels
// still send an entry outside that range to page 0 (one scalar compare) rather than trust it with an address.
//
// attn_decode_paged_kernel<GC, ROPE>, grid (Hkv * G / GC, Z, B), Z = ceil(max_pages * 64 / C), C = kDecSplitKeys:
//   * always the split form: split z owns the cached keys [z C, min((z + 1) C, n)), n = clamp(pos[b], 0,
//     max_pages * 64 - 1), writes (M, L, O[64]) of each of its heads to the workspace slot (b, h, z) of
//     attn_decode_split.hip, and attn_decode_merge_kernel (unchanged) finishes. A split z > 0 without a cached key
//     returns before any load or barrier.
//   * the key -> (wave, load, lane group) mapping is the contiguous kernels': key j -> wave (j % 128) / 32, load
//     (j % 32) / 8, lane group j % 8. A wave's 32-key run of step t of the key loop starts at z C + 128 t + 32 w: it
//     lies inside ONE page, number (C / 64) z + 2 t + w / 2 of the table row (at C = 256: pages w / 2 and 2 + w / 2
//     of the split), at rows 32 (w % 2) + 8 u + g of it.
//   * a wave reads its kDecPagedSteps = C / 128 page ids first of all, through a wave-uniform index
//     (readfirstlane of the wave number: scalar loads), before the new token's row and long before the first key
//     load: the table sits off the dependent chain of the stream. Every key and value address is then
//     page_base + row * 64 with a compile-time row term, kDecUnroll 16-byte loads of K and of V in flight per lane.
//   * everything else is attn_decode_split_kernel, expression for expression: the new token's score starts every
//     state, split 0 / wave 0 / group 0 seeds it from registers, stale rows are predicated off and selected out, the
//     32 states merge in the same fixed order. The arithmetic of a key does not see where its page lies, so out and
//     the appended row equal attn_decode_split on the cache gathered into contiguous form bit for bit, for every
//     GC and every placement of the pages (tests/test_attn_decode_paged_gpu.py).
//   * the append, once per (b, KV head) from head chunk 0: row n % 64 of page block_table[b][n / 64].
//
// kv_fill_paged_kernel: the prompt's K / V out of a layer's padded (already rotated) wide QKV buffer
// [B * S, 3 * H * 64] into the pages, one launch per layer. One lane per 16-byte chunk, 8 lanes per cache row, rows
// s fastest: a wave stores 8 consecutive rows = 1 KiB contiguous inside a page. A grouped-query pool takes every
// (H / Hkv)-th k / v head. Rows at and past a sequence's length are written like the rest (stale by pos).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; ROPE changes none of them):
//   GC                1      2      3      4      6      8     kv_fill_paged_kernel
//   VGPRs            63    105    107    147    197    230     18
//   LDS bytes     1,056  2,112  3,168  4,224  6,336  8,448      0
//   scratch           0      0      0      0      0      0      0
//   waves / SIMD      8      4      4      3      2      2      8
#include "mlt_attn_decode.h"
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

constexpr int kPageRows = 64;                                     // rows of one (page, head): 8 KiB of bf16
constexpr int kPageElems = kPageRows * kDecHead;                  // elements of one (page, head)
constexpr int kDecPagedSteps = kDecSplitKeys / kDecBlockKeys;     // steps of the key loop per split
constexpr int kDecSplitPages = kDecSplitKeys / kPageRows;         // pages per split
static_assert(kPageRows % kDecWaveKeys == 0, "a wave's run of keys must lie inside one page");
static_assert(kDecSplitKeys % kPageRows == 0, "a split is whole pages");

__device__ __forceinline__ float4 pg_f4(float x, float y, float z, float w) {  // make_float4 without a call
  float4 r;
  r.x = x, r.y = y, r.z = z, r.w = w;
  return r;
}

// entry i of a table row, or the null page where the table has no such entry or holds a value outside the pool
__device__ __forceinline__ int pg_page(const int* __restrict__ bt_row, int i, int max_pages, int P) {
  const int p = i < max_pages ? bt_row[i] : 0;
  return (unsigned)p < (unsigned)P ? p : 0;
}

// no-packed-fp32-ops: as attn_decode_split_kernel, whose bits this kernel must reproduce.
template <int GC, bool ROPE>
__attribute__((target("no-packed-fp32-ops"))) __global__
__launch_bounds__(kDecWaves * 64) void attn_decode_paged_kernel(const uint16_t* __restrict__ qkv_new,
                                                                           int64_t ldq, uint16_t* __restrict__ pool,
                                                                           const int* __restrict__ block_table,
                                                                           const int* __restrict__ pos,
                                                                           float* __restrict__ ws, int H, int Hkv,
                                                                           int chunks, int max_pages, int P,
                                                                           float scale,
                                                                           const float* __restrict__ rope) {
  static_assert(GC >= 1 && GC <= 8, "the final sum of head i is lane group i of wave 0");
  __shared__ float s_m[GC][kDecWaves];
  __shared__ float s_l[GC][kDecWaves];
  __shared__ float s_o[GC][kDecWaves][kDecHead];
  const int z = blockIdx.y, Z = gridDim.y, b = blockIdx.z;
  const int Smax = max_pages * kPageRows;
  int n = pos[b];  // cached keys = the new token's row
  MLT_DCHECK(n >= 0 && n < Smax);
  n = min(max(n, 0), Smax - 1);
  const int first = z * kDecSplitKeys;
  if (z > 0 && first >= n) return;  // no key of this split is cached: uniform, before any load or barrier
  const int end = min(first + kDecSplitKeys, n);  // this split's keys: [first, end)

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 3, c = lane & 7;
  // this wave's pages, one per step of the key loop: wave-uniform indices, so the loads are scalar and are issued
  // here, ahead of everything the key loop waits for
  const int* bt_row = block_table + (int64_t)b * max_pages;
  const int wu = __builtin_amdgcn_readfirstlane(w);
  int page[kDecPagedSteps];
#pragma unroll
  for (int t = 0; t < kDecPagedSteps; ++t)
    page[t] = pg_page(bt_row, z * kDecSplitPages + t * (kDecBlockKeys / kPageRows) + wu / 2, max_pages, P);

  const int hkv = blockIdx.x / chunks, ch = blockIdx.x - hkv * chunks;
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
  // this lane's dims of row 0 of page 0 of its KV head; a page is Hkv * kPageElems further, the values P pages
  uint16_t* kc = pool + (int64_t)hkv * kPageElems + c * 8;
  const int64_t page_stride = (int64_t)Hkv * kPageElems, v_off = (int64_t)P * page_stride;
  const bool seed = z == 0 && w == 0 && g == 0;  // the one state that starts with the new token
  if (ch == 0 && seed) {                         // the append, once per (b, KV head)
    uint16_t* dst = kc + pg_page(bt_row, n / kPageRows, max_pages, P) * page_stride + (n % kPageRows) * kDecHead;
    *reinterpret_cast<uint4*>(dst) = kn;
    *reinterpret_cast<uint4*>(dst + v_off) = vn;
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

  const int r0 = (w & 1) * kDecWaveKeys + g;  // this lane's row of load 0 inside the wave's page
#pragma unroll
  for (int t = 0; t < kDecPagedSteps; ++t) {
    const int base = first + t * kDecBlockKeys + w * kDecWaveKeys;
    if (base >= end) break;
    const uint16_t* kp = kc + page[t] * page_stride + r0 * kDecHead;  // key base + u * 8 of this step, load u
    const uint16_t* vp = kp + v_off;
    uint4 kr[kDecUnroll], vr[kDecUnroll];
    bool ok[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {  // all loads first: 8 x 16 bytes in flight per lane, whatever GC
      const int j = base + u * 8 + g;
      ok[u] = j < end;  // end <= n: rows >= n are stale; rows >= (z + 1) C are the next split's
      kr[u] = ok[u] ? *reinterpret_cast<const uint4*>(kp + u * 8 * kDecHead) : dec_u4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u)
      vr[u] = ok[u] ? *reinterpret_cast<const uint4*>(vp + u * 8 * kDecHead) : dec_u4(0, 0, 0, 0);
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
    if (c == 0) *reinterpret_cast<float4*>(slot) = pg_f4(M, L, 0.f, 0.f);
    float4* od = reinterpret_cast<float4*>(slot + 4 + c * 8);
    od[0] = pg_f4(t[0], t[1], t[2], t[3]);
    od[1] = pg_f4(t[4], t[5], t[6], t[7]);
  }
}

int attn_decode_paged_page_rows() { return kPageRows; }

void launch_attn_decode_paged(const uint16_t* qkv_new, int64_t ldq, uint16_t* pool, const int* block_table,
                              const int* pos, uint16_t* out, float* ws, int B, int H, int Hkv, int max_pages, int P,
                              float scale, hipStream_t st, const float* rope, int gc) {
  if (max_pages < 1 || max_pages > 0x7fffffff / kPageRows) throw_no_kernel("launch_attn_decode_paged", "pages", max_pages);
  const int Smax = max_pages * kPageRows;
  const int G = H / Hkv, Z = (Smax + kDecSplitKeys - 1) / kDecSplitKeys;
  // launch_attn_decode_split's rule: no bit depends on it
  if (gc <= 0) gc = attn_decode_gqa_chunk(G, Hkv, (int)std::min<long long>((long long)B * Z, 1 << 30));
  if (G * Hkv != H || G % gc != 0) throw_no_kernel("launch_attn_decode_paged", "heads per KV head", G);
  if (Z > 65535 || B > 65535) throw_no_kernel("launch_attn_decode_paged", "splits", Z);
  if (P < 1) throw_no_kernel("launch_attn_decode_paged", "pool pages", P);
  const int chunks = G / gc;
  const dim3 grid(Hkv * chunks, Z, B), block(kDecWaves * 64);
  const bool hit = dispatch_int<1, 2, 3, 4, 6, 8>(gc, [&](auto c) {
    constexpr int GC = decltype(c)::value;
    dispatch_bools(
        [&](auto r) {
          attn_decode_paged_kernel<GC, decltype(r)::value><<<grid, block, 0, st>>>(
              qkv_new, ldq, pool, block_table, pos, ws, H, Hkv, chunks, max_pages, P, scale, rope);
        },
        rope != nullptr);
  });
  if (!hit) throw_no_kernel("launch_attn_decode_paged", "GC", gc);
  launch_attn_decode_merge(ws, pos, out, B, H, Smax, st);
}

// One lane per 16-byte chunk: item -> (tensor t, b, KV head, s, chunk c), c fastest, then s.
__global__ __launch_bounds__(256) void kv_fill_paged_kernel(const uint16_t* __restrict__ qkv, int64_t ldq,
                                                            uint16_t* __restrict__ pool,
                                                            const int* __restrict__ block_table, int B, int S,
                                                            int Hkv, int max_pages, int P, int koff, int voff,
                                                            int hstride, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * (256 / 8) + (threadIdx.x >> 3);
  if (r >= rows) return;
  const int c = threadIdx.x & 7;
  const int s = (int)(r % S);
  const int64_t bh = r / S;  // (t * B + b) * Hkv + hkv
  const int hkv = (int)(bh % Hkv);
  const int64_t tb = bh / Hkv;
  const int t = (int)(tb / B), b = (int)(tb - (int64_t)t * B);
  const uint4 x = *reinterpret_cast<const uint4*>(qkv + ((int64_t)b * S + s) * ldq + (t ? voff : koff) +
                                                  hkv * hstride + c * 8);
  const int page = pg_page(block_table + (int64_t)b * max_pages, s / kPageRows, max_pages, P);
  uint16_t* dst = pool + (((int64_t)t * P + page) * Hkv + hkv) * kPageElems + (s % kPageRows) * kDecHead + c * 8;
  *reinterpret_cast<uint4*>(dst) = x;
}

void launch_kv_fill_paged(const uint16_t* qkv, int64_t ldq, uint16_t* pool, const int* block_table, int B, int S,
                          int H, int Hkv, int max_pages, int P, hipStream_t st) {
  if (Hkv < 1 || H % Hkv != 0) throw_no_kernel("launch_kv_fill_paged", "KV heads", Hkv);
  if (P < 1 || max_pages < 1 || S > (int64_t)max_pages * kPageRows) throw_no_kernel("launch_kv_fill_paged", "rows", S);
  // the wide buffer [.., 3 H 64]: k / v heads are equal within a group, every (H / Hkv)-th is taken
  const int koff = H * kDecHead, voff = 2 * H * kDecHead, hstride = (H / Hkv) * kDecHead;
  const int64_t rows = 2ll * B * Hkv * S, per = 256 / 8;
  if (rows <= 0) return;
  if ((rows + per - 1) / per > 0x7fffffffll) throw_no_kernel("launch_kv_fill_paged", "rows", rows);
  kv_fill_paged_kernel<<<dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, st>>>(
      qkv, ldq, pool, block_table, B, S, Hkv, max_pages, P, koff, voff, hstride, rows);
}

}  // namespace mlt
