// Multi-token append attention over the key/value cache for gfx950: T = 1 .. 16 new tokens per sequence attend to
// the cached rows and, causally, to each other, in ONE pass over the cache; their k / v are appended. This is the
// decode kernels' function with a query TILE, and therefore the decode path's MFMA form: with one query per head a
// 16x16x32 MFMA has 15 idle columns, with up to 16 new tokens the tile is full.
//
// Function. qkv_new [B * T, ldq] bf16 (row b T + t = token t of sequence b; compact q (H) | k (Hkv) | v (Hkv) heads of
// 64, which is q | k | v when Hkv == H), kv [2, B, Hkv, Smax, 64] bf16, pos int32 [B] on the device. With
// n = clamp(pos[b], 0, Smax - T):
//   out[b T + t, h] = sum_j softmax_j(scale q_t . k_j) v_j   over the cached rows j < n of KV head h / G and the new
//   tokens t' <= t;   cache rows n .. n + T - 1 <- the new k / v;   pos is not changed.
// ROPE: q_t and the new k_t are rotated by position n + t (dec_rotate) and rounded to bf16 before the dot product and
// the append. The new tokens enter the arithmetic from qkv_new, never from the rows just written: no fence, one launch.
//
// Partition. One 256-thread workgroup per (KV head x chunk of GC query heads, key split z, batch): grid
// (Hkv G / GC, Z, B). Wave w of a workgroup takes keys base + 32 w .. + 31 of every 128-key step (kDecBlockKeys), so
// the key -> wave assignment is a function of the key index alone. SPLIT: split z owns the cached keys
// [z C, min((z + 1) C, n)), C = kDecSplitKeys; a split z > 0 with z C >= n returns before any load or barrier.
// Split 0 always runs, owns the T new keys (the causal triangle, in its wave 0) and does the append, from head chunk 0.
//
// Scores, swapped product: S^T (16 keys x 16 queries) = K . Q^T with v_mfma_f32_16x16x32_bf16. The K tile is the A
// operand, one 16-byte global load per lane (key j0 + (lane & 15), dims 32 kh + 8 (lane >> 4) .. + 7) straight from
// the head-major cache row into the VGPRs the MFMA reads: no LDS on the K side. The two loads of a tile (kh = 0, 1)
// are issued back to back and together cover the 16 whole 128-byte rows. The queries of a head are the B operand in
// the same dim order, loaded once (rows t >= T zero), rotated, and held for the whole loop: 8 VGPRs per head. A lane
// then holds query lane & 15 and keys 4 (lane >> 4) + r of each tile.
//
// Softmax state, base 2 (sl2 = scale log2 e, p = exp2(fma(s, sl2, -m))). The running maximum m belongs to the QUERY:
// the P . V MFMA sums over the four key quarters of a query (lanes lane ^ 16, 32, 48), so they must share one scale,
// and the step maximum is exchanged over those lanes. The sum l is lane-local (the lane's own keys) and is taken over
// the bf16-rounded p, the weights the MFMA multiplies, so 1 / l normalises exactly what was summed.
// Finite start: every wave computes the new tile's scores (two MFMAs per head) and starts every state at
// m = its query's own diagonal score, l = 0, O = 0, so no state ever forms exp2(-inf + inf). Only (split 0, wave 0)
// accumulates the new tile: key t' is visible to query t iff t' <= t (and t' < T); invisible scores are selected to
// -inf and their p to 0 before any arithmetic.
//
// P . V: O^T (64 dims x 16 queries) += V^T . P^T per 32 keys. P^T is the bf16 pack of the lane's own accumulators of
// the step's two tiles: element j of the B operand is key 16 (j >> 2) + 4 (lane >> 4) + (j & 3), and V^T is read in
// that same order, so nothing moves between lanes. V^T comes from the wave's 32 V rows (4 KB) in a wave-private LDS
// region, 128-byte rows with the 16-byte chunks xor-swizzled by row & 7, read with ds_read_b64_tr_b16.
// The staging is REGISTER-STAGED (global -> VGPR -> LDS), not global_load_lds_dwordx4: a stale row must be ZERO in
// LDS (the MFMA computes 0 * NaN = NaN where the VALU kernels select), and a predicated-off LDS-direct load leaves
// whatever the region held; the register path also writes the swizzled image with no constraint on the global side,
// and the next step's V waits in registers while this step's MFMAs run, so one region per wave is enough.
// The key loop has wave-level hand-offs only (wave_lds_sync); the 4 K + 4 V sixteen-byte loads of the next step are
// issued before this step's MFMAs. O is 16 accumulator VGPRs per head. Every K fragment and every V^T fragment read
// feeds the MFMAs of all GC heads.
//
// Stale rows (j >= n) are never loaded: their K and V fragments are zeros, their scores selected to -inf, their p
// to 0. A non-finite value in a NEW token can reach the rows of earlier tokens of its sequence through 0 * NaN in
// the triangle's MFMA; that is a property of the MFMA form, not a defect.
//
// Merge: l over the quarters by butterfly (xor 16, 32), then the 4 waves through LDS in wave order, one head at a
// time (the staging regions are reused): M = max, a_w = exp2(m_w - M), L = a_0 l_0 then fma in wave order, O alike.
// No atomics, no counters: bitwise reproducible, and no bit depends on GC, B, Smax or the batch.
// SPLIT = false: out = bf16(O / L). SPLIT = true: (M, L, O[64]) fp32 into ws [B T, H, Z, 68] (the slot layout of
// attn_decode_split.hip, 16-byte stores) and split 0 writes row_pos[b T + t] = n; launch_attn_decode_merge over
// B T rows with row_pos as its pos then finishes: its Za = max(1, ceil(n / C)) is the set of splits that wrote.
#include <algorithm>

#include "mlt_attn_decode.h"
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

namespace {

typedef __bf16 app_bf16x8 __attribute__((ext_vector_type(8)));
typedef short app_s16x4 __attribute__((ext_vector_type(4)));
typedef short app_s16x8 __attribute__((ext_vector_type(8)));
typedef float app_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) app_s16x4 app_lds_s16x4;

constexpr int kAppTokens = 16;              // the query tile: new tokens per sequence and launch
constexpr int kAppWaveKeys = 32;            // keys per wave per step: two score tiles, one P . V contraction
constexpr int kAppWaveBytes = kAppWaveKeys * 128;  // a wave's V staging region
static_assert(kAppWaveKeys * kDecWaves == kDecBlockKeys, "the decode kernels' keys per workgroup step");

__device__ __forceinline__ app_f32x4 app_mfma(app_bf16x8 a, app_bf16x8 b, app_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ app_bf16x8 app_frag(const uint4& r) { return __builtin_bit_cast(app_bf16x8, r); }
__device__ __forceinline__ uint4 app_load(const uint16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p) : dec_u4(0, 0, 0, 0);
}
// [32 rows][64 bf16] image, 128-byte rows, 16-byte chunks xor-swizzled by row & 7
__device__ __forceinline__ int app_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
// V^T fragment: dim col + (lane & 15) of rows 4 g + q and 16 + 4 g + q, q = 0 .. 3 (two ds_read_b64_tr_b16)
__device__ __forceinline__ app_bf16x8 app_frag_tr(const uint8_t* lds, int lane, int col) {
  const int i = lane & 15, g = lane >> 4, q = i >> 2, cc = col + 4 * (i & 3), chunk = cc >> 3, half = (cc & 7) * 2;
  const app_s16x4 lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((app_lds_s16x4*)(lds + app_off(4 * g + q, chunk) + half));
  const app_s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((app_lds_s16x4*)(lds + app_off(16 + 4 * g + q, chunk) + half));
  const app_s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(app_bf16x8, r);
}
// a lane's four V chunks of a step -> the wave's region: row 8 u + (lane >> 3), chunk lane & 7
__device__ __forceinline__ void app_stage(uint8_t* lds, int lane, const uint4 (&v)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) *reinterpret_cast<uint4*>(lds + app_off(8 * u + (lane >> 3), lane & 7)) = v[u];
}
__device__ __forceinline__ float4 app_f4(float x, float y, float z, float w) {
  float4 r;
  r.x = x, r.y = y, r.z = z, r.w = w;
  return r;
}

// One step of a wave: the scores of two 16-key tiles kf[tile][kh] against the GC query tiles, the online softmax of
// the lane's keys (ok[tile][r]: key 16 tile + 4 (lane >> 4) + r takes part), and P . V against the 32 V rows staged
// in vl. m is the query's (shared by its four lanes), l the lane's.
template <int GC>
__device__ __forceinline__ void app_step(const uint4 (&kf)[2][2], const app_bf16x8 (&qf)[GC][2], const bool (&ok)[2][4],
                                         const uint8_t* vl, float sl2, int lane, float (&m)[GC], float (&l)[GC],
                                         app_f32x4 (&o)[GC][4]) {
  app_bf16x8 pb[GC];
#pragma unroll
  for (int hh = 0; hh < GC; ++hh) {
    app_f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = app_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) s[t] = app_mfma(app_frag(kf[t][kh]), qf[hh][kh], s[t]);
    }
    float mx = m[hh];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, ok[t][r] ? s[t][r] * sl2 : -INFINITY);
    mx = fmaxf(mx, dec_xor(mx, lane, 16));  // the query's four key quarters
    mx = fmaxf(mx, dec_xor(mx, lane, 32));
    const float alpha = dec_exp2(m[hh] - mx);  // m is finite from the start
    m[hh] = mx;
    l[hh] *= alpha;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[hh][d] *= alpha;
    app_s16x8 pk;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = ok[t][r] ? dec_exp2(fmaf(s[t][r], sl2, -mx)) : 0.f;
        const uint16_t pr = f32_to_bf16(p);
        l[hh] += bf16_to_f32(pr);  // the weight the MFMA multiplies
        pk[4 * t + r] = (short)pr;
      }
    pb[hh] = __builtin_bit_cast(app_bf16x8, pk);
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {  // one V^T fragment read, GC MFMAs
    const app_bf16x8 va = app_frag_tr(vl, lane, d * 16);
#pragma unroll
    for (int hh = 0; hh < GC; ++hh) o[hh][d] = app_mfma(va, pb[hh], o[hh][d]);
  }
}

}  // namespace

template <int GC, bool ROPE, bool SPLIT>
__global__ __launch_bounds__(kDecWaves * 64) void attn_append_kernel(
    const uint16_t* __restrict__ qkv_new, int64_t ldq, uint16_t* __restrict__ kv, const int* __restrict__ pos,
    uint16_t* __restrict__ out, float* __restrict__ ws, int* __restrict__ row_pos, int T, int H, int Hkv, int chunks,
    int Smax, float scale, const float* __restrict__ rope) {
  __shared__ __attribute__((aligned(16))) uint8_t s_v[kDecWaves * kAppWaveBytes];  // V staging; then the merge's O
  __shared__ float s_m[kDecWaves][kAppTokens];
  __shared__ float s_l[kDecWaves][kAppTokens];
  static_assert(kDecWaves * kAppTokens * kDecHead * 4 <= kDecWaves * kAppWaveBytes, "the merge reuses the staging");
  const int z = SPLIT ? blockIdx.y : 0, Z = gridDim.y, b = blockIdx.z, B = gridDim.z;
  int n = pos[b];  // cached keys = the row the first new token takes
  MLT_DCHECK(n >= 0 && n + T <= Smax);
  n = min(max(n, 0), Smax - T);
  const int first = z * kDecSplitKeys;
  if (z > 0 && first >= n) return;  // no key of this split is cached: uniform, before any load or barrier
  const int end = SPLIT ? min(first + kDecSplitKeys, n) : n;  // this workgroup's cached keys: [first, end)

  const int hkv = blockIdx.x / chunks, ch = blockIdx.x - hkv * chunks;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, i = lane & 15;
  const int h0 = (hkv * chunks + ch) * GC;  // the first query head of this workgroup (G = chunks * GC)
  const int D = H * kDecHead;
  const float sl2 = scale * 1.4426950408889634f;  // exponents in base 2
  uint8_t* vl = s_v + w * kAppWaveBytes;

  const uint16_t* rows = qkv_new + (int64_t)b * T * ldq;  // the T rows of this sequence
  uint16_t* kc = kv + ((int64_t)b * Hkv + hkv) * Smax * kDecHead;
  uint16_t* vc = kc + (int64_t)B * Hkv * Smax * kDecHead;
  const bool tok = i < T;  // this lane's query / new key is a token; the tile's other rows are zeros
  const uint16_t* qrow = rows + (int64_t)min(i, T - 1) * ldq + 8 * g;

  // the first step's loads go out before anything is computed
  const int vrow = lane >> 3, vcol = (lane & 7) * 8;
  uint4 kr[2][2], vr[4];
  const int base0 = first + w * kAppWaveKeys;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int j = base0 + 16 * t + i;
      kr[t][kh] = app_load(kc + (int64_t)j * kDecHead + 32 * kh + 8 * g, j < end);
    }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = base0 + 8 * u + vrow;
    vr[u] = app_load(vc + (int64_t)j * kDecHead + vcol, j < end);
  }

  // the query tiles and the new key tile, in the MFMA's dim order: dims 32 kh + 8 g .. + 7 = rope chunk 4 kh + g
  app_bf16x8 qf[GC][2];
  uint4 kn[2][2];
  {
    float rt[2][8];
    if constexpr (ROPE) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const float4* tp =
            reinterpret_cast<const float4*>(rope + (int64_t)(n + min(i, T - 1)) * kDecHead + (4 * kh + g) * 8);
        const float4 t0 = tp[0], t1 = tp[1];
        rt[kh][0] = t0.x, rt[kh][1] = t0.y, rt[kh][2] = t0.z, rt[kh][3] = t0.w;
        rt[kh][4] = t1.x, rt[kh][5] = t1.y, rt[kh][6] = t1.z, rt[kh][7] = t1.w;
      }
    }
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
      for (int hh = 0; hh < GC; ++hh) {
        uint4 q = app_load(qrow + (h0 + hh) * kDecHead + 32 * kh, tok);
        if constexpr (ROPE) q = dec_rotate(q, rt[kh]);  // zeros stay zeros
        qf[hh][kh] = app_frag(q);
      }
      kn[0][kh] = app_load(qrow + D + hkv * kDecHead + 32 * kh, tok);
      if constexpr (ROPE) kn[0][kh] = dec_rotate(kn[0][kh], rt[kh]);
      kn[1][kh] = dec_u4(0, 0, 0, 0);
    }
  }
  const bool owner = z == 0 && w == 0;  // the wave that holds the new tokens
  if (owner && ch == 0 && tok) {        // the append of k, once per (b, KV head)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
      *reinterpret_cast<uint4*>(kc + (int64_t)(n + i) * kDecHead + 32 * kh + 8 * g) = kn[0][kh];
  }
  if (SPLIT && z == 0 && blockIdx.x == 0 && tid < T) row_pos[b * T + tid] = n;

  // every state starts at its query's own diagonal score: key t' = i sits in lane group i >> 2, element i & 3
  float m[GC], l[GC];
  app_f32x4 o[GC][4];
#pragma unroll
  for (int hh = 0; hh < GC; ++hh) {
    app_f32x4 sn = app_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) sn = app_mfma(app_frag(kn[0][kh]), qf[hh][kh], sn);
    float dg = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) dg = 4 * g + r == i ? sn[r] * sl2 : dg;
    dg = fmaxf(dg, dec_xor(dg, lane, 16));
    dg = fmaxf(dg, dec_xor(dg, lane, 32));
    m[hh] = dg;
    l[hh] = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[hh][d] = app_f32x4{0.f, 0.f, 0.f, 0.f};
  }

  if (owner) {  // the causal triangle: the T new keys as tile 0 of a step whose tile 1 is empty
    uint4 vn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = 8 * u + vrow;
      const bool real = t < T;  // rows t >= T are zero-filled
      vn[u] = app_load(rows + (int64_t)min(t, T - 1) * ldq + D + (Hkv + hkv) * kDecHead + vcol, real);
      if (real && ch == 0) *reinterpret_cast<uint4*>(vc + (int64_t)(n + t) * kDecHead + vcol) = vn[u];  // the append of v
    }
    app_stage(vl, lane, vn);
    wave_lds_sync();
    bool ok[2][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ok[0][r] = 4 * g + r <= i && 4 * g + r < T;
      ok[1][r] = false;
    }
    app_step<GC>(kn, qf, ok, vl, sl2, lane, m, l, o);
  }

  for (int base = base0; base < end; base += kDecBlockKeys) {
    wave_lds_sync();  // the previous step's V^T reads precede this step's image
    app_stage(vl, lane, vr);
    wave_lds_sync();
    uint4 kx[2][2];
    const int nb = base + kDecBlockKeys;  // the next step's loads: in flight over this step's MFMAs
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int j = nb + 16 * t + i;
        kx[t][kh] = app_load(kc + (int64_t)j * kDecHead + 32 * kh + 8 * g, j < end);
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = nb + 8 * u + vrow;
      vr[u] = app_load(vc + (int64_t)j * kDecHead + vcol, j < end);
    }
    bool ok[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) ok[t][r] = base + 16 * t + 4 * g + r < end;  // end <= n: rows >= n are stale
    app_step<GC>(kr, qf, ok, vl, sl2, lane, m, l, o);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) kr[t][kh] = kx[t][kh];
  }

  // merge: l over the query's quarters by butterfly, then the waves through LDS in wave order, head by head
  float* s_o = reinterpret_cast<float*>(s_v);  // [wave][query][64]
  const int qi = tid >> 4, dc = (tid & 15) * 4;
#pragma unroll
  for (int hh = 0; hh < GC; ++hh) {
    float lq = l[hh];
    lq += dec_xor(lq, lane, 16);
    lq += dec_xor(lq, lane, 32);
    dec_barrier();  // every wave is out of its key loop / the previous head is read
#pragma unroll
    for (int d = 0; d < 4; ++d)
      *reinterpret_cast<app_f32x4*>(s_o + (w * kAppTokens + i) * kDecHead + 16 * d + 4 * g) = o[hh][d];
    if (g == 0) {
      s_m[w][i] = m[hh];
      s_l[w][i] = lq;
    }
    dec_barrier();
    float M = s_m[0][qi];
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) M = fmaxf(M, s_m[x][qi]);
    const float a0 = dec_exp2(s_m[0][qi] - M);
    float L = a0 * s_l[0][qi];
    const app_f32x4 o0 = *reinterpret_cast<const app_f32x4*>(s_o + qi * kDecHead + dc);
    float O[4] = {a0 * o0[0], a0 * o0[1], a0 * o0[2], a0 * o0[3]};
#pragma unroll
    for (int x = 1; x < kDecWaves; ++x) {
      const float a = dec_exp2(s_m[x][qi] - M);
      L = fmaf(a, s_l[x][qi], L);
      const app_f32x4 ox = *reinterpret_cast<const app_f32x4*>(s_o + (x * kAppTokens + qi) * kDecHead + dc);
#pragma unroll
      for (int e = 0; e < 4; ++e) O[e] = fmaf(a, ox[e], O[e]);
    }
    if (qi < T) {
      const int64_t row = (int64_t)b * T + qi;
      if constexpr (SPLIT) {
        float* slot = ws + ((row * H + h0 + hh) * Z + z) * kDecSlotFloats;
        if (dc == 0) *reinterpret_cast<float4*>(slot) = app_f4(M, L, 0.f, 0.f);
        *reinterpret_cast<float4*>(slot + 4 + dc) = app_f4(O[0], O[1], O[2], O[3]);
      } else {
        const float inv = 1.0f / L;  // L >= the diagonal's p > 0
        ushort4 u;
        u.x = f32_to_bf16(O[0] * inv);
        u.y = f32_to_bf16(O[1] * inv);
        u.z = f32_to_bf16(O[2] * inv);
        u.w = f32_to_bf16(O[3] * inv);
        *reinterpret_cast<ushort4*>(out + row * D + (h0 + hh) * kDecHead + dc) = u;
      }
    }
  }
}

int attn_append_max_tokens() { return kAppTokens; }

void launch_attn_append(const uint16_t* qkv_new, int64_t ldq, uint16_t* kv, const int* pos, uint16_t* out, float* ws,
                        int* row_pos, int B, int T, int H, int Hkv, int Smax, float scale, hipStream_t st,
                        const float* rope, int gc) {
  const bool split = ws != nullptr;
  const int G = H / Hkv, Z = split ? (Smax + kDecSplitKeys - 1) / kDecSplitKeys : 1;
  if (T < 1 || T > kAppTokens || T > Smax) throw_no_kernel("launch_attn_append", "T", T);
  if (split != (row_pos != nullptr)) throw_no_kernel("launch_attn_append", "ws without row_pos", split);
  // the decode launchers' rule: the largest chunk that still fills the machine; no bit depends on it
  if (gc <= 0) gc = attn_decode_gqa_chunk(G, Hkv, (int)std::min<long long>((long long)B * Z, 1 << 30));
  if (G * Hkv != H || G % gc != 0) throw_no_kernel("launch_attn_append", "heads per KV head", G);
  if (Z > 65535 || B > 65535) throw_no_kernel("launch_attn_append", "splits", Z);
  const int chunks = G / gc;
  const dim3 grid(Hkv * chunks, Z, B), block(kDecWaves * 64);
  // every listed GC is built: none uses scratch (docs/ARCHITECTURE.md has the register table)
  const bool hit = dispatch_int<1, 2, 3, 4>(gc, [&](auto c) {
    constexpr int GC = decltype(c)::value;
    dispatch_bools(
        [&](auto r, auto s) {
          attn_append_kernel<GC, decltype(r)::value, decltype(s)::value><<<grid, block, 0, st>>>(
              qkv_new, ldq, kv, pos, out, ws, row_pos, T, H, Hkv, chunks, Smax, scale, rope);
        },
        rope != nullptr, split);
  });
  if (!hit) throw_no_kernel("launch_attn_append", "GC", gc);
  if (split) launch_attn_decode_merge(ws, row_pos, out, B * T, H, Smax, st);
}

}  // namespace mlt
