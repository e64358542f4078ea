// sample_step for gfx950: the next token of every sequence from its fp32 logits row, in one launch, with the
// token / EOS bookkeeping of generate() done on the device. The definition (steps 1-6) is the header comment of
// mlt_sample.h; this file is how it is computed.
//
// One workgroup per row, kSampleThreads = 1024 threads. A row is 122 KB at a 30,720-wide vocabulary and one
// workgroup runs on one CU, so every pass over it is bound by how many 16-byte loads that CU has in flight: 16
// waves (the most a workgroup can have) put 16 KB in flight per load instruction and a pass is 8 of them per
// thread. The batch is 1 .. 64 rows on 256 CUs: there is no second workgroup to share the CU with, so nothing is
// gained by leaving room for one. The LDS (16.3 KB) and the registers (no scratch) do not limit this.
//
// Passes. Each re-reads the row (L2-resident: the decoder GEMM has just written it) with coalesced 16-byte loads,
// thread t taking vectors t, t + 1024, ...; the passes a setting does not need are skipped.
//   argmax   always. Per thread the maximum of (key << 32 | ~index), key = the order-preserving integer image of
//            the logit (sample_key), reduced by xor butterflies and 16 LDS words: the maximum, smallest index first.
//   top-k    3 radix-select passes over the key (11 + 11 + 10 bits, high to low): an LDS histogram of COUNTS of the
//            keys that match the digits selected so far, a block scan from the highest bin down, the bin where the
//            running count reaches k. After 3 passes the key of T_k is known exactly.
//   top-p    the same 3 passes with uint64 WEIGHT sums (sample_weight, restricted to keys >= key(T_k)) in place of
//            counts; the first pass's grand total is W_K, which gives `need`.
//   draw     thread t owns the contiguous indices [t * C, (t + 1) * C): its weight sum over S, a block exclusive
//            scan of those uint64 sums (W_S is the total), and the thread whose interval holds r walks its range.
// The histograms are filled with integer LDS atomics (ds_add_u64): integer addition is exact and commutative, so
// a bin's value does not depend on arrival order, which is why the weights are fixed-point. A thread adds up a run
// of equal digits in registers before it issues the atomic: logits crowd into a few high-digit bins, and one add
// per run in place of one per element takes most of the same-address serialisation out of the first pass.
// No float atomics, no float sums, no cross-block traffic: a row's block reads and writes only that row's state.
//
// draws[b] < T cannot be checked without a read: debug builds check it (MLT_DCHECK), every build clamps the
// column before it indexes tokens.
#include "mlt_common.h"
#include "mlt_sample.h"

namespace mlt {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / 64;
constexpr int kSampleBins = 2048;  // 11-bit digits (the last digit has 10: its upper bins stay empty)
static_assert(kSampleBins == 2 * kSampleThreads, "the bin scan gives each thread two adjacent bins");

typedef unsigned long long u64;

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
  return ((u64)(uint32_t)__shfl_xor((int)(v >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int o) {
  return ((u64)(uint32_t)__shfl_up((int)(v >> 32), o, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, o, 64);
}

// maximum over the block, in every thread; red holds kSampleWaves words
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = shfl_xor_u64(v, o);
    v = t > v ? t : v;
  }
  __syncthreads();  // red may still be read from an earlier call
  if (lane == 0) red[w] = v;
  __syncthreads();
  u64 r = red[0];
#pragma unroll
  for (int i = 1; i < kSampleWaves; ++i) r = red[i] > r ? red[i] : r;
  return r;
}

// exclusive prefix of v over the threads in thread order, the grand total in `total`; red holds kSampleWaves words
__device__ __forceinline__ u64 block_scan_u64(u64 v, u64* red, u64& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = shfl_up_u64(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) red[w] = inc;
  __syncthreads();
  u64 before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < kSampleWaves; ++i) {
    const u64 t = red[i];
    before += i < w ? t : 0;
    all += t;
  }
  total = all;
  return before + inc - v;
}

// the argmax pass: (m, a) of step 1 in every thread
__device__ __forceinline__ void row_argmax(const float* __restrict__ row, int V, u64* red, float& m, int& a) {
  const int nvec = (V + 3) >> 2;
  u64 best = 0;  // below every packed value: a key is >= key(-inf) > 0
  for (int v = threadIdx.x; v < nvec; v += kSampleThreads) {
    const float4 q = *reinterpret_cast<const float4*>(row + 4 * (int64_t)v);
    const float r[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = 4 * v + c;
      if (i < V) {
        const u64 pk = ((u64)sample_key(sample_logit(r[c], true)) << 32) | (uint32_t)~(uint32_t)i;
        best = pk > best ? pk : best;
      }
    }
  }
  best = block_max_u64(best, red);
  const uint32_t key = (uint32_t)(best >> 32);
  m = __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
  a = (int)~(uint32_t)best;
}

// One radix-select pass. Adds, for every element whose key matches `prefix` above bit `shift + bits` and is
// >= key_floor, its count (WEIGHTED false) or weight to hist[digit]; then finds, from the highest bin down, the bin
// where the running sum reaches `target` (WEIGHTED first pass: target = (p16 * total + 65535) >> 16 once the total
// is known). Returns the digit; `target` becomes the remainder inside that bin. `total` is the sum of all bins.
template <bool WEIGHTED>
__device__ __forceinline__ uint32_t select_pass(const float* __restrict__ row, int V, float m, float s,
                                                uint32_t key_floor, uint32_t prefix, int shift, int bits, u64* hist,
                                                u64* red, uint32_t* sel, u64& target, int p16_first, u64& total) {
  const int tid = threadIdx.x;
  hist[2 * tid] = 0;
  hist[2 * tid + 1] = 0;
  __syncthreads();
  if (tid == 0) {  // target == 0 (a row of NaNs has no weight) selects no bin: digit 0, remainder 0
    sel[0] = 0;
    reinterpret_cast<u64*>(sel + 2)[0] = 0;
  }
  const int nvec = (V + 3) >> 2;
  const uint32_t dmask = (1u << bits) - 1u;
  const int hi_shift = shift + bits;  // 32 on the first pass: nothing above to match
  uint32_t run_d = 0;
  u64 run = 0;
  for (int v = tid; v < nvec; v += kSampleThreads) {
    const float4 q = *reinterpret_cast<const float4*>(row + 4 * (int64_t)v);
    const float r[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool in = 4 * v + c < V;
      const float z = sample_logit(r[c], in);
      const uint32_t key = sample_key(z);
      const bool match = in && key >= key_floor && (hi_shift >= 32 || (key >> hi_shift) == prefix);
      if (match) {
        const u64 add = WEIGHTED ? (u64)sample_weight(r[c], in, z, m, s) : 1ull;
        const uint32_t d = (key >> shift) & dmask;
        if (d != run_d) {
          if (run) atomicAdd(&hist[run_d], run);
          run_d = d;
          run = 0;
        }
        run += add;
      }
    }
  }
  if (run) atomicAdd(&hist[run_d], run);
  __syncthreads();
  // thread t scans bins 2047 - 2t and 2046 - 2t: thread order = descending bin order
  const uint32_t bh = kSampleBins - 1 - 2 * tid, bl = bh - 1;
  const u64 vh = hist[bh], vl = hist[bl];
  const u64 above = block_scan_u64(vh + vl, red, total);
  if (p16_first) target = ((u64)p16_first * total + 65535ull) >> 16;
  if (target > above && target <= above + vh) {
    sel[0] = bh;
    reinterpret_cast<u64*>(sel + 2)[0] = target - above;
  } else if (target > above + vh && target <= above + vh + vl) {
    sel[0] = bl;
    reinterpret_cast<u64*>(sel + 2)[0] = target - above - vh;
  }
  __syncthreads();
  target = reinterpret_cast<const u64*>(sel + 2)[0];
  return sel[0];
}

// the 3 passes: the key whose value is the threshold (T_k for counts, T_p for weights)
template <bool WEIGHTED>
__device__ __forceinline__ uint32_t select_key(const float* __restrict__ row, int V, float m, float s,
                                               uint32_t key_floor, u64 target, int p16, u64* hist, u64* red,
                                               uint32_t* sel) {
  u64 total;
  const uint32_t d0 = select_pass<WEIGHTED>(row, V, m, s, key_floor, 0u, 21, 11, hist, red, sel, target, p16, total);
  const uint32_t d1 = select_pass<WEIGHTED>(row, V, m, s, key_floor, d0, 10, 11, hist, red, sel, target, 0, total);
  const uint32_t p1 = (d0 << 11) | d1;
  const uint32_t d2 = select_pass<WEIGHTED>(row, V, m, s, key_floor, p1, 0, 10, hist, red, sel, target, 0, total);
  return (p1 << 10) | d2;
}

__global__ __launch_bounds__(kSampleThreads) void sample_step_kernel(
    const float* __restrict__ logits, int64_t ldz, int V, const SampleParams* __restrict__ params,
    int* __restrict__ draws, const int* __restrict__ seq_ids, int* __restrict__ finished, int64_t* __restrict__ lengths,
    int64_t* __restrict__ tokens, int T, int64_t* __restrict__ next_ids, int* __restrict__ n_kept) {
  __shared__ u64 s_hist[kSampleBins];
  __shared__ u64 s_red[kSampleWaves];
  __shared__ uint32_t s_sel[4];  // [0] the selected digit / the drawn token, [2..3] a u64 remainder
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (int64_t)b * ldz;
  const SampleParams P = *params;
  const int draw = draws[b];  // read by every thread before thread 0 rewrites it (barriers in between)
  const float s = P.inv_t_log2e;

  float m;
  int a;
  row_argmax(row, V, s_red, m, a);
  int token = a, kept = 1;
  if (s != 0.f) {
    uint32_t key_floor = 0;  // key of the threshold: S = {i : key_i >= key_floor}
    if (P.top_k > 0 && P.top_k < V)
      key_floor = select_key<false>(row, V, m, s, 0u, (u64)P.top_k, 0, s_hist, s_red, s_sel);
    if (P.p16 < 65536) {  // W_K >= 2^24 unless every column is NaN: then need == 0 and the key comes back 0
      const uint32_t kp = select_key<true>(row, V, m, s, key_floor, 0ull, P.p16, s_hist, s_red, s_sel);
      key_floor = kp > key_floor ? kp : key_floor;
    }
    // the draw: thread t owns vectors [t * C, (t + 1) * C)
    const int nvec = (V + 3) >> 2;
    const int C = (nvec + kSampleThreads - 1) / kSampleThreads;
    const int v0 = min(tid * C, nvec), v1 = min(v0 + C, nvec);
    u64 mine = 0;
    uint32_t cnt = 0;
    for (int v = v0; v < v1; ++v) {
      const float4 q = *reinterpret_cast<const float4*>(row + 4 * (int64_t)v);
      const float r[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool in = 4 * v + c < V;
        const float z = sample_logit(r[c], in);
        if (in && sample_key(z) >= key_floor) {
          mine += sample_weight(r[c], in, z, m, s);
          ++cnt;
        }
      }
    }
    u64 WS, nS;
    const u64 before = block_scan_u64(mine, s_red, WS);
    block_scan_u64((u64)cnt, s_red, nS);
    kept = (int)nS;
    const Philox4 x = philox4x32_10((uint32_t)draw, (uint32_t)seq_ids[b], kSampleSite, 0u, P.seed_lo, P.seed_hi);
    // r = (u24 * W_S) >> 24 without a product past 64 bits: W_S = H * 2^24 + L gives u24 * H + ((u24 * L) >> 24)
    const u64 u24 = x.x >> 8;
    const u64 r = u24 * (WS >> 24) + ((u24 * (WS & 0xFFFFFFull)) >> 24);  // r < W_S
    if (tid == 0) s_sel[0] = (uint32_t)a;  // W_S == 0
    __syncthreads();
    if (mine > 0 && r >= before && r < before + mine) {  // exactly one thread when W_S > 0
      u64 cum = before;
      int tok = -1;
      for (int v = v0; v < v1 && tok < 0; ++v) {
        const float4 q = *reinterpret_cast<const float4*>(row + 4 * (int64_t)v);
        const float rr[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool in = 4 * v + c < V;
          const float z = sample_logit(rr[c], in);
          if (tok < 0 && in && sample_key(z) >= key_floor) {
            cum += sample_weight(rr[c], in, z, m, s);
            if (cum > r) tok = 4 * v + c;
          }
        }
      }
      s_sel[0] = (uint32_t)tok;
    }
    __syncthreads();
    token = (int)s_sel[0];
  }

  if (tid == 0) {  // step 6
    MLT_DCHECK(draw >= 0 && draw < T);
    const int col = min(max(draw, 0), T - 1);
    int64_t out = token;
    if (finished[b]) {
      out = P.fill_id;
    } else {
      lengths[b] += 1;
      if (token == P.eos_id) finished[b] = 1;
    }
    tokens[(int64_t)b * T + col] = out;
    next_ids[b] = out;
    draws[b] = draw + 1;
    n_kept[b] = kept;
  }
}

__global__ __launch_bounds__(kSampleThreads) void sample_weights_kernel(const float* __restrict__ logits, int64_t ldz,
                                                                        int V, float s, int* __restrict__ w,
                                                                        int* __restrict__ argmax) {
  __shared__ u64 s_red[kSampleWaves];
  const int b = blockIdx.x;
  const float* row = logits + (int64_t)b * ldz;
  float m;
  int a;
  row_argmax(row, V, s_red, m, a);
  if (threadIdx.x == 0) argmax[b] = a;
  for (int i = threadIdx.x; i < V; i += kSampleThreads) {
    const float raw = row[i];
    w[(int64_t)b * V + i] = (int)sample_weight(raw, true, sample_logit(raw, true), m, s);
  }
}

void launch_sample_step(const float* logits, int64_t ldz, int V, int B, const SampleParams* params, int* draws,
                        const int* seq_ids, int* finished, int64_t* lengths, int64_t* tokens, int T, int64_t* next_ids,
                        int* n_kept, hipStream_t st) {
  sample_step_kernel<<<dim3(B), dim3(kSampleThreads), 0, st>>>(logits, ldz, V, params, draws, seq_ids, finished,
                                                               lengths, tokens, T, next_ids, n_kept);
}

void launch_sample_weights(const float* logits, int64_t ldz, int V, int B, float inv_t_log2e, int* w, int* argmax,
                           hipStream_t st) {
  sample_weights_kernel<<<dim3(B), dim3(kSampleThreads), 0, st>>>(logits, ldz, V, inv_t_log2e, w, argmax);
}

}  // namespace mlt
