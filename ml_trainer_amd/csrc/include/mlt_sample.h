// On-device token sampling (sample.hip): greedy / temperature / top-k / top-p with the token and EOS
// bookkeeping of generate(), one launch per step, the result defined in integers.
//
// THE DEFINITION, shared by the kernel, ops.decode.sample_step_reference and tests/sample_ref.py. Per row b
// of logits z [B][ldz] (V valid columns; s = inv_t_log2e = log2(e) / temperature as fp32):
//  1. Argmax. A NaN logit counts as -inf; columns >= V do not exist. -0 counts as +0. m = the maximum, a = the
//     smallest index that attains it (0 when V columns are all NaN; +inf is a legitimate maximum). Greedy
//     (s == 0): the token is a and n_kept = 1.
//  2. Weights. w_i = 2^24 where z_i == m; otherwise e_i = min(exp2f(s * (z_i - m)), 1) with one fp32 subtract
//     and one fp32 multiply (never contracted) and w_i = (uint32) floorf(e_i * 2^24). NaN columns weigh 0.
//     sample_weight() below is the only place this is written. From here on everything is integer arithmetic.
//  3. Top-k. T_k = the k-th largest logit counted with multiplicity; K = {i : z_i >= T_k}, ties at the threshold
//     all kept. k == 0 or k >= V: K = everything.
//  4. Top-p inside K. W_K = sum_{i in K} w_i (uint64), need = (p16 * W_K + 65535) >> 16, T_p = the largest logit
//     value t with sum_{i in K, z_i >= t} w_i >= need, S = {i in K : z_i >= T_p}. p16 == 65536: S = K. The
//     probability applied is p16 / 65536, p16 = round(top_p * 65536).
//  5. Draw. x = word 0 of philox4x32_10(counter = (draws[b], seq_ids[b], 0x53414D50, 0), key = (seed_lo, seed_hi)),
//     u24 = x >> 8, W_S = sum_{i in S} w_i, r = (u24 * W_S) >> 24; the token is the smallest i in S with
//     sum_{j in S, j <= i} w_j > r: an inverse CDF in vocabulary-index order, no sort. (W_S == 0 only when every
//     column is NaN: the token is a.) n_kept = |S|.
//  6. Bookkeeping. finished[b]: the token becomes fill_id. Otherwise lengths[b] += 1 and finished[b] |= (token ==
//     eos_id). Then tokens[b][draws[b]] = token, next_ids[b] = token, draws[b] += 1.
// Integer sums are exact and commutative, so the result depends neither on thread order nor on the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlt_philox.h"

namespace mlt {

constexpr uint32_t kSampleSite = 0x53414D50u;  // "SAMP": word 2 of the Philox counter
constexpr uint32_t kSampleOne = 1u << 24;      // the weight of the maximum

// the device parameter block (8 x 4 bytes; ops.decode.SamplerState writes it as int32 [8])
struct SampleParams {
  float inv_t_log2e;  // log2(e) / temperature; 0 = greedy
  int top_k;          // 0 = off
  int p16;            // round(top_p * 65536) in [1, 65536]; 65536 = off
  uint32_t seed_lo, seed_hi;
  int eos_id;         // -1 = none
  int fill_id;
  int reserved;
};
static_assert(sizeof(SampleParams) == 32, "SampleParams is int32 [8] on the Python side");

#if defined(__HIP__)
// the logit as the definition sees it: NaN and columns past V are -inf, -0 is +0
__device__ __forceinline__ float sample_logit(float z, bool in_range) {
  return (in_range && z == z) ? (z == 0.f ? 0.f : z) : -INFINITY;
}

// order-preserving integer key of an fp32 that is not NaN: a < b <=> key(a) < key(b)
__device__ __forceinline__ uint32_t sample_key(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// step 2. `raw` is the logit as loaded, `z` = sample_logit(raw, in_range), m the row maximum of z.
__device__ __forceinline__ uint32_t sample_weight(float raw, bool in_range, float z, float m, float s) {
  if (!(in_range && raw == raw)) return 0u;
  if (z == m) return kSampleOne;
  const float e = fminf(exp2f(__fmul_rn(s, __fsub_rn(z, m))), 1.f);
  return (uint32_t)floorf(e * 16777216.f);
}
#endif

// sample_step: one workgroup per row. logits [B][ldz] fp32 (ldz % 4 == 0, 16-byte aligned, columns up to
// round_up(V, 4) readable), the parameter block and the per-row state on the device: draws / seq_ids / finished /
// n_kept int32 [B], lengths / next_ids int64 [B], tokens int64 [B][T]. Nothing is allocated or synchronised.
void launch_sample_step(const float* logits, int64_t ldz, int V, int B, const SampleParams* params, int* draws,
                        const int* seq_ids, int* finished, int64_t* lengths, int64_t* tokens, int T, int64_t* next_ids,
                        int* n_kept, hipStream_t st);
// test support: w int32 [B][V] (the weights of step 2, in [0, 2^24]) and argmax int32 [B]
void launch_sample_weights(const float* logits, int64_t ldz, int V, int B, float inv_t_log2e, int* w, int* argmax,
                           hipStream_t st);

}  // namespace mlt
