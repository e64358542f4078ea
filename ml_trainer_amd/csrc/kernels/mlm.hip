// Masked-LM head kernels for gfx950: the vocabulary-wide softmax cross-entropy with the gradient
// written in place, and the selection / gather / scatter of the masked positions.
//
// vocab_ce: one 512-thread workgroup per row of bf16 logits Z[R, ldz] (ldz % 8 == 0, so every row is
// 16-byte aligned; V <= ldz valid columns, the rest padding). Thread t owns the 16-byte chunks
// t, t + 512, ... of its row:
//   pass 1  loads each chunk once (global_load_dwordx4), keeps it in LDS when the row fits
//           (ldz <= kVocabCeResidentCols) and folds the valid elements into a per-thread online
//           (max, sum of exp, first arg-max) in fp32;
//   reduce  block max (exact), first arg-max as a block min over the indices that hold the max, then
//           the rescaled sums -- wave shuffles, then LDS partials added in wave order. No atomics:
//           bitwise reproducible run to run;
//   pass 2  (write_grad) re-reads the thread's OWN chunks from LDS (no barrier needed for them) -- or
//           from global memory for rows wider than the resident limit -- and stores
//           bf16(exp(z - max) / sum - [c == label]) with 16-byte stores; padding columns get 0.
// Padding columns never enter the max, the sum or the arg-max (they may hold NaN). An ignored row
// (label == ignore_index or outside [0, V)) skips the statistics: its outputs are 0 and, with
// write_grad, the whole row is written as zeros. The probabilities use exp(z - max) / sum rather
// than exp(z - lse): z and max are bf16 values, so the subtraction is exact.
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

constexpr int kVceThreads = 512;
constexpr int kVceWaves = kVceThreads / 64;

int vocab_ce_resident_cols() { return kVocabCeResidentCols; }

__device__ __forceinline__ float vce_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < kVceWaves; ++i) r = fmaxf(r, red[i]);
  return r;
}

__device__ __forceinline__ float vce_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < kVceWaves; ++i) r += red[i];  // wave order: deterministic
  return r;
}

__device__ __forceinline__ int vce_block_min(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int i = 1; i < kVceWaves; ++i) r = min(r, red[i]);
  return r;
}

__device__ __forceinline__ void vce_unpack(const uint4& q, float (&x)[8]) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = __uint_as_float(w[j] << 16);
    x[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

template <bool RESIDENT>
__global__ __launch_bounds__(kVceThreads) void vocab_ce_kernel(uint16_t* __restrict__ Z, int64_t ldz, int V,
                                                               const int64_t* __restrict__ labels,
                                                               float* __restrict__ row_loss,
                                                               float* __restrict__ row_lse,
                                                               float* __restrict__ row_hit, int64_t ignore_index,
                                                               int write_grad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vce_smem[];
  __shared__ float redf[kVceWaves];
  __shared__ int redi[kVceWaves];
  uint4* row_lds = reinterpret_cast<uint4*>(vce_smem);
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  uint4* zrow = reinterpret_cast<uint4*>(Z + row * ldz);
  const int nchunks = (int)(ldz >> 3);
  const int vchunks = (V + 7) >> 3;  // chunks that hold at least one valid column
  const int64_t t64 = labels[row];
  const bool ok = t64 != ignore_index && t64 >= 0 && t64 < (int64_t)V;  // block-uniform
  if (!ok) {
    if (write_grad)
      for (int i = tid; i < nchunks; i += kVceThreads) zrow[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) {
      row_loss[row] = 0.f;
      row_lse[row] = 0.f;
      row_hit[row] = 0.f;
    }
    return;
  }
  const int t = (int)t64;

  // pass 1: per-thread online max / sum / first arg-max over the thread's chunks
  float m = -INFINITY, s = 0.f, zt = 0.f;
  int bi = 0x7fffffff;
  // (four 16-byte loads in flight per lane before the first is folded: one load per trip leaves the
  // memory system a single request per lane to hide its latency with)
  for (int i0 = tid; i0 < vchunks; i0 += 4 * kVceThreads) {
    uint4 q4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * kVceThreads;
      q4[u] = i < vchunks ? zrow[i] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * kVceThreads;
      if (i >= vchunks) break;
      if (RESIDENT) row_lds[i] = q4[u];
      float x[8];
      vce_unpack(q4[u], x);
      const int c0 = i << 3;
      float cm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (c0 + j >= V) x[j] = -INFINITY;  // padding: never read into the statistics
        cm = fmaxf(cm, x[j]);
        if (c0 + j == t) zt = x[j];
      }
      if (cm > m) {  // strictly greater: columns rise within a thread, so the first index is kept
#pragma unroll
        for (int j = 7; j >= 0; --j)
          if (x[j] == cm) bi = c0 + j;
        s *= __expf(m - cm);
        m = cm;
      }
      if (m > -INFINITY) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += __expf(x[j] - m);  // exp(-inf) = 0 at the padding
        s += a;
      }
    }
  }
  const float M = vce_block_max(m, redf);
  const int arg = vce_block_min(m == M ? bi : 0x7fffffff, redi);
  const float S = vce_block_sum(m > -INFINITY ? s * __expf(m - M) : 0.f, redf);
  const float ZT = vce_block_sum(zt, redf);  // one thread holds the label's logit, the rest 0
  const float logS = logf(S);
  if (tid == 0) {
    row_loss[row] = (M - ZT) + logS;
    row_lse[row] = M + logS;
    row_hit[row] = arg == t ? 1.f : 0.f;
  }
  if (!write_grad) return;

  // pass 2: gradient in place (the thread's own chunks: its LDS writes need no barrier)
  const float inv = 1.f / S;
  for (int i = tid; i < nchunks; i += kVceThreads) {
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (i < vchunks) {
      const uint4 q = RESIDENT ? row_lds[i] : zrow[i];
      float x[8];
      vce_unpack(q, x);
      const int c0 = i << 3;
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __expf(x[j] - M) * inv - (c0 + j == t ? 1.f : 0.f);
        h[j] = c0 + j < V ? (uint32_t)f32_to_bf16(p) : 0u;
      }
      o = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
    zrow[i] = o;
  }
}

void launch_vocab_ce(uint16_t* Z, int64_t R, int64_t ldz, int V, const int64_t* labels, float* row_loss,
                     float* row_lse, float* row_hit, int64_t ignore_index, bool write_grad, hipStream_t st) {
  if (R <= 0) return;
  const dim3 grid((unsigned)R), block(kVceThreads);
  if (ldz <= kVocabCeResidentCols)
    hipLaunchKernelGGL(vocab_ce_kernel<true>, grid, block, (size_t)ldz * 2, st, Z, ldz, V, labels, row_loss, row_lse,
                       row_hit, ignore_index, write_grad ? 1 : 0);
  else
    hipLaunchKernelGGL(vocab_ce_kernel<false>, grid, block, 0, st, Z, ldz, V, labels, row_loss, row_lse, row_hit,
                       ignore_index, write_grad ? 1 : 0);
}

// ---------------------------------------------------------------------------
// mlm_select: one wave per sequence compacts the target positions (label != ignore_index) of
// labels[B, S] in order by ballot prefix into P slots. slot_row = base_b + s (base_b = b * S, or
// cu_seqlens[b] for packed batches), slot_label = the label; empty slots hold -1 / ignore_index.
// Targets past the P-th, or at s >= len_b (lens or cu_seqlens given), are dropped and counted in
// seq_overflow[b] (one writer per sequence); overflow_sum_kernel adds those up in order. Waves past
// the B sequences fill the tail slots [B * P, R).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mlm_select_kernel(const int64_t* __restrict__ labels, int B, int S, int P,
                                                         int64_t R, const int* __restrict__ lens,
                                                         const int* __restrict__ cu, int64_t ignore_index,
                                                         int* __restrict__ slot_row,
                                                         int64_t* __restrict__ slot_label,
                                                         int* __restrict__ seq_overflow) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= B) {  // tail slots
    const int64_t i = (int64_t)B * P + (w - B) * 64 + lane;
    if (i < R) {
      slot_row[i] = -1;
      slot_label[i] = ignore_index;
    }
    return;
  }
  const int b = (int)w;
  int len = S, base = b * S;
  if (cu != nullptr) {
    base = cu[b];
    len = cu[b + 1] - base;
  } else if (lens != nullptr) {
    len = lens[b];
  }
  len = min(len, S);
  int count = 0, dropped = 0;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    const int64_t l = s < S ? labels[(int64_t)b * S + s] : ignore_index;
    const bool target = l != ignore_index;
    const bool valid = target && s < len;
    const unsigned long long mask = __ballot(valid);
    const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (valid && slot < P) {
      slot_row[(int64_t)b * P + slot] = base + s;
      slot_label[(int64_t)b * P + slot] = l;
    }
    const unsigned long long lost = __ballot(target && (!valid || slot >= P));
    dropped += __popcll(lost);
    count += __popcll(mask);
  }
  for (int i = min(count, P) + lane; i < P; i += 64) {
    slot_row[(int64_t)b * P + i] = -1;
    slot_label[(int64_t)b * P + i] = ignore_index;
  }
  if (lane == 0) seq_overflow[b] = dropped;
}

__global__ __launch_bounds__(64) void mlm_overflow_sum_kernel(const int* __restrict__ seq_overflow, int B,
                                                              int* __restrict__ overflow) {
  int s = 0;
  for (int i = threadIdx.x; i < B; i += 64) s += seq_overflow[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) overflow[0] = s;
}

void launch_mlm_select(const int64_t* labels, int B, int S, int P, int64_t R, const int* lens, const int* cu,
                       int64_t ignore_index, int* slot_row, int64_t* slot_label, int* seq_overflow, int* overflow,
                       hipStream_t st) {
  const int64_t tail = R - (int64_t)B * P;
  const int64_t waves = B + (tail > 0 ? (tail + 63) / 64 : 0);
  if (waves > 0)
    hipLaunchKernelGGL(mlm_select_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, labels, B, S, P, R,
                       lens, cu, ignore_index, slot_row, slot_label, seq_overflow);
  hipLaunchKernelGGL(mlm_overflow_sum_kernel, dim3(1), dim3(64), 0, st, seq_overflow, B, overflow);
}

// ---------------------------------------------------------------------------
// gather_rows: out[r] = X[slot_row[r]] (16-byte chunks), zeros for empty slots (slot_row < 0; a row
// index >= N is treated as empty, never read). scatter_rows: dX = 0, then dX[slot_row[r]] = G[r] for
// the non-empty slots -- the slots of one batch never share a row, so plain stores.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ X, int64_t N, int hc,
                                                          const int* __restrict__ slot_row, int64_t R,
                                                          uint4* __restrict__ out) {
  const int64_t n = R * hc, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / hc;
    const int c = (int)(i - r * hc);
    const int src = slot_row[r];
    out[i] = (src >= 0 && src < N) ? X[(int64_t)src * hc + c] : make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint4* __restrict__ G, int64_t R, int hc,
                                                           const int* __restrict__ slot_row, int64_t N,
                                                           uint4* __restrict__ dX) {
  const int64_t n = R * hc, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / hc;
    const int c = (int)(i - r * hc);
    const int dst = slot_row[r];
    if (dst >= 0 && dst < N) dX[(int64_t)dst * hc + c] = G[i];
  }
}

static unsigned rows_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

void launch_gather_rows(const uint16_t* X, int64_t N, int h, const int* slot_row, int64_t R, uint16_t* out,
                        hipStream_t st) {
  if (R <= 0 || h <= 0) return;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(rows_grid(R * (h / 8))), dim3(256), 0, st, (const uint4*)X, N, h / 8,
                     slot_row, R, (uint4*)out);
}

void launch_scatter_rows(const uint16_t* G, int64_t R, int h, const int* slot_row, int64_t N, uint16_t* dX,
                         hipStream_t st) {
  if (N <= 0 || h <= 0) return;
  hipMemsetAsync(dX, 0, (size_t)N * h * 2, st);
  if (R <= 0) return;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(rows_grid(R * (h / 8))), dim3(256), 0, st, (const uint4*)G, R, h / 8,
                     slot_row, N, (uint4*)dX);
}

}  // namespace mlt
