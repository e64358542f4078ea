// SwiGLU activation of the gated feed-forward and its backward, for gfx950 (the streaming kernels of training and
// prefill; the decode step's fused form is gemm_skinny_glu_kernel in gemm_skinny.hip).
//
// H1 [rows][ldh >= 2F] bf16 is FFN1's output: columns [0, F) the gate g, [F, 2F) the up-projection u. F % 8 == 0,
// row strides multiples of 8, bases 16-byte aligned (bindings.cpp). The arithmetic is mlt_swiglu.h, nothing else.
//
// swiglu_fwd: A [rows][F] = bf16((g * s) * u). A lane owns one 16-byte chunk (8 columns) of g and the matching
// chunk of u: two 16-byte loads, one 16-byte store, 6 bytes per output element. Flat grid over rows x F / 8 lanes
// (64-bit index), no LDS, no atomics; rows past `rows` and the columns of a stride gap are never touched.
//
// swiglu_bwd: dH1 [rows][2F] = dg | du from dA [rows][F] and H1, and part [row blocks][2F] fp32: the column sums
// of the ROUNDED dH1 over each block of 64 rows, which reduce_col_partials (bindings.cpp) turns into FFN1's bias
// gradient. 10 bytes per element of F (da, g, u in; dg, du out).
//   * A 256-thread block owns 64 rows x 512 gate columns and their 512 up columns; block index = row block *
//     column blocks + column block (flat: no 65,535 limit on the row blocks).
//   * Wave w walks rows 16 w .. 16 w + 15 in order; a lane owns one 16-byte chunk per row (64 lanes x 8 = 512
//     columns, a row's loads and stores are whole 1 KB runs) and keeps 16 fp32 column sums in registers, 8 of dg
//     and 8 of du, added in row order.
//   * The four waves' sums meet in LDS (16 KB) and are added in wave order 0, 1, 2, 3; thread t writes columns
//     t, t + 256, .. of the block's 1,024. One fixed order, no atomics: the same bits every run.
//   * The rows of the last block past `rows` end the wave's walk (wave-uniform): neither loaded nor stored, their
//     sums stay exact zeros. Chunks at or past F (last column block) do nothing and write no partial.
// Why this split and not one row per block: the column sums need many rows per lane to amortise the LDS pass
// (16 rows here: 1/16 of an LDS write per element), and 512 columns keep a wave's accesses contiguous.
//
// Registers (-Rpass-analysis=kernel-resource-usage), scratch 0:
//   swiglu_fwd_kernel: 26 VGPRs,  0 B LDS, 8 waves per SIMD
//   swiglu_bwd_kernel: 62 VGPRs, 16 KB LDS, 8 waves per SIMD
// Measured at 262,144 rows (profiles/swiglu/README.md): forward 92.7 % (F = 2048) / 90.1 % (3072) of the 6.3 TB/s
// streaming figure, backward 78.7 % / 78.6 % with its partial reduction.
// Built without the packed fp32 forms (build.py FILE_FLAGS): plain v_mul_f32 / v_add_f32, as gqa.hip.
#include "mlt_common.h"
#include "mlt_kernels.h"
#include "mlt_swiglu.h"

namespace mlt {

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const uint16_t* __restrict__ H1, int64_t ldh,
                                                         uint16_t* __restrict__ A, int64_t lda, int64_t rows, int F) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = F >> 3;
  const int64_t row = i / per_row;
  if (row >= rows) return;
  const int c = (int)(i - row * per_row) * 8;
  const uint16_t* hp = H1 + row * ldh + c;
  const uint4 gr = *reinterpret_cast<const uint4*>(hp);
  const uint4 ur = *reinterpret_cast<const uint4*>(hp + F);
  float g[8], u[8];
  glu_unpack(gr, g);
  glu_unpack(ur, u);
  uint16_t o[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] = glu_bf16(swiglu_act(g[d], u[d]));
  *reinterpret_cast<uint4*>(A + row * lda + c) = glu_pack(o);
}

constexpr int kGluRows = 64;   // rows of a swiglu_bwd block (kGluRows / 4 per wave)
constexpr int kGluCols = 512;  // gate columns of a swiglu_bwd block: 64 lanes x 8

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const uint16_t* __restrict__ DA, int64_t ldda,
                                                         const uint16_t* __restrict__ H1, int64_t ldh,
                                                         uint16_t* __restrict__ DH1, int64_t lddh,
                                                         float* __restrict__ part, int64_t rows, int F, int ncb) {
  __shared__ float red[4][2 * kGluCols];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t rb = blockIdx.x / ncb;
  const int cb = (int)(blockIdx.x - rb * ncb);
  const int c = cb * kGluCols + lane * 8;
  const bool live = c < F;
  const int64_t row0 = rb * kGluRows + w * (kGluRows / 4);
  const int64_t left = rows - row0;
  const int nr = left >= kGluRows / 4 ? kGluRows / 4 : (left > 0 ? (int)left : 0);  // wave-uniform

  float sg[8], su[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) sg[d] = su[d] = 0.f;
  if (live) {
#pragma unroll 4
    for (int i = 0; i < nr; ++i) {
      const int64_t row = row0 + i;
      const uint16_t* hp = H1 + row * ldh + c;
      const uint4 ar = *reinterpret_cast<const uint4*>(DA + row * ldda + c);
      const uint4 gr = *reinterpret_cast<const uint4*>(hp);
      const uint4 ur = *reinterpret_cast<const uint4*>(hp + F);
      float da[8], g[8], u[8];
      glu_unpack(ar, da);
      glu_unpack(gr, g);
      glu_unpack(ur, u);
      uint16_t og[8], ou[8];
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        float dg, du;
        swiglu_grad(da[d], g[d], u[d], dg, du);
        og[d] = glu_bf16(dg);
        ou[d] = glu_bf16(du);
        sg[d] += bf16_to_f32(og[d]);  // the bias gradient sums what is stored
        su[d] += bf16_to_f32(ou[d]);
      }
      uint16_t* dp = DH1 + row * lddh + c;
      *reinterpret_cast<uint4*>(dp) = glu_pack(og);
      *reinterpret_cast<uint4*>(dp + F) = glu_pack(ou);
    }
  }
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    red[w][lane * 8 + d] = sg[d];
    red[w][kGluCols + lane * 8 + d] = su[d];
  }
  __syncthreads();
  float* prow = part + rb * 2 * (int64_t)F;
#pragma unroll
  for (int k = 0; k < 2 * kGluCols / 256; ++k) {
    const int j = threadIdx.x + 256 * k;          // 0 .. 1023: dg columns, then du columns
    const int which = j >= kGluCols ? 1 : 0;
    const int col = cb * kGluCols + (j - which * kGluCols);
    if (col < F) prow[which * F + col] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

int64_t swiglu_bwd_row_blocks(int64_t rows) { return (rows + kGluRows - 1) / kGluRows; }

void launch_swiglu_fwd(const uint16_t* H1, int64_t ldh, uint16_t* A, int64_t lda, int64_t rows, int F,
                       hipStream_t st) {
  if (rows <= 0) return;
  const int64_t lanes = rows * (F / 8);
  hipLaunchKernelGGL(swiglu_fwd_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, H1, ldh, A, lda, rows,
                     F);
}

void launch_swiglu_bwd(const uint16_t* DA, int64_t ldda, const uint16_t* H1, int64_t ldh, uint16_t* DH1, int64_t lddh,
                       float* part, int64_t rows, int F, hipStream_t st) {
  if (rows <= 0) return;
  const int ncb = (F + kGluCols - 1) / kGluCols;
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3((unsigned)(swiglu_bwd_row_blocks(rows) * ncb)), dim3(256), 0, st, DA, ldda,
                     H1, ldh, DH1, lddh, part, rows, F, ncb);
}

}  // namespace mlt
