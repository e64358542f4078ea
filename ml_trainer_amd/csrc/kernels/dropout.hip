// Stand-alone dropout over a contiguous bf16 [rows, D] tensor for gfx950: the embedding site, the
// one dropout of the BERT path that no LayerNorm kernel streams on both sides. The mask is the
// Philox definition of mlt_philox.h (shared with the fused LayerNorm kernels and the torch oracle),
// recomputed from the flat element index, so the backward is this same kernel on dy.
#include "mlt_common.h"
#include "mlt_kernels.h"
#include "mlt_philox.h"

namespace mlt {

__device__ __forceinline__ uint32_t drop_pair(uint32_t u, uint32_t w0, uint32_t w1, uint32_t thr, float scale) {
  const uint32_t lo = w0 >= thr ? f32_to_bf16(bf16_to_f32((uint16_t)(u & 0xffffu)) * scale) : 0u;
  const uint32_t hi = w1 >= thr ? f32_to_bf16(bf16_to_f32((uint16_t)(u >> 16)) * scale) : 0u;
  return lo | (hi << 16);
}

// out = keep ? bf16(x * scale) : 0. One 16-byte access (8 elements, two Philox calls) per thread.
// x and out may be the same buffer (each thread reads its vector before it writes it).
__global__ __launch_bounds__(256) void dropout_kernel(const uint16_t* x, uint16_t* out, int64_t nvec, DropArgs dr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const uint4 u = reinterpret_cast<const uint4*>(x)[i];
  const Philox4 a = drop_words(2 * (uint64_t)i, dr);
  const Philox4 b = drop_words(2 * (uint64_t)i + 1, dr);
  uint4 o;
  o.x = drop_pair(u.x, a.x, a.y, dr.thr, dr.scale);
  o.y = drop_pair(u.y, a.z, a.w, dr.thr, dr.scale);
  o.z = drop_pair(u.z, b.x, b.y, dr.thr, dr.scale);
  o.w = drop_pair(u.w, b.z, b.w, dr.thr, dr.scale);
  reinterpret_cast<uint4*>(out)[i] = o;
}

void launch_dropout(const uint16_t* x, uint16_t* out, int64_t numel, DropArgs dr, hipStream_t st) {
  const int64_t nvec = numel / 8;
  if (nvec <= 0) return;
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, st, x, out, nvec, dr);
}

}  // namespace mlt
