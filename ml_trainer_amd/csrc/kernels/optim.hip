// Flat multi-tensor optimizers for gfx950.
//
// All parameters of a param-group live in ONE contiguous fp32 buffer (see
// ml_trainer_amd/utils/flat.py), so an optimizer step is a single launch that
// streams p/g/state with 16-byte (float4) accesses. lr and the step counter can
// be read from device memory so the launch is hipGraph-replayable while a LR
// scheduler keeps changing the value (the reference steps schedulers per batch /
// per epoch: src/trainer.py:189-190,198-199).
#include "mlt_common.h"
#include "mlt_kernels.h"
#include "mlt_optim.h"

namespace mlt {

__global__ __launch_bounds__(256) void flat_optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ s1, float* __restrict__ s2,
                                                         int64_t n4, OptHyper h, const float* __restrict__ lr_ptr,
                                                         const int64_t* __restrict__ lr_index_ptr,
                                                         const int64_t* __restrict__ step_ptr, float t_host,
                                                         uint16_t* __restrict__ shadow,
                                                         const float* __restrict__ coef_ptr,
                                                         const unsigned* __restrict__ skip) {
  // all-or-nothing data-parallel step: a collective that failed on this rank (sticky error word,
  // e.g. an xGMI peer timeout that left some slices unreduced) vetoes the whole update
  if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
  const float lr = lr_ptr ? lr_ptr[lr_index_ptr ? (*lr_index_ptr - 1) : 0] : h.lr;
  const float t = step_ptr ? (float)(*step_ptr) : t_host;
  if (coef_ptr) h.grad_scale *= *coef_ptr;  // e.g. clip-by-norm coefficient
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* a4 = reinterpret_cast<float4*>(s1);
  float4* b4 = reinterpret_cast<float4*>(s2);
  const bool has_s2 = (h.kind == OPT_ADAM || h.kind == OPT_ADAMW || h.kind == OPT_ADAMAX);
  const bool has_s1 = has_s2 || h.kind == OPT_ADAGRAD || (h.kind == OPT_SGD && h.momentum != 0.f);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = p4[i];
    const float4 gv = g4[i];
    float4 av = has_s1 ? a4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 bv = has_s2 ? b4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    opt_update(h, lr, t, pv.x, gv.x, av.x, bv.x);
    opt_update(h, lr, t, pv.y, gv.y, av.y, bv.y);
    opt_update(h, lr, t, pv.z, gv.z, av.z, bv.z);
    opt_update(h, lr, t, pv.w, gv.w, av.w, bv.w);
    p4[i] = pv;
    if (has_s1) a4[i] = av;
    if (has_s2) b4[i] = bv;
    if (shadow) {
      ushort4 sv;
      sv.x = f32_to_bf16(pv.x);
      sv.y = f32_to_bf16(pv.y);
      sv.z = f32_to_bf16(pv.z);
      sv.w = f32_to_bf16(pv.w);
      reinterpret_cast<ushort4*>(shadow)[i] = sv;
    }
  }
}

constexpr int kSqNormMaxBlocks = 512;

// sum of squares of a flat fp32 buffer, two fixed-order stages (bitwise reproducible, like the
// loss reductions in losses.hip): (1) each block writes its partial to part[blockIdx.x];
__global__ __launch_bounds__(256) void sq_norm_partial_kernel(const float* __restrict__ x, int64_t n4,
                                                              float* __restrict__ part) {
  __shared__ float red[4];
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// (2) one block sums the nb partials in index order -> out[0] (overwritten: no zeroing by the caller)
__global__ __launch_bounds__(256) void sq_norm_final_kernel(const float* __restrict__ part, int nb,
                                                            float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *out = acc;
}

// clip coefficient: coef = min(1, max_norm / (sqrt(sq) + 1e-6))  (torch.nn.utils.clip_grad_norm_)
__global__ void clip_coef_kernel(const float* sq, float max_norm, float* coef, float* total_norm) {
  const float n = sqrtf(*sq);
  *total_norm = n;
  *coef = fminf(1.f, max_norm / (n + 1e-6f));
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y,
                                                        int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    ushort4 o;
    o.x = f32_to_bf16(v.x);
    o.y = f32_to_bf16(v.y);
    o.z = f32_to_bf16(v.z);
    o.w = f32_to_bf16(v.w);
    reinterpret_cast<ushort4*>(y)[i] = o;
  }
}

static inline int grid_for(int64_t n4) {
  int64_t g = (n4 + 255) / 256;
  if (g > 2048) g = 2048;  // grid-stride the rest (cdna_hip_programming.md Guideline 11)
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------------------------
// Per-tensor updates on the flat buffer: a segment table cuts every tensor into chunks of at most
// kOptChunkElems elements (ops/optim.py builds it once; segments start at multiples of 16 elements,
// so a float4 never straddles two tensors and the gaps hold p = g = 0). One block takes one chunk at
// a time: 256 threads x kOptChunkIters float4s. A table entry that points outside the buffer is
// skipped, never followed.
//   chunks[c] = {tensor id, first float4, float4 count, 0}      tseg[t] = {first chunk, chunk count}
// ---------------------------------------------------------------------------------------------
constexpr int kOptChunkElems = 4096;
constexpr int kOptChunk4 = kOptChunkElems / 4;
constexpr int kOptChunkIters = kOptChunk4 / 256;
static_assert(kOptChunk4 % 256 == 0, "a chunk is a whole number of 256-thread float4 rows");

__device__ __forceinline__ bool seg_chunk(const int4* __restrict__ chunks, int c, int nt, int64_t n4, int& tid,
                                          int64_t& first, int& cnt) {
  const int4 ch = chunks[c];
  tid = ch.x;
  first = ch.y;
  cnt = ch.z;
  return tid >= 0 && tid < nt && first >= 0 && cnt >= 0 && cnt <= kOptChunk4 && first + cnt <= n4;
}

__device__ __forceinline__ bool step_vetoed(const unsigned* skip) {
  return skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
}

// AdamW with a weight decay per tensor: flat_optim_kernel's update (opt_update_k<OPT_ADAMW>, the same
// bits for a tensor as flat_optim with that tensor's decay), walked chunk by chunk. One launch.
__global__ __launch_bounds__(256) void flat_optim_seg_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2, int64_t n4,
    const int4* __restrict__ chunks, int nchunks, const float* __restrict__ wd, int nt, OptHyper h,
    const float* __restrict__ lr_ptr, const int64_t* __restrict__ lr_index_ptr,
    const int64_t* __restrict__ step_ptr, float t_host, uint16_t* __restrict__ shadow,
    const float* __restrict__ coef_ptr, const unsigned* __restrict__ skip) {
  if (step_vetoed(skip)) return;
  const float lr = lr_ptr ? lr_ptr[lr_index_ptr ? (*lr_index_ptr - 1) : 0] : h.lr;
  const float t = step_ptr ? (float)(*step_ptr) : t_host;
  if (coef_ptr) h.grad_scale *= *coef_ptr;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* a4 = reinterpret_cast<float4*>(s1);
  float4* b4 = reinterpret_cast<float4*>(s2);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int tid, cnt;
    int64_t first;
    if (!seg_chunk(chunks, c, nt, n4, tid, first, cnt)) continue;
    h.weight_decay = wd[tid];
#pragma unroll
    for (int k = 0; k < kOptChunkIters; ++k) {
      const int j = threadIdx.x + k * 256;
      if (j >= cnt) break;
      const int64_t i = first + j;
      float4 pv = p4[i];
      const float4 gv = g4[i];
      float4 av = a4[i];
      float4 bv = b4[i];
      opt_update_k<OPT_ADAMW>(h, lr, t, pv.x, gv.x, av.x, bv.x);
      opt_update_k<OPT_ADAMW>(h, lr, t, pv.y, gv.y, av.y, bv.y);
      opt_update_k<OPT_ADAMW>(h, lr, t, pv.z, gv.z, av.z, bv.z);
      opt_update_k<OPT_ADAMW>(h, lr, t, pv.w, gv.w, av.w, bv.w);
      p4[i] = pv;
      a4[i] = av;
      b4[i] = bv;
      if (shadow) {
        ushort4 sv;
        sv.x = f32_to_bf16(pv.x);
        sv.y = f32_to_bf16(pv.y);
        sv.z = f32_to_bf16(pv.z);
        sv.w = f32_to_bf16(pv.w);
        reinterpret_cast<ushort4*>(shadow)[i] = sv;
      }
    }
  }
}

// LAMB, three launches; the two kernel boundaries are the grid-wide dependencies (norms of a whole
// tensor before any of its weights move).
// Stage 1: moments (written), update direction u (not written: stage 2 forms it again from the same
// m, v, w, which costs the same 12 bytes per element as reading a stored u and needs no model-sized
// scratch), and the chunk's sums of w^2 and u^2 -> part[chunk]. The partial index is the chunk index:
// the sums do not depend on the grid.
__global__ __launch_bounds__(256) void lamb_stage1_kernel(
    const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    int64_t n4, const int4* __restrict__ chunks, int nchunks, const float* __restrict__ wd, int nt, OptHyper h,
    const int64_t* __restrict__ step_ptr, float t_host, const float* __restrict__ coef_ptr,
    const unsigned* __restrict__ skip, float2* __restrict__ part) {
  __shared__ float red[8];
  if (step_vetoed(skip)) return;
  const float t = step_ptr ? (float)(*step_ptr) : t_host;
  if (coef_ptr) h.grad_scale *= *coef_ptr;
  const float bc1 = opt_bias_correction(h.omb1, t);
  const float bc2 = opt_bias_correction(h.omb2, t);
  const float4* p4 = reinterpret_cast<const float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int tid, cnt;
    int64_t first;
    float w_sq = 0.f, u_sq = 0.f;
    if (seg_chunk(chunks, c, nt, n4, tid, first, cnt)) {
      const float wdt = wd[tid];
#pragma unroll
      for (int k = 0; k < kOptChunkIters; ++k) {
        const int j = threadIdx.x + k * 256;
        if (j >= cnt) break;
        const int64_t i = first + j;
        const float4 pv = p4[i];
        const float4 gv = g4[i];
        float4 mv = m4[i];
        float4 vv = v4[i];
        lamb_moments(h, gv.x, mv.x, vv.x);
        lamb_moments(h, gv.y, mv.y, vv.y);
        lamb_moments(h, gv.z, mv.z, vv.z);
        lamb_moments(h, gv.w, mv.w, vv.w);
        m4[i] = mv;
        v4[i] = vv;
        const float ux = lamb_direction(wdt, h.eps, bc1, bc2, pv.x, mv.x, vv.x);
        const float uy = lamb_direction(wdt, h.eps, bc1, bc2, pv.y, mv.y, vv.y);
        const float uz = lamb_direction(wdt, h.eps, bc1, bc2, pv.z, mv.z, vv.z);
        const float uw = lamb_direction(wdt, h.eps, bc1, bc2, pv.w, mv.w, vv.w);
        w_sq = fmaf(pv.x, pv.x, w_sq);
        w_sq = fmaf(pv.y, pv.y, w_sq);
        w_sq = fmaf(pv.z, pv.z, w_sq);
        w_sq = fmaf(pv.w, pv.w, w_sq);
        u_sq = fmaf(ux, ux, u_sq);
        u_sq = fmaf(uy, uy, u_sq);
        u_sq = fmaf(uz, uz, u_sq);
        u_sq = fmaf(uw, uw, u_sq);
      }
    }
    w_sq = block_sum(w_sq, red);
    u_sq = block_sum(u_sq, red + 4);
    if (threadIdx.x == 0) part[c] = make_float2(w_sq, u_sq);
  }
}

// Finalize: one block per tensor adds its chunks' partials in a fixed order (thread j takes chunks
// j, j + 256, ... in order, then the block tree) -> norms[t] = {sum w^2, sum u^2}, trust[t].
__global__ __launch_bounds__(256) void lamb_finalize_kernel(const float2* __restrict__ part,
                                                            const int2* __restrict__ tseg,
                                                            const int* __restrict__ adapt, int nt, int nchunks,
                                                            float2* __restrict__ norms, float* __restrict__ trust,
                                                            const unsigned* __restrict__ skip) {
  __shared__ float red[8];
  if (step_vetoed(skip)) return;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const int2 s = tseg[t];
    const bool ok = s.x >= 0 && s.y >= 0 && (int64_t)s.x + s.y <= nchunks;
    float w_sq = 0.f, u_sq = 0.f;
    if (ok) {
      for (int j = threadIdx.x; j < s.y; j += 256) {
        const float2 q = part[s.x + j];
        w_sq += q.x;
        u_sq += q.y;
      }
    }
    w_sq = block_sum(w_sq, red);
    u_sq = block_sum(u_sq, red + 4);
    if (threadIdx.x == 0) {
      norms[t] = make_float2(w_sq, u_sq);
      trust[t] = lamb_trust(adapt[t], w_sq, u_sq);
    }
  }
}

// Stage 2: u again from (p, m, v), w <- w - lr * trust[tensor] * u, and the bf16 shadow.
__global__ __launch_bounds__(256) void lamb_stage2_kernel(
    float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, int64_t n4,
    const int4* __restrict__ chunks, int nchunks, const float* __restrict__ wd, const float* __restrict__ trust,
    int nt, OptHyper h, const float* __restrict__ lr_ptr, const int64_t* __restrict__ lr_index_ptr,
    const int64_t* __restrict__ step_ptr, float t_host, uint16_t* __restrict__ shadow,
    const unsigned* __restrict__ skip) {
  if (step_vetoed(skip)) return;
  const float lr = lr_ptr ? lr_ptr[lr_index_ptr ? (*lr_index_ptr - 1) : 0] : h.lr;
  const float t = step_ptr ? (float)(*step_ptr) : t_host;
  const float bc1 = opt_bias_correction(h.omb1, t);
  const float bc2 = opt_bias_correction(h.omb2, t);
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* m4 = reinterpret_cast<const float4*>(m);
  const float4* v4 = reinterpret_cast<const float4*>(v);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int tid, cnt;
    int64_t first;
    if (!seg_chunk(chunks, c, nt, n4, tid, first, cnt)) continue;
    const float wdt = wd[tid];
    const float r = trust[tid];
#pragma unroll
    for (int k = 0; k < kOptChunkIters; ++k) {
      const int j = threadIdx.x + k * 256;
      if (j >= cnt) break;
      const int64_t i = first + j;
      float4 pv = p4[i];
      const float4 mv = m4[i];
      const float4 vv = v4[i];
      pv.x = lamb_apply(lr, r, lamb_direction(wdt, h.eps, bc1, bc2, pv.x, mv.x, vv.x), pv.x);
      pv.y = lamb_apply(lr, r, lamb_direction(wdt, h.eps, bc1, bc2, pv.y, mv.y, vv.y), pv.y);
      pv.z = lamb_apply(lr, r, lamb_direction(wdt, h.eps, bc1, bc2, pv.z, mv.z, vv.z), pv.z);
      pv.w = lamb_apply(lr, r, lamb_direction(wdt, h.eps, bc1, bc2, pv.w, mv.w, vv.w), pv.w);
      p4[i] = pv;
      if (shadow) {
        ushort4 sv;
        sv.x = f32_to_bf16(pv.x);
        sv.y = f32_to_bf16(pv.y);
        sv.z = f32_to_bf16(pv.z);
        sv.w = f32_to_bf16(pv.w);
        reinterpret_cast<ushort4*>(shadow)[i] = sv;
      }
    }
  }
}

// one block per chunk, capped as grid_for caps the element grids (max_blocks > 0: a lower cap)
static inline int chunk_grid(int nchunks, int max_blocks) {
  int g = nchunks < 2048 ? nchunks : 2048;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return g < 1 ? 1 : g;
}

int optim_chunk_elems() { return kOptChunkElems; }

void launch_flat_optim_seg(float* p, const float* g, float* s1, float* s2, int64_t n, const int* chunks,
                           int nchunks, const float* wd, int nt, const OptHyper& h, const float* lr_ptr,
                           const int64_t* lr_index_ptr, const int64_t* step_ptr, float t_host, uint16_t* shadow,
                           const float* coef_ptr, const unsigned* skip, int max_blocks, hipStream_t stream) {
  if (nchunks <= 0) return;
  hipLaunchKernelGGL(flat_optim_seg_kernel, dim3(chunk_grid(nchunks, max_blocks)), dim3(256), 0, stream, p, g, s1,
                     s2, n / 4, reinterpret_cast<const int4*>(chunks), nchunks, wd, nt, h, lr_ptr, lr_index_ptr,
                     step_ptr, t_host, shadow, coef_ptr, skip);
}

void launch_lamb_step(float* p, const float* g, float* m, float* v, int64_t n, const int* chunks, int nchunks,
                      const int* tseg, const float* wd, const int* adapt, int nt, float* part, float* norms,
                      float* trust, const OptHyper& h, const float* lr_ptr, const int64_t* lr_index_ptr,
                      const int64_t* step_ptr, float t_host, uint16_t* shadow, const float* coef_ptr,
                      const unsigned* skip, int max_blocks, int stages, hipStream_t stream) {
  if (nchunks <= 0 || nt <= 0) return;
  const int64_t n4 = n / 4;
  const int4* ch = reinterpret_cast<const int4*>(chunks);
  const int grid = chunk_grid(nchunks, max_blocks);
  if (stages & 1)
    hipLaunchKernelGGL(lamb_stage1_kernel, dim3(grid), dim3(256), 0, stream, p, g, m, v, n4, ch, nchunks, wd, nt, h,
                       step_ptr, t_host, coef_ptr, skip, reinterpret_cast<float2*>(part));
  if (stages & 2)
    hipLaunchKernelGGL(lamb_finalize_kernel, dim3(chunk_grid(nt, max_blocks)), dim3(256), 0, stream,
                       reinterpret_cast<const float2*>(part), reinterpret_cast<const int2*>(tseg), adapt, nt,
                       nchunks, reinterpret_cast<float2*>(norms), trust, skip);
  if (stages & 4)
    hipLaunchKernelGGL(lamb_stage2_kernel, dim3(grid), dim3(256), 0, stream, p, m, v, n4, ch, nchunks, wd, trust,
                       nt, h, lr_ptr, lr_index_ptr, step_ptr, t_host, shadow, skip);
}

void launch_flat_optim(float* p, const float* g, float* s1, float* s2, int64_t n, const OptHyper& h,
                       const float* lr_ptr, const int64_t* lr_index_ptr, const int64_t* step_ptr, float t_host,
                       uint16_t* shadow, const float* coef_ptr, hipStream_t stream, const unsigned* skip) {
  const int64_t n4 = n / 4;
  if (n4 == 0) return;
  hipLaunchKernelGGL(flat_optim_kernel, dim3(grid_for(n4)), dim3(256), 0, stream, p, g, s1, s2, n4, h, lr_ptr,
                     lr_index_ptr, step_ptr, t_host, shadow, coef_ptr, skip);
}

int sq_norm_partials_needed() { return kSqNormMaxBlocks; }

void launch_sq_norm(const float* x, int64_t n, float* part, float* out, hipStream_t stream) {
  const int64_t n4 = n / 4;
  const int nb = n4 == 0 ? 0 : (grid_for(n4) > kSqNormMaxBlocks ? kSqNormMaxBlocks : grid_for(n4));
  if (nb > 0) hipLaunchKernelGGL(sq_norm_partial_kernel, dim3(nb), dim3(256), 0, stream, x, n4, part);
  hipLaunchKernelGGL(sq_norm_final_kernel, dim3(1), dim3(256), 0, stream, part, nb, out);
}

void launch_clip_coef(const float* sq, float max_norm, float* coef, float* total_norm, hipStream_t stream) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, stream, sq, max_norm, coef, total_norm);
}

void launch_cast_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t stream) {
  const int64_t n4 = n / 4;
  if (n4 == 0) return;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_for(n4)), dim3(256), 0, stream, x, y, n4);
}

}  // namespace mlt
