// LayerNorm forward/backward and BERT embedding gather/scatter for gfx950.
//
// LayerNorm over rows of length D (768 / 1024): one wave per row, 4 rows per
// 256-thread block, bf16 in/out with 8-byte (4 x bf16) vector accesses, fp32
// statistics (two-pass mean / variance in registers), fp32 gamma/beta read
// directly from the master parameters. Backward: dx per row in one pass; dgamma /
// dbeta accumulated per lane across a grid-stride set of rows, reduced across the
// block's waves in LDS, written as per-block partials and summed over blocks by a
// second kernel in a fixed order (deterministic, no atomics).
#include "mlt_common.h"
#include "mlt_kernels.h"
#include "mlt_philox.h"

namespace mlt {

template <int VPL>  // 4-element vectors per lane: D = VPL * 256
__device__ __forceinline__ void load_row(const uint16_t* __restrict__ p, float (&x)[VPL * 4]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const ushort4 u = reinterpret_cast<const ushort4*>(p)[lane + 64 * v];
    x[4 * v + 0] = bf16_to_f32(u.x);
    x[4 * v + 1] = bf16_to_f32(u.y);
    x[4 * v + 2] = bf16_to_f32(u.z);
    x[4 * v + 3] = bf16_to_f32(u.w);
  }
}

// LayerNorm of one row held in registers (x: the wave's E values per lane): statistics, Y, mean / rstd
template <int VPL>
__device__ __forceinline__ void ln_fwd_row(const float (&x)[VPL * 4], const float* __restrict__ gamma,
                                           const float* __restrict__ beta, uint16_t* __restrict__ Y,
                                           float* __restrict__ mean, float* __restrict__ rstd, int64_t row, float eps) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) s += x[i];
  const float mu = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const float d = x[i] - mu;
    q += d * d;
  }
  const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = 4 * (lane + 64 * v);
    const float4 g = *reinterpret_cast<const float4*>(gamma + c);
    const float4 b = *reinterpret_cast<const float4*>(beta + c);
    ushort4 o;
    o.x = f32_to_bf16((x[4 * v + 0] - mu) * rs * g.x + b.x);
    o.y = f32_to_bf16((x[4 * v + 1] - mu) * rs * g.y + b.y);
    o.z = f32_to_bf16((x[4 * v + 2] - mu) * rs * g.z + b.z);
    o.w = f32_to_bf16((x[4 * v + 3] - mu) * rs * g.w + b.w);
    reinterpret_cast<ushort4*>(Y + row * D)[lane + 64 * v] = o;
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

template <int VPL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const uint16_t* __restrict__ X, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, uint16_t* __restrict__ Y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int64_t rows,
                                                     float eps) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float x[E];
  load_row<VPL>(X + row * D, x);
  ln_fwd_row<VPL>(x, gamma, beta, Y, mean, rstd, row, eps);
}

// Z = bf16(dropout(Y0) + RES), Y = LayerNorm(Z): the hidden dropout and the residual add of a
// post-LN sub-layer in the pass that normalises their sum. Y0 is the linear's output (bias
// included, no residual). The statistics and Y come from the bf16-rounded Z through ln_fwd_row,
// so Y / mean / rstd are bitwise what ln_fwd_kernel gives on Z, and the backward recomputes xhat
// from the saved Z. The mask is recomputed from (row, column), nothing is stored (mlt_philox.h).
template <int VPL>
__global__ __launch_bounds__(256) void dropout_add_ln_fwd_kernel(
    const uint16_t* __restrict__ Y0, const uint16_t* __restrict__ RES, const float* __restrict__ gamma,
    const float* __restrict__ beta, uint16_t* __restrict__ Z, uint16_t* __restrict__ Y, float* __restrict__ mean,
    float* __restrict__ rstd, int64_t rows, float eps, DropArgs dr) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float x[E];
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const ushort4 a = reinterpret_cast<const ushort4*>(Y0 + row * D)[lane + 64 * v];
    const ushort4 r = reinterpret_cast<const ushort4*>(RES + row * D)[lane + 64 * v];
    const Philox4 w = drop_words((uint64_t)row * (D / 4) + lane + 64 * v, dr);
    // __fmul_rn: the scaled value is rounded to fp32 before the add (no fma contraction)
    ushort4 z;
    z.x = f32_to_bf16((w.x >= dr.thr ? __fmul_rn(bf16_to_f32(a.x), dr.scale) : 0.f) + bf16_to_f32(r.x));
    z.y = f32_to_bf16((w.y >= dr.thr ? __fmul_rn(bf16_to_f32(a.y), dr.scale) : 0.f) + bf16_to_f32(r.y));
    z.z = f32_to_bf16((w.z >= dr.thr ? __fmul_rn(bf16_to_f32(a.z), dr.scale) : 0.f) + bf16_to_f32(r.z));
    z.w = f32_to_bf16((w.w >= dr.thr ? __fmul_rn(bf16_to_f32(a.w), dr.scale) : 0.f) + bf16_to_f32(r.w));
    reinterpret_cast<ushort4*>(Z + row * D)[lane + 64 * v] = z;
    x[4 * v + 0] = bf16_to_f32(z.x);
    x[4 * v + 1] = bf16_to_f32(z.y);
    x[4 * v + 2] = bf16_to_f32(z.z);
    x[4 * v + 3] = bf16_to_f32(z.w);
  }
  ln_fwd_row<VPL>(x, gamma, beta, Y, mean, rstd, row, eps);
}

// dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)); partial dgamma/dbeta per block.
// DXS: also emit per-block column sums of the (bf16-rounded) dx -- the bias gradient of the
// linear layer whose output (plus residual) fed this LayerNorm, fused here for free.
// DROP (with DXS, without DRES): the LayerNorm's input was dropout(linear) + residual
// (dropout_add_ln_fwd_kernel). DX is the residual's gradient as before; the linear's dY is
// DXM = keep ? bf16(dx_bf16 * scale) : 0 with the forward's mask, and the column sums are DXM's.
// The dropout arguments are a trailing pack (one LnBwdDrop when DROP, empty otherwise), so the
// instantiations without dropout keep the argument list, and with it the code, they had before.
// DX is bitwise the same in every instantiation (DXS or not, DROP or not): the row's fp32 arithmetic is
// written out below with contraction off and every fused multiply-add an explicit fmaf, so which
// products fuse is this source's choice and not the compiler's, which used to follow what else hangs
// off the values (the plain and the DXS instantiation then rounded a few DX per million differently).
struct LnBwdDrop {
  uint16_t* DXM;
  DropArgs dr;
};
__device__ __forceinline__ const LnBwdDrop& ln_bwd_drop_arg(const LnBwdDrop& d) { return d; }

template <int VPL, bool DXS, bool DROP = false, typename... DropT>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const uint16_t* __restrict__ DY, const uint16_t* __restrict__ X,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, uint16_t* __restrict__ DX,
                                                     float* __restrict__ part, int64_t rows,
                                                     const uint16_t* __restrict__ DRES, DropT... drop_args) {
#pragma clang fp contract(off)
  static_assert(!DROP || DXS, "the dropout variant always reduces DXM's column sums");
  static_assert(sizeof...(DropT) == (DROP ? 1 : 0), "one LnBwdDrop exactly when DROP");
  constexpr int D = VPL * 256, E = VPL * 4;
  constexpr int NS = DXS ? 3 : 2;
  __shared__ float red[4][NS * D];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float dg[E], db[E], g[E], dxs[DXS ? E : 1];  // dxs: the column sums of DX, or of DXM when DROP
#pragma unroll
  for (int i = 0; i < E; ++i) {
    dg[i] = 0.f;
    db[i] = 0.f;
    if constexpr (DXS) dxs[i] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const float4 gv = *reinterpret_cast<const float4*>(gamma + 4 * (lane + 64 * v));
    g[4 * v] = gv.x;
    g[4 * v + 1] = gv.y;
    g[4 * v + 2] = gv.z;
    g[4 * v + 3] = gv.w;
  }
  // software-pipelined over the wave's rows: the next row's x / dy / statistics are in flight
  // while this row computes (each wave walks ~rows / 2048 rows; one row of latency per step otherwise)
  const int64_t rstep = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + wid;
  ushort4 nx[VPL], ndy[VPL];
  float nmu = 0.f, nrs = 0.f;
  auto fetch = [&](int64_t r) {
    const int64_t rr = r < rows ? r : rows - 1;  // clamped, branch-free
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      nx[v] = reinterpret_cast<const ushort4*>(X + rr * D)[lane + 64 * v];
      ndy[v] = reinterpret_cast<const ushort4*>(DY + rr * D)[lane + 64 * v];
    }
    nmu = mean[rr];
    nrs = rstd[rr];
  };
  if (row < rows) fetch(row);
  for (; row < rows; row += rstep) {
    float x[E], dy[E];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      x[4 * v + 0] = bf16_to_f32(nx[v].x);
      x[4 * v + 1] = bf16_to_f32(nx[v].y);
      x[4 * v + 2] = bf16_to_f32(nx[v].z);
      x[4 * v + 3] = bf16_to_f32(nx[v].w);
      dy[4 * v + 0] = bf16_to_f32(ndy[v].x);
      dy[4 * v + 1] = bf16_to_f32(ndy[v].y);
      dy[4 * v + 2] = bf16_to_f32(ndy[v].z);
      dy[4 * v + 3] = bf16_to_f32(ndy[v].w);
    }
    const float mu = nmu, rs = nrs;
    fetch(row + rstep);  // unconditional: past the end it re-reads the last row (unused)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const float xh = (x[i] - mu) * rs;
      x[i] = xh;
      const float t = dy[i] * g[i];
      s1 += t;
      s2 = fmaf(t, xh, s2);
      dg[i] = fmaf(dy[i], xh, dg[i]);
      db[i] += dy[i];
    }
    s1 = wave_sum(s1) * (1.f / D);
    s2 = wave_sum(s2) * (1.f / D);
    float dres[E];
    if (DRES) load_row<VPL>(DRES + row * D, dres);
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * v + q;
        // rs * (dy * g - s1 - xh * s2) + dres, one rounding per line
        const float a = fmaf(dy[i], g[i], -s1);
        const float b = fmaf(-x[i], s2, a);
        o[q] = DRES ? fmaf(rs, b, dres[i]) : rs * b;
      }
      ushort4 u;
      u.x = f32_to_bf16(o[0]);
      u.y = f32_to_bf16(o[1]);
      u.z = f32_to_bf16(o[2]);
      u.w = f32_to_bf16(o[3]);
      reinterpret_cast<ushort4*>(DX + row * D)[lane + 64 * v] = u;
      if constexpr (DROP) {
        const LnBwdDrop& drop = ln_bwd_drop_arg(drop_args...);
        // DXM from the stored (bf16-rounded) DX; the mask of the global row (not the pipeline's
        // clamped fetch row), as in the forward
        const Philox4 w = drop_words((uint64_t)row * (D / 4) + lane + 64 * v, drop.dr);
        const uint32_t thr = drop.dr.thr;
        const float sc = drop.dr.scale;
        ushort4 m;
        m.x = w.x >= thr ? f32_to_bf16(bf16_to_f32(u.x) * sc) : (uint16_t)0;
        m.y = w.y >= thr ? f32_to_bf16(bf16_to_f32(u.y) * sc) : (uint16_t)0;
        m.z = w.z >= thr ? f32_to_bf16(bf16_to_f32(u.z) * sc) : (uint16_t)0;
        m.w = w.w >= thr ? f32_to_bf16(bf16_to_f32(u.w) * sc) : (uint16_t)0;
        reinterpret_cast<ushort4*>(drop.DXM + row * D)[lane + 64 * v] = m;
        dxs[4 * v + 0] += bf16_to_f32(m.x);
        dxs[4 * v + 1] += bf16_to_f32(m.y);
        dxs[4 * v + 2] += bf16_to_f32(m.z);
        dxs[4 * v + 3] += bf16_to_f32(m.w);
      } else if constexpr (DXS) {
        dxs[4 * v + 0] += bf16_to_f32(u.x);
        dxs[4 * v + 1] += bf16_to_f32(u.y);
        dxs[4 * v + 2] += bf16_to_f32(u.z);
        dxs[4 * v + 3] += bf16_to_f32(u.w);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 4 * (lane + 64 * v) + q;
      red[wid][c] = dg[4 * v + q];
      red[wid][D + c] = db[4 * v + q];
      if constexpr (DXS) red[wid][2 * D + c] = dxs[4 * v + q];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < NS * D; c += 256)
    part[(int64_t)blockIdx.x * NS * D + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// out_k[c] (+)= sum_r part[r][k*seg + c]: wave = 4 columns, lanes stride the rows, xor tree (fixed order)
__global__ __launch_bounds__(256) void reduce_rows_kernel(const float* __restrict__ part, int R, int64_t ld, int W,
                                                          int seg, SegOut o, int accmask) {
  const int lane = threadIdx.x & 63;
  const int c = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (c >= W) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int r = lane; r < R; r += 64) {
    const float4 v = *reinterpret_cast<const float4*>(part + (int64_t)r * ld + c);
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s.x += __shfl_xor(s.x, off, 64);
    s.y += __shfl_xor(s.y, off, 64);
    s.z += __shfl_xor(s.z, off, 64);
    s.w += __shfl_xor(s.w, off, 64);
  }
  if (lane == 0) {
    const int k = c / seg;
    float* out = o.p[k] + (c - k * seg);
    if ((accmask >> k) & 1) {
      const float4 prev = *reinterpret_cast<const float4*>(out);
      s.x += prev.x;
      s.y += prev.y;
      s.z += prev.z;
      s.w += prev.w;
    }
    *reinterpret_cast<float4*>(out) = s;
  }
}

void launch_reduce_rows(const float* part, int R, int64_t ld, int W, int seg, SegOut outs, int accmask, hipStream_t st) {
  if (W <= 0 || R <= 0) return;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3((W / 4 + 3) / 4), dim3(256), 0, st, part, R, ld, W, seg, outs, accmask);
}

// the row kernels are instantiated for 1..4 float4 per lane: D = 256, 512, 768 or 1024
template <class F>
static void by_vpl(const char* launcher, int D, F&& f) {
  if (D % 256 != 0 || !dispatch_int<1, 2, 3, 4>(D / 256, f)) throw_no_kernel(launcher, "D", D);
}

void launch_ln_fwd(const uint16_t* X, const float* gamma, const float* beta, uint16_t* Y, float* mean, float* rstd,
                   int64_t rows, int D, float eps, hipStream_t st) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  by_vpl("launch_ln_fwd", D, [&](auto v) {
    hipLaunchKernelGGL(ln_fwd_kernel<v()>, grid, block, 0, st, X, gamma, beta, Y, mean, rstd, rows, eps);
  });
}

void launch_dropout_add_ln_fwd(const uint16_t* Y0, const uint16_t* RES, const float* gamma, const float* beta,
                               uint16_t* Z, uint16_t* Y, float* mean, float* rstd, int64_t rows, int D, float eps,
                               DropArgs dr, hipStream_t st) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  by_vpl("launch_dropout_add_ln_fwd", D, [&](auto v) {
    hipLaunchKernelGGL(dropout_add_ln_fwd_kernel<v()>, grid, block, 0, st, Y0, RES, gamma, beta, Z, Y, mean, rstd,
                       rows, eps, dr);
  });
}

int ln_bwd_partial_blocks(int64_t rows) {
  int64_t nb = (rows + 3) / 4;
  return (int)(nb < 512 ? nb : 512);
}

void launch_ln_bwd(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean, const float* rstd,
                   uint16_t* DX, float* part, float* dgamma, float* dbeta, int64_t rows, int D, int accumulate,
                   const uint16_t* DRES, float* dxsum, int dxsum_acc, hipStream_t st) {
  if (rows <= 0) return;
  const int nb = ln_bwd_partial_blocks(rows);
  const dim3 grid(nb), block(256);
  by_vpl("launch_ln_bwd", D, [&](auto v) {
    constexpr int V = decltype(v)::value;
    dispatch_bools(
        [&](auto sum) {
          hipLaunchKernelGGL((ln_bwd_kernel<V, decltype(sum)::value>), grid, block, 0, st, DY, X, gamma, mean, rstd, DX,
                             part, rows, DRES);
        },
        dxsum != nullptr);
  });
  SegOut o{{dgamma, dbeta, dxsum}};
  launch_reduce_rows(part, nb, (dxsum ? 3 : 2) * D, (dxsum ? 3 : 2) * D, D, o, (accumulate ? 3 : 0) | (dxsum_acc ? 4 : 0), st);
}

// the dropout variant: DX as above, DXM = mask * scale * DX, dxsum = column sums of DXM (required)
void launch_ln_bwd_dropout(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean,
                           const float* rstd, uint16_t* DX, uint16_t* DXM, float* part, float* dgamma, float* dbeta,
                           int64_t rows, int D, int accumulate, float* dxsum, int dxsum_acc, DropArgs dr,
                           hipStream_t st) {
  if (rows <= 0) return;
  const int nb = ln_bwd_partial_blocks(rows);
  const dim3 grid(nb), block(256);
  const LnBwdDrop d{DXM, dr};
  const uint16_t* no_res = nullptr;
  by_vpl("launch_ln_bwd_dropout", D, [&](auto v) {
    hipLaunchKernelGGL((ln_bwd_kernel<v(), true, true, LnBwdDrop>), grid, block, 0, st, DY, X, gamma, mean, rstd, DX,
                       part, rows, no_res, d);
  });
  SegOut o{{dgamma, dbeta, dxsum}};
  launch_reduce_rows(part, nb, 3 * D, 3 * D, D, o, (accumulate ? 3 : 0) | (dxsum_acc ? 4 : 0), st);
}

// ---------------------------------------------------------------------------
// BERT embeddings: out[t] = Wword[ids[t]] + Wpos[pos[t]] + Wtype[tt[t]]  (bf16 tables, bf16 out)
// pos[t] = t % S for a padded [B, S] batch; a packed batch (T real tokens, no pads) passes the
// positions explicitly (posv [T], each the index inside the token's own sequence, < S).
// ---------------------------------------------------------------------------
template <int VPL>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tt,
                                                        const uint16_t* __restrict__ Ww, const uint16_t* __restrict__ Wp,
                                                        const uint16_t* __restrict__ Wt, uint16_t* __restrict__ out,
                                                        int64_t rows, int S, int64_t vocab, int ntype,
                                                        const int* __restrict__ posv) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int64_t id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  int64_t ty = tt ? tt[row] : 0;
  ty = ty < 0 ? 0 : (ty >= ntype ? ntype - 1 : ty);
  int pos = posv ? posv[row] : (int)(row % S);
  if (posv) {
    MLT_DCHECK(pos >= 0 && pos < S);
    pos = pos < 0 ? 0 : (pos >= S ? S - 1 : pos);  // (S <= position-table rows, checked by the caller)
  }
  float a[E], b[E], c[E];
  load_row<VPL>(Ww + id * D, a);
  if (Wp) {
    load_row<VPL>(Wp + (int64_t)pos * D, b);
  } else {  // no position table (rotary positions): word + type, the sum a zero table gives
#pragma unroll
    for (int e = 0; e < E; ++e) b[e] = 0.f;
  }
  load_row<VPL>(Wt + ty * D, c);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    ushort4 o;
    o.x = f32_to_bf16(a[4 * v] + b[4 * v] + c[4 * v]);
    o.y = f32_to_bf16(a[4 * v + 1] + b[4 * v + 1] + c[4 * v + 1]);
    o.z = f32_to_bf16(a[4 * v + 2] + b[4 * v + 2] + c[4 * v + 2]);
    o.w = f32_to_bf16(a[4 * v + 3] + b[4 * v + 3] + c[4 * v + 3]);
    reinterpret_cast<ushort4*>(out + row * D)[lane + 64 * v] = o;
  }
}

// word / position grads: fp32 atomics (the vocabulary rows hit are sparse and spread);
// token-type grads: per-block partials over the (few) type rows, reduced in fixed order.
// Embedding backward without atomics (bitwise reproducible):
//  * word rows: the token ids arrive clamped to the table and sorted (stable, host-side torch.sort
//    of ids.clamp(0, vocab - 1), as ops/transformer.py does) with the permutation: two different
//    out-of-range ids would otherwise be two runs, and two writers, for the one row they clamp to;
//    one wave per sorted entry, and the wave that starts a run of equal ids sums that run's
//    gradient rows in token order and adds the sum to its table row (one writer per row);
//  * positions / token types: one wave per position sums the B rows of that position in batch
//    order into gp, and leaves the per-type sums as a partial row for reduce_rows. PACKED: the batch
//    is T token rows with sequence b at rows cu[b] .. cu[b + 1]; the wave of position p sums rows
//    cu[b] + p over the sequences longer than p, still in batch order.
template <int VPL>
__global__ __launch_bounds__(256) void embed_bwd_word_kernel(const int64_t* __restrict__ sid,
                                                             const int64_t* __restrict__ perm,
                                                             const uint16_t* __restrict__ DX, float* __restrict__ gw,
                                                             int64_t rows, int64_t vocab) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= rows) return;
  const int64_t id = sid[i];
  if (i > 0 && sid[i - 1] == id) return;  // not the start of a run
  float acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  for (int64_t j = i; j < rows && sid[j] == id; ++j) {
    float d[E];
    load_row<VPL>(DX + perm[j] * D, d);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += d[e];
  }
  const int64_t row = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    float4* g = reinterpret_cast<float4*>(gw + row * D + 4 * (lane + 64 * v));
    float4 o = *g;
    o.x += acc[4 * v];
    o.y += acc[4 * v + 1];
    o.z += acc[4 * v + 2];
    o.w += acc[4 * v + 3];
    *g = o;
  }
}

template <int VPL, bool PACKED>
__global__ __launch_bounds__(256) void embed_bwd_pos_kernel(const int64_t* __restrict__ tt,
                                                            const uint16_t* __restrict__ DX, float* __restrict__ gp,
                                                            float* __restrict__ part_t, int64_t rows, int S,
                                                            const int* __restrict__ cu, int B) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pos >= S) return;
  float a[E], t0[E], t1[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = t0[e] = t1[e] = 0.f;
  auto add_row = [&](int64_t r) {
    float d[E];
    load_row<VPL>(DX + r * D, d);
    const bool one = tt && tt[r] != 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      a[e] += d[e];
      t0[e] += one ? 0.f : d[e];
      t1[e] += one ? d[e] : 0.f;
    }
  };
  if constexpr (PACKED) {
    for (int b = 0; b < B; ++b) {
      const int c0 = cu[b], c1 = cu[b + 1];
      MLT_DCHECK(c0 >= 0 && c1 >= c0 && c1 - c0 <= S && c1 <= rows);
      if (pos < c1 - c0 && (int64_t)c0 + pos < rows) add_row((int64_t)c0 + pos);
    }
  } else {
    for (int64_t r = pos; r < rows; r += S) add_row(r);
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = 4 * (lane + 64 * v);
    if (gp) {  // (nullptr: no position table, only the token-type partials are wanted)
      float4* g = reinterpret_cast<float4*>(gp + (int64_t)pos * D + c);
      float4 o = *g;
      o.x += a[4 * v];
      o.y += a[4 * v + 1];
      o.z += a[4 * v + 2];
      o.w += a[4 * v + 3];
      *g = o;
    }
    *reinterpret_cast<float4*>(part_t + (int64_t)pos * 2 * D + c) =
        make_float4(t0[4 * v], t0[4 * v + 1], t0[4 * v + 2], t0[4 * v + 3]);
    *reinterpret_cast<float4*>(part_t + (int64_t)pos * 2 * D + D + c) =
        make_float4(t1[4 * v], t1[4 * v + 1], t1[4 * v + 2], t1[4 * v + 3]);
  }
}

void launch_embed_fwd(const int64_t* ids, const int64_t* tt, const uint16_t* Ww, const uint16_t* Wp,
                      const uint16_t* Wt, uint16_t* out, int64_t rows, int S, int D, int64_t vocab, int ntype,
                      hipStream_t st, const int* pos) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  by_vpl("launch_embed_fwd", D, [&](auto v) {
    hipLaunchKernelGGL(embed_fwd_kernel<v()>, grid, block, 0, st, ids, tt, Ww, Wp, Wt, out, rows, S, vocab, ntype, pos);
  });
}

void launch_embed_bwd(const int64_t* sid, const int64_t* perm, const int64_t* tt, const uint16_t* DX, float* gw,
                      float* gp, float* gt, float* part, int64_t rows, int S, int D, int64_t vocab, int ntype,
                      hipStream_t st, const int* cu, int B) {
  if (rows <= 0) return;
  const dim3 gw_grid((unsigned)((rows + 3) / 4)), gp_grid((unsigned)((S + 3) / 4)), block(256);
  const int64_t* tt2 = ntype >= 2 ? tt : nullptr;
  by_vpl("launch_embed_bwd", D, [&](auto v) {
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(embed_bwd_word_kernel<V>, gw_grid, block, 0, st, sid, perm, DX, gw, rows, vocab);
    dispatch_bools(
        [&](auto packed) {
          hipLaunchKernelGGL((embed_bwd_pos_kernel<V, decltype(packed)::value>), gp_grid, block, 0, st, tt2, DX, gp,
                             part, rows, S, cu, B);
        },
        cu != nullptr);
  });
  // token types 0 and 1 (ntype <= 2): the S partial rows summed in position order into gt. A one-row
  // type table takes every token as type 0, as the forward's clamp reads it (tt is not passed on: with
  // it the type-1 tokens' gradient went to the partial that is not summed, and was lost).
  SegOut o{{gt, gt + D, nullptr}};
  launch_reduce_rows(part, S, 2 * D, ntype >= 2 ? 2 * D : D, D, o, ntype >= 2 ? 3 : 1, st);
}

// ---------------------------------------------------------------------------
// Pre-norm blocks. The residual stream h and its norm n are separate tensors there, so the norm
// backward's DX is rstd (...) + DRES with DRES = the stream's own gradient, also under hidden dropout:
// ln_bwd_kernel<VPL, true, true> reads DRES at run time like the other instantiations, only its launcher
// passed none so far. DX is then the total stream gradient and DXM its masked, scaled copy.
// ---------------------------------------------------------------------------
void launch_ln_bwd_dropout_res(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* mean,
                               const float* rstd, uint16_t* DX, uint16_t* DXM, float* part, float* dgamma,
                               float* dbeta, int64_t rows, int D, int accumulate, const uint16_t* DRES, float* dxsum,
                               int dxsum_acc, DropArgs dr, hipStream_t st) {
  if (rows <= 0) return;
  const int nb = ln_bwd_partial_blocks(rows);
  const dim3 grid(nb), block(256);
  const LnBwdDrop d{DXM, dr};
  by_vpl("launch_ln_bwd_dropout_res", D, [&](auto v) {
    hipLaunchKernelGGL((ln_bwd_kernel<v(), true, true, LnBwdDrop>), grid, block, 0, st, DY, X, gamma, mean, rstd, DX,
                       part, rows, DRES, d);
  });
  SegOut o{{dgamma, dbeta, dxsum}};
  launch_reduce_rows(part, nb, 3 * D, 3 * D, D, o, (accumulate ? 3 : 0) | (dxsum_acc ? 4 : 0), st);
}

// ---------------------------------------------------------------------------
// RMSNorm: y = x * rsqrt(mean(x^2) + eps) * g. No centring, no bias; the row-kernel design of the
// LayerNorm kernels above (one wave per row, 8-byte bf16 accesses, fp32 statistics, fixed-order
// partials through reduce_rows). Only rstd is saved.
// ---------------------------------------------------------------------------
template <int VPL>
__device__ __forceinline__ void rms_fwd_row(const float (&x)[VPL * 4], const float* __restrict__ gamma,
                                            uint16_t* __restrict__ Y, float* __restrict__ rstd, int64_t row,
                                            float eps) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) q += x[i] * x[i];
  const float rs = rsqrtf(wave_sum(q) * (1.f / D) + eps);
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * (lane + 64 * v));
    ushort4 o;
    o.x = f32_to_bf16(x[4 * v + 0] * rs * g.x);
    o.y = f32_to_bf16(x[4 * v + 1] * rs * g.y);
    o.z = f32_to_bf16(x[4 * v + 2] * rs * g.z);
    o.w = f32_to_bf16(x[4 * v + 3] * rs * g.w);
    reinterpret_cast<ushort4*>(Y + row * D)[lane + 64 * v] = o;
  }
  if (lane == 0) rstd[row] = rs;
}

template <int VPL>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const uint16_t* __restrict__ X, const float* __restrict__ gamma,
                                                      uint16_t* __restrict__ Y, float* __restrict__ rstd,
                                                      int64_t rows, float eps) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float x[E];
  load_row<VPL>(X + row * D, x);
  rms_fwd_row<VPL>(x, gamma, Y, rstd, row, eps);
}

// Z = bf16(dropout(Y0) + RES), Y = RMSNorm(Z): mask, scaling and rounding of Z as in
// dropout_add_ln_fwd_kernel; Y / rstd through rms_fwd_row from the rounded Z, so bitwise rms_fwd_kernel's on Z.
template <int VPL>
__global__ __launch_bounds__(256) void dropout_add_rms_fwd_kernel(
    const uint16_t* __restrict__ Y0, const uint16_t* __restrict__ RES, const float* __restrict__ gamma,
    uint16_t* __restrict__ Z, uint16_t* __restrict__ Y, float* __restrict__ rstd, int64_t rows, float eps,
    DropArgs dr) {
  constexpr int D = VPL * 256, E = VPL * 4;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float x[E];
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const ushort4 a = reinterpret_cast<const ushort4*>(Y0 + row * D)[lane + 64 * v];
    const ushort4 r = reinterpret_cast<const ushort4*>(RES + row * D)[lane + 64 * v];
    const Philox4 w = drop_words((uint64_t)row * (D / 4) + lane + 64 * v, dr);
    ushort4 z;
    z.x = f32_to_bf16((w.x >= dr.thr ? __fmul_rn(bf16_to_f32(a.x), dr.scale) : 0.f) + bf16_to_f32(r.x));
    z.y = f32_to_bf16((w.y >= dr.thr ? __fmul_rn(bf16_to_f32(a.y), dr.scale) : 0.f) + bf16_to_f32(r.y));
    z.z = f32_to_bf16((w.z >= dr.thr ? __fmul_rn(bf16_to_f32(a.z), dr.scale) : 0.f) + bf16_to_f32(r.z));
    z.w = f32_to_bf16((w.w >= dr.thr ? __fmul_rn(bf16_to_f32(a.w), dr.scale) : 0.f) + bf16_to_f32(r.w));
    reinterpret_cast<ushort4*>(Z + row * D)[lane + 64 * v] = z;
    x[4 * v + 0] = bf16_to_f32(z.x);
    x[4 * v + 1] = bf16_to_f32(z.y);
    x[4 * v + 2] = bf16_to_f32(z.z);
    x[4 * v + 3] = bf16_to_f32(z.w);
  }
  rms_fwd_row<VPL>(x, gamma, Y, rstd, row, eps);
}

// xh = x rstd, t = dy g, s2 = mean(t xh): dx = rstd (t - xh s2) (+ dres); partial dgamma per block.
// DXS / DROP and the trailing pack as in ln_bwd_kernel; DRES is read at run time in every instantiation
// (the pre-norm blocks pass the residual stream's gradient there, with and without dropout). Contraction
// off and explicit fmaf, so DX is bitwise the same in every instantiation.
template <int VPL, bool DXS, bool DROP = false, typename... DropT>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const uint16_t* __restrict__ DY, const uint16_t* __restrict__ X,
                                                      const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                      uint16_t* __restrict__ DX, float* __restrict__ part, int64_t rows,
                                                      const uint16_t* __restrict__ DRES, DropT... drop_args) {
#pragma clang fp contract(off)
  static_assert(!DROP || DXS, "the dropout variant always reduces DXM's column sums");
  static_assert(sizeof...(DropT) == (DROP ? 1 : 0), "one LnBwdDrop exactly when DROP");
  constexpr int D = VPL * 256, E = VPL * 4;
  constexpr int NS = DXS ? 2 : 1;
  __shared__ float red[4][NS * D];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float dg[E], g[E], dxs[DXS ? E : 1];  // dxs: the column sums of DX, or of DXM when DROP
#pragma unroll
  for (int i = 0; i < E; ++i) {
    dg[i] = 0.f;
    if constexpr (DXS) dxs[i] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const float4 gv = *reinterpret_cast<const float4*>(gamma + 4 * (lane + 64 * v));
    g[4 * v] = gv.x;
    g[4 * v + 1] = gv.y;
    g[4 * v + 2] = gv.z;
    g[4 * v + 3] = gv.w;
  }
  // software-pipelined over the wave's rows, as in ln_bwd_kernel
  const int64_t rstep = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + wid;
  ushort4 nx[VPL], ndy[VPL];
  float nrs = 0.f;
  auto fetch = [&](int64_t r) {
    const int64_t rr = r < rows ? r : rows - 1;  // clamped, branch-free
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      nx[v] = reinterpret_cast<const ushort4*>(X + rr * D)[lane + 64 * v];
      ndy[v] = reinterpret_cast<const ushort4*>(DY + rr * D)[lane + 64 * v];
    }
    nrs = rstd[rr];
  };
  if (row < rows) fetch(row);
  for (; row < rows; row += rstep) {
    float x[E], dy[E];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      x[4 * v + 0] = bf16_to_f32(nx[v].x);
      x[4 * v + 1] = bf16_to_f32(nx[v].y);
      x[4 * v + 2] = bf16_to_f32(nx[v].z);
      x[4 * v + 3] = bf16_to_f32(nx[v].w);
      dy[4 * v + 0] = bf16_to_f32(ndy[v].x);
      dy[4 * v + 1] = bf16_to_f32(ndy[v].y);
      dy[4 * v + 2] = bf16_to_f32(ndy[v].z);
      dy[4 * v + 3] = bf16_to_f32(ndy[v].w);
    }
    const float rs = nrs;
    fetch(row + rstep);  // unconditional: past the end it re-reads the last row (unused)
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const float xh = x[i] * rs;
      x[i] = xh;
      const float t = dy[i] * g[i];
      s2 = fmaf(t, xh, s2);
      dg[i] = fmaf(dy[i], xh, dg[i]);
      dy[i] = t;
    }
    s2 = wave_sum(s2) * (1.f / D);
    float dres[E];
    if (DRES) load_row<VPL>(DRES + row * D, dres);
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * v + q;
        // rs * (t - xh * s2) + dres, one rounding per line
        const float b = fmaf(-x[i], s2, dy[i]);
        o[q] = DRES ? fmaf(rs, b, dres[i]) : rs * b;
      }
      ushort4 u;
      u.x = f32_to_bf16(o[0]);
      u.y = f32_to_bf16(o[1]);
      u.z = f32_to_bf16(o[2]);
      u.w = f32_to_bf16(o[3]);
      reinterpret_cast<ushort4*>(DX + row * D)[lane + 64 * v] = u;
      if constexpr (DROP) {
        const LnBwdDrop& drop = ln_bwd_drop_arg(drop_args...);
        // DXM from the stored (bf16-rounded) DX; the mask of the global row, as in the forward
        const Philox4 w = drop_words((uint64_t)row * (D / 4) + lane + 64 * v, drop.dr);
        const uint32_t thr = drop.dr.thr;
        const float sc = drop.dr.scale;
        ushort4 m;
        m.x = w.x >= thr ? f32_to_bf16(bf16_to_f32(u.x) * sc) : (uint16_t)0;
        m.y = w.y >= thr ? f32_to_bf16(bf16_to_f32(u.y) * sc) : (uint16_t)0;
        m.z = w.z >= thr ? f32_to_bf16(bf16_to_f32(u.z) * sc) : (uint16_t)0;
        m.w = w.w >= thr ? f32_to_bf16(bf16_to_f32(u.w) * sc) : (uint16_t)0;
        reinterpret_cast<ushort4*>(drop.DXM + row * D)[lane + 64 * v] = m;
        dxs[4 * v + 0] += bf16_to_f32(m.x);
        dxs[4 * v + 1] += bf16_to_f32(m.y);
        dxs[4 * v + 2] += bf16_to_f32(m.z);
        dxs[4 * v + 3] += bf16_to_f32(m.w);
      } else if constexpr (DXS) {
        dxs[4 * v + 0] += bf16_to_f32(u.x);
        dxs[4 * v + 1] += bf16_to_f32(u.y);
        dxs[4 * v + 2] += bf16_to_f32(u.z);
        dxs[4 * v + 3] += bf16_to_f32(u.w);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 4 * (lane + 64 * v) + q;
      red[wid][c] = dg[4 * v + q];
      if constexpr (DXS) red[wid][D + c] = dxs[4 * v + q];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < NS * D; c += 256)
    part[(int64_t)blockIdx.x * NS * D + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

void launch_rms_fwd(const uint16_t* X, const float* gamma, uint16_t* Y, float* rstd, int64_t rows, int D, float eps,
                    hipStream_t st) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  by_vpl("launch_rms_fwd", D,
         [&](auto v) { hipLaunchKernelGGL(rms_fwd_kernel<v()>, grid, block, 0, st, X, gamma, Y, rstd, rows, eps); });
}

void launch_dropout_add_rms_fwd(const uint16_t* Y0, const uint16_t* RES, const float* gamma, uint16_t* Z, uint16_t* Y,
                                float* rstd, int64_t rows, int D, float eps, DropArgs dr, hipStream_t st) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  by_vpl("launch_dropout_add_rms_fwd", D, [&](auto v) {
    hipLaunchKernelGGL(dropout_add_rms_fwd_kernel<v()>, grid, block, 0, st, Y0, RES, gamma, Z, Y, rstd, rows, eps, dr);
  });
}

// part: ln_bwd_partial_blocks(rows) * (dxsum ? 2 : 1) * D floats. DXM (with dxsum): the dropout variant.
void launch_rms_bwd(const uint16_t* DY, const uint16_t* X, const float* gamma, const float* rstd, uint16_t* DX,
                    uint16_t* DXM, float* part, float* dgamma, int64_t rows, int D, int accumulate,
                    const uint16_t* DRES, float* dxsum, int dxsum_acc, DropArgs dr, hipStream_t st) {
  if (rows <= 0) return;
  const int nb = ln_bwd_partial_blocks(rows);
  const dim3 grid(nb), block(256);
  const int NS = dxsum ? 2 : 1;
  by_vpl("launch_rms_bwd", D, [&](auto v) {
    constexpr int V = decltype(v)::value;
    if (DXM) {
      const LnBwdDrop d{DXM, dr};
      hipLaunchKernelGGL((rms_bwd_kernel<V, true, true, LnBwdDrop>), grid, block, 0, st, DY, X, gamma, rstd, DX, part,
                         rows, DRES, d);
    } else {
      dispatch_bools(
          [&](auto sum) {
            hipLaunchKernelGGL((rms_bwd_kernel<V, decltype(sum)::value>), grid, block, 0, st, DY, X, gamma, rstd, DX,
                               part, rows, DRES);
          },
          dxsum != nullptr);
    }
  });
  SegOut o{{dgamma, dxsum, nullptr}};
  launch_reduce_rows(part, nb, NS * D, NS * D, D, o, (accumulate ? 1 : 0) | (dxsum_acc ? 2 : 0), st);
}

}  // namespace mlt
