// Grouped-query attention around the unchanged flash attention kernels, for gfx950: the compact QKV layout of a
// model with Hkv < H key/value heads expanded to the wide layout the attention kernels read, and the wide dQKV
// they write reduced back.
//
// compact [rows][ldc >= (H + 2 Hkv) * 64] bf16: q (H heads) | k (Hkv heads) | v (Hkv heads) per row;
// wide    [rows][ldw >= 3 * H * 64] bf16:       q | k | v with H heads each. G = H / Hkv, query head h belongs to
// KV head h / G (contiguous groups). Row strides are multiples of 8 and the bases 16-byte aligned.
//
// gqa_expand: a lane owns one 16-byte chunk (8 dims) of a compact row. A q chunk is stored once; a k or v chunk
// is stored G times, to heads hkv * G .. hkv * G + G - 1. compact is read exactly once; the result is a bitwise
// copy. Bytes: rows * 128 * ((H + 2 Hkv) read + 3 H written).
// gqa_reduce: a lane owns one 16-byte chunk of a compact row of dQKV. A dq chunk is copied; a dk / dv chunk is
// ((x_0 + x_1) + ... + x_{G-1}) over the group's heads in ascending order, every addition rounded to fp32, the
// sum rounded once to bf16 (round to nearest even): the sequential fp32 sum of ops/gqa.py is a bitwise oracle.
// Both: the grid is flat over rows x (H + 2 Hkv) x 8 lanes (64-bit index), no LDS, no atomics, 16-byte loads and
// vector stores only; columns past the layouts and rows past `rows` are never touched. Neither knows about
// sequences: padded and packed batches alike.
#include "mlt_common.h"
#include "mlt_kernels.h"

namespace mlt {

// where chunk (slot, c) of a compact row lives in the wide row: its first copy, and how many copies (heads) it has
struct GqaChunk {
  int wide_col;  // element offset of the first head's chunk in the wide row
  int copies;    // 1 for q, G for k / v
};

__device__ __forceinline__ GqaChunk gqa_chunk(int slot, int c, int H, int Hkv) {
  if (slot < H) return {slot * 64 + c * 8, 1};
  const int t = slot - H, which = t >= Hkv ? 1 : 0, hkv = t - which * Hkv, G = H / Hkv;
  return {((1 + which) * H + hkv * G) * 64 + c * 8, G};
}

__global__ __launch_bounds__(256) void gqa_expand_kernel(const uint16_t* __restrict__ compact, int64_t ldc,
                                                         uint16_t* __restrict__ wide, int64_t ldw, int64_t rows, int H,
                                                         int Hkv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = (H + 2 * Hkv) * 8;
  const int64_t row = i / per_row;
  if (row >= rows) return;
  const int r = (int)(i - row * per_row), slot = r >> 3, c = r & 7;
  const uint4 x = *reinterpret_cast<const uint4*>(compact + row * ldc + slot * 64 + c * 8);
  const GqaChunk k = gqa_chunk(slot, c, H, Hkv);
  uint16_t* dst = wide + row * ldw + k.wide_col;
  for (int j = 0; j < k.copies; ++j) *reinterpret_cast<uint4*>(dst + j * 64) = x;
}

__device__ __forceinline__ void gqa_unpack(const uint4& r, float* f) {  // 8 bf16 -> 8 fp32 (exact)
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__global__ __launch_bounds__(256) void gqa_reduce_kernel(const uint16_t* __restrict__ wide, int64_t ldw,
                                                         uint16_t* __restrict__ compact, int64_t ldc, int64_t rows,
                                                         int H, int Hkv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = (H + 2 * Hkv) * 8;
  const int64_t row = i / per_row;
  if (row >= rows) return;
  const int r = (int)(i - row * per_row), slot = r >> 3, c = r & 7;
  const GqaChunk k = gqa_chunk(slot, c, H, Hkv);
  const uint16_t* src = wide + row * ldw + k.wide_col;
  uint4 x = *reinterpret_cast<const uint4*>(src);
  if (k.copies > 1) {
    float acc[8];
    gqa_unpack(x, acc);
    for (int j = 1; j < k.copies; ++j) {  // ascending head order, one fp32 rounding per addition
      float f[8];
      gqa_unpack(*reinterpret_cast<const uint4*>(src + j * 64), f);
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[d] += f[d];
    }
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
      o[d] = (uint32_t)f32_to_bf16(acc[2 * d]) | ((uint32_t)f32_to_bf16(acc[2 * d + 1]) << 16);
    x = make_uint4(o[0], o[1], o[2], o[3]);
  }
  *reinterpret_cast<uint4*>(compact + row * ldc + slot * 64 + c * 8) = x;
}

static dim3 gqa_grid(int64_t rows, int H, int Hkv) {
  const int64_t lanes = rows * (H + 2 * Hkv) * 8;
  return dim3((unsigned)((lanes + 255) / 256));
}

void launch_gqa_expand(const uint16_t* compact, int64_t ldc, uint16_t* wide, int64_t ldw, int64_t rows, int H, int Hkv,
                       hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(gqa_expand_kernel, gqa_grid(rows, H, Hkv), dim3(256), 0, st, compact, ldc, wide, ldw, rows, H,
                     Hkv);
}

void launch_gqa_reduce(const uint16_t* wide, int64_t ldw, uint16_t* compact, int64_t ldc, int64_t rows, int H, int Hkv,
                       hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(gqa_reduce_kernel, gqa_grid(rows, H, Hkv), dim3(256), 0, st, wide, ldw, compact, ldc, rows, H,
                     Hkv);
}

}  // namespace mlt
