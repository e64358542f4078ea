// Philox4x32-10 counter-based generator and the dropout mask built on it.
//
// One definition for every kernel that drops elements and for the torch oracle
// (ml_trainer_amd/ops/dropout.py): flat element e = row * D + col of a [rows, D] tensor at
// dropout site `site` takes word (e & 3) of
//   philox4x32_10(counter = (lo32(e >> 2), hi32(e >> 2), site, rank), key = (lo32(seed), hi32(seed)))
// and is kept iff word >= thr, thr = min(int(p * 2^32), 0xFFFFFFFF). One call serves one aligned
// 4-element vector (the ushort4 of the LayerNorm kernels). Nothing is stored: forward and
// backward recompute the same words. Plain integer arithmetic, so the same code runs on the host.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // a HIP translation unit; plain C++ (the bindings, host tests) takes the inline form
#define MLT_HD __host__ __device__ __forceinline__
#else
#define MLT_HD inline
#endif

namespace mlt {

struct Philox4 {
  uint32_t x, y, z, w;
};

// threshold / scale / stream of one dropout site (host-made, passed by value to the kernels)
struct DropArgs {
  uint32_t thr;      // keep iff word >= thr
  float scale;       // 1 / (1 - p), rounded once from double
  uint32_t seed_lo, seed_hi;
  uint32_t site, rank;
};

MLT_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// the four random words of the vector holding flat elements 4 * vec .. 4 * vec + 3
MLT_HD Philox4 drop_words(uint64_t vec, const DropArgs& d) {
  return philox4x32_10((uint32_t)vec, (uint32_t)(vec >> 32), d.site, d.rank, d.seed_lo, d.seed_hi);
}

// Attention-probability dropout (the flash attention kernels): one BYTE per element, one call per
// 4 x 4 tile of (query, key). With T = ceil(S / 4) and
//   vec = ((b * H + h) * T + (q >> 2)) * T + (k >> 2),
// element (b, h, q, k) takes byte (k & 3) (little-endian) of word (q & 3) of drop_words(vec) at
// site 0x40000000 + layer, and is kept iff byte >= thr8, thr8 = round(p * 256). The probability
// applied is p_eff = thr8 / 256 and kept probabilities are scaled by 1 / (1 - p_eff).
struct AttnDropArgs {
  uint32_t thr8 = 0;  // keep iff byte >= thr8; 0 = no dropout (the plain kernels are launched)
  float scale = 1.f;  // 1 / (1 - thr8 / 256), rounded once from double
  uint32_t seed_lo = 0, seed_hi = 0;
  uint32_t site = 0, rank = 0;
  uint32_t T = 0;     // ceil(S / 4): tiles per row of the S x S matrix
};

// index of the first tile (key tile 0) of tile row qt = q >> 2 of (batch * H + head) bh
MLT_HD uint64_t attn_drop_row(const AttnDropArgs& a, uint32_t bh, uint32_t qt) {
  return ((uint64_t)bh * a.T + qt) * a.T;
}

// the four words of tile `vec`: word j = query 4 qt + j, its byte c = key 4 kt + c
MLT_HD Philox4 attn_drop_words(uint64_t vec, const AttnDropArgs& a) {
  return philox4x32_10((uint32_t)vec, (uint32_t)(vec >> 32), a.site, a.rank, a.seed_lo, a.seed_hi);
}

// the element rule
MLT_HD bool attn_drop_keep(const AttnDropArgs& a, uint32_t bh, uint32_t q, uint32_t k) {
  const Philox4 w = attn_drop_words(attn_drop_row(a, bh, q >> 2) + (k >> 2), a);
  const uint32_t word = (q & 3) == 0 ? w.x : (q & 3) == 1 ? w.y : (q & 3) == 2 ? w.z : w.w;
  return ((word >> (8 * (k & 3))) & 0xFFu) >= a.thr8;
}

}  // namespace mlt
