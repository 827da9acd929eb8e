// mctq_codes_softmax.hpp -- the score-to-probability arithmetic of the softmax on codes, one 16-byte chunk of a row at a time,
// shared by mctq_codes_softmax.hip (rows in global memory) and mctq_qattention.hip (rows in LDS).  The contract is in
// mctq_codes_softmax.hip's header: cmax, S = sum E[cmax - c] (an exact integer), p = float32(E) / float32(S), ql_code(p).
// Byte j of a chunk is an element of the row where lo <= j < hi.
#pragma once
#include "mctq_consumer.hpp"               // u32x4, QlOut, ql_code

namespace mctq {

// pass 1: the chunk's codes as unsigned bytes (pre-table, sign flip), bytes outside the row 0; mx takes their max
template <bool PRE>
__device__ __forceinline__ void softmax_chunk_order(u32x4& v, const uint8_t* __restrict__ pre8, uint32_t flip, int lo, int hi,
                                                    uint32_t& mx) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t w = v[q];
    uint32_t packed = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * q + b;
      uint32_t c = (w >> (8 * b)) & 0xffu;
      if (PRE) c = pre8[c];
      c = (j >= lo && j < hi) ? (c ^ flip) : 0u;
      mx = max(mx, c);
      packed |= c << (8 * b);
    }
    v[q] = packed;
  }
}

// pass 2: the chunk's sum of E[cmax - c] over the bytes inside the row (16 * 2^24 < 2^32)
__device__ __forceinline__ uint32_t softmax_chunk_sum(const u32x4& v, const uint32_t* etab, uint32_t mx, int lo, int hi) {
  uint32_t part = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t c = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
    part += (j >= lo && j < hi) ? etab[mx - c] : 0u;
  }
  return part;
}

// pass 3: one division per element, 16 codes (bytes outside the row: some code, never kept)
__device__ __forceinline__ u32x4 softmax_chunk_codes(const u32x4& v, const uint32_t* etab, uint32_t mx, float fs, const QlOut& o) {
  u32x4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t c = (v[q] >> (8 * b)) & 0xffu;
      const float p = (float)etab[mx - c] / fs;
      word |= ((uint32_t)ql_code(p, o) & 0xffu) << (8 * b);
    }
    r[q] = word;
  }
  return r;
}

// the chunk's first nv (0 .. 16) bytes as they are, the rest pad (pad_code in all four bytes)
__device__ __forceinline__ u32x4 softmax_chunk_pad(const u32x4& codes, int nv, uint32_t pad) {
  u32x4 w;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int nb = min(max(nv - 4 * q, 0), 4);
    const uint32_t keep = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
    w[q] = (codes[q] & keep) | (pad & ~keep);
  }
  return w;
}

}  // namespace mctq
