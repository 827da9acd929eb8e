// mctq_qmatmul.hpp -- what the products of two code tensors share (mctq_qmatmul.hip, mctq_qattention.hip): the fragment load of a
// K-contiguous row, the 4 x 4 byte transpose of the NN form's tile and the host check of an operand given by strides.
#pragma once
#include "mctq_consumer.hpp"

namespace mctq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The 16 bytes of K chunk c (16 * c < Kp64) of a K-contiguous row: beyond the row's last chunk the pad bytes.
__device__ __forceinline__ i32x4 matmul_k_chunk(const uint8_t* __restrict__ row, int c, int last, uint32_t pad4) {
  const i32x4 v = *reinterpret_cast<const i32x4*>(row + 16 * min(c, last));
  const int p = (int)pad4;
  return c <= last ? v : i32x4{p, p, p, p};
}

// 4 x 4 byte transpose (six v_perm_b32): raw[i] = bytes (n .. n + 3) of row k + i  ->  bytes (k .. k + 3) of column n + j, and
// then the rotated write order of the tile (mctq_qmatmul.hip's header): o[j] <- column (j + rot) & 3.
__device__ __forceinline__ void matmul_transpose4(const uint32_t (&raw)[4], int rot, uint32_t (&o)[4]) {
  const uint32_t t0 = __builtin_amdgcn_perm(raw[1], raw[0], 0x05010400u), t1 = __builtin_amdgcn_perm(raw[1], raw[0], 0x07030602u);
  const uint32_t t2 = __builtin_amdgcn_perm(raw[3], raw[2], 0x05010400u), t3 = __builtin_amdgcn_perm(raw[3], raw[2], 0x07030602u);
  uint32_t o0 = __builtin_amdgcn_perm(t2, t0, 0x05040100u), o1 = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  uint32_t o2 = __builtin_amdgcn_perm(t3, t1, 0x05040100u), o3 = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
  if (rot & 1) { const uint32_t s = o0; o0 = o1; o1 = o2; o2 = o3; o3 = s; }        // o_j <- column (j + rot) & 3
  if (rot & 2) { uint32_t s = o0; o0 = o2; o2 = s; s = o1; o1 = o3; o3 = s; }
  o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

// One operand view: strides are non-negative multiples of 16 bytes, a row holds at least `row_bytes`; `span`: the bytes from the
// pointer to the end of the last row the kernel reads.
static int matmul_view_check(const char* who, int64_t s0, int64_t s1, int64_t sr, int64_t b0, int64_t b1, int64_t rows,
                             int64_t row_bytes, int64_t& span) {
  if (s0 < 0 || s1 < 0 || sr < 0) return fail_words(who, ": negative stride");
  if (((s0 | s1 | sr) & 15) != 0) return fail_words(who, ": the batch and row strides must be multiples of 16 bytes");
  if (rows > 1 && sr < row_bytes) return fail_words(who, ": the row stride is shorter than a row (padded to whole 16-byte chunks)");
  // (b0, b1 <= 65535, rows < 2^31, row_bytes <= 2^31: each product below stays inside int64 once the strides are below 2^40)
  if (s0 > (1ll << 40) || s1 > (1ll << 40) || sr > (1ll << 31)) return fail_words(who, ": stride too large");
  span = (b0 - 1) * s0 + (b1 - 1) * s1 + (rows - 1) * sr + row_bytes;
  return 0;
}

}  // namespace mctq
