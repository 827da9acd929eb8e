// mctq_qmatmul.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Batched matrix product of two activation-code tensors (holder x holder: the Q.K^T and P.V products of an attention block) on
// the integer matrix cores (v_mfma_i32_16x16x64_i8), a direct kernel in the style of mctq_qconv_grouped.hip:
//     acc[m][n] = sum over k < K of (a[m][k] - za) * (b[k][n] - zb)          y = float(acc) * (sa * sb)
// per batch (b0, b1), with the output forms of the other consumers (QlOut); no bias, no residual, no activation.
//
// Operands by strides: each is a [B0][B1][rows][cols] view with element (= byte) strides for B0, B1 and rows and unit stride on
// cols; a batch stride of 0 broadcasts.  A is [M][K].  B is [N][K] in the NT form (transposed_b: Q.K^T) and [K][N] in the NN form
// (P.V).  The output is contiguous [B0][B1][M][N].
//
// Wave tile: 16 rows x up to 4 N tiles of 16 columns.  Per K step of 64 the A fragment of lane l is the 16 bytes
// k = 16 * (l >> 4) .. + 15 of row l & 15, a B fragment the same bytes of column l & 15; in the result the column is l & 15 and
// the row 4 * (l >> 4) + reg (mctq_qlinear.hip).  Block: 256 threads = 4 waves = 64 rows of one N slice of 64 columns.  Grid x =
// ceil(M / 64), y = ceil(N / 64), z = B0 * B1.  No atomics, no split-K: every output element is written by exactly one lane.
// Rows beyond M and columns beyond N are computed from clamped indices and not stored.
//
// K-contiguous operands (A in both forms, B in the NT form) are read in whole aligned 16-byte chunks up to Kp = 16 * ceil(K / 16):
// the caller guarantees that bytes K .. Kp - 1 of every row exist and hold that operand's zero-point code.  A chunk beyond Kp
// inside the last K step is loaded from the row's last chunk (a valid address) and replaced by zero-point bytes by select.
//
// NN form: the MFMA wants 16 consecutive k per lane and B is [K][N] with N contiguous (N % 16 == 0), so each K step's 64 x 64
// tile of B is transposed through LDS, shared by the block's four waves.  Form chosen: every thread loads one dword (4
// consecutive n) of each of 4 consecutive k rows (16 lanes cover 64 contiguous bytes of a row), transposes the 4 x 4 bytes
// in registers (six v_perm_b32), and writes four dwords, each the bytes k .. k + 3 of one column; rows k >= K are loaded from
// row K - 1 and replaced by zero-point bytes.  LDS image: [kb = k / 16][n][16 bytes], 4 x 64 x 16 = 4096 bytes, pitch 16 bytes
// per column and 1024 per kb, no padding.  A fragment is one ds_read_b128 at kb * 1024 + n * 16: the instruction serves lanes
// in four groups of 16, each group the rows {0-3, 12-15} of one kb and the rows {4-11} of its neighbour; 1024 is a multiple of
// the 256-byte bank row, so a group's 16 lanes read the 16 different 16-byte slots n & 15 -- all 64 banks once, no conflict.  The
// ds_write_b32 of column 4 * nq + j, dword kq & 3, goes to bank 16 * (nq & 1) + 4 * j + (kq & 3) of 32: with the same j in all
// lanes only 4 banks would be hit by a group of 32 lanes (8-way).  So lane nq writes its columns in the rotated order
// j' = (j + (nq >> 1)) & 3: 2 x 4 x 2 = 16 banks, each hit by two lanes (nq and nq + 8) -- a 2-way conflict, which costs a
// ds_write_b32 no cycle.  Two barriers per K step (single buffer); the next step's global loads are in flight meanwhile.
//
// Both zero points, exactly.  uint8 codes are xor-ed with 0x80 into int8 (z' = z - 128), as in mctq_qlinear.hip.  With the padded
// positions holding za' / zb', over the Kp64 = 64 * ceil(K / 64) columns the kernel multiplies,
//     sum_{k < K} (a - za)(b - zb) = sum a'b' - za' * colsum_b'[n] - zb' * rowsum_a'[m] + Kp64 * za' * zb'.
// The row sums are one more MFMA per K step against a B fragment of ones (every column of that result holds the row's sum:
// each lane finds the sums of its four rows in its own registers), the column sums one more MFMA per N tile with an A
// fragment of ones (every row holds the column's sum: each lane finds its column's sum in its own registers).  Either is
// skipped when that zero point z' is 0 (template flags ZA / ZB).  All terms are added in wrapping arithmetic (ql_corrected's
// rule): each reaches 2^30 and only their total, |sum| <= 255 * 255 * 32768 < 2^31, is known to fit.
//
// Compiled resources (hipcc -O3 --offload-arch=gfx950 with the library's flags; scratch 0 bytes in every instantiation):
//     <ZA, ZB>            NT: VGPRs  LDS bytes        NN: VGPRs  LDS bytes
//     <false, false>           92        0                 68      4096
//     <false, true>           100        0                 72      4096
//     <true,  false>          128        0                104      4096
//     <true,  true>           132        0                108      4096
// Nobody has measured a speed for this kernel against a tuned library product; tools/matmul_consumer_probe.py compares the
// launch with the float32 chain it replaces.
#include "mctq_consumer.hpp"

namespace mctq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct MatmulArgs {
  const uint8_t* a;
  const uint8_t* b;
  void* y;
  int64_t a_s0, a_s1, a_sr, b_s0, b_s1, b_sr;      // byte strides of B0, B1 and rows
  FastDiv b1;                                      // blockIdx.z = b0 * B1 + b1
  uint32_t M, N;
  int32_t K, Kp, Kp64;                             // Kp = 16 * ceil(K / 16), Kp64 = 64 * ceil(K / 64)
  uint32_t flip_a, flip_b;                         // 0x80808080 for uint8 codes, else 0
  uint32_t pad_a, pad_b;                           // the zero-point code in all four bytes (before the flip)
  int32_t zap, zbp;                                // za', zb'
  float scale;                                     // sa * sb
  QlOut oq;
};

// The 16 bytes of K chunk c (16 * c < Kp64) of a K-contiguous row: beyond the row's last chunk the pad bytes.
__device__ __forceinline__ i32x4 matmul_k_chunk(const uint8_t* __restrict__ row, int c, int last, uint32_t pad4) {
  const i32x4 v = *reinterpret_cast<const i32x4*>(row + 16 * min(c, last));
  const int p = (int)pad4;
  return c <= last ? v : i32x4{p, p, p, p};
}

template <bool ZA, bool ZB, bool NN>
__global__ __launch_bounds__(kThreads) void qmatmul_kernel(MatmulArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kb = lane >> 4;
  const uint32_t m0 = blockIdx.x * 64u + (uint32_t)wave * 16u;      // < M + 64 <= 2^31
  if constexpr (!NN) {
    if (m0 >= a.M) return;                                          // an idle wave of the last block (NT: no barrier below)
  }
  uint32_t bi1;
  const uint32_t bi0 = a.b1.divmod(blockIdx.z, bi1);
  const uint8_t* __restrict__ ga = a.a + (int64_t)bi0 * a.a_s0 + (int64_t)bi1 * a.a_s1;
  const uint8_t* __restrict__ gb = a.b + (int64_t)bi0 * a.b_s0 + (int64_t)bi1 * a.b_s1;
  const uint32_t n0 = blockIdx.y * 64u;
  const int nt = (int)min(4u, (a.N - n0 + 15u) / 16u);              // N tiles of this slice: 1 .. 4, uniform over the block
  const int last = a.Kp / 16 - 1;                                   // the last chunk of a K-contiguous row

  // this lane's row of the A fragment, clamped: rows beyond M are computed, never stored
  const uint8_t* __restrict__ arow = ga + (int64_t)min(m0 + (uint32_t)r, a.M - 1) * a.a_sr;

  i32x4 acc[4], cs[4], rs = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) { acc[t] = i32x4{0, 0, 0, 0}; cs[t] = i32x4{0, 0, 0, 0}; }
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const int fa = (int)a.flip_a, fb = (int)a.flip_b;

  if constexpr (!NN) {
    // NT: B rows are K-contiguous like A's.  Column 64 * slice + 16 * t + r, clamped.
    const uint8_t* brow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) brow[t] = gb + (int64_t)min(n0 + 16u * t + (uint32_t)r, a.N - 1) * a.b_sr;
    // K steps of 64: the next step's fragments are in flight while this one multiplies
    i32x4 av = matmul_k_chunk(arow, kb, last, a.pad_a), bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bv[t] = t < nt ? matmul_k_chunk(brow[t], kb, last, a.pad_b) : i32x4{0, 0, 0, 0};
    for (int32_t k0 = 0; k0 < a.Kp64; k0 += 64) {
      i32x4 av_next = av, bv_next[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) bv_next[t] = bv[t];
      if (k0 + 64 < a.Kp64) {
        const int c = (k0 + 64) / 16 + kb;
        av_next = matmul_k_chunk(arow, c, last, a.pad_a);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < nt) bv_next[t] = matmul_k_chunk(brow[t], c, last, a.pad_b);
      }
      av = av ^ fa;                                                 // u8 code c -> int8 (c - 128); z' carries the -128
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nt) {
          const i32x4 b8 = bv[t] ^ fb;
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b8, acc[t], 0, 0, 0);
          if constexpr (ZA) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b8, cs[t], 0, 0, 0);   // every row: the column's sum of b'
        }
      }
      if constexpr (ZB) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, ones, rs, 0, 0, 0);             // every column: the row's sum of a'
      av = av_next;
#pragma unroll
      for (int t = 0; t < 4; ++t) bv[t] = bv_next[t];
    }
  } else {
    // NN: the 64 (k) x 64 (n) tile of B through LDS, [kb][n][16 bytes] (the file header).
    __shared__ __attribute__((aligned(16))) uint32_t tile[4 * 64 * 4];
    const int kq = threadIdx.x >> 4, nq = threadIdx.x & 15;         // this thread's 4 k rows and 4 columns of the tile
    const int rot = (nq >> 1) & 3;
    // columns beyond N: the slice's last whole dword inside the row (N % 16 == 0: N - 4 >= n0), never stored
    const uint8_t* __restrict__ bcol = gb + min(n0 + 4u * (uint32_t)nq, a.N - 4u);
    auto load_b = [&](int32_t k0, uint32_t (&raw)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int32_t k = k0 + 4 * kq + i;
        const uint32_t v = *reinterpret_cast<const uint32_t*>(bcol + (int64_t)min(k, a.K - 1) * a.b_sr);
        raw[i] = k < a.K ? v : a.pad_b;                             // rows behind K hold zb: they add (a - za) * 0
      }
    };
    uint32_t raw[4];
    load_b(0, raw);
    i32x4 av = matmul_k_chunk(arow, kb, last, a.pad_a);
    for (int32_t k0 = 0; k0 < a.Kp64; k0 += 64) {
      i32x4 av_next = av;
      uint32_t raw_next[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) raw_next[i] = raw[i];
      if (k0 + 64 < a.Kp64) {
        av_next = matmul_k_chunk(arow, (k0 + 64) / 16 + kb, last, a.pad_a);
        load_b(k0 + 64, raw_next);
      }
      // 4 x 4 byte transpose: raw[i] = bytes (n .. n + 3) of row k + i  ->  o[j] = bytes (k .. k + 3) of column n + j
      const uint32_t t0 = __builtin_amdgcn_perm(raw[1], raw[0], 0x05010400u), t1 = __builtin_amdgcn_perm(raw[1], raw[0], 0x07030602u);
      const uint32_t t2 = __builtin_amdgcn_perm(raw[3], raw[2], 0x05010400u), t3 = __builtin_amdgcn_perm(raw[3], raw[2], 0x07030602u);
      uint32_t o0 = __builtin_amdgcn_perm(t2, t0, 0x05040100u), o1 = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
      uint32_t o2 = __builtin_amdgcn_perm(t3, t1, 0x05040100u), o3 = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
      if (rot & 1) { const uint32_t s = o0; o0 = o1; o1 = o2; o2 = o3; o3 = s; }        // o_j <- column (j + rot) & 3
      if (rot & 2) { uint32_t s = o0; o0 = o2; o2 = s; s = o1; o1 = o3; o3 = s; }
      uint32_t* const wr = tile + (kq >> 2) * 256 + 16 * nq + (kq & 3);
      __syncthreads();                                              // the step before has read its fragments
      wr[4 * (rot & 3)] = o0;
      wr[4 * ((1 + rot) & 3)] = o1;
      wr[4 * ((2 + rot) & 3)] = o2;
      wr[4 * ((3 + rot) & 3)] = o3;
      __syncthreads();
      av = av ^ fa;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nt) {
          const i32x4 b8 = *reinterpret_cast<const i32x4*>(tile + kb * 256 + (16 * t + r) * 4) ^ fb;
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b8, acc[t], 0, 0, 0);
          if constexpr (ZA) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b8, cs[t], 0, 0, 0);
        }
      }
      if constexpr (ZB) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, ones, rs, 0, 0, 0);
      av = av_next;
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[i] = raw_next[i];
    }
  }

  // epilogue: column l & 15 of every tile, rows 4 * (l >> 4) + i.  Wrapping arithmetic: only the total is known to fit.
  const unsigned tail = (unsigned)a.Kp64 * (unsigned)a.zap * (unsigned)a.zbp;   // what the Kp64 columns hold where a == za, b == zb
  const uint32_t mrow = m0 + 4u * (uint32_t)kb;
  const int64_t ybase = (int64_t)blockIdx.z * a.M;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      const uint32_t n = n0 + 16u * t + (uint32_t)r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned c = 0u - tail;
        if constexpr (ZA) c += (unsigned)a.zap * (unsigned)cs[t][i];
        if constexpr (ZB) c += (unsigned)a.zbp * (unsigned)rs[i];
        const float out = (float)(int)((unsigned)acc[t][i] - c) * a.scale;
        const uint32_t m = mrow + (uint32_t)i;
        if (m < a.M && n < a.N) ql_store(a.y, (ybase + m) * a.N + n, out, a.oq);
      }
    }
  }
}

template <bool ZA, bool ZB>
static void launch_qmatmul(const MatmulArgs& a, bool nn, dim3 grid, hipStream_t stream) {
  if (nn) hipLaunchKernelGGL((qmatmul_kernel<ZA, ZB, true>), grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL((qmatmul_kernel<ZA, ZB, false>), grid, dim3(kThreads), 0, stream, a);
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

using namespace mctq;

extern "C" {

int mctq_qmatmul_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale, int64_t a_stride_b0,
                    int64_t a_stride_b1, int64_t a_stride_row, const void* b_codes, int32_t b_code_dtype, int32_t b_zero_point,
                    float b_scale, int64_t b_stride_b0, int64_t b_stride_b1, int64_t b_stride_row, int32_t transposed_b, void* y,
                    int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                    int64_t batch0, int64_t batch1, int64_t m, int64_t n, int64_t k, void* stream) {
  if (int rc = form_check(a_code_dtype, a_zero_point, a_scale, {"a_code_dtype", "a_zero_point", "a_code_dtype", "a_scale"})) return rc;
  if (int rc = form_check(b_code_dtype, b_zero_point, b_scale, {"b_code_dtype", "b_zero_point", "b_code_dtype", "b_scale"})) return rc;
  if (batch0 < 0 || batch1 < 0 || m < 0 || n < 0) return fail_arg("negative extent");
  constexpr int64_t kMaxK = 1 << 15;
  if (k < 1 || k > kMaxK) return fail_arg("K outside 1 .. 32768: outside the consumer's limit");
  MatmulArgs a;
  if (int rc = ql_output_form(a.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  const bool nn = transposed_b == 0;
  if (nn && n % 16 != 0) return fail_arg("N must be a multiple of 16 where b is [K, N] (transposed_b == 0)");
  if (m > INT32_MAX - 64 || n > 65535ll * 64) return fail_arg("M or N too large for one launch");
  if (batch0 > 65535 || batch1 > 65535 || batch0 * batch1 > 65535)
    return fail_arg("batch0 * batch1 > 65535: too many grid slices (split the batch)");
  const int64_t kp = (k + 15) / 16 * 16, kp64 = (k + 63) / 64 * 64;
  int64_t a_span = 0, b_span = 0;
  if (int rc = matmul_view_check("a_codes", a_stride_b0, a_stride_b1, a_stride_row, batch0, batch1, m, kp, a_span)) return rc;
  if (int rc = matmul_view_check("b_codes", b_stride_b0, b_stride_b1, b_stride_row, batch0, batch1, nn ? k : n, nn ? n : kp, b_span))
    return rc;
  if (batch0 == 0 || batch1 == 0 || m == 0 || n == 0) return 0;                                       // nothing to write
  if (m > INT64_MAX / 4 / n / (batch0 * batch1)) return fail_arg("the output exceeds 2^63 - 1 bytes");
  if (!a_codes || !b_codes || !y) return fail_arg("NULL pointer");
  if ((((uintptr_t)a_codes | (uintptr_t)b_codes | (uintptr_t)y) & 15u) != 0) return fail_arg("codes and output must be 16-byte aligned");
  const size_t y_bytes = (size_t)(batch0 * batch1 * m * n) * (a.oq.mode == 0 ? 4 : 1);
  if (ranges_overlap(y, y_bytes, a_codes, (size_t)a_span) || ranges_overlap(y, y_bytes, b_codes, (size_t)b_span))
    return fail_arg("the output overlaps an operand");
  const bool a_u8 = a_code_dtype == MCTQ_CODE_U8, b_u8 = b_code_dtype == MCTQ_CODE_U8;
  a.a = static_cast<const uint8_t*>(a_codes); a.b = static_cast<const uint8_t*>(b_codes); a.y = y;
  a.a_s0 = a_stride_b0; a.a_s1 = a_stride_b1; a.a_sr = a_stride_row;
  a.b_s0 = b_stride_b0; a.b_s1 = b_stride_b1; a.b_sr = b_stride_row;
  a.b1 = FastDiv::make((uint32_t)batch1);
  a.M = (uint32_t)m; a.N = (uint32_t)n; a.K = (int32_t)k; a.Kp = (int32_t)kp; a.Kp64 = (int32_t)kp64;
  a.flip_a = a_u8 ? 0x80808080u : 0u; a.flip_b = b_u8 ? 0x80808080u : 0u;
  a.pad_a = (uint32_t)(a_zero_point & 0xff) * 0x01010101u; a.pad_b = (uint32_t)(b_zero_point & 0xff) * 0x01010101u;
  a.zap = a_u8 ? a_zero_point - 128 : a_zero_point; a.zbp = b_u8 ? b_zero_point - 128 : b_zero_point;
  a.scale = a_scale * b_scale;                                                                        // one float32 multiply
  const dim3 grid((unsigned)((m + 63) / 64), (unsigned)((n + 63) / 64), (unsigned)(batch0 * batch1));
  const hipStream_t s = (hipStream_t)stream;
  const bool za = a.zap != 0, zb = a.zbp != 0;
  if (za) { if (zb) launch_qmatmul<true, true>(a, nn, grid, s); else launch_qmatmul<true, false>(a, nn, grid, s); }
  else { if (zb) launch_qmatmul<false, true>(a, nn, grid, s); else launch_qmatmul<false, false>(a, nn, grid, s); }
  static const char* const kOps[4] = {"i8 x i8", "u8 x i8", "i8 x u8", "u8 x u8"};
  note_launch(nn ? "qmatmul_nn" : "qmatmul_nt", kOps[(a_u8 ? 1 : 0) + (b_u8 ? 2 : 0)], (za ? 1 : 0) + (zb ? 2 : 0), 0, 1,
              a.oq.mode == 0 ? 4 : 1);
  return check_launch("mctq_qmatmul_i8");
}

}  // extern "C"
