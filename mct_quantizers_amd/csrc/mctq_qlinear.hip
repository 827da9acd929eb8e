// mctq_qlinear.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Integer consumer of the quantizers' codes: y = dequant(A) . dequant(W)^T + bias computed on the 8-bit
// clamp indices the fake-quant kernels would have dequantized (mctq_fq_codes_*), with the gfx950 integer
// matrix cores (v_mfma_i32_16x16x64_i8) and exact int32 accumulation:
//     y[m][n] = float( sum_k (qa[m][k] - za) * qw[n][k] ) * (sa * sw[n]) + bias[n]
// For the small batches of inference the product is bound by streaming the weight codes once (1 B per weight
// instead of re-quantizing 4 B -> 4 B and then reading 4 B again in an fp32 GEMM), so the layout serves the
// memory system first: both operands are K-contiguous, per 256-byte K block every lane fetches four
// 16-byte pieces of one row, the four lanes of a row covering one 64-byte sector per load instruction (the
// pieces feed four MFMA steps; A and B use the same k assignment, which is all an exact integer sum needs), the 8 waves of a block interleave K blocks so that a row is read in 2 KiB
// runs, and the partial sums meet in LDS.  One block = 16 output columns x all rows x all of K; no split-K
// atomics, so the result does not depend on scheduling.
#include "mctq_consumer.hpp"

namespace mctq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kQlKBlock = 256;          // bytes of K per wave step: 4 lane groups x 64 B
extern int g_ql_variant;                // tuning hook "ql_variant": 0 = automatic
// what the calling thread launched last (mctq_last_launch): "qlinear_<kernel>_<tile>" with the code widths
template <bool A_U8>
static void note_ql(const char* shape, int u = 0, bool zp = false, const QlRes* res = nullptr) {   // zp: the form with weight zero points ran
  const char* op = zp ? (A_U8 ? "u8 x i8 zp" : "i8 x i8 zp") : (A_U8 ? "u8 x i8" : "i8 x i8");
  if (res && res->mode) {                 // the residual form ran: "u8 x i8 res(u8) relu"
    static thread_local char op_text[40];
    snprintf(op_text, sizeof(op_text), "%s res(%s)%s", op, res->mode == 1 ? "f32" : res->mode == 2 ? "i8" : "u8",
             res->relu ? " relu" : "");
    op = op_text;
  } else if (res && res->act) {           // the activation form ran (mctq_qlinear_i8_act): "u8 x i8 hardswish"
    static thread_local char op_text[40];
    snprintf(op_text, sizeof(op_text), "%s%s", op, res->act == 1 ? " hardswish" : " hardsigmoid");
    op = op_text;
  }
  note_launch(shape, op, u, 0, 1, 4);
}
extern int g_ql_stagger;                // tuning hook "ql_stagger": half of the tiled kernel's waves copy after multiplying (default off)
extern int g_ql_rot;                    // tuning hook "ql_rot": K rotation between the blocks that share a weight tile (default off)
extern int g_ql_band;                   // tuning hook "ql_band": tile rows per band of the tiled kernel, 0 = automatic

// (QlOut, ql_store and ql_output_form -- the output form of a consumer launch -- live in mctq_consumer.hpp, shared with
// mctq_qconv_dw.hip.)

// Weight zero points (uniform weights, mctq_qlinear_*_zp): per output channel zw[n] in the domain of the int8 codes, and
// per activation row a_rowsum[m] = sum_k (a[m][k] - za) (mctq_codes_rowsum).  Then
//     sum_k (a - za) (w - zw[n]) = sum_k a w - za w_rowsum[n] - zw[n] a_rowsum[m]:
// the kernels' sum and first correction, plus one product per output in the epilogue.  Both pointers null (every other
// entry point): the branch on them is uniform and the epilogue is the one it was.  The terms reach 2^30 each and it is
// their total that is known to fit int32 (255 * 255 * 32768 < 2^31), so they are added in wrapping (unsigned) arithmetic.
struct QlZp {
  const int32_t* w_zero_points;
  const int32_t* a_rowsum;
};
__device__ __forceinline__ int ql_corrected(int acc, int corr, int zw, const QlZp& zp, int m) {
  unsigned c = (unsigned)corr;
  if (zp.a_rowsum) c += (unsigned)zw * (unsigned)zp.a_rowsum[m];
  return (int)((unsigned)acc - c);
}
// Two kernels decide at compile time instead (template flag ZP: qlinear_i8_lds_kernel and qgemm_i8_glds_kernel).  With the
// run-time test they lost more than a build's spread against itself on mctq_qlinear_i8 (profiles/EXPERIMENTS.md: +3.3 % at
// 16 x 4096 x 4096, +2.2 % at 256 x 4096 x 4096), so their ZP = false form is the kernel without zero points, and the
// ZP = true form is instantiated only by the launchers, for a call that brings zero points.
template <bool ZP>
__device__ __forceinline__ int ql_corrected(int acc, int corr, int zw, const QlZp& zp, int m) {
  if constexpr (ZP) return (int)((unsigned)acc - ((unsigned)corr + (unsigned)zw * (unsigned)zp.a_rowsum[m]));
  else return acc - corr;
}

// The streaming kernels' epilogue column of this thread (== en at their top), recomputed behind a statement the compiler
// cannot move: the address of the zero point would otherwise be hoisted out of the loop over row tiles and stay in two
// registers across the K loop of every launch, zero points or not.  The barrier is an empty asm statement, which binds
// the compiler by convention only: after a compiler update, compile this unit with -Rpass-analysis=kernel-resource-usage
// and compare qlinear_i8_kernel's VGPR counts and scratch (0 bytes) with the figures in profiles/EXPERIMENTS.md.
__device__ __forceinline__ int ql_epilogue_column(int n0, int N) {
  int c = (int)(threadIdx.x & 15);
  asm volatile("" : "+v"(c));
  return min(n0 + c, N - 1);
}

template <bool NT>
__device__ __forceinline__ i32x4 ql_load16(const int8_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p));
  else return *reinterpret_cast<const i32x4*>(p);
}

// 4 x 16 B of one row, 64 B apart, starting at k: piece p of the four lanes that share a row covers one
// contiguous 64-byte sector.  FULL: the whole 256-byte K block lies inside K (no guards, straight-line loads);
// otherwise pieces that start at or beyond K read as zero (K % 16 == 0).
template <bool NT, bool FULL>
__device__ __forceinline__ void ql_load_row(const int8_t* row, int64_t k, int64_t K, i32x4* out) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if constexpr (FULL) {
      out[p] = ql_load16<NT>(row + k + 64 * p);
    } else {
      const i32x4 z = {0, 0, 0, 0};
      out[p] = (k + 64 * p < K) ? ql_load16<NT>(row + k + 64 * p) : z;
    }
  }
}

// 4-bit weights (W4): a row holds K / 2 bytes; each group of 8 consecutive k is one dword whose byte j carries
// code k = j in its low and k = j + 4 in its high nibble (two's complement).  (x << 4) & 0xF0F0F0F0 and
// x & 0xF0F0F0F0 are then the int8 values 16 * code of k = 0..3 and k = 4..7 in natural order: two VALU ops per
// 8 weights, and the factor 16 leaves again by an exact shift of the int32 sum.
typedef int i32x2 __attribute__((ext_vector_type(2)));
template <bool NT, bool FULL>
__device__ __forceinline__ void ql_load_row4(const int8_t* row, int64_t k, int64_t K, i32x2* out) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const i32x2 z = {0, 0};
    const i32x2* q = reinterpret_cast<const i32x2*>(row + (k + 64 * p) / 2);
    if (FULL || k + 64 * p < K) out[p] = NT ? __builtin_nontemporal_load(q) : *q;
    else out[p] = z;
  }
}
__device__ __forceinline__ i32x4 ql_unpack4(i32x2 x) {
  return i32x4{(x[0] << 4) & (int)0xF0F0F0F0, x[0] & (int)0xF0F0F0F0, (x[1] << 4) & (int)0xF0F0F0F0, x[1] & (int)0xF0F0F0F0};
}
__device__ __forceinline__ i32x4 ql_unpack4(i32x4 x) { return x; }       // int8 weights: nothing to do

// 4-bit codebook indices (LUT4): the W4 layout with UNSIGNED nibbles 0..15 that index 16 int8 codebook values.  The
// codebook travels in the kernel arguments (four dwords, entry j in byte j % 4 of t[j / 4]): no device read joins the
// dependency chain.  v_perm_b32 D, S0, S1, sel picks byte sel (0..3: of S1, 4..7: of S0) per result byte, so index & 7
// looks up entries 0..7 in {t[1], t[0]} and entries 8..15 in {t[3], t[2]}; bit 3 of the index, spread to a byte mask
// (0x08 << 5) - (0x08 >> 3) = 0xFF per byte, chooses between the two: about two VALU operations per weight.
struct QlLut { int t[4]; };
__device__ __forceinline__ int ql_lut_bytes(unsigned sel, unsigned mask, const QlLut& c) {
  const unsigned lo = __builtin_amdgcn_perm((unsigned)c.t[1], (unsigned)c.t[0], sel);
  const unsigned hi = __builtin_amdgcn_perm((unsigned)c.t[3], (unsigned)c.t[2], sel);
  return (int)((hi & mask) | (lo & ~mask));
}
__device__ __forceinline__ i32x4 ql_unpack_lut4(i32x2 x, const QlLut& c) {
  i32x4 out;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned v = (unsigned)x[h];
    const unsigned b_lo = v & 0x08080808u, b_hi = v & 0x80808080u;       // bit 3 of the indices of k = 0..3 / k = 4..7
    out[2 * h] = ql_lut_bytes(v & 0x07070707u, (b_lo << 5) - (b_lo >> 3), c);
    out[2 * h + 1] = ql_lut_bytes((v >> 4) & 0x07070707u, (b_hi << 1) - (b_hi >> 7), c);
  }
  return out;
}
__device__ __forceinline__ QlLut ql_lut_arg() { return QlLut{{0, 0, 0, 0}}; }
__device__ __forceinline__ QlLut ql_lut_arg(const QlLut& c) { return c; }
__device__ __forceinline__ QlRes ql_res_arg() { return QlRes{nullptr, 0, 0, 0.0f, 0, 0}; }
__device__ __forceinline__ const QlRes& ql_res_arg(const QlRes& r) { return r; }
enum { kQlW8 = 0, kQlW4 = 1, kQlLut4 = 2 };      // weight formats of the streaming kernel

// MT: 16-row tiles of A per pass (1..4).  A_U8: activation codes are uint8 (re-biased to int8 by ^0x80).
// WFMT: kQlW8 int8 weights, kQlW4 packed 4-bit codes, kQlLut4 packed 4-bit codebook indices (above); the codebook of the
// last is the kernel's one trailing argument, which the other formats do not have.
template <int kQlWaves, int MT, bool A_U8, bool W_NT, int WFMT = kQlW8, class... Lut>
__global__ __launch_bounds__(kQlWaves * 64) void qlinear_i8_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ w, const float* __restrict__ w_scales,
    const int32_t* __restrict__ w_rowsum, const float* __restrict__ bias, void* __restrict__ y,
    int M, int N, int64_t K, int za, float sa, QlOut oq, QlZp zp, Lut... lut) {
  static_assert(sizeof...(Lut) == (WFMT == kQlLut4 ? 1 : 0), "the codebook argument belongs to the LUT4 format");
  constexpr bool W4 = WFMT == kQlW4, LUT4 = WFMT == kQlLut4, HALF = W4 || LUT4;      // HALF: half a byte per weight
  constexpr int kQlThreads = kQlWaves * 64;
  __shared__ int red[kQlWaves][MT][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // rows beyond N / M are clamped to the last valid row: they are loaded and multiplied, never stored
  const int8_t* wrow = w + (int64_t)min(n0 + r, N - 1) * (HALF ? K / 2 : K);
  typedef typename std::conditional<HALF, i32x2, i32x4>::type WF;     // a weight piece as loaded
  const int64_t kblocks = (K + kQlKBlock - 1) / kQlKBlock;
  const int64_t full_blocks = K / kQlKBlock;
  // this thread's output column in the epilogue is fixed (block size % 16 == 0): fetch its constants now, not
  // at the end of the dependency chain
  const int en = min(n0 + (int)(threadIdx.x & 15), N - 1);
  const int e_corr = za * w_rowsum[en];
  const float e_scale = sa * w_scales[en];
  const float e_bias = bias ? bias[en] : 0.0f;

  for (int m0 = 0; m0 < M; m0 += 16 * MT) {
    i32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = i32x4{0, 0, 0, 0};
    const int8_t* arow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) arow[t] = a + (int64_t)min(m0 + 16 * t + r, M - 1) * K;

    WF wf0[4], wf1[4];
    i32x4 af0[MT][4], af1[MT][4];                       // two register buffers, swapped by unrolling
    // blocks walk K from different starting points so that they do not all ask L2 for the same lines of A at once
    const int64_t rot = full_blocks ? (int64_t)blockIdx.x % full_blocks : 0;
    auto fetch = [&](int64_t i, WF* wf, i32x4 (*af)[4]) {               // i-th full K block of this wave
      int64_t kblk = wave + i * kQlWaves + rot;
      if (kblk >= full_blocks) kblk -= full_blocks;
      const int64_t k = kblk * kQlKBlock + 16 * g;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#ifdef MCTQ_QL_ABLATE_A                      // timing experiment (tools/kbench_ql.hip): no activation traffic
#pragma unroll
        for (int p = 0; p < 4; ++p) af[t][p] = i32x4{t, p, t, p};
#else
        ql_load_row<false, true>(arow[t], k, K, af[t]);
#endif
      }
      if constexpr (HALF) ql_load_row4<W_NT, true>(wrow, k, K, wf);      // L2-resident activations first, the HBM stream behind them
      else ql_load_row<W_NT, true>(wrow, k, K, wf);
    };
    auto multiply = [&](const WF* wf, const i32x4 (*af)[4]) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        i32x4 wv;
        if constexpr (LUT4) wv = ql_unpack_lut4(wf[p], ql_lut_arg(lut...));
        else wv = ql_unpack4(wf[p]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          i32x4 av = af[t][p];
          if constexpr (A_U8) av = av ^ (int)0x80808080;          // u8 code c -> int8 (c - 128)
#ifdef MCTQ_QL_ABLATE_MFMA                   // timing experiment: loads only
          acc[t] += av ^ wv;
#else
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, wv, acc[t], 0, 0, 0);
#endif
        }
      }
    };
    // full K blocks wave, wave + W, ...: straight-line loads, next block in flight while this one multiplies
    const int64_t n_i = full_blocks > wave ? (full_blocks - wave + kQlWaves - 1) / kQlWaves : 0;
    int64_t i = 0;
    if (n_i > 0) fetch(0, wf0, af0);
    while (i + 2 < n_i) {
      fetch(i + 1, wf1, af1);
      multiply(wf0, af0);
      fetch(i + 2, wf0, af0);
      multiply(wf1, af1);
      i += 2;
    }
    if (n_i - i == 2) {
      fetch(i + 1, wf1, af1);
      multiply(wf0, af0);
      multiply(wf1, af1);
    } else if (n_i - i == 1) {
      multiply(wf0, af0);
    }
    if (full_blocks != kblocks && wave == kQlWaves - 1) {          // ragged end of K: guarded loads, one wave
      const int64_t k = full_blocks * kQlKBlock + 16 * g;
      if constexpr (HALF) ql_load_row4<W_NT, false>(wrow, k, K, wf0);
      else ql_load_row<W_NT, false>(wrow, k, K, wf0);
#pragma unroll
      for (int t = 0; t < MT; ++t) ql_load_row<false, false>(arow[t], k, K, af0[t]);
      if constexpr (LUT4 && A_U8) {       // a zero index decodes to lut[0], not to 0: beyond K the ACTIVATION must be the zero (code 128)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (k + 64 * p >= K) af0[t][p] = i32x4{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
        }
      }
      multiply(wf0, af0);
    }

    // partial sums of the 8 waves meet in LDS
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][t][lane][i] = acc[t][i];
    }
    __syncthreads();
    // (the zero point is fetched here and not next to e_corr: one more register live across the K loop costs the 4-bit
    // formats a wave of occupancy or a spill; only the zero-point form waits for it.  The codebook format never has one.)
    const QlZp zq = LUT4 ? QlZp{nullptr, nullptr} : zp;
    const int e_zw = zq.a_rowsum ? zq.w_zero_points[ql_epilogue_column(n0, N)] : 0;
    for (int e = threadIdx.x; e < MT * 256; e += kQlThreads) {
      const int t = e >> 8, rem = e & 255;
      const int mi = rem >> 4, ni = rem & 15;                    // row / column inside the 16 x 16 tile
      const int src_lane = (mi >> 2) * 16 + ni, src_reg = mi & 3;  // C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg
      int v = 0;
#pragma unroll
      for (int wv = 0; wv < kQlWaves; ++wv) v += red[wv][t][src_lane][src_reg];
      if constexpr (W4) v >>= 4;                                  // the weights entered as 16 * code: exact
      const int m = m0 + 16 * t + mi, n = n0 + ni;
      if (m < M && n < N) {
        float out = (float)ql_corrected(v, e_corr, e_zw, zq, m) * e_scale;
        if (bias) out = out + e_bias;
        ql_store(y, (int64_t)m * N + n, out, oq);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// The same product with the activation codes staged through per-wave LDS (ql_variant 18x, M <= 64 by default).
// In the kernel above every block re-reads ALL of A through L2 as MFMA-fragment-shaped loads: each 16-byte-per-lane
// instruction touches 16 rows x one 64-byte sector, and at M = 64 those 64 MiB of L2 traffic (256 blocks x 256 KiB)
// cost more than the 16 MiB weight stream from HBM (13.1 us vs 6.4 us without them, profiles/r01).  Here a wave
// copies its K block of A global -> LDS with global_load_lds_dwordx4: one instruction = 4 rows x 256 contiguous
// bytes (full lines; the 16-byte chunks of a row are permuted by an XOR swizzle applied on the SOURCE address, so
// the fragment reads below are bank-conflict free), then reads the fragments with ds_read_b128.  Bytes through L2
// are the same; the requests are whole lines instead of half-used sectors.  A wave owns its LDS region: no block
// barrier in the K loop, only vmcnt waits.  MT <= 2: two LDS buffers per wave (copy of block i+1 under the MFMAs of
// block i); MT = 4: one buffer (8 waves x 16 KiB).  The reduction of the 8 waves' partial sums reuses the region.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void ql_lds_void_;
typedef const __attribute__((address_space(1))) void ql_glb_void_;

// Res: empty, or one QlRes -- the residual form (mctq_qlinear_i8_res) and the activation form (mctq_qlinear_i8_act: the
// record's mode is 0 and the add is branched out), a trailing kernel argument that the other instantiations do not have; it
// is read in the epilogue only.
template <int kQlWaves, int MT, bool A_U8, bool W_NT, bool ZP = false, class... Res>
__global__ __launch_bounds__(kQlWaves * 64) void qlinear_i8_lds_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ w, const float* __restrict__ w_scales,
    const int32_t* __restrict__ w_rowsum, const float* __restrict__ bias, void* __restrict__ y,
    int M, int N, int64_t K, int za, float sa, QlOut oq, QlZp zp, Res... res) {
  static_assert(sizeof...(Res) <= 1 && !(ZP && sizeof...(Res)), "the residual form is built without weight zero points");
  constexpr bool RES = sizeof...(Res) == 1;
  constexpr int kQlThreads = kQlWaves * 64;
  constexpr int NBUF = kQlWaves * 2 * MT * 4096 <= 128 * 1024 ? 2 : 1;      // double-buffer when it fits 128 KiB
  constexpr int kSlots = MT * 256;                       // 16-byte slots of one A buffer: MT*16 rows x 16 chunks
  constexpr int kRedSlots = kQlWaves * MT * 64;          // int4 slots of the reduction
  constexpr int kLdsSlots = kQlWaves * NBUF * kSlots > kRedSlots ? kQlWaves * NBUF * kSlots : kRedSlots;
  __shared__ i32x4 lds[kLdsSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int8_t* wrow = w + (int64_t)min(n0 + r, N - 1) * K;
  const int64_t kblocks = (K + kQlKBlock - 1) / kQlKBlock;
  const int64_t full_blocks = K / kQlKBlock;
  const int en = min(n0 + (int)(threadIdx.x & 15), N - 1);
  const int e_corr = za * w_rowsum[en];
  const float e_scale = sa * w_scales[en];
  const float e_bias = bias ? bias[en] : 0.0f;
  i32x4* abuf = lds + wave * NBUF * kSlots;

  for (int m0 = 0; m0 < M; m0 += 16 * MT) {
    i32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = i32x4{0, 0, 0, 0};
    // copy instruction j of a K block covers tile rows 4j .. 4j+3: this lane's source row and swizzled chunk
    const int8_t* asrc[MT * 4];
#pragma unroll
    for (int j = 0; j < MT * 4; ++j) {
      const int row = 4 * j + (lane >> 4);
      asrc[j] = a + (int64_t)min(m0 + row, M - 1) * K + 16 * ((lane & 15) ^ (row & 15));
    }
    const int64_t rot = full_blocks ? (int64_t)blockIdx.x % full_blocks : 0;
    auto kbyte = [&](int64_t i) {
      int64_t kblk = wave + i * kQlWaves + rot;
      if (kblk >= full_blocks) kblk -= full_blocks;
      return kblk * kQlKBlock;
    };
    auto copy_a = [&](int64_t i, int buf) {
      const int64_t k = kbyte(i);
#pragma unroll
      for (int j = 0; j < MT * 4; ++j)
        __builtin_amdgcn_global_load_lds((ql_glb_void_*)(asrc[j] + k), (ql_lds_void_*)&abuf[buf * kSlots + j * 64], 16, 0, 0);
    };
    auto load_w = [&](int64_t i, i32x4* wf) { ql_load_row<W_NT, true>(wrow, kbyte(i) + 16 * g, K, wf); };
    auto multiply = [&](const i32x4* wf, int buf) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          i32x4 av = abuf[buf * kSlots + (16 * t + r) * 16 + ((4 * p + g) ^ r)];
          if constexpr (A_U8) av = av ^ (int)0x80808080;
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, wf[p], acc[t], 0, 0, 0);
        }
      }
    };
    const int64_t n_i = full_blocks > wave ? (full_blocks - wave + kQlWaves - 1) / kQlWaves : 0;
    i32x4 wf0[4], wf1[4];
    if constexpr (NBUF == 2) {
      if (n_i > 0) { copy_a(0, 0); load_w(0, wf0); }
      for (int64_t i = 0; i < n_i; i += 2) {
        if (i + 1 < n_i) {
          copy_a(i + 1, 1); load_w(i + 1, wf1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MT * 4 + 4) : "memory");    // block i has landed, i+1 in flight
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        multiply(wf0, 0);
        if (i + 1 < n_i) {
          if (i + 2 < n_i) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // fragments of buffer 0 are in registers
            copy_a(i + 2, 0); load_w(i + 2, wf0);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MT * 4 + 4) : "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          multiply(wf1, 1);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
      }
    } else {
      if (n_i > 0) load_w(0, wf0);
      for (int64_t i = 0; i < n_i; ++i) {
        copy_a(i, 0);
        if (i + 1 < n_i) load_w(i + 1, (i & 1) ? wf0 : wf1);
        if (i + 1 < n_i) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // A(i) and W(i) landed; W(i+1) may fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        multiply((i & 1) ? wf1 : wf0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    // before the next copy overwrites the buffer
      }
    }
    if (full_blocks != kblocks && wave == kQlWaves - 1) {          // ragged end of K: guarded loads straight from global
      const int64_t k = full_blocks * kQlKBlock + 16 * g;
      i32x4 af[4];
      ql_load_row<W_NT, false>(wrow, k, K, wf0);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        ql_load_row<false, false>(a + (int64_t)min(m0 + 16 * t + r, M - 1) * K, k, K, af);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          i32x4 av = af[p];
          if constexpr (A_U8) av = av ^ (int)0x80808080;
          acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, wf0[p], acc[t], 0, 0, 0);
        }
      }
    }

    // partial sums of the waves meet in LDS (the A buffers are dead now)
    __syncthreads();
    int* red = reinterpret_cast<int*>(lds);                 // [wave][t][lane][4]
#pragma unroll
    for (int t = 0; t < MT; ++t)
      lds[(wave * MT + t) * 64 + lane] = acc[t];
    __syncthreads();
    int e_zw = 0;
    if constexpr (ZP) e_zw = zp.w_zero_points[ql_epilogue_column(n0, N)];     // here, not at the top: see qlinear_i8_kernel
    for (int e = threadIdx.x; e < MT * 256; e += kQlThreads) {
      const int t = e >> 8, rem = e & 255;
      const int mi = rem >> 4, ni = rem & 15;
      const int src_lane = (mi >> 2) * 16 + ni, src_reg = mi & 3;
      int v = 0;
#pragma unroll
      for (int wv = 0; wv < kQlWaves; ++wv) v += red[((wv * MT + t) * 64 + src_lane) * 4 + src_reg];
      const int m = m0 + 16 * t + mi, n = n0 + ni;
      if (m < M && n < N) {
        float out = (float)ql_corrected<ZP>(v, e_corr, e_zw, zp, m) * e_scale;
        if (bias) out = out + e_bias;
        if constexpr (RES) {                   // (+ residual) (ReLU) (activation): branches uniform over the launch
          if (ql_res_arg(res...).mode)
            out = ql_join(out, ql_residual_at(ql_res_arg(res...), (int64_t)m * N + n), ql_res_arg(res...));
          out = ql_act(out, ql_res_arg(res...).act);
        }
        ql_store(y, (int64_t)m * N + n, out, oq);
      }
    }
    __syncthreads();
  }
}

// One checked consumer call, as every launcher receives it (host side; the kernels keep their scalar arguments).
// za is the zero point in the domain the kernels multiply in (uint8 codes are re-biased by 128), zp is {nullptr, nullptr}
// unless the call brings weight zero points; the whole-tile kernels (launch_wide, launch_pp) do not read it.
struct QlCall {
  const void* a;
  const int8_t* w;          // int8 codes, or the packed 4-bit codes / indices of launch_qlinear<..., kQlW4 / kQlLut4>
  const float* w_scales;
  const int32_t* w_rowsum;
  const float* bias;
  void* y;
  int64_t M, N, K;
  int za;
  float sa;
  QlOut oq;
  QlZp zp;
  hipStream_t stream;
  QlRes res;                // mode 0 unless the call brings a residual (mctq_qlinear_i8_res); never together with zp
};
// the kernels' leading arguments, common to all of them
#define MCTQ_QL_ARGS(c) (const int8_t*)(c).a, (c).w, (c).w_scales, (c).w_rowsum, (c).bias, (c).y, (int)(c).M, (int)(c).N, (c).K, (c).za, (c).sa

template <int WAVES, int MT, bool A_U8>
static int launch_qlinear_lds(const QlCall& c) {
  const dim3 grid((unsigned)((c.N + 15) / 16));
  const bool one_pass = c.M <= 16 * MT;
#define MCTQ_QL_LDS(NT_, ZP_) \
  hipLaunchKernelGGL((qlinear_i8_lds_kernel<WAVES, MT, A_U8, NT_, ZP_>), grid, dim3(WAVES * 64), 0, c.stream, \
                     MCTQ_QL_ARGS(c), c.oq, c.zp)
#define MCTQ_QL_LDS_RES(NT_) \
  hipLaunchKernelGGL((qlinear_i8_lds_kernel<WAVES, MT, A_U8, NT_, false, QlRes>), grid, dim3(WAVES * 64), 0, c.stream, \
                     MCTQ_QL_ARGS(c), c.oq, c.zp, c.res)
  // (the residual form last: the kernels are emitted in the order in which they are named here)
  if (c.zp.a_rowsum) { if (one_pass) MCTQ_QL_LDS(true, true); else MCTQ_QL_LDS(false, true); }
  else if (!c.res.mode && !c.res.act) { if (one_pass) MCTQ_QL_LDS(true, false); else MCTQ_QL_LDS(false, false); }
  else { if (one_pass) MCTQ_QL_LDS_RES(true); else MCTQ_QL_LDS_RES(false); }
#undef MCTQ_QL_LDS_RES
#undef MCTQ_QL_LDS
  note_ql<A_U8>(WAVES == 8 ? "qlinear_stream_lds_8waves" : "qlinear_stream_lds_4waves", MT, c.zp.a_rowsum != nullptr, &c.res);
  return check_launch("mctq_qlinear_i8 (LDS-staged activations)");
}

template <int WAVES, int MT, bool A_U8, int WFMT = kQlW8, class... Lut>
static int launch_qlinear(const QlCall& c, Lut... lut) {
  const dim3 grid((unsigned)((c.N + 15) / 16));
  const bool one_pass = c.M <= 16 * MT;           // weights read exactly once: keep them out of the caches
  if (one_pass)
    hipLaunchKernelGGL((qlinear_i8_kernel<WAVES, MT, A_U8, true, WFMT, Lut...>), grid, dim3(WAVES * 64), 0, c.stream,
                       MCTQ_QL_ARGS(c), c.oq, c.zp, lut...);
  else
    hipLaunchKernelGGL((qlinear_i8_kernel<WAVES, MT, A_U8, false, WFMT, Lut...>), grid, dim3(WAVES * 64), 0, c.stream,
                       MCTQ_QL_ARGS(c), c.oq, c.zp, lut...);
  note_ql<A_U8>(WFMT == kQlLut4 ? "qlinear_stream_lut4" : WFMT == kQlW4 ? "qlinear_stream_w4" : WAVES == 8 ? "qlinear_stream_8waves" : "qlinear_stream_4waves", MT,
                c.zp.a_rowsum != nullptr);
  return check_launch("mctq_qlinear_i8");
}

// ------------------------------------------------------------------------------------------------
// Large row counts (M > 128): a conventional LDS-tiled product.  Block tile BM x BN over K in steps of 128 or
// 256 bytes, 4 waves in a 2 x 2 arrangement, each wave (BM/2) x (BN/2) as 16 x 16 MFMA tiles.  Tiles are stored
// as 16-byte chunks, chunk c of row r at slot c ^ swz(r): the lane groups of a ds_read_b128 then touch 16
// different bank groups.
// ------------------------------------------------------------------------------------------------
template <int CPR>
__device__ __forceinline__ int ql_swizzle(int row) {            // CPR = 16-byte chunks per tile row
  if constexpr (CPR == 8) return (row >> 1) & 7;                // 128-byte rows: two rows span the 64 banks
  else return row & (CPR - 1);                                  // 256-byte rows: every row starts on bank 0
}

// The operands are copied global -> LDS directly (global_load_lds_dwordx4: no VGPR staging, no ds_write pass;
// measured 1.3-1.4x over staging through registers).  A wave instruction fills 64 consecutive 16-byte slots, so the LDS image is linear in slot
// order and the swizzle sits on the SOURCE address (slot (row, c') receives chunk c' ^ swz(row) of that row)
// and, identically, on the fragment reads.  One barrier per K step: it retires the copies of the tile about
// to be multiplied and guarantees the other buffer is no longer being read; the next tile's copies are then
// issued and fly while this tile multiplies.
typedef __attribute__((address_space(3))) void ql_lds_void;
typedef const __attribute__((address_space(1))) void ql_glb_void;
__device__ __attribute__((aligned(16))) const int8_t g_ql_zero_chunk[16] = {0};

#ifdef MCTQ_QL_STAMP      // diagnostic build only (tools/kbench_ql_stamps.hip): where a K step of the tiled kernel spends its cycles
__device__ unsigned long long g_ql_stamp[16 * 8];      // per wave of ONE block: wait+barrier, copy issue, multiply, total, steps
#define MCTQ_STAMP(t) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#endif
// ST: LDS buffers in the ring (ST - 1 tiles requested ahead).  ST = 2 is the form above; with ST >= 3 the barrier of a K
// step only retires the copies of the tile about to be multiplied (counted vmcnt: copies return in issue order), so
// ST - 2 later tiles stay in flight across it.
// KG: wave groups (1, 2 or 4).  With KG = 2 the block has 8 waves (4: 16 waves, the groups' sums meet pairwise): both groups copy (twice the waves issuing copies -- the
// tiles run at the copy issue rate, which grows with the waves that issue), group g multiplies the g-th half of the
// 64-byte sub-steps of every K tile into its own accumulators, and the two partial sums meet in LDS at the end (exact
// integer sums: the order does not matter).
// Res: empty, or one QlRes (the residual form, as in qlinear_i8_lds_kernel): read in the epilogue only.
template <int BM, int BN, int kTileBK, bool A_U8, int ST = 2, int KG = 1, bool ZP = false, class... Res>
__global__ __launch_bounds__(256 * KG) void qgemm_i8_glds_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ w, const float* __restrict__ w_scales,
    const int32_t* __restrict__ w_rowsum, const float* __restrict__ bias, void* __restrict__ y,
    int M, int N, int64_t K, int za, float sa, int m_blocks, int n_blocks, int gm, int flags, QlOut oq, QlZp zp, Res... res) {
  static_assert(sizeof...(Res) <= 1 && !(ZP && sizeof...(Res)), "the residual form is built without weight zero points");
  constexpr bool RES = sizeof...(Res) == 1;
  const bool rotate = (flags & 1) != 0;              // K rotation (below)
  const bool stagger = (flags & 2) != 0;             // half of the waves request the later tile AFTER multiplying (below)
  constexpr int TM = BM / 32, TN = BN / 32;
  constexpr int CPR = kTileBK / 16;
  constexpr int SA = BM * CPR, SB = BN * CPR;        // slots of the A and of the B image
  constexpr int T = 256 * KG;                        // threads
  constexpr int LT = (SA + SB) / T;                  // copies per thread per tile
  constexpr int NKS = kTileBK / 64 / KG;             // 64-byte sub-steps of a tile per wave group
  static_assert(ST >= 2 && ST * (SA + SB) * 16 <= 160 * 1024 && (ST - 2) * LT <= 63, "ring depth");
  static_assert((KG == 1 || KG == 2 || KG == 4) && (SA + SB) % T == 0 && LT >= 1 && (kTileBK / 64) % KG == 0, "wave groups");
  static_assert(KG == 1 || (KG / 2) * 4 * TM * TN * 64 <= ST * (SA + SB), "the partial sums of half the groups must fit the ring");
  __shared__ i32x4 lds[ST][SA + SB];

  // Blocks are dealt round-robin to the 8 XCDs, each with its own L2: an XCD takes CONSECUTIVE tiles, ordered in bands
  // of gm tile rows (all gm row tiles of a column tile first), so what one XCD reads -- gm x BM activation rows and its
  // share of the weight rows -- is as small as the host could make it and stays in that XCD's L2 (gm = 1: row-major).
  const int total = m_blocks * n_blocks;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int per_band = gm * n_blocks;
  const int band = id / per_band, in_band = id - band * per_band;
  const int band_rows = min(gm, m_blocks - band * gm);
  const int mb = band * gm + in_band % band_rows, nb = in_band / band_rows;
  const int m0 = mb * BM, n0 = nb * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kg = wave >> 2, w4 = wave & 3;           // wave group, position in the 2 x 2 arrangement
  const int wm = w4 >> 1, wn = w4 & 1;
  const int r = lane & 15, g = lane >> 4;

  const int8_t* src[LT];        // source of this thread's j-th slot at k = 0
  int koff[LT];                 // byte offset of that chunk inside the K step (ragged-K test)
#pragma unroll
  for (int j = 0; j < LT; ++j) {
    const int s = j * T + tid;
    const bool is_a = s < SA;
    const int q = is_a ? s : s - SA;
    const int row = q / CPR, c = (q % CPR) ^ ql_swizzle<CPR>(row);
    koff[j] = 16 * c;
    src[j] = is_a ? a + (int64_t)min(m0 + row, M - 1) * K + 16 * c : w + (int64_t)min(n0 + row, N - 1) * K + 16 * c;
  }
  auto copy_tile = [&](int buf, int64_t k0) {
    const bool full = k0 + kTileBK <= K;
#pragma unroll
    for (int j = 0; j < LT; ++j) {
      const int8_t* p = (full || k0 + koff[j] < K) ? src[j] + k0 : g_ql_zero_chunk;     // beyond K: zeros
      __builtin_amdgcn_global_load_lds((ql_glb_void*)p, (ql_lds_void*)&lds[buf][j * T + wave * 64], 16, 0, 0);
    }
  };

  i32x4 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u) acc[t][u] = i32x4{0, 0, 0, 0};

  const int64_t kt_n = (K + kTileBK - 1) / kTileBK;
  // The band_rows blocks of a band that share a weight tile run in step; started at the same k, all of them would wait
  // for each line's first fetch from HBM.  Block j of them starts its walk over K at tile j * kt_n / band_rows and wraps:
  // a line is then fetched by one block and found in the XCD's L2 by the others a fraction of the K loop later (an exact
  // integer sum does not depend on the order of its terms).  Measured (profiles/r03/qlinear_rot{0,1}.log): 8-15 % for the
  // two-buffer 4-wave tiles at K = 4096, nothing for the ring tiles, and 10-18 % SLOWER at K >= 8192, where the weight
  // tiles of an XCD no longer stay in its L2 for a quarter of the loop -- off by default (tuning key "ql_rot").
  const int64_t kt_rot = rotate ? (int64_t)(in_band % band_rows) * kt_n / band_rows : 0;
  const auto k_of = [&](int64_t kt) { const int64_t t = kt + kt_rot; return (t >= kt_n ? t - kt_n : t) * (int64_t)kTileBK; };
  copy_tile(0, k_of(0));
  if constexpr (ST > 2) {
#pragma unroll
    for (int i = 1; i < ST - 1; ++i)
      if (i < kt_n) copy_tile(i, k_of(i));
  }
  int e_corr[TN];                                    // epilogue constants of this lane's columns, fetched early
  float e_scale[TN], e_bias[TN];
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int n = min(n0 + wn * (BN / 2) + 16 * u + r, N - 1);
    e_corr[u] = za * w_rowsum[n];
    e_scale[u] = sa * w_scales[n];
    e_bias[u] = bias ? bias[n] : 0.0f;
  }
  int buf = 0, nbuf = ST - 1;                         // ring positions of tile kt and of tile kt + ST - 1
#ifdef MCTQ_QL_STAMP
  unsigned long long st_wait = 0, st_copy = 0, st_mul = 0, st_t0, st_a, st_b;
  MCTQ_STAMP(st_t0);
#endif
  for (int64_t kt = 0; kt < kt_n; ++kt) {
#ifdef MCTQ_QL_STAMP
    MCTQ_STAMP(st_a);
#endif
    if constexpr (ST == 2) {
      __syncthreads();                                // tile kt has landed; buffer buf ^ 1 is free
    } else {
      // tile kt has landed in every wave's share (its copies are older than the (ST - 2) * LT newest); the buffer of
      // tile kt - 1, read before this barrier by every wave, is free
      if (kt + ST - 2 < kt_n) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((ST - 2) * LT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
#ifdef MCTQ_QL_STAMP
    MCTQ_STAMP(st_b); st_wait += st_b - st_a;
#endif
    // A wave's copies, fragment reads and products are ONE instruction stream (profiles/r03/kbench_ql_stamps.log: per K step
    // of the 4-wave 64 x 64 x 256 tile 810 cycles issuing 8 copies, 930 reading fragments and multiplying, 280 at the
    // barrier).  Experiment "ql_stagger": half of the waves multiply first and copy afterwards (the buffer they fill, tile
    // kt - 1's, is free in either order) so that the address unit is not idle while all waves multiply -- +-3 %
    // (qlinear_stagger{0,1}.log), off by default.
    const bool copy_first = ST == 2 || !stagger || (((KG > 1 ? kg : wave) & 1) == 0);   // two buffers: the copy has only this step to land
    if (copy_first && kt + ST - 1 < kt_n) copy_tile(nbuf, k_of(kt + ST - 1));
#ifdef MCTQ_QL_STAMP
    MCTQ_STAMP(st_a); st_copy += st_a - st_b;
#endif
#pragma unroll
    for (int ksi = 0; ksi < NKS; ++ksi) {
      const int ks = kg * NKS + ksi;
      i32x4 fa[TM], fb[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int row = wm * (BM / 2) + 16 * t + r;
        fa[t] = lds[buf][row * CPR + ((ks * 4 + g) ^ ql_swizzle<CPR>(row))];
        if constexpr (A_U8) fa[t] = fa[t] ^ (int)0x80808080;
      }
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        const int row = wn * (BN / 2) + 16 * u + r;
        fb[u] = lds[buf][SA + row * CPR + ((ks * 4 + g) ^ ql_swizzle<CPR>(row))];
      }
#pragma unroll
      for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int u = 0; u < TN; ++u)
          acc[t][u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[t], fb[u], acc[t][u], 0, 0, 0);
    }
#ifdef MCTQ_QL_STAMP
    { i32x4 keep = acc[0][0]; asm volatile("" : "+v"(keep)); acc[0][0] = keep; }     // the products of this step are issued before the stamp
    MCTQ_STAMP(st_b); st_mul += st_b - st_a;
#endif
    if (!copy_first && kt + ST - 1 < kt_n) copy_tile(nbuf, k_of(kt + ST - 1));
#ifdef MCTQ_QL_STAMP
    MCTQ_STAMP(st_a); st_copy += st_a - st_b;
#endif
    buf = buf + 1 == ST ? 0 : buf + 1;
    nbuf = nbuf + 1 == ST ? 0 : nbuf + 1;
  }
#ifdef MCTQ_QL_STAMP
  if (blockIdx.x == gridDim.x / 2 && lane == 0) {
    MCTQ_STAMP(st_a);
    unsigned long long* o = g_ql_stamp + wave * 8;
    o[0] = st_wait; o[1] = st_copy; o[2] = st_mul; o[3] = st_a - st_t0; o[4] = (unsigned long long)kt_n;
  }
#endif

  if constexpr (KG > 1) {             // the upper half of the groups hands its partial sums to the lower half through the
    i32x4* red = &lds[0][0];          // (dead) ring, until group 0 holds the whole sum
#pragma unroll
    for (int h = KG / 2; h >= 1; h >>= 1) {
      __syncthreads();                // every wave has read its last fragments / partial sums, every copy has landed
      if (kg >= h && kg < 2 * h) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) red[((((kg - h) * 4 + w4) * TM + t) * TN + u) * 64 + lane] = acc[t][u];
      }
      __syncthreads();
      if (kg < h) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] += red[(((kg * 4 + w4) * TM + t) * TN + u) * 64 + lane];
      }
    }
    if (kg != 0) return;
  }

#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int n = n0 + wn * (BN / 2) + 16 * u + r;
    if (n >= N) continue;
    int e_zw = 0;
    if constexpr (ZP) e_zw = zp.w_zero_points[n];                // here, not with e_corr: nothing more stays live across the K loop
    float e_res[RES ? TM * 4 : 1];                               // this column's residuals, all requested before the first is used
    (void)e_res;
    if constexpr (RES) {
      int64_t at[TM * 4];                                        // (rows beyond M are clamped: loaded, never stored)
#pragma unroll
      for (int t = 0; t < TM; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) at[4 * t + i] = (int64_t)min(m0 + wm * (BM / 2) + 16 * t + 4 * g + i, M - 1) * N + n;
      }
      if (ql_res_arg(res...).mode) ql_residuals<TM * 4>(ql_res_arg(res...), at, e_res);      // (mode 0: the activation form)
    }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * (BM / 2) + 16 * t + 4 * g + i;
        if (m < M) {
          float out = (float)ql_corrected<ZP>(acc[t][u][i], e_corr[u], e_zw, zp, m) * e_scale[u];
          if (bias) out = out + e_bias[u];
          if constexpr (RES) {
            if (ql_res_arg(res...).mode) out = ql_join(out, e_res[4 * t + i], ql_res_arg(res...));
            out = ql_act(out, ql_res_arg(res...).act);
          }
          ql_store(y, (int64_t)m * N + n, out, oq);
        }
      }
    }
  }
}

template <int BM, int BN, int BK, bool A_U8, int ST = 2, int KG = 1>
static int launch_glds(const QlCall& c) {
  const int mbl = (int)((c.M + BM - 1) / BM), nbl = (int)((c.N + BN - 1) / BN);
  // tile rows per band: an XCD's chunk of total / 8 consecutive tiles as a gm x (chunk / gm) rectangle with the least
  // gm * BM + (chunk / gm) * BN, i.e. gm ~ sqrt(chunk * BN / BM)   (tuning key "ql_band" overrides)
  int gm = g_ql_band;
  if (gm <= 0) {
    const double chunk = (double)mbl * nbl / 8.0;
    gm = (int)(sqrt(chunk * BN / BM) + 0.5);
  }
  gm = gm < 1 ? 1 : gm > mbl ? mbl : gm;
  const int flags = (g_ql_rot && gm > 1 ? 1 : 0) | (g_ql_stagger ? 2 : 0);
#define MCTQ_QL_GLDS(ZP_) \
  hipLaunchKernelGGL((qgemm_i8_glds_kernel<BM, BN, BK, A_U8, ST, KG, ZP_>), dim3((unsigned)(mbl * nbl)), dim3(256 * KG), 0, c.stream, \
                     MCTQ_QL_ARGS(c), mbl, nbl, gm, flags, c.oq, c.zp)
  if (c.zp.a_rowsum) MCTQ_QL_GLDS(true);
  else if (!c.res.mode && !c.res.act) MCTQ_QL_GLDS(false);
  else          // the residual / activation form (last: the kernels are emitted in the order in which they are named here)
    hipLaunchKernelGGL((qgemm_i8_glds_kernel<BM, BN, BK, A_U8, ST, KG, false, QlRes>), dim3((unsigned)(mbl * nbl)), dim3(256 * KG), 0,
                       c.stream, MCTQ_QL_ARGS(c), mbl, nbl, gm, flags, c.oq, c.zp, c.res);
#undef MCTQ_QL_GLDS
  static char name[48];                              // "qlinear_tiled[_ring]_<BM>x<BN>x<BK>", formatted once per instantiation
  static const bool named = (snprintf(name, sizeof(name), "qlinear_tiled%s%s_%dx%dx%d", ST > 2 || (BM == 128 && BN == 64) ? "_ring" : "",
                                      KG == 2 ? "_8waves" : KG == 4 ? "_16waves" : "", BM, BN, BK), true);
  (void)named;
  note_ql<A_U8>(name, gm, c.zp.a_rowsum != nullptr, &c.res);
  return check_launch("mctq_qlinear_i8 (tiled, direct-to-LDS)");
}

// ------------------------------------------------------------------------------------------------
// Many rows AND many columns: the 64 x 64 wave tile above needs 8 KB of LDS reads per 256 MFMA cycles and wave; with
// two blocks per CU and the direct-to-LDS copies that is most of the LDS bandwidth, and the kernel stays near a third
// of the int8 peak.  Here one wave owns (16 TM) x (16 TN) outputs (128 x 128 for the 256 x 256 block tile: 16 KB of
// reads per 1024 MFMA cycles), accumulators in the 512-register file of a 1-wave-per-SIMD block.
// K advances in 64-byte steps through a ring of 4 LDS stages: stage kt is multiplied from registers (its fragments were
// read during stage kt-1), stage kt+1 is certified by the one barrier of the iteration (placed in the middle of the
// MFMA stream, so the matrix pipe has work queued while waves meet), stages kt+2 and kt+3 are in flight.
// Whole tiles only (M % BM == N % BN == K % 128 == 0); other shapes use the kernels above.
// ------------------------------------------------------------------------------------------------
template <int I, int N, class F>
__device__ __forceinline__ void ql_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); ql_static_for<I + 1, N>(f); }
}
template <int OFF>
__device__ __forceinline__ void ql_ds_read16(i32x4& v, uint32_t lds_byte) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(lds_byte), "n"(OFF));
}

// A statement that NAMES the A fragments: everything the compiler itself does with them is ordered against it.
// WAIT: the LDS reads that filled them have returned.  Otherwise: a few idle cycles between the compiler's VALU
// writes to them and the matrix instructions (in asm, so their operand hazards are invisible to the compiler).
template <int TM, bool WAIT>
__device__ __forceinline__ void ql_fence_frags(i32x4* f) {
  static_assert(TM == 4 || TM == 8, "4 or 8 row tiles");
  if constexpr (TM == 8) {
    if constexpr (WAIT)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]) :: "memory");
    else
      asm volatile("s_nop 4" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]));
  } else {
    if constexpr (WAIT) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) :: "memory");
    else asm volatile("s_nop 4" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
  }
}

template <int TN>
__device__ __forceinline__ void ql_settle_row(i32x4 (&row)[TN]) {
  static_assert(TN == 4 || TN == 8, "row of 4 or 8 tiles");
  if constexpr (TN == 8)
    asm volatile("s_nop 7" : "+a"(row[0]), "+a"(row[1]), "+a"(row[2]), "+a"(row[3]), "+a"(row[4]), "+a"(row[5]), "+a"(row[6]), "+a"(row[7]));
  else
    asm volatile("s_nop 15" : "+a"(row[0]), "+a"(row[1]), "+a"(row[2]), "+a"(row[3]));
}

// products E .. END-1 of a step: tile (E / TN, E % TN) of the wave's TM x TN accumulator grid
template <int TM, int TN, int E, int END>
__device__ __forceinline__ void ql_mfma_run(i32x4 (&acc)[TM][TN], const i32x4* fa, const i32x4* fb) {
  if constexpr (E < END) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc[E / TN][E % TN]) : "v"(fa[E / TN]), "v"(fb[E % TN]));
    ql_mfma_run<TM, TN, E + 1, END>(acc, fa, fb);
  }
}
template <int TM, int FB, int Q, int QEND>
__device__ __forceinline__ void ql_frag_reads(i32x4* na, i32x4* nb, uint32_t pa, uint32_t pb) {
  if constexpr (Q < QEND) {
    if constexpr (Q < TM) ql_ds_read16<Q * FB>(na[Q], pa);
    else ql_ds_read16<(Q - TM) * FB>(nb[Q - TM], pb);
    ql_frag_reads<TM, FB, Q + 1, QEND>(na, nb, pa, pb);
  }
}
// second half of a step's products (tiles TM/2 .. TM-1) with the NEXT stage's TM + TN fragment reads spread between them
template <int TM, int TN, int FB, bool NEXT, int E>
__device__ __forceinline__ void ql_second_half(i32x4 (&acc)[TM][TN], const i32x4* fa, const i32x4* fb, i32x4* na,
                                               i32x4* nb, uint32_t pa, uint32_t pb) {
  constexpr int H2 = (TM - TM / 2) * TN, NR = TM + TN;
  if constexpr (E < H2) {
    if constexpr (NEXT) {
      constexpr int first = E == 0 ? 0 : ((E - 1) * NR) / H2 + 1;
      constexpr int last = (E * NR) / H2 < NR - 1 ? (E * NR) / H2 : NR - 1;
      ql_frag_reads<TM, FB, first, last + 1>(na, nb, pa, pb);
    }
    constexpr int t = TM / 2 + E / TN, u = E % TN;
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+a"(acc[t][u]) : "v"(fa[t]), "v"(fb[u]));
    ql_second_half<TM, TN, FB, NEXT, E + 1>(acc, fa, fb, na, nb, pa, pb);
  }
}

template <int TM, int TN, bool A_U8, int S = 4, int OCC = 1>
__global__ __launch_bounds__(256, OCC) void qgemm_i8_wide_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ w, const float* __restrict__ w_scales,
    const int32_t* __restrict__ w_rowsum, const float* __restrict__ bias, void* __restrict__ y,
    int M, int N, int64_t K, int za, float sa, int m_blocks, int n_blocks, QlOut oq) {
  constexpr int BM = 32 * TM, BN = 32 * TN, CPR = 4;                // S: LDS stages of the ring (S - 1 in flight)
  constexpr int SA = BM * CPR, SB = BN * CPR, SLOTS = SA + SB;      // 16-byte slots of one stage
  constexpr int LA = SA / 256, LB = SB / 256, LT = LA + LB;          // copies per thread per stage
  static_assert(S >= 4 && (S - 2) * LT <= 63 && OCC * S * SLOTS * 16 <= 160 * 1024, "ring depth / blocks per CU");
  __shared__ i32x4 lds[S * SLOTS];

  const int total = m_blocks * n_blocks;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);    // an XCD takes consecutive tiles ...
  constexpr int GM = 4;                                              // ... which form GM-row bands: shared A rows / W rows stay in its L2
  const int per_band = GM * n_blocks;
  const int band = id / per_band, in_band = id - band * per_band;
  const int band_rows = min(GM, m_blocks - band * GM);
  const int mb = band * GM + in_band % band_rows, nb = in_band / band_rows;
  const int m0 = mb * BM, n0 = nb * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;

  // copy j of a stage fills slots j * 256 + tid: row 64 j + tid / 4, physical chunk tid & 3 <- source chunk ^ swizzle.
  // swizzle(row) = (-(row >> 2)) & 3: a ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31},
  // {32-35,44-47,52-59}, {36-43,48-51,60-63}; with lane = 16 g + r reading row r, chunk g, the four rows of a group that
  // share (r & 3) -- and with it the 64-byte bank segment -- must sit in four different 16-byte slots:
  // {f(0), f(3), f(1)^1, f(2)^1} and {f(1), f(2), f(0)^1, f(3)^1} are permutations of 0..3 for f(x) = -x mod 4.
  const int crow = tid >> 2, cchunk = (tid & 3) ^ ((0 - (crow >> 2)) & 3);
  const int8_t* pa = a + (int64_t)(m0 + crow) * K + 16 * cchunk;
  const int8_t* pw = w + (int64_t)(n0 + crow) * K + 16 * cchunk;
  const int64_t jstride = 64 * K;
  auto copy_stage = [&](int slot, int kt) {
    i32x4* dst = lds + (slot % S) * SLOTS + wave * 64;
    const int64_t k0 = (int64_t)kt * 64;
#pragma unroll
    for (int j = 0; j < LA; ++j)
      __builtin_amdgcn_global_load_lds((ql_glb_void*)(pa + j * jstride + k0), (ql_lds_void*)(dst + j * 256), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < LB; ++j)
      __builtin_amdgcn_global_load_lds((ql_glb_void*)(pw + j * jstride + k0), (ql_lds_void*)(dst + SA + j * 256), 16, 0, 0);
  };

  // Fragment of tile row 16 t + r, k bytes [16 g, 16 g + 16): slot row * 4 + (g ^ swizzle(row)).
  // Fragment reads and products are inline asm: the compiler would otherwise retire all but the newest direct-to-LDS
  // copies before any LDS read (it cannot tell the stages apart), and it keeps the accumulators in VGPRs in some loop
  // blocks and AGPRs in others, copying 128-256 registers per step.  "a" operands pin them to the AGPR half.
  const uint32_t lane_byte = (uint32_t)(r * CPR + (g ^ ((0 - (r >> 2)) & 3))) * 16u;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(ql_lds_void*)lds;
  const uint32_t a_byte = lds0 + lane_byte + (uint32_t)(wm * 16 * TM * CPR) * 16u;
  const uint32_t b_byte = lds0 + lane_byte + (uint32_t)(SA + wn * 16 * TN * CPR) * 16u;
  constexpr uint32_t kStageBytes = SLOTS * 16u;
  constexpr int kFragBytes = 16 * CPR * 16;

  i32x4 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u) acc[t][u] = i32x4{0, 0, 0, 0};

  const int kt_n = (int)(K / 64);                      // even and >= 4 (host check)
  constexpr int H1 = TM / 2 * TN, NR = TM + TN;
  i32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];

  // One K step, the same code for every kt (a loop of ONE basic block keeps the register allocation of the accumulators
  // stable): near the end of K the request for stage kt+3 re-fetches the last stage into a ring slot nobody reads again,
  // and the fragment reads of the non-existent stage kt_n land in registers nobody uses.
  const int kt_last = kt_n - 1;
  auto step = [&](int kt, i32x4* fa, const i32x4* fb, i32x4* na, i32x4* nb_) {
    // this stage's fragments (requested half a step ago); the A fragments are operands so that the compiler's own
    // uses of them (the uint8 re-bias below) stay behind the wait
    ql_fence_frags<TM, true>(fa);
    if constexpr (A_U8) {
#pragma unroll
      for (int t = 0; t < TM; ++t) fa[t] = fa[t] ^ (int)0x80808080;     // uint8 codes -> int8 (za carries the -128)
      ql_fence_frags<TM, false>(fa);
    }
    ql_mfma_run<TM, TN, 0, H1>(acc, fa, fb);
    // stage kt+1 complete in LDS for every wave (own copies retired, then the barrier); stage kt+2 may still fly
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((S - 3) * LT) : "memory");
    copy_stage(kt + S - 1, min(kt + S - 1, kt_last));    // into the slot of kt-1, whose fragments were consumed a step ago
    const uint32_t so = (uint32_t)((kt + 1) % S) * kStageBytes;
    ql_second_half<TM, TN, kFragBytes, true, 0>(acc, fa, fb, na, nb_, a_byte + so, b_byte + so);
  };

  ql_static_for<0, S - 1>([&](auto i_) { copy_stage(decltype(i_)::value, min((int)decltype(i_)::value, kt_last)); });
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((S - 2) * LT) : "memory");
  ql_frag_reads<TM, kFragBytes, 0, NR>(fa0, fb0, a_byte, b_byte);
  for (int kt = 0; kt < kt_n; kt += 2) {                // kt_n is even (host check)
    step(kt, fa0, fb0, fa1, fb1);
    step(kt + 1, fa1, fb1, fa0, fb0);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  // The compiler does not see the matrix pipe behind the asm statements: without a barrier that NAMES the
  // accumulators it may read a tile (v_accvgpr_read) right behind the asm of that tile's last product, before the
  // result has left the pipe.  One statement per row of tiles, after the last product, 8 x 8 idle cycles in all.
  ql_static_for<0, TM>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    ql_settle_row<TN>(acc[t]);
  });

  auto epilogue = [&](auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      const int n = n0 + wn * 16 * TN + 16 * u + r;
      const int e_corr = za * w_rowsum[n];
      const float e_scale = sa * w_scales[n];
      const float e_bias = bias ? bias[n] : 0.0f;
#pragma unroll
      for (int t = 0; t < TM; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t idx = (int64_t)(m0 + wm * 16 * TM + 16 * t + 4 * g + i) * N + n;
          float out = (float)(acc[t][u][i] - e_corr) * e_scale;
          if (bias) out = out + e_bias;
          if constexpr (MODE == 0) {
            static_cast<float*>(y)[idx] = out;
          } else {
            float q = fminf(fmaxf(__builtin_rintf(out * oq.inv) + oq.zf, oq.lo), oq.hi);
            if constexpr (MODE == 1) static_cast<int8_t*>(y)[idx] = (int8_t)(int)q;
            else static_cast<uint8_t*>(y)[idx] = (uint8_t)(int)q;
          }
        }
      }
    }
  };
  if (oq.mode == 0) epilogue(std::integral_constant<int, 0>{});
  else if (oq.mode == 1) epilogue(std::integral_constant<int, 1>{});
  else epilogue(std::integral_constant<int, 2>{});
}

// ------------------------------------------------------------------------------------------------
// The same 256 x 256 block tile with EIGHT waves in two groups that alternate between a memory phase and a product
// phase.  Issuing a direct-to-LDS copy holds a wave's instruction stream for ~100 cycles; with one wave per SIMD
// the matrix pipe idles meanwhile (counters on the 4-wave kernel above: pipe 47 % busy, half of the wave time
// spent waiting to issue).  Here waves w and w + 4 share a SIMD and belong to different groups: while one requests the
// next stage (4 copies) and reads its 12 fragments, the other issues its 32 products; a workgroup barrier swaps the
// roles twice per K step.  Wave tile 128 x 64 (TM 8 x TN 4), fragments single-buffered, ring of 4 stages with the
// request running 3 stages ahead.
//   slot:      2k            2k+1           2k+2
//   group 0:   MEM(k)    |   CMP(k)     |   MEM(k+1)
//   group 1:   CMP(k-1)  |   MEM(k)     |   CMP(k)
// Stage k+1 is certified by the barrier that ends slot 2k+1 (every wave first retires its own copies of it); the
// slot overwritten by MEM(k) held stage k-1, whose last fragment reads (group 1, slot 2k-1) were awaited before
// the barrier that ended that slot.
// ------------------------------------------------------------------------------------------------
template <bool A_U8>
__global__ __launch_bounds__(512, 1) void qgemm_i8_pp_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ w, const float* __restrict__ w_scales,
    const int32_t* __restrict__ w_rowsum, const float* __restrict__ bias, void* __restrict__ y,
    int M, int N, int64_t K, int za, float sa, int m_blocks, int n_blocks, QlOut oq) {
  constexpr int TM = 8, TN = 4, BM = 256, BN = 256, CPR = 4, S = 4;
  constexpr int SA = BM * CPR, SB = BN * CPR, SLOTS = SA + SB;      // 2048 16-byte slots per stage
  constexpr int LA = SA / 512, LB = SB / 512, LT = LA + LB;          // copies per thread per stage: 2 + 2
  __shared__ i32x4 lds[S * SLOTS];

  const int total = m_blocks * n_blocks;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  constexpr int GM = 4;
  const int per_band = GM * n_blocks;
  const int band = id / per_band, in_band = id - band * per_band;
  const int band_rows = min(GM, m_blocks - band * GM);
  const int mb = band * GM + in_band % band_rows, nb = in_band / band_rows;
  const int m0 = mb * BM, n0 = nb * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = (wave >> 1) & 3;
  const int r = lane & 15, g = lane >> 4;

  // copy j of a stage fills slots j * 512 + tid: row 128 j + tid / 4, physical chunk tid & 3 (swizzle as above)
  const int crow = tid >> 2, cchunk = (tid & 3) ^ ((0 - (crow >> 2)) & 3);
  const int8_t* pa = a + (int64_t)(m0 + crow) * K + 16 * cchunk;
  const int8_t* pw = w + (int64_t)(n0 + crow) * K + 16 * cchunk;
  const int64_t jstride = 128 * K;
  auto copy_stage = [&](int slot, int kt) {
    i32x4* dst = lds + (slot & (S - 1)) * SLOTS + wave * 64;
    const int64_t k0 = (int64_t)kt * 64;
#pragma unroll
    for (int j = 0; j < LA; ++j)
      __builtin_amdgcn_global_load_lds((ql_glb_void*)(pa + j * jstride + k0), (ql_lds_void*)(dst + j * 512), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < LB; ++j)
      __builtin_amdgcn_global_load_lds((ql_glb_void*)(pw + j * jstride + k0), (ql_lds_void*)(dst + SA + j * 512), 16, 0, 0);
  };

  const uint32_t lane_byte = (uint32_t)(r * CPR + (g ^ ((0 - (r >> 2)) & 3))) * 16u;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(ql_lds_void*)lds;
  const uint32_t a_byte = lds0 + lane_byte + (uint32_t)(wm * 16 * TM * CPR) * 16u;
  const uint32_t b_byte = lds0 + lane_byte + (uint32_t)(SA + wn * 16 * TN * CPR) * 16u;
  constexpr uint32_t kStageBytes = SLOTS * 16u;
  constexpr int kFragBytes = 16 * CPR * 16;

  i32x4 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u) acc[t][u] = i32x4{0, 0, 0, 0};

  const int kt_n = (int)(K / 64), kt_last = kt_n - 1;
  i32x4 fa[TM], fb[TN];

  auto mem_phase = [&](int kt) {
    const uint32_t so = (uint32_t)(kt & (S - 1)) * kStageBytes;
    ql_frag_reads<TM, kFragBytes, 0, TM + TN>(fa, fb, a_byte + so, b_byte + so);
    copy_stage(kt + 3, min(kt + 3, kt_last));
  };
  auto cmp_phase = [&]() {
    if constexpr (A_U8) {
#pragma unroll
      for (int t = 0; t < TM; ++t) fa[t] = fa[t] ^ (int)0x80808080;
      ql_fence_frags<TM, false>(fa);
    }
    ql_mfma_run<TM, TN, 0, TM * TN>(acc, fa, fb);
  };

  copy_stage(0, 0);
  copy_stage(1, 1);
  copy_stage(2, 2);
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * LT) : "memory");
  if (wave < 4) {
    for (int kt = 0; kt < kt_n; ++kt) {
      mem_phase(kt);
      ql_fence_frags<TM, true>(fa);                                        // fragments in registers (lgkmcnt 0)
      asm volatile("s_barrier" ::: "memory");                              // b(2k)
      cmp_phase();
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * LT) : "memory");   // own copies of stage k+1 retired; b(2k+1)
    }
  } else {
    asm volatile("s_barrier" ::: "memory");                                // b0
    for (int kt = 0; kt < kt_n; ++kt) {
      mem_phase(kt);
      ql_fence_frags<TM, true>(fa);
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * LT) : "memory");   // b(2k+1)
      cmp_phase();
      if (kt + 1 < kt_n) asm volatile("s_barrier" ::: "memory");           // b(2k+2)
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  ql_static_for<0, TM>([&](auto t_) {
    constexpr int t = decltype(t_)::value;
    ql_settle_row<TN>(acc[t]);
  });

  auto epilogue = [&](auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      const int n = n0 + wn * 16 * TN + 16 * u + r;
      const int e_corr = za * w_rowsum[n];
      const float e_scale = sa * w_scales[n];
      const float e_bias = bias ? bias[n] : 0.0f;
#pragma unroll
      for (int t = 0; t < TM; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t idx = (int64_t)(m0 + wm * 16 * TM + 16 * t + 4 * g + i) * N + n;
          float out = (float)(acc[t][u][i] - e_corr) * e_scale;
          if (bias) out = out + e_bias;
          if constexpr (MODE == 0) {
            static_cast<float*>(y)[idx] = out;
          } else {
            float q = fminf(fmaxf(__builtin_rintf(out * oq.inv) + oq.zf, oq.lo), oq.hi);
            if constexpr (MODE == 1) static_cast<int8_t*>(y)[idx] = (int8_t)(int)q;
            else static_cast<uint8_t*>(y)[idx] = (uint8_t)(int)q;
          }
        }
      }
    }
  };
  if (oq.mode == 0) epilogue(std::integral_constant<int, 0>{});
  else if (oq.mode == 1) epilogue(std::integral_constant<int, 1>{});
  else epilogue(std::integral_constant<int, 2>{});
}

template <bool A_U8>
static int launch_pp(const QlCall& c) {
  if (c.M % 256 != 0 || c.N % 256 != 0 || c.K % 64 != 0 || c.K < 256) return fail_arg("ping-pong tiled kernel needs whole 256 x 256 tiles, K % 64 == 0 and K >= 256");
  const int mbl = (int)(c.M / 256), nbl = (int)(c.N / 256);
  hipLaunchKernelGGL((qgemm_i8_pp_kernel<A_U8>), dim3((unsigned)(mbl * nbl)), dim3(512), 0, c.stream,
                     MCTQ_QL_ARGS(c), mbl, nbl, c.oq);
  note_ql<A_U8>("qlinear_pingpong_256x256");
  return check_launch("mctq_qlinear_i8 (ping-pong tiles)");
}

template <int TM, int TN, bool A_U8, int S = 4, int OCC = 1>
static int launch_wide(const QlCall& c) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  if (c.M % BM != 0 || c.N % BN != 0 || c.K % 128 != 0 || c.K < 256) return fail_arg("wide tiled kernel needs whole tiles, K % 128 == 0 and K >= 256");
  const int mbl = (int)(c.M / BM), nbl = (int)(c.N / BN);
  hipLaunchKernelGGL((qgemm_i8_wide_kernel<TM, TN, A_U8, S, OCC>), dim3((unsigned)(mbl * nbl)), dim3(256), 0, c.stream,
                     MCTQ_QL_ARGS(c), mbl, nbl, c.oq);
  static const char* const kName = TM == 8 && TN == 8 ? "qlinear_wide_256x256" : TM == 4 && TN == 8 ? "qlinear_wide_128x256"
      : TM == 8 ? "qlinear_wide_256x128" : "qlinear_wide_128x128";
  note_ql<A_U8>(kName, S);
  return check_launch("mctq_qlinear_i8 (wide tiles)");
}
#undef MCTQ_QL_ARGS

// ------------------------------------------------------------------------------------------------
// Row sums of activation codes, a_rowsum[m] = sum_k (a[m][k] - za): the per-row factor of the weight zero point term
// (QlZp).  A lane loads 16 bytes and sums them with four packed dot products against 0x01010101 (v_dot4_i32_i8 /
// v_dot4_u32_u8: uint8 codes are summed unsigned, no re-bias needed); the lanes' sums meet by wave shuffles and, when a
// whole block walks one row (BLOCK), the four waves' sums through LDS.  No atomics: integer sums, any order, one result.
// ------------------------------------------------------------------------------------------------
constexpr int kRowsumThreads = 256;
template <bool A_U8, bool BLOCK>
__global__ __launch_bounds__(kRowsumThreads) void codes_rowsum_kernel(const int8_t* __restrict__ a, int32_t* __restrict__ out,
                                                                      int M, int K, int za) {
  constexpr int kWaves = kRowsumThreads / 64;
  __shared__ int part[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = BLOCK ? (int)blockIdx.x : (int)blockIdx.x * kWaves + wave;       // grid: M blocks / ceil(M / 4) blocks
  const bool live = m < M;                                                       // (BLOCK: always)
  const int8_t* row = a + (int64_t)(live ? m : M - 1) * K;
  const int first = 16 * (BLOCK ? (int)threadIdx.x : lane), step = 16 * (BLOCK ? kRowsumThreads : 64);
  int sum = 0;
  for (int k = first; k < K; k += step) {                                        // K % 16 == 0: a piece that starts inside K ends inside it
    const i32x4 v = *reinterpret_cast<const i32x4*>(row + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (A_U8) sum = (int)__builtin_amdgcn_udot4((unsigned)v[i], 0x01010101u, (unsigned)sum, false);
      else sum = __builtin_amdgcn_sdot4(v[i], 0x01010101, sum, false);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  const unsigned bias = (unsigned)K * (unsigned)za;                              // wraps like the sum it leaves
  if constexpr (BLOCK) {
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int wv = 0; wv < kWaves; ++wv) total += part[wv];
      out[m] = (int)((unsigned)total - bias);
    }
  } else {
    if (lane == 0 && live) out[m] = (int)((unsigned)sum - bias);
  }
}

// One block per row up to this many rows, one wave per row beyond.  Measured (tools/zp_consumer_probe.py --rowsum-only, both
// forms forced beside the dispatch, profiles/EXPERIMENTS.md): for K = 1024 / 4096 / 32768 and 1 to 1024 rows both forms take
// the time of an empty launch (6.2-6.6 us back to back, the forms within 0.2 us of each other in either direction), so the
// data give no reason to move the crossover; at 4096 rows of 32 KiB, the one cell above that floor, a wave per row wins
// (19.5 against 20.2 us).  64 stays: a few rows of a long K are not walked by a single wave each.
#ifndef MCTQ_ROWSUM_BLOCK_ROWS             // timing experiment (tools/zp_consumer_probe.py --rowsum-only): 0 / 1 << 30 force a form
#define MCTQ_ROWSUM_BLOCK_ROWS 64
#endif
constexpr int64_t kRowsumBlockRows = MCTQ_ROWSUM_BLOCK_ROWS;

}  // namespace mctq

using namespace mctq;

// ------------------------------------------------------------------------------------------------
// The kernels of mctq_qlinear_i8 / _codes / _zp: one row per variant, and a variant is declared nowhere else.
// The rows stand in the order in which the kernels stand in the code object (the compiler instantiates and emits them as
// the rows name their launchers, uint8 activations first): moving a row moves its kernels.  The order in which the
// automatic choice considers them is the column `turn`; a tie goes to the earlier turn (smaller tiles first).
// ------------------------------------------------------------------------------------------------
typedef int (*QlLaunch)(const QlCall&);
enum QlModel {
  kQlStreaming,           // a block = 16 columns x all rows, bm rows per pass: candidate of the cost model for m_lo <= M <= m_hi
  kQlTiles,               // a block = one bm x bn tile: candidate of the cost model
  kQlByFill               // whole-tile kernel weighed in front of the cost model, by how full its last round of blocks is
};
enum { kQlWholeTiles = 1,      // only M % bm == N % bn == K % 128 == 0 and K >= 256
       kQlNoZeroPoints = 2,    // not built for calls that bring weight zero points
       kQlNoResidual = 4,      // not built for calls that bring a residual (mctq_qlinear_i8_res)
       kQlNoActivation = 8 };  // not built for calls that bring a Hardswish / Hardsigmoid (mctq_qlinear_i8_act)
// what a call needs, as the mask of the rule bits that exclude a kernel from it
constexpr unsigned kQlNeeds = kQlNoZeroPoints | kQlNoResidual | kQlNoActivation;
struct QlKernel {
  int variant;            // tuning key "ql_variant"
  QlLaunch launch[2];     // uint8 / int8 activation codes
  QlModel model;
  int turn;               // place in the order the automatic choice considers the variants in: the earlier turn wins a tie
  int bm, bn, occ;        // block tile, resident blocks per CU
  double rate[3];         // fitted: KiB/us a CU takes in with 1 / 2 / 3 resident blocks; kQlByFill: POP/s of full rounds
  unsigned rules;         // admission: 0 = any shape, any call
  int m_lo, m_hi;         // kQlStreaming: the row counts it is a candidate for
};
// Few rows: the weight-streaming kernels (activation codes staged through per-wave LDS: full-line copies instead of
// fragment-shaped L2 reads; profiles/r02/qlinear_probe.log) are candidates of the cost model.
// Between the two regimes every kernel runs at the CU's intake of direct-to-LDS copies, an issue rate: about 36 KiB/us
// with one resident block per CU, 48-58 with two, 64 with three (profiles/r03/qlinear_tile_sweep.log,
// qlinear_small_tiles.log, EXPERIMENTS.md).  So the time of a launch is (operand bytes of a block) x (blocks the busiest
// CU takes) / rate, and the choice is the kernel that makes that least: the weight-streaming kernel (a block = 16
// columns x all rows, 64 rows per pass), 32 x 32 ... 128 x 128 tiles with two or three LDS buffers and four or eight
// waves (eight / sixteen: two / four wave groups that all copy and each multiply a share of a K tile -- more waves
// issuing copies raise the rate by 10-30 %), and the asm-pinned 128 x 128 kernel where the problem is whole tiles.  Earlier candidates win ties (smaller tiles first).
// Many rows and columns, whole tiles: the 256 x 256 ping-pong kernel (2.2-2.3 POP/s against 1.5 for the 128 x 128
// tiles; profiles/r02/qgemm_wide_probe.log) or, when there are too few such tiles for the chip, 128 x 256 wave-wide
// tiles -- weighed by how full their last round of blocks is (one block per CU; the 128 x 128 kernel fits two).
// (Zero-point weights, residuals and activations: those two kernels and the pinned 128 x 128 candidate do not take them; the
// tiled kernels do.)
static const QlKernel kQlKernels[] = {
    // variant, {launcher for uint8, for int8 codes}, model, turn, bm, bn, occ, {rates}[, rules[, m_lo, m_hi]]
    // weight streaming, activation codes through per-wave LDS: 16 / 32 / 64 rows per pass.  A block = 16 weight rows + 16 MT
    // activation rows per pass; MT = 1 fits two blocks per CU.  Rates fitted on profiles/r03/qlinear_small_m.log (16 / 32 rows)
    // and qlinear_small_tiles.log (64 ... 128 rows).
    {181, {launch_qlinear_lds<8, 1, true>, launch_qlinear_lds<8, 1, false>}, kQlStreaming, 0, 16, 16, 2, {29.0, 36.5}, 0, 1, 16},
    {182, {launch_qlinear_lds<8, 2, true>, launch_qlinear_lds<8, 2, false>}, kQlStreaming, 1, 32, 16, 1, {38.0}, 0, 17, 32},
    {184, {launch_qlinear_lds<8, 4, true>, launch_qlinear_lds<8, 4, false>}, kQlStreaming, 2, 64, 16, 1, {47.0}, 0, 33, 128},
    // 8-wave blocks (two wave groups), ring of three LDS buffers: rates fitted on profiles/r03/qlinear_8waves.log
    {83233, {launch_glds<32, 32, 256, true, 3, 2>, launch_glds<32, 32, 256, false, 3, 2>}, kQlTiles, 3, 32, 32, 3, {42, 63, 65}},
    {86433, {launch_glds<64, 32, 256, true, 3, 2>, launch_glds<64, 32, 256, false, 3, 2>}, kQlTiles, 4, 64, 32, 2, {50, 61}},
    {86633, {launch_glds<64, 64, 128, true, 3, 2>, launch_glds<64, 64, 128, false, 3, 2>}, kQlTiles, 7, 64, 64, 3, {36, 56, 59}},   // 128-byte K steps, three blocks per CU
    {812613, {launch_glds<128, 64, 128, true, 3, 2>, launch_glds<128, 64, 128, false, 3, 2>}, kQlTiles, 8, 128, 64, 2, {44, 54}},
    // 16-wave blocks (four wave groups; qlinear_16waves.log): one block per CU
    {166623, {launch_glds<64, 64, 256, true, 3, 4>, launch_glds<64, 64, 256, false, 3, 4>}, kQlTiles, 5, 64, 64, 1, {48}},
    {1612623, {launch_glds<128, 64, 256, true, 3, 4>, launch_glds<128, 64, 256, false, 3, 4>}, kQlTiles, 9, 128, 64, 1, {48}},   // 256-byte K steps
    // 4-wave blocks, two LDS buffers
    {612, {launch_glds<64, 128, 128, true>, launch_glds<64, 128, 128, false>}, kQlTiles, 10, 64, 128, 3, {36, 50, 64}},
    {1212, {launch_glds<128, 128, 128, true>, launch_glds<128, 128, 128, false>}, kQlTiles, 11, 128, 128, 2, {30, 48}},
    {662, {launch_glds<64, 64, 256, true>, launch_glds<64, 64, 256, false>}, kQlTiles, 6, 64, 64, 2, {36, 54}},   // two blocks per CU
    // wave-wide 128 x 128 / 128 x 256 tiles
    {2544, {launch_wide<4, 4, true>, launch_wide<4, 4, false>}, kQlTiles, 12, 128, 128, 2, {38, 43}, kQlWholeTiles | kQlNoZeroPoints | kQlNoResidual | kQlNoActivation},
    {2548, {launch_wide<4, 8, true>, launch_wide<4, 8, false>}, kQlByFill, 14, 128, 256, 1, {2.0}, kQlWholeTiles | kQlNoZeroPoints | kQlNoResidual | kQlNoActivation},
    // 256 x 256 ping-pong tiles
    {2560, {launch_pp<true>, launch_pp<false>}, kQlByFill, 13, 256, 256, 1, {2.25}, kQlWholeTiles | kQlNoZeroPoints | kQlNoResidual | kQlNoActivation},
};

static bool ql_admits(const QlKernel& k, int64_t M, int64_t N, int64_t K, unsigned needs) {
  if (k.rules & needs & kQlNeeds) return false;
  if ((k.rules & kQlWholeTiles) && (M % k.bm != 0 || N % k.bn != 0 || K % 128 != 0 || K < 256)) return false;
  return k.model != kQlStreaming || (M >= k.m_lo && M <= k.m_hi);
}

// The automatic choice for a checked call (M, N >= 1) on a chip of `cus` compute units.  The loops over the table are
// unrolled: a row's model, tile and occupancy then fold into constants, and the divisions by them cost what they cost when
// every candidate was spelled out (a third of the time of the rolled loops, measured on the host alone).
static const QlKernel* ql_choose(int64_t M, int64_t N, int64_t K, unsigned needs, int64_t cus) {
  const auto blocks = [&](int64_t bm, int64_t bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  // Only where the 128 x 128 kernel would fill the chip: smaller problems keep its finer tiles.
  if (blocks(128, 128) >= 2 * cus) {
    const auto fill = [&](int64_t nb, int64_t slots) { return (double)nb / (double)(((nb + slots - 1) / slots) * slots); };
    double best = 1.5 * fill(blocks(128, 128), 2 * cus);        // the 128 x 128 tiles these kernels have to beat
    const QlKernel* pick = nullptr;
#pragma unroll
    for (const QlKernel& k : kQlKernels) {
      if (k.model != kQlByFill || !ql_admits(k, M, N, K, needs)) continue;
      const double rate = k.rate[0] * fill(blocks(k.bm, k.bn), cus);
      if (rate > best || (pick && rate == best && k.turn < pick->turn)) { best = rate; pick = &k; }
    }
    if (pick) return pick;
  }
  double best = 0.0;
  const QlKernel* pick = nullptr;
#pragma unroll
  for (const QlKernel& k : kQlKernels) {
    if (k.model == kQlByFill || !ql_admits(k, M, N, K, needs)) continue;
    // us, up to a common constant: a streaming block takes all row passes of its 16 columns
    const int64_t passes = (M + k.bm - 1) / k.bm, across = (N + k.bn - 1) / k.bn;
    const bool stream = k.model == kQlStreaming;
    const double kib = (double)((stream ? passes : 1) * (k.bm + k.bn)) * (double)K / 1024.0;
    const int64_t per_cu = ((stream ? across : passes * across) + cus - 1) / cus, full = per_cu / k.occ, rem = per_cu % k.occ;
    const double cost = (double)(full * k.occ) * kib / k.rate[k.occ - 1] + (rem ? (double)rem * kib / k.rate[rem - 1] : 0.0);
    if (!pick || cost < best || (cost == best && k.turn < pick->turn)) { best = cost; pick = &k; }
  }
  return pick;
}

// What every consumer entry point checks, in one place; on success c.za becomes the zero point in the kernels' domain.
// false: the entry point returns rc -- an argument error, or 0 for an empty problem (decided before any pointer is looked at).
static bool ql_check_call(QlCall& c, int32_t a_code_dtype, bool with_zp, bool packed, int& rc) {
  rc = 0;
  if (c.M < 0 || c.N < 0 || c.K < 0) rc = fail_arg("negative extent");
  else if (a_code_dtype != MCTQ_CODE_I8 && a_code_dtype != MCTQ_CODE_U8) rc = fail_arg("bad a_code_dtype");
  else if (c.M == 0 || c.N == 0) return false;
  else if (!c.a || !c.w || !c.w_scales || !c.w_rowsum || !c.y) rc = fail_arg("NULL pointer");
  else if (with_zp && (!c.zp.w_zero_points || !c.zp.a_rowsum)) rc = fail_arg("w_zero_points and a_rowsum are both required");
  else if (c.K % 16 != 0) rc = fail_arg("K must be a multiple of 16");
  else if (!packed && (((uintptr_t)c.a | (uintptr_t)c.w) & 15u) != 0) rc = fail_arg("code matrices must be 16-byte aligned");
  else if (packed && ((((uintptr_t)c.a) & 15u) != 0 || (((uintptr_t)c.w) & 7u) != 0))
    rc = fail_arg("a_codes must be 16-byte and the packed weights (w_codes4 / w_idx4) 8-byte aligned");
  else if (c.K > (1 << 15)) rc = fail_arg("K > 32768 could overflow the int32 accumulator");
  else if (c.M > INT32_MAX / 2 || c.N > INT32_MAX / 2) rc = fail_arg("M or N too large");
  if (rc) return false;
  if (a_code_dtype == MCTQ_CODE_U8) c.za -= 128;
  return true;
}

// needs: kQlNoZeroPoints for a call with weight zero points, kQlNoResidual for one with a residual, kQlNoActivation for one
// with a Hardswish / Hardsigmoid (each checked by its entry point)
static int qlinear_dispatch(QlCall c, int32_t a_code_dtype, unsigned needs) {
  int rc;
  if (!ql_check_call(c, a_code_dtype, (needs & kQlNoZeroPoints) != 0, false, rc)) return rc;
  const int which = a_code_dtype == MCTQ_CODE_U8 ? 0 : 1;
  // tuning key "ql_variant": force ONE of the kernels the automatic choice below can select (tests run each of them over
  // ragged shapes against the integer oracle); the experiment variants of round 3 are not built any more
  if (g_ql_variant != 0)
    for (const QlKernel& k : kQlKernels) {
      if (k.variant != g_ql_variant) continue;
      if (k.rules & needs & kQlNoZeroPoints)
        return fail_arg("the register-pinned whole-tile kernels (ql_variant 2544 / 2548 / 2560) are not built for zero-point weights");
      if (k.rules & needs & kQlNoResidual)
        return fail_arg("the register-pinned whole-tile kernels (ql_variant 2544 / 2548 / 2560) are not built for a residual");
      if (k.rules & needs & kQlNoActivation)
        return fail_arg("the register-pinned whole-tile kernels (ql_variant 2544 / 2548 / 2560) are not built for an activation");
      return k.launch[which](c);
    }
  return ql_choose(c.M, c.N, c.K, needs, cu_count())->launch[which](c);
}

// The entry points that stream half a byte per weight: 4-bit codes (lut == nullptr) or 4-bit indices into *lut.
template <int WFMT, class... Lut>
static int launch_packed4(const QlCall& c, bool u8, Lut... lut) {
  if (c.M <= 16) return u8 ? launch_qlinear<8, 1, true, WFMT>(c, lut...) : launch_qlinear<8, 1, false, WFMT>(c, lut...);
  if (c.M <= 32) return u8 ? launch_qlinear<8, 2, true, WFMT>(c, lut...) : launch_qlinear<8, 2, false, WFMT>(c, lut...);
  return u8 ? launch_qlinear<8, 4, true, WFMT>(c, lut...) : launch_qlinear<8, 4, false, WFMT>(c, lut...);
}
static int qlinear_packed4(QlCall c, int32_t a_code_dtype, bool with_zp, const QlLut* lut) {
  int rc;
  if (!ql_check_call(c, a_code_dtype, with_zp, true, rc)) return rc;
  const bool u8 = a_code_dtype == MCTQ_CODE_U8;
  return lut ? launch_packed4<kQlLut4>(c, u8, *lut) : launch_packed4<kQlW4>(c, u8);
}

// The entry points' arguments as a call record that is not checked yet: a_zero_point as given, float32 output.
#define MCTQ_QL_CALL(w_, zw_, ar_)                                                                                      \
  QlCall c{a_codes, reinterpret_cast<const int8_t*>(w_), w_scales, w_rowsum, bias, y, M, N, K, a_zero_point, a_scale, \
           QlOut{}, QlZp{zw_, ar_}, (hipStream_t)stream, QlRes{nullptr, 0, 0, 0.0f, 0, 0}}

extern "C" {

int mctq_qlinear_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                    const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                    float* y, int64_t M, int64_t N, int64_t K, void* stream) {
  MCTQ_QL_CALL(w_codes, nullptr, nullptr);
  return qlinear_dispatch(c, a_code_dtype, 0u);
}

int mctq_qlinear_i8_codes(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                          const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                          void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                          int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream) {
  if (y_code_dtype < 0) return fail_arg("bad y_code_dtype");      // this entry point has no float32 form
  MCTQ_QL_CALL(w_codes, nullptr, nullptr);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  return qlinear_dispatch(c, a_code_dtype, 0u);
}

int mctq_qlinear_w4a8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                      const uint8_t* w_codes4, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                      void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                      int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream) {
  MCTQ_QL_CALL(w_codes4, nullptr, nullptr);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  return qlinear_packed4(c, a_code_dtype, false, nullptr);
}

int mctq_qlinear_lut4a8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const uint8_t* w_idx4, const int8_t* lut16, const float* w_scales, const int32_t* w_rowsum,
                        const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                        int32_t y_quant_min, int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream) {
  if (!lut16) return fail_arg("lut16 is NULL (a HOST pointer to 16 int8 codebook values)");
  QlLut lut;
  memcpy(lut.t, lut16, sizeof(lut.t));                // entry j -> byte j % 4 of dword j / 4 (little endian)
  MCTQ_QL_CALL(w_idx4, nullptr, nullptr);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  return qlinear_packed4(c, a_code_dtype, false, &lut);
}

int mctq_codes_rowsum(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, int32_t* a_rowsum, int64_t M,
                      int64_t K, void* stream) {
  if (M < 0 || K < 0) return fail_arg("negative extent");
  if (a_code_dtype != MCTQ_CODE_I8 && a_code_dtype != MCTQ_CODE_U8) return fail_arg("bad a_code_dtype");
  if (M == 0) return 0;
  if (!a_codes || !a_rowsum) return fail_arg("NULL pointer");
  if (K % 16 != 0) return fail_arg("K must be a multiple of 16");
  if ((((uintptr_t)a_codes) & 15u) != 0) return fail_arg("a_codes must be 16-byte aligned");
  if (K > (1 << 15)) return fail_arg("K > 32768: outside the consumer's limit");
  if (M > INT32_MAX / 2) return fail_arg("M too large");
  const hipStream_t s = (hipStream_t)stream;
  const bool u8 = a_code_dtype == MCTQ_CODE_U8, block = M <= kRowsumBlockRows;
  const dim3 grid((unsigned)(block ? M : (M + 3) / 4));
  const int8_t* a = static_cast<const int8_t*>(a_codes);
#define MCTQ_ROWSUM(U8_, BLOCK_) \
  hipLaunchKernelGGL((codes_rowsum_kernel<U8_, BLOCK_>), grid, dim3(kRowsumThreads), 0, s, a, a_rowsum, (int)M, (int)K, (int)a_zero_point)
  if (u8) { if (block) MCTQ_ROWSUM(true, true); else MCTQ_ROWSUM(true, false); }
  else { if (block) MCTQ_ROWSUM(false, true); else MCTQ_ROWSUM(false, false); }
#undef MCTQ_ROWSUM
  note_launch("codes_rowsum", block ? (u8 ? "u8 block per row" : "i8 block per row") : (u8 ? "u8 wave per row" : "i8 wave per row"), 1, 0, 1, 4);
  return check_launch("mctq_codes_rowsum");
}

int mctq_qlinear_i8_zp(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                       const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                       void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                       int32_t y_quant_max, const int32_t* w_zero_points, const int32_t* a_rowsum, int64_t M, int64_t N,
                       int64_t K, void* stream) {
  MCTQ_QL_CALL(w_codes, w_zero_points, a_rowsum);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  return qlinear_dispatch(c, a_code_dtype, kQlNoZeroPoints);
}

int mctq_qlinear_w4a8_zp(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                         const uint8_t* w_codes4, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                         void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                         int32_t y_quant_max, const int32_t* w_zero_points, const int32_t* a_rowsum, int64_t M, int64_t N,
                         int64_t K, void* stream) {
  MCTQ_QL_CALL(w_codes4, w_zero_points, a_rowsum);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  return qlinear_packed4(c, a_code_dtype, true, nullptr);
}

int mctq_qlinear_i8_res(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                        const void* residual, int32_t r_code_dtype, float r_scale, int32_t r_zero_point, int32_t relu,
                        void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                        int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream) {
  MCTQ_QL_CALL(w_codes, nullptr, nullptr);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  // the residual's own checks, for a problem that is not empty and whose extents ql_check_call will not refuse
  if (M > 0 && N > 0 && M <= INT32_MAX / 2 && N <= INT32_MAX / 2) {
    if (!residual) return fail_arg("residual is NULL");
    if (r_code_dtype >= 0) {                   // the residual as codes: mctq_fq_join_rc_f32's checks
      if (int rc = residual_form_check(r_code_dtype, r_zero_point, r_scale)) return rc;
    } else if (((uintptr_t)residual & 3u) != 0) {
      return fail_arg("a float32 residual must be 4-byte aligned");
    }
    if (y) {                                   // the two byte ranges: a block would read residuals another has overwritten
      const size_t elems = (size_t)M * (size_t)N;
      if (ranges_overlap(y, elems * (y_code_dtype < 0 ? 4u : 1u), residual, elems * (r_code_dtype < 0 ? 4u : 1u)))
        return fail_arg("y overlaps the residual");
    }
  }
  c.res = QlRes{residual, r_code_dtype < 0 ? 1 : r_code_dtype == MCTQ_CODE_I8 ? 2 : 3, (int)r_zero_point, r_scale, relu != 0, 0};
  return qlinear_dispatch(c, a_code_dtype, kQlNoResidual);
}

int mctq_qlinear_i8_act(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                        void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                        int32_t y_quant_max, int32_t act, int64_t M, int64_t N, int64_t K, void* stream) {
  if (act != 1 && act != 2) return fail_arg("act must be 1 (hardswish) or 2 (hardsigmoid)");
  if (y_code_dtype < 0) return fail_arg("bad y_code_dtype");      // an activation leaves as codes only
  MCTQ_QL_CALL(w_codes, nullptr, nullptr);
  if (int rc = ql_output_form(c.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  c.res.act = act;
  return qlinear_dispatch(c, a_code_dtype, kQlNoActivation);
}
#undef MCTQ_QL_CALL

#ifdef MCTQ_QL_STAMP
int mctq_debug_ql_stamps(unsigned long long* out16x8) {      // diagnostic build only
  return -(int)hipMemcpyFromSymbol(out16x8, HIP_SYMBOL(mctq::g_ql_stamp), sizeof(unsigned long long) * 16 * 8);
}
#endif

}  // extern "C"
