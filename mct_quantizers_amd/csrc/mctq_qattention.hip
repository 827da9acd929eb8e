// mctq_qattention.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// The core of an attention block on codes in one launch: scores = Q.K^T into holder A0's codes, [pre-table A0 -> A,] the integer
// softmax of mctq_codes_softmax.hip into holder B's codes, context = P.V.  The result is, byte for byte, that of the three launches
//     s = mctq_qmatmul_i8(q, k, NT, codes of A0);  p = mctq_codes_softmax(s, pre, E, pad to 16);  y = mctq_qmatmul_i8(p, v, NN)
// because both integer sums are exact, S of the softmax is an exact integer, and every float32 step (the two epilogue
// multiplies, ql_code, one division per element) is the same single IEEE operation: this unit shares the code of those steps with
// the two units (mctq_qmatmul.hpp, mctq_codes_softmax.hpp, mctq_consumer.hpp) and is compiled, like the softmax unit, without
// packed float32 instructions.  The [T x T] codes never reach memory.
//
// Work split.  Grid x = ceil(M / 64), z = B0 * B1.  A workgroup of 256 lanes owns 64 query rows of one head, each of its four
// waves 16 of them from the scores to the context.  Rows beyond M are computed from the clamped row M - 1 and never stored; all
// four waves stay in every phase (barriers), the idle waves of the last row block included.
//
// The strip.  LDS holds the workgroup's 64 rows x Tp64 = 64 * ceil(T / 64) codes, first A's, then (in place) B's.  A wave's 16
// rows are stored chunk-major, [c = key / 16][row][16 bytes]: byte address c * 256 + row * 16 + key % 16 inside the wave's own
// Tp64 * 16 bytes.  Bank argument: both wide readers -- phase 3's A fragment (lane l: row l & 15, chunk 4 * step + (l >> 4)) and
// phase 2 (lane l: row l & 15, chunks (l >> 4) + 4 u) -- are one ds_read_b128 at c * 256 + row * 16, exactly the address form of
// the NN tile of mctq_qmatmul.hip: whichever 16 lanes the instruction serves together read 16 different rows, possibly of two
// neighbouring chunks, and 256 is the bank row, so they hit the 16 different 16-byte slots -- all 64 banks once.  A row-major strip
// would need a pitch of 16 * odd bytes and still collide where a group mixes two chunks (rows 11 and 12 at pitch Tp64 + 16); the
// chunk-major form needs no padding at all.  Phase 1 does not write single bytes: a lane holds the codes of rows 4 * kb .. + 3 of
// ONE key, the four lanes of a quad hold four neighbouring keys, so a 4 x 4 byte transpose across the quad (four quad-broadcast
// DPP moves) gives every lane the dword (row 4 * kb + (l & 3), keys 4 * (r >> 2) .. + 3): one ds_write_b32 per lane, the wave's 64
// lanes on 64 consecutive dwords -- no conflict, where four ds_write_b8 per lane would put four lanes on every dword.
//
// Phase 1, scores (NT, as qmatmul_kernel): the wave's Q fragments (D <= 128: two K steps) are loaded once and stay in registers,
// chunks beyond D replaced by zero-point bytes (matmul_k_chunk); per tile of 16 keys the K fragments come straight from global
// memory (all four waves read the same rows; one tile ahead in flight); v_mfma_i32_16x16x64_i8; the zero-point terms by ones-MFMAs
// (rowsum_q' once per wave, colsum_k' per key tile), each skipped where that z' is 0 (a uniform branch -- see "Decisions");
// float(acc) * (sq * sk), ql_code in A0's form, the pre-table.  Keys >= T are computed from the clamped key T - 1; phase 2 never
// lets them into the max or the sum.
// Phase 2, softmax in place: lane l takes row l & 15 and the chunks (l >> 4) + 4 u, kept in registers through the three passes of
// mctq_codes_softmax.hpp; max and sum cross the row's four lanes by __shfl_xor 16 and 32.  A lane sums at most 16 elements in u32
// (one chunk) and adds chunks as u64.  Columns T .. Tp64 - 1 are written as B's zero-point code: phase 3 adds (zb - zb) * .. = 0.
// Phase 3, context (NN, as qmatmul_kernel): A fragments are one ds_read_b128 from the strip; V goes through LDS with that kernel's
// transpose (dwords of 4 consecutive k rows, six v_perm_b32, image [kb][n][16 bytes], rotated write order), the tile widened to
// Dv <= 128 columns (8 KiB) -- one tile serves all four waves and all Dv / 16 <= 8 accumulators of a wave.  Rows k >= T of V are
// replaced by zv bytes; the next step's global loads are in flight across the two barriers.
//
// Decisions, and their basis.
//   Strip templates STEPS = 4 / 8 / 16 K steps (T <= 256 / 512 / 1024): LDS 25.25 / 41.25 / 73.25 KiB a workgroup, so 6 / 3 / 2
//     workgroups fit the 160 KiB of a CU, and phase 2 keeps STEPS chunks (4 * STEPS registers) a lane.  Chosen from that arithmetic
//     and the compiled resources below; no other set has been measured.
//   Phase 2 lane split: four lanes per row (not one wave per row in turn).  With the chunk-major strip a wave-per-row read would
//     put all 64 lanes on one 16-byte slot (stride 256); four lanes per row is the conflict-free address form above and needs two
//     shuffles instead of six.  Chosen from the bank argument, not from a measurement.
//   Zero-point flags: uniform branches on kernel arguments instead of template flags (the ones-MFMAs are skipped all the same):
//     3 instances instead of 48.
//
// Compiled resources (hipcc -O3 --offload-arch=gfx950 with the library's flags, -Rpass-analysis=kernel-resource-usage; scratch 0
// bytes in every instance):
//     STEPS     VGPRs   AGPRs   LDS bytes   waves / SIMD
//       4        106      68       25856         2
//       8        108      68       42240         2
//      16        106      68       75008         2
// The 174 registers, not LDS, set the occupancy today: two workgroups a CU in every instance (the 75008-byte strip allows two as
// well).  Measured once (one MI355X; tools/attention_consumer_probe.py, table in profiles/EXPERIMENTS.md) against the three launches:
// 1.4 - 2.3 x faster on 12 heads x T = 128, 197, 384 at batch 1 and 64; 0.94 x and 0.90 x -- slower -- on 16 x 1024 x 1024 at batch
// 1 and 64, where phase 1 reads K once per 64 rows and two workgroups a CU hide little of it.  The templates and the lane split were
// not chosen from these numbers.
#include "mctq_qmatmul.hpp"                // i32x4, matmul_k_chunk, matmul_transpose4, matmul_view_check
#include "mctq_codes_softmax.hpp"          // softmax_chunk_order / _sum / _codes / _pad

namespace mctq {

constexpr int kAttentionMaxT = 1024, kAttentionMaxD = 128;

struct AttentionArgs {
  const uint8_t* q;
  const uint8_t* k;
  const uint8_t* v;
  void* y;
  const uint32_t* etab;                            // E[256]
  const uint32_t* pre;                             // the pre-table A0 -> A as 64 dwords, or nullptr
  int64_t q_s0, q_s1, q_sr, k_s0, k_s1, k_sr, v_s0, v_s1, v_sr;      // byte strides of B0, B1 and rows
  FastDiv b1;                                      // blockIdx.z = b0 * B1 + b1
  uint32_t M;
  int32_t T, D, Dv, steps;                         // steps = ceil(T / 64)
  uint32_t flip_q, flip_k, flip_p, flip_v;         // 0x80808080 for uint8 codes, else 0 (into int8: mctq_qmatmul.hip)
  uint32_t pad_q, pad_k, pad_p, pad_v;             // the zero-point code in all four bytes (before the flip)
  uint32_t order_a;                                // 0x80 for int8 codes of A (into unsigned order: mctq_codes_softmax.hip), else 0
  int32_t zq, zk, zp, zv;                          // z' of each operand
  float scale_s, scale_y;                          // sq * sk, sb * sv
  QlOut os, op, oy;                                // A0's form, B's form, the output form
};

// byte `sel` (0 .. 3) of the four dwords, into one dword
__device__ __forceinline__ uint32_t attention_gather_byte(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int sel) {
  const int sh = 8 * sel;
  return ((w0 >> sh) & 0xffu) | (((w1 >> sh) & 0xffu) << 8) | (((w2 >> sh) & 0xffu) << 16) | (((w3 >> sh) & 0xffu) << 24);
}

// 1 <= T <= 64 * STEPS, D and Dv multiples of 16 up to 128, M >= 1 (the launcher's checks)
template <int STEPS>
__global__ __launch_bounds__(kThreads) void qattention_kernel(AttentionArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t strip[STEPS * 1024];          // 4 waves x 16 rows x 64 * STEPS bytes
  __shared__ __attribute__((aligned(16))) uint32_t vtile[4 * kAttentionMaxD * 4];  // [kb][n][16 bytes]
  __shared__ uint32_t etab[256];
  __shared__ uint32_t pre[64];
  const uint8_t* __restrict__ pre8 = reinterpret_cast<const uint8_t*>(pre);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kb = lane >> 4;
  const uint32_t m0 = blockIdx.x * 64u + (uint32_t)wave * 16u;
  uint32_t bi1;
  const uint32_t bi0 = a.b1.divmod(blockIdx.z, bi1);
  const uint8_t* __restrict__ gq = a.q + (int64_t)bi0 * a.q_s0 + (int64_t)bi1 * a.q_s1;
  const uint8_t* __restrict__ gk = a.k + (int64_t)bi0 * a.k_s0 + (int64_t)bi1 * a.k_s1;
  const uint8_t* __restrict__ gv = a.v + (int64_t)bi0 * a.v_s0 + (int64_t)bi1 * a.v_s1;
  uint8_t* const sw = reinterpret_cast<uint8_t*>(strip) + wave * (STEPS * 1024);     // this wave's 16 rows
  const bool has_pre = a.pre != nullptr;
  const bool two = a.D > 64;                                                    // a second K step of Q and K
  const int lastd = a.D / 16 - 1;
  const i32x4 zero = {0, 0, 0, 0}, ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

  // the tables, this lane's Q fragments and the first K tile: every load is issued before the barrier
  const uint32_t te = a.etab[tid];
  uint32_t tp = 0;
  if (has_pre) tp = a.pre[tid & 63];
  const uint8_t* __restrict__ qrow = gq + (int64_t)min(m0 + (uint32_t)r, a.M - 1u) * a.q_sr;
  i32x4 qf0 = matmul_k_chunk(qrow, kb, lastd, a.pad_q), qf1 = zero;
  if (two) qf1 = matmul_k_chunk(qrow, 4 + kb, lastd, a.pad_q);
  auto load_k = [&](int j, i32x4& c0, i32x4& c1) {
    const uint8_t* __restrict__ krow = gk + (int64_t)min(16 * j + r, a.T - 1) * a.k_sr;     // keys >= T: the last key, masked in phase 2
    c0 = matmul_k_chunk(krow, kb, lastd, a.pad_k);
    if (two) c1 = matmul_k_chunk(krow, 4 + kb, lastd, a.pad_k);
  };
  i32x4 kf0, kf1 = zero;
  load_k(0, kf0, kf1);
  etab[tid] = te;
  if (has_pre) pre[tid & 63] = tp;                                              // (the four waves write the same 64 dwords)
  __syncthreads();

  // ---- phase 1: the codes of A for 16 rows x T keys, into the strip -------------------------------------------------------
  {
    const int fq = (int)a.flip_q, fk = (int)a.flip_k;
    qf0 = qf0 ^ fq; qf1 = qf1 ^ fq;
    i32x4 rs = zero;                                                            // every column: the row's sum of q'
    if (a.zk != 0) {
      rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf0, ones, rs, 0, 0, 0);
      if (two) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf1, ones, rs, 0, 0, 0);
    }
    const unsigned tail = (two ? 128u : 64u) * (unsigned)a.zq * (unsigned)a.zk;
    const int tiles = (a.T + 15) / 16, quad = r & 3;
    uint32_t* const wr = reinterpret_cast<uint32_t*>(sw + (4 * kb + quad) * 16 + 4 * (r >> 2));
    for (int j = 0; j < tiles; ++j) {
      i32x4 next0 = kf0, next1 = kf1;
      if (j + 1 < tiles) load_k(j + 1, next0, next1);
      const i32x4 b0 = kf0 ^ fk, b1 = kf1 ^ fk;
      i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf0, b0, zero, 0, 0, 0), cs = zero;
      if (two) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf1, b1, acc, 0, 0, 0);
      if (a.zq != 0) {                                                          // every row: the key's sum of k'
        cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b0, cs, 0, 0, 0);
        if (two) cs = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b1, cs, 0, 0, 0);
      }
      // key r of the tile, rows 4 * kb + i.  Wrapping arithmetic: only the total is known to fit (mctq_qmatmul.hip)
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned c = 0u - tail + (unsigned)a.zq * (unsigned)cs[i] + (unsigned)a.zk * (unsigned)rs[i];
        const float out = (float)(int)((unsigned)acc[i] - c) * a.scale_s;
        uint32_t code = (uint32_t)ql_code(out, a.os) & 0xffu;
        if (has_pre) code = pre8[code];
        w |= code << (8 * i);
      }
      // across the quad: this lane's dword becomes row 4 * kb + quad, keys 4 * (r >> 2) .. + 3
      const uint32_t w0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)w, 0x00, 0xf, 0xf, true);
      const uint32_t w1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)w, 0x55, 0xf, 0xf, true);
      const uint32_t w2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)w, 0xaa, 0xf, 0xf, true);
      const uint32_t w3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)w, 0xff, 0xf, 0xf, true);
      wr[j * 64] = attention_gather_byte(w0, w1, w2, w3, quad);
      kf0 = next0; kf1 = next1;
    }
  }
  __syncthreads();

  // ---- phase 2: softmax of the 16 rows in place, four lanes a row ------------------------------------------------------------
  {
    u32x4 v[STEPS];
    uint32_t mx = 0;
#pragma unroll
    for (int u = 0; u < STEPS; ++u)
      if (u < a.steps) {
        const int c = kb + 4 * u;
        v[u] = *reinterpret_cast<const u32x4*>(sw + c * 256 + r * 16);
        softmax_chunk_order<false>(v[u], pre8, a.order_a, 0, a.T - 16 * c, mx);
      }
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 16));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 32));
    unsigned long long sum = 0;
#pragma unroll
    for (int u = 0; u < STEPS; ++u)
      if (u < a.steps) sum += softmax_chunk_sum(v[u], etab, mx, 0, a.T - 16 * (kb + 4 * u));
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float fs = (float)sum;                                                // >= 2^24: the row's max adds E[0]
#pragma unroll
    for (int u = 0; u < STEPS; ++u)
      if (u < a.steps) {
        const int c = kb + 4 * u;
        const u32x4 codes = softmax_chunk_codes(v[u], etab, mx, fs, a.op);
        *reinterpret_cast<u32x4*>(sw + c * 256 + r * 16) = softmax_chunk_pad(codes, min(max(a.T - 16 * c, 0), 16), a.pad_p);
      }
  }
  __syncthreads();

  // ---- phase 3: context = P . V, V through LDS ----------------------------------------------------------------------------------
  const int nt = a.Dv / 16;                                                     // N tiles: 1 .. 8, uniform
  const bool wide = a.Dv > 64;                                                  // a second half of 64 columns in the tile
  const int kq = tid >> 4, nq = tid & 15;                                       // this thread's 4 k rows and 4 columns of a half
  const int rot = (nq >> 1) & 3;
  // columns beyond Dv: the last whole dword inside the row, written to tile slots no fragment reads
  const uint8_t* __restrict__ vcol0 = gv + min(4 * nq, a.Dv - 4);
  const uint8_t* __restrict__ vcol1 = gv + min(64 + 4 * nq, a.Dv - 4);
  auto load_v = [&](int k0, uint32_t (&raw0)[4], uint32_t (&raw1)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 4 * kq + i;
      const int64_t off = (int64_t)min(k, a.T - 1) * a.v_sr;
      const uint32_t x0 = *reinterpret_cast<const uint32_t*>(vcol0 + off);
      raw0[i] = k < a.T ? x0 : a.pad_v;                                         // rows behind T hold zv: they add (p - zb) * 0
      if (wide) {
        const uint32_t x1 = *reinterpret_cast<const uint32_t*>(vcol1 + off);
        raw1[i] = k < a.T ? x1 : a.pad_v;
      }
    }
  };
  i32x4 acc[8], cs[8], rs = zero;
#pragma unroll
  for (int t = 0; t < 8; ++t) { acc[t] = zero; cs[t] = zero; }
  const int fp = (int)a.flip_p, fv = (int)a.flip_v;
  uint32_t raw0[4], raw1[4] = {0u, 0u, 0u, 0u};
  load_v(0, raw0, raw1);
  uint32_t* const vw = vtile + (kq >> 2) * (kAttentionMaxD * 4) + 16 * nq + (kq & 3);
  for (int s = 0; s < a.steps; ++s) {
    uint32_t next0[4], next1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { next0[i] = raw0[i]; next1[i] = raw1[i]; }
    if (s + 1 < a.steps) load_v(64 * (s + 1), next0, next1);
    uint32_t o0[4], o1[4];
    matmul_transpose4(raw0, rot, o0);
    matmul_transpose4(raw1, rot, o1);
    __syncthreads();                                                            // the step before has read its fragments
#pragma unroll
    for (int j = 0; j < 4; ++j) vw[4 * ((j + rot) & 3)] = o0[j];
    if (wide) {
#pragma unroll
      for (int j = 0; j < 4; ++j) vw[256 + 4 * ((j + rot) & 3)] = o1[j];
    }
    __syncthreads();
    const i32x4 pf = *reinterpret_cast<const i32x4*>(sw + (4 * s + kb) * 256 + r * 16) ^ fp;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (t < nt) {
        const i32x4 b8 = *reinterpret_cast<const i32x4*>(vtile + kb * (kAttentionMaxD * 4) + (16 * t + r) * 4) ^ fv;
        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pf, b8, acc[t], 0, 0, 0);
        if (a.zp != 0) cs[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b8, cs[t], 0, 0, 0);
      }
    }
    if (a.zv != 0) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(pf, ones, rs, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { raw0[i] = next0[i]; raw1[i] = next1[i]; }
  }

  // epilogue: column l & 15 of every tile, rows 4 * (l >> 4) + i (qmatmul_kernel's)
  const unsigned tail = (unsigned)(64 * a.steps) * (unsigned)a.zp * (unsigned)a.zv;
  const uint32_t mrow = m0 + 4u * (uint32_t)kb;
  const int64_t ybase = (int64_t)blockIdx.z * a.M;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t < nt) {
      const int n = 16 * t + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned c = 0u - tail + (unsigned)a.zp * (unsigned)cs[t][i] + (unsigned)a.zv * (unsigned)rs[i];
        const float out = (float)(int)((unsigned)acc[t][i] - c) * a.scale_y;
        const uint32_t m = mrow + (uint32_t)i;
        if (m < a.M) ql_store(a.y, (ybase + m) * a.Dv + n, out, a.oy);
      }
    }
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_qattention_i8(const void* q_codes, int32_t q_code_dtype, int32_t q_zero_point, float q_scale, int64_t q_stride_b0,
                       int64_t q_stride_b1, int64_t q_stride_row, const void* k_codes, int32_t k_code_dtype, int32_t k_zero_point,
                       float k_scale, int64_t k_stride_b0, int64_t k_stride_b1, int64_t k_stride_row, const void* v_codes,
                       int32_t v_code_dtype, int32_t v_zero_point, float v_scale, int64_t v_stride_b0, int64_t v_stride_b1,
                       int64_t v_stride_row, int32_t s_code_dtype, float s_scale, int32_t s_zero_point, int32_t s_quant_min,
                       int32_t s_quant_max, int32_t a_code_dtype, int32_t p_code_dtype, float p_scale, int32_t p_zero_point,
                       int32_t p_quant_min, int32_t p_quant_max, const void* exp_table, const void* pre_table, void* y,
                       int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                       int64_t batch0, int64_t batch1, int64_t m, int64_t t, int64_t d, int64_t dv, void* stream) {
  if (int rc = form_check(q_code_dtype, q_zero_point, q_scale, {"q_code_dtype", "q_zero_point", "q_code_dtype", "q_scale"})) return rc;
  if (int rc = form_check(k_code_dtype, k_zero_point, k_scale, {"k_code_dtype", "k_zero_point", "k_code_dtype", "k_scale"})) return rc;
  if (int rc = form_check(v_code_dtype, v_zero_point, v_scale, {"v_code_dtype", "v_zero_point", "v_code_dtype", "v_scale"})) return rc;
  if (int rc = form_check(p_code_dtype, p_zero_point, p_scale, {"p_code_dtype", "p_zero_point", "p_code_dtype", "p_scale"})) return rc;
  if (int rc = form_check_dtype(s_code_dtype, "s_code_dtype")) return rc;
  if (int rc = form_check_dtype(a_code_dtype, "a_code_dtype")) return rc;
  if (int rc = form_check_scale(s_scale, "s_scale")) return rc;
  AttentionArgs a;
  if (int rc = ql_output_form(a.os, s_code_dtype, s_scale, s_zero_point, s_quant_min, s_quant_max)) return rc;
  if (int rc = ql_output_form(a.op, p_code_dtype, p_scale, p_zero_point, p_quant_min, p_quant_max)) return rc;
  if (int rc = ql_output_form(a.oy, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  if (!pre_table && a_code_dtype != s_code_dtype) return fail_arg("without a pre_table the scores are A's codes: a_code_dtype must be s_code_dtype");
  if (batch0 < 0 || batch1 < 0 || m < 0 || t < 0) return fail_arg("negative extent");
  if (d < 16 || d > kAttentionMaxD || d % 16 != 0) return fail_arg("D must be a multiple of 16 in 16 .. 128: outside the fused kernel's limit");
  if (dv < 16 || dv > kAttentionMaxD || dv % 16 != 0) return fail_arg("Dv must be a multiple of 16 in 16 .. 128: outside the fused kernel's limit");
  if (t > kAttentionMaxT) return fail_arg("T above 1024: outside the fused kernel's limit");
  if (m > INT32_MAX - 64) return fail_arg("M too large for one launch");
  if (batch0 > 65535 || batch1 > 65535 || batch0 * batch1 > 65535)
    return fail_arg("batch0 * batch1 > 65535: too many grid slices (split the batch)");
  int64_t q_span = 0, k_span = 0, v_span = 0;
  if (int rc = matmul_view_check("q_codes", q_stride_b0, q_stride_b1, q_stride_row, batch0, batch1, m, d, q_span)) return rc;
  if (int rc = matmul_view_check("k_codes", k_stride_b0, k_stride_b1, k_stride_row, batch0, batch1, t, d, k_span)) return rc;
  if (int rc = matmul_view_check("v_codes", v_stride_b0, v_stride_b1, v_stride_row, batch0, batch1, t, dv, v_span)) return rc;
  if (batch0 == 0 || batch1 == 0 || m == 0 || t == 0) return 0;                 // nothing to write (T == 0: a softmax over no element)
  if (!q_codes || !k_codes || !v_codes || !y) return fail_arg("NULL pointer");
  if (!exp_table) return fail_arg("exp_table is NULL");
  if ((((uintptr_t)q_codes | (uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)y) & 15u) != 0)
    return fail_arg("codes and output must be 16-byte aligned");
  if (((uintptr_t)exp_table & 3u) != 0 || ((uintptr_t)pre_table & 3u) != 0) return fail_arg("the tables must be 4-byte aligned");
  const size_t y_bytes = (size_t)(batch0 * batch1 * m * dv) * (a.oy.mode == 0 ? 4 : 1);   // < 2^16 * 2^31 * 2^7 * 4
  if (ranges_overlap(y, y_bytes, q_codes, (size_t)q_span) || ranges_overlap(y, y_bytes, k_codes, (size_t)k_span) ||
      ranges_overlap(y, y_bytes, v_codes, (size_t)v_span))
    return fail_arg("the output overlaps an operand");
  if (ranges_overlap(y, y_bytes, exp_table, 1024u) || (pre_table && ranges_overlap(y, y_bytes, pre_table, 256u)))
    return fail_arg("the output overlaps a table");
  const bool q_u8 = q_code_dtype == MCTQ_CODE_U8, k_u8 = k_code_dtype == MCTQ_CODE_U8, p_u8 = p_code_dtype == MCTQ_CODE_U8,
             v_u8 = v_code_dtype == MCTQ_CODE_U8;
  a.q = static_cast<const uint8_t*>(q_codes); a.k = static_cast<const uint8_t*>(k_codes); a.v = static_cast<const uint8_t*>(v_codes);
  a.y = y;
  a.etab = static_cast<const uint32_t*>(exp_table); a.pre = static_cast<const uint32_t*>(pre_table);
  a.q_s0 = q_stride_b0; a.q_s1 = q_stride_b1; a.q_sr = q_stride_row;
  a.k_s0 = k_stride_b0; a.k_s1 = k_stride_b1; a.k_sr = k_stride_row;
  a.v_s0 = v_stride_b0; a.v_s1 = v_stride_b1; a.v_sr = v_stride_row;
  a.b1 = FastDiv::make((uint32_t)batch1);
  a.M = (uint32_t)m; a.T = (int32_t)t; a.D = (int32_t)d; a.Dv = (int32_t)dv; a.steps = (int32_t)((t + 63) / 64);
  a.flip_q = q_u8 ? 0x80808080u : 0u; a.flip_k = k_u8 ? 0x80808080u : 0u;
  a.flip_p = p_u8 ? 0x80808080u : 0u; a.flip_v = v_u8 ? 0x80808080u : 0u;
  a.pad_q = (uint32_t)(q_zero_point & 0xff) * 0x01010101u; a.pad_k = (uint32_t)(k_zero_point & 0xff) * 0x01010101u;
  a.pad_p = (uint32_t)(p_zero_point & 0xff) * 0x01010101u; a.pad_v = (uint32_t)(v_zero_point & 0xff) * 0x01010101u;
  a.order_a = a_code_dtype == MCTQ_CODE_I8 ? 0x80u : 0u;
  a.zq = q_u8 ? q_zero_point - 128 : q_zero_point; a.zk = k_u8 ? k_zero_point - 128 : k_zero_point;
  a.zp = p_u8 ? p_zero_point - 128 : p_zero_point; a.zv = v_u8 ? v_zero_point - 128 : v_zero_point;
  a.scale_s = q_scale * k_scale;                                                // one float32 multiply each, as mctq_qmatmul_i8
  a.scale_y = p_scale * v_scale;
  const dim3 grid((unsigned)((m + 63) / 64), 1u, (unsigned)(batch0 * batch1));
  const hipStream_t s = (hipStream_t)stream;
  if (a.steps <= 4) hipLaunchKernelGGL((qattention_kernel<4>), grid, dim3(kThreads), 0, s, a);
  else if (a.steps <= 8) hipLaunchKernelGGL((qattention_kernel<8>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((qattention_kernel<16>), grid, dim3(kThreads), 0, s, a);
  static thread_local char op_text[48];
  snprintf(op_text, sizeof(op_text), "%s x %s . %s x %s%s", q_u8 ? "u8" : "i8", k_u8 ? "u8" : "i8", p_u8 ? "u8" : "i8",
           v_u8 ? "u8" : "i8", pre_table ? " pre" : "");
  note_launch("qattention", op_text, (a.zq != 0 ? 1 : 0) + (a.zk != 0 ? 2 : 0) + (a.zp != 0 ? 4 : 0) + (a.zv != 0 ? 8 : 0), 0, 1,
              a.oy.mode == 0 ? 4 : 1);
  return check_launch("mctq_qattention_i8");
}

}  // extern "C"
