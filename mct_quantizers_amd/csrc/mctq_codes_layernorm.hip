// mctq_codes_layernorm.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// LayerNorm over the rows of a code tensor, between two activation holders A and B: A-codes c_j (j < L) -> B-codes.  Mean and
// variance are exact integers, so that the result does not depend on the order of a sum.  Per row, A of the form (s_a, zp_a):
//     u_j    = c_j - zp_a                                    |u_j| <= 255
//     S1     = sum_j u_j,  S2 = sum_j u_j^2                  exact integers
//     n_j    = L * u_j - S1                                  exact, |n_j| <= 510 L < 2^24
//     V      = L * S2 - S1^2                                 exact int64, >= 0
//     r      = float32(1.0 / sqrt(float64(V) + K))           K = eps * L^2 / s_a^2 from the host; three IEEE float64 operations
//     y_j    = (float32(n_j) * r) * gamma_j + beta_j         two float32 multiplies and one add, not fused
//     code_j = ql_code(y_j)                                  clamp(rint(y_j * (1 / s_b)) + zp_b, qmin, qmax)
// which is (x - mean) / sqrt(var + eps) of x = u * s_a with numerator and denominator multiplied by L / s_a.  Both forms below,
// any split over lanes, and the torch route of ops.codes_layernorm give the same bytes.
//
// Rows are L % 16 == 0 bytes at pitch L in 16-byte aligned buffers: lane l owns the 16-byte chunks l, l + LANES, .. of its row
// (CH = 1 or 2 of them), loads each once, keeps it in registers through both passes and stores 16 codes over it once.  int8
// codes are flipped to unsigned bytes b (zero point zb = zp_a + 128); a lane's sum b and sum b^2 are two v_dot4_u32_u8 per dword
// (against 0x01010101 and against the dword itself; both fit 32 bits for L <= 8192), and S1 = sum b - L zb,
// S2 = sum b^2 - 2 zb sum b + L zb^2 are formed once per row in 64-bit integers behind the reduction.
//
// Wave form: one wave per row at a time (LANES = 64: L <= 1024 with CH = 1, <= 2048 with CH = 2), four waves per workgroup;
// the sums cross the wave by __shfl_xor, no LDS.  Block form: one workgroup per row at a time (LANES = 256: L <= 4096, <= 8192);
// the four waves' sums meet in LDS, in one of two slots by the parity of the round, so that one barrier per row is enough.
// Both are persistent: worker w of W takes rows w, w + W, ..; each lane loads its 16 * CH gammas and betas into registers
// once, before the row loop, and the next row's chunks are loaded before the current row's sums are formed.
#include "mctq_consumer.hpp"               // u32x4, QlOut, ql_code, form_check, ranges_overlap

namespace mctq {

extern int g_layernorm_form;               // tuning key "layernorm_form" (mctq_misc.hip): 0 = auto, 1 = wave form, 2 = block form
extern int g_layernorm_blocks;             // tuning key "layernorm_blocks": 0 = auto, otherwise the grid size

constexpr int kLayerNormMaxLength = 8192;  // 2 chunks x 256 lanes x 16 bytes; sum b^2 <= 8192 * 255^2 < 2^32
constexpr int kLayerNormWaveChunks = 128;  // 2 chunks x 64 lanes

struct LayerNormArgs {
  const u32x4* in;
  u32x4* out;
  const float4* gamma;
  const float4* beta;
  uint32_t rows, chunks;                   // chunks = L / 16
  uint32_t flip;                           // 0x80808080 for int8 codes, 0 for uint8
  int32_t L, zb;                           // zb = zp_a + (int8 ? 128 : 0)
  double k_term;
  QlOut o;
};

template <int CH, bool BLOCK>
__global__ __launch_bounds__(kThreads) void codes_layernorm_kernel(LayerNormArgs a) {
  constexpr uint32_t LANES = BLOCK ? (uint32_t)kThreads : 64u;
  __shared__ uint32_t wave_sums[2][2][4];                                         // [parity of the round][sum b, sum b^2][wave]
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = BLOCK ? tid : (tid & 63u);
  const uint32_t workers = BLOCK ? gridDim.x : gridDim.x * 4u;
  uint32_t row = BLOCK ? blockIdx.x : blockIdx.x * 4u + wave;                     // (uniform over a wave; over the workgroup if BLOCK)

  // the lane's parameters, once: 16 gammas and 16 betas per chunk (a chunk beyond the row: none, and nothing is loaded or stored)
  bool valid[CH];
  float g[CH][16], be[CH][16];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const uint32_t c = lane + (uint32_t)u * LANES;
    valid[u] = c < a.chunks;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 gv = {0.0f, 0.0f, 0.0f, 0.0f}, bv = gv;
      if (valid[u]) { gv = a.gamma[4u * c + (uint32_t)q]; bv = a.beta[4u * c + (uint32_t)q]; }
      g[u][4 * q] = gv.x; g[u][4 * q + 1] = gv.y; g[u][4 * q + 2] = gv.z; g[u][4 * q + 3] = gv.w;
      be[u][4 * q] = bv.x; be[u][4 * q + 1] = bv.y; be[u][4 * q + 2] = bv.z; be[u][4 * q + 3] = bv.w;
    }
  }
  u32x4 v[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    v[u] = u32x4{0u, 0u, 0u, 0u};
    if (row < a.rows && valid[u]) v[u] = a.in[row * a.chunks + lane + (uint32_t)u * LANES];     // < 2^27 chunks: the launcher's check
  }

  for (uint32_t round = 0; row < a.rows; ++round, row += workers) {
    const uint32_t next = row + workers;
    u32x4 nv[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      nv[u] = u32x4{0u, 0u, 0u, 0u};
      if (next < a.rows && valid[u]) nv[u] = a.in[next * a.chunks + lane + (uint32_t)u * LANES];
    }

    // pass 1: the codes as unsigned bytes; the lane's sum b and sum b^2 (a chunk beyond the row adds 0)
    uint32_t sb = 0, sq = 0;
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t w = valid[u] ? (v[u][q] ^ a.flip) : 0u;
        v[u][q] = w;
        sb = __builtin_amdgcn_udot4(w, 0x01010101u, sb, false);
        sq = __builtin_amdgcn_udot4(w, w, sq, false);
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sb += (uint32_t)__shfl_xor((int)sb, off);
      sq += (uint32_t)__shfl_xor((int)sq, off);
    }
    if (BLOCK) {
      // the slot of round i is written again in round i + 2, behind the barrier of round i + 1, which every wave reaches only
      // after it has read round i's
      uint32_t (&slot)[2][4] = wave_sums[round & 1u];
      if ((tid & 63u) == 0) { slot[0][wave] = sb; slot[1][wave] = sq; }
      __syncthreads();
      sb = slot[0][0] + slot[0][1] + slot[0][2] + slot[0][3];
      sq = slot[1][0] + slot[1][1] + slot[1][2] + slot[1][3];
    }
    const int64_t L = a.L, zb = a.zb;
    const int64_t s1 = (int64_t)sb - L * zb;
    const int64_t s2 = (int64_t)sq - 2 * zb * (int64_t)sb + L * zb * zb;
    const int64_t var = L * s2 - s1 * s1;                                         // >= 0 (Cauchy-Schwarz, exact), < 2^47
    const float r = (float)(1.0 / sqrt((double)var + a.k_term));                  // IEEE add, square root and division, one rounding to float32

    // pass 2: n_j = L * b_j - (L * zb + S1), one convert, two multiplies and one add, the holder's code; 16 codes per chunk
    const int base = -(int)(L * zb + s1);
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      u32x4 codes;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int n = (int)((v[u][q] >> (8 * b)) & 0xffu) * a.L + base;
          const float xh = (float)n * r;
          const float y = xh * g[u][4 * q + b] + be[u][4 * q + b];               // (-ffp-contract=off: a multiply and an add)
          word |= ((uint32_t)ql_code(y, a.o) & 0xffu) << (8 * b);
        }
        codes[q] = word;
      }
      if (valid[u]) a.out[row * a.chunks + lane + (uint32_t)u * LANES] = codes;
      v[u] = nv[u];
    }
  }
}

template <bool BLOCK>
static void layernorm_launch(int ch, unsigned blocks, hipStream_t s, const LayerNormArgs& a) {
  if (ch == 1) hipLaunchKernelGGL((codes_layernorm_kernel<1, BLOCK>), dim3(blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((codes_layernorm_kernel<2, BLOCK>), dim3(blocks), dim3(kThreads), 0, s, a);
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_layernorm(const void* in, int32_t in_code_dtype, int32_t in_zero_point, void* out, int32_t out_code_dtype,
                         float out_scale, int32_t out_zero_point, int32_t out_quant_min, int32_t out_quant_max, int64_t rows,
                         int64_t length, const void* gamma, const void* beta, double k_term, void* stream) {
  if (rows < 0 || length < 0) return fail_arg("negative extent");
  if (int rc = form_check_dtype(in_code_dtype, "in_code_dtype")) return rc;
  if (int rc = form_check_zero_point(in_code_dtype, in_zero_point, "in_zero_point", "the input's type")) return rc;
  if (int rc = form_check_dtype(out_code_dtype, "out_code_dtype")) return rc;
  if (int rc = form_check_scale(out_scale, "out_scale")) return rc;
  if (int rc = form_check_zero_point(out_code_dtype, out_zero_point, "out_zero_point", "the output's type")) return rc;
  QlOut o;
  if (int rc = ql_output_form(o, out_code_dtype, out_scale, out_zero_point, out_quant_min, out_quant_max)) return rc;
  if (length % 16 != 0) return fail_arg("length must be a multiple of 16");
  if (length > kLayerNormMaxLength) return fail_arg("a row of more than 8192 codes");
  if (!(k_term > 0.0) || !__builtin_isfinite(k_term)) return fail_arg("k_term must be finite and positive");
  if (rows == 0 || length == 0) return 0;
  if (rows > INT32_MAX / length) return fail_arg("more than 2^31 - 1 bytes in one launch");
  if (!in) return fail_arg("in is NULL");
  if (!out) return fail_arg("out is NULL");
  if (!gamma) return fail_arg("gamma is NULL");
  if (!beta) return fail_arg("beta is NULL");
  if (((uintptr_t)in & 15u) != 0) return fail_arg("in must be 16-byte aligned");
  if (((uintptr_t)out & 15u) != 0) return fail_arg("out must be 16-byte aligned");
  if (((uintptr_t)gamma & 15u) != 0 || ((uintptr_t)beta & 15u) != 0) return fail_arg("gamma and beta must be 16-byte aligned");
  const size_t bytes = (size_t)(rows * length), param_bytes = (size_t)length * sizeof(float);
  if (ranges_overlap(out, bytes, in, bytes)) return fail_arg("out overlaps in");
  if (ranges_overlap(out, bytes, gamma, param_bytes)) return fail_arg("out overlaps gamma");
  if (ranges_overlap(out, bytes, beta, param_bytes)) return fail_arg("out overlaps beta");
  const CodeForm f = code_form(in_code_dtype, in_zero_point);
  const int64_t chunks = length / 16;
  // Auto: the wave form wherever it fits.  Measured (one MI355X; tools/layernorm_consumer_probe.py,
  // profiles/layernorm_consumer/probe.log, table in profiles/EXPERIMENTS.md) on six rows where both fit: the wave form won
  // three (11.3 against 19.0 us on [12608, 768], 11.6 against 19.3 us on [12608, 1024], 10.7 against 13.0 us on [8192, 768])
  // and tied the three batch-1 rows within their spread (10.7 - 11.4 us: the launch floor of the Python route); the block form
  // won none.
  const bool block = chunks > kLayerNormWaveChunks || g_layernorm_form == 2;
  const int64_t lanes = block ? kThreads : 64;
  const int ch = chunks <= lanes ? 1 : 2;
  // Auto grid: eight workgroups per CU, or one worker per row where that is fewer.  Measured in the same run: on [8192, 4096]
  // (block form) 2 / 4 / 8 workgroups per CU took 30.5 / 26.1 / 23.9 us and one workgroup per row 26.2 us; on [12608, 768] and
  // [12608, 1024] (wave form) 12.5 / 11.9 / 11.2 and 12.8 / 12.0 / 11.4 us, one wave per row 11.2 and 11.2 us (a tie with eight
  // per CU).  Four per CU, the first guess, is 8 % slower than eight on the block-form row.  A weak basis: the same launch with
  // the same eight-per-CU grid reads 25.5 us in that run's alternating column (the replaced chain between its rounds) and
  // 23.9 us timed alone, a gap as large as the effect; the grid columns were all timed alone, one after the other.
  const int64_t needed = block ? rows : (rows + 3) / 4, fill = (int64_t)cu_count() * 8;
  const unsigned blocks = (unsigned)(g_layernorm_blocks > 0 ? g_layernorm_blocks : needed < fill ? needed : fill);
  LayerNormArgs a;
  a.in = static_cast<const u32x4*>(in);
  a.out = static_cast<u32x4*>(out);
  a.gamma = static_cast<const float4*>(gamma);
  a.beta = static_cast<const float4*>(beta);
  a.rows = (uint32_t)rows; a.chunks = (uint32_t)chunks;
  a.flip = f.flip;
  a.L = (int32_t)length; a.zb = f.zb;
  a.k_term = k_term;
  a.o = o;
  const hipStream_t s = (hipStream_t)stream;
  if (block) layernorm_launch<true>(ch, blocks, s, a); else layernorm_launch<false>(ch, blocks, s, a);
  static thread_local char op_text[48];
  snprintf(op_text, sizeof(op_text), "%s -> %s %s", f.is_signed ? "i8" : "u8", out_code_dtype == MCTQ_CODE_I8 ? "i8" : "u8",
           block ? "block" : "wave");
  note_launch("codes_layernorm", op_text, ch, 0, 1, 1);
  return check_launch("mctq_codes_layernorm");
}

}  // extern "C"
