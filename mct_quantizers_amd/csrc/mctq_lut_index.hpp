// mctq_lut_index.hpp -- ops of the LUT quantizers' codebook-index codes, shared by mctq_lut_codes.hip (entry points, uint8
// codes through the decision table), mctq_lut_codes_scan.hip (uint8 codes through the literal scan) and mctq_lut_codes4.hip
// (packed 4-bit codes).  Three translation units so that each compiles beside the library's slowest one.
//
// The code is the index torch.argmin returns in the reference's chain (quantizer_utils.py:134) -- first minimum of
// fl32(|t - lut[j]|) in the caller's list order, 0 for a NaN input.  An extension without a reference counterpart, as the
// integer codes of the affine quantizers.
//   * LutIndexTableOp: LutTableOp with the other payload (mctq_lut_build_index_table: same thresholds, word 1 of an entry
//     is index_below | index_above << 16).  locate() is LutTableOp's; decide() picks the 16-bit half.
//   * LutIndexOp: the literal scan carrying the index beside the best distance (any codebook; one more select per entry).
// apply() returns the index as a float; a 1-byte output type narrows it (IO::pack), as for AffineCodesOp.
#pragma once
#include "mctq_kernels.hpp"

namespace mctq {

struct LutIndexTableOp : LutTableOp {
  static constexpr const char* kName = "LutIndexTableOp";
  static constexpr int kFixedU = 4;            // an extension without a reference counterpart: one variant per launch shape

  template <bool FAST>
  __device__ __forceinline__ float decide(float x, float v, f32x2 e, const Param&, const Book&) const {
    const uint32_t pair = __float_as_uint(e.y);
    const uint32_t h = (v >= e.x) ? (pair >> 16) : (pair & 0xffffu);
    const bool nan = (FAST && step_round == 0) ? (x != x) : (v != v);      // as LutTableOp::decide
    return nan ? 0.0f : (float)h;                                          // all-NaN distances: argmin is index 0
  }
  template <bool FAST = false>
  __device__ __forceinline__ float apply(float x, const Param& p, const Book& b) const {
    float v; int k;
    locate<FAST>(x, p, v, k);
    return decide<FAST>(x, v, b.tab[k], p, b);
  }
  template <bool FAST, int NE>
  __device__ __forceinline__ void tile(const float* in, float* out, const Param& p, const Book& b) const {
    float v[NE];
    int k[NE];
    f32x2 e[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) locate<FAST>(in[i], p, v[i], k[i]);
#pragma unroll
    for (int i = 0; i < NE; ++i) e[i] = b.tab[k[i]];
#pragma unroll
    for (int i = 0; i < NE; ++i) out[i] = decide<FAST>(in[i], v[i], e[i], p, b);
  }
};

struct LutIndexOp : LutOp<0> {
  static constexpr const char* kName = "LutIndexOp";
  template <bool FAST = false>
  __device__ __forceinline__ float apply(float x, const Param& p, const Book& b) const {
    const float v = scaled<FAST>(x, p);
    float t = fminf(fmaxf(v, cmin), cmax);
    t = (x != x) ? x : t;                              // torch.clip keeps NaN (see LutOp::apply)
    t = (v != v) ? v : t;
    int best_j = 0;
    float best_d = fabsf(t - b.c[0]);
    for (int j = 1; j < b.n; ++j) {
      const float d = fabsf(t - b.c[j]);               // same address in every lane: LDS broadcast
      const bool lt = d < best_d;                      // strict: first minimum wins; NaN never wins
      best_d = lt ? d : best_d;
      best_j = lt ? j : best_j;
    }
    return (float)best_j;
  }
};

inline LutIndexOp make_index_op(const float* thr, float eps, const float* lut, int n_lut, float mult, float cmin, float cmax,
                                int step_round) {
  LutIndexOp op;
  fill_lut_common(op, thr, eps, mult, cmin, cmax, step_round);
  op.lut = lut; op.n_lut = n_lut;
  return op;
}

// mctq_lut_codes_scan.hip: uint8 codes, literal scan
int lut_codes_scan_per_tensor(const LutIndexOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                              size_t book_bytes, hipStream_t st);
int lut_codes_scan_per_channel(const LutIndexOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                               int dtype, size_t book_bytes, hipStream_t st);
// mctq_lut_codes4.hip: packed 4-bit codes, either op
int lut_codes4_per_tensor(const LutIndexTableOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                          size_t book_bytes, hipStream_t st);
int lut_codes4_per_tensor(const LutIndexOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                          size_t book_bytes, hipStream_t st);
int lut_codes4_per_channel(const LutIndexTableOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                           int dtype, size_t book_bytes, hipStream_t st);
int lut_codes4_per_channel(const LutIndexOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                           int dtype, size_t book_bytes, hipStream_t st);

}  // namespace mctq
