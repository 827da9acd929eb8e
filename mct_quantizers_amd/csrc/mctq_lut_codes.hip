// mctq_lut_codes.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h); ops: mctq_lut_index.hpp
//
// Entry points of the LUT quantizers' codebook-index codes.  uint8 codes go through the shared launchers with a 1-byte output
// type, as AffineCodesOp does (here: the decision-table op; the literal scan's instances are in mctq_lut_codes_scan.hip);
// packed 4-bit codes have launch shapes of their own (mctq_lut_codes4.hip).
#include "mctq_lut_index.hpp"

namespace mctq {

static int check_codes_args(int32_t code_dtype, const float* lut, int32_t n_lut, float mult) {
  if (code_dtype != MCTQ_CODE_U8 && code_dtype != MCTQ_CODE_U4) return fail_arg("LUT codes are MCTQ_CODE_U8 or MCTQ_CODE_U4");
  if (!lut) return fail_arg("lut is NULL");
  if (n_lut < 1) return fail_arg("n_lut must be at least 1");
  if (code_dtype == MCTQ_CODE_U8 && n_lut > 256) return fail_arg("uint8 LUT codes take codebooks of at most 256 entries");
  if (code_dtype == MCTQ_CODE_U4 && n_lut > 16) return fail_arg("4-bit LUT codes take codebooks of at most 16 entries");
  return check_pow2(mult);
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_lut_codes_per_tensor(const void* x, void* codes, int64_t n, int32_t dtype, int32_t code_dtype, int32_t step_round,
                              float thr_div, const float* lut, int32_t n_lut, const float* index_table, int32_t entries,
                              float mult, float clip_min, float clip_max, void* stream) {
  if (n < 0) return fail_arg("n < 0");
  if (n > 0 && (!x || !codes)) return fail_arg("x or codes is NULL");
  if (int rc = check_codes_args(code_dtype, lut, n_lut, mult)) return rc;
  if (step_round != 0 && step_round != MCTQ_DT_F16 && step_round != MCTQ_DT_BF16) return fail_arg("bad step_round");
  const hipStream_t st = (hipStream_t)stream;
  const LutCommon::Param p = LutCommon::make(thr_div, 0.0f, mult);
  const bool u4 = code_dtype == MCTQ_CODE_U4;
  if (index_table) {
    LutIndexTableOp op;
    if (int rc = make_table_op(op, nullptr, 0.f, index_table, entries, mult, clip_min, clip_max, step_round)) return rc;
    if (u4) return lut_codes4_per_tensor(op, p, x, codes, n, dtype, table_bytes(entries), st);
    return with_codes_types(dtype, code_dtype, [&](auto ti, auto to) {
      return launch_flat<decltype(ti), decltype(to)>(op, p, x, codes, n, table_bytes(entries), st);
    });
  }
  const LutIndexOp op = make_index_op(nullptr, 0.f, lut, n_lut, mult, clip_min, clip_max, step_round);
  const size_t book = (size_t)((n_lut + 3) & ~3) * sizeof(float);
  if (u4) return lut_codes4_per_tensor(op, p, x, codes, n, dtype, book, st);
  return lut_codes_scan_per_tensor(op, p, x, codes, n, dtype, book, st);
}

int mctq_lut_codes_per_channel(const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner, int32_t dtype,
                               int32_t code_dtype, const float* thresholds, float eps, const float* lut, int32_t n_lut,
                               const float* index_table, int32_t entries, float mult, float clip_min, float clip_max,
                               void* stream) {
  if (outer < 0 || channels < 0 || inner < 0) return fail_arg("negative extent");
  const int64_t n = outer * channels * inner;
  if (n > 0 && (!x || !codes || !thresholds)) return fail_arg("NULL pointer");
  if (int rc = check_codes_args(code_dtype, lut, n_lut, mult)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const bool u4 = code_dtype == MCTQ_CODE_U4;
  if (index_table) {
    LutIndexTableOp op;
    if (int rc = make_table_op(op, thresholds, eps, index_table, entries, mult, clip_min, clip_max, 0)) return rc;
    if (u4) return lut_codes4_per_channel(op, x, codes, outer, channels, inner, dtype, table_bytes(entries), st);
    return with_codes_types(dtype, code_dtype, [&](auto ti, auto to) {
      return launch_channels<decltype(ti), decltype(to)>(op, x, codes, outer, channels, inner, table_bytes(entries), st);
    });
  }
  const LutIndexOp op = make_index_op(thresholds, eps, lut, n_lut, mult, clip_min, clip_max, 0);
  const size_t book = (size_t)((n_lut + 3) & ~3) * sizeof(float);
  if (u4) return lut_codes4_per_channel(op, x, codes, outer, channels, inner, dtype, book, st);
  return lut_codes_scan_per_channel(op, x, codes, outer, channels, inner, dtype, book, st);
}

}  // extern "C"
