// mctq_lut_codes_scan.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h); ops: mctq_lut_index.hpp
// uint8 codebook-index codes through the literal scan (no index table: non-integer codebooks, lut_values_bitwidth > 10).
#include "mctq_lut_index.hpp"

namespace mctq {

int lut_codes_scan_per_tensor(const LutIndexOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                              size_t book_bytes, hipStream_t st) {
  return with_codes_types(dtype, MCTQ_CODE_U8, [&](auto ti, auto to) {
    return launch_flat<decltype(ti), decltype(to)>(op, p, x, codes, n, book_bytes, st);
  });
}

int lut_codes_scan_per_channel(const LutIndexOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                               int dtype, size_t book_bytes, hipStream_t st) {
  return with_codes_types(dtype, MCTQ_CODE_U8, [&](auto ti, auto to) {
    return launch_channels<decltype(ti), decltype(to)>(op, x, codes, outer, channels, inner, book_bytes, st);
  });
}

}  // namespace mctq
