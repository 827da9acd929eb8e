// mctq_consumer.hpp -- what the integer consumer's translation units share (mctq_qlinear.hip, mctq_codes_im2col.hip,
// mctq_qconv_dw.hip): the output form of a consumer launch and the per-chunk index division.
#pragma once
#include "mctq_kernels.hpp"

namespace mctq {

// Output form: float32 values, or the next layer's activation codes (the fake-quant arithmetic of
// mctq_fq_codes_per_tensor applied to the float32 value in registers: clamp(rint(v * inv) + zp, lo, hi)).
struct QlOut {
  int mode;                 // 0 float32, 1 int8 codes, 2 uint8 codes
  float inv, zf, lo, hi;
};
__device__ __forceinline__ void ql_store(void* __restrict__ y, int64_t idx, float v, const QlOut& o) {
  if (o.mode == 0) {
    static_cast<float*>(y)[idx] = v;
  } else {
    float q = __builtin_rintf(v * o.inv) + o.zf;
    q = fminf(fmaxf(q, o.lo), o.hi);                  // NaN -> lo, as the codes kernel
    if (o.mode == 1) static_cast<int8_t*>(y)[idx] = (int8_t)(int)q;
    else static_cast<uint8_t*>(y)[idx] = (uint8_t)(int)q;
  }
}
// The code ql_store writes for v (o.mode != 0) as an integer, for kernels that pack several codes into one store: its low
// byte is the int8 and the uint8 code alike.
__device__ __forceinline__ int ql_code(float v, const QlOut& o) {
  float q = __builtin_rintf(v * o.inv) + o.zf;
  q = fminf(fmaxf(q, o.lo), o.hi);                    // NaN -> lo, as the codes kernel
  return (int)q;
}

// y_code_dtype < 0: float32 output; otherwise the next layer's codes (mctq_qlinear_i8_codes' checks and parameters).
static int ql_output_form(QlOut& oq, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                          int32_t y_quant_max) {
  oq.mode = 0; oq.inv = oq.zf = oq.lo = oq.hi = 0.0f;
  if (y_code_dtype < 0) return 0;
  if (y_code_dtype != MCTQ_CODE_I8 && y_code_dtype != MCTQ_CODE_U8) return fail_arg("bad y_code_dtype");
  if (y_quant_min > y_quant_max) return fail_arg("quant_min > quant_max");
  if (y_code_dtype == MCTQ_CODE_I8 ? (y_quant_min < -128 || y_quant_max > 127) : (y_quant_min < 0 || y_quant_max > 255))
    return fail_arg("clamp domain does not fit the code type");
  oq.mode = y_code_dtype == MCTQ_CODE_I8 ? 1 : 2;
  oq.inv = 1.0f / y_scale;                           // host IEEE division == the codes kernel's
  oq.zf = (float)y_zero_point; oq.lo = (float)y_quant_min; oq.hi = (float)y_quant_max;
  return 0;
}

// n / d for 32-bit n by magic = floor(2^32 / d) (d = 1: 2^32 - 1): umulhi gives the quotient or one less.
struct FastDiv {
  uint32_t d, magic;
  __host__ static FastDiv make(uint32_t d) { return {d, d == 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / d)}; }
  __device__ __forceinline__ uint32_t divmod(uint32_t n, uint32_t& rem) const {
    uint32_t q = __umulhi(n, magic);
    rem = n - q * d;
    if (rem >= d) { ++q; rem -= d; }
    return q;
  }
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

}  // namespace mctq
