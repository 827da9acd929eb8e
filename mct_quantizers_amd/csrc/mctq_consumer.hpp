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

// The float32 value of one residual code, d = float(code - zero_point) (exact): fma(d, scale, +0), the last step of
// AffineOp::apply and so the value the join that wrote the code would have written in float32.  The product is a float32
// VALUE before the add that follows: without the opaque asm the compiler contracts d * s + x into one v_fma_f32 with a single
// rounding, where the float32 tensor this stands for was rounded once as a product and the add rounds again.  Shared by the
// join (mctq_fq_join.hip) and the residual form of the integer product (mctq_qlinear.hip).
__device__ __forceinline__ float join_residual(float d, float scale) {
  float r = __builtin_fmaf(d, scale, 0.0f);
  asm("" : "+v"(r));
  return r;
}

// Hardswish / Hardsigmoid of the float32 epilogue value, in front of ql_code / ql_store (mctq_qlinear_i8_act,
// mctq_qconv_dw_i8_act).  act: 0 none, 1 hardswish, 2 hardsigmoid.  The expression is the one ATen's GPU kernels evaluate,
//     hardswish(x) = x * min(max(x + 3, 0), 6) * (1.0f / 6.0f)      hardsigmoid(x) = min(max(x + 3, 0), 6) * (1.0f / 6.0f)
// left to right, one rounding per operation, with std::max / std::min semantics (a < b ? b : a; a NaN stays a NaN, and
// hardswish(-inf) = -inf * 0 = NaN) -- equal to F.hardswish / F.hardsigmoid on the GPU for all 2^32 float32 bit patterns
// (docs/KERNEL_NOTES.md; ATen's CPU kernels divide by 6 instead and differ in a quarter / a thirtieth of the patterns).
// x * ramp is a float32 VALUE before the multiplication by 1/6: the opaque asm keeps the compiler from ever folding the
// two constants' side of the chain (x * (ramp * c)), which rounds differently.  The branch on act is uniform over a launch.
__device__ __forceinline__ float ql_act(float v, int act) {
  if (act == 0) return v;
  float t = v + 3.0f;
  t = t < 0.0f ? 0.0f : t;                            // std::max(t, 0.0f)
  t = 6.0f < t ? 6.0f : t;                            // std::min(t, 6.0f)
  if (act == 1) t = v * t;
  asm("" : "+v"(t));
  return t * (1.0f / 6.0f);
}

// The residual operand of a consumer launch (mctq_qlinear_i8_res): [M][N] row-major like y, float32 values or the int8 /
// uint8 codes of another quantizer with its scale and zero point; relu: v < 0 ? 0 : v behind the add (the join's expression).
// act: ql_act's, applied last (mctq_qlinear_i8_act: mode 0 -- the instantiations that take this record then skip the add).
struct QlRes {
  const void* r;
  int mode;                 // 0 none, 1 float32, 2 int8 codes, 3 uint8 codes
  int zp;
  float scale;
  int relu;
  int act;
};
// out (+ residual at idx) (then the ReLU): one float32 add, not contracted (-ffp-contract=off; the code's value is opaque).
// The branches are uniform over the launch.
__device__ __forceinline__ float ql_residual_at(const QlRes& rs, int64_t idx) {
  if (rs.mode == 1) return static_cast<const float*>(rs.r)[idx];
  const int c = rs.mode == 2 ? (int)static_cast<const int8_t*>(rs.r)[idx] : (int)static_cast<const uint8_t*>(rs.r)[idx];
  return join_residual((float)(c - rs.zp), rs.scale);
}
// CNT residuals at once, at idx[0 .. CNT) (valid indices all: the caller clamps rows it will not store): one straight line of
// loads of the residual's type, issued before any is used -- a branch on the type around every single load would make each
// wait for the one before it.
template <class T, int CNT>
__device__ __forceinline__ void ql_residuals_as(const QlRes& rs, const int64_t (&idx)[CNT], float (&out)[CNT]) {
  const T* __restrict__ rp = static_cast<const T*>(rs.r);
  T raw[CNT];
#pragma unroll
  for (int j = 0; j < CNT; ++j) raw[j] = rp[idx[j]];
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
    if constexpr (std::is_same<T, float>::value) out[j] = raw[j];
    else out[j] = join_residual((float)((int)raw[j] - rs.zp), rs.scale);
  }
}
template <int CNT>
__device__ __forceinline__ void ql_residuals(const QlRes& rs, const int64_t (&idx)[CNT], float (&out)[CNT]) {
  if (rs.mode == 1) ql_residuals_as<float, CNT>(rs, idx, out);
  else if (rs.mode == 2) ql_residuals_as<int8_t, CNT>(rs, idx, out);
  else ql_residuals_as<uint8_t, CNT>(rs, idx, out);
}
__device__ __forceinline__ float ql_join(float out, float r, const QlRes& rs) {
  out = out + r;
  if (rs.relu) out = out < 0.0f ? 0.0f : out;
  return out;
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
