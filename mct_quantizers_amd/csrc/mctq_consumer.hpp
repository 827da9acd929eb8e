// mctq_consumer.hpp -- what the integer consumer's translation units share (mctq_qlinear.hip, mctq_qconv_dw.hip, mctq_fq_join.hip
// and the mctq_codes_*.hip operations on codes): the output form of a consumer launch, the per-chunk index division, and on
// the host side the checks of an operand's form, of a window's geometry and of overlapping byte ranges.
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

// One 16-byte chunk of codes of the form (flip, zb, scale) -- CodeForm's, below -- into the output form o, code by code:
// ql_code(join_residual(float(code - zero_point), scale)), the code the holder behind gives the holder's float32 output.
// Shared by the concatenation (mctq_codes_concat.hip) and the nearest upsampling (mctq_codes_upsample.hip).
__device__ __forceinline__ u32x4 requant_chunk(u32x4 v, uint32_t flip, float zb, float scale, const QlOut& o) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t u = v[q] ^ flip;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (float)((u >> (8 * j)) & 0xffu) - zb;                  // float(code - zero_point), exact
      w |= ((uint32_t)ql_code(join_residual(d, scale), o) & 0xffu) << (8 * j);
    }
    v[q] = w;
  }
  return v;
}

// ------------------------------------------------------------------------------------------
// Host side: the argument checks the code-tensor launchers share.  Every step is its own function, so that an entry point
// runs them in its own order between its other checks; none formats or allocates unless it refuses.
// ------------------------------------------------------------------------------------------
static int fail_words(const char* a, const char* b, const char* c = "") {
  char text[160];
  snprintf(text, sizeof(text), "%s%s%s", a, b, c);
  return fail_arg(text);
}

// The form of an int8 / uint8 code operand as the kernels take it: a code c is the byte (c ^ flip) = c + bias, bias = 128 for
// int8 and 0 for uint8, and zb = zero_point + bias, so that byte - zb == code - zero_point.
struct CodeForm { uint32_t flip; int32_t zb; float scale; bool is_signed; };
static CodeForm code_form(int32_t code_dtype, int32_t zero_point = 0, float scale = 1.0f) {
  const bool is_signed = code_dtype == MCTQ_CODE_I8;
  return {is_signed ? 0x80808080u : 0u, zero_point + (is_signed ? 128 : 0), scale, is_signed};
}
// The three checks of a form, each with the caller's words for its operand: "bad <dtype>", "<zero_point> is no code of <type>"
// (behind the first), "<scale> must be finite and positive"
struct FormWords { const char* dtype; const char* zero_point; const char* type; const char* scale; };
static int form_check_dtype(int32_t code_dtype, const char* dtype) {
  return code_dtype == MCTQ_CODE_I8 || code_dtype == MCTQ_CODE_U8 ? 0 : fail_words("bad ", dtype);
}
static int form_check_zero_point(int32_t code_dtype, int32_t zp, const char* zero_point, const char* type) {
  const bool is_code = code_dtype == MCTQ_CODE_I8 ? (zp >= -128 && zp <= 127) : (zp >= 0 && zp <= 255);
  return is_code ? 0 : fail_words(zero_point, " is no code of ", type);
}
static int form_check_scale(float scale, const char* name) {
  return scale > 0.0f && __builtin_isfinite(scale) ? 0 : fail_words(name, " must be finite and positive");
}
static int form_check(int32_t code_dtype, int32_t zp, float scale, const FormWords& w) {
  if (int rc = form_check_dtype(code_dtype, w.dtype)) return rc;
  if (int rc = form_check_zero_point(code_dtype, zp, w.zero_point, w.type)) return rc;
  return form_check_scale(scale, w.scale);
}
// a residual operand on codes (mctq_fq_join_rc_f32, mctq_qlinear_i8_res)
static int residual_form_check(int32_t r_code_dtype, int32_t r_zero_point, float r_scale) {
  return form_check(r_code_dtype, r_zero_point, r_scale, {"r_code_dtype", "r_zero_point", "the residual's type", "r_scale"});
}

// two byte ranges share a byte: a lane would read what another lane has overwritten
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t ab = (uintptr_t)a, bb = (uintptr_t)b;
  return ab < bb + b_bytes && bb < ab + a_bytes;
}

// The copy rule of the requantizing launchers (requant_chunk's callers): an operand whose form is the output's -- the same code
// type, zero point and float32 scale bits, a clamp domain that holds every code of the type -- comes out as it went in, for
// every code: (code - zp) * s * (1 / s) lies within 255 * 3 * 2^-24 of the integer code - zp.  Only scales in
// [2^-100, 2^100], where neither the product nor the reciprocal can overflow or underflow.
static bool form_is_copied(int32_t code_dtype, int32_t zero_point, float scale, int32_t out_code_dtype, int32_t out_zero_point,
                           float out_scale, int32_t quant_min, int32_t quant_max) {
  const bool whole = out_code_dtype == MCTQ_CODE_I8 ? (quant_min == -128 && quant_max == 127) : (quant_min == 0 && quant_max == 255);
  return whole && code_dtype == out_code_dtype && zero_point == out_zero_point
      && __builtin_bit_cast(uint32_t, scale) == __builtin_bit_cast(uint32_t, out_scale)
      && scale >= 0x1p-100f && scale <= 0x1p100f;
}

// A kernel, stride, dilation and padding window over a [B, H, W, C] image, one 16-byte chunk (16 channels) of one output
// pixel per lane.  The caller fills the arguments (dilation 1 where it has none) and leaves the rest 0; the steps below check
// them and fill the rest.
struct WindowGeom {
  int64_t batch, height, width, channels;
  int32_t kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int64_t hp, wp, span_h, span_w;                  // padded extents; dilation * (kernel - 1) + 1                    (geom_check_fit)
  int64_t ho, wo;                                  // output extent: a convolution's (geom_check_fit), a pool's (geom_check_pooled)
  int64_t pixels, c16, chunks;                     // B * Ho * Wo, C / 16, their product; 0: nothing to do           (geom_count)
};
static int geom_check_sizes(const WindowGeom& g, bool half_padding) {      // half_padding: the pools' rule (PyTorch's)
  if (g.batch < 0 || g.height < 0 || g.width < 0 || g.channels < 0) return fail_arg("negative extent");
  if (g.kh < 1 || g.kw < 1) return fail_arg("kernel size below 1");
  if (g.stride_h < 1 || g.stride_w < 1) return fail_arg("stride below 1");
  if (g.dil_h < 1 || g.dil_w < 1) return fail_arg("dilation below 1");
  if (g.pad_h < 0 || g.pad_w < 0) return fail_arg("negative padding");
  if (half_padding && (g.pad_h > g.kh / 2 || g.pad_w > g.kw / 2)) return fail_arg("padding larger than half the kernel size");
  return 0;
}
static int geom_check_channels(const WindowGeom& g) { return g.channels % 16 != 0 ? fail_arg("channels must be a multiple of 16") : 0; }
// The kernels' input coordinates stay within int32: o * stride + k * dilation never exceeds the padded extent, and where the
// kernel subtracts the padding only afterwards (with_span) o * stride - pad + k * dilation stays below padded extent + span.
static int geom_check_fit(WindowGeom& g, bool with_span) {
  g.hp = g.height + 2 * (int64_t)g.pad_h; g.wp = g.width + 2 * (int64_t)g.pad_w;
  g.span_h = (int64_t)g.dil_h * (g.kh - 1) + 1; g.span_w = (int64_t)g.dil_w * (g.kw - 1) + 1;
  if (g.hp + (with_span ? g.span_h : 0) > INT32_MAX || g.wp + (with_span ? g.span_w : 0) > INT32_MAX)
    return fail_arg("padded image extent exceeds 2^31 - 1");
  if (g.hp < g.span_h || g.wp < g.span_w) return fail_arg("the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)");
  g.ho = (g.hp - g.span_h) / g.stride_h + 1; g.wo = (g.wp - g.span_w) / g.stride_w + 1;
  return 0;
}
// PyTorch's pooling_output_shape along one axis (padded extent np = n + 2 * pad, span = dil * (k - 1) + 1 <= np): with
// ceil_mode the division rounds up, and a last window that would start beyond the image plus its left padding is dropped.
static int64_t pooled_extent(int64_t n, int64_t pad, int64_t span, int64_t stride, bool ceil_mode) {
  const int64_t np = n + 2 * pad;
  int64_t out = (np - span + (ceil_mode ? stride - 1 : 0)) / stride + 1;
  if (ceil_mode && (out - 1) * stride >= n + pad) --out;
  return out;
}
// the caller allocated out_height x out_width pixels per image: a disagreement would be an out-of-bounds write
static int geom_check_pooled(WindowGeom& g, bool ceil_mode, int64_t out_height, int64_t out_width) {
  g.ho = pooled_extent(g.height, g.pad_h, g.span_h, g.stride_h, ceil_mode);
  g.wo = pooled_extent(g.width, g.pad_w, g.span_w, g.stride_w, ceil_mode);
  return out_height != g.ho || out_width != g.wo ? fail_arg("out_height / out_width are not the pooled extent") : 0;
}
static int geom_count(WindowGeom& g) {
  if (g.batch == 0 || g.channels == 0) return 0;
  // (padding alone could make room for a kernel on an image without pixels; the clamped loads need one)
  if (g.height == 0 || g.width == 0) return fail_arg("an image of a non-empty batch needs at least one pixel");
  if (g.batch > INT32_MAX / (g.ho * g.wo)) return fail_arg("too many output pixels for one launch");   // ho * wo < 2^62
  g.pixels = g.batch * g.ho * g.wo; g.c16 = g.channels / 16;
  // a lane's index, pixel * (channels / 16) + chunk, is a 32-bit number (beyond it: split the batch)
  if (g.c16 > UINT32_MAX / g.pixels) return fail_arg("more than 2^32 - 1 16-channel chunks of output in one launch");
  g.chunks = g.pixels * g.c16;
  return 0;
}

}  // namespace mctq
