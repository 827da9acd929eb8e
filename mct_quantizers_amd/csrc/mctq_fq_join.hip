// mctq_fq_join.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// The join in front of an activation holder that several layers share (the end of a residual block): the elementwise
// prologue of the holder -- the residual add, the ReLU -- and the holder's two outputs in ONE pass over the tensor:
//     v        = x[i] (+ residual[i])            one float32 rounding, as ATen's add
//     v        = v < 0 ? 0 : v                   with relu; a NaN stays a NaN, as torch.relu
//     y[i]     = AffineOp::apply(v)              the fake-quantized float32 value, for the users that stay in float32
//     codes[i] = ql_code(v)                      the int8 / uint8 code of the same value, for the integer consumers
// Both outputs are the arithmetic of the launches they replace (mctq_fq_per_tensor_f32 and mctq_fq_codes_per_tensor on the
// same float32 v, the same host-computed 1.0f / scale): (codes - zero_point) * scale == y bit for bit.  13 bytes per element
// with both inputs and both outputs, against 28 for add, ReLU, holder and codes as four passes.
//
// A lane owns 16 consecutive elements: four 16-byte loads per input, all issued before the arithmetic, four 16-byte stores
// of float32 and one 16-byte store of codes.  The last n % 16 elements are one more lane's scalar loop.  Plain (cached)
// loads and stores: a product reads the outputs next.
//
// The residual may also arrive as the int8 / uint8 codes of another join (mctq_fq_join_rc_f32: an identity branch that stays on
// codes), with that join's scale and zero point: r = fma(float(code - r_zero_point), r_scale, +0) is the float32 value that
// join would have written (AffineOp::apply's last step), then v = x + r as above.  One 16-byte load of codes per lane stands for
// the four of float32: 6 bytes per element with codes out alone, against 13.
#include "mctq_consumer.hpp"

namespace mctq {

struct JoinArgs {
  const float* x;
  const float* residual;
  float* y;
  uint8_t* codes;
  int64_t n, chunks;                               // elements; whole 16-element chunks (n / 16)
  AffineOp op;                                     // the float32 output's clamp domain (scales / zps unused: per tensor)
  AffineOp::Param p;
  int32_t relu;
  // the residual as codes (RES == 2): the bytes are read as unsigned after ``^ rc_flip`` (0x80 per byte for int8 codes, which
  // maps code c to c + 128), and rc_zb is the zero point with the same bias -- float(byte) - rc_zb == float(code - r_zero_point)
  const uint8_t* rcodes;
  uint32_t rc_flip;
  float rc_zb, rc_scale;
};

// the float32 value of one residual code (b: the flipped byte as a float, exact; b - rc_zb == float(code - r_zero_point), exact
// too): mctq_consumer.hpp's join_residual, which the residual form of the integer product shares
__device__ __forceinline__ float join_residual(float b, const JoinArgs& a) { return join_residual(b - a.rc_zb, a.rc_scale); }

// the code of v in the form of the float32 output's own parameters (one reciprocal, one set of bounds for both outputs)
__device__ __forceinline__ int join_code(float v, const JoinArgs& a) {
  QlOut o;
  o.mode = 1; o.inv = a.p.inv; o.zf = a.p.zf; o.lo = a.op.lo; o.hi = a.op.hi;
  return ql_code(v, o);
}

// RES: 0 no residual, 1 a float32 residual, 2 a residual as codes
template <int RES, bool WY, bool WC>
__global__ __launch_bounds__(kThreads) void fq_join_kernel(JoinArgs a) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const NoBook book;
  if (g < a.chunks) {
    const f32x4* __restrict__ xs = reinterpret_cast<const f32x4*>(a.x) + g * 4;
    const f32x4* __restrict__ rs = reinterpret_cast<const f32x4*>(a.residual) + g * 4;
    f32x4 xv[4], rv[4];
    u32x4 rc;
#pragma unroll
    for (int q = 0; q < 4; ++q) xv[q] = xs[q];
    if constexpr (RES == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) rv[q] = rs[q];
    }
    if constexpr (RES == 2) rc = reinterpret_cast<const u32x4*>(a.rcodes)[g];
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float e = xv[q][j];
        if constexpr (RES == 1) e = e + rv[q][j];
        if constexpr (RES == 2) e = e + join_residual((float)(((rc[q] ^ a.rc_flip) >> (8 * j)) & 0xffu), a);
        if (a.relu) e = e < 0.0f ? 0.0f : e;
        v[4 * q + j] = e;
      }
    }
    if constexpr (WY) {
      f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(a.y) + g * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = a.op.apply(v[4 * q + j], a.p, book);
        dst[q] = o;
      }
    }
    if constexpr (WC) {
      u32x4 c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= ((uint32_t)join_code(v[4 * q + j], a) & 0xffu) << (8 * j);
        c[q] = w;
      }
      reinterpret_cast<u32x4*>(a.codes)[g] = c;
    }
  } else if (g == a.chunks) {                      // the tail, n % 16 elements (the launcher adds this lane only when there is one)
    for (int64_t i = a.chunks * 16; i < a.n; ++i) {
      float e = a.x[i];
      if constexpr (RES == 1) e = e + a.residual[i];
      if constexpr (RES == 2) e = e + join_residual((float)((a.rcodes[i] ^ a.rc_flip) & 0xffu), a);
      if (a.relu) e = e < 0.0f ? 0.0f : e;
      if constexpr (WY) a.y[i] = a.op.apply(e, a.p, book);
      if constexpr (WC) a.codes[i] = (uint8_t)join_code(e, a);
    }
  }
}

template <int RES>
static void launch_fq_join(const JoinArgs& a, unsigned blocks, hipStream_t stream) {
  if (a.y && a.codes) hipLaunchKernelGGL((fq_join_kernel<RES, true, true>), dim3(blocks), dim3(kThreads), 0, stream, a);
  else if (a.y) hipLaunchKernelGGL((fq_join_kernel<RES, true, false>), dim3(blocks), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL((fq_join_kernel<RES, false, true>), dim3(blocks), dim3(kThreads), 0, stream, a);
}

}  // namespace mctq

using namespace mctq;

// Both entry points: ``residual`` (float32) or ``r_codes`` (with its type, scale and zero point, checked by the caller), or neither.
static int fq_join_entry(const char* entry, const float* x, const float* residual, const void* r_codes, int32_t r_code_dtype,
                         float r_scale, int32_t r_zero_point, int32_t relu, float* y, void* codes, int32_t code_dtype, int64_t n,
                         float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream) {
  if (n < 0) return fail_arg("n < 0");
  if (n == 0) return 0;
  if (!x) return fail_arg("x is NULL");
  if (!y && !codes) return fail_arg("neither y nor codes is given");
  if (codes && code_dtype != MCTQ_CODE_I8 && code_dtype != MCTQ_CODE_U8) return fail_arg("bad code_dtype");
  if (codes && (code_dtype == MCTQ_CODE_I8 ? (quant_min < -128 || quant_max > 127) : (quant_min < 0 || quant_max > 255)))
    return fail_arg("clamp domain does not fit the code type");
  if (quant_min > quant_max) return fail_arg("quant_min > quant_max");
  // the float32 output clamps between float bounds: exact up to 2^24 (beyond it ATen's operator is the reference's own call)
  if (y && (quant_min < -(1 << 24) || quant_max > (1 << 24))) return fail_arg("clamp domain beyond 2^24 with a float32 output");
  if ((((uintptr_t)x | (uintptr_t)residual | (uintptr_t)y | (uintptr_t)codes) & 15u) != 0)
    return fail_arg("x, residual, y and codes must be 16-byte aligned");
  if (((uintptr_t)r_codes & 15u) != 0) return fail_arg("r_codes must be 16-byte aligned");
  JoinArgs a;
  a.chunks = n / 16;
  const int64_t lanes = a.chunks + (n % 16 != 0 ? 1 : 0);
  const int64_t blocks = (lanes + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL) return fail_arg("tensor too large for one launch");
  a.x = x; a.residual = residual; a.y = y; a.codes = static_cast<uint8_t*>(codes); a.n = n;
  a.op.scales = nullptr; a.op.zps = nullptr;
  a.op.lo = (float)quant_min; a.op.hi = (float)quant_max;
  a.p = AffineOp::make(scale, zero_point);          // inv = 1.0f / scale on the host, as both launches this one stands for
  a.relu = relu != 0;
  const CodeForm rf = code_form(r_code_dtype, r_zero_point, r_scale);
  a.rcodes = static_cast<const uint8_t*>(r_codes);
  a.rc_flip = rf.flip; a.rc_zb = (float)rf.zb; a.rc_scale = rf.scale;
  const hipStream_t s = (hipStream_t)stream;
  if (r_codes) launch_fq_join<2>(a, (unsigned)blocks, s);
  else if (residual) launch_fq_join<1>(a, (unsigned)blocks, s);
  else launch_fq_join<0>(a, (unsigned)blocks, s);
  static thread_local char op_text[48];
  snprintf(op_text, sizeof(op_text), "%s%s-> %s%s%s", r_codes ? (rf.is_signed ? "addc(i8) " : "addc(u8) ") : residual ? "add " : "",
           a.relu ? "relu " : "", y ? "f32" : "", y && codes ? " + " : "", !codes ? "" : (code_dtype == MCTQ_CODE_I8 ? "i8" : "u8"));
  note_launch("fq_join", op_text, 4, 0, r_codes ? 5 : 4, (y ? 4 : 0) + (codes ? 1 : 0));
  return check_launch(entry);
}

extern "C" {

int mctq_fq_join_f32(const float* x, const float* residual, int32_t relu, float* y, void* codes, int32_t code_dtype,
                     int64_t n, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream) {
  return fq_join_entry("mctq_fq_join_f32", x, residual, nullptr, 0, 0.0f, 0, relu, y, codes, code_dtype, n, scale, zero_point,
                       quant_min, quant_max, stream);
}

int mctq_fq_join_rc_f32(const float* x, const void* r_codes, int32_t r_code_dtype, float r_scale, int32_t r_zero_point,
                        int32_t relu, float* y, void* codes, int32_t code_dtype, int64_t n, float scale, int32_t zero_point,
                        int32_t quant_min, int32_t quant_max, void* stream) {
  if (n < 0) return fail_arg("n < 0");
  if (n == 0) return 0;
  if (!r_codes) return fail_arg("r_codes is NULL");
  if (int rc = residual_form_check(r_code_dtype, r_zero_point, r_scale)) return rc;
  return fq_join_entry("mctq_fq_join_rc_f32", x, nullptr, r_codes, r_code_dtype, r_scale, r_zero_point, relu, y, codes,
                       code_dtype, n, scale, zero_point, quant_min, quant_max, stream);
}

}  // extern "C"
