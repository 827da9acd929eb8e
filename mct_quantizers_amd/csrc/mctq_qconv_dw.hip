// mctq_qconv_dw.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Depthwise convolution on the quantizers' codes (groups == channels, channel multiplier 1): the layer between the two
// pointwise convolutions of a MobileNet-style block.  There is no reduction over channels, so nothing for the matrix
// cores; per output element it is kh * kw multiply-accumulates on bytes:
//     acc[b][oy][ox][c] = sum over taps inside the image of (a[b][iy][ix][c] - za) * (w[ky][kx][c] - zw[c])
//     y = float(acc) * (sa * sw[c]) + bias[c]
// with the epilogue of mctq_qlinear_i8 (one rounding per float32 operation; -ffp-contract=off) and its output forms
// (QlOut: float32, or the next layer's codes); mctq_qconv_dw_i8_act puts a Hardswish / Hardsigmoid (ql_act) in front of the
// codes.
//
// Layout: activations NHWC, weights [kh][kw][C], so that 16 consecutive channels are one aligned 16-byte chunk of either.
// A lane owns one chunk of one output pixel: consecutive lanes take consecutive chunks of a pixel, then consecutive
// pixels (a pixel may straddle two blocks) -- the loads of a tap and the stores are coalesced over the wave.  Per tap one
// 16-byte activation load and one 16-byte weight load (the weights are kh * kw * C bytes in all and stay in cache; the
// input is re-read up to kh * kw times out of cache), 16 int32 accumulators, and at the end four 16-byte stores of
// float32 or one of codes.  Index arithmetic per chunk: three divisions by launch constants (FastDiv).
//
// Padding: a tap outside the image is loaded from a clamped (valid) address and then replaced by 16 zero-point bytes, so
// that it adds (za - za) * (w - zw) = 0: the loads do not depend on a branch and the compiler can issue all of a 3 x 3
// kernel's loads before the first multiply.  This is why a_zero_point must be a code of the activations' type.
//
// The sum is exact: |a - za| <= 255, |w - zw| <= 255, at most 256 taps: 256 * 255 * 255 < 2^24 * 2^8 < 2^31; each product
// fits the 24-bit multiplier (v_mad_i32_i24).
#include "mctq_consumer.hpp"

// 1 (shipped): 3 x 3 kernels run an instance whose tap loops are unrolled at compile time (all 18 loads of a lane in flight
// at once); 0: every kernel size runs the run-time loops (tools/dw_consumer_probe.py times the two builds against each other)
#ifndef MCTQ_DW_UNROLL3
#define MCTQ_DW_UNROLL3 1
#endif

namespace mctq {

struct DwArgs {
  const uint8_t* x;
  const int8_t* w;
  const float* w_scales;
  const int32_t* w_zero_points;
  const float* bias;
  void* y;
  FastDiv c16, wo, ho;                             // chunks per pixel (C / 16), Wo, Ho
  uint32_t chunks;                                 // B * Ho * Wo * C / 16
  int32_t H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t za;
  float sa;
  QlOut oq;
  int act;                                         // ql_act's, in front of the codes (mctq_qconv_dw_i8_act); 0 otherwise
};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// byte j of a dword as an integer: zero-extended (uint8 codes) or sign-extended (int8 codes, weights)
template <bool U8>
__device__ __forceinline__ int dw_byte(uint32_t v, int j) {
  if constexpr (U8) return (int)((v >> (8 * j)) & 0xffu);
  else return (int)(v << (24 - 8 * j)) >> 24;
}

// KK > 0: a KK x KK kernel known at compile time (a.kh == a.kw == KK); KK == 0: a.kh x a.kw
template <bool A_U8, bool ZP, int KK>
__global__ __launch_bounds__(kThreads) void qconv_dw_kernel(DwArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^32: the launcher checks the chunk count
  if (g >= a.chunks) return;
  uint32_t cc, ox, oy;
  const uint32_t m = a.c16.divmod(g, cc);
  const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);
  const int64_t c16 = a.c16.d;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.x) + (int64_t)b * a.H * a.W * c16 + cc;
  const u32x4* __restrict__ wsrc = reinterpret_cast<const u32x4*>(a.w) + cc;
  const int iy0 = (int)oy * a.stride_h - a.pad_h, ix0 = (int)ox * a.stride_w - a.pad_w;
  const uint32_t pad = (uint32_t)(a.za & 0xff) * 0x01010101u;
  const int za = a.za;

  int zw[16];
  if constexpr (ZP) {
    const i32x4* __restrict__ zsrc = reinterpret_cast<const i32x4*>(a.w_zero_points) + (int64_t)cc * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const i32x4 z = zsrc[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) zw[4 * q + j] = z[j];
    }
  }
  int acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0;

  auto tap = [&](int ky, int kx, int kw) {
    const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
    const bool inside = (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
    const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);         // a valid address whatever the tap
    u32x4 av = src[((int64_t)cy * a.W + cx) * c16];
    const u32x4 wv = wsrc[(int64_t)(ky * kw + kx) * c16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t aq = inside ? av[q] : pad;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ae = dw_byte<A_U8>(aq, j) - za;
        int we = dw_byte<false>(wv[q], j);
        if constexpr (ZP) we -= zw[4 * q + j];
        acc[4 * q + j] += __mul24(ae, we);
      }
    }
  };
  if constexpr (KK > 0) {
#pragma unroll
    for (int ky = 0; ky < KK; ++ky) {
#pragma unroll
      for (int kx = 0; kx < KK; ++kx) tap(ky, kx, KK);
    }
  } else {
    for (int ky = 0; ky < a.kh; ++ky)
      for (int kx = 0; kx < a.kw; ++kx) tap(ky, kx, a.kw);
  }

  // epilogue: float(acc) * (sa * sw[c]) (+ bias[c]), one rounding each, as mctq_qlinear_i8
  const f32x4* __restrict__ ssrc = reinterpret_cast<const f32x4*>(a.w_scales) + (int64_t)cc * 4;
  const f32x4* __restrict__ bsrc = reinterpret_cast<const f32x4*>(a.bias) + (int64_t)cc * 4;
  float out[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 s = ssrc[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * q + j] = (float)acc[4 * q + j] * (a.sa * s[j]);
    if (a.bias) {
      const f32x4 bv = bsrc[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) out[4 * q + j] = out[4 * q + j] + bv[j];
    }
  }
  if (a.oq.mode == 0) {
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(a.y) + (int64_t)g * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = f32x4{out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
  } else {
    u32x4 codes;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) v |= ((uint32_t)ql_code(ql_act(out[4 * q + j], a.act), a.oq) & 0xffu) << (8 * j);
      codes[q] = v;
    }
    reinterpret_cast<u32x4*>(a.y)[g] = codes;
  }
}

template <bool A_U8, bool ZP>
static void launch_qconv_dw(const DwArgs& a, unsigned blocks, hipStream_t stream) {
  if (MCTQ_DW_UNROLL3 && a.kh == 3 && a.kw == 3)
    hipLaunchKernelGGL((qconv_dw_kernel<A_U8, ZP, 3>), dim3(blocks), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((qconv_dw_kernel<A_U8, ZP, 0>), dim3(blocks), dim3(kThreads), 0, stream, a);
}

}  // namespace mctq

using namespace mctq;

// The two entry points' checks and launch.  act: 0 (mctq_qconv_dw_i8) or ql_act's 1 / 2, checked by mctq_qconv_dw_i8_act.
static int qconv_dw_call(const char* entry, const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                         const int8_t* w_codes, const float* w_scales, const int32_t* w_zero_points, const float* bias,
                         void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                         int32_t act, int64_t batch, int64_t height, int64_t width, int64_t channels,
                         int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                         int32_t dil_h, int32_t dil_w, void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
  if (int rc = geom_check_sizes(g, false)) return rc;
  if (int rc = geom_check_channels(g)) return rc;
  if (kh > 256 || kw > 256 || kh * kw > 256) return fail_arg("kh * kw > 256: outside the depthwise consumer's limit");
  if (int rc = form_check_dtype(a_code_dtype, "a_code_dtype")) return rc;
  const bool u8 = a_code_dtype == MCTQ_CODE_U8;
  // the zero point is the byte a padded tap is given (it then adds (za - za) * w = 0): it has to be a code
  if (int rc = form_check_zero_point(a_code_dtype, a_zero_point, "a_zero_point", "a_code_dtype")) return rc;
  DwArgs a;
  if (int rc = ql_output_form(a.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  if (int rc = geom_check_fit(g, false)) return rc;
  if (int rc = geom_count(g)) return rc;
  if (g.chunks == 0) return 0;
  if (!a_codes || !w_codes || !w_scales || !y) return fail_arg("NULL pointer");
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)w_scales | (uintptr_t)w_zero_points |
        (uintptr_t)bias) & 15u) != 0)
    return fail_arg("codes, weights, per-channel tables and output must be 16-byte aligned");
  a.x = static_cast<const uint8_t*>(a_codes);
  a.w = w_codes; a.w_scales = w_scales; a.w_zero_points = w_zero_points; a.bias = bias; a.y = y;
  a.c16 = FastDiv::make((uint32_t)g.c16);
  a.wo = FastDiv::make((uint32_t)g.wo);
  a.ho = FastDiv::make((uint32_t)g.ho);
  a.chunks = (uint32_t)g.chunks;
  a.H = (int32_t)height; a.W = (int32_t)width; a.kh = kh; a.kw = kw;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.za = a_zero_point; a.sa = a_scale; a.act = act;
  const unsigned blocks = (unsigned)(((int64_t)a.chunks + kThreads - 1) / kThreads);                  // <= 2^24
  const hipStream_t s = (hipStream_t)stream;
  const bool zp = w_zero_points != nullptr;
  if (u8) { if (zp) launch_qconv_dw<true, true>(a, blocks, s); else launch_qconv_dw<true, false>(a, blocks, s); }
  else { if (zp) launch_qconv_dw<false, true>(a, blocks, s); else launch_qconv_dw<false, false>(a, blocks, s); }
  const char* op = zp ? (u8 ? "u8 x i8 zp" : "i8 x i8 zp") : (u8 ? "u8 x i8" : "i8 x i8");
  if (act) {                                       // "u8 x i8 zp hardswish"
    static thread_local char op_text[40];
    snprintf(op_text, sizeof(op_text), "%s%s", op, act == 1 ? " hardswish" : " hardsigmoid");
    op = op_text;
  }
  note_launch("qconv_dw", op, MCTQ_DW_UNROLL3 && kh == 3 && kw == 3 ? 9 : 1, 0, 1, a.oq.mode == 0 ? 4 : 1);
  return check_launch(entry);
}

extern "C" {

int mctq_qconv_dw_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                     const int8_t* w_codes, const float* w_scales, const int32_t* w_zero_points, const float* bias,
                     void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                     int64_t batch, int64_t height, int64_t width, int64_t channels,
                     int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                     int32_t dil_h, int32_t dil_w, void* stream) {
  return qconv_dw_call("mctq_qconv_dw_i8", a_codes, a_code_dtype, a_zero_point, a_scale, w_codes, w_scales, w_zero_points, bias, y,
                       y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max, 0, batch, height, width, channels, kh, kw,
                       stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, stream);
}

int mctq_qconv_dw_i8_act(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                         const int8_t* w_codes, const float* w_scales, const int32_t* w_zero_points, const float* bias,
                         void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                         int32_t act, int64_t batch, int64_t height, int64_t width, int64_t channels,
                         int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                         int32_t dil_h, int32_t dil_w, void* stream) {
  if (act != 1 && act != 2) return fail_arg("act must be 1 (hardswish) or 2 (hardsigmoid)");
  if (y_code_dtype < 0) return fail_arg("bad y_code_dtype");      // an activation leaves as codes only
  return qconv_dw_call("mctq_qconv_dw_i8_act", a_codes, a_code_dtype, a_zero_point, a_scale, w_codes, w_scales, w_zero_points, bias,
                       y, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max, act, batch, height, width, channels, kh,
                       kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, stream);
}

}  // extern "C"
