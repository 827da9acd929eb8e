// mctq_codes_mul.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Elementwise multiply on NHWC activation codes: a [pixels][C] (1 byte per element, int8 or uint8, with its scale and zero
// point) times a second operand g -> out [pixels][C] in the form of the holder behind the multiply.  A holder's float32
// output is float(code - zp) * scale bit for bit (join_residual: the last step of AffineOp::apply), torch.mul is one IEEE
// float32 multiplication, and the holder behind it codes every element with ql_code's arithmetic, so
//     out[p][c] = ql_code(join_residual(float(ca - za), sa) * join_residual(float(cg - zg), sg))
// is the code that holder gives the float32 product of the two holder outputs, for every element -- nothing is approximated.
//
// g comes in three forms (the kernel's template parameter):
//   kSame   codes [pixels][C], the chunk of the same index;
//   kRow    codes [pixels / n][C], one row per n pixels (the SE gate [B, C, 1, 1] of an image of n = H * W pixels);
//   kRowF32 raw float32 values [pixels / n][C], coded first with ql_code in G's own form (NaN -> lo, as everywhere) and
//           then dequantized like codes: the quantize launch of a tiny tensor is saved.
//
// Form: that of mctq_codes_concat.hip.  A lane owns one 16-byte chunk of the output; consecutive lanes take consecutive
// chunks of a row and then consecutive rows: one 16-byte load of a, one 16-byte load of g (four for float32 gates), one
// 16-byte store, all plain (a product reads the output next; consecutive pixels re-read the same gate row from cache).  The
// gate chunk is (pixel / n) * C/16 + chunk: two FastDivs.  Nothing here is indexed by the lane, so every operand parameter
// is a kernel argument read by scalar loads and stays in scalar registers (what the concatenation kernel has to pin by hand).
// Both dequantized values are float32 VALUES before the multiply (join_residual's pinning), the product is one v_mul_f32
// and ql_code's v * inv another: no contraction is possible between them (-ffp-contract=off besides).  No LDS, no scratch.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, QlOut, ql_code, join_residual

namespace mctq {

enum MulGate { kSame = 0, kRow = 1, kRowF32 = 2 };

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MulArgs {
  const u32x4* a;
  const void* g;                           // u32x4 chunks of codes, or f32x4 quarters of a chunk (kRowF32)
  u32x4* out;
  uint32_t a_flip, g_flip;                 // 0x80808080 for int8 codes (code c -> byte c + 128), 0 for uint8
  float a_zb, g_zb;                        // the zero point with the same bias: float(byte) - zb == float(code - zero_point)
  float a_scale, g_scale;
  FastDiv row;                             // chunks per row (C / 16)
  FastDiv img;                             // pixels per gate row (n)
  uint32_t chunks;                         // pixels * row.d
  QlOut gq;                                // G's form, for float32 gates
  QlOut o;
};

template <int GATE>
__global__ __launch_bounds__(kThreads) void codes_mul_kernel(MulArgs a) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^31: the launcher checks the chunk count
  if (i >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t gi = i;
  if constexpr (GATE != kSame) {
    uint32_t cc, within;
    const uint32_t pixel = a.row.divmod(i, cc);
    gi = a.img.divmod(pixel, within) * a.row.d + cc;                         // <= i: pixel / n <= pixel
  }
  const u32x4 va = a.a[i];
  float dg[16];                                                              // float(cg - zg), exact
  if constexpr (GATE == kRowF32) {
    const f32x4* __restrict__ gp = static_cast<const f32x4*>(a.g) + (size_t)gi * 4;
    f32x4 raw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = gp[q];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) dg[4 * q + j] = (float)ql_code(raw[q][j], a.gq) - a.gq.zf;
  } else {
    const u32x4 vg = static_cast<const u32x4*>(a.g)[gi];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t u = vg[q] ^ a.g_flip;
#pragma unroll
      for (int j = 0; j < 4; ++j) dg[4 * q + j] = (float)((u >> (8 * j)) & 0xffu) - a.g_zb;
    }
  }
  u32x4 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t u = va[q] ^ a.a_flip;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float da = (float)((u >> (8 * j)) & 0xffu) - a.a_zb;              // float(ca - za), exact
      const float m = join_residual(da, a.a_scale) * join_residual(dg[4 * q + j], a.g_scale);
      w |= ((uint32_t)ql_code(m, a.o) & 0xffu) << (8 * j);
    }
    v[q] = w;
  }
  a.out[i] = v;
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_mul_nhwc(const void* a, int32_t a_code_dtype, float a_scale, int32_t a_zero_point, const void* g,
                        int32_t g_code_dtype, float g_scale, int32_t g_zero_point, int32_t g_is_f32, int32_t g_quant_min,
                        int32_t g_quant_max, int64_t gate_pixels, void* out, int32_t out_code_dtype, int64_t pixels,
                        int64_t channels, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream) {
  if (pixels < 0) return fail_arg("pixels < 0");
  const struct { int32_t dtype, zp; float scale; FormWords w; } forms[3] = {
      {a_code_dtype, a_zero_point, a_scale, {"a_code_dtype", "a_zero_point", "a's type", "a_scale"}},
      {g_code_dtype, g_zero_point, g_scale, {"g_code_dtype", "g_zero_point", "g's type", "g_scale"}},
      {out_code_dtype, zero_point, scale, {"out_code_dtype", "zero_point", "the output's type", "scale"}}};
  // every code type, then every zero point, then every scale
  for (const auto& f : forms) if (int rc = form_check_dtype(f.dtype, f.w.dtype)) return rc;
  for (const auto& f : forms) if (int rc = form_check_zero_point(f.dtype, f.zp, f.w.zero_point, f.w.type)) return rc;
  for (const auto& f : forms) if (int rc = form_check_scale(f.scale, f.w.scale)) return rc;
  const CodeForm fa = code_form(a_code_dtype, a_zero_point, a_scale), fg = code_form(g_code_dtype, g_zero_point, g_scale);
  QlOut o, gq;
  if (int rc = ql_output_form(o, out_code_dtype, scale, zero_point, quant_min, quant_max)) return rc;
  if (gate_pixels < 0) return fail_arg("gate_pixels < 0");
  if (g_is_f32) {
    if (gate_pixels == 0) return fail_arg("a float32 g is taken in the row-broadcast form only (gate_pixels >= 1)");
    if (int rc = ql_output_form(gq, g_code_dtype, g_scale, g_zero_point, g_quant_min, g_quant_max)) return rc;
  } else {
    ql_output_form(gq, -1, 1.0f, 0, 0, 0);
  }
  if (channels <= 0 || channels % 16 != 0) return fail_arg("channels must be a positive multiple of 16");
  if (gate_pixels > 0 && pixels % gate_pixels != 0) return fail_arg("pixels is no multiple of gate_pixels");
  if (pixels == 0) return 0;
  const int64_t row = channels / 16;
  // a lane's index, pixel * row + chunk, and its gate chunk index below it are 31-bit numbers (beyond: split the pixels)
  if (row > INT32_MAX || pixels > INT32_MAX / row) return fail_arg("more than 2^31 - 1 16-byte chunks in one launch");
  if (!a) return fail_arg("a is NULL");
  if (!g) return fail_arg("g is NULL");
  if (!out) return fail_arg("out is NULL");
  if (((uintptr_t)a & 15u) != 0) return fail_arg("a must be 16-byte aligned");
  if (((uintptr_t)g & 15u) != 0) return fail_arg("g must be 16-byte aligned");
  if (((uintptr_t)out & 15u) != 0) return fail_arg("out must be 16-byte aligned");
  // the byte ranges: a lane would read codes another lane has overwritten (a and g may be one buffer: x * x)
  const uintptr_t bytes = (uintptr_t)pixels * (uintptr_t)channels;
  const uintptr_t g_bytes = gate_pixels == 0 ? bytes : bytes / (uintptr_t)gate_pixels * (g_is_f32 ? 4u : 1u);
  if (ranges_overlap(out, bytes, a, bytes)) return fail_arg("out overlaps a");
  if (ranges_overlap(out, bytes, g, g_bytes)) return fail_arg("out overlaps g");
  MulArgs k;
  k.a = static_cast<const u32x4*>(a); k.g = g; k.out = static_cast<u32x4*>(out);
  k.a_flip = fa.flip; k.g_flip = fg.flip;
  k.a_zb = (float)fa.zb; k.g_zb = (float)fg.zb;
  k.a_scale = fa.scale; k.g_scale = fg.scale;
  k.row = FastDiv::make((uint32_t)row);
  k.img = FastDiv::make((uint32_t)(gate_pixels == 0 ? 1 : gate_pixels));      // (gate_pixels <= pixels < 2^31, or pixels % it != 0)
  k.chunks = (uint32_t)(pixels * row);
  k.gq = gq; k.o = o;
  const unsigned blocks = (unsigned)(((int64_t)k.chunks + kThreads - 1) / kThreads);                  // <= 2^23
  const char* form;
  if (gate_pixels == 0) {
    hipLaunchKernelGGL(codes_mul_kernel<kSame>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    form = "same";
  } else if (!g_is_f32) {
    hipLaunchKernelGGL(codes_mul_kernel<kRow>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    form = "row";
  } else {
    hipLaunchKernelGGL(codes_mul_kernel<kRowF32>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    form = "row f32";
  }
  static thread_local char op_text[40];
  snprintf(op_text, sizeof(op_text), "%s * %s -> %s %s", fa.is_signed ? "i8" : "u8", fg.is_signed ? "i8" : "u8", o.mode == 1 ? "i8" : "u8", form);
  note_launch("codes_mul", op_text, 1, 0, 1, 1);
  return check_launch("mctq_codes_mul_nhwc");
}

}  // extern "C"
