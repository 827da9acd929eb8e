// mctq_codes_concat.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Channel concatenation on NHWC activation codes: up to 8 operands [pixels][C_k] (1 byte per element, int8 or uint8, each
// with its own scale and zero point) -> out [pixels][sum C_k] in the form of the holder behind the torch.cat.  A holder's
// float32 output is float(code - zp_k) * scale_k bit for bit (join_residual: the last step of AffineOp::apply), torch.cat
// only moves data, and the holder behind it codes every element with ql_code's arithmetic, so
//     out[p][ch] = ql_code(join_residual(float(code_k[p][ch - start_k] - zp_k), scale_k))
// is the code that holder gives the concatenated float32 tensor, for every element -- nothing is approximated.
//
// Form: that of mctq_codes_maxpool.hip.  A lane owns one 16-byte chunk of the output; consecutive lanes take consecutive
// chunks of a row and then consecutive rows.  Every C_k is a multiple of 16, so a chunk of the output is one aligned chunk
// of exactly one operand: one 16-byte load, one 16-byte store, both plain (a product reads the output next).  The pixel
// and the chunk within the row come from one FastDiv; the operand from a compare chain over the 8 prefix sums, which also
// selects the operand's pointer, width and parameters -- constant indices into the kernel arguments, which stay in scalar
// registers (a lane-dependent index would send the arrays to scratch).
//
// Copy operands: an operand whose form is the output's (same scale bits, zero point and code type, a clamp domain that
// holds every code of the type) is marked by the launcher, and its lanes store what they loaded -- for such a form
// ql_code(join_residual(code - zp, s)) == code: (code - zp) * s * (1 / s) lies within 255 * 3 * 2^-24 of the integer
// code - zp.  The launcher marks only scales in [2^-100, 2^100], where neither the product nor the reciprocal can
// overflow or underflow.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, QlOut, requant_chunk, form_is_copied

namespace mctq {

constexpr int kConcatMax = 8;

extern int g_concat_copy;                  // tuning key "concat_copy" (mctq_misc.hip): 0 = no operand is marked as a copy

struct ConcatArgs {
  const u32x4* src[kConcatMax];
  uint32_t end[kConcatMax];                // operand k owns the chunks [end[k - 1], end[k]) of a row; unused ones: the row's length
  uint32_t flip[kConcatMax];               // 0x80808080 for int8 codes (code c -> byte c + 128), 0 for uint8
  float zb[kConcatMax];                    // the zero point with the same bias: float(byte) - zb == float(code - zero_point)
  float scale[kConcatMax];
  uint32_t copy;                           // bit k: operand k has the output's form
  u32x4* out;
  FastDiv row;                             // chunks per output row (sum C_k / 16)
  uint32_t chunks;                         // pixels * row.d
  QlOut o;
};

__global__ __launch_bounds__(kThreads) void codes_concat_kernel(ConcatArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^31: the launcher checks the chunk count
  if (g >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t cc;
  const uint32_t pixel = a.row.divmod(g, cc);
  // Every operand's parameters into scalar registers first, as one batch of scalar loads: left to itself the compiler
  // selects the ADDRESS of the kernel argument per lane and loads pointer and parameters from there, one dependent load
  // after the other in front of the data load.
  const u32x4* srcs[kConcatMax];
  uint32_t ends[kConcatMax], flips[kConcatMax];
  float zbs[kConcatMax], scales[kConcatMax];
#pragma unroll
  for (int k = 0; k < kConcatMax; ++k) {
    srcs[k] = a.src[k]; ends[k] = a.end[k]; flips[k] = a.flip[k]; zbs[k] = a.zb[k]; scales[k] = a.scale[k];
    asm volatile("" : "+s"(srcs[k]), "+s"(ends[k]), "+s"(flips[k]), "+s"(zbs[k]), "+s"(scales[k]));
  }
  // the operand of chunk cc: the last k with end[k - 1] <= cc (end[] is non-decreasing)
  const u32x4* __restrict__ src = srcs[0];
  uint32_t start = 0, width = ends[0], flip = flips[0], k_of = 0;
  float zb = zbs[0], scale = scales[0];
#pragma unroll
  for (int k = 1; k < kConcatMax; ++k) {
    const bool here = cc >= ends[k - 1];
    src = here ? srcs[k] : src; start = here ? ends[k - 1] : start; width = here ? ends[k] - ends[k - 1] : width;
    flip = here ? flips[k] : flip; zb = here ? zbs[k] : zb; scale = here ? scales[k] : scale; k_of = here ? k : k_of;
  }
  const bool copy = ((a.copy >> k_of) & 1u) != 0;
  // pixel < pixels and cc - start < width: the chunk index is below pixels * C_k / 16, and below 2^31 as g is
  u32x4 v = src[pixel * width + (cc - start)];
  if (!copy) v = requant_chunk(v, flip, zb, scale, a.o);
  a.out[g] = v;
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_concat_nhwc(const mctq_concat_item* items, int32_t count, void* out, int32_t out_code_dtype, int64_t pixels,
                           float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream) {
  if (count < 1 || count > kConcatMax) return fail_arg("count must be 1 .. 8");
  if (!items) return fail_arg("items is NULL");
  if (pixels < 0) return fail_arg("pixels < 0");
  const FormWords ow = {"out_code_dtype", "zero_point", "the output's type", "scale"};
  if (int rc = form_check_scale(scale, ow.scale)) return rc;
  QlOut o;
  if (int rc = form_check_dtype(out_code_dtype, ow.dtype)) return rc;
  if (int rc = ql_output_form(o, out_code_dtype, scale, zero_point, quant_min, quant_max)) return rc;
  const bool o_signed = out_code_dtype == MCTQ_CODE_I8;
  if (int rc = form_check_zero_point(out_code_dtype, zero_point, ow.zero_point, ow.type)) return rc;
  int64_t row = 0;                                                           // chunks per output row
  for (int k = 0; k < count; ++k) {
    const mctq_concat_item& it = items[k];
    if (int rc = form_check(it.code_dtype, it.zero_point, it.scale,
                            {"code_dtype of an operand", "an operand's zero_point", "its type", "an operand's scale"})) return rc;
    if (it.channels <= 0 || it.channels % 16 != 0) return fail_arg("an operand's channels must be a positive multiple of 16");
    if (it.channels / 16 > INT32_MAX - row) return fail_arg("more than 2^31 - 1 16-byte chunks in one launch");
    row += it.channels / 16;
  }
  if (pixels == 0) return 0;
  // a lane's index, pixel * row + chunk, and every operand's chunk index below it are 31-bit numbers (beyond: split the pixels)
  if (pixels > INT32_MAX / row) return fail_arg("more than 2^31 - 1 16-byte chunks in one launch");
  if (!out) return fail_arg("out is NULL");
  if (((uintptr_t)out & 15u) != 0) return fail_arg("out must be 16-byte aligned");
  ConcatArgs a;
  a.copy = 0;
  uint32_t end = 0;
  for (int k = 0; k < kConcatMax; ++k) {
    if (k >= count) {                                                        // never selected: cc < row.d == end[k - 1]
      a.src[k] = nullptr; a.end[k] = end; a.flip[k] = 0; a.zb[k] = 0.0f; a.scale[k] = 1.0f;
      continue;
    }
    const mctq_concat_item& it = items[k];
    if (!it.codes) return fail_arg("an operand's codes pointer is NULL");
    if (((uintptr_t)it.codes & 15u) != 0) return fail_arg("an operand's codes must be 16-byte aligned");
    // the two byte ranges: a lane would read codes another lane has overwritten
    if (ranges_overlap(out, (size_t)pixels * (size_t)row * 16u, it.codes, (size_t)pixels * (size_t)it.channels))
      return fail_arg("out overlaps an operand");
    const CodeForm f = code_form(it.code_dtype, it.zero_point, it.scale);
    end += (uint32_t)(it.channels / 16);
    a.src[k] = static_cast<const u32x4*>(it.codes);
    a.end[k] = end;
    a.flip[k] = f.flip; a.zb[k] = (float)f.zb; a.scale[k] = f.scale;
    if (g_concat_copy && form_is_copied(it.code_dtype, it.zero_point, it.scale, out_code_dtype, zero_point, scale, quant_min, quant_max))
      a.copy |= 1u << k;
  }
  a.out = static_cast<u32x4*>(out);
  a.row = FastDiv::make((uint32_t)row);
  a.chunks = (uint32_t)(pixels * row);
  a.o = o;
  const unsigned blocks = (unsigned)(((int64_t)a.chunks + kThreads - 1) / kThreads);                  // <= 2^23
  hipLaunchKernelGGL(codes_concat_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  static thread_local char op_text[24];
  snprintf(op_text, sizeof(op_text), "%d -> %s", (int)count, o_signed ? "i8" : "u8");
  note_launch("codes_concat", op_text, 1, 0, 1, 1);
  return check_launch("mctq_codes_concat_nhwc");
}

}  // extern "C"
