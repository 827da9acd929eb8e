// mctq_codes_upsample.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Nearest resampling on NHWC activation codes: codes [B][H][W][C] (1 byte per element, int8 or uint8, form (scale_a, zp_a)) ->
// out [B][Ho][Wo][C] in the form of the holder behind the upsample.  A holder's float32 output is float(code - zp_a) * scale_a
// bit for bit (join_residual: the last step of AffineOp::apply), nearest interpolation only moves data, and the holder behind it
// codes every element with ql_code's arithmetic, so
//     out[b][ho][wo][c] = ql_code(join_residual(float(code[b][rows[ho]][cols[wo]][c] - zp_a), scale_a))
// is the code that holder gives the resampled float32 tensor, for every element -- nothing is approximated.  This is
// mctq_codes_concat_nhwc's arithmetic for one operand (requant_chunk) behind an index map; the map is separable, a source row
// per output row and a source column per output column, given as two device tables or as two integer factors (src = dst / f).
//
// Two forms with the same bytes (every output element is a function of one input code):
//   gather     that of mctq_codes_maxpool.hip: a lane owns one 16-byte chunk (16 channels) of one OUTPUT pixel, consecutive
//              lanes on consecutive chunks, then consecutive pixels; one 16-byte load through the map, one 16-byte store, both
//              plain.  The source index is 64-bit (a downsampled input may hold more than 2^32 chunks).  Every geometry.
//   replicate  integer factors only, factor_h * factor_w <= 16 (kReplicateMax: a lane's stores stay a short straight run):
//              a lane owns one 16-byte chunk of one INPUT pixel; one load, one requantization, factor_h * factor_w stores
//              into the fh x fw block of output pixels it maps to.  A wave's stores then fall in runs of C bytes
//              factor_w * C bytes apart.
// Tuning key "upsample_form": 0 = the launcher chooses, 1 = gather, 2 = replicate where eligible.  The launcher chooses
// replicate where it is eligible and factor_h * factor_w >= 2: measured 1.77 - 2.25 x faster than gather at batch 64 on 2 x and
// 4 x upsamples and equal at the launch floor at batch 1 (the launcher's comment below; profiles/EXPERIMENTS.md).  Not measured:
// factors other than 2 x 2 and 4 x 4.
//
// A map entry is clamped into [0, H - 1] / [0, W - 1] before it forms an address: the launcher cannot see device tables, and
// whatever they hold the loads stay inside the input.  Copy rule: concat's (form_is_copied, tuning key "concat_copy") -- an input
// whose form is the output's is stored as loaded.  No LDS, no scratch, nothing passes between lanes.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, QlOut, requant_chunk, form_check, form_is_copied, ranges_overlap

namespace mctq {

constexpr int kReplicateMax = 16;          // factor_h * factor_w of the replicate form

extern int g_upsample_form;                // tuning key "upsample_form" (mctq_misc.hip): 0 = auto, 1 = gather, 2 = replicate
extern int g_concat_copy;                  // tuning key "concat_copy" (mctq_misc.hip): 0 = nothing is copied

struct UpArgs {
  const u32x4* src;
  u32x4* out;
  const int32_t* rows;                     // device [Ho], [Wo]; NULL with factors
  const int32_t* cols;
  FastDiv c16;                             // chunks per pixel (C / 16)
  FastDiv wo, ho;                          // gather: the output extent
  FastDiv fh, fw;                          // the factors (1 with maps: unused)
  FastDiv w, h;                            // replicate: the input extent
  uint32_t chunks;                         // lanes: output chunks (gather), input chunks (replicate)
  int32_t H, W;
  uint32_t Wo, Ho;
  uint32_t flip;                           // 0x80808080 for int8 codes (code c -> byte c + 128), 0 for uint8
  float zb;                                // the zero point with the same bias: float(byte) - zb == float(code - zero_point)
  float scale;
  uint32_t copy;                           // the input has the output's form: store what was loaded
  QlOut o;
};

template <bool MAPS>
__global__ __launch_bounds__(kThreads) void codes_upsample_gather_kernel(UpArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^31: the launcher checks the chunk count
  if (g >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t cc, ox, oy;
  const uint32_t m = a.c16.divmod(g, cc);
  const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);                    // oy < Ho, ox < Wo: the tables' extents
  int iy, ix;
  if constexpr (MAPS) {
    iy = a.rows[oy]; ix = a.cols[ox];
  } else {
    uint32_t r;
    iy = (int)a.fh.divmod(oy, r); ix = (int)a.fw.divmod(ox, r);
  }
  iy = min(max(iy, 0), a.H - 1); ix = min(max(ix, 0), a.W - 1);              // a valid address whatever the table holds
  const int64_t c16 = a.c16.d;
  u32x4 v = a.src[(((int64_t)b * a.H + iy) * a.W + ix) * c16 + cc];          // b < B, iy < H, ix < W, cc < C / 16
  if (!a.copy) v = requant_chunk(v, a.flip, a.zb, a.scale, a.o);
  a.out[g] = v;
}

__global__ __launch_bounds__(kThreads) void codes_upsample_replicate_kernel(UpArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^31: input chunks <= output chunks
  if (g >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t cc, ix, iy;
  const uint32_t m = a.c16.divmod(g, cc);
  const uint32_t b = a.h.divmod(a.w.divmod(m, ix), iy);
  u32x4 v = a.src[g];
  if (!a.copy) v = requant_chunk(v, a.flip, a.zb, a.scale, a.o);
  const uint32_t c16 = a.c16.d, fh = a.fh.d, fw = a.fw.d;
  // the block's first output pixel: (b, iy * fh, ix * fw); its last chunk is below B * Ho * Wo * C / 16 < 2^31 as Ho == fh * H
  u32x4* __restrict__ dst = a.out + (((size_t)b * a.Ho + iy * fh) * a.Wo + ix * fw) * c16 + cc;
  for (uint32_t r = 0; r < fh; ++r)
    for (uint32_t s = 0; s < fw; ++s) dst[((size_t)r * a.Wo + s) * c16] = v;
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_upsample_nhwc(const void* codes, void* out, int32_t code_dtype, int32_t in_zero_point, float in_scale,
                             int64_t batch, int64_t height, int64_t width, int64_t channels, int64_t out_height,
                             int64_t out_width, int32_t factor_h, int32_t factor_w, const int32_t* src_rows,
                             const int32_t* src_cols, int32_t out_code_dtype, float scale, int32_t zero_point,
                             int32_t quant_min, int32_t quant_max, void* stream) {
  if (batch < 0 || height < 0 || width < 0 || channels < 0 || out_height < 0 || out_width < 0) return fail_arg("negative extent");
  if (channels % 16 != 0) return fail_arg("channels must be a multiple of 16");
  if (int rc = form_check(code_dtype, in_zero_point, in_scale, {"code_dtype", "in_zero_point", "the input's type", "in_scale"})) return rc;
  const FormWords ow = {"out_code_dtype", "zero_point", "the output's type", "scale"};
  if (int rc = form_check(out_code_dtype, zero_point, scale, ow)) return rc;
  QlOut o;
  if (int rc = ql_output_form(o, out_code_dtype, scale, zero_point, quant_min, quant_max)) return rc;
  const bool maps = src_rows || src_cols, factors = factor_h != 0 || factor_w != 0;
  if (maps == factors) return fail_arg("give either src_rows and src_cols (factors 0) or factor_h and factor_w (maps NULL)");
  if (maps && (!src_rows || !src_cols)) return fail_arg("src_rows and src_cols go together");
  if (factors && (factor_h < 1 || factor_w < 1)) return fail_arg("factor_h and factor_w must be at least 1");
  if (height > INT32_MAX || width > INT32_MAX || out_height > INT32_MAX || out_width > INT32_MAX)
    return fail_arg("an image extent exceeds 2^31 - 1");
  if (factors && (out_height != factor_h * height || out_width != factor_w * width))
    return fail_arg("out_height / out_width are not factor_h * height / factor_w * width");
  if (batch == 0 || channels == 0 || out_height == 0 || out_width == 0) return 0;
  if (height == 0 || width == 0) return fail_arg("a non-empty output needs an image of at least one pixel");
  const int64_t c16 = channels / 16;
  // a lane's index, pixel * (channels / 16) + chunk, is a 31-bit number (beyond it: split the batch)
  int64_t out_chunks, in_chunks;
  if (__builtin_mul_overflow(out_height, out_width, &out_chunks) || __builtin_mul_overflow(out_chunks, batch, &out_chunks)
      || __builtin_mul_overflow(out_chunks, c16, &out_chunks) || out_chunks > INT32_MAX)
    return fail_arg("more than 2^31 - 1 16-byte chunks of output in one launch");
  if (__builtin_mul_overflow(height, width, &in_chunks) || __builtin_mul_overflow(in_chunks, batch, &in_chunks)
      || __builtin_mul_overflow(in_chunks, c16, &in_chunks) || in_chunks > (INT64_MAX >> 5))
    return fail_arg("the input's byte count exceeds 2^62");
  if (!codes || !out) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)out)) & 15u) != 0) return fail_arg("codes and out must be 16-byte aligned");
  if (maps && ((((uintptr_t)src_rows) | ((uintptr_t)src_cols)) & 3u) != 0) return fail_arg("src_rows and src_cols must be 4-byte aligned");
  // the byte ranges: a lane would read codes (or table entries) another lane has overwritten
  const size_t out_bytes = (size_t)out_chunks * 16u;
  if (ranges_overlap(out, out_bytes, codes, (size_t)in_chunks * 16u)) return fail_arg("out overlaps codes");
  if (maps && (ranges_overlap(out, out_bytes, src_rows, (size_t)out_height * 4u) || ranges_overlap(out, out_bytes, src_cols, (size_t)out_width * 4u)))
    return fail_arg("out overlaps a map");
  const CodeForm f = code_form(code_dtype, in_zero_point, in_scale);
  UpArgs a;
  a.src = static_cast<const u32x4*>(codes);
  a.out = static_cast<u32x4*>(out);
  a.rows = src_rows; a.cols = src_cols;
  a.c16 = FastDiv::make((uint32_t)c16);
  a.wo = FastDiv::make((uint32_t)out_width); a.ho = FastDiv::make((uint32_t)out_height);
  a.fh = FastDiv::make((uint32_t)(factors ? factor_h : 1)); a.fw = FastDiv::make((uint32_t)(factors ? factor_w : 1));
  a.w = FastDiv::make((uint32_t)width); a.h = FastDiv::make((uint32_t)height);
  a.H = (int32_t)height; a.W = (int32_t)width; a.Wo = (uint32_t)out_width; a.Ho = (uint32_t)out_height;
  a.flip = f.flip; a.zb = (float)f.zb; a.scale = f.scale;
  a.copy = g_concat_copy && form_is_copied(code_dtype, in_zero_point, in_scale, out_code_dtype, zero_point, scale, quant_min, quant_max);
  a.o = o;
  // Auto: the replicate form wherever it is eligible and has something to replicate (factor_h * factor_w >= 2).  Measured (one
  // MI355X; tools/upsample_consumer_probe.py, section forms; table in profiles/EXPERIMENTS.md): 2 x on 256 x 28 x 28,
  // 128 x 56 x 56, 64 x 112 x 112 and 4 x on 128 x 28 x 28.  At batch 64 replicate takes 1.77 - 2.25 x less (12.2 against 22.1 us
  // ... 43.2 against 79.1 us): a quarter (a sixteenth) of the loads and of the requantization, and the strided runs of stores
  // cost less than that saves.  At batch 1 both sit at the launch floor (8.2 - 8.5 us, 0.99 - 1.02, spreads overlapping).
  const int64_t block = (int64_t)factor_h * factor_w;
  const bool replicate = factors && block <= kReplicateMax && (g_upsample_form == 2 || (g_upsample_form == 0 && block >= 2));
  a.chunks = (uint32_t)(replicate ? in_chunks : out_chunks);                // (factors: in_chunks <= out_chunks)
  const unsigned blocks = (unsigned)(((int64_t)a.chunks + kThreads - 1) / kThreads);                  // <= 2^23
  const hipStream_t s = (hipStream_t)stream;
  if (replicate) hipLaunchKernelGGL(codes_upsample_replicate_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
  else if (maps) hipLaunchKernelGGL(codes_upsample_gather_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(codes_upsample_gather_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, a);
  static thread_local char op_text[32];
  snprintf(op_text, sizeof(op_text), "%s -> %s %s", f.is_signed ? "i8" : "u8", o.mode == 1 ? "i8" : "u8", replicate ? "replicate" : "gather");
  note_launch("codes_upsample", op_text, 1, 0, 1, 1);
  return check_launch("mctq_codes_upsample_nhwc");
}

}  // extern "C"
