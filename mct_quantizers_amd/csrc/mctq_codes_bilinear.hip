// mctq_codes_bilinear.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Bilinear resampling on NHWC activation codes: codes [B][H][W][C] (1 byte per element, int8 or uint8, form (scale_a, zp_a)) ->
// out [B][Ho][Wo][C] in the form of the holder behind the upsample.  A blend creates new values, so unlike the nearest kernel
// (mctq_codes_upsample.hip) this one has a contract of its own, on integers, with fixed-point weights of WB = 11 bits.  Each
// axis has three int32 tables of the output extent: i0 and i1, source indices, and w1, the weight of i1 in [0, 2^WB]; the
// weight of i0 is 2^WB - w1.  Per output element
//     h(r, ox) = (2^WB - wc[ox]) * (c[r][c0[ox]] - zp_a) + wc[ox] * (c[r][c1[ox]] - zp_a)
//     acc      = (2^WB - wr[oy]) * h(r0[oy], ox) + wr[oy] * h(r1[oy], ox)          |acc| <= 2^22 * 255 < 2^31: an exact int32
//     y        = float32(acc) * (float32(scale_a) * 2^-22)                         the factor is exact; one conversion, one multiply
//     code     = ql_code(y)                                                        clamp(rint(y * (1 / scale)) + zp, qmin, qmax)
// Nothing depends on how lanes split the work, so every instance below and the torch route of ops.codes_upsample_bilinear
// give the same bytes.  The arithmetic runs on unsigned bytes (int8 with bit 7 flipped, u = code + bias); the weights of an
// axis sum to 2^WB, so the zero point enters once, as 2^22 * (zp_a + bias) subtracted from the blend of the bytes.
//
// The kernel: a lane owns one 16-byte chunk (16 channels) of one output column for a strip of R consecutive output rows.
// Lanes run fastest over chunk, then column -- a wave's stores are 1 KiB runs of one output row -- and a workgroup lies inside
// one strip of one image, so the row entries r0, r1, wr are uniform over it and need no vector registers.  The lane fetches its
// column entries once.  Walking down the strip it keeps the two horizontally blended input rows it is between (2 x 16 int32):
// when r0 advances to the old r1 that blend is reused, and only the new row is loaded and blended (two 16-byte loads, 32
// multiply-adds).  For a 2 x upsample that cuts loads and horizontal arithmetic by about the vertical factor against R = 1,
// the plain per-pixel form (the same code, a strip of one row).  Tuning key "bilinear_strip": 0 = the launcher chooses, else
// R in {1, 4, 8}.  Whatever the tables hold, indices are clamped into the image and weights into [0, 2^WB] before use.
// No LDS, no scratch, nothing passes between lanes.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, QlOut, ql_code, form_check, ranges_overlap

namespace mctq {

constexpr int kWB = 11;                    // weight bits per axis: 2^(2 * kWB) * 255 < 2^31
constexpr int kOne = 1 << kWB;

extern int g_bilinear_strip;               // tuning key "bilinear_strip" (mctq_misc.hip): 0 = auto, else 1, 4 or 8

struct BlArgs {
  const u32x4* src;
  u32x4* out;
  const int32_t* r0;                       // device [Ho] each
  const int32_t* r1;
  const int32_t* wr;
  const int32_t* c0;                       // device [Wo] each
  const int32_t* c1;
  const int32_t* wc;
  FastDiv c16;                             // chunks per pixel (C / 16)
  FastDiv xblocks;                         // workgroups per output row: ceil(Wo * C / 16 / kThreads)
  FastDiv strips;                          // strips per image: ceil(Ho / R)
  uint32_t row_chunks;                     // Wo * C / 16
  int32_t H, W;
  uint32_t Ho;
  uint32_t flip;                           // 0x80808080 for int8 codes (code c -> byte c + 128), 0 for uint8
  int32_t zb22;                            // 2^22 * (zero point with the same bias) <= 255 * 2^22
  float scale22;                           // float32(scale_a) * 2^-22
  QlOut o;
};

// h[k] = (2^WB - wc) * u0[k] + wc * u1[k] for the 16 bytes of the chunks at columns c0 and c1 of one input row: <= 2^WB * 255
__device__ __forceinline__ void blend_row(const BlArgs& a, int64_t row, int c0, int c1, int wc, uint32_t cc, int (&h)[16]) {
  const int64_t c16 = a.c16.d;
  const u32x4 p = a.src[(row * a.W + c0) * c16 + cc];                        // row < B * H, c0, c1 < W, cc < C / 16
  if (c1 == c0 || wc == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) h[k] = (int)(((p[k >> 2] ^ a.flip) >> (8 * (k & 3))) & 0xffu) << kWB;
    return;
  }
  const u32x4 q = a.src[(row * a.W + c1) * c16 + cc];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int u0 = (int)(((p[k >> 2] ^ a.flip) >> (8 * (k & 3))) & 0xffu);
    const int u1 = (int)(((q[k >> 2] ^ a.flip) >> (8 * (k & 3))) & 0xffu);
    h[k] = (u0 << kWB) + wc * (u1 - u0);
  }
}

template <int R>
__global__ __launch_bounds__(kThreads) void codes_bilinear_kernel(BlArgs a) {
  uint32_t xb, st, cc;
  const uint32_t image = a.strips.divmod(a.xblocks.divmod(blockIdx.x, xb), st);        // < B: the launcher's grid
  const uint32_t oy0 = st * R;                                                         // < Ho
  // the strip's row entries, uniform over the workgroup, fetched before the first store; rows past Ho repeat the last one
  int r0[R], r1[R], wr[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint32_t oy = min(oy0 + j, a.Ho - 1);
    r0[j] = min(max(a.r0[oy], 0), a.H - 1);
    r1[j] = min(max(a.r1[oy], 0), a.H - 1);
    wr[j] = min(max(a.wr[oy], 0), kOne);
  }
  const uint32_t p = xb * (uint32_t)kThreads + threadIdx.x;
  if (p >= a.row_chunks) return;                                                       // the row's last workgroup may be partly empty
  const uint32_t ox = a.c16.divmod(p, cc);                                             // < Wo: the tables' extent
  const int c0 = min(max(a.c0[ox], 0), a.W - 1), c1 = min(max(a.c1[ox], 0), a.W - 1);
  const int wc = min(max(a.wc[ox], 0), kOne);
  const int64_t first_row = (int64_t)image * a.H;
  u32x4* __restrict__ dst = a.out + ((size_t)image * a.Ho + oy0) * a.row_chunks + p;   // < 2^31 chunks: the launcher checks
  int top[16], bot[16];                                                                // the blends of input rows it, ib
  int it = -1, ib = -1;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (oy0 + j >= a.Ho) break;                                                        // a ragged last strip (uniform)
    if (r0[j] != it) {                                                                 // (uniform, like every branch of the walk)
      if (r0[j] == ib) {
#pragma unroll
        for (int k = 0; k < 16; ++k) top[k] = bot[k];
      } else {
        blend_row(a, first_row + r0[j], c0, c1, wc, cc, top);
      }
      it = r0[j];
    }
    const bool two = r1[j] != it && wr[j] != 0;
    if (two && r1[j] != ib) {
      blend_row(a, first_row + r1[j], c0, c1, wc, cc, bot);
      ib = r1[j];
    }
    u32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * q + i;
        int acc = top[k] << kWB;                                                       // <= 2^22 * 255
        if (two) acc += wr[j] * (bot[k] - top[k]);                                     // |.| <= 2^22 * 255; the sum stays in [0, 2^22 * 255]
        const float y = (float)(acc - a.zb22) * a.scale22;
        w |= ((uint32_t)ql_code(y, a.o) & 0xffu) << (8 * i);
      }
      v[q] = w;
    }
    dst[(size_t)j * a.row_chunks] = v;
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_upsample_bilinear_nhwc(const void* codes, void* out, int32_t code_dtype, int32_t in_zero_point, float in_scale,
                                      int64_t batch, int64_t height, int64_t width, int64_t channels, int64_t out_height,
                                      int64_t out_width, const int32_t* row0, const int32_t* row1, const int32_t* row_w1,
                                      const int32_t* col0, const int32_t* col1, const int32_t* col_w1, int32_t out_code_dtype,
                                      float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream) {
  if (batch < 0 || height < 0 || width < 0 || channels < 0 || out_height < 0 || out_width < 0) return fail_arg("negative extent");
  if (channels % 16 != 0) return fail_arg("channels must be a multiple of 16");
  if (int rc = form_check(code_dtype, in_zero_point, in_scale, {"code_dtype", "in_zero_point", "the input's type", "in_scale"})) return rc;
  const FormWords ow = {"out_code_dtype", "zero_point", "the output's type", "scale"};
  if (int rc = form_check(out_code_dtype, zero_point, scale, ow)) return rc;
  QlOut o;
  if (int rc = ql_output_form(o, out_code_dtype, scale, zero_point, quant_min, quant_max)) return rc;
  if (height > INT32_MAX || width > INT32_MAX || out_height > INT32_MAX || out_width > INT32_MAX)
    return fail_arg("an image extent exceeds 2^31 - 1");
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
  const int32_t* tables[6] = {row0, row1, row_w1, col0, col1, col_w1};
  if (!codes || !out) return fail_arg("NULL pointer");
  for (const int32_t* t : tables)
    if (!t) return fail_arg("NULL table");
  if (((((uintptr_t)codes) | ((uintptr_t)out)) & 15u) != 0) return fail_arg("codes and out must be 16-byte aligned");
  for (const int32_t* t : tables)
    if (((uintptr_t)t & 3u) != 0) return fail_arg("the tables must be 4-byte aligned");
  // the byte ranges: a lane would read codes (or table entries) another lane has overwritten
  const size_t out_bytes = (size_t)out_chunks * 16u;
  if (ranges_overlap(out, out_bytes, codes, (size_t)in_chunks * 16u)) return fail_arg("out overlaps codes");
  for (int i = 0; i < 6; ++i)
    if (ranges_overlap(out, out_bytes, tables[i], (size_t)(i < 3 ? out_height : out_width) * 4u)) return fail_arg("out overlaps a table");
  const int64_t row_chunks = out_width * c16;                                          // <= out_chunks
  const int64_t xblocks = (row_chunks + kThreads - 1) / kThreads;
  // Auto: the longest strip that still leaves four workgroups per CU, and R = 1 where the image has fewer than two strips of
  // that length (the reuse down a strip is then short against the rows it serialises).  The rule is grid arithmetic and was
  // written before any measurement; the table it was then held against agrees with it (one MI355X;
  // tools/bilinear_consumer_probe.py, section strips; profiles/EXPERIMENTS.md): 2 x on 256 x 28 x 28, 128 x 56 x 56,
  // 64 x 112 x 112 and 4 x on 128 x 28 x 28.  At batch 64 the rule takes R = 8, the fastest: 1.27 - 1.48 x less than R = 1 (32.2
  // against 40.9 us ... 110.9 against 159.0 us), R = 4 in between.  At batch 1 it takes R = 1: R = 1 and R = 4 sit at the
  // launch floor (8.7 - 8.9 us, spreads overlapping) and R = 8 takes 1 - 18 % more.  Not measured: other factors, downsampling.
  int strip = g_bilinear_strip;
  if (strip == 0) {
    strip = 1;
    for (int r : {8, 4})
      if (out_height >= 2 * r && batch * ((out_height + r - 1) / r) * xblocks >= 4 * (int64_t)cu_count()) { strip = r; break; }
  }
  const int64_t strips = (out_height + strip - 1) / strip;
  const int64_t blocks = batch * strips * xblocks;                                     // <= out_chunks < 2^31
  const CodeForm f = code_form(code_dtype, in_zero_point, in_scale);
  BlArgs a;
  a.src = static_cast<const u32x4*>(codes);
  a.out = static_cast<u32x4*>(out);
  a.r0 = row0; a.r1 = row1; a.wr = row_w1; a.c0 = col0; a.c1 = col1; a.wc = col_w1;
  a.c16 = FastDiv::make((uint32_t)c16);
  a.xblocks = FastDiv::make((uint32_t)xblocks); a.strips = FastDiv::make((uint32_t)strips);
  a.row_chunks = (uint32_t)row_chunks;
  a.H = (int32_t)height; a.W = (int32_t)width; a.Ho = (uint32_t)out_height;
  a.flip = f.flip; a.zb22 = f.zb * (1 << (2 * kWB)); a.scale22 = f.scale * 0x1p-22f;
  a.o = o;
  const hipStream_t s = (hipStream_t)stream;
  if (strip == 8) hipLaunchKernelGGL(codes_bilinear_kernel<8>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else if (strip == 4) hipLaunchKernelGGL(codes_bilinear_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(codes_bilinear_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  static thread_local char op_text[32];
  snprintf(op_text, sizeof(op_text), "%s -> %s strip %d", f.is_signed ? "i8" : "u8", o.mode == 1 ? "i8" : "u8", strip);
  note_launch("codes_bilinear", op_text, 1, 0, 1, 1);
  return check_launch("mctq_codes_upsample_bilinear_nhwc");
}

}  // extern "C"
