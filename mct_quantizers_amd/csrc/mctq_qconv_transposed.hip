// mctq_qconv_transposed.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Transposed convolution on the quantizers' codes (nn.ConvTranspose2d with groups == 1 and dilation == 1, strides of at most 4,
// C % 16 == 0): the learned 2 x 2 stride-2 upsampling of a U-Net decoder, the 4 x 4 stride-2 one of a segmentation head or a GAN
// generator, the 3 x 3 stride-2 one with output_padding 1.
//     acc[b][oy][ox][o] = sum over c, ky, kx with iy * sh = oy + ph - ky, ix * sw = ox + pw - kx, 0 <= iy < H, 0 <= ix < W of
//                         (a[b][iy][ix][c] - za) * (w[c][o][ky][kx] - zw[o])
//     y = float(acc) * (sa * sw[o]) (+ bias[o])
// with the epilogue of mctq_qlinear_i8 (one rounding per float32 operation; -ffp-contract=off) and its output forms (QlOut).
//
// Phase decomposition.  An output pixel has the phase (ry, rx) = ((oy + ph) mod sh, (ox + pw) mod sw) and the quotient (qy, qx) =
// ((oy + ph) div sh, (ox + pw) div sw).  Only the taps ky = ry + sh * ty, kx = rx + sw * tx reach it, ty < Ty(ry) = max(0,
// ceil((kh - ry) / sh)), tx < Tx(rx) likewise, and tap (ty, tx) reads the input pixel (qy - ty, qx - tx).  For the pixels of one
// phase the layer is a plain stride-1 correlation of the NHWC codes with that phase's sub-kernel over K(ry, rx) = Ty * Tx * C
// columns: consecutive output pixels of a phase read consecutive input pixels, and no multiply is spent on the zeros a
// zero-stuffed formulation would insert.  It runs on the integer matrix cores (v_mfma_i32_16x16x64_i8) as mctq_qconv_grouped.hip
// does, with "group" read as "phase".
//
// Wave tile: 16 consecutive pixels (rows) of the phase's own flattened (b, jy, jx) order, M(ry, rx) = B * Hr(ry) * Wr(rx) with
// oy = sh * (qy_lo(ry) + jy) + ry - ph, x up to 4 N tiles of 16 output channels.  The tap list is uniform over the wave.  K order
// inside a phase is (ty, tx, c): C % 16 == 0, so a 16-byte chunk never straddles a tap and is one aligned load.  Fragment layout
// as in mctq_qlinear.hip: lane l holds the 16 bytes k = 16 * (l >> 4) .. + 15 of pixel row l & 15 (A) or of output channel
// l & 15 (B); in the result the column is l & 15 and the row 4 * (l >> 4) + reg.  Weights: the host keeps them as int8
// [P][Op][Kp], P = sh * sw, Op = 16 * ceil(O / 16), Kp = 64 * ceil(max over phases of K / 64), padded rows and columns the code
// 0: every weight load is an unguarded aligned 16-byte load.  The K loop of a block runs to its own phase's extent rounded up to
// 64, not to Kp; a phase without taps (k < s: output pixels no tap reaches) runs no step and writes the bias alone.
//
// Every A address is formed from coordinates clamped into the image; a chunk of a tap outside the image, or of the tail behind
// the phase's K, is loaded from a valid address and replaced by zero-point bytes by select: it adds (za - za) * (w - zw) = 0 (a
// tail chunk stands against weight zeros as well).  No load reads outside a_codes.  uint8 codes are xor-ed with 0x80 into int8
// (za' = za - 128) and the sum is corrected by za' * w_rowsum[phase][o].  Weight zero points: one more MFMA per K step against
// a register fragment of ones gives S[row], the sum of the row's a' over the steps' columns, and sum_k (a - za) = S - steps *
// 64 * za' exactly (mctq_qconv_grouped.hip).  All correction terms are added in wrapping arithmetic: only their total,
// |sum| <= 255 * 255 * 32768 < 2^31, is known to fit.
//
// Block: 256 threads = 4 waves = 64 pixels of ONE phase and one N slice of 64 channels.  Grid x = ceil(max over phases of M / 64),
// grid y = P * ceil(Op / 64).  Waves at or beyond their phase's M return -- a phase with M == 0, which small outputs have,
// included -- before anything is clamped to M - 1.  No LDS, no atomics, no split-K: every output element is written by exactly
// one lane (every output pixel has one phase and one (jy, jx) in it).
#include "mctq_consumer.hpp"

namespace mctq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxStride = 4;

struct TransposedArgs {
  const uint8_t* x;
  const int8_t* w;                                 // [P][Op][Kp]
  const float* w_scales;
  const int32_t* w_rowsum;                         // [P][O]
  const int32_t* w_zero_points;
  const float* bias;
  void* y;
  FastDiv c, slices;                               // C; N slices per phase (ceil(Op / 64))
  // per ry (per rx): the divisor of the phase's rows (columns) and, per rx, of its taps along x -- 1 where the count is 0
  FastDiv hr[kMaxStride], wr[kMaxStride], tx[kMaxStride];
  // per ry (per rx): the first quotient inside the output, the number of output rows (columns), the taps
  int32_t q_lo_y[kMaxStride], cnt_y[kMaxStride], taps_y[kMaxStride];
  int32_t q_lo_x[kMaxStride], cnt_x[kMaxStride], taps_x[kMaxStride];
  int32_t B, H, W, C, O, Op, Kp, Ho, Wo, stride_h, stride_w, pad_h, pad_w;
  int32_t za;                                      // the zero point as a code; the kernel subtracts 128 for uint8 codes
  float sa;
  QlOut oq;
};

// t[i] of a table in the kernel's arguments, i uniform over the block: selects, so that the table stays in scalar registers
template <class T>
__device__ __forceinline__ T pick(const T (&t)[kMaxStride], uint32_t i) {
  return i == 0 ? t[0] : i == 1 ? t[1] : i == 2 ? t[2] : t[3];
}

// What a wave knows of its phase and a lane of its pixel row.
struct TransposedRow {
  FastDiv txd;
  int32_t taps;                                    // Ty * Tx
  int32_t qy, qx;                                  // the pixel's quotients: tap (ty, tx) reads the input pixel (qy - ty, qx - tx)
  int64_t image;                                   // b * H
};

// The 16 bytes k .. k + 15 (k % 16 == 0, k < the phase's K rounded up to 64) of one pixel row's K axis; chunks of taps outside
// the image or behind the phase's K hold the pad byte.
__device__ __forceinline__ i32x4 transposed_a_chunk(const TransposedArgs& a, const TransposedRow& p, uint32_t k, uint32_t pad4) {
  uint32_t cu, txu;
  const uint32_t tap = a.c.divmod(k, cu);
  const int32_t ty = (int32_t)p.txd.divmod(tap, txu);
  const int32_t iy = p.qy - ty, ix = p.qx - (int32_t)txu;            // |.| < 2^31: q < 2^31, taps <= 32768
  // a valid address whatever the tap: 0 <= cy < H, 0 <= cx < W, cu + 16 <= C
  const int32_t cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
  const bool live = (int32_t)tap < p.taps && (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
  const u32x4 v = *reinterpret_cast<const u32x4*>(a.x + (((p.image + cy) * a.W + cx) * (int64_t)a.C + cu));
  i32x4 out;
#pragma unroll
  for (int q = 0; q < 4; ++q) out[q] = (int)(live ? v[q] : pad4);
  return out;
}

template <bool A_U8, bool ZP>
__global__ __launch_bounds__(kThreads) void qconv_transposed_kernel(TransposedArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kb = lane >> 4;
  uint32_t slice;
  const uint32_t phase = a.slices.divmod(blockIdx.y, slice);        // < sh * sw
  const uint32_t usw = (uint32_t)a.stride_w;
  const uint32_t ry = (phase >= usw) + (phase >= 2 * usw) + (phase >= 3 * usw), rx = phase - ry * usw;
  const int32_t Hr = pick(a.cnt_y, ry), Wr = pick(a.cnt_x, rx);
  const uint32_t M = (uint32_t)a.B * (uint32_t)Hr * (uint32_t)Wr;   // <= B * Ho * Wo <= 2^31 - 1
  const uint32_t m0 = blockIdx.x * 64u + (uint32_t)wave * 16u;      // < max M + 64
  if (m0 >= M) return;                                              // an idle wave, an empty phase (no barrier below)
  const FastDiv hrd = pick(a.hr, ry), wrd = pick(a.wr, rx);
  const int32_t qy0 = pick(a.q_lo_y, ry), qx0 = pick(a.q_lo_x, rx);
  TransposedRow p;
  p.txd = pick(a.tx, rx);
  p.taps = pick(a.taps_y, ry) * pick(a.taps_x, rx);
  const int32_t kloop = (p.taps * a.C + 63) & ~63;                  // this phase's K rounded up to 64: <= Kp
  const int nt = min(4, a.Op / 16 - 4 * (int)slice);               // N tiles of this slice: 1 .. 4, uniform over the block

  // this lane's pixel row of the A fragment, clamped: rows beyond M are computed, never stored
  {
    uint32_t jx, jy;
    const uint32_t b = hrd.divmod(wrd.divmod(min(m0 + (uint32_t)r, M - 1), jx), jy);
    p.qy = qy0 + (int32_t)jy; p.qx = qx0 + (int32_t)jx; p.image = (int64_t)b * a.H;
  }
  const uint32_t pad4 = (uint32_t)(a.za & 0xff) * 0x01010101u;
  // this lane's weight row of the B fragments: output channel 64 * slice + 16 * t + r of the phase, K block kb
  const int8_t* __restrict__ wrow = a.w + ((int64_t)phase * a.Op + 64 * (int64_t)slice + r) * a.Kp + 16 * kb;
  const int64_t wtile = 16 * (int64_t)a.Kp;

  i32x4 acc[4], rs = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

  // K steps of 64: the next step's fragments are in flight while this one multiplies.  A phase without taps loads nothing.
  i32x4 av = {0, 0, 0, 0}, wv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) wv[t] = i32x4{0, 0, 0, 0};
  if (kloop > 0) {
    av = transposed_a_chunk(a, p, 16u * kb, pad4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < nt) wv[t] = *reinterpret_cast<const i32x4*>(wrow + t * wtile);
  }
  for (int32_t k0 = 0; k0 < kloop; k0 += 64) {
    i32x4 av_next = av, wv_next[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wv_next[t] = wv[t];
    if (k0 + 64 < kloop) {
      av_next = transposed_a_chunk(a, p, (uint32_t)k0 + 64u + 16u * kb, pad4);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt) wv_next[t] = *reinterpret_cast<const i32x4*>(wrow + t * wtile + k0 + 64);
    }
    if constexpr (A_U8) av = av ^ (int)0x80808080;                  // u8 code c -> int8 (c - 128); za' carries the -128
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < nt) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, wv[t], acc[t], 0, 0, 0);
    if constexpr (ZP) rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, ones, rs, 0, 0, 0);     // every column: the row's sum of a'
    av = av_next;
#pragma unroll
    for (int t = 0; t < 4; ++t) wv[t] = wv_next[t];
  }

  // epilogue: column l & 15 of every tile, rows 4 * (l >> 4) + i, each at its own output pixel
  const int zap = A_U8 ? a.za - 128 : a.za;
  const unsigned tail = (unsigned)kloop * (unsigned)zap;            // what the kloop columns hold where a == za
  const uint32_t mrow = m0 + 4u * (uint32_t)kb;
  int64_t pixel[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t jx, jy;
    const uint32_t b = hrd.divmod(wrd.divmod(min(mrow + (uint32_t)i, M - 1), jx), jy);
    const int32_t oy = a.stride_h * (qy0 + (int32_t)jy) + (int32_t)ry - a.pad_h;           // 0 <= oy < Ho by the host's tables
    const int32_t ox = a.stride_w * (qx0 + (int32_t)jx) + (int32_t)rx - a.pad_w;
    pixel[i] = ((int64_t)b * a.Ho + oy) * a.Wo + ox;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      const int o = 64 * (int)slice + 16 * t + r;
      const int64_t n = min(o, a.O - 1);                            // columns beyond O: a valid channel, never stored
      const unsigned e_corr = (unsigned)zap * (unsigned)a.w_rowsum[(int64_t)phase * a.O + n];
      const float e_scale = a.sa * a.w_scales[n];
      const float e_bias = a.bias ? a.bias[n] : 0.0f;
      unsigned e_zw = 0;
      if constexpr (ZP) e_zw = (unsigned)a.w_zero_points[n];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned c = e_corr;
        if constexpr (ZP) c += e_zw * ((unsigned)rs[i] - tail);
        float out = (float)(int)((unsigned)acc[t][i] - c) * e_scale;
        if (a.bias) out = out + e_bias;
        if (mrow + (uint32_t)i < M && o < a.O) ql_store(a.y, pixel[i] * a.O + n, out, a.oq);
      }
    }
  }
}

// One axis of the phase decomposition: n inputs, kernel k, stride s <= 4, padding p, output_padding op -> the output extent,
// and per residue r < s the taps T(r), the first quotient q_lo(r) whose pixel s * q + r - p is inside the output, and the
// number of such pixels.  Every output pixel is counted in exactly one residue.
struct TransposedAxis {
  int64_t out;
  int32_t q_lo[kMaxStride], cnt[kMaxStride], taps[kMaxStride];
  int32_t max_cnt;
};
static void transposed_axis(TransposedAxis& t, int64_t n, int32_t k, int32_t s, int32_t p, int32_t op) {
  t.out = (n - 1) * s - 2 * (int64_t)p + k + op;
  t.max_cnt = 0;
  for (int r = 0; r < kMaxStride; ++r) {
    t.q_lo[r] = t.cnt[r] = t.taps[r] = 0;
    if (r >= s) continue;
    t.taps[r] = r < k ? (k - r + s - 1) / s : 0;
    if (t.out < 1) continue;
    const int64_t lo = p > r ? ((int64_t)p - r + s - 1) / s : 0, top = t.out - 1 + p - r;
    const int64_t hi = top >= 0 ? top / s : -1;
    t.q_lo[r] = (int32_t)lo;                                        // <= p
    t.cnt[r] = hi >= lo ? (int32_t)(hi - lo + 1) : 0;               // <= out
    if (t.cnt[r] > t.max_cnt) t.max_cnt = t.cnt[r];
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_qconv_transposed_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                             const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const int32_t* w_zero_points,
                             const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                             int32_t y_quant_min, int32_t y_quant_max, int64_t batch, int64_t height, int64_t width,
                             int64_t channels, int64_t out_channels, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w,
                             int32_t pad_h, int32_t pad_w, int32_t out_pad_h, int32_t out_pad_w, void* stream) {
  if (batch < 0 || height < 0 || width < 0 || channels < 0 || out_channels < 0) return fail_arg("negative extent");
  if (kh < 1 || kw < 1) return fail_arg("kernel size below 1");
  if (stride_h < 1 || stride_w < 1) return fail_arg("stride below 1");
  if (stride_h > kMaxStride || stride_w > kMaxStride) return fail_arg("stride above 4: outside the transposed consumer's limit");
  if (pad_h < 0 || pad_w < 0) return fail_arg("negative padding");
  if (out_pad_h < 0 || out_pad_w < 0) return fail_arg("negative output padding");
  if (out_pad_h >= stride_h || out_pad_w >= stride_w) return fail_arg("output padding must be smaller than the stride");
  if (channels == 0 || out_channels == 0) return fail_arg("channels and out_channels must be positive");
  if (channels % 16 != 0) return fail_arg("channels must be a multiple of 16");
  constexpr int64_t kMaxK = 1 << 15;
  const int64_t ty0 = ((int64_t)kh + stride_h - 1) / stride_h, tx0 = ((int64_t)kw + stride_w - 1) / stride_w;   // phase (0, 0) has the most taps
  if (ty0 > kMaxK || tx0 > kMaxK || channels > kMaxK || ty0 * tx0 * channels > kMaxK)
    return fail_arg("taps of a phase * channels > 32768: outside the consumer's limit");
  if (out_channels > INT32_MAX) return fail_arg("out_channels exceed 2^31 - 1");
  if (int rc = form_check_dtype(a_code_dtype, "a_code_dtype")) return rc;
  const bool u8 = a_code_dtype == MCTQ_CODE_U8;
  // the zero point is the byte a tap outside the image is given (it then adds (za - za) * (w - zw) = 0): it has to be a code
  if (int rc = form_check_zero_point(a_code_dtype, a_zero_point, "a_zero_point", "a_code_dtype")) return rc;
  TransposedArgs a;
  if (int rc = ql_output_form(a.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  if (height > INT32_MAX || width > INT32_MAX) return fail_arg("image extent exceeds 2^31 - 1");
  TransposedAxis ay, ax;
  transposed_axis(ay, height, kh, stride_h, pad_h, out_pad_h);      // |out| < 2^34: no overflow
  transposed_axis(ax, width, kw, stride_w, pad_w, out_pad_w);
  if (ay.out < 1 || ax.out < 1) return fail_arg("the padding leaves no output (Ho <= 0 or Wo <= 0)");
  // the kernel's quotients (oy + pad) / stride and its output coordinates stay within int32
  if (ay.out + pad_h > INT32_MAX || ax.out + pad_w > INT32_MAX) return fail_arg("padded output extent exceeds 2^31 - 1");
  if (batch == 0) return 0;                                                                          // nothing to write
  // (kernel and output padding alone could make an output of an image without pixels; the clamped loads need one)
  if (height == 0 || width == 0) return fail_arg("an image of a non-empty batch needs at least one pixel");
  if (batch > INT32_MAX / (ay.out * ax.out)) return fail_arg("too many output pixels for one launch");   // out * out < 2^62
  if (height * width > INT64_MAX / channels / batch) return fail_arg("the codes tensor exceeds 2^63 - 1 bytes");
  const int64_t pixels = batch * ay.out * ax.out;
  if (pixels > INT64_MAX / 4 / out_channels) return fail_arg("the output tensor exceeds 2^63 - 1 bytes");
  const int64_t phases = (int64_t)stride_h * stride_w;
  const int64_t kp = (ty0 * tx0 * channels + 63) / 64 * 64, op = (out_channels + 15) / 16 * 16, slices = (op + 63) / 64;
  if (phases * slices > 65535) return fail_arg("phases * ceil(out_channels / 64) > 65535: too many grid slices");
  if (!a_codes || !w_codes || !w_scales || !w_rowsum || !y) return fail_arg("NULL pointer");
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)w_scales | (uintptr_t)w_rowsum |
        (uintptr_t)w_zero_points | (uintptr_t)bias) & 15u) != 0)
    return fail_arg("codes, weights, per-channel tables and output must be 16-byte aligned");
  a.x = static_cast<const uint8_t*>(a_codes);
  a.w = w_codes; a.w_scales = w_scales; a.w_rowsum = w_rowsum; a.w_zero_points = w_zero_points; a.bias = bias; a.y = y;
  a.c = FastDiv::make((uint32_t)channels);
  a.slices = FastDiv::make((uint32_t)slices);
  for (int r = 0; r < kMaxStride; ++r) {
    a.hr[r] = FastDiv::make((uint32_t)(ay.cnt[r] > 0 ? ay.cnt[r] : 1));
    a.wr[r] = FastDiv::make((uint32_t)(ax.cnt[r] > 0 ? ax.cnt[r] : 1));
    a.tx[r] = FastDiv::make((uint32_t)(ax.taps[r] > 0 ? ax.taps[r] : 1));
    a.q_lo_y[r] = ay.q_lo[r]; a.cnt_y[r] = ay.cnt[r]; a.taps_y[r] = ay.taps[r];
    a.q_lo_x[r] = ax.q_lo[r]; a.cnt_x[r] = ax.cnt[r]; a.taps_x[r] = ax.taps[r];
  }
  a.B = (int32_t)batch; a.H = (int32_t)height; a.W = (int32_t)width; a.C = (int32_t)channels; a.O = (int32_t)out_channels;
  a.Op = (int32_t)op; a.Kp = (int32_t)kp; a.Ho = (int32_t)ay.out; a.Wo = (int32_t)ax.out;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w;
  a.za = a_zero_point; a.sa = a_scale;
  const int64_t max_m = batch * ay.max_cnt * ax.max_cnt;                                              // <= pixels
  const dim3 grid((unsigned)((max_m + 63) / 64), (unsigned)(phases * slices));                        // x <= 2^25, y <= 65535
  const hipStream_t s = (hipStream_t)stream;
  const bool zp = w_zero_points != nullptr;
  if (u8) {
    if (zp) hipLaunchKernelGGL((qconv_transposed_kernel<true, true>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((qconv_transposed_kernel<true, false>), grid, dim3(kThreads), 0, s, a);
  } else {
    if (zp) hipLaunchKernelGGL((qconv_transposed_kernel<false, true>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((qconv_transposed_kernel<false, false>), grid, dim3(kThreads), 0, s, a);
  }
  note_launch("qconv_transposed", zp ? (u8 ? "u8 x i8 zp" : "i8 x i8 zp") : (u8 ? "u8 x i8" : "i8 x i8"), (int)phases, 0, 1,
              a.oq.mode == 0 ? 4 : 1);
  return check_launch("mctq_qconv_transposed_i8");
}

}  // extern "C"
