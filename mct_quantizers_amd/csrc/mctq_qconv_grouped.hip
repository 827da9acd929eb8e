// mctq_qconv_grouped.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Grouped convolution on the quantizers' codes (2 <= groups, Cg = C / G input and Og = O / G output channels per group,
// Cg % 4 == 0): the 3 x 3 layer of a ResNeXt / RegNet bottleneck, ShuffleNet's grouped 1 x 1 layers.  It is G small matrix
// products, so it runs on the integer matrix cores (v_mfma_i32_16x16x64_i8) like the ungrouped product, but as a direct
// convolution on the NHWC codes like the depthwise one: no patch matrix, one launch for all groups.
//     acc[b][oy][ox][n] = sum over taps (ky, kx) inside the image, cg < Cg of
//                         (a[b][iy][ix][g * Cg + cg] - za) * (w[n][cg][ky][kx] - zw[n])            n = g * Og + o
//     y = float(acc) * (sa * sw[n]) (+ bias[n])
// with the epilogue of mctq_qlinear_i8 (one rounding per float32 operation; -ffp-contract=off) and its output forms (QlOut).
//
// Wave tile: 16 consecutive output pixels (rows) x up to 4 N tiles of 16 output channels of one group.  K order inside a
// group is (ky, kx, cg): the group's channels of one tap are contiguous in NHWC.  Per K step of 64 the A fragment of lane l
// is the 16 bytes k = 16 * (l >> 4) .. + 15 of pixel row l & 15, the B fragment the same bytes of output channel l & 15;
// in the result the column is l & 15 and the row 4 * (l >> 4) + reg (mctq_qlinear.hip).  Weights: the host keeps them as
// [G][Ogp][Kgp] int8, Ogp = 16 * ceil(Og / 16), Kgp = 64 * ceil(Kg / 64), padded rows and columns the code 0: every weight
// load is an unguarded aligned 16-byte load.
//
// A chunk: assembled from 16 / P pieces of P bytes, P = 16 where Cg % 16 == 0, else 8 where Cg % 8 == 0, else 4.  Cg % P == 0
// and K offsets are multiples of P, so a piece never straddles a tap and is one aligned load (the image is 16-byte aligned
// and C = G * Cg, g * Cg and cg are multiples of P).  The chunk's first (tap, cg) comes from two FastDiv divisions; from
// there the pieces are walked as codes_im2col_pad_kernel walks them: increment cg, wrap into the next tap.  Every address
// is formed from coordinates clamped into the image; a piece of a tap outside the image, or of the tail behind Kg, is loaded
// from a valid address and replaced by zero-point bytes by select: it adds (za - za) * (w - zw) = 0 (a tail piece stands
// against weight zeros as well).  No load reads outside a_codes.  uint8 codes are xor-ed with 0x80 into int8 (za' = za - 128),
// as in mctq_qlinear.hip, and the sum is corrected by za' * w_rowsum[n].
//
// Weight zero points: zw[n] * sum_k (a - za) needs the activation row sum of each (pixel, group).  It is one more MFMA per K
// step against a B fragment of ones held in registers: S[row] = sum over all Kgp columns of a', the same value in every
// column of the result tile, so every lane finds the sums of its four rows in its own registers -- no spare weight column
// (which a second grid slice over N would not see), no cross-lane reduction, no memory traffic.  Padded taps and the tail hold
// za', so sum_k (a - za) = S - Kgp * za' exactly.  All terms are added in wrapping arithmetic (ql_corrected's rule): each
// reaches 2^30 and only their total, |sum| <= 255 * 255 * 32768 < 2^31, is known to fit.
//
// Block: 256 threads = 4 waves = 64 pixels of the same group and N slice.  Grid x = ceil(M / 64), M = B * Ho * Wo; grid
// y = G * ceil(Ogp / 64).  No LDS, no atomics, no split-K: every output element is written by exactly one lane.  Rows beyond M
// and columns beyond Og are computed from clamped indices and not stored.
#include "mctq_consumer.hpp"

namespace mctq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct GroupedArgs {
  const uint8_t* x;
  const int8_t* w;                                 // [G][Ogp][Kgp]
  const float* w_scales;
  const int32_t* w_rowsum;
  const int32_t* w_zero_points;
  const float* bias;
  void* y;
  FastDiv wo, ho, cg, kw, slices;                  // Wo, Ho, Cg, kw, N slices per group (ceil(Ogp / 64))
  uint32_t M;                                      // B * Ho * Wo
  int32_t H, W, C, O, Og, Ogp, Kgp, kh, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t za;                                      // the zero point as a code; the kernel subtracts 128 for uint8 codes
  float sa;
  QlOut oq;
};

template <int P> struct GroupedPiece;
template <> struct GroupedPiece<16> { typedef u32x4 type; };
template <> struct GroupedPiece<8> { typedef u32x2 type; };
template <> struct GroupedPiece<4> { typedef uint32_t type; };

// The 16 bytes k .. k + 15 (k % 16 == 0, k < Kgp) of one pixel row's K axis: gx = the image batch's codes + g * Cg, image =
// b * H, (iy0, ix0) the window's corner.  Pieces outside the image or behind Kg (ky >= kh) hold the pad byte.
template <int P>
__device__ __forceinline__ i32x4 grouped_a_chunk(const GroupedArgs& a, const uint8_t* __restrict__ gx, int64_t image, int iy0,
                                                 int ix0, uint32_t k, uint32_t pad4) {
  typedef typename GroupedPiece<P>::type piece_t;
  constexpr int N = 16 / P;
  const int32_t Cg = (int32_t)a.cg.d, kwi = (int32_t)a.kw.d;
  uint32_t cgu, kxu;
  const uint32_t tap = a.cg.divmod(k, cgu);
  int32_t ky = (int32_t)a.kw.divmod(tap, kxu);
  int32_t kx = (int32_t)kxu, cg = (int32_t)cgu;
  int32_t iy = iy0 + min(ky, a.kh - 1) * a.dil_h;                  // behind the last tap (ky >= kh) iy stays inside int32
  int32_t ix = ix0 + kx * a.dil_w;
  piece_t v[N];
  bool live[N];
#pragma unroll
  for (int p = 0; p < N; ++p) {
    // a valid address whatever the tap: 0 <= cy < H, 0 <= cx < W, cg + P <= Cg
    const int32_t cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
    live[p] = ky < a.kh && (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
    v[p] = *reinterpret_cast<const piece_t*>(gx + (((image + cy) * a.W + cx) * (int64_t)a.C + cg));
    if constexpr (N > 1) {
      cg += P;
      if (cg == Cg) {                              // the next tap; behind the last one iy stays where it is
        cg = 0; ++kx; ix += a.dil_w;
        if (kx == kwi) { kx = 0; ix = ix0; ++ky; iy = ky < a.kh ? iy + a.dil_h : iy; }
      }
    }
  }
  i32x4 out;
  if constexpr (P == 16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = (int)(live[0] ? v[0][q] : pad4);
  } else if constexpr (P == 8) {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = (int)(live[q >> 1] ? v[q >> 1][q & 1] : pad4);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = (int)(live[q] ? v[q] : pad4);
  }
  return out;
}

template <bool A_U8, bool ZP, int P>
__global__ __launch_bounds__(kThreads) void qconv_grouped_kernel(GroupedArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kb = lane >> 4;
  const uint32_t m0 = blockIdx.x * 64u + (uint32_t)wave * 16u;      // < M + 64 <= 2^31 + 63
  if (m0 >= a.M) return;                                            // an idle wave of the last block (no barrier below)
  uint32_t slice;
  const uint32_t g = a.slices.divmod(blockIdx.y, slice);
  const int32_t Cg = (int32_t)a.cg.d;
  const int nt = min(4, a.Ogp / 16 - 4 * (int)slice);              // N tiles of this slice: 1 .. 4, uniform over the block

  // this lane's pixel row of the A fragment, clamped: rows beyond M are computed, never stored
  uint32_t ox, oy;
  const uint32_t b = a.ho.divmod(a.wo.divmod(min(m0 + (uint32_t)r, a.M - 1), ox), oy);
  const int iy0 = (int)oy * a.stride_h - a.pad_h, ix0 = (int)ox * a.stride_w - a.pad_w;
  const int64_t image = (int64_t)b * a.H;
  const uint8_t* __restrict__ gx = a.x + (int64_t)g * Cg;
  const uint32_t pad4 = (uint32_t)(a.za & 0xff) * 0x01010101u;
  // this lane's weight row of the B fragments: output channel 64 * slice + 16 * t + r of the group, K block kb
  const int8_t* __restrict__ wrow = a.w + ((int64_t)g * a.Ogp + 64 * (int64_t)slice + r) * a.Kgp + 16 * kb;
  const int64_t wtile = 16 * (int64_t)a.Kgp;

  i32x4 acc[4], rs = {0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

  // K steps of 64: the next step's fragments are in flight while this one multiplies
  i32x4 av = grouped_a_chunk<P>(a, gx, image, iy0, ix0, 16u * kb, pad4), wv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) wv[t] = t < nt ? *reinterpret_cast<const i32x4*>(wrow + t * wtile) : i32x4{0, 0, 0, 0};
  for (int32_t k0 = 0; k0 < a.Kgp; k0 += 64) {
    i32x4 av_next = av, wv_next[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wv_next[t] = wv[t];
    if (k0 + 64 < a.Kgp) {
      av_next = grouped_a_chunk<P>(a, gx, image, iy0, ix0, (uint32_t)k0 + 64u + 16u * kb, pad4);
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

  // epilogue: column l & 15 of every tile, rows 4 * (l >> 4) + i
  const int zap = A_U8 ? a.za - 128 : a.za;
  const unsigned tail = (unsigned)a.Kgp * (unsigned)zap;            // what the Kgp columns hold where a == za
  const uint32_t mrow = m0 + 4u * (uint32_t)kb;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      const int o = 64 * (int)slice + 16 * t + r;
      const int64_t n = (int64_t)g * a.Og + min(o, a.Og - 1);       // columns beyond Og: a valid channel, never stored
      const unsigned e_corr = (unsigned)zap * (unsigned)a.w_rowsum[n];
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
        const uint32_t m = mrow + (uint32_t)i;
        if (m < a.M && o < a.Og) ql_store(a.y, (int64_t)m * a.O + n, out, a.oq);
      }
    }
  }
}

template <bool A_U8, bool ZP>
static void launch_qconv_grouped(const GroupedArgs& a, int piece, dim3 grid, hipStream_t stream) {
  if (piece == 16) hipLaunchKernelGGL((qconv_grouped_kernel<A_U8, ZP, 16>), grid, dim3(kThreads), 0, stream, a);
  else if (piece == 8) hipLaunchKernelGGL((qconv_grouped_kernel<A_U8, ZP, 8>), grid, dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL((qconv_grouped_kernel<A_U8, ZP, 4>), grid, dim3(kThreads), 0, stream, a);
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_qconv_grouped_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                          const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const int32_t* w_zero_points,
                          const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                          int32_t y_quant_min, int32_t y_quant_max, int64_t batch, int64_t height, int64_t width,
                          int64_t channels, int64_t out_channels, int32_t groups, int32_t kh, int32_t kw, int32_t stride_h,
                          int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t dil_h, int32_t dil_w, void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
  if (int rc = geom_check_sizes(g, false)) return rc;
  if (out_channels < 0) return fail_arg("negative extent");
  if (groups < 2) return fail_arg("groups below 2: the grouped consumer takes grouped convolutions only");
  if (channels % groups != 0 || out_channels % groups != 0 || channels == 0 || out_channels == 0)
    return fail_arg("channels and out_channels must be positive multiples of groups");
  const int64_t cg = channels / groups, og = out_channels / groups;
  if (cg % 4 != 0) return fail_arg("channels per group must be a multiple of 4");
  constexpr int64_t kMaxK = 1 << 15;
  if (kh > kMaxK || kw > kMaxK || cg > kMaxK || (int64_t)kh * kw * cg > kMaxK)
    return fail_arg("kh * kw * channels per group > 32768: outside the consumer's limit");
  if (channels > INT32_MAX || out_channels > INT32_MAX) return fail_arg("channels or out_channels exceed 2^31 - 1");
  if (int rc = form_check_dtype(a_code_dtype, "a_code_dtype")) return rc;
  const bool u8 = a_code_dtype == MCTQ_CODE_U8;
  // the zero point is the byte a padded tap is given (it then adds (za - za) * (w - zw) = 0): it has to be a code
  if (int rc = form_check_zero_point(a_code_dtype, a_zero_point, "a_zero_point", "a_code_dtype")) return rc;
  GroupedArgs a;
  if (int rc = ql_output_form(a.oq, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  if (int rc = geom_check_fit(g, false)) return rc;
  if (batch == 0) return 0;                                                                          // nothing to write
  // (padding alone could make room for a kernel on an image without pixels; the clamped loads need one)
  if (height == 0 || width == 0) return fail_arg("an image of a non-empty batch needs at least one pixel");
  if (batch > INT32_MAX / (g.ho * g.wo)) return fail_arg("too many output pixels for one launch");   // ho * wo < 2^62
  if (height * width > INT64_MAX / channels / batch) return fail_arg("the codes tensor exceeds 2^63 - 1 bytes");
  const int64_t kg = (int64_t)kh * kw * cg, kgp = (kg + 63) / 64 * 64, ogp = (og + 15) / 16 * 16, slices = (ogp + 63) / 64;
  if (groups * slices > 65535) return fail_arg("groups * ceil(out_channels per group / 64) > 65535: too many grid slices");
  if (!a_codes || !w_codes || !w_scales || !w_rowsum || !y) return fail_arg("NULL pointer");
  if ((((uintptr_t)a_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)w_scales | (uintptr_t)w_rowsum |
        (uintptr_t)w_zero_points | (uintptr_t)bias) & 15u) != 0)
    return fail_arg("codes, weights, per-channel tables and output must be 16-byte aligned");
  const int64_t pixels = batch * g.ho * g.wo;
  a.x = static_cast<const uint8_t*>(a_codes);
  a.w = w_codes; a.w_scales = w_scales; a.w_rowsum = w_rowsum; a.w_zero_points = w_zero_points; a.bias = bias; a.y = y;
  a.wo = FastDiv::make((uint32_t)g.wo);
  a.ho = FastDiv::make((uint32_t)g.ho);
  a.cg = FastDiv::make((uint32_t)cg);
  a.kw = FastDiv::make((uint32_t)kw);
  a.slices = FastDiv::make((uint32_t)slices);
  a.M = (uint32_t)pixels;
  a.H = (int32_t)height; a.W = (int32_t)width; a.C = (int32_t)channels; a.O = (int32_t)out_channels;
  a.Og = (int32_t)og; a.Ogp = (int32_t)ogp; a.Kgp = (int32_t)kgp; a.kh = kh;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.za = a_zero_point; a.sa = a_scale;
  const int piece = cg % 16 == 0 ? 16 : cg % 8 == 0 ? 8 : 4;
  const dim3 grid((unsigned)((pixels + 63) / 64), (unsigned)(groups * slices));                       // x <= 2^25, y <= 65535
  const hipStream_t s = (hipStream_t)stream;
  const bool zp = w_zero_points != nullptr;
  if (u8) { if (zp) launch_qconv_grouped<true, true>(a, piece, grid, s); else launch_qconv_grouped<true, false>(a, piece, grid, s); }
  else { if (zp) launch_qconv_grouped<false, true>(a, piece, grid, s); else launch_qconv_grouped<false, false>(a, piece, grid, s); }
  note_launch("qconv_grouped", zp ? (u8 ? "u8 x i8 zp" : "i8 x i8 zp") : (u8 ? "u8 x i8" : "i8 x i8"), piece, 0, 1,
              a.oq.mode == 0 ? 4 : 1);
  return check_launch("mctq_qconv_grouped_i8");
}

}  // extern "C"
