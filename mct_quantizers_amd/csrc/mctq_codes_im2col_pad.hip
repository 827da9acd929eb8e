// mctq_codes_im2col_pad.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Patch matrix of NHWC activation codes for ANY channel count: codes [B][H][W][C] (1 byte each, C >= 1) -> patches
// [B * Ho * Wo][Kp], K = kh * kw * C, Kp = 16 * ceil(K / 16).  Column k < K is mctq_codes_im2col_nhwc's: row m = (b, oy, ox),
// column (ky * kw + kx) * C + c, a tap outside the image holds the pad byte; columns K .. Kp - 1 hold the pad byte too.  With
// the pad byte the activation's zero-point code za and weight rows padded with the code 0, the integer product over Kp columns
// is the product over K columns exactly: a padded column adds qa * 0 to the sum, 0 to w_rowsum and (za - za) to the row sums
// of mctq_codes_rowsum (docs/KERNEL_NOTES.md).
//
// The shape of mctq_codes_im2col.hip is kept: a block takes a run of whole output rows, consecutive lanes consecutive 16-byte
// chunks of them, one 16-byte store per lane (full lines, plain stores).  What changes is the load side: with C % 16 != 0 a
// chunk is no longer one aligned chunk of the input, so a lane assembles it from 16 / G pieces of G bytes:
//   G = 4  where C % 4 == 0.  Then K % 4 == 0 and every tap starts at a multiple of 4 within the row, so a piece never
//          straddles two taps or the row's end; every pixel starts at a multiple of 4 bytes of the (16-byte aligned) input,
//          so a piece is one aligned dword load.
//   G = 1  byte loads, for every other C.
// Index arithmetic: m -> (b, oy, ox) and the first piece's (tap, c) once per lane by FastDiv; from there the pieces are walked
// by incrementing c and wrapping into the next tap.  No division per piece.  Every load address is formed from coordinates
// clamped into the image (the depthwise kernel's rule), whatever the tap: a piece of a tap outside the image, or of the tail
// behind column K, is loaded from a valid address and replaced by pad bytes by select.  No load reads outside `codes`.
// No LDS, no scratch, no atomics; every output byte is written by exactly one lane.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, WindowGeom

#ifndef MCTQ_IM2COL_PAD_BLOCK_CHUNKS
#define MCTQ_IM2COL_PAD_BLOCK_CHUNKS 256     // chunks a block takes, rounded up to whole rows (mctq_codes_im2col.hip's measured value)
#endif

namespace mctq {

extern int g_im2col_grain;                 // tuning key "im2col_grain" (mctq_misc.hip): 0 = by rule, 1 = bytes, 4 = dwords

struct Im2colPadArgs {
  const uint8_t* x;
  uint8_t* y;
  FastDiv row_chunks, chan, kw, wo, ho;            // chunks per output row (Kp / 16), C, kw, Wo, Ho
  uint32_t rows, rows_per_block;                   // M = B * Ho * Wo
  int32_t H, W, C, kh, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  uint32_t pad4;                                   // the pad byte in all four bytes
};

template <int G> struct Piece;
template <> struct Piece<4> { typedef uint32_t type; };
template <> struct Piece<1> { typedef uint8_t type; };

template <int G>
__global__ __launch_bounds__(kThreads) void codes_im2col_pad_kernel(Im2colPadArgs a) {
  typedef typename Piece<G>::type piece_t;
  constexpr int P = 16 / G;                        // pieces per chunk
  const uint32_t m0 = blockIdx.x * a.rows_per_block;
  const uint32_t live_rows = min(a.rows_per_block, a.rows - m0);                 // the last block may be partly empty
  const uint32_t chunks = live_rows * a.row_chunks.d;
  u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(a.y) + (int64_t)m0 * a.row_chunks.d;
  const int32_t C = a.C, kwi = (int32_t)a.kw.d;
  for (uint32_t i = threadIdx.x; i < chunks; i += kThreads) {
    uint32_t j, cu, kxu, ox, oy;
    const uint32_t m = m0 + a.row_chunks.divmod(i, j);
    const uint32_t tap = a.chan.divmod(j * 16u, cu);                             // the first piece: column j * 16 < K
    int32_t ky = (int32_t)a.kw.divmod(tap, kxu);
    const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);
    int32_t c = (int32_t)cu, kx = (int32_t)kxu;
    const int32_t ix0 = (int32_t)ox * a.stride_w - a.pad_w;
    int32_t iy = (int32_t)oy * a.stride_h + ky * a.dil_h - a.pad_h;
    int32_t ix = ix0 + kx * a.dil_w;
    const int64_t image = (int64_t)b * a.H;
    piece_t v[P];
    bool live[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      // a valid address whatever the tap: b < B, 0 <= cy < H, 0 <= cx < W, c + G <= C
      const int32_t cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
      live[p] = ky < a.kh && (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;     // ky == kh: the tail behind column K
      v[p] = *reinterpret_cast<const piece_t*>(a.x + (((image + cy) * a.W + cx) * C + c));
      c += G;
      if (c == C) {                                // the next tap; behind the last one (ky == kh) iy stays where it is
        c = 0; ++kx; ix += a.dil_w;
        if (kx == kwi) { kx = 0; ix = ix0; ++ky; iy = ky < a.kh ? iy + a.dil_h : iy; }
      }
    }
    u32x4 out;
    if constexpr (G == 4) {
#pragma unroll
      for (int p = 0; p < 4; ++p) out[p] = live[p] ? v[p] : a.pad4;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) w |= (live[4 * q + t] ? (uint32_t)v[4 * q + t] : (a.pad4 & 0xffu)) << (8 * t);
        out[q] = w;
      }
    }
    dst[i] = out;
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_im2col_pad_nhwc(const void* codes, void* patches, int64_t batch, int64_t height, int64_t width, int64_t channels,
                               int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                               int32_t dil_h, int32_t dil_w, int32_t pad_code, void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
  if (int rc = geom_check_sizes(g, false)) return rc;
  if (pad_code < -128 || pad_code > 255) return fail_arg("pad_code outside [-128, 255]");
  constexpr int64_t kMaxK = 1 << 15;
  if (kh > kMaxK || kw > kMaxK || channels > kMaxK || (int64_t)kh * kw * channels > kMaxK)
    return fail_arg("kh * kw * channels > 32768: outside the consumer's limit");                      // Kp <= 32768 with it
  const int grain = g_im2col_grain ? g_im2col_grain : (channels % 4 == 0 ? 4 : 1);
  if (grain == 4 && channels % 4 != 0) return fail_arg("im2col_grain 4 needs channels % 4 == 0");
  if (int rc = geom_check_fit(g, false)) return rc;
  const int64_t ho = g.ho, wo = g.wo;
  if (batch == 0 || channels == 0) return 0;                                                         // nothing to write
  // (padding alone could make room for a kernel on an image without pixels; the clamped loads need one)
  if (height == 0 || width == 0) return fail_arg("an image of a non-empty batch needs at least one pixel");
  if (batch > INT32_MAX / (ho * wo)) return fail_arg("too many output rows for one launch");       // ho * wo < 2^62
  if (height * width > INT64_MAX / channels / batch) return fail_arg("the codes tensor exceeds 2^63 - 1 bytes");
  const int64_t rows = batch * ho * wo, row_chunks = ((int64_t)kh * kw * channels + 15) / 16;
  if (!codes || !patches) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)patches)) & 15u) != 0) return fail_arg("codes and patches must be 16-byte aligned");
  const int64_t rows_per_block = (MCTQ_IM2COL_PAD_BLOCK_CHUNKS + row_chunks - 1) / row_chunks;        // whole rows, at least one
  Im2colPadArgs a;
  a.x = static_cast<const uint8_t*>(codes);
  a.y = static_cast<uint8_t*>(patches);
  a.row_chunks = FastDiv::make((uint32_t)row_chunks);
  a.chan = FastDiv::make((uint32_t)channels);
  a.kw = FastDiv::make((uint32_t)kw);
  a.wo = FastDiv::make((uint32_t)wo);
  a.ho = FastDiv::make((uint32_t)ho);
  a.rows = (uint32_t)rows;
  a.rows_per_block = (uint32_t)rows_per_block;
  a.H = (int32_t)height; a.W = (int32_t)width; a.C = (int32_t)channels; a.kh = kh;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.pad4 = (uint32_t)(pad_code & 0xFF) * 0x01010101u;
  const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;                                // <= rows < 2^31
  if (grain == 4) {
    hipLaunchKernelGGL(codes_im2col_pad_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    note_launch("codes_im2col_pad", "padded gather G=4", 1, 0, 1, 1);
  } else {
    hipLaunchKernelGGL(codes_im2col_pad_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    note_launch("codes_im2col_pad", "padded gather G=1", 1, 0, 1, 1);
  }
  return check_launch("mctq_codes_im2col_pad_nhwc");
}

}  // extern "C"
