// mctq_codes_im2col.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Patch matrix of NHWC activation codes for the integer consumer: codes [B][H][W][C] (1 byte each) -> patches
// [B * Ho * Wo][kh * kw * C], row m = (b, oy, ox), column k = (ky * kw + kx) * C + c; a tap outside the image holds the
// pad byte (the activation's zero-point code, so that it contributes (za - za) * qw = 0 to the product).  A pure byte
// gather: with C % 16 == 0 every 16-byte chunk of an output row is one aligned 16-byte chunk of the input or 16 pad
// bytes, so a lane moves one chunk with one 16-byte load and one 16-byte store.  A block takes a run of whole output
// rows; its chunks are consecutive in memory, consecutive lanes on consecutive chunks.  The input is re-read up to
// kh * kw times (out of L2: plain loads), the output is written once.
//
// Index arithmetic per CHUNK, never per byte: five divisions by launch constants (chunks per row, chunks per tap, kw,
// Wo, Ho), each a multiply-high by a host-computed reciprocal and one correction step.
#include "mctq_consumer.hpp"               // FastDiv, u32x4

// timing experiment (tools/conv_consumer_probe.py --im2col-only): 1 = non-temporal stores of the patch matrix
#ifndef MCTQ_IM2COL_NT
#define MCTQ_IM2COL_NT 0
#endif
// ... and the chunks a block takes, rounded up to whole rows.  Measured (same probe, profiles/EXPERIMENTS.md): one chunk per
// lane is as fast as or faster than eight on every ResNet-50 shape at batch 64; at batch 1 every form is at the launch floor
#ifndef MCTQ_IM2COL_BLOCK_CHUNKS
#define MCTQ_IM2COL_BLOCK_CHUNKS 256
#endif

namespace mctq {

struct Im2colArgs {
  const uint8_t* x;
  uint8_t* y;
  FastDiv row_chunks, tap_chunks, kw, wo, ho;      // chunks per output row, chunks per tap (C / 16), kw, Wo, Ho
  uint32_t rows, rows_per_block;                   // M = B * Ho * Wo
  int32_t H, W, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  uint32_t pad4;                                   // the pad byte in all four bytes
};

__global__ __launch_bounds__(kThreads) void codes_im2col_kernel(Im2colArgs a) {
  const uint32_t m0 = blockIdx.x * a.rows_per_block;
  const uint32_t live_rows = min(a.rows_per_block, a.rows - m0);                 // the last block may be partly empty
  const uint32_t chunks = live_rows * a.row_chunks.d;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.x);
  u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(a.y) + (int64_t)m0 * a.row_chunks.d;
  const int64_t c16 = a.tap_chunks.d;
  for (uint32_t i = threadIdx.x; i < chunks; i += kThreads) {
    uint32_t j, cc, kx, ox, oy;
    const uint32_t m = m0 + a.row_chunks.divmod(i, j);
    const uint32_t tap = a.tap_chunks.divmod(j, cc);
    const uint32_t ky = a.kw.divmod(tap, kx);
    const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);
    const int32_t iy = (int32_t)oy * a.stride_h + (int32_t)ky * a.dil_h - a.pad_h;
    const int32_t ix = (int32_t)ox * a.stride_w + (int32_t)kx * a.dil_w - a.pad_w;
    u32x4 v = {a.pad4, a.pad4, a.pad4, a.pad4};
    if ((uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W)
      v = src[(((int64_t)b * a.H + iy) * a.W + ix) * c16 + cc];
#if MCTQ_IM2COL_NT
    __builtin_nontemporal_store(v, dst + i);
#else
    dst[i] = v;
#endif
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_im2col_nhwc(const void* codes, void* patches, int64_t batch, int64_t height, int64_t width, int64_t channels,
                           int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                           int32_t dil_h, int32_t dil_w, int32_t pad_code, void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
  if (int rc = geom_check_sizes(g, false)) return rc;
  if (pad_code < -128 || pad_code > 255) return fail_arg("pad_code outside [-128, 255]");
  if (int rc = geom_check_channels(g)) return rc;
  constexpr int64_t kMaxK = 1 << 15;
  if (kh > kMaxK || kw > kMaxK || channels > kMaxK || (int64_t)kh * kw * channels > kMaxK)
    return fail_arg("kh * kw * channels > 32768: outside the consumer's limit");
  if (int rc = geom_check_fit(g, false)) return rc;
  const int64_t ho = g.ho, wo = g.wo;
  if (batch == 0) return 0;
  if (batch > INT32_MAX / (ho * wo)) return fail_arg("too many output rows for one launch");       // ho * wo < 2^62
  const int64_t rows = batch * ho * wo, row_chunks = (int64_t)kh * kw * channels / 16;
  if (row_chunks == 0) return 0;                                                                     // no channels: nothing to write
  if (!codes || !patches) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)patches)) & 15u) != 0) return fail_arg("codes and patches must be 16-byte aligned");
  const int64_t rows_per_block = (MCTQ_IM2COL_BLOCK_CHUNKS + row_chunks - 1) / row_chunks;            // whole rows, at least one
  Im2colArgs a;
  a.x = static_cast<const uint8_t*>(codes);
  a.y = static_cast<uint8_t*>(patches);
  a.row_chunks = FastDiv::make((uint32_t)row_chunks);
  a.tap_chunks = FastDiv::make((uint32_t)(channels / 16));
  a.kw = FastDiv::make((uint32_t)kw);
  a.wo = FastDiv::make((uint32_t)wo);
  a.ho = FastDiv::make((uint32_t)ho);
  a.rows = (uint32_t)rows;
  a.rows_per_block = (uint32_t)rows_per_block;
  a.H = (int32_t)height; a.W = (int32_t)width;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.pad4 = (uint32_t)(pad_code & 0xFF) * 0x01010101u;
  const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;                                // <= rows < 2^31
  hipLaunchKernelGGL(codes_im2col_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  note_launch("codes_im2col", "byte gather", 1, MCTQ_IM2COL_NT, 1, 1);
  return check_launch("mctq_codes_im2col_nhwc");
}

}  // extern "C"
