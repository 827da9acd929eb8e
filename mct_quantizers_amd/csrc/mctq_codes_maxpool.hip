// mctq_codes_maxpool.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Max pooling on NHWC activation codes: codes [B][H][W][C] (1 byte each, int8 or uint8) -> pooled [B][Ho][Wo][C] of the
// same type, torch.nn.MaxPool2d's semantics (kernel, stride, padding, dilation, ceil_mode).  A holder's float32 output is
// float(code - zp) * scale with scale > 0: monotone non-decreasing in the code and never NaN, so the maximum of the
// dequantized values is the dequantized maximum of the codes, bit for bit -- nothing is approximated.
//
// Form: that of mctq_qconv_dw.hip without the weights.  A lane owns one 16-byte chunk (16 channels) of one output pixel,
// consecutive lanes on consecutive chunks of a pixel and then on consecutive pixels, so that the loads of a tap and the
// store are coalesced over the wave; per tap one 16-byte load (plain: the input is re-read about kh * kw / (sh * sw) times
// out of cache), at the end one 16-byte store.  Index arithmetic per chunk: three divisions by launch constants (FastDiv).
//
// One unsigned byte-maximum serves both code types: signed order is unsigned order after flipping bit 7 of every byte, so
// int8 codes are XORed with 0x80808080 after each load and before the store.  The sixteen running maxima are kept as
// sixteen 16-bit lanes (even and odd bytes of each dword apart), which v_pk_max_u16 takes two at a time.
//
// Padding: a tap outside the image stands for -inf, not for the zero-point code.  It is loaded from a clamped (valid)
// address and then replaced by 0, the least code of the flipped domain, which is also what the maxima start from: the
// loads do not depend on a branch.  Every window of a geometry PyTorch accepts has a tap inside the image unless the
// image is narrower than the dilation; such a window then gives the least code of the type (0 / -128), which is what
// ATen's integer max pool gives too.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, WindowGeom

// timing experiment (tools/pool_consumer_probe.py, section forms): 1 = 2 x 2 and 3 x 3 kernels run an instance whose tap
// loops are unrolled at compile time (all loads of a lane in flight at once); 0 (shipped): the run-time loops for every size
#ifndef MCTQ_POOL_UNROLL
#define MCTQ_POOL_UNROLL 0
#endif

namespace mctq {

struct PoolArgs {
  const uint8_t* x;
  uint8_t* y;
  FastDiv c16, wo, ho;                             // chunks per pixel (C / 16), Wo, Ho
  uint32_t chunks;                                 // B * Ho * Wo * C / 16
  int32_t H, W, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  uint32_t flip;                                   // 0x80808080 for int8 codes, 0 for uint8
};

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// KK > 0: a KK x KK kernel known at compile time (a.kh == a.kw == KK); KK == 0: a.kh x a.kw
template <int KK>
__global__ __launch_bounds__(kThreads) void codes_maxpool_kernel(PoolArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^32: the launcher checks the chunk count
  if (g >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t cc, ox, oy;
  const uint32_t m = a.c16.divmod(g, cc);
  const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);
  const int64_t c16 = a.c16.d;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.x) + (int64_t)b * a.H * a.W * c16 + cc;
  const int iy0 = (int)oy * a.stride_h - a.pad_h, ix0 = (int)ox * a.stride_w - a.pad_w;

  u16x2 even[4], odd[4];                           // bytes 0 and 2 / 1 and 3 of each dword, zero-extended
#pragma unroll
  for (int q = 0; q < 4; ++q) even[q] = odd[q] = u16x2{0, 0};

  auto tap = [&](int ky, int kx) {
    const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
    const bool inside = (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
    const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);         // a valid address whatever the tap
    const u32x4 v = src[((int64_t)cy * a.W + cx) * c16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t u = inside ? v[q] ^ a.flip : 0u;
      even[q] = __builtin_elementwise_max(even[q], __builtin_bit_cast(u16x2, u & 0x00ff00ffu));
      odd[q] = __builtin_elementwise_max(odd[q], __builtin_bit_cast(u16x2, (u >> 8) & 0x00ff00ffu));
    }
  };
  if constexpr (KK > 0) {
#pragma unroll
    for (int ky = 0; ky < KK; ++ky) {
#pragma unroll
      for (int kx = 0; kx < KK; ++kx) tap(ky, kx);
    }
  } else {
    for (int ky = 0; ky < a.kh; ++ky)
      for (int kx = 0; kx < a.kw; ++kx) tap(ky, kx);
  }

  u32x4 out;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    out[q] = (__builtin_bit_cast(uint32_t, even[q]) | (__builtin_bit_cast(uint32_t, odd[q]) << 8)) ^ a.flip;
  reinterpret_cast<u32x4*>(a.y)[g] = out;
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_maxpool_nhwc(const void* codes, void* pooled, int32_t code_dtype, int64_t batch, int64_t height, int64_t width,
                            int64_t channels, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h,
                            int32_t pad_w, int32_t dil_h, int32_t dil_w, int32_t ceil_mode, int64_t out_height, int64_t out_width,
                            void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w};
  if (int rc = geom_check_sizes(g, true)) return rc;
  if (int rc = geom_check_channels(g)) return rc;
  if (int rc = form_check_dtype(code_dtype, "code_dtype")) return rc;
  if (int rc = geom_check_fit(g, true)) return rc;
  if (int rc = geom_check_pooled(g, ceil_mode != 0, out_height, out_width)) return rc;
  if (int rc = geom_count(g)) return rc;
  if (g.chunks == 0) return 0;
  if (!codes || !pooled) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)pooled)) & 15u) != 0) return fail_arg("codes and pooled must be 16-byte aligned");
  PoolArgs a;
  a.x = static_cast<const uint8_t*>(codes);
  a.y = static_cast<uint8_t*>(pooled);
  a.c16 = FastDiv::make((uint32_t)g.c16);
  a.wo = FastDiv::make((uint32_t)g.wo);
  a.ho = FastDiv::make((uint32_t)g.ho);
  a.chunks = (uint32_t)g.chunks;
  a.H = (int32_t)height; a.W = (int32_t)width; a.kh = kh; a.kw = kw;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.flip = code_form(code_dtype).flip;
  const unsigned blocks = (unsigned)(((int64_t)a.chunks + kThreads - 1) / kThreads);                  // <= 2^24
  const hipStream_t s = (hipStream_t)stream;
  const int fixed = MCTQ_POOL_UNROLL && kh == kw && (kh == 2 || kh == 3) ? kh : 0;
  if (fixed == 2) hipLaunchKernelGGL(codes_maxpool_kernel<2>, dim3(blocks), dim3(kThreads), 0, s, a);
  else if (fixed == 3) hipLaunchKernelGGL(codes_maxpool_kernel<3>, dim3(blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(codes_maxpool_kernel<0>, dim3(blocks), dim3(kThreads), 0, s, a);
  note_launch("codes_maxpool", code_dtype == MCTQ_CODE_U8 ? "u8 max" : "i8 max", fixed ? fixed * fixed : 1, 0, 1, 1);
  return check_launch("mctq_codes_maxpool_nhwc");
}

}  // extern "C"
