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
#include "mctq_consumer.hpp"               // FastDiv, u32x4

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

// PyTorch's pooling_output_shape along one axis (padded extent np = n + 2 * pad, span = dil * (k - 1) + 1 <= np): with
// ceil_mode the division rounds up, and a last window that would start beyond the image plus its left padding is dropped.
static int64_t pooled_extent(int64_t n, int64_t pad, int64_t span, int64_t stride, bool ceil_mode) {
  const int64_t np = n + 2 * pad;
  int64_t out = (np - span + (ceil_mode ? stride - 1 : 0)) / stride + 1;
  if (ceil_mode && (out - 1) * stride >= n + pad) --out;
  return out;
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_maxpool_nhwc(const void* codes, void* pooled, int32_t code_dtype, int64_t batch, int64_t height, int64_t width,
                            int64_t channels, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h,
                            int32_t pad_w, int32_t dil_h, int32_t dil_w, int32_t ceil_mode, int64_t out_height, int64_t out_width,
                            void* stream) {
  if (batch < 0 || height < 0 || width < 0 || channels < 0) return fail_arg("negative extent");
  if (kh < 1 || kw < 1) return fail_arg("kernel size below 1");
  if (stride_h < 1 || stride_w < 1) return fail_arg("stride below 1");
  if (dil_h < 1 || dil_w < 1) return fail_arg("dilation below 1");
  if (pad_h < 0 || pad_w < 0) return fail_arg("negative padding");
  if (pad_h > kh / 2 || pad_w > kw / 2) return fail_arg("padding larger than half the kernel size");
  if (channels % 16 != 0) return fail_arg("channels must be a multiple of 16");
  if (code_dtype != MCTQ_CODE_I8 && code_dtype != MCTQ_CODE_U8) return fail_arg("bad code_dtype");
  // the kernel's input coordinates oy * stride - pad + ky * dilation stay below padded extent + span: within int32
  const int64_t hp = height + 2 * (int64_t)pad_h, wp = width + 2 * (int64_t)pad_w;
  const int64_t span_h = (int64_t)dil_h * (kh - 1) + 1, span_w = (int64_t)dil_w * (kw - 1) + 1;
  if (hp + span_h > INT32_MAX || wp + span_w > INT32_MAX) return fail_arg("padded image extent exceeds 2^31 - 1");
  if (hp < span_h || wp < span_w) return fail_arg("the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)");
  const int64_t ho = pooled_extent(height, pad_h, span_h, stride_h, ceil_mode != 0);
  const int64_t wo = pooled_extent(width, pad_w, span_w, stride_w, ceil_mode != 0);
  // the caller allocated out_height x out_width pixels per image: a disagreement would be an out-of-bounds write
  if (out_height != ho || out_width != wo) return fail_arg("out_height / out_width are not the pooled extent");
  if (batch == 0 || channels == 0) return 0;
  // (padding alone could make room for a kernel on an image without pixels; the clamped loads need one)
  if (height == 0 || width == 0) return fail_arg("an image of a non-empty batch needs at least one pixel");
  if (batch > INT32_MAX / (ho * wo)) return fail_arg("too many output pixels for one launch");       // ho * wo < 2^62
  const int64_t pixels = batch * ho * wo, c16 = channels / 16;
  // a lane's index, pixel * (channels / 16) + chunk, is a 32-bit number (beyond it: split the batch)
  if (c16 > UINT32_MAX / pixels) return fail_arg("more than 2^32 - 1 16-channel chunks of output in one launch");
  if (!codes || !pooled) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)pooled)) & 15u) != 0) return fail_arg("codes and pooled must be 16-byte aligned");
  PoolArgs a;
  a.x = static_cast<const uint8_t*>(codes);
  a.y = static_cast<uint8_t*>(pooled);
  a.c16 = FastDiv::make((uint32_t)c16);
  a.wo = FastDiv::make((uint32_t)wo);
  a.ho = FastDiv::make((uint32_t)ho);
  a.chunks = (uint32_t)(pixels * c16);
  a.H = (int32_t)height; a.W = (int32_t)width; a.kh = kh; a.kw = kw;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dil_h = dil_h; a.dil_w = dil_w;
  a.flip = code_dtype == MCTQ_CODE_I8 ? 0x80808080u : 0u;
  const unsigned blocks = (unsigned)(((int64_t)a.chunks + kThreads - 1) / kThreads);                  // <= 2^24
  const hipStream_t s = (hipStream_t)stream;
  const int fixed = MCTQ_POOL_UNROLL && kh == kw && (kh == 2 || kh == 3) ? kh : 0;
  if (fixed == 2) hipLaunchKernelGGL(codes_maxpool_kernel<2>, dim3(blocks), dim3(kThreads), 0, s, a);
  else if (fixed == 3) hipLaunchKernelGGL(codes_maxpool_kernel<3>, dim3(blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(codes_maxpool_kernel<0>, dim3(blocks), dim3(kThreads), 0, s, a);
  g_note.shape = "codes_maxpool"; g_note.op = code_dtype == MCTQ_CODE_U8 ? "u8 max" : "i8 max";
  g_note.unroll = fixed ? fixed * fixed : 1; g_note.nt = 0; g_note.in_bytes = 1; g_note.out_bytes = 1; ++g_note.count;
  if (g_launch_log) log_launch();
  return check_launch("mctq_codes_maxpool_nhwc");
}

}  // extern "C"
