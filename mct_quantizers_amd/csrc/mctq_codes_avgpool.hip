// mctq_codes_avgpool.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Average pooling on NHWC activation codes: codes [B][H][W][C] (1 byte each, int8 or uint8, form (scale_a, zp_a)) -> pooled
// [B][Ho][Wo][C] in the form of the holder behind the pool, torch.nn.AvgPool2d's semantics (kernel, stride, padding,
// ceil_mode, count_include_pad, divisor_override).  Per output element
//     S    = sum over the window's taps inside the image of (code - zp_a)        int32, exact
//     div  = divisor_override | PyTorch's pool_size (count_include_pad) | the number of taps inside the image
//     v    = fma(float(S), scale_a, +0)                                          join_residual: one float32 rounding
//     m    = v / float(div)                                                      IEEE float32 division
//     code = ql_code(m)                                                          clamp(rint(m * (1 / scale_b)) + zp_b, qmin, qmax)
// float(S) is exact while the window has at most 65536 taps (255 * 65536 < 2^24), the launcher's limit.  The sum is an
// integer and integer addition is associative, so it may be split over lanes in any way: both forms below give the same bytes.
//
// Lane form: that of mctq_codes_maxpool.hip.  A lane owns one 16-byte chunk (16 channels) of one output pixel, consecutive
// lanes on consecutive chunks; per tap one 16-byte load, at the end one 16-byte store.  A tap outside the image is loaded from
// a clamped (valid) address and then replaced by 0: the loads do not depend on a branch.  One unsigned byte sum serves both
// code types: int8 codes have bit 7 flipped on load (code + 128), and (zp + bias) * taps_inside is subtracted once at the end.
// The sixteen sums are kept as sixteen 16-bit lanes (even and odd bytes of each dword apart, v_pk_add_u16 takes two at a
// time) and widened into int32 every 256 taps (255 * 256 < 2^16).
//
// Split form, for few and large windows (global pooling at small batch, an SE squeeze): a workgroup owns one output pixel and
// a group of G <= 16 consecutive chunks; lane t works on chunk t % G of the group and on the taps t / G, t / G + 256 / G, ...
// of the window, so the lanes that share a tap sit on consecutive chunks and neighbouring tap slices on neighbouring pixels.
// The int32 partial sums meet in LDS (256 lanes x 16 sums = 16 KiB): column by column, then one lane per chunk runs the
// epilogue above and stores.  No atomics, nothing passes between workgroups.
#include "mctq_consumer.hpp"               // FastDiv, u32x4, QlOut, ql_code, join_residual

namespace mctq {

extern int g_avgpool_form;                 // tuning key "avgpool_form" (mctq_misc.hip): 0 = auto, 1 = lane form, 2 = split form

struct AvgArgs {
  const uint8_t* x;
  uint8_t* y;
  FastDiv c16, wo, ho;                             // chunks per pixel (C / 16), Wo, Ho
  FastDiv groups, kwd;                             // split form: chunk groups per pixel, kw
  uint32_t chunks;                                 // B * Ho * Wo * C / 16
  uint32_t gshift;                                 // split form: log2(G)
  int32_t H, W, kh, kw, stride_h, stride_w, pad_h, pad_w;
  int32_t include_pad, divisor;                    // count_include_pad; divisor_override (0 = none)
  uint32_t flip;                                   // 0x80808080 for int8 codes (code c -> byte c + 128), 0 for uint8
  int32_t zb;                                      // the zero point with the same bias
  float scale;
  QlOut o;
};

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// sixteen byte sums of the taps given to add(): packed 16-bit partial sums, widened every 256 taps
struct ByteSums {
  u16x2 even[4], odd[4];                           // bytes 0 and 2 / 1 and 3 of each dword
  int32_t wide[16];
  int pending;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < 4; ++q) even[q] = odd[q] = u16x2{0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) wide[j] = 0;
    pending = 0;
  }
  __device__ __forceinline__ void widen() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      wide[4 * q + 0] += even[q][0]; wide[4 * q + 1] += odd[q][0];
      wide[4 * q + 2] += even[q][1]; wide[4 * q + 3] += odd[q][1];
      even[q] = odd[q] = u16x2{0, 0};
    }
    pending = 0;
  }
  __device__ __forceinline__ void add(const u32x4& v, bool inside, uint32_t flip) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t u = inside ? v[q] ^ flip : 0u;
      even[q] += __builtin_bit_cast(u16x2, u & 0x00ff00ffu);
      odd[q] += __builtin_bit_cast(u16x2, (u >> 8) & 0x00ff00ffu);
    }
    if (++pending == 256) widen();                 // uniform over the wave: every lane has taken the same number of taps
  }
};

// the window of output pixel (oy, ox): its first input coordinates, the taps inside the image and the divisor
struct Window { int iy0, ix0, inside, div; };
__device__ __forceinline__ Window window_of(const AvgArgs& a, uint32_t oy, uint32_t ox) {
  Window w;
  w.iy0 = (int)oy * a.stride_h - a.pad_h; w.ix0 = (int)ox * a.stride_w - a.pad_w;
  const int ny = max(min(w.iy0 + a.kh, a.H) - max(w.iy0, 0), 0), nx = max(min(w.ix0 + a.kw, a.W) - max(w.ix0, 0), 0);
  w.inside = ny * nx;
  w.div = a.divisor ? a.divisor
        : a.include_pad ? (min(w.iy0 + a.kh, a.H + a.pad_h) - w.iy0) * (min(w.ix0 + a.kw, a.W + a.pad_w) - w.ix0) : w.inside;
  return w;
}

// sums[j]: the byte sum of channel j of the chunk -> the chunk's sixteen codes
__device__ __forceinline__ u32x4 avg_codes(const AvgArgs& a, const Window& w, const int32_t (&sums)[16]) {
  const int32_t off = a.zb * w.inside;
  const float fdiv = (float)w.div;
  u32x4 out;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = join_residual((float)(sums[4 * q + j] - off), a.scale);
      const float m = w.div > 0 ? v / fdiv : 0.0f;                         // (a window without a tap: 0.0, never a division by 0)
      word |= ((uint32_t)ql_code(m, a.o) & 0xffu) << (8 * j);
    }
    out[q] = word;
  }
  return out;
}

__global__ __launch_bounds__(kThreads) void codes_avgpool_lane_kernel(AvgArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kThreads + threadIdx.x;          // < 2^32: the launcher checks the chunk count
  if (g >= a.chunks) return;                                                 // the last block may be partly empty
  uint32_t cc, ox, oy;
  const uint32_t m = a.c16.divmod(g, cc);
  const uint32_t b = a.ho.divmod(a.wo.divmod(m, ox), oy);
  const int64_t c16 = a.c16.d;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.x) + (int64_t)b * a.H * a.W * c16 + cc;
  const Window w = window_of(a, oy, ox);
  ByteSums s;
  s.clear();
  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = w.iy0 + ky, cy = min(max(iy, 0), a.H - 1);
    for (int kx = 0; kx < a.kw; ++kx) {
      const int ix = w.ix0 + kx, cx = min(max(ix, 0), a.W - 1);              // a valid address whatever the tap
      const bool inside = (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
      s.add(src[((int64_t)cy * a.W + cx) * c16], inside, a.flip);
    }
  }
  s.widen();
  reinterpret_cast<u32x4*>(a.y)[g] = avg_codes(a, w, s.wide);
}

__global__ __launch_bounds__(kThreads) void codes_avgpool_split_kernel(AvgArgs a) {
  __shared__ int32_t part[kThreads * 16];
  const uint32_t t = threadIdx.x, G = 1u << a.gshift, slices = (uint32_t)kThreads >> a.gshift;
  const uint32_t cg = t & (G - 1), slice = t >> a.gshift;
  uint32_t grp, ox, oy;
  const uint32_t pixel = a.groups.divmod(blockIdx.x, grp);                   // < B * Ho * Wo: the launcher's grid
  const uint32_t b = a.ho.divmod(a.wo.divmod(pixel, ox), oy);
  const uint32_t c16 = a.c16.d, cc = grp * G + cg;
  const bool owns = cc < c16;                                                // the last group of a pixel may be partly empty:
  const uint32_t cl = owns ? cc : c16 - 1;                                   // such lanes load a valid chunk and store nothing
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.x) + (int64_t)b * a.H * a.W * c16 + cl;
  const Window w = window_of(a, oy, ox);
  const uint32_t taps = (uint32_t)a.kh * (uint32_t)a.kw;
  ByteSums s;
  s.clear();
  for (uint32_t tap = slice; tap < taps; tap += slices) {
    uint32_t kx;
    const uint32_t ky = a.kwd.divmod(tap, kx);
    const int iy = w.iy0 + (int)ky, ix = w.ix0 + (int)kx;
    const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
    const bool inside = (uint32_t)iy < (uint32_t)a.H && (uint32_t)ix < (uint32_t)a.W;
    s.add(src[((int64_t)cy * a.W + cx) * (int64_t)c16], inside, a.flip);
  }
  s.widen();
  // part[slice][cg][j]: a column (cg, j) is G * 16 ints apart from slice to slice
#pragma unroll
  for (int j = 0; j < 16; ++j) part[t * 16 + j] = s.wide[j];
  __syncthreads();
  const uint32_t cols = G * 16;                                              // <= 256
  if (t < cols) {
    int32_t total = 0;
    for (uint32_t sl = 0; sl < slices; ++sl) total += part[sl * cols + t];
    part[t] = total;                                                         // (column t is read and written by lane t alone)
  }
  __syncthreads();
  if (slice == 0 && owns) {
    int32_t sums[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) sums[j] = part[cg * 16 + j];
    reinterpret_cast<u32x4*>(a.y)[(int64_t)pixel * c16 + cc] = avg_codes(a, w, sums);
  }
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_avgpool_nhwc(const void* codes, void* pooled, int32_t code_dtype, int32_t zero_point, float scale, int64_t batch,
                            int64_t height, int64_t width, int64_t channels, int32_t kh, int32_t kw, int32_t stride_h,
                            int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t ceil_mode, int32_t count_include_pad,
                            int32_t divisor_override, int64_t out_height, int64_t out_width, int32_t y_code_dtype, float y_scale,
                            int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max, void* stream) {
  WindowGeom g = {batch, height, width, channels, kh, kw, stride_h, stride_w, pad_h, pad_w, 1, 1};      // no dilation
  if (int rc = geom_check_sizes(g, true)) return rc;
  if ((int64_t)kh * kw > 65536) return fail_arg("more than 65536 taps in a window");
  if (divisor_override < 0) return fail_arg("negative divisor_override");
  if (int rc = geom_check_channels(g)) return rc;
  if (int rc = form_check(code_dtype, zero_point, scale, {"code_dtype", "zero_point", "the input's type", "scale"})) return rc;
  if (int rc = form_check_scale(y_scale, "y_scale")) return rc;
  QlOut o;
  if (y_code_dtype < 0) return fail_arg("bad y_code_dtype");
  if (int rc = ql_output_form(o, y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max)) return rc;
  if (int rc = geom_check_fit(g, true)) return rc;
  if (int rc = geom_check_pooled(g, ceil_mode != 0, out_height, out_width)) return rc;
  if (int rc = geom_count(g)) return rc;
  if (g.chunks == 0) return 0;
  const int64_t wo = g.wo, ho = g.ho, pixels = g.pixels, c16 = g.c16;
  if (!codes || !pooled) return fail_arg("NULL pointer");
  if (((((uintptr_t)codes) | ((uintptr_t)pooled)) & 15u) != 0) return fail_arg("codes and pooled must be 16-byte aligned");
  AvgArgs a;
  a.x = static_cast<const uint8_t*>(codes);
  a.y = static_cast<uint8_t*>(pooled);
  a.c16 = FastDiv::make((uint32_t)c16);
  a.wo = FastDiv::make((uint32_t)wo);
  a.ho = FastDiv::make((uint32_t)ho);
  a.kwd = FastDiv::make((uint32_t)kw);
  a.chunks = (uint32_t)(pixels * c16);
  a.H = (int32_t)height; a.W = (int32_t)width; a.kh = kh; a.kw = kw;
  a.stride_h = stride_h; a.stride_w = stride_w; a.pad_h = pad_h; a.pad_w = pad_w;
  a.include_pad = count_include_pad != 0; a.divisor = divisor_override;
  const CodeForm f = code_form(code_dtype, zero_point, scale);
  a.flip = f.flip; a.zb = f.zb; a.scale = f.scale;
  a.o = o;
  // split form: G = the least power of two >= C / 16, at most 16, chunks of a pixel per workgroup
  uint32_t gshift = 0;
  while (gshift < 4 && (1ll << gshift) < c16) ++gshift;
  a.gshift = gshift;
  const int64_t groups = (c16 + (1ll << gshift) - 1) >> gshift;
  a.groups = FastDiv::make((uint32_t)groups);
  const int64_t lane_blocks = ((int64_t)a.chunks + kThreads - 1) / kThreads, split_blocks = pixels * groups;       // <= 2^24, < 2^32
  const int64_t taps = (int64_t)kh * kw;
  // Auto: the split form where the lane form would leave most of the device idle under long tap loops -- the output chunks give
  // every CU at most one workgroup of the lane form, and the window has at least 25 taps.  Measured (one MI355X, 256 CUs;
  // tools/avgpool_consumer_probe.py, section forms; table in profiles/EXPERIMENTS.md): global pools of 9 / 16 / 25 / 49 / 196
  // taps at 1 / 32 / 64 / 256 / 2048 lane-form workgroups.  From 25 taps on the split form takes 1.2 - 8.5 x less up to 256
  // workgroups (a tie at the launch floor, 8.0 against 8.2 us, for 25 taps in one workgroup) and 1.2 - 1.6 x MORE at 2048; at 9
  // and 16 taps it ties or loses everywhere but one row.
  bool split = g_avgpool_form == 2 || (g_avgpool_form == 0 && lane_blocks <= (int64_t)cu_count() && taps >= 25);
  if (split_blocks > INT32_MAX) split = false;                               // (the grid's limit: such a launch fills the device anyway)
  const hipStream_t s = (hipStream_t)stream;
  if (split) hipLaunchKernelGGL(codes_avgpool_split_kernel, dim3((unsigned)split_blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(codes_avgpool_lane_kernel, dim3((unsigned)lane_blocks), dim3(kThreads), 0, s, a);
  note_launch("codes_avgpool", f.is_signed ? (split ? "i8 avg split" : "i8 avg lane") : (split ? "u8 avg split" : "u8 avg lane"), 1, 0, 1, 1);
  return check_launch("mctq_codes_avgpool_nhwc");
}

}  // extern "C"
