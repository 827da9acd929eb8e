// mctq_lut_decode.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Decode of the LUT quantizers' codebook-index codes (an extension without a reference counterpart):
//     y = (lut[code] / mult) * thr         -- the two float32 operations LutOp::apply ends with
// 1 byte (uint8) or half a byte (packed 4-bit) read and 4 bytes written per element: narrow reads, wide writes, so the
// accesses are shaped from the WRITE side.  A lane vector is ONE 32-bit word of codes -- 4 uint8 codes -> one 16-byte
// store, or 8 nibbles -> two 16-byte stores -- consecutive lanes take consecutive words (a wave reads 256 contiguous
// bytes and writes 1 or 2 contiguous KiB per step), and a lane keeps U such words in flight.  Every block stages
// qtab[j] = lut[j] / mult (exact: mult is a power of two) in LDS once, zero-padded to the code's range so that no code
// value can read outside it; an element is one LDS read and one v_mul_f32.  The codebook is requested BEFORE the code
// words (vector loads return in order, and the codebook is L2-resident), so the table is in LDS when the codes land.
#include "mctq_kernels.hpp"

namespace mctq {

struct LutDecodeOp { static constexpr const char* kName = "LutDecodeOp"; };

constexpr int kDecU = 4;                        // code words in flight per lane of the flat kernels

// V = elements per code word: 4 (uint8) or 8 (packed 4-bit)
template <int V> struct DecCodes {
  static constexpr int kBits = 32 / V, kTable = 1 << kBits;
  __device__ __forceinline__ static uint32_t code(uint32_t w, int i) { return (w >> (kBits * i)) & (uint32_t)(kTable - 1); }
};

// one block-wide staging of lut[j] / mult; `mine` was loaded by the caller ahead of its data loads
template <int TABLE>
__device__ __forceinline__ float dec_prefetch(const float* __restrict__ lut, int n_lut) {
  return ((int)threadIdx.x < n_lut && (int)threadIdx.x < TABLE) ? lut[threadIdx.x] : 0.0f;
}
template <int TABLE>
__device__ __forceinline__ void dec_commit(float* qtab, float mine, float mult) {
  if ((int)threadIdx.x < TABLE) qtab[threadIdx.x] = mine / mult;
  __syncthreads();
}

template <int V>
__device__ __forceinline__ void dec_store(float* __restrict__ y, const float* qtab, uint32_t w, const float* thr) {
  float q[V];
#pragma unroll
  for (int i = 0; i < V; ++i) q[i] = qtab[DecCodes<V>::code(w, i)];
#pragma unroll
  for (int i = 0; i < V; i += 4) {
    const f32x4 o = {q[i] * thr[i], q[i + 1] * thr[i + 1], q[i + 2] * thr[i + 2], q[i + 3] * thr[i + 3]};
    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(y + i));
  }
}

// Where a lane vector's thresholds come from.
//   kTensor : one threshold for the launch
//   kWhole  : inner % V == 0 -- a vector lies in one channel: c = (v / (inner / V)) % channels, one read per vector
//   kLast   : inner == 1, channels % V == 0 -- the vector's V channels are consecutive: c0 = (v % (channels / V)) * V
//   kRagged : anything else -- the channel of every element on its own
enum { kTensor = 0, kWhole = 1, kLast = 2, kRagged = 3 };

template <int V, int MODE>
__device__ __forceinline__ void dec_thresholds(float* t, uint32_t v, float thr0, const float* __restrict__ thr,
                                               uint32_t inner, uint32_t channels) {
  if constexpr (MODE == kTensor) {
#pragma unroll
    for (int i = 0; i < V; ++i) t[i] = thr0;
  } else if constexpr (MODE == kWhole) {
    const float one = thr[(v / (inner / V)) % channels];
#pragma unroll
    for (int i = 0; i < V; ++i) t[i] = one;
  } else if constexpr (MODE == kLast) {
    const uint32_t c0 = (v % (channels / V)) * V;
#pragma unroll
    for (int i = 0; i < V; ++i) t[i] = thr[c0 + i];
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) t[i] = thr[((v * V + i) / inner) % channels];
  }
}

// flat walk over the nv code words of the tensor (n < 2^32: 32-bit indices); block 0 also takes the n % V trailing codes
// of a uint8 tensor (bytes, read one by one)
template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void lut_decode_kernel(const uint32_t* __restrict__ cw, float* __restrict__ y,
                                                              uint32_t n, uint32_t inner, uint32_t channels, float thr0,
                                                              float mult, int n_lut, const float* __restrict__ lut,
                                                              const float* __restrict__ thr) {
  typedef DecCodes<V> C;
  __shared__ float qtab[C::kTable];
  const uint32_t nv = n / V;
  const uint32_t base = blockIdx.x * (uint32_t)(kThreads * kDecU) + threadIdx.x;
  const float mine = dec_prefetch<C::kTable>(lut, n_lut);
  __builtin_amdgcn_sched_barrier(0);
  uint32_t w[kDecU];
#pragma unroll
  for (int u = 0; u < kDecU; ++u) {
    const uint32_t v = base + u * kThreads;
    w[u] = v < nv ? __builtin_nontemporal_load(cw + v) : 0u;
  }
  __builtin_amdgcn_sched_barrier(0);
  dec_commit<C::kTable>(qtab, mine, mult);
#pragma unroll
  for (int u = 0; u < kDecU; ++u) {
    const uint32_t v = base + u * kThreads;
    if (v < nv) {
      float t[V];
      dec_thresholds<V, MODE>(t, v, thr0, thr, inner, channels);
      dec_store<V>(y + (size_t)v * V, qtab, w[u], t);
    }
  }
  if constexpr (V == 4) {
    const uint32_t e = nv * V + threadIdx.x;
    if (blockIdx.x == 0 && e < n) {
      const uint32_t code = reinterpret_cast<const uint8_t*>(cw)[e];
      const float t = MODE == kTensor ? thr0 : thr[(e / inner) % channels];
      y[e] = qtab[code] * t;
    }
  }
}

// per channel, rows of at least one block of code words (inner % V == 0): block = (row, tile); the row's threshold is
// wave-uniform (one scalar load), no per-lane index arithmetic
template <int V, int U>
__global__ __launch_bounds__(kThreads) void lut_decode_rows_kernel(const uint32_t* __restrict__ cw, float* __restrict__ y,
                                                                   uint32_t tiles, uint32_t innerv, uint32_t channels,
                                                                   float mult, int n_lut, const float* __restrict__ lut,
                                                                   const float* __restrict__ thr) {
  typedef DecCodes<V> C;
  __shared__ float qtab[C::kTable];
  const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const uint32_t first = tile * (uint32_t)(kThreads * U) + threadIdx.x;
  const size_t rbase = (size_t)row * innerv;
  const float mine = dec_prefetch<C::kTable>(lut, n_lut);
  __builtin_amdgcn_sched_barrier(0);
  uint32_t w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t v = first + u * kThreads;
    w[u] = v < innerv ? __builtin_nontemporal_load(cw + rbase + v) : 0u;
  }
  __builtin_amdgcn_sched_barrier(0);
  const float one = thr[row % channels];
  dec_commit<C::kTable>(qtab, mine, mult);
  float t[V];
#pragma unroll
  for (int i = 0; i < V; ++i) t[i] = one;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t v = first + u * kThreads;
    if (v < innerv) dec_store<V>(y + (rbase + v) * V, qtab, w[u], t);
  }
}

// uint8 codes or float32 output that are not word / 16-byte aligned: one element per lane (the slow path, one variant)
__global__ __launch_bounds__(kThreads) void lut_decode_scalar_kernel(const uint8_t* __restrict__ codes, float* __restrict__ y,
                                                                     uint32_t n, uint32_t inner, uint32_t channels,
                                                                     float thr0, float mult, int n_lut,
                                                                     const float* __restrict__ lut,
                                                                     const float* __restrict__ thr) {
  __shared__ float qtab[256];
  dec_commit<256>(qtab, dec_prefetch<256>(lut, n_lut), mult);
  for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (uint64_t)gridDim.x * kThreads) {
    const float t = thr ? thr[((uint32_t)e / inner) % channels] : thr0;
    y[e] = qtab[codes[e]] * t;
  }
}

constexpr int64_t kDecodeMax = (1ll << 32) - 8192;

static int check_decode_args(int32_t code_dtype, const float* lut, int32_t n_lut, float mult) {
  if (code_dtype != MCTQ_CODE_U8 && code_dtype != MCTQ_CODE_U4) return fail_arg("LUT codes are MCTQ_CODE_U8 or MCTQ_CODE_U4");
  if (!lut) return fail_arg("lut is NULL");
  if (n_lut < 1) return fail_arg("n_lut must be at least 1");
  if (code_dtype == MCTQ_CODE_U8 && n_lut > 256) return fail_arg("uint8 LUT codes take codebooks of at most 256 entries");
  if (code_dtype == MCTQ_CODE_U4 && n_lut > 16) return fail_arg("4-bit LUT codes take codebooks of at most 16 entries");
  return check_pow2(mult);
}

template <int V, int MODE>
static int launch_decode_flat(const void* codes, float* y, int64_t n, int64_t inner, int64_t channels, float thr0, float mult,
                              int n_lut, const float* lut, const float* thr, hipStream_t st) {
  const int64_t nv = n / V, per = (int64_t)kThreads * kDecU;
  int64_t blocks = (nv + per - 1) / per;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL((lut_decode_kernel<V, MODE>), dim3((unsigned)blocks), dim3(kThreads), 0, st,
                     static_cast<const uint32_t*>(codes), y, (uint32_t)n, (uint32_t)inner, (uint32_t)channels, thr0, mult, n_lut,
                     lut, thr);
  static const char* const names[2][4] = {
      {"lut_decode_kernel<u8,tensor>", "lut_decode_kernel<u8,whole>", "lut_decode_kernel<u8,lastaxis>", "lut_decode_kernel<u8,ragged>"},
      {"lut_decode_kernel<u4,tensor>", "lut_decode_kernel<u4,whole>", "lut_decode_kernel<u4,lastaxis>", "lut_decode_kernel<u4,ragged>"}};
  note<LutDecodeOp, uint8_t, float>(names[V == 8][MODE], kDecU, 1);
  return check_launch("lut decode launch");
}

static int launch_decode_scalar(const void* codes, float* y, int64_t n, int64_t inner, int64_t channels, float thr0, float mult,
                                int n_lut, const float* lut, const float* thr, hipStream_t st) {
  int64_t blocks = (n + kThreads - 1) / kThreads;
  if (blocks > (int64_t)cu_count() * 32) blocks = (int64_t)cu_count() * 32;
  hipLaunchKernelGGL(lut_decode_scalar_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, static_cast<const uint8_t*>(codes),
                     y, (uint32_t)n, (uint32_t)inner, (uint32_t)channels, thr0, mult, n_lut, lut, thr);
  note<LutDecodeOp, uint8_t, float>("lut_decode_scalar_kernel", 1, 0);
  return check_launch("lut decode scalar launch");
}

template <int V>
static int launch_decode_rows(const void* codes, float* y, int64_t rows, int64_t innerv, int64_t channels, float mult, int n_lut,
                              const float* lut, const float* thr, hipStream_t st, bool& taken) {
  // code words per lane: the widest of {4, 2, 1} whose idle lanes in a row's last tile stay under 1/8
  int u_sel = 1;
  for (int u = 4; u >= 1; u >>= 1) {
    const int64_t per_u = (int64_t)kThreads * u, cap = ((innerv + per_u - 1) / per_u) * per_u;
    if ((cap - innerv) * 8 <= cap) { u_sel = u; break; }
  }
  const int64_t per = (int64_t)kThreads * u_sel, tiles = (innerv + per - 1) / per;
  taken = rows * tiles <= 0x7fffffffLL;
  if (!taken) return 0;
#define MCTQ_DECODE_ROWS(U_)                                                                                                  \
  hipLaunchKernelGGL((lut_decode_rows_kernel<V, U_>), dim3((unsigned)(rows * tiles)), dim3(kThreads), 0, st,                  \
                     static_cast<const uint32_t*>(codes), y, (uint32_t)tiles, (uint32_t)innerv, (uint32_t)channels, mult, n_lut, \
                     lut, thr)
  if (u_sel == 4) MCTQ_DECODE_ROWS(4);
  else if (u_sel == 2) MCTQ_DECODE_ROWS(2);
  else MCTQ_DECODE_ROWS(1);
#undef MCTQ_DECODE_ROWS
  note<LutDecodeOp, uint8_t, float>(V == 8 ? "lut_decode_rows_kernel<u4>" : "lut_decode_rows_kernel<u8>", u_sel, 1);
  return check_launch("lut decode rows launch");
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_lut_decode_per_tensor(const void* codes, float* y, int64_t n, int32_t code_dtype, const float* lut, int32_t n_lut,
                               float mult, float thr_mul, void* stream) {
  if (n < 0) return fail_arg("n < 0");
  if (n > 0 && (!codes || !y)) return fail_arg("codes or y is NULL");
  if (int rc = check_decode_args(code_dtype, lut, n_lut, mult)) return rc;
  if (n > kDecodeMax) return fail_arg("LUT decode takes at most 2^32 - 8192 elements per launch");
  const bool aligned = (((uintptr_t)codes) & 3u) == 0 && (((uintptr_t)y) & 15u) == 0;
  if (code_dtype == MCTQ_CODE_U4) {
    if (n % 8 != 0) return fail_arg("4-bit codes: n must be a multiple of 8");
    if (!aligned) return fail_arg("4-bit codes: y must be 16-byte and codes 4-byte aligned");
    if (n == 0) return 0;
    return launch_decode_flat<8, kTensor>(codes, y, n, 1, 1, thr_mul, mult, n_lut, lut, nullptr, (hipStream_t)stream);
  }
  if (n == 0) return 0;
  if (!aligned) return launch_decode_scalar(codes, y, n, 1, 1, thr_mul, mult, n_lut, lut, nullptr, (hipStream_t)stream);
  return launch_decode_flat<4, kTensor>(codes, y, n, 1, 1, thr_mul, mult, n_lut, lut, nullptr, (hipStream_t)stream);
}

int mctq_lut_decode_per_channel(const void* codes, float* y, int64_t outer, int64_t channels, int64_t inner,
                                int32_t code_dtype, const float* lut, int32_t n_lut, float mult, const float* thresholds,
                                void* stream) {
  if (outer < 0 || channels < 0 || inner < 0) return fail_arg("negative extent");
  if (int rc = check_decode_args(code_dtype, lut, n_lut, mult)) return rc;
  if ((outer > 0 && channels > kDecodeMax / outer) || (outer * channels > 0 && inner > kDecodeMax / (outer * channels)))
    return fail_arg("LUT decode takes at most 2^32 - 8192 elements per launch");
  const int64_t n = outer * channels * inner;
  if (n > 0 && (!codes || !y || !thresholds)) return fail_arg("NULL pointer");
  const bool aligned = (((uintptr_t)codes) & 3u) == 0 && (((uintptr_t)y) & 15u) == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (code_dtype == MCTQ_CODE_U4) {
    const bool whole = inner % 8 == 0, last = inner == 1 && channels % 8 == 0;
    if (n > 0 && !whole && !last) return fail_arg("4-bit codes need inner % 8 == 0, or inner == 1 with channels % 8 == 0");
    if (!aligned) return fail_arg("4-bit codes: y must be 16-byte and codes 4-byte aligned");
    if (n == 0) return 0;
    if (whole && inner / 8 >= kThreads) {
      bool taken = false;
      const int rc = launch_decode_rows<8>(codes, y, outer * channels, inner / 8, channels, mult, n_lut, lut, thresholds, st, taken);
      if (taken) return rc;
    }
    if (whole) return launch_decode_flat<8, kWhole>(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
    return launch_decode_flat<8, kLast>(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
  }
  if (n == 0) return 0;
  if (!aligned) return launch_decode_scalar(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
  if (inner % 4 == 0) {
    if (inner / 4 >= kThreads) {
      bool taken = false;
      const int rc = launch_decode_rows<4>(codes, y, outer * channels, inner / 4, channels, mult, n_lut, lut, thresholds, st, taken);
      if (taken) return rc;
    }
    return launch_decode_flat<4, kWhole>(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
  }
  if (inner == 1 && channels % 4 == 0)
    return launch_decode_flat<4, kLast>(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
  return launch_decode_flat<4, kRagged>(codes, y, n, inner, channels, 0.f, mult, n_lut, lut, thresholds, st);
}

}  // extern "C"
