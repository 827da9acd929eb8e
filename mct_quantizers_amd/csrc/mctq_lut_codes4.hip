// mctq_lut_codes4.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h); ops: mctq_lut_index.hpp
//
// Packed 4-bit codebook-index codes of the LUT quantizers (codebooks of at most 16 entries): two codes per byte, element 2j of
// the storage order in the low nibble.  Three launch shapes modelled on mctq_codes4.hip (flat, rows, last axis): a lane
// vector is one 16-byte load -- 8 indices per 32-bit store for 16-bit inputs, 4 per 16-bit store for float32.
#include "mctq_lut_index.hpp"

namespace mctq {

constexpr int kL4U = 4;                       // lane vectors per lane: 4 x 16 B of input in flight

// a lane vector is one 16-byte load: 4 float32 elements -> 2 bytes of codes, 8 half-precision elements -> 4 bytes
template <class TI> struct L4Vec {
  static constexpr int N = 16 / (int)sizeof(TI);
  typedef typename std::conditional<N == 4, uint16_t, uint32_t>::type Out;
  typedef typename VecT<TI, N>::type VI;
  __device__ __forceinline__ static void load(const TI* p, float* f) {
    const VI a = __builtin_nontemporal_load(reinterpret_cast<const VI*>(p));
#pragma unroll
    for (int i = 0; i < N; ++i) f[i] = (float)a[i];
  }
};

template <bool FAST, class Op, int N>
__device__ __forceinline__ uint32_t l4_word(const Op& op, const float* f, const typename Op::Param& p, const typename Op::Book& b) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t c = (uint32_t)(int32_t)op.template apply<FAST>(f[i], p, b);
    w |= (c & 0xFu) << (4 * i);                                   // element i -> nibble i: bytes hold (2j, 2j + 1)
  }
  return w;
}

// per tensor: nv lane vectors
template <class Op, class TI>
__global__ __launch_bounds__(kThreads) void lut_codes4_flat_kernel(const TI* __restrict__ x, typename L4Vec<TI>::Out* __restrict__ y,
                                                                   int64_t nv, Op op, typename Op::Param p) {
  typedef L4Vec<TI> V;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int64_t base = (int64_t)blockIdx.x * (kThreads * kL4U) + threadIdx.x;
  float f[kL4U][V::N];
#pragma unroll
  for (int u = 0; u < kL4U; ++u)
    if (base + u * kThreads < nv) V::load(x + (base + u * kThreads) * V::N, f[u]);
  const typename Op::Book book = op.setup(smem);
  const bool fast = __builtin_amdgcn_readfirstlane((int)Op::can_fast(p)) != 0;
#pragma unroll
  for (int u = 0; u < kL4U; ++u) {
    const int64_t v = base + u * kThreads;
    if (v < nv) {
      const uint32_t w = fast ? l4_word<true, Op, V::N>(op, f[u], p, book) : l4_word<false, Op, V::N>(op, f[u], p, book);
      __builtin_nontemporal_store((typename V::Out)w, &y[v]);
    }
  }
}

// per channel, inner % 8 == 0: block = (row, tile); the row's parameters are wave-uniform (scalar loads)
template <class Op, class TI>
__global__ __launch_bounds__(kThreads) void lut_codes4_rows_kernel(const TI* __restrict__ x, typename L4Vec<TI>::Out* __restrict__ y,
                                                                   uint32_t tiles, uint32_t innerv, uint32_t channels, Op op) {
  typedef L4Vec<TI> V;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const uint32_t first = tile * (kThreads * kL4U) + threadIdx.x;
  const int64_t rbase = (int64_t)row * innerv;
  float f[kL4U][V::N];
#pragma unroll
  for (int u = 0; u < kL4U; ++u)
    if (first + u * kThreads < innerv) V::load(x + (rbase + first + u * kThreads) * V::N, f[u]);
  const typename Op::Book book = op.setup(smem);
  const typename Op::Param p = op.fetch(row % channels);
  const bool fast = __builtin_amdgcn_readfirstlane((int)Op::can_fast(p)) != 0;
#pragma unroll
  for (int u = 0; u < kL4U; ++u) {
    const uint32_t v = first + u * kThreads;
    if (v < innerv) {
      const uint32_t w = fast ? l4_word<true, Op, V::N>(op, f[u], p, book) : l4_word<false, Op, V::N>(op, f[u], p, book);
      __builtin_nontemporal_store((typename V::Out)w, &y[rbase + v]);
    }
  }
}

// per channel along the fastest axis (inner == 1, channels % 8 == 0): the lanes of bps neighbouring blocks cover k whole
// rows and step down k rows at a time, keeping their channels (cf. codes4_lastaxis_kernel).  A lane owns its divisors, so
// the quotient is the plain IEEE division.
template <class Op, class TI>
__global__ __launch_bounds__(kThreads) void lut_codes4_lastaxis_kernel(const TI* __restrict__ x,
                                                                       typename L4Vec<TI>::Out* __restrict__ y, uint64_t rows,
                                                                       uint32_t vc, uint32_t k, uint32_t bps, Op op) {
  typedef L4Vec<TI> V;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const typename Op::Book book = op.setup(smem);          // every thread: setup synchronises
  const uint32_t g = (blockIdx.x % bps) * kThreads + threadIdx.x;
  const uint32_t ro = g / vc, col = g - ro * vc;
  if (ro >= k) return;
  const uint64_t row0 = (uint64_t)(blockIdx.x / bps) * ((uint64_t)kL4U * k) + ro;
  float f[kL4U][V::N];
#pragma unroll
  for (int u = 0; u < kL4U; ++u) {
    const uint64_t row = row0 + (uint64_t)u * k;
    if (row < rows) V::load(x + (row * vc + col) * V::N, f[u]);
  }
  typename Op::Param p[V::N];
#pragma unroll
  for (int i = 0; i < V::N; ++i) p[i] = op.fetch(col * V::N + i);
#pragma unroll
  for (int u = 0; u < kL4U; ++u) {
    const uint64_t row = row0 + (uint64_t)u * k;
    if (row < rows) {
      uint32_t w = 0;
#pragma unroll
      for (int i = 0; i < V::N; ++i) {
        const uint32_t c = (uint32_t)(int32_t)op.template apply<false>(f[u][i], p[i], book);
        w |= (c & 0xFu) << (4 * i);
      }
      __builtin_nontemporal_store((typename V::Out)w, &y[row * vc + col]);
    }
  }
}

template <class F>
static int with_in_types(int dtype, F f) {
  switch (dtype) {
    case MCTQ_DT_F32: return f(float());
    case MCTQ_DT_F16: return f(_Float16());
    case MCTQ_DT_BF16: return f(__bf16());
    default: return fail_arg("unknown dtype");
  }
}

static bool aligned4(const void* x, const void* codes) { return !(((uintptr_t)x) & 15u) && !(((uintptr_t)codes) & 3u); }

template <class Op>
static int codes4_per_tensor_t(const Op& op, const typename Op::Param& p, const void* x, void* codes, int64_t n, int dtype,
                                 size_t book_bytes, hipStream_t st) {
  if (n % 8 != 0) return fail_arg("4-bit codes: n must be a multiple of 8");
  if (!aligned4(x, codes)) return fail_arg("4-bit codes: x must be 16-byte and codes 4-byte aligned");
  if (n == 0) return 0;
  return with_in_types(dtype, [&](auto ti) {
    typedef decltype(ti) TI;
    typedef L4Vec<TI> V;
    const int64_t nv = n / V::N, blocks = (nv + kThreads * kL4U - 1) / (kThreads * kL4U);
    if (blocks > 0x7fffffffLL) return fail_arg("tensor too large for one launch");
    hipLaunchKernelGGL((lut_codes4_flat_kernel<Op, TI>), dim3((unsigned)blocks), dim3(kThreads), book_bytes, st,
                       static_cast<const TI*>(x), static_cast<typename V::Out*>(codes), nv, op, p);
    note<Op, TI, uint8_t>("lut_codes4_flat_kernel", kL4U, 1);
    return check_launch("lut codes4 flat launch");
  });
}

template <class Op>
static int codes4_per_channel_t(const Op& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                                  int dtype, size_t book_bytes, hipStream_t st) {
  const int64_t n = outer * channels * inner;
  if (n == 0) return 0;
  if (inner % 8 != 0 && !(inner == 1 && channels % 8 == 0))
    return fail_arg("4-bit codes need inner % 8 == 0, or inner == 1 with channels % 8 == 0");
  if (!aligned4(x, codes)) return fail_arg("4-bit codes: x must be 16-byte and codes 4-byte aligned");
  if (inner % 8 == 0) {
    return with_in_types(dtype, [&](auto ti) {
      typedef decltype(ti) TI;
      typedef L4Vec<TI> V;
      const int64_t innerv = inner / V::N, rows = outer * channels;
      const int64_t tiles = (innerv + kThreads * kL4U - 1) / (kThreads * kL4U);
      if (rows * tiles > 0x7fffffffLL || innerv > 0x7fffffffLL || channels > 0x7fffffffLL)
        return fail_arg("tensor too large for one launch");
      hipLaunchKernelGGL((lut_codes4_rows_kernel<Op, TI>), dim3((unsigned)(rows * tiles)), dim3(kThreads), book_bytes, st,
                         static_cast<const TI*>(x), static_cast<typename V::Out*>(codes), (uint32_t)tiles, (uint32_t)innerv,
                         (uint32_t)channels, op);
      note<Op, TI, uint8_t>("lut_codes4_rows_kernel", kL4U, 1);
      return check_launch("lut codes4 rows launch");
    });
  }
  return with_in_types(dtype, [&](auto ti) {
    typedef decltype(ti) TI;
    typedef L4Vec<TI> V;
    const int64_t vc = channels / V::N;
    int64_t k = (2048 + vc - 1) / vc, best = -1;
    for (int64_t c = k; c < k + 16; ++c) {
      const int64_t waste = (kThreads - (c * vc) % kThreads) % kThreads * 4096 / (c * vc);
      if (best < 0 || waste < best) { best = waste; k = c; }
    }
    const int64_t bps = (k * vc + kThreads - 1) / kThreads;
    const int64_t blocks = bps * ((outer + kL4U * k - 1) / (kL4U * k));
    if (blocks > 0x7fffffffLL || k * vc > 0x7fffffffLL) return fail_arg("tensor too large for one launch");
    hipLaunchKernelGGL((lut_codes4_lastaxis_kernel<Op, TI>), dim3((unsigned)blocks), dim3(kThreads), book_bytes, st,
                       static_cast<const TI*>(x), static_cast<typename V::Out*>(codes), (uint64_t)outer, (uint32_t)vc,
                       (uint32_t)k, (uint32_t)bps, op);
    note<Op, TI, uint8_t>("lut_codes4_lastaxis_kernel", kL4U, 1);
    return check_launch("lut codes4 lastaxis launch");
  });
}

int lut_codes4_per_tensor(const LutIndexTableOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                          size_t book_bytes, hipStream_t st) {
  return codes4_per_tensor_t(op, p, x, codes, n, dtype, book_bytes, st);
}
int lut_codes4_per_tensor(const LutIndexOp& op, const LutCommon::Param& p, const void* x, void* codes, int64_t n, int dtype,
                          size_t book_bytes, hipStream_t st) {
  return codes4_per_tensor_t(op, p, x, codes, n, dtype, book_bytes, st);
}
int lut_codes4_per_channel(const LutIndexTableOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                           int dtype, size_t book_bytes, hipStream_t st) {
  return codes4_per_channel_t(op, x, codes, outer, channels, inner, dtype, book_bytes, st);
}
int lut_codes4_per_channel(const LutIndexOp& op, const void* x, void* codes, int64_t outer, int64_t channels, int64_t inner,
                           int dtype, size_t book_bytes, hipStream_t st) {
  return codes4_per_channel_t(op, x, codes, outer, channels, inner, dtype, book_bytes, st);
}

}  // namespace mctq
