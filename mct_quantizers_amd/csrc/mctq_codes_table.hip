// mctq_codes_table.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// An elementwise function between two activation holders, on codes: out[i] = table[raw byte in[i]], a 256-entry byte table.
// Holder A's float32 output is float(code - zp_a) * scale_a bit for bit, so it takes at most 256 values; an elementwise f maps
// each value by itself and holder B codes each element by itself, so B's code is a function of A's code.  The host builds the
// table by running the replaced call itself on the 256 dequantized values (ops.code_table), in the order of the RAW byte -- an
// int8 code c sits at entry (uint8)c -- so the kernel needs no sign flip and the code types only name the launch.
//
// Form: flat over n bytes, any n >= 0 (no shape, no channel count).  A workgroup of 256 lanes covers CH * 256 chunks of 16 bytes
// (CH = 4 by default: 16 KiB; tuning key "table_chunks" 1, 2, 4), chunk u of a lane kThreads chunks behind chunk u - 1, so a wave's
// accesses are 1 KiB straight runs.  A lane issues the load of one table dword (64 lanes hold the table; each of the four waves loads
// and writes the same 64 dwords, so that no branch stands between the loads and the wait) and then all CH of its 16-byte data loads,
// a chunk index beyond the end clamped to the last chunk (loaded again, not stored); vector loads return in order, so the table
// dword is written to LDS and the workgroup's one barrier passed while the data loads are still in flight; then 16 byte reads of
// LDS per chunk and one 16-byte store per chunk, plain (a product reads the output next).  The n % 16 tail bytes are read and
// written byte by byte by lane 0 of block 0 (n < 16: by a launch of one wave).  No byte outside [out, out + n) is written, none
// outside [in, in + n) read.
//
// LDS: 256 B per workgroup.  The table covers each of the 32 banks twice (bank = (address / 4) mod 32), lanes that read the same
// dword are served by one broadcast: a byte read meets at most a 2-way conflict.  Measurements: docs/KERNEL_NOTES.md.
#include "mctq_consumer.hpp"               // u32x4, CodeForm, form_check_dtype, ranges_overlap

namespace mctq {

extern int g_table_chunks;                 // tuning key "table_chunks" (mctq_misc.hip): 16-byte chunks per lane, 1, 2 or 4

// the n % 16 bytes behind the last chunk, by one lane (lut8: the table in LDS, behind the barrier)
__device__ __forceinline__ void table_tail(const uint8_t* __restrict__ lut8, const uint8_t* __restrict__ in8, uint8_t* __restrict__ out8,
                                           uint32_t tail) {
#pragma clang loop vectorize(disable) unroll(disable)
  for (uint32_t j = 0; j < tail; ++j) out8[j] = lut8[in8[j]];
}

// chunks >= 1
template <int CH>
__global__ __launch_bounds__(kThreads) void codes_table_kernel(const u32x4* in, u32x4* __restrict__ out,
                                                               const uint32_t* __restrict__ table, uint32_t chunks, uint32_t tail) {
  __shared__ uint32_t lut[64];
  const uint8_t* __restrict__ lut8 = reinterpret_cast<const uint8_t*>(lut);
  const uint32_t first = blockIdx.x * (uint32_t)(kThreads * CH) + threadIdx.x;        // < 2^31 + kThreads * CH: the launcher checks the chunk count
  const uint32_t t = table[threadIdx.x & 63u];                                      // a wave: entries 4 * lane .. 4 * lane + 3
  u32x4 v[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) v[u] = in[min(first + u * kThreads, chunks - 1)];    // beyond the end: the last chunk again, not stored
  // Every load is issued before the first lookup.  (`in` is not __restrict__ and the empty asm may touch memory: otherwise the
  // compiler moves a guarded chunk's load below the barrier, next to its store, and the table's latency is paid in front of it.)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  lut[threadIdx.x & 63u] = t;                                                       // (the four waves write the same 64 dwords)
  __syncthreads();
  u32x4 r[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t w = v[u][q];
      r[u][q] = (uint32_t)lut8[w & 0xffu] | ((uint32_t)lut8[(w >> 8) & 0xffu] << 8) | ((uint32_t)lut8[(w >> 16) & 0xffu] << 16)
              | ((uint32_t)lut8[w >> 24] << 24);
    }
  // whole workgroups store unguarded, behind one uniform branch; the last one guards each chunk
  if ((blockIdx.x + 1) * (uint32_t)(kThreads * CH) <= chunks) {
#pragma unroll
    for (int u = 0; u < CH; ++u) out[first + u * kThreads] = r[u];
  } else {
#pragma unroll
    for (int u = 0; u < CH; ++u)
      if (first + u * kThreads < chunks) out[first + u * kThreads] = r[u];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && tail != 0)
    table_tail(lut8, reinterpret_cast<const uint8_t*>(in + chunks), reinterpret_cast<uint8_t*>(out + chunks), tail);
}

// n < 16: the tail alone, one wave
__global__ __launch_bounds__(64) void codes_table_tail_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                              const uint32_t* __restrict__ table, uint32_t tail) {
  __shared__ uint32_t lut[64];
  lut[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) table_tail(reinterpret_cast<const uint8_t*>(lut), in, out, tail);
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_table(const void* in, int32_t in_code_dtype, void* out, int32_t out_code_dtype, int64_t n, const void* table,
                     void* stream) {
  if (n < 0) return fail_arg("n < 0");
  if (int rc = form_check_dtype(in_code_dtype, "in_code_dtype")) return rc;
  if (int rc = form_check_dtype(out_code_dtype, "out_code_dtype")) return rc;
  if (n == 0) return 0;
  const int64_t chunks = n / 16;
  // a lane's chunk index is a 31-bit number (beyond it: split the tensor)
  if (chunks > INT32_MAX) return fail_arg("more than 2^31 - 1 16-byte chunks in one launch");
  if (!in) return fail_arg("in is NULL");
  if (!out) return fail_arg("out is NULL");
  if (!table) return fail_arg("table is NULL");
  if (((uintptr_t)in & 15u) != 0) return fail_arg("in must be 16-byte aligned");
  if (((uintptr_t)out & 15u) != 0) return fail_arg("out must be 16-byte aligned");
  if (((uintptr_t)table & 3u) != 0) return fail_arg("table must be 4-byte aligned");
  // the byte ranges: a lane would read codes (or table entries) another lane has overwritten
  if (ranges_overlap(out, (size_t)n, in, (size_t)n)) return fail_arg("out overlaps in");
  if (ranges_overlap(out, (size_t)n, table, 256u)) return fail_arg("out overlaps table");
  const int ch = g_table_chunks;
  const int64_t per_block = (int64_t)kThreads * ch;
  int64_t blocks = (chunks + per_block - 1) / per_block;                             // <= 2^23
  if (blocks == 0) blocks = 1;                                                       // n < 16: the tail alone
  const u32x4* src = static_cast<const u32x4*>(in);
  u32x4* dst = static_cast<u32x4*>(out);
  const uint32_t* tab = static_cast<const uint32_t*>(table);
  const uint32_t nc = (uint32_t)chunks, tail = (uint32_t)(n % 16);
  const hipStream_t s = (hipStream_t)stream;
  if (nc == 0) hipLaunchKernelGGL(codes_table_tail_kernel, dim3(1), dim3(64), 0, s, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), tab, tail);
  else if (ch == 1) hipLaunchKernelGGL(codes_table_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, s, src, dst, tab, nc, tail);
  else if (ch == 2) hipLaunchKernelGGL(codes_table_kernel<2>, dim3((unsigned)blocks), dim3(kThreads), 0, s, src, dst, tab, nc, tail);
  else hipLaunchKernelGGL(codes_table_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, s, src, dst, tab, nc, tail);
  static thread_local char op_text[40];
  snprintf(op_text, sizeof(op_text), "%s -> %s blocks=%u", code_form(in_code_dtype).is_signed ? "i8" : "u8",
           code_form(out_code_dtype).is_signed ? "i8" : "u8", (unsigned)blocks);
  note_launch("codes_table", op_text, ch, 0, 1, 1);
  return check_launch("mctq_codes_table");
}

}  // extern "C"
