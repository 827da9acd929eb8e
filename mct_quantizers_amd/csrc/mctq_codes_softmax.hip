// mctq_codes_softmax.hip -- part of libmctq_hip.so (C ABI: include/mctq_hip.h).
//
// Softmax over the rows of a code tensor, between two activation holders A and B: A-codes c_j (j < L) -> B-codes, defined on
// integers so that the result does not depend on the order of the sum.  Per row
//     c_j    = pre ? pre[raw_j] : raw_j                      an optional 256-entry byte table folds an elementwise prefix
//     cmax   = max_j c_j,  d_j = cmax - c_j                  in 0 .. 255; A's zero point cancels
//     S      = sum_j E[d_j]                                  E[d] = rint(exp(-d * s_a) * 2^24), uint32, built by the host in float64
//     p_j    = float32(E[d_j]) / float32(S)                  E <= 2^24 converts exactly, S <= 2^39 rounds once; one IEEE division
//     code_j = ql_code(p_j)                                  clamp(rint(p_j * (1 / s_b)) + zp_b, qmin, qmax)
// S is an integer and integer addition is associative: both forms below, any split over lanes, and the torch route of
// ops.codes_softmax give the same bytes.
//
// Rows start at any byte (a ViT's rows are 197 bytes), so a row is read as the 16-byte-aligned chunks that cover it: chunk k of
// row r is the aligned chunk (r * in_pitch) / 16 + k of the buffer.  Bytes of a chunk outside the row take no part: they count
// as the least code in the max and add 0 to the sum.  Every chunk address is clamped into the buffer (a clamped chunk is all
// outside the row); the buffer's last chunk, where the buffer does not fill it, is read byte by byte.  The row is read once,
// kept in registers (CH chunks per lane: 4 * CH dwords) through the three passes -- max, sum, codes -- and written once.
//
// Wave form: one wave per row, four rows per workgroup of 256 lanes, lane l on chunks l, l + 64, .. (CH = 1, 2, 4: windows of at
// most 4096 bytes).  The max and the sum cross the wave by __shfl_xor; the lane sums are u32 (at most 64 elements a lane,
// 64 * 2^24 < 2^32) and cross the wave as u64.  Block form: one workgroup per row, lane l on chunks l, l + 256, .. (CH = 1, 2, 4,
// 8: at most 32768 bytes); the four waves' maxima and sums meet in LDS.  Both tables live in LDS (1 KiB + 256 B); their loads and
// all of a lane's data loads are issued before the first barrier, as in mctq_codes_table.hip.
//
// Output: row r is written at out + r * out_pitch, L codes and then pad_code up to out_pitch (the padded rows the integer
// product reads).  Where input and output rows sit alike within their 16-byte chunks -- always, unless the two pitches differ
// -- the lane's chunk of codes is the output chunk.  Otherwise the wave form builds output chunk m from the code chunks of two
// neighbouring lanes (one __shfl of four dwords and a funnel shift by (in - out) mod 16 bytes) and the block form stores its
// codes byte by byte.  An output chunk that lies wholly inside the row's out_pitch bytes is one 16-byte store; the first and the
// last chunk, where a neighbouring row shares them, are stored byte by byte.  No byte outside [out + r * out_pitch, + out_pitch)
// is written by row r's lanes.
#include "mctq_codes_softmax.hpp"          // the three passes over one chunk; u32x4, QlOut, form_check_dtype, ranges_overlap

namespace mctq {

extern int g_softmax_form;                 // tuning key "softmax_form" (mctq_misc.hip): 0 = auto, 1 = wave form, 2 = block form

constexpr int kSoftmaxWaveSlots = 256;     // 16-byte chunks of one row: wave form (64 lanes x 4), block form (256 lanes x 8)
constexpr int kSoftmaxBlockSlots = 2048;

struct SoftmaxArgs {
  const uint8_t* in;
  uint8_t* out;
  const uint32_t* etab;                    // E[256]
  const uint32_t* pre;                     // the pre-table as 64 dwords, or nullptr
  uint32_t rows, L, in_pitch, out_pitch;
  uint32_t total;                          // (rows - 1) * in_pitch + L: the bytes of `in` that may be read
  uint32_t flip;                           // 0x80 for int8 codes (c ^ 0x80 orders them as unsigned bytes), 0 for uint8
  uint32_t pad;                            // pad_code in all four bytes
  QlOut o;
};

// aligned chunk gc of the buffer; the last one byte by byte where the buffer ends inside it
__device__ __forceinline__ u32x4 softmax_load(const uint8_t* in, uint32_t gc, uint32_t total) {
  if (gc * 16u + 16u <= total) return reinterpret_cast<const u32x4*>(in)[gc];
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j)                                                    // (constant indices: the chunk stays in registers)
    if (gc * 16u + (uint32_t)j < total) v[j >> 2] |= (uint32_t)in[gc * 16u + (uint32_t)j] << (8 * (j & 3));
  return v;
}

// The 16 bytes that start dl (0 .. 15) bytes into the eight dwords lo, hi: the dword part of the shift by two rounds of selects
// between named values (an array indexed by dl / 4, or a switch over it, is kept in LDS by the compiler: 6 - 15 KiB a workgroup),
// the byte part by one 64-bit shift per dword.
__device__ __forceinline__ uint32_t softmax_shift(uint32_t high, uint32_t low, uint32_t bytes) {
  return (uint32_t)(((((uint64_t)high) << 32) | low) >> (8u * bytes));
}
__device__ __forceinline__ u32x4 softmax_funnel(const u32x4& lo, const u32x4& hi, uint32_t dl) {
  const bool one = (dl & 4u) != 0, two = (dl & 8u) != 0;
  const uint32_t a0 = one ? lo[1] : lo[0], a1 = one ? lo[2] : lo[1], a2 = one ? lo[3] : lo[2], a3 = one ? hi[0] : lo[3];
  const uint32_t a4 = one ? hi[1] : hi[0], a5 = one ? hi[2] : hi[1], a6 = one ? hi[3] : hi[2];
  const uint32_t b0 = two ? a2 : a0, b1 = two ? a3 : a1, b2 = two ? a4 : a2, b3 = two ? a5 : a3, b4 = two ? a6 : a4;
  const uint32_t db = dl & 3u;
  return u32x4{softmax_shift(b1, b0, db), softmax_shift(b2, b1, db), softmax_shift(b3, b2, db), softmax_shift(b4, b3, db)};
}

// Output chunk m of the row at byte t of `out` (ob = t % 16): the codes of elements e0 .. e0 + 15, e0 = 16 m - ob; elements in
// [0, L) are codes, in [L, out_pitch) pad_code, all others are another row's.
__device__ __forceinline__ void softmax_store(const SoftmaxArgs& a, uint32_t t, uint32_t ob, uint32_t m, const u32x4& codes) {
  const int e0 = 16 * (int)m - (int)ob, L = (int)a.L, width = (int)a.out_pitch;
  if (e0 + 16 <= 0 || e0 >= width) return;
  uint8_t* dst = a.out + (t - ob) + 16u * m;
  if (e0 >= 0 && e0 + 16 <= width) {
    const int nv = min(max(L - e0, 0), 16);                                       // leading bytes that are codes
    *reinterpret_cast<u32x4*>(dst) = softmax_chunk_pad(codes, nv, a.pad);
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int e = e0 + j;
    if (e >= 0 && e < width) dst[j] = (uint8_t)(e < L ? (codes[j >> 2] >> (8 * (j & 3))) : a.pad);
  }
}

// rows >= 1, L >= 1; CH * (BLOCK ? 256 : 64) chunks cover every row's window (the launcher's count)
template <int CH, bool BLOCK, bool PRE>
__global__ __launch_bounds__(kThreads) void codes_softmax_kernel(SoftmaxArgs a) {
  constexpr uint32_t LANES = BLOCK ? (uint32_t)kThreads : 64u;
  __shared__ uint32_t etab[256];
  __shared__ uint32_t pre[64];
  __shared__ uint32_t wave_max[4];
  __shared__ unsigned long long wave_sum[4];
  const uint8_t* __restrict__ pre8 = reinterpret_cast<const uint8_t*>(pre);
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = BLOCK ? tid : (tid & 63u);
  const uint32_t own = BLOCK ? blockIdx.x : blockIdx.x * 4u + wave;
  const bool active = own < a.rows;                                               // (uniform over a wave)
  const uint32_t row = active ? own : a.rows - 1u;                                // an idle wave reads the last row and stores nothing
  const uint32_t s = row * a.in_pitch, t = row * a.out_pitch;                     // < 2^31: the launcher checks the byte counts
  const uint32_t ia = s & 15u, ob = t & 15u;
  // wave form, rows that sit later in their output chunk than in their input chunk: lane l takes input chunk l - 1, so that
  // output chunk m is always made of the code chunks of lanes m and m + 1
  const uint32_t sh = (!BLOCK && ia < ob) ? 1u : 0u;
  const int c0 = (int)(s >> 4), last = (int)((a.total - 1u) >> 4);
  const uint32_t te = a.etab[tid];
  uint32_t tp = 0;
  if (PRE) tp = a.pre[tid & 63u];
  u32x4 v[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int k = (int)(lane + (uint32_t)u * LANES) - (int)sh;
    v[u] = softmax_load(a.in, (uint32_t)min(max(c0 + k, 0), last), a.total);
  }
  // every load is issued before the barrier (mctq_codes_table.hip)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  etab[tid] = te;
  if (PRE) pre[tid & 63u] = tp;                                                   // (the four waves write the same 64 dwords)
  __syncthreads();

  // pass 1: the codes as unsigned bytes (pre-table, sign flip), bytes outside the row 0; the lane's max
  uint32_t mx = 0;
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int k = (int)(lane + (uint32_t)u * LANES) - (int)sh;
    const int lo = (int)ia - 16 * k, hi = (int)(ia + a.L) - 16 * k;               // byte j of the chunk is element j - lo: lo <= j < hi
    softmax_chunk_order<PRE>(v[u], pre8, a.flip, lo, hi, mx);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
  if (BLOCK) {
    if ((tid & 63u) == 0) wave_max[wave] = mx;
    __syncthreads();
    mx = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
  }

  // pass 2: the lane's sum of E[cmax - c] (at most 128 elements a lane: 128 * 2^24 < 2^32), then the row's as u64
  uint32_t part = 0;
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int k = (int)(lane + (uint32_t)u * LANES) - (int)sh;
    const int lo = (int)ia - 16 * k, hi = (int)(ia + a.L) - 16 * k;
    part += softmax_chunk_sum(v[u], etab, mx, lo, hi);
  }
  unsigned long long sum = part;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if (BLOCK) {
    if ((tid & 63u) == 0) wave_sum[wave] = sum;
    __syncthreads();
    sum = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
  }
  const float fs = (float)sum;                                                    // >= 2^24: the row's max adds E[0]

  // pass 3: one division per element, 16 codes per chunk (bytes outside the row: some code, never stored)
  u32x4 r[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) r[u] = softmax_chunk_codes(v[u], etab, mx, fs, a.o);
  if (!active) return;

  if (ia == ob) {                                                                 // the code chunks are the output chunks
#pragma unroll
    for (int u = 0; u < CH; ++u) softmax_store(a, t, ob, lane + (uint32_t)u * LANES, r[u]);
  } else if (!BLOCK) {
    // output chunk m = 16 bytes from dl bytes into the code chunks of lanes m and m + 1 (slot 64 u + 63: lane 0 of slot u + 1)
    const uint32_t dl = (ia - ob) & 15u;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      u32x4 hi;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t next = (uint32_t)__shfl((int)r[u][q], (int)((lane + 1u) & 63u));
        const uint32_t wrap = u + 1 < CH ? (uint32_t)__shfl((int)r[u + 1 < CH ? u + 1 : u][q], 0) : 0u;
        hi[q] = lane == 63u ? wrap : next;
      }
      softmax_store(a, t, ob, lane + (uint32_t)u * LANES, softmax_funnel(r[u], hi, dl));
    }
  } else {
    // block form, rows that sit differently in their input and output chunks: byte stores, the pad by the lane of the row's end
    uint8_t* __restrict__ dst = a.out + t;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int k = (int)(lane + (uint32_t)u * LANES);
      const int lo = (int)ia - 16 * k, hi = (int)(ia + a.L) - 16 * k;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j >= lo && j < hi) dst[j - lo] = (uint8_t)(r[u][j >> 2] >> (8 * (j & 3)));
      if (hi >= 1 && hi <= 16)
        for (uint32_t e = a.L; e < a.out_pitch; ++e) dst[e] = (uint8_t)a.pad;
    }
  }
}

template <bool BLOCK, bool PRE>
static void softmax_launch(int ch, unsigned blocks, hipStream_t s, const SoftmaxArgs& a) {
  if (ch == 1) hipLaunchKernelGGL((codes_softmax_kernel<1, BLOCK, PRE>), dim3(blocks), dim3(kThreads), 0, s, a);
  else if (ch == 2) hipLaunchKernelGGL((codes_softmax_kernel<2, BLOCK, PRE>), dim3(blocks), dim3(kThreads), 0, s, a);
  else if (ch == 4) hipLaunchKernelGGL((codes_softmax_kernel<4, BLOCK, PRE>), dim3(blocks), dim3(kThreads), 0, s, a);
  else if constexpr (BLOCK) hipLaunchKernelGGL((codes_softmax_kernel<8, true, PRE>), dim3(blocks), dim3(kThreads), 0, s, a);
}

}  // namespace mctq

using namespace mctq;

extern "C" {

int mctq_codes_softmax(const void* in, int32_t in_code_dtype, void* out, int32_t out_code_dtype, float out_scale,
                       int32_t out_zero_point, int32_t out_quant_min, int32_t out_quant_max, int64_t rows, int64_t length,
                       int64_t in_pitch, int64_t out_pitch, int32_t pad_code, const void* exp_table, const void* pre_table,
                       void* stream) {
  if (rows < 0 || length < 0) return fail_arg("negative extent");
  if (int rc = form_check_dtype(in_code_dtype, "in_code_dtype")) return rc;
  if (int rc = form_check_dtype(out_code_dtype, "out_code_dtype")) return rc;
  if (int rc = form_check_scale(out_scale, "out_scale")) return rc;
  if (int rc = form_check_zero_point(out_code_dtype, pad_code, "pad_code", "the output's type")) return rc;
  QlOut o;
  if (int rc = ql_output_form(o, out_code_dtype, out_scale, out_zero_point, out_quant_min, out_quant_max)) return rc;
  if (in_pitch < length || out_pitch < length) return fail_arg("in_pitch and out_pitch must be at least the row length");
  if (rows == 0 || length == 0) return 0;
  // a lane's byte offset is a 31-bit number (beyond it: split the rows)
  if (rows > INT32_MAX / in_pitch || rows > INT32_MAX / out_pitch) return fail_arg("more than 2^31 - 1 bytes in one launch");
  if (!in) return fail_arg("in is NULL");
  if (!out) return fail_arg("out is NULL");
  if (!exp_table) return fail_arg("exp_table is NULL");
  if (((uintptr_t)in & 15u) != 0) return fail_arg("in must be 16-byte aligned");
  if (((uintptr_t)out & 15u) != 0) return fail_arg("out must be 16-byte aligned");
  if (((uintptr_t)exp_table & 3u) != 0 || ((uintptr_t)pre_table & 3u) != 0) return fail_arg("the tables must be 4-byte aligned");
  const size_t in_bytes = (size_t)((rows - 1) * in_pitch + length), out_bytes = (size_t)(rows * out_pitch);
  if (ranges_overlap(out, out_bytes, in, in_bytes)) return fail_arg("out overlaps in");
  if (ranges_overlap(out, out_bytes, exp_table, 1024u)) return fail_arg("out overlaps exp_table");
  if (pre_table && ranges_overlap(out, out_bytes, pre_table, 256u)) return fail_arg("out overlaps pre_table");
  // the 16-byte chunks that cover any row's input window and output row; rows that all start on a chunk need no slack
  const bool aligned = in_pitch % 16 == 0 && out_pitch % 16 == 0;
  const int64_t slots = aligned ? (out_pitch + 15) / 16 : (out_pitch + 30) / 16 + 1;
  if (slots > kSoftmaxBlockSlots) return fail_arg("a row of more than 32768 bytes (with its alignment slack)");
  // Auto: the wave form wherever it fits.  Measured (one MI355X; tools/softmax_consumer_probe.py, table in profiles/EXPERIMENTS.md)
  // on six rows where both fit: the wave form won four (3.3 - 3.5 x at batch 64 on 12 x 197^2, 12 x 128^2, 12 x 384^2; 1.6 x on
  // 12 x 384^2 at batch 1) and tied the two small batch-1 launches (12 x 128^2: 10.1 against 10.2 us; 12 x 197^2: 10.6 against
  // 11.4 us); the block form won none.
  const bool block = slots > kSoftmaxWaveSlots || g_softmax_form == 2;
  const int64_t lanes = block ? kThreads : 64;
  int ch = 1;
  while (ch * lanes < slots) ch *= 2;
  SoftmaxArgs a;
  a.in = static_cast<const uint8_t*>(in);
  a.out = static_cast<uint8_t*>(out);
  a.etab = static_cast<const uint32_t*>(exp_table);
  a.pre = static_cast<const uint32_t*>(pre_table);
  a.rows = (uint32_t)rows; a.L = (uint32_t)length; a.in_pitch = (uint32_t)in_pitch; a.out_pitch = (uint32_t)out_pitch;
  a.total = (uint32_t)in_bytes;
  a.flip = in_code_dtype == MCTQ_CODE_I8 ? 0x80u : 0u;
  a.pad = ((uint32_t)pad_code & 0xffu) * 0x01010101u;
  a.o = o;
  const unsigned blocks = (unsigned)(block ? rows : (rows + 3) / 4);
  const hipStream_t s = (hipStream_t)stream;
  if (block) { if (pre_table) softmax_launch<true, true>(ch, blocks, s, a); else softmax_launch<true, false>(ch, blocks, s, a); }
  else { if (pre_table) softmax_launch<false, true>(ch, blocks, s, a); else softmax_launch<false, false>(ch, blocks, s, a); }
  static thread_local char op_text[48];
  snprintf(op_text, sizeof(op_text), "%s -> %s %s%s", in_code_dtype == MCTQ_CODE_I8 ? "i8" : "u8",
           out_code_dtype == MCTQ_CODE_I8 ? "i8" : "u8", block ? "block" : "wave", pre_table ? " pre" : "");
  note_launch("codes_softmax", op_text, ch, 0, 1, 1);
  return check_launch("mctq_codes_softmax");
}

}  // extern "C"
