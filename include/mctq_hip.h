/*
 * mctq_hip.h -- C ABI of libmctq_hip.so, the MI355X (gfx950) implementation of the
 * sony/mct_quantizers PyTorch inferable-quantizer hot path.
 *
 * Every entry point replaces one tensor-runtime call site of the reference
 * (paths relative to /root/reference/mct_quantizers/):
 *
 *   mctq_fq_per_tensor_f32    torch.fake_quantize_per_tensor_affine at
 *                             pytorch/quantizers/weights_inferable_quantizers/weights_symmetric_inferable_quantizer.py:147
 *                             .../weights_uniform_inferable_quantizer.py:161
 *                             pytorch/quantizers/activation_inferable_quantizers/activation_symmetric_inferable_quantizer.py:113
 *                             .../activation_uniform_inferable_quantizer.py:124
 *   mctq_fq_per_channel_f32   torch.fake_quantize_per_channel_affine at
 *                             .../weights_symmetric_inferable_quantizer.py:139, .../weights_uniform_inferable_quantizer.py:153
 *   mctq_lut_per_tensor_f32   lut_quantizer (pytorch/quantizer_utils.py:95-139) with a scalar threshold, called from
 *                             .../activation_lut_pot_inferable_quantizer.py:86 and
 *                             .../weights_lut_symmetric_inferable_quantizer.py:114 (per_channel=False)
 *   mctq_lut_per_channel_f32  lut_quantizer with a per-channel threshold, .../weights_lut_symmetric_inferable_quantizer.py:114
 *   mctq_grid_per_*_f32       the export-time functions quantize_*_torch behind `_use_custom_impl and
 *                             torch.jit.is_tracing()` (file:line at the declarations below)
 *   (dtype-generic forms, the decision-table LUT entry points and the extensions -- integer codes, the integer
 *    consumer mctq_qlinear_* and the patch matrix mctq_codes_im2col_nhwc that feeds it convolutions -- are documented
 *    at their declarations; extensions have no reference call site)
 *
 * Conventions
 *   - x, y, scales, zero_points, thresholds and lut are DEVICE pointers owned by the caller
 *     (torch's caching allocator); the library never allocates, frees, copies or synchronises.
 *   - Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *     the call returns immediately; it is legal inside hipGraph stream capture.
 *   - A tensor is addressed in its dense storage order as [outer][channels][inner], float32.
 *     The channel of linear element i is (i / inner) % channels.
 *   - Return value: 0 on success, a negative hipError_t on a HIP failure, MCTQ_E_ARG (-10001)
 *     on an invalid argument.  mctq_last_error() gives the message for the calling thread.
 *   - Arithmetic contract (bit exact with the reference on finite inputs, |x/scale| < 2^31):
 *       affine: inv = 1.0f/scale (correctly rounded); q = clamp(rint(x*inv) + zp, qmin, qmax);
 *               y = (q - zp) * scale           rint = round-half-to-even
 *       lut   : t = clamp((x / thr_div) * mult, clip_min, clip_max)  (true IEEE division, NaN kept);
 *               j = first index minimising fl32(|t - lut[j]|); y = (lut[j] / mult) * thr_mul
 *     Outside that domain the kernels saturate: +inf -> qmax, -inf and NaN -> qmin.
 */
#ifndef MCTQ_HIP_H
#define MCTQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v8 (round 5): the compact-decision-table entry points (mctq_lut_compact_words, mctq_lut_build_compact, mctq_lutc_*) and the
 * tuning keys "heavy_persistent", "nt" = 0, "unroll" / "heavy_unroll" = 8 and the experiment codes of "ql_variant" left the
 * library with the kernels behind them (measured, not adopted: tools/experiments/); nothing else changed. */
/* Size limit (since v8): a tensor of more than 2^32 - 8192 elements whose per-channel rows are shorter than 256 lane-vectors is
 * taken in ONE launch by the affine fake-quantizers only (16-byte aligned x / y); the LUT, integer-code and export-grid entry
 * points return MCTQ_E_ARG for it ("per-channel rows shorter than 256 lane-vectors above 2^32 elements: affine quantizers
 * only") -- the Python layer (hip/ops.py: _split_rows) cuts such a tensor into row blocks below the limit and issues one launch
 * per block, which is what a caller of the C ABI has to do as well.  Long rows and per-tensor launches have no such limit. */
/* v9 (round 6): + mctq_selftest_reciprocal, + tuning keys "shortrows", "paced"; the channel-last (lastaxis) launch and the new launch of
 * short / ragged per-channel rows (shortrows) invert a lane's own scales with a five-instruction exact reciprocal (no signature
 * changed; results are bit-identical). */
/* v10: + codebook-index codes of the LUT quantizers and their decode (mctq_lut_build_index_table, mctq_lut_codes_per_tensor /
 * _per_channel, mctq_lut_decode_per_tensor / _per_channel); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_im2col_nhwc, the patch matrix of NHWC activation codes that lets k x k,
 * strided, padded and dilated convolutions run on the integer consumer; no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_qconv_dw_i8, the depthwise convolution on NHWC activation codes (the layer between
 * the two pointwise convolutions of a MobileNet-style block); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_fq_join_f32, the residual add, the ReLU and both outputs of a shared activation
 * holder (fake-quantized float32 and integer codes) in one pass; no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_fq_join_rc_f32, the join with its residual operand given as the int8 / uint8 codes
 * of another join (identity branches that stay on codes); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_maxpool_nhwc, torch.nn.MaxPool2d on NHWC activation codes (a max pool between
 * an activation holder and the integer consumers behind it stays on codes); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_qlinear_i8_res, the integer product with the residual add and the ReLU of a residual
 * join in its epilogue (the block's last convolution emits the next block's codes itself); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_concat_nhwc, torch.cat along the channels on NHWC activation codes in the
 * form of the holder behind it (Inception / Fire / skip-connection blocks stay on codes), + tuning key "concat_copy"; no existing
 * signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_avgpool_nhwc, torch.nn.AvgPool2d / global average pooling on NHWC activation
 * codes in the form of the holder behind the pool (classifier heads and SE squeezes stay on codes), + tuning key "avgpool_form"; no
 * existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_mul_nhwc, torch.mul of two holder outputs on NHWC activation codes in the
 * form of the holder behind it, the second operand same-shape codes, row-broadcast codes or row-broadcast float32 values (the
 * multiply of a squeeze-and-excitation block and gated layers stay on codes); no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_qlinear_i8_act and mctq_qconv_dw_i8_act, the integer product and the depthwise
 * convolution with a Hardswish / Hardsigmoid in front of the codes they emit (MobileNetV3's layers and the SE gate stay on codes); no
 * existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_upsample_nhwc, nearest upsampling (torch.nn.Upsample / F.interpolate,
 * modes "nearest" and "nearest-exact") on NHWC activation codes in the form of the holder behind it (decoder stages, necks and
 * segmentation heads stay on codes), + tuning key "upsample_form"; no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_im2col_pad_nhwc, the patch matrix for any channel count with rows padded
 * to whole 16-byte chunks (the integer consumers then take layers whose K is no multiple of 16: a CNN's stem, bottleneck widths of
 * 24 / 40 / 72, SE squeeze widths), + tuning key "im2col_grain"; no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_codes_table, an elementwise function between two activation holders as a
 * 256-entry byte table on codes (sigmoid, SiLU, GELU, tanh and the other smooth activations stay on codes), + tuning key
 * "table_chunks"; no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_qconv_grouped_i8, the grouped convolution on NHWC activation codes as a direct
 * convolution on the integer matrix cores (the 3 x 3 layer of a ResNeXt / RegNet bottleneck stays on codes); no existing signature or
 * result changed. */
/* v10 (additive, the version number stays): + mctq_qconv_transposed_i8, the transposed convolution on NHWC activation codes as
 * one stride-1 correlation per output phase on the integer matrix cores (the learned upsampling of a decoder stage stays on codes);
 * no existing signature or result changed. */
/* v10 (additive, the version number stays): + mctq_qmatmul_i8, the batched product of two activation-code tensors by strides on
 * the integer matrix cores (the Q.K^T and P.V products of an attention block stay on codes); no existing signature or result
 * changed. */
#define MCTQ_ABI_VERSION 10
#define MCTQ_E_ARG (-10001)

/* storage types of x (and of y for the affine entry points); arithmetic is always float32 */
#define MCTQ_DT_F32 0
#define MCTQ_DT_F16 1
#define MCTQ_DT_BF16 2
#define MCTQ_DT_F64 3   /* float64 tensors: ATen's double arithmetic, see "float64" below */

/* storage types of the integer-code outputs */
#define MCTQ_CODE_I8 0
#define MCTQ_CODE_U8 1
#define MCTQ_CODE_I4 2   /* two codes per byte: element 2j in the low nibble, 2j+1 in the high one */
#define MCTQ_CODE_U4 3

/* ABI version of the loaded library (== MCTQ_ABI_VERSION it was built with). */
int mctq_abi_version(void);

/* Content hash of the sources, headers and compiler flags this binary was built from (hip/build.py: tree_build_id()):
 * the loader refuses a library whose id differs from the tree's, so a stale binary cannot be used silently. */
const char* mctq_build_id(void);

/* Message of the last failing call on this thread ("" if none). */
const char* mctq_last_error(void);

/* Diagnostic: which kernel variant the calling thread's last successful elementwise launch used, e.g.
 * "rows_kernel<AffineOp,in4B,out4B,U=4,NT=1>" ("" before the first launch).  Benchmarks use it to tie profiler
 * counters (profiles/pmc_traffic.json) to the variant they were measured on.  Valid until the next call.
 * With MCTQ_LAUNCH_LOG=<file> in the environment when the library is loaded, every variant is also appended to that file
 * the first time the process takes it (the evidence the set of instantiated kernels was cut against). */
const char* mctq_last_launch(void);

/* Diagnostic: number of kernel launches the library has enqueued from the calling thread since it was loaded (every
 * launch that mctq_last_launch() would name counts once; the one-by-one tail of a batched call counts per tensor).
 * Tests use the difference around a model forward to show how many launches the forward issued: the reference issues
 * one per wrapped weight per forward (pytorch/quantize_wrapper.py:228-240); an accelerated model one per storage type. */
int64_t mctq_launch_count(void);

/* y[i] = (clamp(rint(x[i] * (1/scale)) + zero_point, quant_min, quant_max) - zero_point) * scale, i < n. */
int mctq_fq_per_tensor_f32(const float* x, float* y, int64_t n,
                           float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max,
                           void* stream);

/* Same, with scale/zero point taken per channel: scales[channels] float32, zero_points[channels] int32
 * (zero_points may be NULL, meaning all zero: the symmetric quantizers). */
int mctq_fq_per_channel_f32(const float* x, float* y,
                            int64_t outer, int64_t channels, int64_t inner,
                            const float* scales, const int32_t* zero_points,
                            int32_t quant_min, int32_t quant_max,
                            void* stream);

/*
 * The same two operations for x and y stored as float32, float16 or bfloat16 (dtype = MCTQ_DT_*; y has x's
 * type, as ATen's fake_quantize kernels: float32 arithmetic, one round-to-nearest-even narrowing at the store).
 */
int mctq_fq_per_tensor(const void* x, void* y, int64_t n, int32_t dtype,
                       float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max,
                       void* stream);

int mctq_fq_per_channel(const void* x, void* y,
                        int64_t outer, int64_t channels, int64_t inner, int32_t dtype,
                        const float* scales, const int32_t* zero_points,
                        int32_t quant_min, int32_t quant_max,
                        void* stream);

/*
 * float64 (dtype = MCTQ_DT_F64, accepted by mctq_fq_per_tensor, mctq_fq_per_channel, mctq_fq_per_tensor_tqp,
 * mctq_lut_per_tensor, mctq_lut_per_channel and mctq_lut_per_tensor_f64; the reference passes double tensors
 * straight to ATen at the call sites listed at the top).  ATen's double path is not float32 arithmetic on wider
 * storage, and the package reproduces it as measured against the reference (tests/golden/cases_f64.*):
 *   q = clamp(rint(x * (double)(1.0f / scale)) + zp, qmin, qmax)      double product, double rounding
 *   per tensor (float or tensor qparams):  y = (double)((float)(q - zp) * scale)
 *   per channel:                           y = (double)(q - zp) * (double)scale
 *   LUT: the scaled value, the clip and the distances |t - lut[j]| are evaluated in double, the result
 *        (lut[j] / mult) * thr_mul in float32 -- y is float32.
 */

/*
 * Per-tensor fake-quant whose scale and zero point are 1-element DEVICE arrays (read by the kernel through scalar
 * loads; no device->host copy): the tensor-qparams overload of torch.fake_quantize_per_tensor_affine, called by the
 * per-tensor weights quantizers (weights_symmetric_inferable_quantizer.py:147-151, weights_uniform...py:161-165)
 * and recorded as such by an fx trace of a wrapper (saved-model flow, pytorch/load_model.py:23-34).
 */
int mctq_fq_per_tensor_tqp(const void* x, void* y, int64_t n, int32_t dtype,
                           const float* scale, const int32_t* zero_point, int32_t quant_min, int32_t quant_max,
                           void* stream);

/*
 * A LIST of affine fake-quantizations in one call -- one launch per group of up to 48 tensors of one storage
 * type.  PytorchQuantizationWrapper.forward re-quantizes each wrapped layer's weights on every forward
 * (pytorch/quantize_wrapper.py:228-240); a model has tens of such layers, and each separate launch pays its own
 * host cost and ~2 us of ramp/drain on the GPU.  `items` is a HOST array (it is consumed before the call returns:
 * the descriptors and the block -> tensor map travel in the kernel arguments, so the call is legal under hipGraph
 * capture); every pointer
 * inside an item is a DEVICE pointer with the meaning it has in mctq_fq_per_channel.  Per-tensor quantization is
 * outer = channels = 1, inner = n with 1-element device scales / zero_points and flags = MCTQ_FQ_ITEM_PER_TENSOR.  Tensors the batched kernel cannot
 * take (x or y not 16-byte aligned, >= 2^31 elements, float64, more than 2^20 elements in rows shorter than 32) are
 * launched one by one on the same stream, after the batched launches.
 * All items are validated before anything is launched.
 */
typedef struct mctq_fq_item {
  const void* x;
  void* y;
  int64_t outer, channels, inner;
  const float* scales;           /* device float32[channels] */
  const int32_t* zero_points;    /* device int32[channels], or NULL = all zero */
  int32_t quant_min, quant_max;
  int32_t dtype;                 /* MCTQ_DT_*: storage type of x and y */
  int32_t flags;                 /* MCTQ_FQ_ITEM_PER_TENSOR or 0 */
} mctq_fq_item;

/* The item is a per-tensor quantization (torch.fake_quantize_per_tensor_affine with tensor qparams), not a
 * per-channel one that happens to have one channel.  Only float64 tensors can tell the difference (see "float64"). */
#define MCTQ_FQ_ITEM_PER_TENSOR 1

int mctq_fq_batched(const mctq_fq_item* items, int32_t n_items, void* stream);

/*
 * The same list as ONE launch per storage type, whatever its length (a whole model's weights): the descriptors are
 * packed on the host into a table whose DEVICE copy the kernel reads by scalar loads.
 *   mctq_fq_batch_pack  writes the table for `items` into host_table (capacity bytes) and returns its size in bytes;
 *                       with host_table == NULL or a capacity that is too small it writes nothing and returns the size
 *                       needed.  Negative: MCTQ_E_ARG.  Pure host code (no HIP call).
 *   mctq_fq_batch_run   launches a packed table: host_table is the packed bytes (launch geometry, and the tensors
 *                       that are launched one by one, are read from it), device_table a 16-byte aligned device copy
 *                       of the same bytes, made and owned by the caller (the library never allocates or copies).
 * The table holds the items' device pointers: pack again (and refresh the device copy) when one of them changes.
 * Results are bit-identical to mctq_fq_batched and to the single-tensor entry points.
 */
int64_t mctq_fq_batch_pack(const mctq_fq_item* items, int32_t n_items, void* host_table, int64_t capacity);
int mctq_fq_batch_run(const void* host_table, const void* device_table, void* stream);

/*
 * The same table-driven launch for LUT quantizers that have a decision table (mctq_lut_build_table): all LUT weights of a
 * model per forward (weights_lut_symmetric_inferable_quantizer.py:114-122 is called once per wrapped layer,
 * quantize_wrapper.py:228-240), or a group of LUT activation batches.  Per-channel items give `thresholds` (device
 * float32[channels]) and `eps`; per-tensor items give thresholds = NULL and the host floats thr_div / thr_mul with the
 * meaning they have in mctq_lutt_per_tensor (step_round likewise).  y is float32.  Items one grid cannot take (x not
 * vector-aligned, >= 2^31 elements, more than 2^20 elements in rows shorter than 32) are launched one by one.
 * Results are bit-identical to mctq_lutt_per_tensor / mctq_lutt_per_channel.
 */
typedef struct mctq_lut_item {
  const void* x;
  float* y;
  int64_t outer, channels, inner;
  const float* thresholds;       /* device float32[channels], or NULL: per tensor */
  const float* table;            /* device decision table, (entries + 1) x 2 words */
  int32_t entries;
  float eps;
  float thr_div, thr_mul;
  float mult, clip_min, clip_max;
  int32_t dtype;                 /* MCTQ_DT_F32 / F16 / BF16: storage type of x */
  int32_t step_round;
} mctq_lut_item;

int64_t mctq_lutt_batch_pack(const mctq_lut_item* items, int32_t n_items, void* host_table, int64_t capacity);
int mctq_lutt_batch_run(const void* host_table, const void* device_table, void* stream);

/*
 * Integer-code output of the affine quantizers: codes[i] = clamp(rint(x[i] * (1/scale)) + zero_point, quant_min,
 * quant_max), stored as int8 (MCTQ_CODE_I8, domain within [-128, 127]) or uint8 (MCTQ_CODE_U8, within [0, 255]).
 * (codes - zero_point) * scale equals the fake-quantized value of mctq_fq_* bit for bit.  This is the
 * "integer domain" the reference never materialises; consumers that dequantize inside their GEMM
 * read 1 B per element instead of 4.
 * MCTQ_CODE_I4 (domain within [-8, 7], two's-complement nibbles) / MCTQ_CODE_U4 (within [0, 15]): two codes per
 * byte in storage order, element 2j in the low nibble and 2j + 1 in the high nibble; `codes` then holds n / 2
 * bytes (4-byte aligned).  Supported layouts: per tensor with n % 8 == 0; per channel with inner % 8 == 0, or
 * inner == 1 with channels % 8 == 0; anything else returns MCTQ_E_ARG.  mctq_last_launch names these launches
 * "codes4_flat_kernel", "codes4_rows_kernel" (U = the 4 or 8 lane vectors per lane chosen for the row length) and
 * "codes4_lastaxis_kernel", op "AffineCodesOp", out1B; each counts once in mctq_launch_count.
 */
int mctq_fq_codes_per_tensor(const void* x, void* codes, int64_t n, int32_t dtype, int32_t code_dtype,
                             float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max,
                             void* stream);

int mctq_fq_codes_per_channel(const void* x, void* codes,
                              int64_t outer, int64_t channels, int64_t inner, int32_t dtype, int32_t code_dtype,
                              const float* scales, const int32_t* zero_points,
                              int32_t quant_min, int32_t quant_max,
                              void* stream);

/*
 * LUT (codebook) quantizer with one threshold for the whole tensor.
 *   thr_div : float32(threshold + eps), the divisor of quantizer_utils.py:169
 *   thr_mul : float32(threshold), the final multiplier of quantizer_utils.py:137
 *   lut     : device float32[n_lut] codebook in the caller's list order (1 <= n_lut <= 4096)
 *   mult    : 2^(lut_values_bitwidth - signed); clip_min/clip_max: the clamp range of :162-167
 */
int mctq_lut_per_tensor_f32(const float* x, float* y, int64_t n,
                            float thr_div, float thr_mul,
                            const float* lut, int32_t n_lut,
                            float mult, float clip_min, float clip_max,
                            void* stream);

/* LUT quantizer with thresholds[channels] (device float32); the divisor is fl32(thresholds[c] + eps). */
int mctq_lut_per_channel_f32(const float* x, float* y,
                             int64_t outer, int64_t channels, int64_t inner,
                             const float* thresholds, float eps,
                             const float* lut, int32_t n_lut,
                             float mult, float clip_min, float clip_max,
                             void* stream);

/*
 * LUT quantizers for x stored as float32 / float16 / bfloat16 (dtype); y is ALWAYS float32, as the
 * reference's op chain promotes to float32 once the float32 codebook enters (quantizer_utils.py:131-137).
 * step_round (per-tensor only): 0, or MCTQ_DT_F16 / MCTQ_DT_BF16 to round the quotient x/thr_div and the
 * scaled value to that type, which is what the reference's chain does to a half-precision activation
 * divided by a Python-float threshold (activation_lut_pot_inferable_quantizer.py:86-91); thr_div must then
 * already be rounded to that type by the caller.  The literal-scan entry points (mctq_lut_*) accept all four
 * storage types (MCTQ_DT_F64: see "float64"); the decision-table ones (mctq_lutt_*) float32 / float16 / bfloat16.
 */
int mctq_lut_per_tensor(const void* x, float* y, int64_t n, int32_t dtype, int32_t step_round,
                        float thr_div, float thr_mul,
                        const float* lut, int32_t n_lut,
                        float mult, float clip_min, float clip_max,
                        void* stream);

int mctq_lut_per_channel(const void* x, float* y,
                         int64_t outer, int64_t channels, int64_t inner, int32_t dtype,
                         const float* thresholds, float eps,
                         const float* lut, int32_t n_lut,
                         float mult, float clip_min, float clip_max,
                         void* stream);

/* float64 input with a DOUBLE divisor: the activation LUT quantizer divides a double tensor by the Python float
 * threshold + eps (activation_lut_pot_inferable_quantizer.py:86-91), which stays a double; thr_mul = float32(threshold). */
int mctq_lut_per_tensor_f64(const double* x, float* y, int64_t n,
                            double thr_div, float thr_mul,
                            const float* lut, int32_t n_lut,
                            float mult, float clip_min, float clip_max,
                            void* stream);

/*
 * float64 tensors through a sorted threshold list evaluated in DOUBLE (integer codebooks, centres and clip bounds
 * within 2^20): the reference's chain runs quotient, clip and distances in double for a double tensor
 * (quantizer_utils.py:126-134 under type promotion), so the staircase's thresholds are doubles.
 *   mctq_lut_steps_f64_bytes  upper bound of the blob size for a codebook of n_lut entries
 *   mctq_lut_build_steps_f64  host code: fills steps_host (double T[P], float Q[P], float q_nan, float P) and *p_out = P
 *                             by bisecting the literal double scan; MCTQ_E_ARG when the codebook does not qualify
 *   mctq_luts_per_tensor_f64 / _per_channel_f64   the launches; `steps` is a DEVICE copy of that blob.  Arguments as
 *                             mctq_lut_per_tensor_f64 / mctq_lut_per_channel with dtype MCTQ_DT_F64; y is float32.
 */
int32_t mctq_lut_steps_f64_bytes(int32_t n_lut);
int mctq_lut_build_steps_f64(const float* lut_host, int32_t n_lut, float mult, float clip_min, float clip_max,
                             void* steps_host, int32_t* p_out);
int mctq_luts_per_tensor_f64(const double* x, float* y, int64_t n, double thr_div, float thr_mul, const void* steps,
                             int32_t P, float mult, float clip_min, float clip_max, void* stream);
int mctq_luts_per_channel_f64(const double* x, float* y, int64_t outer, int64_t channels, int64_t inner,
                              const float* thresholds, float eps, const void* steps, int32_t P, float mult,
                              float clip_min, float clip_max, void* stream);

/*
 * Decision-table form of the LUT quantizer (integer codebooks, clip range of at most 1023.5 units).
 *
 * The literal scan above costs ~4 VALU ops per codebook entry per element.  For an integer codebook the
 * result of that scan, as a function of the scaled value t, is a staircase whose steps sit within a few
 * ulps of the half-integer points clip_min + k/2.  mctq_lut_build_table() -- host code, no GPU -- runs the
 * literal scan in float32 and records for every point the exact threshold of its step and the dequantized
 * centres on both sides; the mctq_lutt_* kernels stage that table in LDS and decide each element with one
 * LDS read, one compare and one select, bit-identically to the literal scan for every float32 input.
 *
 *   mctq_lut_table_entries : number K of table points for a clip range (= 2*(clip_max-clip_min)+1), or
 *                            MCTQ_E_ARG if the range is not integral or too large for LDS.
 *   mctq_lut_build_table   : lut_host[n_lut] is a HOST array in the caller's list order; table_host receives
 *                            2*(K+1) 32-bit words: K entries {T_k (float32), half2(q_below, q_above)} and one
 *                            trailer {q for NaN input (float32), K}.  Fails (MCTQ_E_ARG) for a non-integer
 *                            codebook; callers then use the literal kernels.
 *   mctq_lutt_per_tensor_f32 / mctq_lutt_per_channel_f32 : as mctq_lut_per_*_f32, with `table` (DEVICE copy
 *                            of table_host) and `entries` = K in place of the codebook.
 */
int32_t mctq_lut_table_entries(float clip_min, float clip_max);

int mctq_lut_build_table(const float* lut_host, int32_t n_lut, float mult, float clip_min, float clip_max,
                         float* table_host);

int mctq_lutt_per_tensor_f32(const float* x, float* y, int64_t n,
                             float thr_div, float thr_mul,
                             const float* table, int32_t entries,
                             float mult, float clip_min, float clip_max,
                             void* stream);

int mctq_lutt_per_channel_f32(const float* x, float* y,
                              int64_t outer, int64_t channels, int64_t inner,
                              const float* thresholds, float eps,
                              const float* table, int32_t entries,
                              float mult, float clip_min, float clip_max,
                              void* stream);

int mctq_lutt_per_tensor(const void* x, float* y, int64_t n, int32_t dtype, int32_t step_round,
                         float thr_div, float thr_mul,
                         const float* table, int32_t entries,
                         float mult, float clip_min, float clip_max,
                         void* stream);

int mctq_lutt_per_channel(const void* x, float* y,
                          int64_t outer, int64_t channels, int64_t inner, int32_t dtype,
                          const float* thresholds, float eps,
                          const float* table, int32_t entries,
                          float mult, float clip_min, float clip_max,
                          void* stream);

/*
 * Codebook-index codes of the LUT quantizers and their decode (an extension: the reference has no counterpart, as for the
 * integer codes of the affine quantizers above).  For an element x with threshold thr (its channel's, or the tensor's):
 *     t    = clip((x / fl32(thr + eps)) * mult, clip_min, clip_max)          as the mctq_lut_* entry points compute it
 *     code = first index j (caller's list order) minimising fl32(|t - lut[j]|);  NaN input -> 0       (torch.argmin)
 *     decode(code) = (lut[code] / mult) * thr                                  two float32 operations
 * so decode(encode(x)) is bit-identical to the fake-quantized value of the mctq_lut_* / mctq_lutt_* entry points for every
 * input.  Duplicate centres yield the FIRST occurrence; two different centres at equal distance the one listed first.
 * Codes are uint8 (MCTQ_CODE_U8, n_lut <= 256) or packed 4-bit (MCTQ_CODE_U4, n_lut <= 16: two codes per byte, element 2j of
 * the storage order in the low nibble; layouts as for the affine 4-bit codes: per tensor n % 8 == 0, per channel
 * inner % 8 == 0, or inner == 1 with channels % 8 == 0; x / y 16-byte and codes 4-byte aligned).
 *   mctq_lut_build_index_table : as mctq_lut_build_table (same K, same thresholds T_k bit for bit, same refusals), but
 *                            word 1 of entry k is index_below | index_above << 16 (first occurrence of the centre in list
 *                            order) and the trailer is {0 (index for NaN input), K}.
 *   mctq_lut_codes_per_tensor / _per_channel : x float32 / float16 / bfloat16 (dtype), codes out.  `lut` (DEVICE, n_lut
 *                            floats, list order) is always given; `index_table` (DEVICE copy of the table above, `entries`
 *                            = K) is optional (NULL: the literal scan carrying the index -- any codebook, slower).
 *                            step_round as mctq_lutt_per_tensor.  5 algorithmic bytes per float32 element (4.5 packed).
 *   mctq_lut_decode_per_tensor / _per_channel : codes in, y float32 out; every block stages lut[j] / mult once and each
 *                            element costs one table read and one multiplication by its threshold.  A code >= n_lut
 *                            (never produced by the encoders) decodes to 0.0 * thr: the staged table is zero-padded to
 *                            the 256 (4-bit: 16) values a code can take.  uint8 codes that are not 4-byte or a y that is
 *                            not 16-byte aligned take a one-element-per-lane kernel; 4-bit codes are refused then.
 * Conventions of every entry point (caller-owned device pointers, stream order, legal under graph capture, no allocation,
 * mctq_last_launch / mctq_launch_count, MCTQ_E_ARG without a GPU, empty tensors launch nothing) hold; the size limit above
 * (2^32 - 8192 elements in short rows) applies to the per-channel encode, and the decode takes at most 2^32 - 8192 elements
 * per launch in any layout.
 */
int mctq_lut_build_index_table(const float* lut_host, int32_t n_lut, float mult, float clip_min, float clip_max,
                               float* table_host);

int mctq_lut_codes_per_tensor(const void* x, void* codes, int64_t n, int32_t dtype, int32_t code_dtype, int32_t step_round,
                              float thr_div,
                              const float* lut, int32_t n_lut,
                              const float* index_table, int32_t entries,
                              float mult, float clip_min, float clip_max,
                              void* stream);

int mctq_lut_codes_per_channel(const void* x, void* codes,
                               int64_t outer, int64_t channels, int64_t inner, int32_t dtype, int32_t code_dtype,
                               const float* thresholds, float eps,
                               const float* lut, int32_t n_lut,
                               const float* index_table, int32_t entries,
                               float mult, float clip_min, float clip_max,
                               void* stream);

int mctq_lut_decode_per_tensor(const void* codes, float* y, int64_t n, int32_t code_dtype,
                               const float* lut, int32_t n_lut, float mult, float thr_mul,
                               void* stream);

int mctq_lut_decode_per_channel(const void* codes, float* y,
                                int64_t outer, int64_t channels, int64_t inner, int32_t code_dtype,
                                const float* lut, int32_t n_lut, float mult,
                                const float* thresholds,
                                void* stream);

/*
 * Threshold-list ("steps") form of the LUT quantizer: INTEGER codebooks whose clip range is too large for the decision
 * table (lut_values_bitwidth > 10; clip bounds and centres within +-2^20).  For such codebooks the literal scan's
 * result is a non-decreasing staircase of the scaled value with one hand-over per pair of adjacent sorted centres;
 * mctq_lut_build_steps() -- host code -- finds each hand-over's exact float32 threshold by bisecting the literal
 * scan over float bit patterns and checks the model on sample points; the mctq_luts_* kernels count the thresholds
 * <= t with a branchless binary search in LDS (log2 of the codebook size reads per element instead of 4 VALU ops per
 * entry), bit-identically to the literal scan (tested for all 2^32 inputs).
 *   mctq_lut_steps_words : upper bound of the array size in floats for a codebook of n_lut entries (lists of 128
 *                          thresholds or more carry a cell index behind the 2 * P + 2 words: see LutCellsOp).
 *   mctq_lut_build_steps : fills steps_host (HOST) and *n_words with the actual size 2 * P + 2; MCTQ_E_ARG for a
 *                          non-integer codebook or one that fails the staircase check (use the literal kernels then).
 *   mctq_luts_per_tensor / _per_channel : as mctq_lutt_*, with `steps` (DEVICE copy) and `n_words` in place of the table.
 */
int32_t mctq_lut_steps_words(int32_t n_lut);

int mctq_lut_build_steps(const float* lut_host, int32_t n_lut, float mult, float clip_min, float clip_max,
                         float* steps_host, int32_t* n_words);

int mctq_luts_per_tensor(const void* x, float* y, int64_t n, int32_t dtype, int32_t step_round,
                         float thr_div, float thr_mul,
                         const float* steps, int32_t n_words,
                         float mult, float clip_min, float clip_max,
                         void* stream);

int mctq_luts_per_channel(const void* x, float* y,
                          int64_t outer, int64_t channels, int64_t inner, int32_t dtype,
                          const float* thresholds, float eps,
                          const float* steps, int32_t n_words,
                          float mult, float clip_min, float clip_max,
                          void* stream);

/*
 * Export-time arithmetic: what the reference's quantizers compute while an ONNX export traces them
 * (`self._use_custom_impl and torch.jit.is_tracing()`), a different last-ulp contract from the fake-quant
 * entry points above: clip, TRUE division by the step, round half even, scale back.
 *     c = x < lo ? lo : x;   c = x > hi ? hi : c;                 (NaN and signed zeros pass through)
 *     y = shifted ? step * rint((c - lo) / step) + lo  :  rint(c / step) * step
 * Replaces (relative to mct_quantizers/pytorch/quantizers/):
 *   weights_inferable_quantizers/weights_symmetric_inferable_quantizer.py:32-70  quantize_sym_weights_torch
 *       (lo = -thr, hi = thr - scale, step = scale = thr / 2^(n-1); also weights_pot_inferable_quantizer.py:106-122)
 *   weights_inferable_quantizers/weights_uniform_inferable_quantizer.py:34-78   quantize_uniform_weights_torch
 *       (lo, hi = range adjusted to contain 0, step = (hi - lo) / (2^n - 1), shifted = 0)
 *   activation_inferable_quantizers/activation_symmetric_inferable_quantizer.py:29-54  quantize_sym_activations_torch
 *   activation_inferable_quantizers/activation_uniform_inferable_quantizer.py:32-65   quantize_uniform_activations_torch
 *       (shifted = 1)
 * float32 in and out; per-channel tables are DEVICE float32[channels]; layout arguments as mctq_fq_per_channel.
 */
int mctq_grid_per_tensor_f32(const float* x, float* y, int64_t n,
                             float lo, float hi, float step, int32_t shifted,
                             void* stream);

int mctq_grid_per_channel_f32(const float* x, float* y,
                              int64_t outer, int64_t channels, int64_t inner,
                              const float* los, const float* his, const float* steps, int32_t shifted,
                              void* stream);

/*
 * Per-tensor codes with a layout change: x [batch][channels][pixels] (NCHW, pixels = H * W) -> codes
 * [batch][pixels][channels] (NHWC), int8 / uint8, same arithmetic as mctq_fq_codes_per_tensor.  What a pointwise
 * (1x1) convolution consumer feeds mctq_qlinear_i8 with (rows = pixels, K = channels) when the activation arrives
 * in PyTorch's default layout.  NaN -> quant_min, +-inf saturate, as there.
 * One block moves a 128 (channels) x 32 (pixels) tile.  Four pixels per lane arrive by one 8- / 16-byte load when
 * pixels % 4 == 0 and x is aligned to four elements, element by element otherwise; 16 channels per lane leave by one
 * 16-byte store when channels % 16 == 0 and codes is 16-byte aligned, byte by byte otherwise: any x aligned to its
 * element and any codes pointer are accepted.  MCTQ_E_ARG for negative extents, quant_min > quant_max, a code type other
 * than MCTQ_CODE_I8 / MCTQ_CODE_U8 or a clamp domain outside it, NULL pointers, more than 2^31 - 1 channels or tiles and an
 * unknown dtype; an empty extent returns 0 without a launch.  mctq_last_launch names the launch "codes_nchw_to_nhwc" with
 * the form it took ("vector loads" / "scalar loads" + "16-byte stores" / "byte stores") and the input's byte width.
 */
int mctq_fq_codes_nchw_to_nhwc(const void* x, void* codes, int64_t batch, int64_t channels, int64_t pixels, int32_t dtype,
                               int32_t code_dtype, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max,
                               void* stream);

/*
 * Patch matrix of activation codes (im2col), what a k x k / strided / padded / dilated convolution feeds the integer
 * consumer with: codes [batch][height][width][channels] (NHWC, int8 or uint8 -- a pure byte gather, the code type does
 * not matter) -> patches [batch * Ho * Wo][kh * kw * channels], both DEVICE, 16-byte aligned, with
 *     Ho = (height + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1,   Wo likewise,
 * row m = (b * Ho + oy) * Wo + ox, column k = (ky * kw + kx) * channels + c holding
 * codes[b][oy * stride_h - pad_h + ky * dil_h][ox * stride_w - pad_w + kx * dil_w][c], or the byte pad_code & 0xFF where
 * that tap lies outside the image.  With pad_code = the activation's zero point a padded tap contributes
 * (a_zero_point - a_zero_point) * w = 0 to mctq_qlinear_*'s sum: the kernels' - a_zero_point * w_rowsum[n] correction
 * makes zero padding exact.  The weights of the product are the convolution's [O][kh][kw][C] (channels innermost).
 * channels % 16 == 0 and kh * kw * channels <= 32768 (the consumer's K limit): every 16-byte chunk of an output row is
 * one aligned 16-byte chunk of the input or 16 pad bytes -- one 16-byte load and one 16-byte store per lane, consecutive
 * lanes on consecutive chunks of a row; the input is re-read up to kh * kw times out of cache, the output written once.
 * MCTQ_E_ARG with a mctq_last_error text for: negative extents; a kernel size, stride or dilation below 1; negative
 * padding; pad_code outside [-128, 255]; channels % 16 != 0; kh * kw * channels > 32768; a padded extent above 2^31 - 1;
 * Ho <= 0 or Wo <= 0; more than 2^31 - 1 output rows; NULL or misaligned pointers of a non-empty problem.  batch == 0
 * returns 0 without a launch.  mctq_last_launch names the launch "codes_im2col".
 */
int mctq_codes_im2col_nhwc(const void* codes, void* patches, int64_t batch, int64_t height, int64_t width, int64_t channels,
                           int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                           int32_t dil_h, int32_t dil_w, int32_t pad_code, void* stream);

/*
 * The same patch matrix for ANY channel count (channels >= 1), its rows padded to whole 16-byte chunks: codes
 * [batch][height][width][channels] -> patches [batch * Ho * Wo][Kp], K = kh * kw * channels, Kp = 16 * ceil(K / 16) <= 32768,
 * both DEVICE, 16-byte aligned.  Column k < K holds what mctq_codes_im2col_nhwc writes there (a tap outside the image: the byte
 * pad_code & 0xFF); columns K .. Kp - 1 hold pad_code & 0xFF.  With pad_code = the activation's zero point and weight rows
 * [N][Kp] whose last Kp - K codes are 0, the product mctq_qlinear_* computes over Kp columns is the product over K columns
 * exactly: a padded column adds a * 0 = 0 to the int32 sum and 0 to w_rowsum[n], and (a_zero_point - a_zero_point) = 0 to
 * mctq_codes_rowsum's sums, so weight zero points are covered too.  For channels % 16 == 0 the bytes are those of
 * mctq_codes_im2col_nhwc.  height = width = kh = kw = 1 re-pitches [batch][channels] rows to [batch][Kp].
 * A lane assembles one 16-byte chunk of an output row from pieces of G bytes and stores it once: G = 4 (aligned dword loads)
 * where channels % 4 == 0 -- a piece then never straddles two taps or the row's end -- and G = 1 (byte loads) elsewhere; tuning
 * key "im2col_grain" forces one.  Every load address is formed from coordinates clamped into the image: no load reads outside
 * `codes`, whatever the geometry.
 * MCTQ_E_ARG with a mctq_last_error text for: negative extents; a kernel size, stride or dilation below 1; negative padding;
 * pad_code outside [-128, 255]; kh * kw * channels > 32768; "im2col_grain" 4 with channels % 4 != 0; a padded extent above
 * 2^31 - 1; Ho <= 0 or Wo <= 0; an image without pixels in a non-empty batch; more than 2^31 - 1 output rows; NULL or misaligned
 * pointers of a non-empty problem.  batch == 0 or channels == 0 returns 0 without a launch.  mctq_last_launch names the launch
 * "codes_im2col_pad", op "padded gather G=4" / "padded gather G=1".
 */
int mctq_codes_im2col_pad_nhwc(const void* codes, void* patches, int64_t batch, int64_t height, int64_t width, int64_t channels,
                               int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                               int32_t dil_h, int32_t dil_w, int32_t pad_code, void* stream);

/*
 * Max pooling on activation codes (extension; the reference runs ATen's float32 max pool on the holder's output):
 * codes [batch][height][width][channels] (NHWC, int8 -- code_dtype MCTQ_CODE_I8 -- or uint8, MCTQ_CODE_U8) -> pooled
 * [batch][Ho][Wo][channels] of the same type, both DEVICE, 16-byte aligned, with torch.nn.MaxPool2d's semantics:
 *     pooled[b][oy][ox][c] = max over the taps (ky, kx) inside the image of
 *                            codes[b][oy * stride_h - pad_h + ky * dil_h][ox * stride_w - pad_w + kx * dil_w][c]
 * in the order of the code type (signed for int8, unsigned for uint8).  A tap outside the image is ignored: it stands for
 * -inf, not for the zero-point code.  A holder's float32 output is float(code - zero_point) * scale with scale > 0, monotone
 * non-decreasing in the code and never NaN, so dequantizing `pooled` gives ATen's max pool of the dequantized `codes` bit
 * for bit.  pad_h <= kh / 2 and pad_w <= kw / 2, as PyTorch requires.  Output extent, PyTorch's rule:
 *     Ho = floor_or_ceil((height + 2 pad_h - dil_h (kh - 1) - 1) / stride_h) + 1   (ceil with ceil_mode != 0),
 *     less one with ceil_mode if (Ho - 1) * stride_h >= height + pad_h (a last window that would start beyond the image
 *     plus its left padding is dropped);   Wo likewise.
 * The caller passes the out_height / out_width it allocated `pooled` for, and the call is refused unless they equal the
 * library's own Ho / Wo: a disagreement about the extent can then never become an out-of-bounds write.
 * A window without any tap inside the image (possible only where the image is narrower than the dilation) gives the least
 * code of the type, 0 / -128, as ATen's integer max pool does.
 * channels % 16 == 0.  A lane owns one 16-channel chunk of one output pixel (consecutive lanes: consecutive chunks, then
 * consecutive pixels): one 16-byte load per tap, one 16-byte store; the input is re-read about kh * kw / (stride_h *
 * stride_w) times out of cache.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: negative extents; a
 * kernel size, stride or dilation below 1; negative padding; padding above half the kernel size; channels % 16 != 0; a bad
 * code_dtype; a padded extent plus kernel span above 2^31 - 1; Ho <= 0 or Wo <= 0; out_height / out_width other than Ho /
 * Wo; a non-empty batch of images without pixels; more than 2^31 - 1 output pixels, or more than 2^32 - 1 16-channel chunks
 * of output (split the batch); NULL or misaligned pointers of a non-empty problem.  batch == 0 or channels == 0 returns 0
 * without a launch.  mctq_last_launch names the launch "codes_maxpool", op "u8 max" / "i8 max".
 */
int mctq_codes_maxpool_nhwc(const void* codes, void* pooled, int32_t code_dtype, int64_t batch, int64_t height, int64_t width,
                            int64_t channels, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h,
                            int32_t pad_w, int32_t dil_h, int32_t dil_w, int32_t ceil_mode, int64_t out_height, int64_t out_width,
                            void* stream);

/*
 * Channel concatenation on activation codes (extension; the reference runs torch.cat on the float32 outputs of the operand
 * holders and the holder behind it on the result): operand k is codes [pixels][channels_k] (NHWC with the leading extents
 * folded; int8 -- MCTQ_CODE_I8 -- or uint8, MCTQ_CODE_U8) with its own scale and zero point, out is
 * [pixels][sum of channels_k] in the form (out_code_dtype, scale, zero_point, quant_min, quant_max); all DEVICE pointers,
 * 16-byte aligned; `items` is a HOST array of `count` operands, 1 .. 8, read before the call returns:
 *     v                          = fma(float(code_k[p][c] - zero_point_k), scale_k, +0)     the operand holder's float32 output
 *     out[p][start_k + c]        = clamp(rint(v * (1.0f / scale)) + zero_point, quant_min, quant_max)
 * -- bit for bit the code the holder behind the concatenation gives that float32 tensor (mctq_fq_codes_per_tensor's
 * arithmetic, the reciprocal computed on the host as there).  count == 1 is a requantization of codes.
 * Every channels_k is a positive multiple of 16: a 16-byte chunk of an output row is one aligned chunk of one operand, and a
 * lane owns one such chunk -- one 16-byte load, one 16-byte store, 1 byte read and 1 written per element.
 * An operand whose form is the output's (the same float32 scale bits, zero point and code type, [quant_min, quant_max] the
 * whole range of the type, scale in [2^-100, 2^100]) is copied: for such a form the arithmetic above returns the code it
 * was given, for every code.  Tuning key "concat_copy" = 0 sends such operands through the arithmetic as well.
 * A lane reads only chunks below pixels * channels_k / 16 of its operand and writes only chunks below
 * pixels * sum(channels_k) / 16.
 * MCTQ_E_ARG with a mctq_last_error text, before anything is launched, for: count outside 1 .. 8; items NULL; pixels < 0; a
 * bad code type; a zero point that is no code of its type (operands and output); a scale that is not finite and positive
 * (operands and output); quant_min > quant_max or a domain outside the output type; channels_k not a positive multiple of
 * 16; more than 2^31 - 1 16-byte chunks of output (split the pixels); NULL or misaligned pointers of a non-empty problem;
 * an `out` whose bytes overlap an operand's.  pixels == 0 returns 0 without a launch.  mctq_last_launch names the launch
 * "codes_concat", op "<count> -> u8" / "<count> -> i8".
 */
typedef struct mctq_concat_item {
  const void* codes;      /* device, [pixels][channels], 16-byte aligned */
  int64_t channels;
  int32_t code_dtype;     /* MCTQ_CODE_I8 / MCTQ_CODE_U8 */
  int32_t zero_point;
  float scale;
} mctq_concat_item;
int mctq_codes_concat_nhwc(const mctq_concat_item* items, int32_t count, void* out, int32_t out_code_dtype, int64_t pixels,
                           float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream);

/*
 * Elementwise multiply on activation codes (extension; the reference runs torch.mul on the float32 outputs of two holders and
 * the holder behind it on the result): a is codes [pixels][channels] (NHWC with the leading extents folded; int8 --
 * MCTQ_CODE_I8 -- or uint8, MCTQ_CODE_U8) of the form (a_scale, a_zero_point), out is [pixels][channels] in the form
 * (out_code_dtype, scale, zero_point, quant_min, quant_max); all DEVICE pointers, 16-byte aligned.  The second operand g:
 *     gate_pixels == 0, g_is_f32 == 0   codes [pixels][channels] of (g_code_dtype, g_scale, g_zero_point)          "same"
 *     gate_pixels == n >= 1, g_is_f32 == 0   codes [pixels / n][channels]: row p / n multiplies pixel p (an SE gate
 *                                            [B, C, 1, 1] over images of n = H * W pixels)                          "row"
 *     gate_pixels == n >= 1, g_is_f32 != 0   raw float32 values [pixels / n][channels], coded first in G's form
 *                                            cg = clamp(rint(g * (1.0f / g_scale)) + g_zero_point, g_quant_min, g_quant_max),
 *                                            NaN -> g_quant_min (mctq_fq_codes_per_tensor's arithmetic)             "row f32"
 * g_quant_min / g_quant_max are read for a float32 g only; a float32 g is taken in the row form only.  Per element
 *     va  = fma(float(ca - a_zero_point), a_scale, +0)        holder A's float32 output
 *     vg  = fma(float(cg - g_zero_point), g_scale, +0)        holder G's float32 output
 *     m   = va * vg                                           one IEEE float32 multiplication, torch.mul's
 *     out = clamp(rint(m * (1.0f / scale)) + zero_point, quant_min, quant_max)        NaN -> quant_min
 * -- bit for bit the code the holder behind the multiply gives that float32 product (the reciprocal computed on the host as
 * in mctq_fq_codes_per_tensor); a function of the two codes alone.
 * channels is a positive multiple of 16.  A lane owns one 16-byte chunk of the output: one 16-byte load of a, one of g (four
 * for float32), one 16-byte store; consecutive pixels re-read the same row of g from cache.  A lane reads only chunks below
 * pixels * channels / 16 of a, below that or (pixels / n) * channels / 16 of g, and writes only chunks below
 * pixels * channels / 16.
 * MCTQ_E_ARG with a mctq_last_error text, before anything is launched, for: pixels < 0; a bad code type (a, g, out); a zero
 * point that is no code of its type (a, g, out); a scale that is not finite and positive (a, g, out); quant_min > quant_max
 * or a domain outside the type (out, and g where it is float32); gate_pixels < 0; a float32 g with gate_pixels == 0;
 * channels not a positive multiple of 16; pixels % gate_pixels != 0; more than 2^31 - 1 16-byte chunks (split the pixels);
 * NULL or misaligned pointers of a non-empty problem; an `out` whose bytes overlap a's or g's (a and g may be one buffer:
 * x * x).  pixels == 0 returns 0 without a launch.  mctq_last_launch names the launch "codes_mul", op
 * "<a> * <g> -> <out> <form>" with the code types "u8" / "i8" and the form "same" / "row" / "row f32".
 */
int mctq_codes_mul_nhwc(const void* a, int32_t a_code_dtype, float a_scale, int32_t a_zero_point, const void* g,
                        int32_t g_code_dtype, float g_scale, int32_t g_zero_point, int32_t g_is_f32, int32_t g_quant_min,
                        int32_t g_quant_max, int64_t gate_pixels, void* out, int32_t out_code_dtype, int64_t pixels,
                        int64_t channels, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream);

/*
 * Average pooling on activation codes (extension; the reference runs ATen's float32 average pool on the holder's output and
 * the holder behind it on the result): codes [batch][height][width][channels] (NHWC; int8 -- MCTQ_CODE_I8 -- or uint8,
 * MCTQ_CODE_U8) of the form (scale, zero_point) -> pooled [batch][out_height][out_width][channels] in the form
 * (y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max), DEVICE pointers, 16-byte aligned; torch.nn.AvgPool2d's
 * kernel, stride, padding, ceil_mode, count_include_pad and divisor_override (0 = none).  Per output element
 *     S    = sum over the window's taps inside the image of (code - zero_point)                int32, exact
 *     div  = divisor_override, or with count_include_pad (min(h0 + kh, H + pad_h) - h0) * (min(w0 + kw, W + pad_w) - w0)
 *            with h0 = oy * stride_h - pad_h (PyTorch's pool_size), or else the number of taps inside the image
 *     v    = fma(float(S), scale, +0)                                                         one float32 rounding
 *     m    = v / float(div)                                                                   IEEE float32 division
 *     out  = clamp(rint(m * (1.0f / y_scale)) + y_zero_point, y_quant_min, y_quant_max)       NaN -> y_quant_min
 * float(S) is exact: a window has at most 65536 taps and 255 * 65536 < 2^24.  A window without a tap inside the image (no
 * geometry PyTorch accepts has one) gives m = 0.0.  Where scale and every div are powers of two this is bit for bit the code
 * the holder behind any float32 average pool of the dequantized codes gives; elsewhere it is the exact mean rounded twice.
 * Two forms with the same bytes (the sum is an integer): "lane", one lane per 16-channel chunk of an output pixel as in
 * mctq_codes_maxpool_nhwc, and "split", the taps of a window divided among the lanes of one workgroup with int32 partial
 * sums meeting in LDS, for few and large windows.  The launcher chooses; tuning key "avgpool_form" forces one.
 * A lane reads only chunks of images below `batch` and writes only chunks below batch * Ho * Wo * channels / 16.
 * MCTQ_E_ARG with a mctq_last_error text, before anything is launched, for: a negative extent; kernel size or stride below
 * 1; negative padding; padding above half the kernel size; kh * kw > 65536; a negative divisor_override; channels % 16 != 0;
 * a bad code_dtype or y_code_dtype; a zero_point that is no code of the input's type; a scale or y_scale that is not finite
 * and positive; y_quant_min > y_quant_max or a domain outside the output type; a padded extent plus kernel above 2^31 - 1;
 * Ho <= 0 or Wo <= 0; out_height / out_width other than Ho / Wo; a non-empty batch of images without pixels; more than
 * 2^31 - 1 output pixels, or more than 2^32 - 1 16-channel chunks of output (split the batch); NULL or misaligned pointers of
 * a non-empty problem.  batch == 0 or channels == 0 returns 0 without a launch.  mctq_last_launch names the launch
 * "codes_avgpool", op "u8 avg lane" / "u8 avg split" / "i8 avg lane" / "i8 avg split".
 */
int mctq_codes_avgpool_nhwc(const void* codes, void* pooled, int32_t code_dtype, int32_t zero_point, float scale, int64_t batch,
                            int64_t height, int64_t width, int64_t channels, int32_t kh, int32_t kw, int32_t stride_h,
                            int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t ceil_mode, int32_t count_include_pad,
                            int32_t divisor_override, int64_t out_height, int64_t out_width, int32_t y_code_dtype, float y_scale,
                            int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max, void* stream);

/*
 * Nearest resampling on activation codes (extension; the reference runs ATen's nearest upsample on the float32 output of a
 * holder and the holder behind it on the result): codes [batch][height][width][channels] (NHWC; int8 -- MCTQ_CODE_I8 -- or
 * uint8, MCTQ_CODE_U8) of the form (in_scale, in_zero_point) -> out [batch][out_height][out_width][channels] in the form
 * (out_code_dtype, scale, zero_point, quant_min, quant_max), DEVICE pointers, 16-byte aligned.  The index map is separable and
 * given in one of two ways: src_rows / src_cols, DEVICE int32 tables of out_height / out_width entries (4-byte aligned) with
 * factor_h == factor_w == 0 -- any geometry, downsampling included -- or factor_h, factor_w >= 1 with both tables NULL,
 * out_height == factor_h * height, out_width == factor_w * width and src = dst / factor.  Per output element
 *     v   = fma(float(code[b][src_rows[ho]][src_cols[wo]][c] - in_zero_point), in_scale, +0)     the holder's float32 output
 *     out = clamp(rint(v * (1.0f / scale)) + zero_point, quant_min, quant_max)
 * -- mctq_codes_concat_nhwc's arithmetic with count == 1, the reciprocal computed on the host; nearest interpolation only
 * moves data, so this is bit for bit the code the holder behind the float32 upsample gives, for every element.  An input
 * whose form is the output's is stored as loaded, under mctq_codes_concat_nhwc's conditions and its tuning key "concat_copy".
 * Two forms with the same bytes: "gather", one lane per 16-channel chunk of an OUTPUT pixel (one 16-byte load through the
 * map, one 16-byte store; every geometry), and "replicate", for integer factors with factor_h * factor_w <= 16, one lane per
 * 16-channel chunk of an INPUT pixel (one load, one requantization, factor_h * factor_w 16-byte stores).  The launcher chooses
 * replicate where it is eligible and factor_h * factor_w >= 2 -- measured on 2 x and 4 x upsamples: 1.77 - 2.25 x faster than gather
 * at batch 64, equal at the launch floor at batch 1 (profiles/EXPERIMENTS.md); other factors not measured -- and gather elsewhere;
 * tuning key "upsample_form" forces one.
 * The launcher cannot see the device tables: the kernel clamps every entry into [0, height - 1] / [0, width - 1] before it
 * forms an address.  A lane reads only chunks below batch * height * width * channels / 16, entries below out_height /
 * out_width of the tables, and writes only chunks below batch * out_height * out_width * channels / 16.
 * MCTQ_E_ARG with a mctq_last_error text, before anything is launched, for: a negative extent; channels % 16 != 0; a bad
 * code_dtype or out_code_dtype; a zero point that is no code of its type (input and output); a scale that is not finite and
 * positive (input and output); quant_min > quant_max or a domain outside the output type; tables and factors both given, or
 * neither; one table without the other; a factor below 1; an image extent above 2^31 - 1; integer factors with out_height !=
 * factor_h * height or out_width != factor_w * width; a non-empty output from an image without pixels; more than 2^31 - 1
 * 16-byte chunks of output (split the batch); NULL or misaligned pointers of a non-empty problem; an `out` whose bytes overlap
 * the codes' or a table's.  batch == 0, channels == 0 or an empty output returns 0 without a launch.  mctq_last_launch names
 * the launch "codes_upsample", op "<in> -> <out> <form>" with the code types "u8" / "i8" and the form "gather" / "replicate".
 */
int mctq_codes_upsample_nhwc(const void* codes, void* out, int32_t code_dtype, int32_t in_zero_point, float in_scale,
                             int64_t batch, int64_t height, int64_t width, int64_t channels, int64_t out_height,
                             int64_t out_width, int32_t factor_h, int32_t factor_w, const int32_t* src_rows,
                             const int32_t* src_cols, int32_t out_code_dtype, float scale, int32_t zero_point,
                             int32_t quant_min, int32_t quant_max, void* stream);

/*
 * An elementwise function between two activation holders on codes (extension; the reference runs the function on the float32
 * output of holder A and holder B on the result): out[i] = table[raw byte in[i]] for i < n.  Holder A's float32 output takes at
 * most 256 values, one per code, and both the function and holder B work element by element, so B's code is a function of A's
 * code.  table: 256 bytes on the DEVICE, 4-byte aligned, indexed by the RAW byte of the input (an int8 code c at entry (uint8_t)c),
 * its entries the raw bytes of the output codes -- the caller builds it by running the replaced function on the 256 dequantized
 * codes (ops.code_table).  in, out: DEVICE pointers, 16-byte aligned, n bytes each, any n >= 0 (flat: no shape, no channel count).
 * in_code_dtype / out_code_dtype (MCTQ_CODE_I8 or MCTQ_CODE_U8) are checked and name the launch; the bytes do not depend on them.
 * A workgroup keeps the table in 256 B of LDS (64 lanes load one dword each, one barrier); a lane owns "table_chunks" (tuning key:
 * 1, 2 or 4, default 4) chunks of 16 bytes, issues all of their loads before the first lookup, and writes one plain 16-byte store
 * per chunk; the n % 16 tail bytes are read and written byte by byte by one lane.  No byte outside [out, out + n) is written.
 * MCTQ_E_ARG with a mctq_last_error text, before anything is launched, for: n < 0; a bad in_code_dtype or out_code_dtype; more
 * than 2^31 - 1 16-byte chunks (split the tensor); with n > 0, a NULL pointer, an in or out that is not 16-byte aligned, a table
 * that is not 4-byte aligned, an `out` whose bytes overlap in's or the table's.  n == 0 returns 0 without a launch.
 * mctq_last_launch names the launch "codes_table", op "<in> -> <out> blocks=<workgroups>" with the code types "u8" / "i8", U = the
 * chunks per lane: a workgroup covers 256 * U * 16 bytes.
 */
int mctq_codes_table(const void* in, int32_t in_code_dtype, void* out, int32_t out_code_dtype, int64_t n, const void* table,
                     void* stream);

/*
 * Depthwise convolution on activation codes (groups == channels, channel multiplier 1; extension, the reference has no
 * counterpart): what a wrapped depthwise torch.nn.Conv2d computes on fake-quantized operands, evaluated on the codes.
 *     acc[b][oy][ox][c] = sum over the taps (ky, kx) inside the image of
 *                         (a[b][oy * stride_h - pad_h + ky * dil_h][ox * stride_w - pad_w + kx * dil_w][c] - a_zero_point)
 *                         * (w[ky][kx][c] - zw[c])
 *     y[b][oy][ox][c]   = float(acc) * (a_scale * w_scales[c]) + bias[c]
 * zw = 0 when w_zero_points is NULL.  Taps outside the image add nothing: zero padding, exact for the reason given at
 * mctq_codes_im2col_nhwc (the kernel gives such a tap the zero-point byte).  The int32 sum is exact (at most 256 taps of
 * |a - za| <= 255 times |w - zw| <= 255: below 2^24 * 2^8); then one float32 multiply of the two scales, one float32
 * multiply and one float32 add, each rounded once -- the arithmetic of mctq_qlinear_i8.  Output forms as for
 * mctq_qlinear_w4a8: y_code_dtype < 0 -> y is float32 [batch][Ho][Wo][channels]; MCTQ_CODE_I8 / _U8 -> y holds the next
 * layer's codes, clamp(rint(y * (1.0f / y_scale)) + y_zero_point, y_quant_min, y_quant_max), NaN -> y_quant_min.
 *     Ho = (height + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1,   Wo likewise.
 * a_codes [batch][height][width][channels] (NHWC) int8 or uint8 (a_code_dtype); w_codes [kh][kw][channels] int8, channel
 * innermost, in the int8-ranged domain of mctq_qlinear_i8_zp's weights (uniform codes and zero points re-biased by half
 * the domain, codebook weights as their int8 codebook values); w_scales float32[channels]; w_zero_points int32[channels],
 * each in [-128, 127], or NULL; bias float32[channels] or NULL.  All DEVICE pointers, 16-byte aligned (the per-channel
 * tables are read 16 bytes at a time too).
 * A lane owns one 16-channel chunk of one output pixel (consecutive lanes: consecutive chunks, then consecutive pixels):
 * per tap one 16-byte activation load and one 16-byte weight load, 16 int32 accumulators, 16-byte stores.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: negative extents; a
 * kernel size, stride or dilation below 1; negative padding; channels % 16 != 0; kh * kw > 256; a bad a_code_dtype;
 * a_zero_point outside the code type's range ([-128, 127] / [0, 255]: it is the byte a padded tap is given); a bad output
 * form (mctq_qlinear_i8_codes' checks); a padded extent above 2^31 - 1; Ho <= 0 or Wo <= 0; a non-empty batch of images
 * without pixels; more than 2^31 - 1 output pixels, or more than 2^32 - 1 16-channel chunks of output (split the batch);
 * NULL or misaligned pointers of a non-empty problem.  batch == 0 or channels == 0 returns 0 without a launch.
 * mctq_last_launch names the launch "qconv_dw", op "u8 x i8" / "i8 x i8", with " zp" appended when w_zero_points was given.
 */
int mctq_qconv_dw_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                     const int8_t* w_codes, const float* w_scales, const int32_t* w_zero_points, const float* bias,
                     void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                     int64_t batch, int64_t height, int64_t width, int64_t channels,
                     int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                     int32_t dil_h, int32_t dil_w, void* stream);

/*
 * Grouped convolution on activation codes (extension; the reference fake-quantizes weight and activation and runs the
 * float32 grouped conv2d): 2 <= groups, Cg = channels / groups input and Og = out_channels / groups output channels per
 * group, output channel n = g * Og + o:
 *     acc[b][oy][ox][n] = sum over taps (ky, kx) inside the image, cg < Cg of
 *                         (a[b][iy][ix][g * Cg + cg] - a_zero_point) * (w[n][cg][ky][kx] - zw[n])
 *     y[b][oy][ox][n]   = float(acc) * (a_scale * w_scales[n]) + bias[n]
 * zw = 0 when w_zero_points is NULL.  Taps outside the image add nothing (the kernel gives such a tap the zero-point byte:
 * a_zero_point must be a code of the activations' type).  The int32 sum is exact (Kg = kh * kw * Cg <= 32768 terms of
 * |a - za| <= 255 times |w - zw| <= 255: below 2^31); then one float32 multiply of the two scales, one float32 multiply and
 * one float32 add, each rounded once -- the arithmetic of mctq_qlinear_i8.  Output forms as for mctq_qconv_dw_i8:
 * y_code_dtype < 0 -> y is float32 [batch][Ho][Wo][out_channels]; MCTQ_CODE_I8 / _U8 -> y holds the next layer's codes.
 *     Ho = (height + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1,   Wo likewise.
 * a_codes [batch][height][width][channels] (NHWC) int8 or uint8 (a_code_dtype).  w_codes int8 [groups][Ogp][Kgp] with
 * Ogp = 16 * ceil(Og / 16), Kgp = 64 * ceil(Kg / 64): row o < Og of group g holds output channel g * Og + o in the K order
 * (ky, kx, cg), column k = (ky * kw + kx) * Cg + cg; rows o >= Og and columns k >= Kg hold the code 0.  The codes are in the
 * int8-ranged domain of mctq_qlinear_i8_zp's weights.  w_scales float32[out_channels]; w_rowsum int32[out_channels], the sum
 * of channel n's Kg codes; w_zero_points int32[out_channels], each in [-128, 127], or NULL; bias float32[out_channels] or
 * NULL.  All DEVICE pointers, 16-byte aligned.
 * One wave owns 16 consecutive output pixels x up to 64 output channels of one group (v_mfma_i32_16x16x64_i8); a block is
 * four waves; grid ceil(pixels / 64) x groups * ceil(Ogp / 64).  No patch matrix, no LDS, no atomics.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: negative extents; a
 * kernel size, stride or dilation below 1; negative padding; groups < 2; channels or out_channels that are no positive
 * multiple of groups; Cg % 4 != 0; kh * kw * Cg > 32768; a bad a_code_dtype; a_zero_point outside the code type's range; a
 * bad output form (mctq_qlinear_i8_codes' checks); a padded extent above 2^31 - 1; Ho <= 0 or Wo <= 0; a non-empty batch of
 * images without pixels; more than 2^31 - 1 output pixels; more than 65535 grid slices (groups * ceil(Ogp / 64)); NULL or
 * misaligned pointers of a non-empty problem.  batch == 0 returns 0 without a launch.
 * mctq_last_launch names the launch "qconv_grouped", op "u8 x i8" / "i8 x i8", with " zp" appended when w_zero_points was
 * given, and U = the piece size (16, 8 or 4 bytes: the largest of them that divides Cg) the activation chunks were assembled from.
 */
int mctq_qconv_grouped_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                          const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const int32_t* w_zero_points,
                          const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                          int32_t y_quant_min, int32_t y_quant_max, int64_t batch, int64_t height, int64_t width,
                          int64_t channels, int64_t out_channels, int32_t groups, int32_t kh, int32_t kw, int32_t stride_h,
                          int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t dil_h, int32_t dil_w, void* stream);

/*
 * Transposed convolution on activation codes (extension; the reference fake-quantizes weight and activation and runs the
 * float32 conv_transpose2d): nn.ConvTranspose2d with groups == 1 and dilation == 1,
 *     Ho = (height - 1) stride_h - 2 pad_h + kh + out_pad_h,   Wo likewise,
 *     acc[b][oy][ox][o] = sum over c, ky, kx with iy * stride_h = oy + pad_h - ky, ix * stride_w = ox + pad_w - kx,
 *                         0 <= iy < height, 0 <= ix < width of (a[b][iy][ix][c] - a_zero_point) * (w[c][o][ky][kx] - zw[o])
 *     y[b][oy][ox][o]   = float(acc) * (a_scale * w_scales[o]) + bias[o]
 * zw = 0 when w_zero_points is NULL.  The int32 sum is exact (at most 32768 terms of |a - za| <= 255 times |w - zw| <= 255:
 * below 2^31); then one float32 multiply of the two scales, one float32 multiply and one float32 add, each rounded once --
 * the arithmetic of mctq_qlinear_i8.  Output forms as for mctq_qconv_grouped_i8: y_code_dtype < 0 -> y is float32
 * [batch][Ho][Wo][out_channels]; MCTQ_CODE_I8 / _U8 -> y holds the next layer's codes.
 * Phases: an output pixel has the phase (ry, rx) = ((oy + pad_h) mod stride_h, (ox + pad_w) mod stride_w), p = ry * stride_w +
 * rx of P = stride_h * stride_w, and the quotient (qy, qx) = ((oy + pad_h) div stride_h, (ox + pad_w) div stride_w).  Only
 * the taps ky = ry + stride_h * ty, ty < Ty(ry) = max(0, ceil((kh - ry) / stride_h)), and kx = rx + stride_w * tx, tx < Tx(rx)
 * likewise, reach it, and tap (ty, tx) reads the input pixel (qy - ty, qx - tx); one outside the image adds nothing (the
 * kernel gives such a tap the zero-point byte: a_zero_point must be a code of the activations' type).  K(p) = Ty * Tx *
 * channels; a phase with K(p) == 0 (kernel smaller than the stride) holds the bias alone.
 * a_codes [batch][height][width][channels] (NHWC) int8 or uint8 (a_code_dtype).  w_codes int8 [P][Op][Kp] with Op = 16 *
 * ceil(out_channels / 16), Kp = 64 * ceil(max over p of K(p) / 64): row o < out_channels of phase p holds output channel o
 * in the K order (ty, tx, c), column k = (ty * Tx + tx) * channels + c the code of w[c][o][ry + stride_h * ty][rx +
 * stride_w * tx]; rows o >= out_channels and columns k >= K(p) hold the code 0.  The codes are in the int8-ranged domain of
 * mctq_qlinear_i8_zp's weights.  w_scales float32[out_channels]; w_rowsum int32[P][out_channels], the sum of row o's K(p)
 * codes of phase p; w_zero_points int32[out_channels], each in [-128, 127], or NULL; bias float32[out_channels] or NULL.  All
 * DEVICE pointers, 16-byte aligned.
 * One wave owns 16 consecutive pixels of one phase x up to 64 output channels (v_mfma_i32_16x16x64_i8); a block is four
 * waves; grid ceil(max over p of the phase's pixels / 64) x P * ceil(Op / 64).  No LDS, no atomics.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: negative extents; a
 * kernel size or stride below 1; a stride above 4; negative padding or output padding; an output padding that is not
 * smaller than the stride; channels or out_channels of 0; channels % 16 != 0; ceil(kh / stride_h) * ceil(kw / stride_w) *
 * channels > 32768; a bad a_code_dtype; a_zero_point outside the code type's range; a bad output form
 * (mctq_qlinear_i8_codes' checks); height or width above 2^31 - 1; Ho <= 0 or Wo <= 0; Ho + pad_h or Wo + pad_w above
 * 2^31 - 1; a non-empty batch of images without pixels; more than 2^31 - 1 output pixels; a codes or output tensor of 2^63
 * bytes or more; more than 65535 grid slices (P * ceil(Op / 64)); NULL or misaligned pointers of a non-empty problem.
 * batch == 0 returns 0 without a launch.
 * mctq_last_launch names the launch "qconv_transposed", op "u8 x i8" / "i8 x i8", with " zp" appended when w_zero_points
 * was given, U = the number of phases P, and out4B / out1B the output's element width.
 */
int mctq_qconv_transposed_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                             const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const int32_t* w_zero_points,
                             const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                             int32_t y_quant_min, int32_t y_quant_max, int64_t batch, int64_t height, int64_t width,
                             int64_t channels, int64_t out_channels, int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w,
                             int32_t pad_h, int32_t pad_w, int32_t out_pad_h, int32_t out_pad_w, void* stream);

/*
 * Batched matrix product of two activation-code tensors (extension; the reference fake-quantizes both operands and runs the
 * float32 torch.matmul): holder x holder, the Q.K^T and P.V products of an attention block.  Per batch (b0, b1)
 *     acc[m][n] = sum over k < K of (a[m][k] - a_zero_point) * (b[k][n] - b_zero_point)
 *     y[m][n]   = float(acc) * (a_scale * b_scale)
 * The int32 sum is exact (K <= 32768 terms of |a - za| <= 255 times |b - zb| <= 255: below 2^31); then one float32 multiply
 * of the two scales and one float32 multiply, each rounded once.  No bias, no residual, no activation.  Output forms as for
 * mctq_qconv_grouped_i8: y_code_dtype < 0 -> y is float32 [batch0][batch1][m][n], contiguous; MCTQ_CODE_I8 / _U8 -> y holds
 * the codes of (y_scale, y_zero_point) clamped to [y_quant_min, y_quant_max].
 * Operands are views given by strides in elements (= bytes): a_codes is [batch0][batch1][m][k] with the strides a_stride_b0,
 * a_stride_b1, a_stride_row and unit stride along k; b_codes is [batch0][batch1][n][k] (transposed_b != 0: "NT", Q.K^T) or
 * [batch0][batch1][k][n] (transposed_b == 0: "NN", P.V; n % 16 == 0) likewise.  A batch stride of 0 broadcasts that operand.
 * Each is int8 or uint8 (its code dtype), in any pair.  The K-contiguous operands (a_codes; b_codes in the NT form) are read
 * in whole 16-byte chunks up to Kp = 16 * ceil(k / 16): the caller guarantees that bytes k .. Kp - 1 of every row exist and
 * hold that operand's zero-point code (mctq_codes_im2col_pad_nhwc writes such rows).  In the NN form each 64 x 64 tile of b is
 * transposed through LDS.  All DEVICE pointers, 16-byte aligned; all strides non-negative multiples of 16.
 * One wave owns 16 rows x up to 64 columns (v_mfma_i32_16x16x64_i8); a block is four waves; grid ceil(m / 64) x
 * ceil(n / 64) x batch0 * batch1.  No atomics, no split-K.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: a bad code dtype; a zero
 * point outside its code type's range; a scale that is not finite and positive; negative extents; k outside 1 .. 32768; a
 * bad output form (mctq_qlinear_i8_codes' checks); n % 16 != 0 in the NN form; m above 2^31 - 65 or n above 65535 * 64;
 * batch0 * batch1 > 65535; negative or misaligned strides, or a row stride shorter than the (padded) row; an output of 2^63
 * bytes or more; NULL or misaligned pointers of a non-empty problem; an output that overlaps an operand.  An empty extent
 * (batch0, batch1, m or n == 0) returns 0 without a launch.
 * mctq_last_launch names the launch "qmatmul_nt" / "qmatmul_nn", op "i8 x i8" / "u8 x i8" / "i8 x u8" / "u8 x u8" (a x b),
 * U = 1 * (the column-sum MFMA ran: za' != 0) + 2 * (the row-sum MFMA ran: zb' != 0), z' = z - 128 for uint8 codes.
 */
int mctq_qmatmul_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale, int64_t a_stride_b0,
                    int64_t a_stride_b1, int64_t a_stride_row, const void* b_codes, int32_t b_code_dtype, int32_t b_zero_point,
                    float b_scale, int64_t b_stride_b0, int64_t b_stride_b1, int64_t b_stride_row, int32_t transposed_b, void* y,
                    int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                    int64_t batch0, int64_t batch1, int64_t m, int64_t n, int64_t k, void* stream);

/*
 * The join in front of an activation holder that several layers share (extension; the reference runs an ATen add, an ATen
 * ReLU and the holder as three passes): per element i of n float32 elements in storage order
 *     v        = x[i]                                   residual == NULL
 *     v        = x[i] + residual[i]                     otherwise: one float32 rounding, as ATen's add
 *     v        = v < 0 ? 0 : v                          relu != 0; a NaN stays a NaN, as torch.relu
 *     y[i]     = (clamp(rint(v * (1.0f / scale)) + zero_point, quant_min, quant_max) - zero_point) * scale
 *     codes[i] =  clamp(rint(v * (1.0f / scale)) + zero_point, quant_min, quant_max)
 * y is what mctq_fq_per_tensor_f32 writes for v (its arithmetic contract, NaN, +-inf and -0 included), codes what
 * mctq_fq_codes_per_tensor writes for it (NaN -> quant_min), as int8 (code_dtype MCTQ_CODE_I8, domain within [-128, 127]) or
 * uint8 (MCTQ_CODE_U8, within [0, 255]): (codes[i] - zero_point) * scale == y[i] bit for bit.  Either output may be NULL (not
 * both): it is then not computed, and code_dtype is ignored without codes.  All four buffers share one dense layout of n
 * elements; DEVICE pointers, 16-byte aligned.  A lane owns 16 consecutive elements (four 16-byte loads per input, four
 * 16-byte stores of y, one of codes); the last n % 16 elements go through a scalar loop.  Cached loads and stores.
 * MCTQ_E_ARG with a mctq_last_error text, before any pointer is read or anything is launched, for: n < 0; x NULL; y and codes
 * both NULL; codes with a code_dtype other than MCTQ_CODE_I8 / _U8; a clamp domain that does not fit the code type;
 * quant_min > quant_max; a clamp domain beyond 2^24 when y is wanted (the kernel's bounds are float32); a pointer that is not
 * 16-byte aligned; more than 2^31 - 1 blocks.  n == 0 returns 0 without a launch.  mctq_last_launch names the launch
 * "fq_join", op e.g. "add relu -> f32 + u8".
 */
int mctq_fq_join_f32(const float* x, const float* residual /* NULL: none */, int32_t relu,
                     float* y /* NULL: no float32 output */, void* codes /* NULL: no codes */, int32_t code_dtype,
                     int64_t n, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream);

/*
 * The same join with the residual given as integer codes (an identity branch that stays on codes: the codes another join wrote,
 * with that join's scale and zero point):
 *     r        = float(r_codes[i] - r_zero_point) * r_scale      one float32 rounding: the float32 value those codes stand for
 *     v        = x[i] + r                                         a second rounding, as ATen's add of that float32 tensor
 * and everything behind v as mctq_fq_join_f32.  r is bit for bit what mctq_fq_join_f32 (or mctq_fq_per_tensor_f32) writes as y
 * next to those codes, so the result equals mctq_fq_join_f32 on that y.  r_codes: int8 (r_code_dtype MCTQ_CODE_I8) or uint8
 * (MCTQ_CODE_U8), n of them in x's layout, a DEVICE pointer, 16-byte aligned: one 16-byte load per lane in place of four.
 * MCTQ_E_ARG as mctq_fq_join_f32, and for: r_codes NULL; an r_code_dtype other than MCTQ_CODE_I8 / _U8; an r_zero_point that is
 * no code of that type; an r_scale that is not finite and positive; r_codes not 16-byte aligned.  n == 0 returns 0 without a
 * launch.  mctq_last_launch names the launch "fq_join", op e.g. "addc(u8) relu -> u8" (the float32 form says "add").
 */
int mctq_fq_join_rc_f32(const float* x, const void* r_codes, int32_t r_code_dtype, float r_scale, int32_t r_zero_point,
                        int32_t relu, float* y /* NULL: no float32 output */, void* codes /* NULL: no codes */, int32_t code_dtype,
                        int64_t n, float scale, int32_t zero_point, int32_t quant_min, int32_t quant_max, void* stream);

/*
 * Integer consumer of the codes (extension; the reference has no counterpart): the product a wrapped
 * torch.nn.Linear computes on fake-quantized operands -- PytorchQuantizationWrapper.forward
 * (pytorch/quantize_wrapper.py:231-257: quantize the weight, then self.layer(x)) fed by an activation holder
 * (pytorch/activation_quantization_holder.py:53) -- evaluated on the 8-bit clamp indices instead:
 *     y[m][n] = float( sum_k (a[m][k] - a_zero_point) * w[n][k] ) * (a_scale * w_scales[n]) + bias[n]
 * with exact int32 accumulation on the integer matrix cores; float32 multiply, then float32 add, each
 * rounded once.  a_codes [M][K] int8 or uint8 (a_code_dtype = MCTQ_CODE_I8 / MCTQ_CODE_U8, from
 * mctq_fq_codes_per_tensor), w_codes [N][K] int8 with zero point 0 (symmetric / power-of-two weights, from
 * mctq_fq_codes_per_channel with axis 0 or _per_tensor), w_scales float32[N], w_rowsum int32[N] =
 * sum_k w[n][k] (computed once per weight), bias float32[N] or NULL, y float32 [M][N]; all DEVICE pointers,
 * code matrices 16-byte aligned, K % 16 == 0, K <= 32768.  The result differs from the float32 product of
 * the dequantized operands only by that product's own rounding (it is the exact sum, scaled once).
 */
int mctq_qlinear_i8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                    const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                    float* y, int64_t M, int64_t N, int64_t K, void* stream);

/*
 * Same product, but the result leaves as the NEXT layer's activation codes: the float32 value y[m][n] above is
 * quantized in registers exactly as mctq_fq_codes_per_tensor would quantize it,
 *     code = clamp(rint(y * (1.0f / y_scale)) + y_zero_point, y_quant_min, y_quant_max),
 * and stored as int8 / uint8 (y_code_dtype) -- for chains activation holder -> wrapped Linear -> activation
 * holder -> wrapped Linear, where the float32 tensor between two layers is only ever quantized again.
 */
int mctq_qlinear_i8_codes(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                          const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                          void* y_codes, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                          int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream);

/*
 * The same consumer for 4-bit weights (quantizers with num_bits <= 4), streamed at half a byte per weight: the
 * weight-streaming kernel only, meant for few rows (every M is computed correctly; beyond ~64 rows the int8 tiled
 * path is faster).  w_codes4 [N][K / 2] holds the codes in the CONSUMER layout, not the storage-order packing of
 * MCTQ_CODE_I4: each group of 8 consecutive k is 4 bytes, byte j = (code[k = j] & 0xF) | (code[k = j + 4] << 4),
 * two's-complement nibbles in [-8, 7]; 8-byte aligned rows (K % 16 == 0).  w_rowsum[n] = sum_k code[n][k].
 * y_code_dtype < 0: y is float32 [M][N]; otherwise y holds the next layer's codes as in mctq_qlinear_i8_codes.
 */
int mctq_qlinear_w4a8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                      const uint8_t* w_codes4, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                      void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                      int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream);

/*
 * The same consumer for LUT (codebook) weights of at most 16 entries whose codebook values are int8 (the LUT quantizers
 * with lut_values_bitwidth <= 8): q(w)[n][k] = float(lut16[idx[n][k]]) * w_scales[n] with w_scales[n] = threshold[n] /
 * 2^(lut_values_bitwidth - 1), so the product is mctq_qlinear_i8's with w[n][k] = lut16[idx[n][k]], streamed at half a
 * byte per weight and decoded index -> int8 in registers in front of the matrix instruction (exact: a byte lookup).
 * w_idx4 [N][K / 2], DEVICE: the codebook indices (mctq_lut_codes_*) in mctq_qlinear_w4a8's consumer layout with
 * UNSIGNED nibbles 0 .. 15 -- each group of 8 consecutive k is 4 bytes, byte j = idx[k = j] | idx[k = j + 4] << 4.
 * lut16: a HOST pointer to 16 int8 codebook values in list order, entries beyond the codebook's length 0.  The call
 * copies them into the kernel's arguments; they are read before it returns and never again.  Under stream capture the
 * captured launch therefore replays the values of the capture: a graph must be re-captured when the codebook changes.
 * w_rowsum[n] = sum_k lut16[idx[n][k]].  Everything else -- alignment (a_codes 16-byte, w_idx4 8-byte), K % 16 == 0,
 * K <= 32768, y_code_dtype < 0 for float32 [M][N] or the next layer's codes -- as for mctq_qlinear_w4a8.
 * mctq_last_launch names the launch "qlinear_stream_lut4".
 */
int mctq_qlinear_lut4a8(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const uint8_t* w_idx4, const int8_t* lut16, const float* w_scales, const int32_t* w_rowsum,
                        const float* bias, void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point,
                        int32_t y_quant_min, int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream);

/*
 * Row sums of activation codes: a_rowsum[m] = sum_k (a_codes[m][k] - a_zero_point) as int32 [M], DEVICE -- the per-row
 * factor of the weight zero point term of mctq_qlinear_i8_zp / mctq_qlinear_w4a8_zp below.  a_codes [M][K] int8 or uint8
 * (a_code_dtype), DEVICE, 16-byte aligned; K % 16 == 0 and K <= 32768 as for mctq_qlinear_i8; M == 0 returns 0 without a
 * launch; anything else returns MCTQ_E_ARG with a mctq_last_error text.  Lanes load 16 bytes and sum them with the packed
 * 8-bit dot product; one block per row up to 64 rows (a 32 KiB row is never walked by one wave alone), one wave per row
 * beyond; no atomics, the result does not depend on scheduling.  mctq_last_launch names the launch "codes_rowsum".
 */
int mctq_codes_rowsum(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, int32_t* a_rowsum, int64_t M,
                      int64_t K, void* stream);

/*
 * The integer consumer for weights WITH a zero point per output channel (the uniform weights quantizers, whose codes
 * (c - zero_point) * scale cover a range [min, max] that need not be symmetric):
 *     y[m][n] = float( sum_k (a[m][k] - a_zero_point) * (w[n][k] - w_zero_points[n]) ) * (a_scale * w_scales[n]) + bias[n]
 * w holds int8 codes and w_zero_points int32[N], DEVICE, are in the same domain, each in [-128, 127] (unsigned 8-bit codes c
 * in 0 .. 255 with zero point z are passed as c - 128 and z - 128; codes of at most 4 bits as c - 8 and z - 8).  The sum is
 * exact int32 -- |a - za| <= 255, |w - zw| <= 255 and K <= 32768 bound it by 255 * 255 * 32768 = 2 130 739 200 < 2^31 --
 * and one float32 multiply and one float32 add follow, each rounded once.  It is evaluated as
 *     sum_k a w  -  a_zero_point * w_rowsum[n]  -  w_zero_points[n] * a_rowsum[m]
 * with w_rowsum[n] = sum_k w[n][k] as for mctq_qlinear_i8 and a_rowsum int32[M], DEVICE, from mctq_codes_rowsum on the same
 * a_codes / a_zero_point (same stream, or ordered before this call); the terms reach 2^30, so the kernels add them in
 * wrapping arithmetic and only the total has to fit.  Both new pointers are required.  y_code_dtype < 0: y is float32
 * [M][N]; otherwise y holds the next layer's codes as in mctq_qlinear_i8_codes.  Everything else as for mctq_qlinear_i8.
 * Launch shapes: the weight-streaming and LDS-tiled kernels under the same cost model and "ql_variant" key; the
 * register-pinned whole-tile kernels do not take zero points, so large whole-tile products run on the ~1.5 POP/s tiled
 * kernels instead of the 2.2 POP/s ones, and ql_variant 2544 / 2548 / 2560 returns MCTQ_E_ARG here.  mctq_last_launch marks
 * the form that ran: "...<u8 x i8 zp,...>".
 */
int mctq_qlinear_i8_zp(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                       const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                       void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                       int32_t y_quant_max, const int32_t* w_zero_points, const int32_t* a_rowsum, int64_t M, int64_t N,
                       int64_t K, void* stream);

/*
 * The same for packed 4-bit codes: mctq_qlinear_w4a8's arguments and layout (two's-complement nibbles in [-8, 7]) plus
 * w_zero_points int32[N] in the same domain and a_rowsum int32[M] as above; w_rowsum[n] = sum_k code[n][k].
 */
int mctq_qlinear_w4a8_zp(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                         const uint8_t* w_codes4, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                         void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                         int32_t y_quant_max, const int32_t* w_zero_points, const int32_t* a_rowsum, int64_t M, int64_t N,
                         int64_t K, void* stream);

/*
 * The integer consumer with the residual add and the ReLU of a residual join in its epilogue (the last 1x1 convolution of a
 * residual block, which then emits the next block's codes itself instead of writing float32 for a mctq_fq_join_* launch):
 *     v       = float( sum_k (a[m][k] - a_zero_point) * w[n][k] ) * (a_scale * w_scales[n])     as mctq_qlinear_i8
 *     v       = v + bias[n]                     if bias
 *     v       = v + r[m][n]                     one float32 add, not contracted
 *     v       = v < 0 ? 0 : v                   if relu: a NaN stays a NaN and -0.0 stays -0.0, the join's expression
 *     y[m][n] = v (y_code_dtype < 0: float32), or the code of v in the output form, as mctq_qlinear_i8_codes
 * residual is [M][N] row-major like y, DEVICE.  r_code_dtype < 0: const float*, 4-byte aligned, r = residual[m * N + n] (r_scale
 * and r_zero_point unused).  r_code_dtype MCTQ_CODE_I8 / MCTQ_CODE_U8: int8 / uint8 codes of another quantizer,
 * r = fma(float(code - r_zero_point), r_scale, +0) -- the value mctq_fq_join_rc_f32 reads its residual as, i.e. bit for bit the
 * float32 tensor written next to those codes; r_zero_point must be a code of that type and r_scale finite and positive.
 * The register of v holds exactly the float32 value mctq_qlinear_i8 would have stored, and the add, the ReLU and the code are
 * the join's own operations on it: the result is bit for bit that of mctq_qlinear_i8 followed by mctq_fq_join_f32 /
 * mctq_fq_join_rc_f32 (codes) or by a float32 add and ReLU (float32 output).  MCTQ_E_ARG for residual == NULL, a misaligned
 * float32 residual and a y whose bytes overlap the residual's; an empty problem (M == 0 or N == 0) returns 0 without a launch.
 * Everything else as for mctq_qlinear_i8.  No weight zero points.  Launch shapes: the weight-streaming and LDS-tiled kernels
 * under the same cost model and "ql_variant" key; the register-pinned whole-tile kernels are not built for a residual, so large
 * whole-tile products run on the ~1.5 POP/s tiled kernels, and ql_variant 2544 / 2548 / 2560 returns MCTQ_E_ARG here.
 * mctq_last_launch marks the form that ran: "...<u8 x i8 res(u8) relu,...>" (res(i8), res(f32); "relu" only when set).
 */
int mctq_qlinear_i8_res(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                        const void* residual, int32_t r_code_dtype, float r_scale, int32_t r_zero_point, int32_t relu,
                        void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                        int32_t y_quant_max, int64_t M, int64_t N, int64_t K, void* stream);

/*
 * The integer consumers with a Hardswish / Hardsigmoid in front of the codes they emit (wrapped layer -> Hardswish -> holder ->
 * wrapped layer without the float32 tensors in between):
 *     v       = float( sum ... ) * (a_scale * w_scales[n]) (+ bias[n])                  as mctq_qlinear_i8 / mctq_qconv_dw_i8
 *     act 1:  v = v * min(max(v + 3, 0), 6) * (1.0f / 6.0f)                             hardswish
 *     act 2:  v =     min(max(v + 3, 0), 6) * (1.0f / 6.0f)                             hardsigmoid
 *     y       = the code of v in the output form, as mctq_qlinear_i8_codes
 * The expression is evaluated left to right with one float32 rounding per operation; max / min are a < b ? b : a and
 * b < a ? b : a (a NaN stays a NaN and then codes to y_quant_min; hardswish(-inf) = -inf * 0 = NaN).  This is what ATen's GPU
 * kernels evaluate: F.hardswish / F.hardsigmoid of a float32 GPU tensor give these bits for every one of the 2^32 float32 bit
 * patterns (tools/hard_act_probe.py).  ATen's CPU kernels divide by 6 instead of multiplying by 1.0f / 6.0f and differ from it in
 * the last bit for about a quarter (hardswish) / a thirtieth (hardsigmoid) of the patterns.  The register of v holds exactly
 * the float32 value the plain entry point would have stored, so the codes are bit for bit those of the plain entry point
 * followed by ATen's GPU activation and mctq_fq_codes_per_tensor.
 * mctq_qlinear_i8_act: the arguments of mctq_qlinear_i8_codes and act in front of M; int8 weights without zero points, no
 * residual.  mctq_qconv_dw_i8_act: the arguments of mctq_qconv_dw_i8 and act in front of batch; weights with or without
 * zero points.  MCTQ_E_ARG for an act other than 1 and 2 and for y_code_dtype < 0 (codes are the only output: the sign of a
 * zero never shows); everything else as for the plain entry points, an empty problem returns 0 without a launch.
 * Launch shapes of the product: the weight-streaming and LDS-tiled kernels under the same cost model and "ql_variant" key;
 * the register-pinned whole-tile kernels are not built for an activation (as for a residual), so large whole-tile products
 * run on the tiled kernels and ql_variant 2544 / 2548 / 2560 returns MCTQ_E_ARG here.
 * mctq_last_launch names the activation: "...<u8 x i8 hardswish,...>" / "...<i8 x i8 zp hardsigmoid,...>".
 */
int mctq_qlinear_i8_act(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                        const int8_t* w_codes, const float* w_scales, const int32_t* w_rowsum, const float* bias,
                        void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min,
                        int32_t y_quant_max, int32_t act, int64_t M, int64_t N, int64_t K, void* stream);
int mctq_qconv_dw_i8_act(const void* a_codes, int32_t a_code_dtype, int32_t a_zero_point, float a_scale,
                         const int8_t* w_codes, const float* w_scales, const int32_t* w_zero_points, const float* bias,
                         void* y, int32_t y_code_dtype, float y_scale, int32_t y_zero_point, int32_t y_quant_min, int32_t y_quant_max,
                         int32_t act, int64_t batch, int64_t height, int64_t width, int64_t channels,
                         int32_t kh, int32_t kw, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w,
                         int32_t dil_h, int32_t dil_w, void* stream);

/*
 * Tuning hook (benchmarks only): selects the launch variant used by later calls on any thread.
 *   key "nt"     : 1 = non-temporal loads and stores (default), 2 = non-temporal loads with cached stores
 *   key "cached_store_max_mb" : with nt = 1, outputs of at most this many MiB are stored through the caches
 *                  (mode 2) so that a consumer launched right after finds them in L2 / the Infinity Cache; default 32, 0 = never
 *   key "unroll" : upper bound of the 16-byte accesses in flight per lane the affine kernels choose from (1, 2 or 4; default 4)
 *   key "heavy_unroll" : the decision-table LUT kernels' lane-vectors per tile (0 = automatic, 1, 2 or 4)
 *   key "rowsteps" : per-channel rows of two or three whole 256-lane-vector steps: 0 = one- / two-step tiles inside a row
 *                  (rows_kernel), 1 = four steps per block across row boundaries (rowsteps_kernel), 2 (default) = rowsteps_kernel
 *                  when its grid is one round of resident blocks, where it measured 5-10 % faster (64 MiB launches)
 *   key "ql_variant" : mctq_qlinear_i8 launch shape: 0 = automatic (cost model, csrc/mctq_qlinear.hip: qlinear_dispatch), or ONE of
 *                  the kernels that choice can select: 181 / 182 / 184 (weight streaming, 16 / 32 / 64 rows per pass), 83233, 86433,
 *                  86633, 812613 (8-wave ring tiles 32x32 ... 128x64), 166623, 1612623 (16-wave), 612, 1212, 662 (two-buffer tiles),
 *                  2544, 2548 (wave-wide tiles), 2560 (256 x 256 ping-pong)
 *   key "ql_band" : tile rows per XCD band of the tiled kernel (0 = automatic); "ql_rot", "ql_stagger": experiments of the
 *                  tiled kernel (K rotation between blocks sharing a weight tile; half of the waves copy after multiplying), 0 / 1, default 0
 *   key "paced" : the affine per-tensor launch through flat_paced_kernel (flat_kernel's tile under another order of waits: loads
 *                  128 clocks apart, every load landed before the first store, every store completed before the next lane-vector):
 *                  0 = never, 1 (default) = launches that fill 3/4 ... 1 round of resident blocks, where it measured 4-6 % faster
 *                  (48-64 MiB of traffic on this chip; 3-9 % slower outside), 2 = every launch for which launch_flat chooses the
 *                  four-vector tile (at least two such blocks per CU; smaller tensors keep flat_kernel's narrower tiles).
 *                  The same key sends symmetric float32 per-channel launches of that window (whole-vector rows) through
 *                  shortrows_kernel with paced stores: 2048 x 4096 12.4 -> 11.3 us, 32768 x 256 12.3 -> 11.3 (16-bit: not taken, +3 %)
 *   key "shortrows" : affine per-channel tensors through shortrows_kernel (per-lane parameter reads behind the tile's data loads,
 *                  no LDS window): 0 = never, 1 (default) = where it measured faster (16-bit storage: every short or ragged row
 *                  shape, and long rows of launches that fill 7/8 ... 1 round of resident blocks; float32: rows of 4 ... 31
 *                  elements), 2 = every eligible tensor (rows of at least one lane-vector, fewer than 2^24 elements per row)
 *   key "filldrain" : symmetric float32 per-channel rows that are a whole number of four-vector tiles (4096 elements) through
 *                  rows_kernel_finetail: rows_kernel's blocks, the last half round of tiles of the launch cut into four blocks of one
 *                  lane-vector per lane each, so that the end of the launch is spread over four times as many blocks and CUs:
 *                  0 = never (rows_kernel), 1 (default) = launches of at least 9/8 rounds of resident blocks (8 per CU), where it
 *                  measured faster (4096 x 4096 22.2 -> 21.55 us; 1-4 % up to four rounds, 0.2-0.8 % at six and eight), 2 = every
 *                  eligible launch that reaches the rows shape (those inside the "paced" window go to that kernel first).
 *                  Launches with a zero-point table and 16-bit storage are never eligible.
 *   key "concat_copy" : mctq_codes_concat_nhwc, operands in the output's own form: 1 (default) = their lanes store what they loaded,
 *                  0 = they run the requantization arithmetic like every other operand (the bytes are the same: the tests' proof)
 *   key "avgpool_form" : mctq_codes_avgpool_nhwc: 0 (default) = the launcher chooses between the lane and the split form, 1 = the lane
 *                  form, 2 = the split form (the bytes are the same: the sums are integers)
 *   key "upsample_form" : mctq_codes_upsample_nhwc: 0 (default) = the launcher chooses (replicate for integer factors with
 *                  2 <= factor_h * factor_w <= 16, where it measured 1.8 - 2.3 x faster at batch 64 and equal at batch 1; gather
 *                  elsewhere), 1 = the gather form, 2 = the replicate form where eligible (integer factors with
 *                  factor_h * factor_w <= 16; gather elsewhere).  The bytes are the same: every output is one input's code
 *   key "im2col_grain" : mctq_codes_im2col_pad_nhwc: bytes per load piece, 0 (default) = by rule (4 where channels % 4 == 0, 1
 *                  elsewhere), 1 = byte loads, 4 = dword loads (MCTQ_E_ARG from the entry point where channels % 4 != 0).  The
 *                  bytes are the same
 *   key "table_chunks" : mctq_codes_table: 16-byte chunks per lane, 1, 2 or 4 (default 4).  The bytes are the same
 * Only variants a default dispatcher can select are instantiated; every value of every key is exercised by the GPU tests.
 * Returns 0, or MCTQ_E_ARG for an unknown key/value.  Numerical results never depend on it.
 */
int mctq_set_tuning(const char* key, int32_t value);

/*
 * Diagnostic: checks the LUT kernels' shared-divisor division (reciprocal + two exact FMA residual
 * corrections) against the compiler's IEEE division for ALL 2^32 float32 numerators, for each of
 * divisors[n_div] (device float32).  mismatches[n_div] (device uint64, zeroed by the caller) receives the
 * number of numerators whose quotient differs inside the domain where the last bit can matter
 * (2^-40 <= |x/d| < 2^59); outside it the two results must agree on sign and saturation (a NaN numerator comes
 * out saturated low: the kernels test the input itself for NaN).
 */
int mctq_selftest_division(const float* divisors, int32_t n_div, uint64_t* mismatches, void* stream);

/*
 * Diagnostic: checks the five-instruction reciprocal the channel-last and short-row launches use for a lane's own scales
 * (v_rcp_f32 + two Newton steps with exact FMA residuals; csrc/mctq_kernels.hpp: recip_exact) against the compiler's IEEE
 * 1.0f / d for EVERY float32 bit pattern with 2^-100 <= |d| <= 2^100 (outside that range the kernels use the IEEE division).
 * out3 (device uint64[3], zeroed by the caller) receives {patterns checked, mismatches, one mismatching pattern + 1}.
 */
int mctq_selftest_reciprocal(uint64_t* out3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCTQ_HIP_H */
