"""Integer consumers of the quantizers' codes (extension; SURVEY §8(f) row 2 -- not part of the reference API).

The reference re-quantizes a wrapped layer's weight on every forward and then runs the float32 layer on the
dequantized tensors (``PytorchQuantizationWrapper.forward``, pytorch/quantize_wrapper.py:231-257, fed by
``PytorchActivationQuantizationHolder.forward``, pytorch/activation_quantization_holder.py:53).  Both operands of
that product are integers times a scale, so on MI355X the product itself can run on the 8-bit clamp indices:

    y[m][n] = float(sum_k (qa[m][k] - za) * qw[n][k]) * (sa * sw[n]) + bias[n]

LUT (codebook) weights with int8 codebook values are the same product with ``qw[n][k] = lut[index[n][k]]`` and
``sw[n] = threshold[n] / 2^(lut_values_bitwidth - 1)``; codebooks of at most 16 entries are also kept as packed 4-bit
indices, which ``mctq_qlinear_lut4a8`` streams at half a byte per weight when there are few rows.

``QuantizedLinear`` keeps the weight's int8 codes (refreshed when the weight tensor changes), turns the incoming
activation into codes with the activation quantizer's own parameters (``mctq_fq_codes_per_tensor``) and calls
``mctq_qlinear_i8`` (include/mctq_hip.h): 1 byte per weight streamed instead of 4 B read + 4 B written by the
fake-quant kernel and 4 B read again by the float32 GEMM.  The result is the exact integer sum scaled once; it
differs from the reference's float32 product only by that product's own accumulation rounding.

Uniform weights (a range [min, max] with a zero point per output channel) are the product with ``qw[n][k] - zw[n]`` in
place of ``qw[n][k]``:

    sum_k (qa - za) * (qw - zw[n]) = sum_k qa * qw - za * w_rowsum[n] - zw[n] * a_rowsum[m],   a_rowsum[m] = sum_k (qa[m][k] - za)

-- the kernels' sum and first correction, plus one int32 per activation row (``mctq_codes_rowsum``, one more small launch)
and one per output channel in the epilogue (``mctq_qlinear_i8_zp`` / ``mctq_qlinear_w4a8_zp``).  The register-pinned
whole-tile kernels do not take zero points: large whole-tile products with uniform weights run on the ~1.5 POP/s tiled
kernels, not the 2.2 POP/s ones.

Convolutions are the same product over a patch matrix (``QuantizedConv2d``: ``ops.codes_im2col`` gathers the NHWC activation
codes into ``[B * Ho * Wo, kh * kw * C]`` rows, the weight codes are kept as ``[O, kh, kw, C]``); a padded tap holds the zero-point
code ``za`` and so adds ``(za - za) * qw = 0``.  A pointwise stride-1 convolution needs no patch matrix (``QuantizedConv1x1``).

Depthwise convolutions (``groups == in_channels == out_channels``: the 3x3 layer between the two pointwise convolutions of a
MobileNet-style block) have no reduction over channels and so no patch matrix worth building: ``QuantizedDepthwiseConv2d`` runs
``mctq_qconv_dw_i8``, a direct convolution on the NHWC codes with the weight codes kept as ``[kh, kw, C]`` -- 1 byte read per
input element, ``kh * kw`` integer multiply-accumulates per output element, the same epilogue and output forms.  With it the
expand -> depthwise -> project layers of such a block can be chained on codes.

The other grouped convolutions (``2 <= groups``, ``Cg = in_channels / groups`` a multiple of 4: the 3x3 layer of a ResNeXt or RegNet
bottleneck, ShuffleNet's grouped pointwise layers) are G small products: ``QuantizedGroupedConv2d`` (opt-in, ``grouped=True``) runs
``mctq_qconv_grouped_i8``, a direct convolution on the NHWC codes on the integer matrix cores -- no patch matrix, one launch for all
groups, the weight codes kept as ``[O, kh, kw, Cg]`` and zero-padded to ``[G, Ogp, Kgp]`` for the kernel, the same epilogue and output
forms.  Layers with 1 to 3 channels per group stay on the float32 path.

Transposed convolutions (``nn.ConvTranspose2d`` with ``groups == 1`` and dilation 1: the learned upsampling of a decoder stage) are
one stride-1 correlation per output phase ``((oy + ph) mod sh, (ox + pw) mod sw)``: ``QuantizedConvTranspose2d`` (opt-in,
``transposed=True``) runs ``mctq_qconv_transposed_i8``, all ``sh * sw`` phases in one launch on the integer matrix cores, the weight
codes kept as ``[O, kh, kw, C]`` and per phase as ``[P, Op, Kp]`` for the kernel, the same epilogue and output forms.

Holders with several users (the end of a residual block: the next block's first convolution, and its identity add or its
downsample convolution) are ``fuse_linear_consumers_fx(..., shared_holders=True)``'s: such a holder becomes a ``QuantizedJoin``,
which folds the residual add and the ReLU in front of it and returns both the fake-quantized float32 tensor, for the users that
stay in float32, and the codes, for the consumers that replace the wrapped layers -- ``mctq_fq_join_f32``, one launch that reads
both operands once (13 bytes per element against 28 for add, ReLU, holder and codes as four passes); both outputs are bit for
bit what the separate launches give.

``fuse_linear_consumers_fx(..., shared_holders=True, stay_on_codes=True)`` then keeps the activations between those layers on
codes: a ReLU, ReLU6 or Hardtanh between a consumer and a holder that only consumers read is a narrower clamp of the codes the
consumer emits itself (``folded_clamp``: the code function is monotone, so clamping the value is clamping the code), and a
residual join reads its identity operand as the codes of the join in front (``mctq_fq_join_rc_f32``: ``(code - zp) * scale`` is
that join's float32 output bit for bit), which then no longer writes float32 -- 6 bytes per element instead of 13.

``fuse_linear_consumers_fx(..., stay_on_codes=True, fused_residuals=True)`` folds the residual joins that are left into the
product in front of them: the block's last convolution reads the identity branch -- the codes of the join in front, or the
downsample branch's float32 output -- in its own epilogue, adds it, applies the ReLU and emits the next block's codes
(``mctq_qlinear_i8_res``): about 2 bytes per element where the product and the join moved 10, and one launch less per block.

``fuse_linear_consumers_fx(..., stay_on_codes=True, hard_activations=True)`` does for Hardswish and Hardsigmoid what
``stay_on_codes`` does for the clamp activations, except that these two are no clamps of the codes: the consumer in front applies
them to its float32 value in its own epilogue, with the float32 expression of ATen's GPU kernels, and emits the holder's codes
(``mctq_qlinear_i8_act``, ``mctq_qconv_dw_i8_act``; ``emit_act``) -- MobileNetV3's layers and the gate of an SE block.

A max pool between a holder and wrapped layers stays on codes with ``pools=True`` (both rewrites): the holder's float32 output
is ``float(code - zp) * scale`` with ``scale > 0``, monotone in the code and never NaN, so the pool of that output is the
dequantized pool of the codes bit for bit.  ``QuantizedMaxPool2d`` (``mctq_codes_maxpool_nhwc``) pools the codes -- a padded tap
is ignored, it stands for -inf and not for the zero point -- and the convolutions behind it become consumers of the pooled codes.

A channel concatenation between holders stays on codes with ``fuse_linear_consumers_fx(..., concats=True)``: every operand
holder's float32 output is ``float(code - zp_i) * scale_i`` bit for bit and ``torch.cat`` only moves data, so the codes the holder
behind the concatenation gives are the operands' codes requantized one by one into its form.  ``QuantizedConcat``
(``mctq_codes_concat_nhwc``) does that in one launch, 1 byte read and 1 written per element, and the layers and pools behind
the holder become consumers of its codes; with ``stay_on_codes=True`` the branch convolutions emit the operands' codes.

An average pool between two holders stays on codes with ``avg_pools=True`` (both rewrites): holder A -> average pool -> holder B,
through at most one flatten behind a global pool, becomes one ``QuantizedAvgPool2d`` (``mctq_codes_avgpool_nhwc``) -- classifier
heads (``AdaptiveAvgPool2d(1)`` / ``x.mean((2, 3))`` -> holder -> flatten -> Linear), SE squeezes, Inception's 3 x 3 branch.  The
contract: S, the sum of ``code - zp_a`` over the window's taps inside the image, is an exact integer (at most 65536 taps:
255 * 65536 < 2^24), and then in float32, each step rounded once, ``v = S * scale_a``, ``m = v / div`` with PyTorch's divisor,
``code = clamp(rint(m * (1 / scale_b)) + zp_b, qmin, qmax)``.  Exactness: where ``scale_a`` and every divisor are powers of two
these are bit for bit the codes B gives any float32 average pool of A's output; everywhere else the exact mean rounded twice,
which can differ from a float32 chain by one code, and only next to a rounding tie (ATen's own average pools do not agree
with each other in the last bit).  Limits: per-tensor quantizers of at most 8 bits whose zero points are codes of their type;
the kernel takes C % 16 == 0 and at most 65536 taps, anything else and CPU tensors run the same contract with torch ops.
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

An elementwise multiply between holders stays on codes with ``fuse_linear_consumers_fx(..., muls=True)``: holders A, G -> ``torch.mul``
-> holder M, the multiply of a squeeze-and-excitation block or a gated layer.  Both operands are ``float(code - zp) * scale`` bit for
bit, ``torch.mul`` is one IEEE float32 multiplication and M codes every element by itself, so M's code is a function of the two operand
codes and nothing is approximated.  ``QuantizedMul`` (``mctq_codes_mul_nhwc``) does that in one launch, 1 byte read and 1 written per
element of the large tensor; the gate ``[B, C, 1, 1]`` may arrive as codes or as the float32 values in front of its holder, which the
kernel codes itself.  With ``shared_holders=True`` and ``avg_pools=True`` the holder in front of an SE block never writes float32.
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

A nearest upsample behind a holder stays on codes with ``upsamples=True`` (both rewrites): holder A -> ``nn.Upsample`` /
``F.interpolate`` ("nearest", "nearest-exact") -> holder B, the low-resolution branch of a decoder stage.  Nearest interpolation only
moves data, so B's codes are A's codes gathered through the upsample's index map and requantized one by one: ``QuantizedUpsample``
(``mctq_codes_upsample_nhwc``) does that in one launch, 1 byte read and 1 written per output element, and with ``concats=True``
A -> upsample -> B -> cat([B, S]) -> C -> conv runs holder to holder on codes.
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

Layers whose K is no multiple of 16 -- a CNN's stem, bottleneck widths of 24 / 40 / 72, SE squeeze widths -- run on codes with
``any_channels=True`` (both rewrites; ``QuantizedLinear``, ``QuantizedConv1x1``, ``QuantizedConv2d``): the weight rows are kept padded with
the code 0 to ``Kp = 16 * ceil(K / 16)`` columns and the activation rows are written at that pitch with the zero-point code in their
tail (``ops.codes_im2col(..., pad_to=16)``, ``mctq_codes_im2col_pad_nhwc``).  A padded column adds ``qa * 0`` to the sum, 0 to the weight's
row sum and ``za - za`` to the activation's, so the product kernels are unchanged and the result is the product over K columns exactly.
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

The smooth activations between two holders -- sigmoid, SiLU, GELU, tanh, Mish, ELU, LeakyReLU, ... -- stay on codes with
``activation_tables=True`` (both rewrites): holder A -> 1 to 4 elementwise activations -> holder B.  A's float32 output takes at most
256 values, ``f`` maps each value by itself and B codes each element by itself, so B's code is a function of A's code: a 256-entry byte
table, built by running the replaced call itself on the 256 dequantized values on the tensor's device.  ``QuantizedActivationTable``
(``mctq_codes_table``) applies it in one launch, 1 byte read and 1 written per element, for any element and channel count.  The table is
the definition: on the GPU, where ATen applies one scalar functor per element whatever its position, the codes are bit for bit those
of the float32 chain (tests/test_gpu_table_consumer.py, every accepted function); on the CPU, where ATen's vector body and scalar
tail round differently, they equal the chain's wherever its float32 value equals the table's and are within one code next to a
rounding tie elsewhere.  Out of scope: the lookup inside the producing consumer's epilogue (``emit_table``, beside ``emit_act``).
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

The activation x activation products stay on codes with ``fuse_linear_consumers_fx(..., matmuls=True)``: ``torch.matmul`` / ``@`` /
``torch.bmm`` of two holder outputs through reshapes and permutes -- the ``Q @ K.transpose(-1, -2)`` and ``P @ V`` of every attention
block as an MCT export of a ViT, DeiT, Swin or BERT decomposes it.  Both operands are ``float(code - zp) * scale`` bit for bit, so the
product is the exact integer ``sum_k (qa - za) * (qb - zb)`` scaled once by ``float32(sa) * float32(sb)``: ``QuantizedMatmul``
(``qmatmul_i8``, ``mctq_qmatmul_i8``) runs it on the integer matrix cores with its operands taken by strides -- ``[B, T, H, D]`` storage
read as ``[B, H, T, D]`` goes to the kernel as it is -- and returns float32 or the codes of the holder behind it; with
``stay_on_codes=True`` the q / k / v consumers emit the operands' codes and the context's codes feed the projection, so Q, K, V and the
context never exist in float32.  It equals the float32 chain bit for bit where that chain's product is exact (power-of-two scales,
``255 * 255 * K < 2^24``) and differs by its accumulation rounding elsewhere.
Measured / not measured: see the README paragraph and ``profiles/EXPERIMENTS.md``.

The six modules derive from ``IntegerConsumer``, which owns what they share: the checks of the quantizers and of the float32
weight and bias, the cache of the weight's codes, the step from ``forward``'s input to activation codes, ``from_wrapper`` and
the ``emit_codes_for`` / ``emit_clamp`` output form.  ``QuantizedLinear`` is the product over ``[O, K]`` rows; ``QuantizedConv1x1``
and ``QuantizedConv2d`` are that product and derive from it; ``QuantizedDepthwiseConv2d``, ``QuantizedGroupedConv2d`` and
``QuantizedConvTranspose2d`` are not and derive from ``IntegerConsumer`` directly.  "Any integer consumer" in the graph rewrites is ``isinstance(m, IntegerConsumer)``.  The modules
without weights -- the pools, ``QuantizedUpsample``, ``QuantizedActivationTable``, ``QuantizedConcat``, ``QuantizedMul``, ``QuantizedMatmul``,
``QuantizedJoin`` --
derive from ``_OnCodes``;
``_operand_codes`` is the one step from an operand of ``forward`` to codes, theirs and the consumers' (the join has its own kernel).

CPU tensors run the same integer arithmetic with torch ops (host logic for tests, bit-identical to the kernel).
"""
import math
import operator
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from mct_quantizers_amd.hip import ops
from mct_quantizers_amd.pytorch.containers import PytorchActivationQuantizationHolder, PytorchQuantizationWrapper

_MAX_K = 32768


def _activation_code_params(q):
    """(scale, zero_point, qmin, qmax) of an affine activation quantizer."""
    if hasattr(q, "scale") and hasattr(q, "zero_point"):              # ActivationUniform
        return float(q.scale), int(q.zero_point), q.min_quantized_domain, q.max_quantized_domain
    if hasattr(q, "scales") and hasattr(q, "zero_points") and not isinstance(q.scales, torch.Tensor):
        return float(q.scales), int(q.zero_points), q.min_quantized_domain, q.max_quantized_domain
    raise TypeError(f"{type(q).__name__} is not an affine per-tensor activation quantizer")


def _check_consumer_operands(a_codes, w_scales, w_rowsum, bias, w_zero_points=None):
    """The kernels read w_scales / bias as float32 and w_rowsum / w_zero_points as int32, all on a_codes' device."""
    device = a_codes.device
    for name, t, dt in (("w_scales", w_scales, torch.float32), ("w_rowsum", w_rowsum, torch.int32), ("bias", bias, torch.float32),
                        ("w_zero_points", w_zero_points, torch.int32)):
        if t is None:
            continue
        if t.dtype != dt or t.device != device or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} tensor on {device}, got {t.dtype} on {t.device}")
    if w_zero_points is not None and w_zero_points.numel() != w_scales.numel():
        raise RuntimeError(f"w_zero_points has {w_zero_points.numel()} entries for {w_scales.numel()} output channels")


def _output_form(out_codes):
    """(tensor dtype, y_code_dtype, scale, zero_point, qmin, qmax) of the entry points whose ``y_code_dtype < 0`` means float32."""
    if out_codes is None:
        return torch.float32, -1, 1.0, 0, 0, 0
    o_scale, o_zp, o_qmin, o_qmax, lo, hi = _with_clamp(out_codes)
    tdt, ocode = ops._code_dtype(o_qmin, o_qmax)
    return tdt, ocode, float(o_scale), int(o_zp), lo, hi


def _with_clamp(out_codes):
    """``out_codes`` as (scale, zero_point, qmin, qmax, lo, hi): the quantizer's own domain [qmin, qmax] decides the code TYPE
    (a signed domain stays int8 whatever is folded into it), [lo, hi] within it is what the codes are clamped to -- the domain
    itself for the four-tuple, narrower where a clamp activation was folded in (``folded_clamp``)."""
    if len(out_codes) == 4:
        return (*out_codes, int(out_codes[2]), int(out_codes[3]))
    o_scale, o_zp, o_qmin, o_qmax, lo, hi = out_codes
    if not o_qmin <= lo <= hi <= o_qmax:
        raise ValueError(f"the narrowed clamp [{lo}, {hi}] does not lie inside the domain [{o_qmin}, {o_qmax}]")
    return o_scale, o_zp, o_qmin, o_qmax, int(lo), int(hi)


def _cpu_out_codes(y, out_codes):
    """The CPU routes' output form: ``ops.fq_codes`` of the float32 result, clamped to [lo, hi], in the domain's code type."""
    o_scale, o_zp, o_qmin, o_qmax, lo, hi = _with_clamp(out_codes)
    return ops.fq_codes(y, None, None, None, lo, hi, o_scale, o_zp).to(ops._code_dtype(o_qmin, o_qmax)[0])


_ACTS = {"hardswish": 1, "hardsigmoid": 2}


def _check_act(act, out_codes):
    """``act`` of ``qlinear_i8`` / ``qconv_dw_i8``: None, "hardswish" or "hardsigmoid"; an activation leaves as codes only."""
    if act is None:
        return None
    if act not in _ACTS:
        raise ValueError(f"act must be None, 'hardswish' or 'hardsigmoid', got {act!r}")
    if out_codes is None:
        raise ValueError(f"act={act!r} needs out_codes: the activation is folded in front of the codes, there is no float32 form")
    return act


def _cpu_epilogue(acc, a_scale, w_scales, bias, out_codes, residual=None, residual_codes=None, relu=False, act=None):
    """The CPU routes' epilogue, the kernels' own: the int32 sums ``acc`` (output channels last) times ``a_scale`` (rounded to
    float32 first) times the channel's weight scale, plus the bias; with ``residual`` (float32, or codes with
    ``residual_codes = (scale, zero_point)``, dequantized) one float32 add and, with ``relu``, ``v < 0 ? 0 : v`` -- a NaN stays a
    NaN and -0.0 stays -0.0, as in the kernel; with ``act`` ``torch.nn.functional.hardswish`` / ``hardsigmoid`` of that value (ATen's
    CPU expression, which divides by 6 where the GPU kernels multiply by 1.0f / 6.0f: see ``qlinear_i8``); float32, or the codes
    of ``out_codes``."""
    y = acc.to(torch.float32) * (torch.tensor(a_scale, dtype=torch.float64).to(torch.float32) * w_scales)
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + (residual if residual_codes is None else ops.dequantize_codes(residual, *residual_codes))
        if relu:
            y = torch.where(y < 0, torch.zeros((), dtype=torch.float32, device=y.device), y)
    if act is not None:
        y = getattr(torch.nn.functional, act)(y)
    return y if out_codes is None else _cpu_out_codes(y, out_codes)


def _check_residual(a_codes, n, residual, residual_codes, relu, w_zero_points):
    """The residual operand of ``qlinear_i8`` as ``(residual, (scale, zero_point) or None)``, or ``(None, None)``."""
    if residual is None:
        if residual_codes is not None:
            raise ValueError("residual_codes describes the residual: it needs one")
        if relu:
            raise ValueError("relu=True needs a residual: the ReLU behind a product alone is a clamp of its codes (folded_clamp)")
        return None, None
    if w_zero_points is not None:
        raise NotImplementedError("a residual together with weight zero points")
    if not isinstance(residual, torch.Tensor) or residual.dtype not in (torch.float32, torch.int8, torch.uint8):
        raise TypeError(f"the residual must be a float32 tensor or int8 / uint8 codes, got {getattr(residual, 'dtype', type(residual).__name__)}")
    if residual.device != a_codes.device or tuple(residual.shape) != (a_codes.shape[0], n):
        raise RuntimeError(f"the residual must be [{a_codes.shape[0]}, {n}] on {a_codes.device}, got {tuple(residual.shape)} on "
                           f"{residual.device}")
    if residual.dtype == torch.float32:
        if residual_codes is not None:
            raise ValueError("residual_codes given with a float32 residual")
        return residual, None
    if residual_codes is None:
        raise ValueError("a residual given as codes needs residual_codes=(scale, zero_point)")
    r_scale, r_zp = float(residual_codes[0]), int(residual_codes[1])
    lo, hi = (0, 255) if residual.dtype == torch.uint8 else (-128, 127)
    if not lo <= r_zp <= hi:
        raise ValueError(f"the residual's zero point {r_zp} is no {residual.dtype} code")
    if not 0.0 < r_scale < float("inf"):
        raise ValueError("the residual's scale must be finite and positive")
    return residual, (r_scale, r_zp)


def folded_clamp(form, a: float, b: float):
    """[lo, hi]: the clamp of the codes of ``form = (scale, zero_point, qmin, qmax)`` that stands for ``clamp(v, a, b)`` in front
    of the quantizer.  The code function c(v) = clamp(rint(v * inv) + zp, qmin, qmax) is monotone non-decreasing in v, so
    c(min(max(v, a), b)) = min(max(c(v), c(a)), c(b)): lo = c(a), hi = c(b), computed here in the kernels' float32 arithmetic
    (float32 ``1.0f / scale``, a float32 multiply, round-half-even, a float32 add of the zero point).  ``a = -inf`` / ``b = inf``
    leave that side at the domain's end.  The one difference: a NaN stays a NaN through torch's clamp and then codes to qmin,
    while the narrowed clamp gives lo -- a consumer's output is an exact integer sum times finite scales plus a bias, so it is
    NaN only if a scale or a bias is."""
    import numpy as np
    scale, zp, qmin, qmax = form
    if not a <= b:
        raise ValueError(f"clamp range [{a}, {b}] is empty")
    f32 = np.float32
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(scale)
        lo, hi = (np.minimum(np.maximum(np.rint(f32(v) * inv) + f32(zp), f32(qmin)), f32(qmax)) for v in (a, b))
    return int(lo), int(hi)


def codes_rowsum(a_codes: torch.Tensor, a_zero_point: int) -> torch.Tensor:
    """a_codes [M, K] int8/uint8 -> int32 [M], ``sum_k (a_codes[m][k] - a_zero_point)``: the per-row factor of the weight
    zero point term (``qlinear_i8(..., w_zero_points=...)``)."""
    if a_codes.dim() != 2 or a_codes.dtype not in (torch.int8, torch.uint8):
        raise TypeError(f"codes_rowsum takes int8 / uint8 codes [M, K], got {a_codes.dtype} {tuple(a_codes.shape)}")
    M, K = a_codes.shape
    if a_codes.is_cuda:
        if K % 16 or K > _MAX_K:
            raise NotImplementedError(f"mctq_codes_rowsum needs K % 16 == 0 and K <= {_MAX_K}, got K={K}")
        a_codes = a_codes.contiguous()
        out = a_codes.new_empty((M,), dtype=torch.int32)
        ops._gpu_call("mctq_codes_rowsum", a_codes, a_codes.data_ptr(), ops._code_of(a_codes), int(a_zero_point), out.data_ptr(),
                      M, K)
        return out
    ops._cpu_route_allowed()
    return (a_codes.to(torch.int32) - int(a_zero_point)).sum(dim=1, dtype=torch.int32)


def _k_mismatch(K, w_k, what):
    return RuntimeError(f"shape mismatch: activations have K={K}, {what} K={w_k}")


def _launch_consumer(name, a_codes, a_zero_point, a_scale, w, lut, w_scales, w_rowsum, bias, out_codes, w_zero_points,
                     residual=None, residual_codes=None, relu=False, act=None):
    """One consumer launch on GPU tensors.  ``name`` is the entry point of the weight format: ``mctq_qlinear_i8`` (``w``: int8
    codes [N, K]), ``mctq_qlinear_w4a8`` (packed 4-bit codes [N, K / 2]) or ``mctq_qlinear_lut4a8`` (packed 4-bit indices
    [N, K / 2] and ``lut = (the 16 codebook bytes,)``; for the others ``lut = ()``).  ``w_zero_points`` selects the ``_zp``
    form of the first two, and ``out_codes`` on int8 weights without zero points ``mctq_qlinear_i8_codes``.  ``residual``
    (checked by ``_check_residual``; int8 weights without zero points only) selects ``mctq_qlinear_i8_res``, ``act`` (checked by
    ``qlinear_i8``: codes out, no zero points, no residual) ``mctq_qlinear_i8_act``."""
    M, K = a_codes.shape
    N, w_k = w.shape
    packed = name != "mctq_qlinear_i8"
    if packed:
        w_k *= 2
    if w_k != K:
        raise _k_mismatch(K, w_k, "packed weights" if packed else "weights")
    if K % 16 or K > _MAX_K:
        raise NotImplementedError(f"{name} needs K % 16 == 0 and K <= {_MAX_K}, got K={K}")
    _check_consumer_operands(a_codes, w_scales, w_rowsum, bias, w_zero_points)
    a_codes, w = a_codes.contiguous(), w.contiguous()
    if w_zero_points is not None:
        name += "_zp"
        a_rowsum = codes_rowsum(a_codes, a_zero_point)       # named: it must outlive the launch, or y is allocated over it
        zp = (w_zero_points.data_ptr(), a_rowsum.data_ptr())
    else:
        zp = ()
        if residual is not None:
            name = "mctq_qlinear_i8_res"
        elif act is not None:
            name = "mctq_qlinear_i8_act"
        elif not packed and out_codes is not None:
            name = "mctq_qlinear_i8_codes"
    res = ()
    if residual is not None:
        residual = residual.contiguous()
        r_scale, r_zp = residual_codes or (0.0, 0)
        res = (residual.data_ptr(), -1 if residual_codes is None else ops._code_of(residual), r_scale, r_zp, int(bool(relu)))
    if name == "mctq_qlinear_i8":
        tdt, form = torch.float32, ()                   # the float32-only entry point: no output form among its arguments
    else:
        tdt, *form = _output_form(out_codes)
    y = a_codes.new_empty((M, N), dtype=tdt)
    ops._gpu_call(name, a_codes, a_codes.data_ptr(), ops._code_of(a_codes), int(a_zero_point), float(a_scale), w.data_ptr(), *lut,
                  w_scales.data_ptr(), w_rowsum.data_ptr(), None if bias is None else bias.data_ptr(), *res, y.data_ptr(), *form, *zp,
                  *(() if act is None else (_ACTS[act],)), M, N, K)
    return y


def qlinear_i8(a_codes: torch.Tensor, a_zero_point: int, a_scale: float, w_codes: torch.Tensor,
               w_scales: torch.Tensor, w_rowsum: torch.Tensor, bias: Optional[torch.Tensor],
               out_codes=None, w_zero_points: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               residual_codes=None, relu: bool = False, *, act: Optional[str] = None) -> torch.Tensor:
    """a_codes [M, K] int8/uint8, w_codes [N, K] int8 (zero point 0 unless ``w_zero_points`` is given) -> float32
    [M, N]; with ``out_codes = (scale, zero_point, qmin, qmax)`` the result leaves as the codes of that activation quantizer
    (int8 / uint8 [M, N]), bit-identical to quantizing the float32 result with ``ops.fq_codes``.  Two more entries,
    ``(..., lo, hi)`` with qmin <= lo <= hi <= qmax, clamp the codes to [lo, hi] instead (a clamp activation folded into the
    codes, ``folded_clamp``); the code type stays that of [qmin, qmax].
    ``w_zero_points`` (int32 [N], each in [-128, 127]): the weights are ``w_codes[n][k] - w_zero_points[n]``; the row sums
    of the activation codes are computed first (``codes_rowsum``) and the product runs on ``mctq_qlinear_i8_zp``.
    ``residual`` [M, N]: the second operand of a residual join, added to the result in the product's epilogue with one float32
    add -- a float32 tensor, or int8 / uint8 codes with ``residual_codes = (scale, zero_point)`` that stand for
    ``ops.dequantize_codes(residual, scale, zero_point)`` -- and with ``relu=True`` the join's ReLU behind the add, before the
    output form: bit for bit ``ops.fq_join(qlinear_i8(...), ..., residual=..., relu=...)`` of the float32 product, without that
    tensor (``mctq_qlinear_i8_res``).  Not together with ``w_zero_points`` (NotImplementedError); ``relu`` needs a residual.
    ``act`` ("hardswish" / "hardsigmoid"; needs ``out_codes``, ValueError otherwise): that activation of the float32 result in
    front of the codes, in the product's epilogue (``mctq_qlinear_i8_act``) -- on the GPU bit for bit
    ``ops.fq_codes(F.hardswish(qlinear_i8(...)), ...)`` of the float32 product, NaNs and infinities included, without the two
    float32 tensors.  The kernel evaluates what ATen's GPU kernels evaluate, ``x * min(max(x + 3, 0), 6) * (1.0f / 6.0f)``; CPU
    tensors take ``F.hardswish`` / ``F.hardsigmoid`` on the CPU, which divide by 6 -- the two float32 values differ in the last
    bit for about a quarter / a thirtieth of all inputs, so the CPU route's codes may differ from the kernel's by one at a rounding
    tie, exactly as the float32 chain's do between the two devices.  Not together with ``residual`` or ``w_zero_points``
    (NotImplementedError).  Whole-tile products with an activation run on the tiled kernels, not the register-pinned ones."""
    residual, residual_codes = _check_residual(a_codes, w_codes.shape[0], residual, residual_codes, relu, w_zero_points)
    if _check_act(act, out_codes) is not None and (residual is not None or w_zero_points is not None):
        raise NotImplementedError("an activation together with a residual or with weight zero points")
    if a_codes.is_cuda:
        return _launch_consumer("mctq_qlinear_i8", a_codes, a_zero_point, a_scale, w_codes, (), w_scales, w_rowsum, bias,
                                out_codes, w_zero_points, residual, residual_codes, relu, act)
    if w_codes.shape[1] != a_codes.shape[1]:
        raise _k_mismatch(a_codes.shape[1], w_codes.shape[1], "weights")
    ops._cpu_route_allowed()
    w32 = w_codes.to(torch.int32)
    if w_zero_points is not None:
        _check_consumer_operands(a_codes, w_scales, None, None, w_zero_points)     # dtype, device, one per output channel
        w32 = w32 - w_zero_points.to(torch.int32).reshape(-1, 1)
    acc = (a_codes.to(torch.int32) - int(a_zero_point)) @ w32.t()
    return _cpu_epilogue(acc, a_scale, w_scales, bias, out_codes, residual, residual_codes, relu, act)


def qconv_dw_i8(a_codes_nhwc: torch.Tensor, a_zero_point: int, a_scale: float, w_codes: torch.Tensor, w_scales: torch.Tensor,
                bias: Optional[torch.Tensor], kernel_size, stride=1, padding=0, dilation=1, out_codes=None,
                w_zero_points: Optional[torch.Tensor] = None, *, act: Optional[str] = None) -> torch.Tensor:
    """Depthwise convolution on codes: a_codes_nhwc [B, H, W, C] int8/uint8, w_codes [kh, kw, C] int8 (zero point 0 unless
    ``w_zero_points``, int32 [C] each in [-128, 127], is given), w_scales / bias float32 [C] -> float32 [B, Ho, Wo, C],

        y[b][oy][ox][c] = float(sum over taps inside the image of (a - a_zero_point) * (w[ky][kx][c] - zw[c])) * (a_scale * w_scales[c]) + bias[c]

    or with ``out_codes = (scale, zero_point, qmin, qmax)`` the codes of that activation quantizer, bit-identical to
    ``ops.fq_codes`` of the float32 result.  ``kernel_size``, ``stride``, ``padding`` and ``dilation`` are ints or pairs.
    ``act`` ("hardswish" / "hardsigmoid"; needs ``out_codes``): that activation of the float32 value in front of the codes, as for
    ``qlinear_i8`` (``mctq_qconv_dw_i8_act``; weights with or without zero points; the same note on the CPU route's expression).
    GPU tensors run ``mctq_qconv_dw_i8`` (C % 16 == 0, kh * kw <= 256); CPU tensors the same arithmetic with torch ops."""
    _check_act(act, out_codes)
    if not isinstance(a_codes_nhwc, torch.Tensor) or a_codes_nhwc.dim() != 4 or a_codes_nhwc.dtype not in (torch.int8, torch.uint8):
        raise TypeError("qconv_dw_i8 takes int8 / uint8 codes [B, H, W, C]")
    b, h, w_, c = a_codes_nhwc.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ho, wo) = ops._conv_geometry(h, w_, kernel_size, stride, padding, dilation, "qconv_dw_i8")
    if w_codes.dtype != torch.int8 or w_codes.device != a_codes_nhwc.device or tuple(w_codes.shape) != (kh, kw, c):
        raise TypeError(f"w_codes must be an int8 tensor [{kh}, {kw}, {c}] on {a_codes_nhwc.device}, got {w_codes.dtype} "
                        f"{tuple(w_codes.shape)} on {w_codes.device}")
    _check_consumer_operands(a_codes_nhwc, w_scales, None, bias, w_zero_points)
    if w_scales.numel() != c or (bias is not None and bias.numel() != c):
        raise RuntimeError(f"w_scales and bias must have one entry per channel ({c})")
    a_zero_point = int(a_zero_point)
    lo, hi = (0, 255) if a_codes_nhwc.dtype == torch.uint8 else (-128, 127)
    if not lo <= a_zero_point <= hi:
        raise ValueError(f"qconv_dw_i8: a_zero_point {a_zero_point} is no {a_codes_nhwc.dtype} code")
    if a_codes_nhwc.is_cuda:
        if c % 16 or kh * kw > 256:
            raise NotImplementedError(f"mctq_qconv_dw_i8 needs C % 16 == 0 and kh * kw <= 256, got C={c}, {kh}x{kw}")
        x, w_codes = a_codes_nhwc.contiguous(), w_codes.contiguous()
        tdt, *form = _output_form(out_codes)
        y = x.new_empty((b, ho, wo, c), dtype=tdt)
        ops._gpu_call("mctq_qconv_dw_i8" if act is None else "mctq_qconv_dw_i8_act", x, x.data_ptr(), ops._code_of(x), a_zero_point,
                      float(a_scale), w_codes.data_ptr(), w_scales.data_ptr(),
                      None if w_zero_points is None else w_zero_points.data_ptr(), None if bias is None else bias.data_ptr(),
                      y.data_ptr(), *form, *(() if act is None else (_ACTS[act],)), b, h, w_, c, kh, kw, sh, sw, ph, pw, dh, dw)
        return y
    ops._cpu_route_allowed()
    w32 = w_codes.to(torch.int32)
    if w_zero_points is not None:
        w32 = w32 - w_zero_points.to(torch.int32).reshape(1, 1, c)
    # a padded tap holds a - za = 0: it adds nothing
    xp = torch.nn.functional.pad(a_codes_nhwc.to(torch.int32) - a_zero_point, (0, 0, pw, pw, ph, ph))
    acc = torch.zeros((b, ho, wo, c), dtype=torch.int32)
    for ky in range(kh):
        for kx in range(kw):
            taps = xp[:, ky * dh:ky * dh + (ho - 1) * sh + 1:sh, kx * dw:kx * dw + (wo - 1) * sw + 1:sw, :]
            acc += taps * w32[ky, kx]
    return _cpu_epilogue(acc, a_scale, w_scales, bias, out_codes, act=act)


def pack_grouped_weights(w_codes: torch.Tensor, groups: int):
    """int8 codes [O, kh, kw, Cg] -> (the layout ``mctq_qconv_grouped_i8`` reads, the row sums): int8 ``[G, Ogp, Kgp]`` with
    ``Ogp = 16 * ceil(Og / 16)`` and ``Kgp = 64 * ceil(Kg / 64)``, ``Kg = kh * kw * Cg``, row ``o`` of group ``g`` output channel
    ``g * Og + o`` in the K order (ky, kx, cg), padded rows and columns the code 0; int32 ``[O]``, the sum of each channel's codes."""
    O = w_codes.shape[0]
    kg, og = math.prod(w_codes.shape[1:]), O // groups
    rows = w_codes.reshape(groups, og, kg)
    padded = torch.nn.functional.pad(rows, (0, -kg % 64, 0, -og % 16)).contiguous()
    return padded, rows.sum(dim=2, dtype=torch.int32).reshape(O).contiguous()


def qconv_grouped_i8(a_codes_nhwc: torch.Tensor, a_zero_point: int, a_scale: float, w_codes: torch.Tensor, w_scales: torch.Tensor,
                     bias: Optional[torch.Tensor], groups: int, kernel_size, stride=1, padding=0, dilation=1, out_codes=None,
                     w_zero_points: Optional[torch.Tensor] = None, *, packed=None) -> torch.Tensor:
    """Grouped convolution on codes: a_codes_nhwc [B, H, W, C] int8/uint8, ``groups >= 2`` groups of ``Cg = C / groups`` input and
    ``Og = O / groups`` output channels, w_codes [O, kh, kw, Cg] int8 (zero point 0 unless ``w_zero_points``, int32 [O] each in
    [-128, 127], is given), w_scales / bias float32 [O] -> float32 [B, Ho, Wo, O], with ``n = g * Og + o``

        y[b][oy][ox][n] = float(sum over taps inside the image, cg < Cg of (a[..][g * Cg + cg] - a_zero_point) * (w[n][ky][kx][cg] - zw[n]))
                          * (a_scale * w_scales[n]) + bias[n]

    or with ``out_codes = (scale, zero_point, qmin, qmax[, lo, hi])`` the codes of that activation quantizer, bit-identical to
    ``ops.fq_codes`` of the float32 result.  ``kernel_size``, ``stride``, ``padding`` and ``dilation`` are ints or pairs.
    GPU tensors run ``mctq_qconv_grouped_i8`` (Cg % 4 == 0, kh * kw * Cg <= 32768) on the padded weight layout and the row sums
    of ``pack_grouped_weights`` -- built here, or given as ``packed`` by a caller that keeps them; CPU tensors run the same integer
    arithmetic with torch ops, for any Cg."""
    if not isinstance(a_codes_nhwc, torch.Tensor) or a_codes_nhwc.dim() != 4 or a_codes_nhwc.dtype not in (torch.int8, torch.uint8):
        raise TypeError("qconv_grouped_i8 takes int8 / uint8 codes [B, H, W, C]")
    b, h, w_, c = a_codes_nhwc.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ho, wo) = ops._conv_geometry(h, w_, kernel_size, stride, padding, dilation, "qconv_grouped_i8")
    groups = int(groups)
    if groups < 2 or c % groups:
        raise ValueError(f"qconv_grouped_i8: groups={groups} must be at least 2 and divide the {c} channels")
    cg = c // groups
    if (not isinstance(w_codes, torch.Tensor) or w_codes.dtype != torch.int8 or w_codes.device != a_codes_nhwc.device or w_codes.dim() != 4
            or tuple(w_codes.shape[1:]) != (kh, kw, cg) or w_codes.shape[0] == 0 or w_codes.shape[0] % groups):
        raise TypeError(f"w_codes must be an int8 tensor [O, {kh}, {kw}, {cg}] with O a positive multiple of {groups} on "
                        f"{a_codes_nhwc.device}, got {getattr(w_codes, 'dtype', None)} {tuple(getattr(w_codes, 'shape', ()))} on "
                        f"{getattr(w_codes, 'device', None)}")
    o = w_codes.shape[0]
    og = o // groups
    _check_consumer_operands(a_codes_nhwc, w_scales, None, bias, w_zero_points)
    if w_scales.numel() != o or (bias is not None and bias.numel() != o):
        raise RuntimeError(f"w_scales and bias must have one entry per output channel ({o})")
    a_zero_point = int(a_zero_point)
    lo, hi = (0, 255) if a_codes_nhwc.dtype == torch.uint8 else (-128, 127)
    if not lo <= a_zero_point <= hi:
        raise ValueError(f"qconv_grouped_i8: a_zero_point {a_zero_point} is no {a_codes_nhwc.dtype} code")
    if a_codes_nhwc.is_cuda:
        if cg % 4 or kh * kw * cg > _MAX_K:
            raise NotImplementedError(f"mctq_qconv_grouped_i8 needs Cg % 4 == 0 and kh * kw * Cg <= {_MAX_K}, got Cg={cg}, {kh}x{kw}")
        w_padded, w_rowsum = pack_grouped_weights(w_codes, groups) if packed is None else packed
        _check_consumer_operands(a_codes_nhwc, w_scales, w_rowsum, None)
        want = (groups, -(-og // 16) * 16, -(-(kh * kw * cg) // 64) * 64)
        if (w_padded.dtype != torch.int8 or w_padded.device != a_codes_nhwc.device or tuple(w_padded.shape) != want
                or not w_padded.is_contiguous() or w_rowsum.numel() != o):
            raise TypeError(f"packed must be pack_grouped_weights' (int8 {list(want)}, int32 [{o}]) on {a_codes_nhwc.device}")
        x = a_codes_nhwc.contiguous()
        tdt, *form = _output_form(out_codes)
        y = x.new_empty((b, ho, wo, o), dtype=tdt)
        ops._gpu_call("mctq_qconv_grouped_i8", x, x.data_ptr(), ops._code_of(x), a_zero_point, float(a_scale), w_padded.data_ptr(),
                      w_scales.data_ptr(), w_rowsum.data_ptr(), None if w_zero_points is None else w_zero_points.data_ptr(),
                      None if bias is None else bias.data_ptr(), y.data_ptr(), *form, b, h, w_, c, o, groups, kh, kw, sh, sw, ph, pw,
                      dh, dw)
        return y
    ops._cpu_route_allowed()
    w32 = w_codes.to(torch.int32)
    if w_zero_points is not None:
        w32 = w32 - w_zero_points.to(torch.int32).reshape(o, 1, 1, 1)
    w32 = w32.reshape(groups, og, kh, kw, cg)
    # a padded tap holds a - za = 0: it adds nothing
    xp = torch.nn.functional.pad(a_codes_nhwc.to(torch.int32) - a_zero_point, (0, 0, pw, pw, ph, ph))
    xp = xp.reshape(b, h + 2 * ph, w_ + 2 * pw, groups, cg)
    acc = torch.zeros((b, ho, wo, groups, og), dtype=torch.int32)
    for ky in range(kh):
        for kx in range(kw):
            taps = xp[:, ky * dh:ky * dh + (ho - 1) * sh + 1:sh, kx * dw:kx * dw + (wo - 1) * sw + 1:sw]
            acc += torch.einsum("bhwgc,goc->bhwgo", taps, w32[:, :, ky, kx])
    return _cpu_epilogue(acc.reshape(b, ho, wo, o), a_scale, w_scales, bias, out_codes)


_MAX_TRANSPOSED_STRIDE = 4                               # mctq_qconv_transposed_i8 keeps its per-phase tables at this size


def _transposed_taps(k: int, s: int):
    """Taps per residue of one axis of a transposed convolution: ``T(r) = max(0, ceil((k - r) / s))`` for r < s."""
    return [max(0, -(-(k - r) // s)) for r in range(s)]


def _transposed_geometry(h: int, w: int, kernel_size, stride, padding, output_padding, caller: str):
    """A transposed convolution (dilation 1) of an ``h`` x ``w`` image, its arguments ints or pairs -> the pairs ``(kh, kw),
    (sh, sw), (ph, pw), (oph, opw)`` and the output size ``(ho, wo)``, ``ho = (h - 1) * sh - 2 * ph + kh + oph``; ValueError, in
    ``caller``'s name, for arguments PyTorch refuses."""
    (kh, kw), (sh, sw) = ops._pair(kernel_size, "kernel_size", caller), ops._pair(stride, "stride", caller)
    (ph, pw), (oph, opw) = ops._pair(padding, "padding", caller), ops._pair(output_padding, "output_padding", caller)
    if min(kh, kw, sh, sw) < 1 or min(ph, pw, oph, opw) < 0:
        raise ValueError(f"{caller}: kernel_size and stride must be at least 1, padding and output_padding at least 0")
    if oph >= sh or opw >= sw:
        raise ValueError(f"{caller}: output_padding {oph}x{opw} must be smaller than the stride {sh}x{sw}")
    ho, wo = (h - 1) * sh - 2 * ph + kh + oph, (w - 1) * sw - 2 * pw + kw + opw
    if ho <= 0 or wo <= 0:
        raise ValueError(f"{caller}: padding {ph}x{pw} leaves no output of the {h}x{w} image")
    return (kh, kw), (sh, sw), (ph, pw), (oph, opw), (ho, wo)


def pack_transposed_weights(w_codes: torch.Tensor, stride):
    """int8 codes [O, kh, kw, C] of a transposed convolution -> (the layout ``mctq_qconv_transposed_i8`` reads, the row sums):
    int8 ``[P, Op, Kp]`` with ``P = sh * sw`` phases, ``Op = 16 * ceil(O / 16)`` and ``Kp = 64 * ceil(max K / 64)``; phase
    ``ry * sw + rx`` holds the taps ``ky = ry + sh * ty``, ``kx = rx + sw * tx`` -- row ``o`` in the K order (ty, tx, c),
    ``K = Ty * Tx * C`` columns -- padded rows and columns the code 0; int32 ``[P, O]``, the sum of each row's codes."""
    sh, sw = ops._pair(stride, "stride", "pack_transposed_weights")
    o, kh, kw, c = w_codes.shape
    kp = -(-(_transposed_taps(kh, sh)[0] * _transposed_taps(kw, sw)[0] * c) // 64) * 64
    packed = w_codes.new_zeros((sh * sw, -(-o // 16) * 16, kp))
    rowsum = torch.zeros((sh * sw, o), dtype=torch.int32, device=w_codes.device)
    for ry in range(sh):
        for rx in range(sw):
            rows = w_codes[:, ry::sh, rx::sw, :].reshape(o, -1)
            packed[ry * sw + rx, :o, :rows.shape[1]] = rows
            rowsum[ry * sw + rx] = rows.sum(dim=1, dtype=torch.int32)
    return packed, rowsum


def qconv_transposed_i8(a_codes_nhwc: torch.Tensor, a_zero_point: int, a_scale: float, w_codes: torch.Tensor, w_scales: torch.Tensor,
                        bias: Optional[torch.Tensor], kernel_size, stride=1, padding=0, output_padding=0, out_codes=None,
                        w_zero_points: Optional[torch.Tensor] = None, *, packed=None) -> torch.Tensor:
    """Transposed convolution on codes (``nn.ConvTranspose2d`` with ``groups == 1`` and ``dilation == 1``): a_codes_nhwc
    [B, H, W, C] int8/uint8, w_codes [O, kh, kw, C] int8 (zero point 0 unless ``w_zero_points``, int32 [O] each in [-128, 127], is
    given), w_scales / bias float32 [O] -> float32 [B, Ho, Wo, O], ``Ho = (H - 1) * sh - 2 * ph + kh + oph``,

        y[b][oy][ox][o] = float(sum over c, ky, kx with iy * sh = oy + ph - ky, ix * sw = ox + pw - kx inside the image of
                                (a[b][iy][ix][c] - a_zero_point) * (w[o][ky][kx][c] - zw[o])) * (a_scale * w_scales[o]) + bias[o]

    or with ``out_codes = (scale, zero_point, qmin, qmax[, lo, hi])`` the codes of that activation quantizer, bit-identical to
    ``ops.fq_codes`` of the float32 result.  ``kernel_size``, ``stride``, ``padding`` and ``output_padding`` are ints or pairs.
    GPU tensors run ``mctq_qconv_transposed_i8`` (C % 16 == 0, strides <= 4, at most 32768 columns per phase) on the per-phase
    weight layout and the row sums of ``pack_transposed_weights`` -- built here, or given as ``packed`` by a caller that keeps
    them; CPU tensors run the same integer arithmetic with torch ops (one strided ``+=`` per tap into a padded canvas, then the
    crop), for any C and any stride."""
    if not isinstance(a_codes_nhwc, torch.Tensor) or a_codes_nhwc.dim() != 4 or a_codes_nhwc.dtype not in (torch.int8, torch.uint8):
        raise TypeError("qconv_transposed_i8 takes int8 / uint8 codes [B, H, W, C]")
    b, h, w_, c = a_codes_nhwc.shape
    (kh, kw), (sh, sw), (ph, pw), (oph, opw), (ho, wo) = _transposed_geometry(h, w_, kernel_size, stride, padding, output_padding,
                                                                              "qconv_transposed_i8")
    if (not isinstance(w_codes, torch.Tensor) or w_codes.dtype != torch.int8 or w_codes.device != a_codes_nhwc.device or w_codes.dim() != 4
            or tuple(w_codes.shape[1:]) != (kh, kw, c) or w_codes.shape[0] == 0):
        raise TypeError(f"w_codes must be an int8 tensor [O, {kh}, {kw}, {c}] with O >= 1 on {a_codes_nhwc.device}, got "
                        f"{getattr(w_codes, 'dtype', None)} {tuple(getattr(w_codes, 'shape', ()))} on {getattr(w_codes, 'device', None)}")
    o = w_codes.shape[0]
    _check_consumer_operands(a_codes_nhwc, w_scales, None, bias, w_zero_points)
    if w_scales.numel() != o or (bias is not None and bias.numel() != o):
        raise RuntimeError(f"w_scales and bias must have one entry per output channel ({o})")
    a_zero_point = int(a_zero_point)
    lo, hi = (0, 255) if a_codes_nhwc.dtype == torch.uint8 else (-128, 127)
    if not lo <= a_zero_point <= hi:
        raise ValueError(f"qconv_transposed_i8: a_zero_point {a_zero_point} is no {a_codes_nhwc.dtype} code")
    if a_codes_nhwc.is_cuda:
        max_k = _transposed_taps(kh, sh)[0] * _transposed_taps(kw, sw)[0] * c
        if c % 16 or max(sh, sw) > _MAX_TRANSPOSED_STRIDE or max_k > _MAX_K:
            raise NotImplementedError(f"mctq_qconv_transposed_i8 needs C % 16 == 0, strides <= {_MAX_TRANSPOSED_STRIDE} and at most "
                                      f"{_MAX_K} columns per phase, got C={c}, {kh}x{kw}, stride {sh}x{sw}")
        w_packed, w_rowsum = pack_transposed_weights(w_codes, (sh, sw)) if packed is None else packed
        _check_consumer_operands(a_codes_nhwc, w_scales, w_rowsum, None)
        want = (sh * sw, -(-o // 16) * 16, -(-max_k // 64) * 64)
        if (w_packed.dtype != torch.int8 or w_packed.device != a_codes_nhwc.device or tuple(w_packed.shape) != want
                or not w_packed.is_contiguous() or tuple(w_rowsum.shape) != (sh * sw, o)):
            raise TypeError(f"packed must be pack_transposed_weights' (int8 {list(want)}, int32 [{sh * sw}, {o}]) on {a_codes_nhwc.device}")
        x = a_codes_nhwc.contiguous()
        tdt, *form = _output_form(out_codes)
        y = x.new_empty((b, ho, wo, o), dtype=tdt)
        ops._gpu_call("mctq_qconv_transposed_i8", x, x.data_ptr(), ops._code_of(x), a_zero_point, float(a_scale), w_packed.data_ptr(),
                      w_scales.data_ptr(), w_rowsum.data_ptr(), None if w_zero_points is None else w_zero_points.data_ptr(),
                      None if bias is None else bias.data_ptr(), y.data_ptr(), *form, b, h, w_, c, o, kh, kw, sh, sw, ph, pw, oph, opw)
        return y
    ops._cpu_route_allowed()
    w32 = w_codes.to(torch.int32)
    if w_zero_points is not None:
        w32 = w32 - w_zero_points.to(torch.int32).reshape(o, 1, 1, 1)
    a32 = a_codes_nhwc.to(torch.int32) - a_zero_point
    # the scatter form: input pixel (iy, ix) adds its tap (ky, kx) to canvas pixel (iy * sh + ky, ix * sw + kx); the output is
    # the canvas from (ph, pw) on, and rows / columns the output padding adds beyond the last tap stay 0
    canvas = torch.zeros((b, (h - 1) * sh + kh + oph, (w_ - 1) * sw + kw + opw, o), dtype=torch.int32)
    for ky in range(kh):
        for kx in range(kw):
            canvas[:, ky:ky + (h - 1) * sh + 1:sh, kx:kx + (w_ - 1) * sw + 1:sw] += torch.einsum("bhwc,oc->bhwo", a32, w32[:, ky, kx])
    acc = canvas[:, ph:ph + ho, pw:pw + wo].contiguous()
    return _cpu_epilogue(acc, a_scale, w_scales, bias, out_codes)


_MATMUL_MAX_BATCH = 65535                                # grid z of one mctq_qmatmul_i8 launch: beyond it the batch is split along B0
_MATMUL_MAX_M, _MATMUL_MAX_N = (1 << 31) - 65, 65535 * 64


def _matmul_form(codes, form, name):
    """``(scale, zero_point)`` of an operand of ``qmatmul_i8`` (the first two entries of ``form``), checked against its codes."""
    if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.int8, torch.uint8):
        raise TypeError(f"qmatmul_i8 takes int8 / uint8 codes, got {getattr(codes, 'dtype', type(codes).__name__)} for {name}")
    if codes.dim() < 1:
        raise RuntimeError(f"qmatmul_i8: {name} must have at least one dimension")
    scale, zp = float(form[0]), int(form[1])
    ops._check_form("qmatmul_i8", codes.dtype, zp, scale, zp_words=f"{name}'s zero point {{}}", scale_words=f"{name}'s scale")
    return scale, zp


def _matmul_view(codes, zp, k_contiguous: bool):
    """An operand of ``mctq_qmatmul_i8`` as the kernel takes it, a view wherever that is possible: unit stride along the last
    dimension, every other stride a non-negative multiple of 16, a 16-byte aligned pointer, rows that do not overlap.  A
    K-contiguous operand whose K is no multiple of 16 is re-pitched to rows of ``Kp = 16 * ceil(K / 16)`` columns whose tail
    holds the zero-point code (``ops.codes_im2col(..., pad_to=16)``: one more launch); any other view that fails is copied."""
    rows, cols = codes.shape[-2:]
    if k_contiguous and cols % 16:
        return ops.codes_im2col(codes.reshape(-1, cols), 1, pad_to=16, pad_code=zp).reshape(*codes.shape[:-1], -1)
    strides_ok = all(codes.shape[d] == 1 or (codes.stride(d) >= 0 and codes.stride(d) % 16 == 0) for d in range(codes.dim() - 1))
    if codes.stride(-1) == 1 and strides_ok and codes.data_ptr() % 16 == 0 and (rows == 1 or codes.stride(-2) >= cols):
        return codes
    return codes.clone(memory_format=torch.contiguous_format)


def _matmul_strides(t):
    """(B0, B1, rows) strides of a 4-D view for the kernel: a dimension of size 1 is never stepped along."""
    return tuple(0 if t.shape[d] == 1 else t.stride(d) for d in range(3))


def qmatmul_i8(a_codes: torch.Tensor, a_form, b_codes: torch.Tensor, b_form, *, transposed_b: bool, out_codes=None) -> torch.Tensor:
    """Batched matrix product of two activation-code tensors: a_codes ``[..., M, K]`` and b_codes ``[..., N, K]``
    (``transposed_b=True``, the Q.K^T form, "NT") or ``[..., K, N]`` (``transposed_b=False``, the P.V form, "NN"), int8 or uint8 in any
    pair, each per-tensor affine with ``form = (scale, zero_point)``; leading dimensions broadcast as ``torch.matmul``'s do (and
    1-D operands are taken as it takes them) ->

        acc[m][n] = sum_k (a[m][k] - za) * (b[k][n] - zb)          an exact integer: K <= 32768, 255 * 255 * 32768 < 2^31
        y = float32(acc) * s,   s = float32(sa) * float32(sb)       one float32 multiply each, as ``_cpu_epilogue``

    float32, or with ``out_codes = (scale, zero_point, qmin, qmax[, lo, hi])`` the codes of that activation quantizer, bit-identical
    to ``ops.fq_codes`` of the float32 result.  No bias, no residual, no activation.

    GPU tensors with one or two batch dimensions (after broadcasting; both operands at least 2-D, one at least 3-D) run
    ``mctq_qmatmul_i8`` on views: ``[B, T, H, D]`` storage read as ``[B, H, T, D]`` goes to the kernel as it is, a broadcast operand
    with a batch stride of 0.  A view is copied only where a stride or the pointer is no multiple of 16 bytes or the last
    dimension is not contiguous; a K-contiguous operand with ``K % 16 != 0`` (the 197-wide probability rows of a ViT) is re-pitched
    to ``Kp = 16 * ceil(K / 16)`` columns with the zero-point code in the tail -- one more launch (two where the view is not
    contiguous), as ``any_channels`` costs.  More than 65535 batches are split along the first batch dimension.  Every other GPU
    case -- 2-D or 1-D operands, more than two batch dimensions, ``N % 16 != 0`` in the NN form, sizes beyond one launch -- and CPU
    tensors run the same contract with exact torch ops (CPU: an int64 product; GPU: a float64 product, exact since
    ``|acc| < 2^53``).

    Where the float32 ``torch.matmul`` of the two dequantized operands is exact (power-of-two scales, ``255 * 255 * K < 2^24``) the
    result equals that chain bit for bit; elsewhere it differs by the float32 accumulation rounding of the chain."""
    import numpy as np
    a_scale, a_zp = _matmul_form(a_codes, a_form, "a_codes")
    b_scale, b_zp = _matmul_form(b_codes, b_form, "b_codes")
    if a_codes.device != b_codes.device:
        raise RuntimeError(f"qmatmul_i8: a_codes on {a_codes.device}, b_codes on {b_codes.device}")
    transposed_b = bool(transposed_b) and b_codes.dim() >= 2              # (the transpose of a vector is the vector)
    K = a_codes.shape[-1]
    b_k = b_codes.shape[-1] if transposed_b or b_codes.dim() == 1 else b_codes.shape[-2]
    if b_k != K:
        raise _k_mismatch(K, b_k, "the second operand")
    if not 1 <= K <= _MAX_K:
        raise NotImplementedError(f"qmatmul_i8 needs 1 <= K <= {_MAX_K}, got K={K}")
    if out_codes is not None:
        _with_clamp(out_codes)
    if a_codes.is_cuda and a_codes.dim() >= 2 and b_codes.dim() >= 2 and max(a_codes.dim(), b_codes.dim()) in (3, 4):
        M, N = a_codes.shape[-2], b_codes.shape[-2 if transposed_b else -1]
        batch = torch.broadcast_shapes(a_codes.shape[:-2], b_codes.shape[:-2])
        b0, b1 = (1, *batch) if len(batch) == 1 else batch
        if (transposed_b or N % 16 == 0) and b1 <= _MATMUL_MAX_BATCH and M <= _MATMUL_MAX_M and N <= _MATMUL_MAX_N:
            tdt, *form = _output_form(out_codes)
            y = a_codes.new_empty((b0, b1, M, N), dtype=tdt)
            if y.numel():
                a4 = _matmul_view(a_codes, a_zp, True)
                b4 = _matmul_view(b_codes, b_zp, transposed_b)
                if a4.shape[:-2] != batch:
                    a4 = a4.expand(*batch, *a4.shape[-2:])
                if b4.shape[:-2] != batch:
                    b4 = b4.expand(*batch, *b4.shape[-2:])
                if len(batch) == 1:
                    a4, b4 = a4.unsqueeze(0), b4.unsqueeze(0)
                step = max(1, _MATMUL_MAX_BATCH // b1)
                for at in range(0, b0, step):
                    a_, b_ = (a4, b4) if step >= b0 else (a4[at:at + step], b4[at:at + step])
                    # (a slab of a split batch is written to a buffer of its own: its offset inside y need not be 16-byte aligned)
                    y_ = y if step >= b0 else y.new_empty((a_.shape[0], b1, M, N))
                    ops._gpu_call("mctq_qmatmul_i8", a_, a_.data_ptr(), ops._code_of(a_), a_zp, a_scale, *_matmul_strides(a_),
                                  b_.data_ptr(), ops._code_of(b_), b_zp, b_scale, *_matmul_strides(b_), int(transposed_b),
                                  y_.data_ptr(), *form, y_.shape[0], b1, M, N, K)
                    if y_ is not y:
                        y[at:at + step].copy_(y_)
            return y.reshape(*batch, M, N)
    elif not a_codes.is_cuda:
        ops._cpu_route_allowed()
    wide = torch.float64 if a_codes.is_cuda else torch.int64
    a_wide, b_wide = a_codes.to(wide) - a_zp, b_codes.to(wide) - b_zp
    acc = torch.matmul(a_wide, b_wide.transpose(-1, -2) if transposed_b else b_wide)
    with np.errstate(all="ignore"):
        s = float(np.float32(a_scale) * np.float32(b_scale))
    y = acc.to(torch.float32) * s
    return y if out_codes is None else _cpu_out_codes(y, out_codes)


def pack_w4(codes: torch.Tensor) -> torch.Tensor:
    """int8 codes in [-8, 7], [N, K] with K % 8 == 0 -> the consumer's 4-bit layout, uint8 [N, K / 2]: per group of 8
    consecutive k, byte j = (code[j] & 0xF) | (code[j + 4] << 4) (include/mctq_hip.h: mctq_qlinear_w4a8)."""
    N, K = codes.shape
    g = codes.reshape(N, K // 8, 8).to(torch.int16) & 0xF
    return (g[..., 0:4] | (g[..., 4:8] << 4)).to(torch.uint8).reshape(N, K // 2).contiguous()


def qlinear_w4a8(a_codes: torch.Tensor, a_zero_point: int, a_scale: float, w_codes4: torch.Tensor,
                 w_scales: torch.Tensor, w_rowsum: torch.Tensor, bias: Optional[torch.Tensor],
                 out_codes=None, w_zero_points: Optional[torch.Tensor] = None) -> torch.Tensor:
    """As ``qlinear_i8`` with the weights as packed 4-bit codes (``pack_w4``); GPU tensors only.  ``w_zero_points`` (int32
    [N], in the codes' domain [-8, 7]) as there, on ``mctq_qlinear_w4a8_zp``."""
    return _launch_consumer("mctq_qlinear_w4a8", a_codes, a_zero_point, a_scale, w_codes4, (), w_scales, w_rowsum, bias,
                            out_codes, w_zero_points)


_W4_MAX_ROWS = 32          # measured: beyond this the int8 kernels are faster than streaming half the bytes


def pack_lut4(indices: torch.Tensor) -> torch.Tensor:
    """uint8 codebook indices in [0, 15], [N, K] with K % 8 == 0 -> the consumer's 4-bit layout, uint8 [N, K / 2]: per
    group of 8 consecutive k, byte j = index[j] | (index[j + 4] << 4) (include/mctq_hip.h: mctq_qlinear_lut4a8)."""
    if indices.dtype != torch.uint8 or indices.dim() != 2 or indices.shape[1] % 8:
        raise ValueError(f"pack_lut4 takes uint8 indices [N, K] with K % 8 == 0, got {indices.dtype} {tuple(indices.shape)}")
    if indices.numel() and int(indices.max()) > 15:
        raise ValueError("pack_lut4: a 4-bit index is at most 15")
    N, K = indices.shape
    g = indices.reshape(N, K // 8, 8)
    return (g[..., 0:4] | (g[..., 4:8] << 4)).reshape(N, K // 2).contiguous()


def _lut16_bytes(lut16) -> bytes:
    """At most 16 integer codebook values in [-128, 127] -> the 16 host bytes mctq_qlinear_lut4a8 reads (zero padded)."""
    if isinstance(lut16, bytes):
        if len(lut16) != 16:
            raise ValueError(f"lut16 as bytes must be 16 bytes long, got {len(lut16)}")
        return lut16
    import numpy as np
    v = np.asarray(lut16.detach().cpu() if isinstance(lut16, torch.Tensor) else lut16, dtype=np.float64).reshape(-1)
    if v.size > 16 or np.any(v != np.rint(v)) or np.any(v < -128) or np.any(v > 127):
        raise ValueError("lut16 must hold at most 16 integers in [-128, 127]")
    out = np.zeros(16, dtype=np.int8)
    out[:v.size] = v.astype(np.int8)
    return out.tobytes()


def qlinear_lut4a8(a_codes: torch.Tensor, a_zero_point: int, a_scale: float, w_idx4: torch.Tensor, lut16,
                   w_scales: torch.Tensor, w_rowsum: torch.Tensor, bias: Optional[torch.Tensor],
                   out_codes=None) -> torch.Tensor:
    """As ``qlinear_i8`` with ``w_codes[n][k] = lut16[index[n][k]]``, the weights given as packed 4-bit codebook indices
    (``pack_lut4``) and ``lut16`` as at most 16 int8 codebook values on the host (a sequence, a CPU tensor or 16 bytes);
    ``w_rowsum`` is the row sum of the looked-up values.  GPU tensors only."""
    if w_idx4.dtype != torch.uint8 or w_idx4.device != a_codes.device:
        raise TypeError(f"w_idx4 must be a uint8 tensor on {a_codes.device}, got {w_idx4.dtype} on {w_idx4.device}")
    return _launch_consumer("mctq_qlinear_lut4a8", a_codes, a_zero_point, a_scale, w_idx4, (_lut16_bytes(lut16),), w_scales,
                            w_rowsum, bias, out_codes, None)


# measured (tools/lut_consumer_probe.py, table in profiles/EXPERIMENTS.md): the largest probed M at which the packed kernel beats
# mctq_qlinear_i8 on every probed shape -- at M = 8 it already loses on 28672 x 8192 and 4096 x 11008 (1.04 / 1.05)
_LUT4_MAX_ROWS = 1


def _is_lut_weights(q) -> bool:
    from mct_quantizers_amd.pytorch.quantizers.lut import WeightsLUTSymmetricInferableQuantizer
    return isinstance(q, WeightsLUTSymmetricInferableQuantizer)          # LUT-POT derives from it


def _is_uniform_weights(q) -> bool:
    from mct_quantizers_amd.pytorch.quantizers.affine import WeightsUniformInferableQuantizer
    return isinstance(q, WeightsUniformInferableQuantizer)


def _operand_codes(x, form, who, whose, *, at="", nhwc=True, float32_only=True):
    """An operand of ``forward`` as contiguous codes of ``form = (scale, zero_point, qmin, qmax)``.  int8 / uint8 tensors already
    are codes and must be of the form's type (TypeError: "... do not match ``whose``", behind ``at``); anything else is quantized
    with the form -- with ``float32_only`` only float32, every other dtype is ``who``'s TypeError.  With ``nhwc`` a 4-D operand
    (codes: NCHW-shaped, NHWC-stored) gives contiguous [N, H, W, C] codes, copied only where they are not; everything else keeps
    its shape."""
    scale, zp, qmin, qmax = form
    nhwc = nhwc and x.dim() == 4
    if x.dtype in (torch.uint8, torch.int8):
        if x.dtype != ops._code_dtype(qmin, qmax)[0]:
            raise TypeError(f"{at}activation codes of type {x.dtype} do not match {whose}")
        if not nhwc:
            return x
        codes = x.permute(0, 2, 3, 1)
        return codes if codes.is_contiguous() else codes.contiguous()
    if float32_only and x.dtype != torch.float32:
        raise TypeError(f"{who} takes float32 tensors or activation codes, got {x.dtype}")
    if nhwc:
        return ops.fq_codes_nhwc(x, qmin, qmax, scale, zp)
    return ops.fq_codes(x, None, None, None, qmin, qmax, scale, zp)


class IntegerConsumer(nn.Module):
    """``activation quantizer -> PytorchQuantizationWrapper(layer)`` evaluated on integer codes: what the four consumers share.

    ``weights_quantizer``: WeightsSymmetric / WeightsPOT (zero point 0), per tensor or per output channel
    (``channel_axis`` 0), at most 8 bits; or WeightsUniform (a zero point per tensor or per output channel, at most 8 bits:
    unsigned codes c and zero points z are kept as c - 2^(num_bits - 1) and z - 2^(num_bits - 1), both int8-ranged); or
    WeightsLUTSymmetric / WeightsLUTPOT with ``lut_values_bitwidth`` <= 8 (int8 codebook values) and at most 256 codebook
    entries, per tensor or per output channel.  ``activation_quantizer``: ActivationSymmetric / POT / Uniform, at most 8 bits.
    ``weight``: the float weight to own in place of ``layer.weight`` (a wrapper has replaced that by a plain tensor and owns the
    parameter itself).  The float weight stays the module's parameter; its codes are rebuilt when it changes.

    A subclass says which layers it takes (``eligible``, ``_takes`` for the messages), which axis of its weight holds the output
    channels (``_out_axis``: 0, and 1 for a transposed convolution -- a per-channel quantizer must run along it), in which layout it keeps the weight
    codes (``_store_weight_codes``) and runs the product (``forward``)."""

    _takes = None
    _out_axis = 0                                        # the weight's output-channel axis (1: nn.ConvTranspose2d's [C, O, kh, kw])

    def __init__(self, layer, weights_quantizer, activation_quantizer, weight=None, any_channels: bool = False):
        super().__init__()
        # (any_channels: QuantizedLinear and the convolutions that are its product; the keyword is passed on only where it is set)
        if not (self.eligible(layer, any_channels=True) if any_channels else self.eligible(layer)):
            raise TypeError(f"{type(self).__name__} takes {self._takes}")
        self._lut_weights = _is_lut_weights(weights_quantizer)
        self._uniform_weights = _is_uniform_weights(weights_quantizer)
        if self._lut_weights:
            if weights_quantizer.lut_values_bitwidth > 8:
                raise NotImplementedError("codebook values wider than 8 bits")
            if len(weights_quantizer._lut_values_np.reshape(-1)) > 256:
                raise NotImplementedError("more than 256 codebook entries")
        elif not self._uniform_weights and (not hasattr(weights_quantizer, "quantize_to_codes")
                                            or not hasattr(weights_quantizer, "threshold_np")):
            raise TypeError("the weights quantizer must be symmetric, power-of-two (zero point 0), uniform or a LUT quantizer")
        if weights_quantizer.per_channel and self._out_axis == 0 and weights_quantizer.channel_axis % 2 != 0:
            raise NotImplementedError("per-channel weight scales must run along the output channels (axis 0)")
        if weights_quantizer.per_channel and self._out_axis != 0 and weights_quantizer.channel_axis % 4 != self._out_axis:
            # (a [C, O, kh, kw] weight: scales along the input channels of a transposed convolution cannot go into an epilogue)
            raise NotImplementedError(f"per-channel weight scales must run along the output channels (axis {self._out_axis})")
        if weights_quantizer.num_bits > 8 or activation_quantizer.num_bits > 8:
            raise NotImplementedError("codes wider than 8 bits")
        weight, bias = layer.weight if weight is None else weight, layer.bias
        # The kernels read the bias as float32 and return float32: a half-precision layer stays on the fake-quant
        # path (its wrapper returns the layer's own type), it is never reinterpreted.
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
            raise TypeError(f"{type(self).__name__} takes float32 layers, got weight {getattr(weight, 'dtype', type(weight).__name__)}"
                            + ("" if bias is None else f" / bias {bias.dtype}"))
        if bias is not None and bias.device != weight.device:
            raise TypeError("weight and bias live on different devices")
        self.weight = weight                             # of the layer's own shape: the codes are taken from it in the class's layout
        self.bias = bias
        self.weights_quantizer = weights_quantizer
        self.activation_quantizer = activation_quantizer
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _activation_code_params(activation_quantizer)
        self._w_key = None
        self._w_codes = self._w_scales = None
        self._w_zps = None                               # uniform weights: int32 zero points in the stored codes' domain
        # chaining (fuse_linear_consumers(chain=True)): parameters of the activation quantizer that would quantize
        # this layer's output next; the output then leaves as that quantizer's codes
        self.emit_codes_for = None
        # fuse_linear_consumers_fx(stay_on_codes=True): (lo, hi) inside emit_codes_for's domain, the clamp that stands for a
        # ReLU / ReLU6 / Hardtanh between this layer and that quantizer (folded_clamp).  Kept apart from emit_codes_for: the
        # code type is the domain's, not the narrowed clamp's.
        self.emit_clamp = None
        # fuse_linear_consumers_fx(fused_residuals=True): the residual join behind this layer folded into its epilogue.
        # emit_residual: None, "float" (forward's second operand is a float32 tensor) or (scale, zero_point) (it is the int8 /
        # uint8 codes of that quantizer); emit_relu: the join's ReLU behind the add.  QuantizedLinear and the convolutions
        # that are its product only.
        self.emit_residual = None
        self.emit_relu = False
        # fuse_linear_consumers_fx(hard_activations=True): "hardswish" / "hardsigmoid", the activation between this layer and
        # the quantizer of emit_codes_for, applied to the float32 value in the epilogue (needs emit_codes_for; the product
        # with int8 weights without zero points and without a residual, and the depthwise convolution).
        self.emit_act = None

    def extra_repr(self) -> str:
        return "" if self.emit_act is None else f"emit_act={self.emit_act!r}"

    @classmethod
    def from_wrapper(cls, wrapper: PytorchQuantizationWrapper, activation_quantizer, any_channels: bool = False):
        quantizers = wrapper.weights_quantizers
        extra = {"any_channels": True} if any_channels else {}
        if list(quantizers) != ["weight"] or not cls.eligible(wrapper.layer, **extra):
            raise TypeError(f"expected wrapped {cls._takes} with one quantizer on 'weight'")
        # (the wrapper owns the float weight as its parameter)
        return cls(wrapper.layer, quantizers["weight"], activation_quantizer, weight=wrapper.weight, **extra)

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of this layer's activation codes: what ``emit_codes_for`` of the layer in front takes."""
        return self._a_scale, self._a_zp, self._a_qmin, self._a_qmax

    def _out_codes(self):
        """``out_codes`` of the launch: None, ``emit_codes_for``, or that with ``emit_clamp`` behind it."""
        if self.emit_codes_for is None or self.emit_clamp is None:
            return self.emit_codes_for
        return (*self.emit_codes_for, *self.emit_clamp)

    def _weight_codes(self, w):
        """The weight kind's part: (int8 codes, scales, int32 zero points or None, (indices, int8 codebook) or None); codes
        and indices shaped like the weight."""
        q = self.weights_quantizer
        if self._lut_weights:
            # q(w)[n][k] = (lut[idx] / 2^(B-1)) * thr[n] == float(lut_i8[idx]) * (thr[n] / 2^(B-1)) bit for bit (the divisor is
            # a power of two, so either side rounds once): int8 codes lut_i8[idx] with scales thr / 2^(B-1).
            idx, lut, thr = q.quantize_to_codes(w.detach())
            bits = q.lut_values_bitwidth
            lut = lut.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
            if bits > 8 or lut.numel() > 256 or not bool(((lut == lut.round()) & (lut >= -128) & (lut <= 127)).all()):
                raise RuntimeError("the codebook no longer holds at most 256 int8 values")
            lut_i8 = lut.to(torch.int8)
            scales = thr.detach().to(device=w.device, dtype=torch.float32) / float(2 ** (bits - 1))
            return lut_i8.to(w.device)[idx.long()], scales, None, (idx, lut_i8)
        codes, scales, zps = q.quantize_to_codes(w.detach())
        if not self._uniform_weights:
            if codes.dtype != torch.int8:
                raise RuntimeError("symmetric weight codes are expected to be int8")
            return codes, scales, None, None
        # unsigned codes c in 0 .. 2^bits - 1 with zero point z: both re-biased by half the domain, so that the codes are
        # int8 (at most 4 bits: [-8, 7], the packed layout's nibbles) and c - z is unchanged
        half = 2 ** (q.num_bits - 1)
        if codes.dtype != torch.uint8:
            raise RuntimeError("uniform weight codes are expected to be uint8")
        zps = zps.to(device=w.device, dtype=torch.int32).reshape(-1) - half
        if zps.numel() and (int(zps.min()) < -128 or int(zps.max()) > 127):     # (a host read, once per weight change)
            raise NotImplementedError("a weight zero point lies outside the codes' domain")
        return (codes.to(torch.int16) - half).to(torch.int8), scales, zps, None

    def _refresh_weight_codes(self):
        """Rebuilds the weight's codes, and its scales and zero points as one value per output channel, when the weight tensor
        changed; the subclass keeps the codes in its own layout (``_store_weight_codes(codes, lut)``)."""
        w = self.weight
        key = (w.data_ptr(), w._version, w.device)
        if key == self._w_key:
            return
        codes, scales, zps, lut = self._weight_codes(w)

        def per_channel(t):
            return (t.expand(w.shape[self._out_axis]) if t.numel() == 1 else t).contiguous()

        self._w_scales = per_channel(scales.to(device=w.device, dtype=torch.float32).reshape(-1))
        if zps is not None:
            self._w_zps = per_channel(zps)
        self._store_weight_codes(codes, lut)
        self._w_key = key

    def _activation_codes(self, x):
        """``forward``'s input as this layer's activation codes.  int8 / uint8 tensors already are codes (chained layers) and
        must be of the quantizer's type; anything else is quantized.  2-D rows stay rows; an [N, C, H, W] tensor (codes:
        NCHW-shaped, NHWC-stored) gives contiguous [N, H, W, C] codes."""
        return _operand_codes(x, self.activation_code_params(), type(self).__name__, "this layer's quantizer", float32_only=False)

    def _bias_for(self, codes):
        """The bias as the kernels read it, a contiguous float32 tensor on the codes' device, or None."""
        if self.bias is None:
            return None
        bias = self.bias.detach()
        if bias.dtype != torch.float32 or bias.device != codes.device or not bias.is_contiguous():
            # (.to() after construction, e.g. model.half(): convert instead of letting the kernel misread it)
            bias = bias.to(device=codes.device, dtype=torch.float32).contiguous()
        return bias


def _padding(conv):
    """(pad_h, pad_w) of a symmetrically zero-padded convolution, or None."""
    if conv.padding == "valid":
        return 0, 0
    if conv.padding == "same":
        spans = [d * (k - 1) for d, k in zip(conv.dilation, conv.kernel_size)]
        return None if any(s % 2 for s in spans) else tuple(s // 2 for s in spans)
    if isinstance(conv.padding, tuple) and len(conv.padding) == 2 and all(isinstance(p, int) and p >= 0 for p in conv.padding):
        return conv.padding
    return None


def _take_conv_geometry(consumer, conv):
    """The geometry a convolution consumer reads on ``forward``.  A tap outside the image adds nothing because it holds the
    activation's zero-point code, which therefore has to be a code."""
    _check_pad_byte(consumer)
    consumer.in_channels = conv.in_channels
    consumer.kernel_size, consumer.stride, consumer.dilation = tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.dilation)
    consumer.padding = _padding(conv)


def _check_pad_byte(consumer):
    """A padded tap or column adds nothing because it holds the activation's zero-point code, which therefore has to be a code."""
    if not consumer._a_qmin <= consumer._a_zp <= consumer._a_qmax:
        raise NotImplementedError("the activation zero point lies outside the codes' domain: it cannot be the pad byte")


def _padded_k(k: int) -> int:
    """Kp = 16 * ceil(K / 16): the row pitch of a layer taken with ``any_channels``."""
    return -(-k // 16) * 16


def _check_nchw(x, channels):
    if x.dim() != 4 or x.shape[1] != channels:
        raise RuntimeError(f"expected [N, {channels}, H, W], got {tuple(x.shape)}")


class QuantizedLinear(IntegerConsumer):
    """``activation quantizer -> PytorchQuantizationWrapper(nn.Linear)`` on integer codes (``IntegerConsumer`` for the
    quantizers it takes): the product over rows.  The weight codes are kept as ``[O, K]`` rows with their row sums; at most 4
    bits per weight -- codes, or the indices of a codebook of at most 16 entries -- are also kept packed, to stream half the
    bytes when there are few activation rows.

    ``any_channels=True`` also takes layers whose K is no multiple of 16 (the kernels' row pitch): the weight codes are then kept
    as ``[O, Kp]`` rows, ``Kp = 16 * ceil(K / 16) <= 32768``, their last ``Kp - K`` columns the code 0, and ``forward`` re-pitches
    the activation codes to ``[M, Kp]`` rows whose last columns hold the zero-point code (``ops.codes_im2col(..., pad_to=16)``,
    one more launch for a Linear or a pointwise convolution; a k x k convolution's patch matrix is gathered at that pitch in the
    first place).  A padded column adds ``qa * 0`` to the sum, 0 to the weight's row sum and ``za - za`` to the activation's, so the
    product is the product over K columns exactly, weight zero points included.  That needs the zero point inside the clamp
    domain (NotImplementedError otherwise).  Padded rows are never packed to 4 bits (index 0 of a codebook decodes to
    ``lut[0]``, not to 0).  A layer with K % 16 == 0 is the layer built without the keyword: same buffers, same launches."""

    _takes = "torch.nn.Linear layers"

    def __init__(self, linear, weights_quantizer, activation_quantizer, weight=None, any_channels: bool = False):
        super().__init__(linear, weights_quantizer, activation_quantizer, weight, any_channels)
        # [O, K] of a Linear, [O, C, 1, 1] of a pointwise and [O, C, kh, kw] of a k x k convolution
        self.out_features, self.in_features = self.weight.shape[0], math.prod(self.weight.shape[1:])
        self._w_rowsum = self._w_codes4 = None
        self._w_idx4 = self._lut16 = None                # LUT weights of at most 16 entries: packed indices + host codebook
        # any_channels: the pitch of the weight and activation rows where K is no multiple of 16; None: rows of K columns
        self._k_pitch = _padded_k(self.in_features) if any_channels and self.in_features % 16 else None
        if self._k_pitch is not None:
            if self._k_pitch > _MAX_K:
                raise TypeError(f"{type(self).__name__} takes K <= {_MAX_K} (padded to a multiple of 16), got K={self.in_features}")
            _check_pad_byte(self)

    @staticmethod
    def eligible(layer, any_channels: bool = False) -> bool:
        return isinstance(layer, nn.Linear)

    def extra_repr(self) -> str:
        parts = [super().extra_repr()] + ([] if self._k_pitch is None else [f"k_pitch={self._k_pitch}"])
        return ", ".join(p for p in parts if p)

    def _pitched_rows(self, codes):
        """Activation codes [M, K] (or NHWC [B, H, W, C] of a pointwise convolution) -> the rows the product takes: [M, K], or
        with a pitch [M, Kp], the last columns holding the zero-point code."""
        if self._k_pitch is None:
            return codes.reshape(-1, self.in_features)
        return ops.codes_im2col(codes, 1, pad_to=16, pad_code=self._a_zp)

    def _as_rows(self, t):
        """Codes or codebook indices shaped like the weight -> [O, K] in the order of the activation rows."""
        return t.reshape(self.out_features, self.in_features)            # [O, C, 1, 1] of a pointwise convolution too

    def _store_weight_codes(self, codes, lut):
        codes = self._as_rows(codes)
        if self._k_pitch is not None:                    # the code 0 in the padded columns: they add nothing to any sum
            codes = torch.nn.functional.pad(codes, (0, self._k_pitch - self.in_features))
        self._w_codes = codes.contiguous()
        self._w_rowsum = codes.sum(dim=1, dtype=torch.int32).contiguous()
        can_pack = self.weight.is_cuda and self.in_features % 16 == 0
        self._w_codes4 = pack_w4(self._w_codes) if lut is None and self.weights_quantizer.num_bits <= 4 and can_pack else None
        self._w_idx4 = self._lut16 = None
        if lut is not None and lut[1].numel() <= 16 and can_pack:
            self._w_idx4, self._lut16 = pack_lut4(self._as_rows(lut[0])), _lut16_bytes(lut[1])

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        lead = x.shape[:-1]
        if residual is not None:
            residual = residual.reshape(-1, self.out_features)
        rows = self._pitched_rows(self._activation_codes(x.reshape(-1, self.in_features)))
        return self._rows_product(rows, residual).reshape(*lead, self.out_features)

    def _residual_rows(self, residual):
        """A convolution's residual -- [B, O, Ho, Wo], NCHW-shaped and NHWC-stored as consumers and joins emit it -- as
        [B * Ho * Wo, O] rows: a view of channels-last storage, a copy of anything else."""
        if residual is None:
            return None
        if residual.dim() != 4 or residual.shape[1] != self.out_features:
            raise RuntimeError(f"expected a residual [N, {self.out_features}, H, W], got {tuple(residual.shape)}")
        rows = residual.permute(0, 2, 3, 1)
        return (rows if rows.is_contiguous() else rows.contiguous()).reshape(-1, self.out_features)

    def _rows_product(self, a_codes, residual=None):
        """This layer's activation codes [M, K] -> [M, O], float32 or the codes of ``emit_codes_for``: what the convolutions
        that are this product call with their pixels or patches as rows (their codes are checked once, not again here).
        ``residual`` [M, O], as ``emit_residual`` says: added (and ``emit_relu``) in the epilogue of ``qlinear_i8``, the one
        route that takes one."""
        self._refresh_weight_codes()
        bias = self._bias_for(a_codes)
        if (residual is not None) != (self.emit_residual is not None):
            raise RuntimeError(f"this layer was built {'with' if self.emit_residual is not None else 'without'} a residual operand")
        if residual is not None:
            as_codes = self.emit_residual != "float"
            if (residual.dtype in (torch.int8, torch.uint8)) != as_codes or (not as_codes and residual.dtype != torch.float32):
                raise TypeError(f"this layer was built for a residual operand {'as codes' if as_codes else 'in float32'}, "
                                f"got {residual.dtype}")
            return qlinear_i8(a_codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._w_rowsum, bias,
                              self._out_codes(), self._w_zps, residual, self.emit_residual if as_codes else None, self.emit_relu,
                              act=self.emit_act)
        if self.emit_act is not None:                    # (the packed 4-bit routes take no activation: int8 codes)
            return qlinear_i8(a_codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._w_rowsum, bias,
                              self._out_codes(), self._w_zps, act=self.emit_act)
        if self._w_codes4 is not None and a_codes.is_cuda and a_codes.shape[0] <= _W4_MAX_ROWS:
            return qlinear_w4a8(a_codes, self._a_zp, self._a_scale, self._w_codes4, self._w_scales, self._w_rowsum, bias,
                                self._out_codes(), self._w_zps)
        if self._w_idx4 is not None and a_codes.is_cuda and a_codes.shape[0] <= _LUT4_MAX_ROWS:
            return qlinear_lut4a8(a_codes, self._a_zp, self._a_scale, self._w_idx4, self._lut16, self._w_scales,
                                  self._w_rowsum, bias, self._out_codes())
        return qlinear_i8(a_codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._w_rowsum, bias,
                          self._out_codes(), self._w_zps)


class QuantizedConv1x1(QuantizedLinear):
    """``activation quantizer -> PytorchQuantizationWrapper(nn.Conv2d 1x1)`` on integer codes: a pointwise convolution
    (kernel 1x1, stride 1, no padding / dilation / groups -- most of the multiply-accumulates of MobileNet-style
    networks) is the same product over the channel axis for every pixel, so it runs on the same kernels with
    M = batch x height x width rows.  Channels-last inputs are quantized in place; NCHW inputs take one fused
    quantize-and-transpose pass (``mctq_fq_codes_nchw_to_nhwc``).  The result has the NCHW shape with channels-last strides."""

    _takes = "1x1, stride-1, unpadded, undilated, ungrouped nn.Conv2d layers"

    @staticmethod
    def eligible(conv, any_channels: bool = False) -> bool:
        return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
                and conv.padding in ((0, 0), 0, "valid") and conv.dilation == (1, 1) and conv.groups == 1
                and conv.padding_mode == "zeros")

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        _check_nchw(x, self.in_features)
        b, _, h, w_ = x.shape
        y = self._rows_product(self._pitched_rows(self._activation_codes(x)), self._residual_rows(residual))
        return y.reshape(b, h, w_, self.out_features).permute(0, 3, 1, 2)


class QuantizedConv2d(QuantizedLinear):
    """``activation quantizer -> PytorchQuantizationWrapper(nn.Conv2d)`` on integer codes for any kernel size, stride,
    dilation and symmetric zero padding (``groups == 1``): the convolution is the same product over a patch matrix.  The
    activation codes, NHWC, are gathered into ``[B * Ho * Wo, kh * kw * C]`` rows (``ops.codes_im2col``, one
    data-movement launch; the matrix is materialised: kh * kw bytes per input element at stride 1) and the weight codes
    are kept as ``[O, kh, kw, C]`` rows; everything behind that is QuantizedLinear's.  Padded taps hold the activation's
    zero-point code, so they add ``(za - za) * qw = 0`` to the sum: zero padding is exact.  That needs the zero point
    inside the clamp domain, ``in_channels % 16 == 0`` (any ``in_channels`` with ``any_channels=True``: the rows of the patch matrix
    are then padded to a multiple of 16 columns, ``QuantizedLinear``) and ``kh * kw * in_channels <= 32768``.  ``padding="same"`` only
    where every ``dilation * (k - 1)`` is even (PyTorch pads one side more otherwise).  The result has the NCHW shape
    with channels-last strides."""

    _takes = f"ungrouped, zero-padded (symmetric) nn.Conv2d layers with in_channels % 16 == 0 and kh * kw * in_channels <= {_MAX_K}"

    def __init__(self, conv, weights_quantizer, activation_quantizer, weight=None, any_channels: bool = False):
        super().__init__(conv, weights_quantizer, activation_quantizer, weight, any_channels)
        _take_conv_geometry(self, conv)

    @staticmethod
    def eligible(conv, any_channels: bool = False) -> bool:
        """``any_channels`` only lifts ``in_channels % 16 == 0`` (to Kp = 16 * ceil(K / 16) <= 32768, which K <= 32768 is)."""
        return (isinstance(conv, nn.Conv2d) and conv.groups == 1 and conv.padding_mode == "zeros"
                and _padding(conv) is not None and (any_channels or conv.in_channels % 16 == 0)
                and conv.kernel_size[0] * conv.kernel_size[1] * conv.in_channels <= _MAX_K)

    def _as_rows(self, t):
        kh, kw = self.kernel_size
        return t.reshape(self.out_features, self.in_channels, kh, kw).permute(0, 2, 3, 1).reshape(self.out_features, self.in_features)

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        _check_nchw(x, self.in_channels)
        b, _, h, w_ = x.shape
        rows = ops.codes_im2col(self._activation_codes(x), self.kernel_size, self.stride, self.padding, self.dilation, self._a_zp,
                                pad_to=1 if self._k_pitch is None else 16)
        y = self._rows_product(rows, self._residual_rows(residual))
        ho, wo = map(ops._conv_out_size, (h, w_), self.kernel_size, self.stride, self.padding, self.dilation)
        return y.reshape(b, ho, wo, self.out_features).permute(0, 3, 1, 2)


class QuantizedDepthwiseConv2d(IntegerConsumer):
    """``activation quantizer -> PytorchQuantizationWrapper(depthwise nn.Conv2d)`` on integer codes: ``groups == in_channels ==
    out_channels`` (channel multiplier 1), any kernel size with ``kh * kw <= 256``, stride, dilation and symmetric zero
    padding, ``in_channels % 16 == 0``.  There is no reduction over channels, so no patch matrix and no product over rows:
    ``qconv_dw_i8`` convolves the NHWC activation codes directly with the weight codes kept as ``[kh, kw, C]`` (a few KiB: no
    row sums, no packed 4-bit copies).  A tap outside the image adds nothing, which the kernel gets by giving it the
    activation's zero-point code: that needs the zero point inside the clamp domain.  All four weight families of
    IntegerConsumer (a per-channel axis is the output-channel axis 0 of the ``[C, 1, kh, kw]`` weight); chaining and
    ``emit_codes_for`` as for the other consumers.  The result has the NCHW shape with channels-last strides."""

    _takes = ("zero-padded (symmetric) nn.Conv2d layers with groups == in_channels == out_channels, in_channels % 16 == 0 "
              "and kh * kw <= 256")

    def __init__(self, conv, weights_quantizer, activation_quantizer, weight=None):
        super().__init__(conv, weights_quantizer, activation_quantizer, weight)
        _take_conv_geometry(self, conv)

    @staticmethod
    def eligible(conv) -> bool:
        return (isinstance(conv, nn.Conv2d) and conv.groups == conv.in_channels == conv.out_channels
                and conv.padding_mode == "zeros" and _padding(conv) is not None and conv.in_channels % 16 == 0
                and conv.kernel_size[0] * conv.kernel_size[1] <= 256)

    def _store_weight_codes(self, codes, lut):
        kh, kw = self.kernel_size
        self._w_codes = codes.reshape(self.in_channels, kh, kw).permute(1, 2, 0).contiguous()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_nchw(x, self.in_channels)
        self._refresh_weight_codes()
        codes = self._activation_codes(x)
        y = qconv_dw_i8(codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._bias_for(codes), self.kernel_size,
                        self.stride, self.padding, self.dilation, self._out_codes(), self._w_zps, act=self.emit_act)
        return y.permute(0, 3, 1, 2)


class QuantizedGroupedConv2d(IntegerConsumer):
    """``activation quantizer -> PytorchQuantizationWrapper(grouped nn.Conv2d)`` on integer codes: ``2 <= groups`` with
    ``Cg = in_channels / groups`` a multiple of 4 (which leaves the depthwise layers to QuantizedDepthwiseConv2d), any ``Og =
    out_channels / groups``, any kernel size with ``kh * kw * Cg <= 32768``, stride, dilation and symmetric zero padding -- the
    3 x 3 layer of a ResNeXt or RegNet bottleneck, ShuffleNet's grouped pointwise layers.  It is G small products, run by
    ``qconv_grouped_i8`` as one direct convolution on the NHWC codes (``mctq_qconv_grouped_i8``: the integer matrix cores, no
    patch matrix, one launch for all groups).  The weight codes are kept as ``[O, kh, kw, Cg]`` and, for the kernel, zero-padded
    to ``[G, Ogp, Kgp]`` with their row sums (``pack_grouped_weights``).  A tap outside the image adds nothing, which the kernel
    gets by giving it the activation's zero-point code: that needs the zero point inside the clamp domain.  All weight families
    of IntegerConsumer (a per-channel axis is the output-channel axis 0); chaining, ``emit_codes_for`` and ``emit_clamp`` as for
    the other consumers; no residual and no ``emit_act``.  The result has the NCHW shape with channels-last strides."""

    _takes = (f"zero-padded (symmetric) nn.Conv2d layers with groups >= 2, in_channels / groups a multiple of 4 and "
              f"kh * kw * in_channels / groups <= {_MAX_K}")

    def __init__(self, conv, weights_quantizer, activation_quantizer, weight=None):
        super().__init__(conv, weights_quantizer, activation_quantizer, weight)
        _take_conv_geometry(self, conv)
        self.groups, self.out_channels = conv.groups, conv.out_channels
        self._w_packed = None                            # pack_grouped_weights of the codes: the kernel's layout, the row sums

    @staticmethod
    def eligible(conv) -> bool:
        if not isinstance(conv, nn.Conv2d) or conv.groups < 2 or QuantizedDepthwiseConv2d.eligible(conv):
            return False
        cg = conv.in_channels // conv.groups
        return (cg % 4 == 0 and conv.padding_mode == "zeros" and _padding(conv) is not None
                and conv.kernel_size[0] * conv.kernel_size[1] * cg <= _MAX_K)

    def extra_repr(self) -> str:
        parts = [super().extra_repr(), f"groups={self.groups}"]
        return ", ".join(p for p in parts if p)

    def _store_weight_codes(self, codes, lut):
        self._w_codes = codes.reshape(self.weight.shape).permute(0, 2, 3, 1).contiguous()          # [O, Cg, kh, kw] -> [O, kh, kw, Cg]
        self._w_packed = pack_grouped_weights(self._w_codes, self.groups)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_nchw(x, self.in_channels)
        if self.emit_residual is not None or self.emit_act is not None:
            raise NotImplementedError("QuantizedGroupedConv2d takes no residual and no activation in its epilogue")
        self._refresh_weight_codes()
        codes = self._activation_codes(x)
        y = qconv_grouped_i8(codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._bias_for(codes), self.groups,
                             self.kernel_size, self.stride, self.padding, self.dilation, self._out_codes(), self._w_zps,
                             packed=self._w_packed)
        return y.permute(0, 3, 1, 2)


class QuantizedConvTranspose2d(IntegerConsumer):
    """``activation quantizer -> PytorchQuantizationWrapper(nn.ConvTranspose2d)`` on integer codes: ``groups == 1``, ``dilation ==
    1``, ``in_channels % 16 == 0``, strides of at most 4, any kernel size, padding and output padding whose largest phase has at
    most 32768 columns (``ceil(kh / sh) * ceil(kw / sw) * in_channels``) -- the learned 2 x 2 stride-2 upsampling of a U-Net
    decoder, the 4 x 4 stride-2 one of a segmentation head or a GAN generator, 3 x 3 stride 2 with ``output_padding=1``.  The
    output pixels of one phase ``((oy + ph) mod sh, (ox + pw) mod sw)`` are a plain stride-1 correlation of the NHWC codes with
    that phase's sub-kernel, so ``qconv_transposed_i8`` runs the layer as ``sh * sw`` such products in one launch
    (``mctq_qconv_transposed_i8``: the integer matrix cores, no zero-stuffed input, no patch matrix).  The ``[C, O, kh, kw]``
    weight's codes are kept as ``[O, kh, kw, C]`` and, for the kernel, per phase as ``[P, Op, Kp]`` with their row sums
    (``pack_transposed_weights``).  A tap outside the image adds nothing, which the kernel gets by giving it the activation's
    zero-point code: that needs the zero point inside the clamp domain.  All weight families of IntegerConsumer; the output
    channels are the weight's axis 1, so a per-channel quantizer runs along axis 1 (one along the input channels, axis 0,
    cannot go into an epilogue and is refused); chaining, ``emit_codes_for`` and ``emit_clamp`` as for the other consumers; no
    residual and no ``emit_act``.  The result has the NCHW shape with channels-last strides."""

    _takes = (f"zero-padded nn.ConvTranspose2d layers with groups == 1, dilation 1, in_channels a multiple of 16, strides <= "
              f"{_MAX_TRANSPOSED_STRIDE} and ceil(kh / sh) * ceil(kw / sw) * in_channels <= {_MAX_K}")
    _out_axis = 1

    def __init__(self, conv, weights_quantizer, activation_quantizer, weight=None):
        super().__init__(conv, weights_quantizer, activation_quantizer, weight)
        _check_pad_byte(self)
        self.in_channels, self.out_channels = conv.in_channels, conv.out_channels
        self.kernel_size, self.stride = tuple(conv.kernel_size), tuple(conv.stride)
        self.padding, self.output_padding = tuple(conv.padding), tuple(conv.output_padding)
        self._w_packed = None                            # pack_transposed_weights of the codes: the kernel's layout, the row sums

    @staticmethod
    def eligible(conv) -> bool:
        if not isinstance(conv, nn.ConvTranspose2d) or conv.groups != 1 or tuple(conv.dilation) != (1, 1):
            return False
        (kh, kw), (sh, sw) = conv.kernel_size, conv.stride
        return (conv.in_channels % 16 == 0 and conv.padding_mode == "zeros" and max(sh, sw) <= _MAX_TRANSPOSED_STRIDE
                and _transposed_taps(kh, sh)[0] * _transposed_taps(kw, sw)[0] * conv.in_channels <= _MAX_K)

    def extra_repr(self) -> str:
        parts = [super().extra_repr(), f"kernel_size={self.kernel_size}, stride={self.stride}"]
        return ", ".join(p for p in parts if p)

    def _store_weight_codes(self, codes, lut):
        self._w_codes = codes.reshape(self.weight.shape).permute(1, 2, 3, 0).contiguous()          # [C, O, kh, kw] -> [O, kh, kw, C]
        self._w_packed = pack_transposed_weights(self._w_codes, self.stride)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_nchw(x, self.in_channels)
        if self.emit_residual is not None or self.emit_act is not None:
            raise NotImplementedError("QuantizedConvTranspose2d takes no residual and no activation in its epilogue")
        self._refresh_weight_codes()
        codes = self._activation_codes(x)
        y = qconv_transposed_i8(codes, self._a_zp, self._a_scale, self._w_codes, self._w_scales, self._bias_for(codes),
                                self.kernel_size, self.stride, self.padding, self.output_padding, self._out_codes(), self._w_zps,
                                packed=self._w_packed)
        return y.permute(0, 3, 1, 2)


def _ints_or_pair(v) -> bool:
    one = lambda e: isinstance(e, int) and not isinstance(e, bool)                     # noqa: E731
    return one(v) or (isinstance(v, (tuple, list)) and len(v) == 2 and all(one(e) for e in v))


class _OnCodes(nn.Module):
    """Base of the modules without weights that read or write activation codes -- the pools, QuantizedUpsample, QuantizedActivationTable,
    QuantizedConcat, QuantizedMul, QuantizedMatmul and QuantizedJoin: with the wrappers, the holders and the integer consumers, the leaves of the graph rewrite's tracer."""


class QuantizedMaxPool2d(_OnCodes):
    """``activation holder -> nn.MaxPool2d`` on integer codes, for the integer consumers behind the pool.  The holder's float32
    output is ``float(code - zp) * scale`` with ``scale > 0``: monotone non-decreasing in the code and never NaN, so the pool of
    the holder's output is the dequantized pool of the codes bit for bit, and the layers behind see a tensor whose codes are the
    pooled codes -- ``ops.codes_maxpool`` (``mctq_codes_maxpool_nhwc``), 1 byte read and a quarter of one written per element
    of a stride-2 pool, where ATen's pool reads 4 and writes 1 and the layers behind quantize that again.

    ``forward`` takes the codes of ``activation_quantizer`` (int8 / uint8 of its code type, NCHW-shaped and NHWC-stored, as the
    consumers and joins emit them) or a float32 [N, C, H, W] tensor, which it quantizes with the holder's parameters
    (``ops.fq_codes_nhwc``); it returns the pooled codes, NCHW-shaped and NHWC-stored, which an ``IntegerConsumer`` of the same
    quantizer takes as they are.  It has no weights and is no ``IntegerConsumer``; ``activation_code_params`` is theirs, so the
    modules in front and behind agree on the form.  GPU tensors need ``C % 16 == 0``."""

    def __init__(self, pool, activation_quantizer):
        super().__init__()
        if not self.eligible(pool):
            raise TypeError("QuantizedMaxPool2d takes torch.nn.MaxPool2d layers without return_indices, their kernel_size, stride, "
                            "padding and dilation ints or pairs, padding at most half the kernel size")
        if activation_quantizer.num_bits > 8:
            raise NotImplementedError("codes wider than 8 bits")
        self.activation_quantizer = activation_quantizer
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _activation_code_params(activation_quantizer)
        ops._code_dtype(self._a_qmin, self._a_qmax)            # (raises for a domain that is no 8-bit code)
        self.kernel_size = ops._pair(pool.kernel_size, "kernel_size", "QuantizedMaxPool2d")
        self.stride = self.kernel_size if pool.stride is None else ops._pair(pool.stride, "stride", "QuantizedMaxPool2d")
        self.padding = ops._pair(pool.padding, "padding", "QuantizedMaxPool2d")
        self.dilation = ops._pair(pool.dilation, "dilation", "QuantizedMaxPool2d")
        self.ceil_mode = bool(pool.ceil_mode)

    @staticmethod
    def eligible(pool) -> bool:
        if type(pool) is not nn.MaxPool2d or pool.return_indices or not isinstance(pool.ceil_mode, bool):
            return False
        stride = pool.kernel_size if pool.stride is None else pool.stride
        if not all(_ints_or_pair(v) for v in (pool.kernel_size, stride, pool.padding, pool.dilation)):
            return False
        k, s, p, d = (ops._pair(v, "", "QuantizedMaxPool2d") for v in (pool.kernel_size, stride, pool.padding, pool.dilation))
        return min(*k, *s, *d) >= 1 and min(p) >= 0 and p[0] <= k[0] // 2 and p[1] <= k[1] // 2

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes this pool reads and returns: what ``emit_codes_for`` of the layer in
        front takes."""
        return self._a_scale, self._a_zp, self._a_qmin, self._a_qmax

    def extra_repr(self) -> str:
        return (f"kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, dilation={self.dilation}, "
                f"ceil_mode={self.ceil_mode}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise RuntimeError(f"expected [N, C, H, W], got {tuple(x.shape)}")
        codes = _operand_codes(x, self.activation_code_params(), "QuantizedMaxPool2d", "this pool's quantizer")
        y = ops.codes_maxpool(codes, self.kernel_size, self.stride, self.padding, self.dilation, self.ceil_mode)
        return y.permute(0, 3, 1, 2)


def _code_form(q):
    """(scale, zero_point, qmin, qmax) of a quantizer of at most 8 bits whose codes and zero point are 8-bit codes of one type."""
    if getattr(q, "num_bits", 9) > 8:
        raise NotImplementedError("codes wider than 8 bits")
    scale, zp, qmin, qmax = _activation_code_params(q)
    tdt, _ = ops._code_dtype(qmin, qmax)                       # (raises for a domain that is no 8-bit code)
    lo, hi = (0, 255) if tdt == torch.uint8 else (-128, 127)
    if not lo <= zp <= hi:
        raise NotImplementedError(f"the zero point {zp} is no {tdt} code")
    if not 0.0 < scale < math.inf:
        raise ValueError("the scale must be finite and positive")
    return scale, zp, qmin, qmax


class QuantizedAvgPool2d(_OnCodes):
    """``activation holder A -> average pool -> activation holder B`` on integer codes, for the integer consumers behind B.
    A's float32 output is ``float(code - zp_a) * scale_a`` bit for bit, so the sum of a window is ``scale_a`` times the exact
    integer sum S of ``code - zp_a`` over its taps inside the image (a padded tap is 0.0 and adds nothing), and B codes the mean:

        code = clamp(rint((float32(S) * scale_a) / float32(div) * (1 / scale_b)) + zp_b, qmin, qmax)

    with ``div`` PyTorch's divisor (``divisor_override``, ``pool_size`` with ``count_include_pad``, or the taps inside the
    image) -- ``ops.codes_avgpool`` (``mctq_codes_avgpool_nhwc``): 1 byte read per tap and 1 written per output element in one
    launch, where A writes 4, ATen's pool reads 4 and writes 4 and B reads 4 again.  Where ``scale_a`` and every ``div`` are
    powers of two these are bit for bit the codes B gives any float32 average pool of A's output; elsewhere the exact mean
    rounded twice, which differs from a float32 chain by at most one code next to a rounding tie (ATen's own average pools do
    not agree with each other in the last bit either).

    ``pool``: an ``nn.AvgPool2d`` (ints or pairs, padding at most half the kernel size), an ``nn.AdaptiveAvgPool2d`` of output
    size 1 -- the kernel is then the input's H x W at forward -- or ``QuantizedAvgPool2d.GLOBAL``, the same global pool
    without a module (``x.mean((2, 3))``).  ``forward`` takes A's codes (int8 / uint8 of A's code type, NCHW-shaped and
    NHWC-stored as the consumers and joins emit them) or a float32 [N, C, H, W] tensor, which it quantizes with A's
    parameters (``ops.fq_codes_nhwc``); it returns B's codes NCHW-shaped and NHWC-stored, or with ``flatten=True`` (global pools
    only) as [N, C] rows, which a ``QuantizedLinear`` of B's quantizer takes as they are.  ``activation_code_params`` is the INPUT
    form, what a producer in front emits (the meaning it has for ``IntegerConsumer`` and ``QuantizedMaxPool2d``);
    ``output_code_params`` is B's form.  It has no weights and is no ``IntegerConsumer``.  GPU tensors whose C is no multiple
    of 16, windows of more than 65536 taps and CPU tensors take torch ops with the same bytes."""

    GLOBAL = "global"

    def __init__(self, pool, in_quantizer, out_quantizer, flatten: bool = False):
        super().__init__()
        if isinstance(pool, nn.AdaptiveAvgPool2d) and not self.eligible(pool):
            raise TypeError(f"QuantizedAvgPool2d takes torch.nn.AdaptiveAvgPool2d layers of output size 1 only, got {pool.output_size!r}")
        if not self.eligible(pool):
            raise TypeError("QuantizedAvgPool2d takes torch.nn.AvgPool2d layers, their kernel_size, stride and padding ints or pairs, "
                            "padding at most half the kernel size, divisor_override None or a positive int; "
                            "torch.nn.AdaptiveAvgPool2d layers of output size 1; or QuantizedAvgPool2d.GLOBAL")
        self.in_quantizer, self.out_quantizer = in_quantizer, out_quantizer
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _code_form(in_quantizer)
        self._out_form = _code_form(out_quantizer)
        self.global_pool = type(pool) is not nn.AvgPool2d
        self.flatten = bool(flatten)
        if self.flatten and not self.global_pool:
            raise ValueError("flatten=True needs a global pool: a windowed pool's output is not 1 x 1")
        self.kernel_size = self.stride = None
        self.padding, self.ceil_mode, self.count_include_pad, self.divisor_override = (0, 0), False, True, None
        if not self.global_pool:
            self.kernel_size = ops._pair(pool.kernel_size, "kernel_size", "QuantizedAvgPool2d")
            self.stride = self.kernel_size if pool.stride is None else ops._pair(pool.stride, "stride", "QuantizedAvgPool2d")
            self.padding = ops._pair(pool.padding, "padding", "QuantizedAvgPool2d")
            self.ceil_mode, self.count_include_pad = bool(pool.ceil_mode), bool(pool.count_include_pad)
            self.divisor_override = pool.divisor_override

    @staticmethod
    def eligible(pool) -> bool:
        if isinstance(pool, str):
            return pool == QuantizedAvgPool2d.GLOBAL
        if type(pool) is nn.AdaptiveAvgPool2d:
            size = pool.output_size
            return (isinstance(size, int) and not isinstance(size, bool) and size == 1) or \
                (isinstance(size, (tuple, list)) and len(size) == 2 and _ints_or_pair(tuple(size)) and tuple(size) == (1, 1))
        if type(pool) is not nn.AvgPool2d or not isinstance(pool.ceil_mode, bool) or not isinstance(pool.count_include_pad, bool):
            return False
        div = pool.divisor_override
        if div is not None and (not isinstance(div, int) or isinstance(div, bool) or div < 1):
            return False
        stride = pool.kernel_size if pool.stride is None else pool.stride
        if not all(_ints_or_pair(v) for v in (pool.kernel_size, stride, pool.padding)):
            return False
        k, s, p = (ops._pair(v, "", "QuantizedAvgPool2d") for v in (pool.kernel_size, stride, pool.padding))
        return min(*k, *s) >= 1 and min(p) >= 0 and p[0] <= k[0] // 2 and p[1] <= k[1] // 2

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes this pool READS (holder A's): what ``emit_codes_for`` of the layer in
        front takes."""
        return self._a_scale, self._a_zp, self._a_qmin, self._a_qmax

    def output_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes ``forward`` returns (holder B's): what the consumers behind read."""
        return self._out_form

    def extra_repr(self) -> str:
        if self.global_pool:
            return f"global, flatten={self.flatten}"
        return (f"kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, ceil_mode={self.ceil_mode}, "
                f"count_include_pad={self.count_include_pad}, divisor_override={self.divisor_override}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise RuntimeError(f"expected [N, C, H, W], got {tuple(x.shape)}")
        codes = _operand_codes(x, self.activation_code_params(), "QuantizedAvgPool2d", "this pool's input quantizer")
        y = ops.codes_avgpool(codes, (self._a_scale, self._a_zp), self._out_form, self.kernel_size, self.stride, self.padding,
                              self.ceil_mode, self.count_include_pad, self.divisor_override)
        return y.reshape(y.shape[0], y.shape[3]) if self.flatten else y.permute(0, 3, 1, 2)


_NEAREST_MODES = ("nearest", "nearest-exact")
_ONE_RAMP_MAX = 1 << 24        # pixels of an image whose indices h * W + w are all float32 integers (QuantizedUpsample.index_maps)


class QuantizedUpsample(_OnCodes):
    """``activation holder A -> nearest upsample -> activation holder B`` on integer codes, for the integer consumers, pools and
    concatenations behind B: a U-Net stage, a YOLO / PANet neck, a segmentation head.  A's float32 output is
    ``float(code - zp_a) * scale_a`` bit for bit (``ops.dequantize_codes``), nearest interpolation only moves data and B codes
    every element by itself, so B's codes are A's codes gathered through the upsample's index map and requantized one by one
    -- ``ops.codes_upsample`` (``mctq_codes_upsample_nhwc``): 1 byte read and 1 written per output element in one launch, where
    A writes float32, ATen's upsample reads it and writes ``fh * fw`` times as much, and B reads and writes that again.  Nothing
    is approximated, whatever the geometry.

    ``upsample``: an ``nn.Upsample`` of mode "nearest" or "nearest-exact" (``size`` or ``scale_factor``, ints, floats or pairs,
    any ``recompute_scale_factor``; downsampling sizes and factors included) or an ``nn.UpsamplingNearest2d`` -- ``eligible`` says
    which; ``F.interpolate(x, ...)`` with constant arguments is ``nn.Upsample(...)`` of the same arguments.  ``in_quantizer`` (A's)
    and ``out_quantizer`` (B's): per-tensor affine activation quantizers of at most 8 bits whose zero points are codes of their
    type; ``out_quantizer=None``: the output form is the input's (no holder behind, as for a max pool), a pure copy of codes.

    ``forward`` takes A's codes (int8 / uint8 of A's code type, NCHW-shaped and NHWC-stored as the consumers and joins emit them)
    or a float32 [N, C, H, W] tensor, which it quantizes with A's parameters at the LOW resolution (``ops.fq_codes_nhwc``); it
    returns B's codes, NCHW-shaped and NHWC-stored.  ``activation_code_params`` is the INPUT form, what a producer in front
    emits; ``output_code_params`` is what the readers behind agree on (``QuantizedAvgPool2d``'s convention).

    The index maps are not derived from PyTorch's scale rules: for every ``(H, W, device)`` first seen, the module resamples an
    index ramp -- float32 ``[1, 1, H, W]`` holding ``h * W + w``; a row ramp and a column ramp where ``H * W`` > 2^24 -- through
    the very call it replaces, on that device, reads ``src_rows = out[:, 0] // W`` and ``src_cols = out[0, :] % W``, checks that
    the map is separable and caches the device int32 maps and the integer factors, if any.  That is one tiny launch and one host
    read per new shape: a hipGraph capture needs one warm-up forward per input shape first (``capture_forward``'s warm-up is
    one).  GPU tensors whose C is no multiple of 16 and CPU tensors take torch ops with the same bytes."""

    def __init__(self, upsample, in_quantizer, out_quantizer=None):
        super().__init__()
        if not self.eligible(upsample):
            raise TypeError("QuantizedUpsample takes torch.nn.Upsample layers of mode 'nearest' or 'nearest-exact' with either a "
                            "size or a scale_factor, a number or a pair of numbers, and torch.nn.UpsamplingNearest2d layers")
        self.upsample = upsample
        self.in_quantizer, self.out_quantizer = in_quantizer, out_quantizer
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _code_form(in_quantizer)
        self._out_form = self.activation_code_params() if out_quantizer is None else _code_form(out_quantizer)
        self._maps = {}                                        # (H, W, device) -> (src_rows, src_cols, factors or None)

    @staticmethod
    def eligible(upsample) -> bool:
        if type(upsample) not in (nn.Upsample, nn.UpsamplingNearest2d):
            return False
        if upsample.mode not in _NEAREST_MODES or upsample.align_corners is not None:
            return False
        if getattr(upsample, "recompute_scale_factor", None) not in (None, True, False):
            return False
        size, factor = upsample.size, upsample.scale_factor
        if (size is None) == (factor is None):
            return False
        number = lambda e, kinds: isinstance(e, kinds) and not isinstance(e, bool) and e > 0 and math.isfinite(e)     # noqa: E731
        kinds = (int,) if factor is None else (int, float)
        v = size if factor is None else factor
        return number(v, kinds) or (isinstance(v, (tuple, list)) and len(v) == 2 and all(number(e, kinds) for e in v))

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes this module READS (holder A's): what ``emit_codes_for`` of the layer in
        front takes."""
        return self._a_scale, self._a_zp, self._a_qmin, self._a_qmax

    def output_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes ``forward`` returns (holder B's, or A's without one)."""
        return self._out_form

    def extra_repr(self) -> str:
        return f"size={self.upsample.size}, scale_factor={self.upsample.scale_factor}, mode={self.upsample.mode}"

    def index_maps(self, height: int, width: int, device):
        """``(src_rows, src_cols, factors)`` of an ``height`` x ``width`` input on ``device``: int32 tensors of lengths Ho / Wo on
        that device, ``upsample(x) == x[:, :, src_rows][:, :, :, src_cols]``, and ``(fh, fw)`` where both maps are those of integer
        factors, else None.  Resampled through the module itself and cached."""
        device = torch.device(device)
        key = (int(height), int(width), str(device))
        hit = self._maps.get(key)
        if hit is not None:
            return hit
        h, w = key[0], key[1]
        with torch.no_grad():
            ys = torch.arange(h, dtype=torch.float32, device=device).reshape(1, 1, h, 1)
            xs = torch.arange(w, dtype=torch.float32, device=device).reshape(1, 1, 1, w)
            if h * w <= _ONE_RAMP_MAX:                         # every index is a float32 integer
                src = self.upsample(ys * w + xs)[0, 0].to(torch.int64)
            else:
                src = self.upsample(ys.expand(1, 1, h, w))[0, 0].to(torch.int64) * w + self.upsample(xs.expand(1, 1, h, w))[0, 0].to(torch.int64)
            rows, cols = src[:, 0] // w, src[0, :] % w
            if not torch.equal(src, rows[:, None] * w + cols[None, :]):
                raise RuntimeError("the upsample's index map is not separable into rows and columns")
        fh, fw = ops.integer_factor(rows.cpu(), h), ops.integer_factor(cols.cpu(), w)
        if len(self._maps) > 64:
            self._maps.clear()
        hit = self._maps[key] = (rows.to(torch.int32), cols.to(torch.int32), (fh, fw) if fh and fw else None)
        return hit

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise RuntimeError(f"expected [N, C, H, W], got {tuple(x.shape)}")
        codes = _operand_codes(x, self.activation_code_params(), "QuantizedUpsample", "this upsample's input quantizer")
        rows, cols, factors = self.index_maps(codes.shape[1], codes.shape[2], codes.device)
        y = ops.codes_upsample(codes, (self._a_scale, self._a_zp), self._out_form, rows, cols, factors)
        return y.permute(0, 3, 1, 2)


_TABLE_CHAIN_MAX = 4           # activations in a row that one QuantizedActivationTable takes


class QuantizedActivationTable(_OnCodes):
    """``activation holder A -> elementwise activation(s) -> activation holder B`` on integer codes, for the integer consumers,
    pools and concatenations behind B: EfficientNet- and YOLO-style ``conv -> holder -> SiLU -> holder -> conv``, GELU blocks,
    sigmoid gates, LeakyReLU necks.  A's float32 output is ``float(code - zp_a) * scale_a`` bit for bit (``ops.dequantize_codes``),
    so it takes at most 256 values; an elementwise ``f`` maps each value by itself and B codes each element by itself, so B's code
    is a function of A's code: a 256-entry byte table -- ``ops.codes_table`` (``mctq_codes_table``): 1 byte read and 1 written per
    element in one launch, where A writes float32, ATen's ``f`` reads and writes it, and B and the reader's quantize launch read
    it again.

    The table is the definition: B's code of ``f``, evaluated on the [256] dequantized values by the replaced call itself on the
    tensor's device (``ops.code_table``).  On the GPU, ATen's elementwise kernels apply one scalar functor per element whatever
    its position, the shape or the layout, so the codes are bit for bit those of the float32 chain A -> f -> B on that GPU, the
    transcendental functions included (tests/test_gpu_table_consumer.py checks every accepted function with strict equality).  On
    the CPU that does not hold: ATen's vector body and scalar tail give different last bits for sigmoid, SiLU, softplus, ELU, Mish,
    tanh and GELU, so there the codes equal the chain's wherever the chain's float32 value equals the table's, and elsewhere can
    differ by one code next to a rounding tie.

    ``fn``: one module or a sequence of 1 to 4 modules, applied in order, each of a type ``eligible`` accepts -- ``nn.Sigmoid``,
    ``Tanh``, ``SiLU``, ``GELU`` (both approximations), ``Mish``, ``Softplus``, ``ELU``, ``CELU``, ``SELU``, ``LeakyReLU``,
    ``Hardswish``, ``Hardsigmoid``, ``Hardtanh``, ``ReLU``, ``ReLU6``, ``LogSigmoid``, ``Softsign``, ``Tanhshrink``, and no subclass
    of them: elementwise, without learnable, per-channel or random state and without a training mode.  ``in_quantizer`` (A's) and
    ``out_quantizer`` (B's): per-tensor affine activation quantizers of at most 8 bits whose zero points are codes of their type.

    ``forward`` takes A's codes (int8 / uint8 of A's code type) or a float32 tensor, which it quantizes with A's parameters, of
    any rank -- a 4-D one NCHW-shaped and NHWC-stored as the consumers and joins emit it -- and returns B's codes in the same shape
    and layout.  ``activation_code_params`` is the INPUT form, what a producer in front emits; ``output_code_params`` is B's
    (``QuantizedAvgPool2d``'s convention).  Tables are cached per device and built on first use there, with a few tiny launches
    and no host read: a hipGraph capture needs one warm-up forward first (``capture_forward``'s warm-up is one).  Any element
    and channel count takes the kernel."""

    TYPES = (nn.Sigmoid, nn.Tanh, nn.SiLU, nn.GELU, nn.Mish, nn.Softplus, nn.ELU, nn.CELU, nn.SELU, nn.LeakyReLU, nn.Hardswish,
             nn.Hardsigmoid, nn.Hardtanh, nn.ReLU, nn.ReLU6, nn.LogSigmoid, nn.Softsign, nn.Tanhshrink)

    def __init__(self, fn, in_quantizer, out_quantizer):
        super().__init__()
        fns = list(fn) if isinstance(fn, (list, tuple, nn.Sequential, nn.ModuleList)) else [fn]
        if not 1 <= len(fns) <= _TABLE_CHAIN_MAX or not all(self.eligible(f) for f in fns):
            raise TypeError(f"QuantizedActivationTable takes 1 to {_TABLE_CHAIN_MAX} elementwise activation modules of the types "
                            + ", ".join(t.__name__ for t in self.TYPES) + " (no subclasses)")
        self.fns = nn.ModuleList(fns)
        self.in_quantizer, self.out_quantizer = in_quantizer, out_quantizer
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _code_form(in_quantizer)
        self._out_form = _code_form(out_quantizer)
        self._out_dtype = ops._code_dtype(self._out_form[2], self._out_form[3])[0]
        self._tables = {}                                      # device -> uint8 [256]

    @staticmethod
    def eligible(fn) -> bool:
        if type(fn) not in QuantizedActivationTable.TYPES:
            return False
        if type(fn) is nn.GELU and fn.approximate not in ("none", "tanh"):
            return False
        return True

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes this module READS (holder A's): what ``emit_codes_for`` of the layer in
        front takes."""
        return self._a_scale, self._a_zp, self._a_qmin, self._a_qmax

    def output_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes ``forward`` returns (holder B's): what the readers behind agree on."""
        return self._out_form

    def extra_repr(self) -> str:
        return "fn=" + " -> ".join(type(f).__name__ for f in self.fns)

    def _apply_fns(self, x):
        for f in self.fns:
            x = f(x)
        return x

    def table(self, device):
        """The byte table on ``device`` (``ops.code_table`` of the activations in order), built on first use there."""
        key = str(torch.device(device))
        hit = self._tables.get(key)
        if hit is None:
            hit = self._tables[key] = ops.code_table(self._apply_fns, self.activation_code_params(), self._out_form, device)
        return hit

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        codes = _operand_codes(x, self.activation_code_params(), "QuantizedActivationTable", "this activation's input quantizer")
        y = ops.codes_table(codes, self.table(codes.device), self._out_dtype)
        return y.permute(0, 3, 1, 2) if x.dim() == 4 else y


class _OperandsOnCodes(_OnCodes):
    """What QuantizedConcat, QuantizedMul and QuantizedMatmul share: several operands, each read as the codes of its own holder's
    quantizer, and one output holder's quantizer, all per-tensor affine of at most 8 bits (``_code_form``).  With
    ``float_output`` (QuantizedMatmul) the output quantizer may be missing: the module then returns float32."""

    def __init__(self, operand_quantizers, activation_quantizer, float_output: bool = False):
        super().__init__()
        self.operand_quantizers = tuple(operand_quantizers)
        self.activation_quantizer = activation_quantizer
        self._forms = tuple(_code_form(q) for q in self.operand_quantizers)
        self._out_form = None if float_output and activation_quantizer is None else _code_form(activation_quantizer)

    def operand_code_params(self, i: int):
        """(scale, zero_point, qmin, qmax) of the codes operand ``i`` is read as."""
        return self._forms[i]

    def activation_code_params(self):
        """(scale, zero_point, qmin, qmax) of the codes ``forward`` returns: what the consumers and pools behind read."""
        return self._out_form

    def _codes_of(self, i: int, x: torch.Tensor, nhwc: bool = True):
        """Operand ``i`` as codes: given codes as they are, float32 quantized in its form; ``nhwc``: 4-D ones as [B, H, W, C]."""
        return _operand_codes(x, self._forms[i], type(self).__name__, "its quantizer", at=f"operand {i}: ", nhwc=nhwc)


class QuantizedConcat(_OperandsOnCodes):
    """``activation holders -> torch.cat(..., dim=1) -> activation holder`` on integer codes, for the integer consumers and
    pools behind that holder.  An operand holder's float32 output is ``float(code - zp_i) * scale_i`` bit for bit
    (``ops.dequantize_codes``), ``torch.cat`` only moves data, and the holder behind it codes every element by itself, so the
    codes of the concatenated tensor are the operands' codes requantized one by one into the output form --
    ``ops.codes_concat`` (``mctq_codes_concat_nhwc``): 1 byte read and 1 written per element in one launch, where every
    operand holder, ``torch.cat`` and the holder behind it each read and write 4.

    ``operand_quantizers`` (1 to any number; more than 8, or channel counts that are no multiple of 16, take the torch route of
    ``ops.codes_concat``) and ``activation_quantizer``, the output holder's: per-tensor affine activation quantizers of at most 8
    bits.  ``forward(*xs)`` takes each operand as the codes of its quantizer (int8 / uint8 of its code type, NCHW-shaped and
    NHWC-stored as the consumers and joins emit them, or ``[M, C]`` rows) or as a float32 tensor, which it quantizes with that
    operand's parameters -- the holder's input and its output give the same codes, since a quantizer's codes of its own
    output are the codes that output was made from.  It returns the output holder's codes, NCHW-shaped and NHWC-stored for
    4-D operands and ``[M, sum C]`` for rows, which an ``IntegerConsumer`` or a ``QuantizedMaxPool2d`` of that quantizer takes as
    they are.  ``activation_code_params`` is the OUTPUT form, what the modules behind agree on; ``operand_code_params(i)`` is
    what ``emit_codes_for`` of the layer in front of operand ``i`` takes."""

    def __init__(self, operand_quantizers, activation_quantizer):
        operand_quantizers = tuple(operand_quantizers)
        if not operand_quantizers:
            raise ValueError("QuantizedConcat needs at least one operand")
        for q in (*operand_quantizers, activation_quantizer):
            if getattr(q, "num_bits", 9) > 8:
                raise NotImplementedError("codes wider than 8 bits")
        super().__init__(operand_quantizers, activation_quantizer)

    def extra_repr(self) -> str:
        return f"operands={len(self._forms)}"

    def forward(self, *xs) -> torch.Tensor:
        if len(xs) != len(self._forms):
            raise RuntimeError(f"this concatenation was built for {len(self._forms)} operands, got {len(xs)}")
        first = xs[0]
        if first.dim() not in (2, 4):
            raise RuntimeError(f"expected [N, C, H, W] or [M, C] operands, got {tuple(first.shape)}")
        parts = []
        for i, (x, (scale, zp, _, _)) in enumerate(zip(xs, self._forms)):
            if x.dim() != first.dim() or x.shape[0] != first.shape[0] or x.shape[2:] != first.shape[2:]:
                raise RuntimeError(f"operand {i} is {tuple(x.shape)} next to {tuple(first.shape)}: the operands of a concatenation "
                                   f"along dimension 1 differ in that dimension only")
            parts.append((self._codes_of(i, x), scale, zp))
        y = ops.codes_concat(parts, self._out_form)
        return y.permute(0, 3, 1, 2) if first.dim() == 4 else y


class QuantizedMul(_OperandsOnCodes):
    """``activation holders A, G -> torch.mul -> activation holder M`` on integer codes, for the integer consumers and pools
    behind M: the multiply of a squeeze-and-excitation block, a gated layer.  A holder's float32 output is
    ``float(code - zp) * scale`` bit for bit (``ops.dequantize_codes``), ``torch.mul`` is one IEEE float32 multiplication and M
    codes every element by itself, so M's codes are a function of the two operand codes --
    ``ops.codes_mul`` (``mctq_codes_mul_nhwc``): 1 byte read and 1 written per element of the large tensor in one launch, where
    the two holders, ``torch.mul`` and M each read and write 4.  Nothing is approximated.

    ``operand_quantizers``: the two operand holders' quantizers, in the order of ``forward``'s operands; ``activation_quantizer``:
    M's.  Per-tensor affine activation quantizers of at most 8 bits.  ``forward(x0, x1)`` takes each operand as the codes of its
    quantizer (int8 / uint8 of its code type; 4-D codes NCHW-shaped and NHWC-stored as the consumers and joins emit them, 2-D
    ones ``[M, C]`` rows) or as a float32 tensor, which stands for the holder's input -- the holder's input and its output
    give the same codes.  The shapes decide at forward time: equal shapes take the kernel's same-shape form (a float32
    operand is quantized first, ``ops.fq_codes_nhwc``); ``[B, C, H, W]`` with ``[B, C, 1, 1]``, in either order, the row-broadcast
    form, where a float32 gate goes to the kernel as it is and is coded there; any other pair of shapes broadcasts as
    ``torch.mul`` does with torch ops (``ops.codes_mul``'s torch route, as for C % 16 != 0 and CPU tensors -- the same bytes).
    It returns M's codes, NCHW-shaped and NHWC-stored for a 4-D result, which an ``IntegerConsumer`` or a ``QuantizedMaxPool2d``
    of that quantizer takes as they are.  ``activation_code_params`` is the OUTPUT form, what the modules behind agree on;
    ``operand_code_params(i)`` is what ``emit_codes_for`` of the layer in front of operand ``i`` takes."""

    def __init__(self, operand_quantizers, activation_quantizer):
        operand_quantizers = tuple(operand_quantizers)
        if len(operand_quantizers) != 2:
            raise ValueError("QuantizedMul takes the quantizers of two operands")
        super().__init__(operand_quantizers, activation_quantizer)

    def forward(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        xs = (x0, x1)
        (s0, z0, _, _), (s1, z1, _, _) = self._forms
        is_gate = lambda g, a: (a.dim() == 4 and g.dim() == 4 and g.shape[:2] == a.shape[:2]              # noqa: E731
                                and tuple(g.shape[2:]) == (1, 1) and g.shape != a.shape)
        if is_gate(x1, x0) or is_gate(x0, x1):
            at = 0 if is_gate(x1, x0) else 1                     # the large operand; the multiplication is commutative
            gate, (gs, gz, gmin, gmax) = xs[1 - at], self._forms[1 - at]
            big = (self._codes_of(at, xs[at]), *self._forms[at][:2])
            if gate.dtype == torch.float32:
                y = ops.codes_mul(big, (gate.permute(0, 2, 3, 1), gs, gz), self._out_form, gate_form=(gmin, gmax))
            else:
                y = ops.codes_mul(big, (self._codes_of(1 - at, gate), gs, gz), self._out_form)
        elif x0.dim() == x1.dim() == 4:
            y = ops.codes_mul((self._codes_of(0, x0), s0, z0), (self._codes_of(1, x1), s1, z1), self._out_form)
        else:                                                    # rows, or operands of different rank: as torch.mul sees them
            y = ops.codes_mul((self._codes_of(0, x0, False), s0, z0), (self._codes_of(1, x1, False), s1, z1), self._out_form)
            return y.contiguous(memory_format=torch.channels_last) if y.dim() == 4 else y
        return y.permute(0, 3, 1, 2) if y.dim() == 4 else y


class QuantizedMatmul(_OperandsOnCodes):
    """``activation holders A, B -> torch.matmul / @ / torch.bmm [-> activation holder C]`` on integer codes: the activation x
    activation product, in practice the two products of every attention block, ``Q @ K.transpose(-1, -2)`` and ``P @ V``.  Both
    operands are ``float(code - zp) * scale`` bit for bit, so the product is the exact integer sum of ``(qa - za) * (qb - zb)`` scaled
    once -- ``qmatmul_i8`` (``mctq_qmatmul_i8``, the integer matrix cores), where the float32 chain runs two holders and a float32
    matmul; it differs from that chain only by the chain's own float32 accumulation rounding (not at all where that is exact:
    power-of-two scales and ``255 * 255 * K < 2^24``).

    ``operand_quantizers``: the two operand holders' quantizers, in the order of ``forward``'s operands; ``activation_quantizer``:
    C's, or None.  Per-tensor affine activation quantizers of at most 8 bits whose zero points are codes of their type.
    ``transposed_b=True``: the second operand arrives as ``[..., N, K]`` and the product is taken with its last two dimensions
    swapped, without moving data (the ``k.transpose(-1, -2)`` of the scores).  ``forward(x0, x1)`` takes each operand as the codes
    of its quantizer (int8 / uint8 of its code type) or as a float32 tensor, which it quantizes in that operand's form -- the
    holder's input and its output give the same codes; these operands are matrices, not images: their shape and strides are
    what they are, a permuted ``[B, T, H, D]`` view goes to the kernel as it is.  It returns float32, or with an
    ``activation_quantizer`` that holder's codes (contiguous ``[..., M, N]``), which a QuantizedLinear or another QuantizedMatmul of
    that quantizer takes as they are -- through reshapes and permutes, which only move data.  ``activation_code_params`` is the
    OUTPUT form (None for float32), ``operand_code_params(i)`` what ``emit_codes_for`` of the layer in front of operand ``i`` takes."""

    def __init__(self, operand_quantizers, activation_quantizer=None, transposed_b: bool = False):
        operand_quantizers = tuple(operand_quantizers)
        if len(operand_quantizers) != 2:
            raise ValueError("QuantizedMatmul takes the quantizers of two operands")
        super().__init__(operand_quantizers, activation_quantizer, float_output=True)
        self.transposed_b = bool(transposed_b)

    def extra_repr(self) -> str:
        return f"transposed_b={self.transposed_b}, output={'float32' if self._out_form is None else 'codes'}"

    def forward(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        a, b = self._codes_of(0, x0, nhwc=False), self._codes_of(1, x1, nhwc=False)
        return qmatmul_i8(a, self._forms[0][:2], b, self._forms[1][:2], transposed_b=self.transposed_b, out_codes=self._out_form)


# In the order they are tried: (class, the switch of the rewrites that enables it or None, what fusing asks of the layer beyond
# ``eligible``, given the layer and ``any_channels``).  The rows kernels need K % 16 == 0 and K <= _MAX_K, which QuantizedConv2d's
# ``eligible`` holds itself; with ``any_channels`` rows of any K are padded to Kp = 16 * ceil(K / 16), and Kp <= _MAX_K is K <= _MAX_K.
_CONSUMERS = (
    (QuantizedLinear, None, lambda layer, any_channels: (any_channels or layer.in_features % 16 == 0) and layer.in_features <= _MAX_K),
    (QuantizedConv1x1, None, lambda layer, any_channels: (any_channels or layer.in_channels % 16 == 0) and layer.in_channels <= _MAX_K),
    (QuantizedConv2d, "convolutions", None),
    (QuantizedDepthwiseConv2d, "depthwise", None),
    (QuantizedGroupedConv2d, "grouped", None),
    (QuantizedConvTranspose2d, "transposed", None),
)


def _consumer_for(wrapper, activation_quantizer, uniform_weights=False, convolutions=False, depthwise=False, any_channels=False,
                  grouped=False, transposed=False):
    """The integer consumer that can stand in for ``wrapper`` fed by ``activation_quantizer``, or None.  Uniform weights
    only with ``uniform_weights``; convolutions that need a patch matrix (QuantizedConv2d) only with ``convolutions``;
    depthwise convolutions (QuantizedDepthwiseConv2d) only with ``depthwise``; the other grouped convolutions
    (QuantizedGroupedConv2d) only with ``grouped``; transposed convolutions (QuantizedConvTranspose2d) only with ``transposed``;
    layers whose K is no multiple of 16 only with ``any_channels`` (QuantizedLinear and the convolutions that are its product;
    never the depthwise, the grouped or the transposed convolution).  Half-precision
    layers are refused by the classes: the integer consumer would change the output type."""
    layer = getattr(wrapper, "layer", None)
    if list(getattr(wrapper, "weights_quantizers", {})) != ["weight"]:
        return None
    if _is_uniform_weights(wrapper.weights_quantizers["weight"]) and not uniform_weights:
        return None
    enabled = {None: True, "convolutions": convolutions, "depthwise": depthwise, "grouped": grouped, "transposed": transposed}
    for cls, switch, fits in _CONSUMERS:
        extra = {"any_channels": True} if any_channels and issubclass(cls, QuantizedLinear) else {}
        if enabled[switch] and cls.eligible(layer, **extra) and (fits is None or fits(layer, bool(extra))):
            try:
                return cls.from_wrapper(wrapper, activation_quantizer, **extra)
            except (TypeError, NotImplementedError):
                return None
    return None


# what reads the activation codes of the module in front as they are
_CODE_READERS = (IntegerConsumer, QuantizedMaxPool2d, QuantizedAvgPool2d, QuantizedUpsample, QuantizedActivationTable)


class _FusedAway(nn.Identity):
    """Placeholder ``fuse_linear_consumers`` leaves in an ``nn.Sequential`` where a module went into the one behind it: an
    activation holder in front of a consumer or a pool, an average pool's second holder, a flatten."""


def _module_of(node, mods):
    """The module a ``call_module`` node calls; None for every other node."""
    return mods.get(node.target) if node.op == "call_module" else None


def _install_consumer(gm, mods, node, fused):
    """Registers ``fused`` as ``<the wrapper's name>_qlinear`` and makes ``node``, the wrapper's call, call it."""
    name = node.target.replace(".", "_") + "_qlinear"
    gm.add_submodule(name, fused)
    mods[name] = fused
    node.target = name


def _plain_holder(m) -> bool:
    """An activation holder that really quantizes (the FLN / preserving variants can be switched to pass-through)."""
    return isinstance(m, PytorchActivationQuantizationHolder) and not getattr(m, "quantization_bypass", False)


def _holder_of(node, mods):
    """The plain holder ``node`` calls on one tensor -- a ``call_module`` node without kwargs whose one argument is a node --
    or None."""
    from torch.fx import Node
    if node.op != "call_module" or node.kwargs or len(node.args) != 1 or not isinstance(node.args[0], Node):
        return None
    holder = mods.get(node.target)
    return holder if _plain_holder(holder) else None


def _holder_calls(gm, mods):
    """``(node, holder)`` for every node of the graph that calls a plain holder on one tensor (``_holder_of``), tested when its
    turn comes: the loops that use this rewrite the graph as they go."""
    for node in list(gm.graph.nodes):
        holder = _holder_of(node, mods)
        if holder is not None:
            yield node, holder


def _wrapped_consumer(user, src, mods, quantizer, consumer_for):
    """The consumer ``consumer_for(wrapper, quantizer)`` gives for ``user`` if it calls a wrapped layer on ``src`` alone, else None."""
    wrapper = _module_of(user, mods)
    if not isinstance(wrapper, PytorchQuantizationWrapper) or user.kwargs or user.args != (src,):
        return None
    return consumer_for(wrapper, quantizer)


def _wrapped_users(src, mods, quantizer, consumer_for, rows: bool):
    """[(user, its consumer)] if every user of ``src`` is a wrapped layer ``consumer_for`` can take, fed by ``src`` alone
    (``_wrapped_consumer``) -- with ``rows`` a QuantizedLinear, without anything else: a 4-D tensor never feeds a QuantizedLinear
    (it would run along the width, not the channels) and rows feed nothing else -- else None."""
    taken = []
    for user in src.users:
        fused = _wrapped_consumer(user, src, mods, quantizer, consumer_for)
        if fused is None or (type(fused) is QuantizedLinear) != rows:
            return None
        taken.append((user, fused))
    return taken


def _const_args(node, names):
    """The arguments of ``node`` behind its first (tensor) operand by name -- ``names`` in positional order -- if every one of
    them is a known name given once and a constant, else None."""
    from torch.fx import Node
    rest = node.args[1:]
    if len(rest) > len(names) or set(node.kwargs) - set(names[len(rest):]):
        return None
    given = dict(zip(names, rest), **node.kwargs)
    return None if any(isinstance(v, Node) for v in given.values()) else given


def _pool_of(node, mods):
    """The ``nn.MaxPool2d`` that ``node`` applies to its one tensor operand -- a call of such a module, or ``F.max_pool2d`` with
    constant arguments, for which one is built -- if QuantizedMaxPool2d can take it, else None."""
    from torch.fx import Node
    if not node.args or not isinstance(node.args[0], Node):
        return None
    pool = None
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        pool = mods.get(node.target)
    elif node.op == "call_function" and node.target is torch.nn.functional.max_pool2d:
        given = _const_args(node, ("kernel_size", "stride", "padding", "dilation", "ceil_mode", "return_indices"))
        if given is None or "kernel_size" not in given:
            return None
        if not all(isinstance(given.get(k, False), bool) for k in ("ceil_mode", "return_indices")):
            return None
        try:
            pool = nn.MaxPool2d(**given)
        except (TypeError, ValueError):
            return None
    return pool if QuantizedMaxPool2d.eligible(pool) else None


class _PoolPlan(NamedTuple):
    """A pool that can run on codes: the ``module`` that replaces it, the ``suffix`` of its node's name, ``taken`` [(user, its
    consumer)], the wrapped layers that read its output, and ``gone``, the nodes between the pool and those that leave the graph.
    An upsample's plan (``_upsample_plan``) also has ``name``, its node's whole name where that is not the pool node's own with the
    suffix, ``pooled`` [(max pool node, its plan)], the max pools that read its codes, and ``readers``, the QuantizedConcat /
    QuantizedMul nodes that do."""
    module: nn.Module
    suffix: str
    taken: list
    gone: list
    name: Optional[str] = None
    pooled: tuple = ()
    readers: tuple = ()


def _pool_plan(node, mods, quantizer, consumer_for):
    """``node`` a user of a plain holder with ``quantizer``: the plan of a QuantizedMaxPool2d if it is a max pool of the holder's
    output that can run on codes -- every user a wrapped convolution ``consumer_for`` can take, fed by the pool alone -- else
    None.  (A pool that also feeds a float32 user, an identity add for instance, is left alone.)"""
    pool = _pool_of(node, mods)
    taken = _wrapped_users(node, mods, quantizer, consumer_for, rows=False) if pool is not None else None
    if not taken:
        return None
    try:
        return _PoolPlan(QuantizedMaxPool2d(pool, quantizer), "_qpool", taken, [])
    except (TypeError, ValueError, NotImplementedError):
        return None


def _install_pool(gm, mods, node, plan, source) -> int:
    """Makes ``node``, the pool's call, a call of ``plan``'s module on ``source`` (the holder's codes, or the float32 tensor the
    holder read), the wrapped layers of the plan consumers of its output, and erases the nodes between them (an average pool's
    second holder and flattens, an upsample's second holder); returns the number of consumers, those behind the max pools of an
    upsample's plan included."""
    name = plan.name or (node.target.replace(".", "_") if node.op == "call_module" else node.name) + plan.suffix
    gm.add_submodule(name, plan.module)
    mods[name] = plan.module
    node.op, node.target, node.args, node.kwargs = "call_module", name, (source,), {}
    for user, fused in plan.taken:
        _install_consumer(gm, mods, user, fused)
        user.args = (node,)
    count = len(plan.taken)
    for user, behind in plan.pooled:
        count += _install_pool(gm, mods, user, behind, node)
    for reader in plan.readers:                              # (where they read the second holder: now this node)
        reader.args = tuple(node if a in plan.gone else a for a in reader.args)
    gone = list(plan.gone)
    while gone:                                              # users first
        free = [g for g in gone if not g.users]
        if not free:
            raise RuntimeError("a node of the pool's chain still has users")
        for g in free:
            gm.graph.erase_node(g)
            gone.remove(g)
    return count


def _avg_pool_of(node, mods):
    """``(pool, flat)`` if ``node`` is an average pool of its one tensor operand that QuantizedAvgPool2d can take: a call of an
    ``nn.AvgPool2d`` / ``nn.AdaptiveAvgPool2d(1)`` module, ``F.avg_pool2d`` with constant arguments, ``F.adaptive_avg_pool2d(x, 1)``,
    or ``x.mean(...)`` / ``torch.mean(x, ...)`` over the constant dims (2, 3) / (-2, -1) in either order with a constant
    ``keepdim`` -- ``pool`` what the class takes, ``flat`` True where the result already is [N, C] (``keepdim=False``).  Else None."""
    from torch.fx import Node
    F = torch.nn.functional
    if not node.args or not isinstance(node.args[0], Node):
        return None
    pool, flat = None, False
    if node.op == "call_module":
        if len(node.args) == 1 and not node.kwargs and isinstance(mods.get(node.target), (nn.AvgPool2d, nn.AdaptiveAvgPool2d)):
            pool = mods.get(node.target)
    elif node.op == "call_function" and node.target is F.avg_pool2d:
        given = _const_args(node, ("kernel_size", "stride", "padding", "ceil_mode", "count_include_pad", "divisor_override"))
        if given is None or "kernel_size" not in given:
            return None
        if not all(isinstance(given.get(k, False), bool) for k in ("ceil_mode", "count_include_pad")):
            return None
        try:
            pool = nn.AvgPool2d(**given)
        except (TypeError, ValueError):
            return None
    elif node.op == "call_function" and node.target is F.adaptive_avg_pool2d:
        given = _const_args(node, ("output_size",))
        if given is None or "output_size" not in given:
            return None
        pool = nn.AdaptiveAvgPool2d(given["output_size"])
    elif (node.op == "call_method" and node.target == "mean") or (node.op == "call_function" and node.target is torch.mean):
        given = _const_args(node, ("dim", "keepdim"))
        if given is None or not isinstance(given.get("keepdim", False), bool):
            return None
        dim = given.get("dim")
        if not isinstance(dim, (tuple, list)) or tuple(dim) not in ((2, 3), (3, 2), (-2, -1), (-1, -2)) \
                or any(isinstance(d, bool) for d in dim):
            return None
        pool, flat = QuantizedAvgPool2d.GLOBAL, not given.get("keepdim", False)
    if pool is None or not QuantizedAvgPool2d.eligible(pool):
        return None
    return pool, flat


def _is_flatten(node, mods) -> bool:
    """``node`` flattens its one tensor operand from dimension 1 on: ``nn.Flatten()`` with the defaults, ``torch.flatten(x, 1)`` or
    ``x.flatten(1)`` (``end_dim`` -1 where given).  ``view`` / ``reshape`` are not recognised: their sizes are not constants."""
    from torch.fx import Node
    if not node.args or not isinstance(node.args[0], Node):
        return False
    if node.op == "call_module":
        m = mods.get(node.target)
        return type(m) is nn.Flatten and m.start_dim == 1 and m.end_dim == -1 and len(node.args) == 1 and not node.kwargs
    if (node.op == "call_function" and node.target is torch.flatten) or (node.op == "call_method" and node.target == "flatten"):
        given = _const_args(node, ("start_dim", "end_dim"))
        if given is None:
            return False
        start, end = given.get("start_dim", 0), given.get("end_dim", -1)
        return all(isinstance(v, int) and not isinstance(v, bool) for v in (start, end)) and start == 1 and end == -1
    return False


def _avg_pool_plan(node, mods, quantizer, consumer_for):
    """``node`` a user of a plain holder A with ``quantizer``: the plan of a QuantizedAvgPool2d, B and the flattens in ``gone``, if
    it is an average pool of A's output (``_avg_pool_of``) whose one user -- through at most one flatten (``_is_flatten``), and
    that behind a global pool only, where H = W = 1 is known without shapes -- is a plain holder B, every user of which is a
    wrapped layer ``consumer_for`` can take, fed by B alone (a 4-D tensor never feeds a QuantizedLinear, rows feed nothing
    else), or, behind a global pool, a flatten all of whose users are such wrapped ``nn.Linear`` layers.  Else None: a float32
    user of the pool or of B, an activation between them, no holder B.  B's users all see rows or all see 4-D tensors."""
    found = _avg_pool_of(node, mods)
    if found is None or len(node.users) != 1:
        return None
    pool, flat = found
    is_global = type(pool) is not nn.AvgPool2d
    gone, nxt, last = [], next(iter(node.users)), node
    if not flat and is_global and _is_flatten(nxt, mods) and len(nxt.users) == 1:
        gone, flat, last, nxt = [nxt], True, nxt, next(iter(nxt.users))
    holder = _holder_of(nxt, mods)
    if holder is None or nxt.args != (last,) or not nxt.users:
        return None
    out_quantizer = holder.activation_holder_quantizer
    if flat:
        taken = _wrapped_users(nxt, mods, out_quantizer, consumer_for, rows=True)
    elif is_global and all(_is_flatten(u, mods) and u.args[0] is nxt and u.users for u in nxt.users):
        taken, flat = [], True
        for u in nxt.users:
            behind = _wrapped_users(u, mods, out_quantizer, consumer_for, rows=True)
            if behind is None:
                return None
            taken += behind
        gone = gone + list(nxt.users)
    else:
        taken = _wrapped_users(nxt, mods, out_quantizer, consumer_for, rows=False)
    if not taken:
        return None
    try:
        return _PoolPlan(QuantizedAvgPool2d(pool, quantizer, out_quantizer, flatten=flat), "_qavgpool", taken, gone + [nxt])
    except (TypeError, ValueError, NotImplementedError):
        return None


def _upsample_of(node, mods):
    """The ``nn.Upsample`` that ``node`` applies to its one tensor operand -- a call of an ``nn.Upsample`` / ``nn.UpsamplingNearest2d``
    module, or ``F.interpolate`` with constant arguments (``antialias`` false), for which one is built -- if QuantizedUpsample can
    take it, else None."""
    from torch.fx import Node
    if not node.args or not isinstance(node.args[0], Node):
        return None
    up = None
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        up = mods.get(node.target)
    elif node.op == "call_function" and node.target is torch.nn.functional.interpolate:
        given = _const_args(node, ("size", "scale_factor", "mode", "align_corners", "recompute_scale_factor", "antialias"))
        if given is None or given.pop("antialias", False) is not False or not isinstance(given.get("mode", "nearest"), str):
            return None
        try:
            up = nn.Upsample(**given)
        except (TypeError, ValueError):
            return None
    return up if QuantizedUpsample.eligible(up) else None


def _between_holders_plan(first, chain, mods, quantizer, consumer_for, pools, build, suffix, copies: bool, rows: bool):
    """What ``_upsample_plan`` and ``_table_plan`` share.  ``first`` is a user of a plain holder A with ``quantizer`` and ``chain`` the
    nodes behind it that belong to the operation with it (the further activations of a table; none for an upsample); the plan is
    that of the module ``build(out_quantizer)`` if all the readers of the last node agree on one code form F and read codes.  Its
    one user may be a plain holder B (F is B's form; B goes into ``gone`` with the chain and the node is named ``<B's name><suffix>``),
    whose users are then the readers; without a B the last node's own users are, and F is A's form (``copies``: the module then
    copies codes, ``build(None)``) unless a reader below says otherwise; without ``copies`` a reader below has to say.  A reader is
    a wrapped layer ``consumer_for`` can take, fed by it alone (a QuantizedLinear only with ``rows``); with ``pools`` a max pool
    that can run on codes (``_pool_plan``); or a QuantizedConcat / QuantizedMul that reads it at exactly one operand, in the form
    F -- what the concatenation and multiply passes leave where they absorbed B.  Else None: a float32 reader, anything else
    between the operation and B, forms that differ."""
    last = chain[-1] if chain else first
    if not last.users:
        return None
    src, gone, name, out_quantizer = last, list(chain), None, None
    if len(last.users) == 1:
        nxt = next(iter(last.users))
        holder = _holder_of(nxt, mods)
        if holder is not None and nxt.args == (last,):
            if not nxt.users:
                return None
            src, gone, name, out_quantizer = nxt, gone + [nxt], nxt.target.replace(".", "_") + suffix, holder.activation_holder_quantizer
    try:
        form = _code_form(quantizer if out_quantizer is None else out_quantizer)
    except (TypeError, ValueError, NotImplementedError):
        return None
    operands, others = [], []                                # (reader, its quantizer and form for this operand); the other users
    for user in src.users:
        m = _module_of(user, mods)
        if not isinstance(m, (QuantizedConcat, QuantizedMul)):
            others.append(user)
            continue
        if user.kwargs or sum(a is src for a in user.args) != 1:
            return None
        at = next(i for i, a in enumerate(user.args) if a is src)
        operands.append((user, m.operand_quantizers[at], m.operand_code_params(at)))
    if src is last and operands and (not copies or operands[0][2] != form):   # no B: F is what the operand is read as
        if others:
            return None                                      # (a layer or a pool would read A's form)
        out_quantizer, form = operands[0][1:]
    if out_quantizer is None and not copies:
        return None                                          # (no B and no operand that supplies the form)
    if any(f != form for _, _, f in operands):
        return None
    reads_as = quantizer if out_quantizer is None else out_quantizer
    taken, pooled = [], []
    for user in others:
        fused = _wrapped_consumer(user, src, mods, reads_as, consumer_for)
        if fused is not None and (rows or type(fused) is not QuantizedLinear):
            taken.append((user, fused))
            continue
        behind = _pool_plan(user, mods, reads_as, consumer_for) if fused is None and pools else None
        if behind is None:
            return None
        pooled.append((user, behind))
    readers = [user for user, _, _ in operands]
    try:
        module = build(out_quantizer)
    except (TypeError, ValueError, NotImplementedError):
        return None
    return _PoolPlan(module, suffix, taken, gone, name, tuple(pooled), tuple(readers))


def _upsample_plan(node, mods, quantizer, consumer_for, pools: bool = False):
    """``node`` a user of a plain holder A with ``quantizer``: the plan of a QuantizedUpsample if it is a nearest upsample of A's
    output (``_upsample_of``) all of whose readers agree on one code form F and read codes (``_between_holders_plan``: through a
    plain holder B or directly, then in A's form or a QuantizedConcat / QuantizedMul operand's; never a QuantizedLinear).  Else
    None: a float32 reader, an activation between the upsample and B, forms that differ."""
    up = _upsample_of(node, mods)
    if up is None:
        return None
    return _between_holders_plan(node, [], mods, quantizer, consumer_for, pools, lambda out: QuantizedUpsample(up, quantizer, out),
                                 "_upsample", copies=True, rows=False)


def _activation_functions():
    """Functional spelling -> (module type, the constant arguments it may be given, in positional order)."""
    F = torch.nn.functional
    return {torch.sigmoid: (nn.Sigmoid, ()), F.sigmoid: (nn.Sigmoid, ()), torch.tanh: (nn.Tanh, ()), F.tanh: (nn.Tanh, ()),
            torch.relu: (nn.ReLU, ()), F.relu: (nn.ReLU, ("inplace",)), F.silu: (nn.SiLU, ("inplace",)),
            F.gelu: (nn.GELU, ("approximate",)), F.mish: (nn.Mish, ("inplace",)), F.softplus: (nn.Softplus, ("beta", "threshold")),
            F.elu: (nn.ELU, ("alpha", "inplace")), F.celu: (nn.CELU, ("alpha", "inplace")), F.selu: (nn.SELU, ("inplace",)),
            F.leaky_relu: (nn.LeakyReLU, ("negative_slope", "inplace")), F.hardswish: (nn.Hardswish, ("inplace",)),
            F.hardsigmoid: (nn.Hardsigmoid, ("inplace",)), F.hardtanh: (nn.Hardtanh, ("min_val", "max_val", "inplace")),
            F.relu6: (nn.ReLU6, ("inplace",)), F.logsigmoid: (nn.LogSigmoid, ()), F.softsign: (nn.Softsign, ()),
            F.tanhshrink: (nn.Tanhshrink, ())}


_ACTIVATION_METHODS = {"sigmoid": nn.Sigmoid, "tanh": nn.Tanh, "relu": nn.ReLU}


def _activation_of(node, mods):
    """The activation module that ``node`` applies to its one tensor operand, if QuantizedActivationTable can take it: a call of
    a module of one of its types, the functional spelling with constant arguments (``torch.sigmoid`` / ``torch.tanh`` /
    ``torch.relu`` and the ``F.*`` counterparts of the types), for which a module is built, or ``x.sigmoid()`` / ``x.tanh()`` /
    ``x.relu()``.  In-place forms only where nobody else looks at the input (``_in_place_ok``).  Else None."""
    from torch.fx import Node
    if not node.args or not isinstance(node.args[0], Node):
        return None
    fn, inplace = None, False
    if node.op == "call_module":
        if len(node.args) == 1 and not node.kwargs:
            fn = mods.get(node.target)
            inplace = getattr(fn, "inplace", False)
    elif node.op == "call_function":
        found = _activation_functions().get(node.target)
        given = _const_args(node, found[1]) if found is not None else None
        if given is None:
            return None
        inplace = given.pop("inplace", False)
        if not all(isinstance(v, (int, float, str)) and not isinstance(v, bool) for v in given.values()):
            return None
        try:
            fn = found[0](**given)
        except (TypeError, ValueError):
            return None
    elif node.op == "call_method" and node.target in _ACTIVATION_METHODS and len(node.args) == 1 and not node.kwargs:
        fn = _ACTIVATION_METHODS[node.target]()
    if fn is None or not QuantizedActivationTable.eligible(fn):
        return None
    if not isinstance(inplace, bool) or not _in_place_ok(node, inplace):
        return None
    return fn


def _table_chain(node, mods):
    """``([nodes], [modules])`` of the run of 1 to 4 elementwise activations (``_activation_of``) that starts at ``node``, each but
    the last with the next as its one user; None if ``node`` is no such activation or the run is longer."""
    nodes, fns = [], []
    while True:
        fn = _activation_of(node, mods)
        if fn is None:
            break
        nodes.append(node)
        fns.append(fn)
        if len(node.users) != 1:
            break
        node = next(iter(node.users))
    return (nodes, fns) if 1 <= len(nodes) <= _TABLE_CHAIN_MAX else None


def _table_plan(node, mods, quantizer, consumer_for, pools: bool = False):
    """``node`` a user of a plain holder A with ``quantizer``: the plan of a QuantizedActivationTable if it starts a run of 1 to 4
    elementwise activations of A's output (``_table_chain``) whose readers agree on one code form F and read codes
    (``_between_holders_plan``): the run's one user a plain holder B, every user of which reads codes in B's form, or without a B
    a QuantizedConcat / QuantizedMul operand that supplies the form.  Else None: no B and no such operand, a float32 reader of the
    run or of B, anything not eligible in the run, a node of it with two tensor operands or a scalar one."""
    found = _table_chain(node, mods)
    if found is None:
        return None
    nodes, fns = found
    return _between_holders_plan(node, nodes[1:], mods, quantizer, consumer_for, pools,
                                 lambda out: QuantizedActivationTable(fns, quantizer, out), "_table", copies=False, rows=True)


class QuantizedJoin(_OnCodes):
    """An activation holder with several consumers (the end of a residual block), its elementwise prologue folded in:
    ``forward(x, residual=None) -> (float32 or None, codes)`` with ``v = relu(x + residual)`` (each part as switched on),
    the float32 tensor what the holder returns for v -- for the users that stay in float32, None with ``want_float=False``
    -- and the codes what the integer consumers behind the holder would make of it themselves.  Dense GPU tensors take one
    launch of ``mctq_fq_join_f32`` (``ops.fq_join``): x and residual are read once.  The codes are NCHW-shaped and
    NHWC-stored, as a consumer's ``emit_codes_for`` output.

    A 4-D input that is NCHW-contiguous and not channels-last (a network's first holder: every consumer emits channels-last)
    takes the routes that were there before: the prologue by torch ops, the holder's own call, ``ops.fq_codes_nhwc``.

    The holder stays a submodule: its quantizer is the one in use, whose parameters are read when the join is built.

    ``residual_codes=(scale, zero_point)`` (with ``has_residual``): the second operand of ``forward`` is then an int8 / uint8
    tensor, the codes of another join with that scale and zero point (an identity branch that stays on codes), standing for
    the float32 tensor ``(codes - zero_point) * scale`` that join would have written: ``mctq_fq_join_rc_f32``, the same bits."""

    def __init__(self, holder, relu: bool = False, has_residual: bool = False, want_float: bool = True, residual_codes=None):
        super().__init__()
        if not _plain_holder(holder):
            raise TypeError("QuantizedJoin takes a PytorchActivationQuantizationHolder that quantizes")
        self.holder = holder
        self.relu, self.has_residual, self.want_float = bool(relu), bool(has_residual), bool(want_float)
        self._a_scale, self._a_zp, self._a_qmin, self._a_qmax = _activation_code_params(holder.activation_holder_quantizer)
        ops._code_dtype(self._a_qmin, self._a_qmax)            # (raises for a domain that is no 8-bit code)
        self.residual_codes = None
        if residual_codes is not None:
            if not self.has_residual:
                raise ValueError("residual_codes describes the residual operand: it needs has_residual=True")
            r_scale, r_zp = residual_codes
            self.residual_codes = (float(r_scale), int(r_zp))

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None):
        if (residual is not None) != self.has_residual:
            raise RuntimeError(f"this join was built {'with' if self.has_residual else 'without'} a residual operand")
        form = (self._a_scale, self._a_zp, self._a_qmin, self._a_qmax)
        r_codes = None
        if residual is not None and (residual.dtype in (torch.int8, torch.uint8)) != (self.residual_codes is not None):
            raise TypeError(f"this join was built for a residual operand {'as codes' if self.residual_codes else 'in float32'}, "
                            f"got {residual.dtype}")
        if self.residual_codes is not None:
            r_codes, residual = (residual, *self.residual_codes), None
        if x.dim() == 4 and x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last):
            if r_codes is not None:
                residual = ops.dequantize_codes(*r_codes)
            v = x if residual is None else x + residual
            if self.relu:
                v = torch.relu(v)
            y = self.holder(v) if self.want_float else None
            codes = ops.fq_codes_nhwc(v, self._a_qmin, self._a_qmax, self._a_scale, self._a_zp)
            return y, codes.permute(0, 3, 1, 2)
        return ops.fq_join(x, *form, residual=residual, relu=self.relu, want_float=self.want_float, want_codes=True,
                           residual_codes=r_codes)


def _in_place_ok(node, inplace) -> bool:
    """The rule for an in-place form (``inplace`` true) of an operation the rewrite folds into a module, which then no longer
    performs it on its first operand: nobody else may be looking at that operand."""
    return not inplace or len(node.args[0].users) == 1


def _relu_input(node, mods):
    """The input node of ``node`` if it is a ReLU of one tensor (``nn.ReLU``, ``F.relu``, ``torch.relu``, ``Tensor.relu``), else None."""
    from torch.fx import Node
    if len(node.args) != 1 or not isinstance(node.args[0], Node):
        return None
    if node.op == "call_module":
        ok = type(mods.get(node.target)) is nn.ReLU and not node.kwargs
    elif node.op == "call_function":
        ok = (node.target is torch.relu and not node.kwargs) or \
            (node.target is torch.nn.functional.relu and not set(node.kwargs) - {"inplace"})
    else:
        ok = node.op == "call_method" and node.target == "relu" and not node.kwargs
    inplace = getattr(_module_of(node, mods), "inplace", False) if node.op == "call_module" else node.kwargs.get("inplace", False)
    return node.args[0] if ok and _in_place_ok(node, inplace) else None


def _binary_operands(node, functions, methods, in_place):
    """The two operand nodes of ``node`` if it calls one of ``functions`` or, as a method, one of ``methods`` on two tensors and
    nothing else (no keyword, no scalar operand); ``in_place``, the in-place operator among ``functions``, under ``_in_place_ok``.
    Else None."""
    from torch.fx import Node
    if node.kwargs or len(node.args) != 2 or not all(isinstance(a, Node) for a in node.args):
        return None
    if node.op == "call_function":
        ok = node.target in functions and _in_place_ok(node, node.target is in_place)
    else:
        ok = node.op == "call_method" and node.target in methods
    return tuple(node.args) if ok else None


def _add_operands(node):
    """The two operand nodes of ``node`` if it is a plain add of two tensors (``+``, ``+=``, ``torch.add``, ``Tensor.add``:
    no ``alpha``, no scalar operand), else None."""
    return _binary_operands(node, (operator.add, operator.iadd, torch.add), ("add",), operator.iadd)


def _mul_operands(node):
    """The two operand nodes of ``node`` if it is a plain multiply of two tensors (``*``, ``*=``, ``torch.mul`` /
    ``torch.multiply``, ``Tensor.mul`` / ``Tensor.multiply``: no scalar operand, no ``out=``), else None."""
    return _binary_operands(node, (operator.mul, operator.imul, torch.mul, torch.multiply), ("mul", "multiply"), operator.imul)


def _join_shared_holders(gm, mods, consumer_for, pools: bool = False, avg_pools: bool = False, upsamples: bool = False,
                         activation_tables: bool = False) -> int:
    """``fuse_linear_consumers_fx(shared_holders=True)``: every plain holder with wrapped layers among its users that
    ``consumer_for(wrapper, quantizer)`` can take becomes a QuantizedJoin, unless it is a lone holder -> layer pair with
    nothing in front to absorb (the pair rewrite's).  With ``pools`` a max pool among the users that can run on codes
    (``_pool_plan``) reads the join's codes as well, as a QuantizedMaxPool2d in front of its own consumers; a lone holder ->
    pool pair with nothing to absorb is left to ``_pool_lone_holders``.  With ``avg_pools`` the same holds for an average pool
    in front of a second holder (``_avg_pool_plan``), as a QuantizedAvgPool2d.  A QuantizedMul among the users
    (``_operator_between_holders``, which built it with this holder's quantizer at that operand) reads the join's codes too, at
    whichever operand position the holder occupies, and so does a user that leads, through layout-only nodes, to operands of a
    QuantizedMatmul built with this holder's quantizer (``_matmuls_on_codes``).  With ``upsamples`` a nearest upsample among the users whose readers all read
    codes (``_upsample_plan``) does so as a QuantizedUpsample, and the holder behind such an upsample is left to that plan; with
    ``activation_tables`` likewise a run of elementwise activations (``_table_plan``), as a QuantizedActivationTable.
    Returns the number of wrapped layers replaced."""
    replaced = 0
    for node, holder in _holder_calls(gm, mods):
        if (upsamples or activation_tables) and node.users and \
                _behind_planned_operation(node, mods, consumer_for, pools, upsamples, activation_tables):
            continue
        quantizer = holder.activation_holder_quantizer
        # F: (user node, its consumer)
        taken = [(user, _wrapped_consumer(user, node, mods, quantizer, consumer_for)) for user in node.users]
        taken = [(user, fused) for user, fused in taken if fused is not None]
        pooled = []                                          # P: (pool node, its plan)
        if pools or avg_pools or upsamples or activation_tables:
            plans = ((user, _any_pool_plan(user, mods, quantizer, consumer_for, pools, avg_pools, upsamples, activation_tables))
                     for user in node.users)
            pooled = [(user, plan) for user, plan in plans if plan is not None]
        # M: the QuantizedMul nodes of ``_operator_between_holders`` that read this holder (built with its quantizer at those operands)
        muls = [user for user in node.users if isinstance(_module_of(user, mods), QuantizedMul) and not user.kwargs]
        # ... and the users that lead, through layout-only nodes, to operands of a QuantizedMatmul built with this quantizer
        # (``_matmuls_on_codes``): they move the join's codes as they would have moved the float32 tensor
        try:
            muls += [user for user in node.users
                     if _reads_as_matmul_operands(user, node, _code_form(quantizer), mods) and all(user is not t for t in muls)]
        except (TypeError, ValueError, NotImplementedError):
            pass
        if not taken and not pooled and not muls:
            continue
        on_codes = [t for t, _ in taken] + [t for t, _ in pooled] + muls
        rest = [u for u in node.users if all(u is not t for t in on_codes)]           # R: they keep the float32 tensor
        src, relu_node, add_node = node.args[0], None, None
        if len(src.users) == 1 and _relu_input(src, mods) is not None:
            relu_node, src = src, _relu_input(src, mods)
        if len(src.users) == 1 and _add_operands(src) is not None:
            add_node = src
        if len(node.users) == 1 and relu_node is None and add_node is None:
            continue                                         # a plain pair
        try:
            join = QuantizedJoin(holder, relu=relu_node is not None, has_residual=add_node is not None, want_float=bool(rest))
        except (TypeError, ValueError):
            continue
        name = node.target.replace(".", "_") + "_join"
        gm.add_submodule(name, join)
        mods[name] = join
        with gm.graph.inserting_before(node):
            jn = gm.graph.call_module(name, _add_operands(add_node) if add_node is not None else (src,))
            as_float = gm.graph.call_function(operator.getitem, (jn, 0)) if rest else None
            as_codes = gm.graph.call_function(operator.getitem, (jn, 1))
        for user, fused in taken:
            _install_consumer(gm, mods, user, fused)
            user.args = (as_codes,)
            replaced += 1
        for user, plan in pooled:
            replaced += _install_pool(gm, mods, user, plan, as_codes)
        for user in muls:                                    # at whichever operand position(s) the holder occupies
            user.args = tuple(as_codes if a is node else a for a in user.args)
        if rest:
            node.replace_all_uses_with(as_float)
        for gone in (node, relu_node, add_node):
            if gone is not None:
                gm.graph.erase_node(gone)
    return replaced


def _any_pool_plan(node, mods, quantizer, consumer_for, pools: bool, avg_pools: bool, upsamples: bool = False,
                   activation_tables: bool = False):
    """``_pool_plan`` (with ``pools``), or else ``_avg_pool_plan`` (with ``avg_pools``), or else ``_upsample_plan`` (with
    ``upsamples``), or else ``_table_plan`` (with ``activation_tables``) of ``node``, or None."""
    plan = _pool_plan(node, mods, quantizer, consumer_for) if pools else None
    if plan is None and avg_pools:
        plan = _avg_pool_plan(node, mods, quantizer, consumer_for)
    if plan is None and upsamples:
        plan = _upsample_plan(node, mods, quantizer, consumer_for, pools)
    if plan is None and activation_tables:
        plan = _table_plan(node, mods, quantizer, consumer_for, pools)
    return plan


def _behind_planned_operation(node, mods, consumer_for, pools: bool, upsamples: bool, activation_tables: bool) -> bool:
    """``node``, a plain holder's call, is the second holder of an upsample or of a run of activations that will run on codes
    (``_upsample_plan`` / ``_table_plan`` of the user of another plain holder that leads to it): it belongs to that plan, whatever
    the number of its users."""
    from torch.fx import Node
    first = node.args[0]
    for _ in range(_TABLE_CHAIN_MAX if activation_tables else 1):
        if not first.args or not isinstance(first.args[0], Node):
            return False
        holder = _holder_of(first.args[0], mods)
        if holder is not None:                               # ``first`` is the user of a holder A that leads here
            quantizer = holder.activation_holder_quantizer
            plan = _upsample_plan(first, mods, quantizer, consumer_for, pools) if upsamples else None
            if plan is None and activation_tables:
                plan = _table_plan(first, mods, quantizer, consumer_for, pools)
            return plan is not None and node in plan.gone
        first = first.args[0]
    return False


def _pool_lone_holders(gm, mods, consumer_for, pools: bool = True, avg_pools: bool = False, upsamples: bool = False,
                       activation_tables: bool = False) -> int:
    """``fuse_linear_consumers_fx(pools=True)``, the pair: a plain holder whose only user is a max pool that can run on codes
    (``_pool_plan``) leaves the graph, the QuantizedMaxPool2d that replaces the pool quantizes the holder's input itself.
    With ``avg_pools`` likewise for an average pool in front of a second holder (``_avg_pool_plan``) and its QuantizedAvgPool2d,
    with ``upsamples`` for a nearest upsample (``_upsample_plan``) and its QuantizedUpsample, with ``activation_tables`` for a run
    of elementwise activations (``_table_plan``) and its QuantizedActivationTable.
    Returns the number of wrapped layers replaced."""
    replaced = 0
    for node, holder in _holder_calls(gm, mods):
        if len(node.users) != 1:
            continue
        user = next(iter(node.users))
        plan = _any_pool_plan(user, mods, holder.activation_holder_quantizer, consumer_for, pools, avg_pools, upsamples,
                              activation_tables)
        if plan is None:
            continue
        replaced += _install_pool(gm, mods, user, plan, node.args[0])
        gm.graph.erase_node(node)
    return replaced


def _cat_operands(node):
    """The operand nodes of ``node`` if it is ``torch.cat`` / ``torch.concat`` / ``torch.concatenate`` of a list or tuple of 2 to
    8 nodes along the constant dimension 1 (positional or ``dim=``; no ``out=``), else None."""
    from torch.fx import Node
    if node.op != "call_function" or node.target not in (torch.cat, torch.concat, torch.concatenate):
        return None
    if not 1 <= len(node.args) <= 2 or set(node.kwargs) - ({"dim"} if len(node.args) == 1 else set()):
        return None
    dim = node.args[1] if len(node.args) == 2 else node.kwargs.get("dim", 0)
    if not isinstance(dim, int) or isinstance(dim, bool) or dim != 1:
        return None
    tensors = node.args[0]
    if not isinstance(tensors, (list, tuple)) or not 2 <= len(tensors) <= 8 or not all(isinstance(t, Node) for t in tensors):
        return None
    return list(tensors)


def _operator_between_holders(gm, mods, consumer_for, pools, operands_of, cls, suffix) -> int:
    """``fuse_linear_consumers_fx(concats=True)`` with ``(_cat_operands, QuantizedConcat, "_concat")`` and ``(muls=True)`` with
    ``(_mul_operands, QuantizedMul, "_mul")``, one whole pass over the graph each: a plain holder whose one argument is that
    operator (``operands_of``) and feeds nothing else, every operand of which is the output of a plain holder, and every user of
    which is a wrapped layer ``consumer_for`` can take, fed by it alone -- or, with ``pools``, a max pool that can run on codes
    (``_pool_plan``) -- becomes a node of ``cls``, named ``<the holder's name><suffix>``, together with the operator; its users
    become consumers and pools of its codes.  An operand holder whose only user was the operator leaves the graph and the module
    quantizes that holder's input (a QuantizedMul a ``[B, C, 1, 1]`` gate inside its kernel); one with other users stays and the
    module quantizes its float32 output (the same codes) until ``_join_shared_holders`` hands a QuantizedMul the codes.
    Returns the number of wrapped layers replaced."""
    replaced = 0
    for node, holder in _holder_calls(gm, mods):
        op = node.args[0]
        operands = operands_of(op)
        if not node.users or operands is None or len(op.users) != 1:
            continue
        sources = [_holder_of(o, mods) for o in operands]
        if None in sources:
            continue
        quantizer = holder.activation_holder_quantizer
        taken, pooled = [], []
        for user in node.users:
            fused = _wrapped_consumer(user, node, mods, quantizer, consumer_for)
            if fused is not None:
                taken.append((user, fused))
                continue
            plan = _pool_plan(user, mods, quantizer, consumer_for) if pools else None
            if plan is None:
                break
            pooled.append((user, plan))
        else:
            try:
                module = cls([h.activation_holder_quantizer for h in sources], quantizer)
            except (TypeError, ValueError, NotImplementedError):
                continue
            name = node.target.replace(".", "_") + suffix
            gm.add_submodule(name, module)
            mods[name] = module
            absorbed = [o for o in dict.fromkeys(operands) if len(o.users) == 1]
            with gm.graph.inserting_before(node):
                on_codes = gm.graph.call_module(name, tuple(o.args[0] if o in absorbed else o for o in operands))
            for user, fused in taken:
                _install_consumer(gm, mods, user, fused)
                user.args = (on_codes,)
                replaced += 1
            for user, plan in pooled:
                replaced += _install_pool(gm, mods, user, plan, on_codes)
            for gone in (node, op, *absorbed):
                gm.graph.erase_node(gone)
    return replaced


_LAYOUT_METHODS = ("reshape", "view", "permute", "transpose", "contiguous", "flatten", "unflatten")
_LAYOUT_FUNCTIONS = (torch.reshape, torch.permute, torch.transpose, torch.flatten, torch.unflatten)


def _layout_input(node):
    """The tensor operand of ``node`` if it is a layout-only node, else None: ``reshape``, ``view``, ``permute``, ``transpose``,
    ``contiguous``, ``flatten``, ``unflatten`` (methods, or the ``torch.`` functions of those names) with integer arguments --
    never a ``view(dtype)`` --, ``operator.getitem`` with one constant integer index, or ``.mT``.  Such a node only moves data, so it
    commutes with coding: the codes of its output are its output on the codes.  The one list of both sides of a QuantizedMatmul."""
    from torch.fx import Node
    if not node.args or not isinstance(node.args[0], Node):
        return None

    def ints(v):
        if isinstance(v, (tuple, list, torch.Size)):
            return all(ints(e) for e in v)
        return isinstance(v, (int, torch.memory_format)) and not isinstance(v, bool)

    rest = node.args[1:]
    if node.op == "call_function" and node.target is operator.getitem:
        ok = len(rest) == 1 and isinstance(rest[0], int) and not isinstance(rest[0], bool) and not node.kwargs
    elif node.op == "call_function" and node.target is getattr:
        ok = rest == ("mT",)
    else:
        ok = (node.op == "call_method" and node.target in _LAYOUT_METHODS) or \
            (node.op == "call_function" and node.target in _LAYOUT_FUNCTIONS)
        ok = ok and ints(rest) and ints(tuple(node.kwargs.values()))
    return node.args[0] if ok else None


def _layout_name(node) -> str:
    return node.target if node.op == "call_method" else getattr(node.target, "__name__", "")


def _behind_layout_chain(node):
    """The node a layout-only chain that ends in ``node`` starts from (``node`` itself where it is no layout node)."""
    while _layout_input(node) is not None:
        node = _layout_input(node)
    return node


def _layout_rank(node):
    """The rank of a layout node's output where its own arguments or those of the chain in front tell it, else None."""
    src = _layout_input(node)
    if src is None:
        return None
    name, rest = _layout_name(node), node.args[1:]
    if name in ("permute", "reshape", "view"):
        return len(rest[0]) if len(rest) == 1 and isinstance(rest[0], (tuple, list)) else len(rest) or None
    if name in ("transpose", "contiguous", "getattr"):
        return _layout_rank(src)
    if name == "getitem":
        rank = _layout_rank(src)
        return None if rank is None else rank - 1
    return None


def _swaps_last_two(node) -> bool:
    """``node`` is ``x.transpose(-1, -2)`` / ``torch.transpose(x, -1, -2)``, in either order, a positive-index spelling of it (where
    the chain in front tells the rank: behind a permute, reshape or view), or ``x.mT``."""
    if _layout_input(node) is None:
        return False
    name = _layout_name(node)
    if name == "getattr":
        return True
    if name != "transpose":
        return False
    dims = tuple(node.args[1:]) + tuple(node.kwargs.get(k) for k in ("dim0", "dim1") if k in node.kwargs)
    if len(dims) != 2:
        return False
    if set(dims) == {-1, -2}:
        return True
    rank = _layout_rank(node)
    return rank is not None and {d % rank for d in dims} == {rank - 1, rank - 2}


def _matmul_operands(node):
    """The two operand nodes of ``node`` if it is ``torch.matmul`` / ``@`` / ``Tensor.matmul`` / ``torch.bmm`` of two tensors without
    keyword arguments, else None."""
    from torch.fx import Node
    if node.kwargs or len(node.args) != 2 or not all(isinstance(a, Node) for a in node.args):
        return None
    if node.op == "call_function":
        ok = node.target in (torch.matmul, operator.matmul, torch.bmm)
    else:
        ok = node.op == "call_method" and node.target == "matmul"
    return tuple(node.args) if ok else None


def _reads_as_matmul_operands(user, via, form, mods) -> bool:
    """``user`` reads ``via`` -- a tensor that is, or stands for, codes of ``form`` -- only as such codes: a QuantizedMatmul that
    takes it at operands of that form, or a layout-only node (``_layout_input``) every user of which does in turn."""
    m = _module_of(user, mods)
    if isinstance(m, QuantizedMatmul):
        return not user.kwargs and len(user.args) == 2 and \
            all(m.operand_code_params(i) == tuple(form) for i, a in enumerate(user.args) if a is via)
    if _layout_input(user) is not via or not user.users:
        return False
    return all(_reads_as_matmul_operands(u, user, form, mods) for u in user.users)


def _matmul_operand_form(node, mods):
    """The one form (scale, zero_point, qmin, qmax) in which every user of ``node`` reads it as a QuantizedMatmul operand,
    through layout-only nodes (``_reads_as_matmul_operands``), or None."""
    at = node
    while at.users:                                      # any one leaf names the form; all of them must agree on it
        user = next(iter(at.users))
        m = _module_of(user, mods)
        if isinstance(m, QuantizedMatmul):
            form = next((m.operand_code_params(i) for i, a in enumerate(user.args) if a is at), None)
            if form is None or not all(_reads_as_matmul_operands(u, node, form, mods) for u in node.users):
                return None
            return form
        if _layout_input(user) is not at:
            return None
        at = user
    return None


def _matmuls_on_codes(gm, mods, consumer_for) -> int:
    """``fuse_linear_consumers_fx(matmuls=True)``, three steps.  (1) Every matmul node (``_matmul_operands``) each operand of which
    leads back to a plain holder's output through layout-only nodes (``_layout_input``) becomes a QuantizedMatmul node with the two
    holders' quantizers; a final swap of the last two dimensions on the second operand that feeds nothing else
    (``_swaps_last_two``) is absorbed as ``transposed_b=True`` and leaves the graph.  (2) A plain holder that is the one user of such
    a node and every user of which reads codes -- through layout-only nodes: a wrapped ``nn.Linear`` ``consumer_for`` can take, fed
    by it alone, which becomes a QuantizedLinear; an operand of a QuantizedMatmul of that form -- is absorbed: the node emits
    its codes.  Likewise where the node's one user is a QuantizedConcat / QuantizedMul that absorbed the holder and reads the
    node at one operand.  (3) An operand holder every user of which leads to QuantizedMatmul operands leaves the graph: the
    module quantizes that holder's input (or, with ``stay_on_codes``, the layer in front emits the codes); a holder with other
    users stays and the module quantizes its float32 output -- the same codes.  Returns the number of wrapped layers replaced."""
    replaced, made = 0, []
    for node in list(gm.graph.nodes):
        operands = _matmul_operands(node)
        if operands is None:
            continue
        x0, x1 = operands
        transposed = _swaps_last_two(x1) and len(x1.users) == 1
        ends = (x0, x1.args[0] if transposed else x1)
        holders = [_holder_of(_behind_layout_chain(e), mods) for e in ends]
        if None in holders:
            continue
        try:
            module = QuantizedMatmul([h.activation_holder_quantizer for h in holders], None, transposed_b=transposed)
        except (TypeError, ValueError, NotImplementedError):
            continue
        name = node.name + "_qmatmul"
        gm.add_submodule(name, module)
        mods[name] = module
        with gm.graph.inserting_before(node):
            new = gm.graph.call_module(name, ends)
        node.replace_all_uses_with(new)
        gm.graph.erase_node(node)
        if transposed:
            gm.graph.erase_node(x1)
        made.append(new)
    for new in made:                                         # (2) the holder behind
        if len(new.users) != 1:
            continue
        behind = next(iter(new.users))
        module, reader = mods[new.target], _module_of(behind, mods)
        taken, quantizer = [], None
        if isinstance(reader, (QuantizedConcat, QuantizedMul)) and not behind.kwargs and sum(a is new for a in behind.args) == 1:
            quantizer, hnode = reader.operand_quantizers[next(i for i, a in enumerate(behind.args) if a is new)], None
        else:
            holder, hnode = _holder_of(behind, mods), behind
            if holder is None or not hnode.users:
                continue
            quantizer = holder.activation_holder_quantizer
            try:
                form = _code_form(quantizer)
            except (TypeError, ValueError, NotImplementedError):
                continue

            def reads_codes(user, via):
                fused = _wrapped_consumer(user, via, mods, quantizer, consumer_for)
                if fused is not None:
                    taken.append((user, fused))
                    return type(fused) is QuantizedLinear
                if isinstance(_module_of(user, mods), QuantizedMatmul):
                    return _reads_as_matmul_operands(user, via, form, mods)
                return _layout_input(user) is via and bool(user.users) and all(reads_codes(u, user) for u in user.users)

            if not all(reads_codes(u, hnode) for u in hnode.users):
                continue
        try:
            emitting = QuantizedMatmul(module.operand_quantizers, quantizer, transposed_b=module.transposed_b)
        except (TypeError, ValueError, NotImplementedError):
            continue
        setattr(gm, new.target, emitting)                    # (the name has no dots: step (1) made it)
        mods[new.target] = emitting
        for user, fused in taken:
            _install_consumer(gm, mods, user, fused)
            replaced += 1
        if hnode is not None:
            hnode.replace_all_uses_with(new)
            gm.graph.erase_node(hnode)
    for node, holder in _holder_calls(gm, mods):             # (3) the operand holders nobody else reads
        try:
            form = _code_form(holder.activation_holder_quantizer)
        except (TypeError, ValueError, NotImplementedError):
            continue
        if node.users and all(_reads_as_matmul_operands(u, node, form, mods) for u in node.users):
            node.replace_all_uses_with(node.args[0])
            gm.graph.erase_node(node)
    return replaced


def _clamp_range(node, mods):
    """(a, b) if ``node`` is a clamp activation of one tensor that ``folded_clamp`` can fold -- a ReLU (as ``_relu_input``),
    ``nn.ReLU6`` / ``F.relu6``, ``nn.Hardtanh`` / ``F.hardtanh`` with finite ``min_val <= max_val`` -- else None.  In-place forms
    only where nobody else looks at the input."""
    from torch.fx import Node
    F = torch.nn.functional
    if _relu_input(node, mods) is not None:
        return 0.0, math.inf
    if not node.args or not isinstance(node.args[0], Node):
        return None
    rng, inplace = None, False
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        m = mods.get(node.target)
        if type(m) is nn.ReLU6:
            rng, inplace = (0.0, 6.0), m.inplace
        elif type(m) is nn.Hardtanh:
            rng, inplace = (m.min_val, m.max_val), m.inplace
    elif node.op == "call_function" and node.target is F.relu6:
        if len(node.args) == 1 and not set(node.kwargs) - {"inplace"}:
            rng, inplace = (0.0, 6.0), node.kwargs.get("inplace", False)
    elif node.op == "call_function" and node.target is F.hardtanh:
        given = _const_args(node, ("min_val", "max_val", "inplace"))
        if given is not None:
            rng, inplace = (given.get("min_val", -1.0), given.get("max_val", 1.0)), given.get("inplace", False)
    if rng is None or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in rng) or not rng[0] <= rng[1]:
        return None
    if not isinstance(inplace, bool) or not _in_place_ok(node, inplace):
        return None
    return float(rng[0]), float(rng[1])


def _hard_activation(node, mods):
    """"hardswish" / "hardsigmoid" if ``node`` is that activation of one tensor -- ``nn.Hardswish`` / ``nn.Hardsigmoid`` modules,
    ``F.hardswish`` / ``F.hardsigmoid`` with at most a constant ``inplace`` -- else None.  In-place forms only where nobody else
    looks at the input (as ``_clamp_range``)."""
    from torch.fx import Node
    F = torch.nn.functional
    if not node.args or not isinstance(node.args[0], Node):
        return None
    kind, inplace = None, False
    if node.op == "call_module" and len(node.args) == 1 and not node.kwargs:
        m = mods.get(node.target)
        if type(m) in (nn.Hardswish, nn.Hardsigmoid):
            kind, inplace = ("hardswish" if type(m) is nn.Hardswish else "hardsigmoid"), m.inplace
    elif node.op == "call_function" and node.target in (F.hardswish, F.hardsigmoid):
        given = _const_args(node, ("inplace",))
        if given is not None:
            kind, inplace = ("hardswish" if node.target is F.hardswish else "hardsigmoid"), given.get("inplace", False)
    if kind is None or not isinstance(inplace, bool) or not _in_place_ok(node, inplace):
        return None
    return kind


def _takes_hard_activation(consumer) -> bool:
    """The entry points with an activation: the depthwise convolution with any weights; the product with int8 weights that
    have no zero points, no packed 4-bit / codebook form and no residual."""
    if isinstance(consumer, QuantizedDepthwiseConv2d):
        return True
    return (isinstance(consumer, QuantizedLinear) and not consumer._uniform_weights and not consumer._lut_weights
            and consumer.weights_quantizer.num_bits > 4 and consumer.emit_residual is None)


def _identities_as_codes(gm, mods) -> int:
    """``fuse_linear_consumers_fx(stay_on_codes=True)``, the identity branches: a join with a residual one of whose add operands
    is the float32 output of another join takes that join's codes in its place (``QuantizedJoin(residual_codes=...)``; IEEE
    addition is commutative, so either operand may move to the second place; where both qualify, one is converted), and a join
    whose float32 output then has no users stops writing it.  Returns the number of joins converted."""

    def pick(node, index):
        """(the join node, its module) if ``node`` is ``join(...)[index]``."""
        if node.op == "call_function" and node.target is operator.getitem and len(node.args) == 2 and node.args[1] == index:
            m = _module_of(node.args[0], mods)
            if isinstance(m, QuantizedJoin):
                return node.args[0], m
        return None

    converted = 0
    for node in list(gm.graph.nodes):
        join = _module_of(node, mods)
        if not isinstance(join, QuantizedJoin) or not join.has_residual or join.residual_codes is not None or len(node.args) != 2:
            continue
        for i in (1, 0):
            as_float = node.args[i]
            up = pick(as_float, 0)
            if up is None:
                continue
            up_node, up_join = up
            as_codes = next((u for u in up_node.users if pick(u, 1) is not None), None)
            if as_codes is None:
                with gm.graph.inserting_after(up_node):
                    as_codes = gm.graph.call_function(operator.getitem, (up_node, 1))
            new = QuantizedJoin(join.holder, relu=join.relu, has_residual=True, want_float=join.want_float,
                                residual_codes=(up_join._a_scale, up_join._a_zp))
            setattr(gm, node.target, new)                # (a join's name has no dots: _join_shared_holders made it)
            mods[node.target] = new
            node.args = (node.args[1 - i], as_codes)
            if not as_float.users:
                gm.graph.erase_node(as_float)
                up_join.want_float = False
            converted += 1
            break
    return converted


def _reads_codes_once(reader, codes, form, mods) -> bool:
    """``reader`` takes the node ``codes`` -- activation codes of ``form`` -- at exactly one operand and reads it as that form:
    a module of ``_CODE_READERS`` whose one argument it is, or a QuantizedMul or QuantizedMatmul, which have two operands, at one
    of them -- or a layout-only node behind which every reader is a QuantizedMatmul operand of that form
    (``_reads_as_matmul_operands``)."""
    m = _module_of(reader, mods)
    if m is None:
        return _reads_as_matmul_operands(reader, codes, form, mods)
    if reader.kwargs or sum(a is codes for a in reader.args) != 1:
        return False
    if isinstance(m, _CODE_READERS):
        return len(reader.args) == 1
    return isinstance(m, (QuantizedMul, QuantizedMatmul)) and len(reader.args) == 2 and \
        m.operand_code_params(0 if reader.args[0] is codes else 1) == tuple(form)


def _fold_clamps_into_producers(gm, mods, hard_activations: bool = False) -> int:
    """``fuse_linear_consumers_fx(stay_on_codes=True)``, the activations between consumers: where a consumer's only user leads
    -- through at most one clamp activation that feeds nothing else (``_clamp_range``; the ReLU a join absorbed counts), or with
    ``hard_activations=True`` one Hardswish / Hardsigmoid (``_hard_activation``) behind a consumer that takes one
    (``_takes_hard_activation``), which is not folded into the clamp but applied in the consumer's epilogue (``emit_act``) -- to a
    holder all of whose users read codes (``_CODE_READERS``: integer consumers, and the pools the passes before this one put
    in front of such), the consumer emits that holder's codes itself, the activation folded into their clamp (``folded_clamp``),
    and the modules behind take them directly.  The holder is either already inside the one reader behind it (the pair
    rewrites) or a residual-free QuantizedJoin that writes no float32 output.  Which kinds of reader occur is decided by the
    modules the earlier passes left in the graph, not by a switch of this function.  The reader may also be a QuantizedConcat
    among whose arguments the consumer's output (or its one clamp activation) occurs exactly once, at index i: the consumer then
    emits the codes of ``operand_code_params(i)``, the clamp folded in, and that one argument becomes the consumer's output.  A
    QuantizedMul is such a reader too, directly or among the readers of a join's codes, where those codes occur at exactly one
    of its two operands (``x * x`` is left to the module's float32 quantize path).  A QuantizedMatmul is such a reader as well,
    directly (a clamp activation in between is folded) or -- without an activation -- through layout-only nodes
    (``_layout_input``: the reshape and permute between a q / k / v layer and the product, which then move int8): every user of the
    consumer must lead to QuantizedMatmul operands of one form (``_matmul_operand_form``), which the consumer then emits.  Returns
    the number of producers that now emit codes."""
    folded = 0
    for node in list(gm.graph.nodes):
        producer = _module_of(node, mods)
        if not isinstance(producer, IntegerConsumer) or producer.emit_codes_for is not None:
            continue
        if node.users and _module_of(next(iter(node.users)), mods) is None:
            # every user leads, through layout-only nodes and no activation, to QuantizedMatmul operands of one form (the holder
            # in between went into them: _matmuls_on_codes): the producer emits that form and the chain moves int8
            form = _matmul_operand_form(node, mods)
            if form is not None and len(node.args) == 1:
                producer.emit_codes_for = form
                folded += 1
                continue
        if len(node.users) != 1:
            continue
        nxt, act, rng, hard = next(iter(node.users)), None, (-math.inf, math.inf), None
        if _clamp_range(nxt, mods) is not None and len(nxt.users) == 1:
            act, rng = nxt, _clamp_range(nxt, mods)
            nxt = next(iter(nxt.users))
        elif hard_activations and _hard_activation(nxt, mods) is not None and len(nxt.users) == 1 \
                and _takes_hard_activation(producer):
            act, hard = nxt, _hard_activation(nxt, mods)
            nxt = next(iter(nxt.users))
        if nxt.op != "call_module" or nxt.kwargs:
            continue
        behind, gone, src, concat_args = mods.get(nxt.target), [nxt], act or node, None
        via = src                                        # what the readers read now
        if isinstance(behind, (QuantizedConcat, QuantizedMul, QuantizedMatmul)):
            if sum(a is src for a in nxt.args) != 1:
                continue                                 # (the same tensor at two places -- x * x, two forms of a cat: left alone)
            at = next(i for i, a in enumerate(nxt.args) if a is src)
            form, readers, gone = behind.operand_code_params(at), [], []
            concat_args = tuple(node if a is src else a for a in nxt.args)
        elif nxt.args != (src,):
            continue
        elif isinstance(behind, _CODE_READERS):
            form, readers, gone = behind.activation_code_params(), [nxt], []
        elif isinstance(behind, QuantizedJoin) and not behind.has_residual and not behind.want_float:
            if behind.relu:
                if act is not None:
                    continue                             # two activations in a row: left alone
                rng = (0.0, math.inf)
            picks = list(nxt.users)
            if len(picks) != 1 or picks[0].target is not operator.getitem or picks[0].args != (nxt, 1):
                continue
            form, readers, via = (behind._a_scale, behind._a_zp, behind._a_qmin, behind._a_qmax), list(picks[0].users), picks[0]
            if not readers or not all(_reads_codes_once(r, via, form, mods) for r in readers):
                continue
            gone = [picks[0], nxt]
        else:
            continue
        try:
            ops._code_dtype(form[2], form[3])
            clamp = folded_clamp(form, *rng)
        except ValueError:
            continue
        producer.emit_codes_for, producer.emit_clamp = form, (None if clamp == (form[2], form[3]) else clamp)
        producer.emit_act = hard                         # (then rng is the whole line and emit_clamp None)
        for r in readers:
            r.args = tuple(node if a is via else a for a in r.args)
        if concat_args is not None:
            nxt.args = concat_args
        for g in gone + ([act] if act is not None else []):
            gm.graph.erase_node(g)
        if gone:
            gm.delete_submodule(nxt.target)
            mods.pop(nxt.target, None)
        folded += 1
    return folded


def _fuse_residuals_into_producers(gm, mods) -> int:
    """``fuse_linear_consumers_fx(fused_residuals=True)``: a residual join that writes codes only, one of whose operands is the
    output of a QuantizedLinear-derived consumer (weights without zero points) that feeds nothing else, emits nothing yet and
    is evaluated after the other operand, leaves the graph: that consumer takes the other operand as its residual, adds it
    and applies the join's ReLU in its own epilogue and emits the join's codes (``mctq_qlinear_i8_res``).  IEEE addition is
    commutative, so either operand may be the product; the one evaluated last is, as the other has to exist when it runs.
    Returns the number of joins removed."""
    order = {n: i for i, n in enumerate(gm.graph.nodes)}
    fused = 0
    for node in list(gm.graph.nodes):
        join = _module_of(node, mods)
        if not isinstance(join, QuantizedJoin) or not join.has_residual or join.want_float or len(node.args) != 2 or node.kwargs:
            continue
        picks = list(node.users)
        if not picks or not all(p.op == "call_function" and p.target is operator.getitem and p.args == (node, 1) for p in picks):
            continue
        for i in ((0,) if join.residual_codes is not None else (0, 1)):       # (codes are the join's second operand)
            prod, other = node.args[i], node.args[1 - i]
            consumer = _module_of(prod, mods)
            if (isinstance(consumer, QuantizedLinear) and not consumer._uniform_weights and consumer.emit_codes_for is None
                    and consumer.emit_residual is None and len(prod.users) == 1 and len(prod.args) == 1 and not prod.kwargs
                    and order[prod] > order[other]):
                break
        else:
            continue
        consumer.emit_codes_for = (join._a_scale, join._a_zp, join._a_qmin, join._a_qmax)
        consumer.emit_residual = join.residual_codes if join.residual_codes is not None else "float"
        consumer.emit_relu = join.relu
        prod.args = (prod.args[0], other)
        for p in picks:
            p.replace_all_uses_with(prod)
            gm.graph.erase_node(p)
        gm.graph.erase_node(node)
        gm.delete_submodule(node.target)
        mods.pop(node.target, None)
        fused += 1
    return fused


def fuse_linear_consumers(model: nn.Module, chain: bool = False, uniform_weights: bool = False,
                          convolutions: bool = False, depthwise: bool = False, pools: bool = False,
                          avg_pools: bool = False, upsamples: bool = False, any_channels: bool = False,
                          activation_tables: bool = False, grouped: bool = False, transposed: bool = False) -> int:
    """In every ``nn.Sequential`` of ``model``: an activation holder directly followed by a wrapped ``nn.Linear`` with
    a symmetric, power-of-two or LUT weights quantizer (int8 codebook values, at most 256 entries) becomes (Identity,
    QuantizedLinear); a wrapped pointwise ``nn.Conv2d`` likewise becomes a QuantizedConv1x1.  Returns the number of pairs
    replaced.  Pairs the integer consumer cannot take (other layers, LUT weights with
    ``lut_values_bitwidth`` > 8 or thresholds along another axis than the output channels, K % 16 != 0) are left alone.

    ``uniform_weights=True`` also fuses pairs whose weights quantizer is uniform (at most 8 bits, per tensor or per output
    channel): the product then honours the weights' zero points at the cost of one small launch per forward (the row sums
    of the activation codes), and large whole-tile products run on the tiled kernels rather than the faster whole-tile
    ones.  By default such pairs are left alone.

    ``convolutions=True`` also fuses the other wrapped ``nn.Conv2d`` layers -- k x k, strided, padded, dilated -- into a
    QuantizedConv2d (``groups == 1``, symmetric zero padding, ``in_channels % 16 == 0``, ``kh * kw * in_channels`` <= 32768,
    the activation zero point inside its clamp domain).  Each of them materialises a patch matrix of ``kh * kw`` bytes per
    output pixel and input channel per forward, so by default such pairs are left alone.

    ``depthwise=True`` also fuses wrapped depthwise ``nn.Conv2d`` layers (``groups == in_channels == out_channels``, symmetric
    zero padding, ``in_channels % 16 == 0``, ``kh * kw`` <= 256, the activation zero point inside its clamp domain) into a
    QuantizedDepthwiseConv2d, a direct convolution on the codes without a patch matrix.  It is independent of
    ``convolutions``: neither switch implies the other, and other grouped convolutions are always left alone unless
    ``grouped=True``.

    ``grouped=True`` also fuses the other wrapped grouped ``nn.Conv2d`` layers (``groups >= 2``, ``in_channels / groups`` a
    multiple of 4, symmetric zero padding, ``kh * kw * in_channels / groups`` <= 32768, the activation zero point inside its
    clamp domain) into a QuantizedGroupedConv2d: the 3 x 3 layer of a ResNeXt or RegNet bottleneck, ShuffleNet's grouped
    pointwise layers -- one direct convolution on the codes on the integer matrix cores (``mctq_qconv_grouped_i8``), without a
    patch matrix.  It is independent of ``convolutions`` and ``depthwise`` and composes with every other switch; depthwise
    layers stay ``depthwise``'s, and layers with 1 to 3 channels per group stay on the float32 path.  By default such pairs are
    left alone.

    ``transposed=True`` also fuses wrapped ``nn.ConvTranspose2d`` layers (``groups == 1``, dilation 1, ``in_channels % 16 == 0``,
    strides of at most 4, ``ceil(kh / sh) * ceil(kw / sw) * in_channels`` <= 32768, any padding and output padding, the activation
    zero point inside its clamp domain, a per-channel weights quantizer along the output channels, axis 1) into a
    QuantizedConvTranspose2d: the learned upsampling of a decoder stage -- one stride-1 correlation per output phase on the codes
    on the integer matrix cores (``mctq_qconv_transposed_i8``), without a zero-stuffed input.  It is independent of
    ``convolutions`` and composes with every other switch.  By default such pairs are left alone.

    ``chain=True``: where one QuantizedLinear feeds the next directly, the float32 tensor between them is never
    materialised -- the first emits the second's activation codes from its epilogue (same codes, bit for bit, as
    quantizing the float32 output).  Modules or hooks that look at that intermediate tensor then see uint8/int8 codes.

    ``pools=True`` also takes (activation holder, ``nn.MaxPool2d``, wrapped convolution the consumer can take under the other
    switches): it becomes (Identity, QuantizedMaxPool2d, consumer), the pool running on the holder's codes
    (``mctq_codes_maxpool_nhwc``; no ``return_indices``, padding at most half the kernel size) and the consumer taking the pooled
    codes; with ``chain=True`` a consumer in front of the triple emits the pool's codes.  Counted as one pair.  The codes are
    monotone in the value, so the pooled codes are bit for bit the codes of the float32 pool of the holder's output, and the model
    rewritten with ``pools=True`` returns, bit for bit, what the same rewrite without it returns wherever the float32 products of
    the layers behind the pools are exact; otherwise it differs by the accumulation rounding of those products, like every pair
    that becomes a consumer.

    ``avg_pools=True`` also takes (holder A, average pool, holder B, wrapped convolution the consumer can take) and (holder A,
    global average pool, holder B, ``nn.Flatten()``, wrapped ``nn.Linear``): they become (Identity, QuantizedAvgPool2d, Identity,
    [Identity,] consumer), the pool and B running as one launch on A's codes (``mctq_codes_avgpool_nhwc``) and the consumer
    taking B's codes.  The pool is an ``nn.AvgPool2d`` (padding at most half the kernel size) or an ``nn.AdaptiveAvgPool2d`` of
    output size 1; the flatten form needs the global pool.  With ``chain=True`` a consumer in front emits A's codes.  Counted
    as one pair.  Where A's scale and every window's divisor are powers of two the codes are bit for bit those of the float32
    chain, elsewhere the exact mean rounded twice (``QuantizedAvgPool2d``).

    ``upsamples=True`` also takes (holder A, ``nn.Upsample`` / ``nn.UpsamplingNearest2d`` in a nearest mode, holder B, wrapped
    convolution the consumer can take) and the same run without B: they become (Identity, QuantizedUpsample, [Identity,] consumer),
    the upsample and B running as one launch on A's codes (``mctq_codes_upsample_nhwc``) and the consumer taking B's codes (A's
    without a B).  With ``chain=True`` a consumer in front emits A's codes.  Counted as one pair.  Nearest interpolation only moves
    data, so the codes are bit for bit those of the float32 chain (``QuantizedUpsample``).

    ``any_channels=True`` (composes with every other switch) also takes the pairs whose K is no multiple of 16: a wrapped
    ``nn.Linear`` or pointwise convolution of any ``in_features`` / ``in_channels`` <= 32768 -- bottleneck widths of 24, 40, 72, SE
    squeeze widths -- and, with ``convolutions=True``, a k x k convolution of any ``in_channels`` (a CNN's stem).  Such a consumer
    keeps its weight rows padded with the code 0 to ``Kp = 16 * ceil(K / 16)`` columns and re-pitches its activation codes to rows
    of ``Kp`` columns whose tail holds the zero-point code (``mctq_codes_im2col_pad_nhwc``: one more launch per Linear or pointwise
    layer; the patch matrix of a k x k convolution is gathered at that pitch in the first place), so the product is exactly the
    product over K columns, weight zero points included.  It needs the activation zero point inside its clamp domain; pairs
    without are left alone.  Layers with K % 16 == 0 become the consumers they become without the switch; depthwise convolutions
    and the pools, concatenations, multiplies and upsamples on codes keep their own conditions.  By default such pairs are left
    alone: at the launch floor the re-pitch launch of a small pointwise layer can cost what the rewrite saves.

    ``activation_tables=True`` (composes with every other switch) also takes (holder A, one elementwise activation module
    ``QuantizedActivationTable.eligible`` accepts -- ``nn.Sigmoid``, ``SiLU``, ``GELU``, ``Tanh``, ``LeakyReLU``, ... -- holder B, wrapped layer
    the consumer can take): it becomes (Identity, QuantizedActivationTable, Identity, consumer), the activation and B running as one
    launch on A's codes (``mctq_codes_table``: B's code of ``f`` as a 256-entry byte table, built by the replaced call on A's 256
    values) and the consumer taking B's codes.  With ``chain=True`` a consumer in front emits A's codes.  Counted as one pair.  The
    table is the definition: bit for bit the float32 chain on the GPU, within one code next to a rounding tie on the CPU
    (``QuantizedActivationTable``)."""
    replaced = 0
    for seq in [m for m in model.modules() if isinstance(m, nn.Sequential)]:
        for i in range(len(seq) - 3 if avg_pools else 0):
            holder, pool, second = seq[i], seq[i + 1], seq[i + 2]
            if not _plain_holder(holder) or not _plain_holder(second) or isinstance(pool, str) or not QuantizedAvgPool2d.eligible(pool):
                continue
            flat = type(seq[i + 3]) is nn.Flatten and seq[i + 3].start_dim == 1 and seq[i + 3].end_dim == -1
            if flat and (type(pool) is nn.AvgPool2d or i + 4 >= len(seq)):
                continue
            wrapper = seq[i + 4] if flat else seq[i + 3]
            if not isinstance(wrapper, PytorchQuantizationWrapper):
                continue
            fused = _consumer_for(wrapper, second.activation_holder_quantizer, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)
            if fused is None or (type(fused) is QuantizedLinear) != flat:
                continue
            try:
                qpool = QuantizedAvgPool2d(pool, holder.activation_holder_quantizer, second.activation_holder_quantizer, flatten=flat)
            except (TypeError, ValueError, NotImplementedError):
                continue
            seq[i], seq[i + 1], seq[i + 2] = _FusedAway(), qpool, _FusedAway()
            if flat:
                seq[i + 3] = _FusedAway()
            seq[i + 4 if flat else i + 3] = fused
            replaced += 1
        for i in range(len(seq) - 2 if upsamples else 0):
            holder, up = seq[i], seq[i + 1]
            second = seq[i + 2] if _plain_holder(seq[i + 2]) and i + 3 < len(seq) else None
            wrapper = seq[i + 2] if second is None else seq[i + 3]
            if not _plain_holder(holder) or not QuantizedUpsample.eligible(up) or not isinstance(wrapper, PytorchQuantizationWrapper):
                continue
            reads_as = (holder if second is None else second).activation_holder_quantizer
            fused = _consumer_for(wrapper, reads_as, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)
            if fused is None or type(fused) is QuantizedLinear:
                continue
            try:
                qup = QuantizedUpsample(up, holder.activation_holder_quantizer, None if second is None else reads_as)
            except (TypeError, ValueError, NotImplementedError):
                continue
            seq[i], seq[i + 1] = _FusedAway(), qup
            if second is not None:
                seq[i + 2] = _FusedAway()
            seq[i + 2 if second is None else i + 3] = fused
            replaced += 1
        for i in range(len(seq) - 3 if activation_tables else 0):
            holder, fn, second, wrapper = seq[i], seq[i + 1], seq[i + 2], seq[i + 3]
            if not _plain_holder(holder) or not _plain_holder(second) or not QuantizedActivationTable.eligible(fn) \
                    or not isinstance(wrapper, PytorchQuantizationWrapper):
                continue
            fused = _consumer_for(wrapper, second.activation_holder_quantizer, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)
            if fused is None:
                continue
            try:
                table = QuantizedActivationTable(fn, holder.activation_holder_quantizer, second.activation_holder_quantizer)
            except (TypeError, ValueError, NotImplementedError):
                continue
            seq[i], seq[i + 1], seq[i + 2], seq[i + 3] = _FusedAway(), table, _FusedAway(), fused
            replaced += 1
        for i in range(len(seq) - 2 if pools else 0):
            holder, pool, wrapper = seq[i], seq[i + 1], seq[i + 2]
            if not _plain_holder(holder) or not QuantizedMaxPool2d.eligible(pool) or not isinstance(wrapper, PytorchQuantizationWrapper):
                continue
            fused = _consumer_for(wrapper, holder.activation_holder_quantizer, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)
            if fused is None or type(fused) is QuantizedLinear:
                continue
            try:
                qpool = QuantizedMaxPool2d(pool, holder.activation_holder_quantizer)
            except (TypeError, ValueError, NotImplementedError):
                continue
            seq[i], seq[i + 1], seq[i + 2] = _FusedAway(), qpool, fused
            replaced += 1
        for i in range(len(seq) - 1):
            holder, wrapper = seq[i], seq[i + 1]
            if not _plain_holder(holder) or not isinstance(wrapper, PytorchQuantizationWrapper):
                continue
            fused = _consumer_for(wrapper, holder.activation_holder_quantizer, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)
            if fused is None:
                continue
            seq[i] = _FusedAway()
            seq[i + 1] = fused
            replaced += 1
        if chain:
            for i in range(len(seq) - 2):
                first, gap, second = seq[i], seq[i + 1], seq[i + 2]
                if isinstance(first, IntegerConsumer) and isinstance(gap, _FusedAway) and isinstance(second, _CODE_READERS):
                    first.emit_codes_for = second.activation_code_params()
    return replaced


def fuse_linear_consumers_fx(model: nn.Module, chain: bool = False, uniform_weights: bool = False,
                             convolutions: bool = False, depthwise: bool = False, shared_holders: bool = False,
                             stay_on_codes: bool = False, pools: bool = False, fused_residuals: bool = False,
                             concats: bool = False, avg_pools: bool = False, muls: bool = False,
                             hard_activations: bool = False, upsamples: bool = False, any_channels: bool = False,
                             activation_tables: bool = False, grouped: bool = False, transposed: bool = False,
                             matmuls: bool = False):
    """The same rewrite on an arbitrary module graph (MCT-exported models are not ``nn.Sequential``): traces ``model``
    with torch.fx keeping wrappers and holders as leaves, and wherever an activation holder's ONLY consumer is a
    wrapped ``nn.Linear`` the integer consumer can take (symmetric, power-of-two or LUT weights, and with
    ``uniform_weights=True`` uniform weights, as for ``fuse_linear_consumers``), replaces the pair by one
    ``QuantizedLinear`` node; wrapped pointwise convolutions likewise, and with ``convolutions=True`` the other
    convolutions a QuantizedConv2d can take, with ``depthwise=True`` the depthwise convolutions a QuantizedDepthwiseConv2d
    can take, and with ``grouped=True`` the other grouped convolutions a QuantizedGroupedConv2d can take (other grouped
    convolutions are always left alone unless ``grouped=True``; the switch needs no other and composes with all of them: such a
    consumer reads and emits codes like the other convolution consumers, takes folded clamps, and takes no residual and no
    Hardswish / Hardsigmoid in its epilogue), and with ``transposed=True`` the transposed convolutions a QuantizedConvTranspose2d
    can take (always left alone otherwise; independent of ``convolutions``, composes with every switch, reads and emits codes and
    folded clamps like the grouped consumer; a call of the module with an ``output_size`` argument is left alone).
    Returns ``(graph_module, wrapped_layers_replaced)``.  Holders with several consumers (residual branches) stay, unless
    ``shared_holders=True``:

    every plain holder then counts whose users include wrapped layers the consumer can take (under the other switches as
    given) that are fed by the holder alone.  A ``ReLU`` in front of the holder (``nn.ReLU``, ``F.relu``, ``torch.relu``,
    ``Tensor.relu``) that feeds nothing else is absorbed, and behind it an add of two tensors (``+``, ``+=``, ``torch.add``,
    ``Tensor.add`` without ``alpha``) that feeds nothing else.  A holder with one user and nothing to absorb is the pair
    above; every other one becomes a QuantizedJoin node -- one launch for add, ReLU, the holder and the codes -- whose
    float32 output replaces the holder for the users that stay (it is not computed when there are none) and whose codes feed
    the consumers that replace the wrapped layers.  With residual networks this is what lets the first convolution of a block
    and its downsample branch run on codes.  Nothing chains across a join.

    ``stay_on_codes=True`` (needs ``shared_holders=True``; ValueError otherwise) keeps the activations between those layers on
    codes, in two exact steps.  A ReLU, ReLU6 or Hardtanh between a consumer and a holder that only consumers read is folded into
    the clamp of the codes the consumer then emits itself (``folded_clamp``; the activation and the holder or its ReLU-only
    join leave the graph).  And a residual join whose identity operand is another join's float32 output reads that join's codes
    instead (``mctq_fq_join_rc_f32``), so that the float32 tensor between two blocks is neither written nor read.  The result
    is bit for bit that of ``shared_holders=True`` alone, except that a NaN in a consumer's output (only from a NaN scale or
    bias) codes to the folded clamp's lower end, not the domain's.

    ``pools=True`` (needs no other switch) keeps a max pool between a holder and wrapped layers on codes.  The candidate is a
    plain holder one of whose users is a max pool -- an ``nn.MaxPool2d`` module or ``F.max_pool2d`` with constant arguments, no
    ``return_indices``, padding at most half the kernel size -- every user of which is a wrapped convolution the consumer can
    take under the other switches, fed by the pool alone.  The pool becomes a QuantizedMaxPool2d on the holder's codes
    (``mctq_codes_maxpool_nhwc``) and those layers consumers of its output.  A holder whose only user is the pool, with nothing
    in front to absorb, leaves the graph: the pool module quantizes.  With ``shared_holders=True`` a ReLU and / or an add in
    front is absorbed into a QuantizedJoin as above, which writes no float32 output when the pool was the holder's only user;
    the holder's other users keep what they get without ``pools``.  Without ``shared_holders`` a holder with other users
    besides the pool is left alone, and so is every pool with another kind of user (an identity add: a residual join does
    not read pooled codes).  With ``stay_on_codes=True`` a QuantizedMaxPool2d counts as a reader of the holder's codes, so that
    consumer -> ReLU / ReLU6 / Hardtanh -> holder -> pool -> consumers runs codes to codes (the VGG pattern).  The codes are
    monotone in the value and a padded tap is ignored, so the pooled codes are bit for bit the codes of the float32 pool of the
    holder's output, and the model rewritten with ``pools=True`` returns, bit for bit, what the same rewrite without it returns
    wherever the float32 products of the layers behind the pools are exact; otherwise it differs by the accumulation rounding of
    those products, like every wrapped layer that becomes a consumer.

    ``fused_residuals=True`` (needs ``stay_on_codes=True``; ValueError otherwise -- without it every residual join also writes
    float32 for the next identity add) folds the residual joins that write codes only into the product in front of them, after
    the two steps of ``stay_on_codes``.  Such a join goes when one of its two operands is the output of a QuantizedLinear,
    QuantizedConv1x1 or QuantizedConv2d with weights without zero points that feeds nothing else, emits nothing yet and is
    evaluated after the other operand: that consumer then takes the other operand -- the codes of the join in front in an
    identity block, the other branch's float32 output in a downsample block -- as its second argument, adds it and applies the
    join's ReLU in its own epilogue and emits the join's codes (``mctq_qlinear_i8_res``; ``emit_residual``, ``emit_relu``).  The
    float32 tensor between the block's last convolution and its join is then neither written nor read, and the join's launch
    goes.  Joins that must write float32, joins without a residual and joins behind a depthwise, uniform-weights or
    non-consumer node stay.  The ReLU stays an operation (it is not folded into the clamp), so the result is bit for bit that
    of the same rewrite without the switch, NaNs included.  Large whole-tile products with a residual run on the tiled kernels,
    not the faster register-pinned ones (as with weight zero points): the rewrite has no cost model and fuses them all the same.

    ``concats=True`` (needs no other switch) keeps a channel concatenation between holders on codes: the Inception block, the
    Fire module, a decoder stage with skip connections.  The candidate is a plain holder whose one argument is ``torch.cat`` /
    ``torch.concat`` / ``torch.concatenate`` of a list or tuple of 2 to 8 tensors along the constant dimension 1 (no ``out=``)
    that feeds nothing else, every operand the output of a plain holder, and every user of which is a wrapped layer the consumer
    can take under the other switches, fed by it alone, or with ``pools=True`` a max pool that can run on codes.  The
    concatenation and the holder become one QuantizedConcat node (``mctq_codes_concat_nhwc``: the operands' codes requantized
    into the holder's form, 1 byte read and 1 written per element) and the users consumers and pools of its codes.  An operand
    holder whose only user was the concatenation leaves the graph, the QuantizedConcat quantizes its input; one with other
    users (a skip connection) stays, and the QuantizedConcat quantizes its float32 output -- or, where ``shared_holders=True``
    turns it into a join, that join's float32 output.  Everything else is left alone: a float32 user of the holder, an operand
    that is no holder's output, a clamp between the concatenation and the holder, another dimension, more than 8 operands.
    With ``stay_on_codes=True`` a consumer in front of an operand -- through at most one ReLU / ReLU6 / Hardtanh -- emits that
    operand's codes itself, so that conv -> ReLU -> holder -> cat -> holder -> conv runs codes to codes.  A holder's float32
    output is ``float(code - zp) * scale`` bit for bit and ``torch.cat`` only moves data, so the codes are bit for bit those of the
    holder behind the float32 concatenation, for any channel counts (counts that are no multiple of 16 take torch ops), and
    the model rewritten with ``concats=True`` returns, bit for bit, what the same rewrite without it returns wherever the
    float32 products of the layers behind the concatenation are exact; otherwise it differs by the accumulation rounding of
    those products, like every wrapped layer that becomes a consumer.

    ``avg_pools=True`` (needs no other switch) keeps an average pool between two holders on codes: classifier heads, SE squeezes,
    Inception's pooling branch.  The candidate is a plain holder A one of whose users is an average pool of its output -- a call
    of an ``nn.AvgPool2d`` (padding at most half the kernel size) or ``nn.AdaptiveAvgPool2d`` of output size 1, ``F.avg_pool2d``
    with constant arguments, ``F.adaptive_avg_pool2d(x, 1 | (1, 1))``, or ``x.mean(...)`` / ``torch.mean(x, ...)`` over the constant
    dims (2, 3) or (-2, -1) in either order with a constant ``keepdim`` (``keepdim=False`` is a global pool that is already flat).
    Through at most one flatten -- ``nn.Flatten()`` with the defaults, ``torch.flatten(x, 1)`` or ``x.flatten(1)``, accepted only
    behind a global pool, where H = W = 1 is known without shapes -- the pool's one user is a plain holder B, and every user of B
    is a wrapped layer the consumer can take under the other switches, fed by B alone (never a QuantizedLinear on an unflattened
    4-D tensor), or such a flatten all of whose users are wrapped ``nn.Linear`` layers the consumer can take.  The pool, B and
    the flatten(s) become one QuantizedAvgPool2d node (``mctq_codes_avgpool_nhwc``) and the layers behind consumers of its codes,
    counted in the returned total.  Holder A is treated as for ``pools``: if the pool is its only user and nothing in front is to
    be absorbed it leaves the graph and the pool module quantizes; with ``shared_holders=True`` a ReLU and / or an add in front
    is absorbed into a QuantizedJoin, which writes no float32 when the pool was A's only user, and A's other users (an SE
    block's multiply) keep what they get today (``muls=True``, below, puts that multiply on codes); without ``shared_holders`` a holder A with other users is left alone.  With
    ``stay_on_codes=True`` the pool counts as a reader of A's codes, so that consumer -> ReLU6 -> A -> pool -> B -> Linear runs
    codes to codes, and with ``fused_residuals=True`` ResNet's last join folds into the last convolution's epilogue.  Left alone:
    a float32 user of B or of the pool; no holder B (``workloads.wrapped_resnet50``'s head as it stands: its Linear reads an
    unquantized mean; ``pooled_holder=True`` builds the exported form); an activation between pool and B; an adaptive output
    size other than 1; ``view`` / ``reshape`` forms of flatten; ``AvgPool1d/3d``; users of B that are partly flattened and partly
    4-D.  Where A's scale and every window's divisor are powers of two the codes are bit for bit those B gives the float32
    pool, and the model returns what the same rewrite without the switch returns wherever the products behind are exact;
    elsewhere the codes are the exact mean rounded twice, within one code of a float32 chain next to a rounding tie.

    ``muls=True`` (needs no other switch) keeps an elementwise multiply between holders on codes: the multiply of a
    squeeze-and-excitation block (RegNetY, MnasNet, MobileNetV3, EfficientNet), a gated layer.  The candidate is a plain holder M
    whose one argument is a multiply of two graph nodes -- ``*``, ``torch.mul`` / ``torch.multiply``, ``Tensor.mul`` /
    ``Tensor.multiply``, ``*=`` only where nobody else reads its first operand; no scalar operand, no ``out=`` -- that feeds nothing
    else, each operand the output of a plain holder, and every user of which is a wrapped layer the consumer can take under the
    other switches, fed by M alone, or with ``pools=True`` a max pool that can run on codes.  The multiply and M become one
    QuantizedMul node (``mctq_codes_mul_nhwc``: 1 byte read and 1 written per element of the large tensor) and the users
    consumers and pools of its codes, counted in the returned total.  An operand holder that the multiply alone reads leaves the
    graph and the QuantizedMul quantizes its input -- a ``[B, C, 1, 1]`` gate in float32 goes to the kernel as it is; one with
    other users stays.  With ``shared_holders=True`` a holder that becomes a QuantizedJoin hands the QuantizedMul its codes, at
    whichever operand position it occupies, and writes no float32 when no float32 user remains: with ``avg_pools=True`` the
    holder in front of an SE block, read by the squeeze and by the multiply, never writes its float32 tensor.  With
    ``stay_on_codes=True`` a QuantizedMul counts as a reader of codes, directly or behind such a join next to other readers, so
    that conv -> ReLU -> A -> {squeeze, multiply} -> M -> conv runs codes to codes; the same tensor at both operands (``x * x``)
    is left to the module's float32 quantize path.  Left alone: a float32 user of M (SE-ResNet's identity add behind M: a
    residual join does not read a QuantizedMul's codes yet); an operand that is no holder's output (``x * sigmoid(y)`` without
    a holder); anything between the multiply and M; ``div``; scalar operands; folding a sigmoid in front of the gate's holder
    into the product in front of it (a hardsigmoid: ``hard_activations=True``, below).  A holder's float32 output is ``float(code - zp) * scale`` bit for bit and
    ``torch.mul`` is one IEEE float32 multiplication, so the codes are bit for bit those M gives the float32 product, for any
    shapes ``torch.mul`` broadcasts (the kernel takes equal shapes and ``[B, C, H, W]`` with ``[B, C, 1, 1]`` where C % 16 == 0,
    everything else torch ops), and the model rewritten with ``muls=True`` returns, bit for bit, what the same rewrite without
    it returns wherever the float32 products of the layers behind M are exact; otherwise it differs by the accumulation
    rounding of those products, like every wrapped layer that becomes a consumer.

    ``hard_activations=True`` (needs ``stay_on_codes=True``; ValueError otherwise) keeps the activations on codes across a
    Hardswish or Hardsigmoid: MobileNetV3's ``conv -> Hardswish -> holder -> conv`` layers, depthwise ones included, and the
    ``fc2 -> Hardsigmoid -> G -> multiply`` gate of its SE blocks.  Where ``stay_on_codes`` accepts one ReLU / ReLU6 / Hardtanh
    between a consumer and the readers of a holder's codes, one ``nn.Hardswish`` / ``F.hardswish`` / ``nn.Hardsigmoid`` /
    ``F.hardsigmoid`` of one tensor that feeds nothing else is accepted too (in-place forms only where nobody else reads the
    input), with every kind of reader: consumers and pools, a residual-free join that writes no float32, and with ``concats`` /
    ``muls`` an operand of a QuantizedConcat / QuantizedMul -- the SE gate then reaches ``mctq_codes_mul_nhwc`` as codes instead of
    float32.  These two activations are no clamps of the codes: the consumer applies them to its float32 value in its own
    epilogue (``emit_act``; ``mctq_qlinear_i8_act``, ``mctq_qconv_dw_i8_act``) and emits the holder's codes, and the activation and
    the holder or join leave the graph -- per folded activation ATen's launch, the quantize launch and two float32 tensors.  Left
    alone: producers the entry points do not take (a product with uniform, 4-bit or LUT weights or one that already takes a
    residual; the depthwise convolution takes every weight kind); a holder with a float32 reader; an activation whose input
    has other users; two activations in a row (a join that absorbed a ReLU behind the Hardswish); sigmoid, SiLU, GELU, tanh,
    which no epilogue can reproduce bit for bit (between two holders they run as a byte table: ``activation_tables=True``, below).  The kernels evaluate the float32 expression of ATen's GPU kernels,
    ``x * min(max(x + 3, 0), 6) * (1.0f / 6.0f)``, equal to them for every float32 bit pattern, on the same float32 value the
    consumer would have written, so on the GPU the result is bit for bit that of the same rewrite without the switch, NaNs
    and infinities included.  On the CPU the consumers apply ``F.hardswish`` / ``F.hardsigmoid`` (ATen's CPU kernels divide by 6:
    another rounding for a quarter of the inputs), so there too the result equals the same rewrite without the switch, while
    CPU and GPU may differ by one code at a rounding tie, with and without the switch.  Large whole-tile products with an
    activation run on the tiled kernels, not the faster register-pinned ones (as with a residual): the rewrite has no cost
    model and folds them all the same (measured on 4096 x 4096 x 256: the tiled launch with the activation 31 us, the
    register-pinned launch 22 us, the three launches it replaces 54 us together; tools/hard_act_probe.py,
    profiles/EXPERIMENTS.md).

    ``upsamples=True`` (needs no other switch) keeps a nearest upsample behind a holder on codes: a U-Net stage, a YOLO / PANet
    neck, a segmentation head.  The candidate is a plain holder A one of whose users is a nearest upsample of its output -- a call
    of an ``nn.Upsample`` of mode "nearest" or "nearest-exact" (``size`` or ``scale_factor``, any ``recompute_scale_factor``) or of
    an ``nn.UpsamplingNearest2d``, or ``F.interpolate`` with constant arguments in one of those modes, ``antialias=False`` and
    ``align_corners=None`` -- every reader of which agrees on one code form F.  (a) The upsample's one user is a plain holder B
    (F is B's form) and every user of B is a wrapped layer the consumer can take under the other switches, fed by B alone (never a
    QuantizedLinear), or with ``pools=True`` a max pool that can run on codes: the upsample and B become one QuantizedUpsample
    node (``mctq_codes_upsample_nhwc``: A's codes gathered through the index map and requantized into B's form, 1 byte read and 1
    written per output element) named ``<B's name>_upsample``, and the users consumers and pools of its codes, counted in the
    returned total.  (b) Without a B the upsample's users are such layers and pools directly; F is A's form and the node a pure
    copy of codes.  (c) With ``concats=True`` / ``muls=True`` a reader may be a QuantizedConcat / QuantizedMul that reads the
    upsample's float32 output, or B's, at exactly one operand -- what those passes, which run first, leave where they absorbed
    B: F is then ``operand_code_params(i)`` and that argument becomes the node's codes, so that A -> upsample -> B ->
    cat([B, S]) -> C -> conv, the decoder stage, runs holder to holder on codes.  Holder A is treated as for ``pools``: read by
    the upsample alone with nothing in front to absorb it leaves the graph and the module quantizes, at the low resolution;
    with ``shared_holders=True`` a join in A's place hands the node its codes and writes no float32 when no float32 user
    remains; with ``stay_on_codes=True`` the node is a reader of A's codes, so that conv -> ReLU -> A -> upsample -> B -> conv
    runs codes to codes with the ReLU folded into the emitted clamp.  The index maps are read from the replaced call itself, per
    input shape (``QuantizedUpsample``): a hipGraph capture needs one warm-up forward first, as ``capture_forward`` makes.  Left
    alone: a float32 user of the upsample or of B (FPN's ``lateral + upsample(top)``: a residual join does not read a
    QuantizedUpsample's codes yet); the modes bilinear, bicubic and area (ATen's interpolation expression is not reproduced bit
    for bit); ``antialias=True``; ``align_corners`` given; a ``size`` that is no constant (``size=skip.shape[2:]``);
    ``nn.PixelShuffle`` (``nn.ConvTranspose2d`` is ``transposed=True``'s); 3-D and 5-D inputs (a ``size`` / ``scale_factor`` of one or three entries);
    an activation between the upsample and B.  A holder's float32 output is ``float(code - zp) * scale`` bit for bit and nearest
    interpolation only moves data, so the codes are bit for bit those B gives the float32 upsample, for any geometry and channel
    count (counts that are no multiple of 16 take torch ops), and the model rewritten with ``upsamples=True`` returns, bit for
    bit, what the same rewrite without it returns wherever the float32 products of the layers behind are exact; otherwise it
    differs by the accumulation rounding of those products, like every wrapped layer that becomes a consumer.

    ``any_channels=True`` (needs no other switch and composes with all of them) lifts the ``K % 16 == 0`` condition of "a wrapped
    layer the consumer can take" everywhere above, as for ``fuse_linear_consumers``: wrapped ``nn.Linear`` layers and pointwise
    convolutions of any K <= 32768, and with ``convolutions=True`` k x k convolutions of any ``in_channels`` (the stem of a CNN behind
    an input holder, the expand layer behind a 24-channel bottleneck, an SE block's ``fc2``).  Such a consumer pads its weight rows
    with the code 0 and re-pitches its activation codes to ``Kp = 16 * ceil(K / 16)`` columns (``mctq_codes_im2col_pad_nhwc``), which
    leaves the integer sum as it is; everything a consumer can emit -- codes, folded clamps, activations, residuals -- works
    unchanged.  It needs the activation zero point inside its clamp domain.  Depthwise convolutions keep ``in_channels % 16 == 0``,
    and the pools, concatenations, multiplies and upsamples on codes keep their torch routes for such channel counts.

    ``activation_tables=True`` (needs no other switch and composes with all of them) keeps the elementwise activations between two
    holders on codes, the smooth ones included: EfficientNet- and YOLO-style conv -> holder -> SiLU -> holder -> conv, GELU blocks,
    sigmoid gates, LeakyReLU necks.  The candidate is a plain holder A one of whose users starts a run of 1 to 4 eligible nodes, each
    with one tensor operand and (but for the last) the next as its one user, behind which stands a plain holder B.  Eligible
    (``QuantizedActivationTable.eligible``) are calls of modules of exactly the types ``nn.Sigmoid``, ``Tanh``, ``SiLU``, ``GELU`` (both
    approximations), ``Mish``, ``Softplus``, ``ELU``, ``CELU``, ``SELU``, ``LeakyReLU``, ``Hardswish``, ``Hardsigmoid``, ``Hardtanh``, ``ReLU``,
    ``ReLU6``, ``LogSigmoid``, ``Softsign``, ``Tanhshrink``, and the functional and method spellings with constant arguments, which are
    mapped onto such a module: ``torch.sigmoid``, ``torch.tanh``, ``torch.relu``, the ``F.*`` counterparts of the types, ``x.sigmoid()``,
    ``x.tanh()``, ``x.relu()``; in-place forms only where nobody else reads the input.  B's users must all read codes in B's form: wrapped
    layers the consumer can take under the other switches, fed by B alone; with ``pools=True`` max pools that can run on codes; or
    the QuantizedConcat / QuantizedMul operand that absorbed B (``concats`` / ``muls``, which run first), which then supplies the
    form.  The run and B become one QuantizedActivationTable node named ``<B's name>_table`` (``mctq_codes_table``: ``out[i] =
    table[in[i]]``, 1 byte read and 1 written per element, any element and channel count) whose ``fn`` is the run in order, and the
    users consumers and pools of its codes, counted in the returned total.  Holder A is treated as for ``pools``: read by the run alone
    with nothing in front to absorb it leaves the graph and the module quantizes its input; with ``shared_holders=True`` a join in
    A's place hands the node its codes; with ``stay_on_codes=True`` the node is a reader of A's codes, so that conv -> [ReLU / ReLU6 /
    Hardtanh] -> A -> f -> B -> conv runs codes to codes.  Tables are built on first use per device, with a few tiny launches and no
    host read: a hipGraph capture needs one warm-up forward first, as ``capture_forward`` makes.  Left alone: no B (except behind such
    an operand); a float32 user of ``f`` or of B; anything not eligible in the run -- learnable or per-channel state (``PReLU``),
    random or mode-dependent (``RReLU``, dropout), across elements (softmax, GLU) -- or more than four nodes; a node with two tensor
    operands (``x * sigmoid(x)`` written out); a scalar operand; a quantizer wider than 8 bits.  The exactness contract: the table is
    the definition -- B's code of ``f`` evaluated on A's [256] values by the replaced call on the tensor's device.  On the GPU ATen's
    elementwise kernels apply one scalar functor per element whatever its position, shape or layout, so the node's codes are bit for
    bit those of the float32 chain A -> f -> B on that GPU and the model returns what the same rewrite without the switch returns
    (tests/test_gpu_table_consumer.py checks every accepted function with strict equality; one that failed would leave the list).
    On the CPU ATen's vector body and scalar tail give different last bits for sigmoid, SiLU, softplus, ELU, Mish, tanh and GELU
    (0.007 - 0.08 % of elements, erf-GELU 2.6 %): there the node equals the chain wherever the chain's float32 value equals the
    table's and can differ by one code next to a rounding tie elsewhere.  Out of scope: looking the table up inside the producing
    consumer's epilogue (``emit_table``, beside ``emit_act``), which would remove the launch.

    ``matmuls=True`` (needs no other switch and composes with all of them; two operands need a graph, so ``fuse_linear_consumers``
    has no such form) keeps the activation x activation products on codes: the ``Q @ K.transpose(-1, -2)`` and ``P @ V`` of an
    attention block as an MCT export of a ViT, DeiT, Swin or BERT decomposes it.  The candidate is a ``torch.matmul`` /
    ``operator.matmul`` (``@``) / ``Tensor.matmul`` / ``torch.bmm`` node of two tensors without keyword arguments, each operand of
    which leads back to a plain holder's output through a layout-only chain: zero or more ``reshape``, ``view``, ``permute``,
    ``transpose``, ``contiguous``, ``flatten``, ``unflatten`` nodes with constant integer arguments and ``operator.getitem`` nodes with
    one constant integer index (``_layout_input``, the one list used on both sides; such nodes only move data, so they commute
    with coding -- which is why a chain node may have other users as well: a fused ``qkv`` tensor is permuted once and indexed
    three times).  The node becomes a QuantizedMatmul (``mctq_qmatmul_i8``) with the two holders' quantizers.  A final
    ``transpose(-1, -2)`` on the second operand -- either order, a positive-index spelling behind a permute, reshape or view that
    tells the rank, or ``.mT`` -- that feeds nothing else is absorbed as ``transposed_b=True`` and not executed.  The operand holders
    are treated as ``concats`` / ``muls`` treat them: one whose every user leads to QuantizedMatmul operands leaves the graph, its
    input runs through the chain and the module quantizes it; one with other users stays and the module quantizes its
    float32 output, the same codes; with ``shared_holders=True`` a holder that became a join hands its codes to the chain.  A
    plain holder directly behind the matmul, which feeds nothing else, is absorbed -- the module emits that holder's codes -- if
    every user of it reads codes, directly or through layout-only chains: a wrapped ``nn.Linear`` the consumer can take under
    the other switches, fed by it alone (it becomes a QuantizedLinear, counted in the returned total), an operand of another
    QuantizedMatmul, and a QuantizedConcat / QuantizedMul that absorbed the holder and reads the node at one operand.
    Otherwise the node returns float32 and the holder stays: the scores' case, whose scale multiply and softmax are float32.
    With ``stay_on_codes=True`` a consumer every user of which leads, through a layout-only chain without a clamp activation, to
    QuantizedMatmul operands of one form emits ``operand_code_params(i)``, and the chain moves int8: ``Linear -> holder -> reshape
    -> permute -> matmul`` and ``matmul -> holder -> permute -> reshape -> Linear`` run codes to codes; Q, K, V and the context
    never exist in float32.  Left alone: ``F.scaled_dot_product_attention`` and ``nn.MultiheadAttention``; the ``* scale`` /
    ``/ sqrt(d)`` and the softmax between the two products; ``einsum``, ``baddbmm``, ``addmm``; an operand that reaches no holder;
    quantizers wider than 8 bits or per-channel; half precision; a producer that writes its codes at the padded pitch directly
    (a K that is no multiple of 16, a ViT's 197 probabilities per row, costs one re-pitch launch per forward, as
    ``any_channels`` does).  The integer sum is exact, so the model returns, bit for bit, what the same rewrite without the switch
    returns wherever the float32 products it replaces (and those of the layers behind an absorbed holder) are exact --
    power-of-two scales, ``255 * 255 * K < 2^24``; otherwise it differs by the accumulation rounding of those float32 products."""
    import torch.fx as fx
    if stay_on_codes and not shared_holders:
        raise ValueError("stay_on_codes=True needs shared_holders=True")
    if fused_residuals and not stay_on_codes:
        raise ValueError("fused_residuals=True needs stay_on_codes=True")
    if hard_activations and not stay_on_codes:
        raise ValueError("hard_activations=True needs stay_on_codes=True")

    class _Tracer(fx.Tracer):
        def is_leaf_module(self, m, qualname):
            return isinstance(m, (PytorchQuantizationWrapper, PytorchActivationQuantizationHolder, IntegerConsumer, _OnCodes)) \
                or super().is_leaf_module(m, qualname)

    graph = _Tracer().trace(model)
    gm = fx.GraphModule(model, graph)
    mods = dict(gm.named_modules())
    replaced = 0
    consumer_for = lambda wrapper, q: _consumer_for(wrapper, q, uniform_weights, convolutions, depthwise, any_channels, grouped, transposed)      # noqa: E731
    # Two whole passes, concatenations first: a concatenation absorbs an operand holder that sits behind a multiply, which the
    # multiply pass then no longer sees.
    if concats:
        replaced = _operator_between_holders(gm, mods, consumer_for, pools, _cat_operands, QuantizedConcat, "_concat")
    if muls:
        replaced += _operator_between_holders(gm, mods, consumer_for, pools, _mul_operands, QuantizedMul, "_mul")
    if matmuls:                                              # (behind the two: it sees the QuantizedConcat / QuantizedMul nodes)
        replaced += _matmuls_on_codes(gm, mods, consumer_for)
    # (an upsample's plan is made where a pool's is, in these two passes: it sees the QuantizedConcat / QuantizedMul nodes above)
    if shared_holders:
        replaced += _join_shared_holders(gm, mods, consumer_for, pools, avg_pools, upsamples, activation_tables)
    if pools or avg_pools or upsamples or activation_tables:
        replaced += _pool_lone_holders(gm, mods, consumer_for, pools, avg_pools, upsamples, activation_tables)
    for src, holder in _holder_calls(gm, mods):              # the pair: a holder whose only user is a wrapped layer
        if len(src.users) != 1:
            continue
        node = next(iter(src.users))
        fused = _wrapped_consumer(node, src, mods, holder.activation_holder_quantizer, consumer_for)
        if fused is None:
            continue
        _install_consumer(gm, mods, node, fused)
        node.args = (src.args[0],)
        gm.graph.erase_node(src)
        replaced += 1
    if chain:
        for node in gm.graph.nodes:
            producer = _module_of(node, mods)
            if isinstance(producer, IntegerConsumer) and len(node.users) == 1:
                user = next(iter(node.users))
                nxt = _module_of(user, mods)
                if isinstance(nxt, _CODE_READERS) and user.args == (node,):
                    producer.emit_codes_for = nxt.activation_code_params()
    if stay_on_codes:
        _identities_as_codes(gm, mods)
        _fold_clamps_into_producers(gm, mods, hard_activations)
    if fused_residuals:
        _fuse_residuals_into_producers(gm, mods)
    gm.graph.lint()
    gm.recompile()
    return gm, replaced
