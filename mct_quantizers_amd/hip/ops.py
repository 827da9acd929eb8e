"""Tensor-level entry points of the hot path.

Each function stands where the reference calls the tensor runtime:

* ``fq_per_tensor``  ~ ``torch.fake_quantize_per_tensor_affine``
  (reference weights_symmetric_inferable_quantizer.py:147, activation_uniform_inferable_quantizer.py:124, ...)
* ``fq_per_channel`` ~ ``torch.fake_quantize_per_channel_affine`` (weights_symmetric_inferable_quantizer.py:139)
* ``lut_per_tensor`` / ``lut_per_channel`` ~ ``lut_quantizer`` (pytorch/quantizer_utils.py:95-139)

Routing:
  * GPU (HIP) float32 / float16 / bfloat16 / float64 tensor -> the gfx950 kernels through the C ABI, on torch's
    current stream.  No fallback: a missing library raises.  Two interchangeable bindings of the SAME extern "C"
    entry points: the compiled one (csrc/binding/mctq_torch.cpp: checks, allocation, stream lookup and launch in
    one CPython call -- small activations are launch-bound) and ctypes (hip/native.py).  Every launch of the ctypes
    binding, here and in consumers.py, is one ``_gpu_call(symbol, tensor, *args)``: it looks the symbol up, makes the
    tensor's device current if it is not, appends torch's current stream of that device (the last argument of every
    launching entry point), and raises in the symbol's name when the library refuses; the callers keep their checks
    and allocations.
  * CPU tensor                -> the very ATen ops the reference runs on a CPU tensor
    (BASELINE config 1, "torch-cpu plumbing"); not a substitute for the GPU path.
  * torch.jit tracing (TorchScript / ONNX export without enable_custom_impl) -> the ATen operators / torch op
    chain the reference itself records there (a raw kernel launch is invisible to the tracer: the graph would
    contain an uninitialised aten::empty_like).
  * fx Proxy / FakeTensor     -> ``torch.ops.mctq_amd.*`` so tracing records one call_function node.
"""
from __future__ import annotations

from typing import Tuple

import math
import os

import torch

from mct_quantizers_amd.hip import native

_LIBNAME = "mctq_amd"


# ------------------------------------------------------------------------------------------
# layout: view a tensor's storage as [outer][channels][inner]
# ------------------------------------------------------------------------------------------

def _is_dense(x: torch.Tensor) -> bool:
    """True if x occupies numel contiguous elements in some dimension order (no gaps, no overlap)."""
    if x.is_contiguous():
        return True
    dims = [(st, sz) for st, sz in zip(x.stride(), x.shape) if sz != 1]
    dims.sort()
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _dense_input(x: torch.Tensor) -> torch.Tensor:
    """A non-overlapping dense tensor the kernels can walk in storage order.  Gapped / overlapping views are compacted
    the way ATen lays out the OUTPUT of its fake-quant operators for them -- ``empty_like(x)`` with the preserve-format
    rule: dimensions keep their stride order (a gapped channels-last view stays channels-last) -- so the result, which
    takes this tensor's strides, has the strides the reference's result has."""
    return x if _is_dense(x) else torch.empty_like(x).copy_(x)


def _channel_view(x: torch.Tensor, axis: int) -> Tuple[int, int, int]:
    """(outer, channels, inner) of a dense tensor in storage order for logical dimension ``axis``."""
    n = x.numel()
    c = x.shape[axis]
    if x.is_contiguous():
        inner = 1
        for s in x.shape[axis + 1:]:
            inner *= s
    else:
        inner = x.stride(axis) if c > 1 else 1
    outer = n // (c * inner) if c * inner else 0
    return outer, c, inner


# What ONE launch of the non-affine per-channel entry points takes when the rows are short (include/mctq_hip.h, "Size limit"):
# larger tensors are cut into row blocks below it, one launch each.  A module constant so that tests can lower it.
_SPLIT_ELEMS = (1 << 32) - 8192


def _split_rows(x: torch.Tensor, axis: int, params, out_dtype, call, limit: int = None) -> torch.Tensor:
    """``call`` applied block by block to a DENSE tensor too large for one launch.  x is walked in storage order as
    [outer][channels][inner]; a block is a run of whole outer slices, or -- when one slice alone exceeds ``limit`` elements -- a
    run of whole channel rows of one slice, with the per-channel ``params`` (1-D tensors of ``channels`` entries) sliced
    alike.  ``call(x_block [k, ch, inner] contiguous, params_block, 1)`` returns that block's result (same dense order).
    Returns the result with x's sizes and strides."""
    limit = _SPLIT_ELEMS if limit is None else limit
    n = x.numel()
    outer, c, inner = _channel_view(x, axis)
    flat = torch.as_strided(x, (n,), (1,), x.storage_offset())
    y = torch.empty(n, dtype=out_dtype, device=x.device)
    per_slice = c * inner
    if per_slice <= limit:
        k = max(1, limit // per_slice)
        for o0 in range(0, outer, k):
            o1 = min(outer, o0 + k)
            piece = flat[o0 * per_slice:o1 * per_slice].view(o1 - o0, c, inner)
            y[o0 * per_slice:o1 * per_slice] = call(piece, tuple(params), 1).reshape(-1)
    else:
        if inner > limit:
            raise NotImplementedError(f"a single channel row of {inner} elements exceeds what one launch takes ({limit})")
        rows = max(1, limit // inner)
        for o in range(outer):
            for ch0 in range(0, c, rows):
                ch1 = min(c, ch0 + rows)
                a, b = (o * c + ch0) * inner, (o * c + ch1) * inner
                piece = flat[a:b].view(1, ch1 - ch0, inner)
                y[a:b] = call(piece, tuple(p[ch0:ch1] for p in params), 1).reshape(-1)
    return torch.as_strided(y, x.shape, x.stride())


_raw_stream = torch._C._cuda_getCurrentRawStream      # (device index) -> hipStream_t as int
_current_device = torch._C._cuda_getDevice


def _gpu_call(name: str, on: torch.Tensor, *args) -> None:
    """THE launch of the ctypes route: the C-ABI entry point ``name(*args, stream)`` on torch's current stream of ``on``'s
    device, that device made current for the call when it is not already (and the previous one restored).  With
    MCTQ_ROCTX=1 the call is wrapped in a roctx range named after the symbol; a refusal raises in the symbol's name."""
    fn = getattr(native.load(), name)
    idx = on.get_device()
    prev = _current_device()
    if prev != idx:
        torch.cuda.set_device(idx)
    try:
        if native.TRACE:
            with native.trace_range(name):
                rc = fn(*args, _raw_stream(idx))
        else:
            rc = fn(*args, _raw_stream(idx))
    finally:
        if prev != idx:
            torch.cuda.set_device(prev)
    if rc:
        native.check(rc, name)


_DTYPES = {torch.float32: native.DT_F32, torch.float16: native.DT_F16, torch.bfloat16: native.DT_BF16,
           torch.float64: native.DT_F64}


def _dtype_code(x: torch.Tensor, what: str) -> int:
    code = _DTYPES.get(x.dtype)
    if code is None:
        raise NotImplementedError(f"{what}: the gfx950 kernels take float32, float16, bfloat16 or float64 tensors, "
                                  f"got {x.dtype}")
    return code


def _param_on(x: torch.Tensor, t: torch.Tensor, name: str, dtype) -> torch.Tensor:
    """A parameter vector as the kernels need it: right dtype, contiguous, ON x's DEVICE (the kernel would otherwise
    dereference another GPU's pointer; ATen raises a device-mismatch error here as well)."""
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device != x.device:
        raise RuntimeError(f"Expected all tensors to be on the same device, but {name} is on {t.device} and the "
                           f"input on {x.device}")
    return t if t.is_contiguous() else t.contiguous()


# compiled binding (None: ctypes only).  Resolved at the first GPU call.
_FAST = None
_FAST_READY = False


def _fast_mod():
    global _FAST, _FAST_READY
    if not _FAST_READY:
        _FAST = native.fast() if torch.cuda.is_available() else None
        _FAST_READY = True
    return _FAST


# ------------------------------------------------------------------------------------------
# GPU launches
# ------------------------------------------------------------------------------------------

def _check_aten_range(zero_point: int, qmin: int, qmax: int):
    """ATen's check of a per-tensor zero point against the clamp domain, with its messages."""
    if not qmin <= zero_point <= qmax:
        if qmin > qmax:
            raise RuntimeError("`quant_min` should be less than or         equal to `quant_max`.")
        raise RuntimeError("`zero_point` must be between `quant_min` and `quant_max`.")


def _hip_fq_per_tensor(x, scale: float, zero_point: int, qmin: int, qmax: int):
    # hot for small activations (launch-bound): keep the Python between the caller and the launch short
    dt = _DTYPES.get(x.dtype)
    if dt is None:
        _dtype_code(x, "fq_per_tensor")
    if not qmin <= zero_point <= qmax:
        _check_aten_range(zero_point, qmin, qmax)
    if not x.is_contiguous():
        x = _dense_input(x)
    y = torch.empty_like(x)
    _gpu_call("mctq_fq_per_tensor", x, x.data_ptr(), y.data_ptr(), x.numel(), dt, scale, zero_point, qmin, qmax)
    return y


def _check_axis(x, n_params: int, axis: int):
    d = x.dim()
    if axis >= d or axis < -d:                    # ATen's own errors, in its order (fake_quantize_per_channel_affine)
        raise IndexError(f"Dimension out of range (expected to be in range of [{-max(d, 1)}, {max(d, 1) - 1}], but got {axis})")
    if axis < 0:
        raise RuntimeError("`axis` must be between 0 and number of dimensions of input")
    if n_params != x.shape[axis]:
        raise RuntimeError("dimensions of scale and zero-point are not consistent with input tensor")


def _hip_fq_per_channel(x, scales, zero_points, axis: int, qmin: int, qmax: int, zero_zps: bool = False):
    """``zero_zps``: the caller knows every zero point is 0 (symmetric quantizers); the table is not read."""
    dt = _DTYPES.get(x.dtype)
    if dt is None:
        _dtype_code(x, "fq_per_channel")
    if not 0 <= axis < x.dim() or scales.numel() != x.shape[axis]:
        _check_axis(x, scales.numel(), axis)
    scales = _param_on(x, scales, "scales", torch.float32)
    zero_points = _param_on(x, zero_points, "zero_points", torch.int32)
    if not x.is_contiguous():
        x = _dense_input(x)
    y = torch.empty_like(x)
    outer, c, inner = _channel_view(x, axis)
    _gpu_call("mctq_fq_per_channel", x, x.data_ptr(), y.data_ptr(), outer, c, inner, dt, scales.data_ptr(),
              None if zero_zps else zero_points.data_ptr(), qmin, qmax)
    return y


def _hip_fq_per_tensor_tqp(x, scale, zero_point, qmin: int, qmax: int):
    """Tensor-qparams overload: ``scale`` float32[1] and ``zero_point`` int32[1] stay on the device (no .item())."""
    dt = _dtype_code(x, "fq_per_tensor_tqp")
    if scale.numel() < 1 or zero_point.numel() < 1:      # (ATen reads element 0 of longer tensors; so does the kernel)
        raise RuntimeError("fq_per_tensor_tqp: scale and zero_point must have at least one element")
    scale, zero_point = scale.reshape(-1)[:1], zero_point.reshape(-1)[:1]
    scale = _param_on(x, scale, "scale", torch.float32)
    zero_point = _param_on(x, zero_point, "zero_point", torch.int32)
    if not x.is_contiguous():
        x = _dense_input(x)
    y = torch.empty_like(x)
    _gpu_call("mctq_fq_per_tensor_tqp", x, x.data_ptr(), y.data_ptr(), x.numel(), dt, scale.data_ptr(), zero_point.data_ptr(),
              qmin, qmax)
    return y


def _hip_fq_batched(items):
    """ctypes route of fq_batched (see below): items = [(x, scales, zero_points | None, axis | None, qmin, qmax)]."""
    n = len(items)
    arr = (native.FqItem * n)()
    outs, keep = [], []
    dev = None
    for k, (x, scales, zps, axis, qmin, qmax) in enumerate(items):
        dt = _dtype_code(x, "fq_batched")
        if dev is None:
            dev = x.device
        elif x.device != dev:
            raise RuntimeError("fq_batched: all tensors of one call must be on the same device")
        if not x.is_contiguous():
            x = _dense_input(x)
        scales = _param_on(x, scales, "scales", torch.float32)
        if zps is not None:
            zps = _param_on(x, zps, "zero_points", torch.int32)
        elif axis is None and dt == native.DT_F64:
            zps = torch.zeros(1, dtype=torch.int32, device=x.device)
        if axis is None:
            outer, c, inner = (1, 1, x.numel()) if x.numel() else (0, 1, 0)
            if scales.numel() != 1:
                raise RuntimeError("fq_batched: a per-tensor item takes 1-element scales / zero_points")
        else:
            _check_axis(x, scales.numel(), axis)
            outer, c, inner = _channel_view(x, axis)
        y = torch.empty_like(x)
        it = arr[k]
        it.x, it.y = x.data_ptr(), y.data_ptr()
        it.outer, it.channels, it.inner = outer, c, inner
        it.scales = scales.data_ptr()
        it.zero_points = zps.data_ptr() if zps is not None else None
        it.quant_min, it.quant_max, it.dtype = qmin, qmax, dt
        it.flags = native.FQ_ITEM_PER_TENSOR if axis is None else 0
        outs.append(y)
        keep.append((x, scales, zps))
    if n:
        _gpu_call("mctq_fq_batched", outs[0], arr, n)
    return outs


def _lut_result(x, y):
    """The reference's LUT op chain ends in an index gather (quantizer_utils.py:135-137), whose result is a CONTIGUOUS
    tensor whatever the input's memory layout -- unlike ATen's fake-quant operators, which keep the input's strides.
    The kernels work in storage order (same strides as the input); a permuted input pays one layout copy here to hand
    back what the reference hands back."""
    return y if x.is_contiguous() else y.contiguous()


def _lut_family(x, dt: int, lut, table, steps, mult: float, cmin: float, cmax: float):
    """Which LUT kernels run on ``x`` -> ``(stem, suffix, book, entries)``: the entry points are
    ``mctq_<stem>_per_{tensor,channel}<suffix>`` and take ``book``'s pointer and ``entries`` as their codebook arguments.
    float64 tensors: the DOUBLE threshold list of an integer codebook ("luts", "_f64"), otherwise the literal scan; other
    storage types: the decision ``table`` ("lutt"), the sorted threshold list ``steps`` of an integer codebook too wide for the
    table (binary search in LDS; "luts"), or the literal first-minimum scan (non-integer codebooks, wide bit widths; "lut")."""
    if dt == native.DT_F64:
        s64 = _op_steps64(lut, mult, cmin, cmax)
        if s64 is not None:
            return "luts", "_f64", s64[0], s64[1]
    elif table is not None:
        table = _param_on(x, table, "table", torch.float32)
        return "lutt", "", table, table.shape[0] - 1
    elif steps is not None:
        steps = _param_on(x, steps, "steps", torch.float32)
        return "luts", "", steps, steps.numel()
    return "lut", "", lut, lut.numel()


def _hip_lut_per_tensor(x, lut, thr_div: float, thr_mul: float, mult: float, cmin: float, cmax: float, table=None,
                        step_round: int = 0, thr_div64: float = None, steps=None):
    """LUT quantizer, one threshold.  Output is float32 whatever x's type (the reference's chain promotes).
    ``thr_div64``: for float64 tensors whose divisor is a Python float (the activation quantizer) the divisor
    stays a double."""
    if not x.is_floating_point() and not x.is_complex():
        x = x.to(torch.float32)          # integer / bool tensors: the chain's first op, a true division, promotes to float32
    dt = _dtype_code(x, "lut_per_tensor")
    if dt != native.DT_F64 and table is not None and native.TRACE is False:
        f = _FAST if _FAST_READY else _fast_mod()
        if f is not None:
            y = f.lutt_per_tensor(x, table, step_round, thr_div, thr_mul, mult, cmin, cmax)
            if y is not NotImplemented:
                return y if x.is_contiguous() else y.contiguous()      # see _lut_result
    x_in = x
    x = _dense_input(x)
    y = torch.empty_like(x, dtype=torch.float32)
    lut = _param_on(x, lut, "lut_values", torch.float32)
    stem, suffix, book, n_book = _lut_family(x, dt, lut, table, steps, mult, cmin, cmax)
    if suffix or (dt == native.DT_F64 and thr_div64 is not None):
        # the divisor stays a double: the activation quantizer's, or a weights quantizer's float32 sum widened -- the same
        # number either way
        _gpu_call(f"mctq_{stem}_per_tensor_f64", x, x.data_ptr(), y.data_ptr(), x.numel(),
                  thr_div if thr_div64 is None else thr_div64, thr_mul, book.data_ptr(), n_book, mult, cmin, cmax)
    else:
        # every storage type, incl. the per-step half-precision roundings of a half activation (step_round)
        _gpu_call(f"mctq_{stem}_per_tensor", x, x.data_ptr(), y.data_ptr(), x.numel(), dt,
                  0 if dt == native.DT_F64 else step_round, thr_div, thr_mul, book.data_ptr(), n_book, mult, cmin, cmax)
    return _lut_result(x_in, y)


def _hip_lut_per_channel(x, lut, thresholds, eps: float, axis: int, mult: float, cmin: float, cmax: float,
                         table=None, steps=None):
    if not x.is_floating_point() and not x.is_complex():
        x = x.to(torch.float32)          # as in _hip_lut_per_tensor
    dt = _dtype_code(x, "lut_per_channel")
    _check_axis(x, thresholds.numel(), axis)
    if x.numel() > _SPLIT_ELEMS and thresholds.numel() > 1:            # more than one launch of the short-row kernels takes
        y = _split_rows(_dense_input(x), axis, (thresholds,), torch.float32,
                        lambda xp, ps, ax: _hip_lut_per_channel(xp, lut, ps[0], eps, ax, mult, cmin, cmax, table, steps))
        return _lut_result(x, y)
    if dt != native.DT_F64 and table is not None and native.TRACE is False:
        f = _FAST if _FAST_READY else _fast_mod()
        if f is not None:
            y = f.lutt_per_channel(x, thresholds, eps, table, axis, mult, cmin, cmax)
            if y is not NotImplemented:
                return y if x.is_contiguous() else y.contiguous()      # see _lut_result
    x_in = x
    x = _dense_input(x)
    y = torch.empty_like(x, dtype=torch.float32)
    outer, c, inner = _channel_view(x, axis)
    thresholds = _param_on(x, thresholds, "thresholds", torch.float32)
    lut = _param_on(x, lut, "lut_values", torch.float32)
    stem, suffix, book, n_book = _lut_family(x, dt, lut, table, steps, mult, cmin, cmax)
    _gpu_call(f"mctq_{stem}_per_channel{suffix}", x, x.data_ptr(), y.data_ptr(), outer, c, inner, *(() if suffix else (dt,)),
              thresholds.data_ptr(), eps, book.data_ptr(), n_book, mult, cmin, cmax)
    return _lut_result(x_in, y)


def _hip_grid_per_tensor(x, lo: float, hi: float, step: float, shifted: bool):
    """Export-time arithmetic (include/mctq_hip.h: mctq_grid_per_tensor_f32), float32 only."""
    if x.dtype != torch.float32:
        raise NotImplementedError(f"export-time quantizer arithmetic on the GPU takes float32 tensors, got {x.dtype}")
    x = _dense_input(x)
    y = torch.empty_like(x)
    _gpu_call("mctq_grid_per_tensor_f32", x, x.data_ptr(), y.data_ptr(), x.numel(), lo, hi, step, int(shifted))
    return y


def _hip_grid_per_channel(x, los, his, steps, axis: int, shifted: bool):
    if x.dtype != torch.float32:
        raise NotImplementedError(f"export-time quantizer arithmetic on the GPU takes float32 tensors, got {x.dtype}")
    _check_axis(x, steps.numel(), axis)
    x = _dense_input(x)
    if x.numel() > _SPLIT_ELEMS and steps.numel() > 1:
        return _split_rows(x, axis, (los.reshape(-1), his.reshape(-1), steps.reshape(-1)), torch.float32,
                           lambda xp, ps, ax: _hip_grid_per_channel(xp, ps[0], ps[1], ps[2], ax, shifted))
    y = torch.empty_like(x)
    outer, c, inner = _channel_view(x, axis)
    los, his, steps = (t.to(device=x.device, dtype=torch.float32).contiguous() for t in (los, his, steps))
    _gpu_call("mctq_grid_per_channel_f32", x, x.data_ptr(), y.data_ptr(), outer, c, inner, los.data_ptr(), his.data_ptr(),
              steps.data_ptr(), int(shifted))
    return y


def _code_dtype(qmin: int, qmax: int):
    if qmin >= 0 and qmax <= 255:
        return torch.uint8, native.CODE_U8
    if qmin >= -128 and qmax <= 127:
        return torch.int8, native.CODE_I8
    raise ValueError(f"clamp domain [{qmin}, {qmax}] does not fit an 8-bit code")


def _code_of(codes: torch.Tensor) -> int:
    """The C ABI's code type of an int8 / uint8 tensor of codes."""
    return native.CODE_U8 if codes.dtype == torch.uint8 else native.CODE_I8


def _is_codes(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in (torch.int8, torch.uint8)


def _nhwc_codes(x, caller: str):
    """The checks of a wrapper that takes int8 / uint8 codes [N, H, W, C]."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{caller} takes [N, H, W, C] tensors")
    if not _is_codes(x):
        raise NotImplementedError(f"{caller}: int8 / uint8 codes only, got {x.dtype}")


def _check_form(caller: str, dtype, zero_point=None, scale=None, zp_words: str = "the zero point {}", scale_words: str = "the scales"):
    """The form of an operand on codes of ``dtype``, in ``caller``'s name and its words for the operand: the zero point (where
    given; ``zp_words`` is formatted with it) is a code of ``dtype``, the scale (or each of several) is finite and positive."""
    if zero_point is not None:
        lo, hi = (0, 255) if dtype == torch.uint8 else (-128, 127)
        if not lo <= zero_point <= hi:
            raise ValueError(f"{caller}: {zp_words.format(zero_point)} is no {dtype} code")
    scales = () if scale is None else scale if isinstance(scale, tuple) else (scale,)
    if not all(0.0 < s < float("inf") for s in scales):
        raise ValueError(f"{caller}: {scale_words} must be finite and positive")


def _out_form(out_form):
    """``(scale, zero_point, qmin, qmax)`` of a holder -> those four, the torch dtype of its codes and the C ABI's code type."""
    scale, zero_point, qmin, qmax = float(out_form[0]), int(out_form[1]), int(out_form[2]), int(out_form[3])
    return (scale, zero_point, qmin, qmax) + _code_dtype(qmin, qmax)


def _contiguous(x: torch.Tensor) -> torch.Tensor:
    return x if x.is_contiguous() else x.contiguous()


def _packed_shape(x):
    return tuple(x.shape[:-1]) + (x.shape[-1] // 2,) if x.dim() and x.shape[-1] % 2 == 0 and x.is_contiguous() \
        else (x.numel() // 2,)


def _pack4_as_stored(q: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """CPU routes: the integer codes ``q`` of ``x`` (x's shape), two per byte in x's STORAGE order."""
    if x.is_contiguous() or not _is_dense(x):
        return pack4(q.contiguous()).reshape(_packed_shape(x))
    flat = torch.empty(x.numel(), dtype=torch.int16)          # dense, permuted storage: pack in STORAGE order
    torch.as_strided(flat, x.shape, x.stride()).copy_(q.to(torch.int16))
    return pack4(flat).reshape(_packed_shape(x))


def _codes_output(x: torch.Tensor, packed4: bool, tdt, code: int, code4: int):
    """GPU routes: ``(output tensor, the C ABI's code type)`` for the codes of ``x`` -- ``packed4``: uint8 of half the elements
    and ``code4``, otherwise x's sizes and strides in ``tdt`` and ``code``."""
    if packed4:
        return torch.empty(_packed_shape(x), dtype=torch.uint8, device=x.device), code4
    return torch.empty_like(x, dtype=tdt), code


def pack4(q: torch.Tensor) -> torch.Tensor:
    """Integer codes in [-8, 15] (any integer dtype, storage order) -> two per byte, element 2j in the low nibble."""
    flat = q.reshape(-1).to(torch.int16) & 0xF
    return (flat[0::2] | (flat[1::2] << 4)).to(torch.uint8)


def unpack4(packed: torch.Tensor, signed: bool, shape=None) -> torch.Tensor:
    """Inverse of the 4-bit packing: uint8 [n/2] (any shape) -> int8 codes [n] (or ``shape``)."""
    b = packed.reshape(-1).to(torch.int16)
    both = torch.stack((b & 0xF, (b >> 4) & 0xF), dim=1).reshape(-1)
    if signed:
        both = torch.where(both > 7, both - 16, both)
    both = both.to(torch.int8)
    return both if shape is None else both.reshape(shape)


def fq_codes(x, scales, zero_points, axis, qmin: int, qmax: int, scale0: float = None, zp0: int = None,
             packed4: bool = False):
    """Integer clamp indices of the affine quantizers as int8 / uint8 (extension, not in the reference).

    ``axis`` None = per-tensor (scale0 / zp0 are the host copies of the single scale and zero point).
    ``(codes - zero_point) * scale`` is bit-identical to the fake-quantized tensor.
    ``packed4``: clamp domains within [-8, 7] or [0, 15] leave as two codes per byte (uint8 tensor of half the
    elements: last dimension halved for contiguous tensors; element 2j of the storage order in the low nibble).
    """
    if packed4:
        if not ((qmin >= -8 and qmax <= 7) or (qmin >= 0 and qmax <= 15)):
            raise ValueError(f"clamp domain [{qmin}, {qmax}] does not fit a 4-bit code")
        if x.numel() % 2:
            raise ValueError("4-bit packing needs an even number of elements")
    tdt, code = _code_dtype(qmin, qmax)
    if not x.is_cuda:
        # CPU tensors: the same arithmetic with torch ops (float32 math, as ATen's CPU kernel)
        xf = x.float()
        if axis is None:
            q = torch.round(xf * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(scale0, dtype=torch.float32))) + zp0
        else:
            shape = [1] * x.dim()
            shape[axis] = -1
            q = torch.round(xf * (1.0 / scales.float().to(x.device)).reshape(shape)) + \
                zero_points.to(x.device).reshape(shape).float()
        q = torch.clamp(torch.nan_to_num(q, nan=float(qmin)), qmin, qmax)
        return _pack4_as_stored(q, x) if packed4 else q.to(tdt)
    dt = _dtype_code(x, "fq_codes")
    if dt == native.DT_F64:
        raise NotImplementedError("fq_codes: integer codes are produced from float32 / float16 / bfloat16 tensors")
    if not x.is_contiguous():
        x = _dense_input(x)
    if axis is not None and not packed4 and x.numel() > _SPLIT_ELEMS and scales.numel() > 1:
        return _split_rows(x, axis, (scales.reshape(-1), zero_points.reshape(-1)), tdt,
                           lambda xp, ps, ax: fq_codes(xp, ps[0], ps[1], ax, qmin, qmax))
    y, code = _codes_output(x, packed4, tdt, code, native.CODE_I4 if qmin < 0 else native.CODE_U4)
    if axis is None:
        _gpu_call("mctq_fq_codes_per_tensor", x, x.data_ptr(), y.data_ptr(), x.numel(), dt, code, scale0, zp0, qmin, qmax)
    else:
        _check_axis(x, scales.numel(), axis)
        scales = _param_on(x, scales, "scales", torch.float32)
        zero_points = _param_on(x, zero_points, "zero_points", torch.int32)
        outer, c, inner = _channel_view(x, axis)
        _gpu_call("mctq_fq_codes_per_channel", x, x.data_ptr(), y.data_ptr(), outer, c, inner, dt, code, scales.data_ptr(),
                  zero_points.data_ptr(), qmin, qmax)
    return y


def fq_codes_nhwc(x, qmin: int, qmax: int, scale: float, zero_point: int):
    """Per-tensor codes of a 4-D activation as a contiguous [N, H, W, C] int8 / uint8 tensor, whatever x's memory
    format.  NCHW-contiguous GPU tensors take one fused quantize-and-transpose pass (mctq_fq_codes_nchw_to_nhwc);
    channels-last ones are quantized in place (their storage order already is NHWC)."""
    if x.dim() != 4:
        raise ValueError("fq_codes_nhwc takes [N, C, H, W] tensors")
    b, c, h, w = x.shape
    if x.is_cuda and x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last):
        tdt, code = _code_dtype(qmin, qmax)
        dt = _dtype_code(x, "fq_codes_nhwc")
        if dt == native.DT_F64:
            raise NotImplementedError("fq_codes_nhwc: float32 / float16 / bfloat16 tensors only")
        y = torch.empty((b, h, w, c), dtype=tdt, device=x.device)
        _gpu_call("mctq_fq_codes_nchw_to_nhwc", x, x.data_ptr(), y.data_ptr(), b, c, h * w, dt, code, float(scale),
                  int(zero_point), qmin, qmax)
        return y
    codes = fq_codes(x, None, None, None, qmin, qmax, scale, zero_point)
    return codes.permute(0, 2, 3, 1).contiguous()          # a no-op view + check for channels-last storage


def dequantize_codes(codes, scale: float, zero_point: int):
    """``(codes - zero_point) * scale`` in float32 with one rounding: bit for bit the fake-quantized tensor the int8 / uint8
    ``codes`` were written next to (``fq_join``, ``fq_codes``); torch ops on the codes' device."""
    if codes.dtype not in (torch.int8, torch.uint8):
        raise TypeError(f"dequantize_codes takes int8 / uint8 codes, got {codes.dtype}")
    return (codes.to(torch.int32) - int(zero_point)).to(torch.float32) * torch.tensor(scale, dtype=torch.float64).to(torch.float32)


def fq_join(x, scale: float, zero_point: int, qmin: int, qmax: int, residual=None, relu: bool = False,
            want_float: bool = True, want_codes: bool = True, residual_codes=None):
    """The prologue and both outputs of an activation holder that several layers share (extension, not in the reference):
    with ``v = x`` (``+ residual``; then ``relu(v)``), returns ``(y, codes)`` where ``y = fq_per_tensor(v, ...)`` is the
    fake-quantized float32 tensor and ``codes = fq_codes(v, ...)`` its int8 / uint8 codes, ``(codes - zero_point) * scale ==
    y`` bit for bit; an output that is not wanted is None.  Both have x's shape and strides (a channels-last x gives
    "NCHW-shaped, NHWC-stored" codes, which the integer consumers take as they are).

    Dense float32 GPU tensors (``residual`` with x's shape, strides and dtype) run ``mctq_fq_join_f32``: one launch that
    reads x and residual once and writes both outputs.  Everything else -- CPU tensors, other dtypes, a broadcasting or
    differently strided residual, a non-dense or misaligned x, clamp domains beyond 2^24 -- composes the same result from
    torch's add and relu, ``fq_per_tensor`` and ``fq_codes``.  No backward, no ``torch.compile`` op.

    ``residual_codes = (codes, scale, zero_point)`` instead of ``residual``: the residual operand as the int8 / uint8 codes of
    another quantizer (an identity branch that stays on codes), standing for ``dequantize_codes(codes, scale, zero_point)`` --
    bit for bit the float32 tensor a join writes next to those codes, so the result is that of ``residual=`` that tensor.
    Dense float32 GPU x with codes of x's shape and strides, both 16-byte aligned, run ``mctq_fq_join_rc_f32``: one launch that
    reads 1 byte per residual element instead of 4.  Everything else dequantizes the codes with torch ops and goes on as above."""
    if not want_float and not want_codes:
        raise ValueError("fq_join: at least one of want_float / want_codes")
    r_codes = None
    if residual_codes is not None:
        if residual is not None:
            raise ValueError("fq_join: residual and residual_codes exclude each other")
        r_codes, r_scale, r_zp = residual_codes
        if not _is_codes(r_codes):
            raise TypeError("fq_join: residual_codes takes an int8 / uint8 tensor")
        r_scale, r_zp = float(r_scale), int(r_zp)
        _check_form("fq_join", r_codes.dtype, r_zp, r_scale, "the residual's zero point {}", "the residual's scale")
    tdt = code = None
    if want_codes:
        tdt, code = _code_dtype(qmin, qmax)
    direct = (_is_real(x) and x.is_cuda and x.dtype == torch.float32 and not _wide(qmin, qmax) and not _tracing()
              and not _compiling() and _is_dense(x) and x.data_ptr() % 16 == 0)
    if direct and residual is not None:
        direct = (_is_real(residual) and residual.device == x.device and residual.dtype == x.dtype
                  and residual.shape == x.shape and residual.stride() == x.stride() and residual.data_ptr() % 16 == 0)
    if direct and r_codes is not None:
        direct = (_is_real(r_codes) and r_codes.device == x.device and r_codes.shape == x.shape
                  and r_codes.stride() == x.stride() and r_codes.data_ptr() % 16 == 0)
    if not direct and r_codes is not None:
        with torch.no_grad():
            residual = dequantize_codes(r_codes, r_scale, r_zp)
    if not direct:
        if _is_real(x) and x.device.type == "cpu":
            _cpu_route_allowed()
        with torch.no_grad():
            v = x if residual is None else x + residual
            if relu:
                v = torch.relu(v)
            y = fq_per_tensor(v, scale, zero_point, qmin, qmax) if want_float else None
            codes = fq_codes(v, None, None, None, qmin, qmax, scale, zero_point) if want_codes else None
        return y, codes
    if want_float:
        _check_aten_range(zero_point, qmin, qmax)           # as fq_per_tensor
    y = torch.empty_like(x) if want_float else None          # preserve_format: a dense x keeps its strides
    codes = torch.empty_like(x, dtype=tdt) if want_codes else None
    outputs = (None if y is None else y.data_ptr(), None if codes is None else codes.data_ptr(), code or 0, x.numel(),
               float(scale), int(zero_point), int(qmin), int(qmax))
    if r_codes is not None:
        _gpu_call("mctq_fq_join_rc_f32", x, x.data_ptr(), r_codes.data_ptr(), _code_of(r_codes), r_scale, r_zp, int(bool(relu)),
                  *outputs)
    else:
        _gpu_call("mctq_fq_join_f32", x, x.data_ptr(), None if residual is None else residual.data_ptr(), int(bool(relu)),
                  *outputs)
    return y, codes


def _pair(v, what: str, caller: str = "codes_im2col"):
    """An int or a pair of ints (torch.nn.Conv2d's kernel_size / stride / padding / dilation) -> (h, w)."""
    if isinstance(v, int):
        return v, v
    v = tuple(v)
    if len(v) != 2 or not all(isinstance(e, int) for e in v):
        raise ValueError(f"{caller}: {what} must be an int or a pair of ints, got {v!r}")
    return v


def _conv_out_size(n: int, k: int, s: int, p: int, d: int) -> int:
    """Outputs along one axis of a convolution: ``n`` inputs, kernel ``k``, stride ``s``, padding ``p``, dilation ``d``."""
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def _pool_out_size(n: int, k: int, s: int, p: int, d: int, ceil_mode: bool) -> int:
    """Outputs along one axis of ``torch.nn.MaxPool2d``: as ``_conv_out_size``, the division rounded up with ``ceil_mode``, less
    the last window where it would start beyond the image plus its left padding."""
    span = n + 2 * p - d * (k - 1) - 1
    out = (-(-span // s) if ceil_mode else span // s) + 1
    if ceil_mode and (out - 1) * s >= n + p:
        out -= 1
    return out


def _conv_geometry(h: int, w: int, kernel_size, stride, padding, dilation, caller: str, ceil_mode=None, dilated: bool = True):
    """A convolution of an ``h`` x ``w`` image, its arguments ints or pairs -> the pairs ``(kh, kw), (sh, sw), (ph, pw), (dh, dw)``
    and the output size ``(ho, wo)``; ValueError, in ``caller``'s name, for arguments that describe no convolution of it.
    With a ``ceil_mode`` it is one of torch's pools: ``stride=None`` means the kernel size, the padding is at most half of it,
    the output size is ``_pool_out_size``'s; ``dilated=False``: a pool without the argument (``dilation=1``), for the messages."""
    pool = ceil_mode is not None
    (kh, kw), (sh, sw) = _pair(kernel_size, "kernel_size", caller), _pair(kernel_size if pool and stride is None else stride, "stride", caller)
    (ph, pw), (dh, dw) = _pair(padding, "padding", caller), _pair(dilation, "dilation", caller)
    if min(kh, kw, sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise ValueError(f"{caller}: kernel_size{', stride and dilation' if dilated else ' and stride'} must be at least 1 and padding at least 0")
    if pool and (ph > kh // 2 or pw > kw // 2):
        raise ValueError(f"{caller}: padding {ph}x{pw} is larger than half the {kh}x{kw} kernel")
    ho, wo = _pool_out_size(h, kh, sh, ph, dh, bool(ceil_mode)), _pool_out_size(w, kw, sw, pw, dw, bool(ceil_mode))
    if ho <= 0 or wo <= 0:
        raise ValueError(f"{caller}: a {kh}x{kw} kernel{f' (dilation {dh}x{dw})' if dilated else ''} does not fit the padded {h}x{w} image")
    return (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ho, wo)


def codes_im2col(codes_nhwc, kernel_size, stride=1, padding=0, dilation=1, pad_code: int = 0, pad_to: int = 1):
    """The patch matrix of a convolution over activation codes: contiguous int8 / uint8 codes [B, H, W, C] (what
    ``fq_codes_nhwc`` returns) -> [B * Ho * Wo, kh * kw * C], row (b, oy, ox), column (ky * kw + kx) * C + c; taps
    outside the image hold ``pad_code`` (the activation's zero point: such a tap then adds nothing to the integer
    consumer's sum).  GPU tensors run mctq_codes_im2col_nhwc (C % 16 == 0, kh * kw * C <= 32768); CPU tensors the same
    gather with torch ops, byte for byte.

    ``pad_to=16`` (1, the default, or 16): the rows are padded with ``pad_code`` to ``Kp = 16 * ceil(K / 16)`` columns,
    K = kh * kw * C, for any C >= 1 -- the rows the integer consumers take where K is no multiple of 16.  GPU tensors with
    K % 16 == 0 and C % 16 == 0 keep the launch above; every other GPU tensor runs mctq_codes_im2col_pad_nhwc (Kp <= 32768);
    CPU tensors the gather above with the columns appended.  A 2-D ``[M, K]`` codes tensor is then taken as ``[M, 1, 1, K]``:
    the row re-pitch of a Linear or pointwise layer."""
    if pad_to not in (1, 16):
        raise ValueError(f"codes_im2col: pad_to must be 1 or 16, got {pad_to!r}")
    if pad_to == 16 and isinstance(codes_nhwc, torch.Tensor) and codes_nhwc.dim() == 2:
        codes_nhwc = codes_nhwc.reshape(codes_nhwc.shape[0], 1, 1, codes_nhwc.shape[1])
    _nhwc_codes(codes_nhwc, "codes_im2col")
    pad_code = int(pad_code)
    _check_form("codes_im2col", codes_nhwc.dtype, pad_code, zp_words="pad_code {}")
    b, h, w, c = codes_nhwc.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ho, wo) = _conv_geometry(h, w, kernel_size, stride, padding, dilation, "codes_im2col")
    x = _contiguous(codes_nhwc)
    k = kh * kw * c
    kp = -(-k // pad_to) * pad_to
    if x.is_cuda:
        y = torch.empty((b * ho * wo, kp), dtype=x.dtype, device=x.device)
        name = "mctq_codes_im2col_nhwc" if pad_to == 1 or (k % 16 == 0 and c % 16 == 0) else "mctq_codes_im2col_pad_nhwc"
        _gpu_call(name, x, x.data_ptr(), y.data_ptr(), b, h, w, c, kh, kw, sh, sw, ph, pw, dh, dw, pad_code)
        return y
    _cpu_route_allowed()
    xp = torch.nn.functional.pad(x, (0, 0, pw, pw, ph, ph), value=pad_code)              # [B, H + 2 ph, W + 2 pw, C]
    sb, sy, sx, sc = xp.stride()
    taps = xp.as_strided((b, ho, wo, kh, kw, c), (sb, sy * sh, sx * sw, sy * dh, sx * dw, sc))
    rows = taps.reshape(b * ho * wo, k)
    return rows if kp == k else torch.nn.functional.pad(rows, (0, kp - k), value=pad_code)


def codes_maxpool(codes_nhwc, kernel_size, stride=None, padding=0, dilation=1, ceil_mode: bool = False):
    """``torch.nn.MaxPool2d`` on activation codes: int8 / uint8 codes [B, H, W, C] (what ``fq_codes_nhwc`` returns) -> contiguous
    [B, Ho, Wo, C] of the same type; ``stride=None`` means ``kernel_size``, padded taps are ignored (they stand for -inf, not for
    the zero point), ``padding`` is at most half the kernel size.  The codes of a quantizer are monotone in the value, so
    ``dequantize_codes(codes_maxpool(c), s, z) == F.max_pool2d(dequantize_codes(c, s, z))`` bit for bit (NCHW views of both).
    GPU tensors run mctq_codes_maxpool_nhwc (C % 16 == 0), which is given the output extent allocated here and refuses one
    that is not its own; CPU tensors run ``F.max_pool2d`` on the codes themselves."""
    _nhwc_codes(codes_nhwc, "codes_maxpool")
    b, h, w, c = codes_nhwc.shape
    ceil_mode = bool(ceil_mode)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ho, wo) = _conv_geometry(h, w, kernel_size, stride, padding, dilation, "codes_maxpool", ceil_mode)
    x = _contiguous(codes_nhwc)
    if x.is_cuda:
        if c % 16:
            raise NotImplementedError(f"mctq_codes_maxpool_nhwc needs C % 16 == 0, got C={c}")
        y = torch.empty((b, ho, wo, c), dtype=x.dtype, device=x.device)
        _gpu_call("mctq_codes_maxpool_nhwc", x, x.data_ptr(), y.data_ptr(), _code_of(x), b, h, w, c, kh, kw, sh, sw, ph, pw, dh, dw,
                  int(ceil_mode), ho, wo)
        return y
    _cpu_route_allowed()
    if 0 in (b, c):
        return x.new_empty((b, ho, wo, c))
    # (NCHW-contiguous: ATen's channels-last kernel keeps its indices in the tensor's own integer type and refuses larger images)
    y = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), (kh, kw), (sh, sw), (ph, pw), (dh, dw), ceil_mode)
    return y.permute(0, 2, 3, 1).contiguous()


_AVGPOOL_MAX_TAPS = 65536    # taps of a window of one mctq_codes_avgpool_nhwc launch: 255 * 65536 < 2^24, float32(S) is exact


def codes_avgpool(codes_nhwc, in_form, out_form, kernel_size, stride=None, padding=0, ceil_mode: bool = False,
                  count_include_pad: bool = True, divisor_override=None):
    """``torch.nn.AvgPool2d`` on activation codes, in the form of the holder behind the pool: int8 / uint8 codes [B, H, W, C] of
    the form ``in_form = (scale, zero_point)`` -> contiguous [B, Ho, Wo, C] codes of ``_code_dtype(qmin, qmax)`` in
    ``out_form = (scale, zero_point, qmin, qmax)``.  ``kernel_size=None`` is the whole image (global pooling), ``stride=None``
    means ``kernel_size``, ``padding`` is at most half the kernel size.  Per output element, with S the exact integer sum of
    ``code - zero_point`` over the window's taps inside the image (a padded tap is 0.0 in float32 and adds nothing) and ``div``
    the divisor -- ``divisor_override``, or PyTorch's ``pool_size`` with ``count_include_pad``, or the taps inside the image --

        code = clamp(rint((float32(S) * scale_in) / float32(div) * (1 / scale_out)) + zp_out, qmin, qmax)

    every operation in float32 and rounded once (a window without a tap gives 0.0).  Where ``scale_in`` and every ``div`` are
    powers of two this is bit for bit the code the holder behind a float32 average pool of the dequantized codes gives, whichever
    way that pool sums; elsewhere it is the exact mean rounded twice, within one code of a float32 chain next to a rounding tie.
    GPU tensors with C % 16 == 0 and at most 65536 taps per window take one launch of mctq_codes_avgpool_nhwc (1 byte read per
    tap, 1 written per output element), which is given the output extent allocated here and refuses one that is not its own;
    anything else on the GPU, and every CPU tensor, evaluates the expression above with torch integer and float32 ops, which the
    kernel matches byte for byte."""
    _nhwc_codes(codes_nhwc, "codes_avgpool")
    a_scale, a_zp = float(in_form[0]), int(in_form[1])
    o_scale, o_zp, qmin, qmax, tdt, ocode = _out_form(out_form)
    _check_form("codes_avgpool", codes_nhwc.dtype, a_zp, (a_scale, o_scale))
    if divisor_override is not None and (not isinstance(divisor_override, int) or isinstance(divisor_override, bool)
                                         or divisor_override < 1):
        raise ValueError(f"codes_avgpool: divisor_override must be a positive int or None, got {divisor_override!r}")
    b, h, w, c = codes_nhwc.shape
    if kernel_size is None:
        kernel_size = (h, w)
    ceil_mode, count_include_pad = bool(ceil_mode), bool(count_include_pad)
    (kh, kw), (sh, sw), (ph, pw), _, (ho, wo) = _conv_geometry(h, w, kernel_size, stride, padding, 1, "codes_avgpool", ceil_mode, dilated=False)
    x = _contiguous(codes_nhwc)
    if x.is_cuda and c % 16 == 0 and kh * kw <= _AVGPOOL_MAX_TAPS:
        y = torch.empty((b, ho, wo, c), dtype=tdt, device=x.device)
        _gpu_call("mctq_codes_avgpool_nhwc", x, x.data_ptr(), y.data_ptr(), _code_of(x), a_zp, a_scale, b, h, w, c, kh, kw, sh, sw,
                  ph, pw, int(ceil_mode), int(count_include_pad), divisor_override or 0, ho, wo, ocode, o_scale, o_zp, qmin, qmax)
        return y
    if not x.is_cuda:
        _cpu_route_allowed()
    if 0 in (b, c):
        return x.new_empty((b, ho, wo, c), dtype=tdt)
    with torch.no_grad():
        # S: the codes less the zero point, zeros around them as far as the last window reaches (ceil_mode: beyond the padding)
        d = x.to(torch.int32) - a_zp
        d = torch.nn.functional.pad(d, (0, 0, pw, max(0, (wo - 1) * sw + kw - w - pw), ph, max(0, (ho - 1) * sh + kh - h - ph)))
        sb, sy, sx, sc = d.stride()
        total = d.as_strided((b, ho, wo, kh, kw, c), (sb, sy * sh, sx * sw, sy, sx, sc)).sum(dim=(3, 4))          # int64, exact
        h0, w0 = torch.arange(ho, device=x.device) * sh - ph, torch.arange(wo, device=x.device) * sw - pw
        if divisor_override is not None:
            div = torch.full((ho, wo), divisor_override, dtype=torch.int64, device=x.device)
        elif count_include_pad:
            div = ((h0 + kh).clamp(max=h + ph) - h0)[:, None] * ((w0 + kw).clamp(max=w + pw) - w0)[None, :]
        else:
            div = ((h0 + kh).clamp(max=h) - h0.clamp(min=0)).clamp(min=0)[:, None] * \
                ((w0 + kw).clamp(max=w) - w0.clamp(min=0)).clamp(min=0)[None, :]
        div = div.to(torch.float32)[None, :, :, None]
        f32 = lambda v: torch.tensor(v, dtype=torch.float64, device=x.device).to(torch.float32)               # noqa: E731
        v = total.to(torch.float32) * f32(a_scale)
        m = torch.where(div > 0, v / div, torch.zeros_like(v))
        q = torch.round(m * (torch.tensor(1.0, dtype=torch.float32, device=x.device) / f32(o_scale))) + float(o_zp)
        q = torch.clamp(torch.nan_to_num(q, nan=float(qmin)), qmin, qmax)
        return q.to(tdt).contiguous()


_CONCAT_MAX = 8           # operands of one mctq_codes_concat_nhwc launch


def codes_concat(operands, out_form):
    """``torch.cat`` along the channels on activation codes, in the form of the holder behind it.  ``operands``: a sequence of
    ``(codes, scale, zero_point)``, int8 / uint8 codes ``[.., C_k]`` (channels last) with the same leading shape on one device;
    ``out_form = (scale, zero_point, qmin, qmax)``.  Returns contiguous codes ``[.., sum C_k]`` of ``_code_dtype(qmin, qmax)``:

        torch.cat([fq_codes(dequantize_codes(c_k, s_k, z_k), None, None, None, qmin, qmax, s, z) for k], -1)

    -- a holder's float32 output is ``dequantize_codes`` of its codes bit for bit and ``torch.cat`` only moves data, so these are
    the codes the holder behind ``torch.cat`` of the operand holders' outputs gives.  GPU tensors with every ``C_k % 16 == 0``
    and at most 8 operands take one launch of mctq_codes_concat_nhwc (1 byte read, 1 byte written per element; an operand in the
    output's own form is copied); anything else on the GPU, and every CPU tensor, evaluates the expression above with torch ops,
    which the kernel matches byte for byte."""
    operands = [(c, float(s), int(z)) for c, s, z in operands]
    if not operands:
        raise ValueError("codes_concat needs at least one operand")
    o_scale, o_zp, qmin, qmax, tdt, ocode = _out_form(out_form)
    first = operands[0][0]
    for c, s, z in operands:
        if not _is_codes(c) or c.dim() < 1:
            raise TypeError("codes_concat takes int8 / uint8 codes [.., C]")
        if c.device != first.device or c.shape[:-1] != first.shape[:-1]:
            raise RuntimeError(f"codes_concat: operands must share the device and the leading shape, got {tuple(c.shape)} on "
                               f"{c.device} next to {tuple(first.shape)} on {first.device}")
        _check_form("codes_concat", c.dtype, z, s, scale_words="an operand's scale")
    _check_form("codes_concat", None, scale=o_scale, scale_words="the output's scale")
    lead, total = tuple(first.shape[:-1]), sum(c.shape[-1] for c, _, _ in operands)
    o_lo, o_hi = (0, 255) if tdt == torch.uint8 else (-128, 127)
    if (first.is_cuda and len(operands) <= _CONCAT_MAX and all(c.shape[-1] > 0 and c.shape[-1] % 16 == 0 for c, _, _ in operands)
            and o_lo <= o_zp <= o_hi):
        pixels = math.prod(lead)
        keep = [_contiguous(c) for c, _, _ in operands]                                 # named: they must outlive the launch
        out = torch.empty(lead + (total,), dtype=tdt, device=first.device)
        items = (native.ConcatItem * len(keep))()
        for it, c, (_, s, z) in zip(items, keep, operands):
            it.codes, it.channels, it.code_dtype, it.zero_point, it.scale = c.data_ptr(), c.shape[-1], _code_of(c), z, s
        _gpu_call("mctq_codes_concat_nhwc", first, items, len(keep), out.data_ptr(), ocode, pixels, o_scale, o_zp, qmin, qmax)
        return out
    if not first.is_cuda:
        _cpu_route_allowed()
    with torch.no_grad():
        parts = [fq_codes(dequantize_codes(c, s, z), None, None, None, qmin, qmax, o_scale, o_zp) for c, s, z in operands]
        return torch.cat(parts, -1).contiguous()


def integer_factor(src, n_in: int):
    """``f`` if the host-side index map ``src`` (a sequence or CPU tensor of ints) is that of an integer factor over ``n_in`` inputs
    -- ``len(src) == f * n_in`` and ``src == arange(len(src)) // f``, f >= 1 -- else None."""
    src = [int(v) for v in (src.tolist() if isinstance(src, torch.Tensor) else src)]
    if n_in < 1 or not src or len(src) % n_in:
        return None
    f = len(src) // n_in
    return f if src == [i // f for i in range(len(src))] else None


def codes_upsample(codes_nhwc, in_form, out_form, src_rows, src_cols, factors=None):
    """Nearest resampling on activation codes, in the form of the holder behind it: int8 / uint8 codes [B, H, W, C] of the form
    ``in_form = (scale, zero_point)`` -> contiguous [B, Ho, Wo, C] codes of ``_code_dtype(qmin, qmax)`` in ``out_form = (scale,
    zero_point, qmin, qmax)``.  ``src_rows`` / ``src_cols``: integer index vectors (tensors) of lengths Ho / Wo, the source row of
    every output row and the source column of every output column -- what ``torch.nn.Upsample`` / ``F.interpolate`` in the
    modes "nearest" and "nearest-exact" compute, up- or downsampling alike:

        fq_codes(dequantize_codes(codes.index_select(1, src_rows).index_select(2, src_cols), s_in, z_in), ..., qmin, qmax, s, z)

    -- a holder's float32 output is ``dequantize_codes`` of its codes bit for bit and nearest interpolation only moves data, so
    these are the codes the holder behind the float32 upsample of a holder's output gives.  ``factors = (fh, fw)``: the caller's
    word that the maps are those of integer factors (``integer_factor``); None has maps on the CPU examined here, maps on the GPU
    are passed to the kernel as they are (no host read).  GPU tensors with C % 16 == 0 take one launch of
    mctq_codes_upsample_nhwc (1 byte read per output element or less, 1 written); anything else on the GPU, and every CPU
    tensor, evaluates the expression above with torch ops, which the kernel matches byte for byte.  Both clamp every map entry
    into ``[0, H - 1]`` / ``[0, W - 1]`` first: no table can make either read outside the image."""
    _nhwc_codes(codes_nhwc, "codes_upsample")
    a_scale, a_zp = float(in_form[0]), int(in_form[1])
    o_scale, o_zp, qmin, qmax, tdt, ocode = _out_form(out_form)
    _check_form("codes_upsample", codes_nhwc.dtype, a_zp, (a_scale, o_scale))
    for m, what in ((src_rows, "src_rows"), (src_cols, "src_cols")):
        if not isinstance(m, torch.Tensor) or m.dim() != 1 or m.dtype.is_floating_point or m.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise TypeError(f"codes_upsample: {what} must be a 1-D integer tensor")
    b, h, w, c = codes_nhwc.shape
    ho, wo = src_rows.numel(), src_cols.numel()
    if ho and wo and 0 in (h, w):
        raise ValueError(f"codes_upsample: a {ho}x{wo} output needs an image of at least one pixel, got {h}x{w}")
    x = _contiguous(codes_nhwc)
    o_lo, o_hi = (0, 255) if tdt == torch.uint8 else (-128, 127)
    if x.is_cuda and c % 16 == 0 and o_lo <= o_zp <= o_hi:
        y = torch.empty((b, ho, wo, c), dtype=tdt, device=x.device)
        if y.numel() == 0:
            return y
        if factors is None and not src_rows.is_cuda and not src_cols.is_cuda:
            fh, fw = integer_factor(src_rows, h), integer_factor(src_cols, w)
            factors = (fh, fw) if fh and fw else None
        if factors is not None:
            fh, fw = int(factors[0]), int(factors[1])
            if fh < 1 or fw < 1 or ho != fh * h or wo != fw * w:
                raise ValueError(f"codes_upsample: factors {fh}x{fw} do not take {h}x{w} to {ho}x{wo}")
            _gpu_call("mctq_codes_upsample_nhwc", x, x.data_ptr(), y.data_ptr(), _code_of(x), a_zp, a_scale, b, h, w, c, ho, wo,
                      fh, fw, None, None, ocode, o_scale, o_zp, qmin, qmax)
            return y
        rows = _contiguous(src_rows.to(device=x.device, dtype=torch.int32))          # named: they must outlive the launch
        cols = _contiguous(src_cols.to(device=x.device, dtype=torch.int32))
        _gpu_call("mctq_codes_upsample_nhwc", x, x.data_ptr(), y.data_ptr(), _code_of(x), a_zp, a_scale, b, h, w, c, ho, wo,
                  0, 0, rows.data_ptr(), cols.data_ptr(), ocode, o_scale, o_zp, qmin, qmax)
        return y
    if not x.is_cuda:
        _cpu_route_allowed()
    with torch.no_grad():
        rows = src_rows.to(device=x.device, dtype=torch.int64).clamp(0, max(h - 1, 0))
        cols = src_cols.to(device=x.device, dtype=torch.int64).clamp(0, max(w - 1, 0))
        moved = x.index_select(1, rows).index_select(2, cols)
        return fq_codes(dequantize_codes(moved, a_scale, a_zp), None, None, None, qmin, qmax, o_scale, o_zp).contiguous()


def code_table(fn, in_form, out_form, device):
    """The byte table of an elementwise function between two holders: ``fn`` applied to the output of a holder A of the form
    ``in_form = (scale, zero_point, qmin, qmax)`` and coded by a holder B of ``out_form`` (likewise), as a uint8 tensor [256] on
    ``device`` indexed by the RAW byte of A's code (an int8 code c at entry ``c & 0xff``) and holding the raw byte of B's code.
    A's float32 output is ``dequantize_codes`` of its codes bit for bit, so it takes at most 256 values; the table is

        fq_codes(fn(dequantize_codes(arange(256, uint8).view(A's type), s_a, z_a)), None, None, None, qmin_b, qmax_b, s_b, z_b)

    -- the replaced call itself, run on ``device`` on a fresh copy of the 256 values under ``no_grad``, and B's own coding
    function, so that NaN and infinite results are coded exactly as B codes them.  The table is the definition of the node that
    applies it (``codes_table``).  TypeError if ``fn`` does not return a float32 tensor of shape [256]."""
    a_scale, a_zp, a_qmin, a_qmax, a_tdt, _ = _out_form(in_form)
    o_scale, o_zp, qmin, qmax, tdt, _ = _out_form(out_form)
    _check_form("code_table", a_tdt, a_zp, a_scale, "the input's zero point {}", "the input's scale")
    _check_form("code_table", tdt, o_zp, o_scale, "the output's zero point {}", "the output's scale")
    device = torch.device(device)
    if device.type == "cpu":
        _cpu_route_allowed()
    with torch.no_grad():
        raw = torch.arange(256, dtype=torch.int16, device=device).to(torch.uint8)
        x = dequantize_codes(raw.view(a_tdt), a_scale, a_zp)
        y = fn(x.clone())
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or tuple(y.shape) != (256,):
            got = f"{y.dtype} {tuple(y.shape)}" if isinstance(y, torch.Tensor) else type(y).__name__
            raise TypeError(f"code_table: fn must return a float32 tensor of shape [256], got {got}")
        codes = fq_codes(y.to(device).contiguous(), None, None, None, qmin, qmax, o_scale, o_zp)
        return codes.view(torch.uint8).contiguous()


def codes_table(codes, table, out_dtype):
    """``table[raw byte of codes]`` as codes of ``out_dtype`` (torch.int8 / torch.uint8): an elementwise function between two
    holders applied to int8 / uint8 ``codes`` of any shape through its byte table (``code_table``; uint8 [256] on the codes'
    device).  The result has the codes' shape and, for dense tensors, their strides.  GPU tensors take one launch of
    mctq_codes_table over the storage (1 byte read and 1 written per element; any element count, no channel rule); a GPU tensor
    that is not dense, or whose first byte is not 16-byte aligned, is compacted first.  CPU tensors take
    ``table[codes.view(uint8).long()].view(out_dtype)``: the same bytes."""
    if not _is_codes(codes):
        raise TypeError("codes_table takes int8 / uint8 codes")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or tuple(table.shape) != (256,):
        raise TypeError("codes_table: the table must be a uint8 tensor of shape [256]")
    if out_dtype not in (torch.int8, torch.uint8):
        raise TypeError(f"codes_table: out_dtype must be torch.int8 or torch.uint8, got {out_dtype}")
    if table.device != codes.device:
        raise RuntimeError(f"codes_table: the table must be on the codes' device, got {table.device} and {codes.device}")
    if codes.is_cuda:
        x = codes if _is_dense(codes) else codes.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()                                       # (preserve_format: a dense tensor keeps its strides)
        y = torch.empty_like(x, dtype=out_dtype)
        t = _contiguous(table)                                  # named: it must outlive the launch
        if x.numel():
            _gpu_call("mctq_codes_table", x, x.data_ptr(), _code_of(x), y.data_ptr(),
                      native.CODE_U8 if out_dtype == torch.uint8 else native.CODE_I8, x.numel(), t.data_ptr())
        return y
    _cpu_route_allowed()
    return table[codes.view(torch.uint8).long()].view(out_dtype)


def codes_mul(a, g, out_form, gate_form=None):
    """``torch.mul`` of two holder outputs on activation codes, in the form of the holder behind it.  ``a = (codes, scale,
    zero_point)``, int8 / uint8 codes ``[.., C]`` (channels last); ``g = (tensor, scale, zero_point)``, codes likewise or, with
    ``gate_form = (qmin, qmax)`` (the clamp domain of g's quantizer), raw float32 values; ``out_form = (scale, zero_point, qmin,
    qmax)``.  Returns contiguous codes of ``_code_dtype(qmin, qmax)`` in the broadcast shape of the two:

        g_codes = g if gate_form is None else fq_codes(g, None, None, None, *gate_form, g_scale, g_zp)
        fq_codes(dequantize_codes(a, a_scale, a_zp) * dequantize_codes(g_codes, g_scale, g_zp), None, None, None, qmin, qmax, s, z)

    -- a holder's float32 output is ``dequantize_codes`` of its codes bit for bit and ``torch.mul`` is one IEEE float32
    multiplication, so these are the codes the holder behind the product of the two holder outputs gives.  GPU tensors with
    ``C % 16 == 0`` take one launch of mctq_codes_mul_nhwc (1 byte read, 1 byte written per element) in three forms: codes of
    the same shape; codes ``[B, 1, .., 1, C]`` next to ``[B, .., C]`` (the gate of a squeeze-and-excitation block, in either
    operand order); float32 values of that gate shape, coded inside the kernel.  Anything else on the GPU -- another ``C``,
    any other broadcast (``[B, H, W, 1]``, ``[1, 1, 1, C]``, operands of different rank), a float32 operand of another shape
    -- and every CPU tensor evaluates the expression above with torch ops, broadcasting as ``torch.mul`` does, which the kernel
    matches byte for byte."""
    (ac, a_scale, a_zp), (gc, g_scale, g_zp) = a, g
    a_scale, a_zp, g_scale, g_zp = float(a_scale), int(a_zp), float(g_scale), int(g_zp)
    o_scale, o_zp, qmin, qmax, tdt, ocode = _out_form(out_form)
    if not _is_codes(ac) or ac.dim() < 1:
        raise TypeError("codes_mul takes int8 / uint8 codes [.., C] as its first operand")
    if gate_form is None:
        if not _is_codes(gc) or gc.dim() < 1:
            raise TypeError("codes_mul takes int8 / uint8 codes [.., C] as its second operand, or float32 values with gate_form")
        g_tdt, g_qmin, g_qmax = gc.dtype, 0, 0
    else:
        if not isinstance(gc, torch.Tensor) or gc.dtype != torch.float32 or gc.dim() < 1:
            raise TypeError("codes_mul: gate_form describes a float32 second operand")
        g_qmin, g_qmax = int(gate_form[0]), int(gate_form[1])
        g_tdt, _ = _code_dtype(g_qmin, g_qmax)
    if gc.device != ac.device:
        raise RuntimeError(f"codes_mul: operands must share the device, got {ac.device} and {gc.device}")
    for dt, z, what in ((ac.dtype, a_zp, "first"), (g_tdt, g_zp, "second"), (tdt, o_zp, "output")):
        _check_form("codes_mul", dt, z, zp_words=f"the zero point {{}} of the {what} form")
    _check_form("codes_mul", None, scale=(a_scale, g_scale, o_scale))

    def gate_of(big, small):
        """small is [B, 1, .., 1, C] next to big [B, .., C]: the pixels per gate row, else None."""
        if small.dim() != big.dim() or big.dim() < 3 or small.shape[0] != big.shape[0] or small.shape[-1] != big.shape[-1]:
            return None
        return math.prod(big.shape[1:-1]) if all(e == 1 for e in small.shape[1:-1]) else None

    n = None                                                     # the kernel's gate_pixels; None: the torch route
    if ac.is_cuda and ac.shape[-1] > 0 and ac.shape[-1] % 16 == 0:
        if gc.shape == ac.shape:
            n = 0 if gate_form is None else 1                    # (float32 values: every pixel its own gate row)
        elif gate_of(ac, gc) is not None:
            n = gate_of(ac, gc)
        elif gate_form is None and gate_of(gc, ac) is not None:   # the gate first: the multiplication is commutative
            n = gate_of(gc, ac)
            ac, a_scale, a_zp, gc, g_scale, g_zp, g_tdt = gc, g_scale, g_zp, ac, a_scale, a_zp, ac.dtype
    if n is not None:
        out = torch.empty(ac.shape, dtype=tdt, device=ac.device)
        if out.numel() == 0:
            return out
        ak, gk = _contiguous(ac), _contiguous(gc)               # named: they must outlive the launch
        _gpu_call("mctq_codes_mul_nhwc", ak, ak.data_ptr(), _code_of(ak), a_scale, a_zp, gk.data_ptr(),
                  native.CODE_U8 if g_tdt == torch.uint8 else native.CODE_I8, g_scale, g_zp, int(gate_form is not None), g_qmin,
                  g_qmax, n, out.data_ptr(), ocode, ak.numel() // ak.shape[-1], ak.shape[-1], o_scale, o_zp, qmin, qmax)
        return out
    if not ac.is_cuda:
        _cpu_route_allowed()
    with torch.no_grad():
        if gate_form is not None:
            gc = fq_codes(gc, None, None, None, g_qmin, g_qmax, g_scale, g_zp)
        v = dequantize_codes(ac, a_scale, a_zp) * dequantize_codes(gc, g_scale, g_zp)
        return fq_codes(v.contiguous(), None, None, None, qmin, qmax, o_scale, o_zp).contiguous()


def make_lut_table(lut_values, mult: float, cmin: float, cmax: float, device):
    """Device copy of the codebook's decision table (see include/mctq_hip.h), or None.

    Built once per quantizer at construction; needs the native library only when a GPU is the
    working device."""
    if torch.device(device).type != "cuda":
        return None
    table = native.build_lut_table(lut_values, mult, cmin, cmax)
    if table is None:
        return None
    return torch.from_numpy(table).to(device)


_index_tables = {}


def make_lut_index_table(lut_values, mult: float, cmin: float, cmax: float, device):
    """Device copy of the codebook's INDEX decision table (include/mctq_hip.h: mctq_lut_build_index_table), or None
    (CPU working device, non-integer codebook, clip range too wide: the literal index scan is used then).  Cached per
    codebook contents, domain and device: quantizers that share a codebook share the table."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return None
    import numpy as np
    lut = np.ascontiguousarray(np.asarray(lut_values, dtype=np.float32).reshape(-1))
    key = (lut.tobytes(), float(mult), float(cmin), float(cmax), str(dev))
    if key in _index_tables:
        return _index_tables[key]
    table = native.build_lut_index_table(lut, mult, cmin, cmax)
    out = None if table is None else torch.from_numpy(table).to(dev)
    if len(_index_tables) > 256:
        _index_tables.clear()
    _index_tables[key] = out
    return out


def _unpacked_shape(codes):
    return tuple(codes.shape[:-1]) + (codes.shape[-1] * 2,) if codes.dim() and codes.is_contiguous() \
        else (codes.numel() * 2,)


def _check_packed4_layout(shape, axis, what: str):
    """The layouts the 4-bit kernels take (include/mctq_hip.h), for a CONTIGUOUS tensor of ``shape``."""
    n = 1
    for s in shape:
        n *= s
    if axis is None:
        ok = n % 8 == 0
    else:
        inner = 1
        for s in shape[axis + 1:]:
            inner *= s
        ok = inner % 8 == 0 or (inner == 1 and shape[axis] % 8 == 0)
    if not ok:
        raise ValueError(f"{what}: 4-bit codes need a multiple of 8 elements per tensor, or per channel row (or, with the "
                         f"channels on the last axis, a multiple of 8 channels); got shape {tuple(shape)}, axis {axis}")


def lut_codes(x, lut, thresholds, axis, eps: float, thr_div: float, mult: float, cmin: float, cmax: float,
              index_table=None, packed4: bool = False, step_round: int = 0):
    """Codebook-index codes of the LUT quantizers as uint8 (extension, not in the reference).

    ``code = argmin_j |clip((x / fl32(thr + eps)) * mult, cmin, cmax) - lut[j]|`` -- the index ``torch.argmin`` returns
    in the reference's chain (first minimum in list order, 0 for a NaN input); ``lut_decode`` of it is bit-identical to
    the fake-quantized tensor.  ``axis`` None = per tensor (``thr_div`` is the host copy of the divisor), otherwise
    ``thresholds`` float32 [C] and ``eps``.  ``index_table``: ``make_lut_index_table``'s, or None (literal scan).
    ``packed4`` (at most 16 codebook entries): two codes per byte, element 2j of the storage order in the low nibble, as
    ``pack4`` (last dimension halved for contiguous tensors).  CPU tensors: the same definition with torch ops."""
    n_lut = lut.numel()
    if n_lut > 256:
        raise ValueError(f"codebook-index codes are 8-bit: at most 256 codebook entries, got {n_lut}")
    if packed4:
        if n_lut > 16:
            raise ValueError(f"4-bit codes take codebooks of at most 16 entries, got {n_lut}")
        if x.numel() % 2:
            raise ValueError("4-bit packing needs an even number of elements")
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"lut_codes: codebook-index codes are produced from float32 / float16 / bfloat16 tensors, "
                                  f"got {x.dtype}")
    if axis is not None:
        _check_axis(x, thresholds.numel(), axis)
    if not x.is_cuda:
        # CPU tensors: the definition, literally (quantizer_utils.py:126-134 of the reference, index kept)
        xf = x.float() if step_round == 0 else x          # a float32 threshold tensor promotes the first division
        lut_c = lut.detach().to(x.device).float().reshape(-1)
        if axis is None:
            t = torch.clip((xf / thr_div) * mult, min=cmin, max=cmax)
        else:
            shape = [1] * x.dim()
            shape[axis] = -1
            thr = thresholds.detach().to(x.device).float().reshape(shape)
            t = torch.clip((xf / (thr + eps)) * mult, min=cmin, max=cmax)
        q = torch.argmin(torch.abs(t.unsqueeze(-1) - lut_c), dim=-1).to(torch.uint8)
        return _pack4_as_stored(q, x) if packed4 else q
    dt = _dtype_code(x, "lut_codes")
    if not x.is_contiguous():
        x = _dense_input(x)
    if axis is not None and not packed4 and x.numel() > _SPLIT_ELEMS and thresholds.numel() > 1:
        return _split_rows(x, axis, (thresholds.reshape(-1),), torch.uint8,
                           lambda xp, ps, ax: lut_codes(xp, lut, ps[0], ax, eps, thr_div, mult, cmin, cmax, index_table))
    y, code = _codes_output(x, packed4, torch.uint8, native.CODE_U8, native.CODE_U4)
    lut = _param_on(x, lut, "lut_values", torch.float32)
    tab_ptr, entries = 0, 0
    if index_table is not None:
        index_table = _param_on(x, index_table, "index_table", torch.float32)
        tab_ptr, entries = index_table.data_ptr(), index_table.shape[0] - 1
    if axis is None:
        _gpu_call("mctq_lut_codes_per_tensor", x, x.data_ptr(), y.data_ptr(), x.numel(), dt, code, step_round, thr_div,
                  lut.data_ptr(), n_lut, tab_ptr, entries, mult, cmin, cmax)
    else:
        thresholds = _param_on(x, thresholds, "thresholds", torch.float32)
        outer, c, inner = _channel_view(x, axis)
        _gpu_call("mctq_lut_codes_per_channel", x, x.data_ptr(), y.data_ptr(), outer, c, inner, dt, code, thresholds.data_ptr(),
                  eps, lut.data_ptr(), n_lut, tab_ptr, entries, mult, cmin, cmax)
    return y


def lut_decode(codes, lut, thresholds, axis, thr_mul: float, mult: float, packed4: bool = False, shape=None):
    """float32 tensor ``(lut[codes] / mult) * thr`` of codebook-index codes (``lut_codes``): the fake-quantized tensor, bit
    for bit.  ``axis`` None = per tensor (``thr_mul``), otherwise ``thresholds`` float32 [C].  uint8 codes keep their
    sizes and strides (dense permuted codes are walked in storage order) unless ``shape`` reshapes them; ``packed4`` codes
    are the storage of a CONTIGUOUS tensor of ``shape`` (default: the last dimension doubled)."""
    if codes.dtype != torch.uint8:
        raise ValueError(f"codebook-index codes are uint8 tensors, got {codes.dtype}")
    n_lut = lut.numel()
    if n_lut > 256 or (packed4 and n_lut > 16):
        raise ValueError(f"{'4-bit' if packed4 else '8-bit'} codes take codebooks of at most {16 if packed4 else 256} "
                         f"entries, got {n_lut}")
    if packed4:
        shape = _unpacked_shape(codes) if shape is None else tuple(shape)
    elif shape is not None:
        shape = tuple(shape)
    if shape is not None:
        n = 1
        for s_ in shape:
            n *= s_
        if n != codes.numel() * (2 if packed4 else 1):
            raise ValueError(f"{codes.numel()} {'bytes of packed ' if packed4 else ''}codes do not fit shape {shape}")
    if packed4:
        if axis is not None:
            _check_axis(torch.empty(shape, device="meta"), thresholds.numel(), axis)
        if codes.is_cuda:
            _check_packed4_layout(shape, axis, "lut_decode")
        c8 = unpack4(codes.contiguous(), False, shape).to(torch.uint8) if not codes.is_cuda else None
    else:
        c8 = codes if shape is None else codes.reshape(shape)
        if axis is not None:
            _check_axis(c8, thresholds.numel(), axis)
    if not codes.is_cuda:
        q = lut.detach().to(codes.device).float().reshape(-1)[c8.long()] / mult
        if axis is None:
            return q * thr_mul
        bshape = [1] * c8.dim()
        bshape[axis] = -1
        return q * thresholds.detach().to(codes.device).float().reshape(bshape)
    lut = _param_on(codes, lut, "lut_values", torch.float32)
    if packed4:
        src = codes if codes.is_contiguous() else codes.contiguous()
        y = torch.empty(shape, dtype=torch.float32, device=codes.device)
        geom = y
        code = native.CODE_U4
    else:
        src = _dense_input(c8)
        if src.numel() > _SPLIT_ELEMS:
            if axis is not None:
                return _split_rows(src, axis, (thresholds.reshape(-1),), torch.float32,
                                   lambda cp, ps, ax: lut_decode(cp, lut, ps[0], ax, thr_mul, mult))
            flat = torch.as_strided(src, (src.numel(),), (1,), src.storage_offset())
            out = torch.empty(src.numel(), dtype=torch.float32, device=src.device)
            step = _SPLIT_ELEMS - _SPLIT_ELEMS % 8
            for a in range(0, src.numel(), step):
                out[a:a + step] = lut_decode(flat[a:a + step], lut, None, None, thr_mul, mult)
            return torch.as_strided(out, src.shape, src.stride())
        y = torch.empty_like(src, dtype=torch.float32)
        geom = src
        code = native.CODE_U8
    if axis is None:
        _gpu_call("mctq_lut_decode_per_tensor", codes, src.data_ptr(), y.data_ptr(), y.numel(), code, lut.data_ptr(), n_lut, mult,
                  thr_mul)
    else:
        thresholds = _param_on(codes, thresholds, "thresholds", torch.float32)
        outer, c, inner = _channel_view(geom, axis)
        _gpu_call("mctq_lut_decode_per_channel", codes, src.data_ptr(), y.data_ptr(), outer, c, inner, code, lut.data_ptr(), n_lut,
                  mult, thresholds.data_ptr())
    return y


def make_lut_steps(lut_values, mult: float, cmin: float, cmax: float, device):
    """Device copy of an integer codebook's sorted threshold list (include/mctq_hip.h: mctq_lut_build_steps), or None.
    The quantizers ask for it only when the decision table does not apply (lut_values_bitwidth > 10)."""
    if torch.device(device).type != "cuda":
        return None
    steps = native.build_lut_steps(lut_values, mult, cmin, cmax)
    if steps is None:
        return None
    return torch.from_numpy(steps).to(device)


# ------------------------------------------------------------------------------------------
# CPU tensors: the ATen ops / op chain the reference itself executes on a CPU tensor
# ------------------------------------------------------------------------------------------

def _cpu_fq_per_tensor(x, scale, zero_point, qmin, qmax):
    return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)


def _cpu_fq_per_channel(x, scales, zero_points, axis, qmin, qmax):
    return torch.fake_quantize_per_channel_affine(x, scales, zero_points, axis, qmin, qmax)


def _cpu_lut(x, lut, thr_div, thr_mul, mult, cmin, cmax):
    # quantizer_utils.py:126-137 on CPU tensors: divide, scale, clip, first-min argmin, gather, rescale
    t = torch.clip((x / thr_div) * mult, min=cmin, max=cmax).unsqueeze(-1)
    idx = torch.argmin(torch.abs(t - lut.reshape([1] * (t.dim() - 1) + [-1])), dim=-1)
    return (lut.flatten()[idx] / mult) * thr_mul


def _cpu_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, step_round: int = 0):
    # step_round == 0: the threshold is a float32 TENSOR in the reference (weights), so a half-precision
    # input is promoted to float32 by the first division; otherwise (activation, Python-float threshold)
    # the chain stays in the input's type until the float32 codebook enters.
    # (a float64 tensor stays float64 either way: the double quotient, clip and distances of ATen's promotion.)
    if step_round == 0 and x.dtype in (torch.float16, torch.bfloat16):
        x = x.float()
    return _cpu_lut(x, lut, thr_div, thr_mul, mult, cmin, cmax)


def _cpu_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax):
    shape = [1] * x.dim()
    shape[axis] = -1
    thr = thresholds.reshape(shape)
    return _cpu_lut(x, lut, thr + eps, thr, mult, cmin, cmax)


def _cpu_grid(x, lo, hi, step, shifted: bool):
    # the reference's export-time chains on a CPU tensor (weights_symmetric...py:67-68, activation_uniform...py:60-64);
    # lo / hi / step: Python floats or broadcastable float32 tensors
    c = torch.where(x < lo, lo, x)
    c = torch.where(x > hi, hi, c)
    if shifted:
        return step * torch.round((c - lo) / step) + lo
    return torch.round(c / step) * step


# ------------------------------------------------------------------------------------------
# torch.library registration (fx tracing / FakeTensor / torch.compile see one opaque op)
# ------------------------------------------------------------------------------------------

_lib_def = torch.library.Library(_LIBNAME, "DEF")
_lib_def.define("fq_per_tensor(Tensor x, float scale, int zero_point, int quant_min, int quant_max) -> Tensor")
_lib_def.define("fq_per_tensor_tqp(Tensor x, Tensor scale, Tensor zero_point, int quant_min, int quant_max) -> Tensor")
_lib_def.define("fq_per_channel(Tensor x, Tensor scales, Tensor zero_points, int axis, int quant_min, "
                "int quant_max) -> Tensor")
_lib_def.define("lut_per_tensor(Tensor x, Tensor lut, float thr_div, float thr_mul, float mult, float clip_min, "
                "float clip_max, int step_round=0) -> Tensor")
_lib_def.define("lut_per_channel(Tensor x, Tensor lut, Tensor thresholds, float eps, int axis, float mult, "
                "float clip_min, float clip_max) -> Tensor")

# decision tables for codebooks that reach the ops without their quantizer (fx graphs): built once per codebook TENSOR
# OBJECT (weak reference + version counter: an address can be reused by another tensor, an object cannot)
_op_books = {}


def _per_codebook(build, lut, mult, cmin, cmax):
    """``build(lut, mult, cmin, cmax)``, once per codebook tensor object and version."""
    import weakref
    key = (build, id(lut), mult, cmin, cmax)
    hit = _op_books.get(key)
    if hit is not None and hit[0]() is lut and hit[1] == lut._version:
        return hit[2]
    if len(_op_books) > 256:
        _op_books.clear()
    val = build(lut, mult, cmin, cmax)
    try:
        _op_books[key] = (weakref.ref(lut), lut._version, val)
    except TypeError:                                   # not weak-referenceable: do not cache
        pass
    return val


def _build_op_table(lut, mult, cmin, cmax):
    lut_np = lut.detach().cpu().numpy()
    table = make_lut_table(lut_np, mult, cmin, cmax, lut.device)
    return table, None if table is not None else make_lut_steps(lut_np, mult, cmin, cmax, lut.device)


def _build_op_steps64(lut, mult, cmin, cmax):
    built = native.build_lut_steps_f64(lut.detach().cpu().numpy(), mult, cmin, cmax)
    return None if built is None else (torch.from_numpy(built[0]).to(lut.device), built[1])


def _op_table(lut, mult, cmin, cmax):
    """(decision table | None, threshold list | None) of a codebook tensor."""
    return _per_codebook(_build_op_table, lut, mult, cmin, cmax)


def _op_steps64(lut, mult, cmin, cmax):
    """(device blob, P) of the DOUBLE threshold list of a codebook tensor for float64 inputs, or None (literal double
    scan).  One device -> host read at the first float64 call: not inside hipGraph capture."""
    return _per_codebook(_build_op_steps64, lut, mult, cmin, cmax)


def _op_hip_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, step_round=0):
    if x.dtype == torch.float64:
        # the schema's float is a double: the activation quantizer's double divisor arrives intact, and a weights
        # quantizer's float32 divisor is the same number either way
        return _hip_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, None, 0, thr_div)
    table, steps = _op_table(lut, mult, cmin, cmax)
    return _hip_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, table, step_round, None, steps)


def _op_hip_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax):
    if x.dtype == torch.float64:
        return _hip_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax, None)
    table, steps = _op_table(lut, mult, cmin, cmax)
    return _hip_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax, table, steps)


def _cpu_fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax):
    return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)


for _name, _gpu, _cpu in (("fq_per_tensor", _hip_fq_per_tensor, _cpu_fq_per_tensor),
                          ("fq_per_tensor_tqp", _hip_fq_per_tensor_tqp, _cpu_fq_per_tensor_tqp),
                          ("fq_per_channel", _hip_fq_per_channel, _cpu_fq_per_channel),
                          ("lut_per_tensor", _op_hip_lut_per_tensor, _cpu_lut_per_tensor),
                          ("lut_per_channel", _op_hip_lut_per_channel, _cpu_lut_per_channel)):
    _lib_def.impl(_name, _gpu, "CUDA")
    _lib_def.impl(_name, _cpu, "CPU")
for _name in ("fq_per_tensor", "fq_per_tensor_tqp", "fq_per_channel"):
    _lib_def.impl(_name, (lambda x, *a: torch.empty_like(x)), "Meta")
for _name in ("lut_per_tensor", "lut_per_channel"):          # the LUT chain's result: float32, contiguous (_lut_result)
    _lib_def.impl(_name, (lambda x, *a: torch.empty(x.shape, dtype=torch.float32, device=x.device)), "Meta")


# ---- autograd: what ATen's operators do at the reference's call sites -----------------------------------------
# torch.fake_quantize_per_{tensor,channel}_affine carry a straight-through backward: the incoming gradient where the
# clamp index q = nearbyint(x * (1.0f / scale)) + zero_point lies inside [quant_min, quant_max], zero elsewhere
# (ATen's *_cachemask kernels record that mask in the forward; here it is recomputed from x in the rare backward, with
# plain torch ops -- this is an inference library, the reference switches gradients off before it calls them:
# weights_symmetric_inferable_quantizer.py:138,146, activation_symmetric_inferable_quantizer.py:112).
# The scale / zero-point tensors get no gradient (nor do they in ATen's tensor-qparams and per-channel operators).
# The LUT chain ends in argmin + gather (quantizer_utils.py:131-137): its result does not depend on x differentiably.

def _ste_mask(x, inv_scale, zero_point, qmin: int, qmax: int):
    q = torch.round(x.detach().float() * inv_scale) + zero_point          # round half to even, as nearbyint
    return (q >= qmin) & (q <= qmax)


def _f32_inverse(scale):
    s = scale if isinstance(scale, torch.Tensor) else torch.tensor(float(scale), dtype=torch.float64)
    return torch.tensor(1.0, dtype=torch.float32, device=s.device) / s.detach().to(torch.float32)    # float32 1.0f / scale


def _ctx_per_tensor(ctx, inputs, output):
    x, scale, zero_point, qmin, qmax = inputs
    ctx.save_for_backward(x)
    ctx.q = (scale, zero_point, qmin, qmax)


def _bwd_per_tensor(ctx, grad):
    (x,) = ctx.saved_tensors
    scale, zero_point, qmin, qmax = ctx.q
    mask = _ste_mask(x, _f32_inverse(scale).to(x.device), zero_point, qmin, qmax)
    return grad * mask, None, None, None, None


def _ctx_per_tensor_tqp(ctx, inputs, output):
    x, scale, zero_point, qmin, qmax = inputs
    ctx.save_for_backward(x, scale, zero_point)
    ctx.q = (qmin, qmax)


def _bwd_per_tensor_tqp(ctx, grad):
    x, scale, zero_point = ctx.saved_tensors
    qmin, qmax = ctx.q
    mask = _ste_mask(x, _f32_inverse(scale.reshape(-1)[:1]), zero_point.reshape(-1)[:1].to(torch.float32), qmin, qmax)
    return grad * mask, None, None, None, None


def _ctx_per_channel(ctx, inputs, output):
    x, scales, zero_points, axis, qmin, qmax = inputs
    ctx.save_for_backward(x, scales, zero_points)
    ctx.q = (axis, qmin, qmax)


def _bwd_per_channel(ctx, grad):
    x, scales, zero_points = ctx.saved_tensors
    axis, qmin, qmax = ctx.q
    shape = [1] * x.dim()
    shape[axis] = -1
    mask = _ste_mask(x, _f32_inverse(scales).reshape(shape), zero_points.to(torch.float32).reshape(shape), qmin, qmax)
    return grad * mask, None, None, None, None, None


def _ctx_nondiff(ctx, inputs, output):
    ctx.mark_non_differentiable(output)


torch.library.register_autograd(f"{_LIBNAME}::fq_per_tensor", _bwd_per_tensor, setup_context=_ctx_per_tensor, lib=_lib_def)
torch.library.register_autograd(f"{_LIBNAME}::fq_per_tensor_tqp", _bwd_per_tensor_tqp, setup_context=_ctx_per_tensor_tqp,
                                lib=_lib_def)
torch.library.register_autograd(f"{_LIBNAME}::fq_per_channel", _bwd_per_channel, setup_context=_ctx_per_channel, lib=_lib_def)
torch.library.register_autograd(f"{_LIBNAME}::lut_per_tensor", lambda ctx, grad: (None,) * 8, setup_context=_ctx_nondiff,
                                lib=_lib_def)
torch.library.register_autograd(f"{_LIBNAME}::lut_per_channel", lambda ctx, grad: (None,) * 8, setup_context=_ctx_nondiff,
                                lib=_lib_def)


def _is_real(x) -> bool:
    return type(x) is torch.Tensor or type(x) is torch.nn.Parameter


def _cpu_route_allowed():
    """CPU tensors run the ATen operators the reference runs on them (BASELINE config 1).  Deployments that
    must never leave the GPU set MCTQ_REQUIRE_HIP=1: a CPU tensor then raises instead."""
    if os.environ.get("MCTQ_REQUIRE_HIP", "0") not in ("", "0"):
        raise RuntimeError("MCTQ_REQUIRE_HIP is set: refusing to quantize a CPU tensor outside the HIP kernels")


def _tracing() -> bool:
    """torch.jit.trace / torch.onnx.export in progress: emit what the reference emits (ATen nodes), never a raw launch."""
    return torch._C._get_tracing_state() is not None


_compiling = torch.compiler.is_compiling      # dynamo / export in progress: the graph must see torch.ops.mctq_amd.*


def _wide(qmin, qmax) -> bool:
    """Clamp domains beyond 2^24 do not fit the kernels' float32 bounds: ATen's operator (the reference's own call) runs."""
    return max(abs(int(qmin)), abs(int(qmax))) > (1 << 24)


def fq_per_tensor(x, scale: float, zero_point: int, qmin: int, qmax: int):
    if _wide(qmin, qmax) and _is_real(x):
        return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)
    if _compiling():
        return torch.ops.mctq_amd.fq_per_tensor(x, scale, zero_point, qmin, qmax)
    f = _FAST if _FAST_READY else _fast_mod()
    if f is not None:
        y = f.fq_per_tensor(x, scale, zero_point, qmin, qmax)
        if y is not NotImplemented:
            return y
    if _is_real(x):
        if _tracing():
            return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)
        if x.is_cuda:
            return _hip_fq_per_tensor(x, scale, zero_point, qmin, qmax)
        if x.device.type == "cpu":
            _cpu_route_allowed()
            return _cpu_fq_per_tensor(x, scale, zero_point, qmin, qmax)
    return torch.ops.mctq_amd.fq_per_tensor(x, scale, zero_point, qmin, qmax)


def fq_per_tensor_tqp(x, scale, zero_point, qmin: int, qmax: int):
    """``torch.fake_quantize_per_tensor_affine(x, scale_tensor, zero_point_tensor, qmin, qmax)``: the parameters are
    1-element tensors (float32 / int32) that the kernel reads on the device."""
    if _wide(qmin, qmax) and _is_real(x):
        return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)
    if _compiling():
        return torch.ops.mctq_amd.fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax)
    f = _FAST if _FAST_READY else _fast_mod()
    if f is not None:
        y = f.fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax)
        if y is not NotImplemented:
            return y
    if _is_real(x):
        if _tracing():
            return torch.fake_quantize_per_tensor_affine(x, scale, zero_point, qmin, qmax)
        if x.is_cuda:
            return _hip_fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax)
        if x.device.type == "cpu":
            _cpu_route_allowed()
            return _cpu_fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax)
    return torch.ops.mctq_amd.fq_per_tensor_tqp(x, scale, zero_point, qmin, qmax)


def fq_per_channel(x, scales, zero_points, axis: int, qmin: int, qmax: int, zero_zps: bool = False):
    if _wide(qmin, qmax) and _is_real(x):
        return torch.fake_quantize_per_channel_affine(x, scales, zero_points, axis, qmin, qmax)
    if _compiling():
        return torch.ops.mctq_amd.fq_per_channel(x, scales, zero_points, axis, qmin, qmax)
    f = _FAST if _FAST_READY else _fast_mod()
    if f is not None:
        y = f.fq_per_channel(x, scales, None if zero_zps else zero_points, axis, qmin, qmax)
        if y is not NotImplemented:
            return y
    if _is_real(x):
        if _tracing():
            return torch.fake_quantize_per_channel_affine(x, scales, zero_points, axis, qmin, qmax)
        if x.is_cuda:
            return _hip_fq_per_channel(x, scales, zero_points, axis, qmin, qmax, zero_zps)
        if x.device.type == "cpu":
            _cpu_route_allowed()
            return _cpu_fq_per_channel(x, scales, zero_points, axis, qmin, qmax)
    return torch.ops.mctq_amd.fq_per_channel(x, scales, zero_points, axis, qmin, qmax)


def fq_batched(items):
    """Affine fake-quantization of a LIST of tensors in one launch (per group of 32 tensors of one storage type).

    ``items``: sequence of ``(x, scales, zero_points | None, axis | None, quant_min, quant_max)``; ``axis`` None =
    per tensor with 1-element device ``scales`` / ``zero_points``.  All tensors dense GPU tensors on one device.
    Returns the list of outputs, each bit-identical to the corresponding single call.  Replaces the per-layer
    quantizer calls of PytorchQuantizationWrapper.forward (pytorch/quantize_wrapper.py:228-240) when a whole
    model's weights are re-quantized together (see pytorch/batching.py)."""
    items = list(items)
    f = _FAST if _FAST_READY else _fast_mod()
    if any(_wide(it[4], it[5]) for it in items):
        f = None
    if f is not None:
        ys = f.fq_batched(items)
        if ys is not NotImplemented:
            return ys
    if all(_is_real(it[0]) and it[0].is_cuda and not _wide(it[4], it[5]) for it in items) and not _tracing():
        return _hip_fq_batched(items)
    out = []
    for x, scales, zps, axis, qmin, qmax in items:            # CPU tensors, traced graphs ...: one by one
        if zps is None:
            zps = torch.zeros(scales.numel(), dtype=torch.int32, device=scales.device)
        if axis is None:
            out.append(fq_per_tensor_tqp(x, scales, zps, qmin, qmax))
        else:
            out.append(fq_per_channel(x, scales, zps, axis, qmin, qmax))
    return out


def lut_per_tensor(x, lut, thr_div: float, thr_mul: float, mult: float, cmin: float, cmax: float, table=None,
                   step_round: int = 0, thr_div64: float = None, steps=None):
    if _compiling():
        return torch.ops.mctq_amd.lut_per_tensor(x, lut, thr_div if thr_div64 is None else thr_div64, thr_mul, mult, cmin,
                                                 cmax, max(step_round, 0))
    if _is_real(x):
        if _tracing():                                        # the reference's own op chain is what gets recorded
            return _cpu_lut_per_tensor(x, lut, thr_div if thr_div64 is None else thr_div64, thr_mul, mult, cmin, cmax,
                                       step_round)
        if x.is_cuda:
            return _hip_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, table, step_round, thr_div64, steps)
        if x.device.type == "cpu":
            _cpu_route_allowed()
            return _cpu_lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, step_round)
    return torch.ops.mctq_amd.lut_per_tensor(x, lut, thr_div, thr_mul, mult, cmin, cmax, max(step_round, 0))


def lut_per_channel(x, lut, thresholds, eps: float, axis: int, mult: float, cmin: float, cmax: float, table=None,
                    steps=None):
    if _compiling():
        return torch.ops.mctq_amd.lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax)
    if _is_real(x):
        if _tracing():
            return _cpu_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax)
        if x.is_cuda:
            return _hip_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax, table, steps)
        if x.device.type == "cpu":
            _cpu_route_allowed()
            return _cpu_lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax)
    return torch.ops.mctq_amd.lut_per_channel(x, lut, thresholds, eps, axis, mult, cmin, cmax)


def grid_per_tensor(x, lo: float, hi: float, step: float, shifted: bool = False):
    """clip -> true division -> round half even -> scale back, one parameter set (export-time arithmetic)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).to(torch.float32)    # noqa: E731  (scalar -> float32, RNE)
    if x.is_cuda:
        if x.dtype is torch.float32:
            return _hip_grid_per_tensor(x, lo, hi, step, shifted)
        # export of a model kept in another storage type (once per export): the reference's op chain on the device
        return _cpu_grid(x, f32(lo).to(x.device), f32(hi).to(x.device), f32(step).to(x.device), shifted)
    _cpu_route_allowed()
    return _cpu_grid(x, f32(lo), f32(hi), f32(step), shifted)


def grid_per_channel(x, los, his, steps, axis: int, shifted: bool = False):
    """Same with float32 parameter vectors along ``axis``."""
    if x.is_cuda and x.dtype is torch.float32:
        return _hip_grid_per_channel(x, los, his, steps, axis, shifted)
    if not x.is_cuda:
        _cpu_route_allowed()
    shape = [1] * x.dim()
    shape[axis] = -1
    los, his, steps = (t.to(x.device).reshape(shape) for t in (los, his, steps))     # non-float32 GPU tensors: see above
    return _cpu_grid(x, los, his, steps, shifted)
