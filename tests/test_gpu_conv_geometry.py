"""The convolution side of the integer consumer on asymmetric geometry and at edge values: mctq_codes_im2col_nhwc,
mctq_codes_im2col_pad_nhwc, mctq_qconv_dw_i8 / _act, mctq_qconv_grouped_i8, mctq_qconv_transposed_i8, mctq_codes_maxpool_nhwc and
the epilogue of mctq_qmatmul_i8 through the raw C ABI, on the cases of tests/test_conv_geometry_cases.py, which proves without a
GPU what they reach and that a kernel with one geometry pair swapped cannot pass them.

Expected values: the loop oracles of the existing tests (numpy); codes are fake_quant_affine(..., return_index=True) of that
float32 value, NaN -> quant_min; behind an activation the float32 chain of that value on the GPU (chain_codes: the expression
documented at ql_act) -- never the kernel's own float32 output.  Bar: equality of every bit or byte of every element, no mask,
no tolerance.  Every output sits in the middle of a 0xA5 frame with 64 guard bytes on each side, which must keep their value;
inside, every byte starts as the complement of its expected value, so an unwritten element shows whatever its expected byte
is.  Every call returns 0, advances mctq_launch_count by exactly one and leaves the launch note the case predicts: the kernel,
the code types, " zp", the output width and the unroll field (9 / 1 for the depthwise instances, the piece size of the grouped
kernel, the phase count of the transposed one, the correction flags of the matmul; "G=" for the padded gather).  The tuning key
im2col_grain is put back to 0 in a ``finally``.

Above the ABI the same geometries go through the Python routes on GPU tensors (equal to their CPU routes), through fused modules
(GPU forward bit-equal to the CPU forward; one geometry per module through the existing oracle-and-float64 helpers, their bounds
as they are) and through QuantizedMaxPool2d.
"""
import numpy as np
import pytest
import torch

import test_conv_geometry_cases as C
from conftest import bits_equal, first_mismatch
from test_conv_consumer import check_conv_against_oracle_and_float64, conv_model, out_hw
from test_dw_consumer import check_dw_against_oracle_and_float64, dw_model
from test_gpu_qlinear_routes import GUARD, GUARD_BYTE, _Frame
from test_grouped_consumer import check_grouped_against_loops_and_float64, grouped_model, piece_size
from test_matmul_consumer import PAIRS
from test_pool_consumer import pot_holder
from test_qlinear_route_cases import EDGE_FORMS, as_bytes
from test_transposed_consumer import out_hw as transposed_out_hw

pytestmark = pytest.mark.gpu

ACT_CODE = {"hardswish": 1, "hardsigmoid": 2}
OPS = {(False, False): "i8 x i8", (True, False): "u8 x i8", (False, True): "i8 x u8", (True, True): "u8 x u8"}


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert (GUARD, GUARD_BYTE) == (64, 0xA5)
    return native.load()


def _dev(v):
    """A read-only numpy operand on the GPU (a fresh allocation: 16-byte aligned), or None."""
    if v is None:
        return None
    t = torch.from_numpy(np.array(v)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _form_args(form):
    """(y_code_dtype, y_scale, y_zero_point, y_quant_min, y_quant_max) of the entry points whose y_code_dtype < 0 means float32."""
    from mct_quantizers_amd.hip import native
    if form is None:
        return -1, 1.0, 0, 0, 0
    return (native.CODE_U8 if form[2] >= 0 else native.CODE_I8), form[0], form[1], form[2], form[3]


def _code(u8):
    from mct_quantizers_amd.hip import native
    return native.CODE_U8 if u8 else native.CODE_I8


def _framed(lib, what, want, item, note, call):
    """One call of an entry point on a framed output: rc == 0, exactly one launch, the note, the expected bytes."""
    from mct_quantizers_amd.hip import native
    assert want.dtype == np.uint8 and want.ndim == 1
    fr = _Frame(want)
    count = native.launch_count()
    rc = call(fr.ptr())
    assert rc == 0, f"{what}: {lib.mctq_last_error()}"
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: took {text}, expected {note}"
    fr.check(f"{what} [{text}]", item)


def _note(name, op, out_bytes, u):
    return f"{name}<{op},in1B,out{out_bytes}B,U={u},NT=0>"


def _conv_op(u8, zp, act=None):
    return f"{'u8' if u8 else 'i8'} x i8{' zp' if zp else ''}{'' if act is None else ' ' + act}"


# ------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------

def _gather(lib, entry, note, codes, geometry, pad_code, want, what):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = geometry
    b, h, w, c = codes.shape
    assert want.shape[0] == b * np.prod(out_hw(h, w, *geometry))
    x = _dev(codes)
    _framed(lib, what, want.reshape(-1).view(np.uint8), 1, note,
            lambda y: getattr(lib, entry)(x.data_ptr(), y, b, h, w, c, kh, kw, sh, sw, ph, pw, dh, dw, pad_code, _stream()))


def _dw(lib, case, bias, form, want, what, act=None):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case["geometry"]
    b, h, w, c = case["a"].shape
    u8 = case["a"].dtype == np.uint8
    a, wc, ws, zw, bias = (_dev(v) for v in (case["a"], case["w"], case["ws"], case["zw"], bias))
    head = (a.data_ptr(), _code(u8), case["za"], case["sa"], wc.data_ptr(), ws.data_ptr(), _ptr(zw), _ptr(bias))
    tail = (b, h, w, c, kh, kw, sh, sw, ph, pw, dh, dw, _stream())
    note = _note("qconv_dw", _conv_op(u8, zw is not None, act), 4 if form is None else 1, 9 if (kh, kw) == (3, 3) else 1)
    if act is None:
        call = lambda y: lib.mctq_qconv_dw_i8(*head, y, *_form_args(form), *tail)                       # noqa: E731
    else:
        call = lambda y: lib.mctq_qconv_dw_i8_act(*head, y, *_form_args(form), ACT_CODE[act], *tail)    # noqa: E731
    _framed(lib, what, want, 4 if form is None else 1, note, call)


def _grouped(lib, case, bias, form, want, what):
    from mct_quantizers_amd import consumers
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case["geometry"]
    b, h, w, c = case["a"].shape
    o, G = case["w"].shape[0], case["groups"]
    u8 = case["a"].dtype == np.uint8
    a, ws, zw, bias = (_dev(v) for v in (case["a"], case["ws"], case["zw"], bias))
    packed, rowsum = consumers.pack_grouped_weights(_dev(case["w"]), G)
    assert packed.data_ptr() % 16 == 0 and rowsum.data_ptr() % 16 == 0
    note = _note("qconv_grouped", _conv_op(u8, zw is not None), 4 if form is None else 1, piece_size(c // G))
    _framed(lib, what, want, 4 if form is None else 1, note,
            lambda y: lib.mctq_qconv_grouped_i8(a.data_ptr(), _code(u8), case["za"], case["sa"], packed.data_ptr(), ws.data_ptr(),
                                                rowsum.data_ptr(), _ptr(zw), _ptr(bias), y, *_form_args(form), b, h, w, c, o, G,
                                                kh, kw, sh, sw, ph, pw, dh, dw, _stream()))


def _transposed(lib, case, bias, form, want, what):
    from mct_quantizers_amd import consumers
    (kh, kw), (sh, sw), (ph, pw), (oph, opw) = case["geometry"]
    b, h, w, c = case["a"].shape
    o = case["w"].shape[0]
    u8 = case["a"].dtype == np.uint8
    assert want.size == b * np.prod(transposed_out_hw(h, w, *case["geometry"])) * o * (4 if form is None else 1)
    a, ws, zw, bias = (_dev(v) for v in (case["a"], case["ws"], case["zw"], bias))
    packed, rowsum = consumers.pack_transposed_weights(_dev(case["w"]), (sh, sw))
    assert packed.data_ptr() % 16 == 0 and rowsum.data_ptr() % 16 == 0
    note = _note("qconv_transposed", _conv_op(u8, zw is not None), 4 if form is None else 1, sh * sw)
    _framed(lib, what, want, 4 if form is None else 1, note,
            lambda y: lib.mctq_qconv_transposed_i8(a.data_ptr(), _code(u8), case["za"], case["sa"], packed.data_ptr(), ws.data_ptr(),
                                                   rowsum.data_ptr(), _ptr(zw), _ptr(bias), y, *_form_args(form), b, h, w, c, o,
                                                   kh, kw, sh, sw, ph, pw, oph, opw, _stream()))


# ------------------------------------------------------------------------------------------------
# 1. asymmetric geometries through the raw C ABI
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [True, False])
def test_im2col_on_asymmetric_geometries(lib, u8):
    n = 0
    for case in C.gather_cases(C.IM2COL_CHANNELS):
        if case[0] != u8:
            continue
        _, ch, g, pad_code = case
        codes, want = C.gather_case(*case)
        assert want.shape[1] == g[0][0] * g[0][1] * ch                     # C % 16 == 0: no pad columns
        _gather(lib, "mctq_codes_im2col_nhwc", _note("codes_im2col", "byte gather", 1, 1), codes, g, pad_code, want, f"im2col {case}")
        n += 1
    assert 2 * n == C.N_GATHER


@pytest.mark.parametrize("u8", [True, False])
def test_padded_gather_on_asymmetric_geometries(lib, u8):
    """C = 3, 12, 24, 32 under im2col_grain 0 (by rule), 1 and, where C % 4 == 0, 4: chunks that straddle taps, wrap into the next
    kernel row and end in the tail behind K."""
    from mct_quantizers_amd.hip import native
    n = 0
    try:
        for case in C.gather_cases(C.PAD_CHANNELS):
            if case[0] != u8:
                continue
            _, ch, g, pad_code = case
            codes, want = C.gather_case(*case)
            for grain in C.grains(ch):
                native.set_tuning("im2col_grain", grain)
                op = f"padded gather G={grain or (4 if ch % 4 == 0 else 1)}"
                _gather(lib, "mctq_codes_im2col_pad_nhwc", _note("codes_im2col_pad", op, 1, 1), codes, g, pad_code, want,
                        f"padded gather {case} grain {grain}")
                n += 1
    finally:
        native.set_tuning("im2col_grain", 0)
    assert 2 * n == C.N_PAD_LAUNCHES


@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
def test_depthwise_on_asymmetric_geometries(lib, u8, codes_out):
    form = C.CODE_FORMS[u8] if codes_out else None
    n = 0
    for case in C.dw_cases():
        if case[0] != u8:
            continue
        c = C.dw_case(*case)
        _dw(lib, c, c["bias"], form, C.code_bytes(c["want"], form), f"depthwise {case} out={form}")
        n += 1
    assert 2 * n == C.N_DW


@pytest.mark.parametrize("act", C.ACTS)
def test_depthwise_with_an_activation_on_asymmetric_geometries(lib, act):
    """Expected: the float32 chain ON THE GPU of the loops' float32 value -- ATen's activation, then the holder's codes."""
    n = 0
    for case in C.act_cases():
        if case[0] != act:
            continue
        _, u8, kind = case
        c, form = C.act_case(act, u8), C.ACT_FORMS[act][kind]
        want = C.chain_codes(_dev(c["want"]), act, form).cpu().numpy()
        assert len(np.unique(want)) > 8
        _dw(lib, c, c["bias"], form, as_bytes(want, form), f"depthwise {case}", act=act)
        n += 1
    assert 2 * n == C.N_ACT


@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("si", range(len(C.GROUP_SHAPES)))
def test_grouped_on_asymmetric_geometries(lib, si, u8, codes_out):
    form = C.CODE_FORMS[u8] if codes_out else None
    n = 0
    for case in C.grouped_cases(si):
        if case[0] != u8:
            continue
        c = C.grouped_case(*case)
        _grouped(lib, c, c["bias"], form, C.code_bytes(c["want"], form), f"grouped {case} out={form}")
        n += 1
    assert 2 * n == C.N_GROUPED


@pytest.mark.parametrize("u8", [True, False])
def test_maxpool_on_asymmetric_geometries(lib, u8):
    from mct_quantizers_amd.hip import native
    n = 0
    for case in C.pool_cases():
        if case[0] != u8:
            continue
        _, ch, g = case
        (kh, kw), (sh, sw), (ph, pw), (dh, dw), ceil_mode = g
        codes, want = C.pool_case(*case)
        x = _dev(codes)
        b, h, w, _ = codes.shape
        ho, wo = want.shape[1:3]
        _framed(lib, f"max pool {case}", want.reshape(-1).view(np.uint8), 1, _note("codes_maxpool", "u8 max" if u8 else "i8 max", 1, 1),
                lambda y: lib.mctq_codes_maxpool_nhwc(x.data_ptr(), y, native.CODE_U8 if u8 else native.CODE_I8, b, h, w, ch, kh, kw,
                                                      sh, sw, ph, pw, dh, dw, int(ceil_mode), ho, wo, _stream()))
        n += 1
    assert 2 * n == C.N_POOL


# ------------------------------------------------------------------------------------------------
# 2. edge values of every epilogue
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("kind", C.EDGE_KINDS)
def test_edge_values_of_the_convolution_epilogues(lib, kind, u8):
    """Rounding ties, both clamps, NaN / +inf / -inf through the bias (codes quant_min, quant_max, quant_min), signed zeros and
    subnormal scales and outputs (the oracle keeps subnormals, and it is the contract): float32 and code outputs."""
    c = C.edge_case(kind, u8)
    launch_of = {"dw": _dw, "grouped": _grouped, "transposed": _transposed}[kind]
    n = 0
    for launch, fi, form in C.edge_forms():
        _, want = C.edge_expected(kind, u8, launch, fi)
        launch_of(lib, c, c["edge_bias"] if launch == "bias" else None, form, want, f"{kind} u8={u8} {launch} out={form}")
        n += 1
    assert n == len(EDGE_FORMS["plain"]) + len(EDGE_FORMS["bias"]) == 10


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("act", C.ACTS)
def test_edge_values_of_the_depthwise_activation(lib, act, u8):
    """The bias launch of the depthwise edge problem behind both activations: a NaN, both infinities, -0.0 and subnormals enter
    ql_act; expected is the float32 chain on the GPU of the oracle's float32 value."""
    c = C.edge_case("dw", u8)
    y = _dev(C.edge_float("dw", u8, "bias"))
    for kind, form in C.ACT_FORMS[act].items():
        want = C.chain_codes(y, act, form).cpu().numpy()
        assert int(want.min()) == form[2] and int(want.max()) == form[3]
        _dw(lib, c, c["edge_bias"], form, as_bytes(want, form), f"depthwise edge u8={u8} {act} {kind}", act=act)


@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_edge_values_of_the_matmul_epilogue(lib, a_u8, b_u8, transposed_b):
    """M = 17, N = 32, K = 80, a_scale * b_scale = 0.5: ties, the 4-bit clamps, exact zeros; the four code-type pairs carry the
    four values of the correction flags."""
    p = C.matmul_problem(a_u8, b_u8)
    M, N, K = C.MATMUL_SHAPE
    a = _dev(p["a"])
    b = _dev(p["b"] if transposed_b else np.ascontiguousarray(p["b"].T))
    b_rows = K if transposed_b else N                                      # b's row stride: [N, K] or [K, N]
    for fi, form in enumerate(EDGE_FORMS["plain"]):
        _, want = C.matmul_expected(a_u8, b_u8, fi)
        note = _note("qmatmul_nt" if transposed_b else "qmatmul_nn", OPS[a_u8, b_u8], 4 if form is None else 1, p["flags"])
        _framed(lib, f"matmul {OPS[a_u8, b_u8]} out={form}", want, 4 if form is None else 1, note,
                lambda y: lib.mctq_qmatmul_i8(a.data_ptr(), _code(a_u8), p["za"], C.MATMUL_SCALES[0], 0, 0, K,
                                              b.data_ptr(), _code(b_u8), p["zb"], C.MATMUL_SCALES[1], 0, 0, b_rows, int(transposed_b),
                                              y, *_form_args(form), 1, 1, M, N, K, _stream()))


# ------------------------------------------------------------------------------------------------
# 3. the same geometries above the ABI
# ------------------------------------------------------------------------------------------------

def test_the_gathers_through_python_on_gpu_tensors_equal_their_cpu_route():
    from mct_quantizers_amd.hip import native, ops
    for channels, pad_to, name in ((C.IM2COL_CHANNELS, 1, "codes_im2col<"), (C.PAD_CHANNELS, 16, "codes_im2col_pad<")):
        for u8, ch, g, pad_code in C.gather_cases(channels):
            codes, want = C.gather_case(u8, ch, g, pad_code)
            K = g[0][0] * g[0][1] * ch
            n0 = native.launch_count()
            y = ops.codes_im2col(_dev(codes), *g, pad_code, pad_to=pad_to)
            launch = native.last_launch()
            assert native.launch_count() == n0 + 1 and launch.startswith(name if ch % 16 else "codes_im2col<"), launch
            cpu = ops.codes_im2col(torch.from_numpy(codes.copy()), *g, pad_code, pad_to=pad_to)
            assert y.dtype == cpu.dtype and torch.equal(y.cpu(), cpu), (u8, ch, g, pad_to)
            assert np.array_equal(cpu.numpy(), want if pad_to == 16 else want[:, :K])


@pytest.mark.parametrize("u8", [True, False])
def test_the_convolutions_through_python_on_gpu_tensors_equal_their_cpu_routes(u8):
    from mct_quantizers_amd.hip import native
    form = C.CODE_FORMS[u8]
    runs = [(C.dw_run, C.dw_case(*case), "qconv_dw<") for case in C.dw_cases() if case[0] == u8]
    runs += [(C.grouped_run, C.grouped_case(*case), "qconv_grouped<") for si in range(len(C.GROUP_SHAPES))
             for case in C.grouped_cases(si) if case[0] == u8]
    for run, c, name in runs:
        n0 = native.launch_count()
        y = run(c, "cuda")
        assert native.launch_count() == n0 + 1 and native.last_launch().startswith(name), native.last_launch()
        cpu = run(c, "cpu").numpy()
        assert bits_equal(y.cpu().numpy(), cpu) and bits_equal(cpu, c["want"]), (name, c["geometry"], first_mismatch(y.cpu().numpy(), cpu))
        assert torch.equal(run(c, "cuda", form).cpu(), run(c, "cpu", form)), (name, c["geometry"])
    assert len(runs) == (C.N_DW + len(C.GROUP_SHAPES) * C.N_GROUPED) // 2


def test_the_max_pool_through_python_on_gpu_tensors_equals_its_cpu_route():
    from mct_quantizers_amd.hip import native, ops
    for u8, ch, g in C.pool_cases():
        codes, want = C.pool_case(u8, ch, g)
        n0 = native.launch_count()
        y = ops.codes_maxpool(_dev(codes), *g)
        assert native.launch_count() == n0 + 1 and native.last_launch().startswith("codes_maxpool<")
        assert torch.equal(y.cpu(), ops.codes_maxpool(torch.from_numpy(codes.copy()), *g)) and np.array_equal(y.cpu().numpy(), want)


# (stride, padding, dilation) of the fused modules: all three asymmetric at once; padding="same" under an asymmetric dilation
MODULE_GEOMETRIES = (dict(stride=(2, 1), padding=(1, 2), dilation=(1, 2)), dict(stride=1, padding="same", dilation=(1, 2)))
MODULES = {"conv": (conv_model, dict(convolutions=True), 16, "QuantizedConv2d", "qlinear", check_conv_against_oracle_and_float64),
           "depthwise": (dw_model, dict(depthwise=True), 16, "QuantizedDepthwiseConv2d", "qconv_dw<", check_dw_against_oracle_and_float64),
           "grouped": (grouped_model, dict(grouped=True), 32, "QuantizedGroupedConv2d", "qconv_grouped<",
                       check_grouped_against_loops_and_float64)}


@pytest.mark.parametrize("family", ["uniform", "lut16"])
@pytest.mark.parametrize("kind", list(MODULES))
def test_fused_modules_on_asymmetric_geometries_equal_their_cpu_forward(kind, family):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    make, switch, channels, cls, launch_name, check = MODULES[kind]
    for i, geometry in enumerate(MODULE_GEOMETRIES):
        kw = dict(k=3, family=family, per_channel=True, bias=i == 0, seed=i, **geometry)
        cpu, gpu = make(**kw), make(**kw).cuda()
        for m in (cpu, gpu):
            assert consumers.fuse_linear_consumers(m, uniform_weights=True, **switch) == 1 and type(m[1]).__name__ == cls
        assert gpu[1].stride == ((2, 1), (1, 1))[i] and gpu[1].dilation == (1, 2) and gpu[1].padding == (1, 2)
        x = torch.randn(C.B, channels, C.H, C.W, generator=torch.Generator().manual_seed(31 + i)) * 1.5
        want = cpu(x)
        y = gpu(x.cuda())
        launch = native.last_launch()
        assert launch.startswith(launch_name) and ((" zp," in launch) == (family == "uniform")), launch
        assert y.is_cuda and y.shape == want.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert bits_equal(y.detach().cpu().numpy(), want.detach().numpy()), (geometry, first_mismatch(y.detach().cpu().numpy(), want.detach().numpy()))
        if i == 0:
            assert tuple(y.shape[2:]) == out_hw(C.H, C.W, *C.ALL_THREE)
            check(gpu[1], x.cuda(), y)


def test_quantized_max_pool2d_on_the_asymmetric_pools():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    for signed in (False, True):
        holder = pot_holder(signed)
        for (k, s, p, d, ceil_mode) in C.POOLS:
            pool = torch.nn.MaxPool2d(k, s, p, d, ceil_mode=ceil_mode)
            qpool = consumers.QuantizedMaxPool2d(pool, holder.activation_holder_quantizer)
            scale, zp, _, _ = qpool.activation_code_params()
            x = torch.randn(C.B, 16, C.H, C.W, generator=torch.Generator().manual_seed(3)) * 2.0
            want = qpool(x)
            n0 = native.launch_count()
            y = qpool(x.cuda())
            assert native.last_launch().startswith("codes_maxpool<") and native.launch_count() >= n0 + 1
            assert y.dtype == (torch.int8 if signed else torch.uint8) and torch.equal(y.cpu(), want)
            assert torch.equal(ops.dequantize_codes(y.cpu(), scale, zp), pool(holder(x)))      # the holder followed by the pool itself
