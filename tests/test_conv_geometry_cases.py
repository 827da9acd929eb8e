"""The cases of tests/test_gpu_conv_geometry.py -- the convolution side of the integer consumer (csrc/mctq_codes_im2col.hip,
mctq_codes_im2col_pad.hip, mctq_qconv_dw.hip, mctq_qconv_grouped.hip, mctq_qconv_transposed.hip, mctq_codes_maxpool.hip and the
epilogue of mctq_qmatmul.hip) on geometries whose height and width components differ and on the edge values of every
epilogue -- and, without a GPU, the proof that they hold what they claim.

Asymmetric geometries.  Every list the convolution tests had holds strides and dilations (1, 1) / (2, 2) only and an unequal
padding only next to kh = 1: ``stride_h`` read where ``stride_w`` belongs, ``dil_h`` for ``dil_w``, or two arguments of a launch
exchanged change no byte any of them compares.  ``ASYMMETRIC`` varies the stride alone, the padding alone, the dilation alone,
all three at once, their mirror, a non-square kernel and a 3 x 5 kernel for the depthwise run-time tap loop, each on
B = 2, H = 6, W = 9; ``POOLS`` are two max pools with unequal stride and dilation.  Expected values are the loop oracles of
the existing tests (dw_loops / dw_epilogue, grouped_loops, im2col_loops and the independent unfold_patches, maxpool_loops),
never a GPU's.  Sensitivity (test_a_swapped_pair_changes_at_least_half_of_the_output): for each of the pairs stride, padding
and dilation there is a case with kh == kw in which only that pair is unequal; the oracle re-evaluated with that one pair
swapped differs, on the extent common to both outputs, in AT LEAST HALF of the elements -- the condition under which a
kernel that swaps the pair cannot pass.

Edge values.  One problem per epilogue implementation, built as tests/test_qlinear_route_cases.py::edge_problem is: a - za in
[-3, 3] with pixel (0, 0, 0) the zero point, weights in {-1, 0, 1}, a_scale = 0.5, and per output channel n the weight scale
EDGE_WS[n % 8] and the bias EDGE_BIAS[n % 8]; every form of EDGE_FORMS (launch "plain" without bias: the rounding ties;
launch "bias": NaN, +inf, -inf, -0.0 and a bias that cancels to subnormals).  Conditions, asserted here on the oracle
alone: every "plain" code form has exact .5 ties, rounded to both sides; it has elements at both clamps, but fewer than
half of all elements there; the "bias" float32 output holds a NaN, +inf, -inf, -0.0 and a subnormal.  The matmul has no
bias and no per-channel scale: its "plain" launch alone, with a_scale * b_scale = 0.5.  Under the recipe its products lie
in [-120, 120] (K = 80 terms of at most 3), so of its forms only the 4-bit domain can be clamped at all: there both clamps
are required, in the 8-bit domains the two extremes +-120 themselves, unclamped.

Codes are fake_quant_affine(..., return_index=True) of the oracle's float32 value with NaN -> quant_min (_want_codes); behind
an activation (mctq_qconv_dw_i8_act) they are test_hard_act_consumer.chain_codes of that value: the float32 chain on the
tensor's device, which is the expression documented at ql_act.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_any_channels_consumer import unfold_patches
from test_conv_consumer import PAD_CODES, im2col_loops, out_hw
from test_dw_consumer import ZERO_POINTS, dw_epilogue, dw_loops, dw_oracle
from test_dw_consumer import run_raw_on as dw_run
from test_grouped_consumer import grouped_loops, grouped_oracle, piece_size
from test_grouped_consumer import run_raw_on as grouped_run
from test_hard_act_consumer import ACTS, chain_codes
from test_hard_act_consumer import OUT_FORMS as ACT_FORMS
from test_matmul_consumer import PAIRS, brute_acc, contract
from test_pool_consumer import maxpool_loops
from test_pool_consumer import out_size as pool_out_size
from test_qlinear_route_cases import EDGE_A_SCALE, EDGE_BIAS, EDGE_FORMS, EDGE_WS, _want_codes, as_bytes
from test_transposed_consumer import run_raw_on as transposed_run
from test_transposed_consumer import transposed_oracle

F32 = np.float32
B, H, W = 2, 6, 9                                             # non-square on purpose
# (kernel, stride, padding, dilation)
STRIDE_ONLY = ((3, 3), (2, 1), (1, 1), (1, 1))
PAD_ONLY = ((3, 3), (1, 1), (2, 1), (1, 1))
DIL_ONLY = ((3, 3), (1, 1), (2, 2), (1, 2))
ALL_THREE = ((3, 3), (2, 1), (1, 2), (1, 2))
MIRROR = ((3, 3), (1, 2), (2, 0), (2, 1))
NON_SQUARE = ((2, 3), (3, 1), (0, 2), (2, 1))
TAP_LOOP = ((3, 5), (1, 3), (3, 1), (1, 1))                   # 15 taps: the depthwise run-time tap loop
ASYMMETRIC = (STRIDE_ONLY, PAD_ONLY, DIL_ONLY, ALL_THREE, MIRROR, NON_SQUARE, TAP_LOOP)
ONE_PAIR = {"stride": STRIDE_ONLY, "padding": PAD_ONLY, "dilation": DIL_ONLY}
PAIR_INDEX = {"stride": 1, "padding": 2, "dilation": 3}
# (kernel, stride, padding, dilation, ceil_mode)
POOLS = (((2, 2), (1, 2), (0, 0), (2, 1), False), ((3, 3), (2, 1), (1, 1), (1, 2), False))
IM2COL_CHANNELS = (16, 32)
PAD_CHANNELS = (3, 12, 24, 32)
DW_CHANNELS = (16, 48)
GROUP_SHAPES = ((4, 4, 8), (8, 12, 4), (16, 80, 2))            # (Cg, Og, G): piece sizes 4, 8, 16; Og = 80: a second N slice
POOL_CHANNELS = (16, 48)
CODE_FORMS = {True: (0.37, 114, 0, 255), False: (0.41, -5, -128, 127)}       # codes out: a uint8 / an int8 quantizer
ACT_GEOMETRY = {"hardswish": ALL_THREE, "hardsigmoid": MIRROR}               # one geometry per activation
A_SCALE = 0.0173


def _flat(geometry):
    return [int(v) for part in geometry for v in (part if isinstance(part, tuple) else (part,))]


def _codes(rng, shape, u8):
    return rng.integers(0, 256, shape).astype(np.uint8).view(np.uint8 if u8 else np.int8)


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def swapped(geometry, pair):
    """``geometry`` with the two components of one pair exchanged."""
    i = PAIR_INDEX[pair]
    return geometry[:i] + (geometry[i][::-1],) + geometry[i + 1:]


def code_bytes(y, form):
    """The bytes a launch must write for the oracle's float32 ``y``: its bits, or its codes of ``form``."""
    if form is None:
        return as_bytes(y, None)
    return as_bytes(_want_codes(y, F32(form[0]), form[1], form[2], form[3]), form)


def grains(C):
    """The settings of the tuning key im2col_grain a channel count takes: by rule, bytes, and dwords where C % 4 == 0."""
    return (0, 1, 4) if C % 4 == 0 else (0, 1)


def chunk_taps(C, kh, kw):
    """Per 16-byte chunk of a patch row in the K order (ky, kx, c), c < C: the taps (ky, kx) its bytes below K belong to --
    what codes_im2col_pad_kernel and grouped_a_chunk walk piece by piece."""
    K = kh * kw * C
    return [sorted({divmod(k // C, kw) for k in range(j, min(j + 16, K))}) for j in range(0, K, 16)]


# ------------------------------------------------------------------------------------------------
# the cases of every launch
# ------------------------------------------------------------------------------------------------

def gather_cases(channels):
    """(code type, C, geometry, pad code): every geometry with each code type and C, the type's three pad codes in turn."""
    n = 0
    for u8 in (True, False):
        for C in channels:
            for g in ASYMMETRIC:
                n += 1
                yield u8, C, g, PAD_CODES[np.uint8 if u8 else np.int8][n % 3]


@functools.lru_cache(maxsize=None)
def gather_case(u8, C, geometry, pad_code):
    """(codes [B, H, W, C], the patch matrix at the pitch Kp = 16 * ceil(K / 16)): unfold_patches, whose K columns must be
    the numpy loops' and whose tail the pad code -- two independent constructions."""
    rng = np.random.default_rng([11, int(u8), C, *_flat(geometry)])
    codes = _codes(rng, (B, H, W, C), u8)
    want = unfold_patches(codes, *geometry, pad_code, 16)
    K = geometry[0][0] * geometry[0][1] * C
    assert np.array_equal(want[:, :K], im2col_loops(codes, *geometry, pad_code)) and want.shape[1] == -(-K // 16) * 16
    assert np.all(want[:, K:] == np.asarray(pad_code).astype(codes.dtype))
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


def dw_cases():
    """(code type, C, geometry, zero point, weight zero points?, bias?); the zero points of ZERO_POINTS in turn, weight zero
    points and bias on and off with different periods, as test_dw_consumer.raw_cases alternates them."""
    n = 0
    for u8 in (True, False):
        for C in DW_CHANNELS:
            for g in ASYMMETRIC:
                n += 1
                yield u8, C, g, ZERO_POINTS[np.uint8 if u8 else np.int8][n % 3], n % 2 == 0, n % 3 != 0


def _conv_operands(rng, w_shape, n_out, with_zp, with_bias):
    w = rng.integers(-128, 128, w_shape).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, n_out).astype(F32)
    zw = None
    if with_zp:
        zw = rng.integers(-128, 128, n_out).astype(np.int32)
        zw[:4] = (-128, 127, 0, -1)
    bias = rng.normal(0, 2.0, n_out).astype(F32) if with_bias else None
    return w, ws, zw, bias


@functools.lru_cache(maxsize=None)
def dw_case(u8, C, geometry, za, with_zp, with_bias):
    """Seeded operands of one depthwise call and the loops' float32 result; read-only, shared by the CPU and the GPU tests."""
    rng = np.random.default_rng([13, int(u8), C, za + 128, int(with_zp), int(with_bias), *_flat(geometry)])
    a = _codes(rng, (B, H, W, C), u8)
    w, ws, zw, bias = _conv_operands(rng, (*geometry[0], C), C, with_zp, with_bias)
    want = dw_oracle(a, za, A_SCALE, w.astype(np.int64) - (0 if zw is None else zw.astype(np.int64)), ws, bias, geometry)
    return _frozen(dict(a=a, za=za, sa=A_SCALE, w=w, ws=ws, zw=zw, bias=bias, geometry=geometry, want=want))


def act_cases():
    """(activation, code type in, kind of the codes out): mctq_qconv_dw_i8_act on one geometry per activation, C = 16."""
    for act in ACTS:
        for u8 in (True, False):
            for kind in ("u8", "i8"):
                yield act, u8, kind


def act_case(act, u8):
    return dw_case(u8, 16, ACT_GEOMETRY[act], ZERO_POINTS[np.uint8 if u8 else np.int8][1], act == "hardswish", True)


def grouped_cases(si):
    """(code type, row of GROUP_SHAPES, geometry, zero point, weight zero points?, bias?) of one shape."""
    n = si
    for u8 in (True, False):
        for g in ASYMMETRIC:
            n += 1
            yield u8, si, g, ZERO_POINTS[np.uint8 if u8 else np.int8][n % 3], n % 2 == 0, n % 3 != 0


@functools.lru_cache(maxsize=None)
def grouped_case(u8, si, geometry, za, with_zp, with_bias):
    cg, og, G = GROUP_SHAPES[si]
    rng = np.random.default_rng([17, int(u8), si, za + 128, int(with_zp), int(with_bias), *_flat(geometry)])
    a = _codes(rng, (B, H, W, G * cg), u8)
    w, ws, zw, bias = _conv_operands(rng, (G * og, *geometry[0], cg), G * og, with_zp, with_bias)
    w_off = w.astype(np.int64) - (0 if zw is None else zw.astype(np.int64).reshape(-1, 1, 1, 1))
    want = grouped_oracle(a, za, A_SCALE, w_off, ws, bias, G, geometry)
    return _frozen(dict(a=a, za=za, sa=A_SCALE, w=w, ws=ws, zw=zw, bias=bias, groups=G, geometry=geometry, want=want))


def pool_cases():
    for u8 in (True, False):
        for C in POOL_CHANNELS:
            for g in POOLS:
                yield u8, C, g


@functools.lru_cache(maxsize=None)
def pool_case(u8, C, geometry):
    """(codes, the loops' maxima) as test_pool_consumer.pool_case builds them: uint8 over the whole range (the compare must not
    be signed), int8 with a last image that is negative throughout (no padded tap and no start value may win)."""
    rng = np.random.default_rng([19, int(u8), C, *_flat(geometry)])
    if u8:
        codes = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    else:
        codes = rng.integers(-128, 128, (B, H, W, C)).astype(np.int8)
        codes[-1] = rng.integers(-128, 0, (H, W, C)).astype(np.int8)
    want = maxpool_loops(codes, *geometry)
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


N_GATHER, N_PAD_GATHER, N_DW, N_ACT, N_GROUPED, N_POOL = 2 * 2 * 7, 2 * 4 * 7, 2 * 2 * 7, 2 * 2 * 2, 2 * 7, 2 * 2 * 2
N_PAD_LAUNCHES = 2 * 7 * (2 + 3 + 3 + 3)                      # C = 3 takes two grains, C = 12, 24, 32 three


# ------------------------------------------------------------------------------------------------
# edge values of every epilogue
# ------------------------------------------------------------------------------------------------

EDGE_TRANSPOSED = ((3, 3), (2, 1), (1, 0), (1, 0))            # (kernel, stride, padding, output padding)
EDGE_KINDS = ("dw", "grouped", "transposed")
EDGE_OUTPUTS = {"dw": 864, "grouped": 864, "transposed": 4224}
MATMUL_SHAPE = (17, 32, 80)                                   # (M, N, K)
MATMUL_SCALES = (EDGE_A_SCALE, 1.0)
# zero points by (a is uint8, b is uint8): the corrected zero point (z - 128 for uint8 codes) of neither, of a, of b, of both is
# non-zero -- the four values of the launch note's correction flags
MATMUL_ZPS = {(False, False): (0, 0), (True, False): (114, 0), (False, True): (0, 131), (True, True): (114, 131)}


@functools.lru_cache(maxsize=None)
def edge_case(kind, u8):
    """The edge problem of one convolution epilogue (the module's docstring): depthwise C = 16 on ALL_THREE; grouped G = 2,
    Cg = Og = 8 on ALL_THREE; transposed C = O = 16 on EDGE_TRANSPOSED."""
    rng = np.random.default_rng([7, EDGE_KINDS.index(kind), int(u8)])
    za = 114 if u8 else -5
    a = (za + rng.integers(-3, 4, (B, H, W, 16))).astype(np.uint8 if u8 else np.int8)
    a[0, 0, 0] = za
    w_shape = {"dw": (3, 3, 16), "grouped": (16, 3, 3, 8), "transposed": (16, 3, 3, 16)}[kind]
    w = rng.integers(-1, 2, w_shape).astype(np.int8)
    ws = np.asarray([EDGE_WS[n % 8] for n in range(16)], F32)
    edge_bias = np.asarray([EDGE_BIAS[n % 8] for n in range(16)], F32)
    case = dict(a=a, za=za, sa=EDGE_A_SCALE, w=w, ws=ws, zw=None, edge_bias=edge_bias,
                geometry=EDGE_TRANSPOSED if kind == "transposed" else ALL_THREE)
    if kind == "grouped":
        case["groups"] = 2
    return _frozen(case)


def edge_run(kind, case, launch, device="cpu", out_codes=None, act=None):
    """The CPU route (or, on GPU tensors, the Python route) of one launch of an edge problem."""
    c = dict(case, bias=case["edge_bias"] if launch == "bias" else None)
    if kind == "dw" and act is not None:
        from mct_quantizers_amd import consumers
        t = lambda v: None if v is None else torch.from_numpy(v.copy()).to(device)      # noqa: E731
        return consumers.qconv_dw_i8(t(c["a"]), c["za"], c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), *c["geometry"],
                                     out_codes=out_codes, act=act)
    return {"dw": dw_run, "grouped": grouped_run, "transposed": transposed_run}[kind](c, device, out_codes)


@functools.lru_cache(maxsize=None)
def edge_float(kind, u8, launch):
    """The oracle's float32 value of one launch of an edge problem."""
    c = edge_case(kind, u8)
    bias = c["edge_bias"] if launch == "bias" else None
    w = c["w"].astype(np.int64)
    with np.errstate(all="ignore"):
        if kind == "dw":
            y = dw_oracle(c["a"], c["za"], c["sa"], w, c["ws"], bias, c["geometry"])
        elif kind == "grouped":
            y = grouped_oracle(c["a"], c["za"], c["sa"], w, c["ws"], bias, c["groups"], c["geometry"])
        else:
            y = transposed_oracle(c["a"], c["za"], c["sa"], w, c["ws"], bias, c["geometry"])
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def edge_expected(kind, u8, launch, fi):
    """(the oracle's float32 value, the bytes the launch must write) for form ``fi`` of EDGE_FORMS[launch]."""
    y = edge_float(kind, u8, launch)
    return y, code_bytes(y, EDGE_FORMS[launch][fi])


def edge_forms():
    for launch, forms in EDGE_FORMS.items():
        for fi, out in enumerate(forms):
            yield launch, fi, out


@functools.lru_cache(maxsize=None)
def matmul_problem(a_u8, b_u8):
    """a [M, K] with a - za in [-3, 3], b [N, K] (the NT operand; the NN one is its transpose) with b - zb in {-1, 0, 1}.  Row 0
    of a is the zero point (exact zeros), rows 1 and 2 are +3 and -3 throughout and rows 0 and 1 of b +1 and -1: the sums
    +-240, the largest the recipe has."""
    M, N, K = MATMUL_SHAPE
    rng = np.random.default_rng([23, int(a_u8), int(b_u8)])
    za, zb = MATMUL_ZPS[a_u8, b_u8]
    a = (za + rng.integers(-3, 4, (M, K))).astype(np.uint8 if a_u8 else np.int8)
    a[0], a[1], a[2] = za, za + 3, za - 3
    b = (zb + rng.integers(-1, 2, (N, K))).astype(np.uint8 if b_u8 else np.int8)
    b[0], b[1] = zb + 1, zb - 1
    acc = brute_acc(torch.from_numpy(a), za, torch.from_numpy(b), zb, True)
    return _frozen(dict(a=a, za=za, b=b, zb=zb, acc=acc, flags=(za - 128 * a_u8 != 0) + 2 * (zb - 128 * b_u8 != 0)))


@functools.lru_cache(maxsize=None)
def matmul_expected(a_u8, b_u8, fi):
    y = contract(matmul_problem(a_u8, b_u8)["acc"], *MATMUL_SCALES)
    return y, code_bytes(y, EDGE_FORMS["plain"][fi])


# ------------------------------------------------------------------------------------------------
# (a) the CPU routes equal the loop oracles, bit for bit
# ------------------------------------------------------------------------------------------------

def test_the_geometries_are_the_asymmetric_ones():
    for pair, g in ONE_PAIR.items():                                       # kh == kw, and only this pair is unequal
        assert g[0][0] == g[0][1] and [p for p in PAIR_INDEX if g[PAIR_INDEX[p]][0] != g[PAIR_INDEX[p]][1]] == [pair]
    for g in (ALL_THREE, MIRROR):
        assert g[0] == (3, 3) and all(g[i][0] != g[i][1] for i in (1, 2, 3))
    assert all((ALL_THREE[i][0] < ALL_THREE[i][1]) != (MIRROR[i][0] < MIRROR[i][1]) for i in (1, 2, 3))
    assert NON_SQUARE[0][0] != NON_SQUARE[0][1] and TAP_LOOP[0] == (3, 5)
    for g in ASYMMETRIC:
        ho, wo = out_hw(H, W, *g)
        assert ho >= 2 and wo >= 2 and ho != wo, (g, ho, wo)
    for g in POOLS:
        assert g[0][0] == g[0][1] and g[1][0] != g[1][1] and g[3][0] != g[3][1] and g[2][0] == g[2][1]
    assert len(set(ASYMMETRIC)) == 7 and H != W


def test_codes_im2col_on_cpu_equals_both_constructions():
    from mct_quantizers_amd.hip import ops
    n = launches = 0
    for channels, pad_to in ((IM2COL_CHANNELS, 1), (PAD_CHANNELS, 16)):
        for u8, C, g, pad_code in gather_cases(channels):
            codes, want = gather_case(u8, C, g, pad_code)
            K = g[0][0] * g[0][1] * C
            got = ops.codes_im2col(torch.from_numpy(codes.copy()), *g, pad_code, pad_to=pad_to)
            assert got.dtype == (torch.uint8 if u8 else torch.int8) and got.is_contiguous()
            assert np.array_equal(got.numpy(), want if pad_to == 16 else want[:, :K]), (u8, C, g, pad_code, pad_to)
            n += 1
            launches += len(grains(C)) if pad_to == 16 else 0
    assert n == N_GATHER + N_PAD_GATHER and launches == N_PAD_LAUNCHES
    for channels in (IM2COL_CHANNELS, PAD_CHANNELS):                       # every geometry meets every pad code of both types
        seen = {(u8, g, pad) for u8, C, g, pad in gather_cases(channels)}
        assert {(u8, pad) for u8, g, pad in seen} == {(u8, p) for u8 in (True, False) for p in PAD_CODES[np.uint8 if u8 else np.int8]}
    assert all(C % 16 == 0 for C in IM2COL_CHANNELS) and {len(grains(C)) for C in PAD_CHANNELS} == {2, 3}


def test_qconv_dw_i8_on_cpu_equals_the_loops():
    n = 0
    for case in dw_cases():
        c = dw_case(*case)
        y = dw_run(c)
        assert y.shape == c["want"].shape and bits_equal(y.numpy(), c["want"]), (case, first_mismatch(y.numpy(), c["want"]))
        form = CODE_FORMS[case[0]]
        codes = dw_run(c, out_codes=form)
        assert np.array_equal(as_bytes(codes.numpy(), form), code_bytes(c["want"], form)) and len(torch.unique(codes)) > 8, case
        n += 1
    assert n == N_DW
    for g in ASYMMETRIC:                                                   # every geometry: both settings of both, three zero points
        mine = [c for c in dw_cases() if c[2] == g]
        assert {c[4] for c in mine} == {c[5] for c in mine} == {True, False} and len({(c[0], c[3]) for c in mine}) == 4


def test_qconv_dw_i8_with_an_activation_on_cpu_is_the_chain():
    from mct_quantizers_amd import consumers
    n = 0
    for act, u8, kind in act_cases():
        c, form = act_case(act, u8), ACT_FORMS[act][kind]
        t = lambda v: None if v is None else torch.from_numpy(v.copy())      # noqa: E731
        got = consumers.qconv_dw_i8(t(c["a"]), c["za"], c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), *c["geometry"], out_codes=form,
                                    w_zero_points=t(c["zw"]), act=act)
        assert torch.equal(got, chain_codes(t(c["want"]), act, form)) and len(torch.unique(got)) > 8, (act, u8, kind)
        n += 1
    assert n == N_ACT and ACT_GEOMETRY["hardswish"] != ACT_GEOMETRY["hardsigmoid"]


@pytest.mark.parametrize("si", range(len(GROUP_SHAPES)))
def test_qconv_grouped_i8_on_cpu_equals_the_loops(si):
    n = 0
    for case in grouped_cases(si):
        c = grouped_case(*case)
        y = grouped_run(c)
        assert y.shape == c["want"].shape and bits_equal(y.numpy(), c["want"]), (case, first_mismatch(y.numpy(), c["want"]))
        form = CODE_FORMS[case[0]]
        codes = grouped_run(c, out_codes=form)
        assert np.array_equal(as_bytes(codes.numpy(), form), code_bytes(c["want"], form)) and len(torch.unique(codes)) > 8, case
        n += 1
    assert n == N_GROUPED
    for g in ASYMMETRIC:                                                   # over the shapes: both settings of both for every geometry
        mine = [c for s in range(len(GROUP_SHAPES)) for c in grouped_cases(s) if c[2] == g]
        assert {c[4] for c in mine} == {c[5] for c in mine} == {True, False} and len({(c[0], c[3]) for c in mine}) == 6


def test_codes_maxpool_on_cpu_equals_the_loops():
    from mct_quantizers_amd.hip import ops
    n = 0
    for u8, C, g in pool_cases():
        codes, want = pool_case(u8, C, g)
        k, s, p, d, ceil_mode = g
        got = ops.codes_maxpool(torch.from_numpy(codes.copy()), k, s, p, d, ceil_mode)
        assert tuple(got.shape) == want.shape == (B, pool_out_size(H, k[0], s[0], p[0], d[0], False), pool_out_size(W, k[1], s[1], p[1], d[1], False), C)
        assert np.array_equal(got.numpy(), want), (u8, C, g)
        if not u8:
            assert int(got[-1].max()) < 0 and int(got[0].max()) > 100
        n += 1
    assert n == N_POOL


# ------------------------------------------------------------------------------------------------
# (b) sensitivity: one pair swapped changes at least half of the output
# ------------------------------------------------------------------------------------------------

def _share_that_differs(x, y):
    """Of the extent [B, min Ho, min Wo, ...] common to both outputs: the share of elements that differ."""
    ho, wo = min(x.shape[1], y.shape[1]), min(x.shape[2], y.shape[2])
    assert x.shape[0] == y.shape[0] and x.shape[3:] == y.shape[3:] and ho >= 2 and wo >= 2
    return float(np.mean(x[:, :ho, :wo] != y[:, :ho, :wo]))


@pytest.mark.parametrize("pair", list(ONE_PAIR))
def test_a_swapped_pair_changes_at_least_half_of_the_output(pair):
    g = ONE_PAIR[pair]
    other = swapped(g, pair)
    assert other != g and swapped(other, pair) == g
    shares = {}
    for u8 in (True, False):
        dt = np.uint8 if u8 else np.int8
        for C in (3, 16):                                                  # the gathers
            codes, _ = gather_case(u8, C, g, PAD_CODES[dt][1])
            patches = [im2col_loops(codes, *geo, PAD_CODES[dt][1]).reshape(B, *out_hw(H, W, *geo), -1) for geo in (g, other)]
            shares["gather", u8, C] = _share_that_differs(*patches)
        c = next(dw_case(*case) for case in dw_cases() if case[0] == u8 and case[2] == g)
        w = c["w"].astype(np.int64) - (0 if c["zw"] is None else c["zw"].astype(np.int64))
        assert bits_equal(c["want"], dw_epilogue(dw_loops(c["a"], c["za"], w, *g), c["sa"], c["ws"], c["bias"]))
        shares["dw", u8] = _share_that_differs(c["want"], dw_oracle(c["a"], c["za"], c["sa"], w, c["ws"], c["bias"], other))
        assert shares["dw", u8] <= _share_that_differs(dw_loops(c["a"], c["za"], w, *g), dw_loops(c["a"], c["za"], w, *other))
        for si in range(len(GROUP_SHAPES)):
            c = next(grouped_case(*case) for case in grouped_cases(si) if case[0] == u8 and case[2] == g)
            w = c["w"].astype(np.int64) - (0 if c["zw"] is None else c["zw"].astype(np.int64).reshape(-1, 1, 1, 1))
            shares["grouped", u8, si] = _share_that_differs(c["want"], grouped_oracle(c["a"], c["za"], c["sa"], w, c["ws"], c["bias"],
                                                                                    c["groups"], other))
            sums = [grouped_loops(c["a"], c["za"], w, c["groups"], *geo) for geo in (g, other)]
            assert shares["grouped", u8, si] <= _share_that_differs(*sums)                     # (a value differs only where its sum does)
        if pair != "padding":                                              # the pools' paddings are equal
            for pool in POOLS:
                codes, want = pool_case(u8, 16, pool)
                i = PAIR_INDEX[pair]
                assert pool[i][0] != pool[i][1]
                shares["pool", u8, pool] = _share_that_differs(want, maxpool_loops(codes, *swapped(pool[:4], pair), pool[4]))
    assert all(share >= 0.5 for share in shares.values()), {k: v for k, v in shares.items() if v < 0.5}
    assert len(shares) == 2 * (2 + 1 + 3 + (2 if pair != "padding" else 0))


def test_the_mirror_differs_from_the_case_it_mirrors():
    """ALL_THREE and MIRROR differ in every pair: a launch that exchanged all three at once would turn one into (nearly) the
    other, so both are in the list, and every case of one has another expected value than the same operands under the other."""
    for u8 in (True, False):
        c = next(dw_case(*case) for case in dw_cases() if case[0] == u8 and case[2] == ALL_THREE)
        w = c["w"].astype(np.int64) - (0 if c["zw"] is None else c["zw"].astype(np.int64))
        full = tuple(ALL_THREE[i] if i == 0 else ALL_THREE[i][::-1] for i in range(4))
        assert _share_that_differs(c["want"], dw_oracle(c["a"], c["za"], c["sa"], w, c["ws"], c["bias"], full)) >= 0.5


# ------------------------------------------------------------------------------------------------
# (c) reach
# ------------------------------------------------------------------------------------------------

def test_the_cases_reach_every_piece_size_instance_and_chunk_walk():
    assert [piece_size(cg) for cg, _, _ in GROUP_SHAPES] == [4, 8, 16]
    assert [-(-(-(-og // 16) * 16) // 64) for _, og, _ in GROUP_SHAPES] == [1, 1, 2]               # N slices: Og = 80 has a second
    assert all(cg * G <= 48 and cg * G % 16 == 0 for cg, _, G in GROUP_SHAPES)
    # im2col_grain: by rule 4 where C % 4 == 0, else 1; both forced where they apply
    assert {C: grains(C) for C in PAD_CHANNELS} == {3: (0, 1), 12: (0, 1, 4), 24: (0, 1, 4), 32: (0, 1, 4)}
    # the unrolled 3 x 3 instance and the run-time one of the depthwise kernel
    kernels = {g[0] for g in ASYMMETRIC}
    assert (3, 3) in kernels and {(2, 3), (3, 5)} <= kernels
    assert ACT_GEOMETRY["hardswish"][0] == (3, 3)
    # a 16-byte chunk that straddles two taps, one that wraps into the next kernel row, a tail behind K -- in the padded
    # gather (pieces of 1 and 4 bytes) and in the grouped kernel's walk (pieces of 4 and 8 bytes; 16: one piece, no walk)
    for what, widths in (("gather", PAD_CHANNELS), ("grouped", [cg for cg, _, _ in GROUP_SHAPES])):
        for width in widths:
            walks = {g[0]: chunk_taps(width, *g[0]) for g in ASYMMETRIC}
            straddles = any(len(taps) > 1 for chunks in walks.values() for taps in chunks)
            wraps = any(len({ky for ky, _ in taps}) > 1 for chunks in walks.values() for taps in chunks)
            assert straddles == wraps == (width % 16 != 0), (what, width)
            if width % 16:
                for k in ((3, 3), (2, 3), (3, 5)):                          # ... under every kernel size
                    assert any(len({ky for ky, _ in taps}) > 1 for taps in walks[k]), (what, width, k)
        assert any(width % 16 == 0 for width in widths)
    assert {(g[0][0] * g[0][1] * C) % 16 != 0 for C in PAD_CHANNELS for g in ASYMMETRIC} == {True, False}
    assert all((g[0][0] * g[0][1] * cg) % 64 != 0 for cg, _, _ in GROUP_SHAPES for g in ASYMMETRIC)       # a tail behind Kg in every case
    # nothing is larger than a 2 x 6 x 9 x 48 input or a 17 x 32 x 80 product
    assert max(DW_CHANNELS + POOL_CHANNELS + PAD_CHANNELS + IM2COL_CHANNELS) <= 48 and MATMUL_SHAPE == (17, 32, 80)
    # more than one block of 64 pixels / 256 chunks in the stride-1 geometries, and a partly filled last one
    assert B * np.prod(out_hw(H, W, *PAD_ONLY)) == 2 * 8 * 9 and (2 * 8 * 9) % 64 != 0


# ------------------------------------------------------------------------------------------------
# the edge problems hold what they claim, and the CPU routes give the oracle's bytes
# ------------------------------------------------------------------------------------------------

def _ties(y, codes, form):
    """Elements whose value times 1 / scale (scale = 1 in the "plain" forms) is an exact .5 tie inside the clamp domain."""
    assert form[0] == 1.0
    v = y.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (np.abs(v - np.floor(v) - 0.5) == 0) & (codes > form[2]) & (codes < form[3])


def _check_plain_form(y, form, both_clamps, what):
    codes = _want_codes(y, F32(form[0]), form[1], form[2], form[3])
    ties = _ties(y, codes, form)
    v = y.astype(np.float64)
    down, up = codes - form[1] == np.floor(v), codes - form[1] == np.floor(v) + 1
    assert ties.any() and (ties & down).any() and (ties & up).any() and np.all((codes[ties] - form[1]) % 2 == 0), (what, form)
    at_min, at_max = int((codes == form[2]).sum()), int((codes == form[3]).sum())
    if both_clamps:
        assert at_min > 0 and at_max > 0, (what, form, at_min, at_max)
    assert 2 * (at_min + at_max) < codes.size, (what, form, at_min, at_max, codes.size)
    return int(ties.sum()), at_min + at_max


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_edge_problems_of_the_convolutions_hold_what_they_claim(kind):
    tiny = F32(np.finfo(np.float32).tiny)
    for u8 in (True, False):
        c = edge_case(kind, u8)
        assert int(c["a"].astype(np.int64).min()) == c["za"] - 3 and int(c["a"].astype(np.int64).max()) == c["za"] + 3
        assert np.all(c["a"][0, 0, 0] == c["za"]) and set(np.unique(c["w"])) == {-1, 0, 1}
        assert c["ws"].tolist() == [EDGE_WS[n % 8] for n in range(16)] and c["sa"] == EDGE_A_SCALE
        y = edge_float(kind, u8, "plain")
        assert y.size == EDGE_OUTPUTS[kind] and y.shape[-1] == 16
        for fi, form in enumerate(EDGE_FORMS["plain"]):
            if form is not None:
                _check_plain_form(y, form, True, (kind, u8))
        # +0.0 from a positive scale and -0.0 from a negative one, without bias; -0.0 through the bias of -0.0
        bits = y.view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any()
        yb = edge_float(kind, u8, "bias")
        cols = np.arange(16) % 8
        assert np.isnan(yb[..., cols == 0]).all() and np.isposinf(yb[..., cols == 1]).all() and np.isneginf(yb[..., cols == 2]).all()
        assert (yb[..., cols == 3].view(np.uint32) == 0x80000000).any()
        assert ((yb != 0) & (np.abs(yb) < tiny)).any() and ((y != 0) & (np.abs(y) < tiny)).any()          # subnormal outputs
        sc = F32(EDGE_A_SCALE) * c["ws"]
        assert np.all((sc[cols == 2] > 0) & (sc[cols == 2] < tiny))                                         # a subnormal scale
        for fi, form in enumerate(EDGE_FORMS["bias"]):
            if form is None:
                continue
            codes = _want_codes(yb, F32(form[0]), form[1], form[2], form[3])
            assert np.all(codes[..., cols == 0] == form[2]) and np.all(codes[..., cols == 1] == form[3])   # NaN -> quant_min, +inf
            assert np.all(codes[..., cols == 2] == form[2]) and len(np.unique(codes)) > (8 if form[3] > 7 else 4)    # -inf


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_the_cpu_routes_give_the_oracles_bytes_on_the_edge_problems(kind):
    n = 0
    for u8 in (True, False):
        c = edge_case(kind, u8)
        for launch, fi, form in edge_forms():
            _, want = edge_expected(kind, u8, launch, fi)
            got = edge_run(kind, c, launch, "cpu", form).numpy()
            assert np.array_equal(as_bytes(got, form), want), (kind, u8, launch, form)
            n += 1
    assert n == 2 * (4 + 6)


def test_the_depthwise_activation_on_the_edge_problem_on_cpu_is_the_chain():
    for u8 in (True, False):
        c = edge_case("dw", u8)
        y = torch.from_numpy(edge_float("dw", u8, "bias").copy())
        for act in ACTS:
            for kind, form in ACT_FORMS[act].items():
                got = edge_run("dw", c, "bias", "cpu", form, act=act)
                want = chain_codes(y, act, form)
                assert torch.equal(got, want) and int(want.min()) == form[2] and int(want.max()) == form[3], (u8, act, kind)


def test_the_matmul_edge_problem_holds_what_it_claims():
    M, N, K = MATMUL_SHAPE
    assert sorted(p["flags"] for p in (matmul_problem(*pair) for pair in PAIRS)) == [0, 1, 2, 3]
    assert F32(MATMUL_SCALES[0]) * F32(MATMUL_SCALES[1]) == F32(0.5)
    for pair in PAIRS:
        p = matmul_problem(*pair)
        da, db = p["a"].astype(np.int64) - p["za"], p["b"].astype(np.int64) - p["zb"]
        assert da.min() == -3 and da.max() == 3 and set(np.unique(db)) == {-1, 0, 1} and not da[0].any()
        y, _ = matmul_expected(*pair, 0)
        assert y.shape == (M, N) and np.array_equal(y.astype(np.float64), p["acc"] * 0.5)
        assert not y[0].view(np.uint32).any()                                                  # +0.0 throughout row 0
        assert y[1, 0] == 120 == -y[1, 1] == -y[2, 0] and np.abs(y).max() == 120               # the largest the recipe has
        for fi, form in enumerate(EDGE_FORMS["plain"]):
            if form is None:
                continue
            reachable = form[3] - form[1] <= 120 and form[1] - form[2] <= 120                  # |y| <= 120: the 4-bit domain only
            _check_plain_form(y, form, reachable, pair)
            codes = _want_codes(y, F32(form[0]), form[1], form[2], form[3])
            if not reachable:                                                                  # the extremes themselves, unclamped
                assert codes.max() == form[1] + 120 < form[3] and codes.min() == form[1] - 120 > form[2]


@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
def test_qmatmul_i8_on_cpu_gives_the_oracles_bytes_on_the_edge_problem(transposed_b):
    from mct_quantizers_amd import consumers
    for pair in PAIRS:
        p = matmul_problem(*pair)
        a = torch.from_numpy(p["a"].copy())
        b = torch.from_numpy(p["b"].copy() if transposed_b else np.ascontiguousarray(p["b"].T))
        for fi, form in enumerate(EDGE_FORMS["plain"]):
            _, want = matmul_expected(*pair, fi)
            got = consumers.qmatmul_i8(a, (MATMUL_SCALES[0], p["za"]), b, (MATMUL_SCALES[1], p["zb"]), transposed_b=transposed_b,
                                       out_codes=form)
            assert np.array_equal(as_bytes(got.numpy(), form), want), (pair, transposed_b, form)
