"""Average pooling on activation codes: host logic and the CPU route (include/mctq_hip.h: mctq_codes_avgpool_nhwc; hip/ops.py:
codes_avgpool; consumers.QuantizedAvgPool2d and the ``avg_pools`` switch of fuse_linear_consumers / fuse_linear_consumers_fx).

The contract, per output element: S = the exact integer sum of ``code - zp_a`` over the window's taps inside the image, ``div``
PyTorch's divisor, and then in float32, every step rounded once: ``v = S * scale_a``, ``m = v / div``,
``code = clamp(rint(m * (1 / scale_b)) + zp_b, qmin, qmax)``.  The op is pinned byte for byte against plain numpy loops that
compute S and div as integers and apply those three steps in ``np.float32``.

What that equals: where ``scale_a`` and every ``div`` are powers of two, every float32 average pool is exact and the codes are
``torch.equal`` to the float32 chain ``holder B(avg_pool2d(dequantize(codes)))``.  Everywhere else the code is checked against
the exact value ``t`` in float64: it must be ``clamp(rint(t))`` unless ``|frac(t) - 0.5| < 1e-3``, where either neighbour
passes -- the three float32 roundings move t by at most about 255 * 3 * 2^-24 = 5e-5, the band is 20 times that -- and at
most 1 % of the elements of a case with scales that are no powers of two may use that exemption (an element whose two
neighbours clamp to the same code does not count: nothing is exempted there).

A model rewritten with ``avg_pools=True`` is compared bit for bit with the same rewrite without it, on models whose float32
products are exact (tests/test_pool_consumer.py says how: power-of-two scales, no bias, short sums) and whose windows have
power-of-two counts."""
import functools
import operator
import warnings

import numpy as np
import pytest
import torch

from test_conv_consumer import weights_quantizer
from test_join_consumer import _targets
from test_pool_consumer import out_size, pot_conv, pot_holder, unsigned_pot

F = torch.nn.functional

# (kernel or None = global, stride, padding, ceil_mode, count_include_pad, divisor_override), each on B=2 images of 7 x 5 with
# 16 and 48 channels
GEOMETRIES = [((2, 2), (2, 2), (0, 0), False, True, None), ((3, 3), (2, 2), (1, 1), False, True, None),
              ((3, 3), (2, 2), (1, 1), False, False, None), ((3, 3), (1, 1), (1, 1), False, True, None),
              ((2, 2), (2, 2), (1, 1), True, True, None), ((3, 2), (2, 3), (1, 0), False, True, None),
              ((2, 2), (2, 2), (0, 0), False, True, 3), ((1, 1), (1, 1), (0, 0), False, True, None), (None, None, (0, 0), False, True, None)]
# about 300 output pixels of 3 chunks: several 256-lane blocks, the last one partly empty
LARGE = dict(B=3, H=20, W=20, C=48, geometry=((2, 2), (2, 2), (0, 0), False, True, None))
# a 17 x 17 = 289-tap window (more than 257 taps: 16-bit partial sums must be widened), windows over every edge and a whole one
WIDE = dict(B=2, H=17, W=17, C=16, geometry=((17, 17), (8, 8), (8, 8), False, False, None))
# a global 24 x 24 = 576-tap window on one image of one chunk
GLOBAL576 = dict(B=1, H=24, W=24, C=16, geometry=(None, None, (0, 0), False, True, None))
# a global 7 x 7 window (ResNet's head)
GLOBAL49 = dict(B=2, H=7, W=7, C=16, geometry=(None, None, (0, 0), False, True, None))

# ((scale_a, zp_a), (scale_b, zp_b, qmin, qmax)) per input code type; the first of each has power-of-two scales.  (The scales of
# the last pair are chosen so that the reference arithmetic alone keeps every case under the cap on elements next to a tie: the
# smallest cases have 16 and 32 elements, where the cap allows none.)
FORMS = {True: [((0.03125, 0), (0.03125, 0, 0, 255)), ((0.0213, 3), (0.0371, 7, 0, 255)), ((0.0269, 5), (0.0331, -4, -128, 127))],
         False: [((0.03125, 0), (0.03125, 0, -128, 127)), ((0.0223, 3), (0.0367, 7, 0, 255)), ((0.0269, -5), (0.0331, 4, -128, 127))]}


def _pot(v):
    m, _ = np.frexp(np.float32(v))
    return m == 0.5


def avgpool_loops(codes, zp, geometry):
    """codes [B, H, W, C] -> (S int64 [B, Ho, Wo, C], div int64 [Ho, Wo]) by plain loops: S sums ``code - zp`` over the taps
    inside the image, div is the divisor PyTorch documents."""
    k, s, p, ceil_mode, include_pad, override = geometry
    B, H, W, C = codes.shape
    if k is None:
        k, s = (H, W), (H, W)
    ho, wo = out_size(H, k[0], s[0], p[0], 1, ceil_mode), out_size(W, k[1], s[1], p[1], 1, ceil_mode)
    S, div = np.zeros((B, ho, wo, C), np.int64), np.zeros((ho, wo), np.int64)
    wide = codes.astype(np.int64) - zp
    for oy in range(ho):
        for ox in range(wo):
            h0, w0 = oy * s[0] - p[0], ox * s[1] - p[1]
            ys = [iy for iy in range(h0, h0 + k[0]) if 0 <= iy < H]
            xs = [ix for ix in range(w0, w0 + k[1]) if 0 <= ix < W]
            assert ys and xs                             # every window of these geometries has a tap inside the image
            S[:, oy, ox] = wide[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].sum(axis=(1, 2))
            if override is not None:
                div[oy, ox] = override
            elif include_pad:
                div[oy, ox] = (min(h0 + k[0], H + p[0]) - h0) * (min(w0 + k[1], W + p[1]) - w0)
            else:
                div[oy, ox] = len(ys) * len(xs)
    return S, div


def contract_codes(S, div, scale_a, out_form):
    """The contract's three float32 steps on the integer S and div, in np.float32 (each numpy operation rounds once)."""
    scale_b, zp_b, qmin, qmax = out_form
    assert np.abs(S).max() < 2 ** 24
    v = S.astype(np.float32) * np.float32(scale_a)
    m = v / div.astype(np.float32)[None, :, :, None]
    assert m.dtype == np.float32
    q = np.rint(m * (np.float32(1.0) / np.float32(scale_b))) + np.float32(zp_b)
    return np.clip(q, qmin, qmax).astype(np.uint8 if qmin >= 0 else np.int8)


def make_codes(u8, B, H, W, C):
    rng = np.random.default_rng(100 * C + 7 * H + u8)
    return rng.integers(0, 256, (B, H, W, C)).astype(np.uint8) if u8 else rng.integers(-128, 128, (B, H, W, C)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def avg_case(u8, form, geometry, B=2, H=7, W=5, C=16):
    """(codes [B, H, W, C], S, div, the contract's codes), computed once and shared by the CPU and GPU tests; read-only."""
    codes = make_codes(u8, B, H, W, C)
    (scale_a, zp_a), out_form = FORMS[u8][form]
    S, div = avgpool_loops(codes, zp_a, geometry)
    want = contract_codes(S, div, scale_a, out_form)
    for a in (codes, S, div, want):
        a.setflags(write=False)
    return codes, S, div, want


def avg_cases():
    """(u8, form index, geometry, shape keywords) of every pool case."""
    for u8 in (True, False):
        for form in range(3):
            for C in (16, 48):
                for g in GEOMETRIES:
                    yield u8, form, g, dict(C=C)
            for extra in (LARGE, WIDE, GLOBAL576, GLOBAL49):
                shape = dict(extra)
                yield u8, form, shape.pop("geometry"), shape


N_CASES = 2 * 3 * (2 * len(GEOMETRIES) + 4)


@functools.lru_cache(maxsize=None)
def extreme_case(u8, zp):
    """The 289-tap window on saturated inputs: image 0 the type's greatest code throughout, image 1 its least, against a zero
    point at either end, into a form of half the scale -- the outputs reach qmin and qmax, and |S| reaches 255 * 289 > 65535.
    Returns (codes, in_form, out_form, geometry, the contract's codes)."""
    lo, hi = (0, 255) if u8 else (-128, 127)
    codes = np.empty((2, 19, 18, 16), np.uint8 if u8 else np.int8)
    codes[0], codes[1] = hi, lo
    in_form, out_form = (0.0625, zp), (0.03125, 128 if u8 else 0, lo, hi)
    geometry = ((17, 17), (1, 1), (0, 0), False, True, None)
    S, div = avgpool_loops(codes, zp, geometry)
    assert np.abs(S).max() >= 254 * 289
    want = contract_codes(S, div, in_form[0], out_form)
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, in_form, out_form, geometry, want


EXTREMES = [(True, 0), (True, 255), (False, 127), (False, -127)]


def float32_chain(codes, in_form, out_form, geometry):
    """holder B(F.avg_pool2d(dequantize(codes))) as NHWC codes."""
    from mct_quantizers_amd.hip import ops
    k, s, p, ceil_mode, include_pad, override = geometry
    x = ops.dequantize_codes(torch.from_numpy(codes.copy()), *in_form).permute(0, 3, 1, 2).contiguous()
    if k is None:
        k = s = tuple(x.shape[2:])
    y = F.avg_pool2d(x, k, s, p, ceil_mode, include_pad, override)
    return ops.fq_codes(y, None, None, None, out_form[2], out_form[3], out_form[0], out_form[1]).permute(0, 2, 3, 1)


def check_against_the_exact_mean(got, S, div, in_form, out_form):
    """``got`` against the exact value in float64; returns the fraction of elements that used the tie exemption."""
    scale_b, zp_b, qmin, qmax = out_form
    t = S.astype(np.float64) * float(np.float32(in_form[0])) / div.astype(np.float64)[None, :, :, None] / float(np.float32(scale_b)) + zp_b
    lower, upper = np.clip(np.floor(t), qmin, qmax), np.clip(np.floor(t) + 1, qmin, qmax)
    near_tie = (np.abs(t - np.floor(t) - 0.5) < 1e-3) & (lower != upper)
    exact = np.clip(np.rint(t), qmin, qmax)
    g = got.astype(np.float64)
    ok = np.where(near_tie, (g == lower) | (g == upper), g == exact)
    assert ok.all(), (in_form, out_form, int((~ok).sum()))
    return float(near_tie.mean())


# ---- the op ----------------------------------------------------------------------------------------------------------------

def test_codes_avgpool_on_cpu_equals_the_loops_and_the_float32_chain_where_that_is_exact():
    from mct_quantizers_amd.hip import ops
    n = chains = 0
    for u8, form, g, shape in avg_cases():
        codes, S, div, want = avg_case(u8, form, g, **shape)
        in_form, out_form = FORMS[u8][form]
        k, s, p, ceil_mode, include_pad, override = g
        got = ops.codes_avgpool(torch.from_numpy(codes.copy()), in_form, out_form, k, s, p, ceil_mode, include_pad, override)
        assert got.is_contiguous() and got.dtype == (torch.uint8 if out_form[2] >= 0 else torch.int8)
        assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want), (u8, form, g, shape)
        exempt = check_against_the_exact_mean(got.numpy(), S, div, in_form, out_form)
        if form != 0:
            print(f"avg pool case u8={u8} form={form} {g} {shape}: {100 * exempt:.3f} % of the elements next to a tie")
            assert exempt <= 0.01, (u8, form, g, shape, exempt)
        elif all(_pot(d) for d in np.unique(div)) or shape.get("H") == shape.get("W") == 7:
            # power-of-two scale and divisors: every float32 pool is exact.  (Global 7 x 7 on the CPU: found equal as well.)
            assert _pot(in_form[0]) and torch.equal(got, float32_chain(codes, in_form, out_form, g)), (u8, g, shape)
            chains += 1
        n += 1
    assert n == N_CASES and chains == 2 * (2 * 3 + 2)       # 2 x 2, 2 x 2 with ceil_mode and 1 x 1 per C; the large case and 7 x 7
    for u8, zp in EXTREMES:
        codes, in_form, out_form, g, want = extreme_case(u8, zp)
        got = ops.codes_avgpool(torch.from_numpy(codes.copy()), in_form, out_form, *g).numpy()
        assert np.array_equal(got, want)
        assert (got.max() == out_form[3]) == (zp in (0, -127)) and (got.min() == out_form[2]) == (zp in (255, 127)), (u8, zp)
    x = torch.from_numpy(avg_case(True, 1, GEOMETRIES[0])[0].copy())
    forms = FORMS[True][1]
    assert torch.equal(ops.codes_avgpool(x, *forms, 2), ops.codes_avgpool(x, *forms, (2, 2), (2, 2), 0, False, True, None))
    assert torch.equal(ops.codes_avgpool(x, *forms, None), ops.codes_avgpool(x, *forms, (7, 5)))
    nhwc_view = x.permute(0, 2, 1, 3)                                                                    # not contiguous
    assert torch.equal(ops.codes_avgpool(nhwc_view, *forms, 2), ops.codes_avgpool(nhwc_view.contiguous(), *forms, 2))
    assert ops.codes_avgpool(x[:0], *forms, 2).shape == (0, 3, 2, 16)
    odd = torch.from_numpy(make_codes(True, 2, 7, 5, 24))                                                # any channel count
    S, div = avgpool_loops(odd.numpy(), 3, GEOMETRIES[1])
    assert np.array_equal(ops.codes_avgpool(odd, *forms, 3, 2, 1).numpy(), contract_codes(S, div, 0.0213, forms[1]))


def test_codes_avgpool_validation():
    from mct_quantizers_amd.hip import ops
    x = torch.zeros(2, 7, 5, 16, dtype=torch.uint8)
    a, o = (0.05, 0), (0.05, 0, 0, 255)
    with pytest.raises(NotImplementedError, match="codes_avgpool: int8 / uint8 codes only"):
        ops.codes_avgpool(x.float(), a, o, 2)
    with pytest.raises(NotImplementedError, match="codes_avgpool: int8 / uint8 codes only"):
        ops.codes_avgpool(x.to(torch.int16), a, o, 2)
    with pytest.raises(ValueError, match="codes_avgpool takes"):
        ops.codes_avgpool(x[0], a, o, 2)
    with pytest.raises(ValueError, match="larger than half"):
        ops.codes_avgpool(x, a, o, 2, 1, 2)
    with pytest.raises(ValueError, match="larger than half"):
        ops.codes_avgpool(x, a, o, (3, 2), 1, (1, 2))
    with pytest.raises(ValueError, match="codes_avgpool: kernel_size must be an int or a pair"):
        ops.codes_avgpool(x, a, o, (2, 2, 2))
    with pytest.raises(ValueError, match="codes_avgpool: stride must be an int or a pair"):
        ops.codes_avgpool(x, a, o, 2, (1.5, 1))
    with pytest.raises(ValueError, match="codes_avgpool: padding must be an int or a pair"):
        ops.codes_avgpool(x, a, o, 2, 2, (0,))
    for bad in (dict(kernel_size=0), dict(kernel_size=2, stride=0), dict(kernel_size=2, padding=-1)):
        with pytest.raises(ValueError, match="at least"):
            ops.codes_avgpool(x, a, o, **bad)
    with pytest.raises(ValueError, match="does not fit"):
        ops.codes_avgpool(x, a, o, 6)                      # 6 > 5
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="divisor_override must be a positive int or None"):
            ops.codes_avgpool(x, a, o, 2, divisor_override=bad)
    for bad_a, bad_o in (((0.0, 0), o), ((float("inf"), 0), o), (a, (float("nan"), 0, 0, 255)), (a, (-1.0, 0, 0, 255))):
        with pytest.raises(ValueError, match="scales must be finite and positive"):
            ops.codes_avgpool(x, bad_a, bad_o, 2)
    with pytest.raises(ValueError, match="zero point -1 is no torch.uint8 code"):
        ops.codes_avgpool(x, (0.05, -1), o, 2)
    with pytest.raises(ValueError, match="does not fit an 8-bit code"):
        ops.codes_avgpool(x, a, (0.05, 0, -128, 255), 2)


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_codes_avgpool_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_codes_avgpool_nhwc\s*\(", header) and "mctq_codes_avgpool_nhwc" in native.SIGNATURES
    assert os.path.join(build.CSRC, "mctq_codes_avgpool.hip") in build.SOURCES
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(x=P, y=P, dt=U8, zp=3, scale=0.05, B=2, H=7, W=5, C=16, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, ceil=0, inc=1, div=0,
                 ho=4, wo=3, ydt=U8, ys=0.04, yzp=7, qmin=0, qmax=255)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_codes_avgpool_nhwc(v["x"], v["y"], v["dt"], v["zp"], v["scale"], v["B"], v["H"], v["W"], v["C"], v["kh"], v["kw"],
                                           v["sh"], v["sw"], v["ph"], v["pw"], v["ceil"], v["inc"], v["div"], v["ho"], v["wo"],
                                           v["ydt"], v["ys"], v["yzp"], v["qmin"], v["qmax"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWC":
        refused(b"negative extent", **{extent: -1})
    for name in ("kh", "kw"):
        refused(b"kernel size below 1", **{name: 0})
    for name in ("sh", "sw"):
        refused(b"stride below 1", **{name: 0})
    for name in ("ph", "pw"):
        refused(b"negative padding", **{name: -1})
        refused(b"padding larger than half the kernel size", **{name: 2})
    refused(b"more than 65536 taps in a window", kh=65537, kw=1, H=70000, ph=0, pw=0, ho=1)
    refused(b"more than 65536 taps in a window", kh=257, kw=256, ph=0, pw=0)
    refused(b"negative divisor_override", div=-1)
    refused(b"channels must be a multiple of 16", C=24)
    for dt in (-1, 2, 3, 77):
        refused(b"bad code_dtype", dt=dt)
    refused(b"bad y_code_dtype", ydt=-1)
    refused(b"bad y_code_dtype", ydt=2)
    refused(b"zero_point is no code of the input's type", zp=256)
    refused(b"zero_point is no code of the input's type", dt=I8, zp=128)
    for name, message in (("scale", b"scale must be finite and positive"), ("ys", b"y_scale must be finite and positive")):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(message, **{name: bad})
    # wrong in two ways: the window's sizes, the taps, the divisor, the channels, the input's form, the output's, then the fit
    refused(b"padding larger than half the kernel size", ph=2, kw=30000)
    refused(b"more than 65536 taps in a window", kh=257, kw=256, ph=0, pw=0, div=-1)
    refused(b"negative divisor_override", div=-1, C=24)
    refused(b"channels must be a multiple of 16", C=24, dt=77)
    refused(b"bad code_dtype", dt=77, zp=256)
    refused(b"zero_point is no code of the input's type", zp=256, scale=0.0)
    refused(b"scale must be finite and positive", scale=0.0, ys=0.0)
    refused(b"y_scale must be finite and positive", ys=0.0, ydt=-1)
    refused(b"bad y_code_dtype", ydt=-1, kw=9)
    refused(b"quant_min > quant_max", qmin=9, qmax=8, H=2 ** 31)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31 - 4, W=0)              # H + 2 + 3 with the kernel; W: no fit
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=9, pw=1, wo=7)
    refused(b"out_height / out_width are not the pooled extent", H=0, kh=2, ph=1, sh=1, ho=2, x=None)
    refused(b"quant_min > quant_max", qmin=9, qmax=8)
    refused(b"clamp domain does not fit the code type", qmin=-1)
    refused(b"clamp domain does not fit the code type", ydt=I8, qmin=0, qmax=128)
    refused(b"NULL pointer", x=None)
    refused(b"NULL pointer", y=None)
    refused(b"codes and pooled must be 16-byte aligned", x=P + 8)
    refused(b"codes and pooled must be 16-byte aligned", y=P + 1)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=9, pw=1, wo=1)                # 9 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", H=1, kh=3, ph=0, ho=1)
    # the extent the caller allocated must be the library's own: one more or one less, either axis, and the ceil_mode rule
    for name, value in (("ho", 3), ("ho", 5), ("wo", 2), ("wo", 4), ("ho", 0), ("wo", -1)):
        refused(b"out_height / out_width are not the pooled extent", **{name: value})
    assert call(kh=2, kw=2, ph=1, pw=1, ceil=1, ho=4, wo=3, B=0) == 0                                       # both last windows dropped
    refused(b"out_height / out_width are not the pooled extent", kh=2, kw=2, ph=1, pw=1, ceil=1, ho=5, wo=3)
    refused(b"out_height / out_width are not the pooled extent", kh=2, kw=2, ph=0, pw=0, ceil=0, ho=4, wo=3)   # 3 x 2 without ceil_mode
    assert call(kh=256, kw=256, H=256, W=256, ph=0, pw=0, ho=1, wo=1, B=0) == 0                               # 65536 taps: the limit itself
    refused(b"too many output pixels for one launch", B=2 ** 31, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, H=1, W=1, ho=1, wo=1)
    refused(b"more than 2^32 - 1 16-channel chunks of output in one launch", B=2 ** 30, C=64, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0,
            H=1, W=1, ho=1, wo=1)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31, ho=2 ** 30)
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, kh=2, ph=1, sh=1, ho=1)
    assert call(B=0) == 0 and call(B=0, x=None, y=None) == 0          # no images: no launch, no pointer is looked at
    assert call(C=0) == 0                                               # no channels: nothing to write
    assert call(B=0, dt=I8, zp=-5, ydt=I8, qmin=-128, qmax=127) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
    # the tuning key
    for value in (1, 2, 0):
        assert lib.mctq_set_tuning(b"avgpool_form", value) == 0
    for value in (-1, 3):
        assert lib.mctq_set_tuning(b"avgpool_form", value) == E and b"avgpool_form must be" in lib.mctq_last_error()


# ---- the module ------------------------------------------------------------------------------------------------------------

def holder8(signed=False):
    """A holder with threshold 8.0: unsigned scale 2^-5 (ReLU6's 6.0 is code 192, inside the domain), signed scale 2^-4."""
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=signed)
    return mq.PytorchActivationQuantizationHolder(q)


def pot_linear(C, O, seed):
    """A wrapped Linear without bias whose weights have power-of-two scales."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    fc = torch.nn.Linear(C, O, bias=False)
    with torch.no_grad():
        fc.weight.copy_(torch.randn_like(fc.weight) * 0.3 + 0.05)
    return mq.PytorchQuantizationWrapper(fc, {"weight": weights_quantizer(fc.weight, "pot", True)})


def check_module(device):
    """QuantizedAvgPool2d on codes and on float32, windowed, global and flattened, against holder -> pool -> holder itself (the
    scales and divisors are powers of two); returns the outputs."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    outs = []
    for signed in (False, True):
        a, b = holder8(signed), pot_holder(signed)
        qa, qb = a.activation_holder_quantizer, b.activation_holder_quantizer
        x = (torch.randn(2, 16, 8, 4, generator=torch.Generator().manual_seed(3)) * 3.0).to(device)
        for pool, flatten, shape in ((torch.nn.AvgPool2d(2), False, (2, 16, 4, 2)), (torch.nn.AvgPool2d((4, 2), (2, 2), (2, 1), ceil_mode=True,
                                                                                                   divisor_override=8), False, (2, 16, 5, 3)),
                                     (torch.nn.AdaptiveAvgPool2d(1), False, (2, 16, 1, 1)), (torch.nn.AdaptiveAvgPool2d((1, 1)), True, (2, 16)),
                                     (consumers.QuantizedAvgPool2d.GLOBAL, True, (2, 16))):
            qpool = consumers.QuantizedAvgPool2d(pool, qa, qb, flatten=flatten)
            scale, zp, qmin, qmax = qpool.activation_code_params()
            assert (scale, zp, qmin, qmax) == ((8.0 / 128, 0, -128, 127) if signed else (8.0 / 256, 0, 0, 255))
            o_scale, o_zp, o_qmin, o_qmax = qpool.output_code_params()
            assert (o_scale, o_zp, o_qmin, o_qmax) == ((4.0 / 128, 0, -128, 127) if signed else (4.0 / 256, 0, 0, 255))
            for xx in (x, x.contiguous(memory_format=torch.channels_last)):
                y = qpool(xx)
                assert y.dtype == (torch.int8 if signed else torch.uint8) and y.shape == shape
                float_pool = pool if isinstance(pool, torch.nn.Module) else torch.nn.AdaptiveAvgPool2d(1)
                want = b(float_pool(a(xx.cpu())))
                got = ops.dequantize_codes(y.cpu(), o_scale, o_zp)
                assert torch.equal(got, want.flatten(1) if flatten else want)
                if not flatten:
                    assert y.permute(0, 2, 3, 1).is_contiguous()                         # NCHW-shaped, NHWC-stored
                codes = ops.fq_codes_nhwc(xx, qmin, qmax, scale, zp).permute(0, 3, 1, 2)
                assert torch.equal(qpool(codes), y)                                      # codes in: the same codes out
                outs.append(y.cpu())
        with pytest.raises(TypeError, match="do not match this pool's input quantizer"):
            qpool(codes.to(torch.uint8 if signed else torch.int8))
        with pytest.raises(TypeError, match="takes float32 tensors or activation codes"):
            qpool(x.double())
        with pytest.raises(RuntimeError):
            qpool(x[0])
    return outs


def test_quantized_avg_pool2d_on_cpu():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    outs = check_module("cpu")
    assert len(outs) == 2 * 5 * 2 and all(len(torch.unique(y)) > 8 for y in outs)
    ok = consumers.QuantizedAvgPool2d.eligible
    nn = torch.nn
    assert ok(nn.AvgPool2d(2)) and ok(nn.AvgPool2d((3, 2), (2, 3), (1, 0), True, False, 5)) and ok(nn.AdaptiveAvgPool2d(1))
    assert ok(nn.AdaptiveAvgPool2d((1, 1))) and ok(nn.AdaptiveAvgPool2d([1, 1])) and ok(consumers.QuantizedAvgPool2d.GLOBAL)
    assert not ok(nn.AvgPool2d(2, padding=2)) and not ok(nn.AvgPool2d((2, 2, 2))) and not ok(nn.AvgPool2d(2.0)) and not ok(nn.AvgPool2d(0))
    assert not ok(nn.AvgPool2d(2, divisor_override=0)) and not ok(nn.AvgPool2d(2, divisor_override=2.0))
    assert not ok(nn.AdaptiveAvgPool2d(2)) and not ok(nn.AdaptiveAvgPool2d((1, 2))) and not ok(nn.AdaptiveAvgPool2d((None, 1)))
    assert not ok(nn.MaxPool2d(2)) and not ok(nn.AvgPool1d(2)) and not ok(nn.AvgPool3d(2)) and not ok(nn.AdaptiveAvgPool1d(1))
    assert not ok("mean") and not ok(None)

    class Mine(nn.AvgPool2d):                                # exactly nn.AvgPool2d: a subclass may compute anything
        pass

    assert not ok(Mine(2))
    q = unsigned_pot()
    with pytest.raises(TypeError, match="output size 1 only"):
        consumers.QuantizedAvgPool2d(nn.AdaptiveAvgPool2d(2), q, q)
    with pytest.raises(TypeError, match="QuantizedAvgPool2d takes"):
        consumers.QuantizedAvgPool2d(nn.AvgPool2d(2, padding=2), q, q)
    with pytest.raises(ValueError, match="flatten=True needs a global pool"):
        consumers.QuantizedAvgPool2d(nn.AvgPool2d(2), q, q, flatten=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=16, threshold=[4.0], signed=False)
    for pair in ((wide, q), (q, wide)):
        with pytest.raises(NotImplementedError, match="wider than 8 bits"):
            consumers.QuantizedAvgPool2d(nn.AvgPool2d(2), *pair)
    assert not isinstance(consumers.QuantizedAvgPool2d(nn.AvgPool2d(2), q, q), consumers.IntegerConsumer)
    assert consumers.QuantizedAvgPool2d in consumers._CODE_READERS


# ---- the rewrites ----------------------------------------------------------------------------------------------------------

class Head(torch.nn.Module):
    """holder -> conv1x1 -> ReLU6 -> holder A -> global average pool -> holder B -> flatten -> Linear: a MobileNet-style head.
    ``how``: the pool and the flatten as modules, as ``F.adaptive_avg_pool2d`` + ``torch.flatten`` (the flatten in front of B),
    as ``x.mean((2, 3))`` / ``torch.mean(x, (-1, -2), keepdim=True)`` + ``x.flatten(1)`` -- and the forms that are left alone."""

    def __init__(self, how="module"):
        super().__init__()
        self.how = how
        self.h0, self.c, self.act = pot_holder(True), pot_conv(16, 32, 1, 1), torch.nn.ReLU6()
        self.a, self.pool, self.b = holder8(), torch.nn.AdaptiveAvgPool2d(2 if how == "adaptive2" else 1), pot_holder()
        self.flat, self.fc = torch.nn.Flatten(), pot_linear(32 * (4 if how == "adaptive2" else 1), 10, 2)
        self.pool1d, self.pool3d = torch.nn.AvgPool1d(16), torch.nn.AvgPool3d((1, 4, 4))

    def forward(self, x):
        a = self.a(self.act(self.c(self.h0(x))))
        how = self.how
        if how in ("module", "adaptive2"):
            return self.fc(self.flat(self.b(self.pool(a))))
        if how == "functional":
            return self.fc(self.b(torch.flatten(F.adaptive_avg_pool2d(a, (1, 1)), 1)))
        if how == "mean":
            return self.fc(self.b(a.mean((2, 3))))
        if how == "mean_keepdim":
            return self.fc(self.b(torch.mean(a, (-1, -2), keepdim=True)).flatten(1))
        # ---- left alone ----
        if how == "no_b":                                    # no holder behind the pool
            return self.fc(self.flat(self.pool(a)))
        if how == "b_feeds_float":                           # a float32 user of B
            p = self.b(self.pool(a))
            return self.fc(self.flat(p)) + p.sum()
        if how == "pool_feeds_float":                        # a float32 user of the pool
            p = self.pool(a)
            return self.fc(self.flat(self.b(p))) + p.sum()
        if how == "activation":                              # an activation between pool and B
            return self.fc(self.flat(self.b(torch.relu(self.pool(a)))))
        if how == "view":
            return self.fc(self.b(self.pool(a)).view(-1, 32))
        if how == "reshape":
            return self.fc(self.b(self.pool(a).reshape(a.shape[0], -1)))
        if how == "flatten0":                                # not a flatten from dimension 1
            return self.fc(self.b(self.pool(a)).flatten(0).reshape(-1, 32))
        if how == "mean_one_dim":
            return self.fc(self.b(a.mean(2).mean(2)))
        if how == "pool1d":
            return self.fc(self.b(self.pool1d(a.flatten(2)).flatten(1)))
        assert how == "pool3d"
        return self.fc(self.flat(self.b(self.pool3d(a))))


TAKEN = ["module", "functional", "mean", "mean_keepdim"]
LEFT_ALONE = ["no_b", "b_feeds_float", "pool_feeds_float", "activation", "view", "reshape", "flatten0", "mean_one_dim", "pool1d", "pool3d",
              "adaptive2"]


def head_input(device="cpu"):
    return (torch.randn(2, 16, 4, 4, generator=torch.Generator().manual_seed(8)) * 1.5).to(device)


class Squeeze(torch.nn.Module):
    """An SE-style squeeze: holder A feeds a global average pool -> holder B -> pointwise convolution AND a float32 multiply."""

    def __init__(self):
        super().__init__()
        self.h0, self.c, self.act, self.a = pot_holder(True), pot_conv(16, 16, 1, 1), torch.nn.ReLU(), holder8()
        self.pool, self.b, self.fc1 = torch.nn.AdaptiveAvgPool2d(1), pot_holder(), pot_conv(16, 16, 1, 2)

    def forward(self, x):
        a = self.a(self.act(self.c(self.h0(x))))
        return a * self.fc1(self.b(self.pool(a)))


class Between(torch.nn.Module):
    """holder -> conv 3 x 3 -> ReLU -> holder A -> AvgPool2d(2) (module or ``F.avg_pool2d``) -> holder B -> conv 1 x 1."""

    def __init__(self, functional=False):
        super().__init__()
        self.functional = functional
        self.h0, self.c1, self.act, self.a = pot_holder(True), pot_conv(16, 16, 3, 1), torch.nn.ReLU(), holder8()
        self.pool, self.b, self.c2 = torch.nn.AvgPool2d(2), pot_holder(), pot_conv(16, 32, 1, 2)

    def forward(self, x):
        a = self.a(self.act(self.c1(self.h0(x))))
        return self.c2(self.b(F.avg_pool2d(a, 2, stride=2, ceil_mode=False) if self.functional else self.pool(a)))


def between_input(device="cpu"):
    return (torch.randn(2, 16, 8, 6, generator=torch.Generator().manual_seed(9)) * 1.5).to(device)


def _of(gm, cls):
    return {name: m for name, m in gm.named_modules() if isinstance(m, cls)}


EVERY = dict(convolutions=True, shared_holders=True, stay_on_codes=True)


@pytest.mark.parametrize("how", TAKEN)
def test_fx_rewrite_of_a_mobilenet_style_head(how):
    from mct_quantizers_amd import consumers
    C = consumers
    x = head_input()
    want = Head(how)(x)
    pool = {"module": "pool", "functional": "adaptive_avg_pool2d", "mean": "mean", "mean_keepdim": "mean"}[how] + "_qavgpool"
    n_without = 2 if how in ("mean", "functional") else 1                     # (B directly in front of the Linear is a plain pair)
    for switches in (dict(), dict(shared_holders=True)):
        gm, n = C.fuse_linear_consumers_fx(Head(how), avg_pools=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(Head(how), **switches)
        assert (n, n0) == (2, n_without)
        # holder A, whose only user is the pool, is gone with nothing to absorb (ReLU6 is no ReLU); B and the flatten are gone
        assert _targets(gm) == ["c_qlinear", "act", pool, "fc_qlinear"]
        assert not _targets(gm, "call_function") and not _targets(gm, "call_method")
        qpool = gm.get_submodule(pool)
        assert isinstance(qpool, C.QuantizedAvgPool2d) and qpool.global_pool and qpool.flatten
        assert qpool.activation_code_params() == (8.0 / 256, 0, 0, 255) and qpool.output_code_params() == (4.0 / 256, 0, 0, 255)
        assert not _of(gm0, C.QuantizedAvgPool2d)
        seen = []
        hook = qpool.register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype, tuple(out.shape))))
        y = gm(x)
        hook.remove()
        assert seen == [(torch.float32, torch.uint8, (2, 32))]
        assert y.shape == (2, 10) and len(torch.unique(y)) > 15 and torch.equal(y, gm0(x)) and torch.equal(y, want)
    # with stay_on_codes the convolution emits A's codes, ReLU6 folded into their clamp: codes from the first holder to the logits
    gm, n = C.fuse_linear_consumers_fx(Head(how), avg_pools=True, **EVERY)
    gm0, n0 = C.fuse_linear_consumers_fx(Head(how), **EVERY)
    assert (n, n0) == (2, n_without) and _targets(gm) == ["c_qlinear", pool, "fc_qlinear"]
    producer, qpool = gm.get_submodule("c_qlinear"), gm.get_submodule(pool)
    assert producer.emit_codes_for == qpool.activation_code_params() and producer.emit_clamp == (0, 192)         # 6.0 / 2^-5
    assert gm.get_submodule("fc_qlinear").activation_code_params() == qpool.output_code_params()
    seen = []
    hook = qpool.register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype)))
    y = gm(x)
    hook.remove()
    assert seen == [(torch.uint8, torch.uint8)] and torch.equal(y, gm0(x)) and torch.equal(y, want)
    # tracing the rewritten graph again keeps the pool a leaf and replaces nothing more
    again, n = C.fuse_linear_consumers_fx(gm, avg_pools=True, **EVERY)
    assert n == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), y)


@pytest.mark.parametrize("how", LEFT_ALONE)
def test_fx_rewrite_leaves_the_other_forms_alone(how):
    from mct_quantizers_amd import consumers
    for switches in (dict(), dict(shared_holders=True), EVERY):
        gm, n = consumers.fuse_linear_consumers_fx(Head(how), avg_pools=True, **switches)
        gm0, n0 = consumers.fuse_linear_consumers_fx(Head(how), **switches)
        assert n == n0 and str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
        assert not _of(gm, consumers.QuantizedAvgPool2d)
    if how not in ("pool1d",):
        x = head_input()
        assert torch.equal(gm(x), Head(how)(x))


def test_fx_rewrite_of_an_se_style_squeeze():
    from mct_quantizers_amd import consumers
    C = consumers
    x = head_input()
    want = Squeeze()(x)
    # shared_holders: A becomes a join (its ReLU absorbed) that writes float32 for the multiply and codes for the pool
    gm, n = C.fuse_linear_consumers_fx(Squeeze(), avg_pools=True, shared_holders=True)
    gm0, n0 = C.fuse_linear_consumers_fx(Squeeze(), shared_holders=True)
    assert (n, n0) == (2, 2)                                  # (without the switch B -> fc1 is a plain pair)
    assert _targets(gm) == ["c_qlinear", "a_join", "pool_qavgpool", "fc1_qlinear"]
    assert _targets(gm0) == ["c_qlinear", "act", "a", "pool", "fc1_qlinear"]
    assert _targets(gm, "call_function") == [operator.getitem, operator.getitem, operator.mul]
    join, qpool = gm.get_submodule("a_join"), gm.get_submodule("pool_qavgpool")
    assert (join.relu, join.has_residual, join.want_float) == (True, False, True)
    assert qpool.global_pool and not qpool.flatten and isinstance(gm.get_submodule("fc1_qlinear"), C.QuantizedConv1x1)
    seen = []
    hook = qpool.register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype, tuple(out.shape))))
    y = gm(x)
    hook.remove()
    assert seen == [(torch.uint8, torch.uint8, (2, 16, 1, 1))]
    assert y.shape == (2, 16, 4, 4) and len(torch.unique(y)) > 50 and torch.equal(y, gm0(x)) and torch.equal(y, want)
    # without shared_holders a holder with another user is left alone
    gm1, n1 = C.fuse_linear_consumers_fx(Squeeze(), avg_pools=True)
    gm2, n2 = C.fuse_linear_consumers_fx(Squeeze())
    assert n1 == n2 == 2 and str(gm1.graph) == str(gm2.graph) and not _of(gm1, C.QuantizedAvgPool2d) and torch.equal(gm1(x), want)


@pytest.mark.parametrize("functional", [False, True])
def test_fx_rewrite_of_an_average_pool_between_two_convolutions(functional):
    from mct_quantizers_amd import consumers
    C = consumers
    x = between_input()
    want = Between(functional)(x)
    pool = ("avg_pool2d" if functional else "pool") + "_qavgpool"
    gm, n = C.fuse_linear_consumers_fx(Between(functional), avg_pools=True, **EVERY)
    gm0, n0 = C.fuse_linear_consumers_fx(Between(functional), **EVERY)
    assert (n, n0) == (2, 2)
    assert _targets(gm) == ["c1_qlinear", pool, "c2_qlinear"] and not _targets(gm, "call_function")
    qpool = gm.get_submodule(pool)
    assert (qpool.kernel_size, qpool.stride, qpool.padding, qpool.ceil_mode, qpool.count_include_pad, qpool.divisor_override) == \
        ((2, 2), (2, 2), (0, 0), False, True, None) and not qpool.global_pool
    producer = gm.get_submodule("c1_qlinear")                 # the ReLU went into a join, the join into the producer's clamp
    assert producer.emit_codes_for == qpool.activation_code_params() == (8.0 / 256, 0, 0, 255) and not _of(gm, C.QuantizedJoin)
    y = gm(x)
    assert y.shape == (2, 32, 4, 3) and len(torch.unique(y)) > 50 and torch.equal(y, gm0(x)) and torch.equal(y, want)
    # the switch alone: A goes, the ReLU stays, the pool quantizes
    gm1, n1 = C.fuse_linear_consumers_fx(Between(functional), convolutions=True, avg_pools=True)
    assert n1 == 2 and _targets(gm1) == ["c1_qlinear", "act", pool, "c2_qlinear"] and torch.equal(gm1(x), want)


def test_sequential_rewrites():
    from mct_quantizers_amd import consumers
    C = consumers

    def head():
        return torch.nn.Sequential(pot_holder(True), pot_conv(16, 32, 1, 1), holder8(True), torch.nn.AdaptiveAvgPool2d(1), pot_holder(True),
                                   torch.nn.Flatten(), pot_linear(32, 10, 2)).eval()

    def between():
        return torch.nn.Sequential(pot_holder(True), pot_conv(16, 16, 3, 1), torch.nn.ReLU(), holder8(), torch.nn.AvgPool2d(2), pot_holder(),
                                   pot_conv(16, 32, 1, 2)).eval()

    x = head_input()
    plain, pooled = head(), head()
    assert C.fuse_linear_consumers(plain, chain=True) == 1 and C.fuse_linear_consumers(pooled, chain=True, avg_pools=True) == 2
    assert [type(m) for m in pooled] == [C._FusedAway, C.QuantizedConv1x1, C._FusedAway, C.QuantizedAvgPool2d, C._FusedAway, C._FusedAway,
                                         C.QuantizedLinear]
    assert pooled[3].flatten and pooled[3].global_pool
    assert pooled[1].emit_codes_for == pooled[3].activation_code_params() == (8.0 / 128, 0, -128, 127)      # chain=True
    assert pooled[6].activation_code_params() == pooled[3].output_code_params() == (4.0 / 128, 0, -128, 127)
    assert plain[1].emit_codes_for is None and isinstance(plain[3], torch.nn.AdaptiveAvgPool2d)
    y = pooled(x)
    assert y.shape == (2, 10) and len(torch.unique(y)) > 15 and torch.equal(y, plain(x)) and torch.equal(y, head()(x))
    x = between_input()
    plain, pooled = between(), between()
    assert C.fuse_linear_consumers(plain, convolutions=True) == 2 and C.fuse_linear_consumers(pooled, convolutions=True, avg_pools=True) == 2
    assert [type(m) for m in pooled] == [C._FusedAway, C.QuantizedConv2d, torch.nn.ReLU, C._FusedAway, C.QuantizedAvgPool2d, C._FusedAway,
                                         C.QuantizedConv1x1]
    assert [type(m) for m in plain][3:6] == [type(pot_holder()), torch.nn.AvgPool2d, C._FusedAway]
    y = pooled(x)
    assert y.shape == (2, 32, 4, 3) and len(torch.unique(y)) > 50 and torch.equal(y, plain(x)) and torch.equal(y, between()(x))
    # left alone: a flatten behind a windowed pool, an adaptive pool of another size, a Linear on a 4-D tensor, no holder B
    for layers in ([pot_holder(), torch.nn.AvgPool2d(4), pot_holder(), torch.nn.Flatten(), pot_linear(16, 10, 2)],
                   [pot_holder(), torch.nn.AdaptiveAvgPool2d(2), pot_holder(), pot_conv(16, 16, 1, 2)],
                   [pot_holder(), torch.nn.AdaptiveAvgPool2d(1), pot_holder(), pot_linear(16, 10, 2)],
                   [pot_holder(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), pot_linear(16, 10, 2)]):
        m = torch.nn.Sequential(*layers)
        C.fuse_linear_consumers(m, avg_pools=True)
        assert not _of(m, C.QuantizedAvgPool2d) and m[1] is layers[1]
    with pytest.raises(TypeError):
        C.fuse_linear_consumers(head(), avg_pool=True)


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers
    for switches in (dict(), dict(convolutions=True), dict(convolutions=True, shared_holders=True), EVERY, dict(pools=True, **EVERY)):
        for make in (Head, Squeeze, Between):
            gm, n = consumers.fuse_linear_consumers_fx(make(), **switches)
            gm_off, n_off = consumers.fuse_linear_consumers_fx(make(), avg_pools=False, **switches)
            assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
            assert not _of(gm, consumers.QuantizedAvgPool2d)


# ---- the workload ----------------------------------------------------------------------------------------------------------

def _inventory(model):
    return [(name, type(m), tuple(m.weight.shape) if isinstance(getattr(m, "weight", None), torch.Tensor) else None)
            for name, m in model.named_modules()]


def test_wrapped_resnet50_with_and_without_the_pooled_holder():
    """Construction, trace and rewrite only: no forward.  The default is the model as it was (the classifier reads an
    unquantized mean, which the rewrite leaves alone); ``pooled_holder=True`` adds one holder behind the pool, and with every
    switch 53 of the 54 wrapped layers are replaced (the 3-channel stem stays), the head being c3 with the last join in its
    epilogue -> the pool on codes -> the classifier's product."""
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers, workloads
    C = consumers
    default, off, on = workloads.wrapped_resnet50(device="cpu"), workloads.wrapped_resnet50(device="cpu", pooled_holder=False), \
        workloads.wrapped_resnet50(device="cpu", pooled_holder=True)
    assert _inventory(default) == _inventory(off) and len(default) == 22
    assert [type(m) for m in default][-3:] == [torch.nn.AdaptiveAvgPool2d, torch.nn.Flatten, mq.PytorchQuantizationWrapper]
    assert len(on) == 23 and isinstance(on[20], mq.PytorchActivationQuantizationHolder) and isinstance(on[19], torch.nn.AdaptiveAvgPool2d)
    assert [type(m) for i, m in enumerate(on) if i != 20] == [type(m) for m in default]
    assert all(torch.equal(p, q) for p, q in zip(default.parameters(), on.parameters()))
    every = dict(pools=True, fused_residuals=True, **EVERY)
    gm, n = C.fuse_linear_consumers_fx(on, avg_pools=True, **every)
    assert n == 53 and len(_of(gm, C.IntegerConsumer)) == 53
    assert [t for t in _targets(gm) if isinstance(gm.get_submodule(t), mq.PytorchQuantizationWrapper)] == ["0"]
    assert _targets(gm)[-3:] == ["18_c3_qlinear", "19_qavgpool", "22_qlinear"]
    last, qpool, fc = (gm.get_submodule(t) for t in _targets(gm)[-3:])
    assert last.emit_codes_for == qpool.activation_code_params() and last.emit_residual is not None and last.emit_relu
    assert qpool.global_pool and qpool.flatten and isinstance(fc, C.QuantizedLinear)
    assert fc.activation_code_params() == qpool.output_code_params() == (8.0 / 256, 0, 0, 255)
    assert not [t for t in _targets(gm) if isinstance(gm.get_submodule(t), (torch.nn.ReLU, torch.nn.AdaptiveAvgPool2d, torch.nn.Flatten))]
    # the model as it stands has no holder B: its head is left alone, with the switch or without
    gm1, n1 = C.fuse_linear_consumers_fx(default, avg_pools=True, **every)
    assert n1 == 52 and not _of(gm1, C.QuantizedAvgPool2d) and _targets(gm1)[-3:] == ["19", "20", "21"]
