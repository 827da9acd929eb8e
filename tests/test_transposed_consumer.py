"""Transposed convolutions on the integer consumer: host logic and the CPU route (include/mctq_hip.h: mctq_qconv_transposed_i8;
consumers.qconv_transposed_i8, consumers.pack_transposed_weights, consumers.QuantizedConvTranspose2d and the ``transposed``
switch of fuse_linear_consumers / fuse_linear_consumers_fx).

Oracle of every exactness check: plain numpy loops in the GATHER form of the header's formula -- per output pixel (oy, ox) and
tap (ky, kx) the input pixel iy = (oy + ph - ky) / sh, ix = (ox + pw - kx) / sw where both divisions are exact and the pixel
lies inside the image, int64 sums over the channels (zero points off) -- then the depthwise tests' epilogue
(tests/test_dw_consumer.py: dw_epilogue, that of oracle/mctq_oracle.py::qlinear_i8).  The CPU route of the package is the SCATTER
form (a strided += per tap into a canvas) and the kernel the phase decomposition: three independent derivations.  The loops are
checked once against ``F.conv_transpose2d`` in float64 on the integer operands (a - za), (w - zw), which is exact: every sum
stays below 2^53.

Bound against float64 (derived in tests/test_conv_consumer.py and used by the grouped and depthwise tests, the same four
roundings): |y - y64| <= 2^-21 (|p64| + |bias|) with p64 the exact integer sum times the float64 product of the two float32
scales.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_concat_consumer import holder_of
from test_conv_consumer import FAMILIES, LUT16, LUT256, activation_quantizer
from test_dw_consumer import ZERO_POINTS, dw_epilogue
from test_grouped_consumer import FORMS
from test_join_consumer import _targets
from test_pool_consumer import pot_conv

F32 = np.float32
# (kernel, stride, padding, output padding): 2 x 2 stride 2; 3 x 3 stride 2 with output padding; 4 x 4 stride 2; stride 1; stride
# 3 with five taps; rectangular with mixed strides; k = 1 < s (pixels no tap reaches); k < s = 4 with the largest output padding;
# rectangular, k < s along x only
GEOMETRIES = [((2, 2), (2, 2), (0, 0), (0, 0)), ((3, 3), (2, 2), (1, 1), (1, 1)), ((4, 4), (2, 2), (1, 1), (0, 0)),
              ((3, 3), (1, 1), (1, 1), (0, 0)), ((5, 5), (3, 3), (2, 2), (2, 2)), ((2, 3), (2, 1), (0, 1), (1, 0)),
              ((1, 1), (2, 2), (0, 0), (1, 1)), ((3, 3), (4, 4), (0, 0), (3, 3)), ((3, 2), (1, 3), (2, 0), (0, 2))]
NO_TAPS = 7                                                # (3, 4, 0, 3): phases without taps
# (C, O): C = 80 gives a K tail behind a full step of 64; O = 72 two N slices, the second with 8 channels
SHAPES = [(c, o) for c in (16, 48, 80) for o in (5, 16, 72)]


def out_hw(h, w, k, s, p, op):
    return (h - 1) * s[0] - 2 * p[0] + k[0] + op[0], (w - 1) * s[1] - 2 * p[1] + k[1] + op[1]


def transposed_loops(a, za, w, k, s, p, op):
    """a [B, H, W, C] codes, w [O, kh, kw, C] integers (zero points already off) -> int64 sums [B, Ho, Wo, O]."""
    B, H, W, C = a.shape
    O = w.shape[0]
    assert w.shape == (O, k[0], k[1], C)
    ho, wo = out_hw(H, W, k, s, p, op)
    a64, w64 = a.astype(np.int64) - int(za), w.astype(np.int64)
    acc = np.zeros((B, ho, wo, O), dtype=np.int64)
    for oy in range(ho):
        for ky in range(k[0]):
            iy, off_y = divmod(oy + p[0] - ky, s[0])
            if off_y or not 0 <= iy < H:
                continue
            for ox in range(wo):
                for kx in range(k[1]):
                    ix, off_x = divmod(ox + p[1] - kx, s[1])
                    if off_x or not 0 <= ix < W:
                        continue
                    acc[:, oy, ox] += a64[:, iy, ix] @ w64[:, ky, kx].T
    return acc


def transposed_oracle(a, za, sa, w, ws, bias, geometry):
    return dw_epilogue(transposed_loops(a, za, w, *geometry), sa, ws, bias)


def _finish(a, za, sa, w, ws, zw, bias, g):
    w_off = w.astype(np.int64) - (0 if zw is None else zw.astype(np.int64).reshape(-1, 1, 1, 1))
    want = transposed_oracle(a, za, sa, w_off, ws, bias, g)
    for t in (a, w, ws, zw, bias, want):
        if t is not None:
            t.setflags(write=False)
    return dict(a=a, za=za, sa=sa, w=w, ws=ws, zw=zw, bias=bias, geometry=g, want=want)


@functools.lru_cache(maxsize=None)
def raw_case(u8, si, gi, za, with_zp, with_bias, B=2, H=5, W=7, C=None, geometry=None):
    """Seeded operands of one raw call and the loops' float32 result, computed once and shared by the CPU and GPU tests;
    read-only.  Weight zero points of both signs, -128 and 127 among them."""
    c, o = SHAPES[si]
    c = C or c
    rng = np.random.default_rng(6151 * si + 37 * gi + 5 * (za + 128) + 2 * with_zp + with_bias + 1000 * B + H)
    g = geometry or GEOMETRIES[gi]
    a = rng.integers(0, 256, (B, H, W, c)).astype(np.uint8).view(np.uint8 if u8 else np.int8)
    w = rng.integers(-128, 128, (o, *g[0], c)).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, o).astype(F32)
    zw = None
    if with_zp:
        zw = rng.integers(-128, 128, o).astype(np.int32)
        zw[:4] = (-128, 127, 0, -1)
    bias = rng.normal(0, 2.0, o).astype(F32) if with_bias else None
    return _finish(a, za, 0.0173, w, ws, zw, bias, g)


def raw_cases(si):
    """(code type, shape, geometry, zero point, weight zero points?, bias?) of one row of SHAPES: every geometry with each code
    type, the type's three zero points in turn; weight zero points and bias alternate on and off with different periods, so
    that over the rows every geometry and code type meets both settings of both."""
    n = si
    for u8 in (True, False):
        for gi in range(len(GEOMETRIES)):
            n += 1
            yield u8, si, gi, ZERO_POINTS[np.uint8 if u8 else np.int8][n % 3], n % 2 == 0, n % 3 != 0


def extreme_case():
    """The largest magnitude the sum reaches: a 4 x 4 stride-1 kernel on a 4 x 4 image of 2048 channels -- with padding 1 the
    output pixel (2, 2) is reached by all 16 taps, K = 32768 terms -- every activation code 255 with za = 0, weights -128
    (even output channels) and 127 (odd ones): -32768 * 255 * 128 and 32768 * 255 * 127, both inside int32."""
    g = ((4, 4), (1, 1), (1, 1), (0, 0))
    a = np.full((1, 4, 4, 2048), 255, dtype=np.uint8)
    w = np.empty((16, 4, 4, 2048), dtype=np.int8)
    w[0::2], w[1::2] = -128, 127
    ws = np.linspace(0.001, 0.01, 16).astype(F32)
    bias = np.linspace(-3, 3, 16).astype(F32)
    c = _finish(a, 0, 0.031, w, ws, None, bias, g)
    acc = transposed_loops(a, 0, w, *g)
    assert acc.shape == (1, 5, 5, 16) and acc.min() == -32768 * 255 * 128 and acc.max() == 32768 * 255 * 127
    assert acc[0, 2, 2, 0] == acc.min() and acc[0, 2, 2, 1] == acc.max()
    return c


def extreme_form(case):
    """A uint8 form whose codes spread over the extreme case's results."""
    lo, hi = float(case["want"].min()), float(case["want"].max())
    return (hi - lo) / 200.0, int(round(-lo / ((hi - lo) / 200.0))) + 20, 0, 255


def run_raw_on(case, device="cpu", out_codes=None, packed=None):
    from mct_quantizers_amd import consumers
    t = lambda v: None if v is None else torch.from_numpy(v.copy()).to(device)      # noqa: E731
    return consumers.qconv_transposed_i8(t(case["a"]), case["za"], case["sa"], t(case["w"]), t(case["ws"]), t(case["bias"]),
                                         *case["geometry"], out_codes=out_codes, w_zero_points=t(case["zw"]), packed=packed)


def check_loops_against_float64(case):
    """The loops' integer sums equal to ``F.conv_transpose2d`` in float64 on the integer operands, exactly; their float32
    result within the derived bound of the exact value."""
    a, w, g = case["a"], case["w"], case["geometry"]
    w_off = w.astype(np.int64) - (0 if case["zw"] is None else case["zw"].astype(np.int64).reshape(-1, 1, 1, 1))
    acc = transposed_loops(a, case["za"], w_off, *g)
    a64 = torch.from_numpy(a.astype(np.float64) - case["za"]).permute(0, 3, 1, 2)
    w64 = torch.from_numpy(w_off.astype(np.float64)).permute(3, 0, 1, 2)                   # [C, O, kh, kw]
    y64 = torch.nn.functional.conv_transpose2d(a64, w64, None, g[1], g[2], g[3]).permute(0, 2, 3, 1).numpy()
    assert np.abs(acc).max() < 2 ** 53 and np.array_equal(y64, acc.astype(np.float64))
    check_bound(case["want"], acc, case["sa"], case["ws"], case["bias"])


def check_bound(got, acc, sa, ws, bias):
    p64 = acc.astype(np.float64) * (np.float64(F32(sa)) * ws.astype(np.float64))
    b64 = np.zeros(ws.shape[0]) if bias is None else bias.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (p64 + b64))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64))
    assert np.all(err <= bound), float((err - bound).max())


def test_the_loops_agree_with_float64_conv_transpose2d():
    seen = set()
    for si in range(len(SHAPES)):
        for n, case in enumerate(raw_cases(si)):
            if n % 9 == si:                             # every shape; every geometry and both code types over the rows
                check_loops_against_float64(raw_case(*case))
                seen.add((case[0], case[2]))
    assert len(seen) == 2 * len(GEOMETRIES)
    check_loops_against_float64(extreme_case())


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_qconv_transposed_i8_on_cpu_equals_the_loops(si):
    from mct_quantizers_amd.hip import ops
    n = 0
    for case in raw_cases(si):
        c = raw_case(*case)
        y = run_raw_on(c)
        assert y.dtype == torch.float32 and y.shape == c["want"].shape and y.is_contiguous()
        assert bits_equal(y.numpy(), c["want"]), (case, first_mismatch(y.numpy(), c["want"]))
        for form in FORMS:
            codes = run_raw_on(c, out_codes=form)
            want = ops.fq_codes(y, None, None, None, form[2], form[3], form[0], form[1])
            assert codes.dtype == (torch.uint8 if form[2] >= 0 else torch.int8) and torch.equal(codes, want), (case, form)
            assert len(torch.unique(want)) > 8
        n += 1
    assert n == 2 * len(GEOMETRIES)


def test_every_setting_meets_every_geometry():
    seen = {(c[0], c[2], c[4], c[5]) for si in range(len(SHAPES)) for c in raw_cases(si)}
    assert len(seen) == 2 * len(GEOMETRIES) * 4
    zps = {(c[0], c[2], c[3]) for si in range(len(SHAPES)) for c in raw_cases(si)}
    assert len(zps) == 2 * len(GEOMETRIES) * 3


def edge_cases(u8):
    """(name, case) of the GPU test's edge cases; the CPU route runs them too."""
    za = 114 if u8 else -3
    two = GEOMETRIES[0]
    yield "one input pixel", raw_case(u8, 4, 0, za, True, True, B=1, H=1, W=1)                      # four phases of one pixel each
    yield "243 pixels per phase", raw_case(u8, 4, 0, za, False, True, B=3, H=9, W=9)               # four blocks, the last with three pixels
    yield "1 x 1 output", raw_case(u8, 4, 0, za, True, True, B=1, H=1, W=1, geometry=((1, 1), (2, 2), (0, 0), (0, 0)))
    yield "phases without taps, bias", raw_case(u8, 5, NO_TAPS, za, True, True)
    yield "phases without taps, no bias", raw_case(u8, 5, NO_TAPS, za, True, False)
    yield "K = 64", raw_case(u8, 4, 0, za, True, True, C=64, geometry=two)


def test_qconv_transposed_i8_on_cpu_edge_values_and_any_channel_count():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    c = extreme_case()
    y = run_raw_on(c)
    assert bits_equal(y.numpy(), c["want"]), first_mismatch(y.numpy(), c["want"])
    form = extreme_form(c)
    codes = run_raw_on(c, out_codes=form)
    assert torch.equal(codes, ops.fq_codes(y, None, None, None, 0, 255, form[0], form[1])) and len(torch.unique(codes)) >= 8
    for u8 in (True, False):
        for name, c in edge_cases(u8):
            assert bits_equal(run_raw_on(c).numpy(), c["want"]), name
    names = dict(edge_cases(True))
    assert names["one input pixel"]["want"].shape == (1, 2, 2, 16) and names["1 x 1 output"]["want"].shape == (1, 1, 1, 16)
    assert names["243 pixels per phase"]["want"].shape == (3, 18, 18, 16)
    # a pixel no tap reaches holds the bias, or 0 without one, bit for bit
    for name, fill in (("phases without taps, bias", None), ("phases without taps, no bias", 0.0)):
        want = names[name]["want"]
        empty = want[:, 3::4, 3::4]                      # ry = rx = 3 >= k = 3
        assert empty.size and bits_equal(empty, np.broadcast_to(names[name]["bias"] if fill is None else F32(fill), empty.shape))
    # ints stand for pairs, as in torch.nn.ConvTranspose2d; a narrowed clamp stays inside the domain's code type
    c = raw_case(True, 4, 1, 114, False, True)
    t = lambda v: torch.from_numpy(v.copy())      # noqa: E731
    y = consumers.qconv_transposed_i8(t(c["a"]), 114, c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), 3, 2, 1, 1)
    assert bits_equal(y.numpy(), c["want"])
    codes = consumers.qconv_transposed_i8(t(c["a"]), 114, c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), 3, 2, 1, 1,
                                          out_codes=(0.41, -5, -128, 127, -5, 100))
    assert codes.dtype == torch.int8 and int(codes.min()) == -5 and int(codes.max()) <= 100
    # the CPU route takes any C and any stride: 3 channels, stride 5
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (1, 3, 4, 3)).astype(np.uint8)
    w = rng.integers(-128, 128, (4, 3, 3, 3)).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, 4).astype(F32)
    y = consumers.qconv_transposed_i8(t(a), 7, 0.02, t(w), t(ws), None, 3, 5, 1, 4)
    assert bits_equal(y.numpy(), transposed_oracle(a, 7, 0.02, w.astype(np.int64), ws, None, ((3, 3), (5, 5), (1, 1), (4, 4))))


def test_pack_transposed_weights_layout():
    from mct_quantizers_amd import consumers
    for gi, si in ((1, 1), (5, 6), (7, 2), (4, 8)):
        k, s = GEOMETRIES[gi][:2]
        w = torch.from_numpy(raw_case(True, si, gi, 114, True, True)["w"].copy())          # [O, kh, kw, C]
        O, C = w.shape[0], w.shape[3]
        packed, rowsum = consumers.pack_transposed_weights(w, s)
        ty = [max(0, -(-(k[0] - r) // s[0])) for r in range(s[0])]
        tx = [max(0, -(-(k[1] - r) // s[1])) for r in range(s[1])]
        P, Op, Kp = s[0] * s[1], -(-O // 16) * 16, -(-(ty[0] * tx[0] * C) // 64) * 64
        assert packed.dtype == torch.int8 and tuple(packed.shape) == (P, Op, Kp) and packed.is_contiguous()
        assert rowsum.dtype == torch.int32 and tuple(rowsum.shape) == (P, O) and rowsum.is_contiguous()
        seen = torch.zeros(k, dtype=torch.int64)
        for ry in range(s[0]):
            for rx in range(s[1]):
                p, K = ry * s[1] + rx, ty[ry] * tx[rx] * C
                assert not packed[p, O:].any() and not packed[p, :, K:].any()                # the padding holds 0
                taps = packed[p, :O, :K].reshape(O, ty[ry], tx[rx], C)
                for a in range(ty[ry]):
                    for b in range(tx[rx]):
                        assert torch.equal(taps[:, a, b], w[:, ry + s[0] * a, rx + s[1] * b])
                        seen[ry + s[0] * a, rx + s[1] * b] += 1
                assert torch.equal(rowsum[p], packed[p, :O].to(torch.int64).sum(dim=1).to(torch.int32))
        assert bool((seen == 1).all())                                                       # every tap exactly once
    if True:                                             # 3 x 3 stride 2: the four phases have 4C, 2C, 2C and C columns
        w = torch.ones((5, 3, 3, 16), dtype=torch.int8)
        packed, rowsum = consumers.pack_transposed_weights(w, 2)
        assert tuple(packed.shape) == (4, 16, 64) and rowsum[:, 0].tolist() == [64, 32, 32, 16]


def test_qconv_transposed_i8_refuses_bad_operands():
    from mct_quantizers_amd import consumers
    c = raw_case(True, 4, 1, 114, True, True)                  # C = 48, O = 16, 3 x 3 stride 2
    a, w, ws, b, zw = (torch.from_numpy(c[k].copy()) for k in ("a", "w", "ws", "bias", "zw"))
    f = consumers.qconv_transposed_i8
    with pytest.raises(TypeError):
        f(a.float(), 114, 0.1, w, ws, b, 3, 2, 1, 1)
    with pytest.raises(TypeError):
        f(a[0], 114, 0.1, w, ws, b, 3, 2, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w.to(torch.int32), ws, b, 3, 2, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w.permute(3, 0, 1, 2).contiguous(), ws, b, 3, 2, 1, 1)          # [C, O, kh, kw]
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w, ws.double(), b, 3, 2, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w, ws, b, 3, 2, 1, 1, w_zero_points=zw.long())
    with pytest.raises(RuntimeError):
        f(a, 114, 0.1, w, ws, b, 3, 2, 1, 1, w_zero_points=zw[:8].contiguous())
    with pytest.raises(RuntimeError):
        f(a, 114, 0.1, w, ws[:8].contiguous(), b, 3, 2, 1, 1)
    with pytest.raises(ValueError):
        f(a, 256, 0.1, w, ws, b, 3, 2, 1, 1)                                            # no uint8 code
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 3, 0, 1, 1)
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 3, 2, 1, 2)                                            # output padding >= stride
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 3, 2, 9, 1)                                            # the padding leaves no output
    with pytest.raises(ValueError, match="qconv_transposed_i8: stride"):               # refused in this function's own name
        f(a, 114, 0.1, w, ws, b, 3, (1, 1, 1), 1)


# ---- wrapped transposed convolutions -------------------------------------------------------------------------------------

def t_weights_quantizer(weight, family, per_channel, axis=1):
    """test_conv_consumer.weights_quantizer for a [C, O, kh, kw] weight: per-channel values run along ``axis`` (1: the output
    channels)."""
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    n = weight.shape[axis]
    w2 = weight.detach().transpose(0, axis).reshape(n, -1)
    ax = axis if per_channel else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if family == "sym":
            thr = [float(v) for v in w2.abs().max(1).values] if per_channel else [float(w2.abs().max())]
            return Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=per_channel, channel_axis=ax)
        if family == "pot":
            thr = [float(2.0 ** (-2 + i % 3)) for i in range(n)] if per_channel else [0.5]
            return Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=thr, per_channel=per_channel, channel_axis=ax)
        if family in ("lut16", "lut256"):
            thr = [float(v) for v in w2.abs().max(1).values] if per_channel else [float(w2.abs().max())]
            return Q.WeightsLUTSymmetricInferableQuantizer(
                num_bits=4 if family == "lut16" else 8, lut_values=LUT16 if family == "lut16" else LUT256, threshold=thr,
                per_channel=per_channel, channel_axis=ax, input_rank=4 if per_channel else None, lut_values_bitwidth=8)
        assert family == "uniform"
        if per_channel:
            lo = [min(float(v), -0.01) for v in w2.min(1).values]
            hi = [max(float(v), 0.01) for v in w2.max(1).values]
            lo[0], hi[0], lo[1], hi[1] = -0.2, 1.3, -1.1, 0.4
            return Q.WeightsUniformInferableQuantizer(num_bits=8, min_range=lo, max_range=hi, per_channel=True, channel_axis=axis)
        return Q.WeightsUniformInferableQuantizer(num_bits=8, min_range=[-0.2], max_range=[1.3], per_channel=False)


def convt_pair(C=32, O=24, k=2, stride=2, padding=0, output_padding=0, family="sym", per_channel=True, bias=True, act="uniform",
               seed=0, axis=1, **kw):
    """[activation holder, wrapped ConvTranspose2d]; weights N(0.1, 0.4): uniform ranges and codebooks are really used."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    conv = torch.nn.ConvTranspose2d(C, O, k, stride=stride, padding=padding, output_padding=output_padding, bias=bias, **kw)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 0.4 + 0.1)
    wq = t_weights_quantizer(conv.weight, family, per_channel, axis)
    return [mq.PytorchActivationQuantizationHolder(activation_quantizer(act)), mq.PytorchQuantizationWrapper(conv, {"weight": wq})]


def convt_model(**kw):
    return torch.nn.Sequential(*convt_pair(**kw))


def t_weight_operands(qc):
    """(int codes [O, kh, kw, C] with the zero points already taken off, float32 scales [O]) of a fused layer, from the weights
    quantizer's own codes of the float [C, O, kh, kw] weight."""
    q, w = qc.weights_quantizer, qc.weight.detach()
    O = w.shape[1]
    order = lambda t: t.cpu().numpy().reshape(w.shape).transpose(1, 2, 3, 0)                    # noqa: E731
    per_row = lambda t: np.broadcast_to(t.detach().cpu().numpy().astype(F32).reshape(-1), (O,)) if t.numel() == 1 \
        else t.detach().cpu().numpy().astype(F32).reshape(-1)                                    # noqa: E731
    if qc._lut_weights:
        idx, lut, thr = q.quantize_to_codes(w)
        lut = lut.cpu().numpy().reshape(-1)
        return lut.astype(np.int32)[order(idx)], per_row(thr) / F32(2.0 ** (q.lut_values_bitwidth - 1))
    codes, scales, zps = q.quantize_to_codes(w)
    codes = order(codes).astype(np.int32)
    if qc._uniform_weights:
        codes = codes - np.broadcast_to(zps.cpu().numpy().astype(np.int32).reshape(-1), (O,))[:, None, None, None]
    return codes, per_row(scales)


def check_transposed_against_loops_and_float64(qc, x, y):
    """x: the float32 [B, C, H, W] input of the fused layer ``qc`` (any memory format, any device), y its float32 output:
    bit-equal to the loops on the layer's own activation codes, and within the derived bound of the exact value."""
    from mct_quantizers_amd.hip import ops
    za, sa = qc._a_zp, qc._a_scale
    a = ops.fq_codes_nhwc(x.detach(), qc._a_qmin, qc._a_qmax, sa, za).cpu().numpy()
    w, ws = t_weight_operands(qc)
    bias = None if qc.bias is None else qc.bias.detach().cpu().numpy()
    g = (qc.kernel_size, qc.stride, qc.padding, qc.output_padding)
    acc = transposed_loops(a, za, w, *g)
    want = dw_epilogue(acc, sa, ws, bias)
    B, ho, wo, O = want.shape
    assert tuple(y.shape) == (B, O, ho, wo) and y.dtype == torch.float32
    got = y.detach().cpu().permute(0, 2, 3, 1).contiguous().numpy()
    assert bits_equal(got, want), first_mismatch(got, want)
    check_bound(got, acc, sa, ws, bias)
    return want


CLASS_GEOMETRIES = [(2, 2, 0, 0), (3, 2, 1, 1), (4, 2, 1, 0), ((2, 3), (2, 1), (0, 1), (1, 0))]


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_conv_transpose2d_on_cpu_equals_the_loops(family, per_channel):
    from mct_quantizers_amd import consumers
    for i, (k, s, p, op) in enumerate(CLASS_GEOMETRIES):
        bias = (i + per_channel) % 2 == 0
        model = convt_model(k=k, stride=s, padding=p, output_padding=op, family=family, per_channel=per_channel, bias=bias, seed=i)
        x = torch.randn(2, 32, 5, 7) * 1.5
        ref = model(x)                                                   # fake-quant + float32 F.conv_transpose2d
        qc = consumers.QuantizedConvTranspose2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
        assert qc._a_zp not in (0, 128) and qc._a_qmin < qc._a_zp < qc._a_qmax and (qc.bias is not None) == bias
        y = qc(x)
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        kk, ss = model[1].layer.kernel_size, model[1].layer.stride
        assert tuple(qc._w_codes.shape) == (24, *kk, 32) and qc._w_codes.dtype == torch.int8 and qc._w_codes.is_contiguous()
        kp = -(-(-(-kk[0] // ss[0]) * -(-kk[1] // ss[1]) * 32) // 64) * 64
        assert tuple(qc._w_packed[0].shape) == (ss[0] * ss[1], 32, kp) and tuple(qc._w_packed[1].shape) == (ss[0] * ss[1], 24)
        assert tuple(qc._w_scales.shape) == (24,)
        check_transposed_against_loops_and_float64(qc, x, y)
        y_cl = qc(x.contiguous(memory_format=torch.channels_last))
        assert bits_equal(y_cl.numpy(), y.numpy())                      # both memory formats: the same bits
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
        if family == "uniform":
            assert qc._w_zps is not None and len(set(qc._w_zps.tolist())) > (1 if per_channel else 0)
        else:
            assert qc._w_zps is None


def test_the_output_channel_axis_is_1():
    from mct_quantizers_amd import consumers
    assert consumers.IntegerConsumer._out_axis == 0 and consumers.QuantizedConvTranspose2d._out_axis == 1
    assert all(cls._out_axis == 0 for cls in (consumers.QuantizedLinear, consumers.QuantizedConv1x1, consumers.QuantizedConv2d,
                                              consumers.QuantizedDepthwiseConv2d, consumers.QuantizedGroupedConv2d))
    for family in ("sym", "uniform", "lut16"):
        # C == O: a quantizer along the input channels has the right number of entries and is still refused
        holder, wrapper = convt_pair(C=32, O=32, family=family, axis=0)
        with pytest.raises(NotImplementedError, match="axis 1"):
            consumers.QuantizedConvTranspose2d.from_wrapper(wrapper, holder.activation_holder_quantizer)
        model = torch.nn.Sequential(holder, wrapper)
        assert consumers.fuse_linear_consumers(model, transposed=True, uniform_weights=True) == 0 and model[1] is wrapper
        gm, n = consumers.fuse_linear_consumers_fx(model, transposed=True, uniform_weights=True)
        assert n == 0
    # a convolution's axis-0 rule is what it was
    from test_conv_consumer import conv_pair
    holder, wrapper = conv_pair(C=16, O=16)
    wrapper.weights_quantizers["weight"].channel_axis = 1
    with pytest.raises(NotImplementedError, match="axis 0"):
        consumers.QuantizedConv2d.from_wrapper(wrapper, holder.activation_holder_quantizer)


def test_transposed_convolutions_the_consumer_cannot_take_stay():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    T = torch.nn.ConvTranspose2d
    E = consumers.QuantizedConvTranspose2d.eligible
    assert E(T(32, 24, 2, 2)) and E(T(32, 24, 3, 4, output_padding=3)) and E(T(16, 8, (3, 2), (1, 3), (2, 0), (0, 2)))
    assert E(T(2048, 4, 4, 1)) and E(T(2048, 4, 8, 2))                                   # 16 taps of 2048 channels: 32768
    for conv in (T(32, 32, 2, 2, groups=2), T(32, 32, 2, 2, groups=32), T(32, 24, 3, 1, dilation=2), T(32, 24, 5, 5), T(32, 24, 2, (2, 5)),
                 T(24, 16, 2, 2), T(2048, 4, 5, 1), T(4096, 4, 6, 2), torch.nn.Conv2d(32, 24, 3), torch.nn.ConvTranspose1d(32, 24, 2, 2)):
        assert not E(conv), conv
        with pytest.raises(TypeError):
            consumers.QuantizedConvTranspose2d(conv, None, None)
    odd = T(32, 24, 2, 2)
    odd.padding_mode = "reflect"                         # (the constructor takes zeros only; the attribute is what is read)
    assert not E(odd)
    left = {"groups": convt_model(C=32, O=32, groups=2), "dilation": convt_model(k=3, stride=1, dilation=2), "stride 5": convt_model(k=5, stride=5),
            "C=24": convt_model(C=24), "half": convt_model().half(), "uniform": convt_model(family="uniform")}
    every = dict(transposed=True, convolutions=True, depthwise=True, grouped=True, any_channels=True)
    for name, model in left.items():
        for kw in (dict(transposed=True), every):
            assert consumers.fuse_linear_consumers(model, **kw) == 0, name
            assert isinstance(model[1], mq.PytorchQuantizationWrapper), name
            if name != "half":
                gm, n = consumers.fuse_linear_consumers_fx(model, **kw)
                assert n == 0, name
    assert consumers.fuse_linear_consumers(left["uniform"], transposed=True, uniform_weights=True) == 1
    assert type(left["uniform"][1]) is consumers.QuantizedConvTranspose2d
    # the pad byte is the zero point: one outside the clamp domain cannot be taken
    model = convt_model()
    model[0].activation_holder_quantizer.zero_point = 300
    with pytest.raises(NotImplementedError, match="pad byte"):
        consumers.QuantizedConvTranspose2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
    assert consumers.fuse_linear_consumers(model, transposed=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)


def test_transposed_class_hierarchy_code_types_and_weight_refresh():
    from mct_quantizers_amd import consumers
    assert issubclass(consumers.QuantizedConvTranspose2d, consumers.IntegerConsumer)
    assert not issubclass(consumers.QuantizedConvTranspose2d, consumers.QuantizedLinear)
    holder, wrapper = convt_pair(act="signed")
    qc = consumers.QuantizedConvTranspose2d.from_wrapper(wrapper, holder.activation_holder_quantizer)
    assert qc(torch.zeros(2, 32, 4, 4, dtype=torch.int8)).dtype == torch.float32     # the quantizer's own code type is taken
    with pytest.raises(TypeError, match="do not match this layer's quantizer"):
        qc(torch.zeros(2, 32, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        qc(torch.zeros(2, 16, 4, 4))
    qc.emit_act = "hardswish"                                     # no entry point takes one: never silently dropped
    with pytest.raises(NotImplementedError):
        qc(torch.zeros(2, 32, 4, 4))
    qc.emit_act, qc.emit_residual = None, "float"
    with pytest.raises(NotImplementedError):
        qc(torch.zeros(2, 32, 4, 4))
    assert not consumers._takes_hard_activation(qc)
    # the codes follow the weight
    model = convt_model(family="lut16")
    assert consumers.fuse_linear_consumers(model, transposed=True) == 1
    qc, x = model[1], torch.randn(1, 32, 4, 4)
    y0, codes0, packed0 = model(x), qc._w_codes.clone(), qc._w_packed[0].clone()
    with torch.no_grad():
        qc.weight.mul_(-0.5)
    y1 = model(x)
    assert not torch.equal(codes0, qc._w_codes) and not torch.equal(packed0, qc._w_packed[0]) and not torch.equal(y0, y1)
    check_transposed_against_loops_and_float64(qc, x, y1)


# ---- the switch -----------------------------------------------------------------------------------------------------------

EXISTING_SWITCHES = (dict(), dict(convolutions=True), dict(convolutions=True, depthwise=True, grouped=True),
                     dict(convolutions=True, depthwise=True, grouped=True, uniform_weights=True, chain=True, any_channels=True,
                          pools=True, avg_pools=True, upsamples=True, activation_tables=True))
FX_ONLY = dict(shared_holders=True, stay_on_codes=True, fused_residuals=True, concats=True, muls=True, hard_activations=True)


def _graph_shape(gm):
    return [(n.op, n.target if isinstance(n.target, str) else getattr(n.target, "__name__", str(n.target))) for n in gm.graph.nodes], \
        [(name, type(m)) for name, m in gm.named_modules() if name]


def test_fusion_of_transposed_convolutions_is_opt_in():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    make = lambda: convt_model(k=3, stride=2, padding=1, output_padding=1)      # noqa: E731
    model = make()
    x = torch.randn(2, 32, 5, 7) * 1.5
    ref = model(x)
    for kw in EXISTING_SWITCHES:
        assert consumers.fuse_linear_consumers(model, **kw) == 0          # left alone, exactly as before
        assert isinstance(model[1], mq.PytorchQuantizationWrapper) and torch.equal(model(x), ref)
        for more in (dict(), FX_ONLY):
            gm, n = consumers.fuse_linear_consumers_fx(model, **kw, **more)
            assert n == 0 and torch.equal(gm(x), ref)
            assert [t for op, t in _graph_shape(gm)[0] if op == "call_module"] == ["0", "1"]
            assert [t for _, t in _graph_shape(gm)[1][:2]] == [type(model[0]), type(model[1])]
            gm_f, n_f = consumers.fuse_linear_consumers_fx(model, transposed=False, **kw, **more)
            assert n_f == 0 and _graph_shape(gm_f) == _graph_shape(gm)
    gm, n = consumers.fuse_linear_consumers_fx(make(), transposed=True)
    assert n == 1 and type(gm.get_submodule("1_qlinear")) is consumers.QuantizedConvTranspose2d
    assert [node.target for node in gm.graph.nodes if node.op == "call_module"] == ["1_qlinear"]
    y_fx = gm(x)
    assert consumers.fuse_linear_consumers(model, transposed=True) == 1
    assert isinstance(model[0], torch.nn.Identity) and type(model[1]) is consumers.QuantizedConvTranspose2d
    y = model(x)
    assert bits_equal(y.detach().numpy(), y_fx.detach().numpy())
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    check_transposed_against_loops_and_float64(model[1], x, y)
    # the switch is independent of the others: it takes no convolution, and convolutions=True takes no transposed one
    from test_conv_consumer import conv_model, conv_pair
    model = conv_model(C=32, O=16, k=3, padding=1)
    assert consumers.fuse_linear_consumers(model, transposed=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)
    assert consumers.fuse_linear_consumers(model, transposed=True, convolutions=True) == 1 and type(model[1]) is consumers.QuantizedConv2d
    # existing positional calls of _consumer_for mean what they meant: the seventh positional argument is grouped
    holder, wrapper = convt_pair()
    q = holder.activation_holder_quantizer
    assert consumers._consumer_for(wrapper, q, True, True, True, True, True) is None
    assert type(consumers._consumer_for(wrapper, q, transposed=True)) is consumers.QuantizedConvTranspose2d
    holder, wrapper = conv_pair(C=32, O=48, groups=4)
    assert type(consumers._consumer_for(wrapper, holder.activation_holder_quantizer, False, False, False, False, True)) \
        is consumers.QuantizedGroupedConv2d


def convt_stack(seed=0):
    """1x1 -> transposed 2x2 stride 2 -> 1x1, each behind its own activation holder (uint8 codes with a zero point, int8 codes,
    uint8 codes again)."""
    from test_conv_consumer import conv_pair
    return torch.nn.Sequential(*conv_pair(C=16, O=32, k=1, padding=0, seed=seed, act="uniform"),
                               *convt_pair(C=32, O=48, k=2, stride=2, seed=seed + 1, act="signed", family="uniform"),
                               *conv_pair(C=48, O=16, k=1, padding=0, seed=seed + 2, act="relu", family="lut16"))


def check_transposed_chain(device):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    plain, chained = convt_stack().to(device), convt_stack().to(device)
    kinds = [consumers.QuantizedConv1x1, consumers.QuantizedConvTranspose2d, consumers.QuantizedConv1x1]
    for model, chain in ((plain, False), (chained, True)):
        assert consumers.fuse_linear_consumers(model, chain=chain, uniform_weights=True, transposed=True) == 3
        assert [type(model[i]) for i in (1, 3, 5)] == kinds
    assert chained[1].emit_codes_for == chained[3].activation_code_params()
    assert chained[3].emit_codes_for == chained[5].activation_code_params() and chained[5].emit_codes_for is None
    x = (torch.randn(2, 16, 6, 5, generator=torch.Generator().manual_seed(11)) * 1.5).to(device)
    for upto, nxt, dt in ((2, chained[3], torch.int8), (4, chained[5], torch.uint8)):
        mid32, mid = plain[:upto](x), chained[:upto](x)
        assert mid32.dtype == torch.float32 and mid.dtype == dt and mid.shape == mid32.shape
        want = ops.fq_codes(mid32, None, None, None, nxt._a_qmin, nxt._a_qmax, nxt._a_scale, nxt._a_zp)
        assert torch.equal(mid, want) and len(torch.unique(want)) > 8     # the same codes, and not a saturated handful
    y = chained(x)
    assert y.dtype == torch.float32 and y.shape == (2, 16, 12, 10) and torch.equal(plain(x), y)
    return x, y


def test_chained_transposed_stack_gives_the_same_bits_cpu():
    check_transposed_chain("cpu")


# ---- the fx rewrite: a decoder stage with a learned upsampling ---------------------------------------------------------------

def pot_convt(C, O, k, seed, stride=2):
    """A wrapped transposed convolution without bias whose weights have power-of-two scales (tests/test_pool_consumer.py's
    pot_conv): with power-of-two activation scales every product and sum is exact in float32."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    conv = torch.nn.ConvTranspose2d(C, O, k, stride=stride, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 0.3 + 0.05)
    return mq.PytorchQuantizationWrapper(conv, {"weight": t_weights_quantizer(conv.weight, "pot", True)})


class Decoder(torch.nn.Module):
    """conv -> ReLU -> A -> ConvTranspose2d (2 x 2, stride 2) -> ReLU -> B -> cat([B, S]) -> C -> conv3x3, S the holder of the
    skip input; with ``sized`` the transposed convolution is called with ``output_size=``."""

    def __init__(self, sized=False):
        super().__init__()
        self.sized = sized
        self.h0 = holder_of("s4")
        self.first = pot_conv(16, 32, 1, 1)
        self.ha, self.hb, self.hs, self.hc = holder_of("u4"), holder_of("u8"), holder_of("u2"), holder_of("u4")
        self.up = pot_convt(32, 16, 2, 5)
        self.last = pot_conv(32, 16, 3, 2)

    def forward(self, x, skip):
        a = self.ha(torch.relu(self.first(self.h0(x))))
        u = self.up(a, output_size=(8, 10)) if self.sized else self.up(a)
        return self.last(self.hc(torch.cat([self.hb(torch.relu(u)), self.hs(skip)], 1)))


def low_input(device="cpu"):
    return (torch.randn(2, 16, 4, 5, generator=torch.Generator().manual_seed(12)) * 1.5).to(device)


def skip_input(device="cpu"):
    return (torch.randn(2, 16, 8, 10, generator=torch.Generator().manual_seed(13)).abs() * 0.7).to(device)


ALL = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, concats=True, muls=True, upsamples=True,
           fused_residuals=True, avg_pools=True, hard_activations=True, any_channels=True, activation_tables=True, grouped=True,
           depthwise=True, uniform_weights=True)


def check_decoder(device):
    """The decoder stage rewritten with every switch: returns (graph module, inputs, output)."""
    from mct_quantizers_amd import consumers
    x, skip = low_input(device), skip_input(device)
    gm, n = consumers.fuse_linear_consumers_fx(Decoder().to(device).eval(), transposed=True, **ALL)
    gm0, n0 = consumers.fuse_linear_consumers_fx(Decoder().to(device).eval(), **ALL)
    assert (n, n0) == (3, 2)
    assert _targets(gm) == ["first_qlinear", "up_qlinear", "hc_concat", "last_qlinear"] and not _targets(gm, "call_function")
    # without the switch: the graph every earlier version gives -- the transposed layer, holder A and both ReLUs stay in float32
    assert _targets(gm0) == ["first_qlinear", "ha", "up", "hc_concat", "last_qlinear"]
    assert _targets(gm0, "call_function") == [torch.relu, torch.relu]
    assert type(gm0.get_submodule("up")).__name__ == "PytorchQuantizationWrapper" and not any(
        isinstance(m, consumers.QuantizedConvTranspose2d) for m in gm0.modules())
    first, up, concat = (gm.get_submodule(t) for t in ("first_qlinear", "up_qlinear", "hc_concat"))
    assert type(up) is consumers.QuantizedConvTranspose2d
    assert first.emit_codes_for == up.activation_code_params() == (4.0 / 256, 0, 0, 255)
    assert up.emit_codes_for == concat.operand_code_params(0) == (8.0 / 256, 0, 0, 255)
    assert (up.emit_residual, up.emit_relu, up.emit_act) == (None, False, None)
    # no float32 tensor between A and the last convolution: codes into and out of the transposed layer, codes out of the
    # concatenation (its second operand is the float32 skip INPUT of the model)
    seen = {}
    hooks = [gm.get_submodule(t).register_forward_hook(lambda m, args, out, t=t: seen.update({t: ([a.dtype for a in args], out.dtype)}))
             for t in ("first_qlinear", "up_qlinear", "hc_concat", "last_qlinear")]
    with torch.no_grad():
        y = gm(x, skip)
        y0 = gm0(x, skip)
    for h in hooks:
        h.remove()
    assert seen["first_qlinear"][1] == torch.uint8 and seen["up_qlinear"] == ([torch.uint8], torch.uint8)
    assert seen["hc_concat"] == ([torch.uint8, torch.float32], torch.uint8) and seen["last_qlinear"] == ([torch.uint8], torch.float32)
    assert y.shape == (2, 16, 8, 10) and len(torch.unique(y)) > 50
    assert torch.equal(y, y0)                            # integer-exact weights: the float32 path gives the same bits
    return gm, (x, skip), y


def test_a_decoder_stage_with_a_transposed_convolution_runs_on_codes_cpu():
    from mct_quantizers_amd import consumers
    gm, (x, skip), y = check_decoder("cpu")
    with torch.no_grad():
        assert torch.equal(y, Decoder().eval()(x, skip))
    # under fewer switches: the same bits
    for switches in (dict(), dict(convolutions=True), dict(convolutions=True, concats=True, shared_holders=True)):
        gm1, n1 = consumers.fuse_linear_consumers_fx(Decoder().eval(), transposed=True, **switches)
        assert "up_qlinear" in _targets(gm1) and torch.equal(gm1(x, skip), y), switches
    # a call with output_size= is left alone: the graph is the one without the switch
    gm2, n2 = consumers.fuse_linear_consumers_fx(Decoder(sized=True).eval(), transposed=True, **ALL)
    gm20, n20 = consumers.fuse_linear_consumers_fx(Decoder(sized=True).eval(), **ALL)
    assert n2 == n20 and "up" in _targets(gm2) and "up_qlinear" not in _targets(gm2) and _graph_shape(gm2) == _graph_shape(gm20)
    with torch.no_grad():
        assert torch.equal(gm2(x, skip), y)


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_qconv_transposed_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_qconv_transposed_i8\s*\(", header) and "mctq_qconv_transposed_i8" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(a=P, adt=U8, za=114, sa=0.5, w=P, ws=P, rs=P, zw=None, bias=None, y=P, ydt=-1, y_scale=0.25, y_zp=0, qmin=0,
                 qmax=255, B=2, H=5, W=7, C=32, O=48, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, oph=1, opw=1)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_qconv_transposed_i8(v["a"], v["adt"], v["za"], v["sa"], v["w"], v["ws"], v["rs"], v["zw"], v["bias"], v["y"],
                                            v["ydt"], v["y_scale"], v["y_zp"], v["qmin"], v["qmax"], v["B"], v["H"], v["W"], v["C"],
                                            v["O"], v["kh"], v["kw"], v["sh"], v["sw"], v["ph"], v["pw"], v["oph"], v["opw"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWCO":
        refused(b"negative extent", **{extent: -1})
    for name in ("kh", "kw"):
        refused(b"kernel size below 1", **{name: 0})
    for name in ("sh", "sw"):
        refused(b"stride below 1", **{name: 0})
        refused(b"stride above 4: outside the transposed consumer's limit", **{name: 5})
    for name in ("ph", "pw"):
        refused(b"negative padding", **{name: -1})
    for name in ("oph", "opw"):
        refused(b"negative output padding", **{name: -1})
        refused(b"output padding must be smaller than the stride", **{name: 2})
    for fault in (dict(C=0), dict(O=0)):
        refused(b"channels and out_channels must be positive", **fault)
    for channels in (8, 24, 40):
        refused(b"channels must be a multiple of 16", C=channels)
    limit = b"taps of a phase * channels > 32768: outside the consumer's limit"
    refused(limit, C=2048, kh=5, kw=4, sh=1, sw=1, oph=0, opw=0)              # 20 taps
    refused(limit, C=32784)                                                     # C alone
    refused(limit, kh=2 ** 31 - 1, kw=2 ** 31 - 1)
    assert call(C=2048, kh=8, kw=8, B=0) == 0                                   # 16 taps per phase: 32768 is inside the limit
    refused(b"out_channels exceed 2^31 - 1", O=2 ** 31)
    refused(b"bad a_code_dtype", adt=77)
    for adt, za in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"a_zero_point is no code of a_code_dtype", adt=adt, za=za)
    for adt, za in ((U8, 0), (U8, 255), (I8, -128), (I8, 127)):
        assert call(adt=adt, za=za, B=0) == 0
    refused(b"bad y_code_dtype", ydt=9)
    refused(b"quant_min > quant_max", ydt=U8, qmin=200, qmax=100)
    refused(b"clamp domain does not fit the code type", ydt=U8, qmax=256)
    # wrong in two ways: the earlier check speaks
    refused(b"negative padding", ph=-1, C=24)
    refused(b"channels must be a multiple of 16", C=24, adt=77)
    refused(b"bad a_code_dtype", adt=77, za=256)
    refused(b"a_zero_point is no code of a_code_dtype", za=256, ydt=9)
    refused(b"bad y_code_dtype", ydt=9, H=2 ** 31)
    refused(b"image extent exceeds 2^31 - 1", H=2 ** 31)
    refused(b"the padding leaves no output (Ho <= 0 or Wo <= 0)", ph=6, a=None)            # 4 * 2 - 12 + 3 + 1 = 0
    refused(b"the padding leaves no output (Ho <= 0 or Wo <= 0)", pw=2 ** 31 - 1)
    refused(b"padded output extent exceeds 2^31 - 1", H=2 ** 30, sh=4, oph=0)
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, kh=4, ph=0)
    refused(b"too many output pixels for one launch", B=2 ** 31, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, oph=0, opw=0, H=1, W=1)
    refused(b"too many output pixels for one launch", B=2 ** 62, H=2 ** 20, W=2 ** 20)
    refused(b"the output tensor exceeds 2^63 - 1 bytes", B=2 ** 9, H=2 ** 10, W=2 ** 9, pw=0, O=2 ** 31 - 1)      # 2^20 * 1026 pixels
    refused(b"phases * ceil(out_channels / 64) > 65535: too many grid slices", O=64 * 16384)
    for pointer in ("a", "w", "ws", "rs", "y"):
        refused(b"NULL pointer", **{pointer: None})
    for pointer, off in (("a", 8), ("w", 4), ("ws", 4), ("rs", 8), ("y", 1), ("zw", 4), ("bias", 8)):
        refused(b"codes, weights, per-channel tables and output must be 16-byte aligned", **{pointer: P + off})
    nothing = dict(a=None, w=None, ws=None, rs=None, y=None)
    assert call(B=0) == 0 and call(B=0, **nothing) == 0                # no images: no launch, no pointer is looked at
    assert call(B=0, ydt=U8) == 0 and call(B=0, zw=P, bias=P) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
