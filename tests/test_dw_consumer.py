"""Depthwise convolutions on the integer consumer: host logic and the CPU route (include/mctq_hip.h: mctq_qconv_dw_i8;
consumers.qconv_dw_i8, consumers.QuantizedDepthwiseConv2d and the ``depthwise`` switch of fuse_linear_consumers /
fuse_linear_consumers_fx).

Oracle of every exactness check: plain numpy loops over (b, oy, ox, ky, kx) in int64, from the layer's own activation codes
and the weights quantizer's own codes of the float weight (zero points taken off as in tests/test_conv_consumer.py:
weight_operands), a tap outside the image skipped; then the epilogue of oracle/mctq_oracle.py::qlinear_i8 -- the float32
product of the two scales, the float32 conversion of the int32 sum, one float32 multiply, one float32 add.  The loops are
tied to the committed oracle once (test_the_loops_equal_the_committed_oracle_channel_by_channel): per channel c the
depthwise layer IS the product of a [M, kh * kw] patch matrix (padded taps hold za) with the one weight row w[:, :, c].

Bound against float64 (derived in tests/test_conv_consumer.py, the same four roundings): |y - y64| <= 2^-21 (|p64| + |bias|)
with p64 the exact integer sum times the float64 product of the two float32 scales; torch's float64 ``conv2d(groups=C)`` of
the dequantized tensors must agree with p64 to float64 accuracy.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES, conv_model, conv_pair, im2col_loops, out_hw, weight_operands

F32 = np.float32
# (kernel, stride, padding, dilation)
DW_GEOMETRIES = [((3, 3), (1, 1), (1, 1), (1, 1)), ((3, 3), (2, 2), (1, 1), (1, 1)), ((5, 5), (1, 1), (2, 2), (1, 1)),
                 ((3, 3), (1, 1), (2, 2), (2, 2)), ((1, 3), (1, 1), (0, 1), (1, 1)), ((7, 7), (2, 2), (3, 3), (1, 1))]
# ... and for the raw entry point alone: a 3 x 3 kernel without padding (on a 3 x 3 image: one output pixel)
RAW_GEOMETRIES = DW_GEOMETRIES + [((3, 3), (1, 1), (0, 0), (1, 1))]
ZERO_POINTS = {np.uint8: (0, 114, 255), np.int8: (-128, -3, 127)}


def dw_loops(a, za, w, k, s, p, d):
    """a [B, H, W, C] codes, w [kh, kw, C] integers (zero points already off) -> int64 sums [B, Ho, Wo, C]; taps outside
    the image add nothing."""
    B, H, W, C = a.shape
    ho, wo = out_hw(H, W, k, s, p, d)
    a64, w64 = a.astype(np.int64) - int(za), w.astype(np.int64)
    acc = np.zeros((B, ho, wo, C), dtype=np.int64)
    for b in range(B):
        for oy in range(ho):
            for ox in range(wo):
                for ky in range(k[0]):
                    for kx in range(k[1]):
                        iy, ix = oy * s[0] - p[0] + ky * d[0], ox * s[1] - p[1] + kx * d[1]
                        if 0 <= iy < H and 0 <= ix < W:
                            acc[b, oy, ox] += a64[b, iy, ix] * w64[ky, kx]
    return acc


def dw_epilogue(acc, sa, ws, bias):
    """oracle/mctq_oracle.py::qlinear_i8's epilogue on the sums [..., C]."""
    assert np.all(np.abs(acc) < 2 ** 31)
    sc = (F32(sa) * np.asarray(ws, dtype=F32).reshape(-1)).astype(F32)
    y = (acc.astype(np.int32).astype(F32) * sc).astype(F32)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=F32)).astype(F32)
    return y


def dw_oracle(a, za, sa, w, ws, bias, geometry):
    return dw_epilogue(dw_loops(a, za, w, *geometry), sa, ws, bias)


@functools.lru_cache(maxsize=None)
def raw_case(u8, C, gi, za, with_zp, with_bias, B=2, H=5, W=7):
    """Seeded operands of one raw call and the loops' float32 result, computed once and shared by the CPU and GPU tests;
    read-only.  Zero points of both signs, -128 and 127 among them."""
    rng = np.random.default_rng(7919 * C + 31 * gi + 5 * (za + 128) + 2 * with_zp + with_bias + 1000 * B + H)
    g = RAW_GEOMETRIES[gi]
    a = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8).view(np.uint8 if u8 else np.int8)
    w = rng.integers(-128, 128, (*g[0], C)).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, C).astype(F32)
    zw = None
    if with_zp:
        zw = rng.integers(-128, 128, C).astype(np.int32)
        zw[:4] = (-128, 127, 0, -1)
    bias = rng.normal(0, 2.0, C).astype(F32) if with_bias else None
    sa = 0.0173
    want = dw_oracle(a, za, sa, w.astype(np.int64) - (0 if zw is None else zw.astype(np.int64)), ws, bias, g)
    for t in (a, w, ws, zw, bias, want):
        if t is not None:
            t.setflags(write=False)
    return dict(a=a, za=za, sa=sa, w=w, ws=ws, zw=zw, bias=bias, geometry=g, want=want)


def extreme_case():
    """The largest magnitude the sum of a 7 x 7 kernel reaches: every activation code 255 with za = 0, every weight -128 with
    zw = 127 -- 49 * 255 * -255 at the pixels that see all taps."""
    C, g = 16, ((7, 7), (1, 1), (3, 3), (1, 1))
    a = np.full((1, 7, 7, C), 255, dtype=np.uint8)
    w = np.full((7, 7, C), -128, dtype=np.int8)
    zw = np.full(C, 127, dtype=np.int32)
    ws = np.linspace(0.001, 0.01, C).astype(F32)
    bias = np.linspace(-3, 3, C).astype(F32)
    acc = dw_loops(a, 0, w.astype(np.int64) - 127, *g)
    assert acc.min() == -49 * 255 * 255
    return dict(a=a, za=0, sa=0.031, w=w, ws=ws, zw=zw, bias=bias, geometry=g, want=dw_epilogue(acc, 0.031, ws, bias))


def run_raw_on(case, device="cpu", out_codes=None):
    from mct_quantizers_amd import consumers
    t = lambda v: None if v is None else torch.from_numpy(v.copy()).to(device)      # noqa: E731
    return consumers.qconv_dw_i8(t(case["a"]), case["za"], case["sa"], t(case["w"]), t(case["ws"]), t(case["bias"]),
                                 *case["geometry"], out_codes=out_codes, w_zero_points=t(case["zw"]))


def raw_cases():
    """(code type, C, geometry, zero point, weight zero points?, bias?): every geometry with each code type, each C and each of
    the type's three zero points; weight zero points and bias alternate on and off with different periods, so that every
    geometry, C and code type meets both settings of both."""
    n = 0
    for u8 in (True, False):
        for C in (16, 48):
            for gi in range(len(DW_GEOMETRIES)):
                for za in ZERO_POINTS[np.uint8 if u8 else np.int8]:
                    n += 1
                    yield u8, C, gi, za, n % 2 == 0, n % 3 != 0


def test_the_loops_equal_the_committed_oracle_channel_by_channel():
    from oracle import mctq_oracle as O
    for u8, gi, za, with_zp in ((True, 0, 114, True), (False, 1, -3, False), (True, 3, 255, True), (False, 5, -128, True)):
        c = raw_case(u8, 16, gi, za, with_zp, True)
        k, s, p, d = c["geometry"]
        w = c["w"].astype(np.int64) - (0 if c["zw"] is None else c["zw"].astype(np.int64))
        B, ho, wo = c["a"].shape[0], *out_hw(5, 7, k, s, p, d)
        want = c["want"].reshape(B * ho * wo, -1)
        for ch in range(16):
            patches = im2col_loops(np.ascontiguousarray(c["a"][..., ch:ch + 1]), k, s, p, d, za)     # [M, kh * kw], padded taps = za
            col = O.qlinear_i8(patches, za, c["sa"], w[:, :, ch].reshape(1, -1), c["ws"][ch:ch + 1], c["bias"][ch:ch + 1])
            assert bits_equal(col[:, 0], want[:, ch]), (gi, ch, first_mismatch(col[:, 0], want[:, ch]))


def test_qconv_dw_i8_on_cpu_equals_the_loops():
    n = 0
    for case in raw_cases():
        c = raw_case(*case)
        y = run_raw_on(c)
        assert y.dtype == torch.float32 and y.shape == c["want"].shape and y.is_contiguous()
        assert bits_equal(y.numpy(), c["want"]), (case, first_mismatch(y.numpy(), c["want"]))
        n += 1
    assert n == 2 * 2 * 6 * 3
    # ints stand for pairs, as in torch.nn.Conv2d
    from mct_quantizers_amd import consumers
    c = raw_case(True, 16, 1, 114, False, True)
    y = consumers.qconv_dw_i8(torch.from_numpy(c["a"].copy()), 114, c["sa"], torch.from_numpy(c["w"].copy()),
                              torch.from_numpy(c["ws"].copy()), torch.from_numpy(c["bias"].copy()), 3, 2, 1, 1)
    assert bits_equal(y.numpy(), c["want"])


def test_qconv_dw_i8_on_cpu_edge_values_and_output_codes():
    from mct_quantizers_amd.hip import ops
    c = extreme_case()
    y = run_raw_on(c)
    assert bits_equal(y.numpy(), c["want"]), first_mismatch(y.numpy(), c["want"])
    for u8 in (True, False):
        for za in ZERO_POINTS[np.uint8 if u8 else np.int8]:
            c = raw_case(u8, 16, 0, za, True, True)
            y = run_raw_on(c)
            assert bits_equal(y.numpy(), c["want"]), (u8, za)
            for form in ((0.37, 114, 0, 255), (0.41, -5, -128, 127), (0.2, 3, -8, 7)):
                codes = run_raw_on(c, out_codes=form)
                want = ops.fq_codes(y, None, None, None, form[2], form[3], form[0], form[1])
                assert codes.dtype == (torch.uint8 if form[2] >= 0 else torch.int8) and torch.equal(codes, want)
                assert len(torch.unique(want)) > (8 if form[3] > 7 else 4)


def test_qconv_dw_i8_refuses_bad_operands():
    from mct_quantizers_amd import consumers
    c = raw_case(True, 16, 0, 114, True, True)
    a, w, ws, b, zw = (torch.from_numpy(c[k].copy()) for k in ("a", "w", "ws", "bias", "zw"))
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a.float(), 114, 0.1, w, ws, b, 3, 1, 1)
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a[0], 114, 0.1, w, ws, b, 3, 1, 1)
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a, 114, 0.1, w.to(torch.int32), ws, b, 3, 1, 1)
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a, 114, 0.1, w.permute(2, 0, 1).contiguous(), ws, b, 3, 1, 1)       # [C, kh, kw]
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a, 114, 0.1, w, ws.double(), b, 3, 1, 1)
    with pytest.raises(TypeError):
        consumers.qconv_dw_i8(a, 114, 0.1, w, ws, b, 3, 1, 1, w_zero_points=zw.long())
    with pytest.raises(RuntimeError):
        consumers.qconv_dw_i8(a, 114, 0.1, w, ws, b, 3, 1, 1, w_zero_points=zw[:8].contiguous())
    with pytest.raises(ValueError):
        consumers.qconv_dw_i8(a, 256, 0.1, w, ws, b, 3, 1, 1)                                      # no uint8 code
    with pytest.raises(ValueError):
        consumers.qconv_dw_i8(a, 114, 0.1, w, ws, b, 3, 0, 1)
    with pytest.raises(ValueError, match="qconv_dw_i8: stride"):                                   # refused in this function's own name
        consumers.qconv_dw_i8(a, 114, 0.1, w, ws, b, 3, (1, 1, 1), 1)
    with pytest.raises(ValueError):
        consumers.qconv_dw_i8(a, 114, 0.1, torch.zeros(9, 9, 16, dtype=torch.int8), ws, b, 9, 1, 1)  # 9 > 5 + 2


# ---- wrapped depthwise convolutions ---------------------------------------------------------------------------------------

def dw_model(C=16, **kw):
    return conv_model(C=C, O=C, groups=C, **kw)


def dw_weight_operands(qc):
    """(integer codes [kh, kw, C] with the zero points off, float32 scales [C]) from the weights quantizer's own codes."""
    w, ws = weight_operands(qc)                                  # [C, kh * kw] of the [C, 1, kh, kw] weight
    kh, kw = qc.kernel_size
    return w.reshape(-1, kh, kw).transpose(1, 2, 0), ws


def check_dw_against_oracle_and_float64(qc, x, y):
    """x: the float32 [B, C, H, W] input of the fused layer ``qc`` (any memory format, any device), y its float32 output:
    bit-equal to the loops on the layer's own activation codes, and within the derived bound of the float64 convolution of
    the dequantized operands (module docstring)."""
    from mct_quantizers_amd.hip import ops
    g = (qc.kernel_size, qc.stride, qc.padding, qc.dilation)
    za, sa = qc._a_zp, qc._a_scale
    a = ops.fq_codes_nhwc(x.detach(), qc._a_qmin, qc._a_qmax, sa, za).cpu().numpy()
    w, ws = dw_weight_operands(qc)
    bias = None if qc.bias is None else qc.bias.detach().cpu().numpy()
    acc = dw_loops(a, za, w, *g)
    want = dw_epilogue(acc, sa, ws, bias)
    B, ho, wo, C = acc.shape
    assert tuple(y.shape) == (B, C, ho, wo) and y.dtype == torch.float32
    got = y.detach().cpu().permute(0, 2, 3, 1).contiguous().numpy()
    assert bits_equal(got, want), first_mismatch(got, want)
    p64 = acc.astype(np.float64) * (np.float64(F32(sa)) * ws.astype(np.float64))
    b64 = np.zeros(C) if bias is None else bias.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (p64 + b64))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64))
    assert np.all(err <= bound), float((err - bound).max())
    # the same float64 convolution by torch, from the dequantized tensors in their own layouts
    a64 = torch.from_numpy((a.astype(np.float64) - za) * np.float64(F32(sa))).permute(0, 3, 1, 2)
    w64 = torch.from_numpy(w.astype(np.float64) * ws.astype(np.float64)).permute(2, 0, 1).unsqueeze(1)       # [C, 1, kh, kw]
    y64 = torch.nn.functional.conv2d(a64, w64, torch.from_numpy(b64), g[1], g[2], g[3], groups=C).permute(0, 2, 3, 1).numpy()
    assert np.allclose(y64, p64 + b64, rtol=1e-12, atol=1e-12 * float(np.abs(p64).max() + 1.0))
    return want


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_depthwise_conv2d_on_cpu_equals_the_oracle(family, per_channel):
    from mct_quantizers_amd import consumers
    for i, (k, s, p, d) in enumerate(DW_GEOMETRIES):
        bias = (i + per_channel) % 2 == 0
        model = dw_model(k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel, bias=bias, seed=i)
        x = torch.randn(2, 16, 5, 7) * 1.5
        ref = model(x)                                                   # fake-quant + float32 grouped F.conv2d
        qc = consumers.QuantizedDepthwiseConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
        assert qc._a_zp not in (0, 128) and qc._a_qmin < qc._a_zp < qc._a_qmax and (qc.bias is not None) == bias
        y = qc(x)
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert tuple(qc._w_codes.shape) == (*k, 16) and qc._w_codes.dtype == torch.int8 and qc._w_codes.is_contiguous()
        check_dw_against_oracle_and_float64(qc, x, y)
        y_cl = qc(x.contiguous(memory_format=torch.channels_last))
        assert bits_equal(y_cl.numpy(), y.numpy())                      # both memory formats: the same bits
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
        if family == "uniform":
            assert qc._w_zps is not None and len(set(qc._w_zps.tolist())) > (1 if per_channel else 0)
        else:
            assert qc._w_zps is None


def test_depthwise_weight_codes_follow_the_weight():
    from mct_quantizers_amd import consumers
    model = dw_model(family="lut16")
    assert consumers.fuse_linear_consumers(model, depthwise=True) == 1
    qc, x = model[1], torch.randn(1, 16, 4, 4)
    y0, codes0 = model(x), model[1]._w_codes.clone()
    with torch.no_grad():
        qc.weight.mul_(-0.5)
    y1 = model(x)
    assert not torch.equal(codes0, qc._w_codes) and not torch.equal(y0, y1)
    check_dw_against_oracle_and_float64(qc, x, y1)


def test_fusion_of_depthwise_convolutions_is_opt_in():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    model = dw_model(C=32, k=3, padding=1)
    x = torch.randn(2, 32, 5, 7) * 1.5
    ref = model(x)
    for kw in (dict(), dict(convolutions=True), dict(convolutions=True, uniform_weights=True, chain=True)):
        assert consumers.fuse_linear_consumers(model, **kw) == 0          # left alone, exactly as before
        assert isinstance(model[1], mq.PytorchQuantizationWrapper) and torch.equal(model(x), ref)
        gm, n = consumers.fuse_linear_consumers_fx(model, **kw)
        assert n == 0 and torch.equal(gm(x), ref)
    assert consumers.fuse_linear_consumers(model, depthwise=True) == 1
    assert isinstance(model[0], torch.nn.Identity) and type(model[1]) is consumers.QuantizedDepthwiseConv2d
    y = model(x)
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    check_dw_against_oracle_and_float64(model[1], x, y)
    # depthwise=True alone leaves an ungrouped 3x3 layer to ``convolutions``
    model = conv_model(C=32, O=16, k=3, padding=1)
    assert consumers.fuse_linear_consumers(model, depthwise=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)
    assert consumers.fuse_linear_consumers(model, depthwise=True, convolutions=True) == 1
    assert type(model[1]) is consumers.QuantizedConv2d


def test_depthwise_convolutions_the_consumer_cannot_take_stay():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    left = {
        "groups=2": conv_model(C=32, O=16, groups=2),
        "multiplier 2": conv_model(C=16, O=32, groups=16),
        "C=24": dw_model(C=24),
        "reflect": dw_model(padding_mode="reflect"),
        "same 2x2": dw_model(k=2, padding="same"),
        "half": dw_model().half(),
        "uniform": dw_model(family="uniform"),
    }
    for name, model in left.items():
        for kw in (dict(depthwise=True), dict(depthwise=True, convolutions=True)):
            assert consumers.fuse_linear_consumers(model, **kw) == 0, name
            assert isinstance(model[1], mq.PytorchQuantizationWrapper), name
    assert consumers.fuse_linear_consumers(left["uniform"], depthwise=True, uniform_weights=True) == 1
    assert type(left["uniform"][1]) is consumers.QuantizedDepthwiseConv2d
    # the pad byte is the zero point: one outside the clamp domain cannot be taken
    model = dw_model()
    model[0].activation_holder_quantizer.zero_point = 300
    with pytest.raises(NotImplementedError, match="pad byte"):
        consumers.QuantizedDepthwiseConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
    assert consumers.fuse_linear_consumers(model, depthwise=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)
    with pytest.raises(TypeError):
        consumers.QuantizedDepthwiseConv2d(torch.nn.Conv2d(32, 32, 3, groups=2), None, None)
    with pytest.raises(TypeError):
        consumers.QuantizedDepthwiseConv2d(torch.nn.Conv2d(16, 16, 17, groups=16), None, None)      # 289 taps


def test_valid_and_same_padding_strings_depthwise():
    from mct_quantizers_amd import consumers
    for padding, k, d in (("valid", 3, 1), ("same", 3, 1), ("same", (3, 5), (2, 1))):
        model = dw_model(k=k, padding=padding, dilation=d)
        x = torch.randn(1, 16, 6, 7) * 1.5
        ref = model(x)
        assert consumers.fuse_linear_consumers(model, depthwise=True) == 1
        y = model(x)
        assert y.shape == ref.shape
        check_dw_against_oracle_and_float64(model[1], x, y)


def dw_stack(seed=0):
    """1x1 expand -> depthwise 3x3 -> 1x1 project, each behind its own activation holder (different quantizers: uint8 codes
    with a zero point, int8 codes, uint8 codes again)."""
    return torch.nn.Sequential(*conv_pair(C=16, O=32, k=1, padding=0, seed=seed, act="uniform"),
                               *conv_pair(C=32, O=32, k=3, padding=1, groups=32, seed=seed + 1, act="signed", family="uniform"),
                               *conv_pair(C=32, O=16, k=1, padding=0, seed=seed + 2, act="relu", family="lut16"))


def check_dw_chain(device):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    plain, chained = dw_stack().to(device), dw_stack().to(device)
    kinds = [consumers.QuantizedConv1x1, consumers.QuantizedDepthwiseConv2d, consumers.QuantizedConv1x1]
    for model, chain in ((plain, False), (chained, True)):
        assert consumers.fuse_linear_consumers(model, chain=chain, uniform_weights=True, depthwise=True) == 3
        assert [type(model[i]) for i in (1, 3, 5)] == kinds
    assert plain[1].emit_codes_for is None and plain[3].emit_codes_for is None
    assert chained[1].emit_codes_for == chained[3].activation_code_params()
    assert chained[3].emit_codes_for == chained[5].activation_code_params() and chained[5].emit_codes_for is None
    # (its own generator: building the layers draws from the global one, and not the same numbers on every device)
    x = (torch.randn(2, 16, 6, 5, generator=torch.Generator().manual_seed(11)) * 1.5).to(device)
    for upto, nxt, dt in ((2, chained[3], torch.int8), (4, chained[5], torch.uint8)):
        mid32, mid = plain[:upto](x), chained[:upto](x)
        assert mid32.dtype == torch.float32 and mid.dtype == dt and mid.shape == mid32.shape
        want = ops.fq_codes(mid32, None, None, None, nxt._a_qmin, nxt._a_qmax, nxt._a_scale, nxt._a_zp)
        assert torch.equal(mid, want) and len(torch.unique(want)) > 8     # the same codes, and not a saturated handful
    y = chained(x)
    assert y.dtype == torch.float32 and torch.equal(plain(x), y)
    return x, y


def test_chained_depthwise_block_gives_the_same_bits_cpu():
    check_dw_chain("cpu")


class InvertedResidual(torch.nn.Module):
    """1x1 expand -> ReLU6 -> depthwise 3x3 -> ReLU6 -> 1x1 project, plus the input (MobileNetV2's block)."""

    def __init__(self, C=16, E=32):
        super().__init__()
        self.h1, self.c1 = conv_pair(C=C, O=E, k=1, padding=0, seed=1)
        self.h2, self.c2 = conv_pair(C=E, O=E, k=3, padding=1, groups=E, seed=2, act="relu")
        self.h3, self.c3 = conv_pair(C=E, O=C, k=1, padding=0, seed=3, act="relu")

    def forward(self, x):
        y = torch.nn.functional.relu6(self.c1(self.h1(x)))
        y = torch.nn.functional.relu6(self.c2(self.h2(y)))
        return x + self.c3(self.h3(y))


def check_inverted_residual(device):
    from mct_quantizers_amd import consumers
    model = InvertedResidual().to(device)
    x = (torch.randn(2, 16, 9, 7, generator=torch.Generator().manual_seed(5)) * 1.5).to(device)
    ref = model(x)
    gm0, n0 = consumers.fuse_linear_consumers_fx(InvertedResidual().to(device))
    assert n0 == 2 and [node.target for node in gm0.graph.nodes if node.op == "call_module"] == ["c1_qlinear", "h2", "c2", "c3_qlinear"]
    gm, n = consumers.fuse_linear_consumers_fx(model, depthwise=True)
    assert n == 3
    fused = {name: type(m) for name, m in gm.named_modules() if isinstance(m, consumers.IntegerConsumer)}
    assert fused == {"c1_qlinear": consumers.QuantizedConv1x1, "c2_qlinear": consumers.QuantizedDepthwiseConv2d,
                     "c3_qlinear": consumers.QuantizedConv1x1}
    assert [node.target for node in gm.graph.nodes if node.op == "call_module"] == ["c1_qlinear", "c2_qlinear", "c3_qlinear"]
    seen = {}
    hook = gm.get_submodule("c2_qlinear").register_forward_hook(lambda m, args, out: seen.update(x=args[0], y=out))
    y = gm(x)
    hook.remove()
    assert y.shape == ref.shape == x.shape
    check_dw_against_oracle_and_float64(gm.get_submodule("c2_qlinear"), seen["x"], seen["y"])
    assert torch.allclose(y, ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))
    return gm, x, y


def test_fx_rewrite_of_an_inverted_residual_cpu():
    check_inverted_residual("cpu")


# ---- what the four consumer classes share -----------------------------------------------------------------------------------

CLASSES = ["QuantizedLinear", "QuantizedConv1x1", "QuantizedConv2d", "QuantizedDepthwiseConv2d"]


def consumer_pairs(act="signed"):
    """class name -> ([activation holder, wrapped layer], the shape of its input): a Linear with 16 inputs, 16-channel
    convolutions on a 4 x 4 image."""
    import mct_quantizers_amd as mq
    from test_conv_consumer import activation_quantizer, weights_quantizer
    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 24)
    linear = [mq.PytorchActivationQuantizationHolder(activation_quantizer(act)),
              mq.PytorchQuantizationWrapper(lin, {"weight": weights_quantizer(lin.weight, "sym", True)})]
    image = (2, 16, 4, 4)
    return {"QuantizedLinear": (linear, (3, 16)), "QuantizedConv1x1": (conv_pair(k=1, padding=0, act=act), image),
            "QuantizedConv2d": (conv_pair(act=act), image), "QuantizedDepthwiseConv2d": (conv_pair(O=16, groups=16, act=act), image)}


@pytest.mark.parametrize("name", CLASSES)
def test_activation_codes_of_the_wrong_type_are_refused(name):
    from mct_quantizers_amd import consumers
    (holder, wrapper), shape = consumer_pairs("signed")[name]
    qc = getattr(consumers, name).from_wrapper(wrapper, holder.activation_holder_quantizer)
    assert qc(torch.zeros(shape, dtype=torch.int8)).dtype == torch.float32           # the quantizer's own code type is taken
    with pytest.raises(TypeError, match="do not match this layer's quantizer"):
        qc(torch.zeros(shape, dtype=torch.uint8))


def test_consumer_class_hierarchy():
    from mct_quantizers_amd import consumers
    assert all(issubclass(getattr(consumers, name), consumers.IntegerConsumer) for name in CLASSES)
    assert issubclass(consumers.QuantizedConv1x1, consumers.QuantizedLinear)          # products over rows: they call its forward
    assert issubclass(consumers.QuantizedConv2d, consumers.QuantizedLinear)
    assert not issubclass(consumers.QuantizedDepthwiseConv2d, consumers.QuantizedLinear)


def test_consumers_construct_no_stand_in_layers(monkeypatch):
    """A consumer reads geometry and bias from the wrapped layer and owns the wrapper's weight: it builds no nn.Linear or
    nn.Conv2d of its own, at construction or on forward."""
    from mct_quantizers_amd import consumers
    pairs = consumer_pairs("uniform")                      # the wrapped models first: they need the real constructors

    def refuse(self, *args, **kwargs):
        raise AssertionError(f"a consumer constructed a {type(self).__name__}")

    monkeypatch.setattr(torch.nn.Linear, "__init__", refuse)
    monkeypatch.setattr(torch.nn.Conv2d, "__init__", refuse)
    with pytest.raises(AssertionError):
        torch.nn.Linear(16, 16)                            # (the patch is in place)
    for name, ((holder, wrapper), shape) in pairs.items():
        qc = getattr(consumers, name).from_wrapper(wrapper, holder.activation_holder_quantizer)
        assert type(qc) is getattr(consumers, name) and qc.weight is wrapper.weight and qc.bias is wrapper.layer.bias
        assert qc(torch.randn(shape)).dtype == torch.float32


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_qconv_dw_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_qconv_dw_i8\s*\(", header) and "mctq_qconv_dw_i8" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(a=P, adt=U8, za=114, sa=0.5, w=P, ws=P, zw=None, bias=None, y=P, ydt=-1, y_scale=0.25, y_zp=0, qmin=0, qmax=255,
                 B=2, H=5, W=7, C=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_qconv_dw_i8(v["a"], v["adt"], v["za"], v["sa"], v["w"], v["ws"], v["zw"], v["bias"], v["y"], v["ydt"],
                                    v["y_scale"], v["y_zp"], v["qmin"], v["qmax"], v["B"], v["H"], v["W"], v["C"], v["kh"], v["kw"],
                                    v["sh"], v["sw"], v["ph"], v["pw"], v["dh"], v["dw"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWC":
        refused(b"negative extent", **{extent: -1})
    for name in ("kh", "kw"):
        refused(b"kernel size below 1", **{name: 0})
    for name in ("sh", "sw"):
        refused(b"stride below 1", **{name: 0})
    for name in ("dh", "dw"):
        refused(b"dilation below 1", **{name: 0})
    for name in ("ph", "pw"):
        refused(b"negative padding", **{name: -1})
    refused(b"channels must be a multiple of 16", C=24)
    refused(b"kh * kw > 256: outside the depthwise consumer's limit", kh=17, kw=16, ph=8, pw=8)
    refused(b"kh * kw > 256: outside the depthwise consumer's limit", kh=2 ** 31 - 1, kw=2 ** 31 - 1, ph=2 ** 30, pw=2 ** 30)
    assert call(kh=16, kw=16, ph=8, pw=8, B=0) == 0                       # 256 taps are inside the limit
    refused(b"bad a_code_dtype", adt=77)
    for adt, za in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"a_zero_point is no code of a_code_dtype", adt=adt, za=za)
    for adt, za in ((U8, 0), (U8, 255), (I8, -128), (I8, 127)):
        assert call(adt=adt, za=za, B=0) == 0
    refused(b"bad y_code_dtype", ydt=9)
    refused(b"quant_min > quant_max", ydt=U8, qmin=200, qmax=100)
    refused(b"clamp domain does not fit the code type", ydt=U8, qmax=256)
    refused(b"clamp domain does not fit the code type", ydt=I8, qmin=-129, qmax=127)
    refused(b"clamp domain does not fit the code type", ydt=I8, qmin=-128, qmax=128)
    # wrong in two ways: the window's sizes, the channels, the tap limit, the activations' form, the output's, then the fit
    refused(b"negative padding", ph=-1, C=24)
    refused(b"channels must be a multiple of 16", C=24, kh=17, kw=16)
    refused(b"kh * kw > 256: outside the depthwise consumer's limit", kh=17, kw=16, adt=77)
    refused(b"bad a_code_dtype", adt=77, za=256)
    refused(b"a_zero_point is no code of a_code_dtype", za=256, ydt=9)
    refused(b"bad y_code_dtype", ydt=9, H=2 ** 31)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31, kw=16)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8, a=None)
    assert call(H=2 ** 31 - 3, B=0) == 0                                                          # the padded extent alone counts, not the kernel
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31)
    refused(b"padded image extent exceeds 2^31 - 1", W=2 ** 31 - 2)                               # + 2 of padding
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8)              # 8 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=5, dw=3)        # 13 > 7 + 2
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, kh=1)                # room for the kernel in the padding alone
    refused(b"too many output pixels for one launch", B=2 ** 31, kh=1, kw=1, ph=0, pw=0, H=1, W=1)
    refused(b"too many output pixels for one launch", B=2 ** 62, H=2 ** 20, W=2 ** 20, kh=1, kw=1, ph=0, pw=0)
    refused(b"more than 2^32 - 1 16-channel chunks of output in one launch", B=2 ** 28, kh=1, kw=1, ph=0, pw=0, H=1, W=1, C=512)
    for pointer in ("a", "w", "ws", "y"):
        refused(b"NULL pointer", **{pointer: None})
    for pointer, off in (("a", 8), ("w", 4), ("ws", 4), ("y", 1), ("zw", P + 4), ("bias", P + 8)):
        refused(b"codes, weights, per-channel tables and output must be 16-byte aligned",
                **{pointer: off if pointer in ("zw", "bias") else P + off})
    nothing = dict(a=None, w=None, ws=None, y=None)
    assert call(B=0) == 0 and call(B=0, **nothing) == 0                # no images: no launch, no pointer is looked at
    assert call(C=0) == 0 and call(C=0, **nothing) == 0                # no channels: nothing to write
    assert call(B=0, ydt=U8) == 0 and call(B=0, zw=P, bias=P) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
