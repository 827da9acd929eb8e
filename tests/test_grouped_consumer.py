"""Grouped convolutions on the integer consumer: host logic and the CPU route (include/mctq_hip.h: mctq_qconv_grouped_i8;
consumers.qconv_grouped_i8, consumers.QuantizedGroupedConv2d and the ``grouped`` switch of fuse_linear_consumers /
fuse_linear_consumers_fx).

Oracle of every exactness check: plain numpy loops over (b, oy, ox, ky, kx) in int64 -- per tap the G small products of the
group's Cg activation codes (zero point off) with its [Og, Cg] weight codes (zero points off), a tap outside the image skipped
-- then the depthwise tests' epilogue (tests/test_dw_consumer.py: dw_epilogue, that of oracle/mctq_oracle.py::qlinear_i8): the
float32 product of the two scales, the float32 conversion of the int32 sum, one float32 multiply, one float32 add.

Bound against float64 (derived in tests/test_conv_consumer.py, the same four roundings): |y - y64| <= 2^-21 (|p64| + |bias|)
with p64 the exact integer sum times the float64 product of the two float32 scales; torch's float64 ``conv2d(groups=G)`` of the
dequantized tensors must agree with p64 to float64 accuracy (rtol 1e-12).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES, conv_model, conv_pair, out_hw, weight_operands
from test_dw_consumer import DW_GEOMETRIES, RAW_GEOMETRIES, ZERO_POINTS, dw_epilogue

F32 = np.float32
# (Cg, Og, G): the smallest shapes at which the kernel can go wrong
GROUP_SHAPES = [(4, 4, 8),        # piece size 4
                (12, 8, 2),       # piece size 4, a 16-byte chunk spans more than one tap
                (8, 12, 4),       # piece size 8
                (24, 24, 2),      # piece size 8, three pieces per tap
                (16, 16, 2),      # piece size 16, a full N tile and no spare column
                (32, 20, 2),      # piece size 16
                (64, 16, 2),      # piece size 16; with a 1 x 1 kernel Kg = 64: no K tail
                (16, 80, 2)]      # two grid slices over N
FORMS = ((0.37, 114, 0, 255), (0.41, -5, -128, 127))            # codes out: a uint8 / an int8 quantizer
# the six geometries every shape runs, and for single cases: 3 x 3 without padding (index 6), 1 x 1 (index 7)
GEOMETRIES = RAW_GEOMETRIES + [((1, 1), (1, 1), (0, 0), (1, 1))]
UNPADDED_3X3, POINTWISE = len(DW_GEOMETRIES), len(DW_GEOMETRIES) + 1


def piece_size(cg):
    return 16 if cg % 16 == 0 else 8 if cg % 8 == 0 else 4


def grouped_loops(a, za, w, groups, k, s, p, d):
    """a [B, H, W, C] codes, w [O, kh, kw, Cg] integers (zero points already off) -> int64 sums [B, Ho, Wo, O]; taps outside
    the image add nothing."""
    B, H, W, C = a.shape
    O, cg, og = w.shape[0], C // groups, w.shape[0] // groups
    assert w.shape == (O, k[0], k[1], cg) and cg * groups == C and og * groups == O
    ho, wo = out_hw(H, W, k, s, p, d)
    a64 = (a.astype(np.int64) - int(za)).reshape(B, H, W, groups, cg)
    w64 = w.astype(np.int64).reshape(groups, og, k[0], k[1], cg)
    acc = np.zeros((B, ho, wo, groups, og), dtype=np.int64)
    for b in range(B):
        for oy in range(ho):
            for ox in range(wo):
                for ky in range(k[0]):
                    for kx in range(k[1]):
                        iy, ix = oy * s[0] - p[0] + ky * d[0], ox * s[1] - p[1] + kx * d[1]
                        if 0 <= iy < H and 0 <= ix < W:
                            acc[b, oy, ox] += np.einsum("gc,goc->go", a64[b, iy, ix], w64[:, :, ky, kx])
    return acc.reshape(B, ho, wo, O)


def grouped_oracle(a, za, sa, w, ws, bias, groups, geometry):
    return dw_epilogue(grouped_loops(a, za, w, groups, *geometry), sa, ws, bias)


@functools.lru_cache(maxsize=None)
def raw_case(u8, si, gi, za, with_zp, with_bias, B=2, H=5, W=7):
    """Seeded operands of one raw call and the loops' float32 result, computed once and shared by the CPU and GPU tests;
    read-only.  Zero points of both signs, -128 and 127 among them."""
    cg, og, G = GROUP_SHAPES[si]
    rng = np.random.default_rng(7919 * si + 31 * gi + 5 * (za + 128) + 2 * with_zp + with_bias + 1000 * B + H)
    g = GEOMETRIES[gi]
    a = rng.integers(0, 256, (B, H, W, G * cg)).astype(np.uint8).view(np.uint8 if u8 else np.int8)
    w = rng.integers(-128, 128, (G * og, *g[0], cg)).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, G * og).astype(F32)
    zw = None
    if with_zp:
        zw = rng.integers(-128, 128, G * og).astype(np.int32)
        zw[:4] = (-128, 127, 0, -1)
    bias = rng.normal(0, 2.0, G * og).astype(F32) if with_bias else None
    sa = 0.0173
    w_off = w.astype(np.int64) - (0 if zw is None else zw.astype(np.int64).reshape(-1, 1, 1, 1))
    want = grouped_oracle(a, za, sa, w_off, ws, bias, G, g)
    for t in (a, w, ws, zw, bias, want):
        if t is not None:
            t.setflags(write=False)
    return dict(a=a, za=za, sa=sa, w=w, ws=ws, zw=zw, bias=bias, groups=G, geometry=g, want=want)


def extreme_case():
    """The largest magnitude the sum reaches: Kg = 8 * 8 * 512 = 32768 terms, every activation code 255 with za = 0, every
    weight -128 with zw = 127 -- -32768 * 255 * 255, which fits int32 with 0.8 % to spare."""
    G, cg, og, g = 2, 512, 4, ((8, 8), (1, 1), (0, 0), (1, 1))
    a = np.full((1, 8, 8, G * cg), 255, dtype=np.uint8)
    w = np.full((G * og, 8, 8, cg), -128, dtype=np.int8)
    zw = np.full(G * og, 127, dtype=np.int32)
    ws = np.linspace(0.001, 0.01, G * og).astype(F32)
    bias = np.linspace(-3, 3, G * og).astype(F32)
    acc = grouped_loops(a, 0, w.astype(np.int64) - 127, G, *g)
    assert acc.shape == (1, 1, 1, G * og) and acc.min() == acc.max() == -32768 * 255 * 255 and acc.min() > -2 ** 31
    return dict(a=a, za=0, sa=0.031, w=w, ws=ws, zw=zw, bias=bias, groups=G, geometry=g, want=dw_epilogue(acc, 0.031, ws, bias))


def extreme_form(case):
    """A uint8 form whose codes spread over the extreme case's results."""
    lo, hi = float(case["want"].min()), float(case["want"].max())
    return (hi - lo) / 200.0, int(round(-lo / ((hi - lo) / 200.0))) + 20, 0, 255


def run_raw_on(case, device="cpu", out_codes=None):
    from mct_quantizers_amd import consumers
    t = lambda v: None if v is None else torch.from_numpy(v.copy()).to(device)      # noqa: E731
    return consumers.qconv_grouped_i8(t(case["a"]), case["za"], case["sa"], t(case["w"]), t(case["ws"]), t(case["bias"]),
                                      case["groups"], *case["geometry"], out_codes=out_codes, w_zero_points=t(case["zw"]))


def raw_cases(si):
    """(code type, shape, geometry, zero point, weight zero points?, bias?) of one row of GROUP_SHAPES: every geometry with each
    code type and each of the type's three zero points; weight zero points and bias alternate on and off with different
    periods, so that every geometry and code type meets both settings of both."""
    n = si
    for u8 in (True, False):
        for gi in range(len(DW_GEOMETRIES)):
            for za in ZERO_POINTS[np.uint8 if u8 else np.int8]:
                n += 1
                yield u8, si, gi, za, n % 2 == 0, n % 3 != 0


def check_loops_against_float64(case):
    """The loops' float32 result within the derived bound of the exact value, and torch's float64 grouped conv2d of the
    dequantized operands equal to that value."""
    a, w, G, g = case["a"], case["w"], case["groups"], case["geometry"]
    w_off = w.astype(np.int64) - (0 if case["zw"] is None else case["zw"].astype(np.int64).reshape(-1, 1, 1, 1))
    acc = grouped_loops(a, case["za"], w_off, G, *g)
    O = w.shape[0]
    p64 = acc.astype(np.float64) * (np.float64(F32(case["sa"])) * case["ws"].astype(np.float64))
    b64 = np.zeros(O) if case["bias"] is None else case["bias"].astype(np.float64)
    err = np.abs(case["want"].astype(np.float64) - (p64 + b64))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64))
    assert np.all(err <= bound), float((err - bound).max())
    a64 = torch.from_numpy((a.astype(np.float64) - case["za"]) * np.float64(F32(case["sa"]))).permute(0, 3, 1, 2)
    w64 = torch.from_numpy(w_off.astype(np.float64) * case["ws"].astype(np.float64).reshape(-1, 1, 1, 1)).permute(0, 3, 1, 2)
    y64 = torch.nn.functional.conv2d(a64, w64, torch.from_numpy(b64), g[1], g[2], g[3], groups=G).permute(0, 2, 3, 1).numpy()
    assert np.allclose(y64, p64 + b64, rtol=1e-12, atol=1e-12 * float(np.abs(p64).max() + 1.0))


def test_the_loops_agree_with_float64_grouped_conv2d():
    for si in range(len(GROUP_SHAPES)):
        for n, case in enumerate(raw_cases(si)):
            if n % 7 == si % 7:                         # every shape, every geometry and both code types over the rows
                check_loops_against_float64(raw_case(*case))
    check_loops_against_float64(extreme_case())
    # with groups == 1 the loops are the ungrouped convolution the committed oracle computes from a patch matrix
    from oracle import mctq_oracle as O
    from test_conv_consumer import im2col_loops
    c = raw_case(True, 2, 1, 114, True, True)
    half = np.ascontiguousarray(c["a"][..., :8])         # the first group alone: channels 0 .. 7, output channels 0 .. 11
    k, s, p, d = c["geometry"]
    w = c["w"][:12].astype(np.int64) - c["zw"][:12].astype(np.int64).reshape(-1, 1, 1, 1)
    want = O.qlinear_i8(im2col_loops(half, k, s, p, d, 114), 114, c["sa"], w.reshape(12, -1), c["ws"][:12], c["bias"][:12])
    assert bits_equal(want.reshape(c["want"].shape[:3] + (12,)), c["want"][..., :12])


@pytest.mark.parametrize("si", range(len(GROUP_SHAPES)))
def test_qconv_grouped_i8_on_cpu_equals_the_loops(si):
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
    assert n == 2 * 6 * 3


def test_qconv_grouped_i8_on_cpu_edge_values_and_any_channel_count():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    c = extreme_case()
    y = run_raw_on(c)
    assert bits_equal(y.numpy(), c["want"]), first_mismatch(y.numpy(), c["want"])
    form = extreme_form(c)
    codes = run_raw_on(c, out_codes=form)
    assert torch.equal(codes, ops.fq_codes(y, None, None, None, 0, 255, form[0], form[1])) and len(torch.unique(codes)) == 8
    # one output pixel, and the 243 pixels of the GPU test's four blocks
    for shape in (dict(B=1, H=3, W=3), dict(B=3, H=9, W=9)):
        c = raw_case(True, 2, UNPADDED_3X3 if shape["H"] == 3 else 0, 114, True, True, **shape)
        assert bits_equal(run_raw_on(c).numpy(), c["want"])
    # a pointwise grouped layer on 64 channels per group: Kg = 64
    c = raw_case(False, 6, POINTWISE, -3, True, True)
    assert c["want"].shape == (2, 5, 7, 32) and bits_equal(run_raw_on(c).numpy(), c["want"])
    # ints stand for pairs, as in torch.nn.Conv2d; a narrowed clamp stays inside the domain's code type
    c = raw_case(True, 2, 1, 114, False, True)
    t = lambda v: torch.from_numpy(v.copy())      # noqa: E731
    y = consumers.qconv_grouped_i8(t(c["a"]), 114, c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), 4, 3, 2, 1, 1)
    assert bits_equal(y.numpy(), c["want"])
    codes = consumers.qconv_grouped_i8(t(c["a"]), 114, c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), 4, 3, 2, 1, 1,
                                       out_codes=(0.41, -5, -128, 127, -5, 100))
    assert codes.dtype == torch.int8 and int(codes.min()) == -5 and int(codes.max()) <= 100
    # the CPU route takes any Cg: 3 channels per group
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (1, 4, 4, 6)).astype(np.uint8)
    w = rng.integers(-128, 128, (4, 3, 3, 3)).astype(np.int8)
    ws = rng.uniform(0.001, 0.02, 4).astype(F32)
    y = consumers.qconv_grouped_i8(t(a), 7, 0.02, t(w), t(ws), None, 2, 3, 1, 1)
    assert bits_equal(y.numpy(), grouped_oracle(a, 7, 0.02, w.astype(np.int64), ws, None, 2, ((3, 3), (1, 1), (1, 1), (1, 1))))


def test_pack_grouped_weights_layout():
    from mct_quantizers_amd import consumers
    w = torch.from_numpy(raw_case(True, 1, 0, 114, True, True)["w"].copy())            # [16, 3, 3, 12]: Og = 8, Kg = 108
    padded, rowsum = consumers.pack_grouped_weights(w, 2)
    assert padded.dtype == torch.int8 and tuple(padded.shape) == (2, 16, 128) and padded.is_contiguous()
    assert torch.equal(padded[:, :8, :108], w.reshape(2, 8, 108))
    assert not padded[:, 8:].any() and not padded[:, :, 108:].any()
    assert rowsum.dtype == torch.int32 and torch.equal(rowsum, w.to(torch.int64).sum(dim=(1, 2, 3)).to(torch.int32))


def test_qconv_grouped_i8_refuses_bad_operands():
    from mct_quantizers_amd import consumers
    c = raw_case(True, 2, 0, 114, True, True)                  # C = 32, O = 48, G = 4
    a, w, ws, b, zw = (torch.from_numpy(c[k].copy()) for k in ("a", "w", "ws", "bias", "zw"))
    f = consumers.qconv_grouped_i8
    with pytest.raises(TypeError):
        f(a.float(), 114, 0.1, w, ws, b, 4, 3, 1, 1)
    with pytest.raises(TypeError):
        f(a[0], 114, 0.1, w, ws, b, 4, 3, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w.to(torch.int32), ws, b, 4, 3, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w.permute(0, 3, 1, 2).contiguous(), ws, b, 4, 3, 1, 1)        # [O, Cg, kh, kw]
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w[:46].contiguous(), ws, b, 4, 3, 1, 1)                        # O is no multiple of the groups
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w, ws.double(), b, 4, 3, 1, 1)
    with pytest.raises(TypeError):
        f(a, 114, 0.1, w, ws, b, 4, 3, 1, 1, w_zero_points=zw.long())
    with pytest.raises(RuntimeError):
        f(a, 114, 0.1, w, ws, b, 4, 3, 1, 1, w_zero_points=zw[:8].contiguous())
    with pytest.raises(RuntimeError):
        f(a, 114, 0.1, w, ws[:8].contiguous(), b, 4, 3, 1, 1)
    with pytest.raises(ValueError):
        f(a, 256, 0.1, w, ws, b, 4, 3, 1, 1)                                          # no uint8 code
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 1, 3, 1, 1)                                          # ungrouped
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 5, 3, 1, 1)                                          # 5 does not divide 32
    with pytest.raises(ValueError):
        f(a, 114, 0.1, w, ws, b, 4, 3, 0, 1)
    with pytest.raises(ValueError, match="qconv_grouped_i8: stride"):                 # refused in this function's own name
        f(a, 114, 0.1, w, ws, b, 4, 3, (1, 1, 1), 1)


# ---- wrapped grouped convolutions ---------------------------------------------------------------------------------------

def grouped_model(C=32, O=48, groups=4, **kw):
    """Cg = 8 and Og = 12: Og != Cg, and the N tile is partial."""
    return conv_model(C=C, O=O, groups=groups, **kw)


def check_grouped_against_loops_and_float64(qc, x, y):
    """x: the float32 [B, C, H, W] input of the fused layer ``qc`` (any memory format, any device), y its float32 output:
    bit-equal to the loops on the layer's own activation codes, and within the derived bound of the float64 grouped
    convolution of the dequantized operands (module docstring)."""
    from mct_quantizers_amd.hip import ops
    za, sa = qc._a_zp, qc._a_scale
    a = ops.fq_codes_nhwc(x.detach(), qc._a_qmin, qc._a_qmax, sa, za).cpu().numpy()
    w, ws = weight_operands(qc)                                 # [O, kh * kw * Cg], the zero points off
    w = w.reshape(w.shape[0], *qc.kernel_size, -1)
    bias = None if qc.bias is None else qc.bias.detach().cpu().numpy()
    case = dict(a=a, za=za, sa=sa, w=w, ws=ws, zw=None, bias=bias, groups=qc.groups,
                geometry=(qc.kernel_size, qc.stride, qc.padding, qc.dilation))
    case["want"] = grouped_oracle(a, za, sa, w, ws, bias, qc.groups, case["geometry"])
    B, ho, wo, O = case["want"].shape
    assert tuple(y.shape) == (B, O, ho, wo) and y.dtype == torch.float32
    got = y.detach().cpu().permute(0, 2, 3, 1).contiguous().numpy()
    assert bits_equal(got, case["want"]), first_mismatch(got, case["want"])
    check_loops_against_float64(case)
    return case["want"]


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_grouped_conv2d_on_cpu_equals_the_loops(family, per_channel):
    from mct_quantizers_amd import consumers
    for i, (k, s, p, d) in enumerate(DW_GEOMETRIES):
        bias = (i + per_channel) % 2 == 0
        model = grouped_model(k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel, bias=bias, seed=i)
        x = torch.randn(2, 32, 5, 7) * 1.5
        ref = model(x)                                                   # fake-quant + float32 grouped F.conv2d
        qc = consumers.QuantizedGroupedConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
        assert qc._a_zp not in (0, 128) and qc._a_qmin < qc._a_zp < qc._a_qmax and (qc.bias is not None) == bias
        y = qc(x)
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert tuple(qc._w_codes.shape) == (48, *k, 8) and qc._w_codes.dtype == torch.int8 and qc._w_codes.is_contiguous()
        kgp = -(-k[0] * k[1] * 8 // 64) * 64
        assert tuple(qc._w_packed[0].shape) == (4, 16, kgp) and tuple(qc._w_packed[1].shape) == (48,)
        check_grouped_against_loops_and_float64(qc, x, y)
        y_cl = qc(x.contiguous(memory_format=torch.channels_last))
        assert bits_equal(y_cl.numpy(), y.numpy())                      # both memory formats: the same bits
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
        if family == "uniform":
            assert qc._w_zps is not None and len(set(qc._w_zps.tolist())) > (1 if per_channel else 0)
        else:
            assert qc._w_zps is None


def test_grouped_weight_codes_follow_the_weight():
    from mct_quantizers_amd import consumers
    model = grouped_model(family="lut16")
    assert consumers.fuse_linear_consumers(model, grouped=True) == 1
    qc, x = model[1], torch.randn(1, 32, 4, 4)
    y0, codes0, packed0 = model(x), qc._w_codes.clone(), qc._w_packed[0].clone()
    with torch.no_grad():
        qc.weight.mul_(-0.5)
    y1 = model(x)
    assert not torch.equal(codes0, qc._w_codes) and not torch.equal(packed0, qc._w_packed[0]) and not torch.equal(y0, y1)
    check_grouped_against_loops_and_float64(qc, x, y1)


def test_grouped_class_hierarchy_and_code_types():
    from mct_quantizers_amd import consumers
    assert issubclass(consumers.QuantizedGroupedConv2d, consumers.IntegerConsumer)
    assert not issubclass(consumers.QuantizedGroupedConv2d, consumers.QuantizedLinear)
    assert consumers.IntegerConsumer in consumers._CODE_READERS
    holder, wrapper = conv_pair(C=32, O=48, groups=4, act="signed")
    qc = consumers.QuantizedGroupedConv2d.from_wrapper(wrapper, holder.activation_holder_quantizer)
    assert qc(torch.zeros(2, 32, 4, 4, dtype=torch.int8)).dtype == torch.float32     # the quantizer's own code type is taken
    with pytest.raises(TypeError, match="do not match this layer's quantizer"):
        qc(torch.zeros(2, 32, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        qc(torch.zeros(2, 16, 4, 4))
    qc.emit_act = "hardswish"                                     # no entry point takes one: never silently dropped
    with pytest.raises(NotImplementedError):
        qc(torch.zeros(2, 32, 4, 4))


# ---- the switch -----------------------------------------------------------------------------------------------------------

EXISTING_SWITCHES = (dict(), dict(convolutions=True), dict(depthwise=True), dict(convolutions=True, depthwise=True),
                     dict(convolutions=True, depthwise=True, uniform_weights=True, chain=True, any_channels=True, pools=True,
                          avg_pools=True, upsamples=True, activation_tables=True))
FX_ONLY = dict(shared_holders=True, stay_on_codes=True, fused_residuals=True, concats=True, muls=True, hard_activations=True)


def test_fusion_of_grouped_convolutions_is_opt_in():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    model = grouped_model(k=3, padding=1)
    x = torch.randn(2, 32, 5, 7) * 1.5
    ref = model(x)
    for kw in EXISTING_SWITCHES:
        assert consumers.fuse_linear_consumers(model, **kw) == 0          # left alone, exactly as before
        assert isinstance(model[1], mq.PytorchQuantizationWrapper) and torch.equal(model(x), ref)
        for more in (dict(), FX_ONLY):
            gm, n = consumers.fuse_linear_consumers_fx(model, **kw, **more)
            assert n == 0 and torch.equal(gm(x), ref)
    gm, n = consumers.fuse_linear_consumers_fx(grouped_model(k=3, padding=1), grouped=True)
    assert n == 1 and type(gm.get_submodule("1_qlinear")) is consumers.QuantizedGroupedConv2d
    assert [node.target for node in gm.graph.nodes if node.op == "call_module"] == ["1_qlinear"]
    y_fx = gm(x)
    assert consumers.fuse_linear_consumers(model, grouped=True) == 1
    assert isinstance(model[0], torch.nn.Identity) and type(model[1]) is consumers.QuantizedGroupedConv2d
    y = model(x)
    assert bits_equal(y.detach().numpy(), y_fx.detach().numpy())
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    check_grouped_against_loops_and_float64(model[1], x, y)
    # the switch is independent of the others: a depthwise layer stays depthwise's, an ungrouped one convolutions'
    model = conv_model(C=32, O=32, groups=32)
    assert consumers.fuse_linear_consumers(model, grouped=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)
    assert consumers.fuse_linear_consumers(model, grouped=True, depthwise=True) == 1
    assert type(model[1]) is consumers.QuantizedDepthwiseConv2d
    model = conv_model(C=32, O=16, k=3, padding=1)
    assert consumers.fuse_linear_consumers(model, grouped=True, depthwise=True) == 0
    assert isinstance(model[1], mq.PytorchQuantizationWrapper)
    assert consumers.fuse_linear_consumers(model, grouped=True, depthwise=True, convolutions=True) == 1
    assert type(model[1]) is consumers.QuantizedConv2d
    # existing positional calls of _consumer_for mean what they meant: the sixth positional argument is any_channels
    holder, wrapper = conv_pair(C=32, O=48, groups=4)
    q = holder.activation_holder_quantizer
    assert consumers._consumer_for(wrapper, q, True, True, True, True) is None
    assert type(consumers._consumer_for(wrapper, q, grouped=True)) is consumers.QuantizedGroupedConv2d
    holder, wrapper = conv_pair(C=24, O=16, k=1, padding=0)
    assert type(consumers._consumer_for(wrapper, holder.activation_holder_quantizer, False, False, False, True)) is consumers.QuantizedConv1x1


def test_grouped_convolutions_the_consumer_cannot_take_stay():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    left = {
        "Cg=2": conv_model(C=8, O=16, groups=4),
        "multiplier 2": conv_model(C=16, O=32, groups=16),
        "reflect": grouped_model(padding_mode="reflect"),
        "same 2x2": grouped_model(k=2, padding="same"),
        "half": grouped_model().half(),
        "uniform": grouped_model(family="uniform"),
    }
    for name, model in left.items():
        for kw in (dict(grouped=True), dict(grouped=True, convolutions=True, depthwise=True, any_channels=True)):
            assert consumers.fuse_linear_consumers(model, **kw) == 0, name
            assert isinstance(model[1], mq.PytorchQuantizationWrapper), name
            if name != "half":
                gm, n = consumers.fuse_linear_consumers_fx(model, **kw)
                assert n == 0, name
    assert consumers.fuse_linear_consumers(left["uniform"], grouped=True, uniform_weights=True) == 1
    assert type(left["uniform"][1]) is consumers.QuantizedGroupedConv2d
    # the pad byte is the zero point: one outside the clamp domain cannot be taken
    model = grouped_model()
    model[0].activation_holder_quantizer.zero_point = 300
    with pytest.raises(NotImplementedError, match="pad byte"):
        consumers.QuantizedGroupedConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
    assert consumers.fuse_linear_consumers(model, grouped=True) == 0 and isinstance(model[1], mq.PytorchQuantizationWrapper)
    for conv in (torch.nn.Conv2d(32, 32, 3), torch.nn.Conv2d(32, 32, 3, groups=32), torch.nn.Conv2d(8, 8, 3, groups=4),
                 torch.nn.Conv2d(2048, 8, 8, groups=2)):                               # ungrouped, depthwise, Cg = 2, Kg = 2 * 32768
        assert not consumers.QuantizedGroupedConv2d.eligible(conv)
        with pytest.raises(TypeError):
            consumers.QuantizedGroupedConv2d(conv, None, None)
    assert consumers.QuantizedGroupedConv2d.eligible(torch.nn.Conv2d(1024, 8, 8, groups=2))       # Kg = 32768: inside the limit


def test_valid_and_same_padding_strings_grouped():
    from mct_quantizers_amd import consumers
    for padding, k, d in (("valid", 3, 1), ("same", 3, 1), ("same", (3, 5), (2, 1))):
        model = grouped_model(k=k, padding=padding, dilation=d)
        x = torch.randn(1, 32, 6, 7) * 1.5
        ref = model(x)
        assert consumers.fuse_linear_consumers(model, grouped=True) == 1
        y = model(x)
        assert y.shape == ref.shape
        check_grouped_against_loops_and_float64(model[1], x, y)


def grouped_stack(seed=0):
    """1x1 -> grouped 3x3 -> 1x1, each behind its own activation holder (uint8 codes with a zero point, int8 codes, uint8
    codes again)."""
    return torch.nn.Sequential(*conv_pair(C=16, O=32, k=1, padding=0, seed=seed, act="uniform"),
                               *conv_pair(C=32, O=48, k=3, padding=1, groups=4, seed=seed + 1, act="signed", family="uniform"),
                               *conv_pair(C=48, O=16, k=1, padding=0, seed=seed + 2, act="relu", family="lut16"))


def check_grouped_chain(device):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    plain, chained = grouped_stack().to(device), grouped_stack().to(device)
    kinds = [consumers.QuantizedConv1x1, consumers.QuantizedGroupedConv2d, consumers.QuantizedConv1x1]
    for model, chain in ((plain, False), (chained, True)):
        assert consumers.fuse_linear_consumers(model, chain=chain, uniform_weights=True, grouped=True) == 3
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
    assert y.dtype == torch.float32 and torch.equal(plain(x), y)
    return x, y


def test_chained_grouped_stack_gives_the_same_bits_cpu():
    check_grouped_chain("cpu")


# ---- the fx rewrite: a ResNeXt-style bottleneck ---------------------------------------------------------------------------

class Bottleneck(torch.nn.Module):
    """holder -> 1x1 32 -> 64 -> ReLU -> holder -> 3x3 groups=16 (Cg = 4) -> ReLU -> holder -> 1x1 64 -> 32, plus the first
    holder's output (the identity), ReLU, holder."""

    def __init__(self):
        super().__init__()
        self.h0, self.c1 = conv_pair(C=32, O=64, k=1, padding=0, seed=1)
        self.h1, self.c2 = conv_pair(C=64, O=64, k=3, padding=1, groups=16, seed=2, act="relu")
        self.h2, self.c3 = conv_pair(C=64, O=32, k=1, padding=0, seed=3, act="relu")
        self.h3 = conv_pair(C=16, O=16, seed=4, act="relu")[0]
        with torch.no_grad():                            # products of a size the holders' ranges resolve
            for wrapper in (self.c1, self.c2, self.c3):
                wrapper.weight.mul_(0.25)

    def forward(self, x):
        x = self.h0(x)
        y = self.h1(torch.relu(self.c1(x)))
        y = self.h2(torch.relu(self.c2(y)))
        return self.h3(torch.relu(self.c3(y) + x))


BOTTLENECK_SWITCHES = dict(convolutions=True, shared_holders=True, stay_on_codes=True, fused_residuals=True)


def bottleneck_input(device="cpu"):
    return (torch.randn(2, 32, 6, 6, generator=torch.Generator().manual_seed(5)) * 1.5).to(device)


def bottleneck_layer_by_layer(x):
    """The rewritten bottleneck's value on the CPU route, one layer at a time: every consumer built on its own from a fresh
    twin (the same seeds), float32 between the layers, the ReLUs, the add and the holders as they stand in the model."""
    from mct_quantizers_amd import consumers
    twin = Bottleneck()
    c1 = consumers.QuantizedConv1x1.from_wrapper(twin.c1, twin.h0.activation_holder_quantizer)
    c2 = consumers.QuantizedGroupedConv2d.from_wrapper(twin.c2, twin.h1.activation_holder_quantizer)
    c3 = consumers.QuantizedConv1x1.from_wrapper(twin.c3, twin.h2.activation_holder_quantizer)
    a0 = twin.h0(x)
    a1 = twin.h1(torch.relu(c1(a0)))
    a2 = twin.h2(torch.relu(c2(a1)))
    return twin.h3(torch.relu(c3(a2) + a0))


def check_bottleneck(device):
    from mct_quantizers_amd import consumers
    model = Bottleneck().to(device)
    x = bottleneck_input(device)
    ref = model(x)
    gm0, n0 = consumers.fuse_linear_consumers_fx(Bottleneck().to(device), **BOTTLENECK_SWITCHES)
    assert n0 == 2 and isinstance(gm0.get_submodule("c2"), type(model.c2))                # without the switch: as today
    gm, n = consumers.fuse_linear_consumers_fx(model, grouped=True, **BOTTLENECK_SWITCHES)
    assert n == 3
    fused = {name: type(m) for name, m in gm.named_modules() if isinstance(m, consumers.IntegerConsumer)}
    assert fused == {"c1_qlinear": consumers.QuantizedConv1x1, "c2_qlinear": consumers.QuantizedGroupedConv2d,
                     "c3_qlinear": consumers.QuantizedConv1x1}
    c1, c2, c3 = (gm.get_submodule(f"c{i}_qlinear") for i in (1, 2, 3))
    assert c1.emit_codes_for == c2.activation_code_params() and c2.emit_codes_for == c3.activation_code_params()
    lo, hi = c2.emit_clamp                                   # the ReLU behind the grouped layer, folded into its codes
    assert (lo, hi) == consumers.folded_clamp(c3.activation_code_params(), 0.0, float("inf")) and lo == c3._a_zp > c3._a_qmin
    assert c2.emit_residual is None and c2.emit_relu is False and c2.emit_act is None
    targets = [node.target for node in gm.graph.nodes if node.op == "call_module"]
    assert not any(t in targets for t in ("h1", "h2", "c1", "c2", "c3")) and "c2_qlinear" in targets
    seen = {}
    hook = c2.register_forward_hook(lambda m, args, out: seen.update(x=args[0], y=out))
    y = gm(x)
    hook.remove()
    assert seen["x"].dtype == torch.uint8 and seen["y"].dtype == torch.uint8              # codes in, codes out
    assert y.shape == ref.shape == x.shape
    assert torch.allclose(y, ref, rtol=1e-4, atol=2 * float(model.h3.activation_holder_quantizer.scale))
    return gm, x, y


def test_fx_rewrite_of_a_resnext_bottleneck_cpu():
    _, x, y = check_bottleneck("cpu")
    want = bottleneck_layer_by_layer(x)
    assert bits_equal(y.detach().numpy(), want.detach().numpy()), first_mismatch(y.detach().numpy(), want.detach().numpy())
    assert len(torch.unique(y)) > 16


class _GroupedInFrontOfAJoin(torch.nn.Module):
    """holder -> grouped 3x3 -> + identity -> ReLU -> holder -> 1x1: the join behind the grouped layer writes codes only."""

    def __init__(self, act=None):
        super().__init__()
        self.h0, self.c1 = conv_pair(C=32, O=32, k=3, padding=1, groups=4, seed=1)
        self.h1, self.c2 = conv_pair(C=32, O=16, k=1, padding=0, seed=2, act="relu")
        self.act = act

    def forward(self, x):
        x = self.h0(x)
        if self.act is not None:
            return self.c2(self.h1(self.act(self.c1(x))))
        return self.c2(self.h1(torch.relu(self.c1(x) + x)))


def test_the_grouped_consumer_takes_no_residual_and_no_hard_activation():
    from mct_quantizers_amd import consumers
    x = bottleneck_input()
    switches = dict(BOTTLENECK_SWITCHES, hard_activations=True)
    # the residual join stays a join: the grouped layer writes float32 into it
    gm, n = consumers.fuse_linear_consumers_fx(_GroupedInFrontOfAJoin(), grouped=True, **switches)
    gm0, n0 = consumers.fuse_linear_consumers_fx(_GroupedInFrontOfAJoin(), grouped=True, convolutions=True, shared_holders=True)
    assert n == n0 == 2
    c1 = gm.get_submodule("c1_qlinear")
    assert type(c1) is consumers.QuantizedGroupedConv2d and not consumers._takes_hard_activation(c1)
    assert (c1.emit_residual, c1.emit_relu, c1.emit_act, c1.emit_codes_for) == (None, False, None, None)
    joins = [name for name, m in gm.named_modules() if isinstance(m, consumers.QuantizedJoin) and m.has_residual]
    assert joins == ["h1_join"]
    assert bits_equal(gm(x).detach().numpy(), gm0(x).detach().numpy())
    # a Hardswish behind it stays in the graph, in float32
    gm, n = consumers.fuse_linear_consumers_fx(_GroupedInFrontOfAJoin(torch.nn.Hardswish()), grouped=True, **switches)
    c1 = gm.get_submodule("c1_qlinear")
    assert n == 2 and (c1.emit_act, c1.emit_codes_for) == (None, None)
    assert "act" in [node.target for node in gm.graph.nodes if node.op == "call_module"]
    want = _GroupedInFrontOfAJoin(torch.nn.Hardswish())(x)
    assert torch.allclose(gm(x), want, rtol=1e-4, atol=1e-4 * float(want.detach().abs().max()))


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_qconv_grouped_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_qconv_grouped_i8\s*\(", header) and "mctq_qconv_grouped_i8" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(a=P, adt=U8, za=114, sa=0.5, w=P, ws=P, rs=P, zw=None, bias=None, y=P, ydt=-1, y_scale=0.25, y_zp=0, qmin=0,
                 qmax=255, B=2, H=5, W=7, C=32, O=48, G=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_qconv_grouped_i8(v["a"], v["adt"], v["za"], v["sa"], v["w"], v["ws"], v["rs"], v["zw"], v["bias"], v["y"],
                                         v["ydt"], v["y_scale"], v["y_zp"], v["qmin"], v["qmax"], v["B"], v["H"], v["W"], v["C"],
                                         v["O"], v["G"], v["kh"], v["kw"], v["sh"], v["sw"], v["ph"], v["pw"], v["dh"], v["dw"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWCO":
        refused(b"negative extent", **{extent: -1})
    for name in ("kh", "kw"):
        refused(b"kernel size below 1", **{name: 0})
    for name in ("sh", "sw"):
        refused(b"stride below 1", **{name: 0})
    for name in ("dh", "dw"):
        refused(b"dilation below 1", **{name: 0})
    for name in ("ph", "pw"):
        refused(b"negative padding", **{name: -1})
    for groups in (1, 0, -4):
        refused(b"groups below 2: the grouped consumer takes grouped convolutions only", G=groups)
    for fault in (dict(C=30), dict(O=50), dict(C=0), dict(O=0), dict(G=5)):
        refused(b"channels and out_channels must be positive multiples of groups", **fault)
    for channels in (4, 8, 24, 40):                                       # Cg = 1, 2, 6, 10
        refused(b"channels per group must be a multiple of 4", C=channels)
    limit = b"kh * kw * channels per group > 32768: outside the consumer's limit"
    refused(limit, C=64, kh=64, kw=64, ph=32, pw=32)                      # Cg = 16: 65536
    refused(limit, C=4 * 32772)                                           # Cg alone
    refused(limit, kh=2 ** 31 - 1, kw=2 ** 31 - 1, ph=2 ** 30, pw=2 ** 30)
    assert call(C=32, kh=64, kw=64, ph=32, pw=32, B=0) == 0               # Kg = 32768 is inside the limit
    refused(b"bad a_code_dtype", adt=77)
    for adt, za in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"a_zero_point is no code of a_code_dtype", adt=adt, za=za)
    for adt, za in ((U8, 0), (U8, 255), (I8, -128), (I8, 127)):
        assert call(adt=adt, za=za, B=0) == 0
    refused(b"bad y_code_dtype", ydt=9)
    refused(b"quant_min > quant_max", ydt=U8, qmin=200, qmax=100)
    refused(b"clamp domain does not fit the code type", ydt=U8, qmax=256)
    refused(b"clamp domain does not fit the code type", ydt=I8, qmin=-129, qmax=127)
    # wrong in two ways: the window's sizes, the groups, the channels, the K limit, the activations' form, the output's, the fit
    refused(b"negative padding", ph=-1, G=1)
    refused(b"groups below 2: the grouped consumer takes grouped convolutions only", G=1, C=30)
    refused(b"channels and out_channels must be positive multiples of groups", C=30, adt=77)
    refused(b"channels per group must be a multiple of 4", C=24, kh=2 ** 20, kw=2 ** 20)
    refused(limit, C=64, kh=64, kw=64, adt=77)
    refused(b"bad a_code_dtype", adt=77, za=256)
    refused(b"a_zero_point is no code of a_code_dtype", za=256, ydt=9)
    refused(b"bad y_code_dtype", ydt=9, H=2 ** 31)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8, a=None)      # 8 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=5, dw=3)        # 13 > 7 + 2
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, kh=1)
    refused(b"too many output pixels for one launch", B=2 ** 31, kh=1, kw=1, ph=0, pw=0, H=1, W=1)
    refused(b"too many output pixels for one launch", B=2 ** 62, H=2 ** 20, W=2 ** 20, kh=1, kw=1, ph=0, pw=0)
    refused(b"the codes tensor exceeds 2^63 - 1 bytes", B=2 ** 30, H=2 ** 20, W=2 ** 20, kh=1, kw=1, ph=0, pw=0, sh=2 ** 20, sw=2 ** 20)
    refused(b"groups * ceil(out_channels per group / 64) > 65535: too many grid slices", C=4 * 65536, O=65536, G=65536)
    for pointer in ("a", "w", "ws", "rs", "y"):
        refused(b"NULL pointer", **{pointer: None})
    for pointer, off in (("a", 8), ("w", 4), ("ws", 4), ("rs", 8), ("y", 1), ("zw", 4), ("bias", 8)):
        refused(b"codes, weights, per-channel tables and output must be 16-byte aligned", **{pointer: P + off})
    nothing = dict(a=None, w=None, ws=None, rs=None, y=None)
    assert call(B=0) == 0 and call(B=0, **nothing) == 0                # no images: no launch, no pointer is looked at
    assert call(B=0, ydt=U8) == 0 and call(B=0, zw=P, bias=P) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
