"""k x k, strided, padded and dilated convolutions on the integer consumer: host logic and the CPU route
(include/mctq_hip.h: mctq_codes_im2col_nhwc; hip/ops.py: codes_im2col; consumers.QuantizedConv2d and the ``convolutions``
switch of fuse_linear_consumers / fuse_linear_consumers_fx).

Oracle of every exactness check: a patch matrix built by plain numpy loops over (b, oy, ox, ky, kx) from the layer's
activation codes -- padded taps hold the zero-point code -- fed to oracle/mctq_oracle.py::qlinear_i8 together with the
weights quantizer's own codes transposed to [O, kh, kw, C] here (``w - zw[:, None]`` for uniform weights, as in
tests/test_zp_consumer.py).  The layer's output must equal it bit for bit.

Bound against float64 (tests/test_zp_consumer.py derives it): four float32 roundings of 2^-24 each -- the product of the
two scales, the conversion of the int32 sum, the multiply, the bias add -- with a factor 2 for second-order terms:
|y - y64| <= 2^-21 * (|p64| + |bias|), where y64 = p64 + bias is the float64 convolution of the dequantized operands.
p64 is evaluated exactly (the integer sum times the float64 product of the two float32 scales); torch's float64
``conv2d`` of the dequantized tensors, which knows nothing of patch matrices, must agree with it to float64 accuracy.
A padded tap dequantizes to (za - za) * sa = 0, the zero ``conv2d`` pads with: that is why the zero point is the pad byte.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch

# (kernel, stride, padding, dilation) of the issue's list; every one on B=2, 5x7 images with C in {16, 48}
GEOMETRIES = [((3, 3), (1, 1), (1, 1), (1, 1)), ((3, 3), (2, 2), (1, 1), (1, 1)), ((1, 1), (2, 2), (0, 0), (1, 1)),
              ((1, 3), (1, 1), (0, 1), (1, 1)), ((3, 3), (1, 1), (2, 2), (2, 2)), ((7, 7), (2, 2), (3, 3), (1, 1))]
PAD_CODES = {np.uint8: (0, 128, 255), np.int8: (-128, -3, 127)}

LUT16 = [-120.0, 77.0, -2.0, 38.0, -96.0, 3.0, 127.0, -50.0, 11.0, -33.0, 100.0, -9.0, 24.0, -70.0, 55.0, -20.0]
LUT256 = [float(v) for v in np.random.default_rng(5).permutation(np.arange(-128, 128))]
FAMILIES = ["sym", "pot", "lut16", "lut256", "uniform"]


def out_hw(h, w, k, s, p, d):
    return tuple((n + 2 * p[i] - d[i] * (k[i] - 1) - 1) // s[i] + 1 for i, n in enumerate((h, w)))


def im2col_loops(codes, k, s, p, d, pad_code):
    """codes [B, H, W, C] -> [B * Ho * Wo, kh * kw * C] by plain loops; taps outside the image hold pad_code."""
    B, H, W, C = codes.shape
    ho, wo = out_hw(H, W, k, s, p, d)
    out = np.full((B, ho, wo, k[0], k[1], C), pad_code, dtype=codes.dtype)
    for b in range(B):
        for oy in range(ho):
            for ox in range(wo):
                for ky in range(k[0]):
                    for kx in range(k[1]):
                        iy, ix = oy * s[0] - p[0] + ky * d[0], ox * s[1] - p[1] + kx * d[1]
                        if 0 <= iy < H and 0 <= ix < W:
                            out[b, oy, ox, ky, kx] = codes[b, iy, ix]
    return out.reshape(B * ho * wo, k[0] * k[1] * C)


@functools.lru_cache(maxsize=None)
def im2col_case(u8, C, geometry, pad_code, B=2, H=5, W=7):
    """(codes [B, H, W, C], the loops' patch matrix), computed once and shared by the CPU and GPU tests; read-only."""
    dt = np.uint8 if u8 else np.int8
    rng = np.random.default_rng(1000 * C + 10 * GEOMETRIES.index(geometry) + u8 + B)
    codes = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8).view(dt)
    want = im2col_loops(codes, *geometry, pad_code)
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


def im2col_cases():
    for u8 in (True, False):
        for C in (16, 48):
            for g in GEOMETRIES:
                for pad_code in PAD_CODES[np.uint8 if u8 else np.int8]:
                    yield u8, C, g, pad_code


def test_codes_im2col_on_cpu_equals_the_numpy_loops():
    from mct_quantizers_amd.hip import ops
    n = 0
    for u8, C, g, pad_code in im2col_cases():
        codes, want = im2col_case(u8, C, g, pad_code)
        got = ops.codes_im2col(torch.from_numpy(codes.copy()), *g, pad_code)
        assert got.dtype == (torch.uint8 if u8 else torch.int8) and got.is_contiguous()
        assert got.shape == want.shape and np.array_equal(got.numpy(), want), (u8, C, g, pad_code)
        n += 1
    assert n == 2 * 2 * 6 * 3
    # ints stand for pairs, as in torch.nn.Conv2d
    codes, want = im2col_case(True, 16, GEOMETRIES[1], 128)
    assert np.array_equal(ops.codes_im2col(torch.from_numpy(codes.copy()), 3, 2, 1, 1, 128).numpy(), want)
    # a non-contiguous view is gathered in its logical order
    t = torch.from_numpy(np.ascontiguousarray(codes.transpose(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert not t.is_contiguous() and np.array_equal(ops.codes_im2col(t, 3, 2, 1, 1, 128).numpy(), want)


def test_codes_im2col_refuses_what_fq_codes_nhwc_refuses():
    from mct_quantizers_amd.hip import ops
    x = torch.zeros(2, 5, 7, 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.codes_im2col(x[0], 3, 1, 1, 1, 0)                            # rank
    with pytest.raises(NotImplementedError):
        ops.codes_im2col(x.to(torch.int32), 3, 1, 1, 1, 0)              # dtype
    with pytest.raises(NotImplementedError):
        ops.codes_im2col(x.float(), 3, 1, 1, 1, 0)
    with pytest.raises(ValueError):
        ops.codes_im2col(x, 3, 1, 1, 1, 256)                            # no uint8 code
    with pytest.raises(ValueError):
        ops.codes_im2col(x.to(torch.int8), 3, 1, 1, 1, 128)             # no int8 code
    with pytest.raises(ValueError):
        ops.codes_im2col(x, 3, 0, 1, 1, 0)
    with pytest.raises(ValueError):
        ops.codes_im2col(x, 9, 1, 1, 1, 0)                              # 9 > 5 + 2: no output row


# ---- wrapped convolutions ----------------------------------------------------------------------------------------------

def activation_quantizer(kind="uniform"):
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "uniform":                # zero point 114 of 0 .. 255: neither 0 nor the middle of the domain
            return Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-2.5], max_range=[3.1])
        if kind == "relu":                   # what follows a ReLU whose range was calibrated a little below zero
            return Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-0.4], max_range=[5.0])
        return Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[3.3], signed=True)


def weights_quantizer(weight, family, per_channel, bits=None):
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    n = weight.shape[0]
    w2 = weight.detach().reshape(n, -1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if family == "sym":
            thr = [float(v) for v in w2.abs().max(1).values] if per_channel else [float(w2.abs().max())]
            return Q.WeightsSymmetricInferableQuantizer(num_bits=bits or 8, threshold=thr, per_channel=per_channel,
                                                        channel_axis=0 if per_channel else None)
        if family == "pot":
            thr = [float(2.0 ** (-2 + i % 3)) for i in range(n)] if per_channel else [0.5]
            return Q.WeightsPOTInferableQuantizer(num_bits=bits or 8, threshold=thr, per_channel=per_channel,
                                                  channel_axis=0 if per_channel else None)
        if family in ("lut16", "lut256"):
            thr = [float(v) for v in w2.abs().max(1).values] if per_channel else [float(w2.abs().max())]
            return Q.WeightsLUTSymmetricInferableQuantizer(
                num_bits=4 if family == "lut16" else 8, lut_values=LUT16 if family == "lut16" else LUT256, threshold=thr,
                per_channel=per_channel, channel_axis=0 if per_channel else None, input_rank=4 if per_channel else None,
                lut_values_bitwidth=8)
        assert family == "uniform"
        if per_channel:                      # the rows' own ranges, two of them forced well off centre
            lo = [min(float(v), -0.01) for v in w2.min(1).values]
            hi = [max(float(v), 0.01) for v in w2.max(1).values]
            lo[0], hi[0], lo[1], hi[1] = -0.2, 1.3, -1.1, 0.4
            return Q.WeightsUniformInferableQuantizer(num_bits=bits or 8, min_range=lo, max_range=hi, per_channel=True, channel_axis=0)
        return Q.WeightsUniformInferableQuantizer(num_bits=bits or 8, min_range=[-0.2], max_range=[1.3], per_channel=False)


def conv_pair(C=16, O=24, k=3, stride=1, padding=1, dilation=1, family="sym", per_channel=True, bias=True, act="uniform",
              seed=0, bits=None, **conv_kw):
    """[activation holder, wrapped Conv2d]; weights N(0.1, 0.4): uniform ranges and codebooks are really used."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(C, O, k, stride=stride, padding=padding, dilation=dilation, bias=bias, **conv_kw)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 0.4 + 0.1)
    wq = weights_quantizer(conv.weight, family, per_channel, bits)
    return [mq.PytorchActivationQuantizationHolder(activation_quantizer(act)), mq.PytorchQuantizationWrapper(conv, {"weight": wq})]


def conv_model(**kw):
    return torch.nn.Sequential(*conv_pair(**kw))


def weight_operands(qc):
    """(int codes [O, kh * kw * C] with the zero points already taken off, float32 scales [O]) of a fused layer, from the
    weights quantizer's own codes of the float weight -- the [O, C, kh, kw] -> [O, kh, kw, C] order is redone here."""
    q, w = qc.weights_quantizer, qc.weight.detach()
    O = w.shape[0]
    rows = lambda t: t.cpu().numpy().reshape(w.shape).transpose(0, 2, 3, 1).reshape(O, -1)      # noqa: E731
    per_row = lambda t: np.broadcast_to(t.detach().cpu().numpy().astype(np.float32).reshape(-1), (O,)) if t.numel() == 1 \
        else t.detach().cpu().numpy().astype(np.float32).reshape(-1)                             # noqa: E731
    if qc._lut_weights:
        idx, lut, thr = q.quantize_to_codes(w)
        lut = lut.cpu().numpy().reshape(-1)
        assert np.array_equal(lut, np.rint(lut)) and lut.min() >= -128 and lut.max() <= 127
        return lut.astype(np.int32)[rows(idx)], per_row(thr) / np.float32(2.0 ** (q.lut_values_bitwidth - 1))
    codes, scales, zps = q.quantize_to_codes(w)
    codes = rows(codes).astype(np.int32)
    if qc._uniform_weights:
        zps = zps.cpu().numpy().astype(np.int32).reshape(-1)
        codes = codes - np.broadcast_to(zps, (O,))[:, None]
    return codes, per_row(scales)


def check_conv_against_oracle_and_float64(qc, x, y):
    """x: the float32 [B, C, H, W] input of the fused layer ``qc`` (any memory format, any device), y its float32 output:
    bit-equal to the oracle on the layer's own activation codes, and within the derived bound of the float64 convolution
    of the dequantized operands (module docstring)."""
    from oracle import mctq_oracle as O
    from mct_quantizers_amd.hip import ops
    k, s, p, d = qc.kernel_size, qc.stride, qc.padding, qc.dilation
    za, sa = qc._a_zp, qc._a_scale
    a = ops.fq_codes_nhwc(x.detach(), qc._a_qmin, qc._a_qmax, sa, za).cpu().numpy()
    patches = im2col_loops(a, k, s, p, d, za)
    w, ws = weight_operands(qc)
    bias = None if qc.bias is None else qc.bias.detach().cpu().numpy()
    B, ho, wo = a.shape[0], *out_hw(a.shape[1], a.shape[2], k, s, p, d)
    assert tuple(y.shape) == (B, w.shape[0], ho, wo) and y.dtype == torch.float32
    got = y.detach().cpu().permute(0, 2, 3, 1).reshape(B * ho * wo, -1).numpy()
    want = O.qlinear_i8(patches, za, sa, w, ws, bias)
    assert bits_equal(got, want), first_mismatch(got, want)
    acc = (patches.astype(np.int64) - za) @ w.astype(np.int64).T
    p64 = acc.astype(np.float64) * (np.float64(np.float32(sa)) * ws.astype(np.float64))[None, :]
    b64 = np.zeros(ws.shape[0]) if bias is None else bias.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (p64 + b64[None, :]))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64)[None, :])
    assert np.all(err <= bound), float((err - bound).max())
    # the same float64 convolution by torch, from the dequantized tensors in their own layouts
    a64 = torch.from_numpy((a.astype(np.float64) - za) * np.float64(np.float32(sa))).permute(0, 3, 1, 2)
    w64 = torch.from_numpy(w.astype(np.float64) * ws.astype(np.float64)[:, None])
    w64 = w64.reshape(w.shape[0], k[0], k[1], -1).permute(0, 3, 1, 2)
    y64 = torch.nn.functional.conv2d(a64, w64, torch.from_numpy(b64), s, p, d).permute(0, 2, 3, 1).reshape(B * ho * wo, -1).numpy()
    assert np.allclose(y64, p64 + b64[None, :], rtol=1e-12, atol=1e-12 * float(np.abs(p64).max() + 1.0))
    return want


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_conv2d_on_cpu_equals_the_oracle(family, per_channel):
    from mct_quantizers_amd import consumers
    for i, (k, s, p, d) in enumerate([GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[4], GEOMETRIES[3]]):
        bias = (i + per_channel) % 2 == 0
        model = conv_model(C=16, O=24, k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel, bias=bias,
                           seed=i)
        x = torch.randn(2, 16, 5, 7) * 1.5
        ref = model(x)                                                   # fake-quant + float32 F.conv2d
        qc = consumers.QuantizedConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
        assert qc._a_zp not in (0, 128) and qc._a_qmin < qc._a_zp < qc._a_qmax and (qc.bias is not None) == bias
        y = qc(x)
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        check_conv_against_oracle_and_float64(qc, x, y)
        y_cl = qc(x.contiguous(memory_format=torch.channels_last))
        assert bits_equal(y_cl.numpy(), y.numpy())                      # both memory formats: the same bits
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
        if family == "uniform":
            assert qc._w_zps is not None and len(set(qc._w_zps.tolist())) > (1 if per_channel else 0)


def test_valid_and_same_padding_strings():
    from mct_quantizers_amd import consumers
    for padding, k, d in (("valid", 3, 1), ("same", 3, 1), ("same", (3, 5), (2, 1))):
        model = conv_model(k=k, padding=padding, dilation=d)
        x = torch.randn(1, 16, 6, 7) * 1.5
        ref = model(x)
        assert consumers.fuse_linear_consumers(model, convolutions=True) == 1
        y = model(x)
        assert y.shape == ref.shape
        check_conv_against_oracle_and_float64(model[1], x, y)


def test_fusion_of_convolutions_is_opt_in():
    from mct_quantizers_amd import consumers
    for kw in (dict(k=3, padding=1), dict(k=1, stride=2, padding=0), dict(k=3, stride=2, padding=1)):
        model = conv_model(C=32, O=16, **kw)
        x = torch.randn(2, 32, 5, 7) * 1.5
        ref = model(x)
        assert consumers.fuse_linear_consumers(model) == 0              # default: left alone, exactly as before
        assert not isinstance(model[1], consumers.IntegerConsumer) and torch.equal(model(x), ref)
        assert consumers.fuse_linear_consumers(model, convolutions=True) == 1
        assert isinstance(model[0], torch.nn.Identity) and type(model[1]) is consumers.QuantizedConv2d
        y = model(x)
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
        check_conv_against_oracle_and_float64(model[1], x, y)
    # a pointwise stride-1 convolution keeps the consumer without a patch matrix, with or without the switch
    model = conv_model(C=32, O=16, k=1, padding=0)
    assert consumers.fuse_linear_consumers(model, convolutions=True) == 1 and type(model[1]) is consumers.QuantizedConv1x1


def test_convolutions_the_consumer_cannot_take_stay():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    left = {
        "groups": conv_model(C=32, O=16, groups=2),
        "C=24": conv_model(C=24),
        "reflect": conv_model(padding_mode="reflect"),
        "same 2x2": conv_model(k=2, padding="same"),
        "K > 32768": conv_model(C=4096, O=1, per_channel=False),
        "half": conv_model().half(),
        "uniform": conv_model(family="uniform"),
    }
    for name, model in left.items():
        assert consumers.fuse_linear_consumers(model, convolutions=True) == 0, name
        assert isinstance(model[1], mq.PytorchQuantizationWrapper), name
    assert consumers.fuse_linear_consumers(left["uniform"], convolutions=True, uniform_weights=True) == 1
    # the pad byte is the zero point: one outside the clamp domain cannot be taken
    model = conv_model()
    model[0].activation_holder_quantizer.zero_point = 300
    with pytest.raises(NotImplementedError, match="pad byte"):
        consumers.QuantizedConv2d.from_wrapper(model[1], model[0].activation_holder_quantizer)
    assert consumers.fuse_linear_consumers(model, convolutions=True) == 0
    with pytest.raises(TypeError):
        consumers.QuantizedConv2d(torch.nn.Conv2d(24, 8, 3), None, None)


def conv_stack(seed=0):
    """3x3 -> 1x1 -> 3x3 stride 2, each behind its activation holder (different quantizers, so the codes really change)."""
    return torch.nn.Sequential(*conv_pair(C=16, O=32, k=3, padding=1, seed=seed, act="uniform"),
                               *conv_pair(C=32, O=16, k=1, padding=0, seed=seed + 1, act="signed", family="uniform"),
                               *conv_pair(C=16, O=24, k=3, stride=2, padding=1, seed=seed + 2, act="relu", family="lut16"))


def check_conv_chain(device):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    plain, chained = conv_stack().to(device), conv_stack().to(device)
    kinds = [consumers.QuantizedConv2d, consumers.QuantizedConv1x1, consumers.QuantizedConv2d]
    for model, chain in ((plain, False), (chained, True)):
        assert consumers.fuse_linear_consumers(model, chain=chain, uniform_weights=True, convolutions=True) == 3
        assert [type(model[i]) for i in (1, 3, 5)] == kinds
    assert chained[1].emit_codes_for == chained[3].activation_code_params() and chained[5].emit_codes_for is None
    # (its own generator: building the layers draws from the global one, and not the same numbers on every device)
    x = (torch.randn(2, 16, 6, 5, generator=torch.Generator().manual_seed(11)) * 1.5).to(device)
    mid32, mid = plain[:4](x), chained[:4](x)
    nxt = chained[5]
    assert mid32.dtype == torch.float32 and mid.dtype == torch.uint8 and mid.shape == mid32.shape
    want = ops.fq_codes(mid32, None, None, None, nxt._a_qmin, nxt._a_qmax, nxt._a_scale, nxt._a_zp)
    assert torch.equal(mid, want) and len(torch.unique(want)) > 8     # the same codes, and not a saturated handful
    y = chained(x)
    assert y.dtype == torch.float32 and torch.equal(plain(x), y)
    return x, y


def test_chained_convolutions_give_the_same_bits_cpu():
    check_conv_chain("cpu")


def test_weight_codes_follow_the_weight():
    from mct_quantizers_amd import consumers
    model = conv_model(family="lut16")
    consumers.fuse_linear_consumers(model, convolutions=True)
    qc, x = model[1], torch.randn(1, 16, 4, 4)
    y0, codes0 = model(x), model[1]._w_codes.clone()
    with torch.no_grad():
        qc.weight.mul_(-0.5)
    y1 = model(x)
    assert not torch.equal(codes0, qc._w_codes) and not torch.equal(y0, y1)
    check_conv_against_oracle_and_float64(qc, x, y1)


class Bottleneck(torch.nn.Module):
    """1x1 -> 3x3 stride 2 -> 1x1, and a stride-2 1x1 downsample branch that shares the input's activation holder."""

    def __init__(self):
        super().__init__()
        self.h_in, self.c1 = conv_pair(C=32, O=16, k=1, padding=0, seed=1)
        self.h2, self.c2 = conv_pair(C=16, O=16, k=3, stride=2, padding=1, seed=2, act="relu")
        self.h3, self.c3 = conv_pair(C=16, O=64, k=1, padding=0, seed=3, act="relu")
        self.cd = conv_pair(C=32, O=64, k=1, stride=2, padding=0, seed=4)[1]

    def forward(self, x):
        a = self.h_in(x)
        main = self.c3(self.h3(torch.relu(self.c2(self.h2(torch.relu(self.c1(a)))))))
        return torch.relu(main + self.cd(a))


def check_bottleneck(device):
    """The fx rewrite with ``convolutions=True``: the holders with ONE consumer are folded (h2 -> c2 becomes a
    QuantizedConv2d, h3 -> c3 a QuantizedConv1x1), the shared input holder and its two convolutions stay.  Every fused
    layer, on the input it really got, equals the oracle and stays within the derived bound of the float64 convolution
    (computed on the CPU); the whole module agrees with the unfused one as far as float32 convolutions agree."""
    from mct_quantizers_amd import consumers
    model = Bottleneck().to(device)
    x = (torch.randn(2, 32, 9, 7) * 1.5).to(device)
    ref = model(x)
    gm0, n0 = consumers.fuse_linear_consumers_fx(Bottleneck().to(device))
    assert n0 == 1 and type(gm0.get_submodule("c3_qlinear")) is consumers.QuantizedConv1x1
    gm, n = consumers.fuse_linear_consumers_fx(model, convolutions=True)
    assert n == 2
    fused = {name: m for name, m in gm.named_modules() if isinstance(m, consumers.IntegerConsumer)}
    assert {name: type(m) for name, m in fused.items()} == {"c2_qlinear": consumers.QuantizedConv2d,
                                                             "c3_qlinear": consumers.QuantizedConv1x1}
    called = [node.target for node in gm.graph.nodes if node.op == "call_module"]
    assert called == ["h_in", "c1", "c2_qlinear", "c3_qlinear", "cd"]
    seen = {}
    hook = fused["c2_qlinear"].register_forward_hook(lambda m, args, out: seen.update(x=args[0], y=out))
    y = gm(x)
    hook.remove()
    assert y.shape == ref.shape == (2, 64, 5, 4)
    check_conv_against_oracle_and_float64(fused["c2_qlinear"], seen["x"], seen["y"])
    assert torch.allclose(y, ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))
    return gm, x, y


def test_fx_rewrite_of_a_bottleneck_cpu():
    check_bottleneck("cpu")


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def test_im2col_argument_validation_needs_no_gpu():
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    E, P = native.MCTQ_E_ARG, 4096              # an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(x=P, y=P, B=2, H=5, W=7, C=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, pad=114)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_codes_im2col_nhwc(v["x"], v["y"], v["B"], v["H"], v["W"], v["C"], v["kh"], v["kw"], v["sh"], v["sw"],
                                          v["ph"], v["pw"], v["dh"], v["dw"], v["pad"], None)

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
    refused(b"pad_code outside [-128, 255]", pad=256)
    refused(b"pad_code outside [-128, 255]", pad=-129)
    refused(b"channels must be a multiple of 16", C=24)
    refused(b"NULL pointer", x=None)
    refused(b"NULL pointer", y=None)
    refused(b"codes and patches must be 16-byte aligned", x=P + 8)
    refused(b"codes and patches must be 16-byte aligned", y=P + 1)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8)              # 8 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=5, dw=3)        # 13 > 7 + 2
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", C=4096)                  # 9 * 4096
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", C=32784, kh=1, kw=1)
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", kh=2 ** 31 - 1, kw=2 ** 31 - 1, ph=2 ** 30, pw=2 ** 30)
    refused(b"too many output rows for one launch", B=2 ** 31, kh=1, kw=1, ph=0, pw=0, H=1, W=1)
    refused(b"too many output rows for one launch", B=2 ** 62, H=2 ** 20, W=2 ** 20, kh=1, kw=1, ph=0, pw=0)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31)
    assert call(H=2 ** 31 - 3, B=0) == 0                               # the padded extent alone counts, not the kernel
    # wrong in two ways: the window's sizes, the pad code, the channels, the limit, the padded extent, the fit, the rows
    refused(b"negative padding", ph=-1, pad=256)
    refused(b"pad_code outside [-128, 255]", pad=256, C=24)
    refused(b"channels must be a multiple of 16", C=24, kh=2 ** 31 - 1)
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", C=4096, H=2 ** 31)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31, kw=16)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8, B=2 ** 62)
    refused(b"too many output rows for one launch", B=2 ** 31, kh=1, kw=1, ph=0, pw=0, H=1, W=1, x=None)
    assert call(B=0) == 0 and call(B=0, x=None, y=None) == 0          # no images: no launch, no pointer is looked at
    assert call(C=0) == 0                                               # no channels: nothing to write
    assert call(pad=-128, B=0) == 0 and call(pad=255, B=0) == 0
    assert lib.mctq_launch_count() == count                            # refused and empty calls launch nothing
