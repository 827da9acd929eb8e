"""Uniform (zero-point) weights on the integer consumer: host logic and the CPU route (include/mctq_hip.h: mctq_codes_rowsum,
mctq_qlinear_i8_zp; consumers.QuantizedLinear with a WeightsUniformInferableQuantizer).

Oracle: oracle/mctq_oracle.py::qlinear_i8 on ``w_codes - zw[:, None]`` -- the exact int64 product of (a - za) and (w - zw),
scaled once in float32: the contract of the zero-point entry points.  The CPU route must equal it bit for bit.
Against the float64 product of the dequantized operands the result carries four float32 roundings of 2^-24 each (the
product of the two scales, the conversion of the int32 sum, the multiply, the bias add); with a factor 2 for second-order
terms: |y - y64| <= 2^-21 * (|p64| + |bias|).
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch


def zp_problem(rng, M, N, K, u8, with_bias=True, w_lo=-128, w_hi=128):
    """Random codes, scales and zero points in the codes' domain [w_lo, w_hi)."""
    a = rng.integers(0, 256, (M, K)).astype(np.uint8) if u8 else rng.integers(-128, 128, (M, K)).astype(np.int8)
    w = rng.integers(w_lo, w_hi, (N, K)).astype(np.int8)
    zw = rng.integers(w_lo, w_hi, N).astype(np.int32)
    za = int(rng.integers(0, 256)) if u8 else int(rng.integers(-128, 128))
    sa = float(rng.uniform(0.001, 0.1))
    ws = rng.uniform(0.001, 0.1, N).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if with_bias else None
    return a, za, sa, w, zw, ws, bias


def zp_oracle(a, za, sa, w, zw, ws, bias):
    from oracle import mctq_oracle as O
    return O.qlinear_i8(a, za, sa, np.asarray(w).astype(np.int32) - np.asarray(zw).astype(np.int32)[:, None], ws, bias)


def uniform_model(K=64, N=24, bits=8, per_channel=True, act="uniform", seed=0, conv=False):
    """activation holder -> wrapped Linear (or 1x1 convolution) with a uniform weights quantizer whose ranges do not
    straddle zero symmetrically (per tensor [-0.2, 1.3]; per channel the row's own minimum and maximum, rows 0 and 1
    forced to [-0.2, 1.3] and [-1.1, 0.4]), so that the zero points are neither 0 nor the middle of the domain."""
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    torch.manual_seed(seed)
    layer = torch.nn.Conv2d(K, N, 1) if conv else torch.nn.Linear(K, N)
    with torch.no_grad():
        layer.weight.copy_(torch.randn_like(layer.weight) * 0.4 + 0.3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if per_channel:
            w2 = layer.weight.detach().reshape(N, -1)
            lo = [min(float(v), -0.01) for v in w2.min(1).values]
            hi = [max(float(v), 0.01) for v in w2.max(1).values]
            lo[0], hi[0] = -0.2, 1.3
            lo[1], hi[1] = -1.1, 0.4
            wq = Q.WeightsUniformInferableQuantizer(num_bits=bits, min_range=lo, max_range=hi, per_channel=True, channel_axis=0)
        else:
            wq = Q.WeightsUniformInferableQuantizer(num_bits=bits, min_range=[-0.2], max_range=[1.3], per_channel=False)
        if act == "uniform":
            aq = Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-2.5], max_range=[3.1])
        elif act == "signed":
            aq = Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[3.3], signed=True)
        else:
            aq = Q.ActivationPOTInferableQuantizer(num_bits=8, threshold=[4.0], signed=False)
    return torch.nn.Sequential(mq.PytorchActivationQuantizationHolder(aq), mq.PytorchQuantizationWrapper(layer, {"weight": wq}))


def check_against_oracle_and_float64(ql, x2, y2):
    """x2 [M, K] float32 input rows, y2 [M, N] the consumer's float32 output: bit-equal to the oracle on the module's own
    codes, and within the derived bound of the float64 product of the dequantized operands."""
    from mct_quantizers_amd.hip import ops
    a_codes = ops.fq_codes(x2, None, None, None, ql._a_qmin, ql._a_qmax, ql._a_scale, ql._a_zp).cpu().numpy()
    w, zw, ws = ql._w_codes.cpu().numpy(), ql._w_zps.cpu().numpy(), ql._w_scales.cpu().numpy()
    bias = None if ql.bias is None else ql.bias.detach().cpu().numpy()
    got = y2.detach().cpu().numpy()
    want = zp_oracle(a_codes, ql._a_zp, ql._a_scale, w, zw, ws, bias)
    assert bits_equal(got, want), first_mismatch(got, want)
    # exact integer sum times the exact product of the two float32 scales, rounded once in float64
    acc = (a_codes.astype(np.int64) - ql._a_zp) @ (w.astype(np.int64) - zw.astype(np.int64)[:, None]).T
    p64 = acc.astype(np.float64) * (np.float64(np.float32(ql._a_scale)) * ws.astype(np.float64))[None, :]
    b64 = np.zeros(ws.shape[0]) if bias is None else bias.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (p64 + b64[None, :]))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64)[None, :])
    assert np.all(err <= bound), float((err - bound).max())


@pytest.mark.parametrize("u8", [False, True])
def test_codes_rowsum_on_cpu_matches_numpy(u8):
    from mct_quantizers_amd import consumers
    rng = np.random.default_rng(11 + u8)
    for (M, K) in [(1, 16), (5, 1008), (3, 32768)]:
        a = rng.integers(0, 256, (M, K)).astype(np.uint8) if u8 else rng.integers(-128, 128, (M, K)).astype(np.int8)
        if K == 32768:
            a[0] = 255 if u8 else -128
            a[1] = 0 if u8 else 127
        for za in ((0, 255, 114) if u8 else (-128, 127, 5)):
            got = consumers.codes_rowsum(torch.from_numpy(a), za)
            assert got.dtype == torch.int32 and got.shape == (M,)
            assert np.array_equal(got.numpy(), (a.astype(np.int64) - za).sum(1))
    with pytest.raises(TypeError):
        consumers.codes_rowsum(torch.zeros(4, 16), 0)


def test_qlinear_i8_on_cpu_with_zero_points_equals_the_oracle():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    rng = np.random.default_rng(21)
    for (M, N, K) in [(1, 16, 16), (5, 100, 256), (17, 33, 272)]:
        for u8 in (False, True):
            a, za, sa, w, zw, ws, bias = zp_problem(rng, M, N, K, u8, with_bias=(M + N) % 2 == 1)
            t = lambda v: None if v is None else torch.from_numpy(v)     # noqa: E731
            rs = torch.from_numpy(w.astype(np.int32).sum(1, dtype=np.int32))
            got = consumers.qlinear_i8(t(a), za, sa, t(w), t(ws), rs, t(bias), w_zero_points=t(zw))
            want = zp_oracle(a, za, sa, w, zw, ws, bias)
            assert bits_equal(got.numpy(), want), f"M={M} N={N} K={K} u8={u8}: {first_mismatch(got.numpy(), want)}"
            out = (0.07, 5, -128, 127)
            codes = consumers.qlinear_i8(t(a), za, sa, t(w), t(ws), rs, t(bias), out, w_zero_points=t(zw))
            assert torch.equal(codes, ops.fq_codes(got, None, None, None, out[2], out[3], out[0], out[1]))
    # the accumulator's two extremes: +-255 * 255 * 32768 fits int32, the intermediate terms alone would not add up in order
    K = 32768
    for (av, adt, za, wv, zv) in ((255, np.uint8, 0, -128, 127), (-128, np.int8, 127, 127, -128)):
        a, w = np.full((2, K), av, adt), np.full((3, K), wv, np.int8)
        zw, ws = np.full(3, zv, np.int32), np.asarray([0.5, 0.25, 1.0], np.float32)
        rs = torch.from_numpy(w.astype(np.int32).sum(1, dtype=np.int32))
        got = consumers.qlinear_i8(torch.from_numpy(a), za, 1.0, torch.from_numpy(w), torch.from_numpy(ws), rs, None,
                                   w_zero_points=torch.from_numpy(zw))
        assert bits_equal(got.numpy(), zp_oracle(a, za, 1.0, w, zw, ws, None))
        assert abs(float(got[0, 2])) == float(np.float32(255 * 255 * 32768))


def test_qlinear_i8_on_cpu_refuses_malformed_zero_points():
    from mct_quantizers_amd import consumers
    a, w = torch.zeros(2, 16, dtype=torch.int8), torch.zeros(3, 16, dtype=torch.int8)
    ws, rs = torch.ones(3), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="2 entries for 3 output channels"):
        consumers.qlinear_i8(a, 0, 1.0, w, ws, rs, None, w_zero_points=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="w_zero_points"):
        consumers.qlinear_i8(a, 0, 1.0, w, ws, rs, None, w_zero_points=torch.zeros(3, dtype=torch.int64))


@pytest.mark.parametrize("bits", [8, 4, 3])
@pytest.mark.parametrize("per_channel", [True, False])
def test_quantized_linear_takes_uniform_weights_on_cpu(bits, per_channel):
    from mct_quantizers_amd import consumers
    model = uniform_model(bits=bits, per_channel=per_channel)
    holder, wrapper = model[0], model[1]
    ql = consumers.QuantizedLinear.from_wrapper(wrapper, holder.activation_holder_quantizer)
    x = torch.randn(3, 5, 64) * 1.5
    ref = model(x)                                                   # fake-quant + float32 F.linear
    y = ql(x)
    assert y.shape == ref.shape == (3, 5, 24) and y.dtype == torch.float32
    # the stored codes: int8, re-biased by half the domain together with the zero points; dequantized they are q(w) exactly
    half = 2 ** (bits - 1)
    assert ql._w_codes.dtype == torch.int8 and ql._w_zps.dtype == torch.int32 and ql._w_zps.shape == (24,)
    assert int(ql._w_codes.min()) >= -half and int(ql._w_codes.max()) <= half - 1
    zw = ql._w_zps.numpy()
    assert np.any(zw != 0) and np.any(zw != -half) and zw.min() >= -half and zw.max() <= half - 1
    if per_channel:
        assert len(set(zw.tolist())) > 1
    deq = (ql._w_codes.to(torch.int32) - ql._w_zps[:, None]).to(torch.float32) * ql._w_scales[:, None]
    wq = wrapper.weights_quantizers["weight"](wrapper.weight.detach().clone())
    assert bits_equal(deq.numpy(), wq.numpy()), first_mismatch(deq.numpy(), wq.numpy())
    assert np.array_equal(ql._w_rowsum.numpy(), ql._w_codes.numpy().astype(np.int64).sum(1))
    check_against_oracle_and_float64(ql, x.reshape(-1, 64), y.reshape(-1, 24))
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))


def test_fusion_of_uniform_weights_is_opt_in():
    from mct_quantizers_amd import consumers
    model = uniform_model()
    x = torch.randn(7, 64) * 1.5
    ref = model(x)
    assert consumers.fuse_linear_consumers(model) == 0               # default: left alone, exactly as before
    assert not isinstance(model[1], consumers.IntegerConsumer) and torch.equal(model(x), ref)
    assert consumers.fuse_linear_consumers(model, uniform_weights=True) == 1
    assert isinstance(model[0], torch.nn.Identity) and isinstance(model[1], consumers.QuantizedLinear)
    y = model(x)
    assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    check_against_oracle_and_float64(model[1], x, y)
    # a pointwise convolution with uniform weights likewise
    conv = uniform_model(K=32, N=16, conv=True)
    xc = torch.randn(2, 32, 5, 3) * 1.5
    refc = conv(xc)
    assert consumers.fuse_linear_consumers(conv) == 0 and consumers.fuse_linear_consumers(conv, uniform_weights=True) == 1
    assert isinstance(conv[1], consumers.QuantizedConv1x1)
    yc = conv(xc)
    assert yc.shape == refc.shape and torch.allclose(yc, refc, rtol=1e-5, atol=2e-6 * float(refc.detach().abs().max()))


class _TwoLayers(torch.nn.Module):
    def __init__(self):
        super().__init__()
        first, second = uniform_model(K=64, N=32, seed=4), uniform_model(K=32, N=16, seed=5, per_channel=False, act="signed")
        self.h1, self.l1, self.h2, self.l2 = first[0], first[1], second[0], second[1]

    def forward(self, x):
        return self.l2(self.h2(torch.relu(self.l1(self.h1(x)))))


def test_fx_fusion_of_uniform_weights_is_opt_in():
    from mct_quantizers_amd import consumers
    model = _TwoLayers()
    x = torch.randn(9, 64) * 1.5
    ref = model(x)
    gm, n = consumers.fuse_linear_consumers_fx(model)
    assert n == 0 and torch.equal(gm(x), ref)
    gm, n = consumers.fuse_linear_consumers_fx(model, uniform_weights=True)
    assert n == 2 and [type(m).__name__ for m in gm.modules()].count("QuantizedLinear") == 2
    assert torch.allclose(gm(x), ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))


def uniform_into_symmetric_stack():
    """uniform-weights layer -> symmetric-weights layer, each behind its activation holder."""
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    first = uniform_model(K=64, N=32, seed=7)
    torch.manual_seed(8)
    lin = torch.nn.Linear(32, 16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in lin.weight.detach().abs().max(1).values]
        second = [mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(8, [40.0], True)),
                  mq.PytorchQuantizationWrapper(lin, {"weight": Q.WeightsSymmetricInferableQuantizer(
                      num_bits=8, threshold=thr, per_channel=True, channel_axis=0)})]
    return torch.nn.Sequential(first[0], first[1], *second)


def check_chain(device):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    plain, chained = uniform_into_symmetric_stack().to(device), uniform_into_symmetric_stack().to(device)
    assert consumers.fuse_linear_consumers(plain, uniform_weights=True) == 2
    assert consumers.fuse_linear_consumers(chained, chain=True, uniform_weights=True) == 2
    assert chained[1].emit_codes_for is not None and chained[1]._uniform_weights and not chained[3]._uniform_weights
    x = (torch.randn(7, 64) * 1.5).to(device)
    mid32, mid = plain[:2](x), chained[:2](x)
    nxt = chained[3]
    assert mid32.dtype == torch.float32 and mid.dtype == torch.int8
    want = ops.fq_codes(mid32, None, None, None, nxt._a_qmin, nxt._a_qmax, nxt._a_scale, nxt._a_zp)
    assert torch.equal(mid, want) and len(torch.unique(want)) > 8     # the same codes, and not a saturated handful
    assert torch.equal(plain(x), chained(x))


def test_chained_uniform_layer_emits_the_codes_of_the_float32_intermediate_cpu():
    check_chain("cpu")


def test_uniform_weight_codes_follow_the_weight_and_refuse_zero_points_outside_the_domain():
    from mct_quantizers_amd import consumers
    model = uniform_model()
    consumers.fuse_linear_consumers(model, uniform_weights=True)
    ql = model[1]
    x = torch.randn(4, 64)
    y0 = model(x)
    codes0 = ql._w_codes.clone()
    with torch.no_grad():
        ql.weight.mul_(0.5)
    y1 = model(x)
    assert not torch.equal(codes0, ql._w_codes) and not torch.equal(y0, y1)
    q = ql.weights_quantizer
    q.zero_points = q.zero_points + 300                              # 8 bits: zw = z - 128 > 127
    with torch.no_grad():
        ql.weight.mul_(2.0)
    with pytest.raises(NotImplementedError):
        model(x)
