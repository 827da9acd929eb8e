"""Integer consumers for any channel count: host logic and the CPU route (include/mctq_hip.h: mctq_codes_im2col_pad_nhwc;
hip/ops.py: codes_im2col(..., pad_to=16); the ``any_channels`` keyword of consumers.QuantizedLinear / QuantizedConv1x1 /
QuantizedConv2d and of fuse_linear_consumers / fuse_linear_consumers_fx).

A layer whose K is no multiple of 16 keeps its weight rows padded with the code 0 to Kp = 16 * ceil(K / 16) columns and reads
activation rows padded with the zero-point code za.  Padding is exact: a padded column adds qa * 0 to the int32 sum, 0 to the
weight's row sum and (za - za) to the activation's row sum, so every check of an unpadded consumer holds unchanged:

* the patch matrix against an independent construction (``F.unfold`` of the codes as float, reordered to (ky, kx, c), the pad
  columns appended), byte for byte;
* a padded layer against the oracle (oracle/mctq_oracle.py::qlinear_i8 on the UNPADDED rows and weight codes), bit for bit, and
  against the float64 evaluation of the exact integer sum within the bound tests/test_conv_consumer.py derives and uses,
  |y - y64| <= 2^-21 * (|p64| + |bias|); against the float32 chain (holder -> wrapper) with that file's tolerances;
* emitted codes against quantizing the float32 output; a chain against the unchained rewrite, bit for bit.

The opt-in is guarded twice: without the switch the C = 24, K = 24 and stem models are left alone, and a C = 32 model comes out
module for module as without it."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import (LUT16, activation_quantizer, check_conv_against_oracle_and_float64, conv_model, conv_pair,
                                weights_quantizer)

F = torch.nn.functional
FAMILIES = ["sym", "pot", "lut16", "uniform"]            # the four weight families


# ---- the patch matrix --------------------------------------------------------------------------------------------------------

def unfold_patches(codes, k, s, p, d, pad_code, pad_to):
    """codes [B, H, W, C] (numpy int8 / uint8) -> [B * Ho * Wo, Kp]: ``F.unfold`` of the codes as float32 (shifted by pad_code,
    so that unfold's zero padding stands for it), its (c, ky, kx) rows reordered to (ky, kx, c), pad columns appended."""
    B, H, W, C = codes.shape
    x = torch.from_numpy(codes.astype(np.float32) - float(pad_code)).permute(0, 3, 1, 2)
    cols = F.unfold(x, k, dilation=d, padding=p, stride=s)                       # [B, C * kh * kw, L]
    L = cols.shape[-1]
    rows = cols.reshape(B, C, k[0], k[1], L).permute(0, 4, 2, 3, 1).reshape(B * L, k[0] * k[1] * C) + float(pad_code)
    K = rows.shape[1]
    Kp = -(-K // pad_to) * pad_to
    out = np.full((B * L, Kp), pad_code, dtype=codes.dtype)
    out[:, :K] = rows.numpy().astype(np.int64).astype(codes.dtype)
    return out


def pad_cases():
    """(u8, C, (k, s, p, d), pad_code): every C with every kernel size, stride and padding, and one dilated case per C."""
    for u8, pad_code in ((True, 131), (False, -7)):
        for C in (1, 3, 4, 12, 17, 24, 40, 16):
            for k in (1, 3, 7):
                for s in (1, 2):
                    for p in (0, 1, 3):
                        yield u8, C, ((k, k), (s, s), (p, p), (1, 1)), pad_code
            yield u8, C, ((3, 2), (1, 2), (2, 1), (2, 3)), pad_code


@functools.lru_cache(maxsize=None)
def pad_case(u8, C, geometry, pad_code, B=2, H=9, W=8):
    """(codes [B, H, W, C], the patch matrix at pitch Kp by ``unfold_patches``), computed once and shared; read-only."""
    rng = np.random.default_rng([C, int(u8), B, H, *(v for pair in geometry for v in pair)])
    codes = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8).view(np.uint8 if u8 else np.int8)
    want = unfold_patches(codes, *geometry, pad_code, 16)
    codes.setflags(write=False)
    want.setflags(write=False)
    return codes, want


def test_codes_im2col_pad_to_16_on_cpu_equals_the_unfold_construction():
    from mct_quantizers_amd.hip import ops
    n = 0
    for u8, C, g, pad_code in pad_cases():
        codes, want = pad_case(u8, C, g, pad_code)
        K = g[0][0] * g[0][1] * C
        t = torch.from_numpy(codes.copy())
        got = ops.codes_im2col(t, *g, pad_code, pad_to=16)
        assert got.dtype == t.dtype and got.is_contiguous() and got.shape == want.shape and got.shape[1] % 16 == 0
        assert got.shape[1] - K < 16 and np.array_equal(got.numpy(), want), (u8, C, g)
        # pad_to=1, given or not, returns what it returned before: the K real columns
        for plain in (ops.codes_im2col(t, *g, pad_code), ops.codes_im2col(t, *g, pad_code, pad_to=1)):
            assert plain.shape == (want.shape[0], K) and np.array_equal(plain.numpy(), want[:, :K]), (u8, C, g)
        n += 1
    assert n == 2 * 8 * (3 * 2 * 3 + 1)
    # [M, K] rows are [M, 1, 1, K] images: the re-pitch of a Linear layer's rows
    rows = torch.arange(5 * 6, dtype=torch.int32).reshape(5, 6).to(torch.int8)
    got = ops.codes_im2col(rows, 1, pad_to=16, pad_code=-3)
    assert got.shape == (5, 16) and torch.equal(got[:, :6], rows) and bool((got[:, 6:] == -3).all())
    with pytest.raises(ValueError):
        ops.codes_im2col(rows, 1, pad_to=1)                   # without the pitch a 2-D tensor is refused as before
    with pytest.raises(ValueError):
        ops.codes_im2col(rows, 1, pad_to=8)
    with pytest.raises(ValueError):
        ops.codes_im2col(rows.to(torch.uint8), 1, pad_to=16, pad_code=256)


# ---- padded layers -----------------------------------------------------------------------------------------------------------

def linear_pair(K, O, family, per_channel, bias, act="uniform", seed=0):
    """[activation holder, wrapped Linear]; weights N(0.1, 0.4) as tests/test_conv_consumer.py::conv_pair."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, O, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn_like(lin.weight) * 0.4 + 0.1)
    if family == "lut16":
        w2 = lin.weight.detach()
        thr = [float(v) for v in w2.abs().max(1).values] if per_channel else [float(w2.abs().max())]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wq = mq.pytorch_quantizers.WeightsLUTSymmetricInferableQuantizer(
                num_bits=4, lut_values=LUT16, threshold=thr, per_channel=per_channel, channel_axis=0 if per_channel else None,
                input_rank=2 if per_channel else None, lut_values_bitwidth=8)
    else:
        wq = weights_quantizer(lin.weight, family, per_channel)
    return [mq.PytorchActivationQuantizationHolder(activation_quantizer(act)), mq.PytorchQuantizationWrapper(lin, {"weight": wq})]


def weight_rows(qc):
    """(int codes [O, K] with the zero points taken off, float32 scales [O]) of a fused layer from the weights quantizer's own
    codes of the float weight, in the order of the activation rows; K is the layer's own, never the pitch."""
    q, w = qc.weights_quantizer, qc.weight.detach()
    O = w.shape[0]

    def rows(t):
        t = t.cpu().numpy().reshape(w.shape)
        return (t.transpose(0, 2, 3, 1) if t.ndim == 4 else t).reshape(O, -1)

    def per_row(t):
        t = t.detach().cpu().numpy().astype(np.float32).reshape(-1)
        return np.broadcast_to(t, (O,)) if t.size == 1 else t

    if qc._lut_weights:
        idx, lut, thr = q.quantize_to_codes(w)
        lut = lut.cpu().numpy().reshape(-1)
        return lut.astype(np.int32)[rows(idx)], per_row(thr) / np.float32(2.0 ** (q.lut_values_bitwidth - 1))
    codes, scales, zps = q.quantize_to_codes(w)
    codes = rows(codes).astype(np.int32)
    if qc._uniform_weights:
        codes = codes - np.broadcast_to(zps.cpu().numpy().astype(np.int32).reshape(-1), (O,))[:, None]
    return codes, per_row(scales)


def check_rows_against_oracle_and_float64(qc, a_rows, y_rows):
    """A padded Linear / pointwise layer: ``a_rows`` its UNPADDED activation codes [M, K] (numpy), ``y_rows`` its float32 output
    [M, O]: bit-equal to the oracle on those rows, and within 2^-21 * (|p64| + |bias|) of the exact integer sum in float64."""
    from oracle import mctq_oracle as O
    za, sa = qc._a_zp, qc._a_scale
    w, ws = weight_rows(qc)
    assert w.shape[1] == a_rows.shape[1] == qc.in_features
    bias = None if qc.bias is None else qc.bias.detach().cpu().numpy()
    got = y_rows.detach().cpu().numpy()
    want = O.qlinear_i8(a_rows, za, sa, w, ws, bias)
    assert bits_equal(got, want), first_mismatch(got, want)
    acc = (a_rows.astype(np.int64) - za) @ w.astype(np.int64).T
    p64 = acc.astype(np.float64) * (np.float64(np.float32(sa)) * ws.astype(np.float64))[None, :]
    b64 = np.zeros(ws.shape[0]) if bias is None else bias.astype(np.float64)
    err = np.abs(got.astype(np.float64) - (p64 + b64[None, :]))
    bound = 2.0 ** -21 * (np.abs(p64) + np.abs(b64)[None, :])
    assert np.all(err <= bound), float((err - bound).max())


def padded_layer(kind, family, per_channel, bias, device="cpu", seed=0):
    """(holder, wrapper, padded consumer, float32 input) of one of the issue's four shapes: the stem scaled down (3 -> 8 channels,
    7 x 7 / 2 pad 3 on 11 x 13), a 24 -> 10 pointwise convolution, Linear layers with K = 6 and K = 24."""
    from mct_quantizers_amd import consumers
    gen = torch.Generator().manual_seed(100 + seed)
    if kind == "stem":
        pair = conv_pair(C=3, O=8, k=7, stride=2, padding=3, family=family, per_channel=per_channel, bias=bias, seed=seed)
        cls, x = consumers.QuantizedConv2d, torch.randn(2, 3, 11, 13, generator=gen) * 1.5
    elif kind == "pointwise":
        pair = conv_pair(C=24, O=10, k=1, padding=0, family=family, per_channel=per_channel, bias=bias, seed=seed)
        cls, x = consumers.QuantizedConv1x1, torch.randn(2, 24, 5, 7, generator=gen) * 1.5
    else:
        K = {"linear6": 6, "linear24": 24}[kind]
        pair = linear_pair(K, 10, family, per_channel, bias, seed=seed)
        cls, x = consumers.QuantizedLinear, torch.randn(3, 5, K, generator=gen) * 1.5
    holder, wrapper = (m.to(device) for m in pair)
    qc = cls.from_wrapper(wrapper, holder.activation_holder_quantizer, any_channels=True)
    return holder, wrapper, qc, x.to(device)


KINDS = ["stem", "pointwise", "linear6", "linear24"]


def check_padded_layer(qc, x, y):
    """The exact checks of a padded layer's float32 output, whatever its kind."""
    from mct_quantizers_amd.hip import ops
    if hasattr(qc, "kernel_size"):
        return check_conv_against_oracle_and_float64(qc, x, y)            # (its loops build the UNPADDED patch matrix)
    if x.dim() == 4:
        a = ops.fq_codes_nhwc(x.detach(), qc._a_qmin, qc._a_qmax, qc._a_scale, qc._a_zp).cpu().numpy().reshape(-1, qc.in_features)
        y_rows = y.detach().permute(0, 2, 3, 1).reshape(-1, qc.out_features)
    else:
        a = ops.fq_codes(x.detach(), None, None, None, qc._a_qmin, qc._a_qmax, qc._a_scale, qc._a_zp).cpu().numpy().reshape(-1, qc.in_features)
        y_rows = y.detach().reshape(-1, qc.out_features)
    check_rows_against_oracle_and_float64(qc, a, y_rows)


@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_padded_consumers_on_cpu_equal_the_oracle_and_stay_within_the_float64_bound(kind, family, per_channel):
    for bias in (True, False):
        holder, wrapper, qc, x = padded_layer(kind, family, per_channel, bias, seed=int(bias))
        ref = wrapper(holder(x))                                            # fake-quant + the float32 layer
        K = qc.in_features
        assert K % 16 != 0 and qc._k_pitch == 16 * -(-K // 16) and (qc.bias is not None) == bias
        # the activation zero point is neither 0 nor mid-domain (a wrong pad byte shows), uniform weights have non-zero zero points
        assert qc._a_zp not in (0, 128) and qc._a_qmin < qc._a_zp < qc._a_qmax
        y = qc(x)
        assert y.shape == ref.shape and y.dtype == torch.float32
        assert tuple(qc._w_codes.shape) == (qc.out_features, qc._k_pitch) and not bool(qc._w_codes[:, K:].any())
        assert torch.equal(qc._w_rowsum, qc._w_codes[:, :K].sum(dim=1, dtype=torch.int32))
        assert qc._w_codes4 is None and qc._w_idx4 is None                   # padded rows are never packed
        if family == "uniform":
            assert qc._w_zps is not None and bool((qc._w_zps != 0).any())
        check_padded_layer(qc, x, y)
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))


def test_emitted_codes_and_a_folded_clamp_from_a_padded_layer_equal_quantizing_its_float32_output():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    for kind in KINDS:
        for family in ("sym", "uniform"):
            _, _, qc, x = padded_layer(kind, family, True, True)
            y = qc(x)
            form = (0.031, 7, 0, 255)
            lo, hi = consumers.folded_clamp(form, 0.0, 3.0)                  # a ReLU-style clamp: lo is the zero point
            assert (lo, hi) == (7, 104)
            for clamp in (None, (lo, hi)):
                qc.emit_codes_for, qc.emit_clamp = form, clamp
                codes = qc(x)
                want = ops.fq_codes(y if clamp is None else y.clamp(0.0, 3.0), None, None, None, 0, 255, form[0], form[1])
                assert codes.dtype == torch.uint8 and torch.equal(codes, want) and len(torch.unique(want)) > 8, (kind, family)


def chain_24_24_16(device="cpu"):
    """C = 24 -> 24 -> 16 pointwise / 3 x 3 / pointwise, each behind its own holder: every K is 24 or 216."""
    return torch.nn.Sequential(*conv_pair(C=24, O=24, k=1, padding=0, seed=1, act="uniform"),
                               *conv_pair(C=24, O=24, k=3, padding=1, seed=2, act="signed", family="uniform"),
                               *conv_pair(C=24, O=16, k=1, padding=0, seed=3, act="relu", family="lut16")).to(device)


def check_padded_chain(device):
    from mct_quantizers_amd import consumers
    plain, chained = chain_24_24_16(device), chain_24_24_16(device)
    kinds = [consumers.QuantizedConv1x1, consumers.QuantizedConv2d, consumers.QuantizedConv1x1]
    for model, chain in ((plain, False), (chained, True)):
        assert consumers.fuse_linear_consumers(model, chain=chain, uniform_weights=True, convolutions=True, any_channels=True) == 3
        assert [type(model[i]) for i in (1, 3, 5)] == kinds and [model[i]._k_pitch for i in (1, 3, 5)] == [32, 224, 32]
    assert chained[1].emit_codes_for == chained[3].activation_code_params()
    assert chained[3].emit_codes_for == chained[5].activation_code_params() and chained[5].emit_codes_for is None
    x = (torch.randn(2, 24, 6, 5, generator=torch.Generator().manual_seed(11)) * 1.5).to(device)
    assert chained[:2](x).dtype == torch.int8 and chained[:4](x).dtype == torch.uint8
    y = chained(x)
    assert y.dtype == torch.float32 and torch.equal(plain(x), y)
    return x, y


def test_a_padded_chain_run_codes_to_codes_equals_the_unchained_rewrite():
    check_padded_chain("cpu")


# ---- the rewrites ------------------------------------------------------------------------------------------------------------

def _left_alone_models():
    return {"C=24 3x3": (lambda: conv_model(C=24), dict(convolutions=True)),
            "C=24 1x1": (lambda: conv_model(C=24, k=1, padding=0), dict()),
            "K=24 linear": (lambda: torch.nn.Sequential(*linear_pair(24, 10, "sym", True, True)), dict()),
            "stem": (lambda: conv_model(C=3, O=8, k=7, stride=2, padding=3), dict(convolutions=True))}


@pytest.mark.parametrize("name", list(_left_alone_models()))
def test_the_rewrites_take_such_layers_only_with_the_switch(name):
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    make, kw = _left_alone_models()[name]
    model = make()
    assert consumers.fuse_linear_consumers(model, **kw) == 0
    assert isinstance(model[0], mq.PytorchActivationQuantizationHolder) and isinstance(model[1], mq.PytorchQuantizationWrapper)
    gm, n = consumers.fuse_linear_consumers_fx(make(), **kw)
    assert n == 0 and not any(isinstance(m, consumers.IntegerConsumer) for m in gm.modules())
    x = torch.randn(2, 24) if "linear" in name else torch.randn(2, model[1].layer.in_channels, 9, 8)
    ref = model(x)
    assert consumers.fuse_linear_consumers(model, any_channels=True, **kw) == 1
    assert isinstance(model[0], torch.nn.Identity) and isinstance(model[1], consumers.IntegerConsumer) and model[1]._k_pitch is not None
    gm, n = consumers.fuse_linear_consumers_fx(make(), any_channels=True, **kw)
    fused = [m for m in gm.modules() if isinstance(m, consumers.IntegerConsumer)]
    assert n == 1 and len(fused) == 1 and type(fused[0]) is type(model[1]) and fused[0]._k_pitch == model[1]._k_pitch
    assert [type(gm.get_submodule(node.target)) for node in gm.graph.nodes if node.op == "call_module"] == [type(model[1])]
    for y in (model(x), gm(x)):
        assert torch.allclose(y, ref, rtol=1e-5, atol=2e-6 * float(ref.detach().abs().max()))
    if "3x3" in name or name == "stem":
        # QuantizedConv2d still needs convolutions=True
        assert consumers.fuse_linear_consumers(make(), any_channels=True) == 0


def test_a_model_of_32_channels_is_rewritten_as_without_the_switch():
    from mct_quantizers_amd import consumers
    from test_conv_consumer import Bottleneck, conv_stack
    for make, kw in ((conv_stack, dict(chain=True, uniform_weights=True, convolutions=True)), (Bottleneck, dict(convolutions=True))):
        if make is conv_stack:
            a, b = make(), make()
            assert consumers.fuse_linear_consumers(a, **kw) == consumers.fuse_linear_consumers(b, any_channels=True, **kw) == 3
        (a, na), (b, nb) = consumers.fuse_linear_consumers_fx(make(), **kw), consumers.fuse_linear_consumers_fx(make(), any_channels=True, **kw)
        assert na == nb
        ma, mb = list(a.named_modules()), list(b.named_modules())
        assert [(n, type(m).__name__, m.extra_repr()) for n, m in ma] == [(n, type(m).__name__, m.extra_repr()) for n, m in mb]
        assert all(type(m) is type(o) for (_, m), (_, o) in zip(ma[1:], mb[1:]))           # (the roots are two GraphModule classes)
        assert [str(node) for node in a.graph.nodes] == [str(node) for node in b.graph.nodes]
        for (_, m), (_, o) in zip(ma, mb):
            if isinstance(m, consumers.QuantizedLinear):
                assert o._k_pitch is None and m._k_pitch is None
        x = torch.randn(2, 32 if make is Bottleneck else 16, 9, 7, generator=torch.Generator().manual_seed(2)) * 1.5
        assert torch.equal(a(x), b(x))
    # ... and built directly: the same buffers
    pair = conv_pair(C=32, O=16, k=3, padding=1, family="sym", bits=4)
    q0 = consumers.QuantizedConv2d.from_wrapper(pair[1], pair[0].activation_holder_quantizer)
    q1 = consumers.QuantizedConv2d.from_wrapper(pair[1], pair[0].activation_holder_quantizer, any_channels=True)
    x = torch.randn(1, 32, 5, 5)
    assert torch.equal(q0(x), q1(x)) and torch.equal(q0._w_codes, q1._w_codes) and q1._w_codes.shape == (16, 288)


def test_pairs_the_padded_consumer_cannot_take_stay():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    # the pad byte is the zero point: one outside the clamp domain cannot be taken (an unpadded Linear of K = 32 does not need it)
    for make, kw in ((lambda: conv_model(C=24, k=1, padding=0), {}), (lambda: torch.nn.Sequential(*linear_pair(24, 10, "sym", True, True)), {}),
                     (lambda: conv_model(C=3, O=8, k=7, stride=2, padding=3), dict(convolutions=True))):
        model = make()
        model[0].activation_holder_quantizer.zero_point = 300
        cls = consumers.QuantizedLinear if isinstance(model[1].layer, torch.nn.Linear) else (
            consumers.QuantizedConv2d if kw else consumers.QuantizedConv1x1)
        with pytest.raises(NotImplementedError, match="pad byte"):
            cls.from_wrapper(model[1], model[0].activation_holder_quantizer, any_channels=True)
        assert consumers.fuse_linear_consumers(model, any_channels=True, **kw) == 0
        assert isinstance(model[1], mq.PytorchQuantizationWrapper)
        gm, n = consumers.fuse_linear_consumers_fx(model, any_channels=True, **kw)
        assert n == 0
    # Kp > 32768
    for model, kw in ((conv_model(C=4097, O=1, per_channel=False), dict(convolutions=True)),
                      (conv_model(C=32770, O=1, k=1, padding=0, per_channel=False), {}),
                      (torch.nn.Sequential(*linear_pair(32770, 1, "sym", False, False)), {})):
        assert consumers.fuse_linear_consumers(model, any_channels=True, **kw) == 0
        assert isinstance(model[1], mq.PytorchQuantizationWrapper)
    # depthwise convolutions are out of scope: C = 24 stays with both switches
    model = conv_model(C=24, O=24, groups=24)
    assert consumers.fuse_linear_consumers(model, depthwise=True, convolutions=True, any_channels=True) == 0


def test_eligible_and_the_constructors_without_the_keyword_are_unchanged():
    from mct_quantizers_amd import consumers
    conv = torch.nn.Conv2d
    ok = consumers.QuantizedConv2d.eligible
    assert ok(conv(32, 8, 3)) and not ok(conv(24, 8, 3)) and not ok(conv(3, 8, 7, 2, 3)) and not ok(conv(4096, 1, 3))
    assert ok(conv(24, 8, 3), any_channels=True) and ok(conv(3, 8, 7, 2, 3), any_channels=True) and ok(conv(32, 8, 3), any_channels=True)
    assert not ok(conv(4097, 1, 3), any_channels=True) and not ok(conv(24, 8, 3), any_channels=False)
    assert not ok(conv(24, 24, 3, groups=2), any_channels=True) and not ok(conv(24, 8, 3, padding_mode="reflect"), any_channels=True)
    ok1 = consumers.QuantizedConv1x1.eligible
    assert ok1(conv(24, 8, 1)) and ok1(conv(24, 8, 1), any_channels=True) and not ok1(conv(24, 8, 3), any_channels=True)
    assert consumers.QuantizedLinear.eligible(torch.nn.Linear(6, 4)) and consumers.QuantizedLinear.eligible(torch.nn.Linear(6, 4), any_channels=True)
    assert not consumers.QuantizedDepthwiseConv2d.eligible(conv(24, 24, 3, groups=24))
    with pytest.raises(TypeError):
        consumers.QuantizedConv2d(conv(24, 8, 3), None, None)
    pair = conv_pair(C=24)
    with pytest.raises(TypeError):
        consumers.QuantizedConv2d.from_wrapper(pair[1], pair[0].activation_holder_quantizer)
    with pytest.raises(TypeError):
        consumers.QuantizedConv2d(pair[1].layer, pair[1].weights_quantizers["weight"], pair[0].activation_holder_quantizer,
                                  weight=pair[1].weight)


def test_wrapped_resnet50_takes_an_input_holder():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers, workloads
    plain = workloads.wrapped_resnet50(device="cpu", pooled_holder=True)
    model = workloads.wrapped_resnet50(device="cpu", pooled_holder=True, input_holder=True)
    assert len(model) == len(plain) + 1 and isinstance(model[0], mq.PytorchActivationQuantizationHolder)
    assert not isinstance(plain[0], mq.PytorchActivationQuantizationHolder)
    q = model[0].activation_holder_quantizer
    assert consumers._activation_code_params(q) == (4.0 / 128, 0, -128, 127)
    every = dict(chain=True, convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, fused_residuals=True,
                 avg_pools=True)
    _, without = consumers.fuse_linear_consumers_fx(model, **every)
    gm, with_it = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu", pooled_holder=True, input_holder=True),
                                                     any_channels=True, **every)
    assert (without, with_it) == (53, 54)                                # all 54 wrapped layers: the stem is the 54th
    called = [gm.get_submodule(node.target) for node in gm.graph.nodes if node.op == "call_module"]
    assert not any(isinstance(m, (mq.PytorchQuantizationWrapper, mq.PytorchActivationQuantizationHolder)) for m in called)
    stem = called[0]
    assert type(stem) is consumers.QuantizedConv2d and stem._k_pitch == 160 and stem.in_features == 147
    assert sum(isinstance(m, consumers.IntegerConsumer) for m in called) == 54


# ---- whole models: every switch, with and without any_channels ---------------------------------------------------------------
# Built as the models of tests/test_pool_consumer.py are (its docstring says why): power-of-two activation and weight scales, no
# bias, sums of at most 147 products of |a| <= 255 and |w| <= 128 in the layers the switch replaces -- their float32 products are
# exact, so the rewrite with ``any_channels=True`` must return, bit for bit, what the same rewrite without it returns.

EVERY = dict(chain=True, uniform_weights=True, convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True, pools=True,
             fused_residuals=True, concats=True, avg_pools=True, muls=True, hard_activations=True, upsamples=True)


class StemNet(torch.nn.Module):
    """input holder -> 7 x 7 / 2 stem (3 channels) -> ReLU -> holder -> max pool -> a bottleneck with a downsample branch -> a
    last convolution: the front of workloads.wrapped_resnet50(input_holder=True), scaled down."""

    def __init__(self):
        super().__init__()
        from test_pool_consumer import pot_conv, pot_holder
        self.h_in, self.c0, self.h0 = pot_holder(True), pot_conv(3, 16, 7, 1, stride=2), pot_holder()
        self.pool = torch.nn.MaxPool2d(3, 2, 1)
        self.c1, self.h1, self.c2, self.h2 = pot_conv(16, 16, 1, 2), pot_holder(), pot_conv(16, 16, 3, 3), pot_holder()
        self.c3, self.down, self.h3, self.last = pot_conv(16, 32, 1, 4), pot_conv(16, 32, 1, 5), pot_holder(), pot_conv(32, 16, 1, 6)

    def forward(self, x):
        a = self.pool(self.h0(torch.relu(self.c0(self.h_in(x)))))
        y = self.c3(self.h2(torch.relu(self.c2(self.h1(torch.relu(self.c1(a)))))))
        return self.last(self.h3(torch.relu(y + self.down(a))))


class InvertedBlock(torch.nn.Module):
    """MobileNetV2's real block 24 -> 144 -> 144 -> 24 with its identity, a holder behind the add and a last 24 -> 16 layer."""

    def __init__(self):
        super().__init__()
        from test_hard_act_consumer import pot_dw
        from test_pool_consumer import pot_conv, pot_holder
        self.h_in, self.e, self.h1 = pot_holder(True), pot_conv(24, 144, 1, 1), pot_holder()
        self.dw, self.h2, self.p = pot_dw(144, 2), pot_holder(), pot_conv(144, 24, 1, 3)
        self.h_out, self.last = pot_holder(True), pot_conv(24, 16, 1, 4)
        with torch.no_grad():
            self.p.weight.mul_(0.25)

    def forward(self, x):
        relu6 = torch.nn.functional.relu6
        a = self.h_in(x)
        y = relu6(self.dw(self.h1(relu6(self.e(a)))))
        return self.last(self.h_out(a + self.p(self.h2(y))))


# model -> (class, input shape, wrapped layers replaced without / with the switch, the consumers that are padded)
MODELS = {"stem": (StemNet, (2, 3, 17, 13), 5, 6, {"c0_qlinear": 160}),
          "inverted": (InvertedBlock, (2, 24, 9, 7), 2, 4, {"e_qlinear": 32, "last_qlinear": 32})}


def model_input(name, device="cpu"):
    return (torch.randn(*MODELS[name][1], generator=torch.Generator().manual_seed(21)) * 1.5).to(device)


def rewritten_pair(name, device="cpu"):
    """(the rewrite with every switch and any_channels, the same rewrite without it) of one of MODELS, their counts checked."""
    from mct_quantizers_amd import consumers
    make, _, n_without, n_with, padded = MODELS[name]
    gm, n = consumers.fuse_linear_consumers_fx(make().to(device).eval(), any_channels=True, **EVERY)
    gm0, n0 = consumers.fuse_linear_consumers_fx(make().to(device).eval(), **EVERY)
    assert (n0, n) == (n_without, n_with), (n0, n)
    pitches = {k: m._k_pitch for k, m in gm.named_modules() if isinstance(m, consumers.QuantizedLinear) and m._k_pitch is not None}
    assert pitches == padded, pitches
    assert not any(isinstance(m, consumers.QuantizedLinear) and m._k_pitch is not None for m in gm0.modules())
    return gm, gm0


@pytest.mark.parametrize("name", list(MODELS))
def test_whole_models_with_every_switch_equal_the_rewrite_without_any_channels_cpu(name):
    import mct_quantizers_amd as mq
    gm, gm0 = rewritten_pair(name)
    called = [gm.get_submodule(node.target) for node in gm.graph.nodes if node.op == "call_module"]
    assert not any(isinstance(m, (mq.PytorchQuantizationWrapper, mq.PytorchActivationQuantizationHolder)) for m in called)
    x = model_input(name)
    y, y0 = gm(x), gm0(x)
    assert y.dtype == torch.float32 and torch.equal(y, y0) and len(torch.unique(y)) > 50
    assert torch.equal(y, MODELS[name][0]().eval()(x))                    # exact products: the float32 chain itself


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------

def test_im2col_pad_argument_validation_needs_no_gpu():
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    E, P = native.MCTQ_E_ARG, 4096              # an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(x=P, y=P, B=2, H=5, W=7, C=24, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, pad=114)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_codes_im2col_pad_nhwc(v["x"], v["y"], v["B"], v["H"], v["W"], v["C"], v["kh"], v["kw"], v["sh"], v["sw"],
                                              v["ph"], v["pw"], v["dh"], v["dw"], v["pad"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    for extent in "BHWC":
        refused(b"negative extent", **{extent: -1})
    refused(b"kernel size below 1", kh=0)
    refused(b"stride below 1", sw=0)
    refused(b"dilation below 1", dh=0)
    refused(b"negative padding", pw=-1)
    refused(b"pad_code outside [-128, 255]", pad=256)
    refused(b"pad_code outside [-128, 255]", pad=-129)
    refused(b"NULL pointer", x=None)
    refused(b"NULL pointer", y=None)
    refused(b"codes and patches must be 16-byte aligned", x=P + 8)
    refused(b"codes and patches must be 16-byte aligned", y=P + 1)
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kh=8)              # 8 > 5 + 2
    refused(b"the kernel does not fit the padded image (Ho <= 0 or Wo <= 0)", kw=5, dw=3)        # 13 > 7 + 2
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", C=3641)                  # 9 * 3641 = 32769: Kp > 32768
    refused(b"kh * kw * channels > 32768: outside the consumer's limit", C=32769, kh=1, kw=1, ph=0, pw=0)
    assert call(C=32760, kh=1, kw=1, ph=0, pw=0, B=0) == 0
    refused(b"too many output rows for one launch", B=2 ** 31, kh=1, kw=1, ph=0, pw=0, H=1, W=1)
    refused(b"padded image extent exceeds 2^31 - 1", H=2 ** 31)
    refused(b"an image of a non-empty batch needs at least one pixel", H=0, ph=2)                # padding alone makes room
    # the tuning key: 4-byte pieces need channels % 4 == 0
    try:
        assert lib.mctq_set_tuning(b"im2col_grain", 4) == 0
        refused(b"im2col_grain 4 needs channels % 4 == 0", C=6)
        assert call(B=0) == 0                                              # C = 24: fine
        assert lib.mctq_set_tuning(b"im2col_grain", 1) == 0 and call(C=6, B=0) == 0
        assert lib.mctq_set_tuning(b"im2col_grain", 2) == E
        assert lib.mctq_last_error() == b"im2col_grain must be 0 (by rule), 1 (bytes) or 4 (dwords)"
    finally:
        assert lib.mctq_set_tuning(b"im2col_grain", 0) == 0
    assert call(C=6, B=0) == 0
    # an empty batch returns 0: no launch, no pointer is looked at; so do no channels
    assert call(B=0) == 0 and call(B=0, x=None, y=None) == 0 and call(C=0) == 0
    assert call(pad=-128, B=0) == 0 and call(pad=255, B=0) == 0
    for C in (1, 3, 16, 17, 40):
        assert call(C=C, B=0) == 0                                         # any channel count is taken
    assert lib.mctq_launch_count() == count                                # refused and empty calls launch nothing
