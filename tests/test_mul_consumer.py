"""Elementwise multiply on activation codes: host logic and the CPU route (include/mctq_hip.h: mctq_codes_mul_nhwc; hip/ops.py:
codes_mul; consumers.QuantizedMul and the ``muls`` switch of fuse_linear_consumers_fx).

Everything here is exact, so every check is equality.  A holder's float32 output is ``float(code - zp) * scale`` bit for bit,
``torch.mul`` is one IEEE float32 multiplication and the holder behind it codes every element by itself, so the code of a product
is a function of the two operand codes: ``ql_code(join_residual(ca - za, sa) * join_residual(cg - zg, sg))`` in the output's
form.  The op is pinned against that definition written in numpy float32, for all 65 536 pairs of codes of every combination of
code types, and against real holders around ``torch.mul``.

A model rewritten with ``muls=True`` is compared bit for bit with the same rewrite without it and with the model as built.
Without the switch the layers behind the multiply stay float32 wrappers, so the models are built as those of
tests/test_pool_consumer.py are (its docstring says why): power-of-two activation and weight scales, no bias, sums of at most 144
products -- their float32 products are exact and equal the consumers' integer sums; the squeeze averages 16 pixels, so its mean
is exact too (tests/test_avgpool_consumer.py)."""
import functools
import itertools
import operator
import warnings

import numpy as np
import pytest
import torch

from test_concat_consumer import _form, holder_of as _holder_of
from test_join_consumer import _targets
from test_pool_consumer import _of, pot_conv, unsigned_pot

F = torch.nn.functional


def holder_of(kind):
    """tests/test_concat_consumer.py's holders, and "u1": unsigned with threshold 1 (scale 1 / 256), what follows a hardsigmoid."""
    import mct_quantizers_amd as mq
    return mq.PytorchActivationQuantizationHolder(unsigned_pot(1.0)) if kind == "u1" else _holder_of(kind)


# ---- the op's cases: shared by the CPU and GPU tests --------------------------------------------------------------------------

COMBOS = list(itertools.product((False, True), repeat=3))          # (a is int8, g is int8, out is int8): all 8


def form_triples(a_signed, g_signed, o_signed):
    """Two triples ((sa, za), (sg, zg), (so, zo, qmin, qmax)) per combination of code types.  The first: scales that are no
    powers of two, zero points inside the types, so that both operands take both signs and the products pass both ends of the
    output's whole type.  The second: power-of-two scales (every product is exact and many land on rounding ties), a zero
    point at the end of a type, a 7-bit output domain."""
    first = ((0.05, -5 if a_signed else 114), (0.011, 17 if g_signed else 30),
             (0.03, -5, -128, 127) if o_signed else (0.03, 114, 0, 255))
    second = ((1.0 / 32, 0 if a_signed else 128), (1.0 / 128, -128 if g_signed else 0),
              (1.0 / 64, 0, -64, 63) if o_signed else (1.0 / 64, 64, 0, 127))
    return first, second


def code_reference(v, scale, zp, qmin, qmax):
    """The code of float32 values: clamp(rint(v * (1 / scale)) + zp, qmin, qmax), NaN -> qmin; int32."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(v, f32) * (f32(1.0) / f32(scale))).astype(f32) + f32(zp)
    q = np.where(np.isnan(q), f32(qmin), q)
    return np.clip(q, f32(qmin), f32(qmax)).astype(np.int32)


def mul_reference(a, g, out_form, gate_form=None):
    """The definition in numpy float32: a = (codes, scale, zero point), g likewise or, with ``gate_form = (qmin, qmax)``, raw
    float32 values that are coded in g's form first -> codes of the broadcast shape in ``out_form = (scale, zp, qmin, qmax)``."""
    (ac, sa, za), (gc, sg, zg) = a, g
    scale, zp, qmin, qmax = out_form
    f32 = np.float32
    if gate_form is not None:
        gc = code_reference(gc, sg, zg, *gate_form)
    with np.errstate(all="ignore"):
        va = (ac.astype(np.int32) - np.int32(za)).astype(f32) * f32(sa)                # holder A's float32 output
        vg = (gc.astype(np.int32) - np.int32(zg)).astype(f32) * f32(sg)                # holder G's
        m = (va * vg).astype(f32)                                                       # torch.mul: one float32 rounding
    return code_reference(m, scale, zp, qmin, qmax).astype(np.uint8 if qmin >= 0 else np.int8)


def every_code(signed):
    return np.arange(-128, 128).astype(np.int8) if signed else np.arange(256).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pairs_case(combo, which):
    """All 65 536 pairs (ca, cg) as a 256 x 256 same-shape case (256 pixels of 256 channels): (a, g, out_form, the reference's
    result), computed once and shared; read-only."""
    a_signed, g_signed, o_signed = combo
    (sa, za), (sg, zg), out_form = form_triples(*combo)[which]
    ac = np.repeat(every_code(a_signed)[:, None], 256, axis=1)
    gc = np.repeat(every_code(g_signed)[None, :], 256, axis=0)
    want = mul_reference((ac, sa, za), (gc, sg, zg), out_form)
    for arr in (ac, gc, want):
        arr.setflags(write=False)
    return (ac, sa, za), (gc, sg, zg), out_form, want


# (B, H * W, C): one pixel; the gate row is the pixel; 315 chunks with image boundaries inside a wavefront and a partly empty last
# block; a row longer than a wavefront
SMALL = [(1, 1, 16), (2, 1, 16), (3, 35, 48), (2, 49, 272)]
GATES = ("same", "row", "row f32")


def tie_values(rng, shape, scale, zp, qmin, qmax):
    """float32 values to be coded in (scale, zp, qmin, qmax): random ones, rounding ties (k + 0.5) * scale, values beyond both
    clamps, +-inf and NaN."""
    v = (rng.uniform(qmin - zp - 4, qmax - zp + 4, shape) * scale).astype(np.float32)
    flat = v.reshape(-1)
    ties = (rng.integers(qmin - zp - 2, qmax - zp + 2, flat.size // 3) + 0.5) * scale
    flat[:ties.size] = ties.astype(np.float32)
    special = [np.inf, -np.inf, np.nan, (qmax - zp + 1000) * scale, (qmin - zp - 1000) * scale, 0.0, -0.0]
    flat[-len(special):] = special if flat.size >= 2 * len(special) else flat[-len(special):]
    return flat.reshape(shape)


@functools.lru_cache(maxsize=None)
def small_case(index, gate):
    """(a, g, out_form, gate_form or None, the reference's result) for SMALL[index] and a gate form, a as [B, H * W, C], g as
    [B, H * W, C] ("same") or [B, 1, C]; the code types rotate through COMBOS; read-only."""
    B, n, C = SMALL[index]
    combo = COMBOS[(3 * index + GATES.index(gate)) % 8]
    (sa, za), (sg, zg), out_form = form_triples(*combo)[index % 2]
    rng = np.random.default_rng(100 * index + GATES.index(gate))
    codes = lambda signed, shape: (rng.integers(-128, 128, shape).astype(np.int8) if signed              # noqa: E731
                                   else rng.integers(0, 256, shape).astype(np.uint8))
    ac = codes(combo[0], (B, n, C))
    gate_form = None
    if gate == "same":
        gc = codes(combo[1], (B, n, C))
    elif gate == "row":
        gc = codes(combo[1], (B, 1, C))
    else:
        gate_form = (-128, 127) if combo[1] else (0, 255)
        gc = tie_values(rng, (B, 1, C), sg, zg, *gate_form)
    want = mul_reference((ac, sa, za), (gc, sg, zg), out_form, gate_form)
    for arr in (ac, gc, want):
        arr.setflags(write=False)
    return (ac, sa, za), (gc, sg, zg), out_form, gate_form, want


def small_cases():
    for index in range(len(SMALL)):
        for gate in GATES:
            if gate == "same" and index == 3:
                continue
            yield index, gate


def as_tensor(operand, device="cpu"):
    c, s, z = operand
    return torch.from_numpy(c.copy()).to(device), s, z


# ---- the op ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBOS)
def test_codes_mul_on_cpu_equals_the_reference_for_every_pair_of_codes(combo):
    from mct_quantizers_amd.hip import ops
    for which in (0, 1):
        a, g, out_form, want = pairs_case(combo, which)
        # the comparison cannot pass on a constant: both ends of the clamp are reached, and many codes between them
        assert want.min() == out_form[2] and want.max() == out_form[3] and len(np.unique(want)) > 50, (combo, which)
        got = ops.codes_mul(as_tensor(a), as_tensor(g), out_form)
        assert got.dtype == (torch.int8 if combo[2] else torch.uint8) and got.is_contiguous() and tuple(got.shape) == (256, 256)
        assert np.array_equal(got.numpy(), want), (combo, which)
        assert got.dtype == ops._code_dtype(out_form[2], out_form[3])[0]


def test_codes_mul_small_shapes_on_cpu_equal_the_reference():
    from mct_quantizers_amd.hip import ops
    n = 0
    for index, gate in small_cases():
        a, g, out_form, gate_form, want = small_case(index, gate)
        got = ops.codes_mul(as_tensor(a), as_tensor(g), out_form, gate_form)
        assert tuple(got.shape) == SMALL[index] and np.array_equal(got.numpy(), want), (index, gate)
        n += 1
    assert n == 11


@pytest.mark.parametrize("kinds", [("s", "uni", "u4"), ("u4", "u2", "s"), ("uni", "s", "uni"), ("s4", "s", "s4")])
def test_codes_mul_gives_the_codes_of_the_holder_behind_torch_mul(kinds):
    """The contract is the float32 chain's, not just self-consistent: real holders around ``torch.mul`` on random values, on
    rounding ties of both operand holders and on values beyond their clamps."""
    from mct_quantizers_amd.hip import ops
    ha, hg, hm = (holder_of(k) for k in kinds)
    rng = np.random.default_rng(31)
    fa, fg, (s, z, qmin, qmax) = _form(ha), _form(hg), _form(hm)
    x = torch.from_numpy(tie_values(rng, (2, 16, 5, 3), *fa))
    v = torch.from_numpy(tie_values(rng, (2, 16, 5, 3), *fg))
    x, v = torch.nan_to_num(x, nan=0.3), torch.nan_to_num(v, nan=-0.2)                   # (a holder keeps a NaN; its code is qmin)
    with torch.no_grad():
        chain = hm(ha(x) * hg(v))                                                          # float32, what the model as built computes
    want = ops.fq_codes_nhwc(chain, qmin, qmax, s, z)
    a = (ops.fq_codes_nhwc(x, fa[2], fa[3], fa[0], fa[1]), fa[0], fa[1])
    g = (ops.fq_codes_nhwc(v, fg[2], fg[3], fg[0], fg[1]), fg[0], fg[1])
    got = ops.codes_mul(a, g, (s, z, qmin, qmax))
    assert torch.equal(got, want) and len(torch.unique(got)) > 20
    assert torch.equal(ops.dequantize_codes(got, s, z).permute(0, 3, 1, 2), chain)       # ... and they stand for that tensor
    assert np.array_equal(got.numpy(), mul_reference((a[0].numpy(), *fa[:2]), (g[0].numpy(), *fg[:2]), (s, z, qmin, qmax)))
    # the gate of an SE block: [B, C, 1, 1] next to [B, C, H, W], given as codes and as float32 values
    gate = v[:, :, :1, :1].contiguous()
    with torch.no_grad():
        chain = hm(ha(x) * hg(gate))
    want = ops.fq_codes_nhwc(chain, qmin, qmax, s, z)
    gate_codes = ops.fq_codes_nhwc(gate, fg[2], fg[3], fg[0], fg[1])
    assert torch.equal(ops.codes_mul(a, (gate_codes, fg[0], fg[1]), (s, z, qmin, qmax)), want)
    assert torch.equal(ops.codes_mul(a, (gate.permute(0, 2, 3, 1), fg[0], fg[1]), (s, z, qmin, qmax), gate_form=fg[2:]), want)


def test_broadcast_gates_in_both_operand_orders():
    from mct_quantizers_amd.hip import ops
    rng = np.random.default_rng(7)
    for combo in COMBOS:
        (sa, za), (sg, zg), out_form = form_triples(*combo)[0]
        ac = (rng.integers(-128, 128, (2, 3, 5, 16)).astype(np.int8) if combo[0] else rng.integers(0, 256, (2, 3, 5, 16)).astype(np.uint8))
        gc = (rng.integers(-128, 128, (2, 1, 1, 16)).astype(np.int8) if combo[1] else rng.integers(0, 256, (2, 1, 1, 16)).astype(np.uint8))
        a, g = (ac, sa, za), (gc, sg, zg)
        want = mul_reference(a, g, out_form)
        assert want.shape == (2, 3, 5, 16)
        assert np.array_equal(ops.codes_mul(as_tensor(a), as_tensor(g), out_form).numpy(), want)
        assert np.array_equal(ops.codes_mul(as_tensor(g), as_tensor(a), out_form).numpy(), want)      # the gate first
        # ... which is torch.mul of the dequantized operands, coded
        v = ops.dequantize_codes(*as_tensor(a)) * ops.dequantize_codes(*as_tensor(g))
        assert np.array_equal(ops.fq_codes(v, None, None, None, out_form[2], out_form[3], out_form[0], out_form[1]).numpy(), want)


def test_float32_gates_equal_coding_the_gate_first():
    from mct_quantizers_amd.hip import ops
    rng = np.random.default_rng(9)
    for combo in COMBOS:
        for which in (0, 1):
            (sa, za), (sg, zg), out_form = form_triples(*combo)[which]
            gate_form = ((-128, 127) if combo[1] else (0, 255)) if which == 0 else ((-100, 90) if combo[1] else (3, 200))
            ac = (rng.integers(-128, 128, (2, 7, 32)).astype(np.int8) if combo[0] else rng.integers(0, 256, (2, 7, 32)).astype(np.uint8))
            gv = tie_values(rng, (2, 1, 32), sg, zg, *gate_form)
            assert np.isnan(gv).any() and np.isinf(gv).any()
            got = ops.codes_mul(as_tensor((ac, sa, za)), as_tensor((gv, sg, zg)), out_form, gate_form)
            coded = ops.fq_codes(torch.from_numpy(gv.copy()), None, None, None, *gate_form, sg, zg)
            assert coded.dtype == (torch.int8 if combo[1] else torch.uint8)
            assert int(coded.min()) == gate_form[0] and int(coded.max()) == gate_form[1]          # both clamps of G are reached
            assert torch.equal(got, ops.codes_mul(as_tensor((ac, sa, za)), (coded, sg, zg), out_form))
            assert np.array_equal(got.numpy(), mul_reference((ac, sa, za), (gv, sg, zg), out_form, gate_form))
            assert np.array_equal(coded.numpy(), code_reference(gv, sg, zg, *gate_form))


TORCH_ROUTE_SHAPES = [((2, 3, 5, 24), (2, 1, 1, 24)), ((2, 3, 5, 24), (2, 3, 5, 24)),      # C = 24
                      ((2, 3, 5, 16), (2, 3, 5, 1)),                                      # [B, 1, H, W] in NCHW terms
                      ((2, 3, 5, 16), (1, 1, 1, 16)),                                     # [1, C, 1, 1]
                      ((2, 3, 5, 16), (16,)), ((5, 16), (2, 3, 1, 16))]                   # operands of different rank


def torch_route_case(index, float_gate=False):
    """(a, g, out_form, gate_form, the reference's result) for TORCH_ROUTE_SHAPES[index]."""
    sa_, sg_ = TORCH_ROUTE_SHAPES[index]
    combo = COMBOS[(index + 3) % 8]
    (sa, za), (sg, zg), out_form = form_triples(*combo)[0]
    rng = np.random.default_rng(50 + index)
    ac = rng.integers(-128, 128, sa_).astype(np.int8) if combo[0] else rng.integers(0, 256, sa_).astype(np.uint8)
    gate_form = None
    if float_gate:
        gate_form = (-128, 127) if combo[1] else (0, 255)
        gc = tie_values(rng, sg_, sg, zg, *gate_form)
    else:
        gc = rng.integers(-128, 128, sg_).astype(np.int8) if combo[1] else rng.integers(0, 256, sg_).astype(np.uint8)
    return (ac, sa, za), (gc, sg, zg), out_form, gate_form, mul_reference((ac, sa, za), (gc, sg, zg), out_form, gate_form)


def test_shapes_of_the_torch_route():
    from mct_quantizers_amd.hip import ops
    for index in range(len(TORCH_ROUTE_SHAPES)):
        for float_gate in (False, True):
            a, g, out_form, gate_form, want = torch_route_case(index, float_gate)
            got = ops.codes_mul(as_tensor(a), as_tensor(g), out_form, gate_form)
            assert got.is_contiguous() and tuple(got.shape) == want.shape == tuple(np.broadcast_shapes(a[0].shape, g[0].shape))
            assert np.array_equal(got.numpy(), want), (index, float_gate)
    # a non-contiguous operand, and an empty batch
    a, g, out_form, _, want = small_case(2, "row")
    x = torch.from_numpy(a[0].copy()).permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not x.is_contiguous() and np.array_equal(ops.codes_mul((x, *a[1:]), as_tensor(g), out_form).numpy(), want)
    empty = ops.codes_mul((torch.zeros(0, 4, 16, dtype=torch.uint8), 0.1, 0), (torch.zeros(0, 1, 16, dtype=torch.int8), 0.1, 0), (0.03, -5, -128, 127))
    assert empty.shape == (0, 4, 16) and empty.dtype == torch.int8


def test_codes_mul_validation():
    from mct_quantizers_amd.hip import ops
    u8, out = torch.zeros(2, 3, 16, dtype=torch.uint8), (0.05, 3, 0, 255)
    with pytest.raises(TypeError):
        ops.codes_mul((u8.float(), 0.1, 0), (u8, 0.1, 0), out)                          # a float32 first operand
    with pytest.raises(TypeError):
        ops.codes_mul((u8, 0.1, 0), (u8.float(), 0.1, 0), out)                          # float32 values without G's domain
    with pytest.raises(TypeError):
        ops.codes_mul((u8, 0.1, 0), (u8, 0.1, 0), out, gate_form=(0, 255))              # G's domain with codes
    for bad_zp, t in ((-1, u8), (256, u8), (128, u8.to(torch.int8)), (-129, u8.to(torch.int8))):
        with pytest.raises(ValueError, match="zero point"):
            ops.codes_mul((t, 0.1, bad_zp), (u8, 0.1, 0), out)
        with pytest.raises(ValueError, match="zero point"):
            ops.codes_mul((u8, 0.1, 0), (t, 0.1, bad_zp), out)
    with pytest.raises(ValueError, match="zero point"):
        ops.codes_mul((u8, 0.1, 0), (u8, 0.1, 0), (0.05, 256, 0, 255))
    with pytest.raises(ValueError, match="zero point"):
        ops.codes_mul((u8, 0.1, 0), (u8.float(), 0.1, 200), out, gate_form=(-128, 127))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for args in (((u8, bad, 0), (u8, 0.1, 0), out), ((u8, 0.1, 0), (u8, bad, 0), out), ((u8, 0.1, 0), (u8, 0.1, 0), (bad, 0, 0, 255))):
            with pytest.raises(ValueError, match="scales"):
                ops.codes_mul(*args)
    with pytest.raises(ValueError, match="8-bit code"):
        ops.codes_mul((u8, 0.1, 0), (u8, 0.1, 0), (0.1, 0, -1, 255))
    with pytest.raises(RuntimeError):
        ops.codes_mul((u8, 0.1, 0), (u8[:, :2], 0.1, 0), out)                           # shapes torch.mul does not broadcast


# ---- the module ------------------------------------------------------------------------------------------------------------

def check_mul_module(device):
    """QuantizedMul on float32 operands, on codes and on a mix, in both operand orders, 4-D, gates, rows and the shapes of the
    torch route, against the holders around torch.mul; returns the outputs."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    outs = []
    g = torch.Generator().manual_seed(21)
    for kinds, C in ((("u8", "uni", "u4"), 16), (("s", "u2", "s4"), 32), (("uni", "s", "uni"), 24)):
        ha, hg, hm = (holder_of(k) for k in kinds)
        qm = consumers.QuantizedMul([ha.activation_holder_quantizer, hg.activation_holder_quantizer], hm.activation_holder_quantizer)
        swapped = consumers.QuantizedMul([hg.activation_holder_quantizer, ha.activation_holder_quantizer], hm.activation_holder_quantizer)
        assert qm.activation_code_params() == _form(hm) and [qm.operand_code_params(i) for i in (0, 1)] == [_form(ha), _form(hg)]
        assert not isinstance(qm, consumers.IntegerConsumer)
        s, z, qmin, qmax = _form(hm)
        fa, fg = _form(ha), _form(hg)
        x = (torch.randn(2, C, 5, 3, generator=g) * 3.0).to(device)
        shapes = [(2, C, 5, 3), (2, C, 1, 1), (2, 1, 5, 3), (1, C, 1, 1), (C, 1, 1), (3,)]
        for shape in shapes:
            v = (torch.randn(*shape, generator=g) * 1.5).to(device)
            with torch.no_grad():
                want = hm(ha(x.cpu()) * hg(v.cpu()))
            y = qm(x, v)
            assert y.dtype == ops._code_dtype(qmin, qmax)[0] and y.shape == (2, C, 5, 3), shape
            assert y.is_contiguous(memory_format=torch.channels_last)                    # NCHW-shaped, NHWC-stored
            assert torch.equal(ops.dequantize_codes(y.cpu(), s, z), want), (kinds, shape)
            xc = ops.fq_codes_nhwc(x, fa[2], fa[3], fa[0], fa[1]).permute(0, 3, 1, 2)
            vc = ops.fq_codes(v, None, None, None, fg[2], fg[3], fg[0], fg[1])
            if v.dim() == 4:
                vc = vc.contiguous(memory_format=torch.channels_last)
            assert torch.equal(qm(xc, vc), y) and torch.equal(qm(xc, v), y) and torch.equal(qm(x, vc), y)     # codes in, and mixes
            assert torch.equal(swapped(v, x), y) and torch.equal(swapped(vc, xc), y) and torch.equal(swapped(v, xc), y)
            with torch.no_grad():
                assert torch.equal(qm(ha(x.cpu()).to(device), hg(v.cpu()).to(device)), y)  # the holders' outputs: the same codes
            outs.append(y.cpu())
        rows, vrows = x.permute(0, 2, 3, 1).reshape(-1, C), (torch.randn(30, C, generator=g) * 1.5).to(device)   # [M, C] rows
        with torch.no_grad():
            want = hm(ha(rows.cpu()) * hg(vrows.cpu()))
        y2 = qm(rows, vrows)
        assert y2.shape == (30, C) and torch.equal(ops.dequantize_codes(y2.cpu(), s, z), want)
        assert torch.equal(qm(ops.fq_codes(rows, None, None, None, fa[2], fa[3], fa[0], fa[1]), vrows), y2)
        outs.append(y2.cpu())
        empty = qm(x[:0], x[:0, :, :1, :1])
        assert empty.shape == (0, C, 5, 3) and empty.dtype == y.dtype
        assert qm(x[:0], x[:0]).shape == (0, C, 5, 3)
        wrong = torch.int8 if xc.dtype == torch.uint8 else torch.uint8
        with pytest.raises(TypeError):
            qm(xc.to(wrong), x)
        with pytest.raises(TypeError):
            qm(x, ops.fq_codes(x, None, None, None, fg[2], fg[3], fg[0], fg[1]).to(torch.int8 if fg[2] >= 0 else torch.uint8))
        with pytest.raises(TypeError):
            qm(x.double(), x)
        with pytest.raises(TypeError):
            qm(x, x[:, :, :1, :1].double())
    return outs


def test_quantized_mul_on_cpu():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    assert len(check_mul_module("cpu")) == 21
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=16, threshold=[4.0], signed=True)
        lut = mq.pytorch_quantizers.ActivationLutPOTInferableQuantizer(num_bits=4, lut_values=[0.0, 32.0, 64.0, 96.0], threshold=[4.0],
                                                                       signed=False, lut_values_bitwidth=8)
    ok = unsigned_pot()
    for bad in ([ok, wide], [wide, ok]):
        with pytest.raises(NotImplementedError, match="wider than 8 bits"):
            consumers.QuantizedMul(bad, ok)
    with pytest.raises(NotImplementedError, match="wider than 8 bits"):
        consumers.QuantizedMul([ok, ok], wide)
    with pytest.raises(TypeError):
        consumers.QuantizedMul([ok, lut], ok)
    for count in ([], [ok], [ok, ok, ok]):
        with pytest.raises(ValueError):
            consumers.QuantizedMul(count, ok)


# ---- the rewrite -----------------------------------------------------------------------------------------------------------

class SE(torch.nn.Module):
    """A squeeze-and-excitation block as MCT exports it: conv -> ReLU -> A -> {mean((2, 3), keepdim) -> B -> fc1 -> ReLU -> C ->
    fc2 -> Hardsigmoid -> G} -> mul -> M -> conv.  ``how``: the way the multiply is written, and which operand comes first."""

    def __init__(self, how="operator"):
        super().__init__()
        self.how = how
        self.h0, self.c, self.a = holder_of("s4"), pot_conv(16, 16, 3, 1), holder_of("u8")
        self.b, self.fc1, self.hc, self.fc2 = holder_of("u4"), pot_conv(16, 16, 1, 2), holder_of("u4"), pot_conv(16, 16, 1, 3)
        self.gate, self.g = torch.nn.Hardsigmoid(), holder_of("u1")
        self.m, self.last = holder_of("u8"), pot_conv(16, 16, 1, 4)

    def forward(self, x):
        a = self.a(torch.relu(self.c(self.h0(x))))
        s = self.b(a.mean((2, 3), keepdim=True))
        h = self.hc(torch.relu(self.fc1(s)))
        g = self.g(self.gate(self.fc2(h)))
        how = self.how
        if how == "operator":
            m = a * g
        elif how == "gate_first":
            m = g * a
        elif how == "torch.mul":
            m = torch.mul(a, g)
        elif how == "torch.multiply":
            m = torch.multiply(g, a)
        elif how == "method":
            m = a.mul(g)
        else:
            assert how == "multiply_method"
            m = g.multiply(a)
        return self.last(self.m(m))


class Gated(torch.nn.Module):
    """A gated layer: two conv -> ReLU -> holder branches multiplied, same shape; ``how``: ``*`` or ``*=`` (the first operand's
    holder has no other reader)."""

    def __init__(self, how="operator"):
        super().__init__()
        self.how = how
        self.h0 = holder_of("s4")
        self.p, self.q = pot_conv(16, 16, 3, 1), pot_conv(16, 16, 1, 2)
        self.h_p, self.h_q = holder_of("u4"), holder_of("s4")
        self.m, self.last = holder_of("u8"), pot_conv(16, 16, 3, 3)

    def forward(self, x):
        x = self.h0(x)
        p = self.h_p(torch.relu(self.p(x)))
        q = self.h_q(F.relu6(self.q(x)))
        if self.how == "inplace":
            p *= q
        else:
            p = p * q
        return self.last(self.m(p))


def block_input(device="cpu"):
    return (torch.randn(2, 16, 4, 4, generator=torch.Generator().manual_seed(12)) * 1.5).to(device)


ALL = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, avg_pools=True, concats=True,
           fused_residuals=True, depthwise=True, uniform_weights=True, chain=True)
SWITCH_SETS = [dict(), dict(convolutions=True), dict(convolutions=True, shared_holders=True),
               dict(convolutions=True, shared_holders=True, avg_pools=True),
               dict(convolutions=True, shared_holders=True, stay_on_codes=True, avg_pools=True), ALL]


def rewritten(make, device="cpu", muls=True, **switches):
    from mct_quantizers_amd import consumers
    return consumers.fuse_linear_consumers_fx(make().to(device).eval(), muls=muls, **(switches or ALL))


@pytest.mark.parametrize("how", ["operator", "gate_first", "torch.mul", "torch.multiply", "method", "multiply_method"])
def test_se_block_keeps_its_multiply_on_codes(how):
    from mct_quantizers_amd import consumers as C
    make = lambda: SE(how)                                   # noqa: E731
    x = block_input()
    with torch.no_grad():
        want = make().eval()(x)
    assert len(torch.unique(want)) > 50
    for switches in SWITCH_SETS:
        gm, n = C.fuse_linear_consumers_fx(make().eval(), muls=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(make().eval(), **switches)
        # fc1, fc2 and last, the layer behind M; c, a 3 x 3 convolution, with ``convolutions``
        assert n == n0 == (4 if switches.get("convolutions") else 3), switches
        assert len(_of(gm, C.QuantizedMul)) == 1 and not _of(gm0, C.QuantizedMul)
        y = gm(x)
        assert torch.equal(y, gm0(x)) and torch.equal(y, want), switches
        assert "m" not in _targets(gm) and "g" not in _targets(gm) and "m_mul" in _targets(gm) and "last_qlinear" in _targets(gm)
        assert not [t for t in _targets(gm, "call_function") + _targets(gm, "call_method") if "mul" in str(t)]
    big = 1 if how in ("gate_first", "torch.multiply", "multiply_method") else 0          # the large operand's position
    # without shared_holders A, read by the squeeze and the multiply, stays a holder; G, read by the multiply alone, is gone
    gm, _ = C.fuse_linear_consumers_fx(make().eval(), muls=True, convolutions=True)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["m_mul"].args[big] is nodes["a"] and nodes["m_mul"].args[1 - big] is nodes["gate"]
    assert [u.target for u in nodes["m_mul"].users] == ["last_qlinear"]
    # shared_holders + avg_pools: A's join writes no float32 -- its codes go to the squeeze and to the multiply
    gm, _ = C.fuse_linear_consumers_fx(make().eval(), muls=True, convolutions=True, shared_holders=True, avg_pools=True)
    gm0, _ = C.fuse_linear_consumers_fx(make().eval(), convolutions=True, shared_holders=True, avg_pools=True)
    join, join0 = gm.get_submodule("a_join"), gm0.get_submodule("a_join")
    assert isinstance(join, C.QuantizedJoin) and join.relu and not join.want_float and join0.want_float
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    codes = nodes["m_mul"].args[big]
    assert codes.op == "call_function" and codes.args == (nodes["a_join"], 1) and nodes["m_mul"].args[1 - big] is nodes["gate"]
    assert sorted(str(u.target) for u in codes.users) == ["m_mul", "mean_qavgpool"]
    qmul = gm.get_submodule("m_mul")
    assert qmul.operand_code_params(big) == (8.0 / 256, 0, 0, 255) and qmul.operand_code_params(1 - big) == (1.0 / 256, 0, 0, 255)
    assert qmul.activation_code_params() == gm.get_submodule("last_qlinear").activation_code_params() == (8.0 / 256, 0, 0, 255)
    seen = []
    hook = qmul.register_forward_hook(lambda m, args, out: seen.append(([(a.dtype, tuple(a.shape)) for a in args], out.dtype)))
    gm(x)
    hook.remove()
    operands = [(torch.uint8, (2, 16, 4, 4)), (torch.float32, (2, 16, 1, 1))]
    assert seen == [(operands[::-1] if big else operands, torch.uint8)]
    # stay_on_codes: no join is left, the convolution in front emits A's codes with the ReLU folded into their clamp
    gm, _ = rewritten(make)
    assert not _of(gm, C.QuantizedJoin) and torch.relu not in _targets(gm, "call_function")
    producer = gm.get_submodule("c_qlinear")
    assert producer.emit_codes_for == qmul.operand_code_params(big) == (8.0 / 256, 0, 0, 255)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["m_mul"].args[big] is nodes["c_qlinear"] and sorted(u.target for u in nodes["c_qlinear"].users) == ["m_mul", "mean_qavgpool"]
    assert torch.equal(gm(x), want)
    # tracing the rewritten graph again keeps the multiply a leaf and replaces nothing more
    again, n = rewritten(lambda: gm)
    assert n == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), want)


@pytest.mark.parametrize("how", ["operator", "inplace"])
def test_gated_block_keeps_its_multiply_on_codes(how):
    from mct_quantizers_amd import consumers as C
    make = lambda: Gated(how)                                # noqa: E731
    x = block_input()
    with torch.no_grad():
        want = make().eval()(x)
    assert len(torch.unique(want)) > 50
    for switches in SWITCH_SETS:
        gm, n = C.fuse_linear_consumers_fx(make().eval(), muls=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(make().eval(), **switches)
        # last, the layer behind M, is 3 x 3: without ``convolutions`` no consumer takes it and the multiply is left alone;
        # p and q sit behind h0, which has two readers: they need ``shared_holders``
        expected = 0 if not switches.get("convolutions") else (3 if switches.get("shared_holders") else 1)
        assert n == n0 == expected, switches
        assert len(_of(gm, C.QuantizedMul)) == (1 if expected else 0) and not _of(gm0, C.QuantizedMul)
        y = gm(x)
        assert torch.equal(y, gm0(x)) and torch.equal(y, want), switches
    # both operand holders are read by the multiply alone: they leave the graph and the module quantizes the activations' outputs
    gm, n = C.fuse_linear_consumers_fx(make().eval(), muls=True, convolutions=True)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert n == 1 and "h_p" not in nodes and "h_q" not in nodes and "m" not in nodes
    assert nodes["m_mul"].args[0].target is torch.relu and nodes["m_mul"].args[1].target is F.relu6
    # with every switch the branch convolutions emit the operands' codes, each activation folded into its clamp
    gm, n = rewritten(make)
    gm0, n0 = rewritten(make, muls=False)
    assert (n, n0) == (3, 3)
    assert _targets(gm) == ["h0_join", "p_qlinear", "q_qlinear", "m_mul", "last_qlinear"]
    assert not [t for t in _targets(gm, "call_function") if t in (torch.relu, F.relu6)]
    qmul, p, q = gm.get_submodule("m_mul"), gm.get_submodule("p_qlinear"), gm.get_submodule("q_qlinear")
    assert p.emit_codes_for == qmul.operand_code_params(0) == (4.0 / 256, 0, 0, 255) and p.emit_clamp is None
    assert q.emit_codes_for == qmul.operand_code_params(1) == (4.0 / 128, 0, -128, 127) and q.emit_clamp == (0, 127)
    seen = []
    hook = qmul.register_forward_hook(lambda m, args, out: seen.append(([a.dtype for a in args], out.dtype)))
    y = gm(x)
    hook.remove()
    assert seen == [([torch.uint8, torch.int8], torch.uint8)] and torch.equal(y, want) and torch.equal(gm0(x), want)


class Odd(torch.nn.Module):
    """What the switch leaves alone, one at a time."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.h_a, self.h_g, self.m = holder_of("u4"), holder_of("u2"), holder_of("u8")
        self.last = pot_conv(16, 16, 1, 1)

    def forward(self, x):
        a, g, kind = self.h_a(x), self.h_g(x), self.kind
        if kind == "float_user":                             # SE-ResNet: an identity add behind M
            m = self.m(a * g)
            return self.last(m) + m
        if kind == "operand":                                # an operand that is no holder's output
            return self.last(self.m(a * torch.sigmoid(g)))
        if kind == "between":                                # something between the multiply and M
            return self.last(self.m(torch.relu(a * g)))
        if kind == "div":
            return self.last(self.m(a / (g + 1.0)))
        if kind == "scalar":
            return self.last(self.m(a * 0.5))
        if kind == "scalar_mul":
            return self.last(self.m(torch.mul(a, 2)))
        if kind == "out":
            return self.last(self.m(torch.mul(a, g, out=torch.empty_like(x))))
        if kind == "shared_mul":                             # the product feeds something besides M
            p = a * g
            return self.last(self.m(p)) + p
        assert kind == "three"
        return self.last(self.m(torch.stack([a, g]).prod(0)))


@pytest.mark.parametrize("kind", ["float_user", "operand", "between", "div", "scalar", "scalar_mul", "out", "shared_mul", "three"])
def test_what_the_switch_leaves_alone(kind):
    from mct_quantizers_amd import consumers as C
    x = block_input()
    for switches in (dict(), dict(convolutions=True, shared_holders=True), ALL):
        gm, n = C.fuse_linear_consumers_fx(Odd(kind).eval(), muls=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(Odd(kind).eval(), **switches)
        assert n == n0 and not _of(gm, C.QuantizedMul), (kind, switches)
        assert str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
        assert torch.equal(gm(x), gm0(x))


def test_the_same_tensor_at_both_operands():
    """``x * x``: the holder is read by the multiply alone (twice) and leaves; with stay_on_codes the producer keeps its float32
    output, which the module quantizes once per operand."""
    from mct_quantizers_amd import consumers as C

    class Square(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.h0, self.c, self.a, self.m, self.last = holder_of("s4"), pot_conv(16, 16, 1, 1), holder_of("u2"), holder_of("u4"), pot_conv(16, 16, 1, 2)

        def forward(self, x):
            a = self.a(torch.relu(self.c(self.h0(x))))
            return self.last(self.m(a * a))

    x = block_input()
    with torch.no_grad():
        want = Square().eval()(x)
    for switches in (dict(), ALL):
        gm, n = C.fuse_linear_consumers_fx(Square().eval(), muls=True, **switches)
        assert n == 2 and len(_of(gm, C.QuantizedMul)) == 1 and torch.equal(gm(x), want)
        node = next(node for node in gm.graph.nodes if node.target == "m_mul")
        assert node.args[0] is node.args[1] and node.args[0].target is torch.relu
        assert gm.get_submodule("c_qlinear").emit_codes_for is None


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers as C
    for switches in SWITCH_SETS:
        for make in (SE, Gated):
            gm, n = C.fuse_linear_consumers_fx(make().eval(), **switches)
            gm_off, n_off = C.fuse_linear_consumers_fx(make().eval(), muls=False, **switches)
            assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
            assert not _of(gm, C.QuantizedMul)


def test_an_in_place_multiply_needs_a_first_operand_nobody_else_reads():
    """torch.fx traces ``p *= q`` on proxies as ``operator.mul`` (the Gated block's "inplace" form); a graph that does hold
    ``operator.imul`` is taken only where the multiply is the first operand's one reader."""
    import operator
    import torch.fx as fx
    from mct_quantizers_amd import consumers as C
    for shared in (False, True):
        graph = fx.Graph()
        x, y = graph.placeholder("x"), graph.placeholder("y")
        other = graph.call_function(operator.add, (x, y)) if shared else None
        node = graph.call_function(operator.imul, (x, y))
        graph.output((node, other))
        assert C._mul_operands(node) == (None if shared else (x, y))
    graph = fx.Graph()
    x = graph.placeholder("x")
    for target, args, kwargs, ok in ((operator.mul, (x, x), {}, True), (torch.mul, (x, x), {}, True), (torch.multiply, (x, x), {}, True),
                                     (operator.mul, (x, 2.0), {}, False), (operator.mul, (2.0, x), {}, False),
                                     (torch.mul, (x, x), {"out": x}, False), (torch.div, (x, x), {}, False),
                                     (operator.truediv, (x, x), {}, False), (torch.mul, (x,), {"other": x}, False)):
        assert (C._mul_operands(graph.call_function(target, args, kwargs)) is not None) == ok, target
    for name, ok in (("mul", True), ("multiply", True), ("mul_", False), ("div", False)):
        assert (C._mul_operands(graph.call_method(name, (x, x))) is not None) == ok, name


def test_a_block_whose_channels_no_consumer_takes_is_left_alone():
    """MobileNetV3's 72- and 120-channel SE blocks: QuantizedMul takes them (the torch route of check_mul_module's C = 24 case),
    but no integer consumer reads K % 16 != 0, so the layer behind M stays a wrapper and the rewrite leaves the block alone."""
    from mct_quantizers_amd import consumers as C

    class Narrow(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.h0, self.c, self.a = holder_of("s4"), pot_conv(16, 24, 1, 1), holder_of("u8")
            self.fc, self.gate, self.g = pot_conv(24, 24, 1, 2), torch.nn.Hardsigmoid(), holder_of("u1")
            self.b, self.m, self.last = holder_of("u4"), holder_of("u8"), pot_conv(24, 16, 1, 3)

        def forward(self, x):
            a = self.a(torch.relu(self.c(self.h0(x))))
            g = self.g(self.gate(self.fc(self.b(a.mean((2, 3), keepdim=True)))))
            return self.last(self.m(a * g))

    x = block_input()
    gm, n = C.fuse_linear_consumers_fx(Narrow().eval(), muls=True, **ALL)
    gm0, n0 = C.fuse_linear_consumers_fx(Narrow().eval(), **ALL)
    assert n == n0 and not _of(gm, C.QuantizedMul) and str(gm.graph) == str(gm0.graph) and torch.equal(gm(x), gm0(x))


class MulIntoCat(torch.nn.Module):
    """holder A, holder G -> mul -> holder M -> cat([M, holder P], 1) -> holder H -> 1 x 1 convolution: M is the holder behind a
    multiply and an operand holder of a concatenation at once."""

    def __init__(self):
        super().__init__()
        self.a, self.g, self.m, self.p = holder_of("s4"), holder_of("u1"), holder_of("u4"), holder_of("u8")
        self.h, self.last = holder_of("u8"), pot_conv(32, 16, 1, 5)

    def forward(self, x):
        m = self.m(self.a(x) * self.g(x))
        return self.last(self.h(torch.cat([m, self.p(x)], 1)))


# the call targets after fuse_linear_consumers_fx(MulIntoCat(), **switches), as recorded before the two passes became one function
MUL_INTO_CAT = {
    (): (["a", "g", "m", "p", "last_qlinear"], [operator.mul, torch.cat]),
    ("concats",): (["a", "g", "h_concat", "last_qlinear"], [operator.mul]),
    ("muls",): (["a", "g", "m", "p", "last_qlinear"], [operator.mul, torch.cat]),
    ("concats", "muls"): (["a", "g", "h_concat", "last_qlinear"], [operator.mul]),
}


@pytest.mark.parametrize("on", list(MUL_INTO_CAT), ids=lambda on: "+".join(on) or "neither")
def test_a_concatenation_whose_operand_holder_sits_behind_a_multiply(on):
    """The concatenations are rewritten in one whole pass, then the multiplies.  With ``concats`` the QuantizedConcat absorbs M
    and P and reads the float32 product; the multiply stays an operation with and without ``muls``: M's reader is ``torch.cat``,
    no wrapped layer, so M is no candidate of the multiply pass, and behind the concatenation pass no holder is left behind the
    multiply.  A and G, which the multiply reads, stay holders.  Every form returns what the rewrite with neither switch does."""
    from mct_quantizers_amd import consumers as C
    x = block_input()
    gm, n = C.fuse_linear_consumers_fx(MulIntoCat().eval(), **dict.fromkeys(on, True))
    gm0, n0 = C.fuse_linear_consumers_fx(MulIntoCat().eval())
    assert n == n0 == 1
    assert (_targets(gm), _targets(gm, "call_function")) == MUL_INTO_CAT[on]
    assert len(_of(gm, C.QuantizedConcat)) == ("concats" in on) and not _of(gm, C.QuantizedMul)
    y = gm(x)
    assert len(torch.unique(y)) > 50 and torch.equal(y, gm0(x))


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def check_refusals(lib, native, P=4096):
    """Every refusal of mctq_codes_mul_nhwc: each returns before a launch (the addresses are never dereferenced), so none can
    fault.  ``P``: an aligned address, on the GPU that of a real buffer of at least 4096 bytes."""
    E, I8, U8 = native.MCTQ_E_ARG, native.CODE_I8, native.CODE_U8
    count = lib.mctq_launch_count()
    A, G = P + 1024, P + 2048                             # out at P: [P, P + 4 * 32) reaches neither

    def call(a=A, a_dt=U8, a_scale=0.1, a_zp=0, g=G, g_dt=I8, g_scale=0.2, g_zp=-5, g_f32=0, g_qmin=-128, g_qmax=127, n=0, out=P,
             dt=U8, pixels=4, channels=32, scale=0.05, zp=3, qmin=0, qmax=255):
        return lib.mctq_codes_mul_nhwc(a, a_dt, a_scale, a_zp, g, g_dt, g_scale, g_zp, g_f32, g_qmin, g_qmax, n, out, dt, pixels,
                                       channels, scale, zp, qmin, qmax, None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    refused(b"pixels < 0", pixels=-1)
    for dt in (-1, 2, 3, 77):                            # the 4-bit code types among them
        refused(b"bad a_code_dtype", a_dt=dt)
        refused(b"bad g_code_dtype", g_dt=dt)
        refused(b"bad g_code_dtype", g_dt=dt, g_f32=1, n=1)
        refused(b"bad out_code_dtype", dt=dt)
    for dt, zp in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"a_zero_point is no code of a's type", a_dt=dt, a_zp=zp)
        refused(b"g_zero_point is no code of g's type", g_dt=dt, g_zp=zp)
    refused(b"zero_point is no code of the output's type", zp=256)
    refused(b"zero_point is no code of the output's type", zp=-1)
    refused(b"zero_point is no code of the output's type", dt=I8, qmin=-128, qmax=127, zp=128)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        refused(b"a_scale must be finite and positive", a_scale=bad)
        refused(b"g_scale must be finite and positive", g_scale=bad)
        refused(b"scale must be finite and positive", scale=bad)
    # wrong in two ways: every code type is looked at before any zero point, every zero point before any scale, a before g before out
    refused(b"bad out_code_dtype", dt=77, a_zp=256)
    refused(b"bad a_code_dtype", a_dt=77, g_dt=77)
    refused(b"zero_point is no code of the output's type", zp=256, a_scale=0.0)
    refused(b"a_zero_point is no code of a's type", a_zp=256, g_zp=128)
    refused(b"a_scale must be finite and positive", a_scale=0.0, g_scale=0.0, scale=0.0)
    refused(b"scale must be finite and positive", scale=0.0, qmin=9, qmax=8)
    refused(b"quant_min > quant_max", qmin=9, qmax=8)
    refused(b"clamp domain does not fit the code type", qmax=256)
    refused(b"clamp domain does not fit the code type", dt=I8, qmin=-129, qmax=127)
    refused(b"clamp domain does not fit the code type", dt=I8, qmin=0, qmax=255)
    # G's clamp domain is read for float32 gates only
    refused(b"quant_min > quant_max", g_f32=1, n=2, g_qmin=9, g_qmax=8)
    refused(b"clamp domain does not fit the code type", g_f32=1, n=2, g_qmin=-129)
    refused(b"clamp domain does not fit the code type", g_f32=1, n=2, g_dt=U8, g_zp=5, g_qmin=-1, g_qmax=255)
    refused(b"gate_pixels < 0", n=-1)
    refused(b"a float32 g is taken in the row-broadcast form only (gate_pixels >= 1)", g_f32=1, n=0)
    for channels in (24, 0, -16, 8):
        refused(b"channels must be a positive multiple of 16", channels=channels)
    refused(b"pixels is no multiple of gate_pixels", n=3)
    refused(b"pixels is no multiple of gate_pixels", n=8)
    refused(b"pixels is no multiple of gate_pixels", n=2 ** 40, g_f32=1)
    refused(b"more than 2^31 - 1 16-byte chunks in one launch", pixels=2 ** 30)          # 2^30 pixels of 2 chunks
    refused(b"more than 2^31 - 1 16-byte chunks in one launch", pixels=1, channels=16 * 2 ** 31)
    refused(b"a is NULL", a=None)
    refused(b"g is NULL", g=None)
    refused(b"out is NULL", out=None)
    refused(b"a must be 16-byte aligned", a=A + 8)
    refused(b"g must be 16-byte aligned", g=G + 4)
    refused(b"g must be 16-byte aligned", g=G + 4, g_f32=1, n=4)
    refused(b"out must be 16-byte aligned", out=P + 1)
    # out overlapping an operand: the same address, the operand's last byte, out's last byte; a and g may be one buffer
    refused(b"out overlaps a", a=P)
    refused(b"out overlaps a", a=P - 112)
    refused(b"out overlaps a", a=P + 112)
    refused(b"out overlaps g", g=P)
    refused(b"out overlaps g", g=P - 16, n=4)                # a gate row of 32 bytes
    refused(b"out overlaps g", g=P - 112, n=4, g_f32=1)      # ... of 128 bytes in float32
    refused(b"out overlaps g", g=P + 112, n=2)
    assert call(pixels=0) == 0                                                          # nothing to do: no launch
    assert call(pixels=0, a=None, g=None, out=None) == 0                                # ... and no pointer is looked at
    refused(b"channels must be a positive multiple of 16", pixels=0, channels=24)
    assert lib.mctq_launch_count() == count                                             # refused and empty calls launch nothing


def test_codes_mul_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_codes_mul_nhwc\s*\(", header) and "mctq_codes_mul_nhwc" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    declared = re.search(r"int mctq_codes_mul_nhwc\((.*?)\);", header, flags=re.S).group(1)
    assert len(declared.split(",")) == len(native.SIGNATURES["mctq_codes_mul_nhwc"][1]) == 21
    assert "mctq_codes_mul.hip" in [os.path.basename(s) for s in build.SOURCES]
    assert "mctq_codes_mul_nhwc" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    check_refusals(lib, native)
