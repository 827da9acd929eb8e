"""Channel concatenation on activation codes: host logic and the CPU route (include/mctq_hip.h: mctq_codes_concat_nhwc;
hip/ops.py: codes_concat; consumers.QuantizedConcat and the ``concats`` switch of fuse_linear_consumers_fx).

Everything here is exact, so every check is equality.  A holder's float32 output is ``float(code - zp) * scale`` bit for bit and
``torch.cat`` only moves data, so the codes the holder behind a concatenation gives are the operands' codes requantized one by
one: ``ql_code(join_residual(code - zp_k, scale_k))`` in the output's form.  The op is pinned against that definition written
in numpy float32 and against real holders around ``torch.cat``.

A model rewritten with ``concats=True`` is compared bit for bit with the same rewrite without it and with the model as built.
Without the switch the layers behind the concatenation stay float32 wrappers, so the models are built as those of
tests/test_pool_consumer.py are (its docstring says why): power-of-two activation and weight scales, no bias, sums of at most 288
products -- their float32 products are exact and equal the consumers' integer sums."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_join_consumer import _targets
from test_pool_consumer import _of, pot_conv, signed_pot, unsigned_pot

F = torch.nn.functional

# ---- the op's cases: shared by the CPU and GPU tests --------------------------------------------------------------------------

# (int8?, scale, zero point) of the operands, taken in this order: the first spans both ends of every output form below by
# itself (a concatenation of one operand must reach them too); scales larger (0.05, 0.061, 0.1) and smaller (0.022, 0.009,
# 0.004) than the outputs'; zero points 0, 114 and -5 among them
OPERAND_FORMS = [(True, 0.05, 0), (False, 0.061, 0), (False, 0.022, 114), (True, 0.009, -5), (False, 0.004, 30), (True, 0.027, -5),
                 (False, 0.031, 0), (True, 0.1, 17)]
# (scale, zero point, qmin, qmax): an unsigned and a signed output over the whole type, and a 7-bit domain (no copy operands)
OUT_FORMS = [(0.025, 114, 0, 255), (0.03, -5, -128, 127), (0.025, 20, 0, 127)]
CHANNEL_SETS = [(16, 48, 32), (16,), (16,) * 8, (32, 16)]
# 30 and 126 pixels: with 96 channels the second is 756 chunks, three 256-lane blocks, the last one partly filled
LEADS = [(2, 3, 5), (2, 7, 9)]


def concat_reference(operands, out_form):
    """The definition in numpy float32: operands [(codes [.., C_k], scale, zero point)] -> codes [.., sum C_k]."""
    scale, zp, qmin, qmax = out_form
    f32 = np.float32
    inv = f32(1.0) / f32(scale)
    parts = []
    for codes, s, z in operands:
        v = (codes.astype(np.int32) - np.int32(z)).astype(f32) * f32(s)                # the operand holder's float32 output
        q = np.rint(v * inv).astype(f32) + f32(zp)
        parts.append(np.clip(q, f32(qmin), f32(qmax)).astype(np.int32))
    out = np.concatenate(parts, axis=-1)
    return out.astype(np.uint8 if qmin >= 0 else np.int8)


@functools.lru_cache(maxsize=None)
def concat_case(channels, lead, out_index):
    """(operands [(codes, scale, zero point)], out_form, the reference's result), computed once and shared; read-only.  The
    last operand of the two-operand set has the output's own form where that is a whole type: a copy operand next to one that
    runs the arithmetic."""
    out_form = OUT_FORMS[out_index]
    rng = np.random.default_rng(1000 * len(channels) + 10 * lead[1] + out_index)
    operands = []
    for k, c in enumerate(channels):
        signed, s, z = OPERAND_FORMS[k]
        if channels == (32, 16) and k == 1 and out_form[3] - out_form[2] == 255:
            signed, s, z = out_form[2] < 0, out_form[0], out_form[1]
        codes = rng.integers(-128, 128, lead + (c,)).astype(np.int8) if signed else rng.integers(0, 256, lead + (c,)).astype(np.uint8)
        codes.setflags(write=False)
        operands.append((codes, s, z))
    want = concat_reference(operands, out_form)
    want.setflags(write=False)
    # both ends of the output clamp are reached, by values beyond them
    assert want.min() == out_form[2] and want.max() == out_form[3], (channels, lead, out_index)
    return tuple(operands), out_form, want


def concat_cases():
    for channels in CHANNEL_SETS:
        for lead in LEADS:
            for out_index in range(len(OUT_FORMS)):
                yield channels, lead, out_index


def as_tensors(operands, device="cpu"):
    return [(torch.from_numpy(c.copy()).to(device), s, z) for c, s, z in operands]


def all_codes(signed):
    """Every code of the type once, as [16, 16] codes (one 16-byte chunk per pixel)."""
    return (np.arange(-128, 128).astype(np.int8) if signed else np.arange(256).astype(np.uint8)).reshape(16, 16)


# forms whose own codes must come back unchanged: both types, zero points at the ends and inside, scales that are powers of two
# and that are not, tiny and large
IDENTITY_FORMS = [(False, 0.025, 114), (False, 1.0 / 64, 0), (False, 3.7e-5, 255), (False, 812.3, 7), (True, 0.03, -5),
                  (True, 0.5, -128), (True, 6.1e-4, 127), (True, 97.0, 0)]


def test_reference_cases_cover_what_they_should():
    n = sum(1 for _ in concat_cases())
    assert n == 4 * 2 * 3
    for channels, lead, out_index in concat_cases():
        operands, out_form, want = concat_case(channels, lead, out_index)
        assert want.shape == lead + (sum(channels),) and len(operands) == len(channels)
    kinds = {(c.dtype.name, z) for c, _, z in concat_case((16,) * 8, LEADS[0], 0)[0]}
    assert {("int8", 0), ("uint8", 114), ("int8", -5)} <= kinds
    ops_, out_form, _ = concat_case((32, 16), LEADS[0], 1)
    assert (ops_[1][1], ops_[1][2]) == out_form[:2] and ops_[1][0].dtype == np.int8          # the copy operand


# ---- the op ----------------------------------------------------------------------------------------------------------------

def test_codes_concat_on_cpu_equals_the_reference():
    from mct_quantizers_amd.hip import ops
    for channels, lead, out_index in concat_cases():
        operands, out_form, want = concat_case(channels, lead, out_index)
        got = ops.codes_concat(as_tensors(operands), out_form)
        assert got.dtype == (torch.uint8 if out_form[2] >= 0 else torch.int8) and got.is_contiguous()
        assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want), (channels, lead, out_index)
    # channel counts that are no multiple of 16, and more than eight operands: the same definition
    rng = np.random.default_rng(5)
    odd = [(rng.integers(0, 256, (3, 5, c)).astype(np.uint8), 0.02 + 0.01 * i, 3 * i) for i, c in enumerate((24, 7, 1))]
    assert np.array_equal(ops.codes_concat(as_tensors(odd), OUT_FORMS[1]).numpy(), concat_reference(odd, OUT_FORMS[1]))
    nine = [(rng.integers(-128, 128, (4, 16)).astype(np.int8), 0.01 * (i + 1), i - 4) for i in range(9)]
    assert np.array_equal(ops.codes_concat(as_tensors(nine), OUT_FORMS[0]).numpy(), concat_reference(nine, OUT_FORMS[0]))
    # a non-contiguous operand, and an empty batch
    x = torch.from_numpy(odd[0][0].copy())
    assert torch.equal(ops.codes_concat([(x.permute(1, 0, 2), 0.02, 0)], OUT_FORMS[0]),
                       ops.codes_concat([(x.permute(1, 0, 2).contiguous(), 0.02, 0)], OUT_FORMS[0]))
    empty = ops.codes_concat([(torch.zeros(0, 4, 16, dtype=torch.uint8), 0.1, 0), (torch.zeros(0, 4, 32, dtype=torch.int8), 0.1, 0)], OUT_FORMS[1])
    assert empty.shape == (0, 4, 48) and empty.dtype == torch.int8


def test_codes_concat_validation():
    from mct_quantizers_amd.hip import ops
    u8 = torch.zeros(2, 3, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at least one operand"):
        ops.codes_concat([], OUT_FORMS[0])
    with pytest.raises(TypeError):
        ops.codes_concat([(u8.float(), 0.1, 0)], OUT_FORMS[0])
    with pytest.raises(RuntimeError, match="leading shape"):
        ops.codes_concat([(u8, 0.1, 0), (u8[:1], 0.1, 0)], OUT_FORMS[0])
    with pytest.raises(ValueError, match="zero point"):
        ops.codes_concat([(u8, 0.1, -1)], OUT_FORMS[0])
    with pytest.raises(ValueError, match="zero point"):
        ops.codes_concat([(u8.to(torch.int8), 0.1, 128)], OUT_FORMS[0])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            ops.codes_concat([(u8, bad, 0)], OUT_FORMS[0])
        with pytest.raises(ValueError, match="scale"):
            ops.codes_concat([(u8, 0.1, 0)], (bad, 0, 0, 255))
    with pytest.raises(ValueError, match="8-bit code"):
        ops.codes_concat([(u8, 0.1, 0)], (0.1, 0, -1, 255))


def holder_of(kind):
    """Real holders: "u4" / "u8" unsigned symmetric (threshold 4 / 8), "s" signed symmetric with a scale that is no power of two,
    "uni" uniform with zero point 64 and scale 1 / 64."""
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Q = mq.pytorch_quantizers
        q = {"u4": lambda: unsigned_pot(4.0), "u8": lambda: unsigned_pot(8.0), "u2": lambda: unsigned_pot(2.0),
             "s4": lambda: signed_pot(4.0),
             "s": lambda: Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[3.7], signed=True),
             "uni": lambda: Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-1.0], max_range=[-1.0 + 255.0 / 64])}[kind]()
        return mq.PytorchActivationQuantizationHolder(q)


def _form(holder):
    from mct_quantizers_amd import consumers
    return consumers._activation_code_params(holder.activation_holder_quantizer)


def test_uniform_test_holder_has_a_power_of_two_scale():
    assert _form(holder_of("uni")) == (1.0 / 64, 64, 0, 255) and _form(holder_of("s"))[1:] == (0, -128, 127)


@pytest.mark.parametrize("out_kind", ["s", "uni", "u4"])
def test_codes_concat_gives_the_codes_of_the_holder_behind_torch_cat(out_kind):
    from mct_quantizers_amd.hip import ops
    g = torch.Generator().manual_seed(11)
    kinds, channels = ("s", "uni", "u4"), (16, 8, 24)
    holders, hc = [holder_of(k) for k in kinds], holder_of(out_kind)
    xs = [torch.randn(2, c, 5, 3, generator=g) * 3.0 for c in channels]
    with torch.no_grad():
        chain = hc(torch.cat([h(x) for h, x in zip(holders, xs)], 1))                   # float32, what the model as built computes
    s, z, qmin, qmax = _form(hc)
    want = ops.fq_codes_nhwc(chain, qmin, qmax, s, z)
    operands = []
    for h, x in zip(holders, xs):
        hs, hz, hmin, hmax = _form(h)
        operands.append((ops.fq_codes_nhwc(x, hmin, hmax, hs, hz), hs, hz))
    got = ops.codes_concat(operands, (s, z, qmin, qmax))
    assert torch.equal(got, want) and len(torch.unique(got)) > 50
    assert torch.equal(ops.dequantize_codes(got, s, z).permute(0, 3, 1, 2), chain)       # ... and they stand for that tensor


def test_every_code_comes_back_through_a_copy_form_operand():
    from mct_quantizers_amd.hip import ops
    for signed, s, z in IDENTITY_FORMS:
        codes = torch.from_numpy(all_codes(signed).copy())
        out_form = (s, z, -128, 127) if signed else (s, z, 0, 255)
        assert torch.equal(ops.codes_concat([(codes, s, z)], out_form), codes), (signed, s, z)
        assert np.array_equal(concat_reference([(codes.numpy(), s, z)], out_form), codes.numpy())


# ---- the module ------------------------------------------------------------------------------------------------------------

def check_concat_module(device):
    """QuantizedConcat on float32 operands, on codes and on a mix, on holder inputs and holder outputs, 4-D and rows, against the
    holders around torch.cat; returns the outputs."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    outs = []
    for kinds, out_kind, channels in ((("u4", "s", "uni"), "uni", (16, 32, 16)), (("s", "u8"), "s4", (16, 16)), (("uni", "u4"), "u4", (8, 24))):
        holders, hc = [holder_of(k) for k in kinds], holder_of(out_kind)
        qc = consumers.QuantizedConcat([h.activation_holder_quantizer for h in holders], hc.activation_holder_quantizer)
        assert qc.activation_code_params() == _form(hc) and [qc.operand_code_params(i) for i in range(len(kinds))] == [_form(h) for h in holders]
        s, z, qmin, qmax = _form(hc)
        g = torch.Generator().manual_seed(21)
        xs = [(torch.randn(2, c, 5, 3, generator=g) * 3.0).to(device) for c in channels]
        with torch.no_grad():
            want = hc(torch.cat([h(x.cpu()) for h, x in zip(holders, xs)], 1))
        y = qc(*xs)
        assert y.dtype == ops._code_dtype(qmin, qmax)[0] and y.shape == (2, sum(channels), 5, 3)
        assert y.is_contiguous(memory_format=torch.channels_last)                       # NCHW-shaped, NHWC-stored
        assert torch.equal(ops.dequantize_codes(y.cpu(), s, z), want)
        codes = [ops.fq_codes_nhwc(x, *_form(h)[2:], *_form(h)[:2]).permute(0, 3, 1, 2) for h, x in zip(holders, xs)]
        assert torch.equal(qc(*codes), y)                                               # codes in
        assert torch.equal(qc(codes[0], *xs[1:]), y)                                    # a mix
        assert torch.equal(qc(*[x.contiguous(memory_format=torch.channels_last) for x in xs]), y)
        with torch.no_grad():
            assert torch.equal(qc(*[h(x.cpu()).to(device) for h, x in zip(holders, xs)]), y)   # the holders' outputs: the same codes
        rows = [x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs]               # [M, C] rows
        y2 = qc(*rows)
        assert y2.shape == (30, sum(channels)) and torch.equal(y2, y.permute(0, 2, 3, 1).reshape(30, -1))
        assert torch.equal(qc(*[c.permute(0, 2, 3, 1).reshape(30, -1) for c in codes]), y2)
        wrong = torch.int8 if codes[0].dtype == torch.uint8 else torch.uint8
        with pytest.raises(TypeError):
            qc(codes[0].to(wrong), *xs[1:])
        with pytest.raises(TypeError):
            qc(xs[0].double(), *xs[1:])
        with pytest.raises(RuntimeError):
            qc(*xs[:-1])                                                                # an operand short
        with pytest.raises(RuntimeError):
            qc(xs[0][:1], *xs[1:])                                                      # another batch
        with pytest.raises(RuntimeError):
            qc(xs[0][:, :, :4], *xs[1:])                                                # another height
        with pytest.raises(RuntimeError):
            qc(rows[0], *xs[1:])                                                        # another rank
        with pytest.raises(RuntimeError):
            qc(*[x[0] for x in xs])                                                     # 3-D
        outs += [y.cpu(), y2.cpu()]
    return outs


def test_quantized_concat_on_cpu():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    assert len(check_concat_module("cpu")) == 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=16, threshold=[4.0], signed=True)
        lut = mq.pytorch_quantizers.ActivationLutPOTInferableQuantizer(num_bits=4, lut_values=[0.0, 32.0, 64.0, 96.0], threshold=[4.0],
                                                                       signed=False, lut_values_bitwidth=8)
    ok = unsigned_pot()
    with pytest.raises(NotImplementedError):
        consumers.QuantizedConcat([ok, wide], ok)
    with pytest.raises(NotImplementedError):
        consumers.QuantizedConcat([ok, ok], wide)
    with pytest.raises(TypeError):
        consumers.QuantizedConcat([ok, lut], ok)
    with pytest.raises(ValueError):
        consumers.QuantizedConcat([], ok)


# ---- the rewrite -----------------------------------------------------------------------------------------------------------

class Fire(torch.nn.Module):
    """SqueezeNet's Fire module: 1x1 squeeze -> ReLU -> holder -> {1x1, 3x3 expand} -> ReLU -> holders -> cat -> holder -> 1x1.
    The 3x3 branch's holder is signed, so that the ReLU in front of it is a real narrowing of its codes."""

    def __init__(self, e1=16, e3=32):
        super().__init__()
        self.h0 = holder_of("s4")
        self.squeeze = pot_conv(16, 16, 1, 1)
        self.h1 = holder_of("u4")
        self.e1, self.e3 = pot_conv(16, e1, 1, 2), pot_conv(16, e3, 3, 3)
        self.h_e1, self.h_e3 = holder_of("u8"), holder_of("s4")
        self.hc = holder_of("u4")
        self.last = pot_conv(e1 + e3, 16, 1, 4)

    def forward(self, x):
        s = self.h1(torch.relu(self.squeeze(self.h0(x))))
        a = self.h_e1(torch.relu(self.e1(s)))
        b = self.h_e3(torch.relu(self.e3(s)))
        return self.last(self.hc(torch.cat([a, b], 1)))


class Inception(torch.nn.Module):
    """An Inception-style block: three branches (1x1; 1x1 -> 3x3; 1x1 behind a holder with a zero point) -> cat -> holder, which
    feeds two 1x1 convolutions and a MaxPool2d(3, 1, 1) in front of a third.  The first branch's holder has the form of the
    concatenation's holder: a copy operand."""

    def __init__(self):
        super().__init__()
        self.h0 = holder_of("s4")
        self.b1, self.b2a, self.b2b, self.b3 = pot_conv(16, 16, 1, 1), pot_conv(16, 16, 1, 2), pot_conv(16, 32, 3, 3), pot_conv(16, 16, 1, 4)
        self.h1, self.h2a, self.h2b, self.h3 = holder_of("u4"), holder_of("u4"), holder_of("u8"), holder_of("uni")
        self.hc = holder_of("u4")
        self.pool = torch.nn.MaxPool2d(3, 1, 1)
        self.c1, self.c2, self.c3 = pot_conv(64, 16, 1, 5), pot_conv(64, 16, 1, 6), pot_conv(64, 16, 1, 7)

    def forward(self, x):
        x = self.h0(x)
        a = self.h1(F.relu(self.b1(x)))
        b = self.h2b(F.relu(self.b2b(self.h2a(F.relu(self.b2a(x))))))
        c = self.h3(F.relu(self.b3(x)))
        t = self.hc(torch.cat((a, b, c), dim=1))
        return self.c1(t) + self.c2(t) + self.c3(self.pool(t))


def block_input(device="cpu"):
    return (torch.randn(2, 16, 7, 5, generator=torch.Generator().manual_seed(12)) * 1.5).to(device)


ALL = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True)


def rewritten(make, device="cpu", concats=True, **switches):
    from mct_quantizers_amd import consumers
    return consumers.fuse_linear_consumers_fx(make().to(device).eval(), concats=concats, **(switches or ALL))


def test_fire_module_runs_codes_to_codes():
    from mct_quantizers_amd import consumers as C
    x = block_input()
    with torch.no_grad():
        want = Fire().eval()(x)
    gm, n = rewritten(Fire)
    gm0, n0 = rewritten(Fire, concats=False)
    assert (n, n0) == (4, 4)
    y = gm(x)
    assert y.shape == (2, 16, 7, 5) and len(torch.unique(y)) > 50
    assert torch.equal(y, gm0(x)) and torch.equal(y, want)
    # the cat, its holder and both operand holders are gone; the ReLUs were folded into the branch consumers
    assert _targets(gm) == ["squeeze_qlinear", "e1_qlinear", "e3_qlinear", "hc_concat", "last_qlinear"]
    assert not _targets(gm, "call_function") and not _targets(gm, "call_method")
    assert torch.cat in _targets(gm0, "call_function") and not _of(gm0, C.QuantizedConcat)
    concat = gm.get_submodule("hc_concat")
    e1, e3 = gm.get_submodule("e1_qlinear"), gm.get_submodule("e3_qlinear")
    assert e1.emit_codes_for == concat.operand_code_params(0) == (8.0 / 256, 0, 0, 255) and e1.emit_clamp is None
    assert e3.emit_codes_for == concat.operand_code_params(1) == (4.0 / 128, 0, -128, 127) and e3.emit_clamp == (0, 127)
    assert concat.activation_code_params() == gm.get_submodule("last_qlinear").activation_code_params() == (4.0 / 256, 0, 0, 255)
    assert gm.get_submodule("last_qlinear").emit_codes_for is None
    seen = []
    hook = concat.register_forward_hook(lambda m, args, out: seen.append(([a.dtype for a in args], out.dtype)))
    gm(x)
    hook.remove()
    assert seen == [([torch.uint8, torch.int8], torch.uint8)]
    # without stay_on_codes the ReLUs stay and the concat quantizes their float32 outputs
    gm1, n1 = rewritten(Fire, convolutions=True, shared_holders=True)
    assert n1 == 4 and _targets(gm1) == ["squeeze_qlinear", "h1_join", "e1_qlinear", "e3_qlinear", "hc_concat", "last_qlinear"]
    assert _targets(gm1, "call_function").count(torch.relu) == 2 and torch.equal(gm1(x), want)
    # concats alone: the concat and the layer behind it, nothing else needs a switch
    gm2, n2 = rewritten(Fire, concats=True, convolutions=False)
    assert n2 == 2 and "hc_concat" in _targets(gm2) and "last_qlinear" in _targets(gm2) and torch.equal(gm2(x), want)
    # tracing the rewritten graph again keeps the concat a leaf and replaces nothing more
    again, n = rewritten(lambda: gm)
    assert n == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), y)


def test_inception_block_runs_codes_to_codes():
    from mct_quantizers_amd import consumers as C
    x = block_input()
    with torch.no_grad():
        want = Inception().eval()(x)
    gm, n = rewritten(Inception)
    gm0, n0 = rewritten(Inception, concats=False)
    assert (n, n0) == (7, 7)
    y = gm(x)
    assert y.shape == (2, 16, 7, 5) and len(torch.unique(y)) > 50
    assert torch.equal(y, gm0(x)) and torch.equal(y, want)
    targets = _targets(gm)
    assert "hc_concat" in targets and "pool_qpool" in targets and not [t for t in targets if t in ("hc", "h1", "h2b", "h3", "pool")]
    assert torch.cat not in _targets(gm, "call_function") and F.relu not in _targets(gm, "call_function")
    assert len(_of(gm, C.QuantizedConcat)) == 1 and not _of(gm0, C.QuantizedConcat)
    concat, nodes = gm.get_submodule("hc_concat"), {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert [a.target for a in nodes["hc_concat"].args] == ["b1_qlinear", "b2b_qlinear", "b3_qlinear"]
    assert sorted(u.target for u in nodes["hc_concat"].users) == ["c1_qlinear", "c2_qlinear", "pool_qpool"]
    assert [u.target for u in nodes["pool_qpool"].users] == ["c3_qlinear"]
    for i, (name, form, clamp) in enumerate((("b1_qlinear", (4.0 / 256, 0, 0, 255), None), ("b2b_qlinear", (8.0 / 256, 0, 0, 255), None),
                                             ("b3_qlinear", (1.0 / 64, 64, 0, 255), (64, 255)))):
        m = gm.get_submodule(name)
        assert m.emit_codes_for == concat.operand_code_params(i) == form and m.emit_clamp == clamp, name
    assert concat.activation_code_params() == gm.get_submodule("pool_qpool").activation_code_params() == (4.0 / 256, 0, 0, 255)
    # without pools the block's max pool is a float32 user of the concatenation's holder: left alone
    gm1, n1 = rewritten(Inception, convolutions=True, shared_holders=True, stay_on_codes=True)
    gm10, n10 = rewritten(Inception, concats=False, convolutions=True, shared_holders=True, stay_on_codes=True)
    assert n1 == n10 and not _of(gm1, C.QuantizedConcat) and str(gm1.graph) == str(gm10.graph) and torch.equal(gm1(x), want)


class Skip(torch.nn.Module):
    """A decoder stage with a skip connection: the first operand's holder also feeds a wrapped convolution and a float32 add."""

    def __init__(self):
        super().__init__()
        self.h0 = holder_of("s4")
        self.a, self.b = pot_conv(16, 16, 1, 1), pot_conv(16, 16, 3, 2)
        self.h_a, self.h_b, self.hc = holder_of("u4"), holder_of("u8"), holder_of("u4")
        self.last = pot_conv(32, 16, 1, 3)

    def forward(self, x):
        a = self.h_a(torch.relu(self.a(self.h0(x))))
        b = self.h_b(torch.relu(self.b(a)))
        return self.last(self.hc(torch.cat([a, b], 1))) + a


def test_a_skip_connection_keeps_its_holder():
    from mct_quantizers_amd import consumers as C
    import mct_quantizers_amd as mq
    x = block_input()
    with torch.no_grad():
        want = Skip().eval()(x)
    # without shared_holders h_a, with three users, stays a holder; the concat reads its float32 output
    gm, n = rewritten(Skip, convolutions=True)
    gm0, n0 = rewritten(Skip, concats=False, convolutions=True)
    assert (n, n0) == (2, 2)                             # a and last (b sits behind the shared holder) / a and last
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert isinstance(gm.get_submodule("h_a"), mq.PytorchActivationQuantizationHolder) and "h_a" in nodes and "h_b" not in nodes
    assert nodes["hc_concat"].args[0] is nodes["h_a"] and nodes["hc_concat"].args[1].target is torch.relu
    assert torch.equal(gm(x), want) and torch.equal(gm0(x), want)
    # with every switch it becomes a join that still writes float32 (for the add); the concat reads that output
    gm, n = rewritten(Skip)
    gm0, n0 = rewritten(Skip, concats=False)
    assert (n, n0) == (3, 3)
    join = gm.get_submodule("h_a_join")
    assert isinstance(join, C.QuantizedJoin) and join.want_float and join.relu
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    first, second = nodes["hc_concat"].args
    assert first.op == "call_function" and first.args == (nodes["h_a_join"], 0) and second is nodes["b_qlinear"]
    assert gm.get_submodule("b_qlinear").emit_codes_for == gm.get_submodule("hc_concat").operand_code_params(1)
    y = gm(x)
    assert torch.equal(y, want) and torch.equal(gm0(x), want) and len(torch.unique(y)) > 50


class Odd(torch.nn.Module):
    """What the switch leaves alone, one at a time."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        count = 9 if kind == "nine" else 2
        self.hs = torch.nn.ModuleList([holder_of("u4") for _ in range(count)])
        self.hc = holder_of("u8")
        self.last = pot_conv(16 if kind == "dim0" else 16 * count, 16, 1, 1)

    def forward(self, x):
        parts = [h(x) for h in self.hs]
        if self.kind == "operand":
            parts[1] = torch.relu(parts[1])              # an operand that is no holder's output
        if self.kind == "clamp":
            t = self.hc(torch.relu(torch.cat(parts, 1)))
        elif self.kind == "dim0":
            t = self.hc(torch.cat(parts, 0))
        elif self.kind == "keyword0":
            t = self.hc(torch.cat(parts, dim=-3))        # the same axis, not written as the constant 1
        elif self.kind == "shared_cat":
            c = torch.cat(parts, 1)
            return self.last(self.hc(c)) + c[:, :16]
        else:
            t = self.hc(torch.cat(parts, 1))
        y = self.last(t)
        return y + t[:, :16] if self.kind == "float_user" else y


@pytest.mark.parametrize("kind", ["dim0", "float_user", "operand", "nine", "clamp", "keyword0", "shared_cat"])
def test_what_the_switch_leaves_alone(kind):
    from mct_quantizers_amd import consumers as C
    x = block_input()
    for switches in (dict(), dict(convolutions=True, shared_holders=True), ALL):
        gm, n = C.fuse_linear_consumers_fx(Odd(kind).eval(), concats=True, **switches)
        gm0, n0 = C.fuse_linear_consumers_fx(Odd(kind).eval(), **switches)
        assert n == n0 and not _of(gm, C.QuantizedConcat), (kind, switches)
        assert str(gm.graph) == str(gm0.graph) and gm.code == gm0.code
        assert torch.cat in _targets(gm, "call_function") and torch.equal(gm(x), gm0(x))


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers as C
    for switches in (dict(), dict(convolutions=True), dict(convolutions=True, shared_holders=True), ALL):
        for make in (Fire, Inception, Skip):
            gm, n = C.fuse_linear_consumers_fx(make().eval(), **switches)
            gm_off, n_off = C.fuse_linear_consumers_fx(make().eval(), concats=False, **switches)
            assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
            assert not _of(gm, C.QuantizedConcat)


def test_channel_counts_that_are_no_multiple_of_16():
    from mct_quantizers_amd import consumers as C
    x = block_input()
    make = lambda: Fire(8, 24)                           # noqa: E731  (8 + 24 = 32 channels into the last convolution)
    with torch.no_grad():
        want = make().eval()(x)
    gm, n = rewritten(make)
    gm0, n0 = rewritten(make, concats=False)
    assert (n, n0) == (4, 4) and len(_of(gm, C.QuantizedConcat)) == 1
    y = gm(x)
    assert torch.equal(y, gm0(x)) and torch.equal(y, want) and len(torch.unique(y)) > 50


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------

def check_refusals(lib, native, P=4096):
    """Every refusal of mctq_codes_concat_nhwc: each returns before a launch (the addresses are never dereferenced), so none can
    fault.  ``P``: an aligned address, on the GPU that of a real buffer of at least 2 * 64 * 16 bytes."""
    E, I8, U8 = native.MCTQ_E_ARG, native.CODE_I8, native.CODE_U8
    count = lib.mctq_launch_count()
    Q = P + 1024                                          # the operands' address; out at P: [P, P + 2 * 32) does not reach it

    def call(items=((Q, 16, U8, 0, 0.1), (Q, 16, I8, -5, 0.2)), n=None, out=P, dt=U8, pixels=2, scale=0.05, zp=3, qmin=0, qmax=255):
        arr = (native.ConcatItem * max(len(items), 1))()
        for it, (codes, channels, code_dtype, zero_point, s) in zip(arr, items):
            it.codes, it.channels, it.code_dtype, it.zero_point, it.scale = codes, channels, code_dtype, zero_point, s
        return lib.mctq_codes_concat_nhwc(arr, len(items) if n is None else n, out, dt, pixels, scale, zp, qmin, qmax, None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    one = (Q, 16, U8, 0, 0.1)
    refused(b"count must be 1 .. 8", items=())
    refused(b"count must be 1 .. 8", items=(one,) * 9)
    refused(b"count must be 1 .. 8", n=-1)
    assert lib.mctq_codes_concat_nhwc(None, 1, P, U8, 2, 0.05, 3, 0, 255, None) == E and lib.mctq_last_error() == b"items is NULL"
    refused(b"pixels < 0", pixels=-1)
    for channels in (24, 0, -16, 8):
        refused(b"an operand's channels must be a positive multiple of 16", items=(one, (Q, channels, U8, 0, 0.1)))
    refused(b"an operand's codes must be 16-byte aligned", items=((Q + 8, 16, U8, 0, 0.1),))
    refused(b"an operand's codes pointer is NULL", items=(one, (None, 16, U8, 0, 0.1)))
    refused(b"out must be 16-byte aligned", out=P + 4)
    refused(b"out is NULL", out=None)
    for dt in (-1, 2, 3, 77):                            # the 4-bit code types among them
        refused(b"bad code_dtype of an operand", items=((Q, 16, dt, 0, 0.1),))
        refused(b"bad out_code_dtype", dt=dt)
    for dt, zp in ((U8, -1), (U8, 256), (I8, -129), (I8, 128)):
        refused(b"an operand's zero_point is no code of its type", items=((Q, 16, dt, zp, 0.1),))
    refused(b"zero_point is no code of the output's type", zp=256)
    refused(b"zero_point is no code of the output's type", zp=-1)
    refused(b"zero_point is no code of the output's type", dt=I8, qmin=-128, qmax=127, zp=128)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        refused(b"an operand's scale must be finite and positive", items=(one, (Q, 16, U8, 0, bad)))
        refused(b"scale must be finite and positive", scale=bad)
    # wrong in two ways: the output's scale, its code type, its clamp domain, its zero point, then the operands in their order,
    # of each the code type, the zero point, the scale
    refused(b"scale must be finite and positive", scale=0.0, dt=77)
    refused(b"bad out_code_dtype", dt=77, qmin=9, qmax=8)
    refused(b"quant_min > quant_max", qmin=9, qmax=8, zp=256)
    refused(b"zero_point is no code of the output's type", zp=256, items=((Q, 16, 77, 0, 0.1),))
    refused(b"an operand's zero_point is no code of its type", items=((Q, 16, U8, 256, 0.0),))
    refused(b"an operand's scale must be finite and positive", items=((Q, 16, U8, 0, 0.0), (Q, 16, 77, 0, 0.1)))
    refused(b"an operand's scale must be finite and positive", items=((Q, 24, U8, 0, 0.0),))
    refused(b"quant_min > quant_max", qmin=9, qmax=8)
    refused(b"clamp domain does not fit the code type", qmax=256)
    refused(b"clamp domain does not fit the code type", dt=I8, qmin=-129, qmax=127)
    refused(b"clamp domain does not fit the code type", dt=I8, qmin=0, qmax=255)
    refused(b"more than 2^31 - 1 16-byte chunks in one launch", pixels=2 ** 30)          # 2^30 pixels of 2 chunks
    refused(b"more than 2^31 - 1 16-byte chunks in one launch", items=((Q, 16 * (2 ** 31 - 1), U8, 0, 0.1), one))
    # out overlapping an operand: the same address, the operand's last byte, out's last byte
    refused(b"out overlaps an operand", items=((P, 16, U8, 0, 0.1),))
    refused(b"out overlaps an operand", items=(one, (P - 16, 16, U8, 0, 0.1)))
    refused(b"out overlaps an operand", items=(one, (P + 48, 16, U8, 0, 0.1)))
    assert call(pixels=0) == 0                                                          # nothing to do: no launch
    assert call(pixels=0, out=None, items=((None, 16, U8, 0, 0.1),)) == 0               # ... and no pointer is looked at
    refused(b"an operand's channels must be a positive multiple of 16", pixels=0, items=((Q, 24, U8, 0, 0.1),))
    for value in (2, -1):
        assert lib.mctq_set_tuning(b"concat_copy", value) == E and lib.mctq_last_error() == b"concat_copy must be 0 or 1"
    assert lib.mctq_launch_count() == count                                             # refused and empty calls launch nothing


def test_codes_concat_argument_validation_needs_no_gpu():
    import ctypes
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_codes_concat_nhwc\s*\(", header) and "mctq_codes_concat_nhwc" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    # the ctypes structure has the C structure's layout: 8 + 8 + 4 + 4 + 4 bytes, padded to 32
    assert ctypes.sizeof(native.ConcatItem) == 32 and native.ConcatItem.scale.offset == 24
    m = re.search(r"typedef struct mctq_concat_item \{(.*?)\} mctq_concat_item;", header, flags=re.S)
    assert m and re.findall(r"(\w+);", m.group(1)) == [name for name, _ in native.ConcatItem._fields_]
    assert "mctq_codes_concat.hip" in [os.path.basename(s) for s in build.SOURCES]
    assert "mctq_codes_concat_nhwc" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    check_refusals(lib, native)
