"""Activations that stay on codes between integer consumers: host logic and the CPU route (include/mctq_hip.h:
mctq_fq_join_rc_f32; hip/ops.py: fq_join(residual_codes=...); consumers.folded_clamp, QuantizedJoin(residual_codes=...) and the
``stay_on_codes`` switch of fuse_linear_consumers_fx).

Both steps are exact, so every check is bit equality:

* the clamp fold -- ``fq_codes(clamp(v, a, b))`` against ``fq_codes(v)`` clamped to ``folded_clamp(form, a, b)`` -- because the
  code function is monotone non-decreasing in v (NaN is the documented exception, asserted apart);
* the dequantized residual -- a join given another join's codes against the same join given that join's float32 output.

A rewritten model is compared with the same model under ``shared_holders=True`` alone, which tests/test_join_consumer.py pins
against its private-holders twin."""
import functools
import math
import operator
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES, activation_quantizer, conv_pair, weights_quantizer
from test_dw_consumer import InvertedResidual
from test_join_consumer import FORMS, ResidualStack, _Block, _holder, _targets, join_case, ties

F32 = np.float32
F = torch.nn.functional
OUTPUTS = [(True, True), (True, False), (False, True)]                 # (want_float, want_codes)
N_JOIN = 4096 * 3 + 16 * 5 + 7
# both FORMS entries, 8/256 and 6/255 unsigned (what follows a ReLU / a ReLU6), signed with zp = -128, a zero point outside the domain
FOLD_FORMS = {"u8": FORMS["u8"], "i8": FORMS["i8"], "8/256": (8.0 / 256, 0, 0, 255), "6/255": (6.0 / 255, 0, 0, 255),
              "zp-128": (0.02, -128, -128, 127), "zp outside": (0.05, 300, 0, 255)}
RANGES = [(0.0, math.inf), (0.0, 6.0), (-1.0, 1.0), (-2.5, 3.1), (0.0, 0.0)]
# the residual's form differs from either output form
R_FORMS = {torch.int8: (0.23, -7), torch.uint8: (0.19, 101)}


def clamp_activation(v, a, b):
    if (a, b) == (0.0, math.inf):
        return torch.relu(v)
    if (a, b) == (0.0, 6.0):
        return F.relu6(v)
    return F.hardtanh(v, a, b)


def fold_values(form, a, b, n=40_000):
    scale, zp, qmin, qmax = form
    rng = np.random.default_rng(1000 + int(1000 * scale) + zp + int(10 * a))
    lo, hi = (qmin - 40 - zp) * scale, (qmax + 40 - zp) * scale
    ends = [e for e in (a, b) if math.isfinite(e)]
    parts = [rng.uniform(lo, hi, n), rng.uniform(min(ends) - 2.0, max(ends) + 2.0, n), rng.uniform(-0.5, 0.5, n // 4) * scale * 8]
    edge = [0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45, np.inf, -np.inf, 3e38, -3e38, a, b if math.isfinite(b) else 0.0]
    for e in ends:
        edge += [np.nextafter(F32(e), F32(np.inf)), np.nextafter(F32(e), F32(-np.inf))]
    v = np.concatenate([np.concatenate(parts).astype(F32), np.array(edge, dtype=F32), np.array(ties(scale), dtype=F32)])
    assert not np.isnan(v).any()
    return torch.from_numpy(v)


# ---- the two identities --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FOLD_FORMS))
def test_a_clamp_in_front_of_the_quantizer_is_a_narrower_clamp_of_the_codes(name):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    form = FOLD_FORMS[name]
    scale, zp, qmin, qmax = form
    narrowed = 0
    for a, b in RANGES:
        v = fold_values(form, a, b)
        lo, hi = consumers.folded_clamp(form, a, b)
        assert qmin <= lo <= hi <= qmax
        want = ops.fq_codes(clamp_activation(v, a, b), None, None, None, qmin, qmax, scale, zp)
        got = ops.fq_codes(v, None, None, None, lo, hi, scale, zp).to(want.dtype)
        assert torch.equal(got, want), (name, a, b, int((got != want).sum()), v[got != want][:4])
        assert int(want.min()) == lo and int(want.max()) == hi               # values past both ends of the range were there
        # the ends are the codes of a and b themselves, in the library's own arithmetic
        ends = ops.fq_codes(torch.tensor([a, min(b, 3e38)], dtype=torch.float32), None, None, None, qmin, qmax, scale, zp)
        assert (lo, hi) == (int(ends[0]), int(ends[1]) if math.isfinite(b) else qmax)
        narrowed += (lo, hi) != (qmin, qmax)
    assert narrowed >= 3
    with pytest.raises(ValueError):
        consumers.folded_clamp(form, 1.0, -1.0)


def test_the_documented_nan_difference():
    """torch.relu keeps a NaN, which then codes to qmin; the narrowed clamp sends it to its own lower end."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    scale, zp, qmin, qmax = form = FORMS["u8"]
    lo, hi = consumers.folded_clamp(form, 0.0, math.inf)
    assert (lo, hi) == (zp, qmax) and lo != qmin
    nan = torch.tensor([float("nan")])
    assert int(ops.fq_codes(torch.relu(nan), None, None, None, qmin, qmax, scale, zp)) == qmin
    assert int(ops.fq_codes(nan, None, None, None, lo, hi, scale, zp)) == lo


@functools.lru_cache(maxsize=None)
def residual_case(n, form, r_dtype):
    """(x, residual codes, their float32 value by numpy) for ``join_case(n, form)``'s x: read-only."""
    x = join_case(n, form)[0]
    s, z = R_FORMS[r_dtype]
    rng = np.random.default_rng(n + (1 if r_dtype == torch.int8 else 2))
    lo, hi = (-128, 127) if r_dtype == torch.int8 else (0, 255)
    c = rng.integers(lo, hi + 1, n).astype(np.int8 if r_dtype == torch.int8 else np.uint8)
    k = min(n, 6)
    c[:k] = np.array([lo, hi, z, z + 1, z - 1, lo], dtype=np.int64)[:k].astype(c.dtype)
    deq = ((c.astype(np.int32) - z).astype(F32) * F32(s)).astype(F32)
    c.setflags(write=False)
    deq.setflags(write=False)
    return x, c, deq


@functools.lru_cache(maxsize=None)
def cpu_route_rc(n, form, r_dtype, relu):
    """(y, codes) as numpy of the float32-residual join on the CPU for ``residual_case``: the reference of the GPU tests too."""
    from mct_quantizers_amd.hip import ops
    x, c, deq = residual_case(n, form, r_dtype)
    y, codes = ops.fq_join(torch.from_numpy(x.copy()), *FORMS[form], residual=torch.from_numpy(deq.copy()), relu=relu)
    return y.numpy(), codes.numpy()


@pytest.mark.parametrize("form", ["u8", "i8"])
@pytest.mark.parametrize("r_dtype", [torch.int8, torch.uint8])
@pytest.mark.parametrize("relu", [False, True])
def test_a_residual_given_as_codes_is_the_residual_given_dequantized_on_cpu(form, r_dtype, relu):
    from mct_quantizers_amd.hip import ops
    x, c, deq = (torch.from_numpy(a.copy()) for a in residual_case(N_JOIN, form, r_dtype))
    s, z = R_FORMS[r_dtype]
    assert bits_equal(ops.dequantize_codes(c, s, z).numpy(), deq.numpy())
    want_y, want_c = cpu_route_rc(N_JOIN, form, r_dtype, relu)
    for want_float, want_codes in OUTPUTS:
        y, codes = ops.fq_join(x, *FORMS[form], relu=relu, want_float=want_float, want_codes=want_codes, residual_codes=(c, s, z))
        assert (y is None) == (not want_float) and (codes is None) == (not want_codes)
        if want_float:
            assert bits_equal(y.numpy(), want_y), first_mismatch(y.numpy(), want_y, x.numpy())
        if want_codes:
            assert codes.dtype == (torch.uint8 if form == "u8" else torch.int8) and np.array_equal(codes.numpy(), want_c)
    assert len(np.unique(want_c)) > 100 and np.isnan(x.numpy()).any()
    with pytest.raises(ValueError):
        ops.fq_join(x, *FORMS[form], residual=deq, residual_codes=(c, s, z))
    with pytest.raises(TypeError):
        ops.fq_join(x, *FORMS[form], residual_codes=(deq, s, z))
    with pytest.raises(ValueError):
        ops.fq_join(x, *FORMS[form], residual_codes=(c, s, 300))
    with pytest.raises(ValueError):
        ops.fq_join(x, *FORMS[form], residual_codes=(c, 0.0, z))


def test_quantized_join_with_a_residual_as_codes_on_cpu():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    holder = _holder("relu")
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 5, 7, generator=g) * 3
    c = torch.randint(-128, 128, (2, 16, 5, 7), generator=g).to(torch.int8)
    s, z = R_FORMS[torch.int8]
    deq = ops.dequantize_codes(c, s, z)
    plain = consumers.QuantizedJoin(holder, relu=True, has_residual=True)
    coded = consumers.QuantizedJoin(holder, relu=True, has_residual=True, residual_codes=(s, z))
    cl = torch.channels_last
    for xx, cc, dd in ((x, c, deq), (x.contiguous(memory_format=cl), c.contiguous(memory_format=cl), deq.contiguous(memory_format=cl))):
        (y, codes), (wy, wc) = coded(xx, cc), plain(xx, dd)
        assert bits_equal(y.numpy(), wy.numpy()) and torch.equal(codes, wc) and codes.stride() == wc.stride()
    with pytest.raises(TypeError):
        coded(x, deq)                                    # built for codes
    with pytest.raises(TypeError):
        plain(x, c)                                      # built for float32
    with pytest.raises(ValueError):
        consumers.QuantizedJoin(holder, residual_codes=(s, z))           # no residual operand to describe


# ---- what a consumer emits -----------------------------------------------------------------------------------------------

class _Emitter(torch.nn.Module):
    """holder -> wrapped layer -> clamp activation -> holder -> wrapped pointwise layer."""

    def __init__(self, first, act, second):
        super().__init__()
        (self.h1, self.c1), self.act, (self.h2, self.c2) = first, act, second

    def forward(self, x):
        return self.c2(self.h2(self.act(self.c1(self.h1(x)))))


def linear_pair(K, N, family, act, seed, bits=None, per_channel=True):
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N)
    with torch.no_grad():
        lin.weight.copy_(torch.randn_like(lin.weight) * 0.4 + 0.1)
    wq = weights_quantizer(lin.weight, family, per_channel, bits)
    return [mq.PytorchActivationQuantizationHolder(activation_quantizer(act)), mq.PytorchQuantizationWrapper(lin, {"weight": wq})]


def emitter(kind, family, act, holder_kind, bits=None):
    """(model, input, the producer's class name): a consumer of class ``kind`` in front of ``act`` and a ``holder_kind`` holder."""
    from mct_quantizers_amd import consumers
    x4 = torch.randn(2, 16, 6, 5, generator=torch.Generator().manual_seed(11)) * 1.5
    lut = family.startswith("lut")
    if kind == "linear":
        first = linear_pair(32, 48, family, "uniform", 1, bits, per_channel=not lut)
        second = linear_pair(48, 16, "sym", holder_kind, 2)
        x = torch.randn(1 if bits or lut else 5, 32, generator=torch.Generator().manual_seed(12)) * 1.5
        return _Emitter(first, act, second), x, consumers.QuantizedLinear
    second = conv_pair(C=32, O=16, k=1, padding=0, seed=2, act=holder_kind)
    if kind == "1x1":
        return _Emitter(conv_pair(C=16, O=32, k=1, padding=0, seed=1, family=family), act, second), x4, consumers.QuantizedConv1x1
    if kind == "kxk":
        return _Emitter(conv_pair(C=16, O=32, k=3, stride=2, seed=1, family=family), act, second), x4, consumers.QuantizedConv2d
    x32 = torch.randn(2, 32, 6, 5, generator=torch.Generator().manual_seed(13)) * 1.5
    first = conv_pair(C=32, O=32, k=3, groups=32, seed=1, family=family)
    return _Emitter(first, act, second), x32, consumers.QuantizedDepthwiseConv2d


ACTIVATIONS = {"relu": (lambda: torch.nn.ReLU(), "signed", torch.relu),
               "relu6": (lambda: torch.nn.ReLU6(), "relu", F.relu6),
               "hardtanh": (lambda: torch.nn.Hardtanh(-1.0, 1.0), "uniform", lambda v: F.hardtanh(v, -1.0, 1.0))}
SWITCHES = dict(uniform_weights=True, convolutions=True, depthwise=True, shared_holders=True)


def check_emitted_codes(kind, family, act_name, device="cpu", bits=None):
    """The producer emits the holder's codes of act(its float32 output) -- the float32 output taken from the same model rewritten
    without ``stay_on_codes`` on the same device -- in the code type of the holder's own domain.  Returns the launch names."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    make_act, holder_kind, fn = ACTIVATIONS[act_name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, x, cls = emitter(kind, family, make_act(), holder_kind, bits)
        twin = emitter(kind, family, make_act(), holder_kind, bits)[0]
    model, twin, x = model.to(device), twin.to(device), x.to(device)
    gm, n = consumers.fuse_linear_consumers_fx(model, stay_on_codes=True, **SWITCHES)
    gm0, n0 = consumers.fuse_linear_consumers_fx(twin, **SWITCHES)
    assert n == n0 == 2
    assert _targets(gm) == ["c1_qlinear", "c2_qlinear"] and not _targets(gm, "call_function") and not _targets(gm, "call_method")
    producer, behind = gm.get_submodule("c1_qlinear"), gm.get_submodule("c2_qlinear")
    assert type(producer) is cls and producer.emit_codes_for == behind.activation_code_params()
    scale, zp, qmin, qmax = behind.activation_code_params()
    seen, seen0, names = {}, {}, []

    def keep(m, args, out):
        seen["y"] = out
        names.append(native.last_launch())

    hooks = [producer.register_forward_hook(keep),
             gm0.get_submodule("c1_qlinear").register_forward_hook(lambda m, a, out: seen0.update(y=out))]
    y, y0 = gm(x), gm0(x)
    for h in hooks:
        h.remove()
    want = ops.fq_codes(fn(seen0["y"]), None, None, None, qmin, qmax, scale, zp)
    got = seen["y"]
    assert seen0["y"].dtype == torch.float32 and got.dtype == want.dtype == (torch.int8 if qmin < 0 else torch.uint8)
    assert got.shape == want.shape and torch.equal(got.cpu(), want.cpu()), int((got.cpu() != want.cpu()).sum())
    lo, hi = producer.emit_clamp
    assert (lo, hi) == consumers.folded_clamp((scale, zp, qmin, qmax), *{"relu": (0.0, math.inf), "relu6": (0.0, 6.0),
                                                                      "hardtanh": (-1.0, 1.0)}[act_name])
    assert (lo, hi) != (qmin, qmax) and int(got.min()) == lo and len(torch.unique(got)) > 8
    assert bits_equal(y.cpu().numpy(), y0.cpu().numpy())
    return names


@pytest.mark.parametrize("act", list(ACTIVATIONS))
@pytest.mark.parametrize("kind,family", [("linear", "sym"), ("linear", "uniform"), ("linear", "lut16")]
                         + [(k, f) for k in ("1x1", "kxk", "dw") for f in FAMILIES])
def test_a_consumer_emits_the_holders_codes_with_the_activation_folded_in(kind, family, act):
    check_emitted_codes(kind, family, act)


def test_a_signed_domain_narrowed_to_its_upper_half_stays_int8():
    """[-128, 127] behind a ReLU is clamped to [0, 127], which ``ops._code_dtype`` alone would call uint8."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    assert ops._code_dtype(0, 127)[0] == torch.uint8
    a = torch.randint(0, 256, (5, 32), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    w = torch.randint(-128, 128, (16, 32), generator=torch.Generator().manual_seed(2)).to(torch.int8)
    ws, rs = torch.full((16,), 0.01), w.sum(dim=1, dtype=torch.int32)
    y = consumers.qlinear_i8(a, 114, 0.02, w, ws, rs, None)
    narrowed = consumers.qlinear_i8(a, 114, 0.02, w, ws, rs, None, out_codes=(0.1, 0, -128, 127, 0, 127))
    assert narrowed.dtype == torch.int8 and torch.equal(narrowed, ops.fq_codes(torch.relu(y), None, None, None, -128, 127, 0.1, 0))
    assert int(narrowed.min()) == 0 and int(narrowed.max()) > 50 and bool((y < 0).any())
    with pytest.raises(ValueError):
        consumers.qlinear_i8(a, 114, 0.02, w, ws, rs, None, out_codes=(0.1, 0, -128, 127, -129, 127))


# ---- the rewritten graphs ------------------------------------------------------------------------------------------------

class FourBlocks(torch.nn.Module):
    """An input holder and four bottleneck blocks: the first strided with a downsample branch, then three identity blocks."""

    def __init__(self):
        super().__init__()
        self.h0 = _holder("uniform")
        self.A = _Block(16, 16, 32, 2, True, 10)
        self.B = _Block(32, 16, 32, 1, False, 20)
        self.C = _Block(32, 16, 32, 1, False, 30)
        self.D = _Block(32, 16, 32, 1, False, 40)
        # (smaller last convolutions in the identity blocks: with _Block's weights as they are, four residual adds in a row
        # saturate the holders and the output is a handful of values)
        with torch.no_grad():
            for block in (self.B, self.C, self.D):
                block.c3.weight.mul_(0.1)
                block.c3.layer.bias.mul_(0.1)

    def forward(self, x):
        return self.D(self.C(self.B(self.A(self.h0(x)))))


def block_input(device="cpu", channels_last=False):
    x = (torch.randn(2, 16, 9, 7, generator=torch.Generator().manual_seed(5)) * 1.5).to(device)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


MODELS = {"four blocks": (FourBlocks, dict(convolutions=True, shared_holders=True)),
          "inverted residual": (InvertedResidual, dict(depthwise=True, shared_holders=True))}


def rewritten(name, device="cpu"):
    """(with ``stay_on_codes``, without) of a fresh model each; the same seeds build the same weights."""
    from mct_quantizers_amd import consumers
    make, switches = MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = make().to(device), make().to(device)
    gm, n = consumers.fuse_linear_consumers_fx(a, stay_on_codes=True, **switches)
    gm0, n0 = consumers.fuse_linear_consumers_fx(b, **switches)
    assert n == n0 == (13 if name == "four blocks" else 3)
    return gm, gm0


def _joins(gm):
    from mct_quantizers_amd import consumers
    return {name: m for name, m in gm.named_modules() if isinstance(m, consumers.QuantizedJoin)}


def test_four_block_stack_graph():
    from mct_quantizers_amd import consumers
    import mct_quantizers_amd as mq
    gm, gm0 = rewritten("four blocks")
    assert len(_joins(gm0)) == 1 + 8 + 3
    joins = {name: (m.relu, m.has_residual, m.want_float, m.residual_codes is not None) for name, m in _joins(gm).items()}
    # the input holder (nothing in front to emit its codes) and the three block ends; the eight ReLU-only joins are gone
    assert joins == {"h0_join": (False, False, False, False), "A_a3_1_join": (True, True, False, False),
                     "B_a3_1_join": (True, True, False, True), "C_a3_1_join": (True, True, True, True)}
    consumers_ = {name: m for name, m in gm.named_modules() if isinstance(m, consumers.IntegerConsumer)}
    assert len(consumers_) == 13
    emitting = sorted(name for name, m in consumers_.items() if m.emit_codes_for is not None)
    assert emitting == sorted(f"{b}_{c}_qlinear" for b in "ABCD" for c in ("c1", "c2"))
    for name in emitting:                                 # the ReLU in front of the "relu" holder (zero point 19 of 0 .. 255)
        m = consumers_[name]
        assert m.emit_clamp == (m.emit_codes_for[1], 255) and m.emit_codes_for[2:] == (0, 255) and m.emit_codes_for[1] > 0
    assert _targets(gm) == ["h0_join", "A_c1_qlinear", "A_c2_qlinear", "A_c3_qlinear", "A_down_qlinear", "A_a3_1_join",
                            "B_c1_qlinear", "B_c2_qlinear", "B_c3_qlinear", "B_a3_1_join",
                            "C_c1_qlinear", "C_c2_qlinear", "C_c3_qlinear", "C_a3_1_join",
                            "D_c1_qlinear", "D_c2_qlinear", "D_c3_qlinear", "D.a3.0", "D.a3.1"]
    nodes = {n.target: n for n in gm.graph.nodes if n.op == "call_module"}

    def picks(join):
        return {u.args[1]: u for u in nodes[join].users}

    # the second and third block-end joins take the codes of the join in front, as their second operand
    for join, up, c3 in (("B_a3_1_join", "A_a3_1_join", "B_c3_qlinear"), ("C_a3_1_join", "B_a3_1_join", "C_c3_qlinear")):
        assert nodes[join].args == (nodes[c3], picks(up)[1])
        m, u = gm.get_submodule(join), gm.get_submodule(up)
        assert m.residual_codes == (u._a_scale, u._a_zp)
    # the one in the middle takes codes and gives nothing but codes, to the next block's c1 and to the next join
    assert set(picks("A_a3_1_join")) == set(picks("B_a3_1_join")) == {1} and set(picks("C_a3_1_join")) == {0, 1}
    assert sorted(u.target for u in picks("B_a3_1_join")[1].users) == ["C_a3_1_join", "C_c1_qlinear"]
    # the last block's add and ReLU stay in float32, in front of the plain holder D.a3.1; nothing else computes in float
    funcs = [n.target for n in gm.graph.nodes if n.op == "call_function" and n.target is not operator.getitem]
    assert funcs == [operator.add] and not _targets(gm, "call_method")
    relus = [t for t in _targets(gm) if isinstance(gm.get_submodule(t), torch.nn.ReLU)]
    assert relus == ["D.a3.0"] and isinstance(gm.get_submodule("D.a3.1"), mq.PytorchActivationQuantizationHolder)
    assert [u.target for u in picks("C_a3_1_join")[0].users] == [operator.add]
    # tracing the rewritten graph again replaces nothing more
    again, n = consumers.fuse_linear_consumers_fx(gm, stay_on_codes=True, **MODELS["four blocks"][1])
    assert n == 0 and _targets(again) == _targets(gm) and len(list(again.graph.nodes)) == len(list(gm.graph.nodes))
    assert {k: (m.relu, m.has_residual, m.want_float, m.residual_codes is not None) for k, m in _joins(again).items()} == joins


def test_inverted_residual_graph():
    from mct_quantizers_amd import consumers
    gm, gm0 = rewritten("inverted residual")
    assert F.relu6 in _targets(gm0, "call_function") and not _joins(gm0) and not _joins(gm)
    assert _targets(gm) == ["c1_qlinear", "c2_qlinear", "c3_qlinear"]
    assert [t for t in _targets(gm, "call_function")] == [operator.add] and not _targets(gm, "call_method")
    c1, c2, c3 = (gm.get_submodule(f"c{i}_qlinear") for i in (1, 2, 3))
    assert c1.emit_codes_for == c2.activation_code_params() and c2.emit_codes_for == c3.activation_code_params()
    assert c3.emit_codes_for is None and c3.emit_clamp is None
    for m in (c1, c2):                                   # ReLU6 in front of the "relu" holder: both ends move
        lo, hi = m.emit_clamp
        assert (lo, hi) == consumers.folded_clamp(m.emit_codes_for, 0.0, 6.0) and 0 < lo < hi <= 255


def check_bits_against_the_rewrite_without(name, device, channels_last):
    gm, gm0 = rewritten(name, device)
    x = block_input(device, channels_last)
    y, y0 = gm(x), gm0(x)
    assert y.dtype == torch.float32 and y.shape == y0.shape and len(torch.unique(y)) > 50
    assert bits_equal(y.cpu().numpy(), y0.cpu().numpy()), first_mismatch(y.cpu().numpy(), y0.cpu().numpy())
    # an in-place weight update: both models refresh their codes and still agree
    with torch.no_grad():
        for g in (gm, gm0):
            for m in g.modules():
                if hasattr(m, "_refresh_weight_codes"):
                    m.weight.mul_(0.75)
    y2, y02 = gm(x), gm0(x)
    assert bits_equal(y2.cpu().numpy(), y02.cpu().numpy()) and not torch.equal(y2, y)
    return y, y2


@pytest.mark.parametrize("name", list(MODELS))
def test_rewritten_models_give_the_bits_of_the_rewrite_without_on_cpu(name):
    y, y2 = check_bits_against_the_rewrite_without(name, "cpu", False)
    yc, yc2 = check_bits_against_the_rewrite_without(name, "cpu", True)
    assert bits_equal(y.numpy(), yc.numpy()) and bits_equal(y2.numpy(), yc2.numpy())


# ---- guard rails ----------------------------------------------------------------------------------------------------------

def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers
    for switches in (dict(convolutions=True), dict(convolutions=True, shared_holders=True),
                     dict(convolutions=True, shared_holders=True, chain=True)):
        gm, n = consumers.fuse_linear_consumers_fx(ResidualStack(), **switches)
        gm_off, n_off = consumers.fuse_linear_consumers_fx(ResidualStack(), stay_on_codes=False, **switches)
        assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
        assert all(m.emit_clamp is None for m in gm.modules() if isinstance(m, consumers.IntegerConsumer))
    gm, _ = consumers.fuse_linear_consumers_fx(ResidualStack(), convolutions=True, shared_holders=True)
    assert _targets(gm) == ["h0_join", "A_c1_qlinear", "A_a1_1_join", "A_c2_qlinear", "A_a2_1_join", "A_c3_qlinear",
                            "A_down_qlinear", "A_a3_1_join", "B_c1_qlinear", "B_a1_1_join", "B_c2_qlinear", "B_a2_1_join",
                            "B_c3_qlinear", "B.a3.0", "B.a3.1"]
    assert all(m.residual_codes is None for m in _joins(gm).values())
    for switches in (dict(), dict(convolutions=True), dict(chain=True), dict(shared_holders=False)):
        with pytest.raises(ValueError):
            consumers.fuse_linear_consumers_fx(ResidualStack(), stay_on_codes=True, **switches)
    with pytest.raises(TypeError):
        consumers.fuse_linear_consumers(torch.nn.Sequential(), stay_on_codes=True)


class _Rail(torch.nn.Module):
    """c0 -> (what ``how`` says) -> holder -> c1 (and c2)."""

    def __init__(self, how):
        super().__init__()
        self.how = how
        self.h0, self.c0 = conv_pair(C=16, O=16, k=1, padding=0, seed=1)
        self.h, self.c1 = conv_pair(C=16, O=16, k=1, padding=0, seed=2, act="relu")
        self.c2 = conv_pair(C=16, O=16, k=1, padding=0, seed=3)[1]
        self.act = torch.nn.ReLU(inplace=True)

    def forward(self, x):
        y = self.c0(self.h0(x))
        if self.how == "float user":                     # the holder's float32 tensor is read by an add as well
            a = self.h(torch.relu(y))
            return self.c1(a) + self.c2(a) + a
        if self.how == "activation twice":
            v = F.relu6(y)
            a = self.h(v)
            return self.c1(a) + self.c2(a) + v
        if self.how == "empty hardtanh":
            a = self.h(F.hardtanh(y, 2.0, 1.0))
            return self.c1(a) + self.c2(a)
        if self.how == "inplace twice":
            a = self.h(self.act(y))                      # rewrites y, which the last add reads as well
            return self.c1(a) + self.c2(a) + y
        a = self.h(F.hardtanh(y, -1.0, max_val=2.0) if self.how == "hardtanh" else F.relu6(y))
        return self.c1(a) + self.c2(a)


def test_what_the_rewrite_leaves_alone():
    from mct_quantizers_amd import consumers
    for how in ("float user", "activation twice", "empty hardtanh", "inplace twice", "relu6", "hardtanh"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm0, n0 = consumers.fuse_linear_consumers_fx(_Rail(how), shared_holders=True)
            gm, n = consumers.fuse_linear_consumers_fx(_Rail(how), shared_holders=True, stay_on_codes=True)
        assert n == n0 == 3
        c0 = gm.get_submodule("c0_qlinear")
        if how in ("relu6", "hardtanh"):                 # the positive cases: a shared holder behind the activation is taken
            assert c0.emit_codes_for is not None and not _joins(gm) and len(_joins(gm0)) == 1, how
            assert _targets(gm) == ["c0_qlinear", "c1_qlinear", "c2_qlinear"], how
            assert c0.emit_clamp == consumers.folded_clamp(c0.emit_codes_for, *((0.0, 6.0) if how == "relu6" else (-1.0, 2.0)))
            x = block_input()
            assert bits_equal(gm(x).numpy(), gm0(x).numpy())
        else:
            assert c0.emit_codes_for is None and c0.emit_clamp is None, how
            assert str(gm.graph) == str(gm0.graph) and gm.code == gm0.code, how


def test_wrapped_resnet50_structure():
    """Trace and rewrite only.  53 convolutions, of which the stem (3 channels) and the first block's c1 and downsample (behind
    the max-pool, no holder in front) stay wrappers: 50 consumers.  47 joins without ``stay_on_codes``: 32 ReLU-only ones (two per
    block) and 15 block ends (the 16th block's add stays plain, in front of the pool).  With it 31 of the ReLU-only joins go --
    the one behind the first block's c1 stays, its producer being a wrapper -- and the 11 block ends whose identity is the
    join in front (16 blocks less 4 with a downsample branch less the last, which is no join) take codes; only the 15th
    join, which feeds the last block's plain add, still writes float32."""
    from mct_quantizers_amd import consumers, workloads
    switches = dict(convolutions=True, shared_holders=True)
    gm0, n0 = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu"), **switches)
    gm, n = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu"), stay_on_codes=True, **switches)
    assert n == n0 == 50 and len(_joins(gm0)) == 47
    joins = _joins(gm)
    names = [t for t in _targets(gm) if t in joins]
    assert len(names) == len(joins) == 16
    residual = [t for t in names if joins[t].has_residual]
    assert len(residual) == 15 and [t for t in names if not joins[t].has_residual] == ["3_a1_1_join"]
    assert (joins["3_a1_1_join"].relu, joins["3_a1_1_join"].want_float) == (True, False)
    assert sum(joins[t].residual_codes is not None for t in residual) == 11
    assert [t for t in names if joins[t].want_float] == [residual[-1]] == ["17_a3_1_join"]
    emitting = [m for m in gm.modules() if isinstance(m, consumers.IntegerConsumer) and m.emit_codes_for is not None]
    assert len(emitting) == 31 and len([m for m in gm.modules() if isinstance(m, consumers.IntegerConsumer)]) == 50
    # an unsigned domain with zero point 0: the ReLU's code is the domain's lower end, nothing is left to narrow
    assert all(m.emit_clamp is None and m.emit_codes_for[1:] == (0, 0, 255) for m in emitting)
    relus = [t for t in _targets(gm) if isinstance(gm.get_submodule(t), torch.nn.ReLU)]
    assert relus == ["1.0", "18.a3.0"]                    # the stem's and the last block's


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------

def test_fq_join_rc_argument_validation_needs_no_gpu():
    import os
    import re
    from conftest import REPO
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_fq_join_rc_f32\s*\(", header) and "mctq_fq_join_rc_f32" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, I8, U8 = native.MCTQ_E_ARG, 4096, native.CODE_I8, native.CODE_U8      # P: an aligned address that is never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(x=P, rc=P, rdt=I8, rs=0.25, rz=-3, relu=1, y=P, codes=P, cdt=U8, n=100, scale=0.5, zp=3, qmin=0, qmax=255)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_fq_join_rc_f32(v["x"], v["rc"], v["rdt"], v["rs"], v["rz"], v["relu"], v["y"], v["codes"], v["cdt"], v["n"],
                                       v["scale"], v["zp"], v["qmin"], v["qmax"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    refused(b"n < 0", n=-1)
    refused(b"r_codes is NULL", rc=None)
    for rdt in (-1, 2, 3, 77):                                             # the 4-bit code types among them
        refused(b"bad r_code_dtype", rdt=rdt)
    for rdt, rz in ((I8, -129), (I8, 128), (U8, -1), (U8, 256)):
        refused(b"r_zero_point is no code of the residual's type", rdt=rdt, rz=rz)
    for rs in (0.0, -0.5, float("inf"), float("nan")):
        refused(b"r_scale must be finite and positive", rs=rs)
    # wrong in two ways: the residual's code type, its zero point, its scale, then what mctq_fq_join_f32 looks at
    refused(b"bad r_code_dtype", rdt=77, rz=256)
    refused(b"r_zero_point is no code of the residual's type", rz=128, rs=0.0)
    refused(b"r_scale must be finite and positive", rs=0.0, x=None)
    # ... and everything mctq_fq_join_f32 refuses
    refused(b"x is NULL", x=None)
    refused(b"neither y nor codes is given", y=None, codes=None)
    refused(b"bad code_dtype", cdt=2)
    refused(b"clamp domain does not fit the code type", cdt=I8, qmin=-128, qmax=128)
    refused(b"quant_min > quant_max", qmin=200, qmax=100)
    refused(b"clamp domain beyond 2^24 with a float32 output", codes=None, qmax=2 ** 24 + 1)
    for pointer, off in (("x", 4), ("y", 4), ("codes", 1)):
        refused(b"x, residual, y and codes must be 16-byte aligned", **{pointer: P + off})
    for off in (1, 4, 8):
        refused(b"r_codes must be 16-byte aligned", rc=P + off)
    refused(b"tensor too large for one launch", n=(2 ** 31) * 4096)
    assert call(n=0) == 0 and call(n=0, x=None, rc=None, y=None, codes=None) == 0
    assert call(n=0, rdt=77) == 0 and call(n=0, rs=-1.0) == 0 and call(n=0, rc=P + 1) == 0
    assert lib.mctq_launch_count() == count                                # refused and empty calls launch nothing
