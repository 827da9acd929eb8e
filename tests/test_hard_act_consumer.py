"""Hardswish and Hardsigmoid folded into the integer consumers' epilogues: host logic and the CPU route (include/mctq_hip.h:
mctq_qlinear_i8_act, mctq_qconv_dw_i8_act; consumers.qlinear_i8(act=...), qconv_dw_i8(act=...), IntegerConsumer.emit_act and the
``hard_activations`` switch of fuse_linear_consumers_fx).

Everything here is exact, so every check is equality.  The CPU routes apply ``F.hardswish`` / ``F.hardsigmoid`` to the float32
value the plain call returns, in front of ``ops.fq_codes``: by construction what the float32 chain gives on the CPU.  (The
kernels evaluate the expression of ATen's GPU kernels, which rounds differently for a quarter of all inputs: the GPU tests take
the float32 chain on the GPU as their reference, not this route.)  A model rewritten with ``hard_activations=True`` is compared
bit for bit with the same rewrite without it.

The problems of the raw product -- shared with tests/test_gpu_hard_act_consumer.py -- are those of
tests/test_gpu_residual_consumer.py with the weight scales aimed at pre-activation values of about [-8, 8], every region of the
two activations, and in the bias a NaN, both infinities and a -0.0."""
import functools

import numpy as np
import pytest
import torch

from test_concat_consumer import holder_of
from test_conv_consumer import weights_quantizer
from test_gpu_residual_consumer import A_SCALE, SHAPES
from test_join_consumer import _targets
from test_mul_consumer import ALL, SE, block_input
from test_pool_consumer import _of, pot_conv

F = torch.nn.functional
ACTS = ("hardswish", "hardsigmoid")
# (scale, zero_point, qmin, qmax) of the codes behind each activation, uint8 and int8: hardswish gives [-0.375, inf), hardsigmoid
# [0, 1] -- forms whose both clamp ends those values reach (the uint8 form behind the hardsigmoid is the SE gate's own)
OUT_FORMS = {"hardswish": {"u8": (0.02, 10, 0, 255), "i8": (0.03, -120, -128, 127)},
             "hardsigmoid": {"u8": (1.0 / 256, 0, 0, 255), "i8": (1.0 / 256, -128, -128, 127)}}
SPECIAL = {3: float("nan"), 5: float("inf"), 7: float("-inf")}             # bias column -> value (shapes with N >= 16)
ZERO_COLUMN = 9                                                             # its weight scale underflows: sums of both signs -> +-0.0


@functools.lru_cache(maxsize=None)
def act_problem(M, N, K, u8):
    """One problem per (shape, code type), shared by every launch variant and both activations: the operands and the exact int32
    sums.  Pre-activation values of the order of 4, reaching beyond +-8; K = 32768 holds the accumulator's extremes."""
    g = torch.Generator().manual_seed(11 * M + 5 * N + K + u8)
    a = torch.randint(0, 256, (M, K), generator=g).to(torch.uint8) if u8 else torch.randint(-128, 128, (M, K), generator=g).to(torch.int8)
    w = torch.randint(-128, 128, (N, K), generator=g).to(torch.int8)
    za = 114 if u8 else -5
    if K == 32768:
        if u8:
            a[:], za, w[:] = 255, 0, -128                                    # sum = 255 * (-128) * 32768
            w[1] = 127                                                       # ... and 255 * 127 * 32768
        else:
            a[:], za, w[:] = -128, 127, 127                                  # sum = (-255) * 127 * 32768
            w[1] = -128                                                      # ... and (-255) * (-128) * 32768
    ws = ((torch.rand(N, generator=g) + 0.5) * (4.0 / (A_SCALE * 5476.0 * K ** 0.5))).float().contiguous()
    bias = ((torch.rand(N, generator=g) - 0.5) * 4).float().contiguous()
    if N >= 16:
        for col, v in SPECIAL.items():
            bias[col] = v
        ws[ZERO_COLUMN], bias[ZERO_COLUMN] = 1e-45, -0.0                     # A_SCALE * 1e-45 rounds to 0: sum * 0 = +-0.0
    acc = (a.to(torch.int32) - za) @ w.to(torch.int32).t()
    return dict(a=a, za=za, w=w, ws=ws, rowsum=w.sum(dim=1, dtype=torch.int32).contiguous(), bias=bias, acc=acc)


def act_combos():
    """(activation, with bias, output kind): all eight."""
    for act in ACTS:
        for with_bias in (False, True):
            for kind in ("u8", "i8"):
                yield act, with_bias, kind


def pre_activation(p, with_bias):
    from mct_quantizers_amd import consumers
    return consumers._cpu_epilogue(p["acc"], A_SCALE, p["ws"], p["bias"] if with_bias else None, None)


def chain_codes(y, act, form):
    """The float32 chain behind a plain call, on y's device: ATen's activation, then the holder's codes."""
    from mct_quantizers_amd.hip import ops
    return ops.fq_codes(getattr(F, act)(y), None, None, None, form[2], form[3], form[0], form[1])


# ---- the functions on CPU tensors -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES[:6])
def test_qlinear_i8_with_an_activation_on_cpu_is_the_float32_chain(shape):
    from mct_quantizers_amd import consumers
    for u8 in (False, True):
        p = act_problem(*shape, u8)
        for act, with_bias, kind in act_combos():
            form, bias = OUT_FORMS[act][kind], p["bias"] if with_bias else None
            y = consumers.qlinear_i8(p["a"], p["za"], A_SCALE, p["w"], p["ws"], p["rowsum"], bias)
            assert torch.equal(y.view(torch.int32), pre_activation(p, with_bias).view(torch.int32))
            got = consumers.qlinear_i8(p["a"], p["za"], A_SCALE, p["w"], p["ws"], p["rowsum"], bias, form, act=act)
            assert got.dtype == (torch.uint8 if kind == "u8" else torch.int8)
            assert torch.equal(got, chain_codes(y, act, form)), (shape, u8, act, with_bias, kind)


def test_the_cases_hold_what_they_claim():
    """Both clamp ends and more than 50 distinct codes in every output; among the pre-activation values every region of the two
    activations, a NaN, both infinities and a -0.0; the accumulator's extremes at the largest K."""
    for shape in SHAPES[1:]:
        for u8 in (False, True):
            p = act_problem(*shape, u8)
            x = pre_activation(p, True)
            xn = x.numpy()
            if shape[1] >= 16:
                assert (xn <= -3).any() and ((xn > -3) & (xn < 0)).any() and ((xn > 0) & (xn < 3)).any() and (xn >= 3).any()
                assert np.isnan(xn).any() and (xn == np.inf).any() and (xn == -np.inf).any()
                assert ((xn == 0) & np.signbit(xn)).any() and ((xn == 0) & ~np.signbit(xn)).any()
                assert np.isnan(F.hardswish(x).numpy()[xn == -np.inf]).all()             # -inf * 0
                assert shape[2] == 32768 or float(np.nanmin(xn[np.isfinite(xn)])) < -8 and float(np.nanmax(xn[np.isfinite(xn)])) > 8
                for act in ACTS:
                    for kind, form in OUT_FORMS[act].items():
                        codes = chain_codes(x, act, form).numpy()
                        assert codes.min() == form[2] and codes.max() == form[3] and len(np.unique(codes)) > 50, (shape, act, kind)
    acc = act_problem(2, 3, 32768, True)["acc"]
    assert int(acc.min()) == 255 * -128 * 32768 and int(acc.max()) == 255 * 127 * 32768
    acc = act_problem(2, 3, 32768, False)["acc"]
    assert int(acc.min()) == -255 * 127 * 32768 and int(acc.max()) == 255 * 128 * 32768


def test_qconv_dw_i8_with_an_activation_on_cpu_is_the_float32_chain():
    from test_dw_consumer import raw_case, raw_cases, run_raw_on
    from mct_quantizers_amd import consumers
    n = 0
    for case in list(raw_cases())[::5]:
        c = raw_case(*case)
        y = run_raw_on(c, "cpu")
        t = lambda v: None if v is None else torch.from_numpy(v.copy())      # noqa: E731
        for act in ACTS:
            for kind, form in OUT_FORMS[act].items():
                got = consumers.qconv_dw_i8(t(c["a"]), c["za"], c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), *c["geometry"],
                                            out_codes=form, w_zero_points=t(c["zw"]), act=act)
                assert torch.equal(got, chain_codes(y, act, form)) and len(torch.unique(got)) > 8, (case, act, kind)
        n += (c["zw"] is not None) + 2 * (c["bias"] is not None)
    assert n > 6                                                             # with and without zero points, with and without bias


def test_the_functions_refuse_what_the_entry_points_do_not_take():
    from mct_quantizers_amd import consumers
    p = act_problem(5, 100, 256, True)
    args = (p["a"], p["za"], A_SCALE, p["w"], p["ws"], p["rowsum"], p["bias"])
    form = OUT_FORMS["hardswish"]["u8"]
    with pytest.raises(ValueError, match="needs out_codes"):
        consumers.qlinear_i8(*args, act="hardswish")
    with pytest.raises(ValueError, match="act must be"):
        consumers.qlinear_i8(*args, form, act="sigmoid")
    with pytest.raises(NotImplementedError):
        consumers.qlinear_i8(*args, form, w_zero_points=torch.zeros(100, dtype=torch.int32), act="hardswish")
    with pytest.raises(NotImplementedError):
        consumers.qlinear_i8(*args, form, residual=torch.zeros(5, 100), act="hardsigmoid")
    from test_dw_consumer import raw_case
    c = raw_case(True, 16, 0, 114, False, True)
    t = lambda v: None if v is None else torch.from_numpy(v.copy())          # noqa: E731
    dw = (t(c["a"]), c["za"], c["sa"], t(c["w"]), t(c["ws"]), t(c["bias"]), *c["geometry"])
    with pytest.raises(ValueError, match="needs out_codes"):
        consumers.qconv_dw_i8(*dw, act="hardswish")
    with pytest.raises(ValueError, match="act must be"):
        consumers.qconv_dw_i8(*dw, out_codes=form, act="relu")


def test_argument_validation_of_the_entry_points_needs_no_gpu():
    from mct_quantizers_amd.hip import native
    lib = native.load()
    E = native.MCTQ_E_ARG
    ql = lambda act, y_dt, M=4: lib.mctq_qlinear_i8_act(None, native.CODE_U8, 0, 1.0, None, None, None, None, None, y_dt, 1.0, 0,      # noqa: E731
                                                        0, 255, act, M, 16, 16, None)
    dw = lambda act, y_dt, B=2: lib.mctq_qconv_dw_i8_act(None, native.CODE_U8, 0, 1.0, None, None, None, None, None, y_dt, 1.0, 0,     # noqa: E731
                                                         0, 255, act, B, 5, 5, 16, 3, 3, 1, 1, 1, 1, 1, 1, None)
    for call in (ql, dw):
        for act in (0, 3, -1):
            assert call(act, native.CODE_U8) == E and b"act must be" in lib.mctq_last_error()
        for act in (1, 2):
            assert call(act, -1) == E and b"y_code_dtype" in lib.mctq_last_error()      # float32 output: refused
            assert call(act, native.CODE_U8, 0) == 0                                     # empty: nothing launched
            assert call(act, native.CODE_U8) == E and b"NULL" in lib.mctq_last_error()
    assert lib.mctq_abi_version() == 10


# ---- recognising the activation ---------------------------------------------------------------------------------------------

SPELLINGS = {"module": lambda kind: (torch.nn.Hardswish if kind == "hardswish" else torch.nn.Hardsigmoid)(),
             "module inplace": lambda kind: (torch.nn.Hardswish if kind == "hardswish" else torch.nn.Hardsigmoid)(inplace=True),
             "function": lambda kind: getattr(F, kind),
             "function inplace=": lambda kind: functools.partial(getattr(F, kind), inplace=True),
             "function inplace=False": lambda kind: functools.partial(getattr(F, kind), inplace=False),
             "function positional": lambda kind: (lambda x: getattr(F, kind)(x, True))}


class _Spelled(torch.nn.Module):
    def __init__(self, act, second_reader=False):
        super().__init__()
        self.lin, self.second_reader = torch.nn.Linear(4, 4), second_reader
        if isinstance(act, torch.nn.Module):
            self.act = act
        else:
            self.fn = act

    def forward(self, x):
        y = self.lin(x)
        z = self.act(y) if hasattr(self, "act") else self.fn(y)
        return z + y if self.second_reader else z


def _recognised(model):
    import torch.fx as fx
    from mct_quantizers_amd import consumers
    gm = fx.symbolic_trace(model)
    mods = dict(gm.named_modules())
    found = [consumers._hard_activation(n, mods) for n in gm.graph.nodes if n.op in ("call_module", "call_function")]
    return [k for k in found if k is not None]


@pytest.mark.parametrize("kind", ACTS)
@pytest.mark.parametrize("spelling", list(SPELLINGS))
def test_every_spelling_is_recognised(kind, spelling):
    assert _recognised(_Spelled(SPELLINGS[spelling](kind))) == [kind]
    in_place = spelling in ("module inplace", "function inplace=", "function positional")
    # a second reader of the input: the in-place forms would hand it the activation's output
    assert _recognised(_Spelled(SPELLINGS[spelling](kind), second_reader=True)) == ([] if in_place else [kind])


def test_other_activations_are_not_recognised():
    for act in (torch.nn.Sigmoid(), torch.nn.SiLU(), torch.nn.GELU(), torch.nn.Tanh(), torch.nn.ReLU6(), torch.nn.Hardtanh(),
                torch.sigmoid, F.silu, F.gelu, torch.tanh, F.relu6, lambda x: F.hardswish(x) * 2.0):
        found = _recognised(_Spelled(act))
        assert found == ([] if isinstance(act, torch.nn.Module) or act.__name__ != "<lambda>" else ["hardswish"])


# ---- the rewrite ------------------------------------------------------------------------------------------------------------

def pot_dw(C, seed):
    """A wrapped depthwise 3 x 3 convolution built like ``pot_conv``."""
    import mct_quantizers_amd as mq
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 0.3 + 0.05)
    return mq.PytorchQuantizationWrapper(conv, {"weight": weights_quantizer(conv.weight, "pot", True)})


class Pointwise(torch.nn.Module):
    """conv 1x1 -> Hardswish -> holder -> conv 1x1"""

    def __init__(self, spelling="module"):
        super().__init__()
        self.h0, self.c1, self.h1, self.c2 = holder_of("s4"), pot_conv(16, 16, 1, 1), holder_of("s4"), pot_conv(16, 16, 1, 2)
        self.act = SPELLINGS[spelling]("hardswish")

    def forward(self, x):
        return self.c2(self.h1(self.act(self.c1(self.h0(x)))))


class Depthwise(torch.nn.Module):
    """conv 1x1 -> Hardswish -> holder -> depthwise 3x3 -> Hardswish -> holder -> conv 1x1: MobileNetV3's block"""

    def __init__(self):
        super().__init__()
        self.h0, self.c1, self.h1, self.dw = holder_of("s4"), pot_conv(16, 16, 1, 1), holder_of("s4"), pot_dw(16, 5)
        self.h2, self.c2 = holder_of("s"), pot_conv(16, 16, 1, 2)
        self.act1, self.act2 = torch.nn.Hardswish(), torch.nn.Hardswish(inplace=True)

    def forward(self, x):
        return self.c2(self.h2(self.act2(self.dw(self.h1(self.act1(self.c1(self.h0(x))))))))


class Cat(torch.nn.Module):
    """Two branches into a concatenation, one behind a Hardswish, one behind a ReLU"""

    def __init__(self):
        super().__init__()
        self.h0, self.p, self.q = holder_of("s4"), pot_conv(16, 16, 1, 1), pot_conv(16, 16, 3, 2)
        self.hp, self.hq, self.hc, self.last = holder_of("s4"), holder_of("u4"), holder_of("s4"), pot_conv(32, 16, 1, 3)

    def forward(self, x):
        x = self.h0(x)
        return self.last(self.hc(torch.cat([self.hp(F.hardswish(self.p(x))), self.hq(torch.relu(self.q(x)))], 1)))


# name -> (constructor, the producers that take an activation and which, activations folded)
HARD_MODELS = {"pointwise": (Pointwise, {"c1_qlinear": "hardswish"}),
               "depthwise": (Depthwise, {"c1_qlinear": "hardswish", "dw_qlinear": "hardswish"}),
               "se": (SE, {"fc2_qlinear": "hardsigmoid"}),
               "cat": (Cat, {"p_qlinear": "hardswish"})}
SWITCHES = dict(ALL, muls=True)


def rewrite_pair(make, device="cpu", **switches):
    """(with hard_activations, without), both under the other switches."""
    from mct_quantizers_amd import consumers
    switches = switches or SWITCHES
    on = consumers.fuse_linear_consumers_fx(make().to(device).eval(), hard_activations=True, **switches)
    off = consumers.fuse_linear_consumers_fx(make().to(device).eval(), **switches)
    return on, off


def _activation_nodes(gm):
    from mct_quantizers_amd import consumers
    mods = dict(gm.named_modules())
    return [n for n in gm.graph.nodes if consumers._hard_activation(n, mods) is not None]


@pytest.mark.parametrize("name", list(HARD_MODELS))
def test_rewritten_models(name):
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers as C
    make, producers = HARD_MODELS[name]
    (gm, n), (gm0, n0) = rewrite_pair(make)
    assert n == n0 and n >= len(producers) + 1                  # the switch replaces no layer: it changes what they emit
    assert len(_activation_nodes(gm0)) == len(producers) and not _activation_nodes(gm)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    for target in producers:                                 # no holder and no join is left behind them: their readers read codes
        readers = [gm.get_submodule(u.target) for u in nodes[target].users]
        assert readers and all(isinstance(m, (C.IntegerConsumer, C.QuantizedMul, C.QuantizedConcat)) for m in readers), readers
    stays = lambda g: [t for t in _targets(g) if isinstance(g.get_submodule(t), (mq.PytorchActivationQuantizationHolder, C.QuantizedJoin))]      # noqa: E731
    assert set(stays(gm)) <= set(stays(gm0))                 # (what is left is the input's: nothing new appears)
    for target, kind in producers.items():
        p, p0 = gm.get_submodule(target), gm0.get_submodule(target)
        assert p.emit_act == kind and p.emit_codes_for is not None and p.emit_clamp is None and f"emit_act='{kind}'" in repr(p)
        assert p0.emit_act is None and p0.emit_codes_for is None and "emit_act" not in repr(p0)
    others = [m for t, m in _of(gm, C.IntegerConsumer).items() if t not in producers]
    assert others and all(m.emit_act is None for m in others)
    x = block_input()
    y = gm(x)
    assert torch.equal(y, gm0(x)) and len(torch.unique(y)) > 50
    # tracing the rewritten graph again changes nothing
    again, k = C.fuse_linear_consumers_fx(gm, hard_activations=True, **SWITCHES)
    assert k == 0 and _targets(again) == _targets(gm) and torch.equal(again(x), y)


def test_graph_shapes():
    from mct_quantizers_amd import consumers as C
    (gm, _), (gm0, _) = rewrite_pair(Pointwise)
    assert _targets(gm) == ["c1_qlinear", "c2_qlinear"] and _targets(gm0) == ["c1_qlinear", "act", "c2_qlinear"]
    assert gm.get_submodule("c1_qlinear").emit_codes_for == gm.get_submodule("c2_qlinear").activation_code_params()
    (gm, _), _ = rewrite_pair(Depthwise)
    assert _targets(gm) == ["c1_qlinear", "dw_qlinear", "c2_qlinear"]
    assert isinstance(gm.get_submodule("dw_qlinear"), C.QuantizedDepthwiseConv2d)
    assert gm.get_submodule("dw_qlinear").emit_codes_for == gm.get_submodule("c2_qlinear").activation_code_params()
    # the SE gate reaches the multiply as codes of G's form, where it was float32
    (gm, _), (gm0, _) = rewrite_pair(SE)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["m_mul"].args[1] is nodes["fc2_qlinear"] and "gate" not in nodes and "gate" in _targets(gm0)
    assert gm.get_submodule("fc2_qlinear").emit_codes_for == gm.get_submodule("m_mul").operand_code_params(1) == (1.0 / 256, 0, 0, 255)
    seen = []
    hook = gm.get_submodule("m_mul").register_forward_hook(lambda m, args, out: seen.append([a.dtype for a in args]))
    gm(block_input())
    hook.remove()
    assert seen == [[torch.uint8, torch.uint8]]
    # the concatenation's operand behind the Hardswish
    (gm, _), _ = rewrite_pair(Cat)
    nodes = {node.target: node for node in gm.graph.nodes if node.op == "call_module"}
    assert nodes["hc_concat"].args[0] is nodes["p_qlinear"]
    assert gm.get_submodule("p_qlinear").emit_codes_for == gm.get_submodule("hc_concat").operand_code_params(0)


@pytest.mark.parametrize("spelling", list(SPELLINGS))
def test_every_spelling_folds(spelling):
    (gm, _), (gm0, _) = rewrite_pair(lambda: Pointwise(spelling))
    assert gm.get_submodule("c1_qlinear").emit_act == "hardswish" and not _activation_nodes(gm)
    x = block_input()
    assert torch.equal(gm(x), gm0(x))


def test_the_switch_needs_stay_on_codes_and_without_it_nothing_changes():
    from mct_quantizers_amd import consumers as C
    with pytest.raises(ValueError, match="needs stay_on_codes"):
        C.fuse_linear_consumers_fx(Pointwise().eval(), hard_activations=True, convolutions=True, shared_holders=True)
    with pytest.raises(ValueError, match="needs stay_on_codes"):
        C.fuse_linear_consumers_fx(Pointwise().eval(), hard_activations=True)
    for make, _ in HARD_MODELS.values():
        gm, _ = C.fuse_linear_consumers_fx(make().eval(), **SWITCHES)
        assert all(m.emit_act is None for m in _of(gm, C.IntegerConsumer).values()) and _activation_nodes(gm)


class Odd(Pointwise):
    """What the switch leaves alone.  ``kind``: "float reader" (the holder's float32 output is read too), "shared input" (the
    activation's input has another reader), "two activations" (a ReLU behind the Hardswish), or a weights family / bit width
    whose entry points take no activation."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        if kind in ("uniform", "lut16", "lut256", "4 bits"):
            import mct_quantizers_amd as mq
            torch.manual_seed(1)
            conv = torch.nn.Conv2d(16, 16, 1, bias=False)
            wq = weights_quantizer(conv.weight, "sym" if kind == "4 bits" else kind, True, 4 if kind == "4 bits" else None)
            self.c1 = mq.PytorchQuantizationWrapper(conv, {"weight": wq})

    def forward(self, x):
        y = self.c1(self.h0(x))
        a = self.act(y)
        if self.kind == "two activations":
            a = torch.relu(a)
        h = self.h1(a)
        out = self.c2(h)
        return out + h if self.kind == "float reader" else out + y if self.kind == "shared input" else out


@pytest.mark.parametrize("kind", ["float reader", "shared input", "two activations", "uniform", "lut16", "lut256", "4 bits"])
def test_what_the_switch_leaves_alone(kind):
    from mct_quantizers_amd import consumers as C
    (gm, n), (gm0, n0) = rewrite_pair(lambda: Odd(kind))
    assert n == n0 == 2 and _targets(gm) == _targets(gm0) and len(_activation_nodes(gm)) == 1
    assert all(m.emit_act is None for m in _of(gm, C.IntegerConsumer).values())
    x = block_input()
    assert torch.equal(gm(x), gm0(x))


def test_a_product_that_takes_a_residual_is_refused_an_activation():
    from mct_quantizers_amd import consumers as C
    gm, _ = C.fuse_linear_consumers_fx(Pointwise().eval(), **SWITCHES)
    producer = gm.get_submodule("c1_qlinear")
    assert C._takes_hard_activation(producer)
    producer.emit_residual = "float"
    assert not C._takes_hard_activation(producer)
    producer.emit_residual = None
    # ... and the modules say so themselves where one is set by hand
    producer.emit_codes_for, producer.emit_act, producer.emit_residual = (0.03, 0, -128, 127), "hardswish", "float"
    with pytest.raises(NotImplementedError):
        producer(torch.randn(1, 16, 2, 2), torch.randn(1, 16, 2, 2))
