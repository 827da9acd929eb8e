"""The residual add and the ReLU of a residual join in the integer product's epilogue: host logic and the CPU route
(include/mctq_hip.h: mctq_qlinear_i8_res; consumers.qlinear_i8(residual=..., residual_codes=..., relu=...), IntegerConsumer's
``emit_residual`` / ``emit_relu`` and the ``fused_residuals`` switch of fuse_linear_consumers_fx).

The fused epilogue is the join's own arithmetic on the float32 value the product would have stored, so every check is bit
equality: ``qlinear_i8`` with a residual against ``ops.fq_join`` of the float32 product, and a rewritten model against the same
rewrite without the switch, which tests/test_stay_on_codes.py pins against the rewrite without ``stay_on_codes``."""
import functools
import operator
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, bits_equal, first_mismatch
from test_conv_consumer import conv_pair
from test_join_consumer import FORMS, _holder, _targets, ties
from test_stay_on_codes import FourBlocks, MODELS, _Block, _joins, block_input

F32 = np.float32
# the residual's form differs from either output form; its zero point at either end of the codes' domain
R_FORMS = {(torch.int8, "lo"): (0.23, -128), (torch.int8, "hi"): (0.23, 127), (torch.uint8, "lo"): (0.19, 0),
           (torch.uint8, "hi"): (0.19, 255)}
RESIDUALS = [(torch.float32, None)] + list(R_FORMS)
# output forms: both FORMS entries, each also narrowed (a folded clamp), the signed one to its upper half
OUT_FORMS = {"u8": FORMS["u8"], "i8": FORMS["i8"], "u8 narrowed": (*FORMS["u8"], 120, 250), "i8 narrowed": (*FORMS["i8"], 3, 127)}
M, N, K = 37, 48, 64
DENORMAL_COLUMN, NAN_COLUMN = N - 1, N - 2


@functools.lru_cache(maxsize=None)
def product_case(a_dtype, form, m=M, n=N, k=K, seed=0):
    """The operands of one product whose float32 result x spreads over ``form``'s domain and past both ends.  Rows 0 and 1 of the
    activations hold the zero point, so there x is the bias exactly: the bias holds ``form``'s rounding ties t (x = t with a zero
    residual) and t / 2 (x + r = t, an exact sum, with a float32 residual of t / 2).  One bias entry is NaN; the last weight
    channel has a denormal scale, so its products are +-0.0 and, the bias entry being -0.0, x = -0.0 where the sum is negative."""
    scale, zp, qmin, qmax = FORMS[form]
    g = torch.Generator().manual_seed(100 + seed + (1 if a_dtype == torch.int8 else 0))
    lo, hi = (0, 256) if a_dtype == torch.uint8 else (-128, 128)
    za = 114 if a_dtype == torch.uint8 else -5
    a = torch.randint(lo, hi, (m, k), generator=g).to(a_dtype)
    a[:2] = za
    w = torch.randint(-128, 128, (n, k), generator=g).to(torch.int8)
    a_scale = 0.02
    span = scale * (qmax - qmin)
    # |sum| is about 8 * 74 * 74 * 0.7: the scales put x at about 0.8 of the span, a third of the outputs beyond an end
    w_scales = (torch.rand(n, generator=g) + 0.5) * float(0.8 * span / (a_scale * 8 * 74 * 74 * 0.7))
    w_scales[DENORMAL_COLUMN] = 1e-45
    t = ties(scale)
    bias = (torch.rand(n, generator=g) - 0.5) * float(0.3 * span)
    bias[:len(t)] = torch.tensor(np.array(t, dtype=F32))
    bias[len(t):2 * len(t)] = torch.tensor(np.array(t, dtype=F32) / F32(2))
    bias[NAN_COLUMN], bias[DENORMAL_COLUMN] = float("nan"), -0.0
    assert 2 * len(t) < NAN_COLUMN
    return dict(a=a, za=za, a_scale=a_scale, w=w, w_scales=w_scales.float().contiguous(),
                w_rowsum=w.sum(dim=1, dtype=torch.int32).contiguous(), bias=bias.float().contiguous(), n_ties=len(t))


@functools.lru_cache(maxsize=None)
def residual_operand(r_dtype, end, form, n_ties, m=M, n=N, seed=0):
    """(residual [m, n], (scale, zero_point) or None).  Codes cover their whole domain, both ends included, and are the zero
    point in rows 0 and 1 (a zero residual); a float32 residual is zero in row 0's tie columns, t / 2 in the t / 2 columns, -0.0
    in the denormal column, and holds an infinity."""
    g = torch.Generator().manual_seed(7 + seed)
    scale, zp, qmin, qmax = FORMS[form]
    if r_dtype == torch.float32:
        r = (torch.rand(m, n, generator=g) - 0.5) * float(scale * (qmax - qmin))
        r[:2, :n_ties] = 0.0
        r[:2, n_ties:2 * n_ties] = torch.tensor(np.array(ties(scale), dtype=F32) / F32(2))
        r[:, DENORMAL_COLUMN] = -0.0
        r[5, 5], r[6, 6] = float("inf"), float("-inf")
        return r.contiguous(), None
    r_scale, r_zp = R_FORMS[(r_dtype, end)]
    lo, hi = (0, 256) if r_dtype == torch.uint8 else (-128, 128)
    r = torch.randint(lo, hi, (m, n), generator=g).to(r_dtype)
    r[:2] = r_zp
    r[2, 0], r[2, 1] = lo, hi - 1
    return r.contiguous(), (r_scale, r_zp)


def call(case, out_codes=None, **kw):
    from mct_quantizers_amd import consumers
    bias = kw.pop("bias", case["bias"])
    return consumers.qlinear_i8(case["a"], case["za"], case["a_scale"], case["w"], case["w_scales"], case["w_rowsum"], bias,
                                out_codes, **kw)


def composed_codes(case, out_codes, residual, residual_codes, relu, bias="case"):
    """The launches the fused form replaces, on the CPU: the float32 product, then the join -- its codes as int32 (a narrowed
    clamp is the join with that clamp as its domain, whose code TYPE may differ)."""
    from mct_quantizers_amd.hip import ops
    x = call(case, bias=case["bias"] if bias == "case" else bias)
    scale, zp, qmin, qmax = out_codes[:4]
    lo, hi = out_codes[4:] if len(out_codes) == 6 else (qmin, qmax)
    kw = dict(residual=residual) if residual_codes is None else dict(residual_codes=(residual, *residual_codes))
    return ops.fq_join(x, scale, zp, lo, hi, relu=relu, want_float=False, want_codes=True, **kw)[1].to(torch.int32), x


@pytest.mark.parametrize("a_dtype", [torch.uint8, torch.int8])
@pytest.mark.parametrize("r_dtype,end", RESIDUALS)
@pytest.mark.parametrize("relu", [False, True])
def test_qlinear_i8_with_a_residual_is_the_product_and_the_join_on_cpu(a_dtype, r_dtype, end, relu):
    from mct_quantizers_amd.hip import ops
    for name, out_codes in OUT_FORMS.items():
        form = name.split()[0]
        scale, zp, qmin, qmax = FORMS[form]
        case = product_case(a_dtype, form)
        residual, rc = residual_operand(r_dtype, end, form, case["n_ties"])
        for bias in (case["bias"], None):
            got = call(case, out_codes, bias=bias, residual=residual, residual_codes=rc, relu=relu)
            want, x = composed_codes(case, out_codes, residual, rc, relu, bias)
            assert got.dtype == ops._code_dtype(qmin, qmax)[0] and got.shape == (M, N)
            assert torch.equal(got.to(torch.int32), want), (name, bias is None, int((got.to(torch.int32) != want).sum()))
        # the case holds what it claims (with the bias): ties, both ends of the clamp, a NaN column, negative sums under the ReLU
        got = call(case, out_codes, residual=residual, residual_codes=rc, relu=relu)
        x = call(case)
        v = x + (residual if rc is None else ops.dequantize_codes(residual, *rc))
        lo, hi = out_codes[4:] if len(out_codes) == 6 else (qmin, qmax)
        assert int(got.min()) == lo and int(got.max()) == hi and bool((got[:, NAN_COLUMN] == lo).all())
        assert bool(torch.isnan(v[:, NAN_COLUMN]).all()) and bool((v < 0).any())
        p = (torch.relu(v) if relu else v)[:2] * (torch.tensor(1.0) / torch.tensor(scale, dtype=torch.float32))
        assert int((p - torch.floor(p) == 0.5).sum()) >= (12 if rc is None else 6) * (1 if relu else 2) // 2, name
        if relu and len(out_codes) == 4:
            at_zero = torch.clamp(torch.tensor(zp), qmin, qmax)
            assert bool((got[(v < 0)] == at_zero).all())
        if rc is not None:
            r_lo, r_hi = (0, 255) if r_dtype == torch.uint8 else (-128, 127)
            assert int(residual.min()) == r_lo and int(residual.max()) == r_hi and rc[1] in (r_lo, r_hi)


@pytest.mark.parametrize("a_dtype", [torch.uint8, torch.int8])
@pytest.mark.parametrize("r_dtype,end", RESIDUALS)
@pytest.mark.parametrize("relu", [False, True])
def test_qlinear_i8_with_a_residual_in_float32_on_cpu(a_dtype, r_dtype, end, relu):
    """The float32 output form: x + r, one float32 add, then v < 0 ? 0 : v -- a NaN stays a NaN and -0.0 stays -0.0."""
    from mct_quantizers_amd.hip import ops
    case = product_case(a_dtype, "u8")
    residual, rc = residual_operand(r_dtype, end, "u8", case["n_ties"])
    x = call(case)
    v = x + (residual if rc is None else ops.dequantize_codes(residual, *rc))
    want = torch.where(v < 0, torch.zeros(()), v) if relu else v
    got = call(case, None, residual=residual, residual_codes=rc, relu=relu)
    assert got.dtype == torch.float32 and bits_equal(got.numpy(), want.numpy()), first_mismatch(got.numpy(), want.numpy())
    assert bool(torch.isnan(got[:, NAN_COLUMN]).all()) and bool(torch.isinf(got).any()) == (rc is None)
    column = got[:, DENORMAL_COLUMN].numpy()
    if rc is None:                                       # (a residual given as codes is never -0.0: fma(d, s, +0))
        assert np.signbit(x[:, DENORMAL_COLUMN].numpy()).any() and not np.signbit(x[:2, DENORMAL_COLUMN].numpy()).any()
        assert np.array_equal(np.signbit(column), np.signbit(x[:, DENORMAL_COLUMN].numpy())) and np.all(column == 0.0)
    if relu:
        assert not bool((got < 0).any()) and bool((v < 0).any())


def test_qlinear_i8_residual_arguments():
    from mct_quantizers_amd import consumers
    case = product_case(torch.uint8, "u8")
    r32, _ = residual_operand(torch.float32, None, "u8", case["n_ties"])
    r8, rc = residual_operand(torch.uint8, "lo", "u8", case["n_ties"])
    with pytest.raises(ValueError):
        call(case, relu=True)                                              # a ReLU without a residual
    with pytest.raises(ValueError):
        call(case, residual_codes=rc)
    with pytest.raises(ValueError):
        call(case, residual=r8)                                            # codes without their form
    with pytest.raises(ValueError):
        call(case, residual=r32, residual_codes=rc)                        # float32 with one
    with pytest.raises(NotImplementedError):
        call(case, residual=r32, w_zero_points=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(TypeError):
        call(case, residual=r32.double())
    with pytest.raises(RuntimeError):
        call(case, residual=r32[:, :-1])
    for bad in ((0.19, 256), (0.19, -1), (0.0, 3), (float("inf"), 3), (float("nan"), 3)):
        with pytest.raises(ValueError):
            call(case, residual=r8, residual_codes=bad)
    # without the keywords the call is what it was
    assert bits_equal(call(case).numpy(), call(case, residual=None, residual_codes=None, relu=False).numpy())
    assert consumers.qlinear_i8.__defaults__[-3:] == (None, None, False)


# ---- the modules ----------------------------------------------------------------------------------------------------------

def test_consumer_modules_take_a_residual():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops
    form = FORMS["u8"]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16, 5, 7, generator=g) * 1.5
    for k, cls in ((1, consumers.QuantizedConv1x1), (3, consumers.QuantizedConv2d)):
        holder, wrapper = conv_pair(C=16, O=32, k=k, padding=k // 2, seed=4)
        fused = cls.from_wrapper(wrapper, holder.activation_holder_quantizer)
        y = fused(x)
        with pytest.raises(RuntimeError):
            fused(x, torch.zeros_like(y))                                   # built without a residual
        r32 = torch.randn(2, 32, 5, 7, generator=g)
        rc8 = torch.randint(0, 256, (2, 32, 5, 7), generator=g).to(torch.uint8)
        for residual, how, relu in ((r32, "float", True), (rc8, (0.19, 101), True), (rc8, (0.19, 101), False)):
            fused.emit_codes_for, fused.emit_residual, fused.emit_relu = form, how, relu
            kw = dict(residual=residual) if how == "float" else dict(residual_codes=(residual, *how))
            want = ops.fq_join(y, *form, relu=relu, want_float=False, **kw)[1]
            for r in (residual, residual.contiguous(memory_format=torch.channels_last)):
                got = fused(x, r)
                assert got.shape == want.shape and torch.equal(got, want) and got.permute(0, 2, 3, 1).is_contiguous()
            with pytest.raises(RuntimeError):
                fused(x)                                                    # built with one
            with pytest.raises(TypeError):
                fused(x, r32 if how != "float" else rc8)                    # the other kind of residual
        fused.emit_codes_for, fused.emit_residual, fused.emit_relu = None, "float", False
        assert bits_equal(fused(x, r32).numpy(), (y + r32).numpy())         # float32 out
    holder, wrapper = conv_pair(C=16, O=32, k=1, padding=0, seed=4)
    linear = torch.nn.Linear(16, 32)
    import mct_quantizers_amd as mq
    from test_conv_consumer import weights_quantizer
    wrapped = mq.PytorchQuantizationWrapper(linear, {"weight": weights_quantizer(linear.weight, "sym", True)})
    fused = consumers.QuantizedLinear.from_wrapper(wrapped, holder.activation_holder_quantizer)
    rows, r = torch.randn(3, 5, 16, generator=g), torch.randn(3, 5, 32, generator=g)
    y = fused(rows)
    fused.emit_residual, fused.emit_relu = "float", True
    assert bits_equal(fused(rows, r).numpy(), torch.relu(y + r).numpy()) and fused(rows, r).shape == (3, 5, 32)


# ---- the rewritten graphs ---------------------------------------------------------------------------------------------------

SWITCHES = dict(convolutions=True, shared_holders=True, stay_on_codes=True)


def rewrite(make, device="cpu", **switches):
    """(with ``fused_residuals``, without) of a fresh model each; the same seeds build the same weights."""
    from mct_quantizers_amd import consumers
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = make().to(device), make().to(device)
    switches = dict(SWITCHES, **switches)
    gm, n = consumers.fuse_linear_consumers_fx(a, fused_residuals=True, **switches)
    gm0, n0 = consumers.fuse_linear_consumers_fx(b, **switches)
    assert n == n0
    return gm, gm0


def test_four_block_stack_graph_with_fused_residuals():
    from mct_quantizers_amd import consumers
    gm, gm0 = rewrite(FourBlocks)
    assert sorted(_joins(gm0)) == ["A_a3_1_join", "B_a3_1_join", "C_a3_1_join", "h0_join"]
    # C's join writes float32 for the last block's plain add: it stays
    assert sorted(_joins(gm)) == ["C_a3_1_join", "h0_join"]
    assert _targets(gm) == [t for t in _targets(gm0) if t not in ("A_a3_1_join", "B_a3_1_join")]
    nodes = {n.target: n for n in gm.graph.nodes if n.op == "call_module"}
    h0_codes = next(iter(nodes["h0_join"].users))
    assert h0_codes.target is operator.getitem and h0_codes.args == (nodes["h0_join"], 1)
    # the downsample branch, evaluated last, takes c3's float32 output as its residual and emits the codes of A's holder
    down, a_join = gm.get_submodule("A_down_qlinear"), gm0.get_submodule("A_a3_1_join")
    assert nodes["A_down_qlinear"].args == (h0_codes, nodes["A_c3_qlinear"])
    a_form = (a_join._a_scale, a_join._a_zp, a_join._a_qmin, a_join._a_qmax)
    assert (down.emit_residual, down.emit_relu, down.emit_codes_for, down.emit_clamp) == ("float", True, a_form, None)
    c3 = gm.get_submodule("A_c3_qlinear")
    assert (c3.emit_residual, c3.emit_relu, c3.emit_codes_for) == (None, False, None)
    # B's c3 takes those codes, as A's holder's
    b_c3, b_join = gm.get_submodule("B_c3_qlinear"), gm0.get_submodule("B_a3_1_join")
    assert nodes["B_c3_qlinear"].args == (nodes["B_c2_qlinear"], nodes["A_down_qlinear"])
    assert b_c3.emit_residual == (a_join._a_scale, a_join._a_zp) == b_join.residual_codes and b_c3.emit_relu is True
    assert b_c3.emit_codes_for == (b_join._a_scale, b_join._a_zp, b_join._a_qmin, b_join._a_qmax)
    assert sorted(u.target for u in nodes["A_down_qlinear"].users) == ["B_c1_qlinear", "B_c3_qlinear"]
    assert sorted(u.target for u in nodes["B_c3_qlinear"].users) == ["C_a3_1_join", "C_c1_qlinear"]
    c_join = gm.get_submodule("C_a3_1_join")
    assert nodes["C_a3_1_join"].args == (nodes["C_c3_qlinear"], nodes["B_c3_qlinear"])
    assert (c_join.want_float, c_join.residual_codes) == (True, (b_join._a_scale, b_join._a_zp))
    assert gm.get_submodule("C_c3_qlinear").emit_residual is None and gm.get_submodule("D_c3_qlinear").emit_residual is None
    with_residual = [name for name, m in gm.named_modules() if isinstance(m, consumers.IntegerConsumer) and m.emit_residual is not None]
    assert with_residual == ["A_down_qlinear", "B_c3_qlinear"]
    # a second trace changes nothing
    again, n = consumers.fuse_linear_consumers_fx(gm, fused_residuals=True, **SWITCHES)
    shape = lambda g: [(nd.op, str(nd.target), [str(getattr(a, "target", a)) for a in nd.args]) for nd in g.graph.nodes]   # noqa: E731
    assert n == 0 and shape(again) == shape(gm) and sorted(_joins(again)) == sorted(_joins(gm))
    again_b = again.get_submodule("B_c3_qlinear")
    assert (again_b.emit_residual, again_b.emit_relu, again_b.emit_codes_for) == (b_c3.emit_residual, True, b_c3.emit_codes_for)


class DownFirst(torch.nn.Module):
    """A block that evaluates its downsample branch FIRST: then c3 is the later operand and takes the branch's float32 output."""

    def __init__(self):
        super().__init__()
        self.h0 = _holder("uniform")
        self.A = _Block(16, 16, 32, 2, True, 10)
        self.B = _Block(32, 16, 32, 1, False, 20)
        self.C = _Block(32, 16, 32, 1, False, 30)       # (its add stays plain, so B's join writes float32 and stays)
        with torch.no_grad():
            for block in (self.B, self.C):
                block.c3.weight.mul_(0.1)
                block.c3.layer.bias.mul_(0.1)

    def forward(self, x):
        x = self.h0(x)
        A = self.A
        identity = A.down(x)
        y = A.c3(A.a2(A.c2(A.a1(A.c1(x)))))
        return self.C(self.B(A.a3(identity + y)))


def test_a_downsample_first_block_fuses_into_c3():
    gm, gm0 = rewrite(DownFirst)
    assert sorted(_joins(gm0)) == ["A_a3_1_join", "B_a3_1_join", "h0_join"] and sorted(_joins(gm)) == ["B_a3_1_join", "h0_join"]
    nodes = {n.target: n for n in gm.graph.nodes if n.op == "call_module"}
    assert nodes["A_c3_qlinear"].args == (nodes["A_c2_qlinear"], nodes["A_down_qlinear"])
    c3, down = gm.get_submodule("A_c3_qlinear"), gm.get_submodule("A_down_qlinear")
    assert (c3.emit_residual, c3.emit_relu, down.emit_residual, down.emit_codes_for) == ("float", True, None, None)
    x = block_input()
    assert bits_equal(gm(x).numpy(), gm0(x).numpy())


class InvertedStack(torch.nn.Module):
    """Two MobileNetV2 blocks with an identity, a holder behind each add, and a last convolution: the holders behind the adds
    become residual joins that write codes only, the second reading the first one's codes."""

    def __init__(self, C=16, E=32, uniform_project=False):
        super().__init__()
        self.h0 = _holder("uniform")
        for b, seed in (("a", 1), ("b", 5)):
            setattr(self, f"{b}1", conv_pair(C=C, O=E, k=1, padding=0, seed=seed)[1])
            h2, c2 = conv_pair(C=E, O=E, k=3, padding=1, groups=E, seed=seed + 1, act="relu")
            h3, c3 = conv_pair(C=E, O=C, k=1, padding=0, seed=seed + 2, act="relu", family="uniform" if uniform_project else "sym")
            for name, m in (("h2", h2), ("2", c2), ("h3", h3), ("3", c3)):
                setattr(self, b + name, m)
            setattr(self, f"{b}_out", _holder("uniform"))
        with torch.no_grad():
            self.a3.weight.mul_(0.05)
            self.b3.weight.mul_(0.05)
        self.last = conv_pair(C=C, O=24, k=1, padding=0, seed=9)[1]

    def block(self, b, x):
        relu6, get = torch.nn.functional.relu6, lambda name: getattr(self, b + name)       # noqa: E731
        y = relu6(get("1")(x))
        y = relu6(get("2")(get("h2")(y)))
        return get("_out")(x + get("3")(get("h3")(y)))

    def forward(self, x):
        return self.last(self.block("b", self.block("a", self.h0(x))))


INVERTED = dict(convolutions=False, depthwise=True)
RESIDUAL_MODELS = {"four blocks": (FourBlocks, {}, 2), "down first": (DownFirst, {}, 1), "inverted stack": (InvertedStack, INVERTED, 2)}


def test_inverted_residual_stack_graph():
    gm, gm0 = rewrite(InvertedStack, **INVERTED)
    assert sorted(_joins(gm0)) == ["a_out_join", "b_out_join", "h0_join"] and sorted(_joins(gm)) == ["h0_join"]
    assert all(not j.want_float and j.residual_codes is not None for name, j in _joins(gm0).items() if name != "h0_join")
    a3, b3 = gm.get_submodule("a3_qlinear"), gm.get_submodule("b3_qlinear")
    h0, a_out = gm0.get_submodule("h0_join"), gm0.get_submodule("a_out_join")
    assert a3.emit_residual == (h0._a_scale, h0._a_zp) and b3.emit_residual == (a_out._a_scale, a_out._a_zp)
    assert (a3.emit_relu, b3.emit_relu) == (False, False)
    assert not [t for t in _targets(gm, "call_function") if t is operator.add]


def check_bits_against_the_rewrite_without(name, device, channels_last):
    make, switches, removed = RESIDUAL_MODELS[name]
    gm, gm0 = rewrite(make, device, **switches)
    assert len(_joins(gm0)) - len(_joins(gm)) == removed
    x = block_input(device, channels_last)
    y, y0 = gm(x), gm0(x)
    assert y.dtype == torch.float32 and y.shape == y0.shape and len(torch.unique(y)) > 50
    assert bits_equal(y.cpu().numpy(), y0.cpu().numpy()), first_mismatch(y.cpu().numpy(), y0.cpu().numpy())
    with torch.no_grad():                                 # an in-place weight update: both models refresh their codes
        for g in (gm, gm0):
            for m in g.modules():
                if hasattr(m, "_refresh_weight_codes"):
                    m.weight.mul_(0.75)
    y2, y02 = gm(x), gm0(x)
    assert bits_equal(y2.cpu().numpy(), y02.cpu().numpy()) and not torch.equal(y2, y)
    return y, y2


@pytest.mark.parametrize("name", list(RESIDUAL_MODELS))
def test_rewritten_models_give_the_bits_of_the_rewrite_without_on_cpu(name):
    y, y2 = check_bits_against_the_rewrite_without(name, "cpu", False)
    yc, yc2 = check_bits_against_the_rewrite_without(name, "cpu", True)
    assert bits_equal(y.numpy(), yc.numpy()) and bits_equal(y2.numpy(), yc2.numpy())


# ---- guard rails ------------------------------------------------------------------------------------------------------------

def test_fused_residuals_needs_stay_on_codes():
    from mct_quantizers_amd import consumers
    for switches in (dict(), dict(convolutions=True, shared_holders=True), dict(shared_holders=True, pools=True)):
        with pytest.raises(ValueError):
            consumers.fuse_linear_consumers_fx(FourBlocks(), fused_residuals=True, **switches)
    with pytest.raises(TypeError):
        consumers.fuse_linear_consumers(torch.nn.Sequential(), fused_residuals=True)     # no adds, no switch


def test_without_the_keyword_nothing_changes():
    from mct_quantizers_amd import consumers
    x = block_input()
    for name, (make, switches) in MODELS.items():
        kw = dict(switches, stay_on_codes=True)
        gm, n = consumers.fuse_linear_consumers_fx(make(), **kw)
        gm_off, n_off = consumers.fuse_linear_consumers_fx(make(), fused_residuals=False, **kw)
        assert n == n_off and str(gm.graph) == str(gm_off.graph) and gm.code == gm_off.code
        assert all(m.emit_residual is None and m.emit_relu is False for m in gm.modules() if isinstance(m, consumers.IntegerConsumer))
        assert bits_equal(gm(x).numpy(), gm_off(x).numpy())
    targets = _targets(consumers.fuse_linear_consumers_fx(FourBlocks(), **SWITCHES)[0])
    assert [t for t in targets if t.endswith("_join")] == ["h0_join", "A_a3_1_join", "B_a3_1_join", "C_a3_1_join"]


def test_producers_that_keep_their_join():
    """A uniform-weights product (its kernel form has no residual) and a depthwise one (its own kernel) in front of the join."""
    from mct_quantizers_amd import consumers
    gm, gm0 = rewrite(lambda: InvertedStack(uniform_project=True), uniform_weights=True, **INVERTED)
    assert sorted(_joins(gm)) == sorted(_joins(gm0)) == ["a_out_join", "b_out_join", "h0_join"]
    assert str(gm.graph) == str(gm0.graph)

    class DepthwiseProject(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.h0 = _holder("uniform")
            self.h1, self.dw = conv_pair(C=16, O=16, k=3, padding=1, groups=16, seed=2)
            self.out = _holder("uniform")
            self.c1, self.c2 = conv_pair(C=16, O=16, k=1, padding=0, seed=3)[1], conv_pair(C=16, O=16, k=1, padding=0, seed=4)[1]

        def forward(self, x):
            x = self.h0(x)
            y = self.out(x + self.dw(x))
            return self.c1(y) + self.c2(y)

    gm, gm0 = rewrite(DepthwiseProject, **INVERTED)
    assert "out_join" in _joins(gm) and str(gm.graph) == str(gm0.graph)
    join = gm.get_submodule("out_join")
    assert join.has_residual and not join.want_float
    assert isinstance(gm.get_submodule("dw_qlinear"), consumers.QuantizedDepthwiseConv2d)
    assert gm.get_submodule("dw_qlinear").emit_residual is None


def test_wrapped_resnet50_structure_with_fused_residuals():
    """Trace and rewrite only: of the 15 residual joins the 14 that write codes only go (tests/test_stay_on_codes.py counts
    them); the 15th feeds the last block's plain add in float32 and stays, as does the ReLU-only join behind the first c1."""
    from mct_quantizers_amd import consumers, workloads
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True)
    gm0, n0 = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu"), **switches)
    gm, n = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(device="cpu"), fused_residuals=True, **switches)
    joins0, joins = _joins(gm0), _joins(gm)
    fusable = [t for t, j in joins0.items() if j.has_residual and not j.want_float]
    assert n == n0 and len(joins0) - len(joins) == len(fusable) and not set(fusable) & set(joins)
    assert not [t for t, j in joins.items() if j.has_residual and not j.want_float]
    assert [t for t, j in joins.items() if j.has_residual] == ["17_a3_1_join"] and joins["17_a3_1_join"].want_float
    fused = [m for m in gm.modules() if isinstance(m, consumers.IntegerConsumer) and m.emit_residual is not None]
    assert len(fused) == len(fusable) and all(m.emit_relu and m.emit_codes_for is not None for m in fused)
    assert sum(m.emit_residual == "float" for m in fused) == sum(joins0[t].residual_codes is None for t in fusable)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------

def test_qlinear_i8_res_argument_validation_needs_no_gpu():
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    lib = native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mctq_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmctq_qlinear_i8_res\s*\(", header) and "mctq_qlinear_i8_res" in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    E, P, R, I8, U8 = native.MCTQ_E_ARG, 4096, 1 << 20, native.CODE_I8, native.CODE_U8    # aligned addresses, never dereferenced
    count = lib.mctq_launch_count()
    valid = dict(a=P, adt=U8, za=3, sa=0.5, w=P, w_scales=P, w_rowsum=P, bias=None, r=R, rdt=U8, rs=0.25, rz=3, relu=1, y=P,
                 ydt=U8, y_scale=0.25, y_zp=0, qmin=0, qmax=255, M=4, N=8, K=64)

    def call(**over):
        v = dict(valid, **over)
        return lib.mctq_qlinear_i8_res(v["a"], v["adt"], v["za"], v["sa"], v["w"], v["w_scales"], v["w_rowsum"], v["bias"], v["r"],
                                       v["rdt"], v["rs"], v["rz"], v["relu"], v["y"], v["ydt"], v["y_scale"], v["y_zp"], v["qmin"],
                                       v["qmax"], v["M"], v["N"], v["K"], None)

    def refused(message, **fault):
        assert call(**fault) == E, fault
        assert lib.mctq_last_error() == message, (fault, lib.mctq_last_error())

    refused(b"residual is NULL", r=None)
    refused(b"residual is NULL", r=None, rdt=-1)
    for rdt in (2, 3, 77):                                                 # the 4-bit code types among them
        refused(b"bad r_code_dtype", rdt=rdt)
    for rdt, rz in ((I8, -129), (I8, 128), (U8, -1), (U8, 256)):
        refused(b"r_zero_point is no code of the residual's type", rdt=rdt, rz=rz)
    for rs in (0.0, -0.5, float("inf"), float("nan")):
        refused(b"r_scale must be finite and positive", rs=rs)
    # wrong in two ways: the output's form, then the residual's code type, its zero point, its scale, then the overlap
    refused(b"bad y_code_dtype", ydt=9, r=None)
    refused(b"bad r_code_dtype", rdt=77, rz=256)
    refused(b"r_zero_point is no code of the residual's type", rz=256, rs=0.0)
    refused(b"r_scale must be finite and positive", rs=0.0, r=P)
    for off in (1, 2, 3):
        refused(b"a float32 residual must be 4-byte aligned", rdt=-1, r=R + off)
    # y [4][8] overlapping the residual: the byte ranges, each in its own element size
    for ydt, rdt, r in ((U8, U8, P), (U8, U8, P + 31), (U8, U8, P - 31), (-1, -1, P + 124), (-1, U8, P + 127), (U8, -1, P - 124)):
        refused(b"y overlaps the residual", ydt=ydt, rdt=rdt, r=r)
    # ... and everything the other consumer entry points refuse
    refused(b"negative extent", M=-1)
    refused(b"bad a_code_dtype", adt=77)
    refused(b"K must be a multiple of 16", K=24)
    refused(b"NULL pointer", y=None)
    refused(b"code matrices must be 16-byte aligned", a=P + 1)
    refused(b"bad y_code_dtype", ydt=9)
    refused(b"clamp domain does not fit the code type", qmax=256)
    # the register-pinned whole-tile kernels are not built for a residual
    try:
        for variant in (2544, 2548, 2560):
            assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
            assert call(M=256, N=256, K=256) == E
            assert b"residual" in lib.mctq_last_error() and b"2544 / 2548 / 2560" in lib.mctq_last_error()
    finally:
        assert lib.mctq_set_tuning(b"ql_variant", 0) == 0
    # empty problems: nothing is looked at, nothing is launched
    nothing = dict(a=None, w=None, w_scales=None, w_rowsum=None, y=None, r=None)
    assert call(M=0, **nothing) == 0 and call(N=0, **nothing) == 0 and call(M=0, rdt=77, rs=-1.0, **nothing) == 0
    assert call(M=0, ydt=-1, rdt=-1, **nothing) == 0
    assert lib.mctq_launch_count() == count                                # refused and empty calls launch nothing
