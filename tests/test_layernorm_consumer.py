"""LayerNorm on codes on the CPU: ops.codes_layernorm against a float64 LayerNorm and against a direct loop over the contract's
lines, and the ``layernorms`` switch of fuse_linear_consumers_fx on the encoder block (consumers.QuantizedLayerNorm)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mct_quantizers_amd as mq
from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import ops

Q = mq.pytorch_quantizers
FORMS = [(2.0 ** -5, 0, torch.int8), (0.0731, -7, torch.int8), (0.0213, 113, torch.uint8)]
OUT_FORM = (8.0 / 128, 3, -128, 127)
EPS = 1e-5
SWITCHES = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True, activation_tables=True)


def _case(rows, L, dtype, seed):
    """Random codes, gamma and beta; row 0 constant, row 1 the least code with the greatest at its end."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (0, 255) if dtype == torch.uint8 else (-128, 127)
    codes = torch.randint(lo, hi + 1, (rows, L), generator=g, dtype=torch.int16)
    codes[0] = 41
    codes[1], codes[1, -1] = lo, hi
    return codes.to(dtype), 1.0 + 0.5 * torch.randn(L, generator=g), 0.3 * torch.randn(L, generator=g)


@pytest.mark.parametrize("L", [16, 768, 8192])
@pytest.mark.parametrize("scale,zp,dtype", FORMS)
def test_codes_layernorm_against_float64(L, scale, zp, dtype):
    """Every code within one of a float64 LayerNorm of the dequantized codes, and off only within its row's delta of a rounding
    tie.  delta is derived, per row: the contract has five float32 roundings (r, n * r, * gamma, + beta, * inv) of at most 2^-24 relative each, on
    values of at most |xh gamma| + |beta| (+ |zp_b| s_b behind the last), so 8 * 2^-24 of that, in codes, bounds their sum."""
    codes, gamma, beta = _case(24, L, dtype, L)
    got = ops.codes_layernorm(codes, (scale, zp), OUT_FORM, gamma, beta, EPS)
    assert got.shape == codes.shape and got.dtype == torch.int8
    s_b, zp_b, qmin, qmax = OUT_FORM
    x = (codes.numpy().astype(np.float64) - zp) * np.float64(np.float32(scale))
    xh = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + EPS)
    q = (xh * gamma.numpy().astype(np.float64) + beta.numpy().astype(np.float64)) / np.float64(np.float32(s_b)) + zp_b
    diff = np.abs(got.numpy().astype(np.int64) - np.clip(np.rint(q), qmin, qmax))
    delta = 8 * 2.0 ** -24 * (np.abs(xh * gamma.numpy()) + np.abs(beta.numpy()) + abs(zp_b) * s_b).max(-1, keepdims=True) / s_b
    off = diff > 0
    tie = np.abs(np.abs(q[off] - np.floor(q[off])) - 0.5)
    print(f"max difference {diff.max()}, elements that differ {int(off.sum())} of {diff.size}, each row's delta {delta.min():.3g} .. "
          f"{delta.max():.3g}, distances to a tie {tie.tolist()}")
    assert diff.max() <= 1 and (tie <= np.broadcast_to(delta, q.shape)[off]).all()
    # the constant row: V = 0, r = 1 / sqrt(K), every n_j = 0 and every code is beta's
    want = torch.clamp(torch.round(beta * (torch.tensor(1.0) / torch.tensor(s_b))) + zp_b, qmin, qmax).to(torch.int8)
    assert torch.equal(got[0], want)


def test_cpu_route_equals_a_direct_loop_over_the_contract():
    (scale, zp, dtype), L = FORMS[1], 48
    codes, gamma, beta = _case(4, L, dtype, 7)
    got = ops.codes_layernorm(codes, (scale, zp), OUT_FORM, gamma, beta, EPS)
    k = np.float64(EPS) * L * L / np.float64(np.float32(scale)) ** 2
    inv = np.float32(1.0) / np.float32(OUT_FORM[0])
    for row, out in zip(codes.tolist(), got.tolist()):
        u = [c - zp for c in row]
        s1, s2 = sum(u), sum(v * v for v in u)
        r = np.float32(1.0 / np.sqrt(np.float64(L * s2 - s1 * s1) + k))
        for j in range(L):
            y = np.float32(np.float32(np.float32(L * u[j] - s1) * r) * np.float32(gamma[j])) + np.float32(beta[j])
            assert out[j] == int(min(max(np.rint(np.float32(y * inv)) + OUT_FORM[1], OUT_FORM[2]), OUT_FORM[3]))


@pytest.mark.parametrize("uniform", [False, True])
def test_rewrite_of_the_encoder_block(uniform):
    """Chosen assertion: ``torch.equal`` between the rewrite with and without ``layernorms`` on a seeded input that keeps every
    norm output away from a rounding tie (every product of this block is exact, so nothing else can differ)."""
    x = torch.randn(3, 17, 64, generator=torch.Generator().manual_seed(11)) * 1.5
    gm, n = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(uniform=uniform), layernorms=True, **SWITCHES)
    base, n_base = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(uniform=uniform), **SWITCHES)
    norms = {name for name, m in gm.named_modules() if isinstance(m, consumers.QuantizedLayerNorm)}
    assert norms == {"attn_a_in_layernorm", "a_n2_layernorm"} and n == n_base == 6
    assert not any(isinstance(m, consumers.QuantizedLayerNorm) for m in base.modules())
    readers = {node.target: [type(gm.get_submodule(u.target)) for u in node.users] for node in gm.graph.nodes if node.target in norms}
    assert readers == {"attn_a_in_layernorm": [consumers.QuantizedLinear] * 3, "a_n2_layernorm": [consumers.QuantizedLinear]}
    seen = []
    gm.a_n2_layernorm.register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.dtype)))
    y, want = gm(x), base(x)
    step = consumers._code_form(gm.a_out.activation_holder_quantizer)[0]
    print(f"equal {torch.equal(y, want)}, max difference {((y - want).abs().max() / step).item()} steps")
    assert seen == [(torch.uint8 if uniform else torch.int8,) * 2]                # the join in front hands over its codes
    assert torch.equal(y, want) and len(y.unique()) > 100


class _Variant(nn.Module):
    """[holder A ->] LayerNorm -> holder B -> Linear, one of the forms the rewrite leaves alone."""

    def __init__(self, variant):
        super().__init__()
        self.variant = variant
        holder = lambda: mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(8, [4.0], True))   # noqa: E731
        self.a, self.b = holder(), holder()
        self.norm = nn.LayerNorm((4, 16) if variant == "two dimensions" else 16, eps=0.0 if variant == "eps" else 1e-5)
        self.fc = mq.PytorchQuantizationWrapper(nn.Linear(16, 16), {"weight": Q.WeightsPOTInferableQuantizer(
            num_bits=8, threshold=[1.0] * 16, per_channel=True, channel_axis=0)})

        self.register_buffer("gain", torch.full((16,), 1.5))

    def forward(self, x):
        x = x if self.variant == "no holder A" else self.a(x)
        if self.variant.startswith("functional"):                                  # F.layer_norm on the module's Parameters, or on a buffer
            weight = self.gain if self.variant == "functional, a buffer" else self.norm.weight
            p = self.b(nn.functional.layer_norm(x, (16,), weight, bias=self.norm.bias, eps=1e-5))
        else:
            p = self.b(self.norm(x))
        return self.fc(p) + p if self.variant == "float user" else self.fc(p)


@pytest.mark.parametrize("variant", ["taken", "functional", "functional, a buffer", "float user", "no holder A", "eps", "two dimensions"])
def test_variants_taken_and_left_alone(variant):
    model, x = _Variant(variant).eval(), torch.randn(2, 4, 16, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        model.norm.weight.copy_(torch.linspace(0.5, 1.5, 16).expand_as(model.norm.weight))
    gm, _ = consumers.fuse_linear_consumers_fx(model, layernorms=True)
    assert any(isinstance(m, consumers.QuantizedLayerNorm) for m in gm.modules()) == (variant in ("taken", "functional"))
    # a code of B is 1 / 32 and nn.Linear(16, 16) draws |w| <= 1 / 4: at most 16 / 128 through the layer, 1 / 32 beside it
    assert (gm(x) - model(x)).abs().max() <= 0.16
