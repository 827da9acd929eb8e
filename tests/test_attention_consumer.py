"""The fused attention consumer on the CPU: the graph rewrite, and ``qattention_i8`` against a float64 reference."""
import pytest
import torch

from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import ops

SWITCHES = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True)


def _count(gm, cls):
    return sum(isinstance(m, cls) for m in gm.modules())


@pytest.mark.parametrize("fused_qkv", [False, True])
@pytest.mark.parametrize("uniform", [False, True])
def test_rewrite_makes_one_attention_node_with_the_same_output(fused_qkv, uniform):
    x = torch.randn(2, 17, 64, generator=torch.Generator().manual_seed(3))
    block = lambda: workloads.wrapped_attention_block(fused_qkv=fused_qkv, uniform=uniform)        # noqa: E731
    plain, replaced = consumers.fuse_linear_consumers_fx(block(), **SWITCHES)
    fused, replaced_too = consumers.fuse_linear_consumers_fx(block(), attentions=True, **SWITCHES)
    assert replaced_too == replaced
    assert _count(plain, consumers.QuantizedMatmul) == 2 and _count(plain, consumers.QuantizedSoftmax) == 1
    assert _count(fused, consumers.QuantizedAttention) == 1
    assert _count(fused, consumers.QuantizedMatmul) == 0 and _count(fused, consumers.QuantizedSoftmax) == 0
    with torch.no_grad():
        assert torch.equal(fused(x), plain(x))


@pytest.mark.parametrize("missing", ["matmuls", "softmaxes"])
def test_rewrite_needs_both_switches(missing):
    switches = dict(SWITCHES, **{missing: False})
    with pytest.raises(ValueError, match="attentions=True needs"):
        consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(), attentions=True, **switches)


def test_rewrite_leaves_probabilities_with_a_second_reader_alone():
    gm, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(), **SWITCHES)
    soft = next(n for n in gm.graph.nodes if isinstance(gm.get_submodule(n.target) if n.op == "call_module" else None,
                                                        consumers.QuantizedSoftmax))
    out = next(n for n in gm.graph.nodes if n.op == "output")
    out.args = ((out.args[0], soft),)                              # the probabilities leave the model as well
    assert consumers._attentions_on_codes(gm, dict(gm.named_modules())) == 0
    assert _count(gm, consumers.QuantizedAttention) == 0 and _count(gm, consumers.QuantizedMatmul) == 2


def _fq64(x, form):
    """A holder in float64: ``form = (scale, zero_point, qmin, qmax)`` with a power-of-two scale."""
    scale, zp, qmin, qmax = form
    return (torch.clamp(torch.round(x / scale) + zp, qmin, qmax) - zp) * scale


@pytest.mark.parametrize("with_prefix", [False, True])
def test_qattention_against_float64(with_prefix):
    """The softmax contract keeps each probability code within one of the float64 chain's, so per element
    ``|y - ref| <= s_p * s_v * sum_k |v[k][n] - z_v|``; all scales are powers of two, so the last product adds no float32 rounding.
    Observed share of differing elements: docs/KERNEL_NOTES.md."""
    gen = torch.Generator().manual_seed(11)
    B, H, M, T, D, Dv = 2, 2, 19, 37, 16, 16
    q = torch.randint(-128, 128, (B, H, M, D), generator=gen).to(torch.int8)
    k = torch.randint(0, 256, (B, H, T, D), generator=gen).to(torch.uint8)
    v = torch.randint(-128, 128, (B, H, T, Dv), generator=gen).to(torch.int8)
    q_form, k_form, v_form = (2.0 ** -7, 3), (2.0 ** -7, 131), (2.0 ** -5, -7)
    scores_form, probs_form = (2.0 ** -3, 5, -128, 127), (2.0 ** -8, 0, 0, 255)
    a_form = (2.0 ** -5, -2, -128, 127) if with_prefix else scores_form
    prefix = (lambda s: s * D ** -0.5) if with_prefix else (lambda s: s)
    pre = ops.code_table(prefix, scores_form, a_form, "cpu") if with_prefix else None
    y = consumers.qattention_i8(q, q_form, k, k_form, v, v_form, scores_form=scores_form, a_form=a_form, probs_form=probs_form,
                                pre_table=pre)
    q64, k64 = (q.double() - q_form[1]) * q_form[0], (k.double() - k_form[1]) * k_form[0]
    v64 = (v.double() - v_form[1]) * v_form[0]
    s = _fq64(q64 @ k64.transpose(-1, -2), scores_form)
    if with_prefix:
        s = _fq64(prefix(s), a_form)
    ref = _fq64(torch.softmax(s, dim=-1), probs_form) @ v64
    bound = probs_form[0] * v_form[0] * (v.double() - v_form[1]).abs().sum(-2, keepdim=True)
    diff = (y.double() - ref).abs()
    print(f"differing elements: {(diff > 0).double().mean().item():.4f}, largest difference / bound: {(diff / bound).max().item():.4f}")
    assert y.dtype == torch.float32 and y.shape == (B, H, M, Dv)
    assert bool((diff <= bound).all())
