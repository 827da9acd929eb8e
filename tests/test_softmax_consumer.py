"""Softmax on codes on the CPU: ops.codes_softmax against a float64 reference, its edge rows and padding, and the ``softmaxes``
switch of fuse_linear_consumers_fx on the attention block (consumers.QuantizedSoftmax)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mct_quantizers_amd as mq
from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import ops

Q = mq.pytorch_quantizers
SCALES = {"pot": (2.0 ** -3, 2.0 ** -8), "odd": (0.0731, 1.0 / 255)}
SWITCHES = dict(shared_holders=True, stay_on_codes=True, matmuls=True)
BLOCK_INPUT = torch.randn(3, 17, 64, generator=torch.Generator().manual_seed(11)) * 1.5


def _reference(codes, a_scale, out_form):
    """Softmax of the dequantized A-values, coded by B, all in float64 (A's zero point cancels)."""
    s, z, lo, hi = out_form
    x = codes.numpy().astype(np.float64) * np.float64(np.float32(a_scale))
    p = np.exp(x - x.max(-1, keepdims=True))
    return np.clip(np.rint(p / p.sum(-1, keepdims=True) / np.float64(np.float32(s))) + z, lo, hi)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 197])
@pytest.mark.parametrize("in_dtype,out_form", [(torch.int8, (0, 255)), (torch.uint8, (-128, 127))])
@pytest.mark.parametrize("scales", ["pot", "odd"])
@pytest.mark.parametrize("pre", [False, True])
def test_codes_softmax_against_float64(L, in_dtype, out_form, scales, pre):
    a_scale, b_scale = SCALES[scales]
    out_form = (b_scale, out_form[0], *out_form)                                   # zero point: the domain's lower end (p >= 0)
    raw = torch.randint(0, 256, (1000, L), generator=torch.Generator().manual_seed(L), dtype=torch.int16).to(torch.uint8).view(in_dtype)
    table, a_codes = None, raw
    if pre:                                                                        # the prefix ``* 0.5`` between A0 (scale 2 a) and A
        in_lo = -128 if in_dtype == torch.int8 else 0
        table = ops.code_table(lambda v: v * 0.5, (2 * a_scale, 3, in_lo, in_lo + 255), (a_scale, 3, in_lo, in_lo + 255), "cpu")
        a_codes = ops.codes_table(raw, table, in_dtype)
    got = ops.codes_softmax(raw, (a_scale, 3, *((-128, 127) if in_dtype == torch.int8 else (0, 255))), out_form, pre_table=table)
    assert got.shape == raw.shape and got.dtype == ops._code_dtype(*out_form[2:])[0]
    diff = np.abs(got.numpy().astype(np.float64) - _reference(a_codes, a_scale, out_form))
    print(f"max difference {diff.max()}, elements that differ {int((diff > 0).sum())} of {diff.size}")
    assert diff.max() <= 1 and (diff > 0).mean() <= 1e-3


@pytest.mark.parametrize("L", [1, 5, 197])
def test_equal_codes_give_one_over_L_and_the_pad_is_the_zero_point(L):
    out_form = (2.0 ** -12, -100, -128, 127)
    codes = torch.full((3, L), 41, dtype=torch.int8)
    got = ops.codes_softmax(codes, (0.3, 0), out_form, pad_to=16)
    want = min(127, round(float(np.float32(1.0) / np.float32(L)) * 4096) - 100)
    assert got.shape == (3, -(-L // 16) * 16) and (got[:, :L] == want).all() and (got[:, L:] == -100).all()


def _nodes(gm):
    return [n.target if isinstance(n.target, str) else n.target.__name__ for n in gm.graph.nodes]


def test_rewrite_of_the_attention_block():
    gm, n = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(), softmaxes=True, **SWITCHES)
    base, n_base = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(), **SWITCHES)
    nodes = _nodes(gm)
    at = nodes.index("matmul_qmatmul")
    assert n == n_base and nodes[at:at + 3] == ["matmul_qmatmul", "a_probs_softmax", "matmul_1_qmatmul"]
    assert _nodes(base)[at:at + 6] == ["matmul_qmatmul", "a_scores", "mul", "a_scaled", "softmax", "matmul_1_qmatmul"]
    scores, softmax, context = (gm.get_submodule(name) for name in nodes[at:at + 3])
    assert type(softmax) is consumers.QuantizedSoftmax and softmax.pad_rows and context.a_padded
    assert scores.activation_code_params() == softmax.activation_code_params() == (32.0 / 128, 0, -128, 127)
    # the same model with the float32 stretch replaced by the contract in torch
    block = workloads.wrapped_attention_block()
    holder_codes = lambda h, x: ops.fq_codes(x, None, None, None, *consumers._code_form(h.activation_holder_quantizer)[2:],    # noqa: E731
                                             *consumers._code_form(h.activation_holder_quantizer)[:2])
    forms = [consumers._code_form(h.activation_holder_quantizer) for h in (block.a_scores, block.a_scaled, block.a_probs)]

    def contract(scores_f32):
        c = holder_codes(block.a_scaled, ops.dequantize_codes(holder_codes(block.a_scores, scores_f32), *forms[0][:2]) * block.scale)
        e = torch.from_numpy(ops.softmax_exp_table(forms[1][0]).astype(np.int64))[c.long().amax(-1, keepdim=True) - c.long()]
        p = e.float() / e.sum(-1, keepdim=True).float()
        return ops.dequantize_codes(ops.fq_codes(p, None, None, None, *forms[2][2:], *forms[2][:2]), *forms[2][:2])

    # the block's forward with ``contract`` in place of a_scores -> * scale -> a_scaled -> softmax -> a_probs
    x = block.a_in(block.norm(BLOCK_INPUT))
    q, k, v = (a(layer(x)).reshape(-1, block.tokens, block.heads, block.head_dim).permute(0, 2, 1, 3)
               for layer, a in ((block.q, block.a_q), (block.k, block.a_k), (block.v, block.a_v)))
    ctx = block.a_ctx(contract(q @ k.transpose(-1, -2)) @ v)
    want = block.proj(ctx.permute(0, 2, 1, 3).reshape(-1, block.tokens, block.dim))
    y = gm(BLOCK_INPUT)
    assert torch.equal(y, want) and len(y.unique()) > 100


class _Variant(nn.Module):
    """holder -> [variant] -> softmax -> holder -> Linear, one of the forms the rewrite leaves alone."""

    def __init__(self, variant):
        super().__init__()
        self.variant = variant
        holder = lambda: mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(8, [8.0], True))   # noqa: E731
        self.a, self.a2 = holder(), holder()
        self.b = mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(8, [1.0], False))
        self.fc = mq.PytorchQuantizationWrapper(nn.Linear(16, 16), {"weight": Q.WeightsPOTInferableQuantizer(
            num_bits=8, threshold=[1.0] * 16, per_channel=True, channel_axis=0)})

    def forward(self, x, mask):
        x = self.a(x)
        if self.variant == "mask":
            x = x + mask
        if "prefix" in self.variant:                                               # A0 -> * c -> A, the two one holder or two
            x = (self.a if self.variant == "shared prefix" else self.a2)(x * 0.25)
        if self.variant == "log_softmax":
            p = self.b(torch.log_softmax(x, dim=-1))
        else:
            p = self.b(torch.softmax(x, dim=-2 if self.variant == "dim" else -1))
        return self.fc(p) + p if self.variant == "float user" else self.fc(p)


@pytest.mark.parametrize("variant", ["taken", "mask", "dim", "log_softmax", "float user"])
def test_variants_left_alone(variant):
    gm, _ = consumers.fuse_linear_consumers_fx(_Variant(variant), softmaxes=True)
    assert any(isinstance(m, consumers.QuantizedSoftmax) for m in gm.modules()) == (variant == "taken")


@pytest.mark.parametrize("variant", ["prefix", "shared prefix"])
def test_prefix_between_two_holders_or_one_holder_called_twice(variant):
    """The node's codes against holder B's float32 output in the model as it was: at most one code off, at most 0.1 % off."""
    model = _Variant(variant)
    gm, n = consumers.fuse_linear_consumers_fx(_Variant(variant), softmaxes=True)
    node = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedSoftmax))
    assert n == 1 and node.has_prefix and len(node.fns) == 1
    seen = {}
    model.b.register_forward_hook(lambda m, args, out: seen.__setitem__("want", out))
    node.register_forward_hook(lambda m, args, out: seen.__setitem__("got", out))
    x = torch.randn(400, 16, generator=torch.Generator().manual_seed(5)) * 4
    model(x, None), gm(x, None)
    diff = (seen["got"].double() - seen["want"].double() * 256).abs()
    print(f"max difference {diff.max()} codes, elements that differ {int((diff > 0).sum())} of {diff.numel()}")
    assert diff.max() <= 1 and (diff > 0).double().mean() <= 1e-3
