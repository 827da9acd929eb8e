"""The fused attention kernel (``mctq_qattention_i8``) against the CPU composition of the three calls it replaces, byte for byte."""
import pytest
import torch

from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

pytestmark = pytest.mark.gpu

I8, U8 = torch.int8, torch.uint8
# (q, k, v) as (dtype, zero point); holder A0, holder A behind a prefix, holder B as (dtype, zero point); the context holder
ZERO = dict(ops=((I8, 0), (I8, 0), (I8, 0)), a0=(I8, 0), a=(I8, 0), b=(U8, 0), out=(2.0 ** -5, 0, -128, 127))
SAME = dict(ops=((U8, 131), (U8, 120), (U8, 125)), a0=(I8, -9), a=(U8, 133), b=(I8, -128), out=(2.0 ** -5, 3, -128, 127))
MIXED = dict(ops=((U8, 131), (I8, -5), (U8, 120)), a0=(U8, 125), a=(I8, 7), b=(I8, -128), out=(2.0 ** -5, 3, -128, 127))


def _domain(dtype):
    return (0, 255) if dtype == U8 else (-128, 127)


def _codes(shape, dtype, gen):
    lo, hi = _domain(dtype)
    x = torch.randint(lo, hi + 1, shape, generator=gen).to(dtype)
    x.view(-1)[0], x.view(-1)[-1] = lo, hi                           # both extreme codes are present
    return x


def _case(shape, forms, pre, codes_out, layout, device, seed=0):
    """The operands on ``device`` (as views where ``layout`` says so; the same codes on every device) and the keyword arguments
    of ``qattention_i8``."""
    b0, b1, M, T, D, Dv = shape
    gen = torch.Generator().manual_seed(seed)
    (qt, qz), (kt, kz), (vt, vz) = forms["ops"]
    if layout == "qkv":                                              # one fused [B, T, 3, H, D] tensor, permuted and indexed
        assert M == T and D == Dv and qt == kt == vt
        q, k, v = _codes((b0, T, 3, b1, D), qt, gen).to(device).permute(2, 0, 3, 1, 4)
    else:
        kb = (1, 1) if layout == "k_broadcast" else (b0, b1)
        q, k, v = (_codes(s, t, gen).to(device) for s, t in (((b0, b1, M, D), qt), ((*kb, T, D), kt), ((b0, b1, T, Dv), vt)))
        k = k.expand(b0, b1, T, D)                                   # (a batch stride of 0 where K is broadcast)
    # q - zq and k - zk spread like 74 codes, a score like 74^2 sqrt(D) 2^-14: A0 spreads it over about 30 codes, unsaturated
    s_scale = 74.0 ** 2 * D ** 0.5 * 2.0 ** -14 / 30.0
    scores_form = (s_scale, forms["a0"][1], *_domain(forms["a0"][0]))
    a_form = (s_scale * D ** -0.5, forms["a"][1], *_domain(forms["a"][0])) if pre else scores_form
    kwargs = dict(scores_form=scores_form, a_form=a_form, probs_form=(2.0 ** -8, forms["b"][1], *_domain(forms["b"][0])),
                  out_codes=forms["out"] if codes_out else None)
    return (q, (2.0 ** -7, qz), k, (2.0 ** -7, kz), v, (2.0 ** -5, vz)), kwargs


def _reference(args, kwargs, pre):
    """The three public calls on CPU tensors (int64 sums), and the conditions the inputs must meet on them."""
    q, q_form, k, k_form, v, v_form = args
    T = k.shape[-2]
    s = consumers.qmatmul_i8(q, q_form, k, k_form, transposed_b=True, out_codes=kwargs["scores_form"])
    p = ops.codes_softmax(s, kwargs["a_form"], kwargs["probs_form"], pre_table=pre, pad_to=16)
    y = consumers.qmatmul_i8(p, kwargs["probs_form"][:2], v, v_form, transposed_b=False, out_codes=kwargs["out_codes"], a_padded_k=T)
    if T >= 64:
        assert s.unique().numel() >= 64                              # the score codes are not saturated
    one_hot = ((p[..., :T] != kwargs["probs_form"][1]).sum(-1) <= 1).float().mean().item()
    assert T == 1 or one_hot <= 0.5                                  # the probability rows are not one-hot
    return y


CASES = [
    pytest.param((1, 1, 1, 1, 16, 16), MIXED, True, True, None, True, id="one-element"),
    pytest.param((1, 2, 17, 17, 16, 16), ZERO, False, False, None, True, id="partial-tile"),
    pytest.param((1, 2, 17, 17, 16, 16), SAME, True, True, "qkv", True, id="partial-tile-qkv-view"),
    pytest.param((1, 1, 64, 64, 64, 64), MIXED, True, True, None, True, id="no-remainder"),
    pytest.param((1, 1, 64, 64, 64, 64), ZERO, False, False, "qkv", True, id="no-remainder-qkv-view"),
    pytest.param((2, 3, 65, 197, 64, 64), MIXED, True, True, None, True, id="vit-row-idle-waves"),
    pytest.param((2, 3, 65, 197, 64, 64), ZERO, False, False, "k_broadcast", True, id="vit-row-k-broadcast"),
    pytest.param((1, 1, 16, 63, 32, 16), MIXED, False, True, None, True, id="T63"),
    pytest.param((1, 1, 16, 64, 32, 16), ZERO, True, False, None, True, id="T64"),
    pytest.param((1, 1, 16, 65, 32, 16), MIXED, True, False, None, True, id="T65"),
    pytest.param((1, 1, 20, 130, 128, 80), MIXED, False, True, None, True, id="two-q-steps-five-n-tiles"),
    pytest.param((1, 1, 20, 130, 128, 80), ZERO, True, False, "k_broadcast", True, id="two-q-steps-zero-forms"),
    pytest.param((1, 1, 80, 1024, 128, 128), MIXED, True, False, None, True, id="largest-strip"),
    pytest.param((1, 1, 16, 1040, 64, 64), MIXED, False, True, None, False, id="T-above-limit-falls-back"),
    pytest.param((1, 1, 16, 64, 24, 64), ZERO, True, False, None, False, id="D24-falls-back"),
]


@pytest.mark.parametrize("shape, forms, with_pre, codes_out, layout, fused", CASES)
def test_kernel_equals_the_three_calls(shape, forms, with_pre, codes_out, layout, fused):
    args, kwargs = _case(shape, forms, with_pre, codes_out, layout, "cpu")
    prefix = lambda s: s * shape[4] ** -0.5                                                          # noqa: E731
    table = lambda device: ops.code_table(prefix, kwargs["scores_form"], kwargs["a_form"], device) if with_pre else None   # noqa: E731
    want = _reference(args, kwargs, table("cpu"))
    on_gpu, _ = _case(shape, forms, with_pre, codes_out, layout, "cuda")
    got = consumers.qattention_i8(*on_gpu, pre_table=table("cuda"), **kwargs)
    assert ("qattention" in native.last_launch()) == fused
    assert got.dtype == want.dtype and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dim, heads, tokens", [(64, 2, 17), (768, 12, 197)])
def test_rewrite_on_the_gpu(dim, heads, tokens):
    switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True)
    block = lambda: workloads.wrapped_attention_block(dim=dim, heads=heads, tokens=tokens, device="cuda")   # noqa: E731
    plain, _ = consumers.fuse_linear_consumers_fx(block(), **switches)
    fused, _ = consumers.fuse_linear_consumers_fx(block(), attentions=True, **switches)
    x = torch.randn(2, tokens, dim, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        want = plain(x)
        attention = next(m for m in fused.modules() if isinstance(m, consumers.QuantizedAttention))
        seen = []
        hook = attention.register_forward_hook(lambda *_: seen.append(native.last_launch()))
        got = fused(x)
        hook.remove()
    assert seen and "qattention" in seen[0]
    assert torch.equal(got, want)


def test_raw_entry_point_refuses():
    lib = native.load()
    q, k, v = (torch.zeros(1, 1, 16, 32, dtype=I8, device="cuda") for _ in range(3))
    etab = torch.from_numpy(ops.softmax_exp_table(0.5).view("int32")).cuda()
    y = torch.full((16 * 32 + 16,), 7.0, device="cuda")

    def call(qp=0, t=16, d=32, out=None):
        strides = (16 * 32, 16 * 32, 32)
        rc = lib.mctq_qattention_i8(q.data_ptr() + qp, native.CODE_I8, 0, 1.0, *strides, k.data_ptr(), native.CODE_I8, 0, 1.0, *strides,
                                    v.data_ptr(), native.CODE_I8, 0, 1.0, *strides, native.CODE_I8, 1.0, 0, -128, 127, native.CODE_I8,
                                    native.CODE_U8, 2.0 ** -8, 0, 0, 255, etab.data_ptr(), None, y.data_ptr() if out is None else out,
                                    -1, 1.0, 0, 0, 0, 1, 1, 16, t, d, 32, None)
        torch.cuda.synchronize()
        return rc, lib.mctq_last_error().decode()

    rc, text = call(qp=1)
    assert rc != 0 and "16-byte aligned" in text
    rc, text = call(d=24)
    assert rc != 0 and "D must be a multiple of 16" in text
    rc, text = call(out=v.data_ptr())
    assert rc != 0 and "overlaps an operand" in text
    rc, _ = call(t=0)
    assert rc == 0 and bool((y == 7.0).all())                         # nothing launched, nothing written
    rc, _ = call()
    assert rc == 0 and bool((y[:16 * 32] != 7.0).all()) and bool((y[16 * 32:] == 7.0).all())
