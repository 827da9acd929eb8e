"""mctq_codes_softmax on the GPU: the kernel must equal the CPU route of ops.codes_softmax byte for byte -- the contract is on
integers -- in both forms, at every row length where it takes another path, and write nothing outside its rows."""
import pytest
import torch

from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

pytestmark = pytest.mark.gpu
DOMAINS = {torch.int8: (-128, 127), torch.uint8: (0, 255)}


def _codes(rows, L, dtype):
    """Random codes; row 0 all equal, row 1 with the least and the greatest int8 code (as raw bytes) at its ends."""
    raw = torch.randint(0, 256, (rows, L), generator=torch.Generator().manual_seed(L), dtype=torch.int16).to(torch.uint8)
    raw[0] = 41
    raw[1, 0], raw[1, -1] = 0x80, 0x7f
    return raw.view(dtype)


def _check(codes, in_form, out_form, **kw):
    want = ops.codes_softmax(codes, in_form, out_form, **kw)
    kw = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    got = ops.codes_softmax(codes.cuda(), in_form, out_form, **kw)
    assert got.is_cuda and torch.equal(got.cpu(), want), (codes.shape, native.last_launch())
    return native.last_launch()


# rows x L: misaligned one-chunk rows; the lane-count edge of the 1- and 2-chunk wave forms; the wave / block boundary; the cap
@pytest.mark.parametrize("rows,L", [(5, 1), (5, 15), (5, 16), (7, 17), (6, 197), (5, 1024), (5, 1025), (5, 4080), (5, 4097), (3, 32768)])
def test_kernel_equals_the_cpu_route(rows, L):
    launch = _check(_codes(rows, L, torch.int8), (2.0 ** -5, 3, -128, 127), (1.0 / 255, 0, 0, 255))
    assert launch.startswith(f"codes_softmax<i8 -> u8 {'wave' if L <= 4080 else 'block'},"), launch


@pytest.mark.parametrize("L", [197, 1025])
@pytest.mark.parametrize("form", [1, 2], ids=["wave", "block"])
@pytest.mark.parametrize("pad_to", [None, 16])
def test_both_forms_give_the_same_bytes(L, form, pad_to):
    native.set_tuning("softmax_form", form)
    try:
        launch = _check(_codes(6, L, torch.int8), (0.0731, -7, -128, 127), (2.0 ** -8, -128, -128, 127), pad_to=pad_to)
    finally:
        native.set_tuning("softmax_form", 0)
    assert f" {'wave' if form == 1 else 'block'}," in launch, launch


@pytest.mark.parametrize("in_dtype", [torch.int8, torch.uint8])
@pytest.mark.parametrize("out_dtype", [torch.int8, torch.uint8])
@pytest.mark.parametrize("pre", [False, True])
def test_code_types_and_the_pre_table(in_dtype, out_dtype, pre):
    in_form, out_form = (0.0731, 3, *DOMAINS[in_dtype]), (1.0 / 255, DOMAINS[out_dtype][0], *DOMAINS[out_dtype])
    table = ops.code_table(lambda v: torch.tanh(v * 0.125), (0.21, 5, *DOMAINS[in_dtype]), in_form, "cpu") if pre else None
    launch = _check(_codes(6, 197, in_dtype), in_form, out_form, pre_table=table, pad_to=16)
    assert launch.startswith("codes_softmax<") and (" pre," in launch) == pre, launch


def test_padded_rows_and_nothing_outside_them():
    rows, L, pitch, guard = 6, 197, 208, 256
    codes = _codes(rows, L, torch.int8)
    want = ops.codes_softmax(codes, (2.0 ** -5, 0), (1.0 / 256, 9, 0, 255), pad_to=16)
    buf = torch.full((guard + rows * pitch + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    dev, exp = codes.cuda(), torch.from_numpy(ops.softmax_exp_table(2.0 ** -5).view("int32")).cuda()
    rc = native.load().mctq_codes_softmax(dev.data_ptr(), native.CODE_I8, buf.data_ptr() + guard, native.CODE_U8, 1.0 / 256, 9, 0, 255,
                                          rows, L, L, pitch, 9, exp.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == 0, native.load().mctq_last_error()
    got = buf.cpu()
    assert torch.equal(got[guard:-guard].view(rows, pitch), want) and (want[:, L:] == 9).all()
    assert (got[:guard] == 0x5a).all() and (got[-guard:] == 0x5a).all()


@pytest.mark.parametrize("tokens", [17, 16])
def test_rewritten_attention_block_on_gpu_equals_its_cpu_run(tokens):
    switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True)
    cpu, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(64, 2, tokens), **switches)
    gpu, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(64, 2, tokens, device="cuda"), **switches)
    x = torch.randn(2, tokens, 64, generator=torch.Generator().manual_seed(tokens)) * 1.5
    seen = []
    gpu.get_submodule("a_probs_softmax").register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, out.shape[-1], native.last_launch())))
    y = gpu(x.cuda())
    assert seen[0][:2] == (torch.int8, 32 if tokens == 17 else 16) and seen[0][2].startswith("codes_softmax<i8 -> u8 wave pre,"), seen
    assert torch.equal(y.cpu(), cpu(x)) and len(y.unique()) > 100
