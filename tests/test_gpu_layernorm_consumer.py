"""mctq_codes_layernorm on the GPU: the kernel must equal the CPU route of ops.codes_layernorm byte for byte -- mean and variance
are integers -- in both forms, at every row length where it takes another path, and write nothing outside its rows."""
import math

import pytest
import torch

from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

pytestmark = pytest.mark.gpu
DOMAINS = {torch.int8: (-128, 127), torch.uint8: (0, 255)}
EPS = 1e-5


def _case(rows, L, dtype=torch.int8):
    """Random codes, gamma and beta; row 0 all equal, row 1 with the least and the greatest code at its ends."""
    g = torch.Generator().manual_seed(L)
    lo, hi = DOMAINS[dtype]
    codes = torch.randint(lo, hi + 1, (rows, L), generator=g, dtype=torch.int16)
    codes[0] = 41
    codes[1, 0], codes[1, -1] = lo, hi
    return codes.to(dtype), 1.0 + 0.5 * torch.randn(L, generator=g), 0.3 * torch.randn(L, generator=g)


def _check(case, in_form, out_form, **tuning):
    codes, gamma, beta = case
    want = ops.codes_layernorm(codes, in_form, out_form, gamma, beta, EPS)
    for key, value in tuning.items():
        native.set_tuning(key, value)
    try:
        got = ops.codes_layernorm(codes.cuda(), in_form, out_form, gamma.cuda(), beta.cuda(), EPS)
    finally:
        for key in tuning:
            native.set_tuning(key, 0)
    assert got.is_cuda and torch.equal(got.cpu(), want), (codes.shape, native.last_launch())
    return native.last_launch()


# rows x L: the lane-count edges of one and two chunks per lane in each form, and the boundary between the forms
@pytest.mark.parametrize("rows,L,form,ch", [(5, 16, "wave", 1), (5, 1024, "wave", 1), (5, 1040, "wave", 2), (5, 2048, "wave", 2),
                                            (3, 2064, "block", 1), (3, 4096, "block", 1), (3, 4112, "block", 2), (2, 8192, "block", 2)])
def test_kernel_equals_the_cpu_route(rows, L, form, ch):
    launch = _check(_case(rows, L), (0.0731, -7), (8.0 / 128, 3, -128, 127))
    assert launch.startswith(f"codes_layernorm<i8 -> i8 {form},") and f"U={ch}" in launch, launch


@pytest.mark.parametrize("form", [1, 2], ids=["wave", "block"])
def test_both_forms_give_the_same_bytes(form):
    launch = _check(_case(5, 1040), (2.0 ** -5, 0), (1.0 / 32, -20, -128, 127), layernorm_form=form)
    assert f" {'wave' if form == 1 else 'block'}," in launch, launch


@pytest.mark.parametrize("rows,L,form", [(11, 48, 1), (5, 2064, 2)], ids=["wave", "block"])
def test_one_workgroup_walks_every_row(rows, L, form):
    _check(_case(rows, L), (0.0731, -7), (8.0 / 128, 3, -128, 127), layernorm_form=form, layernorm_blocks=1)


@pytest.mark.parametrize("in_dtype", [torch.int8, torch.uint8])
@pytest.mark.parametrize("out_dtype", [torch.int8, torch.uint8])
def test_code_types(in_dtype, out_dtype):
    launch = _check(_case(5, 208, in_dtype), (0.0213, DOMAINS[in_dtype][0] + 113), (0.05, DOMAINS[out_dtype][0] + 120, *DOMAINS[out_dtype]))
    assert launch.startswith(f"codes_layernorm<{'i8' if in_dtype == torch.int8 else 'u8'} -> {'i8' if out_dtype == torch.int8 else 'u8'} wave,")


def test_raw_entry_point_writes_its_rows_alone_and_refuses_what_it_cannot_take():
    rows, L, guard = 6, 208, 256
    codes, gamma, beta = _case(rows, L)
    want = ops.codes_layernorm(codes, (0.0731, -7), (0.05, 9, 0, 255), gamma, beta, EPS)
    buf = torch.full((guard + rows * L + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    dev, g, b = codes.cuda(), gamma.cuda(), beta.cuda()
    k = EPS * L * L / float(torch.tensor(0.0731, dtype=torch.float32).double()) ** 2
    lib = native.load()

    def call(src=dev.data_ptr(), dst=buf.data_ptr() + guard, length=L, k_term=k, params=(g, b)):
        return lib.mctq_codes_layernorm(src, native.CODE_I8, -7, dst, native.CODE_U8, 0.05, 9, 0, 255, rows, length,
                                        params[0].data_ptr(), params[1].data_ptr(), k_term, None)

    rc = call()
    torch.cuda.synchronize()
    assert rc == 0, lib.mctq_last_error()
    got = buf.cpu()
    assert torch.equal(got[guard:-guard].view(rows, L), want)
    assert (got[:guard] == 0x5a).all() and (got[-guard:] == 0x5a).all()
    # separate buffers with room for the length tried, so that nothing but the length can be what is refused
    big, wide = torch.empty(2, rows * 8208, dtype=torch.uint8, device="cuda"), torch.ones(2, 8208, device="cuda")
    for refused in (dict(length=200), dict(length=8208, src=big[0].data_ptr(), dst=big[1].data_ptr(), params=wide),
                    dict(dst=buf.data_ptr() + guard + 4),
                    dict(k_term=0.0), dict(k_term=math.inf), dict(dst=dev.data_ptr())):
        assert call(**refused) != 0, refused


def test_rewritten_encoder_block_on_gpu_equals_its_cpu_run():
    switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True, layernorms=True)
    cpu, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(), **switches)
    gpu, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(device="cuda"), **switches)
    x = torch.randn(2, 17, 64, generator=torch.Generator().manual_seed(17)) * 1.5
    seen = []
    gpu.get_submodule("a_n2_layernorm").register_forward_hook(lambda m, args, out: seen.append((args[0].dtype, native.last_launch())))
    y = gpu(x.cuda())
    assert seen[0][0] == torch.int8 and seen[0][1].startswith("codes_layernorm<i8 -> i8 wave,"), seen
    assert torch.equal(y.cpu(), cpu(x)) and len(y.unique()) > 100
