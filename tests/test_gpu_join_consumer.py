"""mctq_fq_join_f32, ops.fq_join and consumers.QuantizedJoin on the GPU.

The kernel stands for four launches whose results the suite already pins down (ATen add, ATen ReLU, the holder's fake-quant,
the codes): the raw entry point must equal the CPU route of ops.fq_join bit for bit -- both outputs, every prologue, edge
values included -- and write nothing outside its outputs; a rewritten model on the GPU must equal its own CPU route and its
private-holders twin bit for bit."""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_join_consumer import (FORMS, PROLOGUES, ResidualStack, check_fq_join, check_stack_output_bits, composed, join_case,
                                rewritten_stack, stack_input)

GUARD, SENTINEL = 64, 0xA5
# one lane; the tail alone; one whole chunk; a chunk and a tail; whole blocks; several blocks, the last partly empty, and a tail
SIZES = [1, 15, 16, 17, 4096, 4096 * 3 + 16 * 5 + 7]
OUTPUTS = [(True, True), (True, False), (False, True)]


@functools.lru_cache(maxsize=None)
def cpu_route(n, form, residual, relu):
    """(y, codes) of ops.fq_join on the CPU for join_case(n, form): computed once, read-only."""
    from mct_quantizers_amd.hip import ops
    x, r = (torch.from_numpy(a.copy()) for a in join_case(n, form))
    y, codes = ops.fq_join(x, *FORMS[form], residual=r if residual else None, relu=relu)
    return y.numpy(), codes.numpy()


def _raw_into_guarded_buffers(n, form, residual, relu, want_float, want_codes):
    """The raw entry point on device copies of the case, each output in the middle of a sentinel-filled buffer -> (y or None,
    codes or None) as numpy; the sentinels on both sides of both buffers, and the whole buffer of an output that is switched
    off, are checked here, and that the call was exactly one launch named fq_join."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    scale, zp, qmin, qmax = FORMS[form]
    x, r = (torch.from_numpy(a.copy()).cuda() for a in join_case(n, form))
    ybuf = torch.full((4 * n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (ybuf.data_ptr() + GUARD) % 16 == 0 and (cbuf.data_ptr() + GUARD) % 16 == 0 and x.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0
    count = native.launch_count()
    rc = lib.mctq_fq_join_f32(x.data_ptr(), r.data_ptr() if residual else None, int(relu),
                              ybuf.data_ptr() + GUARD if want_float else None, cbuf.data_ptr() + GUARD if want_codes else None,
                              native.CODE_U8 if qmin >= 0 else native.CODE_I8, n, scale, zp, qmin, qmax,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    assert native.launch_count() - count == 1 and launch.startswith("fq_join<"), launch
    assert ("add " in launch) == residual and ("relu " in launch) == relu and ("f32" in launch) == want_float, launch
    assert (("u8" if qmin >= 0 else "i8") in launch) == want_codes, launch
    yb, cb = ybuf.cpu().numpy(), cbuf.cpu().numpy()
    what = (n, form, residual, relu, want_float, want_codes)
    assert np.all(yb[:GUARD] == SENTINEL) and np.all(yb[GUARD + 4 * n:] == SENTINEL), what
    assert np.all(cb[:GUARD] == SENTINEL) and np.all(cb[GUARD + n:] == SENTINEL), what
    if not want_float:
        assert np.all(yb == SENTINEL), what
    if not want_codes:
        assert np.all(cb == SENTINEL), what
    y = yb[GUARD:GUARD + 4 * n].view(np.float32) if want_float else None
    codes = cb[GUARD:GUARD + n].view(np.uint8 if qmin >= 0 else np.int8) if want_codes else None
    return y, codes


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["u8", "i8"])
@pytest.mark.parametrize("residual,relu", PROLOGUES)
def test_fq_join_kernel_equals_the_cpu_route_and_stays_inside_its_outputs(form, residual, relu):
    for n in SIZES:
        want_y, want_c = cpu_route(n, form, residual, relu)
        x = join_case(n, form)[0]
        for want_float, want_codes in OUTPUTS:
            y, codes = _raw_into_guarded_buffers(n, form, residual, relu, want_float, want_codes)
            what = (n, want_float, want_codes)
            if want_float:
                assert bits_equal(y, want_y), (what, first_mismatch(y, want_y, x))
            if want_codes:
                assert np.array_equal(codes, want_c), (what, int((codes != want_c).sum()))
    assert len(np.unique(want_c)) > 100 and np.isnan(join_case(SIZES[-1], form)[0]).any()      # the largest case holds the edge values


@pytest.mark.gpu
def test_fq_join_on_layouts_is_one_launch_with_the_inputs_strides():
    from mct_quantizers_amd.hip import native
    g = torch.Generator().manual_seed(8)
    x4 = (torch.randn(2, 16, 5, 7, generator=g) * 30).contiguous(memory_format=torch.channels_last)
    r4 = (torch.randn(2, 16, 5, 7, generator=g) * 10).contiguous(memory_format=torch.channels_last)
    x2, r2 = torch.randn(3, 48, generator=g) * 30, torch.randn(3, 48, generator=g) * 10
    for x, r in ((x4, r4), (x2, r2), (x2.t(), r2.t())):
        for form in FORMS.values():
            for residual, relu in PROLOGUES:
                for want_float, want_codes in OUTPUTS:
                    rr = r if residual else None
                    want = composed(x, rr, relu, form)                  # on the CPU
                    count = native.launch_count()
                    y, codes = check_fq_join(x.cuda(), None if rr is None else rr.cuda(), relu, form, want_float, want_codes, want)
                    assert native.launch_count() - count == 1 and native.last_launch().startswith("fq_join<")
    # ... shapes, strides and dtypes as the input's: channels-last codes are NCHW-shaped, NHWC-stored
    y, codes = check_fq_join(x4.cuda(), r4.cuda(), True, FORMS["u8"], want=composed(x4, r4, True, FORMS["u8"]))
    assert y.shape == codes.shape == x4.shape and y.stride() == codes.stride() == x4.stride()
    assert y.dtype == torch.float32 and codes.dtype == torch.uint8 and codes.permute(0, 2, 3, 1).is_contiguous()
    # what the kernel does not take runs the composed route: the same bits, no join launch
    wide = torch.randn(2, 16, 5, 14, generator=g) * 30
    flat = torch.randn(2 * 16 * 5 * 7 + 1, generator=g) * 30
    others = [(x4.cuda(), r4[:, :, :1, :1].cuda(), x4, r4[:, :, :1, :1]),                          # a broadcasting residual
              (wide.cuda()[..., ::2], None, wide[..., ::2], None),                                 # a non-dense x
              (x4.cuda(), r4.contiguous().cuda(), x4, r4.contiguous()),                            # a differently strided residual
              (flat.cuda()[1:], None, flat[1:], None),                                             # dense, but not 16-byte aligned
              (x4.cuda().half(), r4.cuda().half(), x4.half(), r4.half())]                          # another dtype
    for xg, rg, xc, rc in others:
        for form in FORMS.values():
            if xg.dtype == torch.float16:
                from mct_quantizers_amd.hip import ops
                y, codes = ops.fq_join(xg, *form, residual=rg, relu=True)
                wy, wc = composed(xg, rg, True, form)                   # half sums: against the same chain on the GPU
                assert y.dtype == torch.float16 and torch.equal(y, wy) and torch.equal(codes, wc)
            else:
                check_fq_join(xg, rg, True, form, want=composed(xc, rc, True, form), strides=False)
            assert not native.last_launch().startswith("fq_join<")


def _join_launches(gm, x):
    """gm(x) with every join's launch name recorded -> (output, {join name: name of the last launch when it returned})."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    seen, hooks = {}, []
    for name, m in gm.named_modules():
        if isinstance(m, consumers.QuantizedJoin):
            hooks.append(m.register_forward_hook(lambda mod, args, out, name=name: seen.__setitem__(name, native.last_launch())))
    y = gm(x)
    for h in hooks:
        h.remove()
    return y, seen


@pytest.mark.gpu
@pytest.mark.parametrize("channels_last", [False, True])
def test_rewritten_stack_on_gpu_equals_its_cpu_route_and_its_twin(channels_last):
    y = check_stack_output_bits("cuda", channels_last, against_unrewritten=False)        # the twin on the GPU, bit for bit
    assert y.is_cuda and y.shape == (2, 32, 5, 4) and y.is_contiguous(memory_format=torch.channels_last)
    want = rewritten_stack("cpu")[0](stack_input("cpu", channels_last))
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
    gm, _ = rewritten_stack("cuda")
    y2, launches = _join_launches(gm, stack_input("cuda", channels_last))
    assert torch.equal(y2, y) and len(launches) == 6
    for name, launch in launches.items():
        # an NCHW-contiguous input takes the first join's transposing route; every other join is the one launch
        assert launch.startswith("fq_join<") == (channels_last or name != "h0_join"), (name, launch)
    assert "add relu -> f32 + u8" in launches["A_a3_1_join"] and "relu -> u8" in launches["A_a1_1_join"]


@pytest.mark.gpu
def test_rewritten_stack_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = rewritten_stack("cuda")
    x = stack_input("cuda", channels_last=True)
    want = gm(x)                                                      # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # strictly sequential, one stream: joins, patch matrices, products
        out, launches = _join_launches(gm, static_x)
    assert native.launch_count() - n0 >= 6 + 7                        # six joins and seven products at least
    assert len(launches) == 6 and all(v.startswith("fq_join<") for v in launches.values()), launches
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5)) and not torch.equal(out, want)
