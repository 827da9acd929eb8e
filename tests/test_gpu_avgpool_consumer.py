"""mctq_codes_avgpool_nhwc, consumers.QuantizedAvgPool2d and the ``avg_pools`` rewrites on the GPU.

The window sum is an integer and the three float32 steps behind it are single IEEE operations, so everything here is
equality: the raw entry point must give the bytes of the CPU route of ops.codes_avgpool and of the numpy loops of
tests/test_avgpool_consumer.py, in the lane form and in the split form alike, and write nothing outside its output; the module
and the rewritten models must equal their CPU routes, and the rewrite with ``avg_pools=True`` the same rewrite without it, bit
for bit (tests/test_avgpool_consumer.py says why those models are exact)."""
import numpy as np
import pytest
import torch

from test_avgpool_consumer import (EVERY, EXTREMES, FORMS, GEOMETRIES, GLOBAL576, N_CASES, Between, Head, Squeeze, TAKEN, avg_case, avg_cases,
                                   between_input, check_module, extreme_case, head_input, make_codes)

GUARD, SENTINEL = 64, 0xA5


def _raw_into_guarded_buffer(codes, in_form, out_form, geometry):
    """The raw entry point on a device copy of ``codes``, its output in the middle of a sentinel-filled buffer -> (output as numpy
    [B, Ho, Wo, C], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    k, s, (ph, pw), ceil_mode, include_pad, override = geometry
    B, H, W, C = codes.shape
    kh, kw = (H, W) if k is None else k
    sh, sw = (kh, kw) if s is None else s
    ho, wo = ops._pool_out_size(H, kh, sh, ph, 1, ceil_mode), ops._pool_out_size(W, kw, sw, pw, 1, ceil_mode)
    n = B * ho * wo * C
    x = torch.from_numpy(codes.copy()).cuda()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and x.data_ptr() % 16 == 0
    out_dtype = np.uint8 if out_form[2] >= 0 else np.int8
    rc = lib.mctq_codes_avgpool_nhwc(x.data_ptr(), buf.data_ptr() + GUARD, native.CODE_U8 if codes.dtype == np.uint8 else native.CODE_I8,
                                     in_form[1], in_form[0], B, H, W, C, kh, kw, sh, sw, ph, pw, int(ceil_mode), int(include_pad),
                                     override or 0, ho, wo, native.CODE_U8 if out_dtype == np.uint8 else native.CODE_I8, out_form[0],
                                     out_form[1], out_form[2], out_form[3], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (geometry, C)
    return got[GUARD:GUARD + n].view(out_dtype).reshape(B, ho, wo, C), launch


def _both_forms(codes, in_form, out_form, geometry, want):
    """The case in the lane form and in the split form: each equal to ``want``, its note naming the form asked for."""
    from mct_quantizers_amd.hip import native
    kind = "u8 avg" if codes.dtype == np.uint8 else "i8 avg"
    try:
        for value, name in ((1, "lane"), (2, "split")):
            native.set_tuning("avgpool_form", value)
            got, launch = _raw_into_guarded_buffer(codes, in_form, out_form, geometry)
            assert launch.startswith("codes_avgpool<") and f"{kind} {name}" in launch, launch
            assert got.shape == want.shape and np.array_equal(got, want), (name, in_form, out_form, geometry, codes.shape)
    finally:
        native.set_tuning("avgpool_form", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [True, False])
def test_codes_avgpool_kernel_equals_the_cpu_route_in_both_forms_and_stays_inside_its_output(u8):
    from mct_quantizers_amd.hip import ops
    n = 0
    for case_u8, form, g, shape in avg_cases():
        if case_u8 != u8:
            continue
        codes, S, div, want = avg_case(u8, form, g, **shape)
        in_form, out_form = FORMS[u8][form]
        k, s, p, ceil_mode, include_pad, override = g
        cpu = ops.codes_avgpool(torch.from_numpy(codes.copy()), in_form, out_form, k, s, p, ceil_mode, include_pad, override).numpy()
        assert np.array_equal(cpu, want)
        _both_forms(codes, in_form, out_form, g, want)     # (both equal to ``want``: identical to each other)
        n += 1
    assert n == N_CASES // 2
    for case_u8, zp in EXTREMES:
        if case_u8 == u8:
            codes, in_form, out_form, g, want = extreme_case(u8, zp)
            assert want.max() == out_form[3] or want.min() == out_form[2]
            _both_forms(codes, in_form, out_form, g, want)


@pytest.mark.gpu
def test_the_launcher_chooses_the_split_form_for_one_large_window_and_the_lane_form_for_small_ones():
    from mct_quantizers_amd.hip import native
    native.set_tuning("avgpool_form", 0)
    for u8 in (True, False):
        shape = dict(GLOBAL576)
        g = shape.pop("geometry")
        codes, S, div, want = avg_case(u8, 1, g, **shape)
        got, launch = _raw_into_guarded_buffer(codes, *FORMS[u8][1], g)
        assert "avg split" in launch and np.array_equal(got, want), launch
        for C in (16, 48):
            for g in [g for g in GEOMETRIES if g[0] == (2, 2)]:
                codes, S, div, want = avg_case(u8, 1, g, C=C)
                got, launch = _raw_into_guarded_buffer(codes, *FORMS[u8][1], g)
                assert "avg lane" in launch and np.array_equal(got, want), launch


@pytest.mark.gpu
def test_codes_avgpool_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    g = ((3, 3), (2, 2), (1, 1), False, False, None)
    for u8 in (True, False):
        in_form, out_form = FORMS[u8][2]
        codes, S, div, want = avg_case(u8, 2, g, C=48)
        n0 = native.launch_count()
        y = ops.codes_avgpool(torch.from_numpy(codes.copy()).cuda(), in_form, out_form, 3, 2, 1, count_include_pad=False)
        assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_avgpool<")
        assert y.is_cuda and y.is_contiguous() and y.dtype == torch.int8 and np.array_equal(y.cpu().numpy(), want)
    # a channel count that is no multiple of 16: torch ops on the GPU, the same bytes as on the CPU
    in_form, out_form = FORMS[True][1]
    odd = torch.from_numpy(make_codes(True, 2, 7, 5, 24))
    n0 = native.launch_count()
    y = ops.codes_avgpool(odd.cuda(), in_form, out_form, 3, 2, 1)
    assert native.launch_count() == n0 and y.is_cuda and y.shape == (2, 4, 3, 24)
    assert torch.equal(y.cpu(), ops.codes_avgpool(odd, in_form, out_form, 3, 2, 1))
    y = ops.codes_avgpool(odd.cuda(), in_form, out_form, None)
    assert torch.equal(y.cpu(), ops.codes_avgpool(odd, in_form, out_form, None))
    empty = ops.codes_avgpool(torch.zeros(0, 4, 4, 16, dtype=torch.uint8, device="cuda"), in_form, out_form, 2)
    assert empty.shape == (0, 2, 2, 16) and empty.dtype == torch.uint8 and native.launch_count() == n0


@pytest.mark.gpu
def test_quantized_avg_pool2d_on_gpu_equals_its_cpu_route():
    from mct_quantizers_amd.hip import native
    want = check_module("cpu")
    got = check_module("cuda")
    assert native.last_launch().startswith("codes_avgpool<")
    assert len(got) == len(want) == 20 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("how", TAKEN)
def test_head_gives_the_bits_of_the_rewrite_without_avg_pools_gpu(how):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    x = head_input("cuda")
    for switches in (dict(), EVERY):
        gm, n = consumers.fuse_linear_consumers_fx(Head(how).cuda(), avg_pools=True, **switches)
        gm0, n0 = consumers.fuse_linear_consumers_fx(Head(how).cuda(), **switches)
        assert n == 2
        seen = []
        hook = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedAvgPool2d)).register_forward_hook(
            lambda m, args, out: seen.append(native.last_launch()))
        y, y0 = gm(x), gm0(x)
        hook.remove()
        assert len(seen) == 1 and seen[0].startswith("codes_avgpool<u8 avg")
        assert y.shape == (2, 10) and len(torch.unique(y)) > 15 and torch.equal(y, y0)
        cpu, _ = consumers.fuse_linear_consumers_fx(Head(how), avg_pools=True, **switches)
        assert torch.equal(y.cpu(), cpu(x.cpu()))


@pytest.mark.gpu
def test_squeeze_and_windowed_models_give_the_bits_of_the_rewrite_without_avg_pools_gpu():
    from mct_quantizers_amd import consumers
    C = consumers
    x = head_input("cuda")
    gm, n = C.fuse_linear_consumers_fx(Squeeze().cuda(), avg_pools=True, shared_holders=True)
    gm0, n0 = C.fuse_linear_consumers_fx(Squeeze().cuda(), shared_holders=True)
    assert (n, n0) == (2, 2) and len(list(m for m in gm.modules() if isinstance(m, C.QuantizedAvgPool2d))) == 1
    y = gm(x)
    assert y.shape == (2, 16, 4, 4) and len(torch.unique(y)) > 50 and torch.equal(y, gm0(x))
    assert torch.equal(y.cpu(), C.fuse_linear_consumers_fx(Squeeze(), avg_pools=True, shared_holders=True)[0](x.cpu()))
    x = between_input("cuda")
    for functional in (False, True):
        gm, n = C.fuse_linear_consumers_fx(Between(functional).cuda(), avg_pools=True, **EVERY)
        gm0, n0 = C.fuse_linear_consumers_fx(Between(functional).cuda(), **EVERY)
        assert (n, n0) == (2, 2)
        y = gm(x)
        assert y.shape == (2, 32, 4, 3) and len(torch.unique(y)) > 50 and torch.equal(y, gm0(x))
        assert torch.equal(y.cpu(), C.fuse_linear_consumers_fx(Between(functional), avg_pools=True, **EVERY)[0](x.cpu()))
    # the Sequential rewrite of the same stack
    seq = torch.nn.Sequential(*[m for _, m in Between().named_children()]).cuda().eval()      # h0, c1, act, a, pool, b, c2
    assert isinstance(seq[4], torch.nn.AvgPool2d) and len(seq) == 7
    assert C.fuse_linear_consumers(seq, convolutions=True, avg_pools=True) == 2 and isinstance(seq[4], C.QuantizedAvgPool2d)
    assert torch.equal(seq(x), y)


@pytest.mark.gpu
def test_wrapped_resnet50_head_stays_on_codes():
    """``workloads.wrapped_resnet50(pooled_holder=True)`` with every switch and ``avg_pools=True``, batch 2 on 64 x 64 inputs (the
    final map is 2 x 2): 53 layers replaced; the last three library launches of a forward are the last block's c3 with the
    residual join in its epilogue (emitting codes), the pool, and the classifier's product.  The pool's hook-captured output is
    compared with ``ops.codes_avgpool`` of its captured input on the CPU, and -- the final map being 2 x 2 and the scale 2^-5 --
    with the codes of the float32 chain.  (The logits are not compared with a CPU forward of the whole model: where there is a
    GPU the weights quantizer of the unfused 3-channel stem keeps its parameters there, so that forward does not run.)"""
    from mct_quantizers_amd.hip import ops
    from mct_quantizers_amd import consumers, workloads
    from mct_quantizers_amd.hip import native
    model = workloads.wrapped_resnet50(pooled_holder=True)
    gm, n = consumers.fuse_linear_consumers_fx(model, pools=True, fused_residuals=True, avg_pools=True, **EVERY)
    assert n == 53
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    gm(x)                                                    # (refreshes the weight codes)
    seen, pooled = [], []
    leaves = {node.target for node in gm.graph.nodes if node.op == "call_module"}
    hooks = [gm.get_submodule(t).register_forward_hook(
        lambda m, args, out, t=t: seen.append((t, native.launch_count(), native.last_launch(), getattr(out, "dtype", None),
                                            tuple(getattr(out, "shape", ()))))) for t in leaves]       # (a join returns a pair)
    hooks.append(gm.get_submodule("19_qavgpool").register_forward_hook(lambda m, args, out: pooled.append((args[0], out))))
    y = gm(x)
    for h in hooks:
        h.remove()
    assert [s[0] for s in seen[-3:]] == ["18_c3_qlinear", "19_qavgpool", "22_qlinear"]
    (_, n_c3, l_c3, dt_c3, shape_c3), (_, n_pool, l_pool, dt_pool, shape_pool), (_, n_fc, l_fc, dt_fc, shape_fc) = seen[-3:]
    assert (n_pool - n_c3, n_fc - n_pool) == (1, 1)         # the head: two library launches behind the last product
    assert l_c3.startswith("qlinear_") and "res(u8) relu" in l_c3 and (dt_c3, shape_c3) == (torch.uint8, (2, 2048, 2, 2))
    assert l_pool.startswith("codes_avgpool<u8 avg") and (dt_pool, shape_pool) == (torch.uint8, (2, 2048))
    assert l_fc.startswith("qlinear_") and "res(" not in l_fc and (dt_fc, shape_fc) == (torch.float32, (2, 1000))
    assert y.shape == (2, 1000) and len(torch.unique(y)) > 500
    (codes_in, codes_out), = pooled
    form = (8.0 / 256, 0, 0, 255)
    nhwc = codes_in.cpu().permute(0, 2, 3, 1).contiguous()
    want = ops.codes_avgpool(nhwc, form[:2], form, None).reshape(2, 2048)
    assert len(torch.unique(want)) > 20 and torch.equal(codes_out.cpu(), want)
    chain = torch.nn.functional.adaptive_avg_pool2d(ops.dequantize_codes(codes_in.cpu(), *form[:2]), 1)
    assert torch.equal(want, ops.fq_codes(chain, None, None, None, 0, 255, *form[:2]).reshape(2, 2048))
