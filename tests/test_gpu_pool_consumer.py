"""mctq_codes_maxpool_nhwc, consumers.QuantizedMaxPool2d and the ``pools`` rewrites on the GPU.

A maximum of bytes is exact: the raw entry point must equal the CPU route of ops.codes_maxpool (ATen's max pool of the codes)
and the numpy loops of tests/test_pool_consumer.py byte for byte and write nothing outside its output; the module and the
rewritten models must equal their CPU routes, and the rewrite with ``pools=True`` the same rewrite without it, bit for bit
(tests/test_pool_consumer.py says why the float32 products of those models are exact)."""
import numpy as np
import pytest
import torch

from test_pool_consumer import Stem, check_module, pool_case, pool_cases, stem_input, vgg, vgg_input

GUARD, SENTINEL = 64, 0xA5


def _raw_into_guarded_buffer(codes, geometry):
    """The raw entry point on a device copy of ``codes``, its output in the middle of a sentinel-filled buffer -> (output as numpy
    [B, Ho, Wo, C], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw), ceil_mode = geometry
    B, H, W, C = codes.shape
    ho, wo = ops._pool_out_size(H, kh, sh, ph, dh, ceil_mode), ops._pool_out_size(W, kw, sw, pw, dw, ceil_mode)
    n = B * ho * wo * C
    x = torch.from_numpy(codes.copy()).cuda()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and x.data_ptr() % 16 == 0
    rc = lib.mctq_codes_maxpool_nhwc(x.data_ptr(), buf.data_ptr() + GUARD, native.CODE_U8 if codes.dtype == np.uint8 else native.CODE_I8,
                                     B, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw, int(ceil_mode), ho, wo,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (geometry, C)
    return got[GUARD:GUARD + n].view(codes.dtype).reshape(B, ho, wo, C), launch


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [True, False])
def test_codes_maxpool_kernel_equals_the_cpu_route_and_stays_inside_its_output(u8):
    from mct_quantizers_amd.hip import ops
    n = 0
    for case_u8, C, g, shape in pool_cases():
        if case_u8 != u8:
            continue
        codes, want = pool_case(u8, C, g, **shape)
        k, s, p, d, ceil_mode = g
        cpu = ops.codes_maxpool(torch.from_numpy(codes.copy()), k, s, p, d, ceil_mode).numpy()
        got, launch = _raw_into_guarded_buffer(codes, g)
        assert launch.startswith("codes_maxpool<") and (("u8 max" in launch) == u8), launch
        assert got.shape == cpu.shape and np.array_equal(got, cpu) and np.array_equal(got, want), (u8, C, g, shape)
        if u8:
            assert got.max() >= 250 and got.min() < 128        # codes on both sides of 128 among the maxima
        else:
            assert got[-1].max() < 0 and got[0].max() > 100   # the all-negative image stays negative
        n += 1
    assert n == 2 * 9 + 1


@pytest.mark.gpu
def test_codes_maxpool_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    for u8 in (True, False):
        codes, want = pool_case(u8, 48, ((3, 3), (2, 2), (1, 1), (1, 1), True))
        n0 = native.launch_count()
        y = ops.codes_maxpool(torch.from_numpy(codes.copy()).cuda(), 3, 2, 1, ceil_mode=True)
        assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_maxpool<")
        assert y.is_cuda and y.is_contiguous() and y.dtype == (torch.uint8 if u8 else torch.int8) and np.array_equal(y.cpu().numpy(), want)
    with pytest.raises(NotImplementedError):
        ops.codes_maxpool(torch.zeros(1, 4, 4, 24, dtype=torch.uint8, device="cuda"), 2)
    assert ops.codes_maxpool(torch.zeros(0, 4, 4, 16, dtype=torch.uint8, device="cuda"), 2).shape == (0, 2, 2, 16)


@pytest.mark.gpu
def test_quantized_max_pool2d_on_gpu_equals_its_cpu_route():
    from mct_quantizers_amd.hip import native
    want = check_module("cpu")
    got = check_module("cuda")
    assert native.last_launch().startswith("codes_maxpool<")
    assert len(got) == len(want) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["module", "functional"])
def test_stem_style_model_gives_the_bits_of_the_rewrite_without_pools_gpu(how):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    x = stem_input("cuda")
    for switches in (dict(), dict(shared_holders=True)):
        gm, n = consumers.fuse_linear_consumers_fx(Stem(how).cuda(), pools=True, **switches)
        gm0, n0 = consumers.fuse_linear_consumers_fx(Stem(how).cuda(), **switches)
        assert (n, n0) == (2, 0)
        seen = []
        hook = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedMaxPool2d)).register_forward_hook(
            lambda m, args, out: seen.append(native.last_launch()))
        y, y0 = gm(x), gm0(x)
        hook.remove()
        assert len(seen) == 1 and seen[0].startswith("codes_maxpool<")
        assert y.shape == (2, 16, 5, 4) and len(torch.unique(y)) > 50 and torch.equal(y, y0)


def _vgg_arms(device):
    from mct_quantizers_amd import consumers
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True)
    gm, n = consumers.fuse_linear_consumers_fx(vgg(device), pools=True, **switches)
    gm0, n0 = consumers.fuse_linear_consumers_fx(vgg(device), **switches)
    assert (n, n0) == (3, 1)
    return gm, gm0


@pytest.mark.gpu
def test_vgg_style_model_gives_the_bits_of_the_rewrite_without_pools_gpu():
    from mct_quantizers_amd import consumers
    gm, gm0 = _vgg_arms("cuda")
    x = vgg_input("cuda")
    y, y0 = gm(x), gm0(x)
    assert y.shape == (2, 16, 3, 2) and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    assert torch.equal(y.cpu(), _vgg_arms("cpu")[0](x.cpu()))
    # the Sequential rewrite of the same stack
    seq, seq0 = vgg("cuda"), vgg("cuda")
    assert consumers.fuse_linear_consumers(seq, convolutions=True, pools=True) == 3
    assert consumers.fuse_linear_consumers(seq0, convolutions=True) == 1
    assert torch.equal(seq(x), y) and torch.equal(seq0(x), y)


@pytest.mark.gpu
def test_rewritten_vgg_style_model_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = _vgg_arms("cuda")
    x = vgg_input("cuda")
    want = gm(x)                                                      # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # strictly sequential: no parallel branches
        out = gm(static_x)
    assert native.launch_count() - n0 >= 5                            # three consumers and two pools are in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5)) and not torch.equal(out, want)
