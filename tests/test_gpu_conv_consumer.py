"""mctq_codes_im2col_nhwc and consumers.QuantizedConv2d on the GPU.

The patch-matrix kernel is a byte gather: it must equal the CPU route of ops.codes_im2col (itself equal to plain numpy
loops, tests/test_conv_consumer.py) byte for byte and write nothing outside its output.  A fused convolution runs that
kernel and then the integer consumer's kernels, each of which is bit-exact: the GPU layer must equal its own CPU route
bit for bit, and through it the oracle and the float64 bound of tests/test_conv_consumer.py."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import (FAMILIES, GEOMETRIES, check_bottleneck, check_conv_against_oracle_and_float64, check_conv_chain,
                                conv_model, im2col_case, im2col_cases)

GUARD, SENTINEL = 64, 0xA5


def _im2col_into_guarded_buffer(codes, geometry, pad_code):
    """The raw entry point on a device copy of ``codes``, its output in the middle of a sentinel-filled buffer ->
    (patch matrix as numpy, launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = geometry
    B, H, W, C = codes.shape
    ho, wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    n = B * ho * wo * kh * kw * C
    x = torch.from_numpy(codes.copy()).cuda()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    rc = lib.mctq_codes_im2col_nhwc(x.data_ptr(), buf.data_ptr() + GUARD, B, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw, pad_code,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (geometry, C)
    return got[GUARD:GUARD + n].view(codes.dtype).reshape(B * ho * wo, kh * kw * C), launch


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [True, False])
def test_im2col_kernel_equals_the_cpu_route_and_stays_inside_its_output(u8):
    from mct_quantizers_amd.hip import ops
    for case in im2col_cases():
        if case[0] != u8:
            continue
        _, C, geometry, pad_code = case
        codes, want = im2col_case(*case)
        cpu = ops.codes_im2col(torch.from_numpy(codes.copy()), *geometry, pad_code).numpy()
        got, launch = _im2col_into_guarded_buffer(codes, geometry, pad_code)
        assert launch.startswith("codes_im2col<"), launch
        assert np.array_equal(got, cpu) and np.array_equal(got, want), (C, geometry, pad_code)
    # several blocks, the last one partly empty: 243 rows of 18 chunks, 15 rows (270 chunks: a second pass of the lanes) per block
    pad_code = 114 if u8 else -3
    codes, want = im2col_case(u8, 32, GEOMETRIES[0], pad_code, B=3, H=9, W=9)
    cpu = ops.codes_im2col(torch.from_numpy(codes.copy()), *GEOMETRIES[0], pad_code).numpy()
    got, _ = _im2col_into_guarded_buffer(codes, GEOMETRIES[0], pad_code)
    assert got.shape == (243, 288) and np.array_equal(got, cpu) and np.array_equal(got, want)
    # ... and through ops.codes_im2col
    y = ops.codes_im2col(torch.from_numpy(codes.copy()).cuda(), *GEOMETRIES[0], pad_code)
    assert y.is_cuda and y.dtype == (torch.uint8 if u8 else torch.int8) and np.array_equal(y.cpu().numpy(), want)


def _pair_of_models(**kw):
    from mct_quantizers_amd import consumers
    cpu, gpu = conv_model(**kw), conv_model(**kw).cuda()
    for m in (cpu, gpu):
        assert consumers.fuse_linear_consumers(m, uniform_weights=True, convolutions=True) == 1
        assert type(m[1]) is consumers.QuantizedConv2d
    return cpu, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_conv2d_on_gpu_equals_its_cpu_route(family, per_channel):
    from mct_quantizers_amd.hip import native
    for i, (k, s, p, d) in enumerate([GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[4]]):
        cpu, gpu = _pair_of_models(C=16, O=24, k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel,
                                   bias=(i + per_channel) % 2 == 0, seed=i)
        x = torch.randn(2, 16, 5, 7) * 1.5
        want = cpu(x)
        y = gpu(x.cuda())
        assert native.last_launch().startswith("qlinear") and ((" zp," in native.last_launch()) == (family == "uniform"))
        assert y.is_cuda and y.shape == want.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
        y_cl = gpu(x.cuda().contiguous(memory_format=torch.channels_last))           # quantized in place, no transposition
        assert bits_equal(y_cl.cpu().numpy(), want.numpy())
        if i == 0:
            check_conv_against_oracle_and_float64(gpu[1], x.cuda(), y)


@pytest.mark.gpu
def test_quantized_conv2d_rows_from_one_to_past_the_4bit_limit():
    """M = B * Ho * Wo rows reach the consumer: M = 1 (a 3x3 kernel on a 3x3 image, no padding), and with 4-bit weights an M
    on either side of the packed kernels' row limit -- symmetric and uniform codes, and a 16-entry codebook at its own."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    assert consumers._W4_MAX_ROWS == 32 and consumers._LUT4_MAX_ROWS == 1
    for family, bits in (("sym", 4), ("uniform", 4), ("lut16", None)):
        cpu, gpu = _pair_of_models(C=32, O=40, k=3, padding=0, family=family, bits=bits)
        for (b, h, w), packed in (((1, 3, 3), True), ((2, 6, 6), family != "lut16"), ((1, 5, 13), False)):
            x = torch.randn(b, 32, h, w) * 1.5
            want = cpu(x)
            y = gpu(x.cuda())
            rows = b * (h - 2) * (w - 2)
            assert rows in (1, 32, 33) and y.shape == (b, 40, h - 2, w - 2)
            launch = native.last_launch()
            assert (("qlinear_stream_lut4" if family == "lut16" else "qlinear_stream_w4") in launch) == packed, (rows, launch)
            assert bits_equal(y.cpu().numpy(), want.numpy()), (family, rows, first_mismatch(y.cpu().numpy(), want.numpy()))
        assert (gpu[1]._w_idx4 if family == "lut16" else gpu[1]._w_codes4) is not None


@pytest.mark.gpu
def test_chained_convolutions_give_the_same_bits_gpu():
    x, y = check_conv_chain("cuda")
    _, want = check_conv_chain("cpu")                                  # the same seeded stack and input on the CPU route
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())


@pytest.mark.gpu
def test_fused_convolution_replays_in_a_hip_graph():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = conv_model(C=32, O=48, k=3, padding=1).cuda()
    assert consumers.fuse_linear_consumers(model, convolutions=True) == 1
    x = torch.randn(2, 32, 9, 9, device="cuda")
    want = model(x)                                                   # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):
        out = model(static_x)
    assert native.launch_count() - n0 >= 2                            # the patch matrix and the product are both in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(x * 0.5)) and not torch.equal(out, want)


@pytest.mark.gpu
def test_fx_rewrite_of_a_bottleneck_gpu():
    check_bottleneck("cuda")
