"""mctq_qconv_dw_i8 and consumers.QuantizedDepthwiseConv2d on the GPU.

The kernel's sum is an exact integer and its epilogue rounds once per operation: the raw entry point must equal the CPU
route of consumers.qconv_dw_i8 and the numpy loops of tests/test_dw_consumer.py bit for bit and write nothing outside its
output; a fused layer on the GPU must equal its own CPU route bit for bit, and through it the oracle and the float64 bound."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES
from test_dw_consumer import (DW_GEOMETRIES, InvertedResidual, check_dw_against_oracle_and_float64, check_dw_chain, check_inverted_residual, dw_model,
                              extreme_case, raw_case, raw_cases, run_raw_on)

GUARD, SENTINEL = 64, 0xA5
FORMS = {False: None, True: {True: (0.37, 114, 0, 255), False: (0.41, -5, -128, 127)}}      # codes out: a uint8 / an int8 quantizer


def _raw_into_guarded_buffer(case, out_codes):
    """The raw entry point on device copies of the case's operands, its output in the middle of a sentinel-filled buffer
    -> (output as numpy [B, Ho, Wo, C], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case["geometry"]
    B, H, W, C = case["a"].shape
    ho, wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    tdt, *form = consumers._output_form(out_codes)
    ndt = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int8: np.int8}[tdt]
    n = B * ho * wo * C * np.dtype(ndt).itemsize
    dev = lambda v: None if v is None else torch.from_numpy(v.copy()).cuda()          # noqa: E731
    a, w, ws, zw, bias = (dev(case[k]) for k in ("a", "w", "ws", "zw", "bias"))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()                                # noqa: E731
    rc = lib.mctq_qconv_dw_i8(a.data_ptr(), native.CODE_U8 if a.dtype == torch.uint8 else native.CODE_I8, case["za"], case["sa"],
                              w.data_ptr(), ws.data_ptr(), ptr(zw), ptr(bias), buf.data_ptr() + GUARD, *form, B, H, W, C,
                              kh, kw, sh, sw, ph, pw, dh, dw, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (case["geometry"], C)
    return got[GUARD:GUARD + n].view(ndt).reshape(B, ho, wo, C), launch


def _check_raw(case, out_codes, what):
    from mct_quantizers_amd.hip import ops
    cpu = run_raw_on(case, "cpu", out_codes).numpy()
    got, launch = _raw_into_guarded_buffer(case, out_codes)
    assert launch.startswith("qconv_dw<"), launch
    assert (" zp," in launch) == (case["zw"] is not None), launch
    assert ("u8 x i8" in launch) == (case["a"].dtype == np.uint8), launch
    if out_codes is None:
        assert bits_equal(got, cpu) and bits_equal(got, case["want"]), (what, first_mismatch(got, case["want"]))
    else:
        want = ops.fq_codes(torch.from_numpy(case["want"].copy()), None, None, None, out_codes[2], out_codes[3], out_codes[0],
                            out_codes[1]).numpy()
        assert np.array_equal(got, cpu) and np.array_equal(got, want), what
        assert len(np.unique(want)) > 8


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
def test_qconv_dw_kernel_equals_the_cpu_route_and_stays_inside_its_output(u8, codes_out):
    out_codes = FORMS[codes_out][u8] if codes_out else None
    n = 0
    for case in raw_cases():
        if case[0] != u8:
            continue
        _check_raw(raw_case(*case), out_codes, case)
        n += 1
    assert n == 2 * 6 * 3
    za = 114 if u8 else -3
    # (a) one output pixel: a 3 x 3 kernel on a 3 x 3 image without padding
    one = raw_case(u8, 16, len(DW_GEOMETRIES), za, True, True, B=1, H=3, W=3)
    assert one["want"].shape == (1, 1, 1, 16)
    _check_raw(one, out_codes, "M = 1")
    # (b) several blocks, the last one partly empty: 243 pixels of 2 chunks over 256-lane blocks
    _check_raw(raw_case(u8, 32, 0, za, True, True, B=3, H=9, W=9), out_codes, "486 chunks")
    # (d) 65 chunks per pixel: pixels straddle the 256-lane blocks
    _check_raw(raw_case(u8, 1040, 0, za, True, False, B=1, H=3, W=3), out_codes, "C = 1040")
    # (c) the largest magnitude of a 7 x 7 kernel's sum (uint8 activations by construction)
    if u8:                                                            # (sums of -3.2 million: a form whose codes they spread over)
        _check_raw(extreme_case(), (4.0, 250, 0, 255) if codes_out else None, "extreme values")


@pytest.mark.gpu
def test_qconv_dw_i8_through_python_on_gpu_tensors():
    c = raw_case(True, 48, 1, 114, True, True)
    y = run_raw_on(c, "cuda")
    assert y.is_cuda and y.dtype == torch.float32 and bits_equal(y.cpu().numpy(), c["want"])
    codes = run_raw_on(c, "cuda", (0.37, 114, 0, 255))
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), run_raw_on(c, "cpu", (0.37, 114, 0, 255)))


def _pair_of_models(**kw):
    from mct_quantizers_amd import consumers
    cpu, gpu = dw_model(**kw), dw_model(**kw).cuda()
    for m in (cpu, gpu):
        assert consumers.fuse_linear_consumers(m, uniform_weights=True, depthwise=True) == 1
        assert type(m[1]) is consumers.QuantizedDepthwiseConv2d
    return cpu, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_depthwise_conv2d_on_gpu_equals_its_cpu_route(family, per_channel):
    from mct_quantizers_amd.hip import native
    for i, (k, s, p, d) in enumerate([DW_GEOMETRIES[0], DW_GEOMETRIES[1], DW_GEOMETRIES[3]]):
        cpu, gpu = _pair_of_models(k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel,
                                   bias=(i + per_channel) % 2 == 0, seed=i)
        x = torch.randn(2, 16, 5, 7) * 1.5
        want = cpu(x)
        y = gpu(x.cuda())
        assert native.last_launch().startswith("qconv_dw<") and ((" zp," in native.last_launch()) == (family == "uniform"))
        assert y.is_cuda and y.shape == want.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
        y_cl = gpu(x.cuda().contiguous(memory_format=torch.channels_last))           # quantized in place, no transposition
        assert bits_equal(y_cl.cpu().numpy(), want.numpy())
        if i == 0 and per_channel:
            check_dw_against_oracle_and_float64(gpu[1], x.cuda(), y)


@pytest.mark.gpu
def test_chained_depthwise_block_gives_the_same_bits_gpu():
    x, y = check_dw_chain("cuda")
    _, want = check_dw_chain("cpu")                                    # the same seeded stack and input on the CPU route
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())


@pytest.mark.gpu
def test_fused_depthwise_convolution_replays_in_a_hip_graph():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = dw_model(C=32, k=3, padding=1).cuda()
    assert consumers.fuse_linear_consumers(model, depthwise=True) == 1
    x = torch.randn(2, 32, 9, 9, device="cuda")
    want = model(x)                                                   # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # strictly sequential: the codes, then the convolution
        out = model(static_x)
    assert native.launch_count() - n0 >= 1 and native.last_launch().startswith("qconv_dw<")     # the convolution is in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(x * 0.5)) and not torch.equal(out, want)


@pytest.mark.gpu
def test_fx_rewrite_of_an_inverted_residual_gpu():
    from mct_quantizers_amd import consumers
    _, x, y = check_inverted_residual("cuda")
    # the same seeded block, fused, on the CPU route (a wrapper left unfused on CPU tensors is not what a GPU machine runs)
    gm, n = consumers.fuse_linear_consumers_fx(InvertedResidual(), depthwise=True)
    assert n == 3
    want = gm(x.cpu())
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
