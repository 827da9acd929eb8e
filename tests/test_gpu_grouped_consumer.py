"""mctq_qconv_grouped_i8 and consumers.QuantizedGroupedConv2d on the GPU.

The kernel's sum is an exact integer and its epilogue rounds once per operation: the raw entry point must equal the CPU
route of consumers.qconv_grouped_i8 and the numpy loops of tests/test_grouped_consumer.py bit for bit, write nothing outside
its output and name the piece size and form it ran; a fused layer on the GPU must equal its own CPU route bit for bit, and
through it the loops and the float64 bound."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES
from test_dw_consumer import DW_GEOMETRIES
from test_grouped_consumer import (BOTTLENECK_SWITCHES, GROUP_SHAPES, POINTWISE, UNPADDED_3X3, Bottleneck, bottleneck_layer_by_layer,
                                   check_bottleneck, check_grouped_against_loops_and_float64, check_grouped_chain, extreme_case,
                                   extreme_form, grouped_model, piece_size, raw_case, raw_cases, run_raw_on)

GUARD, SENTINEL = 64, 0xA5
FORMS = {True: (0.37, 114, 0, 255), False: (0.41, -5, -128, 127)}      # codes out: a uint8 / an int8 quantizer


def _raw_into_guarded_buffer(case, out_codes):
    """The raw entry point on device copies of the case's operands, its output in the middle of a sentinel-filled buffer
    -> (output as numpy [B, Ho, Wo, O], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case["geometry"]
    B, H, W, C = case["a"].shape
    O, G = case["w"].shape[0], case["groups"]
    ho, wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    tdt, *form = consumers._output_form(out_codes)
    ndt = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int8: np.int8}[tdt]
    n = B * ho * wo * O * np.dtype(ndt).itemsize
    dev = lambda v: None if v is None else torch.from_numpy(v.copy()).cuda()          # noqa: E731
    a, ws, zw, bias = (dev(case[k]) for k in ("a", "ws", "zw", "bias"))
    w, rowsum = consumers.pack_grouped_weights(dev(case["w"]), G)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()                                # noqa: E731
    rc = lib.mctq_qconv_grouped_i8(a.data_ptr(), native.CODE_U8 if a.dtype == torch.uint8 else native.CODE_I8, case["za"],
                                   case["sa"], w.data_ptr(), ws.data_ptr(), rowsum.data_ptr(), ptr(zw), ptr(bias),
                                   buf.data_ptr() + GUARD, *form, B, H, W, C, O, G, kh, kw, sh, sw, ph, pw, dh, dw,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (case["geometry"], C, O, G)
    return got[GUARD:GUARD + n].view(ndt).reshape(B, ho, wo, O), launch


def _check_raw(case, out_codes, what):
    from mct_quantizers_amd.hip import ops
    cpu = run_raw_on(case, "cpu", out_codes).numpy()
    got, launch = _raw_into_guarded_buffer(case, out_codes)
    assert launch.startswith("qconv_grouped<"), launch
    assert (" zp," in launch) == (case["zw"] is not None), launch
    assert ("u8 x i8" in launch) == (case["a"].dtype == np.uint8), launch
    assert f",U={piece_size(case['a'].shape[3] // case['groups'])}," in launch, launch
    assert f",out{4 if out_codes is None else 1}B," in launch, launch
    if out_codes is None:
        assert bits_equal(got, cpu) and bits_equal(got, case["want"]), (what, first_mismatch(got, case["want"]))
    else:
        want = ops.fq_codes(torch.from_numpy(case["want"].copy()), None, None, None, out_codes[2], out_codes[3], out_codes[0],
                            out_codes[1]).numpy()
        assert np.array_equal(got, cpu) and np.array_equal(got, want), what
        assert len(np.unique(want)) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("si", range(len(GROUP_SHAPES)))
def test_qconv_grouped_kernel_equals_the_cpu_route_and_stays_inside_its_output(si, u8, codes_out):
    """Every geometry on B = 2, H = 5, W = 7 -- 70 pixels at stride 1: a second block with one partly filled wave and three
    idle ones."""
    out_codes = FORMS[u8] if codes_out else None
    n = 0
    for case in raw_cases(si):
        if case[0] != u8:
            continue
        _check_raw(raw_case(*case), out_codes, case)
        n += 1
    assert n == 6 * 3


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
def test_qconv_grouped_kernel_edge_cases(u8, codes_out):
    out_codes = FORMS[u8] if codes_out else None
    za = 114 if u8 else -3
    for si in (0, 2, 4, 7):                                           # each piece size, and the two grid slices
        # one output pixel: a 3 x 3 kernel on a 3 x 3 image without padding
        one = raw_case(u8, si, UNPADDED_3X3, za, True, True, B=1, H=3, W=3)
        assert one["want"].shape == (1, 1, 1, GROUP_SHAPES[si][1] * GROUP_SHAPES[si][2])
        _check_raw(one, out_codes, ("M = 1", si))
        # 243 pixels: four blocks, the last with three pixels
        _check_raw(raw_case(u8, si, 0, za, si != 2, si != 4, B=3, H=9, W=9), out_codes, ("243 pixels", si))
    # a 1 x 1 kernel on 64 channels per group: Kg = 64, no K tail and no second K step
    _check_raw(raw_case(u8, 6, POINTWISE, za, True, True), out_codes, "Kg = 64")
    # the largest magnitude of the sum (uint8 activations by construction), codes that spread over the result
    if u8:
        c = extreme_case()
        _check_raw(c, extreme_form(c) if codes_out else None, "extreme values")


@pytest.mark.gpu
def test_qconv_grouped_i8_through_python_on_gpu_tensors():
    from mct_quantizers_amd import consumers
    c = raw_case(True, 2, 1, 114, True, True)
    y = run_raw_on(c, "cuda")
    assert y.is_cuda and y.dtype == torch.float32 and bits_equal(y.cpu().numpy(), c["want"])
    codes = run_raw_on(c, "cuda", (0.37, 114, 0, 255))
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), run_raw_on(c, "cpu", (0.37, 114, 0, 255)))
    t = lambda v: torch.from_numpy(v.copy()).cuda()      # noqa: E731
    with pytest.raises(NotImplementedError):             # Cg = 2: the CPU route's, never quietly another path
        consumers.qconv_grouped_i8(torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device="cuda"), 0, 0.1,
                                   torch.zeros(2, 3, 3, 2, dtype=torch.int8, device="cuda"), t(c["ws"][:2]), None, 2, 3, 1, 1)


def _pair_of_models(**kw):
    from mct_quantizers_amd import consumers
    cpu, gpu = grouped_model(**kw), grouped_model(**kw).cuda()
    for m in (cpu, gpu):
        assert consumers.fuse_linear_consumers(m, uniform_weights=True, grouped=True) == 1
        assert type(m[1]) is consumers.QuantizedGroupedConv2d
    return cpu, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_grouped_conv2d_on_gpu_equals_its_cpu_route(family, per_channel):
    from mct_quantizers_amd.hip import native
    for i, (k, s, p, d) in enumerate([DW_GEOMETRIES[0], DW_GEOMETRIES[1], DW_GEOMETRIES[3]]):
        cpu, gpu = _pair_of_models(k=k, stride=s, padding=p, dilation=d, family=family, per_channel=per_channel,
                                   bias=(i + per_channel) % 2 == 0, seed=i)
        x = torch.randn(2, 32, 5, 7) * 1.5
        want = cpu(x)
        y = gpu(x.cuda())
        launch = native.last_launch()
        assert launch.startswith("qconv_grouped<") and ((" zp," in launch) == (family == "uniform")) and ",U=8," in launch, launch
        assert y.is_cuda and y.shape == want.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
        y_cl = gpu(x.cuda().contiguous(memory_format=torch.channels_last))           # quantized in place, no transposition
        assert bits_equal(y_cl.cpu().numpy(), want.numpy())
        if i == 0 and per_channel:
            check_grouped_against_loops_and_float64(gpu[1], x.cuda(), y)


@pytest.mark.gpu
def test_chained_grouped_stack_gives_the_same_bits_gpu():
    x, y = check_grouped_chain("cuda")
    _, want = check_grouped_chain("cpu")                              # the same seeded stack and input on the CPU route
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())


@pytest.mark.gpu
def test_fx_rewrite_of_a_resnext_bottleneck_gpu():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    gm, x, y = check_bottleneck("cuda")
    n0 = native.launch_count()
    gm.get_submodule("c2_qlinear")(torch.zeros(1, 64, 4, 4, dtype=torch.uint8, device="cuda"))
    assert native.launch_count() == n0 + 1 and native.last_launch().startswith("qconv_grouped<u8 x i8,in1B,out1B,U=4,")
    # the same seeded block, rewritten, on the CPU route, and that route layer by layer
    gm_cpu, n = consumers.fuse_linear_consumers_fx(Bottleneck(), grouped=True, **BOTTLENECK_SWITCHES)
    assert n == 3
    want = gm_cpu(x.cpu()).detach().numpy()
    assert bits_equal(y.detach().cpu().numpy(), want), first_mismatch(y.detach().cpu().numpy(), want)
    assert bits_equal(want, bottleneck_layer_by_layer(x.cpu()).detach().numpy())


@pytest.mark.gpu
def test_fused_grouped_convolution_replays_in_a_hip_graph():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = grouped_model(k=3, padding=1).cuda()
    assert consumers.fuse_linear_consumers(model, grouped=True) == 1
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
    assert native.launch_count() - n0 >= 1 and native.last_launch().startswith("qconv_grouped<")     # the convolution is in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(x * 0.5)) and not torch.equal(out, want)
