"""mctq_qconv_transposed_i8 and consumers.QuantizedConvTranspose2d on the GPU.

The kernel's sum is an exact integer and its epilogue rounds once per operation: the raw entry point must equal the CPU
route of consumers.qconv_transposed_i8 and the numpy loops of tests/test_transposed_consumer.py bit for bit, write nothing
outside its output and name the form and the number of phases it ran; a fused layer on the GPU must equal its own CPU route
bit for bit, and through it the loops and the float64 bound."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_conv_consumer import FAMILIES
from test_transposed_consumer import (ALL, CLASS_GEOMETRIES, GEOMETRIES, SHAPES, Decoder, check_decoder, check_transposed_against_loops_and_float64,
                                      check_transposed_chain, convt_model, edge_cases, extreme_case, extreme_form, out_hw, raw_case,
                                      raw_cases, run_raw_on)

GUARD, SENTINEL = 64, 0xA5
FORMS = {True: (0.37, 114, 0, 255), False: (0.41, -5, -128, 127)}      # codes out: a uint8 / an int8 quantizer


def _raw_into_guarded_buffer(case, out_codes):
    """The raw entry point on device copies of the case's operands, its output in the middle of a sentinel-filled buffer
    -> (output as numpy [B, Ho, Wo, O], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (oph, opw) = case["geometry"]
    B, H, W, C = case["a"].shape
    O = case["w"].shape[0]
    ho, wo = out_hw(H, W, *case["geometry"])
    tdt, *form = consumers._output_form(out_codes)
    ndt = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int8: np.int8}[tdt]
    n = B * ho * wo * O * np.dtype(ndt).itemsize
    dev = lambda v: None if v is None else torch.from_numpy(v.copy()).cuda()          # noqa: E731
    a, ws, zw, bias = (dev(case[k]) for k in ("a", "ws", "zw", "bias"))
    w, rowsum = consumers.pack_transposed_weights(dev(case["w"]), (sh, sw))
    pad = -n % 16                                        # (the rear guard starts where the output ends, aligned or not)
    buf = torch.full((n + pad + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()                                # noqa: E731
    rc = lib.mctq_qconv_transposed_i8(a.data_ptr(), native.CODE_U8 if a.dtype == torch.uint8 else native.CODE_I8, case["za"],
                                      case["sa"], w.data_ptr(), ws.data_ptr(), rowsum.data_ptr(), ptr(zw), ptr(bias),
                                      buf.data_ptr() + GUARD, *form, B, H, W, C, O, kh, kw, sh, sw, ph, pw, oph, opw,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (case["geometry"], C, O)
    return got[GUARD:GUARD + n].view(ndt).reshape(B, ho, wo, O), launch


def _check_raw(case, out_codes, what, spread=True):
    from mct_quantizers_amd.hip import ops
    cpu = run_raw_on(case, "cpu", out_codes).numpy()
    got, launch = _raw_into_guarded_buffer(case, out_codes)
    sh, sw = case["geometry"][1]
    assert launch.startswith("qconv_transposed<"), launch
    assert (" zp," in launch) == (case["zw"] is not None), launch
    assert ("u8 x i8" in launch) == (case["a"].dtype == np.uint8), launch
    assert f",U={sh * sw}," in launch, launch
    assert f",out{4 if out_codes is None else 1}B," in launch, launch
    if out_codes is None:
        assert bits_equal(got, cpu) and bits_equal(got, case["want"]), (what, first_mismatch(got, case["want"]))
    else:
        want = ops.fq_codes(torch.from_numpy(case["want"].copy()), None, None, None, out_codes[2], out_codes[3], out_codes[0],
                            out_codes[1]).numpy()
        assert np.array_equal(got, cpu) and np.array_equal(got, want), what
        assert not spread or len(np.unique(want)) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_qconv_transposed_kernel_equals_the_cpu_route_and_stays_inside_its_output(si, u8, codes_out):
    """Every geometry on B = 2, H = 5, W = 7: phases of 70 pixels (a second block with one partly filled wave and three idle
    ones), of 48, 40 and fewer, and phases without taps."""
    out_codes = FORMS[u8] if codes_out else None
    n = 0
    for case in raw_cases(si):
        if case[0] != u8:
            continue
        _check_raw(raw_case(*case), out_codes, case)
        n += 1
    assert n == len(GEOMETRIES)


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("u8", [True, False])
def test_qconv_transposed_kernel_edge_cases(u8, codes_out):
    out_codes = FORMS[u8] if codes_out else None
    for name, case in edge_cases(u8):
        # (one input pixel and the 1 x 1 output have 64 and 16 output values: too few to ask for a spread of codes)
        _check_raw(case, out_codes, name, spread=case["want"].size > 64)
    # the largest magnitude of the sum (uint8 activations by construction), codes that spread over the result
    if u8:
        c = extreme_case()
        _check_raw(c, extreme_form(c) if codes_out else None, "extreme values")


@pytest.mark.gpu
def test_qconv_transposed_i8_through_python_on_gpu_tensors():
    from mct_quantizers_amd import consumers
    c = raw_case(True, 4, 1, 114, True, True)             # C = 48, O = 16, 3 x 3 stride 2
    y = run_raw_on(c, "cuda")
    assert y.is_cuda and y.dtype == torch.float32 and bits_equal(y.cpu().numpy(), c["want"])
    codes = run_raw_on(c, "cuda", (0.37, 114, 0, 255))
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), run_raw_on(c, "cpu", (0.37, 114, 0, 255)))
    t = lambda v: torch.from_numpy(v.copy()).cuda()      # noqa: E731
    packed = consumers.pack_transposed_weights(t(c["w"]), 2)
    assert tuple(packed[0].shape) == (4, 16, 192) and bits_equal(run_raw_on(c, "cuda", packed=packed).cpu().numpy(), c["want"])
    f = consumers.qconv_transposed_i8
    with pytest.raises(NotImplementedError):             # C = 24: the CPU route's, never quietly another path
        f(torch.zeros(1, 4, 4, 24, dtype=torch.uint8, device="cuda"), 0, 0.1, torch.zeros(16, 2, 2, 24, dtype=torch.int8, device="cuda"),
          t(c["ws"]), None, 2, 2)
    with pytest.raises(NotImplementedError):             # stride 5
        f(t(c["a"]), 114, 0.1, torch.zeros(16, 5, 5, 48, dtype=torch.int8, device="cuda"), t(c["ws"]), None, 5, 5)
    args = (t(c["a"]), 114, c["sa"], t(c["w"]), t(c["ws"]), None, 3, 2, 1, 1)
    with pytest.raises(TypeError):                       # a non-contiguous packed form
        f(*args, packed=(packed[0].transpose(1, 2).contiguous().transpose(1, 2), packed[1]))
    with pytest.raises(TypeError):                       # the layout of another stride
        f(*args, packed=consumers.pack_transposed_weights(t(c["w"]), 1))
    from mct_quantizers_amd.hip import native
    misaligned = torch.zeros(packed[0].numel() + 16, dtype=torch.int8, device="cuda")[4:4 + packed[0].numel()].view(packed[0].shape)
    misaligned.copy_(packed[0])
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 == 4
    with pytest.raises(Exception, match="16-byte aligned"):
        f(*args, packed=(misaligned, packed[1]))
    assert native.last_launch().startswith("qconv_transposed<")       # (the last launch is still the good one above)


def _pair_of_models(**kw):
    from mct_quantizers_amd import consumers
    cpu, gpu = convt_model(**kw), convt_model(**kw).cuda()
    for m in (cpu, gpu):
        assert consumers.fuse_linear_consumers(m, uniform_weights=True, transposed=True) == 1
        assert type(m[1]) is consumers.QuantizedConvTranspose2d
    return cpu, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantized_conv_transpose2d_on_gpu_equals_its_cpu_route(family, per_channel):
    from mct_quantizers_amd.hip import native
    for i, (k, s, p, op) in enumerate(CLASS_GEOMETRIES):
        cpu, gpu = _pair_of_models(k=k, stride=s, padding=p, output_padding=op, family=family, per_channel=per_channel,
                                   bias=(i + per_channel) % 2 == 0, seed=i)
        x = torch.randn(2, 32, 5, 7) * 1.5
        want = cpu(x)
        y = gpu(x.cuda())
        launch = native.last_launch()
        phases = gpu[1].stride[0] * gpu[1].stride[1]
        assert launch.startswith("qconv_transposed<") and ((" zp," in launch) == (family == "uniform")) and f",U={phases}," in launch, launch
        assert y.is_cuda and y.shape == want.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
        y_cl = gpu(x.cuda().contiguous(memory_format=torch.channels_last))           # quantized in place, no transposition
        assert bits_equal(y_cl.cpu().numpy(), want.numpy())
        if i == 1 and per_channel:
            check_transposed_against_loops_and_float64(gpu[1], x.cuda(), y)


@pytest.mark.gpu
def test_chained_transposed_stack_gives_the_same_bits_gpu():
    x, y = check_transposed_chain("cuda")
    _, want = check_transposed_chain("cpu")                           # the same seeded stack and input on the CPU route
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())


@pytest.mark.gpu
def test_rewritten_decoder_stage_on_gpu_equals_its_cpu_run():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    gm, (x, skip), y = check_decoder("cuda")
    n0 = native.launch_count()
    gm.get_submodule("up_qlinear")(torch.zeros(1, 32, 4, 4, dtype=torch.uint8, device="cuda"))
    assert native.launch_count() == n0 + 1 and native.last_launch().startswith("qconv_transposed<u8 x i8,in1B,out1B,U=4,")
    gm_cpu, n = consumers.fuse_linear_consumers_fx(Decoder().eval(), transposed=True, **ALL)
    assert n == 3
    with torch.no_grad():
        want = gm_cpu(x.cpu(), skip.cpu()).numpy()
    assert bits_equal(y.cpu().numpy(), want), first_mismatch(y.cpu().numpy(), want)
