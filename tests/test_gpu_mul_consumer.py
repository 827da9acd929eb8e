"""mctq_codes_mul_nhwc, consumers.QuantizedMul and the ``muls`` rewrite on the GPU.

The code of a product is exact arithmetic on at most 256 x 256 pairs of codes per triple of forms: the raw entry point must
equal the CPU route of ops.codes_mul and the numpy definition of tests/test_mul_consumer.py byte for byte, for every pair and
every combination of code types, and write nothing outside its output; the module and the rewritten blocks must equal their CPU
routes, and the rewrite with ``muls=True`` the same rewrite without it, bit for bit (tests/test_pool_consumer.py says why the
float32 products of those blocks are exact)."""
import numpy as np
import pytest
import torch

from test_mul_consumer import (COMBOS, GATES, SE, SMALL, TORCH_ROUTE_SHAPES, Gated, as_tensor, block_input, check_mul_module,
                               check_refusals, mul_reference, pairs_case, rewritten, small_case, small_cases, torch_route_case)

GUARD, SENTINEL = 64, 0xA5


def _raw_into_guarded_buffer(a, g, out_form, gate_form, gate_pixels):
    """The raw entry point on device copies of the operands, its output in the middle of a sentinel-filled buffer -> (output as
    numpy in a's shape, launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    scale, zp, qmin, qmax = out_form
    tdt, ocode = ops._code_dtype(qmin, qmax)
    (ac, sa, za), (gc, sg, zg) = as_tensor(a, "cuda"), as_tensor(g, "cuda")
    C = ac.shape[-1]
    n = ac.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and ac.data_ptr() % 16 == 0 and gc.data_ptr() % 16 == 0
    if gate_form is None:
        g_code, g_qmin, g_qmax = ops._code_of(gc), 0, 0
    else:
        g_code, (g_qmin, g_qmax) = ops._code_dtype(*gate_form)[1], gate_form
    rc = lib.mctq_codes_mul_nhwc(ac.data_ptr(), ops._code_of(ac), sa, za, gc.data_ptr(), g_code, sg, zg, int(gate_form is not None),
                                 g_qmin, g_qmax, gate_pixels, buf.data_ptr() + GUARD, ocode, n // C, C, scale, zp, qmin, qmax,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (a[0].shape, gate_pixels)
    return got[GUARD:GUARD + n].view(np.uint8 if tdt == torch.uint8 else np.int8).reshape(a[0].shape), launch


def _types(a, g, out_form, gate_form):
    name = lambda signed: "i8" if signed else "u8"           # noqa: E731
    g_signed = (gate_form[0] < 0) if gate_form is not None else g[0].dtype == np.int8
    return f"{name(a[0].dtype == np.int8)} * {name(g_signed)} -> {name(out_form[2] < 0)}"


@pytest.mark.gpu
@pytest.mark.parametrize("combo", COMBOS)
def test_codes_mul_kernel_equals_the_cpu_route_for_every_pair_of_codes(combo):
    from mct_quantizers_amd.hip import ops
    for which in (0, 1):
        a, g, out_form, want = pairs_case(combo, which)
        cpu = ops.codes_mul(as_tensor(a), as_tensor(g), out_form).numpy()
        got, launch = _raw_into_guarded_buffer(a, g, out_form, None, 0)
        assert launch.startswith("codes_mul<") and ("<" + _types(a, g, out_form, None) + " same,") in launch, launch
        assert got.dtype == cpu.dtype and np.array_equal(got, cpu) and np.array_equal(got, want), (combo, which)
        assert got.min() == out_form[2] and got.max() == out_form[3] and len(np.unique(got)) > 50


@pytest.mark.gpu
def test_codes_mul_kernel_on_the_smallest_shapes_of_every_gate_form():
    """One pixel; the gate row is the pixel; image boundaries inside a wavefront and a partly empty last block; a row longer than
    a wavefront -- as same-shape codes, as a code gate and as a float32 gate (rounding ties, both clamps, +-inf and NaN in it).
    The launch note names the form that ran."""
    from mct_quantizers_amd.hip import ops
    n = 0
    for index, gate in small_cases():
        a, g, out_form, gate_form, want = small_case(index, gate)
        cpu = ops.codes_mul(as_tensor(a), as_tensor(g), out_form, gate_form).numpy()
        got, launch = _raw_into_guarded_buffer(a, g, out_form, gate_form, 0 if gate == "same" else SMALL[index][1])
        assert launch.startswith("codes_mul<") and ("<" + _types(a, g, out_form, gate_form) + " " + gate + ",") in launch, launch
        assert np.array_equal(got, cpu) and np.array_equal(got, want), (index, gate)
        n += 1
    assert n == 11 and set(GATES) == {gate for _, gate in small_cases()}
    # the operand with itself (x * x): a and g may be one buffer
    a, _, out_form, _, _ = small_case(2, "same")
    got, _ = _raw_into_guarded_buffer(a, a, out_form, None, 0)
    assert np.array_equal(got, mul_reference(a, a, out_form))


@pytest.mark.gpu
def test_codes_mul_refusals_come_before_any_launch():
    from mct_quantizers_amd.hip import native
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 2048 + 255) // 256 * 256          # (the checks look 112 bytes below it)
    check_refusals(native.load(), native, P=base)
    check_refusals(native.load(), native)


@pytest.mark.gpu
def test_codes_mul_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    for index, gate in ((2, "same"), (2, "row"), (2, "row f32"), (3, "row"), (3, "row f32"), (1, "row f32")):
        a, g, out_form, gate_form, want = small_case(index, gate)
        n0 = native.launch_count()
        y = ops.codes_mul(as_tensor(a, "cuda"), as_tensor(g, "cuda"), out_form, gate_form)
        assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_mul<"), (index, gate)
        assert (" " + gate + ",") in native.last_launch()
        assert y.is_cuda and y.is_contiguous() and y.dtype == (torch.uint8 if out_form[2] >= 0 else torch.int8)
        assert np.array_equal(y.cpu().numpy(), want)
        if gate == "row":                                    # the gate first: the same launch
            n0 = native.launch_count()
            y = ops.codes_mul(as_tensor(g, "cuda"), as_tensor(a, "cuda"), out_form)
            assert native.launch_count() - n0 == 1 and " row," in native.last_launch()
            assert np.array_equal(y.cpu().numpy(), want)
    # the torch route: C = 24, the other broadcasts, operands of different rank
    for index in range(len(TORCH_ROUTE_SHAPES)):
        for float_gate in (False, True):
            a, g, out_form, gate_form, want = torch_route_case(index, float_gate)
            n0 = native.launch_count()
            y = ops.codes_mul(as_tensor(a, "cuda"), as_tensor(g, "cuda"), out_form, gate_form)
            assert y.is_cuda and y.is_contiguous() and not native.last_launch().startswith("codes_mul<")
            assert native.launch_count() - n0 >= 1 + float_gate           # the quantize launch(es) of the definition
            assert np.array_equal(y.cpu().numpy(), want), (index, float_gate)
            assert torch.equal(y.cpu(), ops.codes_mul(as_tensor(a), as_tensor(g), out_form, gate_form))
    # non-contiguous operands are made contiguous, an empty batch launches nothing
    a, g, out_form, _, want = small_case(2, "row")
    x = as_tensor(a, "cuda")[0].permute(1, 0, 2).contiguous().permute(1, 0, 2)
    gate = torch.repeat_interleave(as_tensor(g, "cuda")[0], 2, dim=-1)[..., ::2]                 # every other byte of a wider row
    assert not x.is_contiguous() and not gate.is_contiguous()
    n0 = native.launch_count()
    y = ops.codes_mul((x, *a[1:]), (gate, *g[1:]), out_form)
    assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_mul<") and np.array_equal(y.cpu().numpy(), want)
    n0 = native.launch_count()
    empty = ops.codes_mul((torch.zeros(0, 4, 16, dtype=torch.uint8, device="cuda"), 0.1, 0),
                          (torch.zeros(0, 1, 16, dtype=torch.int8, device="cuda"), 0.1, 0), (0.03, -5, -128, 127))
    assert empty.shape == (0, 4, 16) and empty.dtype == torch.int8 and empty.is_cuda and native.launch_count() == n0


@pytest.mark.gpu
def test_quantized_mul_on_gpu_equals_its_cpu_route():
    want = check_mul_module("cpu")
    got = check_mul_module("cuda")
    assert len(got) == len(want) == 21 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("make", [SE, Gated])
def test_rewritten_blocks_give_the_bits_of_the_rewrite_without_muls_gpu(make):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    x = block_input("cuda")
    gm, n = rewritten(make, "cuda")
    gm0, n0 = rewritten(make, "cuda", muls=False)
    assert n == n0 == (4 if make is SE else 3)
    qmul = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedMul))
    seen = []

    def before(m, args):
        seen.append(native.launch_count())

    def after(m, args, out):
        seen.append((native.launch_count(), native.last_launch(), [(a.dtype, tuple(a.shape)) for a in args]))

    hooks = [qmul.register_forward_pre_hook(before), qmul.register_forward_hook(after)]
    y, y0 = gm(x), gm0(x)
    for h in hooks:
        h.remove()
    count0, (count1, launch, operands) = seen
    assert count1 - count0 == 1 and launch.startswith("codes_mul<")            # the module is that one launch
    if make is SE:                                           # A's codes from the convolution in front; the gate, whose holder was absorbed, in float32
        assert operands == [(torch.uint8, (2, 16, 4, 4)), (torch.float32, (2, 16, 1, 1))] and "<u8 * u8 -> u8 row f32," in launch
    else:
        assert operands == [(torch.uint8, (2, 16, 4, 4)), (torch.int8, (2, 16, 4, 4))] and "<u8 * i8 -> u8 same," in launch
    assert y.shape == (2, 16, 4, 4) and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    assert torch.equal(y.cpu(), rewritten(make)[0](x.cpu()))
    assert not [m for m in gm0.modules() if isinstance(m, consumers.QuantizedMul)]


@pytest.mark.gpu
def test_rewritten_se_block_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = rewritten(SE, "cuda")
    x = block_input("cuda")
    want = gm(x)                                                      # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # one stream: the squeeze branch is captured in front of the multiply
        out = gm(static_x)
    assert native.launch_count() - n0 >= 6                            # four consumers, the squeeze and the multiply are in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5)) and not torch.equal(out, want)
