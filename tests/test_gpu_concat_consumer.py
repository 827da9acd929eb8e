"""mctq_codes_concat_nhwc, consumers.QuantizedConcat and the ``concats`` rewrite on the GPU.

Requantizing a code is exact arithmetic on at most 256 values per form: the raw entry point must equal the CPU route of
ops.codes_concat and the numpy definition of tests/test_concat_consumer.py byte for byte and write nothing outside its output;
operands in the output's own form, which the launcher copies, must give the bytes the arithmetic gives; the module and the
rewritten models must equal their CPU routes, and the rewrite with ``concats=True`` the same rewrite without it, bit for bit
(tests/test_pool_consumer.py says why the float32 products of those models are exact)."""
import numpy as np
import pytest
import torch

from test_concat_consumer import (Fire, IDENTITY_FORMS, Inception, all_codes, as_tensors, block_input, check_concat_module,
                                  check_refusals, concat_case, concat_cases, concat_reference, rewritten)

GUARD, SENTINEL = 64, 0xA5


def _raw_into_guarded_buffer(operands, out_form):
    """The raw entry point on device copies of ``operands``, its output in the middle of a sentinel-filled buffer -> (output as
    numpy [.., sum C_k], launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    scale, zp, qmin, qmax = out_form
    tdt, ocode = ops._code_dtype(qmin, qmax)
    lead = operands[0][0].shape[:-1]
    pixels, total = int(np.prod(lead)), sum(c.shape[-1] for c, _, _ in operands)
    n = pixels * total
    dev = as_tensors(operands, "cuda")
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and all(c.data_ptr() % 16 == 0 for c, _, _ in dev)
    items = (native.ConcatItem * len(dev))()
    for it, (c, s, z) in zip(items, dev):
        it.codes, it.channels, it.code_dtype, it.zero_point, it.scale = c.data_ptr(), c.shape[-1], ops._code_of(c), z, s
    rc = lib.mctq_codes_concat_nhwc(items, len(dev), buf.data_ptr() + GUARD, ocode, pixels, scale, zp, qmin, qmax,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (lead, total)
    return got[GUARD:GUARD + n].view(np.uint8 if tdt == torch.uint8 else np.int8).reshape(*lead, total), launch


@pytest.mark.gpu
def test_codes_concat_kernel_equals_the_cpu_route_and_stays_inside_its_output():
    from mct_quantizers_amd.hip import ops
    n = 0
    for channels, lead, out_index in concat_cases():
        operands, out_form, want = concat_case(channels, lead, out_index)
        cpu = ops.codes_concat(as_tensors(operands), out_form).numpy()
        got, launch = _raw_into_guarded_buffer(operands, out_form)
        assert launch.startswith("codes_concat<") and f"{len(channels)} -> {'u8' if out_form[2] >= 0 else 'i8'}" in launch, launch
        assert got.dtype == cpu.dtype and got.shape == cpu.shape, (channels, lead, out_index)
        assert np.array_equal(got, cpu) and np.array_equal(got, want), (channels, lead, out_index)
        assert got.min() == out_form[2] and got.max() == out_form[3]
        n += 1
    assert n == 24


@pytest.mark.gpu
def test_copy_operands_give_the_bytes_of_the_arithmetic_for_every_code():
    """An operand in the output's own form is copied by the launcher; with the tuning key ``concat_copy`` = 0 it runs the
    requantization arithmetic like any other.  Both give the operand's own bytes, for all 256 codes of every form."""
    from mct_quantizers_amd.hip import native
    try:
        for signed, s, z in IDENTITY_FORMS:
            codes = all_codes(signed)
            out_form = (s, z, -128, 127) if signed else (s, z, 0, 255)
            other = all_codes(not signed)                 # a second operand that always runs the arithmetic
            operands = ((codes, s, z), (other, 0.7 * s, 1))
            native.set_tuning("concat_copy", 1)
            copied, _ = _raw_into_guarded_buffer(operands, out_form)
            native.set_tuning("concat_copy", 0)
            computed, _ = _raw_into_guarded_buffer(operands, out_form)
            assert np.array_equal(copied, computed), (signed, s, z)
            assert np.array_equal(copied[:, :16], codes) and np.array_equal(copied, concat_reference(operands, out_form))
    finally:
        native.set_tuning("concat_copy", 1)


@pytest.mark.gpu
def test_codes_concat_refusals_come_before_any_launch():
    from mct_quantizers_amd.hip import native
    check_refusals(native.load(), native)


@pytest.mark.gpu
def test_codes_concat_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    for channels, out_index in (((16, 48, 32), 0), ((16,) * 8, 1), ((32, 16), 1)):
        operands, out_form, want = concat_case(channels, (2, 7, 9), out_index)
        dev = as_tensors(operands, "cuda")
        n0 = native.launch_count()
        y = ops.codes_concat(dev, out_form)
        assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_concat<")
        assert y.is_cuda and y.is_contiguous() and y.dtype == (torch.uint8 if out_form[2] >= 0 else torch.int8)
        assert np.array_equal(y.cpu().numpy(), want)
    # the torch route: a channel count that is no multiple of 16, and nine operands
    rng = np.random.default_rng(6)
    odd = [(rng.integers(0, 256, (3, 5, c)).astype(np.uint8), 0.02 + 0.01 * i, 3 * i) for i, c in enumerate((24, 16))]
    nine = [(rng.integers(-128, 128, (4, 16)).astype(np.int8), 0.01 * (i + 1), i - 4) for i in range(9)]
    for operands, out_form in ((odd, (0.03, -5, -128, 127)), (nine, (0.025, 114, 0, 255))):
        n0 = native.launch_count()
        y = ops.codes_concat(as_tensors(operands, "cuda"), out_form)
        assert y.is_cuda and not native.last_launch().startswith("codes_concat<")
        assert native.launch_count() - n0 >= len(operands)                   # a quantize launch per operand
        assert np.array_equal(y.cpu().numpy(), concat_reference(operands, out_form))
        assert torch.equal(y.cpu(), ops.codes_concat(as_tensors(operands), out_form))
    # a non-contiguous operand is made contiguous, an empty batch launches nothing
    c = torch.from_numpy(concat_case((16,), (2, 3, 5), 0)[0][0][0].copy()).cuda()
    assert torch.equal(ops.codes_concat([(c.permute(1, 0, 2, 3), 0.05, 0)], (0.025, 114, 0, 255)).cpu(),
                       ops.codes_concat([(c.cpu().permute(1, 0, 2, 3), 0.05, 0)], (0.025, 114, 0, 255)))
    n0 = native.launch_count()
    empty = ops.codes_concat([(torch.zeros(0, 4, 16, dtype=torch.uint8, device="cuda"), 0.1, 0),
                              (torch.zeros(0, 4, 32, dtype=torch.int8, device="cuda"), 0.1, 0)], (0.03, -5, -128, 127))
    assert empty.shape == (0, 4, 48) and empty.dtype == torch.int8 and empty.is_cuda and native.launch_count() == n0


@pytest.mark.gpu
def test_quantized_concat_on_gpu_equals_its_cpu_route():
    want = check_concat_module("cpu")
    got = check_concat_module("cuda")
    assert len(got) == len(want) == 6 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("make", [Fire, Inception])
def test_rewritten_blocks_give_the_bits_of_the_rewrite_without_concats_gpu(make):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    x = block_input("cuda")
    gm, n = rewritten(make, "cuda")
    gm0, n0 = rewritten(make, "cuda", concats=False)
    assert n == n0 == (4 if make is Fire else 7)
    concat = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedConcat))
    seen = []

    def before(m, args):
        seen.append(native.launch_count())

    def after(m, args, out):
        seen.append((native.launch_count(), native.last_launch(), [a.dtype for a in args]))

    hooks = [concat.register_forward_pre_hook(before), concat.register_forward_hook(after)]
    y, y0 = gm(x), gm0(x)
    for h in hooks:
        h.remove()
    count0, (count1, launch, dtypes) = seen
    assert count1 - count0 == 1 and launch.startswith("codes_concat<")         # codes in: the module is that one launch
    assert all(d in (torch.int8, torch.uint8) for d in dtypes)
    assert y.shape == (2, 16, 7, 5) and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    assert torch.equal(y.cpu(), rewritten(make)[0](x.cpu()))
    assert not [m for m in gm0.modules() if isinstance(m, consumers.QuantizedConcat)]


@pytest.mark.gpu
def test_rewritten_inception_block_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = rewritten(Inception, "cuda")
    x = block_input("cuda")
    want = gm(x)                                                      # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # one stream: the branches are captured one after the other
        out = gm(static_x)
    assert native.launch_count() - n0 >= 9                            # seven consumers, the concat and the pool are in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5)) and not torch.equal(out, want)
