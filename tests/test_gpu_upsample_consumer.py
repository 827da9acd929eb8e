"""mctq_codes_upsample_nhwc, consumers.QuantizedUpsample and the ``upsamples`` rewrite on the GPU.

Moving and requantizing a code is exact: the raw entry point, in both of its forms and with maps and factors alike, must equal
the CPU route of ops.codes_upsample and the numpy definition of tests/test_upsample_consumer.py byte for byte and write nothing
outside its output; an input in the output's own form, which the launcher copies, must give the bytes the arithmetic gives; map
entries outside the image must read the image's edge; the module must give the codes of the float32 chain around ATen's
upsample on the device; and the rewritten models must equal their CPU routes and the same rewrite without ``upsamples``."""
import numpy as np
import pytest
import torch

from test_upsample_consumer import (ALL, Chain, Decoder, EVERY_CODE_PAIRS, FACTORS, GEOMETRIES, IN_FORMS, OUT_FORMS, all_codes,
                                    check_refusals, check_upsample_module, float_chain, index_maps, low_input, rewritten, skip_input,
                                    upsample_case, upsample_reference)

GUARD, SENTINEL = 64, 0xA5
F = torch.nn.functional


def _raw_into_guarded_buffer(codes, in_form, out_form, rows=None, cols=None, factors=None, out_hw=None):
    """The raw entry point on a device copy of ``codes`` [B, H, W, C], its output in the middle of a sentinel-filled buffer ->
    (output as numpy [B, Ho, Wo, C], launch name); the sentinels on both sides are checked here.  ``rows`` / ``cols``: the maps
    as sequences of ints (made device int32 tables), or ``factors``."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    scale, zp, qmin, qmax = out_form
    tdt, ocode = ops._code_dtype(qmin, qmax)
    b, h, w, c = codes.shape
    if factors is not None:
        ho, wo, fh, fw, drows, dcols = factors[0] * h, factors[1] * w, factors[0], factors[1], None, None
    else:
        drows, dcols = (torch.tensor(list(m), dtype=torch.int32, device="cuda") for m in (rows, cols))
        ho, wo, fh, fw = len(drows), len(dcols), 0, 0
    if out_hw is not None:
        assert (ho, wo) == tuple(out_hw)
    n = b * ho * wo * c
    dev = torch.from_numpy(np.array(codes)).cuda()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and dev.data_ptr() % 16 == 0
    rc = lib.mctq_codes_upsample_nhwc(dev.data_ptr(), buf.data_ptr() + GUARD, ops._code_of(dev), in_form[1], in_form[0], b, h, w, c,
                                      ho, wo, fh, fw, None if drows is None else drows.data_ptr(), None if dcols is None else dcols.data_ptr(),
                                      ocode, scale, zp, qmin, qmax, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (codes.shape, ho, wo)
    return got[GUARD:GUARD + n].view(np.uint8 if tdt == torch.uint8 else np.int8).reshape(b, ho, wo, c), launch


def _codes(shape, signed, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-128, 128, shape).astype(np.int8) if signed else rng.integers(0, 256, shape).astype(np.uint8)


# (input shape, factors or None, output size through maps or None): one chunk per pixel; a chunk count that is no power of two;
# several workgroups with a ragged last one (2 * 14 * 18 * 3 = 1512 and 2 * 21 * 9 * 3 = 1134 output chunks, 378 input chunks);
# non-integer upsampling and downsampling through maps
KERNEL_CASES = [((1, 3, 2, 16), (2, 2), None), ((2, 3, 5, 48), (2, 2), None), ((2, 7, 9, 48), (2, 2), None), ((2, 7, 9, 48), (3, 1), None),
                ((2, 9, 11, 48), None, 1), ((2, 9, 11, 16), None, 6), ((2, 9, 11, 48), None, 3), ((2, 7, 9, 48), (1, 1), None)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_codes_upsample_kernel_equals_the_cpu_route_and_stays_inside_its_output(form):
    from mct_quantizers_amd.hip import native, ops
    try:
        native.set_tuning("upsample_form", form)
        for n, (shape, factors, geometry) in enumerate(KERNEL_CASES):
            for in_kind, out_kind in (("u8", "i8"), ("i8", "u8")):
                signed, s, z = IN_FORMS[in_kind]
                codes, out_form = _codes(shape, signed, 10 * n + signed), OUT_FORMS[out_kind]
                if factors is not None:
                    rows, cols = np.arange(factors[0] * shape[1]) // factors[0], np.arange(factors[1] * shape[2]) // factors[1]
                else:
                    rows, cols = (m.numpy() for m in index_maps(geometry))
                    assert (len(rows), len(cols)) == {1: (13, 29), 6: (13, 29), 3: (4, 5)}[geometry]
                want = upsample_reference(codes, (s, z), out_form, rows, cols)
                cpu = ops.codes_upsample(torch.from_numpy(codes.copy()), (s, z), out_form, torch.from_numpy(rows), torch.from_numpy(cols))
                # through the maps: always the gather form
                got, launch = _raw_into_guarded_buffer(codes, (s, z), out_form, rows, cols)
                op = f"{in_kind} -> {out_kind}"
                assert launch.startswith("codes_upsample<") and f"{op} gather" in launch, launch
                assert got.dtype == want.dtype and np.array_equal(got, want) and np.array_equal(got, cpu.numpy()), (shape, geometry, op)
                if factors is not None:                      # through the factors: the form the tuning key asks for
                    got, launch = _raw_into_guarded_buffer(codes, (s, z), out_form, factors=factors)
                    assert f"{op} {'gather' if form == 1 else 'replicate'}" in launch, launch
                    assert np.array_equal(got, want), (shape, factors, op)
        # factors beyond the replicate form's cap (5 * 4 > 16) take the gather form under either key
        codes = _codes((1, 2, 3, 16), False, 77)
        got, launch = _raw_into_guarded_buffer(codes, (0.061, 114), OUT_FORMS["i8"], factors=(5, 4))
        assert "gather" in launch and np.array_equal(got, upsample_reference(codes, (0.061, 114), OUT_FORMS["i8"], np.arange(10) // 5, np.arange(12) // 4))
        got, launch = _raw_into_guarded_buffer(codes, (0.061, 114), OUT_FORMS["i8"], factors=(4, 4))
        assert ("replicate" if form == 2 else "gather") in launch
        assert np.array_equal(got, upsample_reference(codes, (0.061, 114), OUT_FORMS["i8"], np.arange(8) // 4, np.arange(12) // 4))
    finally:
        native.set_tuning("upsample_form", 0)
    # the launcher's own choice: replicate where it is eligible and there is something to replicate, gather elsewhere
    for factors, want in (((2, 2), "replicate"), ((3, 1), "replicate"), ((4, 4), "replicate"), ((1, 1), "gather"), ((5, 4), "gather")):
        got, launch = _raw_into_guarded_buffer(codes, (0.061, 114), OUT_FORMS["i8"], factors=factors)
        assert want in launch, (factors, launch)
        rows, cols = np.arange(2 * factors[0]) // factors[0], np.arange(3 * factors[1]) // factors[1]
        assert np.array_equal(got, upsample_reference(codes, (0.061, 114), OUT_FORMS["i8"], rows, cols))
    _, launch = _raw_into_guarded_buffer(codes, (0.061, 114), OUT_FORMS["i8"], [0, 0, 1, 1], [0, 0, 1, 1, 2, 2])
    assert "gather" in launch                                # (tables are never examined: they live on the device)


@pytest.mark.gpu
def test_empty_problems_launch_nothing():
    from mct_quantizers_amd.hip import native, ops
    n0 = native.launch_count()
    rows, cols = torch.arange(6, device="cuda") // 2, torch.arange(8, device="cuda") // 2
    for shape in ((0, 3, 4, 16), (2, 3, 4, 0)):
        y = ops.codes_upsample(torch.zeros(shape, dtype=torch.uint8, device="cuda"), (0.1, 0), (0.1, 0, -128, 127), rows, cols)
        assert y.shape == (shape[0], 6, 8, shape[3]) and y.dtype == torch.int8 and y.is_cuda
    y = ops.codes_upsample(torch.zeros((2, 3, 4, 16), dtype=torch.uint8, device="cuda"), (0.1, 0), (0.1, 0, 0, 255), rows[:0], cols)
    assert y.shape == (2, 0, 8, 16) and native.launch_count() == n0


@pytest.mark.gpu
def test_every_code_and_the_copy_rule_on_the_gpu():
    """All 256 codes through the four type pairs, a narrow clamp and the identical-form pairs, in both forms.  An input in the
    output's own form is copied by the launcher; with the tuning key ``concat_copy`` = 0 it runs the requantization arithmetic.
    Both give the input's own bytes."""
    from mct_quantizers_amd.hip import native
    rows = cols = np.arange(8) // 2
    try:
        for kind, out_form in EVERY_CODE_PAIRS:
            codes, in_form = all_codes(kind == "i8"), IN_FORMS[kind][1:]
            want = upsample_reference(codes, in_form, out_form, rows, cols)
            results = []
            for copy in (1, 0):
                native.set_tuning("concat_copy", copy)
                for form in (1, 2):
                    native.set_tuning("upsample_form", form)
                    results.append(_raw_into_guarded_buffer(codes, in_form, out_form, factors=(2, 2))[0])
                results.append(_raw_into_guarded_buffer(codes, in_form, out_form, rows, cols)[0])
            assert all(np.array_equal(r, want) for r in results), (kind, out_form)
            if in_form == out_form[:2]:
                assert np.array_equal(want, codes[:, rows][:, :, cols])
    finally:
        native.set_tuning("concat_copy", 1)
        native.set_tuning("upsample_form", 0)


@pytest.mark.gpu
def test_map_entries_outside_the_image_read_its_edge():
    """The launcher cannot see the device tables: the kernel clamps every entry.  Tables that point beyond the last row and
    column, and before the first, give the edge's bytes, and nothing is written outside the output."""
    codes = _codes((2, 7, 9, 48), False, 5)
    in_form, out_form = (0.061, 114), OUT_FORMS["i8"]
    got, _ = _raw_into_guarded_buffer(codes, in_form, out_form, [7 + 5] * 6, [9 + 5] * 4)
    assert np.array_equal(got, upsample_reference(codes, in_form, out_form, [6] * 6, [8] * 4))
    got, _ = _raw_into_guarded_buffer(codes, in_form, out_form, [-3, 2, 2 ** 31 - 1, -2 ** 31], [1, -1, 100000])
    assert np.array_equal(got, upsample_reference(codes, in_form, out_form, [0, 2, 6, 0], [1, 0, 8]))


@pytest.mark.gpu
def test_codes_upsample_refusals_come_before_any_launch():
    from mct_quantizers_amd.hip import native
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 4096 + 255) // 256 * 256         # (the overlap rows reach 112 bytes below the address)
    check_refusals(native.load(), native, base)


@pytest.mark.gpu
def test_codes_upsample_through_python_on_gpu_tensors():
    from mct_quantizers_amd.hip import native, ops
    for index in (0, 1, 2, 3, 6):
        rows, cols = index_maps(index)
        codes, in_form, out_form, want = upsample_case(index, 48)
        dev = torch.from_numpy(codes.copy()).cuda()
        for maps in ((rows, cols), (rows.cuda(), cols.to(torch.int32).cuda())):          # host maps are examined for factors
            n0 = native.launch_count()
            y = ops.codes_upsample(dev, in_form, out_form, *maps)
            assert native.launch_count() - n0 == 1 and native.last_launch().startswith("codes_upsample<")
            assert y.is_cuda and y.is_contiguous() and y.dtype == torch.int8 and np.array_equal(y.cpu().numpy(), want)
        assert torch.equal(y, float_chain(dev, in_form, out_form, GEOMETRIES[index]))     # ATen's upsample on the device
        if FACTORS[index]:
            assert torch.equal(ops.codes_upsample(dev, in_form, out_form, rows.cuda(), cols.cuda(), factors=FACTORS[index]), y)
    # the torch route: a channel count that is no multiple of 16
    codes, in_form, out_form, want = upsample_case(1, 5)
    n0 = native.launch_count()
    y = ops.codes_upsample(torch.from_numpy(codes.copy()).cuda(), in_form, out_form, *index_maps(1))
    assert y.is_cuda and not native.last_launch().startswith("codes_upsample<") and native.launch_count() > n0
    assert np.array_equal(y.cpu().numpy(), want)
    # a non-contiguous input is made contiguous
    c = torch.from_numpy(upsample_case(0, 16)[0].copy()).cuda()
    rows, cols = torch.arange(4) // 2, torch.arange(18) // 2
    assert torch.equal(ops.codes_upsample(c.permute(1, 0, 2, 3), (0.05, 0), (0.025, 114, 0, 255), cols, rows).cpu(),
                       ops.codes_upsample(c.cpu().permute(1, 0, 2, 3), (0.05, 0), (0.025, 114, 0, 255), cols, rows))


@pytest.mark.gpu
def test_quantized_upsample_on_gpu_equals_its_cpu_route():
    want = check_upsample_module("cpu")
    got = check_upsample_module("cuda")
    assert len(got) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", [GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[6], dict(scale_factor=(3, 1), mode="nearest-exact")])
def test_the_module_gives_the_codes_of_the_float_chain_around_atens_upsample(geometry):
    """holder_B(F.interpolate(holder_A(x))) in float32 on the device, coded by fq_codes, against QuantizedUpsample(A, B)(x)."""
    from test_concat_consumer import _form, holder_of
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    ha, hb = holder_of("s").cuda(), holder_of("uni").cuda()
    q = consumers.QuantizedUpsample(torch.nn.Upsample(**geometry), ha.activation_holder_quantizer, hb.activation_holder_quantizer)
    x = (torch.randn(2, 48, 9, 11, generator=torch.Generator().manual_seed(41)) * 3.0).cuda()
    with torch.no_grad():
        chain = hb(F.interpolate(ha(x), **geometry))
    s, z, qmin, qmax = _form(hb)
    want = ops.fq_codes(chain, None, None, None, qmin, qmax, s, z)
    y = q(x)                                                 # the first forward of this shape derives the maps
    n0 = native.launch_count()
    again = q(x)
    assert native.launch_count() - n0 == 2 and native.last_launch().startswith("codes_upsample<")     # quantize, then the one launch
    assert torch.equal(y, want) and torch.equal(again, want) and y.shape == chain.shape and len(torch.unique(y)) > 50
    assert torch.equal(ops.dequantize_codes(y, s, z), chain)
    rows, cols, factors = q.index_maps(9, 11, x.device)
    assert rows.is_cuda and rows.dtype == torch.int32 and (factors is not None) == (geometry.get("scale_factor") in (2, (3, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("make", [Chain, lambda: Chain(False), Decoder])
def test_rewritten_models_give_the_bits_of_the_rewrite_without_upsamples_gpu(make):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    args = (low_input("cuda"), skip_input("cuda")) if make is Decoder else (low_input("cuda"),)
    gm, n = rewritten(make, "cuda", **ALL)
    gm0, n0 = rewritten(make, "cuda", upsamples=False, **ALL)
    up = next(m for m in gm.modules() if isinstance(m, consumers.QuantizedUpsample))
    seen = []

    def before(m, a):
        seen.append(native.launch_count())

    def after(m, a, out):
        seen.append((native.launch_count(), native.last_launch(), a[0].dtype))

    hooks = [up.register_forward_pre_hook(before), up.register_forward_hook(after)]
    gm(*args)                                                # (derives the maps)
    del seen[:]
    y, y0 = gm(*args), gm0(*args)
    for h in hooks:
        h.remove()
    count0, (count1, launch, dtype) = seen
    assert count1 - count0 == 1 and launch.startswith("codes_upsample<") and dtype == torch.uint8     # codes in: that one launch
    assert y.shape[2:] == (8, 10) and len(torch.unique(y)) > 50 and torch.equal(y, y0)
    assert torch.equal(y.cpu(), rewritten(make, **ALL)[0](*[a.cpu() for a in args]))
    assert not [m for m in gm0.modules() if isinstance(m, consumers.QuantizedUpsample)]


@pytest.mark.gpu
def test_rewritten_decoder_stage_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = rewritten(Decoder, "cuda", **ALL)
    x, skip = low_input("cuda"), skip_input("cuda")
    want = gm(x, skip)                                       # the warm-up forward: weight codes and the index maps, outside the capture
    static_x, static_skip = x.clone(), skip.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x, static_skip)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):
        out = gm(static_x, static_skip)
    assert native.launch_count() - n0 >= 4                   # two consumers, the upsample and the concatenation are in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5, skip)) and not torch.equal(out, want)
