"""mctq_codes_upsample_bilinear_nhwc, consumers.QuantizedBilinearUpsample and the ``bilinear_upsamples`` rewrite on the GPU.

The contract is on integers, so every instance of the kernel (tuning key ``bilinear_strip``) must equal the CPU route of
ops.codes_upsample_bilinear byte for byte and write nothing outside its output."""
import pytest
import torch

import test_bilinear_consumer as cpu_tests
from test_bilinear_consumer import FORMS, Head, random_codes, tables_of
from test_upsample_consumer import holder_of, low_input

GUARD, SENTINEL = 64, 0xA5
EXTREME = {"u8 255": (torch.uint8, 255, (1.0 / 32, 0), (1.0 / 64, -128, -128, 127)), "u8 0": (torch.uint8, 0, (0.061, 255), (0.03, 127, -128, 127)),
           "i8 -128": (torch.int8, -128, (0.05, 127), (0.025, 255, 0, 255)), "i8 127": (torch.int8, 127, (1.0 / 32, -128), (1.0 / 16, 0, 0, 255))}
# (geometry, B x H x W x C): C = 16 and 48; Ho = 3 below every strip with H = W = 1 (i1 clamps onto i0); Ho = 4 and 8 equal to a
# strip; Ho = 14 and 13 no multiple of one; 90 x 3 = 270 chunks per row: two workgroups, the last ragged; downsampling (r0 jumps)
CASES = [(dict(scale_factor=3), (2, 1, 1, 16)), (dict(scale_factor=2), (1, 2, 1, 48)), (dict(scale_factor=2), (2, 4, 3, 16)),
         (dict(scale_factor=2), (2, 7, 9, 48)), (dict(size=(13, 9), align_corners=True), (2, 7, 5, 48)),
         (dict(scale_factor=2), (1, 3, 45, 48)), (dict(size=(4, 5)), (2, 9, 11, 16)), (dict(scale_factor=(4, 1.5)), (1, 9, 11, 16))]


def raw_into_guarded_buffer(codes, in_form, out_form, rows, cols):
    """The raw entry point on a device copy of ``codes``, its output in the middle of a sentinel-filled buffer -> the output on
    the CPU; the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    scale, zp, qmin, qmax = out_form
    tdt, ocode = ops._code_dtype(qmin, qmax)
    (b, h, w, c), ho, wo = codes.shape, rows[0].numel(), cols[0].numel()
    n = b * ho * wo * c
    dev = codes.cuda()
    tables = [m.to(device="cuda", dtype=torch.int32).contiguous() for m in (*rows, *cols)]
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and dev.data_ptr() % 16 == 0
    rc = lib.mctq_codes_upsample_bilinear_nhwc(dev.data_ptr(), buf.data_ptr() + GUARD, ops._code_of(dev), in_form[1], in_form[0], b, h, w, c,
                                               ho, wo, *(m.data_ptr() for m in tables), ocode, scale, zp, qmin, qmax,
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    got = buf.cpu()
    assert bool((got[:GUARD] == SENTINEL).all()) and bool((got[GUARD + n:] == SENTINEL).all()), (codes.shape, ho, wo)
    return got[GUARD:GUARD + n].view(tdt).reshape(b, ho, wo, c)


@pytest.mark.gpu
@pytest.mark.parametrize("strip", [1, 4, 8])
def test_every_kernel_instance_equals_the_cpu_route_and_stays_inside_its_output(strip):
    from mct_quantizers_amd.hip import native, ops
    try:
        native.set_tuning("bilinear_strip", strip)
        for n, (geometry, shape) in enumerate(CASES):
            rows, cols = tables_of(geometry, shape[1], shape[2])
            for dtype, in_form, out_form in (FORMS["u8"], FORMS["i8"], FORMS["pot"]):
                codes = random_codes(dtype, shape, seed=n)
                got = raw_into_guarded_buffer(codes, in_form, out_form, rows, cols)
                assert f"strip {strip}" in native.last_launch() and native.last_launch().startswith("codes_bilinear<")
                assert torch.equal(got, ops.codes_upsample_bilinear(codes, in_form, out_form, rows, cols)), (geometry, shape, dtype)
        # tables with entries outside the image and weights outside [0, 2^11]: the image's edge, as the CPU route clamps them
        rows, cols = tables_of(dict(scale_factor=2), 7, 9)
        wild = ((rows[0] - 9, rows[1] + 2 ** 30, rows[2] * 5 - 4000), (cols[0] + 7, cols[1] - 2 ** 30, cols[2] + 2 ** 20))
        dtype, in_form, out_form = FORMS["u8"]
        codes = random_codes(dtype, (2, 7, 9, 48), seed=50)
        assert torch.equal(raw_into_guarded_buffer(codes, in_form, out_form, *wild), ops.codes_upsample_bilinear(codes, in_form, out_form, *wild))
        # all-0 and all-255 bytes against zero points at the other end of the type: acc reaches +-2^22 * 255
        for dtype, fill, in_form, out_form in EXTREME.values():
            codes = torch.full((1, 3, 3, 16), fill, dtype=dtype)
            got = raw_into_guarded_buffer(codes, in_form, out_form, *tables_of(dict(scale_factor=1.5), 3, 3))
            want = ops.codes_upsample_bilinear(codes, in_form, out_form, *tables_of(dict(scale_factor=1.5), 3, 3))
            assert torch.equal(got, want) and len(torch.unique(got)) == 1
    finally:
        native.set_tuning("bilinear_strip", 0)


@pytest.mark.gpu
def test_the_module_and_the_rewritten_model_equal_their_cpu_routes():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    for geometry, kinds in ((dict(scale_factor=2), ("s", "uni")), (dict(size=(13, 29), align_corners=True), ("uni", "u4"))):
        q = consumers.QuantizedBilinearUpsample(torch.nn.Upsample(mode="bilinear", **geometry), holder_of(kinds[0]).activation_holder_quantizer,
                                                holder_of(kinds[1]).activation_holder_quantizer)
        x = torch.randn(2, 48, 9, 11, generator=torch.Generator().manual_seed(41)) * 3.0
        y = q(x.cuda())                                      # the first forward of this shape builds the tables
        n0 = native.launch_count()
        assert torch.equal(q(x.cuda()).cpu(), q(x)) and torch.equal(y.cpu(), q(x)) and len(torch.unique(y)) > 50
        assert native.launch_count() - n0 == 2 and native.last_launch().startswith("codes_bilinear<")     # quantize, then the one launch
        assert q.tables(9, 11, "cuda")[0][0].is_cuda and y.is_contiguous(memory_format=torch.channels_last)
    cpu_tests.test_the_rewrite_takes_a_bilinear_upsample_between_two_holders("module", device="cuda")
    gm, _ = consumers.fuse_linear_consumers_fx(Head("functional").cuda(), bilinear_upsamples=True, convolutions=True, shared_holders=True, stay_on_codes=True)
    cpu, _ = consumers.fuse_linear_consumers_fx(Head("functional"), bilinear_upsamples=True, convolutions=True, shared_holders=True, stay_on_codes=True)
    assert torch.equal(gm(low_input("cuda")).cpu(), cpu(low_input()))
