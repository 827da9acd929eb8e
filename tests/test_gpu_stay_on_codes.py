"""mctq_fq_join_rc_f32, ops.fq_join(residual_codes=...) and fuse_linear_consumers_fx(stay_on_codes=True) on the GPU.

The codes-residual join stands for the float32-residual join on the dequantized codes, which tests/test_gpu_join_consumer.py pins
to the CPU route: the raw entry point must equal that CPU route bit for bit and write nothing outside its outputs.  A model
rewritten with ``stay_on_codes`` must equal the same rewrite without it on the GPU, and its own CPU route, bit for bit: the
integer sums are exact and the epilogue arithmetic is the same, so a difference would be a finding about the epilogues."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_join_consumer import FORMS
from test_stay_on_codes import (MODELS, OUTPUTS, R_FORMS, _joins, block_input, check_emitted_codes, cpu_route_rc, residual_case,
                                rewritten)

GUARD, SENTINEL = 64, 0xA5
# one lane; the tail alone; one whole chunk; a chunk and a tail; whole blocks; several blocks, the last partly empty, and a tail
SIZES = [1, 15, 16, 17, 4096, 4096 * 3 + 87]


def _raw_into_guarded_buffers(n, form, r_dtype, relu, want_float, want_codes):
    """The raw entry point on device copies of ``residual_case``, each output in the middle of a sentinel-filled buffer -> (y or
    None, codes or None) as numpy; the sentinels around both outputs, the whole buffer of an output that is switched off, and
    that the call was exactly one launch that names the codes-residual form are checked here."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    scale, zp, qmin, qmax = FORMS[form]
    x, c, _ = residual_case(n, form, r_dtype)
    x, c = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(c.copy()).cuda()
    s, z = R_FORMS[r_dtype]
    ybuf = torch.full((4 * n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (ybuf.data_ptr() + GUARD) % 16 == 0 and (cbuf.data_ptr() + GUARD) % 16 == 0 and x.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0
    count = native.launch_count()
    rc = lib.mctq_fq_join_rc_f32(x.data_ptr(), c.data_ptr(), native.CODE_I8 if r_dtype == torch.int8 else native.CODE_U8, s, z,
                                 int(relu), ybuf.data_ptr() + GUARD if want_float else None,
                                 cbuf.data_ptr() + GUARD if want_codes else None, native.CODE_U8 if qmin >= 0 else native.CODE_I8,
                                 n, scale, zp, qmin, qmax, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    assert native.launch_count() - count == 1 and launch.startswith("fq_join<"), launch
    assert ("addc(i8) " if r_dtype == torch.int8 else "addc(u8) ") in launch and "add " not in launch, launch
    assert ("relu " in launch) == relu and ("f32" in launch) == want_float, launch
    assert (("-> u8" if qmin >= 0 else "-> i8") in launch or ("+ u8" if qmin >= 0 else "+ i8") in launch) == want_codes, launch
    yb, cb = ybuf.cpu().numpy(), cbuf.cpu().numpy()
    what = (n, form, r_dtype, relu, want_float, want_codes)
    assert np.all(yb[:GUARD] == SENTINEL) and np.all(yb[GUARD + 4 * n:] == SENTINEL), what
    assert np.all(cb[:GUARD] == SENTINEL) and np.all(cb[GUARD + n:] == SENTINEL), what
    if not want_float:
        assert np.all(yb == SENTINEL), what
    if not want_codes:
        assert np.all(cb == SENTINEL), what
    y = yb[GUARD:GUARD + 4 * n].view(np.float32) if want_float else None
    codes = cb[GUARD:GUARD + n].view(np.uint8 if qmin >= 0 else np.int8) if want_codes else None
    return y, codes


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["u8", "i8"])
@pytest.mark.parametrize("r_dtype", [torch.int8, torch.uint8])
@pytest.mark.parametrize("relu", [False, True])
def test_codes_residual_kernel_equals_the_cpu_route_and_stays_inside_its_outputs(form, r_dtype, relu):
    for n in SIZES:
        want_y, want_c = cpu_route_rc(n, form, r_dtype, relu)
        x = residual_case(n, form, r_dtype)[0]
        for want_float, want_codes in OUTPUTS:
            y, codes = _raw_into_guarded_buffers(n, form, r_dtype, relu, want_float, want_codes)
            what = (n, want_float, want_codes)
            if want_float:
                assert bits_equal(y, want_y), (what, first_mismatch(y, want_y, x))
            if want_codes:
                assert np.array_equal(codes, want_c), (what, int((codes != want_c).sum()))
    assert len(np.unique(want_c)) > 100 and np.isnan(x).any()             # the largest case holds the edge values


@pytest.mark.gpu
def test_fq_join_with_residual_codes_on_layouts():
    from mct_quantizers_amd.hip import native, ops
    g = torch.Generator().manual_seed(8)
    cl = torch.channels_last
    x4 = (torch.randn(2, 16, 5, 7, generator=g) * 30).contiguous(memory_format=cl)
    c4 = torch.randint(0, 256, (2, 16, 5, 7), generator=g).to(torch.uint8).contiguous(memory_format=cl)
    s, z = R_FORMS[torch.uint8]
    for form in FORMS.values():
        for relu in (False, True):
            for want_float, want_codes in OUTPUTS:
                kw = dict(relu=relu, want_float=want_float, want_codes=want_codes)
                wy, wc = ops.fq_join(x4, *form, residual=ops.dequantize_codes(c4, s, z), **kw)               # on the CPU
                count = native.launch_count()
                y, codes = ops.fq_join(x4.cuda(), *form, residual_codes=(c4.cuda(), s, z), **kw)
                launch = native.last_launch()
                assert native.launch_count() - count == 1 and launch.startswith("fq_join<") and "addc(u8)" in launch, launch
                if want_float:
                    assert y.stride() == x4.stride() and bits_equal(y.cpu().numpy(), wy.numpy())
                if want_codes:
                    assert codes.stride() == x4.stride() and codes.permute(0, 2, 3, 1).is_contiguous() and torch.equal(codes.cpu(), wc)
    # codes with other strides, and a misaligned view of them: the composed route (no codes-residual launch), the same bits
    form = FORMS["u8"]
    wy, wc = ops.fq_join(x4, *form, residual=ops.dequantize_codes(c4, s, z), relu=True)
    flat = torch.randint(0, 256, (x4.numel() + 1,), generator=g).to(torch.uint8)
    xf = torch.randn(x4.numel(), generator=g) * 30
    wyf, wcf = ops.fq_join(xf, *form, residual=ops.dequantize_codes(flat[1:], s, z), relu=True)
    for xg, cg, want in ((x4.cuda(), c4.contiguous().cuda(), (wy, wc)), (xf.cuda(), flat.cuda()[1:], (wyf, wcf))):
        y, codes = ops.fq_join(xg, *form, residual_codes=(cg, s, z), relu=True)
        assert "addc" not in native.last_launch()
        assert bits_equal(y.cpu().numpy(), want[0].numpy()) and torch.equal(codes.cpu(), want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,family,bits", [("linear", "sym", None), ("linear", "sym", 4), ("linear", "uniform", 4),
                                              ("linear", "lut16", None), ("1x1", "uniform", None), ("kxk", "sym", None),
                                              ("dw", "uniform", None), ("dw", "lut16", None)])
def test_consumers_emit_narrowed_codes_on_gpu(kind, family, bits):
    """Every consumer class, the weight zero point forms and the packed 4-bit routes (one activation row: ``bits=4`` runs
    mctq_qlinear_w4a8 / _zp, a 16-entry codebook mctq_qlinear_lut4a8), behind a ReLU and a signed holder: int8 codes."""
    names = check_emitted_codes(kind, family, "relu", device="cuda", bits=bits)
    assert len(names) == 1
    if kind == "linear" and (bits == 4 or family == "lut16"):
        assert ("lut4" if family == "lut16" else "w4") in names[0], names
    check_emitted_codes(kind, family, "relu6", device="cuda", bits=bits)


def _launches_per_forward(gm, x):
    from mct_quantizers_amd.hip import native
    gm(x)                                                 # (refreshes the weight codes)
    count = native.launch_count()
    y = gm(x)
    return y, native.launch_count() - count


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("channels_last", [False, True])
def test_rewritten_models_on_gpu(name, channels_last):
    """Bit for bit the rewrite without ``stay_on_codes`` on the GPU and the model's own CPU route.  Launches per forward: every
    removed join was one launch and its producer's launch only changed its output form, so the stack saves exactly the eight
    ReLU-only joins; the inverted-residual block has no joins, there the two consumers behind the ReLU6s no longer launch
    their own quantization of a float32 input."""
    gm, gm0 = rewritten(name, "cuda")
    x = block_input("cuda", channels_last)
    (y, launches), (y0, launches0) = _launches_per_forward(gm, x), _launches_per_forward(gm0, x)
    assert y.is_cuda and len(torch.unique(y)) > 50
    assert bits_equal(y.cpu().numpy(), y0.cpu().numpy()), first_mismatch(y.cpu().numpy(), y0.cpu().numpy())
    want = rewritten(name, "cpu")[0](block_input("cpu", channels_last))
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
    removed = len(_joins(gm0)) - len(_joins(gm))
    assert removed == (8 if name == "four blocks" else 0)
    assert launches0 - launches == (removed if name == "four blocks" else 2), (launches0, launches)


@pytest.mark.gpu
def test_rewritten_stack_replays_in_a_hip_graph():
    from mct_quantizers_amd.hip import native
    gm, _ = rewritten("four blocks", "cuda")
    x = block_input("cuda", channels_last=True)
    want = gm(x)                                                      # (refreshes the weight codes outside the capture)
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gm(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):                                         # strictly sequential, one stream
        out = gm(static_x)
    assert native.launch_count() - n0 >= 4 + 13                       # four joins and thirteen products at least
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, gm(x * 0.5)) and not torch.equal(out, want)
