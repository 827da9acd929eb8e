"""mctq_codes_im2col_pad_nhwc and the padded integer consumers (``any_channels=True``) on the GPU.

The kernel is a byte gather: it must equal the CPU route of ops.codes_im2col(..., pad_to=16) (itself equal to an independent
construction, tests/test_any_channels_consumer.py) byte for byte, under both piece sizes, and write nothing outside its output.
A padded layer runs that kernel and then the integer consumer's kernels, each of which is bit-exact: the GPU layer must equal its
own CPU route bit for bit, and through it the oracle and the float64 bound of tests/test_conv_consumer.py."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_any_channels_consumer import (FAMILIES, KINDS, MODELS, check_padded_chain, check_padded_layer, model_input, padded_layer,
                                        rewritten_pair, unfold_patches)
from test_conv_consumer import conv_model

GUARD, SENTINEL = 64, 0xA5                     # the sentinel bands of tests/test_gpu_conv_consumer.py

# (C, kernel, stride, padding, dilation), each on B = 2 images of 5 x 7 and 9 x 6
KERNEL_CASES = [
    (3, (1, 1), (1, 1), (0, 0), (1, 1)),       # K = 3 < 16: one chunk per row, almost all of it tail
    (17, (1, 1), (1, 1), (0, 0), (1, 1)),      # K = 17: one byte in the second chunk
    (3, (7, 7), (2, 2), (3, 3), (1, 1)),       # the stem: five taps and a third per chunk
    (24, (1, 1), (1, 1), (0, 0), (1, 1)),      # the re-pitch of a pointwise layer
    (24, (3, 3), (2, 2), (1, 1), (1, 1)),
    (40, (3, 3), (1, 1), (2, 2), (2, 2)),      # dilated
    (12, (1, 5), (1, 1), (0, 2), (1, 1)),      # pieces of two taps in one chunk
    (16, (3, 3), (1, 1), (1, 1), (1, 1)),      # C % 16 == 0: the existing kernel's bytes
    (32, (3, 3), (1, 1), (1, 1), (1, 1)),
]


def _into_guarded_buffer(entry, codes, geometry, pad_code, Kp):
    """The raw entry point ``entry`` on a device copy of ``codes``, its output in the middle of a sentinel-filled buffer ->
    (patch matrix as numpy, launch name); the sentinels on both sides are checked here."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = geometry
    B, H, W, C = codes.shape
    ho, wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    n = B * ho * wo * Kp
    x = torch.from_numpy(codes.copy()).cuda()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0 and x.data_ptr() % 16 == 0
    rc = getattr(lib, entry)(x.data_ptr(), buf.data_ptr() + GUARD, B, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw, pad_code,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), (geometry, C)
    return got[GUARD:GUARD + n].view(codes.dtype).reshape(B * ho * wo, Kp), launch


def _check_kernel_case(u8, C, geometry, pad_code, shape):
    """One case through the raw entry point, under every piece size it can take; returns the number of launches checked."""
    from mct_quantizers_amd.hip import native, ops
    rng = np.random.default_rng([C, int(u8), *shape, *(v for pair in geometry for v in pair)])
    codes = rng.integers(0, 256, (*shape, C)).astype(np.uint8).view(np.uint8 if u8 else np.int8)
    want = unfold_patches(codes, *geometry, pad_code, 16)
    cpu = ops.codes_im2col(torch.from_numpy(codes.copy()), *geometry, pad_code, pad_to=16).numpy()
    assert np.array_equal(cpu, want)
    Kp = want.shape[1]
    grains = (0, 1, 4) if C % 4 == 0 else (0, 1)
    try:
        for grain in grains:
            native.set_tuning("im2col_grain", grain)
            got, launch = _into_guarded_buffer("mctq_codes_im2col_pad_nhwc", codes, geometry, pad_code, Kp)
            assert launch.startswith("codes_im2col_pad<"), launch
            assert (f"G={grain}" if grain else ("G=4" if C % 4 == 0 else "G=1")) in launch, (grain, launch)
            assert np.array_equal(got, want), (C, geometry, shape, grain)
    finally:
        native.set_tuning("im2col_grain", 0)
    if C % 16 == 0:                                                      # the bytes of the existing entry point
        old, launch = _into_guarded_buffer("mctq_codes_im2col_nhwc", codes, geometry, pad_code, Kp)
        assert launch.startswith("codes_im2col<") and np.array_equal(old, want)
    return len(grains)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [True, False])
def test_the_padded_gather_equals_the_cpu_route_and_stays_inside_its_output(u8):
    from mct_quantizers_amd.hip import native, ops
    pad_code = 131 if u8 else -7
    n = 0
    for C, *geometry in KERNEL_CASES:
        for shape in ((2, 5, 7), (2, 9, 6)):
            n += _check_kernel_case(u8, C, tuple(geometry), pad_code, shape)
    assert n == 2 * (3 * 2 + 6 * 3)
    # several blocks, the last one partly empty: 243 rows of 14 chunks, 19 rows (266 chunks: a second pass of the lanes) per
    # block, 15 rows in the 13th; and rows of one chunk, 256 per block, 99 in the last
    _check_kernel_case(u8, 24, ((3, 3), (1, 1), (1, 1), (1, 1)), pad_code, (3, 9, 9))
    _check_kernel_case(u8, 3, ((1, 1), (1, 1), (0, 0), (1, 1)), pad_code, (1, 17, 19))
    # ... and through ops.codes_im2col: the new launch where C or K is no multiple of 16, the existing one elsewhere
    for C, launch in ((24, "codes_im2col_pad<"), (3, "codes_im2col_pad<"), (32, "codes_im2col<")):
        codes = torch.randint(0, 256, (2, 5, 7, C), dtype=torch.uint8).to(torch.uint8 if u8 else torch.int8)
        n0 = native.launch_count()
        y = ops.codes_im2col(codes.cuda(), 3, 2, 1, 1, pad_code, pad_to=16)
        assert native.launch_count() - n0 == 1 and native.last_launch().startswith(launch), native.last_launch()
        assert y.is_cuda and y.dtype == codes.dtype and y.shape[1] % 16 == 0
        assert torch.equal(y.cpu(), ops.codes_im2col(codes, 3, 2, 1, 1, pad_code, pad_to=16))
    rows = torch.randint(-128, 128, (33, 6), dtype=torch.int8) if not u8 else torch.randint(0, 256, (33, 6), dtype=torch.uint8)
    y = ops.codes_im2col(rows.cuda(), 1, pad_to=16, pad_code=pad_code)                # [M, K] rows: the re-pitch of a Linear layer
    assert y.shape == (33, 16) and torch.equal(y.cpu(), ops.codes_im2col(rows, 1, pad_to=16, pad_code=pad_code))
    n0 = native.launch_count()                                                       # empty problems launch nothing
    assert ops.codes_im2col(rows[:0].cuda(), 1, pad_to=16, pad_code=pad_code).shape == (0, 16) and native.launch_count() == n0


# M = 1, 7, 33, 300 rows per kind: from one row to past the tile sizes (the weight-streaming kernel is left behind)
INPUTS = {"stem": [(1, 3, 1, 1), (1, 3, 1, 13), (1, 3, 5, 21), (2, 3, 19, 29)],
          "pointwise": [(1, 24, 1, 1), (1, 24, 1, 7), (1, 24, 3, 11), (2, 24, 10, 15)],
          "linear6": [(1, 6), (7, 6), (33, 6), (3, 100, 6)], "linear24": [(1, 24), (7, 24), (33, 24), (3, 100, 24)]}


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_padded_consumers_on_gpu_equal_their_cpu_routes(kind, family):
    from mct_quantizers_amd.hip import native
    for per_channel, bias in ((True, True), (False, False)):
        _, _, cpu, _ = padded_layer(kind, family, per_channel, bias, "cpu", seed=3)
        _, _, gpu, _ = padded_layer(kind, family, per_channel, bias, "cuda", seed=3)
        assert cpu._a_zp not in (0, 128) and gpu._k_pitch is not None                # uniform weights: zero points with za != 0
        rows = []
        for i, shape in enumerate(INPUTS[kind]):
            x = torch.randn(*shape, generator=torch.Generator().manual_seed(i)) * 1.5
            cpu.emit_codes_for = gpu.emit_codes_for = None
            want = cpu(x)
            if i == 0:
                gpu(x.cuda())                                            # (the weight's codes: launches of the first forward only)
            n0 = native.launch_count()
            y = gpu(x.cuda())
            launches = native.launch_count() - n0
            # quantize, the padded gather, the row sums of uniform weights, the product
            assert launches == 3 + (family == "uniform"), (launches, native.last_launch())
            assert native.last_launch().startswith("qlinear") and ((" zp," in native.last_launch()) == (family == "uniform"))
            assert y.is_cuda and y.shape == want.shape
            assert bits_equal(y.cpu().numpy(), want.numpy()), (shape, first_mismatch(y.cpu().numpy(), want.numpy()))
            rows.append(want.numel() // cpu.out_features)
            if i == 2 and per_channel:
                check_padded_layer(gpu, x.cuda(), y)
            cpu.emit_codes_for = gpu.emit_codes_for = (0.043, 9, 0, 255)              # emitted codes: the same bytes
            codes, want_codes = gpu(x.cuda()), cpu(x)
            assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), want_codes), (shape, family)
        assert rows == [1, 7, 33, 300]
        assert gpu._w_codes4 is None and gpu._w_idx4 is None


@pytest.mark.gpu
def test_a_padded_chain_gives_the_same_bits_gpu():
    x, y = check_padded_chain("cuda")
    _, want = check_padded_chain("cpu")                                # the same seeded stack and input on the CPU route
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())


def _expected_launches(m, dtype):
    """Library launches of one forward of an integer consumer: the quantize pass of a float32 input, the gather (every
    QuantizedConv2d; a padded Linear or pointwise layer), the row sums of weights with zero points, the product."""
    from mct_quantizers_amd import consumers
    if isinstance(m, consumers.QuantizedDepthwiseConv2d):
        return (dtype == torch.float32) + 1
    gathers = type(m) is consumers.QuantizedConv2d or m._k_pitch is not None
    return (dtype == torch.float32) + gathers + (m._w_zps is not None) + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_whole_models_with_every_switch_equal_the_rewrite_without_any_channels_gpu(name):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    gm, gm0 = rewritten_pair(name, "cuda")
    x = model_input(name, "cuda")
    gm(x)                                                              # (weight codes)
    seen, hooks = {}, []
    for mod_name, m in gm.named_modules():
        if isinstance(m, (consumers.IntegerConsumer, consumers._OnCodes)):
            hooks.append(m.register_forward_pre_hook(lambda m, a, k=mod_name: seen.__setitem__(k, [native.launch_count(), a[0].dtype])))
            hooks.append(m.register_forward_hook(lambda m, a, out, k=mod_name: seen[k].append(native.launch_count())))
    n0 = native.launch_count()
    y = gm(x)
    total = native.launch_count() - n0
    for h in hooks:
        h.remove()
    y0 = gm0(x)
    assert y.dtype == torch.float32 and torch.equal(y, y0) and len(torch.unique(y)) > 50
    gm_cpu, _ = rewritten_pair(name, "cpu")
    assert torch.equal(y.cpu(), gm_cpu(x.cpu()))
    per_module = {k: after - before for k, (before, _, after) in seen.items()}
    for k, (_, dtype, _) in seen.items():
        m = gm.get_submodule(k)
        if isinstance(m, consumers.IntegerConsumer):
            assert per_module[k] == _expected_launches(m, dtype), (k, per_module[k], dtype)
            # only the model's first layer quantizes: everything behind it arrives as codes
            assert dtype in (torch.int8, torch.uint8) or k == "c0_qlinear", (k, dtype)
    # every library launch of the forward belongs to one of those modules: nothing runs fake-quant or a float32 product
    assert total == sum(per_module.values()), (total, per_module)
    padded = [k for k in per_module if getattr(gm.get_submodule(k), "_k_pitch", None) is not None]
    assert sorted(padded) == sorted(MODELS[name][4])


@pytest.mark.gpu
def test_a_padded_layer_replays_from_a_hip_graph():
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    model = conv_model(C=3, O=8, k=7, stride=2, padding=3).cuda()
    assert consumers.fuse_linear_consumers(model, convolutions=True, any_channels=True) == 1 and model[1]._k_pitch == 160
    x = torch.randn(2, 3, 11, 13, device="cuda") * 1.5
    captured = mq.capture_forward(model, x, batch_weights=False)
    x2 = x * 0.5 + 0.25
    out = captured(x2).clone()                                          # one capture, one replay
    eager = model(x2)
    assert bits_equal(out.cpu().numpy(), eager.detach().cpu().numpy()) and not torch.equal(out, model(x))
