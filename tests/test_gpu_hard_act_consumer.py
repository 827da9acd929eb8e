"""mctq_qlinear_i8_act, mctq_qconv_dw_i8_act, consumers.qlinear_i8(act=...) / qconv_dw_i8(act=...) and
fuse_linear_consumers_fx(hard_activations=True) on the GPU.

Reference, everywhere: the float32 chain ON THE GPU -- the float32 result of the plain entry point, ``F.hardswish`` /
``F.hardsigmoid`` of that GPU tensor, ``ops.fq_codes`` in the output form.  The integer sums are exact, the register in front of
the activation holds the float32 value the plain entry point stores, and the kernels evaluate the expression of ATen's GPU kernels
(docs/KERNEL_NOTES.md), so every check is ``torch.equal``: there is no tolerance anywhere.  (The CPU route is no reference here:
ATen's CPU kernels round differently for a quarter of all inputs.)  The problems are those of tests/test_hard_act_consumer.py."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_residual_consumer import A_SCALE, GUARD, SENTINEL, SHAPES, VARIANTS
from test_gpu_stay_on_codes import _launches_per_forward
from test_hard_act_consumer import (ACTS, HARD_MODELS, OUT_FORMS, SWITCHES, _activation_nodes, act_combos, act_problem, chain_codes,
                                    rewrite_pair)

F = torch.nn.functional
ACT_CODE = {"hardswish": 1, "hardsigmoid": 2}


def _form_args(form):
    from mct_quantizers_amd.hip import native
    return (native.CODE_U8 if form[2] >= 0 else native.CODE_I8, form[0], form[1], form[2], form[3])


@functools.lru_cache(maxsize=None)
def _on_gpu(M, N, K, u8):
    """The problem's operands on the GPU and, per combination, the GPU chain's codes behind the plain entry point (automatic
    launch choice): computed once, shared by every launch variant."""
    from mct_quantizers_amd import consumers
    p = act_problem(M, N, K, u8)
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in p.items() if k != "acc"}
    want = {}
    for with_bias in (False, True):
        y = consumers.qlinear_i8(dev["a"], dev["za"], A_SCALE, dev["w"], dev["ws"], dev["rowsum"], dev["bias"] if with_bias else None)
        assert y.dtype == torch.float32
        for act in ACTS:
            for kind, form in OUT_FORMS[act].items():
                want[(act, with_bias, kind)] = chain_codes(y, act, form)
    return dev, want


def _raw_into_guarded_buffer(lib, dev, M, N, K, u8, act, with_bias, form):
    """One call of the raw entry point, y in the middle of a sentinel-filled buffer -> (codes [M, N] on the GPU, the launch
    note); the sentinels are checked here."""
    from mct_quantizers_amd.hip import native
    size = M * N
    buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    count = native.launch_count()
    rc = lib.mctq_qlinear_i8_act(dev["a"].data_ptr(), native.CODE_U8 if u8 else native.CODE_I8, dev["za"], A_SCALE, dev["w"].data_ptr(),
                                 dev["ws"].data_ptr(), dev["rowsum"].data_ptr(), dev["bias"].data_ptr() if with_bias else None,
                                 buf.data_ptr() + GUARD, *_form_args(form), ACT_CODE[act], M, N, K,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    assert native.launch_count() - count == 1, launch
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + size:] == SENTINEL).all()), (M, N, K, u8, act, launch)
    y = buf[GUARD:GUARD + size]
    return (y if form[2] >= 0 else y.view(torch.int8)).reshape(M, N), launch


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_activation_kernel_equals_the_gpu_chain_and_stays_inside_its_output(variant):
    from mct_quantizers_amd.hip import native
    lib = native.load()
    problems = [(shape, u8, *_on_gpu(*shape, u8)) for shape in SHAPES for u8 in (False, True)]       # (plain launches: automatic)
    assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
    try:
        for (M, N, K), u8, dev, want in problems:
            for act, with_bias, kind in act_combos():
                got, launch = _raw_into_guarded_buffer(lib, dev, M, N, K, u8, act, with_bias, OUT_FORMS[act][kind])
                what = f"variant {variant} M={M} N={N} K={K} u8={u8} {act} bias={with_bias} {kind} [{launch}]"
                assert launch.startswith("qlinear") and f" {act}," in launch, what
                assert ("u8 x i8" in launch) == u8 and "wide" not in launch and "pingpong" not in launch, what
                w = want[(act, with_bias, kind)]
                assert got.dtype == w.dtype and torch.equal(got, w), f"{what}: {int((got != w).sum())} codes differ"
    finally:
        lib.mctq_set_tuning(b"ql_variant", 0)


@pytest.mark.gpu
def test_the_register_pinned_kernels_refuse_an_activation():
    from mct_quantizers_amd.hip import native
    lib = native.load()
    dev, _ = _on_gpu(*SHAPES[0], True)
    M, N, K = SHAPES[0]
    y = torch.empty(M * N, dtype=torch.uint8, device="cuda")
    try:
        for variant in (2544, 2548, 2560):
            assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
            rc = lib.mctq_qlinear_i8_act(dev["a"].data_ptr(), native.CODE_U8, dev["za"], A_SCALE, dev["w"].data_ptr(), dev["ws"].data_ptr(),
                                         dev["rowsum"].data_ptr(), None, y.data_ptr(), *_form_args(OUT_FORMS["hardswish"]["u8"]), 1,
                                         M, N, K, torch.cuda.current_stream().cuda_stream)
            assert rc == native.MCTQ_E_ARG and b"not built for an activation" in lib.mctq_last_error()
    finally:
        lib.mctq_set_tuning(b"ql_variant", 0)


@pytest.mark.gpu
def test_an_activation_sends_whole_tile_products_to_the_tiled_kernels():
    """4096 x 4096 x 256 fills the chip with whole tiles: the plain form goes to a register-pinned kernel, the activation form to
    the tiled ones, and equals the chain behind the plain form."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    M, N, K = 4096, 4096, 256
    g = torch.Generator().manual_seed(78)
    a = torch.randint(0, 256, (M, K), generator=g).to(torch.uint8).cuda()
    w = torch.randint(-128, 128, (N, K), generator=g).to(torch.int8)
    ws = ((torch.rand(N, generator=g) + 0.5) * (4.0 / (A_SCALE * 5476.0 * 16))).float().cuda()
    bias = ((torch.rand(N, generator=g) - 0.5) * 4).float().cuda()
    rowsum, w = w.sum(dim=1, dtype=torch.int32).cuda(), w.cuda()
    x = consumers.qlinear_i8(a, 114, A_SCALE, w, ws, rowsum, bias)
    plain = native.last_launch()
    assert plain.startswith("qlinear_wide") or plain.startswith("qlinear_pingpong"), plain
    for act in ACTS:
        form = OUT_FORMS[act]["u8"]
        got = consumers.qlinear_i8(a, 114, A_SCALE, w, ws, rowsum, bias, form, act=act)
        launch = native.last_launch()
        assert launch.startswith("qlinear_tiled") and f" {act}," in launch, launch
        want = chain_codes(x, act, form)
        assert got.dtype == torch.uint8 and torch.equal(got, want), int((got != want).sum())
        assert len(torch.unique(got)) > 200


def _bit_patterns(bits):
    """int64 bit patterns (any device) -> the float32 values that have them"""
    bits = bits & 0xFFFFFFFF
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)


def _sweep_values():
    """Every 257th float32 bit pattern of both signs (16.7 million), every pattern within 4096 ulps of -3, -0.0, +0.0, 3 and
    the infinities, and NaN payloads of both signs: as chunks of 2^20 values (the last one padded with zeros)."""
    f2b = lambda v: int(np.float32(v).view(np.uint32))                       # noqa: E731
    every = torch.arange(0, 1 << 32, 257, dtype=torch.int64, device="cuda")
    near = torch.arange(-4096, 4097, dtype=torch.int64, device="cuda")
    centres = [f2b(-3.0), f2b(-0.0), f2b(0.0), f2b(3.0), f2b(np.inf), f2b(-np.inf)]          # (past an infinity: NaNs)
    nans = torch.tensor([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5], dtype=torch.int64,
                        device="cuda")
    bits = torch.cat([every] + [near + c for c in centres] + [nans])
    values = _bit_patterns(bits)
    pad = -values.numel() % (1 << 20)
    return torch.cat([values, values.new_zeros(pad)]).reshape(-1, 1 << 20)


@pytest.mark.gpu
def test_every_kind_of_float32_value_through_the_bias():
    """K = 16, activation codes at the zero point, weights 0: the epilogue's value is exactly bias[n], whatever float32 that is.
    M = 1, N = 2^20 per launch."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    N, K = 1 << 20, 16
    chunks = _sweep_values()
    assert chunks.shape[0] >= 16 and bool(chunks.isnan().any()) and bool((chunks == float("inf")).any())
    w = torch.zeros((N, K), dtype=torch.int8, device="cuda")
    rowsum = torch.zeros(N, dtype=torch.int32, device="cuda")
    ws = torch.ones(N, dtype=torch.float32, device="cuda")
    for u8 in (True, False):
        za = 114 if u8 else -5
        a = torch.full((1, K), za, dtype=torch.uint8 if u8 else torch.int8, device="cuda")
        for bias in chunks:
            bias = bias.contiguous()
            y = consumers.qlinear_i8(a, za, 0.5, w, ws, rowsum, bias)
            same = (y.view(torch.int32) == bias.view(torch.int32)) | (y.isnan() & bias.isnan()) | ((y == 0) & (bias == 0))
            assert bool(same.all())                                          # (0 + -0.0 = +0.0: the one value that changes)
            for act in ACTS:
                form = OUT_FORMS[act]["u8" if u8 else "i8"]
                got = consumers.qlinear_i8(a, za, 0.5, w, ws, rowsum, bias, form, act=act)
                assert f" {act}," in native.last_launch()
                want = chain_codes(y, act, form)
                assert torch.equal(got, want), (act, u8, int((got != want).sum()))


def _dw_raw(case, form, act):
    """The raw depthwise entry point with an activation, its output in the middle of a sentinel-filled buffer."""
    from mct_quantizers_amd.hip import native
    lib = native.load()
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case["geometry"]
    B, H, W, C = case["a"].shape
    ho, wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    n = B * ho * wo * C
    dev = lambda v: None if v is None else torch.from_numpy(v.copy()).cuda()          # noqa: E731
    a, w, ws, zw, bias = (dev(case[k]) for k in ("a", "w", "ws", "zw", "bias"))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    ptr = lambda t: None if t is None else t.data_ptr()                                # noqa: E731
    rc = lib.mctq_qconv_dw_i8_act(a.data_ptr(), native.CODE_U8 if a.dtype == torch.uint8 else native.CODE_I8, case["za"], case["sa"],
                                  w.data_ptr(), ws.data_ptr(), ptr(zw), ptr(bias), buf.data_ptr() + GUARD, *_form_args(form),
                                  ACT_CODE[act], B, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), (case["geometry"], C)
    y = buf[GUARD:GUARD + n]
    return (y if form[2] >= 0 else y.view(torch.int8)).reshape(B, ho, wo, C), launch


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
def test_depthwise_activation_kernel_equals_the_gpu_chain_and_stays_inside_its_output(act):
    from test_dw_consumer import raw_case, raw_cases, run_raw_on
    with_zp = 0
    for i, case in enumerate(raw_cases()):
        c = raw_case(*case)
        y = run_raw_on(c, "cuda")                                            # the plain entry point's float32
        form = OUT_FORMS[act]["u8" if i % 2 else "i8"]
        got, launch = _dw_raw(c, form, act)
        assert launch.startswith("qconv_dw<") and f" {act}," in launch and (" zp " in launch) == (c["zw"] is not None), launch
        want = chain_codes(y, act, form)
        assert got.dtype == want.dtype and torch.equal(got, want), (case, int((got != want).sum()))
        with_zp += c["zw"] is not None
    assert i == 71 and with_zp == 36


@pytest.mark.gpu
def test_consumer_modules_emit_an_activation_on_gpu():
    """QuantizedLinear, QuantizedConv1x1, QuantizedConv2d and QuantizedDepthwiseConv2d with ``emit_act``, NCHW and channels-last:
    the chain behind the module's own float32 output."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    from test_conv_consumer import conv_pair
    from test_stay_on_codes import linear_pair
    g = torch.Generator().manual_seed(13)
    x4 = (torch.randn(2, 16, 9, 7, generator=g) * 1.5).cuda()
    layers = [(consumers.QuantizedConv1x1, conv_pair(C=16, O=32, k=1, padding=0, seed=4), x4),
              (consumers.QuantizedConv2d, conv_pair(C=16, O=32, k=3, padding=1, seed=5), x4),
              (consumers.QuantizedDepthwiseConv2d, conv_pair(C=16, O=16, k=3, padding=1, seed=6, groups=16), x4),
              (consumers.QuantizedDepthwiseConv2d, conv_pair(C=16, O=16, k=3, padding=1, seed=7, groups=16, family="uniform"), x4),
              (consumers.QuantizedLinear, linear_pair(48, 40, "sym", "signed", 8), (torch.randn(5, 48, generator=g) * 1.5).cuda())]
    for cls, (holder, wrapper), x in layers:
        fused = cls.from_wrapper(wrapper.cuda(), holder.activation_holder_quantizer)
        y = fused(x)
        assert y.dtype == torch.float32
        for act in ACTS:
            for form in OUT_FORMS[act].values():
                fused.emit_codes_for, fused.emit_act = form, act
                want = chain_codes(y, act, form)
                for xx in ((x, x.contiguous(memory_format=torch.channels_last)) if x.dim() == 4 else (x,)):
                    got = fused(xx)
                    assert f" {act}," in native.last_launch(), native.last_launch()
                    assert torch.equal(got, want) and got.stride() == want.stride(), (cls.__name__, act, form)
        fused.emit_codes_for = fused.emit_act = None


# Library launches per forward saved by the switch, from the graphs (tests/test_hard_act_consumer.py: test_graph_shapes).  A folded
# activation in front of a consumer or of a concatenation's operand: the reader no longer launches the quantization of a float32
# tensor -- one launch each; the producer's launch only changes its form and ATen's activation launch (not a library launch)
# goes too.  The SE gate: the multiply's kernel codes a float32 [B, C, 1, 1] gate itself (C % 16 == 0), so there no library launch
# goes, only ATen's.
LAUNCHES_SAVED = {"pointwise": 1, "depthwise": 2, "se": 0, "cat": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HARD_MODELS))
@pytest.mark.parametrize("channels_last", [False, True])
def test_rewritten_models_on_gpu(name, channels_last):
    """Bit for bit the same rewrite without ``hard_activations`` on the GPU."""
    from test_mul_consumer import block_input
    make, producers = HARD_MODELS[name]
    (gm, n), (gm0, n0) = rewrite_pair(make, "cuda")
    x = block_input("cuda")
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    (y, launches), (y0, launches0) = _launches_per_forward(gm, x), _launches_per_forward(gm0, x)
    assert n == n0 and y.is_cuda and len(torch.unique(y)) > 50
    assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), int((y != y0).sum())
    assert len(_activation_nodes(gm0)) == len(producers) and not _activation_nodes(gm)
    assert launches0 - launches == LAUNCHES_SAVED[name], (launches0, launches)
    assert SWITCHES["stay_on_codes"]
