"""mctq_qlinear_i8_res, consumers.qlinear_i8(residual=...) and fuse_linear_consumers_fx(fused_residuals=True) on the GPU.

Reference: the CPU route (consumers.qlinear_i8 on CPU tensors), which tests/test_residual_consumer.py pins to the float32 product
followed by the join.  The integer sums are exact and the epilogue is the same float32 arithmetic, so every kernel the residual
form can be dispatched to must equal it bit for bit, for every shape, tail, code type and residual form, at the extremes of the
int32 accumulator included, and write nothing outside its output.  A model rewritten with ``fused_residuals`` must equal the
same rewrite without it on the GPU, and its own CPU route, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_gpu_stay_on_codes import _launches_per_forward
from test_join_consumer import FORMS
from test_residual_consumer import RESIDUAL_MODELS, _joins, block_input, rewrite

GUARD, SENTINEL = 64, 0xA5
VARIANTS = [0, 181, 182, 184, 83233, 86433, 86633, 812613, 166623, 1612623, 612, 1212, 662]
# ragged in M and N against every tile (16 ... 128 rows, 16 ... 128 columns), the smallest and the largest K
SHAPES = [(1, 16, 16), (5, 100, 256), (16, 33, 272), (17, 16, 4096), (130, 20, 528), (129, 130, 144), (300, 257, 1040),
          (2, 3, 32768)]
R_KINDS = {"f32": None, "i8": (0.23, -7), "u8": (0.19, 101)}                # the residual's (scale, zero_point)
OUTS = [None, FORMS["u8"], FORMS["i8"]]                                     # float32, uint8 codes, int8 codes
A_SCALE = 0.02


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, u8):
    """One problem per (shape, code type), shared by every launch variant: the operands, the exact int32 sums, the three
    residuals.  x is of the order of 30, inside and beyond both output domains; K = 32768 holds the accumulator's extremes."""
    g = torch.Generator().manual_seed(7 * M + 3 * N + K + u8)
    a = torch.randint(0, 256, (M, K), generator=g).to(torch.uint8) if u8 else torch.randint(-128, 128, (M, K), generator=g).to(torch.int8)
    w = torch.randint(-128, 128, (N, K), generator=g).to(torch.int8)
    za = 114 if u8 else -5
    if K == 32768:
        if u8:
            a[:], za, w[:] = 255, 0, -128                                    # sum = 255 * (-128) * 32768
            w[1] = 127                                                       # ... and 255 * 127 * 32768
        else:
            a[:], za, w[:] = -128, 127, 127                                  # sum = (-255) * 127 * 32768
            w[1] = -128                                                      # ... and (-255) * (-128) * 32768
    ws = ((torch.rand(N, generator=g) + 0.5) * (30.0 / (A_SCALE * 5476.0 * K ** 0.5))).float().contiguous()
    bias = ((torch.rand(N, generator=g) - 0.5) * 20).float().contiguous()
    acc = (a.to(torch.int32) - za) @ w.to(torch.int32).t()
    r32 = ((torch.rand(M, N, generator=g) - 0.5) * 80).float()
    flat = r32.reshape(-1)
    flat[::7] = -flat[::7].abs() - 40                                        # sums well below zero under the ReLU
    for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
        flat[(i * 5) % flat.numel()] = v
    residuals = {"f32": r32.contiguous(), "i8": torch.randint(-128, 128, (M, N), generator=g).to(torch.int8),
                 "u8": torch.randint(0, 256, (M, N), generator=g).to(torch.uint8)}
    return dict(a=a, za=za, w=w, ws=ws, rowsum=w.sum(dim=1, dtype=torch.int32).contiguous(), bias=bias, acc=acc, residuals=residuals)


def _combos():
    """(residual kind, relu, with bias, output form): every residual x ReLU x bias, the three output forms dealt over them."""
    i = 0
    for kind in R_KINDS:
        for relu in (False, True):
            for with_bias in (False, True):
                yield kind, relu, with_bias, OUTS[i % 3]
                i += 1


@functools.lru_cache(maxsize=None)
def _wanted(M, N, K, u8):
    """The CPU route's result for every combination, from the shared int32 sums (consumers._cpu_epilogue is that route's
    epilogue); the first combination is also computed by the public function, sums and all."""
    from mct_quantizers_amd import consumers
    p = _problem(M, N, K, u8)
    want = {}
    for kind, relu, with_bias, out in _combos():
        want[(kind, relu, with_bias)] = consumers._cpu_epilogue(p["acc"], A_SCALE, p["ws"], p["bias"] if with_bias else None, out,
                                                                p["residuals"][kind], R_KINDS[kind], relu).numpy()
    kind, relu, with_bias, out = next(_combos())
    public = consumers.qlinear_i8(p["a"], p["za"], A_SCALE, p["w"], p["ws"], p["rowsum"], None, out, residual=p["residuals"][kind],
                                  residual_codes=R_KINDS[kind], relu=relu).numpy()
    assert bits_equal(public, want[(kind, relu, with_bias)])
    return want


def _raw_into_guarded_buffer(lib, dev, M, N, K, u8, kind, relu, with_bias, out):
    """One call of the raw entry point, y in the middle of a sentinel-filled buffer -> (y as numpy, the launch note); the
    sentinels are checked here."""
    from mct_quantizers_amd.hip import native
    size = M * N * (4 if out is None else 1)
    buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    r = dev["residuals"][kind]
    r_scale, r_zp = R_KINDS[kind] or (0.0, 0)
    rdt = -1 if kind == "f32" else native.CODE_I8 if kind == "i8" else native.CODE_U8
    form = (-1, 1.0, 0, 0, 0) if out is None else (native.CODE_U8 if out[2] >= 0 else native.CODE_I8, out[0], out[1], out[2], out[3])
    count = native.launch_count()
    rc = lib.mctq_qlinear_i8_res(dev["a"].data_ptr(), native.CODE_U8 if u8 else native.CODE_I8, dev["za"], A_SCALE, dev["w"].data_ptr(),
                                 dev["ws"].data_ptr(), dev["rowsum"].data_ptr(), dev["bias"].data_ptr() if with_bias else None,
                                 r.data_ptr(), rdt, r_scale, r_zp, int(relu), buf.data_ptr() + GUARD, *form, M, N, K,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    assert native.launch_count() - count == 1, launch
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + size:] == SENTINEL), (M, N, K, u8, kind, relu, launch)
    y = got[GUARD:GUARD + size]
    y = y.view(np.float32) if out is None else y.view(np.uint8 if out[2] >= 0 else np.int8)
    return y.reshape(M, N), launch


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_residual_kernel_is_bit_exact_against_the_cpu_route_and_stays_inside_its_output(variant):
    from mct_quantizers_amd.hip import native
    lib = native.load()
    assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
    try:
        for (M, N, K) in SHAPES:
            for u8 in (False, True):
                p, want = _problem(M, N, K, u8), _wanted(M, N, K, u8)
                dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in p.items() if k != "acc"}
                dev["residuals"] = {k: v.cuda() for k, v in p["residuals"].items()}
                for kind, relu, with_bias, out in _combos():
                    got, launch = _raw_into_guarded_buffer(lib, dev, M, N, K, u8, kind, relu, with_bias, out)
                    what = f"variant {variant} M={M} N={N} K={K} u8={u8} res={kind} relu={relu} bias={with_bias} [{launch}]"
                    assert launch.startswith("qlinear") and f" res({kind})" in launch and (" relu" in launch) == relu, what
                    assert ("u8 x i8" in launch) == u8 and "wide" not in launch and "pingpong" not in launch, what
                    w = want[(kind, relu, with_bias)]
                    assert bits_equal(got, w), f"{what}: {first_mismatch(got, w)}"
    finally:
        lib.mctq_set_tuning(b"ql_variant", 0)


def test_the_cases_hold_what_they_claim():
    """(No GPU.)  Both clamp ends and many codes in every codes output (behind a ReLU the lower end is the code of zero, unless
    a NaN is among the sums), a NaN in the float32 ones, negative sums in front of every ReLU, the accumulator's extremes at the
    largest K."""
    for (M, N, K) in SHAPES[1:]:
        for u8 in (False, True):
            want = _wanted(M, N, K, u8)
            for kind, relu, with_bias, out in _combos():
                w = want[(kind, relu, with_bias)]
                if out is not None:
                    low = out[1] if relu and kind != "f32" else out[2]
                    assert w.min() == low and w.max() == out[3] and (K == 32768 or len(np.unique(w)) > 50), (M, N, K, kind, relu)
                elif kind == "f32":
                    assert np.isnan(w).any()
                if relu and out is None:
                    assert not (w < 0).any() and (w == 0).any()
    acc = _problem(2, 3, 32768, True)["acc"]
    assert int(acc.min()) == 255 * -128 * 32768 and int(acc.max()) == 255 * 127 * 32768
    acc = _problem(2, 3, 32768, False)["acc"]
    assert int(acc.min()) == -255 * 127 * 32768 and int(acc.max()) == 255 * 128 * 32768


@pytest.mark.gpu
def test_a_residual_sends_whole_tile_products_to_the_tiled_kernels():
    """4096 x 4096 x 256 fills the chip with whole tiles: the plain form goes to a register-pinned kernel, the residual form to
    the tiled ones.  The exact sums come from a float64 product (|sum| < 2^24), the rest is the CPU route's epilogue."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    M, N, K = 4096, 4096, 256
    g = torch.Generator().manual_seed(77)
    a = torch.randint(0, 256, (M, K), generator=g).to(torch.uint8)
    w = torch.randint(-128, 128, (N, K), generator=g).to(torch.int8)
    ws = ((torch.rand(N, generator=g) + 0.5) * (30.0 / (A_SCALE * 5476.0 * 16))).float()
    bias = ((torch.rand(N, generator=g) - 0.5) * 20).float()
    rc8 = torch.randint(0, 256, (M, N), generator=g).to(torch.uint8)
    rowsum = w.sum(dim=1, dtype=torch.int32)
    acc = ((a.double() - 114) @ w.double().t()).to(torch.int32)
    form, r_form = FORMS["u8"], R_KINDS["u8"]
    want = consumers._cpu_epilogue(acc, A_SCALE, ws, bias, form, rc8, r_form, True)
    at, wt, wst, bt, rt, rst = (t.cuda() for t in (a, w, ws, bias, rc8, rowsum))
    x = consumers.qlinear_i8(at, 114, A_SCALE, wt, wst, rst, bt)
    plain = native.last_launch()
    assert plain.startswith("qlinear_wide") or plain.startswith("qlinear_pingpong"), plain
    got = consumers.qlinear_i8(at, 114, A_SCALE, wt, wst, rst, bt, form, residual=rt, residual_codes=r_form, relu=True)
    launch = native.last_launch()
    assert launch.startswith("qlinear_tiled") and " res(u8) relu" in launch, launch
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    # ... and the two launches it replaces, on the GPU
    pair = ops.fq_join(x, *form, residual_codes=(rt, *r_form), relu=True, want_float=False)[1]
    assert torch.equal(got, pair)
    assert len(torch.unique(got)) == 256 - form[1]                          # behind the ReLU: the code of zero and everything above


@pytest.mark.gpu
def test_consumer_modules_take_a_residual_on_gpu():
    """QuantizedConv1x1 and QuantizedConv2d with a float32 and a codes residual, channels-last (a view) and NCHW-contiguous (a
    copy): the join of the module's own float32 output."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    from test_conv_consumer import conv_pair
    form = FORMS["u8"]
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 16, 9, 7, generator=g) * 1.5).cuda()
    r32 = torch.randn(2, 32, 9, 7, generator=g).cuda()
    rc8 = torch.randint(0, 256, (2, 32, 9, 7), generator=g).to(torch.uint8).cuda()
    for k, cls in ((1, consumers.QuantizedConv1x1), (3, consumers.QuantizedConv2d)):
        holder, wrapper = conv_pair(C=16, O=32, k=k, padding=k // 2, seed=4)
        fused = cls.from_wrapper(wrapper.cuda(), holder.activation_holder_quantizer)
        y = fused(x)
        for residual, how in ((r32, "float"), (rc8, (0.19, 101))):
            fused.emit_codes_for, fused.emit_residual, fused.emit_relu = form, how, True
            kw = dict(residual=residual) if how == "float" else dict(residual_codes=(residual, *how))
            want = ops.fq_join(y, *form, relu=True, want_float=False, **kw)[1]
            for r in (residual, residual.contiguous(memory_format=torch.channels_last)):
                got = fused(x, r)
                assert " res(" in native.last_launch() and " relu" in native.last_launch(), native.last_launch()
                assert torch.equal(got, want) and got.stride() == want.stride()
        fused.emit_codes_for = fused.emit_residual = None
        fused.emit_relu = False


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RESIDUAL_MODELS))
@pytest.mark.parametrize("channels_last", [False, True])
def test_rewritten_models_on_gpu(name, channels_last):
    """Bit for bit the rewrite without ``fused_residuals`` on the GPU and the model's own CPU route.  Every removed join was one
    launch and its producer's launch only changed its form, so the launches per forward drop by exactly the joins removed."""
    make, switches, removed = RESIDUAL_MODELS[name]
    gm, gm0 = rewrite(make, "cuda", **switches)
    x = block_input("cuda", channels_last)
    (y, launches), (y0, launches0) = _launches_per_forward(gm, x), _launches_per_forward(gm0, x)
    assert y.is_cuda and len(torch.unique(y)) > 50
    assert bits_equal(y.cpu().numpy(), y0.cpu().numpy()), first_mismatch(y.cpu().numpy(), y0.cpu().numpy())
    want = rewrite(make, "cpu", **switches)[0](block_input("cpu", channels_last))
    assert bits_equal(y.cpu().numpy(), want.numpy()), first_mismatch(y.cpu().numpy(), want.numpy())
    assert len(_joins(gm0)) - len(_joins(gm)) == removed and launches0 - launches == removed, (launches0, launches)
