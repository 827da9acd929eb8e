"""mctq_codes_rowsum, mctq_qlinear_i8_zp, mctq_qlinear_w4a8_zp and the uniform-weights routes of consumers.QuantizedLinear
on the GPU.

Oracle: oracle/mctq_oracle.py::qlinear_i8 on ``w_codes - zw[:, None]`` (tests/test_zp_consumer.py: zp_oracle): the exact
integer product scaled once.  Every kernel the zero-point form can be dispatched to must equal it bit for bit, for every
shape, tail and code type, at the two extremes of the int32 accumulator included."""
import functools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_zp_consumer import check_against_oracle_and_float64, check_chain, uniform_model, zp_oracle, zp_problem

OUTS = ((0.05, 3, -128, 127), (0.11, 100, 0, 255), (0.5, 0, -8, 7))
ZP_VARIANTS = [0, 181, 182, 184, 83233, 86433, 86633, 812613, 166623, 1612623, 612, 1212, 662]
ZP_SHAPES = [(1, 16, 16), (5, 100, 256), (16, 33, 272), (17, 16, 4096), (130, 20, 528), (129, 130, 144), (300, 257, 1040),
             (2, 3, 32768)]


def _dev(*arrays):
    return tuple(None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in arrays)


def _rowsum_w(w):
    return torch.from_numpy(np.asarray(w).astype(np.int32).sum(1, dtype=np.int32)).cuda()


def _run_zp(a, za, sa, w, zw, ws, bias, out=None):
    from mct_quantizers_amd import consumers
    at, wt, zt, wst, bt = _dev(a, w, zw, ws, bias)
    return consumers.qlinear_i8(at, za, sa, wt, wst, _rowsum_w(w), bt, out, w_zero_points=zt)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True])
def test_codes_rowsum_kernel_matches_numpy_and_stays_inside_its_output(u8):
    from mct_quantizers_amd.hip import native
    lib = native.load()
    rng = np.random.default_rng(5 + u8)
    st = torch.cuda.current_stream().cuda_stream
    code = native.CODE_U8 if u8 else native.CODE_I8
    GUARD, SENTINEL = 8, -0x5A5A5A5B
    for M in (1, 3, 64, 65, 300):                                    # one block per row up to 64 rows, one wave per row beyond
        for K in (16, 1008, 1024, 1040, 32768):
            a = rng.integers(0, 256, (M, K)).astype(np.uint8) if u8 else rng.integers(-128, 128, (M, K)).astype(np.int8)
            if K == 32768:
                a[0] = 255 if u8 else -128                           # the longest row of the extreme code
                if M > 1:
                    a[M - 1] = 0 if u8 else 127
            za = int(rng.integers(0, 256)) if u8 else int(rng.integers(-128, 128))
            if K == 32768 and M == 1:
                za = 0 if u8 else 127                                # |sum| = 255 * 32768
            at, = _dev(a)
            buf = torch.full((M + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
            rc = lib.mctq_codes_rowsum(at.data_ptr(), code, za, buf.data_ptr() + 4 * GUARD, M, K, st)
            assert rc == 0, lib.mctq_last_error()
            assert native.last_launch().startswith("codes_rowsum<"), native.last_launch()
            assert ("block per row" in native.last_launch()) == (M <= 64), native.last_launch()
            got = buf.cpu().numpy()
            assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + M:] == SENTINEL), (M, K)
            assert np.array_equal(got[GUARD:GUARD + M], (a.astype(np.int64) - za).sum(1)), (M, K, u8)


@pytest.mark.gpu
def test_codes_rowsum_rejects_bad_arguments():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    lib = native.load()
    a = torch.zeros(4, 64, dtype=torch.int8, device="cuda")
    o = torch.zeros(4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    E = native.MCTQ_E_ARG
    n0 = native.launch_count()
    assert lib.mctq_codes_rowsum(None, native.CODE_I8, 0, None, 0, 64, st) == 0                      # no rows: no launch
    assert native.launch_count() == n0
    assert lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_I8, 0, o.data_ptr(), 4, 24, st) == E
    assert b"multiple of 16" in lib.mctq_last_error()
    assert lib.mctq_codes_rowsum(a.data_ptr(), 77, 0, o.data_ptr(), 4, 64, st) == E
    assert lib.mctq_codes_rowsum(a.data_ptr() + 1, native.CODE_I8, 0, o.data_ptr(), 4, 64, st) == E
    assert lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_I8, 0, o.data_ptr(), 4, 65536, st) == E
    assert lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_I8, 0, None, 4, 64, st) == E
    assert lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_I8, 0, o.data_ptr(), -1, 64, st) == E
    assert native.launch_count() == n0
    assert torch.equal(consumers.codes_rowsum(a + 3, 1), torch.full((4,), 128, dtype=torch.int32, device="cuda"))


@functools.lru_cache(maxsize=None)
def _zp_case(M, N, K, u8):
    """One problem per (shape, code type) and its oracle result, shared by every launch variant."""
    rng = np.random.default_rng(7 * M + 3 * N + K + u8)
    a, za, sa, w, zw, ws, bias = zp_problem(rng, M, N, K, u8, with_bias=((M + N) % 2 == 1) == u8)
    if K == 32768:                                                   # the two extremes of the accumulator
        if u8:
            a[:], za, w[:], zw[:] = 255, 0, -128, 127                # sum = 255 * (-255) * 32768
        else:
            a[:], za, w[:], zw[:] = -128, 127, 127, -128             # sum = (-255) * 255 * 32768
    return (a, za, sa, w, zw, ws, bias), zp_oracle(a, za, sa, w, zw, ws, bias)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ZP_VARIANTS)
def test_qlinear_zp_kernel_is_bit_exact_against_the_integer_oracle(variant):
    from mct_quantizers_amd.hip import native
    lib = native.load()
    assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
    try:
        biased = set()
        for (M, N, K) in ZP_SHAPES:
            for u8 in (False, True):
                args, want = _zp_case(M, N, K, u8)
                biased.add((u8, args[-1] is not None))
                got = _run_zp(*args).cpu().numpy()
                launch = native.last_launch()
                assert launch.startswith("qlinear") and (" zp," in launch) and ("u8 x i8" in launch) == u8, launch
                assert "wide" not in launch and "pingpong" not in launch, launch
                assert bits_equal(got, want), f"variant {variant} M={M} N={N} K={K} u8={u8} [{launch}]: {first_mismatch(got, want)}"
        assert len(biased) == 4                                       # both code types, each with and without bias
    finally:
        lib.mctq_set_tuning(b"ql_variant", 0)


@pytest.mark.gpu
def test_qlinear_zp_skips_the_whole_tile_kernels_and_refuses_their_variants():
    from mct_quantizers_amd.hip import native
    lib = native.load()
    rng = np.random.default_rng(77)
    M, N, K = 4096, 4096, 256                                         # whole tiles, fills the chip: the plain form goes to the pinned kernels
    a, za, sa, w, zw, ws, bias = zp_problem(rng, M, N, K, True)
    try:
        got = _run_zp(a, za, sa, w, zw, ws, bias).cpu().numpy()
        launch = native.last_launch()
        assert launch.startswith("qlinear_tiled") and " zp," in launch, launch
        want = zp_oracle(a, za, sa, w, zw, ws, bias)
        assert bits_equal(got, want), first_mismatch(got, want)
        at, wt, zt, wst = _dev(a[:256], w[:256], zw[:256], ws[:256])
        rs, ars = _rowsum_w(w[:256]), torch.zeros(256, dtype=torch.int32, device="cuda")
        y = torch.zeros(256, 256, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        call = lambda zp_ptr, ars_ptr: lib.mctq_qlinear_i8_zp(                                   # noqa: E731
            at.data_ptr(), native.CODE_U8, za, sa, wt.data_ptr(), wst.data_ptr(), rs.data_ptr(), None, y.data_ptr(), -1, 1.0,
            0, 0, 0, zp_ptr, ars_ptr, 256, 256, 256, st)
        for variant in (2544, 2548, 2560):
            assert lib.mctq_set_tuning(b"ql_variant", variant) == 0
            assert call(zt.data_ptr(), ars.data_ptr()) == native.MCTQ_E_ARG
            assert b"zero-point" in lib.mctq_last_error()
        assert lib.mctq_set_tuning(b"ql_variant", 0) == 0
        assert call(None, ars.data_ptr()) == native.MCTQ_E_ARG and b"required" in lib.mctq_last_error()
        assert call(zt.data_ptr(), None) == native.MCTQ_E_ARG
        assert call(zt.data_ptr(), ars.data_ptr()) == 0
    finally:
        lib.mctq_set_tuning(b"ql_variant", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 17, 33, 130])
def test_w4a8_zp_kernel_is_bit_exact_against_the_integer_oracle(M):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    rng = np.random.default_rng(40 + M)
    for (N, K) in [(16, 16), (33, 272), (64, 4096)]:
        for u8 in (False, True):
            a, za, sa, w, zw, ws, bias = zp_problem(rng, M, N, K, u8, with_bias=(M + N + u8) % 2 == 1, w_lo=-8, w_hi=8)
            if K == 4096 and u8:
                w[:], zw[:] = -8, 7                                  # extreme codes
            at, wt, zt, wst, bt = _dev(a, w, zw, ws, bias)
            packed = consumers.pack_w4(wt)
            got = consumers.qlinear_w4a8(at, za, sa, packed, wst, _rowsum_w(w), bt, w_zero_points=zt)
            launch = native.last_launch()
            assert "qlinear_stream_w4" in launch and " zp," in launch, launch
            want = zp_oracle(a, za, sa, w, zw, ws, bias)
            g = got.cpu().numpy()
            assert bits_equal(g, want), f"M={M} N={N} K={K} u8={u8}: {first_mismatch(g, want)}"
            out = OUTS[0]
            codes = consumers.qlinear_w4a8(at, za, sa, packed, wst, _rowsum_w(w), bt, out, w_zero_points=zt)
            assert torch.equal(codes, ops.fq_codes(got, None, None, None, out[2], out[3], out[0], out[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 64, 300])
def test_requantizing_epilogue_with_zero_points_equals_the_codes_kernel(M):
    from mct_quantizers_amd.hip import ops
    rng = np.random.default_rng(M)
    N, K = 200, 512
    args = zp_problem(rng, M, N, K, True)
    y = _run_zp(*args)
    for out in OUTS:
        got = _run_zp(*args, out=out)
        want = ops.fq_codes(y, None, None, None, out[2], out[3], out[0], out[1])
        assert got.dtype == want.dtype and torch.equal(got, want), out


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("K,N,batch", [(64, 24, (3, 5)), (1024, 1000, (1,)), (4096, 512, (64,))])
def test_quantized_linear_with_uniform_weights_on_gpu(K, N, batch, per_channel):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    cpu_model = uniform_model(K=K, N=N, per_channel=per_channel)
    model = uniform_model(K=K, N=N, per_channel=per_channel).cuda()
    assert consumers.fuse_linear_consumers(model) == 0
    assert consumers.fuse_linear_consumers(model, uniform_weights=True) == 1
    assert consumers.fuse_linear_consumers(cpu_model, uniform_weights=True) == 1
    x = torch.randn(*batch, K) * 1.5
    y = model(x.cuda())
    assert " zp," in native.last_launch(), native.last_launch()
    assert y.is_cuda and y.shape == (*batch, N)
    assert torch.equal(y.cpu(), cpu_model(x))                         # its own CPU route, bit for bit
    check_against_oracle_and_float64(model[1], x.cuda().reshape(-1, K), y.reshape(-1, N))


@pytest.mark.gpu
def test_quantized_linear_routes_4bit_uniform_weights_by_batch_size():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = uniform_model(K=1024, N=256, bits=4).cuda()
    assert consumers.fuse_linear_consumers(model, uniform_weights=True) == 1
    ql = model[1]
    limit = consumers._W4_MAX_ROWS
    x = torch.randn(limit + 1, 1024, device="cuda") * 1.5
    y_small = model(x[:limit])
    assert "qlinear_stream_w4" in native.last_launch() and " zp," in native.last_launch(), native.last_launch()
    assert ql._w_codes4 is not None and ql._w_codes4.shape == (256, 512)
    assert int(ql._w_codes.min()) >= -8 and int(ql._w_codes.max()) <= 7
    y_big = model(x)
    assert "w4" not in native.last_launch() and " zp," in native.last_launch(), native.last_launch()
    assert torch.equal(y_small, y_big[:limit])                        # both routes compute the same integers
    check_against_oracle_and_float64(ql, x, y_big)


@pytest.mark.gpu
def test_pointwise_convolution_with_uniform_weights_on_gpu():
    from mct_quantizers_amd import consumers
    cpu_model, model = uniform_model(K=32, N=16, conv=True), uniform_model(K=32, N=16, conv=True).cuda()
    ref_model = uniform_model(K=32, N=16, conv=True).cuda()
    assert consumers.fuse_linear_consumers(model, uniform_weights=True) == 1
    assert consumers.fuse_linear_consumers(cpu_model, uniform_weights=True) == 1
    assert isinstance(model[1], consumers.QuantizedConv1x1)
    x = torch.randn(2, 32, 7, 5) * 1.5
    y, ref = model(x.cuda()), ref_model(x.cuda())
    assert y.shape == ref.shape == (2, 16, 7, 5)
    assert torch.equal(y.cpu(), cpu_model(x))
    assert torch.allclose(y, ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))


@pytest.mark.gpu
def test_chained_uniform_layer_emits_the_codes_of_the_float32_intermediate_gpu():
    check_chain("cuda")


@pytest.mark.gpu
def test_fused_uniform_linear_replays_in_a_hip_graph():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = uniform_model(K=1024, N=256).cuda()
    consumers.fuse_linear_consumers(model, uniform_weights=True)
    x = torch.randn(16, 1024, device="cuda")
    want = model(x)                                                   # (refreshes the weight codes outside the capture)
    assert " zp," in native.last_launch()
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):
        out = model(static_x)
    assert native.launch_count() - n0 >= 2                            # the row sums and the product are both in the graph
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(x * 0.5)) and not torch.equal(out, want)
