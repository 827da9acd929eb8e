"""mctq_qmatmul_i8, consumers.qmatmul_i8 and consumers.QuantizedMatmul on the GPU.

The kernel's sum is an exact integer and its epilogue rounds once per operation, so every comparison here is strict equality
with the CPU route of consumers.qmatmul_i8 (tests/test_matmul_consumer.py holds that route to a brute-force int64 einsum): no
tolerance exists or is needed.  The raw entry point writes into the middle of a sentinel-filled buffer and must leave the
sentinels alone."""
import itertools

import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_matmul_consumer import ALL_SWITCHES, OUT_FORMS, PAIRS, _block, rand_codes

GUARD, SENTINEL = 64, 0xA5
OP_NAMES = {(False, False): "i8 x i8", (True, False): "u8 x i8", (False, True): "i8 x u8", (True, True): "u8 x u8"}


def _zero_points(u8, nonzero):
    """A zero point whose z' (z - 128 for uint8 codes) is 0 -- the kernel then skips that correction's MFMA -- or is not."""
    return (131 if u8 else -7) if nonzero else (128 if u8 else 0)


def _operands(a_u8, b_u8, batch, M, N, K, transposed_b, seed):
    rng = np.random.default_rng(seed)
    a = rand_codes((*batch, M, K), a_u8, rng)
    b = rand_codes((*batch, N, K) if transposed_b else (*batch, K, N), b_u8, rng)
    return a, b


def _raw_into_guarded_buffer(a, fa, b, fb, transposed_b, out_codes):
    """The raw entry point on 4-D device operands (K-contiguous ones re-pitched where K % 16 != 0, as the Python route does), its
    output in the middle of a sentinel-filled buffer -> (output as a CPU tensor [B0, B1, M, N], launch name); the sentinels on
    both sides are checked here."""
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    lib = native.load()
    b0, b1, M, K = a.shape
    N = b.shape[-2 if transposed_b else -1]
    a4 = consumers._matmul_view(a.cuda(), fa[1], True)
    b4 = consumers._matmul_view(b.cuda(), fb[1], transposed_b)
    tdt, *form = consumers._output_form(out_codes)
    n = b0 * b1 * M * N * (4 if tdt == torch.float32 else 1)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    rc = lib.mctq_qmatmul_i8(a4.data_ptr(), ops._code_of(a4), fa[1], fa[0], *consumers._matmul_strides(a4),
                             b4.data_ptr(), ops._code_of(b4), fb[1], fb[0], *consumers._matmul_strides(b4), int(transposed_b),
                             buf.data_ptr() + GUARD, *form, b0, b1, M, N, K, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mctq_last_error()
    launch = native.last_launch()
    got = buf.cpu()
    assert bool((got[:GUARD] == SENTINEL).all()) and bool((got[GUARD + n:] == SENTINEL).all()), (a.shape, b.shape, transposed_b)
    return got[GUARD:GUARD + n].view(tdt).reshape(b0, b1, M, N), launch


def _check_raw(a, fa, b, fb, transposed_b, out_codes, what):
    from mct_quantizers_amd import consumers
    want = consumers.qmatmul_i8(a, fa, b, fb, transposed_b=transposed_b, out_codes=out_codes)           # the CPU route
    got, launch = _raw_into_guarded_buffer(a, fa, b, fb, transposed_b, out_codes)
    assert launch.startswith("qmatmul_nt<" if transposed_b else "qmatmul_nn<"), launch
    assert OP_NAMES[a.dtype == torch.uint8, b.dtype == torch.uint8] + "," in launch, launch
    za, zb = (z - (128 if t.dtype == torch.uint8 else 0) for z, t in ((fa[1], a), (fb[1], b)))
    assert f",U={(za != 0) + 2 * (zb != 0)}," in launch, launch            # which correction MFMAs ran
    assert f",out{4 if out_codes is None else 1}B," in launch, launch
    if out_codes is None:
        assert bits_equal(got.numpy(), want.numpy()), (what, first_mismatch(got.numpy(), want.numpy()))
    else:
        assert got.dtype == want.dtype and torch.equal(got, want), what
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_qmatmul_kernel_equals_the_cpu_route_and_stays_inside_its_output(a_u8, b_u8, transposed_b, codes_out):
    """M: one lane row, a ragged tile, a second block.  N: one tile, a ragged tile (NT), a second slice with a partial one.
    K: a partial 64-step, two steps, two whole steps; 17 and 197 through the re-pitch.  Both batch forms; every combination of
    the two correction flags."""
    Ms, Ns, Ks = (1, 17, 65), ((16, 17, 80) if transposed_b else (16, 80)), (16, 80, 128, 17, 197)
    flags = itertools.cycle(itertools.product((False, True), repeat=2))
    n = 0
    for i, (M, N, K, batch) in enumerate(itertools.product(Ms, Ns, Ks, ((1, 1), (2, 3)))):
        nz_a, nz_b = next(flags)
        fa, fb = (0.9, _zero_points(a_u8, nz_a)), (0.7, _zero_points(b_u8, nz_b))
        out_codes = None
        if codes_out:                                                      # a scale that spreads the sums over the codes
            out_codes = (0.63 * 128 * 64 * np.sqrt(K) / 100, *OUT_FORMS[i % 2 == 0][1:])
        a, b = _operands(a_u8, b_u8, batch, M, N, K, transposed_b, 100 + i)
        got = _check_raw(a, fa, b, fb, transposed_b, out_codes, (M, N, K, batch, fa, fb))
        if codes_out and M * N * batch[1] >= 256:
            assert len(got.unique()) >= 8
        n += 1
    assert n == len(Ms) * len(Ns) * len(Ks) * 2


@pytest.mark.gpu
@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
@pytest.mark.parametrize("a_u8,b_u8", PAIRS)
def test_qmatmul_kernel_edge_values(a_u8, b_u8, transposed_b):
    """All-extreme codes at K = 32768, M = N = 16: |acc| = 255 * 255 * 32768 in every element, both signs, float32 and codes;
    and codes equal to the zero point everywhere: an exact 0."""
    K = 32768
    ends = lambda u8: ((0, 255) if u8 else (-128, 127))                   # noqa: E731
    dt = lambda u8: torch.uint8 if u8 else torch.int8                      # noqa: E731
    (alo, ahi), (blo, bhi) = ends(a_u8), ends(b_u8)
    a = torch.full((1, 1, 16, K), ahi, dtype=dt(a_u8))
    b = torch.full((1, 1, 16, K) if transposed_b else (1, 1, K, 16), bhi, dtype=dt(b_u8))
    y = _check_raw(a, (1.0, alo), b, (1.0, blo), transposed_b, None, "largest")
    assert y.unique().tolist() == [float(np.float32(2130739200))]
    y = _check_raw(a, (1.0, alo), torch.full_like(b, blo), (1.0, bhi), transposed_b, None, "smallest")
    assert y.unique().tolist() == [float(np.float32(-2130739200))]
    codes = _check_raw(a, (1.0, alo), b, (1.0, blo), transposed_b, (float(2 ** 24), 0, -128, 127), "largest as codes")
    assert codes.unique().tolist() == [127]
    codes = _check_raw(a, (0.5, alo), torch.full_like(b, blo), (0.5, bhi), transposed_b, (float(2 ** 23), 200, 0, 255), "smallest as codes")
    assert codes.unique().tolist() == [200 - 64]                           # rint(-2130739200 / 4 / 2^23) = -64 (63.5 and a bit)
    # every code the zero point: the two corrections and the tail term cancel the product exactly
    for K0 in (16, 197, 4096):
        za, zb = (77 if a_u8 else -128), (255 if b_u8 else 55)
        az = torch.full((2, 1, 17, K0), za, dtype=dt(a_u8))
        bz = torch.full((2, 1, 32, K0) if transposed_b else (2, 1, K0, 32), zb, dtype=dt(b_u8))
        y = _check_raw(az, (0.3, za), bz, (0.2, zb), transposed_b, None, ("zero", K0))
        assert not y.view(torch.int32).any()                               # +0.0 in every element
        assert _check_raw(az, (0.3, za), bz, (0.2, zb), transposed_b, OUT_FORMS[True], ("zero", K0)).unique().tolist() == [114]


def _spy_on_launches(monkeypatch):
    """Records (a pointer, b pointer) of every mctq_qmatmul_i8 launch the Python route makes."""
    from mct_quantizers_amd.hip import ops
    seen, real = [], ops._gpu_call

    def spy(name, on, *args):
        if name == "mctq_qmatmul_i8":
            seen.append((args[0], args[7]))
        return real(name, on, *args)

    monkeypatch.setattr(ops, "_gpu_call", spy)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("codes_out", [False, True])
@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
def test_strided_views_reach_the_kernel_without_a_copy(transposed_b, codes_out, monkeypatch):
    """[2, 17, 3, 32] storage read as [2, 3, 17, 32] -- the permuted view every attention block makes -- for both operands; a
    stride-0 broadcast operand; a misaligned view, which is copied."""
    from mct_quantizers_amd import consumers
    rng = np.random.default_rng(9)
    fa, fb = (0.9, 131), (0.7, -7)
    out_codes = (600.0, 3, -128, 127) if codes_out else None
    a_store = rand_codes((2, 17, 3, 32), True, rng)
    b_store = rand_codes((2, 17, 3, 32) if transposed_b else (2, 32, 3, 48), False, rng)       # NT: [.., N = 17, K = 32]; NN: [.., K = 32, N = 48]
    seen = _spy_on_launches(monkeypatch)

    def run(a, b):
        got = consumers.qmatmul_i8(a.cuda() if not a.is_cuda else a, fa, b.cuda() if not b.is_cuda else b, fb,
                                   transposed_b=transposed_b, out_codes=out_codes)
        want = consumers.qmatmul_i8(a.cpu(), fa, b.cpu(), fb, transposed_b=transposed_b, out_codes=out_codes)
        assert got.is_cuda and got.is_contiguous() and got.dtype == want.dtype and got.shape == want.shape
        assert bits_equal(got.cpu().numpy(), want.numpy()) if out_codes is None else torch.equal(got.cpu(), want)
        return got

    a_dev, b_dev = a_store.cuda(), b_store.cuda()
    a, b = a_dev.permute(0, 2, 1, 3), b_dev.permute(0, 2, 1, 3)
    assert not a.is_contiguous() and not b.is_contiguous()
    run(a, b)
    assert seen == [(a_dev.data_ptr(), b_dev.data_ptr())]                  # the views themselves, not copies
    # one head of a fused qkv tensor: a view with an offset
    qkv = rand_codes((2, 17, 3, 2, 32), True, rng).cuda().permute(2, 0, 3, 1, 4)
    q = qkv[1]
    run(q, b[:, :2])
    assert seen[-1] == (q.data_ptr(), b_dev.data_ptr()) and q.data_ptr() == qkv.data_ptr() + 64
    # a stride-0 broadcast: one b for every batch and head, as a 2-D tensor and as an expanded one
    b2 = b_dev[0, :, 0]
    run(a, b2)
    assert seen[-1] == (a_dev.data_ptr(), b2.data_ptr())
    run(a, b2.expand(2, 3, *b2.shape))
    assert seen[-1] == (a_dev.data_ptr(), b2.data_ptr())
    run(a[:1].expand(2, -1, -1, -1), b)                                    # ... and a broadcast along B0 only
    assert seen[-1] == (a_dev.data_ptr(), b_dev.data_ptr())
    # 3-D operands (torch.bmm's): one batch dimension
    run(a[0], b[0])
    assert seen[-1] == (a_dev.data_ptr(), b_dev.data_ptr())
    # a misaligned view: Python makes it contiguous
    flat = torch.zeros(a_store.numel() + 16, dtype=torch.uint8, device="cuda")
    off = flat[1:1 + a_store.numel()].view(a_store.shape)
    off.copy_(a_dev)
    assert off.data_ptr() % 16 == 1
    run(off.permute(0, 2, 1, 3), b)
    assert seen[-1][0] != off.data_ptr() and seen[-1][0] % 16 == 0 and seen[-1][1] == b_dev.data_ptr()
    # a last dimension that is not contiguous (a transpose that was executed): copied as well
    odd = b.transpose(-1, -2).contiguous().transpose(-1, -2)               # b's values, its last dimension strided
    assert odd.shape == b.shape and odd.stride(-1) != 1
    run(a, odd)
    assert seen[-1][0] == a_dev.data_ptr() and seen[-1][1] != odd.data_ptr()
    assert len(seen) == 8


@pytest.mark.gpu
def test_cases_the_kernel_does_not_take_run_the_contract_with_torch_ops(monkeypatch):
    from mct_quantizers_amd import consumers
    rng = np.random.default_rng(4)
    seen = _spy_on_launches(monkeypatch)
    fa, fb = (0.9, 3), (0.7, 250)
    cases = [((5, 19), (7, 19), True), ((5, 19), (19, 7), False),          # 2-D operands
             ((2, 2, 2, 5, 32), (2, 2, 2, 7, 32), True),                   # three batch dimensions
             ((2, 5, 32), (2, 32, 24), False),                             # N % 16 != 0 in the NN form
             ((19,), (2, 19, 4), False), ((2, 5, 19), (19,), False)]       # 1-D operands
    for sa, sb, t in cases:
        a, b = rand_codes(sa, False, rng), rand_codes(sb, True, rng)
        for out_codes in (None, (40.0, 3, -128, 127)):
            got = consumers.qmatmul_i8(a.cuda(), fa, b.cuda(), fb, transposed_b=t, out_codes=out_codes)
            want = consumers.qmatmul_i8(a, fa, b, fb, transposed_b=t, out_codes=out_codes)
            assert got.is_cuda and got.shape == want.shape and got.dtype == want.dtype
            assert bits_equal(got.cpu().numpy(), want.numpy()) if out_codes is None else torch.equal(got.cpu(), want)
    assert seen == []
    # an empty product: no launch, an empty result
    y = consumers.qmatmul_i8(torch.zeros(2, 0, 16, dtype=torch.int8, device="cuda"), fa, torch.zeros(2, 5, 16, dtype=torch.uint8, device="cuda"),
                             fb, transposed_b=True)
    assert y.shape == (2, 0, 5) and seen == []


@pytest.mark.gpu
def test_a_batch_beyond_one_launch_is_split(monkeypatch):
    from mct_quantizers_amd import consumers
    monkeypatch.setattr(consumers, "_MATMUL_MAX_BATCH", 4)                 # the grid limit, lowered: 3 x 3 batches take three launches
    seen = _spy_on_launches(monkeypatch)
    rng = np.random.default_rng(6)
    a, b = rand_codes((3, 3, 5, 19), True, rng), rand_codes((3, 1, 7, 19), False, rng)
    for out_codes in (None, (40.0, 3, 0, 255)):
        got = consumers.qmatmul_i8(a.cuda(), (0.9, 3), b.cuda(), (0.7, -3), transposed_b=True, out_codes=out_codes)
        want = consumers.qmatmul_i8(a, (0.9, 3), b, (0.7, -3), transposed_b=True, out_codes=out_codes)
        assert torch.equal(got.cpu(), want)
    assert len(seen) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("transposed_b", [True, False], ids=["NT", "NN"])
def test_quantized_matmul_on_gpu_equals_its_cpu_route(transposed_b):
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    Q = mq.pytorch_quantizers
    qa = Q.ActivationUniformInferableQuantizer(8, [-3.1], [2.7])
    qb = Q.ActivationSymmetricInferableQuantizer(8, [3.0], True)
    qc = Q.ActivationUniformInferableQuantizer(8, [-40.0], [55.0])
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 70, 48, generator=gen) * 1.5
    y = torch.randn(2, 3, 80, 48, generator=gen) * 1.5
    if not transposed_b:
        y = y.transpose(-1, -2).contiguous()
    for out_q in (None, qc):
        m = consumers.QuantizedMatmul([qa, qb], out_q, transposed_b=transposed_b)
        want = m(x, y)
        got = m(x.cuda(), y.cuda())
        assert native.last_launch().startswith("qmatmul_nt<u8 x i8" if transposed_b else "qmatmul_nn<u8 x i8"), native.last_launch()
        assert got.is_cuda and got.dtype == want.dtype == (torch.float32 if out_q is None else torch.uint8)
        assert bits_equal(got.cpu().numpy(), want.numpy()) if out_q is None else torch.equal(got.cpu(), want)
        assert len(want.unique()) > 50
        # a permuted float32 operand: its codes keep its strides and go to the kernel as they are
        xs = x.permute(0, 2, 1, 3).contiguous().cuda().permute(0, 2, 1, 3)
        again = m(xs, y.cuda())
        assert torch.equal(again, got)


def _rewritten_pair(tokens, **kw):
    from mct_quantizers_amd import consumers
    cpu, n = consumers.fuse_linear_consumers_fx(_block(tokens=tokens, **kw), matmuls=True, **ALL_SWITCHES)
    gpu, n_gpu = consumers.fuse_linear_consumers_fx(_block(tokens=tokens, device="cuda", **kw), matmuls=True, **ALL_SWITCHES)
    assert n == n_gpu == (2 if kw.get("fused_qkv") else 4)
    return cpu, gpu


@pytest.mark.gpu
@pytest.mark.parametrize("uniform", [False, True], ids=["pot", "uniform"])
@pytest.mark.parametrize("tokens", [17, 197])
def test_rewritten_attention_block_on_gpu_equals_its_cpu_run(tokens, uniform):
    """heads = 2, batch 2, every switch: bit for bit.  tokens = 17 and 197 are both ragged K for the context product (one
    re-pitch launch); 197 rows are four blocks, the last with five rows."""
    from mct_quantizers_amd.hip import native
    cpu, gpu = _rewritten_pair(tokens, uniform=uniform)
    x = torch.randn(2, tokens, 64, generator=torch.Generator().manual_seed(tokens)) * 1.5
    want = cpu(x)
    n0 = native.launch_count()
    names = []
    for name in ("matmul_qmatmul", "matmul_1_qmatmul"):
        gpu.get_submodule(name).register_forward_hook(lambda m, args, out: names.append(native.last_launch()))
    y = gpu(x.cuda())
    assert names[0].startswith("qmatmul_nt<") and names[1].startswith("qmatmul_nn<"), names
    assert ",out4B," in names[0] and ",out1B," in names[1], names
    assert native.launch_count() > n0
    assert y.is_cuda and y.shape == want.shape == (2, tokens, 64)
    assert bits_equal(y.cpu().numpy(), want.detach().numpy()), first_mismatch(y.cpu().numpy(), want.detach().numpy())
    assert len(want.unique()) > 100


@pytest.mark.gpu
def test_rewritten_fused_qkv_block_on_gpu_equals_its_cpu_run():
    cpu, gpu = _rewritten_pair(17, fused_qkv=True, uniform=True)
    x = torch.randn(2, 17, 64, generator=torch.Generator().manual_seed(1)) * 1.5
    want, y = cpu(x), gpu(x.cuda())
    assert bits_equal(y.cpu().numpy(), want.detach().numpy()), first_mismatch(y.cpu().numpy(), want.detach().numpy())


@pytest.mark.gpu
def test_rewritten_attention_block_replays_in_a_hip_graph():
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model, _ = consumers.fuse_linear_consumers_fx(_block(device="cuda", uniform=True), matmuls=True, **ALL_SWITCHES)
    x = torch.randn(2, 17, 64, device="cuda") * 1.5
    want = model(x)                                                       # the warm-up forward: weight codes, outside the capture
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    n0 = native.launch_count()
    with torch.cuda.graph(g):
        out = model(static_x)
    assert native.launch_count() - n0 >= 6                                # the join, three products by weights, two by activations, ...
    other = torch.randn(2, 17, 64, device="cuda") * 1.5                    # (not x * 0.5: the block starts with a LayerNorm)
    static_x.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(other)) and not torch.equal(out, want)
