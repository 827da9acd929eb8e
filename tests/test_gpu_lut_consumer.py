"""mctq_qlinear_lut4a8 and the LUT-weights routes of consumers.QuantizedLinear on the GPU.

Oracle: oracle/mctq_oracle.py::qlinear_i8 on lut_i8[idx] (the exact integer product, scaled once); the kernel decodes the
packed 4-bit indices with byte lookups, so it must equal the oracle bit for bit for every shape, tail and codebook."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch
from test_lut_consumer import lut_model, lut_operands

LUT16 = [-120, 77, -2, 38, -96, 3, 127, -50, 11, -33, 100, -9, 24, -70, 55, -128]
LUT9 = [22, -53, 62, 0, -66, -21, 44, -40, 91]            # index 8 crosses the 8-entry boundary of the decode
LUT3 = [3, 3, -8]
SHAPES = [(16, 16), (100, 256), (33, 272), (64, 4096), (1000, 4112), (48, 11008)]
OUT = (0.07, 5, -128, 127)


def _check(M, N, K, u8, a, za, sa, idx, lut, ws, bias):
    from oracle import mctq_oracle as O
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    dev = torch.device("cuda")
    w = np.asarray(lut, np.int8)[idx]
    at, it, wst = (torch.from_numpy(v).to(dev) for v in (a, idx, ws))
    bt = None if bias is None else torch.from_numpy(bias).to(dev)
    rs = torch.from_numpy(w.astype(np.int32).sum(1, dtype=np.int32)).to(dev)
    packed = consumers.pack_lut4(it)
    got = consumers.qlinear_lut4a8(at, za, sa, packed, lut, wst, rs, bt)
    assert "qlinear_stream_lut4" in native.last_launch(), native.last_launch()
    want = O.qlinear_i8(a, za, sa, w, ws, bias)
    g = got.cpu().numpy()
    assert bits_equal(g, want), f"M={M} N={N} K={K} u8={u8} lut={len(lut)}: {first_mismatch(g, want)}"
    codes = consumers.qlinear_lut4a8(at, za, sa, packed, lut, wst, rs, bt, OUT)
    assert torch.equal(codes, ops.fq_codes(got, None, None, None, OUT[2], OUT[3], OUT[0], OUT[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64, 130])
def test_lut4a8_kernel_is_bit_exact_against_the_integer_oracle(M):
    rng = np.random.default_rng(1000 + M)
    for (N, K) in SHAPES:
        for u8 in (False, True):
            for lut in (LUT16, LUT9, LUT3):
                a = rng.integers(0, 256, (M, K)).astype(np.uint8) if u8 else rng.integers(-128, 128, (M, K)).astype(np.int8)
                za = int(rng.integers(0, 256)) if u8 else int(rng.integers(-128, 128))
                sa = float(rng.uniform(0.001, 0.1))
                ws = rng.uniform(0.001, 0.1, N).astype(np.float32)
                bias = rng.standard_normal(N).astype(np.float32) if (M + N) % 2 == 1 else None
                idx = rng.integers(0, len(lut), (N, K)).astype(np.uint8)
                _check(M, N, K, u8, a, za, sa, idx, lut, ws, bias)
    # every index 15; and the accumulator's worst case of this K: every index at -128 under all-255 activations
    N, K = SHAPES[-1]
    ws = rng.uniform(0.001, 0.1, N).astype(np.float32)
    a = rng.integers(0, 256, (M, K)).astype(np.uint8)
    _check(M, N, K, True, a, 114, 0.02, np.full((N, K), 15, np.uint8), LUT16, ws, None)
    a[:] = 255
    _check(M, N, K, True, a, 0, 0.02, np.full((N, K), 15, np.uint8), LUT16, ws, ws.copy())


@pytest.mark.gpu
def test_quantized_linear_routes_lut_weights_by_batch_size(monkeypatch):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = lut_model(k=1024, n=256, codebook="16").cuda()
    ref_model = lut_model(k=1024, n=256, codebook="16").cuda()
    assert consumers.fuse_linear_consumers(model) == 1
    ql = model[1]
    def run(batch, packed):
        x = torch.randn(batch, 1024, device="cuda") * 1.5
        ref = ref_model(x)
        y = model(x)
        launch = native.last_launch()
        assert ("qlinear_stream_lut4" in launch) == packed and launch.startswith("qlinear"), launch
        assert ql._w_idx4 is not None and ql._w_idx4.shape == (256, 512) and len(ql._lut16) == 16
        assert torch.allclose(y, ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))
    # the shipped limit is the measured crossover (profiles/EXPERIMENTS.md): batches up to it stream the packed indices
    limit = consumers._LUT4_MAX_ROWS
    assert 1 <= limit <= 32
    for batch in (1, limit, limit + 1, 200):
        run(batch, batch <= limit)
    # the routing itself, at the limit the kernel was written for (W4's 32): packed at batch 8, int8 at batch 200
    monkeypatch.setattr(consumers, "_LUT4_MAX_ROWS", 32)
    run(8, True)
    run(200, False)
    # the codes kept for the int8 route are the fake-quantized weight, bit for bit, on the GPU's own LUT kernels too
    w_codes, ws, _ = lut_operands(ql.weights_quantizer, ql.weight)
    assert np.array_equal(ql._w_codes.cpu().numpy(), w_codes) and bits_equal(ql._w_scales.cpu().numpy(), ws)
    wq = ref_model[1].weights_quantizers["weight"](ref_model[1].weight.detach().clone())
    assert bits_equal(w_codes.astype(np.float32) * ws[:, None], wq.cpu().numpy())
    # both routes compute the same integers: identical results for the same 32 rows
    x = torch.randn(32, 1024, device="cuda")
    monkeypatch.setattr(consumers, "_LUT4_MAX_ROWS", 32)
    y_packed = model(x)
    assert "qlinear_stream_lut4" in native.last_launch()
    monkeypatch.setattr(consumers, "_LUT4_MAX_ROWS", 0)
    y_int8 = model(x)
    assert "lut4" not in native.last_launch()
    assert torch.equal(y_packed, y_int8)
    # a 32-entry codebook fuses and has no packed layout
    big = lut_model(k=1024, n=256, codebook="32").cuda()
    big_ref = lut_model(k=1024, n=256, codebook="32").cuda()
    assert consumers.fuse_linear_consumers(big) == 1
    x = torch.randn(8, 1024, device="cuda") * 1.5
    ref = big_ref(x)
    y = big(x)
    assert big[1]._w_idx4 is None and "lut4" not in native.last_launch()
    assert torch.allclose(y, ref, rtol=1e-4, atol=1e-5 * float(ref.detach().abs().max()))


@pytest.mark.gpu
def test_fused_lut_linear_replays_in_a_hip_graph(monkeypatch):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native
    model = lut_model(k=1024, n=256, codebook="16").cuda()
    consumers.fuse_linear_consumers(model)
    monkeypatch.setattr(consumers, "_LUT4_MAX_ROWS", max(consumers._LUT4_MAX_ROWS, 1))
    x = torch.randn(1, 1024, device="cuda")                         # one row: the packed route, codebook in the launch's arguments
    want = model(x)
    assert "qlinear_stream_lut4" in native.last_launch()
    static_x = x.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        model(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model(static_x)
    static_x.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, model(x * 0.5)) and not torch.equal(out, want)


@pytest.mark.gpu
def test_chained_lut_layers_emit_the_codes_of_the_float32_intermediate(monkeypatch):
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import ops

    def stack():
        a = lut_model(k=256, n=128, codebook="16", seed=1, act="uniform")
        b = lut_model(k=128, n=64, codebook="8", kind="pot", seed=2, act="signed")
        return torch.nn.Sequential(a[0], a[1], b[0], b[1]).cuda()
    plain, chained = stack(), stack()
    assert consumers.fuse_linear_consumers(plain) == 2 and consumers.fuse_linear_consumers(chained, chain=True) == 2
    monkeypatch.setattr(consumers, "_LUT4_MAX_ROWS", 8)              # 1 and 7 rows: the packed route, whatever the shipped limit
    for batch in (1, 7, 200):                                        # packed route twice, int8 route
        x = torch.randn(batch, 256, device="cuda") * 1.5
        mid32, mid = plain[:2](x), chained[:2](x)
        nxt = chained[3]
        assert mid.dtype == torch.int8
        assert torch.equal(mid, ops.fq_codes(mid32, None, None, None, nxt._a_qmin, nxt._a_qmax, nxt._a_scale, nxt._a_zp))
        assert torch.equal(plain(x), chained(x))
