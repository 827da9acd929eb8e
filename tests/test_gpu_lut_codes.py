"""GPU parity of the LUT quantizers' codebook-index codes and their decode: the fixture recorded from the reference through
the classes, the C ABI against the oracle over the per-channel geometry list, all 2^32 float32 inputs (index table ==
literal scan, decode(encode(x)) == the fake-quant kernel), the wide-codebook literal route, graph capture, full size."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

LUTS = {
    "l3dup": [3.0, 3.0, -8.0],
    "l16": [-128.0, -96.0, -64.0, -40.0, -24.0, -12.0, -5.0, 0.0, 5.0, 12.0, 24.0, 40.0, 64.0, 96.0, 120.0, 127.0],
    "l256": [float(v) for v in np.random.default_rng(6).permutation(np.arange(-128, 128))],
    # the every-float sweeps: a signed 8-bit codebook with duplicates (shuffled), and 16 entries
    "l64dup": [float(v) for v in np.random.default_rng(9).choice(np.arange(-128, 128), 40, replace=False)] +
              [float(v) for v in np.random.default_rng(9).choice(np.arange(-128, 128), 40, replace=False)[5:29]],
}
GEOMETRY = [(1, 3, 1), (50, 3, 1), (4, 6, 5), (2, 8, 100), (2, 6, 1024), (3, 5, 1028), (1, 16, 11008), (1, 3000, 3),
            (1, 2, 70000), (41, 64, 1), (3, 4096, 1)]

with open(os.path.join(GOLDEN, "lut_index_cases.json")) as _f:
    CASES = json.load(_f)
IDS = [f"{c['id']}-{c['cls'][:12]}-{c['kwargs']['num_bits']}b-{c['kind']}-ax{c['axis']}" for c in CASES]


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


@pytest.fixture(scope="module")
def arrays():
    return np.load(os.path.join(GOLDEN, "lut_index_cases.npz"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _make(cls, kwargs):
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(mq.pytorch_quantizers, cls)(**kwargs)


def _index_table(lut, mult=128.0, cmin=-128.0, cmax=127.0):
    from mct_quantizers_amd.hip import native
    tab = native.build_lut_index_table(lut, mult, cmin, cmax)
    assert tab is not None
    return _dev(tab)


def _lut_inputs(rng, shape, thr_b):
    x = rng.standard_normal(int(np.prod(shape))).astype(np.float32).reshape(shape) * thr_b * np.float32(0.6)
    mid = (rng.integers(-130, 130, size=shape).astype(np.float32) + np.float32(0.5)) / np.float32(128.0) * thr_b
    x = np.where(rng.integers(0, 4, size=shape) == 0, mid, x).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:
        flat[:8] = np.asarray([0.0, -0.0, 1e-9, -1e-9, 1e-39, 3e5, -3e5, 1e30], dtype=np.float32)
    return x


# ---- 6. the fixture through the classes -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_classes_on_the_gpu_equal_the_reference(lib, arrays, case):
    from mct_quantizers_amd.hip import native, ops
    x, y, idx = (arrays[case["id"] + s] for s in ("_x", "_y", "_idx"))
    q = _make(case["cls"], case["kwargs"])
    xd = _dev(x)
    count = native.launch_count()
    codes, lut, thr = q.quantize_to_codes(xd)
    assert native.launch_count() == count + 1 and "LutIndexTableOp" in native.last_launch(), native.last_launch()
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.shape == xd.shape
    assert np.array_equal(codes.cpu().numpy(), idx)
    out = q.dequantize_codes(codes)
    assert native.launch_count() == count + 2 and "lut_decode" in native.last_launch(), native.last_launch()
    assert out.dtype == torch.float32 and bits_equal(out.cpu().numpy(), y), first_mismatch(out.cpu().numpy(), y, x)
    assert bits_equal(q(xd).cpu().numpy(), y)
    if len(case["kwargs"]["lut_values"]) <= 16:
        packed, _, _ = q.quantize_to_codes(xd, packed4=True)
        assert "lut_codes4" in native.last_launch(), native.last_launch()
        assert packed.shape == xd.shape[:-1] + (xd.shape[-1] // 2,)
        assert np.array_equal(ops.unpack4(packed.cpu(), False, x.shape).numpy().astype(np.uint8), idx)
        out4 = q.dequantize_codes(packed, shape=x.shape)
        assert "u4" in native.last_launch(), native.last_launch()
        assert bits_equal(out4.cpu().numpy(), y), first_mismatch(out4.cpu().numpy(), y, x)
    # a dense permuted input: codes keep its strides, the decode walks them in storage order
    if x.ndim == 3 and case["axis"] is not None:
        xp = xd.permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not xp.is_contiguous()
        cp, _, _ = q.quantize_to_codes(xp)
        assert cp.stride() == xp.stride() and np.array_equal(cp.cpu().numpy(), idx)
        assert bits_equal(q.dequantize_codes(cp).cpu().numpy(), y)


def test_attribute_assignment_reaches_the_codes(lib):
    rng = np.random.default_rng(12)
    q = _make("WeightsLUTSymmetricInferableQuantizer",
              dict(num_bits=3, lut_values=[3.0, 3.0, -8.0, 0.0, 5.0, -2.0, 77.0, 1.0], threshold=[0.5, 1.3, 2.0, 0.11],
                   per_channel=True, channel_axis=0, input_rank=2))
    x = _dev((rng.standard_normal((4, 512)) * 0.8).astype(np.float32))
    c0, _, _ = q.quantize_to_codes(x)
    q._threshold_torch = torch.tensor([1.0, 1.0, 4.0, 0.25], device="cuda")
    c1, _, thr = q.quantize_to_codes(x)
    assert thr.tolist() == [1.0, 1.0, 4.0, 0.25] and not torch.equal(c0, c1)
    assert torch.equal(q.dequantize_codes(c1).view(torch.int32), q(x).view(torch.int32))
    q._lut_values_torch = torch.tensor([1.0, -1.0, 64.0, -64.0], device="cuda")
    c2, lut, _ = q.quantize_to_codes(x)
    assert lut.tolist() == [1.0, -1.0, 64.0, -64.0] and int(c2.max()) <= 3
    assert torch.equal(q.dequantize_codes(c2).view(torch.int32), q(x).view(torch.int32))


# ---- 7. C ABI vs oracle over the per-channel geometry list -----------------------------------------------------------

@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("lut_name", ["l3dup", "l16", "l256"])
@pytest.mark.parametrize("outer,C,inner", GEOMETRY)
def test_abi_codes_and_decode_per_channel_vs_oracle(lib, lut_name, outer, C, inner, dt):
    from mct_quantizers_amd.hip import native, ops
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(C * 31 + inner + 1)
    lut = LUTS[lut_name]
    thr = rng.uniform(0.05, 4.0, size=C).astype(np.float32)
    shape = (outer, C, inner)
    xs = _dev(_lut_inputs(rng, shape, thr.reshape(1, C, 1))).to(getattr(torch, dt))
    x_np = xs.float().cpu().numpy()
    want_y, want_idx = O.lut_quantize(x_np, lut, thr, True, 8, 1e-8, per_channel=True, channel_axis=1, return_index=True)
    code = {"float32": native.DT_F32, "float16": native.DT_F16, "bfloat16": native.DT_BF16}[dt]
    t_d, lut_d, tab = _dev(thr), _dev(np.float32(lut)), _index_table(lut)
    u4_ok = len(lut) <= 16 and (inner % 8 == 0 or (inner == 1 and C % 8 == 0))
    for packed in ((False, True) if u4_ok else (False,)):
        n = outer * C * inner
        codes = torch.full((n // 2 if packed else n,), 0xEE, dtype=torch.uint8, device="cuda")
        cd = native.CODE_U4 if packed else native.CODE_U8
        rc = lib.mctq_lut_codes_per_channel(xs.data_ptr(), codes.data_ptr(), outer, C, inner, code, cd, t_d.data_ptr(), 1e-8,
                                            lut_d.data_ptr(), len(lut), tab.data_ptr(), tab.shape[0] - 1, 128.0, -128.0, 127.0,
                                            _stream())
        assert rc == 0, lib.mctq_last_error()
        launch = native.last_launch()
        assert "LutIndexTableOp" in launch and ("lut_codes4" in launch) == packed, launch
        got_idx = ops.unpack4(codes.cpu(), False).numpy().astype(np.int64) if packed else codes.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_idx.reshape(shape), want_idx), (launch, int((got_idx.reshape(shape) != want_idx).sum()))
        y = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.mctq_lut_decode_per_channel(codes.data_ptr(), y.data_ptr(), outer, C, inner, cd, lut_d.data_ptr(), len(lut),
                                             128.0, t_d.data_ptr(), _stream())
        assert rc == 0, lib.mctq_last_error()
        launch = native.last_launch()
        assert "lut_decode" in launch and "LutDecodeOp" in launch and ("u4" in launch) == packed, launch
        assert bits_equal(y.cpu().numpy(), want_y), (launch, first_mismatch(y.cpu().numpy(), want_y, x_np))


@pytest.mark.parametrize("n,offset", [(5, 0), (4096 + 3, 0), (100000, 1), (1 << 20, 0)])
def test_abi_codes_and_decode_per_tensor_vs_oracle(lib, n, offset):
    """Per tensor, incl. the n % 4 tail and codes / outputs that are not word / 16-byte aligned (the scalar decode)."""
    from mct_quantizers_amd.hip import native, ops
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(n)
    for lut_name in ("l3dup", "l16", "l256"):
        lut = LUTS[lut_name]
        thr = np.float32(1.7)
        x_np = _lut_inputs(rng, (n,), thr)
        x_np[-1] = np.nan
        want_y, want_idx = O.lut_quantize(x_np, lut, np.asarray([thr]), True, 8, 1e-8, return_index=True)
        xs = torch.empty(n + 4, dtype=torch.float32, device="cuda")[offset:offset + n].copy_(torch.from_numpy(x_np))
        lut_d, tab = _dev(np.float32(lut)), _index_table(lut)
        codes = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")[offset:offset + n]
        y = torch.empty(n + 4, dtype=torch.float32, device="cuda")[offset:offset + n]
        thr_div = float(thr + np.float32(1e-8))
        rc = lib.mctq_lut_codes_per_tensor(xs.data_ptr(), codes.data_ptr(), n, native.DT_F32, native.CODE_U8, 0, thr_div,
                                           lut_d.data_ptr(), len(lut), tab.data_ptr(), tab.shape[0] - 1, 128.0, -128.0, 127.0,
                                           _stream())
        assert rc == 0, lib.mctq_last_error()
        assert np.array_equal(codes.cpu().numpy().astype(np.int64), want_idx)
        rc = lib.mctq_lut_decode_per_tensor(codes.data_ptr(), y.data_ptr(), n, native.CODE_U8, lut_d.data_ptr(), len(lut), 128.0,
                                            float(thr), _stream())
        assert rc == 0, lib.mctq_last_error()
        assert ("scalar" in native.last_launch()) == bool(offset), native.last_launch()
        assert bits_equal(y.cpu().numpy(), want_y), first_mismatch(y.cpu().numpy(), want_y, x_np)
        if len(lut) <= 16 and n % 8 == 0 and not offset:
            c4 = torch.zeros(n // 2, dtype=torch.uint8, device="cuda")
            assert lib.mctq_lut_codes_per_tensor(xs.data_ptr(), c4.data_ptr(), n, native.DT_F32, native.CODE_U4, 0, thr_div,
                                                 lut_d.data_ptr(), len(lut), tab.data_ptr(), tab.shape[0] - 1, 128.0, -128.0,
                                                 127.0, _stream()) == 0
            assert torch.equal(c4, ops.pack4(codes))
            y.fill_(0)
            assert lib.mctq_lut_decode_per_tensor(c4.data_ptr(), y.data_ptr(), n, native.CODE_U4, lut_d.data_ptr(), len(lut),
                                                  128.0, float(thr), _stream()) == 0
            assert bits_equal(y.cpu().numpy(), want_y)


def test_half_activation_step_rounding_matches_the_oracle_index(lib):
    """step_round (half-precision activations): the index of the chain whose quotient and scaled value are rounded to the
    tensor's type, table route and literal route."""
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(41)
    lut = LUTS["l16"]
    lut_d, tab = _dev(np.float32(lut)), _index_table(lut)
    x32 = (rng.standard_normal(5 * 704) * 1.4).astype(np.float32)
    for dt, name, code in ((torch.float16, "float16", native.DT_F16), (torch.bfloat16, "bfloat16", native.DT_BF16)):
        x = torch.from_numpy(x32).to(dt).cuda()
        div = float(torch.tensor([2.0 + 1e-8], dtype=torch.float64).to(dt).item())
        _, want = O.lut_quantize(x.float().cpu().numpy(), lut, 2.0, True, 8, 1e-8, return_index=True, step_dtype=name)
        for table in (tab, None):
            codes = torch.empty(x.numel(), dtype=torch.uint8, device="cuda")
            rc = lib.mctq_lut_codes_per_tensor(x.data_ptr(), codes.data_ptr(), x.numel(), code, native.CODE_U8, code, div,
                                               lut_d.data_ptr(), len(lut), table.data_ptr() if table is not None else None,
                                               tab.shape[0] - 1 if table is not None else 0, 128.0, -128.0, 127.0, _stream())
            assert rc == 0, lib.mctq_last_error()
            assert np.array_equal(codes.cpu().numpy().astype(np.int64), want), (name, native.last_launch())


# ---- 8. every float32 input ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lut_name", ["l64dup", "l16"])
def test_codes_for_every_float(lib, lut_name):
    """All 2^32 float32 inputs: index-table encode == literal-scan encode, and decode(encode(x)) == the fake-quant kernel
    (mctq_lutt_per_tensor_f32) bit for bit; the 16-entry codebook also through the packed 4-bit codes."""
    from mct_quantizers_amd.hip import native, ops
    lut = LUTS[lut_name]
    assert lut_name != "l64dup" or len(set(lut)) < len(lut)
    lut_d, itab = _dev(np.asarray(lut, dtype=np.float32)), _index_table(lut)
    vtab = _dev(native.build_lut_table(lut, 128.0, -128.0, 127.0))
    chunk = 1 << 28
    c_lit = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    c_tab = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    c4 = torch.empty(chunk // 2, dtype=torch.uint8, device="cuda")
    y_fq = torch.empty(chunk, dtype=torch.float32, device="cuda")
    y_dec = torch.empty(chunk, dtype=torch.float32, device="cuda")
    U8, U4 = native.CODE_U8, native.CODE_U4
    for c in range(16):
        bits = torch.arange(c * chunk - (1 << 31), (c + 1) * chunk - (1 << 31), dtype=torch.int64, device="cuda")
        x = bits.to(torch.int32).view(torch.float32)
        del bits
        # thr_div = 1, mult = 128: t = clamp(x * 128) sweeps every float in the clip range
        assert lib.mctq_lut_codes_per_tensor(x.data_ptr(), c_lit.data_ptr(), chunk, 0, U8, 0, 1.0, lut_d.data_ptr(), len(lut),
                                             None, 0, 128.0, -128.0, 127.0, _stream()) == 0
        assert "LutIndexOp" in native.last_launch()
        assert lib.mctq_lut_codes_per_tensor(x.data_ptr(), c_tab.data_ptr(), chunk, 0, U8, 0, 1.0, lut_d.data_ptr(), len(lut),
                                             itab.data_ptr(), itab.shape[0] - 1, 128.0, -128.0, 127.0, _stream()) == 0
        if not torch.equal(c_lit, c_tab):
            i = int(torch.nonzero(c_lit != c_tab)[0])
            raise AssertionError(f"chunk {c}: x={x[i].item()!r} literal={c_lit[i].item()} table={c_tab[i].item()}")
        assert lib.mctq_lutt_per_tensor_f32(x.data_ptr(), y_fq.data_ptr(), chunk, 1.0, 1.0, vtab.data_ptr(), vtab.shape[0] - 1,
                                            128.0, -128.0, 127.0, _stream()) == 0
        assert lib.mctq_lut_decode_per_tensor(c_tab.data_ptr(), y_dec.data_ptr(), chunk, U8, lut_d.data_ptr(), len(lut), 128.0,
                                              1.0, _stream()) == 0
        if not torch.equal(y_fq.view(torch.int32), y_dec.view(torch.int32)):
            i = int(torch.nonzero(y_fq.view(torch.int32) != y_dec.view(torch.int32))[0])
            raise AssertionError(f"chunk {c}: x={x[i].item()!r} fake-quant={y_fq[i].item()!r} decode={y_dec[i].item()!r}")
        if len(lut) <= 16:
            assert lib.mctq_lut_codes_per_tensor(x.data_ptr(), c4.data_ptr(), chunk, 0, U4, 0, 1.0, lut_d.data_ptr(), len(lut),
                                                 itab.data_ptr(), itab.shape[0] - 1, 128.0, -128.0, 127.0, _stream()) == 0
            pairs = c_tab.view(chunk // 2, 2)
            assert torch.equal(c4, pairs[:, 0] | (pairs[:, 1] << 4)), f"chunk {c}: packed 4-bit codes"
            y_dec.fill_(0)
            assert lib.mctq_lut_decode_per_tensor(c4.data_ptr(), y_dec.data_ptr(), chunk, U4, lut_d.data_ptr(), len(lut), 128.0,
                                                  1.0, _stream()) == 0
            assert torch.equal(y_fq.view(torch.int32), y_dec.view(torch.int32)), f"chunk {c}: 4-bit decode"
        del x


# ---- 9. wide codebook: no table, the literal index scan --------------------------------------------------------------

def test_wide_codebook_takes_the_literal_index_route(lib):
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(77)
    lut = [float(v) for v in rng.choice(np.arange(-2048, 2048), 16, replace=False)]
    thr = rng.uniform(0.3, 3.0, size=6).astype(np.float32)
    kwargs = dict(num_bits=4, lut_values=lut, threshold=[float(t) for t in thr], per_channel=True, channel_axis=0, input_rank=2,
                  lut_values_bitwidth=12)
    q = _make("WeightsLUTSymmetricInferableQuantizer", kwargs)
    assert q._lut_index_table_torch is None
    x_np = (rng.standard_normal((6, 4104)) * thr.reshape(6, 1) * 0.7).astype(np.float32)
    x_np[:, :64] = ((rng.integers(-2050, 2050, size=(6, 64)) + 0.5) / 2048.0 * thr.reshape(6, 1)).astype(np.float32)
    x_np[0, 100] = np.nan
    want_y, want_idx = O.lut_quantize(x_np, lut, thr, True, 12, 1e-8, per_channel=True, channel_axis=0, return_index=True)
    x = _dev(x_np)
    for packed in (False, True):
        codes, _, _ = q.quantize_to_codes(x, packed4=packed)
        assert "LutIndexOp" in native.last_launch(), native.last_launch()
        from mct_quantizers_amd.hip import ops
        got = ops.unpack4(codes.cpu(), False, x_np.shape).numpy() if packed else codes.cpu().numpy()
        assert np.array_equal(got.astype(np.int64), want_idx)
        out = q.dequantize_codes(codes, shape=x_np.shape)
        assert bits_equal(out.cpu().numpy(), want_y), first_mismatch(out.cpu().numpy(), want_y, x_np)
        assert bits_equal(out.cpu().numpy(), q(x).cpu().numpy())


# ---- 10. graph capture --------------------------------------------------------------------------------------------------

def test_encode_and_decode_replay_under_a_captured_graph(lib):
    rng = np.random.default_rng(5)
    thr = [float(t) for t in rng.uniform(0.2, 3.0, size=64)]
    q = _make("WeightsLUTSymmetricInferableQuantizer",
              dict(num_bits=4, lut_values=LUTS["l16"], threshold=thr, per_channel=True, channel_axis=0, input_rank=2))
    x = torch.randn(64, 2048, device="cuda")
    q.quantize_to_codes(x), q.quantize_to_codes(x, packed4=True)            # warm: tables, module load
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        q.dequantize_codes(q.quantize_to_codes(x)[0])
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        codes = q.quantize_to_codes(x)[0]
        out = q.dequantize_codes(codes)
        codes4 = q.quantize_to_codes(x, packed4=True)[0]
        out4 = q.dequantize_codes(codes4, shape=x.shape)
    for seed in (1, 2):
        x.copy_(torch.randn(64, 2048, device="cuda", generator=torch.Generator("cuda").manual_seed(seed)) * 1.3)
        g.replay()
        torch.cuda.synchronize()
        want_codes = q.quantize_to_codes(x)[0]
        want = q(x)
        assert torch.equal(codes, want_codes) and torch.equal(codes4, q.quantize_to_codes(x, packed4=True)[0])
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        assert torch.equal(out4.view(torch.int32), want.view(torch.int32))


# ---- 11. full size ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1])
def test_full_size_per_channel_round_trip(lib, axis):
    from mct_quantizers_amd.hip import native
    rng = np.random.default_rng(axis)
    thr = [float(t) for t in rng.uniform(0.2, 3.0, size=4096)]
    q = _make("WeightsLUTSymmetricInferableQuantizer",
              dict(num_bits=4, lut_values=LUTS["l16"], threshold=thr, per_channel=True, channel_axis=axis, input_rank=2))
    x = torch.randn(4096, 4096, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    want = q(x)
    codes, _, _ = q.quantize_to_codes(x)
    out = q.dequantize_codes(codes)
    assert ("rows" in native.last_launch()) == (axis == 0), native.last_launch()
    assert torch.equal(out, want) and torch.equal(out.view(torch.int32), want.view(torch.int32))
    packed, _, _ = q.quantize_to_codes(x, packed4=True)
    assert packed.shape == (4096, 2048)
    pairs = codes.view(-1, 2)
    assert torch.equal(packed.view(-1), pairs[:, 0] | (pairs[:, 1] << 4))
    out4 = q.dequantize_codes(packed, shape=x.shape)
    assert torch.equal(out4, want) and torch.equal(out4.view(torch.int32), want.view(torch.int32))
