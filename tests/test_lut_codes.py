"""Codebook-index codes of the LUT quantizers and their decode, without a GPU: the fixture recorded from the reference
(tests/golden/lut_index_cases.*, tools/gen_golden_lut_index.py) against the oracle, the host-side index decision table,
the Python layers on CPU tensors, the C ABI's argument validation, and the decode kernels' compiled resources."""
import ctypes
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, bits_equal, first_mismatch


def _cases():
    with open(os.path.join(GOLDEN, "lut_index_cases.json")) as f:
        return json.load(f)


CASES = _cases()
IDS = [f"{c['id']}-{c['cls'][:12]}-{c['kwargs']['num_bits']}b-{c['kind']}-ax{c['axis']}" for c in CASES]


@pytest.fixture(scope="module")
def arrays():
    return np.load(os.path.join(GOLDEN, "lut_index_cases.npz"))


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import build, native
    build.build()                               # hipcc cross-compiles for gfx950 without a GPU
    return native.load()


def _make(case):
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(mq.pytorch_quantizers, case["cls"])(**case["kwargs"])


def _oracle(case, x):
    from oracle import mctq_oracle as O
    kw = case["kwargs"]
    if case["cls"].startswith("Activation"):
        return O.lut_quantize(x, kw["lut_values"], float(kw["threshold"][0]), kw["signed"], kw["lut_values_bitwidth"], kw["eps"],
                              return_index=True)
    return O.lut_quantize(x, kw["lut_values"], np.asarray(kw["threshold"], np.float32), True, kw["lut_values_bitwidth"],
                          kw["eps"], per_channel=kw["per_channel"], channel_axis=kw["channel_axis"], return_index=True)


# ---- 1. fixture vs oracle ------------------------------------------------------------------------------------------

def test_fixture_covers_what_it_should(arrays):
    assert len(CASES) >= 40
    assert {c["kwargs"]["num_bits"] for c in CASES} == {2, 3, 4, 8}
    assert {c["axis"] for c in CASES} == {None, 0, 1, 2}
    assert {c["kind"] for c in CASES} == {"sorted", "shuffled", "dup"}
    assert {c["cls"] for c in CASES} == {"WeightsLUTSymmetricInferableQuantizer", "WeightsLUTPOTInferableQuantizer",
                                         "ActivationLutPOTInferableQuantizer"}
    x = np.concatenate([arrays[c["id"] + "_x"].reshape(-1) for c in CASES])
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert (x == 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    dup = [c for c in CASES if c["kind"] == "dup"]
    assert all(len(set(c["kwargs"]["lut_values"])) < len(c["kwargs"]["lut_values"]) for c in dup)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_reproduces_the_reference_indices_and_outputs(case, arrays):
    x, y, idx = (arrays[case["id"] + s] for s in ("_x", "_y", "_idx"))
    got_y, got_idx = _oracle(case, x)
    assert np.array_equal(got_idx, idx.astype(np.int64))
    assert bits_equal(got_y, y), first_mismatch(got_y, y, x)
    # the contract's decode: two float32 operations on the indexed centre
    kw = case["kwargs"]
    mult = np.float32(2.0 ** (kw["lut_values_bitwidth"] - int(case["signed"])))
    thr = np.asarray(kw["threshold"], np.float32)
    thr = thr[0] if case["axis"] is None else thr.reshape([-1 if d == case["axis"] else 1 for d in range(x.ndim)])
    assert bits_equal((np.asarray(kw["lut_values"], np.float32)[idx] / mult) * thr, y)


# ---- 2. the host-side index decision table ---------------------------------------------------------------------------

def test_index_table_builder_matches_the_oracle_scan(lib):
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(0)
    luts = [[-5.0, 5.0], [3.0, 3.0, -8.0], [22.0, -53.0, 62.0, 0.0, -66.0, -21.0, 44.0, -40.0],
            [float(v) for v in rng.permutation(np.arange(-128, 128))], [7.0], [-1.0, 0.0, 1.0, 2.0, 3.0]]
    for lut in luts:
        val = native.build_lut_table(lut, 128.0, -128.0, 127.0)
        tab = native.build_lut_index_table(lut, 128.0, -128.0, 127.0)
        assert tab is not None and tab.shape == (512, 2)
        # one bisection, two payloads: the thresholds are the value table's, bit for bit
        assert np.array_equal(tab[:511, 0].view(np.uint32), val[:511, 0].view(np.uint32))
        k = rng.integers(-256, 255, size=100000).astype(np.float32) * np.float32(0.5)
        off = rng.integers(-40, 41, size=k.size).astype(np.int64)
        b = k.view(np.int32).astype(np.int64)
        b = np.where(k > 0, b + off, np.where(k < 0, b - off, b))          # walk +-40 ulps around each point
        t = np.concatenate([b.astype(np.int32).view(np.float32), rng.uniform(-128, 127, 50000).astype(np.float32)])
        t = np.clip(t, -128, 127).astype(np.float32)
        _, want = O.lut_quantize(t, lut, np.asarray([128.0], np.float32), True, 8, 0.0, return_index=True)   # t == x
        e = tab[(t * np.float32(2) + np.float32(256.5)).astype(np.int32)]
        pair = np.ascontiguousarray(e[:, 1]).view(np.uint32)
        got = np.where(t >= e[:, 0], pair >> 16, pair & 0xffff).astype(np.int64)
        assert np.array_equal(got, want), lut[:8]
        # every index is the FIRST occurrence of its centre
        assert all(lut.index(lut[j]) == j for j in np.unique(got))
        assert tab[511].view(np.uint32)[0] == 0 and tab[511, 1] == np.float32(511)     # NaN input -> index 0; K
    # refusals: the value table's
    for args in (([0.5, 1.0], 128.0, -128.0, 127.0), ([1.0], 2.0 ** 12, -2048.0, 2047.0), ([1.0], 3.0, -128.0, 127.0)):
        assert native.build_lut_table(*args) is None and native.build_lut_index_table(*args) is None
    assert lib.mctq_lut_build_index_table(None, 4, 128.0, -128.0, 127.0, None) == native.MCTQ_E_ARG


# ---- 3. the Python layers on CPU tensors ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_classes_on_cpu_tensors_equal_the_fixture(case, arrays):
    from mct_quantizers_amd.hip import ops
    x, y, idx = (arrays[case["id"] + s] for s in ("_x", "_y", "_idx"))
    q = _make(case)
    xt = torch.from_numpy(x.copy())
    codes, lut, thr = q.quantize_to_codes(xt)
    assert codes.dtype == torch.uint8 and codes.shape == xt.shape
    assert np.array_equal(codes.numpy(), idx)
    assert lut.dtype == torch.float32 and lut.tolist() == case["kwargs"]["lut_values"]
    assert thr.dtype == torch.float32 and np.array_equal(thr.numpy(), np.asarray(case["kwargs"]["threshold"], np.float32))
    out = q.dequantize_codes(codes)
    assert out.dtype == torch.float32 and bits_equal(out.numpy(), y), first_mismatch(out.numpy(), y, x)
    assert bits_equal(q(xt).numpy(), y)                                   # and both equal the fake-quantized tensor
    if len(case["kwargs"]["lut_values"]) <= 16:
        packed, _, _ = q.quantize_to_codes(xt, packed4=True)
        assert packed.dtype == torch.uint8 and packed.numel() * 2 == xt.numel()
        assert packed.shape == xt.shape[:-1] + (xt.shape[-1] // 2,)
        assert np.array_equal(ops.unpack4(packed, False, xt.shape).numpy().astype(np.uint8), idx)
        assert bits_equal(q.dequantize_codes(packed, shape=xt.shape).numpy(), y)
    else:
        with pytest.raises(ValueError):
            q.quantize_to_codes(xt, packed4=True)


def test_permuted_input_reassignment_and_errors(arrays):
    from mct_quantizers_amd.hip import ops
    import mct_quantizers_amd as mq
    Q = mq.pytorch_quantizers
    rng = np.random.default_rng(3)
    lut = [3.0, 3.0, -8.0, 0.0, 5.0, -2.0, 77.0, 1.0, -100.0, 127.0, -128.0, 40.0]
    thr = [0.5, 1.3, 2.0, 0.11]
    q = Q.WeightsLUTSymmetricInferableQuantizer(num_bits=4, lut_values=lut, threshold=thr, per_channel=True, channel_axis=1,
                                                input_rank=4)
    x = torch.from_numpy((rng.standard_normal((2, 4, 6, 8)) * 0.8).astype(np.float32))
    xcl = x.contiguous(memory_format=torch.channels_last)                 # dense, permuted storage
    codes, _, _ = q.quantize_to_codes(xcl)
    assert torch.equal(codes, q.quantize_to_codes(x)[0])
    assert bits_equal(q.dequantize_codes(codes).numpy(), q(x).numpy())
    packed, _, _ = q.quantize_to_codes(xcl, packed4=True)                 # packed in the contiguous order
    assert torch.equal(packed, q.quantize_to_codes(x, packed4=True)[0])
    assert bits_equal(q.dequantize_codes(packed, shape=x.shape).numpy(), q(x).numpy())
    # ops level: a dense permuted tensor is packed in STORAGE order, as fq_codes does
    p_ops = ops.lut_codes(xcl, torch.tensor(lut), torch.tensor(thr), 1, 1e-8, 0.0, 128.0, -128.0, 127.0, None, True)
    storage = torch.as_strided(codes.contiguous(memory_format=torch.channels_last), (x.numel(),), (1,))
    assert torch.equal(p_ops.reshape(-1), ops.pack4(storage))
    # attribute reassignment takes effect (the existing _stale / _resync path)
    before = q(x).clone()
    q._threshold_torch = torch.tensor([1.0, 1.0, 4.0, 0.25])
    codes2, _, thr2 = q.quantize_to_codes(x)
    assert thr2.tolist() == [1.0, 1.0, 4.0, 0.25] and not torch.equal(codes2, codes)
    assert bits_equal(q.dequantize_codes(codes2).numpy(), q(x).numpy()) and not torch.equal(q(x), before)
    q._lut_values_torch = torch.tensor([1.0, -1.0, 64.0, -64.0])
    codes3, lut3, _ = q.quantize_to_codes(x)
    assert lut3.tolist() == [1.0, -1.0, 64.0, -64.0] and int(codes3.max()) <= 3
    assert bits_equal(q.dequantize_codes(codes3).numpy(), q(x).numpy())
    a = Q.ActivationLutPOTInferableQuantizer(num_bits=2, lut_values=[0.0, 3.0, 9.0, 200.0], threshold=[4.0], signed=False)
    xa = x.abs()
    ca, _, ta = a.quantize_to_codes(xa)
    assert ta.tolist() == [4.0] and bits_equal(a.dequantize_codes(ca).numpy(), a(xa).numpy())
    a.threshold = 8.0
    cb, _, tb = a.quantize_to_codes(xa)
    assert tb.tolist() == [8.0] and bits_equal(a.dequantize_codes(cb).numpy(), a(xa).numpy())
    # errors
    with pytest.raises(NotImplementedError):
        q.quantize_to_codes(x.double())
    with pytest.raises(NotImplementedError):
        a.quantize_to_codes(xa.half())
    with pytest.raises(NotImplementedError):
        ops.lut_codes(x.double(), torch.tensor(lut), None, None, 0.0, 1.0, 128.0, -128.0, 127.0)
    with pytest.raises(ValueError):
        q.dequantize_codes(codes3.to(torch.int8))                          # dtype
    with pytest.raises(ValueError):
        q.dequantize_codes(codes3, shape=(2, 4, 6, 7))                     # size does not fit the shape
    with pytest.raises(ValueError):
        ops.lut_decode(codes3, torch.tensor(lut), None, None, 1.0, 128.0, True, (2, 4, 6, 8))   # not half the bytes
    wide = Q.WeightsLUTSymmetricInferableQuantizer(num_bits=5, lut_values=[float(v) for v in range(-16, 16)], threshold=[1.0],
                                                   per_channel=False)
    with pytest.raises(ValueError):
        wide.quantize_to_codes(x, packed4=True)                            # more than 16 entries
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        huge = Q.WeightsLUTSymmetricInferableQuantizer(num_bits=9, lut_values=[float(v) for v in range(-256, 256)],
                                                       threshold=[1.0], per_channel=False, lut_values_bitwidth=10)
    with pytest.raises(ValueError):
        huge.quantize_to_codes(x)                                          # more than 256 entries
    with pytest.raises(RuntimeError):
        q.quantize_to_codes(x[0])                                          # rank


# ---- 4. the C ABI without a GPU ---------------------------------------------------------------------------------------

def test_abi_symbols_version_and_argument_validation(lib):
    from mct_quantizers_amd.hip import native
    E = native.MCTQ_E_ARG
    U8, U4, I8 = native.CODE_U8, native.CODE_U4, native.CODE_I8
    for name in ("mctq_lut_build_index_table", "mctq_lut_codes_per_tensor", "mctq_lut_codes_per_channel",
                 "mctq_lut_decode_per_tensor", "mctq_lut_decode_per_channel"):
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert lib.mctq_abi_version() == 10 == native.ABI_VERSION
    text = open(os.path.join(REPO, "include", "mctq_hip.h")).read()
    assert "#define MCTQ_ABI_VERSION 10" in text and "v10" in text
    P = 0x1000                      # an aligned non-NULL address: validation dereferences nothing
    enc_t = lib.mctq_lut_codes_per_tensor
    enc_c = lib.mctq_lut_codes_per_channel
    dec_t = lib.mctq_lut_decode_per_tensor
    dec_c = lib.mctq_lut_decode_per_channel

    def err(rc, msg):
        assert rc == E, rc
        assert msg in lib.mctq_last_error(), lib.mctq_last_error()

    # negative extents
    err(enc_t(P, P, -1, 0, U8, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"n < 0")
    err(enc_c(P, P, 1, -2, 3, 0, U8, P, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"negative extent")
    err(dec_t(P, P, -1, U8, P, 4, 128.0, 1.0, None), b"n < 0")
    err(dec_c(P, P, 1, 2, -3, U8, P, 4, 128.0, P, None), b"negative extent")
    # NULL pointers with n > 0
    err(enc_t(None, P, 8, 0, U8, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"NULL")
    err(enc_c(P, P, 1, 2, 8, 0, U8, None, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"NULL")
    err(enc_t(P, P, 8, 0, U8, 0, 1.0, None, 4, None, 0, 128.0, -128.0, 127.0, None), b"lut is NULL")
    err(dec_t(P, None, 8, U8, P, 4, 128.0, 1.0, None), b"NULL")
    err(dec_c(P, P, 1, 2, 8, U8, P, 4, 128.0, None, None), b"NULL")
    err(dec_t(P, P, 8, U8, None, 4, 128.0, 1.0, None), b"lut is NULL")
    # n_lut out of range for the code type; unknown code types; mult
    err(enc_t(P, P, 8, 0, U8, 0, 1.0, P, 257, None, 0, 128.0, -128.0, 127.0, None), b"256")
    err(enc_t(P, P, 8, 0, U4, 0, 1.0, P, 17, None, 0, 128.0, -128.0, 127.0, None), b"16")
    err(enc_t(P, P, 8, 0, U8, 0, 1.0, P, 0, None, 0, 128.0, -128.0, 127.0, None), b"n_lut")
    err(dec_t(P, P, 8, U8, P, 257, 128.0, 1.0, None), b"256")
    err(dec_c(P, P, 1, 2, 8, U4, P, 17, 128.0, P, None), b"16")
    err(enc_t(P, P, 8, 0, I8, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"MCTQ_CODE_U8")
    err(dec_t(P, P, 8, I8, P, 4, 128.0, 1.0, None), b"MCTQ_CODE_U8")
    err(enc_t(P, P, 8, 0, U8, 0, 1.0, P, 4, None, 0, 100.0, -128.0, 127.0, None), b"power of two")
    err(dec_t(P, P, 8, U8, P, 4, 100.0, 1.0, None), b"power of two")
    err(enc_t(P, P, 8, 0, U8, 7, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"step_round")
    err(enc_t(P, P, 8, 9, U8, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"dtype")
    err(enc_t(P, P, 8, 0, U8, 0, 1.0, P, 4, P, 17, 128.0, -128.0, 127.0, None), b"entries")      # table of another clip range
    # U4 layout rules
    err(enc_t(P, P, 12, 0, U4, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"multiple of 8")
    err(dec_t(P, P, 12, U4, P, 4, 128.0, 1.0, None), b"multiple of 8")
    err(enc_c(P, P, 2, 3, 12, 0, U4, P, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"inner % 8")
    err(enc_c(P, P, 2, 12, 1, 0, U4, P, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"channels % 8")
    err(dec_c(P, P, 2, 3, 12, U4, P, 4, 128.0, P, None), b"inner % 8")
    err(dec_c(P, P, 2, 12, 1, U4, P, 4, 128.0, P, None), b"channels % 8")
    err(enc_t(P + 4, P, 16, 0, U4, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None), b"aligned")
    err(dec_t(P + 2, P, 16, U4, P, 4, 128.0, 1.0, None), b"aligned")
    # the documented size limit
    err(dec_t(P, P, (1 << 32) - 8191, U8, P, 4, 128.0, 1.0, None), b"2^32 - 8192")
    err(dec_c(P, P, 1 << 20, 1 << 12, 3, U8, P, 4, 128.0, P, None), b"2^32 - 8192")
    # empty tensors launch nothing
    count = lib.mctq_launch_count()
    assert enc_t(None, None, 0, 0, U8, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None) == 0
    assert enc_t(None, None, 0, 0, U4, 0, 1.0, P, 4, None, 0, 128.0, -128.0, 127.0, None) == 0
    assert enc_c(None, None, 0, 4, 8, 0, U8, None, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None) == 0
    assert enc_c(None, None, 3, 4, 0, 0, U4, None, 1e-8, P, 4, None, 0, 128.0, -128.0, 127.0, None) == 0
    assert dec_t(None, None, 0, U8, P, 4, 128.0, 1.0, None) == 0
    assert dec_t(None, None, 0, U4, P, 4, 128.0, 1.0, None) == 0
    assert dec_c(None, None, 0, 4, 8, U8, P, 4, 128.0, None, None) == 0
    assert dec_c(None, None, 3, 0, 8, U4, P, 4, 128.0, None, None) == 0
    assert lib.mctq_launch_count() == count


# ---- 5. the decode kernels' compiled resources -----------------------------------------------------------------------

def test_decode_kernels_fit_64_vgprs_without_scratch_and_store_16_bytes(tmp_path):
    """The decode is narrow reads and wide writes: its access shape is a property of the compiled code.  From the code
    hipcc generates from the shipped source with the shipped flags: every decode kernel uses at most 64 VGPRs and no
    scratch, and the vector kernels write through global_store_dwordx4 -- one per 4 codes -- with at most the single
    element store of the n % 4 tail (flat uint8 kernels only)."""
    import shutil
    import subprocess
    from mct_quantizers_amd.hip import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build the library at all"
    asm = tmp_path / "decode.s"
    subprocess.run([hipcc, *B.FLAGS, "-I", os.path.join(REPO, "include"), "-I", B.CSRC, "--cuda-device-only", "-S", "-o", str(asm),
                    os.path.join(B.CSRC, "mctq_lut_decode.hip")], check=True, capture_output=True)
    text = asm.read_text()
    names = re.findall(r"^(_ZN4mctq\d+lut_decode\w+):", text, flags=re.M)
    flat = [n for n in names if "17lut_decode_kernel" in n]
    rows = [n for n in names if "22lut_decode_rows_kernel" in n]
    scalar = [n for n in names if "24lut_decode_scalar_kernel" in n]
    assert len(flat) == 7 and len(rows) == 6 and len(scalar) == 1, names     # u8 x 4 modes + u4 x 3; {u8, u4} x U {1, 2, 4}
    for name in names:
        start = text.index(name + ":")
        body = text[start:text.index(".Lfunc_end", start)]                 # (cold blocks may follow the first s_endpgm)
        report = text[start:text.index("; ScratchSize:", start) + 40]      # the compiler's own report behind the kernel
        vgprs = int(re.search(r"; NumVgprs: (\d+)", report).group(1))
        scratch = int(re.search(r"; ScratchSize: (\d+)", report).group(1))
        assert report.count("; NumVgprs:") == 1, name
        assert vgprs <= 64 and scratch == 0, (name, vgprs, scratch)
        assert "scratch_" not in body and "buffer_store" not in body, name
        ins = [ln.split(";")[0].strip() for ln in body.splitlines()]
        stores = [ln.split()[0] for ln in ins if ln.startswith("global_store")]
        if name in scalar:
            assert set(stores) == {"global_store_dword"}, (name, stores)
            continue
        wide = [s for s in stores if s == "global_store_dwordx4"]
        other = [s for s in stores if s != "global_store_dwordx4"]
        assert wide, name
        u8_flat = name in flat and "ILi4E" in name
        assert other == (["global_store_dword"] if u8_flat else []), (name, other)
        # a lane reads ONE 32-bit word of codes per store group (wider loads, if any, fetch per-lane thresholds)
        assert sum(ln.split()[0] == "global_load_dword" for ln in ins if ln.startswith("global_load")) >= 1, name
