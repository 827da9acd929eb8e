"""GPU: the one launch function of the ctypes route (``ops._gpu_call``) -- a refused launch names the exported symbol that
refused it, and each entry point enqueues exactly one launch with the right answer."""
import numpy as np
import pytest
import torch

from conftest import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctypes_ops(monkeypatch):
    """``ops`` with the compiled binding switched off, and ``native`` (loaded)."""
    from mct_quantizers_amd.hip import native, ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    native.load()
    monkeypatch.setattr(ops, "_FAST", None)
    monkeypatch.setattr(ops, "_FAST_READY", True)
    return ops, native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _one_launch(native, f):
    before = native.launch_count()
    out = f()
    assert native.launch_count() - before == 1
    return out


def test_refused_launches_name_their_symbol(ctypes_ops):
    ops, native = ctypes_ops
    x = torch.randn(6, 12, device="cuda")
    s = torch.ones(6, device="cuda")
    z = torch.zeros(6, dtype=torch.int32, device="cuda")
    before = native.launch_count()
    with pytest.raises(RuntimeError, match="mctq_fq_codes_per_channel failed"):
        ops.fq_codes(x, s, z, 0, -8, 7, packed4=True)                      # inner = 12: not a multiple of 8
    with pytest.raises(RuntimeError, match="mctq_fq_codes_per_tensor failed"):
        ops.fq_codes(torch.randn(70, device="cuda"), None, None, None, 0, 15, 0.1, 0, packed4=True)      # even, no multiple of 8
    assert native.launch_count() == before


def test_affine_calls_launch_once_and_match_the_oracle(ctypes_ops):
    ops, native = ctypes_ops
    from oracle import mctq_oracle as O
    rng = np.random.default_rng(5)
    x_np = (rng.standard_normal((7,)) * 2).astype(np.float32)
    x = _dev(x_np)
    got = _one_launch(native, lambda: ops.fq_per_tensor(x, 0.0219, 114, 0, 255)).cpu().numpy()
    want = O.fake_quant_affine(x_np, [0.0219], [114], 0, 255)
    assert bits_equal(got, want), first_mismatch(got, want, x_np)
    x_np = (rng.standard_normal((3, 5)) * 2).astype(np.float32)
    x = _dev(x_np)
    for axis in (0, 1):
        C = x_np.shape[axis]
        s = rng.uniform(0.01, 0.1, size=C).astype(np.float32)
        z = rng.integers(-3, 4, size=C).astype(np.int32)
        sd, zd = _dev(s), _dev(z)
        got = _one_launch(native, lambda: ops.fq_per_channel(x, sd, zd, axis, -128, 127)).cpu().numpy()
        want = O.fake_quant_affine(x_np, s, z, -128, 127, axis=axis)
        assert bits_equal(got, want), (axis, first_mismatch(got, want, x_np))


def test_code_calls_launch_once_and_match_their_cpu_routes(ctypes_ops):
    ops, native = ctypes_ops
    from mct_quantizers_amd import consumers
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 256, (1, 3, 3, 16), generator=g).to(torch.uint8)
    codes_d = codes.cuda()
    got = _one_launch(native, lambda: ops.codes_im2col(codes_d, 3, padding=1, pad_code=7))
    want = ops.codes_im2col(codes, 3, padding=1, pad_code=7)
    assert got.dtype == want.dtype and got.shape == want.shape == (9, 144) and torch.equal(got.cpu(), want)
    rows = torch.randint(0, 256, (2, 16), generator=g).to(torch.uint8)
    rows_d = rows.cuda()
    got = _one_launch(native, lambda: consumers.codes_rowsum(rows_d, 114))
    want = consumers.codes_rowsum(rows, 114)
    assert got.dtype == want.dtype == torch.int32 and torch.equal(got.cpu(), want)
