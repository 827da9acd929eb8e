"""The 8-bit code kernels on every launch route and at edge values: mctq_fq_codes_per_tensor / mctq_fq_codes_per_channel with
MCTQ_CODE_I8 / MCTQ_CODE_U8 (AffineCodesOp on the shared launchers of csrc/mctq_kernels.hpp with a 1-byte output: flat_kernel,
flat_scalar_kernel, rows_kernel, lastaxis_kernel<ZP>, window_kernel<vector | scalar>) and mctq_fq_codes_nchw_to_nhwc
(csrc/mctq_codes_nhwc.hip), through the raw C ABI.

Expected values: oracle.mctq_oracle.fake_quant_affine(..., return_index=True) on the values as stored, widened to float32.  A NaN
input has the code qmin (the CPU route's nan_to_num(nan=qmin)): the oracle's numpy maximum would propagate the NaN, so
qmin is substituted there.  +-inf and huge finite values go through the oracle's float arithmetic unchanged -- its clamp answers
them.  Bar: equality byte for byte on EVERY element: no mask, no tolerance.  Raw calls write into the middle of a frame of 0xA5
bytes, 64 guard bytes on each side, which must keep their value; inside the frame each output byte starts as the complement of
its expected value, so an unwritten byte shows.  Every successful call must advance mctq_launch_count by exactly one and leave the
launch note the case names.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5
DTYPES = ("float32", "float16", "bfloat16")
DT_CODE = {"float32": 0, "float16": 1, "bfloat16": 2}
VEC = {"float32": 4, "float16": 8, "bfloat16": 8}            # N: elements of a lane vector (IO<TI, uint8_t>::N = 16 / sizeof(TI))
THREADS = 256                                                # kThreads
U = 4                                                        # AffineCodesOp::kFixedU: lane vectors per lane, one variant per route

# (scale, zero_point, qmin, qmax): the zero point at either end of either domain, domains narrower than the type, a step with an
# inexact reciprocal, one so large that only the saturating ends of float32 / bfloat16 leave the zero point and one so small
# that every normal float32 saturates (3e-33 < 2^-100: fetch_lane takes the IEEE division; 1e30 is just below 2^100 = 1.27e30,
# among the largest divisors recip_exact takes)
PARAMS = ((0.25, -128, -128, 127), (0.2, 127, -128, 127), (0.3, 0, 0, 255), (0.0123, 255, 0, 255), (0.05, 3, -8, 7),
          (0.11, 7, 0, 15), (0.017, 100, 3, 200), (1.7 / 127, 0, -128, 127), (1e30, -1, -128, 127), (3e-33, 100, 0, 255))
SIGNED = tuple(p for p in PARAMS if p[2] < 0)
UNSIGNED = tuple(p for p in PARAMS if p[2] >= 0)


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _note(shape, dt, u=U, nt=1):
    return f"{shape}<AffineCodesOp,in{16 // VEC[dt]}B,out1B,U={u},NT={nt}>"


def _shifted(xd, off):
    """The same elements ``off`` elements past a 16-byte boundary."""
    buf = torch.zeros(xd.numel() + 16, dtype=xd.dtype, device="cuda")
    x = buf[off:off + xd.numel()]
    x.copy_(xd.reshape(-1))
    assert x.data_ptr() % 16 == (off * xd.element_size()) % 16
    return x


def _store(x32, dt, off=0):
    """float32 values -> (device tensor of storage type dt, ``off`` elements past a 16-byte boundary; the values it holds,
    widened to float32)."""
    x = _shifted(_dev(np.asarray(x32, dtype=np.float32).reshape(-1)).to(getattr(torch, dt)), off)
    return x, x.float().cpu().numpy()


def _table(values, dtype, off=0):
    """Device copy of a parameter table, ``off`` elements (4 bytes each) past a 16-byte boundary."""
    t = _shifted(_dev(np.asarray(values, dtype=dtype)), off)
    assert t.data_ptr() % 16 == 4 * off
    return t


def _want_codes(x_np, scales, zps, qmin, qmax, axis=None):
    """The oracle's clamp index of every element; NaN -> qmin."""
    from oracle import mctq_oracle as O
    with np.errstate(invalid="ignore"):                       # the NaN elements' cast, replaced in the next line
        _, idx = O.fake_quant_affine(x_np, scales, zps, qmin, qmax, axis=axis, return_index=True)
    idx = np.where(np.isnan(x_np), qmin, idx)
    assert idx.min() >= qmin and idx.max() <= qmax
    return idx


def _bytes(idx):
    """Codes as stored: the low byte of the two's-complement value, int8 and uint8 alike."""
    return (np.asarray(idx, dtype=np.int64).reshape(-1) & 0xFF).astype(np.uint8)


def _codes(raw, qmin):
    raw = np.asarray(raw, dtype=np.uint8)
    return (raw.view(np.int8) if qmin < 0 else raw).astype(np.int64)


def _assert_codes(got, want_idx, x_np, qmin, what):
    want = _bytes(want_idx)
    assert got.shape == want.shape, f"{what}: {got.shape} bytes, expected {want.shape}"
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.size} of {want.size} codes differ, first at element {i}: x={x_np.reshape(-1)[i]!r} "
                         f"got {int(_codes(got, qmin)[i])} want {int(_codes(want, qmin)[i])}")


class _Frame:
    """One output byte per element in the middle of a 0xA5 frame, ``yoff`` bytes past a 16-byte boundary; the bytes inside start
    as the complement of ``want_idx`` (``fill`` instead when there is nothing to expect).  Outputs of wider elements
    (tests/test_gpu_affine_routes.py) give their starting bytes as ``inside``."""

    def __init__(self, want_idx=None, nbytes=None, fill=0x3C, yoff=0, inside=None):
        if inside is None:
            inside = np.full(nbytes, fill, np.uint8) if want_idx is None else ~_bytes(want_idx)
        inside = np.ascontiguousarray(inside, dtype=np.uint8).reshape(-1)
        self.inside = inside
        self.nb = inside.size
        self.at = GUARD + yoff
        self.buf = torch.full((self.nb + 2 * GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.y = self.buf[self.at:self.at + self.nb]
        self.y.copy_(_dev(inside))
        assert self.buf.data_ptr() % 16 == 0 and self.ptr() % 16 == yoff % 16

    def ptr(self):
        return self.buf.data_ptr() + self.at

    def result(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        edge = np.concatenate([b[:self.at], b[self.at + self.nb:]])
        assert edge.size >= 2 * GUARD and np.all(edge == GUARD_BYTE), f"{what}: wrote outside its {self.nb} bytes"
        return b[self.at:self.at + self.nb]

    def untouched(self, what):
        assert np.array_equal(self.result(what), self.inside), f"{what}: wrote into the output"


def _code8(qmin):
    from mct_quantizers_amd.hip import native
    return native.CODE_I8 if qmin < 0 else native.CODE_U8


def _run_tensor(lib, xd, x_np, dt, prm, note, what, yoff=0):
    """One per-tensor call on the framed output: the oracle's bytes, one launch, the note.  Returns the codes."""
    from mct_quantizers_amd.hip import native
    scale, zp, qmin, qmax = prm
    want = _want_codes(x_np, np.float32(scale), zp, qmin, qmax)
    fr = _Frame(want, yoff=yoff)
    count = native.launch_count()
    rc = lib.mctq_fq_codes_per_tensor(xd.data_ptr(), fr.ptr(), x_np.size, DT_CODE[dt], _code8(qmin), float(scale), zp, qmin,
                                      qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: took {text}, expected {note}"
    got = fr.result(f"{what} [{text}]")
    _assert_codes(got, want, x_np, qmin, f"{what} [{text}]")
    return _codes(got, qmin)


def _run_channels(lib, xd, x_np, dt, scales, zps, qmin, qmax, note, what, yoff=0, null_zps=False, tab_off=(0, 0)):
    """One per-channel call ([outer, C, inner] = x_np.shape) on the framed output, as _run_tensor.  ``null_zps``: the call has
    no zero-point table and the oracle zero points of 0."""
    from mct_quantizers_amd.hip import native
    outer, C, inner = x_np.shape
    scales = np.asarray(scales, dtype=np.float32)
    zps = np.zeros(C, np.int32) if null_zps else np.asarray(zps, dtype=np.int32)
    want = _want_codes(x_np, scales, zps, qmin, qmax, axis=1)
    fr = _Frame(want, yoff=yoff)
    s_d, z_d = _table(scales, np.float32, tab_off[0]), _table(zps, np.int32, tab_off[1])
    count = native.launch_count()
    rc = lib.mctq_fq_codes_per_channel(xd.data_ptr(), fr.ptr(), outer, C, inner, DT_CODE[dt], _code8(qmin), s_d.data_ptr(),
                                       None if null_zps else z_d.data_ptr(), qmin, qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: took {text}, expected {note}"
    got = fr.result(f"{what} [{text}]")
    _assert_codes(got, want, x_np, qmin, f"{what} [{text}]")
    return _codes(got, qmin)


# ------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------

def _grid_values(prm):
    """k s, (k + 1/2) s and its two float32 neighbours, for every k from three below the domain to three above it."""
    scale, zp, qmin, qmax = prm
    s = np.float32(scale)
    k = np.arange(qmin - 3 - zp, qmax + 3 - zp + 1).astype(np.float32)
    with np.errstate(over="ignore"):                           # 258 * 1e30 and the like: +-inf are inputs as good as any
        half = ((k + np.float32(0.5)) * s).astype(np.float32)
        return np.concatenate([(k * s).astype(np.float32), half, np.nextafter(half, np.float32(-np.inf)),
                               np.nextafter(half, np.float32(np.inf))]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sweep_host(dt):
    """Every bit pattern of the 16-bit types, widened; for float32 every exponent x {mantissa 0, 1, 2, 0x3fffff, 0x400000,
    0x7ffffe, 0x7fffff and 40 seeded random ones} x both signs (+-0.0, denormals, +-inf and NaN payloads among them), +-3e38,
    and the steps, ties and tie neighbours of every grid of PARAMS; zeros up to whole 8192-element blocks.  Returns (bit
    patterns, values as float32)."""
    if dt == "float32":
        rng = np.random.default_rng(8)
        mant = np.concatenate([np.asarray([0, 1, 2, 0x3fffff, 0x400000, 0x7ffffe, 0x7fffff], dtype=np.uint32),
                               rng.integers(0, 1 << 23, size=40).astype(np.uint32)])
        expo = np.arange(256, dtype=np.uint32) << 23
        pos = (expo[:, None] | mant[None, :]).reshape(-1)
        bits = np.concatenate([pos, pos | np.uint32(1 << 31)]).astype(np.uint32)
        x = np.concatenate([bits.view(np.float32), np.asarray([3e38, -3e38], np.float32)] + [_grid_values(p) for p in PARAMS])
        x = np.concatenate([x, np.zeros(-x.size % 8192, np.float32)]).astype(np.float32)
        bits = x.view(np.uint32).copy()
    else:
        bits = np.arange(1 << 16, dtype=np.uint16)
        x = torch.from_numpy(bits.view(np.int16).copy()).view(getattr(torch, dt)).float().numpy()
    assert x.size % 8192 == 0
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x == 0).any()
    if dt != "float16":                                                          # (float16's denormals widen to normal float32 values)
        assert (np.abs(x[np.isfinite(x) & (x != 0)]) < 1e-38).any()              # denormals
    x.setflags(write=False)
    return bits, x


@functools.lru_cache(maxsize=None)
def _sweep(dt):
    """(device tensor of storage type dt, 16-byte aligned; the values it holds as float32)."""
    bits, x = _sweep_host(dt)
    if dt == "float32":
        xd = _dev(bits.view(np.int32)).view(torch.float32)
    else:
        xd = _dev(bits.view(np.int16)).view(getattr(torch, dt))
    assert xd.data_ptr() % 16 == 0
    assert np.array_equal(xd.view(torch.int32 if dt == "float32" else torch.int16).cpu().numpy().view(bits.dtype), bits)
    return xd, x


def _assert_covers(dt, x_np, want, scale, qmin, qmax, what):
    """A sweep that saturated everything to one end, or nothing at all, could not pass: FINITE inputs reach both ends of the
    domain.  One pair cannot give that: no finite float16 (|x| <= 65504) reaches half a step of 1e30, so there -inf / NaN ->
    qmin and +inf -> qmax are the ends' only witnesses."""
    keep = np.isfinite(x_np) if not (dt == "float16" and scale > 2 * 65504) else np.ones(x_np.shape, bool)
    w = want[np.broadcast_to(keep, want.shape)]
    assert w.min() == qmin and w.max() == qmax, (what, int(w.min()), int(w.max()))


def _channel_sets(sets, C):
    """Per-channel tables cycling ``sets``; every (qmin, qmax) among them is launched once with all of the tables."""
    scales = [sets[c % len(sets)][0] for c in range(C)]
    zps = [sets[c % len(sets)][1] for c in range(C)]
    domains = sorted({(p[2], p[3]) for p in sets})
    return scales, zps, domains


def _dequantized(codes, scales, zps, axis_shape=None):
    """float32(code - z) * s with one float32 multiply per element."""
    s = np.asarray(scales, dtype=np.float32)
    z = np.asarray(zps, dtype=np.int64)
    if axis_shape is not None:
        s, z = s.reshape(axis_shape), z.reshape(axis_shape)
    return ((codes - z).astype(np.float32) * s).astype(np.float32)


def _same_bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1).view(np.uint32)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} dequantized codes differ from the fake-quantized tensor, first at {int(bad[0])}"


# ------------------------------------------------------------------------------------------------
# (a) value sweeps through every route.  Per-channel sweeps give every channel the whole value vector, so every value meets
#     the steps, ties and tie neighbours of its OWN channel's grid.  float32 storage: the second witness -- the codes
#     dequantize, bit for bit and with NaN and +-inf included, to what mctq_fq_per_tensor / mctq_fq_per_channel write.
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["flat_kernel", "flat_scalar_kernel"])
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_per_tensor(lib, dt, route):
    xd, x = _sweep(dt)
    assert x.size // VEC[dt] > THREADS * U                              # more than one block of the flat kernel
    if route == "flat_scalar_kernel":
        xd = _shifted(xd, 1)                                            # x one element off: one element per lane
    note = _note(route, dt) if route == "flat_kernel" else _note(route, dt, 1, 0)
    for prm in PARAMS:
        what = f"{route} {dt} {prm}"
        want = _want_codes(x, np.float32(prm[0]), prm[1], prm[2], prm[3])
        _assert_covers(dt, x, want, prm[0], prm[2], prm[3], what)
        got = _run_tensor(lib, xd, x, dt, prm, note, what)
        if dt == "float32":
            y = torch.full((x.size,), 12345.0, dtype=torch.float32, device="cuda")
            rc = lib.mctq_fq_per_tensor(xd.data_ptr(), y.data_ptr(), x.size, 0, float(prm[0]), prm[1], prm[2], prm[3], _stream())
            assert rc == 0, lib.mctq_last_error()
            _same_bits(_dequantized(got, prm[0], prm[1]), y.cpu().numpy(), what)


def _sweep_layout(dt, route, C):
    """The sweep vector laid out for a per-channel route -> (device tensor, values [outer, C, inner], launch note, x offset).
      rows_kernel            [2, C, n]: every row the whole vector; n / N >= 256 whole lane vectors -> several tiles a row
      lastaxis_kernel        [n, 8, 1]: every column the whole vector (C = 8: a multiple of N for every storage type)
      window_kernel<vector>  [n, 5, 1]: as above with C % N != 0: the whole table staged, the per-element walk
      window_kernel<scalar>  the same with x one element off its vector boundary"""
    xd1, x1 = _sweep(dt)
    if route == "rows_kernel":
        x = np.ascontiguousarray(np.broadcast_to(x1, (2, C, x1.size)))
        return xd1.repeat(2 * C), x, _note(route, dt)
    x = np.ascontiguousarray(np.broadcast_to(x1[:, None, None], (x1.size, C, 1)))
    xd = xd1.repeat_interleave(C)
    if route == "lastaxis_kernel":
        return xd, x, _note(route, dt, 2)
    if route == "window_kernel<scalar>":
        xd = _shifted(xd, 1)
    return xd, x, _note(route, dt)


@pytest.mark.parametrize("sets", [SIGNED, UNSIGNED], ids=["signed", "unsigned"])
@pytest.mark.parametrize("route", ["rows_kernel", "lastaxis_kernel", "window_kernel<vector>", "window_kernel<scalar>"])
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_per_channel(lib, dt, route, sets):
    C = 8 if route == "lastaxis_kernel" else 5
    assert len(sets) == 5
    xd, x, note = _sweep_layout(dt, route, C)
    assert xd.data_ptr() % 16 == (0 if route != "window_kernel<scalar>" else xd.element_size())
    scales, zps, domains = _channel_sets(sets, C)
    for qmin, qmax in domains:
        what = f"{route} {dt} {x.shape} [{qmin}, {qmax}]"
        want = _want_codes(x, np.float32(scales), zps, qmin, qmax, axis=1)
        for c in range(C):
            _assert_covers(dt, x[:, c], want[:, c], scales[c], qmin, qmax, f"{what} channel {c}")
        got = _run_channels(lib, xd, x, dt, scales, zps, qmin, qmax, note, what)
        if dt == "float32":
            y = torch.full((x.size,), 12345.0, dtype=torch.float32, device="cuda")
            s_d, z_d = _table(scales, np.float32), _table(zps, np.int32)
            rc = lib.mctq_fq_per_channel(xd.data_ptr(), y.data_ptr(), *x.shape, 0, s_d.data_ptr(), z_d.data_ptr(), qmin, qmax,
                                         _stream())
            assert rc == 0, lib.mctq_last_error()
            _same_bits(_dequantized(got.reshape(x.shape), scales, zps, (1, C, 1)), y.cpu().numpy(), what)


# ------------------------------------------------------------------------------------------------
# (b) launch geometry.  The shapes follow from the launchers' arithmetic in mctq_kernels.hpp as it stands (launch_flat,
#     launch_channels); a change there needs new shapes here.  A lane vector is 16 bytes of input: N = 4 float32 / 8 half
#     elements; kThreads = 256; AffineCodesOp::kFixedU = 4, so a tile of the flat, rows and window launches is 1024 lane
#     vectors = 1024 N elements.  The shortrows, rowsteps, paced and finetail launches are AffineOp's alone.
# ------------------------------------------------------------------------------------------------

def _edge_values(rng, shape, s_b, zp_b, qmin, qmax):
    """Inputs dense in round-half ties and clamp edges of their own channel's grid (as tests/test_gpu_parity.py), with NaN,
    +-inf, +-0.0, a denormal and +-3e38 sprinkled over one element in 16."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore", invalid="ignore"):
        x = (rng.standard_normal(n).astype(np.float32).reshape(shape) * s_b * np.float32(0.4 * (qmax - qmin)))
        k = rng.integers(qmin - 2, qmax + 3, size=shape).astype(np.float32) - zp_b
        kind = rng.integers(0, 6, size=shape)
        x = np.where(kind == 0, (k + np.float32(0.5)) * s_b, x)
        x = np.where(kind == 1, k * s_b, x)
    special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], dtype=np.float32)
    pick = rng.integers(0, 16 * special.size, size=shape)
    return np.where(pick < special.size, special[pick % special.size], x).astype(np.float32)


FLAT_PARAMS = ((0.0371, 5, 0, 255), (0.113, -3, -128, 127), (0.21, 15, 0, 15))


def _rounds(n):
    """Launches of a case: shapes of fewer than 256 elements are run until 256 values have gone through them, so that a
    one-element case sees ties and both clamp ends as the large ones do."""
    return -(-256 // n) if n < 256 else 1


# launch_flat, x and codes on a vector boundary: nv = n / N lane vectors, blocks = max(1, ceil(nv / 1024)); block 0 also writes
# the n % N trailing elements one per lane.
#   1              nv = 0: one block whose tile is empty, only the scalar tail
#   N              one lane vector, no tail
#   1024 N         one exactly full block (the unguarded tile)
#   1024 N + N + 1 a second block of one lane vector, a tail of one element
#   2348 N + 3     three blocks, the last 300 of 1024 lane vectors, a tail of three
@pytest.mark.parametrize("kind", ["1", "N", "1024N", "1024N+N+1", "2348N+3"])
@pytest.mark.parametrize("dt", DTYPES)
def test_flat_kernel_geometry(lib, dt, kind):
    N = VEC[dt]
    n = {"1": 1, "N": N, "1024N": 1024 * N, "1024N+N+1": 1024 * N + N + 1, "2348N+3": 2348 * N + 3}[kind]
    rng = np.random.default_rng([n, DT_CODE[dt]])
    for prm in FLAT_PARAMS:
        seen = set()
        for _ in range(_rounds(n)):
            x32 = _edge_values(rng, (n,), np.float32(prm[0]), np.float32(prm[1]), prm[2], prm[3])
            xd, x = _store(x32, dt)
            seen.update(_run_tensor(lib, xd, x, dt, prm, _note("flat_kernel", dt), f"flat {dt} n={n} {prm}").tolist())
        assert {prm[2], prm[3]} <= seen                                  # both ends of the domain were asked for


# launch_flat off a vector boundary (x % 16 != 0, or codes % N != 0): flat_scalar_kernel, one element per lane, a grid-stride
# loop.  2348 N + 3 elements: several blocks; codes + 1 is odd, off every boundary the vector stores could want.
@pytest.mark.parametrize("xoff,yoff", [(1, 0), (0, 1), (1, 1)], ids=["x+1", "codes+1", "both"])
@pytest.mark.parametrize("dt", DTYPES)
def test_flat_scalar_kernel(lib, dt, xoff, yoff):
    n = 2348 * VEC[dt] + 3
    rng = np.random.default_rng([n, DT_CODE[dt], xoff, yoff])
    for prm in FLAT_PARAMS:
        x32 = _edge_values(rng, (n,), np.float32(prm[0]), np.float32(prm[1]), prm[2], prm[3])
        xd, x = _store(x32, dt, xoff)
        _run_tensor(lib, xd, x, dt, prm, _note("flat_scalar_kernel", dt, 1, 0), f"flat scalar {dt} x+{xoff} y+{yoff} {prm}", yoff)


def _channel_case(rng, shape, dt, qmin, qmax, xoff=0, scales=None):
    """Edge-heavy [outer, C, inner] input of storage type dt with a scale and a zero point (anywhere in the domain) per channel."""
    C = shape[1]
    if scales is None:
        scales = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
    zps = rng.integers(qmin, qmax + 1, size=C).astype(np.int32)
    x32 = _edge_values(rng, shape, scales.reshape(1, C, 1), zps.reshape(1, C, 1).astype(np.float32), qmin, qmax)
    xd, x = _store(x32.reshape(-1), dt, xoff)
    return xd, x.reshape(shape), scales, zps


def _channel_forms(lib, shape, dt, note, xoff=0, yoff=0, tab_off=(0, 0), scales=None):
    """One shape on one route in the three forms of a per-channel call: int8 and uint8 with a zero-point table, int8 with
    zero_points == NULL."""
    rng = np.random.default_rng([*shape, DT_CODE[dt], xoff, yoff])
    for qmin, qmax, null_zps in ((-128, 127, False), (0, 255, False), (-128, 127, True)):
        if null_zps and tab_off[1]:
            continue                                                  # no table to misalign
        xd, x, s, z = _channel_case(rng, shape, dt, qmin, qmax, xoff, scales)
        if null_zps:                                                  # the inputs around a zero point of 0
            x32 = _edge_values(rng, shape, s.reshape(1, -1, 1), np.float32(0), qmin, qmax)
            xd, x = _store(x32.reshape(-1), dt, xoff)
            x = x.reshape(shape)
        _run_channels(lib, xd, x, dt, s, z, qmin, qmax, note,
                      f"{dt} {shape} x+{xoff} y+{yoff} tables+{tab_off} [{qmin}, {qmax}]{' NULL zero points' if null_zps else ''}",
                      yoff, null_zps, tab_off)


# rows_kernel: inner % N == 0 and innerv = inner / N >= 256; tiles = ceil(innerv / 1024) per row, grid = rows * tiles; the
# channel of a row is row % C (taken when row >= C: outer > 1).
#   innerv   tiles   last tile
#    256       1     a quarter filled (the guarded path)
#   1024       1     exactly full (the unguarded path)
#   1025       2     one lane vector
#   2348       3     300 of 1024
# outer x C = 2 x 3 and 3 x 5: rows past the first outer slice wrap to channel row % C with tiles > 1 and with one tile.
@pytest.mark.parametrize("outer,C,innerv", [(2, 3, 256), (2, 3, 1024), (2, 3, 1025), (2, 3, 2348), (3, 5, 256), (3, 5, 1025)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES)
def test_rows_kernel_geometry(lib, dt, outer, C, innerv):
    _channel_forms(lib, (outer, C, innerv * VEC[dt]), dt, _note("rows_kernel", dt))


def _slab_rows(vc):
    """launch_channels' rows per slab of the last-axis launch for vc lane vectors per row: the candidate k in [ceil(2048 / vc),
    ceil(2048 / vc) + 16) with the least (256 - (k vc) % 256) % 256 * 4096 / (k vc), first of equals."""
    k0 = -(-2048 // vc)
    waste = [(THREADS - (k * vc) % THREADS) % THREADS * 4096 // (k * vc) for k in range(k0, k0 + 16)]
    return k0 + waste.index(min(waste))


# lastaxis_kernel: inner == 1, C % N == 0, both tables 16-byte aligned; vc = C / N lane vectors per row; a slab is k rows
# (_slab_rows), ceil(k vc / 256) blocks wide; every lane steps down two slabs (the note's U = 2): a group is 2 k rows,
# grid.y = ceil(outer / 2 k).  ZP = true with a zero-point table, false with NULL (_channel_forms runs both).
#   C         vc (f32 / halves)   k            outer
#   N           1                 2048         1: one row of the first slab;  4096: one whole group (the unguarded body);
#                                              4097: a second group of one row
#   3 N         3  (float32)      698          2 k + 1 (a slab that is no multiple of 256 lanes: idle lanes in its last block)
#   64         16 / 8             128 / 256    2 k + 3
#   1024 N   1024                 2            5: groups of 4 rows; the second group has one row -- its first slab half
#                                              filled, its second slab idle
LASTAXIS_CASES = [(dt, cname, outer) for dt in DTYPES
                  for cname, outer in (("N", 1), ("N", 4096), ("N", 4097), ("3N", None), ("64", None), ("1024N", 5))
                  if cname != "3N" or dt == "float32"]


@pytest.mark.parametrize("dt,cname,outer", LASTAXIS_CASES, ids=lambda v: str(v))
def test_lastaxis_kernel_geometry(lib, dt, cname, outer):
    N = VEC[dt]
    C = {"N": N, "3N": 3 * N, "64": 64, "1024N": 1024 * N}[cname]
    k = _slab_rows(C // N)
    assert k == {"N": 2048, "3N": 698, "64": 2048 * N // 64, "1024N": 2}[cname]
    if outer is None:
        outer = 2 * k + (1 if cname == "3N" else 3)
    _channel_forms(lib, (outer, C, 1), dt, _note("lastaxis_kernel", dt, 2))


# fetch_lane's two reciprocal forms: recip_exact when every active lane of the WAVE has its N scales in [2^-100, 2^100], the
# IEEE division otherwise.  C = 256 N: vc = 256, k = 8 -- a block is one row, wave w of it owns channels [64 N w, 64 N (w + 1)).
# 3e-33 (< 2^-100) in a channel of wave 0 and 2e31 (> 2^100) in one of wave 2: waves 0 and 2 divide, waves 1 and 3 do not.
@pytest.mark.parametrize("dt", DTYPES)
def test_lastaxis_kernel_takes_both_reciprocal_forms(lib, dt):
    N = VEC[dt]
    C = 256 * N
    assert _slab_rows(256) == 8
    scales = np.random.default_rng(5).uniform(0.01, 0.9, size=C).astype(np.float32)
    scales[5] = np.float32(3e-33)
    scales[2 * 64 * N + 3] = np.float32(2e31)
    assert scales[5] < 2.0 ** -100 and scales[2 * 64 * N + 3] > 2.0 ** 100
    _channel_forms(lib, (17, C, 1), dt, _note("lastaxis_kernel", dt, 2), scales=scales)


# A table 4 bytes off a 16-byte boundary cannot be read by 16-byte loads: the same call takes the window launch.
@pytest.mark.parametrize("tab_off", [(1, 0), (0, 1)], ids=["scales+4", "zero_points+4"])
@pytest.mark.parametrize("dt", DTYPES)
def test_lastaxis_falls_back_to_the_window_launch_on_misaligned_tables(lib, dt, tab_off):
    _channel_forms(lib, (259, 64, 1), dt, _note("window_kernel<vector>", dt), tab_off=tab_off)


# window_kernel<vector> (x and codes on a vector boundary; rows no rows_kernel or lastaxis launch takes): block b owns
# elements [1024 N b, 1024 N (b + 1)) of the dense storage; it stages the parameters of the rows it touches -- the whole table
# when C <= that number of rows ("whole"), else the window of rows with ONE wrap from channel C - 1 to 0 ("window") -- and a
# lane vector then lies in one row ("same"), crosses exactly one boundary ("straddle": inner >= N, inner % N != 0) or is
# walked element by element ("walk": inner < N).  Every shape has more than one block and a ragged last one.
#   shape (float32 / halves)                     rows   staging  note
#   (1500, 3, 1) / (3000, 3, 1)                  walk   whole    inner == 1, C % N != 0
#   (300, 5, 3) / (600, 5, 3)                    walk   whole    a lane vector crosses one or two (halves: two or three) boundaries
#   (2, 300, 8) / (2, 600, 8)                    same   whole
#   (2, 30, 104) / (2, 50, 104)                  same   whole
#   (3, 16, 100)                                 same   whole    float32: 100 % 4 == 0
#   (150, 6, 5), (100, 6, 7), (3, 16, 102)       straddle whole  float32
#   (70, 10, 12), (6, 16, 100), (2, 5, 1028)     straddle whole  halves
#   (2, 700, 7) / (2, 1300, 7)                   straddle / walk  window  586 / 1172 rows per tile < C; the second block crosses the wrap
#   (3, 6001, 1)                                 walk   window   float32: U = 4 (4096 rows staged); halves: the 8192 rows of a U = 4
#                                                                tile need min(C, 8192) * 3 words = 72 012 bytes of LDS > 64 KiB, so the
#                                                                launch takes the one-vector tile: U = 1, 2048 rows per tile
WINDOW_CASES = {"float32": ((1500, 3, 1), (300, 5, 3), (2, 300, 8), (2, 30, 104), (3, 16, 100), (150, 6, 5), (100, 6, 7),
                            (3, 16, 102), (2, 700, 7), (3, 6001, 1)),
                "float16": ((3000, 3, 1), (600, 5, 3), (2, 600, 8), (2, 50, 104), (70, 10, 12), (6, 16, 100), (2, 5, 1028),
                            (2, 1300, 7), (3, 6001, 1))}
WINDOW_CASES["bfloat16"] = WINDOW_CASES["float16"]


@pytest.mark.parametrize("dt,shape", [(dt, shape) for dt in DTYPES for shape in WINDOW_CASES[dt]], ids=lambda v: str(v))
def test_window_kernel_vector_geometry(lib, dt, shape):
    N = VEC[dt]
    n = shape[0] * shape[1] * shape[2]
    one_vector_tile = shape == (3, 6001, 1) and N == 8
    tile = THREADS * (1 if one_vector_tile else U) * N
    assert n > tile and n % tile != 0
    if shape[1] in (700, 1300, 6001):                                  # the row window: fewer rows in a tile than channels
        assert (tile - 1 + shape[2] - 1) // shape[2] + 1 < shape[1] and shape[0] > 1
    _channel_forms(lib, shape, dt, _note("window_kernel<vector>", dt, 1 if one_vector_tile else U))


# window_kernel<scalar>: x or codes off its vector boundary: one element per lane access, tiles of 1024 elements, the same
# staging.  The three row kinds of the vector form (here they differ in the rows a tile touches), each with x, codes or both off.
@pytest.mark.parametrize("xoff,yoff", [(1, 0), (0, 1), (1, 1)], ids=["x+1", "codes+1", "both"])
@pytest.mark.parametrize("shape", [(700, 3, 1), (2, 150, 8), (50, 6, 7), (2, 700, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES)
def test_window_kernel_scalar_geometry(lib, dt, shape, xoff, yoff):
    _channel_forms(lib, shape, dt, _note("window_kernel<scalar>", dt), xoff=xoff, yoff=yoff)


# ------------------------------------------------------------------------------------------------
# (c) refusals and empties through the raw entry points: nothing launched, nothing noted, nothing written.  Every call has
#     valid device pointers with room for the call as if it were accepted.
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_refused_and_empty_calls_launch_nothing(lib, dt):
    from mct_quantizers_amd.hip import native
    E = native.MCTQ_E_ARG
    n = 96                                                            # the accepted size: [2, 6, 8] or [12, 8, 1]
    xb = torch.zeros(n, dtype=getattr(torch, dt), device="cuda")
    s_d, z_d = _dev(np.full(16, 0.25, np.float32)), _dev(np.zeros(16, np.int32))
    fr = _Frame(nbytes=n)
    x, y, s, z, st = xb.data_ptr(), fr.ptr(), s_d.data_ptr(), z_d.data_ptr(), _stream()
    dtc, I8, U8 = DT_CODE[dt], native.CODE_I8, native.CODE_U8
    assert lib.mctq_fq_codes_per_tensor(x, y, n, dtc, I8, 0.25, 0, -128, 127, st) == 0     # a note of this file's own to hold on to
    fr.y.copy_(_dev(fr.inside))
    torch.cuda.synchronize()
    count, text = native.launch_count(), native.last_launch()
    assert text == _note("flat_kernel", dt)

    def per_tensor(xp, yp, nn, dtype=dtc, code=I8, qmin=-128, qmax=127):
        return lib.mctq_fq_codes_per_tensor(xp, yp, nn, dtype, code, 0.25, 0, qmin, qmax, st)

    def per_channel(xp, yp, o, c, i, dtype=dtc, code=I8, qmin=-128, qmax=127, sp=s, zp=z):
        return lib.mctq_fq_codes_per_channel(xp, yp, o, c, i, dtype, code, sp, zp, qmin, qmax, st)

    calls = [("n == 0", 0, lambda: per_tensor(x, y, 0)),
             ("n == 0, NULL pointers", 0, lambda: per_tensor(None, None, 0)),
             ("outer == 0", 0, lambda: per_channel(x, y, 0, 6, 8)),
             ("channels == 0", 0, lambda: per_channel(x, y, 2, 0, 8)),
             ("inner == 0", 0, lambda: per_channel(x, y, 2, 6, 0)),
             ("outer == 0, last axis", 0, lambda: per_channel(x, y, 0, 8, 1)),
             ("n < 0", E, lambda: per_tensor(x, y, -1)),
             ("negative extent", E, lambda: per_channel(x, y, 2, -6, 8)),
             ("x NULL, per tensor", E, lambda: per_tensor(None, y, n)),
             ("codes NULL, per tensor", E, lambda: per_tensor(x, None, n)),
             ("x NULL, per channel", E, lambda: per_channel(None, y, 2, 6, 8)),
             ("codes NULL, per channel", E, lambda: per_channel(x, None, 2, 6, 8)),
             ("scales NULL", E, lambda: per_channel(x, y, 2, 6, 8, sp=None)),
             ("quant_min > quant_max, per tensor", E, lambda: per_tensor(x, y, n, qmin=5, qmax=4)),
             ("quant_min > quant_max, per channel", E, lambda: per_channel(x, y, 2, 6, 8, qmin=5, qmax=4)),
             ("[-129, 127] as int8", E, lambda: per_tensor(x, y, n, qmin=-129)),
             ("[-128, 128] as int8", E, lambda: per_channel(x, y, 12, 8, 1, qmax=128)),
             ("[-1, 255] as uint8", E, lambda: per_tensor(x, y, n, code=U8, qmin=-1, qmax=255)),
             ("[0, 256] as uint8", E, lambda: per_channel(x, y, 2, 6, 8, code=U8, qmin=0, qmax=256)),
             ("dtype 3 (float64), per tensor", E, lambda: per_tensor(x, y, n, dtype=3)),
             ("dtype 7, per tensor", E, lambda: per_tensor(x, y, n, dtype=7)),
             ("dtype 7, per channel", E, lambda: per_channel(x, y, 2, 6, 8, dtype=7)),
             ("code type 9, per tensor", E, lambda: per_tensor(x, y, n, code=9)),
             ("code type -1, per channel", E, lambda: per_channel(x, y, 12, 8, 1, code=-1))]
    for what, want_rc, call in calls:
        assert call() == want_rc, (what, lib.mctq_last_error())
        assert native.launch_count() == count and native.last_launch() == text, what
        fr.untouched(what)


# ------------------------------------------------------------------------------------------------
# (d) through Python: ops.fq_codes on a permuted and on a channels-last tensor, quantize_to_codes of two quantizers
# ------------------------------------------------------------------------------------------------

CL_SHAPE = (2, 1032, 5, 19)     # storage order [2, 5, 19, 1032]: 190 rows of 1032 channels -- more than one last-axis group
                                # (2 k = 46 / 62 rows) and 196080 elements: 48 / 24 blocks of the flat kernel


def _launched(f, note):
    from mct_quantizers_amd.hip import native
    count = native.launch_count()
    out = f()
    assert native.launch_count() == count + 1 and native.last_launch() == note, native.last_launch()
    return out


@pytest.mark.parametrize("dt", DTYPES)
def test_python_routes_on_permuted_and_channels_last_tensors(lib, dt):
    import warnings
    import mct_quantizers_amd as mq
    from mct_quantizers_amd.hip import ops
    from oracle import oracle_call
    Q = mq.pytorch_quantizers
    tdt = getattr(torch, dt)
    C = CL_SHAPE[1]
    assert _slab_rows(C // VEC[dt]) == {4: 23, 8: 31}[VEC[dt]]
    rng = np.random.default_rng([8, DT_CODE[dt]])
    scales = rng.uniform(0.05, 0.5, size=C).astype(np.float32)
    zps = rng.integers(0, 256, size=C).astype(np.int32)
    x32 = _edge_values(rng, CL_SHAPE, scales.reshape(1, C, 1, 1), zps.reshape(1, C, 1, 1).astype(np.float32), 0, 255)
    x_cpu = torch.from_numpy(x32).to(tdt).contiguous(memory_format=torch.channels_last)
    x = x_cpu.cuda()
    assert x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    x_np = x_cpu.float().numpy()
    s_d, z_d = _dev(scales), _dev(zps)

    def check(got, want, cpu, what):
        assert got.dtype == torch.uint8 and got.shape == want.shape
        g = got.cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, f"{what} {dt}: {bad.size} codes differ from the oracle, first at {int(bad[0])}"
        assert torch.equal(cpu, got.cpu()), f"{what} {dt}: the CPU route differs"

    # channels-last, per channel on axis 1: storage [190, 1032, 1] -> the last-axis launch; per tensor: the flat launch
    got = _launched(lambda: ops.fq_codes(x, s_d, z_d, 1, 0, 255), _note("lastaxis_kernel", dt, 2))
    check(got, _want_codes(x_np, scales, zps, 0, 255, axis=1),
          ops.fq_codes(x_cpu, torch.from_numpy(scales), torch.from_numpy(zps), 1, 0, 255), "fq_codes channels-last axis 1")
    s0, z0 = float(scales[0]), int(zps[0])
    got = _launched(lambda: ops.fq_codes(x, None, None, None, 0, 255, s0, z0), _note("flat_kernel", dt))
    check(got, _want_codes(x_np, scales[0], z0, 0, 255), ops.fq_codes(x_cpu, None, None, None, 0, 255, s0, z0),
          "fq_codes channels-last per tensor")

    # permuted: [300, 40] with strides (1, 300), per channel on axis 1: storage [1, 40, 300] -> rows of 300 elements, the
    # window launch (75 whole float32 lane vectors a row; 37.5 of a 16-bit type: straddling)
    sp, zp = scales[:40].copy(), zps[:40].copy()
    p32 = _edge_values(rng, (40, 300), sp.reshape(40, 1), zp.reshape(40, 1).astype(np.float32), 0, 255)
    p_cpu = torch.from_numpy(p32).to(tdt).t()
    p = p_cpu.cuda()
    assert p.shape == (300, 40) and p.stride() == (1, 300)
    got = _launched(lambda: ops.fq_codes(p, s_d[:40], z_d[:40], 1, 0, 255), _note("window_kernel<vector>", dt))
    check(got, _want_codes(p_cpu.float().numpy(), sp, zp, 0, 255, axis=1),
          ops.fq_codes(p_cpu, torch.from_numpy(sp), torch.from_numpy(zp), 1, 0, 255), "fq_codes permuted axis 1")

    # one weights and one activation quantizer: codes against the oracle and the CPU route (finite inputs: the oracle call
    # has no NaN rule of its own)
    xq32 = np.where(np.isfinite(x32), x32, np.float32(0.75))
    xq_cpu = torch.from_numpy(xq32).to(tdt).contiguous(memory_format=torch.channels_last)
    xq_cpu = torch.where(torch.isfinite(xq_cpu), xq_cpu, torch.zeros_like(xq_cpu))       # (3e38 is inf as float16)
    xq, xq_np = xq_cpu.cuda(), xq_cpu.float().numpy()
    assert xq.is_contiguous(memory_format=torch.channels_last) and np.isfinite(xq_np).all()
    hi = rng.uniform(0.5, 3.0, C)
    cases = (("WeightsSymmetricInferableQuantizer", _note("lastaxis_kernel", dt, 2), torch.int8,
              dict(num_bits=8, threshold=[float(v) for v in hi], per_channel=True, channel_axis=1)),
             ("ActivationUniformInferableQuantizer", _note("flat_kernel", dt), torch.uint8,
              dict(num_bits=8, min_range=[-1.0], max_range=[2.0])))
    for name, note, cdt, kw in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            q = getattr(Q, name)(**kw)
        codes, _, _ = _launched(lambda: q.quantize_to_codes(xq), note)
        _, idx = oracle_call(name, kw, xq_np, return_index=True)
        assert codes.dtype == cdt and codes.shape == xq.shape
        assert np.array_equal(codes.cpu().numpy().astype(np.int64), idx), f"{name} {dt}"
        assert len(np.unique(idx)) > 100
        assert torch.equal(q.quantize_to_codes(xq_cpu)[0], codes.cpu()), f"{name} {dt}: the CPU route differs"


# ------------------------------------------------------------------------------------------------
# (e) mctq_fq_codes_nchw_to_nhwc: x [B][C][P] -> codes [B][P][C], 128 (channels) x 32 (pixels) tiles, 256 lanes.  In: lane t
#     reads four pixels of channel rows t / 8 + 32 j by one vector load when P % 4 == 0 and x is aligned to four elements,
#     element by element otherwise.  Out: lane t writes 16 channels of pixel t / 8 by one 16-byte store when C % 16 == 0 and
#     codes is 16-byte aligned, byte by byte otherwise.  grid = B * ceil(C / 128) * ceil(P / 32).
# ------------------------------------------------------------------------------------------------

NHWC_PARAMS = ((0.25, -128, -128, 127), (0.2, 127, -128, 127), (0.3, 0, 0, 255), (0.0123, 255, 0, 255), (0.11, 7, 0, 15))

# (B, C, P), x offset in elements, codes offset in bytes, vector loads, 16-byte stores
NHWC_CASES = (((1, 1, 1), 0, 0, False, False),      # scalar loads, byte stores
              ((1, 16, 4), 0, 0, True, True),       # vector loads, one 16-byte store per pixel, the rest of the tile idle
              ((2, 128, 32), 0, 0, True, True),     # one full tile per image, batch 2
              ((1, 130, 36), 0, 0, True, False),    # a second channel tile of 2 channels, C % 16 != 0; a second pixel tile of 4
              ((3, 144, 33), 0, 0, False, True),    # a second channel tile of 16; P odd: scalar loads, a pixel tail of 1
              ((1, 48, 35), 0, 0, False, True),     # scalar loads, P % 4 == 3
              ((2, 272, 40), 0, 0, True, True),     # three channel tiles x two pixel tiles x two images: the block-index decomposition
              ((1, 16, 8), 1, 0, False, True),      # scalar loads chosen by the pointer
              ((1, 16, 8), 0, 1, True, False))      # byte stores chosen by the pointer
# all 2^16 patterns of a 16-bit type through three of the shapes, a launch per slice of the pattern vector
NHWC_PATTERNS = {((2, 272, 40), "float16"): "float16", ((3, 144, 33), "bfloat16"): "bfloat16", ((1, 130, 36), "float32"): "float16"}


def _nhwc_note(dt, vload, vstore):
    return (f"codes_nchw_to_nhwc<{'vector' if vload else 'scalar'} loads + {'16-byte' if vstore else 'byte'} stores,"
            f"in{16 // VEC[dt]}B,out1B,U=4,NT=1>")


def _run_nhwc(lib, x32, shape, dt, prm, xoff, yoff, note, what):
    from mct_quantizers_amd.hip import native, ops
    B, C, P = shape
    scale, zp, qmin, qmax = prm
    xd, x = _store(x32, dt, xoff)
    x = x.reshape(shape)
    want = np.ascontiguousarray(_want_codes(x, np.float32(scale), zp, qmin, qmax).transpose(0, 2, 1))
    fr = _Frame(want, yoff=yoff)
    count = native.launch_count()
    rc = lib.mctq_fq_codes_nchw_to_nhwc(xd.data_ptr(), fr.ptr(), B, C, P, DT_CODE[dt], _code8(qmin), float(scale), zp, qmin, qmax,
                                        _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: took {text}, expected {note}"
    got = fr.result(f"{what} [{text}]")
    _assert_codes(got, want, np.ascontiguousarray(x.transpose(0, 2, 1)), qmin, f"{what} [{text}]")
    # the per-tensor entry point's bytes, transposed
    flat = torch.empty(x.size, dtype=torch.uint8, device="cuda")
    rc = lib.mctq_fq_codes_per_tensor(xd.data_ptr(), flat.data_ptr(), x.size, DT_CODE[dt], _code8(qmin), float(scale), zp, qmin, qmax,
                                      _stream())
    assert rc == 0, lib.mctq_last_error()
    assert np.array_equal(flat.cpu().numpy().reshape(shape).transpose(0, 2, 1).reshape(-1), got), f"{what}: per-tensor codes differ"
    # the CPU route of ops.fq_codes_nhwc on the same stored values ([B, C, P, 1] -> [B, P, 1, C])
    cpu = ops.fq_codes_nhwc(xd.cpu().reshape(B, C, P, 1), qmin, qmax, float(scale), zp)
    assert cpu.shape == (B, P, 1, C) and np.array_equal(_bytes(cpu.numpy()), got), f"{what}: the CPU route differs"


def _nhwc_inputs(rng, n, prm):
    """Half from the structured float32 edge set (_sweep_host), half dense in the ties and clamp edges of the grid."""
    x = _edge_values(rng, (n,), np.float32(prm[0]), np.float32(prm[1]), prm[2], prm[3])
    edge = _sweep_host("float32")[1]
    return np.where(rng.integers(0, 2, size=n) == 0, edge[rng.integers(0, edge.size, size=n)], x).astype(np.float32)


@pytest.mark.parametrize("case", NHWC_CASES, ids=lambda c: f"{'x'.join(map(str, c[0]))}-x{c[1]}y{c[2]}")
@pytest.mark.parametrize("dt", DTYPES)
def test_codes_nchw_to_nhwc_geometry(lib, dt, case):
    shape, xoff, yoff, vload, vstore = case
    n = shape[0] * shape[1] * shape[2]
    note = _nhwc_note(dt, vload, vstore)
    rng = np.random.default_rng([*shape, xoff, yoff, DT_CODE[dt]])
    for prm in NHWC_PARAMS:
        for _ in range(_rounds(n)):
            _run_nhwc(lib, _nhwc_inputs(rng, n, prm), shape, dt, prm, xoff, yoff, note, f"nhwc {dt} {shape} x+{xoff} y+{yoff} {prm}")
    pattern_dt = NHWC_PATTERNS.get((shape, dt))
    if pattern_dt is not None:
        values = _sweep_host(pattern_dt)[1]                              # (float32 storage: the float16 patterns, widened)
        seen = 0
        for prm in (NHWC_PARAMS[0], NHWC_PARAMS[3]):
            for at in range(0, values.size, n):
                x32 = values[at:at + n]
                x32 = np.concatenate([x32, _nhwc_inputs(rng, n - x32.size, prm)])
                _run_nhwc(lib, x32, shape, dt, prm, xoff, yoff, note, f"nhwc {dt} {shape} patterns {at}.. {prm}")
                seen += min(n, values.size - at)
        assert seen == 2 * (1 << 16)


@pytest.mark.parametrize("dt", DTYPES)
def test_codes_nchw_to_nhwc_refusals_and_empties(lib, dt):
    from mct_quantizers_amd.hip import native
    E = native.MCTQ_E_ARG
    B, C, P = 2, 16, 8
    xb = torch.zeros(B * C * P, dtype=getattr(torch, dt), device="cuda")
    fr = _Frame(nbytes=B * C * P)
    x, y, st = xb.data_ptr(), fr.ptr(), _stream()
    dtc, I8, U8 = DT_CODE[dt], native.CODE_I8, native.CODE_U8

    def call(xp=x, yp=y, b=B, c=C, p=P, dtype=dtc, code=I8, qmin=-128, qmax=127):
        return lib.mctq_fq_codes_nchw_to_nhwc(xp, yp, b, c, p, dtype, code, 0.25, 0, qmin, qmax, st)

    assert call() == 0                                                 # a note of this file's own to hold on to
    fr.y.copy_(_dev(fr.inside))
    torch.cuda.synchronize()
    count, text = native.launch_count(), native.last_launch()
    assert text == _nhwc_note(dt, True, True)
    calls = [("batch == 0", 0, lambda: call(b=0)), ("channels == 0", 0, lambda: call(c=0)), ("pixels == 0", 0, lambda: call(p=0)),
             ("empty with NULL pointers", 0, lambda: call(xp=None, yp=None, b=0)),
             ("negative batch", E, lambda: call(b=-1)), ("negative channels", E, lambda: call(c=-16)),
             ("negative pixels", E, lambda: call(p=-8)),
             ("x NULL", E, lambda: call(xp=None)), ("codes NULL", E, lambda: call(yp=None)),
             ("MCTQ_CODE_I4", E, lambda: call(code=native.CODE_I4, qmin=-8, qmax=7)),
             ("MCTQ_CODE_U4", E, lambda: call(code=native.CODE_U4, qmin=0, qmax=15)),
             ("code type 9", E, lambda: call(code=9)),
             ("quant_min > quant_max", E, lambda: call(qmin=5, qmax=4)),
             ("[-129, 127] as int8", E, lambda: call(qmin=-129)), ("[-128, 128] as int8", E, lambda: call(qmax=128)),
             ("[-1, 255] as uint8", E, lambda: call(code=U8, qmin=-1, qmax=255)),
             ("[0, 256] as uint8", E, lambda: call(code=U8, qmin=0, qmax=256)),
             ("dtype 3 (float64)", E, lambda: call(dtype=3)), ("dtype 7", E, lambda: call(dtype=7))]
    for what, want_rc, f in calls:
        assert f() == want_rc, (what, lib.mctq_last_error())
        assert native.launch_count() == count and native.last_launch() == text, what
        fr.untouched(what)
