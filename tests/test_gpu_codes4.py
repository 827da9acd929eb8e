"""The affine 4-bit code kernels (csrc/mctq_codes4.hip: codes4_flat_kernel, codes4_rows_kernel<TI, 4 | 8>,
codes4_lastaxis_kernel) on every launch form and at edge values.

Expected values: oracle.mctq_oracle.fake_quant_affine(..., return_index=True) on the values as stored, widened to float32,
packed with oracle.mctq_oracle.pack4.  A NaN input has the code qmin (the CPU route's nan_to_num(nan=qmin)): the
oracle's numpy maximum would propagate the NaN, so qmin is substituted there.  +-inf and huge finite values go through the
oracle's float arithmetic unchanged -- its clamp answers them.  Bar: equality byte for byte on EVERY element: no mask, no
tolerance.  Raw calls write into the middle of a frame of 0xA5 bytes, 64 guard bytes on each side, which must keep their
value; inside the frame each output byte starts as the complement of its expected value, so an unwritten byte shows.
Every successful call must advance mctq_launch_count by exactly one and leave the launch note of the kernel it names.
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
VEC = {"float32": 4, "float16": 8, "bfloat16": 8}            # elements of a lane vector: one 16-byte load
THREADS = 256                                                # kThreads
FLAT_U = 8                                                   # kC4U: lane vectors per lane in the flat and last-axis kernels

# (scale, zero_point, qmin, qmax): the zero point at both ends of either domain, domains narrower than 4 bits, a step
# with an inexact reciprocal, and one so large that only the saturating ends of float32 / bfloat16 leave the zero point
PARAMS = ((0.25, 0, -8, 7), (0.2, 7, 0, 15), (0.3, -8, -8, 7), (0.0123, 15, 0, 15), (1.7 / 7, 0, 0, 7), (0.5, 3, -4, 3),
          (1e30, -1, -8, 7))
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


def _note(shape, dt, u):
    return f"{shape}<AffineCodesOp,in{16 // VEC[dt]}B,out1B,U={u},NT=1>"


def _store(x32, dt):
    """float32 values -> (device tensor of storage type dt, 16-byte aligned; the values it holds, widened to float32)."""
    x = _dev(np.asarray(x32, dtype=np.float32)).to(getattr(torch, dt))
    assert x.data_ptr() % 16 == 0
    return x, x.float().cpu().numpy()


def _want_codes(x_np, scales, zps, qmin, qmax, axis=None):
    """The oracle's clamp index of every element; NaN -> qmin."""
    from oracle import mctq_oracle as O
    with np.errstate(invalid="ignore"):                       # the NaN elements' cast, replaced in the next line
        _, idx = O.fake_quant_affine(x_np, scales, zps, qmin, qmax, axis=axis, return_index=True)
    idx = np.where(np.isnan(x_np), qmin, idx)
    assert idx.min() >= qmin and idx.max() <= qmax
    return idx


def _unpack(packed):
    """bytes -> nibbles in storage order (0 .. 15)."""
    b = np.asarray(packed, dtype=np.uint8).reshape(-1)
    return np.stack((b & 0xF, b >> 4), axis=1).reshape(-1)


def _assert_bytes(got, want_idx, x_np, what):
    from oracle import mctq_oracle as O
    want = O.pack4(want_idx)
    assert got.shape == want.shape, f"{what}: {got.shape} bytes, expected {want.shape}"
    if np.array_equal(got, want):
        return
    g, w = _unpack(got), _unpack(want)
    bad = np.flatnonzero(g != w)
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.size} of {w.size} codes differ, first at element {i}: x={x_np.reshape(-1)[i]!r} "
                         f"got nibble {int(g[i])} want {int(w[i])}")


class _Frame:
    """n / 2 output bytes in the middle of a 0xA5 frame; the bytes inside start as the complement of ``want_idx`` packed
    (``fill`` instead when there is nothing to expect)."""

    def __init__(self, want_idx=None, nbytes=None, fill=0x3C):
        from oracle import mctq_oracle as O
        inside = np.full(nbytes, fill, np.uint8) if want_idx is None else ~O.pack4(want_idx)
        self.inside = inside
        self.nb = inside.size
        self.buf = torch.full((self.nb + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.y = self.buf[GUARD:GUARD + self.nb]
        self.y.copy_(_dev(inside))
        assert (self.buf.data_ptr() + GUARD) % 4 == 0

    def ptr(self, off=0):
        return self.buf.data_ptr() + GUARD + off

    def result(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        edge = np.concatenate([b[:GUARD], b[GUARD + self.nb:]])
        assert edge.size == 2 * GUARD and np.all(edge == GUARD_BYTE), f"{what}: wrote outside its {self.nb} bytes"
        return b[GUARD:GUARD + self.nb]

    def untouched(self, what):
        assert np.array_equal(self.result(what), self.inside), f"{what}: wrote into the output"


def _code4(qmin):
    from mct_quantizers_amd.hip import native
    return native.CODE_I4 if qmin < 0 else native.CODE_U4


def _code8(qmin):
    from mct_quantizers_amd.hip import native
    return (native.CODE_I8, torch.int8) if qmin < 0 else (native.CODE_U8, torch.uint8)


def _run_tensor(lib, xd, x_np, dt, prm, what):
    """One per-tensor 4-bit call on the framed output, compared with the oracle.  Returns (nibbles, launch note)."""
    from mct_quantizers_amd.hip import native
    scale, zp, qmin, qmax = prm
    want = _want_codes(x_np, np.float32(scale), zp, qmin, qmax)
    fr = _Frame(want)
    count = native.launch_count()
    rc = lib.mctq_fq_codes_per_tensor(xd.data_ptr(), fr.ptr(), x_np.size, DT_CODE[dt], _code4(qmin), float(scale), zp, qmin,
                                      qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    got = fr.result(f"{what} [{text}]")
    _assert_bytes(got, want, x_np, f"{what} [{text}]")
    return _unpack(got), text


def _run_channels(lib, xd, x_np, dt, scales, zps, qmin, qmax, what, null_zps=False):
    """One per-channel 4-bit call ([outer, C, inner] = x_np.shape) on the framed output, compared with the oracle."""
    from mct_quantizers_amd.hip import native
    outer, C, inner = x_np.shape
    scales = np.asarray(scales, dtype=np.float32)
    zps = np.asarray(zps, dtype=np.int32)
    want = _want_codes(x_np, scales, zps, qmin, qmax, axis=1)
    fr = _Frame(want)
    s_d, z_d = _dev(scales), _dev(zps)
    count = native.launch_count()
    rc = lib.mctq_fq_codes_per_channel(xd.data_ptr(), fr.ptr(), outer, C, inner, DT_CODE[dt], _code4(qmin), s_d.data_ptr(),
                                       None if null_zps else z_d.data_ptr(), qmin, qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    got = fr.result(f"{what} [{text}]")
    _assert_bytes(got, want, x_np, f"{what} [{text}]")
    return _unpack(got), text


def _codes8_tensor(lib, xd, n, dt, prm):
    scale, zp, qmin, qmax = prm
    code, tdt = _code8(qmin)
    y = torch.empty(n, dtype=tdt, device="cuda")
    rc = lib.mctq_fq_codes_per_tensor(xd.data_ptr(), y.data_ptr(), n, DT_CODE[dt], code, float(scale), zp, qmin, qmax,
                                      _stream())
    assert rc == 0, lib.mctq_last_error()
    return y.cpu().numpy().astype(np.int64).reshape(-1) & 0xF


def _codes8_channels(lib, xd, shape, dt, scales, zps, qmin, qmax):
    code, tdt = _code8(qmin)
    y = torch.empty(shape, dtype=tdt, device="cuda")
    s_d, z_d = _dev(np.asarray(scales, dtype=np.float32)), _dev(np.asarray(zps, dtype=np.int32))
    rc = lib.mctq_fq_codes_per_channel(xd.data_ptr(), y.data_ptr(), *shape, DT_CODE[dt], code, s_d.data_ptr(), z_d.data_ptr(),
                                       qmin, qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    return y.cpu().numpy().astype(np.int64).reshape(-1) & 0xF


# ------------------------------------------------------------------------------------------------
# (a) value sweep through each of the three kernels
# ------------------------------------------------------------------------------------------------

def _grid_values(prm):
    """k s, (k + 1/2) s and its two float32 neighbours, for every k from three below the domain to three above it."""
    scale, zp, qmin, qmax = prm
    s = np.float32(scale)
    k = np.arange(qmin - 3 - zp, qmax + 3 - zp + 1).astype(np.float32)
    half = ((k + np.float32(0.5)) * s).astype(np.float32)
    return np.concatenate([(k * s).astype(np.float32), half, np.nextafter(half, np.float32(-np.inf)),
                           np.nextafter(half, np.float32(np.inf))]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sweep(dt):
    """(device tensor, stored values as float32): every bit pattern of the 16-bit types; for float32 every exponent x
    {mantissa 0, 1, 2, 0x3fffff, 0x400000, 0x7ffffe, 0x7fffff and 40 seeded random ones} x both signs (denormals, +-inf and
    NaN payloads among them) and the ties, steps and neighbours of every grid of PARAMS.  Padded with zeros to whole
    8192-element blocks."""
    if dt == "float32":
        rng = np.random.default_rng(4)
        mant = np.concatenate([np.asarray([0, 1, 2, 0x3fffff, 0x400000, 0x7ffffe, 0x7fffff], dtype=np.uint32),
                               rng.integers(0, 1 << 23, size=40).astype(np.uint32)])
        expo = np.arange(256, dtype=np.uint32) << 23
        pos = (expo[:, None] | mant[None, :]).reshape(-1)
        bits = np.concatenate([pos, pos | np.uint32(1 << 31)]).astype(np.uint32)
        x = np.concatenate([bits.view(np.float32)] + [_grid_values(p) for p in PARAMS])
        x = np.concatenate([x, np.zeros(-x.size % 8192, np.float32)])
        xd = _dev(x)
    else:
        bits = np.arange(1 << 16, dtype=np.uint16)
        xd = _dev(bits.view(np.int16)).view(getattr(torch, dt))
        assert np.array_equal(xd.view(torch.int16).cpu().numpy().view(np.uint16), bits)
        x = xd.float().cpu().numpy()
    assert x.size % 8192 == 0 and xd.data_ptr() % 16 == 0
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    x.setflags(write=False)
    return xd, x


def _reachable(dt, prm):
    """The codes the sweep must produce under ``prm``: the whole domain -- a sweep that saturated everything could not pass.
    One pair cannot give it: no finite float16 (|x| <= 65504) reaches half a step of 1e30, so there only 0 -> z,
    -inf / NaN -> qmin and +inf -> qmax exist."""
    scale, zp, qmin, qmax = prm
    if dt == "float16" and scale > 2 * 65504:
        return {qmin, min(max(zp, qmin), qmax), qmax}
    return set(range(qmin, qmax + 1))


@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_flat_kernel(lib, dt):
    xd, x = _sweep(dt)
    assert x.size // VEC[dt] > THREADS * FLAT_U                          # more than one block
    for prm in PARAMS:
        what = f"flat {dt} {prm}"
        got, text = _run_tensor(lib, xd, x, dt, prm, what)
        assert text == _note("codes4_flat_kernel", dt, FLAT_U), text
        want = _want_codes(x, np.float32(prm[0]), prm[1], prm[2], prm[3])
        assert set(np.unique(want).tolist()) == _reachable(dt, prm), (what, np.unique(want))
        assert np.array_equal(_codes8_tensor(lib, xd, x.size, dt, prm), got), f"{what}: 8-bit codes & 0xF differ"


def _channel_sets(sets, C):
    """Per-channel tables cycling ``sets``; every (qmin, qmax) among them is launched once with all of the tables."""
    scales = [sets[c % len(sets)][0] for c in range(C)]
    zps = [sets[c % len(sets)][1] for c in range(C)]
    domains = sorted({(p[2], p[3]) for p in sets})
    return scales, zps, domains


@pytest.mark.parametrize("sets", [SIGNED, UNSIGNED], ids=["signed", "unsigned"])
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_rows_kernel(lib, dt, sets):
    """[2, C, n]: every row is the whole value vector, C = one channel per parameter set, so that row % channels wraps.
    Rows of whole 8192-element blocks: waste(8) == waste(4) == 0 -> U = 8, several tiles."""
    xd1, x1 = _sweep(dt)
    C = len(sets)
    x = np.ascontiguousarray(np.broadcast_to(x1, (2, C, x1.size)))
    xd = xd1.repeat(2 * C)
    assert xd.data_ptr() % 16 == 0
    scales, zps, domains = _channel_sets(sets, C)
    for qmin, qmax in domains:
        what = f"rows {dt} {x.shape} [{qmin}, {qmax}]"
        got, text = _run_channels(lib, xd, x, dt, scales, zps, qmin, qmax, what)
        assert text == _note("codes4_rows_kernel", dt, 8), text
        want = _want_codes(x, np.float32(scales), zps, qmin, qmax, axis=1)
        assert set(np.unique(want).tolist()) == set(range(qmin, qmax + 1)), (what, np.unique(want))
        assert np.array_equal(_codes8_channels(lib, xd, x.shape, dt, scales, zps, qmin, qmax), got), \
            f"{what}: 8-bit codes & 0xF differ"


@pytest.mark.parametrize("sets", [SIGNED, UNSIGNED], ids=["signed", "unsigned"])
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_lastaxis_kernel(lib, dt, sets):
    """[n, 8, 1]: every column is the whole value vector, the 8 channels cycle the parameter sets."""
    xd1, x1 = _sweep(dt)
    C = 8
    x = np.ascontiguousarray(np.broadcast_to(x1[:, None, None], (x1.size, C, 1)))
    xd = xd1.repeat_interleave(C)
    assert xd.data_ptr() % 16 == 0
    scales, zps, domains = _channel_sets(sets, C)
    for qmin, qmax in domains:
        what = f"lastaxis {dt} {x.shape} [{qmin}, {qmax}]"
        got, text = _run_channels(lib, xd, x, dt, scales, zps, qmin, qmax, what)
        assert text == _note("codes4_lastaxis_kernel", dt, FLAT_U), text
        want = _want_codes(x, np.float32(scales), zps, qmin, qmax, axis=1)
        assert set(np.unique(want).tolist()) == set(range(qmin, qmax + 1)), (what, np.unique(want))
        assert np.array_equal(_codes8_channels(lib, xd, x.shape, dt, scales, zps, qmin, qmax), got), \
            f"{what}: 8-bit codes & 0xF differ"


# ------------------------------------------------------------------------------------------------
# (b) launch geometry.  The shapes follow from the launchers' arithmetic in mctq_codes4.hip as it stands; a change there
#     needs new shapes here (the asserted U and the block counts in the comments say what each one is for).
#     A lane vector is 16 bytes of input: VEC = 4 float32 / 8 half elements.  kThreads = 256, kC4U = 8.
# ------------------------------------------------------------------------------------------------

def _tie_heavy(rng, shape, s_b, zp_b, qmin, qmax):
    """Inputs dense in round-half ties and clamp edges of their own channel's grid (as tests/test_gpu_parity.py)."""
    n = int(np.prod(shape))
    x = (rng.standard_normal(n).astype(np.float32).reshape(shape) * s_b * np.float32(0.4 * (qmax - qmin)))
    k = rng.integers(qmin - 2, qmax + 3, size=shape).astype(np.float32) - zp_b
    kind = rng.integers(0, 6, size=shape)
    x = np.where(kind == 0, (k + np.float32(0.5)) * s_b, x)
    x = np.where(kind == 1, k * s_b, x)
    return x.astype(np.float32)


def _channel_case(rng, shape, dt, qmin, qmax):
    """Tie-heavy [outer, C, inner] input of storage type dt with a scale and a zero point (anywhere in the domain) per channel."""
    C = shape[1]
    scales = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
    zps = rng.integers(qmin, qmax + 1, size=C).astype(np.int32)
    x32 = _tie_heavy(rng, shape, scales.reshape(1, C, 1), zps.reshape(1, C, 1).astype(np.float32), qmin, qmax)
    xd, x = _store(x32.reshape(-1), dt)
    return xd, x.reshape(shape), scales, zps


# codes4_per_tensor: nv = n / VEC lane vectors, blocks = ceil(nv / (kThreads * kC4U)) = ceil(nv / 2048): a block covers
# B = 2048 * VEC elements.  n = 8: one block with 2 (float32) / 1 (halves) vectors; B: one exactly full block;
# B + 8: a second block holding 2 / 1 vectors; 3 B - 8: three blocks, the last 2 / 1 vectors short.
@pytest.mark.parametrize("kind", ["8", "B", "B+8", "3B-8"])
@pytest.mark.parametrize("dt", DTYPES)
def test_flat_kernel_geometry(lib, dt, kind):
    B = THREADS * FLAT_U * VEC[dt]
    assert B == {4: 8192, 8: 16384}[VEC[dt]]
    n = {"8": 8, "B": B, "B+8": B + 8, "3B-8": 3 * B - 8}[kind]
    rng = np.random.default_rng([n, DT_CODE[dt]])
    for prm in ((0.0371, 5, 0, 15), (0.113, -3, -8, 7)):
        x32 = _tie_heavy(rng, (n,), np.float32(prm[0]), np.float32(prm[1]), prm[2], prm[3])
        xd, x = _store(x32, dt)
        _, text = _run_tensor(lib, xd, x, dt, prm, f"flat {dt} n={n} {prm}")
        assert text == _note("codes4_flat_kernel", dt, FLAT_U), text


# codes4_per_channel, inner % 8 == 0: innerv = inner / VEC; waste(u) = (256 u - innerv % (256 u)) % (256 u) idle vector slots
# in a row's last tile; U = 4 if waste(4) < waste(8) else 8; tiles = ceil(innerv / (256 U)); grid = rows * tiles.
#   innerv    waste(4)  waste(8)   U  tiles  last tile        float32 inner   halves inner
#   2 / 1       1022/3   2046/7    4    1    2 / 1 vectors          8              8
#   1280         768      768      8    1    1280 of 2048         5120             -
#   1025        1023     1023      8    1    1025 of 2048           -            8200
#   2050        1022     2046      4    3    2 vectors            8200          16400
#   3328         768      768      8    2    1280 of 2048        13312          26624
# outer x C = 2 x 3: six rows, so that row % channels wraps and blockIdx.x / tiles, blockIdx.x - row * tiles see tiles > 1.
ROWS_CASES = {"float32": ((8, 4), (5120, 8), (8200, 4), (13312, 8)),
              "float16": ((8, 4), (8200, 8), (16400, 4), (26624, 8)),
              "bfloat16": ((8, 4), (8200, 8), (16400, 4), (26624, 8))}


@pytest.mark.parametrize("dt,inner,u", [(dt, inner, u) for dt in DTYPES for inner, u in ROWS_CASES[dt]],
                         ids=lambda v: str(v))
def test_rows_kernel_geometry(lib, dt, inner, u):
    shape = (2, 3, inner)
    rng = np.random.default_rng([inner, DT_CODE[dt]])
    for qmin, qmax in ((-8, 7), (0, 15)):
        xd, x, scales, zps = _channel_case(rng, shape, dt, qmin, qmax)
        _, text = _run_channels(lib, xd, x, dt, scales, zps, qmin, qmax, f"rows {dt} {shape} [{qmin}, {qmax}]")
        assert text == _note("codes4_rows_kernel", dt, u), text


@pytest.mark.parametrize("dt", DTYPES)
def test_null_zero_points_equal_a_table_of_zeros(lib, dt):
    """zero_points == NULL (the symmetric quantizers' call): the oracle's result for zero points of 0, in both per-channel
    kernels."""
    rng = np.random.default_rng(11)
    for shape, kernel, u in (((2, 3, 8200), "codes4_rows_kernel", 4 if dt == "float32" else 8),      # see ROWS_CASES
                             ((77, 24, 1), "codes4_lastaxis_kernel", FLAT_U)):
        C = shape[1]
        scales = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
        zeros = np.zeros(C, np.int32)
        x32 = _tie_heavy(rng, shape, scales.reshape(1, C, 1), np.float32(0), -8, 7)
        xd, x = _store(x32.reshape(-1), dt)
        _, text = _run_channels(lib, xd, x.reshape(shape), dt, scales, zeros, -8, 7, f"NULL zero points {dt} {shape}",
                                null_zps=True)
        assert text == _note(kernel, dt, u), text


# codes4_per_channel, inner == 1 and C % 8 == 0: vc = C / VEC vectors per row; k = the candidate in [ceil(2048 / vc),
# ceil(2048 / vc) + 16) with the least (256 - (k vc) % 256) % 256 * 4096 / (k vc) (first of equals); bps = ceil(k vc / 256)
# blocks cover k rows, the lanes past k vc idle (the `ro >= k` cut); every lane steps kC4U = 8 times down k rows: a group is
# 8 k rows, grid = bps * ceil(outer / (8 k)).
#   float32:   C    vc     k   bps  idle lanes  group   outer -> groups
#              8     2  1024     8       0       8192    8197: one full, one of 5 rows
#             40    10   220     9     104       1760    3523: two full, one of 3 rows
#           1032   258    23    24     210        184     185: one full, one of 1 row
#          16384  4096     1    16       0          8      17: two full, one of 1 row
#   halves:    8     1  2048     8       0      16384   16389: one full, one of 5 rows
#             40     5   425     9     179       3400    6803: two full, one of 3 rows
#           1032   129    31    16      97        248     249: one full, one of 1 row
#          16384  2048     1     8       0          8      17: two full, one of 1 row
LASTAXIS_CASES = {"float32": ((8, 8197), (40, 3523), (1032, 185), (16384, 17)),
                  "float16": ((8, 16389), (40, 6803), (1032, 249), (16384, 17)),
                  "bfloat16": ((8, 16389), (40, 6803), (1032, 249), (16384, 17))}


@pytest.mark.parametrize("dt,C,outer", [(dt, C, outer) for dt in DTYPES for C, outer in LASTAXIS_CASES[dt]],
                         ids=lambda v: str(v))
def test_lastaxis_kernel_geometry(lib, dt, C, outer):
    shape = (outer, C, 1)
    rng = np.random.default_rng([outer, C, DT_CODE[dt]])
    for qmin, qmax in ((-8, 7), (0, 15)):
        xd, x, scales, zps = _channel_case(rng, shape, dt, qmin, qmax)
        _, text = _run_channels(lib, xd, x, dt, scales, zps, qmin, qmax, f"lastaxis {dt} {shape} [{qmin}, {qmax}]")
        assert text == _note("codes4_lastaxis_kernel", dt, FLAT_U), text


# ------------------------------------------------------------------------------------------------
# (c) refusals and empties through the raw entry points: nothing launched, nothing noted, nothing written.  Every call
#     has valid device pointers with room for the call as if it were accepted.
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
def test_refused_and_empty_calls_launch_nothing(lib, dt):
    from mct_quantizers_amd.hip import native
    E = native.MCTQ_E_ARG
    n = 96                                                            # the accepted size: [2, 6, 8] or [12, 8, 1]
    xb = torch.zeros(n + 16, dtype=getattr(torch, dt), device="cuda")  # room for x moved by 4 bytes
    s_d, z_d = _dev(np.full(16, 0.25, np.float32)), _dev(np.zeros(16, np.int32))
    fr = _Frame(nbytes=n // 2)
    x, y, st = xb.data_ptr(), fr.ptr(), _stream()
    dtc, c4 = DT_CODE[dt], native.CODE_I4
    assert x % 16 == 0 and y % 4 == 0
    lib.mctq_fq_codes_per_tensor(x, fr.ptr(), n, dtc, c4, 0.25, 0, -8, 7, st)       # a note of this file's own to hold on to
    fr.y.copy_(_dev(fr.inside))
    torch.cuda.synchronize()
    count, text = native.launch_count(), native.last_launch()
    assert text == _note("codes4_flat_kernel", dt, FLAT_U)

    def per_tensor(xp, yp, nn):
        return lib.mctq_fq_codes_per_tensor(xp, yp, nn, dtc, c4, 0.25, 0, -8, 7, st)

    def per_channel(xp, yp, o, c, i):
        return lib.mctq_fq_codes_per_channel(xp, yp, o, c, i, dtc, c4, s_d.data_ptr(), z_d.data_ptr(), -8, 7, st)

    calls = [("n == 0", 0, lambda: per_tensor(x, y, 0)),
             ("outer == 0", 0, lambda: per_channel(x, y, 0, 6, 8)),
             ("outer == 0, last axis", 0, lambda: per_channel(x, y, 0, 8, 1)),
             ("x + 4 bytes, per tensor", E, lambda: per_tensor(x + 4, y, n)),
             ("x + 4 bytes, rows", E, lambda: per_channel(x + 4, y, 2, 6, 8)),
             ("x + 4 bytes, last axis", E, lambda: per_channel(x + 4, y, 12, 8, 1)),
             ("codes + 1 byte, per tensor", E, lambda: per_tensor(x, y + 1, n)),
             ("codes + 2 bytes, per tensor", E, lambda: per_tensor(x, y + 2, n)),
             ("codes + 1 byte, rows", E, lambda: per_channel(x, y + 1, 2, 6, 8)),
             ("codes + 2 bytes, rows", E, lambda: per_channel(x, y + 2, 2, 6, 8)),
             ("codes + 1 byte, last axis", E, lambda: per_channel(x, y + 1, 12, 8, 1)),
             ("codes + 2 bytes, last axis", E, lambda: per_channel(x, y + 2, 12, 8, 1)),
             ("inner == 1, C % 8 != 0", E, lambda: per_channel(x, y, 8, 12, 1)),
             ("inner == 1, C == 4", E, lambda: per_channel(x, y, 24, 4, 1))]
    for what, want_rc, call in calls:
        assert call() == want_rc, (what, lib.mctq_last_error())
        assert native.launch_count() == count and native.last_launch() == text, what
        fr.untouched(what)


# ------------------------------------------------------------------------------------------------
# (d) through Python: ops.fq_codes(packed4=True) and quantize_to_codes(packed4=True) on a channels-last 4-D tensor
# ------------------------------------------------------------------------------------------------

CL_SHAPE = (2, 1032, 5, 19)     # storage order [2, 5, 19, 1032]: 190 rows of 1032 channels -- more than one last-axis group
                                # (184 / 248 rows, see above) and 196080 elements: 24 / 12 blocks of the flat kernel


def _storage_order(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dt", DTYPES)
def test_python_routes_on_a_channels_last_tensor(lib, dt):
    import warnings
    import mct_quantizers_amd as mq
    from mct_quantizers_amd.hip import native, ops
    from oracle import oracle_call, mctq_oracle as O
    Q = mq.pytorch_quantizers
    tdt = getattr(torch, dt)
    C = CL_SHAPE[1]
    rng = np.random.default_rng([3, DT_CODE[dt]])
    scales = rng.uniform(0.05, 0.5, size=C).astype(np.float32)
    zps = rng.integers(0, 16, size=C).astype(np.int32)
    x32 = _tie_heavy(rng, CL_SHAPE, scales.reshape(1, C, 1, 1), zps.reshape(1, C, 1, 1).astype(np.float32), 0, 15)
    x_cpu = torch.from_numpy(x32).to(tdt).contiguous(memory_format=torch.channels_last)
    x = x_cpu.cuda()
    assert x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    x_np = x_cpu.float().numpy()
    s_d, z_d = _dev(scales), _dev(zps)

    def launched(f, kernel):
        count = native.launch_count()
        out = f()
        assert native.launch_count() == count + 1 and native.last_launch() == _note(kernel, dt, FLAT_U), native.last_launch()
        return out

    # ops.fq_codes, per channel on axis 1 (the last-axis kernel) and per tensor (the flat kernel)
    got = launched(lambda: ops.fq_codes(x, s_d, z_d, 1, 0, 15, packed4=True), "codes4_lastaxis_kernel")
    want = _want_codes(x_np, scales, zps, 0, 15, axis=1)
    assert got.dtype == torch.uint8 and got.numel() == x.numel() // 2
    _assert_bytes(got.cpu().numpy().reshape(-1), _storage_order(want), _storage_order(x_np), f"fq_codes axis 1 {dt}")
    assert torch.equal(ops.fq_codes(x_cpu, torch.from_numpy(scales), torch.from_numpy(zps), 1, 0, 15, packed4=True).reshape(-1),
                       got.cpu().reshape(-1))
    s0, z0 = float(scales[0]), int(zps[0])
    got = launched(lambda: ops.fq_codes(x, None, None, None, 0, 15, s0, z0, packed4=True), "codes4_flat_kernel")
    want = _want_codes(x_np, scales[0], z0, 0, 15)
    _assert_bytes(got.cpu().numpy().reshape(-1), _storage_order(want), _storage_order(x_np), f"fq_codes per tensor {dt}")
    assert torch.equal(ops.fq_codes(x_cpu, None, None, None, 0, 15, s0, z0, packed4=True).reshape(-1), got.cpu().reshape(-1))

    # the quantizer classes: codes, the CPU route, the oracle, and dequantization == the fake-quantized tensor
    hi = rng.uniform(0.5, 3.0, C)
    lo = -rng.uniform(0.5, 3.0, C)
    cases = (("WeightsSymmetricInferableQuantizer", "codes4_lastaxis_kernel",
              dict(num_bits=4, threshold=[float(v) for v in hi], per_channel=True, channel_axis=1)),
             ("WeightsUniformInferableQuantizer", "codes4_lastaxis_kernel",
              dict(num_bits=4, min_range=[float(v) for v in lo], max_range=[float(v) for v in hi], per_channel=True,
                   channel_axis=1)),
             ("ActivationUniformInferableQuantizer", "codes4_flat_kernel", dict(num_bits=4, min_range=[-1.0], max_range=[2.0])),
             ("ActivationSymmetricInferableQuantizer", "codes4_flat_kernel", dict(num_bits=3, threshold=[1.7], signed=True)))
    for name, kernel, kw in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            q = getattr(Q, name)(**kw)
        packed, s, z = launched(lambda: q.quantize_to_codes(x, packed4=True), kernel)
        _, idx = oracle_call(name, kw, x_np, return_index=True)
        _assert_bytes(packed.cpu().numpy().reshape(-1), _storage_order(idx), _storage_order(x_np), f"{name} {dt}")
        assert torch.equal(q.quantize_to_codes(x_cpu, packed4=True)[0].reshape(-1), packed.cpu().reshape(-1)), name
        n, _, h, w = CL_SHAPE
        codes = ops.unpack4(packed.cpu(), q.min_quantized_domain < 0, (n, h, w, C)).permute(0, 3, 1, 2)
        if torch.is_tensor(s):
            s_b, z_b = s.cpu().reshape(1, C, 1, 1), z.cpu().reshape(1, C, 1, 1).float()
        else:
            s_b, z_b = torch.tensor(s, dtype=torch.float64).to(torch.float32), float(z)
        deq = ((codes.float() - z_b) * s_b).to(tdt)
        y = q(x).cpu()
        assert y.shape == deq.shape and torch.equal(_bits(deq), _bits(y)), f"{name} {dt}: dequantized codes != fake-quant"
