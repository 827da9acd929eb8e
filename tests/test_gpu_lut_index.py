"""The LUT index-code and decode kernels on every launch route: mctq_lut_codes_per_tensor / _per_channel with MCTQ_CODE_U8
(LutIndexTableOp and LutIndexOp on the shared launchers of csrc/mctq_kernels.hpp with a 1-byte output) and MCTQ_CODE_U4
(csrc/mctq_lut_codes4.hip), mctq_lut_decode_per_tensor / _per_channel (csrc/mctq_lut_decode.hip), through the raw C ABI.

The case tables, the re-derived routes and the expected values are those of tests/test_lut_index_cases.py (the oracle's indices on
the values as stored; the decode in numpy float32 from the codes themselves, a code >= n_lut giving 0.0 * thr).  Bar: equality
byte for byte (codes) or bit for bit (float32) on EVERY element: no mask, no tolerance.  Outputs sit in the middle of a frame of
0xA5 bytes, 64 guard bytes on each side, which must keep their value; inside the frame every output byte starts as the complement
of its expected value, so an unwritten byte shows.  Every successful call must advance mctq_launch_count by exactly one and leave
exactly the launch note the case names; every refused call returns MCTQ_E_ARG, launches nothing and leaves the frame untouched.
"""
import numpy as np
import pytest
import torch

from test_lut_index_cases import (CMAX, CMIN, DEC_BAD_LUTS, DEC_LUTS, DIVISORS, DT_CODE, DTYPES, ENTRIES, F32, LUTS, MULT, NIBBLE_LUTS,
                                  OP_NAME, OP_U, OPS, T, VEC, Case, case_shape, dec_cases, dec_note, decode_inputs, enc4_cases,
                                  enc8_cases, enc_note, encode_inputs, first_indices, index_table, luts_of, note, rows_u, sweep,
                                  tensor_divisor, value_table, want_decode, want_indices)

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # (a copy: the shared expectations are read-only)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _shifted(xd, off):
    """The same elements ``off`` elements past a 16-byte boundary."""
    buf = torch.zeros(xd.numel() + 16, dtype=xd.dtype, device="cuda")
    x = buf[off:off + xd.numel()]
    x.copy_(xd.reshape(-1))
    assert x.data_ptr() % 16 == (off * xd.element_size()) % 16
    return x


def _store(x, dt, off=0):
    """float32 values a storage type holds exactly -> device tensor of that type, ``off`` elements past a 16-byte boundary."""
    xd = _shifted(_dev(np.ascontiguousarray(x, dtype=F32).reshape(-1)).to(getattr(torch, dt)), off)
    assert np.array_equal(xd.float().cpu().numpy(), np.asarray(x, dtype=F32).reshape(-1), equal_nan=True)
    return xd


_BOOKS = {}


def _book(lut_name):
    """Device copies of a codebook, its index table and its value table (None without a table)."""
    if lut_name not in _BOOKS:
        it, vt = index_table(lut_name), value_table(lut_name)
        _BOOKS[lut_name] = (_dev(np.asarray(LUTS[lut_name], dtype=F32)), None if it is None else _dev(it), None if vt is None else _dev(vt))
    return _BOOKS[lut_name]


def _table_args(lut_name, op):
    lut_d, itab, _ = _book(lut_name)
    if op == "table":
        assert itab is not None
        return lut_d.data_ptr(), len(LUTS[lut_name]), itab.data_ptr(), ENTRIES
    return lut_d.data_ptr(), len(LUTS[lut_name]), None, 0


class _Frame:
    """``want`` output bytes in the middle of a 0xA5 frame, ``yoff`` bytes past a 16-byte boundary; the bytes inside start as the
    complement of ``want`` (``fill`` instead when there is nothing to expect)."""

    def __init__(self, want=None, nbytes=None, fill=0x3C, yoff=0):
        inside = np.full(nbytes, fill, np.uint8) if want is None else ~np.ascontiguousarray(want).reshape(-1).view(np.uint8)
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


def _launched(lib, count, want_note, what):
    from mct_quantizers_amd.hip import native
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == want_note, f"{what}: took {text}, expected {want_note}"
    return text


def _run_encode(lib, case, dt, op, x, thr, eps, want, packed, what):
    """One encode call on the framed output: the oracle's bytes, one launch, the whole note.  Returns the codes (unpacked)."""
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    want_flat = np.asarray(want).reshape(-1)
    want_bytes = O.pack4(want_flat) if packed else want_flat.astype(np.uint8)
    xd = _store(x, dt, case.xoff)
    fr = _Frame(want_bytes, yoff=case.yoff)
    code = native.CODE_U4 if packed else native.CODE_U8
    books = _table_args(case.lut, op)
    want_note = enc_note(case, dt, op)
    count = native.launch_count()
    if case.kind == "tensor":
        div = float(tensor_divisor(thr, eps, dt if case.step else "float32"))
        rc = lib.mctq_lut_codes_per_tensor(xd.data_ptr(), fr.ptr(), x.size, DT_CODE[dt], code, DT_CODE[dt] if case.step else 0, div,
                                           *books, MULT, CMIN, CMAX, _stream())
    else:
        outer, C, inner = x.shape
        t_d = _shifted(_dev(np.asarray(thr, dtype=F32)), case.toff)
        assert t_d.data_ptr() % 16 == 4 * case.toff
        rc = lib.mctq_lut_codes_per_channel(xd.data_ptr(), fr.ptr(), outer, C, inner, DT_CODE[dt], code, t_d.data_ptr(), eps, *books,
                                            MULT, CMIN, CMAX, _stream())
    assert rc == 0, (what, lib.mctq_last_error())
    text = _launched(lib, count, want_note, what)
    got = fr.result(f"{what} [{text}]")
    if not np.array_equal(got, want_bytes):
        bad = np.flatnonzero(got != want_bytes)
        i = int(bad[0])
        j = 2 * i if packed else i
        raise AssertionError(f"{what} [{text}]: {bad.size} of {want_bytes.size} code bytes differ, first at byte {i}: "
                             f"x={x.reshape(-1)[j:j + (2 if packed else 1)]!r} got {int(got[i]):#x} want {int(want_bytes[i]):#x}")
    return want_flat


def _same_bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)
    b = np.ascontiguousarray(b, dtype=F32).reshape(-1).view(np.uint32)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first at {int(bad[0])}: {a[bad[0]]:#x} vs {b[bad[0]]:#x}"


def _fake_quant(lib, x, thr, eps, lut_name, op):
    """The fake-quant kernel's float32 output for the same arguments: the value-table kernel under the table op, the literal scan
    under the literal op."""
    lut_d, _, vtab = _book(lut_name)
    xd = _store(x, "float32")
    y = torch.full((x.size,), 12345.0, dtype=torch.float32, device="cuda")
    book = (vtab.data_ptr(), ENTRIES) if op == "table" else (lut_d.data_ptr(), len(LUTS[lut_name]))
    if x.ndim == 1:
        f = lib.mctq_lutt_per_tensor_f32 if op == "table" else lib.mctq_lut_per_tensor_f32
        rc = f(xd.data_ptr(), y.data_ptr(), x.size, float(tensor_divisor(thr, eps)), float(F32(thr)), *book, MULT, CMIN, CMAX, _stream())
    else:
        f = lib.mctq_lutt_per_channel_f32 if op == "table" else lib.mctq_lut_per_channel_f32
        t_d = _dev(np.asarray(thr, dtype=F32))
        rc = f(xd.data_ptr(), y.data_ptr(), *x.shape, t_d.data_ptr(), eps, *book, MULT, CMIN, CMAX, _stream())
    assert rc == 0, lib.mctq_last_error()
    return y.cpu().numpy()


def _run_decode(lib, case, code, lut_name, codes, thr, want, what):
    """One decode call on the framed float32 output: bit equality, one launch, the whole note."""
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    cb = codes.reshape(-1).astype(np.uint8) if code == "u8" else O.pack4(codes)
    cd = _shifted(_dev(cb), case.xoff)
    fr = _Frame(np.ascontiguousarray(want, dtype=F32), yoff=case.yoff)
    lut_d = _book(lut_name)[0]
    cdt = native.CODE_U8 if code == "u8" else native.CODE_U4
    count = native.launch_count()
    if case.kind == "tensor":
        rc = lib.mctq_lut_decode_per_tensor(cd.data_ptr(), fr.ptr(), codes.size, cdt, lut_d.data_ptr(), len(LUTS[lut_name]), MULT,
                                            float(thr), _stream())
    else:
        t_d = _shifted(_dev(np.asarray(thr, dtype=F32)), case.toff)
        assert t_d.data_ptr() % 16 == 4 * case.toff
        rc = lib.mctq_lut_decode_per_channel(cd.data_ptr(), fr.ptr(), *codes.shape, cdt, lut_d.data_ptr(), len(LUTS[lut_name]), MULT,
                                             t_d.data_ptr(), _stream())
    assert rc == 0, (what, lib.mctq_last_error())
    text = _launched(lib, count, dec_note(case), what)
    got = fr.result(f"{what} [{text}]").view(np.uint32)
    want_w = np.ascontiguousarray(want, dtype=F32).reshape(-1).view(np.uint32)
    if not np.array_equal(got, want_w):
        bad = np.flatnonzero(got != want_w)
        i = int(bad[0])
        raise AssertionError(f"{what} [{text}]: {bad.size} of {want_w.size} words differ, first at element {i}: code "
                             f"{int(codes.reshape(-1)[i])} got {got[i:i + 1].view(F32)[0]!r} want {want_w[i:i + 1].view(F32)[0]!r}")


# ------------------------------------------------------------------------------------------------
# (a) value sweeps through every route, per storage type and op, at the smallest layout that takes the route.  Per tensor: every
#     divisor class.  Per channel: every channel holds the sweep of its OWN divisor and the table mixes 1.7, 2^70, 2^-70 and 1.0
#     with eps = 0 -- where a lane owns its channels (last axis, window) lanes of one wave disagree about the fast division.
#     float32: decode(encode(x)) equals the fake-quant kernel's output bit for bit, NaN and +-inf included.
# ------------------------------------------------------------------------------------------------

def _covers(idx, lut_name, dt, thr, what):
    """test_lut_index_cases.test_sweep_reaches_every_first_occurrence_index, on what this launch was asked for."""
    first, seen = first_indices(lut_name), set(np.asarray(idx).reshape(-1).tolist())
    big = not 2.0 ** -60 < thr < 2.0 ** 60
    if not big or dt == "float32" or (dt == "bfloat16" and thr > 1):
        assert seen == first, (what, sorted(first - seen))
    else:
        assert len(seen) >= min(3, len(first)), (what, sorted(seen))


def _padded(x, m):
    return np.concatenate([x, np.zeros(-x.size % m, F32)])


SWEEP_TENSOR = (("flat_kernel", False, 0), ("flat_scalar_kernel", False, 1), ("lut_codes4_flat_kernel", True, 0))


@pytest.mark.parametrize("route,packed,xoff", SWEEP_TENSOR, ids=[r[0] for r in SWEEP_TENSOR])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_per_tensor(lib, dt, op, route, packed, xoff):
    u, nt = (4, 1) if packed else (OP_U[op], 1) if route == "flat_kernel" else (1, 0)
    for lut_name in luts_of(op, NIBBLE_LUTS if packed else tuple(LUTS)):
        for dname, thr, eps in DIVISORS:
            for step in ((False, True) if dt != "float32" and thr < 2 else (False,)):
                what = f"{route} {dt} {op} {lut_name} d={dname}{' step_round' if step else ''}"
                x = sweep(float(tensor_divisor(thr, eps)), dt)
                x = _padded(x, 8) if packed else x
                case = Case("sweep", "tensor", x.shape, xoff, 0, 0, lut_name, route, u, nt, step)
                want = want_indices(x, lut_name, thr, eps, step_dtype=dt if step else "float32")
                if not step:
                    _covers(want, lut_name, dt, thr, what)
                _run_encode(lib, case, dt, op, x, thr, eps, want, packed, what)
                if dt == "float32":
                    dec = Case("sweep", "tensor", x.shape, 0, 0, 0, lut_name, f"lut_decode_kernel<{'u4' if packed else 'u8'},tensor>", 4, 1, False)
                    y = want_decode(want, lut_name, F32(thr))
                    _run_decode(lib, dec, "u4" if packed else "u8", lut_name, want, F32(thr), y, what + " decode")
                    _same_bits(y, _fake_quant(lib, x, thr, eps, lut_name, op), what + ": decode(encode(x)) vs the fake-quant kernel")


# route -> (packed, rows layout, C, x offset)
SWEEP_CHANNEL = {"rows_kernel": (False, True, 4, 0), "lastaxis_kernel": (False, False, 8, 0), "window_kernel<vector>": (False, False, 5, 0),
                 "window_kernel<scalar>": (False, False, 5, 1), "lut_codes4_rows_kernel": (True, True, 4, 0),
                 "lut_codes4_lastaxis_kernel": (True, False, 8, 0)}
MIXED = (1.7, 2.0 ** 70, 2.0 ** -70, 1.0)


@pytest.mark.parametrize("route", list(SWEEP_CHANNEL))
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_value_sweep_per_channel(lib, dt, op, route):
    """rows: [1, 4, 3112], a row the sweep of its channel twice over (389 / 778 lane vectors: at least 256); the others
    [1555, C, 1], a column the sweep of its channel: C = 8 a multiple of N for every type, C = 5 of none."""
    packed, rows, C, xoff = SWEEP_CHANNEL[route]
    N = VEC[dt]
    thr = np.asarray([MIXED[c % 4] for c in range(C)], dtype=F32)
    cols = [sweep(float(t), dt) for t in thr]
    if rows:
        x = np.stack([_padded(np.concatenate([c, c]), 8) for c in cols])[None]
        assert x.shape == (1, C, 3112) and x.shape[2] % N == 0 and x.shape[2] // N >= T
    else:
        x = np.ascontiguousarray(np.stack(cols, axis=1)[:, :, None])
        assert x.shape == (1555, C, 1) and (C % N == 0) == (C == 8)
    u = 4 if packed or route.startswith("window") else 2 if route == "lastaxis_kernel" else OP_U[op]
    for lut_name in luts_of(op, NIBBLE_LUTS if packed else tuple(LUTS)):
        what = f"{route} {dt} {op} {lut_name} {x.shape}"
        case = Case("sweep", "channel", x.shape, xoff, 0, 0, lut_name, route, u, 1, False)
        want = want_indices(x, lut_name, thr, 0.0, per_channel=True)
        for c in range(C):
            _covers(want[:, c], lut_name, dt, float(thr[c]), f"{what} channel {c}")
        _run_encode(lib, case, dt, op, x, thr, 0.0, want, packed, what)
        if dt == "float32":
            code = "u4" if packed else "u8"
            droute = f"lut_decode_rows_kernel<{code}>" if rows else f"lut_decode_kernel<{code},{'lastaxis' if C == 8 else 'ragged'}>"
            dec = Case("sweep", "channel", x.shape, 0, 0, 0, lut_name, droute, rows_u(x.shape[2] // (8 if packed else 4)) if rows else 4, 1, False)
            y = want_decode(want, lut_name, thr.reshape(1, C, 1))
            _run_decode(lib, dec, code, lut_name, want, thr, y, what + " decode")
            _same_bits(y, _fake_quant(lib, x, thr, 0.0, lut_name, op), what + ": decode(encode(x)) vs the fake-quant kernel")


# ------------------------------------------------------------------------------------------------
# (b), (c) encode geometry: the case tables of test_lut_index_cases.py (their shapes are checked against the launchers'
#     arithmetic there).  Per channel the thresholds hold 2^70 on channel 1: fast and IEEE divisors in one launch.
# ------------------------------------------------------------------------------------------------

def _enc_params(cases_of):
    return [pytest.param(dt, op, c, id=f"{dt}-{op}-{c.id}") for dt in DTYPES for op in OPS for c in cases_of(dt, op)]


@pytest.mark.parametrize("dt,op,case", _enc_params(enc8_cases))
def test_encode_u8_geometry(lib, dt, op, case):
    cus = _cus()
    x, thr, eps, want = encode_inputs(case, dt, cus)
    if case.shape is None:
        assert -(-x.size // T) > 32 * cus and case_shape(case, cus) == x.shape      # the grid-stride loop turns twice
    _run_encode(lib, case, dt, op, x, thr, eps, want, False, f"{dt} {op} {case.id} {x.shape}")


@pytest.mark.parametrize("dt,op,case", _enc_params(enc4_cases))
def test_encode_u4_geometry(lib, dt, op, case):
    x, thr, eps, want = encode_inputs(case, dt)
    _run_encode(lib, case, dt, op, x, thr, eps, want, True, f"{dt} {op} {case.id} {x.shape}")


# ------------------------------------------------------------------------------------------------
# (d) decode: codes drawn by a seeded generator, independent of any encoder; every route once per codebook, and again with a
#     tenth of the codes beyond the codebook (0.0 * thr: the zero padding of the LDS table).
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code,case", [pytest.param(code, c, id=f"{code}-{c.id}") for code in ("u8", "u4") for c in dec_cases(code)])
def test_decode_geometry(lib, code, case):
    cus = _cus()
    runs = [(name, False) for name in DEC_LUTS[code]] + [(name, True) for name in DEC_BAD_LUTS[code]]
    if case.shape is None:
        runs = [("l16", False), ("l16", True)]
        assert -(-case_shape(case, cus)[0] // T) > 32 * cus
    for lut_name, bad in runs:
        codes, thr, want = decode_inputs(case, lut_name, code, bad, cus)
        n_lut = len(LUTS[lut_name])
        if codes.size >= n_lut and not bad:                                         # every code value occurs (``bad``: it did before a
            assert set(range(n_lut)) <= set(codes.reshape(-1).tolist())             # tenth was replaced: decode_inputs asserts it)
        assert bad == bool((codes >= n_lut).any())
        _run_decode(lib, case, code, lut_name, codes, thr, want, f"decode {code} {case.id} {lut_name}{' + codes beyond it' if bad else ''}")


# ------------------------------------------------------------------------------------------------
# refusals and empties through the raw entry points: nothing launched, nothing noted, nothing written.  Every call has valid
# device pointers with room for the call as if it were accepted.
# ------------------------------------------------------------------------------------------------

def _check_calls(lib, fr, calls, count, text):
    from mct_quantizers_amd.hip import native
    for what, want_rc, call in calls:
        assert call() == want_rc, (what, lib.mctq_last_error())
        assert native.launch_count() == count and native.last_launch() == text, what
        fr.untouched(what)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_refused_and_empty_encodes_launch_nothing(lib, dt, op):
    from mct_quantizers_amd.hip import native
    E, U8, U4 = native.MCTQ_E_ARG, native.CODE_U8, native.CODE_U4
    N = VEC[dt]
    n = 192                                                            # the accepted size: [2, 12, 8], [24, 8, 1]
    xb = torch.zeros(n + 16, dtype=getattr(torch, dt), device="cuda")
    fr = _Frame(nbytes=n)
    x, y, st, dtc = xb.data_ptr(), fr.ptr(), _stream(), DT_CODE[dt]
    books = _table_args("l16", op)
    lut17 = _dev(np.arange(17, dtype=F32))
    books17 = (lut17.data_ptr(), 17) + books[2:]
    t_d = _dev(np.full(16, 1.5, F32))
    thr = t_d.data_ptr()

    def per_tensor(xp=x, yp=y, nn=n, code=U8, step=0, bk=books, mult=MULT):
        return lib.mctq_lut_codes_per_tensor(xp, yp, nn, dtc, code, step, 1.5, *bk, mult, CMIN, CMAX, st)

    def per_channel(xp=x, yp=y, o=2, c=12, i=8, code=U8, bk=books, tp=thr):
        return lib.mctq_lut_codes_per_channel(xp, yp, o, c, i, dtc, code, tp, 1e-8, *bk, MULT, CMIN, CMAX, st)

    assert per_tensor() == 0                                           # a note of this test's own to hold on to
    fr.y.copy_(_dev(fr.inside))
    torch.cuda.synchronize()
    count, text = native.launch_count(), native.last_launch()
    assert text == note("flat_kernel", OP_NAME[op], 16 // N, 1, OP_U[op], 1)
    es = xb.element_size()
    calls = [("n == 0", 0, lambda: per_tensor(nn=0)),
             ("n == 0, 4-bit", 0, lambda: per_tensor(nn=0, code=U4)),
             ("outer == 0", 0, lambda: per_channel(o=0)),
             ("channels == 0, 4-bit", 0, lambda: per_channel(c=0, code=U4)),
             ("inner == 0", 0, lambda: per_channel(i=0)),
             ("outer == 0, last axis, 4-bit", 0, lambda: per_channel(o=0, c=8, i=1, code=U4)),
             ("step_round 3", E, lambda: per_tensor(step=3)),
             ("step_round 3, 4-bit", E, lambda: per_tensor(step=3, code=U4)),
             ("n < 0", E, lambda: per_tensor(nn=-8)),
             ("x NULL", E, lambda: per_tensor(xp=None)),
             ("codes NULL", E, lambda: per_channel(yp=None)),
             ("thresholds NULL", E, lambda: per_channel(tp=None)),
             ("mult = 3.0", E, lambda: per_tensor(mult=3.0)),
             ("uint8 codes of 257 entries", E, lambda: per_tensor(bk=(books[0], 257) + books[2:])),
             ("4-bit: n % 8 != 0", E, lambda: per_tensor(nn=n - 4, code=U4)),
             ("4-bit: inner % 8 != 0", E, lambda: per_channel(o=4, c=12, i=4, code=U4)),
             ("4-bit: inner == 1, channels % 8 != 0", E, lambda: per_channel(o=16, c=12, i=1, code=U4)),
             ("4-bit: x off 16 bytes, per tensor", E, lambda: per_tensor(xp=x + es, code=U4)),
             ("4-bit: x off 16 bytes, per channel", E, lambda: per_channel(xp=x + 8, code=U4)),
             ("4-bit: codes off 4 bytes, per tensor", E, lambda: per_tensor(yp=y + 2, code=U4)),
             ("4-bit: codes off 4 bytes, last axis", E, lambda: per_channel(yp=y + 1, o=24, c=8, i=1, code=U4)),
             ("4-bit: n_lut = 17, per tensor", E, lambda: per_tensor(code=U4, bk=books17)),
             ("4-bit: n_lut = 17, per channel", E, lambda: per_channel(code=U4, bk=books17))]
    _check_calls(lib, fr, calls, count, text)


@pytest.mark.parametrize("code", ["u8", "u4"])
def test_refused_and_empty_decodes_launch_nothing(lib, code):
    from mct_quantizers_amd.hip import native
    E = native.MCTQ_E_ARG
    cdt = native.CODE_U8 if code == "u8" else native.CODE_U4
    n = 192                                                            # [2, 12, 8], [24, 8, 1]
    cb = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    fr = _Frame(nbytes=4 * n)
    c, y, st = cb.data_ptr(), fr.ptr(), _stream()
    big = _dev(np.arange(300, dtype=F32))
    lut = big.data_ptr()
    t_d = _dev(np.full(16, 1.5, F32))
    thr = t_d.data_ptr()

    def per_tensor(cp=c, yp=y, nn=n, lp=lut, n_lut=3, mult=MULT):
        return lib.mctq_lut_decode_per_tensor(cp, yp, nn, cdt, lp, n_lut, mult, 1.5, st)

    def per_channel(cp=c, yp=y, o=2, ch=12, i=8, lp=lut, n_lut=3, mult=MULT, tp=thr):
        return lib.mctq_lut_decode_per_channel(cp, yp, o, ch, i, cdt, lp, n_lut, mult, tp, st)

    assert per_tensor() == 0                                           # a note of this test's own to hold on to
    fr.y.copy_(_dev(fr.inside))
    torch.cuda.synchronize()
    count, text = native.launch_count(), native.last_launch()
    assert text == note(f"lut_decode_kernel<{code},tensor>", "LutDecodeOp", 1, 4, 4, 1)
    calls = [("n == 0", 0, lambda: per_tensor(nn=0)),
             ("n == 0, NULL pointers", 0, lambda: per_tensor(cp=None, yp=None, nn=0)),
             ("outer == 0", 0, lambda: per_channel(o=0)),
             ("channels == 0", 0, lambda: per_channel(ch=0)),
             ("inner == 0", 0, lambda: per_channel(i=0)),
             ("outer == 0 with NULL thresholds", 0, lambda: per_channel(o=0, tp=None)),
             ("n < 0", E, lambda: per_tensor(nn=-8)),
             ("negative extent", E, lambda: per_channel(ch=-12)),
             ("codes NULL", E, lambda: per_tensor(cp=None)),
             ("y NULL", E, lambda: per_channel(yp=None)),
             ("n_lut = 0, per tensor", E, lambda: per_tensor(n_lut=0)),
             ("n_lut = 0, per channel", E, lambda: per_channel(n_lut=0)),
             ("n_lut beyond the code, per tensor", E, lambda: per_tensor(n_lut=257 if code == "u8" else 17)),
             ("n_lut beyond the code, per channel", E, lambda: per_channel(n_lut=257 if code == "u8" else 17)),
             ("mult = 3.0, per tensor", E, lambda: per_tensor(mult=3.0)),
             ("mult = 3.0, per channel", E, lambda: per_channel(mult=3.0)),
             ("lut NULL, per tensor", E, lambda: per_tensor(lp=None)),
             ("lut NULL, per channel", E, lambda: per_channel(lp=None)),
             ("thresholds NULL with n > 0", E, lambda: per_channel(tp=None)),
             ("code type MCTQ_CODE_I8", E, lambda: lib.mctq_lut_decode_per_tensor(c, y, n, native.CODE_I8, lut, 3, MULT, 1.5, st))]
    if code == "u4":
        calls += [("n % 8 != 0", E, lambda: per_tensor(nn=n - 4)),
                  ("neither whole nor last: inner % 8 != 0", E, lambda: per_channel(o=4, ch=12, i=4)),
                  ("neither whole nor last: inner == 1, channels % 8 != 0", E, lambda: per_channel(o=16, ch=12, i=1)),
                  ("codes off 4 bytes, per tensor", E, lambda: per_tensor(cp=c + 1)),
                  ("codes off 4 bytes, per channel", E, lambda: per_channel(cp=c + 2)),
                  ("y off 16 bytes, per tensor", E, lambda: per_tensor(yp=y + 4)),
                  ("y off 16 bytes, last axis", E, lambda: per_channel(yp=y + 8, o=24, ch=8, i=1))]
    _check_calls(lib, fr, calls, count, text)
