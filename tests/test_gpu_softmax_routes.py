"""mctq_codes_softmax through the raw C ABI on every row placement and edge value: the cases of
tests/test_softmax_route_cases.py, which proves without a GPU what they reach -- every shift dl of both forms at every chunk
count, both values of sh, gap bytes that would change every row, ties, clamps, zero table entries, full-width sums -- and that
its numpy oracle is the contract.

Expected values: that oracle (softmax_rows), never a GPU's result and never ops.codes_softmax.  Bar: equality of every byte of
the ``rows * out_pitch`` region, codes and pad bytes alike; no mask, no tolerance.  The output lies in a buffer filled with 0x5a
with 256 guard bytes on each side, which must keep their value; the input is a fresh device buffer of exactly
``(rows - 1) * in_pitch + L`` bytes.  Every call returns 0, advances mctq_launch_count by one and leaves the launch note the
cases module predicts from the launcher's documented slot count (form, " pre", U = CH).  The tuning key softmax_form is put
back to 0 in a ``finally``.  The refusals of the ABI return nonzero with a message, launch nothing and leave the frame as it was.
"""
import numpy as np
import pytest
import torch

import test_softmax_route_cases as C
from conftest import first_mismatch

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0x5a
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


def _dev(v):
    """A numpy operand on the GPU (a fresh allocation: 16-byte aligned)."""
    t = torch.from_numpy(np.array(v)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class _Frame:
    """``nbytes`` output bytes in the middle of a 0x5a buffer with GUARD bytes on each side."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def read(self, what):
        """The inner bytes, after the guard bands were found untouched."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == FILL) and np.all(b[GUARD + self.nbytes:] == FILL), f"{what}: wrote outside its {self.nbytes} bytes"
        return b[GUARD:GUARD + self.nbytes]

    def untouched(self, what):
        assert np.all(self.read(what) == FILL), f"{what}: the output was written"


def _operands(case):
    """(input bytes, exp table, pre-table or None) of a case on the GPU."""
    from mct_quantizers_amd.hip import ops
    buf, _, _ = C.case_data(case)
    x = _dev(buf)
    assert x.numel() == case.total
    pre = None if case.pre is None else _dev(C.pre_table(case.pre))
    return x, _dev(ops.softmax_exp_table(case.scale_a).view(np.int32)), pre


def _call(lib, case, in_ptr, out_ptr, exp_ptr, pre_ptr, **other):
    """mctq_codes_softmax with the case's arguments, ``other`` in place of those it names."""
    from mct_quantizers_amd.hip import native
    s_b, zp, qmin, qmax = case.out_form
    a = dict(in_code=native.CODE_U8 if case.in_u8 else native.CODE_I8, out_code=native.CODE_U8 if case.out_u8 else native.CODE_I8,
             rows=case.rows, L=case.L, in_pitch=case.in_pitch, out_pitch=case.out_pitch, pad_code=case.pad_code)
    assert set(other) <= set(a)
    a.update(other)
    return lib.mctq_codes_softmax(in_ptr, a["in_code"], out_ptr, a["out_code"], s_b, zp, qmin, qmax, a["rows"], a["L"], a["in_pitch"],
                                  a["out_pitch"], a["pad_code"], exp_ptr, pre_ptr, torch.cuda.current_stream().cuda_stream)


def _where(case, got, want):
    """The first byte that differs, by row and column and with the row's placement."""
    i = int(np.flatnonzero(got != want)[0])
    r, col = divmod(i, case.out_pitch)
    pl = {k: int(v[r]) for k, v in C.placements(case.place).items()}
    return f"{first_mismatch(got, want)}: row {r} column {col} ({'code' if col < case.L else 'pad'}), {pl}"


def _run(lib, case):
    """One launch of a case on a framed output: rc == 0, one launch, the note, the oracle's bytes, the guard bands."""
    from mct_quantizers_amd.hip import native
    _, want, _ = C.case_data(case)
    x, exp, pre = _operands(case)
    fr = _Frame(case.rows * case.out_pitch)
    count = native.launch_count()
    native.set_tuning("softmax_form", case.form)
    try:
        rc = _call(lib, case, x.data_ptr(), fr.ptr(), exp.data_ptr(), None if pre is None else pre.data_ptr())
        torch.cuda.synchronize()
    finally:
        native.set_tuning("softmax_form", 0)
    assert rc == 0, f"{case.name}: {lib.mctq_last_error().decode()}"
    launch = native.last_launch()
    assert native.launch_count() == count + 1 and launch == C.note(case), f"{case.name}: took {launch}, expected {C.note(case)}"
    got = fr.read(case.name)
    assert np.array_equal(got, want), f"{case.name} [{launch}]: {_where(case, got, want)}"


# ------------------------------------------------------------------------------------------------
# 1. placements and edge values through the raw C ABI
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.PLACEMENT, ids=C.ids(C.PLACEMENT))
def test_row_placements(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", C.EDGE, ids=C.ids(C.EDGE))
def test_edge_values(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", C.OPS_ROUTE, ids=C.ids(C.OPS_ROUTE))
def test_the_pitches_of_the_python_route(lib, case):
    _run(lib, case)


# ------------------------------------------------------------------------------------------------
# 2. the Python route on GPU tensors against the same oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.OPS_ROUTE, ids=C.ids(C.OPS_ROUTE))
def test_codes_softmax_on_gpu_tensors_gives_the_oracles_bytes(case):
    from mct_quantizers_amd.hip import native
    _, want, _ = C.case_data(case)
    codes = C.row_codes(case).cuda()
    count = native.launch_count()
    native.set_tuning("softmax_form", case.form)
    try:
        got = C.ops_call(case, codes, pad_to=16 if case.out_pitch > case.L else None)
        torch.cuda.synchronize()
    finally:
        native.set_tuning("softmax_form", 0)
    assert native.launch_count() == count + 1 and native.last_launch() == C.note(case), native.last_launch()
    assert got.is_cuda and tuple(got.shape) == (case.rows, case.out_pitch) and got.dtype == (torch.uint8 if case.out_u8 else torch.int8)
    got = got.cpu().view(torch.uint8).numpy().reshape(-1)
    assert np.array_equal(got, want), f"{case.name}: {_where(case, got, want)}"


# ------------------------------------------------------------------------------------------------
# 3. what the ABI refuses, and what it takes as nothing to do
# ------------------------------------------------------------------------------------------------

BASE = C.PLACEMENT[0]                                          # 19 rows of 37 bytes, pitches 41 / 38, uint8 output
MIRROR = C.PLACEMENT[1]                                        # ... 38 / 41
# (what, arguments in place of the case's, byte offsets added to in / out / exp_table / pre_table, words of the message)
REFUSALS = [
    ("in off by one byte", {}, (1, 0, 0, 0), "in must be 16-byte aligned"),
    ("out off by one byte", {}, (0, 1, 0, 0), "out must be 16-byte aligned"),
    ("exp_table off by one byte", {}, (0, 0, 1, 0), "tables must be 4-byte aligned"),
    ("pre_table off by one byte", {}, (0, 0, 0, 1), "tables must be 4-byte aligned"),
    ("in_pitch < L", dict(in_pitch=36), (0, 0, 0, 0), "at least the row length"),
    ("out_pitch < L", dict(out_pitch=36), (0, 0, 0, 0), "at least the row length"),
    ("out overlaps in", {}, ("out+16", 0, 0, 0), "out overlaps in"),
    ("out overlaps exp_table", {}, (0, 0, "out+32", 0), "out overlaps exp_table"),
    ("out overlaps pre_table", {}, (0, 0, 0, "out+64"), "out overlaps pre_table"),
    ("in bytes beyond 2^31 - 1", dict(rows=INT32_MAX // 41 + 1), (0, 0, 0, 0), "more than 2^31 - 1 bytes"),
    ("pad_code 256 of uint8", dict(pad_code=256), (0, 0, 0, 0), "pad_code is no code of"),
    ("pad_code -1 of uint8", dict(pad_code=-1), (0, 0, 0, 0), "pad_code is no code of"),
    ("pad_code 128 of int8", dict(pad_code=128, out_code="i8"), (0, 0, 0, 0), "pad_code is no code of"),
    ("rows < 0", dict(rows=-1), (0, 0, 0, 0), "negative extent"),
    ("L < 0", dict(L=-1), (0, 0, 0, 0), "negative extent"),
]


def _refused(lib, fr, what, words, call):
    from mct_quantizers_amd.hip import native
    count = native.launch_count()
    rc = call()
    torch.cuda.synchronize()
    text = lib.mctq_last_error().decode()
    assert rc != 0 and text and words in text, f"{what}: rc {rc}, message {text!r}"
    assert native.launch_count() == count, f"{what}: launched {native.last_launch()}"
    fr.untouched(what)


@pytest.mark.parametrize("what,other,offsets,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(lib, what, other, offsets, words):
    from mct_quantizers_amd.hip import native
    x, exp, _ = _operands(BASE)
    pre = _dev(C.pre_table("identity"))
    fr = _Frame(BASE.rows * BASE.out_pitch)
    assert BASE.out_u8 and BASE.out_form[2:] == (0, 255) and BASE.rows * BASE.out_pitch > 64 + 256
    if other.get("out_code") == "i8":                          # (the clamp domain stays uint8's: the pad code is checked first)
        other = dict(other, out_code=native.CODE_I8)
    base = dict(zip(("in", "out", "exp", "pre"), (x.data_ptr(), fr.ptr(), exp.data_ptr(), pre.data_ptr())))
    ptrs = [base["out"] + int(o[4:]) if isinstance(o, str) else base[name] + o for name, o in zip(base, offsets)]
    _refused(lib, fr, what, words, lambda: _call(lib, BASE, *ptrs, **other))


def test_out_bytes_beyond_int32_are_refused_before_any_launch(lib):
    """rows * out_pitch alone is too much: 38 * rows fits, 41 * rows does not."""
    rows = INT32_MAX // 41 + 1
    assert MIRROR.place[2:4] == (38, 41) and rows * 38 <= INT32_MAX < rows * 41
    x, exp, _ = _operands(MIRROR)
    fr = _Frame(MIRROR.rows * MIRROR.out_pitch)
    _refused(lib, fr, "out bytes beyond 2^31 - 1", "more than 2^31 - 1 bytes", lambda: _call(lib, MIRROR, x.data_ptr(), fr.ptr(), exp.data_ptr(), None, rows=rows))


def test_one_chunk_more_than_the_block_form_holds_is_refused(lib):
    """out_pitch = 32738 under unaligned pitches: 2049 chunks with the alignment slack.  The buffers are real and whole."""
    rows, L, in_pitch, out_pitch, _ = C.REFUSED
    case = C.Case("refused", rows, L, in_pitch, out_pitch, 0, False, (2.0 ** -22, 0, 0, 255), 0xc3, 2.0 ** -5, "random")
    x, exp, _ = _operands(case)
    fr = _Frame(rows * out_pitch)
    _refused(lib, fr, "out_pitch 32738", "more than 32768 bytes", lambda: _call(lib, case, x.data_ptr(), fr.ptr(), exp.data_ptr(), None))


@pytest.mark.parametrize("other", [dict(rows=0), dict(L=0, in_pitch=16, out_pitch=16)], ids=["rows = 0", "L = 0"])
def test_nothing_to_do_returns_zero_and_writes_nothing(lib, other):
    from mct_quantizers_amd.hip import native
    x, exp, _ = _operands(BASE)
    fr = _Frame(BASE.rows * BASE.out_pitch)
    count = native.launch_count()
    rc = _call(lib, BASE, x.data_ptr(), fr.ptr(), exp.data_ptr(), None, **other)
    assert rc == 0 and native.launch_count() == count
    fr.untouched(str(other))
