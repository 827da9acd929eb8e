"""The cases of tests/test_gpu_softmax_routes.py -- mctq_codes_softmax (csrc/mctq_codes_softmax.hip) on every placement of a row
within its 16-byte chunks, in both forms and at every chunk count, and at the edge values of its arithmetic -- and, without a
GPU, the proof that they hold what they claim.

The oracle.  ``softmax_rows`` is the contract in the kernel's header, line for line, in numpy and Python integers: per row
c = pre[raw] or raw, ordered by sign for int8; d = max c - c; S = sum E[d] as a Python integer; p = float32(E[d]) / float32(S);
code = clamp(rint(p * (float32(1) / float32(s_b))) + zp).  It takes the flat input buffer and the two pitches and returns the
``rows * out_pitch`` bytes a launch must leave, ``pad_code`` behind every row.  Of ops it uses softmax_exp_table alone.  Proved
here: ops.codes_softmax on CPU tensors gives the oracle's bytes on the rows of every case; the oracle is within one code of the
float64 softmax of the dequantized values (test_softmax_consumer._reference) everywhere, and on the random-value cases differs
from it in at most 1e-3 of the elements (the edge-value cases sit on ties on purpose).

Placements.  A case is (rows, L, in_pitch, out_pitch, form); ``placements`` gives per row ia = (r * in_pitch) % 16,
ob = (r * out_pitch) % 16, dl = (ia - ob) & 15 and sh (the wave form's rows with ia < ob, whose lanes take input chunk l - 1).
Asserted on the helper alone: per form and chunk count CH (wave 1, 2, 4; block 1, 2, 4) every dl in 1 .. 15 occurs and both signs
of ia - ob; ia == ob != 0 with in_pitch > L; aligned pitches with a gap; rows shorter than a chunk that straddle two; the slot
boundaries 4065 / 4066 / 32737 (32738 is refused); buffers that end inside a chunk in both forms.  Every input byte outside a
row is the greatest code of the input type and every row's own codes lie below it: the oracle recomputed with one such byte
counted into the rows differs in every row (test_a_gap_byte_counted_into_a_row_changes_that_row), the condition under which a
kernel that lets a byte outside the row into the max or the sum cannot pass.

Edge values (``EDGE``; L + 1 / L + 2 pitches, both forms): exact .5 ties of p * (1 / s_b) for k + .5, k in 0, 1, 2, 3, 100, 101,
found by a seeded search; both clamps, a 4-bit domain, int8 output from zero point -128; exp tables with zero entries
(scale_a = 1, 8), S = 2^24 and one-hot rows; sums beyond 2^32 (wave) and 2^38 (block) with an inexact float32(S) and a lane
partial of 2^31; the extreme codes of both input types side by side, L = 1, the maximum first and last; pre-tables (identity,
constant, tanh with int8 entries under uint8 bytes and the reverse).
"""
import functools
import typing

import numpy as np
import pytest
import torch

from mct_quantizers_amd.hip import ops
from test_softmax_consumer import _reference

F32 = np.float32
WAVE_SLOTS, BLOCK_SLOTS = 256, 2048                            # 16-byte chunks of one row: 64 lanes x 4, 256 lanes x 8
GREATEST = {False: 0x7f, True: 0xff}                           # the raw byte of the greatest code, by "the codes are uint8"
LEAST = {False: 0x80, True: 0x00}
DOMAIN = {False: (-128, 127), True: (0, 255)}
TIE_KS = (0, 1, 2, 3, 100, 101)
RAW_U8 = {"tanh_i8_from_u8": True, "tanh_u8_from_i8": False}   # pre-tables whose entries' type is not the raw bytes'


class Case(typing.NamedTuple):
    name: str
    rows: int
    L: int
    in_pitch: int
    out_pitch: int
    form: int                 # tuning key softmax_form: 0 auto, 1 wave, 2 block
    in_u8: bool               # the type of A's codes (with a pre-table: of its entries)
    out_form: tuple           # (s_b, zp, qmin, qmax)
    pad_code: int
    scale_a: float
    values: str               # what the rows hold (_row_codes)
    pre: typing.Optional[str] = None

    @property
    def place(self):
        return self.rows, self.L, self.in_pitch, self.out_pitch, self.form

    @property
    def total(self):
        return (self.rows - 1) * self.in_pitch + self.L

    @property
    def raw_u8(self):
        return RAW_U8.get(self.pre, self.in_u8)

    @property
    def out_u8(self):
        return self.out_form[2] >= 0


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------

def _ordered(c, in_dtype):
    """The bytes ``c`` as the integers their code type orders them by."""
    assert in_dtype in (np.int8, np.uint8)
    return (c.view(np.int8) if in_dtype == np.int8 else c).astype(np.int64)


def softmax_rows(buf, rows, L, in_pitch, out_pitch, in_dtype, out_form, pad_code, pre=None, *, scale_a, details=False):
    """The ``rows * out_pitch`` bytes of mctq_codes_softmax for the flat input bytes ``buf`` (row r at r * in_pitch): L codes and
    then ``pad_code`` up to out_pitch.  ``details``: also, per row, S and the arrays d, E[d], p, p * (1 / s_b) and the code before
    the clamp."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= (rows - 1) * in_pitch + L and min(in_pitch, out_pitch) >= L >= 1
    s_b, zp, lo, hi = out_form
    E = ops.softmax_exp_table(scale_a)
    inv = F32(1) / F32(s_b)
    out = np.full((rows, out_pitch), pad_code & 0xff, np.uint8)
    seen = []
    for r in range(rows):
        raw = buf[r * in_pitch:r * in_pitch + L]
        c = _ordered(raw if pre is None else pre[raw], in_dtype)
        d = int(c.max()) - c
        e = E[d]
        S = sum(e.tolist())                                                       # Python integers: exact
        p = e.astype(F32) / F32(S)
        prod = p * inv
        q = np.rint(prod) + F32(zp)
        code = np.clip(q, F32(lo), F32(hi))
        assert p.dtype == prod.dtype == q.dtype == code.dtype == F32
        out[r, :L] = (code.astype(np.int64) & 0xff).astype(np.uint8)
        seen.append(dict(S=S, d=d, e=e, p=p, prod=prod, q=q))
    out = out.reshape(-1)
    return (out, seen) if details else out


# ------------------------------------------------------------------------------------------------
# placements and the launcher's documented choice
# ------------------------------------------------------------------------------------------------

def slots(in_pitch, out_pitch):
    """The launcher's count of 16-byte chunks that cover any row's input window and output row (rows that all start on a chunk
    need no slack)."""
    aligned = in_pitch % 16 == 0 and out_pitch % 16 == 0
    return -(-out_pitch // 16) if aligned else (out_pitch + 30) // 16 + 1


def launch_form(place):
    """("wave" | "block", CH) of a case that runs, or None where the launcher refuses the row."""
    rows, L, in_pitch, out_pitch, form = place
    n = slots(in_pitch, out_pitch)
    if n > BLOCK_SLOTS:
        return None
    block = n > WAVE_SLOTS or form == 2
    ch = 1
    while ch * (256 if block else 64) < n:
        ch *= 2
    return ("block" if block else "wave"), ch


def placements(place):
    """Per row: ia, ob, dl = (ia - ob) & 15 and sh (wave form, ia < ob: lane l takes input chunk l - 1)."""
    rows, L, in_pitch, out_pitch, form = place
    r = np.arange(rows, dtype=np.int64)
    ia, ob = (r * in_pitch) % 16, (r * out_pitch) % 16
    wave = launch_form(place)[0] == "wave"
    return dict(ia=ia, ob=ob, dl=(ia - ob) & 15, sh=((ia < ob) & wave).astype(np.int64))


def lanes_of(place, row):
    """The lane that holds each element of ``row``: element e lies in input chunk k = (ia + e) // 16, slot k + sh, and lane l
    holds the slots l, l + LANES, .."""
    form, _ = launch_form(place)
    pl = placements(place)
    k = (int(pl["ia"][row]) + np.arange(place[1])) // 16 + int(pl["sh"][row])
    return k % (256 if form == "block" else 64)


def note(case):
    """The launch note of a case."""
    form, ch = launch_form(case.place)
    kinds = f"{'u8' if case.in_u8 else 'i8'} -> {'u8' if case.out_u8 else 'i8'}"
    return f"codes_softmax<{kinds} {form}{' pre' if case.pre else ''},in1B,out1B,U={ch},NT=0>"


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------

def _out_form(L, u8):
    """A power-of-two output scale under which a row of L elements spreads over the domain: 1 / s_b = 2^ceil(log2(64 L))."""
    s_b = 2.0 ** -int(np.ceil(np.log2(64 * L)))
    return (s_b, 0, 0, 255) if u8 else (s_b, -128, -128, 127)


def _placed(name, rows, L, in_pitch, out_pitch, form, in_u8=False, out_u8=True):
    return Case(name, rows, L, in_pitch, out_pitch, form, in_u8, _out_form(L, out_u8), 0xc3 if out_u8 else -61, 2.0 ** -5, "random")


def _pair(name, rows, L, form, **kw):
    """in = L + 4, out = L + 1 and its mirror."""
    return [_placed(f"{name} in>out", rows, L, L + 4, L + 1, form, **kw), _placed(f"{name} in<out", rows, L, L + 1, L + 4, form, **kw)]


def _placement_cases():
    cases = []
    for in_u8 in (False, True):                                                   # both input types: one chunk a lane, forced block
        cases += _pair(f"wave 37 {'u8' if in_u8 else 'i8'}", 19, 37, 0, in_u8=in_u8, out_u8=not in_u8)
        cases += _pair(f"block 37 {'u8' if in_u8 else 'i8'}", 19, 37, 2, in_u8=in_u8, out_u8=in_u8)
    cases += _pair("wave 1030", 19, 1030, 0) + _pair("wave 2100", 19, 2100, 0, out_u8=False)
    cases += _pair("block 1030", 19, 1030, 2, out_u8=False)
    cases += _pair("block 4100", 17, 4100, 0) + _pair("block 9000", 17, 9000, 0, out_u8=False)
    for form in (0, 2):
        cases.append(_placed(f"same place {form}", 9, 37, 45, 45, form, out_u8=form == 0))
        cases.append(_placed(f"aligned gap {form}", 5, 37, 48, 64, form, out_u8=form == 2))
        for L in (1, 2, 15, 16, 17):
            cases.append(_placed(f"short {L} {form}", 19, L, L + 3, L + 6, form, out_u8=(L + form) % 4 != 1))
    for pitch in (4065, 4066, 32737):                                             # the slot boundaries: wave | block | the last that runs
        cases.append(_placed(f"boundary {pitch}", 3, pitch, pitch + 1, pitch, 0))
    return cases


REFUSED = (3, 32738, 32739, 32738, 0)                                             # one chunk more than the block form holds


def _edge(name, rows, L, form, out_form, scale_a, values, in_u8=False, pre=None, pad_code=None, pitches=None):
    in_pitch, out_pitch = pitches or (L + 1, L + 2)
    pad = pad_code if pad_code is not None else (0xc3 if out_form[2] >= 0 else -61)
    return Case(name, rows, L, in_pitch, out_pitch, form, in_u8, out_form, pad, scale_a, values, pre)


CLAMP_FORMS = {"top": (1.0 / 256, 0, 0, 255), "bottom": (1.0 / 255, 0, 16, 128), "4-bit": (1.0 / 15, 0, 0, 15),
               "int8": (1.0 / 256, -128, -128, 127)}
U8_OUT, I8_OUT = (1.0 / 255, 0, 0, 255), (1.0 / 255, -128, -128, 127)


def _edge_cases():
    cases = []
    for form in (1, 2):
        for k in TIE_KS:
            scale_a, d, j, s_b = tie(k)
            cases.append(_edge(f"tie {k} {form}", len(d), len(d), form, (s_b, 0, 0, 255), scale_a, f"tie {k}"))
        for name, out_form in CLAMP_FORMS.items():
            cases.append(_edge(f"clamp {name} {form}", 8, 5, form, out_form, 1.0, "clamp"))
        for scale_a in (1.0, 8.0):
            cases.append(_edge(f"zero entries {scale_a} {form}", 8, 37, form, U8_OUT, scale_a, "one hot"))
        for in_u8 in (False, True):
            cases.append(_edge(f"extremes {'u8' if in_u8 else 'i8'} {form}", 4, 37, form, I8_OUT if in_u8 else U8_OUT, 2.0 ** -5, "extremes", in_u8))
        cases.append(_edge(f"L = 1 {form}", 8, 1, form, U8_OUT, 0.0731, "random"))
        cases.append(_edge(f"identity table {form}", 6, 37, form, U8_OUT, 2.0 ** -5, "random", True, "identity"))
        cases.append(_edge(f"constant table {form}", 6, 37, form, _out_form(37, False), 2.0 ** -5, "random", False, "constant"))
        cases.append(_edge(f"tanh table int8 entries, uint8 bytes {form}", 6, 37, form, U8_OUT, 0.0731, "random", False, "tanh_i8_from_u8"))
        cases.append(_edge(f"tanh table uint8 entries, int8 bytes {form}", 6, 37, form, I8_OUT, 0.0731, "random", True, "tanh_u8_from_i8"))
    # full-width sums: the form and the pitches the lengths dictate
    cases.append(_edge("equal rows 4064", 3, 4064, 0, (2.0 ** -19, 0, 0, 255), 0.3, "equal", pitches=(4065, 4065)))
    cases.append(_edge("equal rows 32736", 3, 32736, 0, (2.0 ** -22, 0, 0, 255), 0.3, "equal", pitches=(32737, 32737)))
    cases.append(_edge("adjacent codes 4064", 3, 4064, 0, (2.0 ** -19, 0, 0, 255), 2.0 ** -5, "adjacent", pitches=(4065, 4065)))
    cases.append(_edge("adjacent codes 32736", 3, 32736, 0, (2.0 ** -22, -128, -128, 127), 2.0 ** -5, "adjacent", pitches=(32737, 32737)))
    return cases


def _ops_cases():
    """What ops.codes_softmax launches: in_pitch = L, out_pitch = L or 16 * ceil(L / 16), the pad the zero point."""
    cases = []
    for L in (37, 1030):
        for pad_to in (None, 16):
            for form in (1, 2):
                out_u8 = (L + form) % 2 == 0
                out_form = _out_form(L, out_u8)
                lp = -(-L // 16) * 16 if pad_to else L
                cases.append(Case(f"ops {L} pad_to={pad_to} {form}", 6, L, L, lp, form, False, out_form, out_form[1], 0.0731, "random"))
    cases.append(Case("ops 37 pad_to=16 table", 6, 37, 37, 48, 0, False, U8_OUT, 0, 0.0731, "random", "tanh_i8_from_u8"))
    return cases


@functools.lru_cache(maxsize=None)
def tie(k):
    """(scale_a, d, j, s_b): a row with the differences d from its maximum and an output scale under which the float32 product
    p_j * (1 / s_b) is exactly k + 0.5 -- the first hit of a seeded search over rows of 2 .. 5 codes with differences below 24."""
    rng = np.random.default_rng([29, k])
    half = F32(k + 0.5)
    for _ in range(20000):
        scale_a = (0.0731, 2.0 ** -3, 0.25)[int(rng.integers(3))]
        d = rng.integers(0, 24, int(rng.integers(2, 6)))
        d[0] = 0
        e = ops.softmax_exp_table(scale_a)[d]
        p = e.astype(F32) / F32(sum(e.tolist()))
        for j in range(len(d)):
            s_b = F32(p[j] / half)
            if s_b > 0 and p[j] * (F32(1) / s_b) == half:
                return scale_a, tuple(int(v) for v in d), j, float(s_b)
    raise AssertionError(f"no tie found for {k}")


@functools.lru_cache(maxsize=None)
def pre_table(name):
    if name == "identity":
        table = np.arange(256).astype(np.uint8)
    elif name == "constant":
        table = np.full(256, 0x85, np.uint8)
    else:
        a_u8 = not RAW_U8[name]                                                   # the entries' type is the other one
        zp = 125 if a_u8 else -3                                                  # entries on both sides of 0x80 in either type
        t = ops.code_table(lambda v: torch.tanh(v * 0.125), (0.21, 5, *DOMAIN[RAW_U8[name]]), (0.0731, zp, *DOMAIN[a_u8]), "cpu")
        table = t.numpy().copy()
    table.setflags(write=False)
    return table


def _row_codes(case):
    """The rows' own bytes [rows, L]."""
    rows, L = case.rows, case.L
    rng = np.random.default_rng([3, rows, L, case.in_pitch, case.out_pitch, int(case.in_u8)])
    lo, hi = DOMAIN[case.raw_u8]
    if case.values == "random":                                                   # strictly below the greatest code
        c = rng.integers(lo, hi, (rows, L))
    elif case.values.startswith("tie"):
        _, d, _, _ = tie(int(case.values.split()[1]))
        c = np.stack([50 - np.roll(np.asarray(d), r) for r in range(rows)])      # the same differences, rotated: a tie in every row
    elif case.values == "clamp":                                                  # scale_a = 1: row 0 is one-hot, the others are close
        c = rng.integers(60, 63, (rows, L))
        c[0], c[0, 2] = 0, 100
    elif case.values == "one hot":                                                # the maximum once, everything else >= 18 below it
        c = rng.integers(lo, 120 - 18, (rows, L))
        c[:, 0] = 120 - 18                                                        # distance 18 exactly: the first zero entry at scale_a = 1
        c[np.arange(rows), (5 * np.arange(rows) + 3) % L] = 120
    elif case.values == "extremes":
        c = rng.integers(lo + 1, hi, (rows, L))
        c[0, 17], c[0, 18] = lo, hi                                               # least and greatest side by side, across a chunk's dwords
        c[1, -1] = hi                                                             # the maximum is the last element,
        c[2, 0] = hi                                                              # the first,
        c[3, 0], c[3, 1] = hi, lo                                                 # and the two extremes in the other order
    elif case.values == "equal":
        c = np.repeat(41 + np.arange(rows)[:, None], L, axis=1)
    elif case.values == "adjacent":                                               # c and c - 1; row 0: lane 0 holds the maximum throughout
        c = 77 - rng.integers(0, 2, (rows, L))
        c[0, lanes_of(case.place, 0) == 0] = 77
        c[1:, 0] = 77
    else:
        raise AssertionError(case.values)
    assert c.min() >= lo and c.max() <= hi
    return (c & 0xff).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(the input bytes [total], the expected bytes [rows * out_pitch], the oracle's per-row values): the rows' codes at their
    pitch and, in every gap between them, the greatest code of the raw bytes' type.  Read-only, shared by the CPU and GPU tests."""
    codes = _row_codes(case)
    buf = np.full(case.total, GREATEST[case.raw_u8], np.uint8)
    for r in range(case.rows):
        buf[r * case.in_pitch:r * case.in_pitch + case.L] = codes[r]
    want, seen = _oracle(case, buf, details=True)
    buf.setflags(write=False)
    want.setflags(write=False)
    return buf, want, seen


def _oracle(case, buf, details=False, extend=0):
    return softmax_rows(buf, case.rows, case.L + extend, case.in_pitch, case.out_pitch + extend, np.uint8 if case.in_u8 else np.int8,
                        case.out_form, case.pad_code, None if case.pre is None else pre_table(case.pre), scale_a=case.scale_a,
                        details=details)


def row_codes(case):
    """The rows of a case without the gaps, as a CPU tensor of the raw bytes' type."""
    buf, _, _ = case_data(case)
    rows = np.stack([buf[r * case.in_pitch:r * case.in_pitch + case.L] for r in range(case.rows)])
    return torch.from_numpy(rows.copy()).view(torch.uint8 if case.raw_u8 else torch.int8)


def ops_call(case, codes, pad_to=None):
    """ops.codes_softmax on ``codes`` [rows, L] under the case's forms."""
    table = None if case.pre is None else torch.from_numpy(pre_table(case.pre).copy()).to(codes.device)
    return ops.codes_softmax(codes, (case.scale_a, 3, *DOMAIN[case.in_u8]), case.out_form, pre_table=table, pad_to=pad_to)


def as_rows(case, flat):
    return np.asarray(flat).reshape(case.rows, case.out_pitch)


PLACEMENT = _placement_cases()
EDGE = _edge_cases()
OPS_ROUTE = _ops_cases()
ALL = PLACEMENT + EDGE + OPS_ROUTE
RANDOM_VALUE = [c for c in PLACEMENT + OPS_ROUTE if c.values == "random"]


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------
# (a) the oracle against ops.codes_softmax on the CPU and against float64
# ------------------------------------------------------------------------------------------------

def test_the_lists_are_what_the_module_says():
    assert len({c.name for c in ALL}) == len(ALL) and len({c[1:] for c in ALL}) == len(ALL)
    for c in ALL:
        assert c.in_pitch >= c.L >= 1 and c.out_pitch >= c.L and launch_form(c.place) is not None, c.name
        assert DOMAIN[c.out_u8][0] <= c.pad_code <= DOMAIN[c.out_u8][1] and c.rows * max(c.in_pitch, c.out_pitch) <= 17 * 9004
    assert all(c.rows <= 8 and c.form in (1, 2) and (c.in_pitch, c.out_pitch) == (c.L + 1, c.L + 2) for c in EDGE if c.form)
    assert all(c.in_pitch == c.L and c.out_pitch in (c.L, -(-c.L // 16) * 16) and c.pad_code == c.out_form[1] for c in OPS_ROUTE)
    assert {(c.L, c.out_pitch) for c in OPS_ROUTE} >= {(37, 37), (37, 48), (1030, 1030), (1030, 1040)}
    # int8 and uint8 input on the one-chunk wave pair and the forced-block pair, int8 elsewhere
    assert {c.place for c in PLACEMENT if c.in_u8} == {(19, 37, a, b, f) for a, b in ((41, 38), (38, 41)) for f in (0, 2)}
    assert {c.place for c in PLACEMENT if c.in_u8} <= {c.place for c in PLACEMENT if not c.in_u8}


@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_codes_softmax_on_cpu_gives_the_oracles_bytes(case):
    _, want, _ = case_data(case)
    want = as_rows(case, want)
    got = ops_call(case, row_codes(case)).view(torch.uint8).numpy()
    assert got.shape == (case.rows, case.L) and np.array_equal(got, want[:, :case.L]), case.name
    assert np.all(want[:, case.L:] == (case.pad_code & 0xff))
    if case in OPS_ROUTE:                                                         # the route as it launches: the padded rows, whole
        padded = ops_call(case, row_codes(case), pad_to=16 if case.out_pitch > case.L else None)
        assert padded.dtype == (torch.uint8 if case.out_u8 else torch.int8) and np.array_equal(padded.view(torch.uint8).numpy(), want)


def _against_float64(case):
    """(the largest difference in codes, the elements that differ, all elements) between the oracle and the float64 softmax."""
    _, want, _ = case_data(case)
    codes = row_codes(case)
    if case.pre is not None:
        codes = torch.from_numpy(pre_table(case.pre)[codes.view(torch.uint8).numpy()].copy())
    a_codes = codes.view(torch.uint8 if case.in_u8 else torch.int8)
    got = as_rows(case, want)[:, :case.L]
    got = (got if case.out_u8 else got.view(np.int8)).astype(np.float64)
    diff = np.abs(got - _reference(a_codes, case.scale_a, case.out_form))
    return diff.max(), int((diff > 0).sum()), diff.size


@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_the_oracle_is_within_one_code_of_float64(case):
    worst, differ, n = _against_float64(case)
    print(f"max difference {worst}, elements that differ {differ} of {n}")
    assert worst <= 1
    if case in RANDOM_VALUE:
        assert differ / n <= 1e-3


# ------------------------------------------------------------------------------------------------
# (b) placements
# ------------------------------------------------------------------------------------------------

def _find(place):
    return [c for c in PLACEMENT if c.place == place]


def test_one_chunk_wave_pair():
    for (in_pitch, out_pitch), below in (((41, 38), 8), ((38, 41), 9)):
        place = (19, 37, in_pitch, out_pitch, 0)
        assert len(_find(place)) == 2 and launch_form(place) == ("wave", 1)
        pl = placements(place)
        assert sorted(pl["dl"][:16].tolist()) == list(range(16)) and sorted(pl["dl"][3:19].tolist()) == list(range(16))
        assert int((pl["ia"] < pl["ob"]).sum()) == below == int(pl["sh"].sum())
    assert 19 % 4 == 3                                                            # one of the last workgroup's four waves is idle


def test_every_shift_in_every_form_and_chunk_count():
    groups = {}
    for c in PLACEMENT:
        if (c.in_pitch, c.out_pitch) in ((c.L + 4, c.L + 1), (c.L + 1, c.L + 4)):
            pl = placements(c.place)
            groups.setdefault(launch_form(c.place), set()).update(zip(pl["dl"].tolist(), np.sign(pl["ia"] - pl["ob"]).tolist(), pl["sh"].tolist()))
    assert sorted(groups) == [("block", 1), ("block", 2), ("block", 4), ("wave", 1), ("wave", 2), ("wave", 4)]
    for (form, ch), seen in groups.items():
        assert {dl for dl, _, _ in seen} == set(range(16)), (form, ch)
        assert {sign for dl, sign, _ in seen if dl} == {-1, 1}, (form, ch)
        assert {sh for _, _, sh in seen} == ({0, 1} if form == "wave" else {0}), (form, ch)
        # both rounds of selects of the funnel shift, alone and together, with a byte part and without
        assert {(dl >> 2, dl & 3 != 0) for dl, _, _ in seen} == {(q, b) for q in range(4) for b in (False, True)}
    natural = {c.L: launch_form(c.place) for c in PLACEMENT if c.form == 0 and c.rows == 17}
    assert natural == {4100: ("block", 2), 9000: ("block", 4)}
    assert {c.L for c in PLACEMENT if c.form == 2 and c.in_pitch == c.L + 4} == {37, 1030}
    assert {launch_form(c.place) for c in PLACEMENT if c.L in (1030, 2100) and c.form == 0} == {("wave", 2), ("wave", 4)}


def test_rows_that_sit_alike_gaps_and_short_rows():
    clamped = False
    for form, name in ((0, "wave"), (2, "block")):
        (same,) = _find((9, 37, 45, 45, form))
        pl = placements(same.place)
        # no row but the first starts on a chunk: every first and last chunk is shared with a neighbour
        assert launch_form(same.place) == (name, 1) and np.array_equal(pl["ia"], pl["ob"]) and (pl["ia"] != 0).sum() == 8 and 45 % 16
        (gap,) = _find((5, 37, 48, 64, form))
        assert slots(48, 64) == 4 and launch_form(gap.place) == (name, 1) and not placements(gap.place)["dl"].any()
        for L in (1, 2, 15, 16, 17):
            (short,) = _find((19, L, L + 3, L + 6, form))
            pl = placements(short.place)
            assert launch_form(short.place) == (name, 1) and (short.out_pitch - L > L) == (L <= 2)      # a gap wider than the row
            if 2 <= L < 16:                                                       # shorter than a chunk, in two chunks
                assert any(ia + L > 16 for ia in pl["ia"].tolist())
            if name == "wave":                                                    # lane 0 of a row in the buffer's first chunk takes chunk -1
                clamped |= any(sh and r * short.in_pitch < 16 for r, sh in enumerate(pl["sh"].tolist()))
    assert clamped


def test_slot_boundaries():
    assert [slots(p + 1, p) for p in (4065, 4066, 32737, 32738)] == [256, 257, 2048, 2049]
    assert [launch_form((3, p, p + 1, p, 0)) for p in (4065, 4066, 32737)] == [("wave", 4), ("block", 2), ("block", 8)]
    assert launch_form(REFUSED) is None and REFUSED[3] == 32738 and REFUSED[2] % 16 and REFUSED[3] % 16
    assert all(len(_find((3, p, p + 1, p, 0))) == 1 for p in (4065, 4066, 32737))
    assert [note(c) for p in (4065, 4066, 32737) for c in _find((3, p, p + 1, p, 0))] == [
        "codes_softmax<i8 -> u8 wave,in1B,out1B,U=4,NT=0>", "codes_softmax<i8 -> u8 block,in1B,out1B,U=2,NT=0>",
        "codes_softmax<i8 -> u8 block,in1B,out1B,U=8,NT=0>"]
    # the aligned boundaries the older tests have differ: no slack
    assert slots(4096, 4096) == 256 and slots(32768, 32768) == 2048


def test_buffers_that_end_inside_a_chunk():
    inside = {launch_form(c.place)[0] for c in PLACEMENT if c.total % 16}
    assert inside == {"wave", "block"}


@pytest.mark.parametrize("case", PLACEMENT, ids=ids(PLACEMENT))
def test_a_gap_byte_counted_into_a_row_changes_that_row(case):
    buf, want, _ = case_data(case)
    greatest = GREATEST[case.in_u8]
    codes = row_codes(case).view(torch.uint8).numpy()
    assert (_ordered(codes, np.uint8 if case.in_u8 else np.int8) < _ordered(np.asarray([greatest], np.uint8), np.uint8 if case.in_u8 else np.int8)).all()
    mask = np.ones(case.total, bool)
    for r in range(case.rows):
        mask[r * case.in_pitch:r * case.in_pitch + case.L] = False
    assert case.in_pitch > case.L and mask.sum() == (case.rows - 1) * (case.in_pitch - case.L) and np.all(buf[mask] == greatest)
    longer = np.concatenate([buf, np.asarray([greatest], np.uint8)])            # (the last row's neighbour lies behind the buffer)
    other = _oracle(case, longer, extend=1).reshape(case.rows, case.out_pitch + 1)[:, :case.L]
    changed = (other != as_rows(case, want)[:, :case.L]).any(axis=1)
    assert changed.all(), (case.name, np.flatnonzero(~changed))


# ------------------------------------------------------------------------------------------------
# (c) edge values
# ------------------------------------------------------------------------------------------------

def _named(prefix):
    found = [c for c in EDGE if c.name.startswith(prefix)]
    assert found, prefix
    return found


def test_edge_cases_run_in_both_forms():
    for c in EDGE:
        if c.form:
            assert launch_form(c.place) == ("wave" if c.form == 1 else "block", 1)
            other = c._replace(name=c.name[:-1] + str(3 - c.form), form=3 - c.form)
            assert other in EDGE and np.array_equal(case_data(other)[0], case_data(c)[0]), c.name
    assert sum(1 for c in EDGE if not c.form) == 4


def test_ties():
    parity = set()
    for k in TIE_KS:
        scale_a, d, j, s_b = tie(k)
        assert 2 <= len(d) <= 5 and max(d) < 24 and scale_a in (0.0731, 2.0 ** -3, 0.25)
        for c in _named(f"tie {k} "):
            _, want, seen = case_data(c)
            want = as_rows(c, want)
            for r in range(c.rows):
                at = (j + r) % c.L                                                # the differences are rotated by r
                assert seen[r]["prod"][at] == F32(k + 0.5) and seen[r]["prod"].dtype == F32
                assert want[r, at] == (k if k % 2 == 0 else k + 1)                # to the even code
                if k % 2 == 0:
                    assert want[r, at] != int(np.floor(float(seen[r]["prod"][at]) + 0.5))       # round-half-up gives k + 1
        parity.add(k % 2)
    assert parity == {0, 1}


def test_clamps():
    for c in _named("clamp "):
        _, want, seen = case_data(c)
        _, zp, lo, hi = c.out_form
        codes = as_rows(c, want)[:, :c.L]
        codes = (codes if c.out_u8 else codes.view(np.int8)).astype(np.int64)
        at_lo, at_hi = int((codes == lo).sum()), int((codes == hi).sum())
        assert at_lo > 0 and at_hi > 0 and 2 * (at_lo + at_hi) < codes.size, (c.name, at_lo, at_hi)
        q = np.stack([s["q"] for s in seen])
        kind = c.name.split()[1]
        if kind in ("top", "int8"):                                               # a one-hot row: 256 + zp is one more than the domain holds
            assert q.max() == 256 + zp == hi + 1
        if kind == "bottom":
            assert q.min() < lo and q.max() > hi
        if kind == "4-bit":
            assert (lo, hi) == (0, 15) and q.max() == 15 and len(np.unique(codes)) > 4
        if kind == "int8":
            assert zp == -128 == lo and not c.out_u8


def test_zero_table_entries():
    firsts = {}
    for scale_a in (1.0, 8.0):
        E = ops.softmax_exp_table(scale_a)
        firsts[scale_a] = int(np.argmax(E == 0))
        assert E[firsts[scale_a] - 1] > 0 and not E[firsts[scale_a]:].any()
        for c in _named(f"zero entries {scale_a} "):
            _, want, seen = case_data(c)
            want = as_rows(c, want)
            for r in range(c.rows):
                assert seen[r]["S"] == 2 ** 24 and (seen[r]["d"] == 0).sum() == 1 and np.sort(seen[r]["d"])[1] == 18
                assert (seen[r]["d"] >= 18).sum() == c.L - 1 and seen[r]["d"].max() > 100
                hot = int(np.argmax(seen[r]["d"] == 0))
                assert want[r, hot] == 255 and not np.delete(want[r, :c.L], hot).any()               # B's code of 1.0, and of 0.0
            assert len({int(np.argmax(s["d"] == 0)) // 16 for s in seen}) == 3                     # the maximum in every chunk of the row
    assert firsts == {1.0: 18, 8.0: 3}


def test_full_width_sums():
    for L, form in ((4064, ("wave", 4)), (32736, ("block", 8))):
        (equal,), (mixed,) = _named(f"equal rows {L}"), _named(f"adjacent codes {L}")
        for c in (equal, mixed):
            assert launch_form(c.place) == form and c.in_pitch == c.out_pitch == L + 1 and slots(L + 1, L + 1) == (256 if L == 4064 else 2048)
        _, want, seen = case_data(equal)
        assert all(s["S"] == L * 2 ** 24 >= 2 ** 32 for s in seen)
        codes = as_rows(equal, want)[:, :L]
        assert len(np.unique(codes)) == 1 and codes[0, 0] == round(1 / L / equal.out_form[0]) and 100 < codes[0, 0] < 255
        _, want, seen = case_data(mixed)
        E = ops.softmax_exp_table(mixed.scale_a)
        for r, s in enumerate(seen):
            assert set(np.unique(s["d"]).tolist()) == {0, 1} and s["S"] >= 2 ** 32
            partial = np.bincount(lanes_of(mixed.place, r), weights=s["e"].astype(np.float64)).astype(np.int64)   # (< 2^53: exact)
            assert partial.sum() == s["S"] and partial.max() < 2 ** 32                                              # a lane's sum fits 32 bits
            if L == 32736:
                assert s["S"] > 2 ** 38 and int(F32(s["S"])) != s["S"]                                              # float32(S) rounds
                if r == 0:                                                         # lane 0: 128 elements, all the maximum
                    assert partial[0] == partial.max() == 2 ** 31 >= 2 ** 31 - int(E[1]) and (lanes_of(mixed.place, 0) == 0).sum() == 128
        assert len(np.unique(as_rows(mixed, want)[:, :L])) == 2
    assert 32736 * 2 ** 24 < 2 ** 39


def test_extremes():
    for in_u8 in (False, True):
        lo, hi = LEAST[in_u8], GREATEST[in_u8]
        for c in _named(f"extremes {'u8' if in_u8 else 'i8'} "):
            buf, want, seen = case_data(c)
            rows = row_codes(c).view(torch.uint8).numpy()
            assert (rows[0, 17], rows[0, 18]) == (lo, hi) and (rows[3, 0], rows[3, 1]) == (hi, lo)
            assert seen[0]["d"][17] == 255 == seen[3]["d"][1] and seen[0]["d"][18] == 0 == seen[3]["d"][0]
            assert int(np.argmin(seen[1]["d"])) == c.L - 1 and (seen[1]["d"] == 0).sum() == 1      # the maximum last,
            assert int(np.argmin(seen[2]["d"])) == 0 and (seen[2]["d"] == 0).sum() == 1            # first
            assert ops.softmax_exp_table(c.scale_a)[255] > 0                                        # the least code still adds to S
            # ordered as raw bytes instead, the least int8 code would be the maximum
            if not in_u8:
                assert lo > hi
    for c in _named("L = 1 "):
        _, want, seen = case_data(c)
        assert all(s["S"] == 2 ** 24 and s["p"][0] == 1 for s in seen) and np.all(as_rows(c, want)[:, 0] == 255)


def test_pre_tables():
    assert np.array_equal(pre_table("identity"), np.arange(256)) and len(np.unique(pre_table("constant"))) == 1
    for c in _named("identity table "):
        assert np.array_equal(case_data(c)[1], _oracle(c._replace(pre=None), case_data(c)[0]))
    for c in _named("constant table "):
        _, want, seen = case_data(c)
        assert all(s["S"] == c.L * 2 ** 24 and not s["d"].any() for s in seen)
        assert len(np.unique(as_rows(c, want)[:, :c.L])) == 1 and len(np.unique(row_codes(c))) > 100
    for name, entries_u8 in (("tanh table int8 entries, uint8 bytes ", False), ("tanh table uint8 entries, int8 bytes ", True)):
        for c in _named(name):
            assert c.in_u8 == entries_u8 != c.raw_u8 and (row_codes(c).dtype == torch.uint8) == c.raw_u8
            table = pre_table(c.pre)
            assert len(np.unique(table)) > 8 and _ordered(table, np.int8).min() < 0                # both orders differ on the entries
            wrong = softmax_rows(case_data(c)[0], c.rows, c.L, c.in_pitch, c.out_pitch, np.int8 if c.in_u8 else np.uint8, c.out_form,
                                 c.pad_code, table, scale_a=c.scale_a)
            assert not np.array_equal(wrong, case_data(c)[1])                                      # the entries' type decides
