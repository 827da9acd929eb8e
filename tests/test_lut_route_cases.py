"""The cases of tests/test_gpu_lut_routes.py -- the float-output LUT fake-quant kernels (LutTableOp, LutOp<registers>, LutOp<lds>,
LutStepsOp and LutCellsOp of csrc/mctq_kernels.hpp behind mctq_lutt_*, mctq_lut_* and mctq_luts_*) on every launch route and at
edge values -- and, without a GPU, the proof that they reach what they claim.

Routes.  ``route`` replays launch_flat's heavy branch, launch_channels without its affine-only blocks (rows with the heavy U rule,
last axis, the window with its loop over tile forms and its LDS sum, the lean form of an op whose book leaves no room), nt_mode,
heavy_unroll, kFixedU (and NT = 1 for fixed-U ops) and steps_layout (csrc/mctq_lut_steps.hip) AS THEY STAND, and returns the exact
text of mctq_last_launch().  Whoever changes one of those functions changes the replay with it: the GPU file compares the whole
string on every call.

``cases(cus)`` is the one table; the tests below prove, for CU counts on both sides of the MI355X's 256, that it names every
route, every U / NT instance and every branch for every op, and that each shape satisfies the arithmetic of its route.

Expected values: oracle.mctq_oracle.lut_quantize on the values as stored, widened (lut_quantize_f64 for float64 input; step_dtype
where a per-tensor case sets step_round); a NaN input gives index 0, (lut[0] / mult) * thr.  No value comes from the library:
native.build_lut_steps only chooses INPUTS (the thresholds of the list, with their float32 neighbours).
"""
import collections
import functools
import zlib

import numpy as np
import pytest

from test_affine_route_cases import flat_branches, lastaxis_branches, rows_branches
from test_lut_index_cases import DIVISORS, LUTS as LUTS8, SPECIALS, narrow, rows_u, slab_rows, sweep, tensor_divisor

F32 = np.float32
T = 256                                                      # kThreads
DTYPES = ("float32", "float16", "bfloat16")
DT_CODE = {"float32": 0, "float16": 1, "bfloat16": 2}
VEC = {"float32": 4, "float16": 4, "bfloat16": 4}            # IO<TI, float>::N: the 16-byte lane vector is the OUTPUT's; a 16-bit
                                                             # input is read 8 bytes a lane (and must be 8-byte aligned)
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2}
CUS = (64, 104, 128, 228, 256, 304)
LDS_LIMIT = 64 * 1024
KWORDS = 4                                                   # LutCommon::kWords
DEFAULTS = {"heavy_unroll": 0, "nt": 1, "cached_store_max_mb": 32}
OPS = ("table", "registers", "lds", "steps", "cells")
OP_NAME = {"table": "LutTableOp", "registers": "LutOp<registers>", "lds": "LutOp<lds>", "steps": "LutStepsOp", "cells": "LutCellsOp"}
FIXED_U = {"table": 0, "registers": 2, "lds": 2, "steps": 4, "cells": 4}     # kFixedU
CELL_HEADER, CELL_MIN_P, CELL_MAX_PER = 4, 128, 4            # mctq_tb::kCellHeader, kCellMinP, kCellMaxPer


# ------------------------------------------------------------------------------------------------
# codebooks
# ------------------------------------------------------------------------------------------------

Book = collections.namedtuple("Book", "name op lut bits signed")


def _shuffled(seed, values):
    return [float(v) for v in np.random.default_rng(seed).permutation(np.asarray(values, dtype=np.int64))]


def _cells_codebook(seed, total, lo, hi, unit):
    """``total`` distinct integers of [lo, hi] in a shuffled order: a run ``unit`` apart (four hand-overs per cell of 4 unit), a
    run alternating unit and 2 unit (two or three per cell), a run 2 unit apart (two per cell), the rest spread over the remaining
    range (none or one per cell)."""
    runs, at = [], lo + 8 * unit
    for steps in ((unit,) * 40, (unit, 2 * unit) * 20, (2 * unit,) * 40):
        for s in steps:
            runs.append(at)
            at += s
        at += 16 * unit
    rest = total - len(runs)
    spread = np.linspace(at + 16 * unit, hi, rest).round().astype(np.int64)
    values = np.asarray(runs + spread.tolist(), dtype=np.int64)
    assert len(set(values.tolist())) == total and values.min() >= lo and values.max() <= hi and np.diff(spread).min() > 4 * unit
    return _shuffled(seed, values)


def _books():
    rng = np.random.default_rng(2024)
    l16 = LUTS8["l16"]
    t10 = [-512, 511] + rng.choice(np.arange(-511, 511), 62, replace=False).tolist()
    u12 = rng.choice(np.arange(0, 4096), 64, replace=False).tolist()
    s16 = rng.choice(np.arange(-32768, 32768), 4096, replace=False).tolist()
    out = [
        Book("t8s", "table", LUTS8["l256"], 8, True),                      # 511 entries: a book of 4096 bytes
        Book("t8u", "table", [0.0, 255.0, 9.0, 40.0, 100.0, 100.0, 180.0, 17.0, 254.0, 1.0], 8, False),
        Book("t10s", "table", _shuffled(1, t10), 10, True),               # 2047 entries: 16 KiB
        Book("r16", "registers", l16, 8, True),
        Book("r3dup", "registers", LUTS8["l3dup"], 8, True),
        Book("r1", "registers", LUTS8["l1"], 8, True),
        Book("r16q", "registers", LUTS8["l16q"], 8, True),                 # non-integer: no other kernel
        Book("l17", "lds", l16 + [100.0], 8, True),
        Book("l256", "lds", LUTS8["l256"], 8, True),
        Book("s2", "steps", [3.0, 3.0, -8.0], 12, True),                   # P = 2, a duplicate
        Book("s64", "steps", _shuffled(2, u12), 12, False),                # P = 64
        Book("s4096", "steps", _shuffled(3, s16), 16, True),               # P = 4096: 32 784 bytes, no room for a cell index
        Book("c128", "cells", _cells_codebook(4, 128, -2048, 2047, 1), 12, True),
        Book("c256", "cells", _cells_codebook(5, 256, -32768, 32767, 16), 16, True),
        Book("c2048", "cells", _cells_codebook(6, 2048, -32768, 32767, 2), 16, True),      # 49 184 bytes
    ]
    return collections.OrderedDict((b.name, b) for b in out)


BOOKS = _books()
BOOKS_OF = {op: tuple(b for b in BOOKS.values() if b.op == op) for op in OPS}


def domain(b):
    """(mult, clip_min, clip_max) of lut_values_bitwidth = b.bits."""
    mult = float(2 ** (b.bits - int(b.signed)))
    return (mult, float(-2 ** (b.bits - 1)), float(2 ** (b.bits - 1) - 1)) if b.signed else (mult, 0.0, float(2 ** b.bits - 1))


def distinct(b):
    return len(set(b.lut))


def first_centres(b):
    """float32 value of every centre (a duplicate's second index decides nothing: the values are those of the first)."""
    return np.unique(np.asarray(b.lut, dtype=F32))


def steps_p(b):
    p = 1
    while p < distinct(b):
        p <<= 1
    return p


def cells_for(p):
    return 0 if p < CELL_MIN_P else (1024 if p <= 256 else (4096 if p <= 1024 else 8192))       # mctq_tb::steps_cells_for


def steps_words(b):
    """n_words of the list mctq_lut_build_steps writes: 2 P + 2, and the cell index where it is appended (P >= 128, at most 64 KiB,
    at most four thresholds a cell: the cells books are built for that)."""
    p = steps_p(b)
    g = cells_for(p)
    has_cells = g and (2 * p + 2 + CELL_HEADER + g) * 4 <= LDS_LIMIT
    assert bool(has_cells) == (b.op == "cells"), b.name
    return 2 * p + 2 + (CELL_HEADER + g if has_cells else 0)


def steps_layout(n_words):
    """steps_layout of csrc/mctq_lut_steps.hip -> (P, cells)."""
    if n_words >= 4 and n_words % 2 == 0:
        p = (n_words - 2) // 2
        if 1 <= p <= 4096 and p & (p - 1) == 0:
            return p, False
    p = CELL_MIN_P
    while p <= 4096:
        if n_words == 2 * p + 2 + CELL_HEADER + cells_for(p):
            return p, True
        p <<= 1
    raise AssertionError(f"bad steps size {n_words}")


def table_entries(b):
    _, cmin, cmax = domain(b)
    return int(2 * (cmax - cmin) + 1)


def book_count(b):
    """The count argument behind the book pointer: entries, n_lut or n_words."""
    return table_entries(b) if b.op == "table" else len(b.lut) if b.op in ("registers", "lds") else steps_words(b)


def book_bytes(b):
    """Dynamic LDS of the op's book."""
    if b.op == "table":
        return (((table_entries(b) + 1) * 2 + 3) & ~3) * 4
    if b.op == "registers":
        return 0
    if b.op == "lds":
        return ((len(b.lut) + 3) & ~3) * 4
    return ((steps_words(b) + 3) & ~3) * 4


def lean_bytes(b):
    """LutCellsOp::lean_bytes: the list without its cell index."""
    return ((2 * steps_p(b) + 2 + 3) & ~3) * 4


@functools.lru_cache(maxsize=None)
def steps_list(name):
    """native.build_lut_steps (host code) of an integer codebook: to choose inputs, and as the book of the steps / cells ops."""
    from mct_quantizers_amd.hip import native
    b = BOOKS[name]
    st = native.build_lut_steps(b.lut, *domain(b))
    assert st is not None, name
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def value_table(name):
    from mct_quantizers_amd.hip import native
    b = BOOKS[name]
    tab = native.build_lut_table(b.lut, *domain(b))
    assert tab is not None and tab.shape == (table_entries(b) + 1, 2), name
    return tab


def cell_counts(name):
    """Thresholds per cell, read from the cell index behind the built list."""
    st = steps_list(name)
    p = steps_p(BOOKS[name])
    head = st[2 * p + 2:2 * p + 2 + CELL_HEADER]
    words = st[2 * p + 2 + CELL_HEADER:].view(np.uint32)
    assert words.size == int(head[0]) == cells_for(p)
    return (words >> 16).astype(np.int64), int(head[1])


# ------------------------------------------------------------------------------------------------
# the launchers' arithmetic
# ------------------------------------------------------------------------------------------------

def tuned(**keys):
    t = dict(DEFAULTS)
    t.update(keys)
    return t


def nt_mode(out_bytes, t):
    if t["nt"] != 1:
        return t["nt"]
    cap = t["cached_store_max_mb"] << 20
    return 2 if cap > 0 and out_bytes <= cap else 1


def _text(kernel, op_name, dt, u, nt):
    return f"{kernel}<{op_name},in{ESIZE[dt]}B,out4B,U={u},NT={nt}>"


def window_plan(book, C, inner, N, vec_ok):
    """launch_channels' loop over wu -> (vector form?, wu, tile, staged rows, LDS bytes); the last form tried is returned even
    where it does not fit."""
    wu = 4
    while True:
        tile = T * wu * (N if vec_ok else 1)
        entries = min(C, (tile - 1 + inner - 1) // inner + 1)
        lds = book + (entries | 1) * KWORDS * 4
        if lds <= LDS_LIMIT or wu == 1 or not vec_ok:
            return vec_ok, wu, tile, entries, lds
        wu = 1


def route(b, dt, kind, shape, x_aligned=True, y_aligned=True, t_aligned=True, cus=256, tuning=None):
    """-> (mctq_last_launch() after the call, or None for a refusal; what the note does not show)."""
    t = tuned(**(tuning or {}))
    N = VEC[dt]
    vec_ok = x_aligned and y_aligned
    name, fixed, bbytes = OP_NAME[b.op], FIXED_U[b.op], book_bytes(b)
    if b.op in ("steps", "cells"):
        assert steps_layout(steps_words(b)) == (steps_p(b), b.op == "cells")
    n = int(np.prod(shape))
    assert n > 0
    nt = 1 if fixed else nt_mode(n * 4, t)
    if kind == "tensor":
        if not vec_ok:
            return _text("flat_scalar_kernel", name, dt, 1, 0), {"blocks": min(-(-n // T), 32 * cus)}
        u = fixed or (t["heavy_unroll"] or 4)
        return _text("flat_kernel", name, dt, u, nt), {"U": u}
    outer, C, inner = shape
    if vec_ok and inner % N == 0 and inner // N >= T:
        u = rows_u(inner // N)
        if t["heavy_unroll"]:
            u = t["heavy_unroll"]
        if fixed:
            u = fixed
        return _text("rows_kernel", name, dt, u, nt), {"U": u}
    if vec_ok and inner == 1 and C % N == 0 and t_aligned:
        k = slab_rows(C // N)
        if k * (C // N) < 1 << 24:
            return _text("lastaxis_kernel", name, dt, 2, nt), {"U": 2, "k": k}
    lean = False
    vec, wu, tile, entries, lds = window_plan(bbytes, C, inner, N, vec_ok)
    if lds > LDS_LIMIT:
        if b.op != "cells":
            return None, {"lds": lds}
        lean, name = True, OP_NAME["steps"]                      # LutCellsOp::lean: kFixedU = 4 as well
        vec, wu, tile, entries, lds = window_plan(lean_bytes(b), C, inner, N, vec_ok)
        assert lds <= LDS_LIMIT
    info = {"wu": wu, "V": N if vec else 1, "tile": tile, "entries": entries, "lds": lds, "lean": lean}
    if not vec:
        return _text("window_kernel<scalar>", name, dt, 4, 1), info
    return _text("window_kernel<vector>", name, dt, wu, nt), info


def window_branches(n, inner, C, V, wu, vec):
    """window_kernel's index arithmetic on every block: which branches a shape runs."""
    tile = T * wu * (V if vec else 1)
    step = V if vec else 1
    out = set()
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        row0, rem0 = divmod(e0, inner)
        nrows = (rem0 + count - 1) // inner + 1
        whole, c0 = C <= nrows, row0 % C
        out.add("whole" if whole else "partial")
        if not whole and c0 + nrows > C:
            out.add("wrap")
        out.add("small" if rem0 + tile < 1 << 24 and c0 + nrows < 1 << 24 else "wide")
        off = np.arange(T * wu, dtype=np.int64) * step
        off = off[off < count]
        pos = rem0 + off
        lrow, lrem = pos // inner, pos % inner
        full = (off + step <= count) if vec else np.zeros(off.size, bool)
        if vec and full.any():
            if inner % V == 0:
                out.add("same_row")
            elif inner >= V:
                inside = full & (lrem + V <= inner)
                cross = full & ~inside
                if inside.any():
                    out.add("inside")
                if cross.any():
                    out.add("crossing")
                    li = (c0 + lrow) % C if whole else lrow
                    if whole and (li[cross] + 1 == C).any():
                        out.add("li2==channels")
            else:
                out.add("walk")
        if (~full).any():
            out.add("tail" if vec else "scalar")
    return out


def window_wave_kinds(n, inner, C, V, wu, fast):
    """The outcomes of window_kernel's ballot (lane vectors inside one row only: the others never ask): per wave and lane
    vector "fast" (every active lane's channel can take the exact-reciprocal division), "ieee" (none can) or "mixed"."""
    fast = np.asarray(fast, bool)
    tile = T * wu * V
    out = set()
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        row0, rem0 = divmod(e0, inner)
        for u in range(wu):
            off = (u * T + np.arange(T, dtype=np.int64)) * V
            pos = rem0 + off
            asks = (off + V <= count) & ((inner % V == 0) | (pos % inner + V <= inner))
            c = (row0 + pos // inner) % C
            for w in range(T // 64):
                lanes = slice(64 * w, 64 * (w + 1))
                if asks[lanes].any():
                    f = fast[c[lanes]][asks[lanes]]
                    out.add("fast" if f.all() else "ieee" if not f.any() else "mixed")
    return out


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------

# shape: (n,) or (outer, C, inner); xoff / yoff: elements past a 16-byte boundary; toff: thresholds, 4-byte words past one;
# step: the per-tensor call passes step_round = the storage type; route: the family the row is filed under; u: the U it names
Case = collections.namedtuple("Case", "id op book dt kind shape xoff yoff toff tuning route u step")
KERNEL = {"flat": "flat_kernel<", "flat_scalar": "flat_scalar_kernel<", "rows": "rows_kernel<", "lastaxis": "lastaxis_kernel<",
          "window": "window_kernel<vector><", "window_scalar": "window_kernel<scalar><"}
STEP_BOOKS = ("t8s", "r16", "r16q", "l17", "l256")          # 8-bit signed: bounds a 16-bit type holds exactly


def wu1_pair(book, N):
    """inner == 1: the largest channel count with C % N != 0 whose four-vector window fits beside the book, and the smallest
    above it with C % N != 0 (C % N == 0 with aligned thresholds is the last-axis route)."""
    fits = lambda C: book + (C | 1) * KWORDS * 4 <= LDS_LIMIT
    c4 = (LDS_LIMIT - book) // (KWORDS * 4)
    while not fits(c4) or c4 % N == 0:
        c4 -= 1
    c1 = c4 + 1
    while fits(c1) or c1 % N == 0:
        c1 += 1
    return c4, c1


def _op_rows(op, dt, cus):
    """(tag, kind, shape, route, u | None, offsets, tuning, book name | None, step) of one op and storage type."""
    N, fixed = VEC[dt], FIXED_U[op]
    rows = []
    add = lambda tag, shape, route_, u=None, off=(0, 0, 0), tuning=None, book=None, step=False: rows.append(
        (tag, "tensor" if len(shape) == 1 else "channel", shape, route_, u, off, tuning or {}, book, step))
    fu = fixed or 4
    for n in (1, N, 1024 * N, 1024 * N + N + 1, 2348 * N + 3):
        add(f"flat-{n}", (n,), "flat", fu)
    add("flat-scalar-x+1", (2348 * N + 3,), "flat_scalar", 1, (1, 0, 0))
    add("flat-scalar-y+1", (2348 * N + 3,), "flat_scalar", 1, (0, 1, 0))
    add("flat-scalar-second-pass", (32 * cus * T + 1000,), "flat_scalar", 1, (1, 0, 0), book=BOOKS_OF[op][0].name)
    if dt != "float32":
        for bk in (b.name for b in BOOKS_OF[op] if b.name in STEP_BOOKS):
            add("flat-step-round", (1024 * N + N + 1,), "flat", fu, book=bk, step=True)
            add("flat-scalar-step-round", (3 * T + 5,), "flat_scalar", 1, (1, 0, 0), book=bk, step=True)
    if not fixed:
        for hu in (1, 2, 4):
            for mb in (32, 0):
                keys = {"heavy_unroll": hu, "cached_store_max_mb": mb}
                add("flat-tuned", (1024 * N + N + 1,), "flat", hu, tuning=keys)
                add("rows-tuned", (2, 3, 1040), "rows", hu, tuning=keys)
        for inner, u in ((1024, 1), (2048, 2), (4096, 4), (3584, 4), (3580, 1), (1040, 1)):
            add(f"rows-{inner}", (2, 3, inner), "rows", u)
        for shape, route_ in (((37, 64, 1), "lastaxis"), ((3, 5, 7), "window")):
            add(route_ + "-nt", shape, route_, tuning={"cached_store_max_mb": 0})
    else:
        add("rows-one-tile", (2, 3, 1024), "rows", fixed)
        add("rows-ragged", (2, 3, 4100), "rows", fixed)
    k64, k3 = slab_rows(64 // N), slab_rows(3)
    for shape in ((37, 64, 1), (2 * k64 + 3, 64, 1), (2 * k3 + 1, 3 * N, 1), (1, 8, 1)):
        add("lastaxis", shape, "lastaxis", 2)
    if op == "cells":
        add("lastaxis-1024-channels", (5, 1024, 1), "lastaxis", 2, book="c2048")
    for shape in ((3, 5, 1), (3, 5, 3), (3, 5, 7), (3, 5, 8), (2, 40, 200)):
        add("window", shape, "window", 4)
    add("window-thresholds+4", (41, 64, 1), "window", 4, (0, 0, 1))
    for b in BOOKS_OF[op]:
        c4, c1 = wu1_pair(book_bytes(b), N)
        add("window-still-four", (2, c4, 1), "window", 4, book=b.name)
        # (the lean form of the largest cells book has the whole table in its four-vector window again)
        add("window-one-vector", (2, c1, 1), "window", 4 if b.name == "c2048" else 1, book=b.name)
    if op == "cells":                                           # item 4: no window fits beside 49 184 bytes
        add("window-no-room-C1022", (2, 1022, 1), "window", 4, (0, 0, 1), book="c2048")
        add("window-no-room-C4097", (2, 4097, 1), "window", 1, (0, 0, 1), book="c2048")     # its lean form at wu = 1
    return rows


@functools.lru_cache(maxsize=None)
def cases(cus):
    out = []
    for dt in DTYPES:
        for op in OPS:
            books = BOOKS_OF[op]
            base = _op_rows(op, dt, cus)
            more = []
            for j, (tag, kind, shape, route_, u, off, tuning, book, step) in enumerate(base):
                if kind == "channel":
                    # every per-channel case again with x, then y, one element off: window_kernel<scalar>, whatever the
                    # tuning keys and the thresholds' alignment
                    more.append((tag + "-x+1", kind, shape, "window_scalar", 4, (1, 0, off[2]), tuning, book, step))
                    more.append((tag + "-y+1", kind, shape, "window_scalar", 4, (0, 1, off[2]), tuning, book, step))
            for j, (tag, kind, shape, route_, u, off, tuning, book, step) in enumerate(base + more):
                book = book or books[j % len(books)].name
                keys = "".join(f"-{k}{v}" for k, v in sorted(tuning.items()))
                size = "second-pass" if "second-pass" in tag else "x".join(map(str, shape))
                cid = f"{dt}-{op}-{tag}-{size}-{book}{keys}"
                out.append(Case(cid, op, book, dt, kind, shape, off[0], off[1], off[2], tuning, route_, u, step))
    assert len({c.id for c in out}) == len(out), [i for i, k in collections.Counter(c.id for c in out).items() if k > 1]
    return tuple(out)


def case_route(c, cus):
    return route(BOOKS[c.book], c.dt, c.kind, c.shape, c.xoff == 0, c.yoff == 0, c.toff == 0, cus, c.tuning)


# ------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------

# (name, threshold, eps) of the per-tensor sweeps: the four of DIVISORS and a zero threshold (0 / 0: a NaN inside the chain,
# x / 0: infinities; (lut / mult) * 0: a signed zero)
TENSOR_DIVISORS = DIVISORS + (("0", 0.0, 0.0),)
# the thresholds of the per-channel sweeps, eps = 0, channel c -> set c % 5: 1.7 and 1.0 divide fast, the others by IEEE
MIXED = (1.7, 2.0 ** 70, 2.0 ** -70, 1.0, 0.0)
MIXED_FAST = tuple(2.0 ** -60 < v < 2.0 ** 60 for v in MIXED)
# window_kernel's ballot: 192 channels, a lane vector a row, 64 consecutive rows a wave: waves of fast, of IEEE, of mixed channels
WAVES_C = 192
WAVES_SETS = np.concatenate([np.tile([0, 3], 32), np.tile([1, 2, 4, 1], 16), np.tile([0, 1, 3, 2, 4, 0, 3, 1], 8)])


def _oracle(x, b, thr, eps, per_channel=False, step_dtype="float32"):
    from oracle import mctq_oracle as O
    chunk = max(1, (1 << 22) // len(b.lut))
    if per_channel:
        return O.lut_quantize(x, b.lut, np.asarray(thr, dtype=F32), b.signed, b.bits, eps, per_channel=True, channel_axis=1,
                              chunk_elems=chunk)
    return O.lut_quantize(x, b.lut, float(thr), b.signed, b.bits, eps, chunk_elems=chunk, step_dtype=step_dtype)


def wide(b):
    return not (b.bits == 8 and b.signed)


@functools.lru_cache(maxsize=None)
def t_points(name):
    """Wide ranges, in t: every threshold of the built list, every midpoint of adjacent sorted centres and both clip bounds, each
    with both float32 neighbours."""
    b = BOOKS[name]
    _, cmin, cmax = domain(b)
    st = steps_list(name)
    thr = st[1:distinct(b)]
    thr = thr[np.isfinite(thr)]
    srt = first_centres(b)
    mids = ((srt[:-1] + srt[1:]) * F32(0.5)).astype(F32)
    pts = np.concatenate([thr, mids, np.asarray([cmin, cmax], dtype=F32)]).astype(F32)
    pts = np.unique(np.concatenate([pts, np.nextafter(pts, F32(-np.inf)), np.nextafter(pts, F32(np.inf))]).astype(F32))
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def sweep_x(name, divisor, dt):
    """The sweep of a book for a divisor: the index cases' 8-bit sweep, or x = (t / mult) d (exact for powers of two) over
    t_points with the specials appended; narrowed to dt.  Read-only float32."""
    b = BOOKS[name]
    if not wide(b):
        return sweep(divisor, dt)
    with np.errstate(over="ignore"):
        x = ((t_points(name) / F32(domain(b)[0])) * F32(divisor)).astype(F32)
    x = narrow(np.concatenate([x, SPECIALS]).astype(F32), dt)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tensor_sweep(name, dname, dt, step=False):
    """-> (x, expected, thr_div, thr_mul) of a per-tensor sweep."""
    b = BOOKS[name]
    thr, eps = {d[0]: d[1:] for d in TENSOR_DIVISORS}[dname]
    x = sweep_x(name, float(tensor_divisor(thr, eps)) if thr else 1.0, dt)
    want = _oracle(x, b, thr, eps, step_dtype=dt if step else "float32")
    want.setflags(write=False)
    return x, want, float(tensor_divisor(thr, eps, dt if step else "float32")), float(F32(thr))


@functools.lru_cache(maxsize=None)
def channel_sweep(name, dt):
    """-> (X [L, 5], expected [L, 5]): column j is the sweep for MIXED[j] (for the zero threshold: the sweep of 1.0) and what
    the oracle gives a channel of that threshold with eps = 0."""
    b = BOOKS[name]
    X = np.stack([sweep_x(name, float(F32(v)) if v else 1.0, dt) for v in MIXED], axis=1)
    want = _oracle(X, b, np.asarray(MIXED, dtype=F32), 0.0, per_channel=True)
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


# route -> (kind, layout, x offset); layouts of sweep_layout
SWEEPS = collections.OrderedDict([
    ("flat", ("tensor", None, 0)), ("flat_scalar", ("tensor", None, 1)),
    ("rows", ("channel", "rows", 0)), ("lastaxis", ("channel", "columns8", 0)),
    ("window", ("channel", "columns5", 0)), ("window_scalar", ("channel", "columns5", 1)),
    ("window-waves", ("channel", "waves", 0)), ("window-wu1", ("channel", "sets", 0))])


def sweep_books(route_):
    """The ballot is the kernel's, not the op's: its sweep runs under the first book of every op."""
    return [b.name for b in BOOKS.values()] if route_ != "window-waves" else [BOOKS_OF[op][0].name for op in OPS]


def sweep_layout(route_, name, dt):
    """-> ((outer, C, inner), index into the sweep for every element (-1: a padding zero), threshold set of every channel).
    "rows": [2, 5, L padded to whole lane vectors and at least 256 of them]; "columns": [L, C, 1]; "waves": [L / V, 192, V],
    every channel sees the whole sweep in all three; "sets" (the one-vector window needs thousands of channels): channel c has
    set c % 5 and element [o, c] is value (K o + c // 5) mod L with K = floor(C / 5), so every SET sees the whole sweep."""
    layout = SWEEPS[route_][1]
    N = VEC[dt]
    L = sweep_x(name, 1.0, dt).size
    if layout == "rows":
        inner = max(-(-L // N) * N, T * N)
        idx = np.arange(inner)
        idx[idx >= L] = -1
        return (2, 5, inner), np.broadcast_to(idx, (2, 5, inner)), np.arange(5)
    if layout in ("columns8", "columns5"):
        C = int(layout[7:])
        return (L, C, 1), np.broadcast_to(np.arange(L)[:, None, None], (L, C, 1)), np.arange(C) % 5
    if layout == "waves":
        rows = -(-L // N)
        idx = np.arange(rows * N)
        idx[idx >= L] = -1
        return (rows, WAVES_C, N), np.broadcast_to(idx.reshape(rows, 1, N), (rows, WAVES_C, N)), WAVES_SETS
    assert layout == "sets"
    C = wu1_pair(book_bytes(BOOKS[name]), N)[1]
    K = C // 5
    outer = -(-L // K)
    idx = (np.arange(outer)[:, None] * K + (np.arange(C) // 5)[None, :]) % L
    return (outer, C, 1), idx[:, :, None], np.arange(C) % 5


def sweep_case(route_, name, dt):
    """-> (shape, x [shape], expected [shape], thresholds [C]) of a per-channel sweep."""
    shape, idx, sets = sweep_layout(route_, name, dt)
    X, W = channel_sweep(name, dt)
    s = np.broadcast_to(np.asarray(sets)[None, :, None], shape)
    pad = idx < 0
    x = np.where(pad, F32(0), X[np.maximum(idx, 0), s]).astype(F32)
    want = W[np.maximum(idx, 0), s]
    if pad.any():                                               # a padding zero: what the oracle gives 0.0 in that channel
        b = BOOKS[name]
        zero = _oracle(np.zeros((1, len(MIXED)), F32), b, np.asarray(MIXED, dtype=F32), 0.0, per_channel=True)[0]
        want = np.where(pad, zero[s], want)
    return shape, x, np.ascontiguousarray(want, dtype=F32), np.asarray(MIXED, dtype=F32)[np.asarray(sets)]


BLOCK = 65521                                                # a prime: the tiled inputs of the large case line up with no tile
PLANTED = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], dtype=F32)


def geometry_inputs(c, cus):
    """-> (x as stored, widened, shaped; threshold: a number per tensor, float32 [C] per channel; eps; expected).  Tie-heavy
    values (a third at midpoints of adjacent centres), every special at a fixed place of the launch and a NaN in its last element
    (the scalar tail where there is one); per channel ordinary thresholds with 2^70 on channel 1: fast and IEEE in one launch."""
    b = BOOKS[c.book]
    mult = F32(domain(b)[0])
    shape = c.shape                                             # (of cases(cus): the second-pass size follows the CU count)
    n = int(np.prod(shape))
    rng = np.random.default_rng([zlib.crc32(c.id.encode()), DT_CODE[c.dt]])
    srt = first_centres(b)
    mids = ((srt[:-1] + srt[1:]) * F32(0.5)).astype(F32) if srt.size > 1 else srt

    def values(shape_, thr_b):
        with np.errstate(over="ignore", invalid="ignore"):
            x = rng.standard_normal(shape_).astype(F32) * thr_b * F32(0.6)
            mid = mids[rng.integers(0, mids.size, size=shape_)] / mult * thr_b
            return np.where(rng.integers(0, 3, size=shape_) == 0, mid, x).astype(F32)

    def plant(x):
        flat = x.reshape(-1)
        if flat.size >= 8:
            flat[(np.arange(8) * flat.size) // 8] = PLANTED
        flat[-1] = np.nan
        return x

    if c.kind == "tensor":
        thr = 1.7
        step = c.dt if c.step else "float32"
        if n > BLOCK:                                           # the oracle on one block, the block repeated
            x1 = narrow(plant(values((BLOCK,), F32(thr))), c.dt)
            return np.resize(x1, n), thr, 1e-8, np.resize(_oracle(x1, b, thr, 1e-8, step_dtype=step), n)
        x = narrow(plant(values(shape, F32(thr))), c.dt)
        return x, thr, 1e-8, _oracle(x, b, thr, 1e-8, step_dtype=step)
    C = shape[1]
    thr = rng.uniform(0.05, 4.0, size=C).astype(F32)
    if C >= 3:
        thr[1] = F32(2.0 ** 70)
    x = narrow(plant(values(shape, thr.reshape(1, C, 1))), c.dt)
    return x, thr, 1e-8, _oracle(x, b, thr, 1e-8, per_channel=True)


# float64: (entry, shape); aligned and x one element off
F64_SHAPES = ((1,), (3,), (1027,), (3, 5, 1), (3, 5, 7), (2, 3, 1024))
F64_BOOKS = ("r16", "l17", "s64", "c256")
PLANTED64 = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, 1e300, -1e300], dtype=np.float64)


def f64_inputs(name, shape):
    """-> (x float64, threshold: a number or float32 [C], expected float32)."""
    from oracle import mctq_oracle as O
    b = BOOKS[name]
    mult = domain(b)[0]
    rng = np.random.default_rng([zlib.crc32(name.encode()), *shape])
    srt = first_centres(b).astype(np.float64)
    mids = (srt[:-1] + srt[1:]) * 0.5
    C = shape[1] if len(shape) == 3 else 1
    thr = rng.uniform(0.05, 4.0, size=C).astype(F32)
    thr[0] = F32(2.0)                                           # a power of two: the midpoints land exactly
    tb = thr.astype(np.float64).reshape(1, C, 1) if len(shape) == 3 else float(thr[0])
    x = rng.standard_normal(shape) * tb * 0.6
    mid = mids[rng.integers(0, mids.size, size=shape)] / mult * tb
    kind = rng.integers(0, 6, size=shape)
    x = np.where(kind == 0, mid, np.where(kind == 1, np.nextafter(mid, np.inf), np.where(kind == 2, np.nextafter(mid, -np.inf), x)))
    flat = x.reshape(-1)
    if flat.size >= 8:
        flat[(np.arange(8) * flat.size) // 8] = PLANTED64
    flat[-1] = np.nan
    if len(shape) == 3:
        want = O.lut_quantize_f64(x, b.lut, thr, b.signed, b.bits, 1e-8, per_channel=True, channel_axis=1)
        return x, thr, want
    want = O.lut_quantize_f64(x, b.lut, float(thr[0]), b.signed, b.bits, 1e-8)
    return x, float(thr[0]), want


# ------------------------------------------------------------------------------------------------
# tests (no GPU)
# ------------------------------------------------------------------------------------------------

def test_the_books_are_what_the_cases_assume():
    sizes = {n: book_bytes(b) for n, b in BOOKS.items()}
    assert sizes["t8s"] == sizes["t8u"] == 4096 and table_entries(BOOKS["t8s"]) == table_entries(BOOKS["t8u"]) == 511
    assert sizes["t10s"] == 16384 and table_entries(BOOKS["t10s"]) == 2047
    assert [len(BOOKS[n].lut) for n in ("r16", "r3dup", "r1", "r16q", "l17", "l256")] == [16, 3, 1, 16, 17, 256]
    assert distinct(BOOKS["r3dup"]) == 2 and any(v != int(v) for v in BOOKS["r16q"].lut)
    assert [steps_p(BOOKS[n]) for n in ("s2", "s64", "s4096", "c128", "c256", "c2048")] == [2, 64, 4096, 128, 256, 2048]
    assert sizes["s4096"] == 32784 and sizes["c2048"] == 49184 and lean_bytes(BOOKS["c2048"]) == 16400
    from mct_quantizers_amd.hip import native
    for name, b in BOOKS.items():
        mult, cmin, cmax = domain(b)
        integer = all(v == int(v) for v in b.lut)
        assert (native.build_lut_table(b.lut, mult, cmin, cmax) is not None) == (integer and b.bits <= 10), name
        if b.op == "table":
            value_table(name)
        if b.op in ("steps", "cells"):
            assert steps_list(name).size == steps_words(b), (name, steps_list(name).size)      # a cell index was appended, or not
            assert steps_layout(steps_list(name).size) == (steps_p(b), b.op == "cells")
        if b.op == "cells":
            per_cell, maxc = cell_counts(name)
            assert distinct(b) == steps_p(b)                    # the last threshold is T[P - 1]: min(1 + first + j, P - 1) is live
            assert per_cell.sum() == distinct(b) - 1 and maxc == per_cell.max() <= CELL_MAX_PER
            if b.bits == 16:
                assert set(per_cell.tolist()) == {0, 1, 2, 3, 4}, (name, sorted(set(per_cell.tolist())))
    assert native.build_lut_steps(BOOKS["r16q"].lut, *domain(BOOKS["r16q"])) is None
    # the divisor classes: p.r != 0 inside (2^-60, 2^60) only
    for _, thr, eps in TENSOR_DIVISORS:
        d = float(tensor_divisor(thr, eps))
        assert (2.0 ** -60 < abs(d) < 2.0 ** 60) == (thr in (1.0, 1.7))
    assert MIXED_FAST == (True, False, False, True, False)


def test_the_window_no_longer_refuses_any_book():
    """The refusal as it stood: 49 184 + 16 * 1025 > 65 536, so the one-vector tile (1024 rows and one, whatever the input type:
    the lane vector is the float32 output's) had no room beside the cells book of 1025 ... 2048 centres, and the unaligned form
    has the same tile; the list alone (16 400 bytes) has."""
    big = book_bytes(BOOKS["c2048"])
    assert big + 16 * 1025 > LDS_LIMIT >= big + 16 * 1021
    for dt in DTYPES:
        for aligned in (True, False):
            plan = window_plan(big, 1022, 1, VEC[dt], aligned)
            assert plan[4] > LDS_LIMIT and plan[2] == 1024, (dt, aligned, plan)
            note, info = route(BOOKS["c2048"], dt, "channel", (2, 1022, 1), aligned, True, False)
            assert info["lean"] and "LutStepsOp" in note and info["lds"] <= LDS_LIMIT, note
            assert note.startswith("window_kernel<vector><" if aligned else "window_kernel<scalar><")
    assert route(BOOKS["c2048"], "float32", "channel", (5, 1024, 1))[0] == "lastaxis_kernel<LutCellsOp,in4B,out4B,U=2,NT=1>"
    s = book_bytes(BOOKS["s4096"])                              # the largest book without a lean form: room for 1025 rows
    assert LDS_LIMIT >= s + 16 * 1025
    assert route(BOOKS["s4096"], "bfloat16", "channel", (2, 2049, 1))[0] == "window_kernel<vector><LutStepsOp,in2B,out4B,U=1,NT=1>"
    for b in BOOKS.values():                                    # whatever the shape: some form fits
        for dt in DTYPES:
            for C in (1021, 1022, 1025, 2047, 2049, 4097, 9001):
                for inner in (1, 2, 3):
                    for aligned in (True, False):
                        assert route(b, dt, "channel", (2, C, inner), aligned, True, False)[0] is not None, (b.name, dt, C, inner)


def test_the_one_vector_thresholds_per_book():
    got = {b.name: wu1_pair(book_bytes(b), 4) for b in BOOKS.values()}
    assert got["t8s"] == (3839, 3841) and got["t10s"] == (3071, 3073) and got["r16"] == (4095, 4097), got
    assert got["l256"] == (4031, 4033) and got["s4096"] == (2047, 2049) and got["c2048"] == (1021, 1022), got


def _required_notes(op, dt):
    name, fixed = OP_NAME[op], FIXED_U[op]
    out = {_text("flat_scalar_kernel", name, dt, 1, 0), _text("window_kernel<scalar>", name, dt, 4, 1)}
    if fixed:
        out |= {_text("flat_kernel", name, dt, fixed, 1), _text("rows_kernel", name, dt, fixed, 1),
                _text("lastaxis_kernel", name, dt, 2, 1), _text("window_kernel<vector>", name, dt, 4, 1),
                _text("window_kernel<vector>", name, dt, 1, 1)}
        if op == "cells":
            out |= {_text("window_kernel<vector>", "LutStepsOp", dt, u, 1) for u in (4, 1)} | {_text("window_kernel<scalar>", "LutStepsOp", dt, 4, 1)}
        return out
    for nt in (1, 2):
        out |= {_text(k, name, dt, u, nt) for k in ("flat_kernel", "rows_kernel") for u in (1, 2, 4)}
        out |= {_text("lastaxis_kernel", name, dt, 2, nt), _text("window_kernel<vector>", name, dt, 4, nt)}
    out.add(_text("window_kernel<vector>", name, dt, 1, 2))
    return out


REQUIRED_BRANCHES = {"flat/full", "flat/guarded", "flat/tail", "rows/full", "rows/guarded", "rows/tiles_per_row=1",
                     "rows/tiles_per_row>1", "rows/row>=channels", "lastaxis/full_group", "lastaxis/short_group",
                     "lastaxis/idle_lanes", "window/whole", "window/partial", "window/wrap", "window/small", "window/same_row",
                     "window/inside", "window/crossing", "window/li2==channels", "window/walk", "window/tail", "window/wu=4",
                     "window/wu=1", "window_scalar/whole", "window_scalar/partial", "window_scalar/wrap", "window_scalar/scalar"}


def _branches(c, cus):
    note, info = case_route(c, cus)
    N = VEC[c.dt]
    n = int(np.prod(c.shape))
    if c.route == "flat":
        got = flat_branches(n, N, info["U"])
    elif c.route == "rows":
        got = rows_branches(c.shape[0] * c.shape[1], c.shape[1], c.shape[2] // N, info["U"])
    elif c.route == "lastaxis":
        got = lastaxis_branches(c.shape[0], c.shape[1], N, False)
    elif c.route in ("window", "window_scalar"):
        got = window_branches(n, c.shape[2], c.shape[1], N, info["wu"], info["V"] > 1)
        if info["V"] > 1:
            got.add(f"wu={info['wu']}")
    else:
        got = set()
    return {f"{c.route}/{b}" for b in got}


@pytest.mark.parametrize("cus", CUS)
def test_the_table_names_every_route_instance_and_branch_for_every_op(cus):
    table = cases(cus)
    assert [c.id for c in table] == [c.id for c in cases(256)]
    for dt in DTYPES:
        for op in OPS:
            notes, branches = set(), set()
            mine = [c for c in table if c.dt == dt and c.op == op]
            assert {c.book for c in mine} == {b.name for b in BOOKS_OF[op]}
            for c in mine:
                note, info = case_route(c, cus)
                assert note is not None and note.startswith(KERNEL[c.route]), f"{c.id} (cus = {cus}) goes to {note}"
                if c.u is not None:
                    assert f",U={c.u}," in note, f"{c.id} (cus = {cus}): {note}, filed under U = {c.u}"
                notes.add(note)
                branches |= _branches(c, cus)
            need = _required_notes(op, dt)
            assert not need - notes, (dt, op, sorted(need - notes))
            assert not REQUIRED_BRANCHES - branches, (dt, op, sorted(REQUIRED_BRANCHES - branches))
            if dt != "float32" and any(b.name in STEP_BOOKS for b in BOOKS_OF[op]):
                assert {c.route for c in mine if c.step} == {"flat", "flat_scalar"}


def test_shapes_satisfy_the_arithmetic_of_their_route():
    for cus in (64, 256, 304):
        for c in cases(cus):
            note, info = case_route(c, cus)
            N, b = VEC[c.dt], BOOKS[c.book]
            n = int(np.prod(c.shape))
            what = f"{c.id} (cus = {cus})"
            if "second-pass" in c.id:                            # more blocks than the capped grid, by less than another grid
                assert 32 * cus < -(-n // T) < 2 * 32 * cus, f"{what}: the cap of the flat scalar grid is no longer 32 blocks a CU"
            if c.route == "rows":
                innerv = c.shape[2] // N
                assert c.shape[2] % N == 0 and innerv >= T, f"{what}: the rows route no longer starts at {T} lane vectors"
                if not FIXED_U[c.op] and not c.tuning.get("heavy_unroll"):
                    cap = -(-innerv // (T * c.u)) * T * c.u
                    assert (cap - innerv) * 8 <= cap or c.u == 1, f"{what}: the idle-lane bound of the heavy rows rule moved"
                    if innerv == 896:                            # exactly 1/8 idle: still the widest tile
                        assert (cap - innerv) * 8 == cap and c.u == 4, what
                    if innerv == 895:                            # one lane vector more idle: no U qualifies
                        assert all((-(-innerv // (T * u)) * T * u - innerv) * 8 > -(-innerv // (T * u)) * T * u for u in (4, 2, 1)), what
            if c.route == "lastaxis":
                assert c.shape[2] == 1 and c.shape[1] % N == 0 and c.toff == 0, what
            if c.route == "window" and "still-four" in c.id:
                assert info["wu"] == 4 and info["entries"] == c.shape[1] and LDS_LIMIT - info["lds"] < 3 * KWORDS * 4, \
                    f"{what}: the LDS sum of the window moved ({info})"
            if c.route == "window" and "one-vector" in c.id:
                four = book_bytes(b) + (min(c.shape[1], T * 4 * N) | 1) * KWORDS * 4
                assert four > LDS_LIMIT, f"{what}: a four-vector window fits again"
                assert info["wu"] == c.u and info["lean"] == (c.book == "c2048"), what
            if "no-room" in c.id:
                assert info["lean"] and "LutStepsOp" in note, f"{what}: {note}"
            if c.route == "window_scalar":
                assert info["V"] == 1 and info["wu"] == 4 and info["tile"] == 4 * T, what


@pytest.mark.parametrize("dt", DTYPES)
def test_the_waves_of_the_ballot_sweep(dt):
    """From the kernel's lane-to-channel arithmetic: the waves table has waves whose lanes all divide fast, waves where none does
    and mixed waves; the five-channel column layout never asks (inner < V: apply<false>)."""
    N = VEC[dt]
    assert WAVES_SETS.size == WAVES_C
    name = BOOKS_OF["table"][0].name
    shape, idx, sets = sweep_layout("window-waves", name, dt)
    note, info = route(BOOKS[name], dt, "channel", shape)
    assert note.startswith("window_kernel<vector><") and info["wu"] == 4
    fast = np.asarray(MIXED_FAST)[sets]
    assert window_wave_kinds(int(np.prod(shape)), shape[2], shape[1], N, 4, fast) == {"fast", "ieee", "mixed"}
    for lo, kind in ((0, {True}), (64, {False}), (128, {True, False})):
        assert set(fast[lo:lo + 64].tolist()) == kind
        assert set(np.asarray(sets)[lo:lo + 64].tolist()) >= ({0, 3} if lo == 0 else {1, 2, 4})      # every divisor of the kind
    # every channel holds the whole sweep: NaN, +inf and -inf in each kind of wave
    L = sweep_x(name, 1.0, dt).size
    seen = np.zeros((WAVES_C, L), bool)
    ch = np.broadcast_to(np.arange(WAVES_C)[None, :, None], shape)
    seen[ch[idx >= 0], idx[idx >= 0]] = True
    assert seen.all()
    shape5, _, _ = sweep_layout("window", name, dt)
    assert window_wave_kinds(int(np.prod(shape5)), 1, 5, N, 4, np.asarray(MIXED_FAST)) == set()


@pytest.mark.parametrize("cus", (64, 256, 304))
def test_the_value_sweeps_reach_their_routes(cus):
    for route_, (kind, layout, xoff) in SWEEPS.items():
        for name in sweep_books(route_):
            for dt in DTYPES:
                b = BOOKS[name]
                L = sweep_x(name, 1.0, dt).size
                if kind == "tensor":
                    note, _ = route(b, dt, "tensor", (L,), xoff == 0, cus=cus)
                    assert note.startswith(KERNEL[route_]), (route_, name, dt, note)
                    continue
                shape, idx, sets = sweep_layout(route_, name, dt)
                assert idx.shape == shape and idx.size <= 1 << 21, (route_, name, dt, shape)
                note, info = route(b, dt, "channel", shape, xoff == 0, cus=cus)
                fam = route_.split("-")[0]
                assert note.startswith(KERNEL[fam]), (route_, name, dt, note)
                if route_ == "window-wu1":                      # one vector a lane, or the lean form where that has no room
                    assert info["wu"] == 1 or info["lean"], (name, dt, info)
                elif fam == "window":
                    assert info["wu"] == 4 and not info["lean"]
                # every channel (sets layout: every threshold set) holds the whole sweep
                key = np.broadcast_to(np.asarray(sets)[None, :, None] if layout == "sets" else np.arange(shape[1])[None, :, None], shape)
                seen = np.zeros((5 if layout == "sets" else shape[1], L), bool)
                seen[key[idx >= 0], idx[idx >= 0]] = True
                assert seen.all(), (route_, name, dt)
                assert set(np.asarray(sets).tolist()) == set(range(5))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("name", list(BOOKS))
def test_the_sweeps_are_not_empty(name):
    """For the oracle alone: the expected output of every sweep holds every first-occurrence centre of the codebook (float16 at
    2^70 / 2^-70 and bfloat16 at 2^-70 hold -inf, 0, +inf and NaN only: the clip bounds' and zero's centres), a duplicate's second
    index decides nothing (the values are those of the first), a NaN input gives (lut[0] / mult) * thr, two channels differ."""
    b = BOOKS[name]
    mult = F32(domain(b)[0])
    centres = first_centres(b)
    for dt in DTYPES:
        for dname, thr, eps in TENSOR_DIVISORS:
            x, want, div, mul = tensor_sweep(name, dname, dt)
            assert want.shape == x.shape and np.isnan(x).sum() == 1
            values = set(_bits((centres / mult) * F32(thr)).tolist())
            got = set(_bits(want).tolist())
            assert got <= values, (name, dt, dname)
            # (a 16-bit type cannot tell the points of a wide range apart: all centres for float32 there, several for the others)
            full = (thr in (1.0, 1.7) or (thr and (dt == "float32" or (dt == "bfloat16" and thr > 1)))) and (dt == "float32" or not wide(b))
            if full:
                assert got == values, (name, dt, dname, len(values - got))
            elif thr:
                assert len(got) >= min(3 if b.signed else 2, len(values)), (name, dt, dname, len(got))
            assert _bits(want[np.isnan(x)])[0] == _bits((F32(b.lut[0]) / mult) * F32(thr))[0]
        X, W = channel_sweep(name, dt)
        for j, thr in enumerate(MIXED):
            values = set(_bits((centres / mult) * F32(thr)).tolist())
            got = set(_bits(W[:, j]).tolist())
            assert got <= values
            if (j in (0, 3) or (j == 1 and dt != "float16") or (j == 2 and dt == "float32")) and (dt == "float32" or not wide(b)):
                assert got == values, (name, dt, thr, len(values - got))
            elif thr:
                assert len(got) >= min(3 if b.signed else 2, len(values)), (name, dt, thr, len(got))
            nan_rows = np.isnan(X[:, j])
            assert nan_rows.sum() == 1 and _bits(W[nan_rows, j])[0] == _bits((F32(b.lut[0]) / mult) * F32(thr))[0]
        if distinct(b) > 1:
            assert not np.array_equal(_bits(W[:, 0]), _bits(W[:, 3]))
    if name == "r3dup":                                         # index 1 repeats index 0's value: nothing else to tell them by
        assert b.lut[0] == b.lut[1]


@pytest.mark.parametrize("dt", DTYPES)
def test_expected_values_of_the_geometry_cases(dt):
    """Every case has an expectation of its shape that a NaN input produced part of; per channel, two channels differ."""
    for c in cases(256):
        if c.dt != dt or c.xoff or c.yoff or "second-pass" in c.id or c.tuning:
            continue                                            # (the offset and tuned forms share these inputs' construction)
        b = BOOKS[c.book]
        x, thr, eps, want = geometry_inputs(c, 256)
        assert want.shape == x.shape == tuple(c.shape) and np.isnan(x.reshape(-1)[-1]), c.id
        mult = F32(domain(b)[0])
        t_last = F32(thr) if c.kind == "tensor" else thr[(x.size - 1) // c.shape[2] % c.shape[1]]
        assert _bits(want)[-1] == _bits((F32(b.lut[0]) / mult) * t_last)[0], c.id
        if c.kind == "channel" and distinct(b) > 1 and x.size >= 64:
            per = [tuple(_bits(want[:, k]).tolist()) for k in range(min(c.shape[1], 4))]
            assert len(set(per)) > 1, c.id


def test_expected_values_of_the_float64_cases():
    for name in F64_BOOKS:
        for shape in F64_SHAPES:
            x, thr, want = f64_inputs(name, shape)
            assert x.dtype == np.float64 and want.dtype == F32 and want.shape == x.shape and np.isnan(x.reshape(-1)[-1])
            if x.size >= 8:
                assert np.isinf(x).sum() >= 2
