"""Case tables and expected values of the LUT index-code and decode kernels (mctq_lut_codes_* / mctq_lut_decode_*), shared with
tests/test_gpu_lut_index.py, and the tests of them that need no GPU.

Expected indices: oracle.mctq_oracle.lut_quantize(..., return_index=True) on the values as stored, widened to float32 (step_dtype
where a case uses step_round).  Expected decode: numpy float32 from the codes themselves, (lut[code] / mult) * thr with one rounding
per operation; a code >= n_lut gives 0.0 * thr.  Packed 4-bit codes: oracle.mctq_oracle.pack4.

The route of every case is re-derived here from the launchers' arithmetic as it stands (launch_flat / launch_channels of
csrc/mctq_kernels.hpp, mctq_lut_codes4.hip, mctq_lut_decode.hip): kThreads = 256, a lane vector of N = 4 (float32) / 8 (16-bit)
elements, U lane vectors per lane, 4 parameter words per staged row (LutCommon::kWords) beside the op's book in at most 64 KiB of
LDS.  A change to a launcher fails test_shapes_satisfy_the_arithmetic_of_their_route with a message, not a GPU run with a note.
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

F32 = np.float32
MULT, CMIN, CMAX, BITS = 128.0, -128.0, 127.0, 8
T = 256                                                      # kThreads
DTYPES = ("float32", "float16", "bfloat16")
DT_CODE = {"float32": 0, "float16": 1, "bfloat16": 2}
VEC = {"float32": 4, "float16": 8, "bfloat16": 8}            # N: elements of a 16-byte lane vector
OPS = ("table", "literal")
OP_NAME = {"table": "LutIndexTableOp", "literal": "LutIndexOp"}
OP_U = {"table": 4, "literal": 2}                            # kFixedU on the flat, rows launches
L4U = DEC_U = 4                                              # kL4U, kDecU
LDS_LIMIT = 64 * 1024
KWORDS = 4                                                   # LutCommon::kWords (AffineCodesOp: 3)
ENTRIES = int(2 * (CMAX - CMIN) + 1)                         # table_entries(): 511
NOMINAL_CUS = 256                                            # for the CU-dependent size where no GPU tells

_L16 = [-128.0, -96.0, -64.0, -40.0, -24.0, -12.0, -5.0, 0.0, 5.0, 12.0, 24.0, 40.0, 64.0, 96.0, 120.0, 127.0]
LUTS = {
    "l16": _L16,
    "l256": [float(v) for v in np.random.default_rng(6).permutation(np.arange(-128, 128))],
    "l3dup": [3.0, 3.0, -8.0],                               # a duplicate: index 1 must never appear
    "l1": [5.0],
    "l16q": [v + 0.25 for v in _L16],                        # non-integer: no index table, the literal scan only
}
NIBBLE_LUTS = ("l16", "l3dup", "l1", "l16q")


def ops_of(lut_name):
    return ("literal",) if lut_name == "l16q" else OPS


def luts_of(op, names=tuple(LUTS)):
    return tuple(n for n in names if op in ops_of(n))


def first_indices(lut_name):
    lut = LUTS[lut_name]
    return {lut.index(v) for v in lut}


@functools.lru_cache(maxsize=None)
def index_table(lut_name):
    """native.build_lut_index_table's [ENTRIES + 1, 2] float32 words (host code), or None."""
    from mct_quantizers_amd.hip import native
    tab = native.build_lut_index_table(LUTS[lut_name], MULT, CMIN, CMAX)
    if tab is not None:
        assert tab.shape == (ENTRIES + 1, 2)
        tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def value_table(lut_name):
    from mct_quantizers_amd.hip import native
    return native.build_lut_table(LUTS[lut_name], MULT, CMIN, CMAX)


def table_bytes(entries=ENTRIES):
    return (((entries + 1) * 2 + 3) & ~3) * 4


def book_bytes(op, lut_name):
    """Dynamic LDS the op's book takes: the index table, or the codebook rounded up to four floats."""
    return table_bytes() if op == "table" else ((len(LUTS[lut_name]) + 3) & ~3) * 4


# ------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------

# (name, threshold, eps): 1.0 and 1.7 take the fast exact division; 2^70 and 2^-70 lie outside (2^-60, 2^60): p.r == 0, the
# IEEE division (eps = 0 beside 2^-70: 1e-8 would swamp it)
DIVISORS = (("1.0", 1.0, 1e-8), ("1.7", 1.7, 1e-8), ("2^70", 2.0 ** 70, 1e-8), ("2^-70", 2.0 ** -70, 0.0))
SPECIALS = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-39, -1e-39, 3e38, -3e38, 1e-45], dtype=F32)
SWEEP_SIZE = 1555


def narrow(x32, dt):
    """float32 values as storage type dt holds them, widened again."""
    x32 = np.ascontiguousarray(x32, dtype=F32)
    if dt == "float32":
        return x32
    return torch.from_numpy(x32).to(getattr(torch, dt)).float().numpy()


def tensor_divisor(thr, eps, step_dtype="float32"):
    """The per-tensor divisor as the classes form it: fl32(double(thr) + eps), then the tensor's type under step_round."""
    from oracle import mctq_oracle as O
    div = F32(float(thr) + eps)
    if step_dtype != "float32":
        div = F32(O.narrow(np.asarray([div], dtype=F32), step_dtype).reshape(-1)[0])
    return div


@functools.lru_cache(maxsize=None)
def sweep(divisor, dt):
    """In t: every half-integer point from -129 to 128 with its two float32 neighbours; x = (t / 128) * d (exact for powers of
    two); the specials appended; narrowed to dt.  Read-only float32 [1555]."""
    d = F32(divisor)
    half = np.arange(-258, 257).astype(F32) * F32(0.5)
    t = np.concatenate([half, np.nextafter(half, F32(-np.inf)), np.nextafter(half, F32(np.inf))]).astype(F32)
    x = np.concatenate([((t / F32(MULT)) * d).astype(F32), SPECIALS]).astype(F32)
    assert x.size == SWEEP_SIZE
    x = narrow(x, dt)
    x.setflags(write=False)
    return x


def want_indices(x, lut_name, thr, eps, per_channel=False, step_dtype="float32"):
    """The oracle's index of every element.  per_channel: x [outer, C, inner], thr float32 [C]; else thr a number."""
    from oracle import mctq_oracle as O
    lut = LUTS[lut_name]
    chunk = max(1, (1 << 22) // len(lut))
    if per_channel:
        _, idx = O.lut_quantize(x, lut, np.asarray(thr, dtype=F32), True, BITS, eps, per_channel=True, channel_axis=1,
                                return_index=True, chunk_elems=chunk)
    else:
        _, idx = O.lut_quantize(x, lut, float(thr), True, BITS, eps, return_index=True, chunk_elems=chunk, step_dtype=step_dtype)
    assert idx.min() >= 0 and idx.max() < len(lut)
    return idx


def want_decode(codes, lut_name, thr):
    """(lut[code] / mult) * thr in float32, one rounding per operation; a code >= n_lut reads 0.0.  thr broadcasts."""
    lut = np.asarray(LUTS[lut_name], dtype=F32)
    c = np.asarray(codes, dtype=np.int64)
    q = (np.where(c < lut.size, lut[np.minimum(c, lut.size - 1)], F32(0.0)).astype(F32) / F32(MULT)).astype(F32)
    return (q * np.asarray(thr, dtype=F32)).astype(F32)


def lut_inputs(rng, shape, thr_b):
    """Inputs dense in the half-integer points of t (ties of integer centres) with NaN, +-inf, +-0.0, a denormal and +-3e38 over
    one element in 16."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = rng.standard_normal(int(np.prod(shape))).astype(F32).reshape(shape) * thr_b * F32(0.6)
        mid = (rng.integers(-130, 130, size=shape).astype(F32) + F32(0.5)) / F32(128.0) * thr_b
        x = np.where(rng.integers(0, 4, size=shape) == 0, mid, x).astype(F32)
    special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], dtype=F32)
    pick = rng.integers(0, 16 * special.size, size=shape)
    return np.where(pick < special.size, special[pick % special.size], x).astype(F32)


# ------------------------------------------------------------------------------------------------
# routes, re-derived
# ------------------------------------------------------------------------------------------------

def note(route, op_name, in_bytes, out_bytes, u, nt):
    return f"{route}<{op_name},in{in_bytes}B,out{out_bytes}B,U={u},NT={nt}>"


def slab_rows(vc):
    """Rows per slab of the last-axis launches for vc lane vectors per row: the k in [ceil(2048 / vc), + 16) with the least
    (256 - (k vc) % 256) % 256 * 4096 / (k vc), first of equals."""
    k0 = -(-2048 // vc)
    waste = [(T - (k * vc) % T) % T * 4096 // (k * vc) for k in range(k0, k0 + 16)]
    return k0 + waste.index(min(waste))


def window_plan(shape, V, book):
    """launch_channels' window launch for lane vectors of V elements (1: unaligned) -> (wu, tile, staged rows, LDS bytes)."""
    inner, C = shape[2], shape[1]
    for wu in (4, 1):
        tile = T * wu * V
        max_rows = (tile - 1 + inner - 1) // inner + 1
        entries = min(C, max_rows)
        lds = book + (entries | 1) * KWORDS * 4
        if lds <= LDS_LIMIT or V == 1:
            break
    assert lds <= LDS_LIMIT
    return wu, tile, entries, lds


def rows_u(innerv):
    """The widest of {4, 2, 1} whose idle lanes in a row's last tile stay under 1/8, else 1 (launch_decode_rows)."""
    for u in (4, 2, 1):
        cap = -(-innerv // (T * u)) * T * u
        if (cap - innerv) * 8 <= cap:
            return u
    return 1


def enc8_route(case, dt, op):
    """(route, U, NT) of a uint8 encode: launch_flat / launch_channels, heavy dispatch, one variant per op."""
    N = VEC[dt]
    vec_ok = case.xoff % N == 0 and case.yoff % N == 0
    if case.kind == "tensor":
        return ("flat_kernel", OP_U[op], 1) if vec_ok else ("flat_scalar_kernel", 1, 0)
    _, C, inner = case.shape
    if vec_ok and inner % N == 0 and inner // N >= T:
        return "rows_kernel", OP_U[op], 1
    if vec_ok and inner == 1 and C % N == 0 and case.toff % 4 == 0:
        assert slab_rows(C // N) * (C // N) < 1 << 24
        return "lastaxis_kernel", 2, 1
    if not vec_ok:
        window_plan(case.shape, 1, book_bytes(op, case.lut))
        return "window_kernel<scalar>", 4, 1
    return "window_kernel<vector>", window_plan(case.shape, N, book_bytes(op, case.lut))[0], 1


def enc4_route(case, dt):
    """Route of a packed 4-bit encode (mctq_lut_codes4.hip), or None for a refusal."""
    n = int(np.prod(case.shape))
    if case.xoff % VEC[dt] or case.yoff % 4 or len(LUTS[case.lut]) > 16:
        return None
    if case.kind == "tensor":
        return ("lut_codes4_flat_kernel", L4U, 1) if n % 8 == 0 else None
    _, C, inner = case.shape
    if inner % 8 == 0:
        return "lut_codes4_rows_kernel", L4U, 1
    return ("lut_codes4_lastaxis_kernel", L4U, 1) if inner == 1 and C % 8 == 0 else None


def dec_route(case, code):
    """Route of a decode (mctq_lut_decode.hip): code "u8" / "u4"; xoff = byte offset of the codes, yoff = of y."""
    V = 4 if code == "u8" else 8
    aligned = case.xoff % 4 == 0 and case.yoff % 16 == 0
    if not aligned:
        return ("lut_decode_scalar_kernel", 1, 0) if code == "u8" else None
    if case.kind == "tensor":
        return f"lut_decode_kernel<{code},tensor>", DEC_U, 1
    _, C, inner = case.shape
    if inner % V == 0:
        if inner // V >= T:
            return f"lut_decode_rows_kernel<{code}>", rows_u(inner // V), 1
        return f"lut_decode_kernel<{code},whole>", DEC_U, 1
    if inner == 1 and C % V == 0:
        return f"lut_decode_kernel<{code},lastaxis>", DEC_U, 1
    return (f"lut_decode_kernel<{code},ragged>", DEC_U, 1) if code == "u8" else None


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------

# shape: (n,) or (outer, C, inner), None for the one size that depends on the CU count (case_shape); xoff: elements (encode) or
# bytes (decode codes) past a 16-byte boundary; yoff: bytes; toff: thresholds, 4-byte words past a 16-byte boundary; step: the
# per-tensor call passes step_round = the storage type
Case = collections.namedtuple("Case", "id kind shape xoff yoff toff lut route u nt step")


def case_shape(case, cus=NOMINAL_CUS):
    """n = 32 CUs T + 1000 for the grid-stride case: the capped grid of 32 CUs blocks turns a second time."""
    return case.shape if case.shape is not None else (32 * cus * T + 1000,)


class _Table:
    def __init__(self, luts):
        self.luts, self.cases = luts, []

    def add(self, id_, shape, route, u, nt=1, xoff=0, yoff=0, toff=0, lut=None, step=False):
        kind = "tensor" if shape is None or len(shape) == 1 else "channel"
        lut = lut or self.luts[len(self.cases) % len(self.luts)]
        self.cases.append(Case(f"{id_}-{lut}", kind, shape, xoff, yoff, toff, lut, route, u, nt, step))


# the window shapes of tests/test_gpu_codes8.py (walk / same / straddle rows x whole table / row window), less (3, 6001, 1)
WINDOW_SHAPES = {"float32": ((1500, 3, 1), (300, 5, 3), (2, 300, 8), (2, 30, 104), (3, 16, 100), (150, 6, 5), (100, 6, 7),
                             (3, 16, 102), (2, 700, 7)),
                 "float16": ((3000, 3, 1), (600, 5, 3), (2, 600, 8), (2, 50, 104), (70, 10, 12), (6, 16, 100), (2, 5, 1028),
                             (2, 1300, 7))}
WINDOW_SHAPES["bfloat16"] = WINDOW_SHAPES["float16"]
SCALAR_SHAPES = ((700, 3, 1), (2, 150, 8), (50, 6, 7), (2, 700, 3))
OFF_FORMS = (("x+1", 1, 0), ("codes+1", 0, 1), ("both", 1, 1))


def one_vector_pair(op, lut_name):
    """Channel counts (inner == 1, fewer than the 4096 rows a float32 four-vector tile touches) either side of the LDS limit:
    the largest odd C with book + 16 C <= 64 KiB, and C + 2."""
    c = (LDS_LIMIT - book_bytes(op, lut_name)) // (KWORDS * 4)
    c -= 1 - c % 2
    return c, c + 2


@functools.lru_cache(maxsize=None)
def enc8_cases(dt, op):
    N, U = VEC[dt], OP_U[op]
    tb = _Table(luts_of(op))
    tb.add("flat-tail-only", (N - 1,), "flat_kernel", U)
    tb.add("flat-2-tiles-ragged-tail", (2 * T * U * N + 3 * N + (N - 1),), "flat_kernel", U)
    for name, xo, yo in OFF_FORMS:
        tb.add(f"flat-scalar-{name}", (3 * T + 5,), "flat_scalar_kernel", 1, 0, xoff=xo, yoff=yo)
    tb.add("flat-scalar-second-turn", None, "flat_scalar_kernel", 1, 0, xoff=1, lut="l16" if op == "table" else "l16q")
    if dt != "float32":
        tb.add("flat-step-round", (2 * T * U * N + 3 * N + (N - 1),), "flat_kernel", U, lut="l16", step=True)
        tb.add("flat-scalar-step-round", (3 * T + 5,), "flat_scalar_kernel", 1, 0, xoff=1, lut="l256", step=True)
    tb.add("rows-wrap", (2, 3, T * N), "rows_kernel", U)
    tb.add("rows-ragged", (1, 2, 1281 * N), "rows_kernel", U)
    for C in (64, 8):
        k = slab_rows(C // N)
        tb.add(f"lastaxis-C{C}-full-group", (2 * 2 * k + 3, C, 1), "lastaxis_kernel", 2)
        tb.add(f"lastaxis-C{C}-ragged-group", (2 * k + 3, C, 1), "lastaxis_kernel", 2)
    tb.add("lastaxis-thresholds+4", (259, 64, 1), "window_kernel<vector>", 4, toff=1)
    for shape in WINDOW_SHAPES[dt]:
        tb.add("window-" + "x".join(map(str, shape)), shape, "window_kernel<vector>", 4)
    if dt == "float32":
        for lut in (("l256",) if op == "table" else ("l256", "l16q")):
            c4, c1 = one_vector_pair(op, lut)
            tb.add(f"window-C{c4}-still-four", (2, c4, 1), "window_kernel<vector>", 4, lut=lut)
            tb.add(f"window-C{c1}-one-vector", (2, c1, 1), "window_kernel<vector>", 1, lut=lut)
    tb.add("window-3x6001x1-one-vector", (3, 6001, 1), "window_kernel<vector>", 1)
    for shape in SCALAR_SHAPES:
        for name, xo, yo in OFF_FORMS:
            tb.add(f"window-scalar-{'x'.join(map(str, shape))}-{name}", shape, "window_kernel<scalar>", 4, xoff=xo, yoff=yo)
    return tuple(tb.cases)


@functools.lru_cache(maxsize=None)
def enc4_cases(dt, op):
    N = VEC[dt]
    tb = _Table(luts_of(op, NIBBLE_LUTS))
    for step in ((False, True) if dt != "float32" else (False,)):
        s = "-step-round" if step else ""
        tb.add("flat4-one-word" + s, (8,), "lut_codes4_flat_kernel", L4U, step=step)
        tb.add("flat4-2-tiles-ragged" + s, (2 * T * L4U * N + 24,), "lut_codes4_flat_kernel", L4U, step=step)
    tb.add("rows4-short", (3, 5, 8), "lut_codes4_rows_kernel", L4U)
    tb.add("rows4-2-tiles-wrap", (2, 3, T * L4U * N + 8), "lut_codes4_rows_kernel", L4U)
    for C in (8, 64):
        k = slab_rows(C // N)
        for toff in (0, 1):
            tb.add(f"lastaxis4-C{C}-thresholds+{4 * toff}", (4 * k + 3, C, 1), "lut_codes4_lastaxis_kernel", L4U, toff=toff)
    return tuple(tb.cases)


DEC_OFF_FORMS = (("codes+1", 1, 0), ("y+4", 0, 4), ("both", 1, 4))
DEC_LUTS = {"u8": ("l16", "l256", "l3dup", "l1"), "u4": ("l16", "l3dup", "l1")}
DEC_BAD_LUTS = {"u8": ("l3dup", "l16"), "u4": ("l3dup",)}    # codebooks run again with a tenth of the codes >= n_lut
RAGGED_SHAPES = ((1500, 3, 1), (300, 5, 3), (100, 6, 7), (3, 16, 102),      # n % 4 == 0
                 (1501, 3, 1), (301, 5, 3), (101, 6, 7), (3, 15, 102))      # n % 4 != 0: block 0's byte tail per channel


@functools.lru_cache(maxsize=None)
def dec_cases(code):
    """Every case runs with every codebook of DEC_LUTS[code]; Case.lut is unused."""
    V = 4 if code == "u8" else 8
    tb = _Table(("any",))
    name = lambda shape: "x".join(map(str, shape))
    if code == "u8":
        for n in (1, 2, 3):
            tb.add(f"tensor-byte-tail-{n}", (n,), "lut_decode_kernel<u8,tensor>", DEC_U)
        tb.add("tensor-2-tiles-ragged-tail", (2 * T * DEC_U * 4 + 20 + 3,), "lut_decode_kernel<u8,tensor>", DEC_U)
        for f, xo, yo in DEC_OFF_FORMS:
            tb.add(f"scalar-tensor-{f}", (3 * T + 5,), "lut_decode_scalar_kernel", 1, 0, xoff=xo, yoff=yo)
            for shape in ((50, 6, 7), (2, 150, 8)):
                tb.add(f"scalar-{name(shape)}-{f}", shape, "lut_decode_scalar_kernel", 1, 0, xoff=xo, yoff=yo)
        tb.add("scalar-second-turn", None, "lut_decode_scalar_kernel", 1, 0, xoff=1)
        rows = ((4096, 4), (2048, 2), (1024, 1), (3600, 4), (1028, 1))
    else:
        tb.add("tensor-one-word", (8,), "lut_decode_kernel<u4,tensor>", DEC_U)
        tb.add("tensor-2-tiles-ragged", (2 * T * DEC_U * 8 + 40,), "lut_decode_kernel<u4,tensor>", DEC_U)
        rows = ((8192, 4), (4096, 2), (2048, 1), (2056, 1))
    for inner, u in rows:
        tb.add(f"rows-{inner}", (2, 3, inner), f"lut_decode_rows_kernel<{code}>", u)
    for shape in ((3, 5, 8), (2, 300, 8), (2, 30, 104), (4, 300, 8)):      # (the last: more than one block of nibble words too)
        tb.add("whole-" + name(shape), shape, f"lut_decode_kernel<{code},whole>", DEC_U)
    for shape in ((259, 64, 1), (1031, 8, 1)):
        tb.add("lastaxis-" + name(shape), shape, f"lut_decode_kernel<{code},lastaxis>", DEC_U)
    tb.add("lastaxis-259x64x1-thresholds+4", (259, 64, 1), f"lut_decode_kernel<{code},lastaxis>", DEC_U, toff=1)   # read one by one
    if code == "u8":
        for shape in RAGGED_SHAPES:
            tb.add("ragged-" + name(shape), shape, "lut_decode_kernel<u8,ragged>", DEC_U)
    return tuple(tb.cases)


def enc_note(case, dt, op):
    return note(case.route, OP_NAME[op], 16 // VEC[dt], 1, case.u, case.nt)


def dec_note(case):
    return note(case.route, "LutDecodeOp", 1, 4, case.u, case.nt)


def case_seed(case, *more):
    return [zlib.crc32(case.id.encode()), *more]


def encode_inputs(case, dt, cus=NOMINAL_CUS):
    """-> (x as stored, widened, shaped; threshold: a number per tensor, float32 [C] per channel; eps; expected indices).
    Per channel the thresholds are ordinary ones with 2^70 on channel 1 (from three channels): fast and IEEE divisors in one
    launch."""
    shape = case_shape(case, cus)
    rng = np.random.default_rng(case_seed(case, DT_CODE[dt]))
    if case.kind == "tensor":
        thr = 1.7
        x = narrow(lut_inputs(rng, shape, F32(thr)), dt)
        return x, thr, 1e-8, want_indices(x, case.lut, thr, 1e-8, step_dtype=dt if case.step else "float32")
    C = shape[1]
    thr = rng.uniform(0.05, 4.0, size=C).astype(F32)
    if C >= 3:
        thr[1] = F32(2.0 ** 70)
    x = narrow(lut_inputs(rng, shape, thr.reshape(1, C, 1)), dt)
    return x, thr, 1e-8, want_indices(x, case.lut, thr, 1e-8, per_channel=True)


def decode_inputs(case, lut_name, code, bad, cus=NOMINAL_CUS):
    """Codes drawn uniformly from 0 .. n_lut - 1 by a seeded generator, every value at least once where the size allows; ``bad``:
    a tenth of them replaced by values >= n_lut.  -> (codes int64 shaped, thresholds, expected float32)."""
    shape = case_shape(case, cus)
    n, n_lut = int(np.prod(shape)), len(LUTS[lut_name])
    top = 256 if code == "u8" else 16
    rng = np.random.default_rng(case_seed(case, n_lut, int(bad)))
    codes = rng.integers(0, n_lut, size=n)
    if n >= n_lut:
        codes[rng.permutation(n)[:n_lut]] = np.arange(n_lut)
        assert set(codes.tolist()) == set(range(n_lut))
    if bad:
        assert n_lut < top
        pos = rng.permutation(n)[:max(1, n // 10)]
        codes[pos] = rng.integers(n_lut, top, size=pos.size)
        codes[pos[0]] = top - 1
    codes = codes.reshape(shape)
    if case.kind == "tensor":
        thr = F32(1.7)
        return codes, thr, want_decode(codes, lut_name, thr)
    thr = rng.uniform(0.05, 4.0, size=shape[1]).astype(F32) * rng.choice(np.asarray([1.0, -1.0], dtype=F32), size=shape[1])
    return codes, thr, want_decode(codes, lut_name, thr.reshape(1, -1, 1))


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------

def test_sweep_and_codebooks_are_what_the_cases_assume():
    assert sorted(LUTS["l256"]) == [float(v) for v in range(-128, 128)] and len(LUTS["l16"]) == 16
    assert first_indices("l3dup") == {0, 2} and first_indices("l1") == {0}
    assert index_table("l16q") is None and value_table("l16q") is None
    for name in ("l16", "l256", "l3dup", "l1"):
        assert index_table(name) is not None and value_table(name) is not None
    assert table_bytes() == 4096 and book_bytes("literal", "l256") == 1024 and book_bytes("literal", "l3dup") == 16
    x = sweep(1.0, "float32")
    assert x.size == SWEEP_SIZE and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
    t = x[:1545] * F32(128.0)
    assert t.min() < -129 and t.max() > 128 and np.all(np.isin(np.arange(-258, 257) * 0.5, t))
    # the divisor classes: p.r != 0 inside (2^-60, 2^60) only
    for _, thr, eps in DIVISORS:
        d = float(tensor_divisor(thr, eps))
        assert (2.0 ** -60 < d < 2.0 ** 60) == (thr in (1.0, 1.7))
    assert float(F32(2.0 ** -70) + F32(1e-8)) == float(F32(1e-8))          # why eps = 0 goes with 2^-70


@pytest.mark.parametrize("lut_name", list(LUTS))
def test_sweep_reaches_every_first_occurrence_index(lut_name):
    """Every storage type at 1.0 and 1.7, float32 and bfloat16 at 2^70, float32 at 2^-70: every first-occurrence index of the
    codebook.  float16 at 2^70 / 2^-70 (and bfloat16 at 2^-70, not asked for) holds -inf, 0, +inf and NaN only: t = -128, 0, 127,
    so three indices, or as many as the codebook has."""
    first = first_indices(lut_name)
    for dname, thr, eps in DIVISORS:
        d = tensor_divisor(thr, eps)
        for dt in DTYPES:
            idx = set(want_indices(sweep(float(d), dt), lut_name, thr, eps).reshape(-1).tolist())
            assert idx <= first, (lut_name, dname, dt, sorted(idx - first))
            full = thr in (1.0, 1.7) or dt == "float32" or (dt == "bfloat16" and dname == "2^70")
            if full:
                assert idx == first, (lut_name, dname, dt, sorted(first - idx))
            else:
                assert len(idx) >= min(3, len(first)), (lut_name, dname, dt, sorted(idx))


def required_routes(dt, op):
    U = OP_U[op]
    return ([("flat_kernel", U, 1), ("flat_scalar_kernel", 1, 0), ("rows_kernel", U, 1), ("lastaxis_kernel", 2, 1),
             ("window_kernel<vector>", 4, 1), ("window_kernel<vector>", 1, 1), ("window_kernel<scalar>", 4, 1)],
            [("lut_codes4_flat_kernel", 4, 1), ("lut_codes4_rows_kernel", 4, 1), ("lut_codes4_lastaxis_kernel", 4, 1)])


REQUIRED_DECODE = {
    "u8": [("lut_decode_kernel<u8,tensor>", 4, 1), ("lut_decode_scalar_kernel", 1, 0), ("lut_decode_rows_kernel<u8>", 4, 1),
           ("lut_decode_rows_kernel<u8>", 2, 1), ("lut_decode_rows_kernel<u8>", 1, 1), ("lut_decode_kernel<u8,whole>", 4, 1),
           ("lut_decode_kernel<u8,lastaxis>", 4, 1), ("lut_decode_kernel<u8,ragged>", 4, 1)],
    "u4": [("lut_decode_kernel<u4,tensor>", 4, 1), ("lut_decode_rows_kernel<u4>", 4, 1), ("lut_decode_rows_kernel<u4>", 2, 1),
           ("lut_decode_rows_kernel<u4>", 1, 1), ("lut_decode_kernel<u4,whole>", 4, 1), ("lut_decode_kernel<u4,lastaxis>", 4, 1)]}


def test_route_table_is_complete():
    for dt in DTYPES:
        for op in OPS:
            need8, need4 = required_routes(dt, op)
            have8 = {(c.route, c.u, c.nt) for c in enc8_cases(dt, op)}
            have4 = {(c.route, c.u, c.nt) for c in enc4_cases(dt, op)}
            assert have8 == set(need8), (dt, op, have8 ^ set(need8))
            assert have4 == set(need4), (dt, op, have4 ^ set(need4))
            for cases in (enc8_cases(dt, op), enc4_cases(dt, op)):
                assert len({c.id for c in cases}) == len(cases)
                assert {c.lut for c in cases} >= set(luts_of(op, NIBBLE_LUTS if cases is enc4_cases(dt, op) else tuple(LUTS)))
            if dt != "float32":                                     # step_round through both flat kernels, both code widths
                assert {c.route for c in enc8_cases(dt, op) if c.step} == {"flat_kernel", "flat_scalar_kernel"}
                assert sum(c.step for c in enc4_cases(dt, op)) == 2
            # the scalar forms: x, codes, both
            for route in ("flat_scalar_kernel", "window_kernel<scalar>"):
                assert {(c.xoff, c.yoff) for c in enc8_cases(dt, op) if c.route == route and not c.step} == {(1, 0), (0, 1), (1, 1)}
    for code in ("u8", "u4"):
        have = {(c.route, c.u, c.nt) for c in dec_cases(code)}
        assert have == set(REQUIRED_DECODE[code]), (code, have ^ set(REQUIRED_DECODE[code]))
    sc = [c for c in dec_cases("u8") if c.route == "lut_decode_scalar_kernel"]
    assert {(c.kind, c.xoff, c.yoff) for c in sc} >= {(k, x, y) for k in ("tensor", "channel") for x, y in ((1, 0), (0, 4), (1, 4))}
    assert sum(c.shape is None for c in sc) == 1


def test_shapes_satisfy_the_arithmetic_of_their_route():
    for dt in DTYPES:
        N = VEC[dt]
        for op in OPS:
            U = OP_U[op]
            for c in enc8_cases(dt, op):
                what = f"{dt} {op} {c.id}"
                assert enc8_route(c, dt, op) == (c.route, c.u, c.nt), (what, enc8_route(c, dt, op))
                shape = case_shape(c)
                n = int(np.prod(shape))
                if c.route == "flat_kernel":
                    tile = T * U * N
                    assert n < N or (n // N > 2 * T * U and (n // N) % (T * U) != 0 and n % N != 0), what
                    assert tile == T * c.u * N
                elif c.route == "flat_scalar_kernel":
                    blocks = -(-n // T)
                    assert blocks > 1 and n % T != 0, what
                    if c.shape is None:                              # more blocks than the cap, by less than another grid
                        assert 32 * NOMINAL_CUS < blocks < 2 * 32 * NOMINAL_CUS, what
                elif c.route == "rows_kernel":
                    innerv = shape[2] // N
                    assert shape[2] % N == 0 and innerv >= T, what
                    if "wrap" in c.id:                               # rows past the first outer slice; a quarter-full tile under U = 4
                        assert shape[0] > 1 and shape[1] > 1 and innerv == T, what
                    else:                                            # several tiles, the last ragged
                        assert innerv > T * U and innerv % (T * U) != 0, what
                elif c.route == "lastaxis_kernel":
                    k = slab_rows(shape[1] // N)
                    assert shape[0] > 2 * k and shape[0] % (2 * k) != 0, what       # a full group and a ragged one
                    if "full" in c.id:
                        assert shape[0] > 2 * 2 * k, what
                elif c.route == "window_kernel<vector>":
                    wu, tile, entries, lds = window_plan(shape, N, book_bytes(op, c.lut))
                    assert n > tile and n % tile != 0, what                         # more than one block, a ragged last one
                    if "still-four" in c.id:                          # the last channel count whose window fits beside the book
                        assert wu == 4 and entries == shape[1] and LDS_LIMIT - lds < 2 * KWORDS * 4, what
                    if "one-vector" in c.id:
                        assert wu == 1 and min(shape[1], (T * 4 * N - 1) // shape[2] + 1) * KWORDS * 4 + book_bytes(op, c.lut) > LDS_LIMIT, what
                    if shape[1] in (700, 1300, 6001):                 # the row window: fewer rows in a tile than channels
                        assert entries < shape[1] and shape[0] > 1, what
                else:
                    assert c.route == "window_kernel<scalar>" and n > T * 4 and n % (T * 4) != 0, what
            # the LUT ops reach the one-vector tile a quarter fewer channels in than a 3-word op without a book would
            c4, c1 = one_vector_pair(op, "l256")
            assert c1 == c4 + 2 and c1 < 4096 and c4 * 16 + book_bytes(op, "l256") <= LDS_LIMIT < (c1 | 1) * 16 + book_bytes(op, "l256")
            assert (c4, c1) == ((3839, 3841) if op == "table" else (4031, 4033))
            for c in enc4_cases(dt, op):
                what = f"{dt} {op} {c.id}"
                assert enc4_route(c, dt) == (c.route, c.u, c.nt), (what, enc4_route(c, dt))
                shape = c.shape
                n = int(np.prod(shape))
                assert n % 8 == 0 or c.route == "lut_codes4_lastaxis_kernel"
                if c.route == "lut_codes4_flat_kernel":
                    nv = n // N
                    assert nv in (1, 2) if n == 8 else (nv > 2 * T * L4U and nv % (T * L4U) != 0), what
                elif c.route == "lut_codes4_rows_kernel":
                    innerv = shape[2] // N
                    assert shape[0] > 1 and (innerv <= 2 or T * L4U < innerv <= T * L4U + 2), what
                else:
                    k = slab_rows(shape[1] // N)
                    assert shape[0] == 4 * k + 3 and shape[1] % 8 == 0, what
    for code in ("u8", "u4"):
        V = 4 if code == "u8" else 8
        for c in dec_cases(code):
            what = f"{code} {c.id}"
            assert dec_route(c, code) == (c.route, c.u, c.nt), (what, dec_route(c, code))
            shape = case_shape(c)
            n = int(np.prod(shape))
            if "rows" in c.route:
                innerv = shape[2] // V
                tiles = -(-innerv // (T * c.u))
                assert shape[0] > 1 and shape[1] > 1, what
                if shape[2] in (4096 * V // 4, 2048 * V // 4, 1024 * V // 4):
                    assert innerv == T * c.u and tiles == 1, what                  # exact fits
                else:
                    assert innerv % (T * c.u) != 0, what
                    if c.u == 1:
                        assert tiles == 2 and innerv - T == 1, what                # second tile one lane
            elif c.route == "lut_decode_scalar_kernel":
                assert -(-n // T) > 1, what
                if c.shape is None:
                    assert 32 * NOMINAL_CUS < -(-n // T) < 2 * 32 * NOMINAL_CUS, what
            elif c.kind == "channel":
                assert (n // V) % (T * DEC_U) != 0, what                           # a ragged last block
                if shape != (3, 5, 8) and (code == "u8" or shape not in ((2, 300, 8), (2, 30, 104))):
                    assert n // V > T * DEC_U, what                                # and more than one
                if "ragged" in c.route:
                    assert shape[2] % 4 != 0 and not (shape[2] == 1 and shape[1] % 4 == 0), what
        if code == "u8":
            tails = {int(np.prod(c.shape)) % 4 != 0 for c in dec_cases(code) if "ragged" in c.route}
            assert tails == {True, False}
            for shape in RAGGED_SHAPES[:4]:
                assert int(np.prod(shape)) % 4 == 0
            for shape in RAGGED_SHAPES[4:]:
                assert int(np.prod(shape)) % 4 != 0


def _cpu_x(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, dt))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_cpu_route_gives_the_expected_indices(dt, op):
    """ops.lut_codes on CPU tensors (the definition with torch ops) for every encode case: the expectation code runs here before
    any GPU visit.  The CPU route has no index table to take or leave: the op only selects the cases."""
    from mct_quantizers_amd.hip import ops
    from oracle import mctq_oracle as O
    for packed, cases in ((False, enc8_cases(dt, op)), (True, enc4_cases(dt, op))):
        for c in cases:
            x, thr, eps, want = encode_inputs(c, dt)
            lut = torch.tensor(LUTS[c.lut], dtype=torch.float32)
            xt = _cpu_x(x, dt)
            assert np.array_equal(xt.float().numpy(), x, equal_nan=True)
            assert len(np.unique(want)) >= min(3, len(first_indices(c.lut))) or x.size < 64, (c.id, np.unique(want))
            if c.kind == "tensor":
                div = float(tensor_divisor(thr, eps, dt if c.step else "float32"))
                got = ops.lut_codes(xt, lut, None, None, eps, div, MULT, CMIN, CMAX, packed4=packed,
                                    step_round=DT_CODE[dt] if c.step else 0)
            else:
                got = ops.lut_codes(xt, lut, torch.from_numpy(thr), 1, eps, 0.0, MULT, CMIN, CMAX, packed4=packed)
            want_bytes = O.pack4(want) if packed else want.reshape(-1).astype(np.uint8)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy().reshape(-1), want_bytes), (dt, op, c.id)


@pytest.mark.parametrize("code", ["u8", "u4"])
def test_cpu_route_gives_the_expected_decode(code):
    from conftest import bits_equal, first_mismatch
    from mct_quantizers_amd.hip import ops
    from oracle import mctq_oracle as O
    for c in dec_cases(code):
        for lut_name in DEC_LUTS[code]:
            codes, thr, want = decode_inputs(c, lut_name, code, False)
            lut = torch.tensor(LUTS[lut_name], dtype=torch.float32)
            if code == "u8":
                ct, kw = torch.from_numpy(codes.astype(np.uint8)), {}
            else:
                ct, kw = torch.from_numpy(O.pack4(codes)), dict(packed4=True, shape=codes.shape)
            if c.kind == "tensor":
                got = ops.lut_decode(ct, lut, None, None, float(thr), MULT, **kw)
            else:
                got = ops.lut_decode(ct, lut, torch.from_numpy(thr), 1, 0.0, MULT, **kw)
            assert got.dtype == torch.float32 and bits_equal(got.numpy().reshape(codes.shape), want), \
                (code, c.id, lut_name, first_mismatch(got.numpy(), want))
    # a code beyond the codebook: 0.0 * thr, the sign of the threshold kept
    out = want_decode(np.asarray([0, 2, 3, 255]), "l3dup", np.asarray([-2.0], dtype=F32))
    assert out.tolist()[:2] == [-0.046875, 0.125] and np.signbit(out[2:]).all() and (out[2:] == 0).all()
