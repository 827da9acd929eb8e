"""The cases of tests/test_gpu_affine_routes.py -- the float-output affine fake-quant kernels (AffineOp of csrc/mctq_kernels.hpp
behind mctq_fq_per_tensor / mctq_fq_per_channel / mctq_fq_per_tensor_tqp) on every launch route and at edge values -- and,
without a GPU, the proof that they reach what they claim.

Routes.  ``expected_note`` replays the three entry points of csrc/mctq_affine.hip and, under them, launch_flat, launch_channels,
paced_rows_window, nt_mode (csrc/mctq_kernels.hpp) and fq_gather_one_f32 (csrc/mctq_batched.hpp) AS THEY STAND, and returns the
exact text of mctq_last_launch(); ``instance`` returns what that text cannot show (the shortrows instance, bulk / tail of the
finetail launch, wu of the window launch).  Whoever changes one of those functions changes the replay with it: the GPU file
compares the whole string on every call.

Branches.  ``flat_branches`` ... ``window_branches`` replay the kernels' index arithmetic and say which branches a shape runs;
``tile_branches`` does it for batched_tile (the gather launch and the batched lists).

``cases(cus)`` is the one table of (entry, storage type, outer, C, inner, offsets, zero points, tuning) -> route; the tests below
prove, for CU counts on both sides of the MI355X's 256, that it names every route, every U / NT instance and every branch, and
that each case goes where it is filed.  ``want`` is the expected value of every GPU test: the numpy oracle with NaN -> -inf.
"""
import collections
import functools

import numpy as np
import pytest
import torch

from test_gpu_codes8 import (FLAT_PARAMS, PARAMS, SIGNED, UNSIGNED, THREADS, VEC, _assert_covers, _channel_sets, _edge_values,
                             _rounds, _slab_rows, _sweep_host)

DTYPES = ("float32", "float16", "bfloat16")
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2}
DEFAULTS = {"paced": 1, "shortrows": 1, "rowsteps": 2, "filldrain": 1, "unroll": 4, "nt": 1, "cached_store_max_mb": 32}
CUS = (64, 104, 128, 228, 256, 304)
# the ten pairs of test_gpu_codes8.py and a scale above 2^100 whose reciprocal is still a normal float
ALL_PARAMS = PARAMS + ((2e31, 0, -128, 127),)
# five sets whose scales all lie in recip_exact's range [2^-100, 2^100]: every wave takes the five-instruction reciprocal
INRANGE = tuple(p for p in PARAMS if 1e-3 < p[0] < 1 and (p[2], p[3]) in ((-128, 127), (0, 255)))
# SIGNED with its largest scale above 2^100.  (SIGNED's own 1e30 is BELOW 2^100 = 1.27e30: it is recip_exact's largest divisor
# of these tables, not a fallback; UNSIGNED's 3e-33 < 2^-100 and this table's 2e31 force the IEEE division.)
HUGE = tuple(p if p[0] < 1e29 else (2e31,) + p[1:] for p in SIGNED)
TABLES = {"inrange": INRANGE, "signed": SIGNED, "unsigned": UNSIGNED, "huge": HUGE}
EXACT_TABLES = ("inrange", "signed")                       # every wave inverts by recip_exact; under the others the waves divide


def tuned(**keys):
    t = dict(DEFAULTS)
    t.update(keys)
    return t


# ------------------------------------------------------------------------------------------------
# the launchers' arithmetic
# ------------------------------------------------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


def nt_mode(out_bytes, t):
    if t["nt"] != 1:
        return t["nt"]
    cap = t["cached_store_max_mb"] << 20
    return 2 if cap > 0 and out_bytes <= cap else 1


def _text(shape, dt, u, nt):
    return f"{shape}<AffineOp,in{ESIZE[dt]}B,out{ESIZE[dt]}B,U={u},NT={nt}>"


def paced_rows_window(N, n, inner, C, cus):
    tile = THREADS * 4 * N
    if inner % N != 0 or inner < N or C <= 1:
        return False
    if n >= (1 << 32) - tile or inner + tile >= (1 << 24) or C + tile >= (1 << 24):
        return False
    blocks, rnd = _ceil(n, tile), 8 * cus
    return blocks * 4 >= rnd * 3 and blocks <= rnd


def _launch_flat(dt, n, aligned, cus, t):
    N = VEC[dt]
    if not aligned:
        return _text("flat_scalar_kernel", dt, 1, 0), {}
    nv = n // N
    u_sel = t["unroll"]
    while u_sel > 1 and nv < THREADS * u_sel * 2 * cus:
        u_sel >>= 1
    nt = nt_mode(n * ESIZE[dt], t)
    blocks4, rnd = _ceil(nv, THREADS * 4), 8 * cus
    window = blocks4 * 4 >= rnd * 3 and blocks4 <= rnd
    if u_sel == 4 and nv >= THREADS * 4 and ((t["paced"] == 1 and window) or t["paced"] == 2):
        return _text("flat_paced_kernel", dt, 4, nt), {"U": 4}
    u = (u_sel if u_sel in (1, 2) else 4) if dt == "float32" else (2 if u_sel in (1, 2) else 4)
    return _text("flat_kernel", dt, u, nt), {"U": u}


def _rows_best_u(innerv, unroll):
    best_u, best_waste, u = 1, -1, 1
    while u <= unroll:
        per = THREADS * u
        waste = _ceil(innerv, per) * per - innerv
        if best_waste < 0 or waste <= best_waste:
            best_waste, best_u = waste, u
        u <<= 1
    return best_u


def _launch_channels(dt, outer, C, inner, vec_ok, tables_aligned, has_zp, cus, t):
    N, es = VEC[dt], ESIZE[dt]
    n, rows, rnd = outer * C * inner, outer * C, 8 * cus
    nt = nt_mode(n * es, t)
    tile = THREADS * 4 * N
    eligible = vec_ok and inner >= N and C > 1 and n < (1 << 32) - tile and inner + tile < (1 << 24) and C + tile < (1 << 24)
    long_rows = inner % N == 0 and inner // N >= THREADS
    sr_blocks = _ceil(n, tile)
    one_round = sr_blocks <= rnd and sr_blocks * 8 > rnd * 7
    window = es == 4 and paced_rows_window(N, n, inner, C, cus) and not has_zp
    paced = es == 4 and (t["paced"] == 2 or (t["paced"] == 1 and window))
    steps_row = long_rows and (inner // N) % THREADS == 0 and inner // N <= 3 * THREADS
    f32_window = (t["paced"] == 1 and window and (not long_rows or t["rowsteps"] != 1)
                  and (not steps_row or sr_blocks * 8 > rnd * 7))
    if es == 2:
        rule = not long_rows or (one_round and t["rowsteps"] != 1)
    else:
        rule = (not long_rows and inner < 32) or f32_window
    if eligible and (t["shortrows"] == 2 or (t["shortrows"] == 1 and rule)):
        return _text("shortrows_kernel", dt, 4, nt), {"ZP": has_zp, "WHOLE": inner % N == 0, "paced": paced,
                                                      "shift": inner & (inner - 1) == 0}
    if vec_ok and inner % N == 0 and inner // N >= THREADS:
        innerv = inner // N
        best_u = _rows_best_u(innerv, t["unroll"])
        total_steps = rows * (innerv // THREADS)
        rs_blocks = _ceil(total_steps, 4)
        rs_round = rs_blocks <= rnd and rs_blocks * 4 >= rnd * 3
        if ((t["rowsteps"] == 1 or (t["rowsteps"] == 2 and rs_round)) and best_u < 4 and t["unroll"] >= 4
                and innerv % THREADS == 0):
            return _text("rowsteps_kernel", dt, 4, nt), {"U": 4}
        if dt == "float32":
            total = rows * (innerv // (THREADS * 4))
            if ((t["filldrain"] == 2 or (t["filldrain"] == 1 and total * 8 >= rnd * 9)) and not has_zp and best_u == 4
                    and innerv % (THREADS * 4) == 0):
                tail = min(total, rnd // 2)
                return _text("rows_kernel_finetail", dt, 4, nt), {"bulk": total - tail, "tail": tail}
        if dt != "float32" and best_u < 2:
            best_u = 2
        return _text("rows_kernel", dt, best_u, nt), {"U": best_u}
    if vec_ok and inner == 1 and C % N == 0 and tables_aligned:
        vc = C // N
        k = _slab_rows(vc)
        if k * vc < (1 << 24):
            lu = 4 if has_zp else 2
            return _text("lastaxis_kernel", dt, lu, nt), {"U": lu, "ZP": has_zp}
    V = N if vec_ok else 1
    wu = 4
    while True:
        tile = THREADS * wu * V
        entries = min(C, (tile - 1 + inner - 1) // inner + 1)
        lds = (entries | 1) * 3 * 4
        if lds <= 64 * 1024 or wu == 1 or not vec_ok:
            break
        wu = 1
    if not vec_ok:
        return _text("window_kernel<scalar>", dt, 4, 1), {"wu": 4, "V": 1}
    return _text("window_kernel<vector>", dt, wu, nt), {"wu": wu, "V": V}


def _per_channel(dt, outer, C, inner, x_aligned, y_aligned, tables_aligned, has_zp, cus, t):
    n = outer * C * inner
    long_rows = inner % 4 == 0 and inner // 4 >= 2 * THREADS
    if long_rows:
        innerv = inner // 4
        tiles = _ceil(innerv, THREADS)
        if (tiles * THREADS - innerv) * 12 > tiles * THREADS:
            long_rows = False
    paced_window = t["paced"] == 1 and t["shortrows"] != 0 and not has_zp and paced_rows_window(4, n, inner, C, cus)
    if (dt == "float32" and inner >= 32 and C > 1 and not long_rows and t["shortrows"] != 2 and not paced_window
            and x_aligned and y_aligned and n < (1 << 31) - 4096):
        return _text("gather_kernel", dt, 4, nt_mode(n * 4, t)), {"U": 4}
    return _launch_channels(dt, outer, C, inner, x_aligned and y_aligned, tables_aligned, has_zp, cus, t)


def _route(entry, dt, outer, C, inner, x_aligned, y_aligned, tables_aligned, has_zp, cus, tuning):
    t = tuned(**(tuning or {}))
    if entry == "tensor":
        assert outer == 1 and C == 1
        return _launch_flat(dt, inner, x_aligned and y_aligned, cus, t)
    if entry == "tqp":                                     # one row of one channel, always with a zero-point pointer
        assert outer == 1 and C == 1
        return _per_channel(dt, 1, 1, inner, x_aligned, y_aligned, True, True, cus, t)
    assert entry == "channel"
    return _per_channel(dt, outer, C, inner, x_aligned, y_aligned, tables_aligned, has_zp, cus, t)


def expected_note(entry, dt, outer, C, inner, *, x_aligned=True, y_aligned=True, tables_aligned=True, has_zp=True, cus=256,
                  tuning=None):
    """mctq_last_launch() after mctq_fq_per_tensor (entry "tensor": n = inner), mctq_fq_per_channel ("channel") or
    mctq_fq_per_tensor_tqp ("tqp": n = inner) on a non-empty tensor of storage type dt."""
    return _route(entry, dt, outer, C, inner, x_aligned, y_aligned, tables_aligned, has_zp, cus, tuning)[0]


def instance(entry, dt, outer, C, inner, *, x_aligned=True, y_aligned=True, tables_aligned=True, has_zp=True, cus=256,
             tuning=None):
    """What the note does not show: shortrows {ZP, WHOLE, paced, shift (True: shift < 32, False: division)}, finetail
    {bulk, tail}, window {wu, V}, lastaxis {U, ZP}."""
    return _route(entry, dt, outer, C, inner, x_aligned, y_aligned, tables_aligned, has_zp, cus, tuning)[1]


# ------------------------------------------------------------------------------------------------
# the kernels' index arithmetic: which branches a shape runs
# ------------------------------------------------------------------------------------------------

def flat_branches(n, N, U, paced=False):
    nv = n // N
    per = THREADS * U
    out = set()
    for b in range(max(1, _ceil(nv, per))):
        out.add(("paced" if paced else "full") if (b + 1) * per <= nv else "guarded")
    if nv * N < n:
        out.add("tail")
    return out


def rows_branches(rows, C, innerv, U):
    per = THREADS * U
    tiles = _ceil(innerv, per)
    out = {"tiles_per_row=1" if tiles == 1 else "tiles_per_row>1"}
    if innerv >= per:
        out.add("full")
    if innerv % per:
        out.add("guarded")
    if rows > C:
        out.add("row>=channels")
    return out


def rowsteps_branches(rows, C, innerv):
    spr = innerv // THREADS
    total = rows * spr
    out = set()
    for s0 in range(0, total, 4):
        out.add("full" if s0 + 4 <= total else "partial")
        if s0 // spr != (min(s0 + 4, total) - 1) // spr:
            out.add("two_rows")
    if rows > C:
        out.add("row>=channels")
    return out


def finetail_branches(rows, C, innerv, bulk, tail):
    tpr = innerv // (THREADS * 4)
    assert bulk + tail == rows * tpr
    out = set()
    if bulk:
        out.add("bulk")
    if tail:
        out.add("fine")
    if any(t % tpr for t in range(bulk, bulk + tail)):
        out.add("fine_tile_inside_row")
    if tail and bulk % tpr:                                   # t = bulk + piece / 4 starts off a row start
        out.add("tail_starts_inside_row")
    if rows > C:
        out.add("row>=channels")
    return out


def shortrows_branches(n, inner, C, N):
    tile = THREADS * 4 * N
    out = {"shift" if inner & (inner - 1) == 0 else "division"}
    off = np.arange(0, tile, N, dtype=np.int64)
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        out.add("full_block" if count == tile else "partial_block")
        row0, rem0 = divmod(e0, inner)
        nrows = (rem0 + count - 1) // inner + 1
        out.add("wraps" if row0 % C + nrows > C else "no_wraps")
        live = off[off < count]
        whole = live[live + N <= count]
        split = inner - (rem0 + whole) % inner
        if (split < N).any():
            out.add("crossing")
        if (split >= N).any():
            out.add("in_row")
        if whole.size < live.size:
            out.add("partial_vector")
    return out


def shortrows_exact(n, inner, C, N, scales, whole):
    """The outcomes of the wave ballot: a wave inverts by recip_exact when the scales of all its lanes' rows (and, where
    vectors can cross, of the rows behind them) lie in [2^-100, 2^100]; idle lanes vote with the tile's first row."""
    ok = (np.asarray(scales, np.float32) >= np.float32(2.0 ** -100)) & (np.asarray(scales, np.float32) <= np.float32(2.0 ** 100))
    tile = THREADS * 4 * N
    out = set()
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        row0, rem0 = divmod(e0, inner)
        lane = np.arange(THREADS)
        off = (np.arange(4)[:, None] * THREADS + lane[None, :]) * N
        pos = rem0 + np.where(off < count, off, 0)
        c = (row0 % C + pos // inner) % C
        good = ok[c] if whole else ok[c] & ok[(c + 1) % C]
        for w in range(THREADS // 64):
            out.add(bool(good[:, 64 * w:64 * (w + 1)].all()))
    return out


def tile_branches(n, inner, C, N):
    """batched_tile (csrc/mctq_batched.hpp) on every tile of one tensor: the gather launch and the batched lists."""
    tile = THREADS * 4 * N
    out = set()
    off = np.arange(0, tile, N, dtype=np.int64)
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        row0, rem0 = (e0 // inner, e0 % inner) if C > 1 else (0, e0)
        partial = count % N != 0
        if C == 1 or rem0 + count <= inner:
            out.add("one_row")
            if partial:
                out.add("one_row/partial_vector")
            continue
        c0 = row0 % C
        if rem0 + count <= 2 * inner:
            bnd = inner - rem0
            assert 0 < bnd < count
            whole = off[off + N <= count]
            out.add("two_rows/straddle" if ((whole < bnd) & (bnd < whole + N)).any() else "two_rows/aligned")
            if c0 + 1 == C:
                out.add("wraps")
            if partial:
                out.add("two_rows/partial_vector")
            continue
        nrows = (rem0 + count - 1) // inner + 1
        if c0 + nrows > C:
            out.add("wraps")
        whole = off[off + N <= count]
        rem = (rem0 + whole) % inner
        if (rem + N <= inner).any():
            out.add("several/in_row")
        if (rem + N > inner).any():
            out.add("several/crossing" if inner >= N else "several/walk")
        if partial:
            out.add("several/partial_vector")
    return out


def lastaxis_branches(outer, C, N, has_zp):
    vc = C // N
    k = _slab_rows(vc)
    lu = 4 if has_zp else 2
    out = set()
    if outer >= lu * k:
        out.add("full_group")
    if outer % (lu * k):
        out.add("short_group")
    if (k * vc) % THREADS:
        out.add("idle_lanes")
    return out


def window_branches(n, inner, C, V, wu):
    tile = THREADS * wu * V
    out = set()
    for e0 in range(0, n, tile):
        count = min(tile, n - e0)
        nrows = (e0 % inner + count - 1) // inner + 1
        out.add("whole" if C <= nrows else "window")
    return out


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "id route entry dt outer C inner xoff yoff tab_off has_zp tuning")


def _case(route, entry, dt, shape, tag="", xoff=0, yoff=0, tab_off=(0, 0), has_zp=True, **tuning):
    shape_id = shape if isinstance(shape, str) else "x".join(map(str, shape))
    keys = "".join(f"-{k}{v}" for k, v in sorted(tuning.items()))
    cid = f"{route}-{dt}-{shape_id}{'-' + tag if tag else ''}{'-zp' if has_zp and entry == 'channel' else ''}{keys}"
    return [route, entry, dt, shape, cid, xoff, yoff, tab_off, has_zp, tuning]


def _base_cases():
    """Shapes may be strings: sizes that depend on the CU count, resolved by ``cases(cus)``."""
    f32, halves = "float32", ("float16", "bfloat16")
    out = []
    # ---- shortrows_kernel: rows of at least one lane vector; float32 rows of 4 ... 31 elements and every short or ragged 16-bit row
    for zp in (False, True):
        for shape in ((3, 5, 4), (3, 5, 7), (3, 5, 16), (3, 5, 20)):
            out.append(_case("shortrows", "channel", f32, shape, has_zp=zp))
        for dt in halves:
            for shape in ((3, 5, 8), (3, 5, 12), (3, 5, 1020)):
                out.append(_case("shortrows", "channel", dt, shape, has_zp=zp))
    out.append(_case("shortrows", "channel", f32, (3, 5, 100), has_zp=False, shortrows=2))
    out.append(_case("shortrows", "channel", f32, (2, 3, 4096), has_zp=True, shortrows=2))
    out.append(_case("shortrows", "channel", f32, (2, 3, 4102), has_zp=False, shortrows=2))
    out.append(_case("shortrows", "channel", "bfloat16", (2, 3, 4096), has_zp=False, shortrows=2))
    out.append(_case("shortrows", "channel", f32, (3, 5, 20), has_zp=False, paced=2))
    out.append(_case("shortrows", "channel", f32, (3, 5, 7), has_zp=True, paced=2))
    # ---- gather_kernel (float32 rows of 32 elements and more that rows_kernel does not take)
    for shape, zp in (((50, 3, 33), True), ((50, 3, 33), False), ((2, 3, 36), True), ((2, 3, 3002), True), ((2, 3, 4100), False),
                      ((2, 3, 4099), True), ((1, 5, 1024), True), ((1, 2, 2047), False)):
        out.append(_case("gather", "channel", f32, shape, has_zp=zp))
    # ---- rows_kernel
    for shape, zp in (((2, 3, 2988), True), ((2, 3, 2048), False), ((2, 3, 4096), True), ((2, 3, 4096), False)):
        out.append(_case("rows", "channel", f32, shape, has_zp=zp))
    for dt in halves:
        for shape, zp in (((3, 5, 2048), True), ((3, 5, 2056), False), ((2, 3, 8192), True)):
            out.append(_case("rows", "channel", dt, shape, has_zp=zp))
    # ---- rowsteps_kernel (forced: its default window is a launch of one round)
    for shape, zp in (((2, 3, 2048), True), ((2, 3, 3072), False)):
        out.append(_case("rowsteps", "channel", f32, shape, has_zp=zp, rowsteps=1))
    for dt in halves:
        for shape, zp in (((2, 3, 2048), False), ((5, 3, 6144), True)):
            out.append(_case("rowsteps", "channel", dt, shape, has_zp=zp, rowsteps=1))
    # ---- rows_kernel_finetail (forced below 9/8 rounds); the same launch with a zero-point table stays rows_kernel
    out.append(_case("finetail", "channel", f32, (2, 3, 4096), has_zp=False, filldrain=2))
    out.append(_case("finetail", "channel", f32, (3, 2, 8192), has_zp=False, filldrain=2))
    out.append(_case("finetail", "channel", f32, "1x(4cus+3)x4096", has_zp=False, filldrain=2))
    out.append(_case("rows", "channel", f32, "1x(4cus+3)x4096", has_zp=True, filldrain=2))
    out.append(_case("finetail", "channel", f32, "1xRx(4096T)", has_zp=False, filldrain=2))       # the tail starts inside a row
    # ---- lastaxis_kernel: U = 2 without a zero-point table, U = 4 with one
    for dt in DTYPES:
        for zp in (False, True):
            out.append(_case("lastaxis", "channel", dt, (37, 64, 1), has_zp=zp))
            out.append(_case("lastaxis", "channel", dt, "(LUk+3)x64x1", has_zp=zp))
            out.append(_case("lastaxis", "channel", dt, "(LUk+1)x3Nx1", has_zp=zp))
        out.append(_case("lastaxis", "channel", dt, (1, 8, 1), has_zp=True))
        out.append(_case("window", "channel", dt, (37, 64, 1), tag="scales+4", tab_off=(1, 0), has_zp=True))
        out.append(_case("window", "channel", dt, (37, 64, 1), tag="zps+4", tab_off=(0, 1), has_zp=True))
    # ---- window_kernel<vector>: rows shorter than a lane vector, C % N != 0 on the last axis
    for shape, zp in (((3, 5, 3), True), ((3, 5, 1), False), ((3, 6001, 1), True)):
        out.append(_case("window", "channel", f32, shape, has_zp=zp))
    for dt in halves:
        for shape, zp in (((3, 5, 6), True), ((3, 5, 1), False), ((9, 6001, 1), True)):
            out.append(_case("window", "channel", dt, shape, has_zp=zp))
    # ---- per tensor
    for dt in DTYPES:
        for name in ("1", "N", "1024N", "1024N+N+1", "2348N+3"):
            out.append(_case("flat", "tensor", dt, name))
        out.append(_case("flat", "tensor", dt, "(2048cus+300)N+N-1"))
        out.append(_case("flat_paced", "tensor", dt, "(2048cus+300)N+N-1", paced=2))
        out.append(_case("flat_scalar", "tensor", dt, "2348N+3", tag="x+1", xoff=1))
        out.append(_case("flat_scalar", "tensor", dt, "2348N+3", tag="y+1", yoff=1))
    out.append(_case("flat", "tensor", f32, "(1024cus+300)N+N-1"))
    # ---- tensor qparams: one row of one channel through mctq_fq_per_channel
    for dt, n, route in ((f32, 4096, "rows"), (f32, 1024, "rows"), (f32, 1000, "window"), ("float16", 8192, "rows"),
                         ("bfloat16", 2048, "rows"), ("float16", 77, "window"), ("bfloat16", 77, "window")):
        out.append(_case(route, "tqp", dt, (1, 1, n)))
    # ---- every per-channel case above (the tensor-qparams ones too: they are per-channel calls) with x or y, in turn, one
    #      element off its vector boundary: window_kernel<scalar>, whatever the tuning keys and the tables' alignment
    for j, (route, entry, dt, shape, cid, xoff, yoff, tab_off, has_zp, tuning) in enumerate(list(out)):
        if entry == "tensor":
            continue
        x1 = j % 2 == 0
        out.append(["window_scalar", entry, dt, shape, f"window_scalar-{'x+1' if x1 else 'y+1'}-{cid}", int(x1), int(not x1),
                    tab_off, has_zp, tuning])
    return out


def _resolve(shape, dt, cus, has_zp):
    if not isinstance(shape, str):
        return shape
    N = VEC[dt]
    lu = 4 if has_zp else 2
    if shape == "1x(4cus+3)x4096":
        return (1, 4 * cus + 3, 4096)
    if shape == "1xRx(4096T)":
        # T = 3, 5 or 7 tiles a row and R rows with 4 cus < R T <= 4 cus + 3 and bulk = R T - 4 cus no multiple of T: the first fine
        # tile lies inside a row (two tiles a row cannot: R T - 4 cus is even)
        for T in (3, 5, 7):
            rows = (4 * cus + 3) // T
            bulk = rows * T - 4 * cus
            if bulk >= 1 and bulk % T:
                return (1, rows, 4096 * T)
        raise AssertionError(f"no finetail launch of one round whose tail starts inside a row for {cus} CUs")
    if shape == "(LUk+3)x64x1":
        return (lu * _slab_rows(64 // N) + 3, 64, 1)
    if shape == "(LUk+1)x3Nx1":
        return (lu * _slab_rows(3) + 1, 3 * N, 1)
    n = {"1": 1, "N": N, "1024N": 1024 * N, "1024N+N+1": 1024 * N + N + 1, "2348N+3": 2348 * N + 3,
         "(2048cus+300)N+N-1": (2048 * cus + 300) * N + N - 1, "(1024cus+300)N+N-1": (1024 * cus + 300) * N + N - 1}[shape]
    return (1, 1, n)


@functools.lru_cache(maxsize=None)
def cases(cus):
    """Every geometry case under both cache modes: stores through the caches (NT = 2, the default for outputs up to 32 MiB)
    and non-temporal stores (NT = 1: cached_store_max_mb = 0).  The ids do not depend on ``cus``."""
    out = []
    for route, entry, dt, shape, cid, xoff, yoff, tab_off, has_zp, tuning in _base_cases():
        outer, C, inner = _resolve(shape, dt, cus, has_zp)
        for mode in (2, 1):
            t = dict(tuning)
            if mode == 1:
                t["cached_store_max_mb"] = 0
            out.append(Case(f"{cid}-NT{mode}", route, entry, dt, outer, C, inner, xoff, yoff, tab_off, has_zp, t))
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case_note(c, cus):
    return expected_note(c.entry, c.dt, c.outer, c.C, c.inner, x_aligned=c.xoff == 0, y_aligned=c.yoff == 0,
                         tables_aligned=c.tab_off == (0, 0), has_zp=c.has_zp, cus=cus, tuning=c.tuning)


def case_instance(c, cus):
    return instance(c.entry, c.dt, c.outer, c.C, c.inner, x_aligned=c.xoff == 0, y_aligned=c.yoff == 0,
                    tables_aligned=c.tab_off == (0, 0), has_zp=c.has_zp, cus=cus, tuning=c.tuning)


KERNEL = {"shortrows": "shortrows_kernel<", "gather": "gather_kernel<", "rows": "rows_kernel<", "rowsteps": "rowsteps_kernel<",
          "finetail": "rows_kernel_finetail<", "lastaxis": "lastaxis_kernel<", "window": "window_kernel<vector><",
          "window_scalar": "window_kernel<scalar><", "flat": "flat_kernel<", "flat_paced": "flat_paced_kernel<",
          "flat_scalar": "flat_scalar_kernel<"}

# (a) the value sweeps of the GPU file: route -> (entry, [outer, C, inner] with L = the sweep vector's length padded to a
# multiple of inner, x offset, zero-point table, tuning).  "chunks": the vector is cut into L / inner rows and every row is
# given to all C channels ([L / inner, C, inner]); "columns": [L, C, 1]; "sets": [55, 6001, 1], see sweep_layout.
SWEEPS = {
    "flat": ("tensor", None, 0, True, {}),
    "flat_scalar": ("tensor", None, 1, True, {}),
    "flat_paced": ("tensor", "paced", 0, True, {"paced": 2}),
    "rows": ("channel", ("rows", 5), 0, True, {}),
    "rowsteps": ("channel", ("chunks", 5, 2048), 0, True, {"rowsteps": 1}),
    "finetail": ("channel", ("chunks", 5, 4096), 0, False, {"filldrain": 2}),
    "shortrows-whole": ("channel", ("chunks", 5, 16), 0, False, {}),
    "shortrows-whole-zp": ("channel", ("chunks", 5, 16), 0, True, {}),
    "shortrows-ragged": ("channel", ("chunks", 5, {4: 7, 8: 12}), 0, False, {}),
    "shortrows-ragged-zp": ("channel", ("chunks", 5, {4: 7, 8: 12}), 0, True, {}),
    "shortrows-whole-paced": ("channel", ("chunks", 5, 16), 0, False, {"paced": 2}),
    "shortrows-ragged-zp-paced": ("channel", ("chunks", 5, {4: 7, 8: 12}), 0, True, {"paced": 2}),
    "gather-short": ("channel", ("chunks", 5, 33), 0, True, {}),
    "gather-long": ("channel", ("chunks", 5, 4100), 0, True, {}),
    "lastaxis": ("channel", ("columns", 8), 0, False, {}),
    "lastaxis-zp": ("channel", ("columns", 8), 0, True, {}),
    "window": ("channel", ("columns", 5), 0, True, {}),
    "window-wu1": ("channel", ("sets",), 0, True, {}),
    "window_scalar": ("channel", ("columns", 5), 1, True, {}),
}
SWEEP_DTYPES = {"finetail": ("float32",), "shortrows-whole-paced": ("float32",), "shortrows-ragged-zp-paced": ("float32",),
                "gather-short": ("float32",), "gather-long": ("float32",), "window-wu1": ("float16", "bfloat16")}
SWEEP_KERNEL = {"shortrows": "shortrows", "gather": "gather", "window-wu1": "window"}


def sweep_routes():
    return [(route, dt) for route in SWEEPS for dt in SWEEP_DTYPES.get(route, DTYPES)]


def sweep_layout(route, dt, cus):
    """-> (entry, (outer, C, inner), gather index into the sweep vector for every element (-1: a padding zero), xoff, has_zp,
    tuning).  "sets" (the one-vector window tile needs C >= 5462 on the last axis, so not every CHANNEL can see 65536 values
    below 2^23 elements): channel c = 5 a + j has parameter set j (_channel_sets cycles five) and element [o, c] is value
    (1200 o + a) mod L, so every SET sees the whole vector."""
    entry, layout, xoff, has_zp, tuning = SWEEPS[route]
    L = _sweep_host(dt)[1].size
    N = VEC[dt]
    if layout is None:
        return entry, (1, 1, L), np.arange(L), xoff, has_zp, tuning
    if layout == "paced":                                  # flat_paced_kernel needs 2048 cus lane vectors: whole copies of the vector
        copies = _ceil((2048 * cus + 300) * N, L)
        return entry, (1, 1, copies * L), np.tile(np.arange(L), copies), xoff, has_zp, tuning
    if layout[0] == "rows":
        C = layout[1]
        return entry, (2, C, L), np.broadcast_to(np.arange(L), (2, C, L)), xoff, has_zp, tuning
    if layout[0] == "columns":
        C = layout[1]
        return entry, (L, C, 1), np.broadcast_to(np.arange(L)[:, None, None], (L, C, 1)), xoff, has_zp, tuning
    if layout[0] == "sets":
        C, outer = 6001, _ceil(L, 1200)
        a = np.arange(C) // 5
        idx = (np.arange(outer)[:, None] * 1200 + a[None, :]) % L
        return entry, (outer, C, 1), idx[:, :, None], xoff, has_zp, tuning
    C, inner = layout[1], layout[2]
    if isinstance(inner, dict):
        inner = inner[N]
    rows = _ceil(L, inner)
    idx = np.arange(rows * inner)
    idx[idx >= L] = -1
    return entry, (rows, C, inner), np.broadcast_to(idx.reshape(rows, 1, inner), (rows, C, inner)), xoff, has_zp, tuning


def sweep_values(dt, idx):
    x = _sweep_host(dt)[1]
    return np.where(idx >= 0, x[np.maximum(idx, 0)], np.float32(0)).astype(np.float32)


# (c) the batched lists: (outer, C, inner as a function of N, zero-point table, per-tensor flag)
def batch_items(N):
    T = THREADS * 4 * N                                    # elements of a tile
    return (((1, 1, T + 5 * N + 3), True, True),           # per tensor: one row, a partial last vector
            ((1, 1, 3), False, True),                      # per tensor: less than a lane vector
            ((2, 3, 2 * T), True, False),                  # every tile inside one row
            ((2, 3, T + N), False, False),                 # two rows, the boundary on a vector boundary
            ((2, 3, T + 3), True, False),                  # two rows, a straddling vector
            ((1, 2, T // 2 - 1), False, False),            # one tile of two rows, a straddling vector, a partial last vector
            ((2, 3, 5 * N), False, False),                 # several rows, whole vectors, wraps
            ((50, 3, 4 * N + 1), True, False),             # several rows, vectors that cross one boundary
            ((10, 6, 3), True, False),                     # several rows shorter than a lane vector: the per-element walk
            ((1, 7, 2 * N), False, False))                 # several rows, outer == 1: no wrap


# ------------------------------------------------------------------------------------------------
# expected values
# ------------------------------------------------------------------------------------------------

def want(x, scales, zps, qmin, qmax, axis, dt):
    """The oracle on the values as stored (float32), every NaN replaced by -inf, narrowed to the storage type.  DESIGN.md:
    +inf -> qmax, -inf / NaN -> qmin, y = (q - z) s."""
    from oracle import mctq_oracle as O
    x = np.asarray(x, dtype=np.float32)
    xs = np.where(np.isnan(x), np.float32(-np.inf), x)
    return O.narrow(O.fake_quant_affine(xs, scales, zps, qmin, qmax, axis=axis), dt)


def want64(x, scales, zps, qmin, qmax, axis):
    from oracle import mctq_oracle as O
    x = np.asarray(x, dtype=np.float64)
    return O.fake_quant_affine_f64(np.where(np.isnan(x), -np.inf, x), scales, zps, qmin, qmax, axis=axis)


def stored_bits(y32, dt):
    """float32 values that are exact in dt -> the bit patterns of their storage (uint32 / uint16)."""
    y32 = np.ascontiguousarray(y32, dtype=np.float32).reshape(-1)
    if dt == "float32":
        return y32.view(np.uint32).copy()
    if dt == "float16":
        with np.errstate(over="ignore"):
            h = y32.astype(np.float16)
        assert np.array_equal(h.astype(np.float32).view(np.uint32), y32.view(np.uint32))
        return h.view(np.uint16).copy()
    u = y32.view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def as_stored(x32, dt):
    """float32 values -> what a tensor of storage type dt holds of them, widened back."""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(getattr(torch, dt)).float().numpy()


BLOCK = 65521                                                # a prime: tiled inputs of the large cases line up with no tile
SPECIALS = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], dtype=np.float32)


def plant(x32, r):
    """Every special value at a fixed place of launch ``r`` and a NaN in its last element (the scalar tails); below eight
    elements one special every other launch in turn.  _edge_values sprinkles them over one element in 16 at random: a case
    of 256 values has no NaN at all once in seven, and then a clamp that sends NaN to the wrong end passes it."""
    flat = x32.reshape(-1)
    assert np.shares_memory(flat, x32)
    n = flat.size
    if n >= 8:
        flat[(np.arange(8) * n) // 8] = SPECIALS
        flat[n - 1] = np.nan
    elif r % 2 == 0:
        flat[(r // 2) % n] = SPECIALS[(r // 2) % 8]
    return x32


def _geometry_inputs(rng, c, k):
    shape = (c.outer, c.C, c.inner)
    n = c.outer * c.C * c.inner
    if c.entry != "channel":
        scale, zp, qmin, qmax = FLAT_PARAMS[k % 3]
        x = _edge_values(rng, (min(n, BLOCK),), np.float32(scale), np.float32(zp), qmin, qmax)
        return np.resize(x, n).reshape(shape), np.asarray([scale], np.float32), np.asarray([zp], np.int32), qmin, qmax
    qmin, qmax = ((-128, 127), (0, 255))[k % 2]
    big = n > 1 << 18 and c.outer == 1 and c.C > 16           # 16 rows of edge values and tables of period 16, repeated
    Cg = 16 if big else c.C
    scales = rng.uniform(0.01, 0.9, size=Cg).astype(np.float32)
    zps = rng.integers(qmin, qmax + 1, size=Cg).astype(np.int32) if c.has_zp else None
    z_b = np.float32(0) if zps is None else zps.reshape(1, Cg, 1).astype(np.float32)
    x = _edge_values(rng, (c.outer, Cg, c.inner), scales.reshape(1, Cg, 1), z_b, qmin, qmax)
    if big:
        reps = -(-c.C // 16)
        x = np.tile(x, (1, reps, 1))[:, :c.C]
        scales = np.tile(scales, reps)[:c.C]
        zps = None if zps is None else np.tile(zps, reps)[:c.C]
    return np.ascontiguousarray(x), scales, zps, qmin, qmax


def geometry_launches(c, k):
    """The launches of case ``k`` of the table, (x32 [outer, C, inner], scales, zps | None, qmin, qmax) each: inputs dense in the
    ties and clamp edges of the element's own channel (_edge_values) with the specials planted; shapes under 256 elements until
    256 values have gone through (_rounds).  Cases 2 j and 2 j + 1 are one geometry under the two cache modes: the same launches."""
    n = c.outer * c.C * c.inner
    rng = np.random.default_rng([k // 2, n])
    for r in range(_rounds(n)):
        x32, scales, zps, qmin, qmax = _geometry_inputs(rng, c, k // 2)
        yield plant(np.ascontiguousarray(x32), r), scales, zps, qmin, qmax


def case_want(c, x, scales, zps, qmin, qmax):
    """``want`` of one launch of a case; ``x``: the values as stored."""
    if c.entry != "channel":
        return want(x, scales, zps, qmin, qmax, None, c.dt)
    z = np.zeros(len(scales), np.int32) if zps is None else np.asarray(zps, np.int32)
    return want(x, np.asarray(scales, np.float32), z, qmin, qmax, 1, c.dt)


def batch_launch(rng, k, shape, has_zp):
    """Item ``k`` of the batched list -> (x32, scales, zps | None, qmin, qmax)."""
    C = shape[1]
    qmin, qmax = ((-128, 127), (0, 255), (-8, 7))[k % 3]
    scales = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
    zps = rng.integers(qmin, qmax + 1, size=C).astype(np.int32) if has_zp else None
    z_b = np.float32(0) if zps is None else zps.reshape(1, C, 1).astype(np.float32)
    x32 = plant(np.ascontiguousarray(_edge_values(rng, shape, scales.reshape(1, C, 1), z_b, qmin, qmax)), 2 * k)
    return x32, scales, zps, qmin, qmax


def batch_specs():
    return [(dt, item) for dt in DTYPES for item in batch_items(VEC[dt])]


def four_operations(x, s, z, qmin, qmax):
    """AffineOp::apply in numpy: fma(med3(rint(x inv), lo - z, hi - z), s, +0); med3 answers the smaller bound for a NaN."""
    x, s, z = np.asarray(x, np.float32), np.float32(s), np.float32(z)
    with np.errstate(all="ignore"):
        r = np.rint(x * (np.float32(1.0) / s))
        a, b = np.float32(qmin) - z, np.float32(qmax) - z
        q = np.where(np.isnan(r), a, np.minimum(np.maximum(r, a), b)).astype(np.float32)
        return ((q * s).astype(np.float32) + np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# tests (no GPU)
# ------------------------------------------------------------------------------------------------

def _branches(c, cus):
    """Which kernel branches a case runs, as "<route>/<branch>"."""
    N = VEC[c.dt]
    n, rows = c.outer * c.C * c.inner, c.outer * c.C
    inst = case_instance(c, cus)
    if c.route in ("flat", "flat_paced"):
        got = flat_branches(n, N, inst["U"], c.route == "flat_paced")
    elif c.route == "rows":
        got = rows_branches(rows, c.C, c.inner // N, inst["U"])
    elif c.route == "rowsteps":
        got = rowsteps_branches(rows, c.C, c.inner // N)
    elif c.route == "finetail":
        got = finetail_branches(rows, c.C, c.inner // N, inst["bulk"], inst["tail"])
    elif c.route == "shortrows":
        got = shortrows_branches(n, c.inner, c.C, N)
        got |= {f"ZP={int(inst['ZP'])},WHOLE={int(inst['WHOLE'])}", f"paced={int(inst['paced'])}"}
    elif c.route == "gather":
        got = tile_branches(n, c.inner, c.C, N)
    elif c.route == "lastaxis":
        got = lastaxis_branches(c.outer, c.C, N, c.has_zp)
    elif c.route in ("window", "window_scalar"):
        got = window_branches(n, c.inner, c.C, inst["V"], inst["wu"]) | {f"wu={inst['wu']}"}
    else:
        got = set()
    return {f"{c.route}/{b}" for b in got}


REQUIRED_BRANCHES = {
    "flat/full", "flat/guarded", "flat/tail", "flat_paced/paced", "flat_paced/guarded", "flat_paced/tail",
    "rows/full", "rows/guarded", "rows/tiles_per_row=1", "rows/tiles_per_row>1", "rows/row>=channels",
    "rowsteps/full", "rowsteps/partial", "rowsteps/two_rows", "rowsteps/row>=channels",
    "finetail/bulk", "finetail/fine", "finetail/fine_tile_inside_row", "finetail/tail_starts_inside_row", "finetail/row>=channels",
    "shortrows/ZP=0,WHOLE=0", "shortrows/ZP=0,WHOLE=1", "shortrows/ZP=1,WHOLE=0", "shortrows/ZP=1,WHOLE=1",
    "shortrows/paced=0", "shortrows/paced=1", "shortrows/shift", "shortrows/division", "shortrows/wraps", "shortrows/no_wraps",
    "shortrows/crossing", "shortrows/in_row", "shortrows/partial_vector", "shortrows/full_block", "shortrows/partial_block",
    "gather/one_row", "gather/two_rows/straddle", "gather/two_rows/aligned", "gather/several/in_row", "gather/several/crossing",
    "gather/wraps", "gather/one_row/partial_vector", "gather/two_rows/partial_vector", "gather/several/partial_vector",
    "lastaxis/full_group", "lastaxis/short_group", "lastaxis/idle_lanes",
    "window/whole", "window/window", "window/wu=4", "window/wu=1", "window_scalar/whole", "window_scalar/window"}


def _required_notes():
    out = set()
    for nt in (1, 2):
        for u in (1, 2, 4):
            out |= {_text("flat_kernel", "float32", u, nt), _text("rows_kernel", "float32", u, nt)}
        for dt in ("float16", "bfloat16"):
            for u in (2, 4):
                out |= {_text("flat_kernel", dt, u, nt), _text("rows_kernel", dt, u, nt)}
            out.add(_text("window_kernel<vector>", dt, 1, nt))
        for dt in DTYPES:
            for shape, u in (("flat_paced_kernel", 4), ("rowsteps_kernel", 4), ("shortrows_kernel", 4), ("lastaxis_kernel", 2),
                             ("lastaxis_kernel", 4), ("window_kernel<vector>", 4)):
                out.add(_text(shape, dt, u, nt))
        out |= {_text("rows_kernel_finetail", "float32", 4, nt), _text("gather_kernel", "float32", 4, nt)}
    for dt in DTYPES:
        out |= {_text("flat_scalar_kernel", dt, 1, 0), _text("window_kernel<scalar>", dt, 4, 1)}
    return out


@pytest.mark.parametrize("cus", CUS)
def test_the_table_names_every_route_instance_and_branch(cus):
    table = cases(cus)
    assert [c.id for c in table] == [c.id for c in cases(256)]
    notes, branches = set(), set()
    for c in table:
        n = c.outer * c.C * c.inner
        assert 0 < n <= 1 << 23, c.id
        note = case_note(c, cus)
        assert note.startswith(KERNEL[c.route]), f"{c.id} (cus = {cus}) goes to {note}"
        notes.add(note)
        branches |= _branches(c, cus)
        if c.route == "finetail":                             # at most one round of 4 cus + 3 tiles
            assert n // 4096 <= 4 * cus + 3 and sum(case_instance(c, cus).values()) == n // 4096
    assert not _required_notes() - notes, sorted(_required_notes() - notes)
    assert not REQUIRED_BRANCHES - branches, sorted(REQUIRED_BRANCHES - branches)
    # the shape that is finetail without a zero-point table, and has bulk = 3, is rows_kernel with one
    bulk = [c for c in table if c.route == "finetail" and c.C == 4 * cus + 3]
    assert bulk and all(case_instance(c, cus) == {"bulk": 3, "tail": 4 * cus} for c in bulk)


def test_the_examples_of_the_notes_read_as_the_library_writes_them():
    assert expected_note("channel", "bfloat16", 3, 5, 8) == "shortrows_kernel<AffineOp,in2B,out2B,U=4,NT=2>"
    assert expected_note("channel", "float32", 2, 3, 3000) == "rows_kernel<AffineOp,in4B,out4B,U=1,NT=2>"
    assert expected_note("channel", "float32", 2, 3, 3002) == "gather_kernel<AffineOp,in4B,out4B,U=4,NT=2>"
    assert expected_note("tensor", "float32", 1, 1, 5, x_aligned=False) == "flat_scalar_kernel<AffineOp,in4B,out4B,U=1,NT=0>"
    assert expected_note("tensor", "float16", 1, 1, 4096, tuning={"nt": 2}) == "flat_kernel<AffineOp,in2B,out2B,U=2,NT=2>"
    # the launches bench.py measures: 4096 x 4096 float32 per channel along axis 0 (two rounds: the fine tail), bfloat16 (one
    # round: shortrows), 64 MiB per tensor (one round: paced)
    assert expected_note("channel", "float32", 1, 4096, 4096, has_zp=False,
                         tuning={"cached_store_max_mb": 0}) == "rows_kernel_finetail<AffineOp,in4B,out4B,U=4,NT=1>"
    assert expected_note("channel", "bfloat16", 1, 4096, 4096, has_zp=False) == "shortrows_kernel<AffineOp,in2B,out2B,U=4,NT=2>"
    assert expected_note("tensor", "float32", 1, 1, 2048 * 4096).startswith("flat_paced_kernel<")


@pytest.mark.parametrize("cus", CUS)
def test_the_value_sweeps_reach_their_routes(cus):
    for route, dt in sweep_routes():
        entry, (outer, C, inner), idx, xoff, has_zp, tuning = sweep_layout(route, dt, cus)
        assert idx.shape == ((outer, C, inner) if entry == "channel" else (inner,)) and idx.size <= 1 << 23
        note = expected_note(entry, dt, outer, C, inner, x_aligned=xoff == 0, has_zp=has_zp, cus=cus, tuning=tuning)
        kernel = route.split("-")[0]
        assert note.startswith(KERNEL[kernel]), f"{route} {dt} (cus = {cus}) goes to {note}"
        inst = instance(entry, dt, outer, C, inner, x_aligned=xoff == 0, has_zp=has_zp, cus=cus, tuning=tuning)
        if kernel == "shortrows":
            assert inst["ZP"] == ("zp" in route) and inst["WHOLE"] == ("whole" in route) and inst["paced"] == ("paced" in route)
            for name, sets in TABLES.items():                 # the wave ballot: every wave exact / the waves with work not (an idle
                                                              # wave of the last block votes with the tile's first row alone)
                scales = _channel_sets(sets, C)[0]
                got = shortrows_exact(outer * C * inner, inner, C, VEC[dt], scales, inst["WHOLE"])
                assert got == {True} if name in EXACT_TABLES else False in got, (route, dt, name, got)
        if route == "window-wu1":
            assert inst["wu"] == 1
        elif kernel == "window":
            assert inst["wu"] == 4
        if route == "lastaxis":
            assert inst == {"U": 2, "ZP": False}
        if route == "lastaxis-zp":
            assert inst == {"U": 4, "ZP": True}
        if route == "gather-short":
            assert {"several/in_row", "several/crossing"} <= tile_branches(outer * C * inner, inner, C, 4)
        if route == "gather-long":
            assert {"one_row", "two_rows/aligned"} <= tile_branches(outer * C * inner, inner, C, 4)


def test_the_tables_of_the_sweeps():
    assert len(INRANGE) == 5 and all(2.0 ** -100 <= np.float32(p[0]) <= 2.0 ** 100 for p in INRANGE)
    assert len(SIGNED) == 5 and all(2.0 ** -100 <= np.float32(p[0]) <= 2.0 ** 100 for p in SIGNED) and max(p[0] for p in SIGNED) == 1e30
    for sets in (UNSIGNED, HUGE):                              # one scale outside recip_exact's range each: the IEEE division
        assert len(sets) == 5 and sum(not 2.0 ** -100 <= np.float32(p[0]) <= 2.0 ** 100 for p in sets) == 1
    for p in ALL_PARAMS:                                       # normal scales with a finite, normal reciprocal
        s = np.float32(p[0])
        assert np.isfinite(np.float32(1) / s) and s >= np.finfo(np.float32).tiny and np.float32(1) / s >= np.finfo(np.float32).tiny


@pytest.mark.parametrize("dt", DTYPES)
def test_expected_values_follow_the_saturation_rule_and_the_four_operation_form(dt):
    from oracle import mctq_oracle as O
    x = _sweep_host(dt)[1]
    expo = (x.view(np.uint32) >> 23) & 0xFF
    if dt == "float32":
        assert len(np.unique(expo)) == 256                     # every float32 exponent
    nan, pinf, ninf = np.isnan(x), np.isposinf(x), np.isneginf(x)
    assert nan.sum() > 2 and pinf.any() and ninf.any()
    for scale, zp, qmin, qmax in ALL_PARAMS:
        y = want(x, np.float32(scale), zp, qmin, qmax, None, dt)
        assert not np.isnan(y).any()
        s = np.float32(scale)
        lo = O.narrow(np.float32(np.float32(qmin - zp) * s), dt)
        hi = O.narrow(np.float32(np.float32(qmax - zp) * s), dt)
        assert (y[nan].view(np.uint32) == lo.view(np.uint32)).all() and (y[ninf].view(np.uint32) == lo.view(np.uint32)).all()
        assert (y[pinf].view(np.uint32) == hi.view(np.uint32)).all()
        four = O.narrow(four_operations(x, scale, zp, qmin, qmax), dt)
        assert np.array_equal(four.view(np.uint32), y.view(np.uint32)), (dt, scale, zp, qmin, qmax)
        stored_bits(y, dt)                                     # exact in the storage type


@pytest.mark.parametrize("route,dt", sweep_routes())
def test_finite_inputs_of_the_sweeps_reach_both_ends_of_every_channel(route, dt):
    entry, (outer, C, inner), idx, xoff, has_zp, tuning = sweep_layout(route, dt, 256)
    x1 = _sweep_host(dt)[1]
    if entry == "tensor":
        for prm in ALL_PARAMS:
            y, q = _index(x1, np.float32(prm[0]), prm[1], prm[2], prm[3], None)
            _assert_covers(dt, x1, q, prm[0], prm[2], prm[3], f"{route} {dt} {prm}")
        return
    # every channel (window-wu1: every parameter set) holds the whole vector
    flat_c = np.broadcast_to(np.arange(C)[None, :, None], idx.shape)
    key = flat_c % 5 if route == "window-wu1" else flat_c
    groups = 5 if route == "window-wu1" else C
    seen = np.zeros((groups, x1.size), bool)
    seen[key[idx >= 0], idx[idx >= 0]] = True
    assert seen.all(), f"{route} {dt}: a channel misses {int((~seen).sum())} values"
    for name, sets in TABLES.items():
        scales, zps, domains = _channel_sets(sets, C)
        if not has_zp:
            zps = [0] * C
        for qmin, qmax in domains:
            for c in range(min(C, len(sets))):
                y, q = _index(x1, np.float32(scales[c]), zps[c], qmin, qmax, None)
                assert not np.isnan(y).any()
                _assert_covers(dt, x1, q, scales[c], qmin, qmax, f"{route} {dt} {name} channel {c} [{qmin}, {qmax}]")


@pytest.mark.parametrize("half", range(2))
def test_expected_values_of_the_geometry_cases_hold_no_nan(half):
    table = cases(256)
    for k in range(0, len(table), 2):                          # (k + 1: the same launches under the other cache mode)
        if (k // 2) % 2 != half:
            continue
        c = table[k]
        assert table[k + 1][1:-1] == c[1:-1]
        nans = 0
        for x32, scales, zps, qmin, qmax in geometry_launches(c, k):
            x = as_stored(x32, c.dt)
            nans += int(np.isnan(x).sum())
            y = case_want(c, x, scales, zps, qmin, qmax)
            assert y.shape == x.shape and not np.isnan(y).any(), c.id
            stored_bits(y, c.dt)
        assert nans >= 2, c.id                                 # ... although NaN went in


def test_expected_values_of_the_batched_items_hold_no_nan():
    rng = np.random.default_rng(77)
    for k, (dt, (shape, has_zp, _)) in enumerate(batch_specs()):
        x32, scales, zps, qmin, qmax = batch_launch(rng, k, shape, has_zp)
        x = as_stored(x32, dt)
        z = np.zeros(shape[1], np.int32) if zps is None else zps
        y = want(x, scales, z, qmin, qmax, 1, dt)
        assert (np.isnan(x).any() or x.size < 8) and not np.isnan(y).any(), (dt, shape)


def _index(x, scale, zp, qmin, qmax, axis):
    from oracle import mctq_oracle as O
    xs = np.where(np.isnan(x), np.float32(-np.inf), x)
    return O.fake_quant_affine(xs, scale, zp, qmin, qmax, axis=axis, return_index=True)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_batched_items_reach_every_branch_of_the_tile(dt):
    N = VEC[dt]
    got = set()
    for (outer, C, inner), _, per_tensor in batch_items(N):
        assert (C == 1) == per_tensor
        n = outer * C * inner
        assert n <= 1 << 20                                    # small tensors ride the grid whatever their rows
        got |= tile_branches(n, inner, C, N)
    assert got >= {"one_row", "one_row/partial_vector", "two_rows/aligned", "two_rows/straddle", "two_rows/partial_vector",
                   "several/in_row", "several/crossing", "several/walk", "several/partial_vector", "wraps"}, sorted(got)
