"""The cases of tests/test_gpu_qlinear_routes.py -- the integer product (csrc/mctq_qlinear.hip) on every tile order, K walk and
edge value -- and, without a GPU, the proof that they hold what they claim.

Tile order.  qgemm_i8_glds_kernel, qgemm_i8_wide_kernel and qgemm_i8_pp_kernel map blockIdx.x to a tile in three steps: the
XCD remap ``if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3)``, bands of ``gm`` tile rows, and
``band_rows = min(gm, m_blocks - band * gm)`` for a last, shorter band.  ``tile_map`` replays that arithmetic and ``tiled_gm``
replays launch_glds' choice of gm (``sqrt(chunk * bn / bm)``, tuning key "ql_band", the clamp to m_blocks); the tests below
prove that the grids of ``order_cases`` reach {remap, no remap} x {full bands only, full bands and a shorter last one, a single
band shorter than asked for}.  For the tiled kernels the launcher clamps gm to m_blocks, so the third layout is what a ql_band
above m_blocks (or an automatic gm above it) becomes: one band of all rows.  For the whole-tile kernels GM = 4 is fixed and a
grid of three tile rows is one band of three.

K walk.  ``k_tiled`` / ``k_stream``: every tail length of a 256-byte block and of a 128-byte tile, K below one step, 1 ... 5
and 7 tiles of the variant's own K step with and without a tail, and for the streaming kernels 0 ... 6 full blocks per wave.

Edge values.  ``edge_problem``: one launch without bias whose columns are exact rounding ties (a_scale = 0.5, w_scale = 1,
y_scale = 1), both clamps, a subnormal a_scale * w_scale, a negative scale (a zero sum gives -0.0); one with a bias of NaN,
+inf, -inf, -0.0 and one that cancels to subnormal outputs.

Expected values come from oracle.mctq_oracle.qlinear_i8 (zp_oracle for the zero-point forms, consumers._cpu_epilogue on the
exact int32 sums for the residual form) and, for codes, from fake_quant_affine(..., return_index=True) of that float32 value
with NaN -> quant_min (_want_codes of test_gpu_codes8.py) -- never from a GPU.
"""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_codes8 import _bytes, _want_codes
from test_zp_consumer import zp_oracle

E_ARG = -10001
# variant -> (bm, bn, K step in bytes, LDS buffers of the ring, wave groups): the rows of kQlKernels that launch_glds serves
TILED = {83233: (32, 32, 256, 3, 2), 86433: (64, 32, 256, 3, 2), 86633: (64, 64, 128, 3, 2), 812613: (128, 64, 128, 3, 2),
         166623: (64, 64, 256, 3, 4), 1612623: (128, 64, 256, 3, 4), 612: (64, 128, 128, 2, 1), 1212: (128, 128, 128, 2, 1),
         662: (64, 64, 256, 2, 1)}
# variant -> (bm, bn, the note's kernel name, the note's U): whole tiles only, GM = 4 tile rows per band
WHOLE = {2544: (128, 128, "qlinear_wide_128x128", 4), 2548: (128, 256, "qlinear_wide_128x256", 4),
         2560: (256, 256, "qlinear_pingpong_256x256", 0)}
WHOLE_GM = 4
STREAMS = {181: 1, 182: 2, 184: 4}                            # variant -> MT, 16-row tiles per pass
STREAM_WAVES = 8
LUT16 = (-77, 0, 1, -1, 38, -96, 3, 127, 11, -33, 100, -9, 24, -70, 55, -128)      # entry 0 is not 0: the LUT4 tail rule matters
CODE_FORMS = {False: (0.25, 3, -128, 127), True: (0.3, 100, 0, 255)}               # by parity of the case: int8 / uint8 codes
R_FORM = (0.19, 101)                                          # the uint8 residual's (scale, zero_point)
A_SCALE = 0.02


# ------------------------------------------------------------------------------------------------
# the launchers' arithmetic
# ------------------------------------------------------------------------------------------------

def tiled_name(variant):
    bm, bn, bk, st, kg = TILED[variant]
    ring = "_ring" if st > 2 or (bm == 128 and bn == 64) else ""
    return f"qlinear_tiled{ring}{'_8waves' if kg == 2 else '_16waves' if kg == 4 else ''}_{bm}x{bn}x{bk}"


def note(name, u8, u, zp=False, tail=""):
    """mctq_last_launch of a consumer launch: the kernel, the code types, the form, U."""
    return f"{name}<{'u8' if u8 else 'i8'} x i8{' zp' if zp else ''}{tail},in1B,out4B,U={u},NT=0>"


def tiled_gm(variant, m_blocks, n_blocks, band):
    """(gm as asked for, gm after the clamp): launch_glds with the tuning key ql_band = ``band``."""
    bm, bn = TILED[variant][:2]
    asked = band
    if asked <= 0:
        asked = int(math.sqrt(m_blocks * n_blocks / 8.0 * bn / bm) + 0.5)
    return asked, min(max(asked, 1), m_blocks)


def tile_map(m_blocks, n_blocks, gm):
    """(mb, nb) of every blockIdx.x, as the three kernels compute it."""
    total = m_blocks * n_blocks
    out = []
    for block in range(total):
        i = block
        if total & 7 == 0:
            i = (i & 7) * (total >> 3) + (i >> 3)
        per_band = gm * n_blocks
        band, in_band = divmod(i, per_band)
        band_rows = min(gm, m_blocks - band * gm)
        out.append((band * gm + in_band % band_rows, in_band // band_rows))
    return out


def band_layout(m_blocks, asked):
    """'full': bands of ``asked`` rows only; 'full+short': such bands and a shorter last one; 'short': a single band of fewer
    rows than asked for."""
    asked = max(asked, 1)
    return "short" if asked > m_blocks else "full" if m_blocks % asked == 0 else "full+short"


ORDER_GRIDS = ((3, 8), (5, 8), (5, 3))


def order_bands(m_blocks):
    return (0, 1, 2, 3, m_blocks + 5)


def order_shape(bm, bn, m_blocks, n_blocks):
    """Ragged in M and N by less than a tile."""
    return bm * m_blocks - bm // 2 - 1, bn * n_blocks - 3, 272


def order_cases(variant):
    """[(M, N, K, u8, ql_band, form)] of a tiled variant: three grids x five bands x four forms, both code types dealt."""
    bm, bn = TILED[variant][:2]
    cases = []
    for gi, (mbl, nbl) in enumerate(ORDER_GRIDS):
        M, N, K = order_shape(bm, bn, mbl, nbl)
        for bi, band in enumerate(order_bands(mbl)):
            for fi, form in enumerate(("f32", "codes", "zp", "res")):
                cases.append((M, N, K, (gi + bi + fi) % 2 == 1, band, form))
    return cases


# (6, 4), (5, 8), (5, 3), (3, 8): remap with bands of 4 + 2 and 4 + 1, no remap, remap with a single band of 3; (4, 2), (4, 3)
# and (3, 3) add full bands only with and without the remap and the single shorter band without it.
WHOLE_GRIDS = ((6, 4), (5, 8), (5, 3), (3, 8), (4, 2), (4, 3), (3, 3))


def whole_cases(variant):
    """[(M, N, K, u8, form)]: whole tiles, K = 256 (kt_n = 4, the least these kernels take)."""
    bm, bn = WHOLE[variant][:2]
    return [(bm * mbl, bn * nbl, 256, u8, form) for (mbl, nbl) in WHOLE_GRIDS for u8 in (False, True) for form in ("f32", "codes")]


K_TAILS = tuple(256 + 16 * j for j in range(16))              # every tail length of a 256-byte block and of a 128-byte tile
K_SHORT = (16, 32, 64, 128, 192, 240)                         # less than one step: some wave groups have nothing
STREAM_BLOCKS = (1, 7, 8, 9, 15, 16, 17, 24, 25, 33, 41)
K_STREAM = tuple(256 * b + t for b in STREAM_BLOCKS for t in (0, 16, 144))
TILE_COUNTS = (1, 2, 3, 4, 5, 7)
STREAM_M = (5, 17, 33, 130)
KEY_SETTINGS = ({}, {"ql_rot": 1, "ql_band": 2}, {"ql_stagger": 1})


def k_tiled(variant):
    bk = TILED[variant][2]
    return tuple(sorted(set(K_TAILS + K_SHORT + tuple(bk * c + t for c in TILE_COUNTS for t in (0, 16)))))


def k_stream():
    return tuple(sorted(set(K_TAILS + K_SHORT + K_STREAM)))


def walk_shape(variant):
    bm, bn = TILED[variant][:2]
    return 2 * bm + 1, bn + 1


def packed_mt(M):
    return 1 if M <= 16 else 2 if M <= 32 else 4


# ------------------------------------------------------------------------------------------------
# problems and expected values, one per (shape, code type, weight format)
# ------------------------------------------------------------------------------------------------

def _w_domain(wkind):
    return (-8, 8) if wkind == "w4" else (-128, 128)


def _exact_sums(a, za, w):
    """sum_k (a - za) w as int64: a float64 product is exact here (every partial sum is an integer below 2^53)."""
    acc = np.rint((a.astype(np.float64) - za) @ w.astype(np.float64).T).astype(np.int64)
    assert np.all(np.abs(acc) < 2 ** 31)
    return acc


def pack4(codes):
    """The consumer's 4-bit layout: per group of 8 consecutive k, byte j = (code[j] & 0xF) | (code[j + 4] << 4)."""
    N, K = codes.shape
    g = codes.reshape(N, K // 8, 8).astype(np.int16) & 0xF
    return (g[..., 0:4] | (g[..., 4:8] << 4)).astype(np.uint8).reshape(N, K // 2)


@functools.lru_cache(maxsize=None)
def problem(M, N, K, u8, wkind="i8"):
    """Random codes over their whole domains, outputs of the order of 30 (inside and beyond both code domains), a bias for
    every second (shape, type).  wkind: 'i8', 'w4' (codes in [-8, 7]) or 'lut' (indices into LUT16)."""
    rng = np.random.default_rng([M, N, K, int(u8), ("i8", "w4", "lut").index(wkind)])
    a = rng.integers(0, 256, (M, K)).astype(np.uint8) if u8 else rng.integers(-128, 128, (M, K)).astype(np.int8)
    za = int(rng.integers(0, 256)) if u8 else int(rng.integers(-128, 128))
    p = dict(M=M, N=N, K=K, u8=u8, wkind=wkind, a=a, za=za, sa=A_SCALE)
    if wkind == "lut":
        idx = rng.integers(0, 16, (N, K)).astype(np.uint8)
        w = np.asarray(LUT16, np.int8)[idx]
        p["packed"] = pack4(idx)
    else:
        lo, hi = _w_domain(wkind)
        w = rng.integers(lo, hi, (N, K)).astype(np.int8)
        if wkind == "w4":
            p["packed"] = pack4(w)
        p["zw"] = rng.integers(lo, hi, N).astype(np.int32)
        p["a_rowsum"] = (a.astype(np.int64) - za).sum(1).astype(np.int32)
    w_std = 4.6 if wkind == "w4" else 74.0
    p["w"] = w
    p["rowsum"] = w.astype(np.int32).sum(1, dtype=np.int32)
    p["ws"] = ((rng.random(N) + 0.5) * (30.0 / (A_SCALE * 74.0 * w_std * K ** 0.5))).astype(np.float32)
    p["bias"] = ((rng.random(N) - 0.5) * 20).astype(np.float32) if (M + N + K // 16 + u8) % 2 == 1 else None
    p["residual"] = rng.integers(0, 256, (M, N)).astype(np.uint8)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def out_form(form, u8):
    """The output form of a case: None for float32, else (scale, zero_point, quant_min, quant_max)."""
    return {"f32": None, "codes": CODE_FORMS[u8], "zp": CODE_FORMS[not u8] if u8 else None,
            "res": CODE_FORMS[u8] if u8 else None, "w4": None, "w4zp": None, "lut": None}[form]


def as_bytes(y, out):
    """The output as stored: float32 bits, or the low byte of every code."""
    if out is None:
        return np.ascontiguousarray(y, dtype=np.float32).reshape(-1).view(np.uint8)
    return _bytes(y)


@functools.lru_cache(maxsize=None)
def expected(M, N, K, u8, wkind, form):
    """(the oracle's float32 value, the bytes the launch must write) for one form of one problem."""
    from oracle import mctq_oracle as O
    p = problem(M, N, K, u8, wkind)
    out = out_form(form, u8)
    if form in ("zp", "w4zp"):
        y = zp_oracle(p["a"], p["za"], p["sa"], p["w"], p["zw"], p["ws"], p["bias"])
    elif form == "res":
        from mct_quantizers_amd import consumers
        acc = torch.from_numpy(_exact_sums(p["a"], p["za"], p["w"]).astype(np.int32))
        t = lambda v: None if v is None else torch.from_numpy(np.array(v))      # noqa: E731  (a writable copy)
        y = consumers._cpu_epilogue(acc, p["sa"], t(p["ws"]), t(p["bias"]), out, t(p["residual"]), R_FORM, True).numpy()
        return y, (as_bytes(y, None) if out is None else _bytes(y))
    else:
        y = O.qlinear_i8(p["a"], p["za"], p["sa"], p["w"], p["ws"], p["bias"])
    if out is None:
        return y, as_bytes(y, None)
    return y, _bytes(_want_codes(y, np.float32(out[0]), out[1], out[2], out[3]))


# ------------------------------------------------------------------------------------------------
# edge values of the epilogue
# ------------------------------------------------------------------------------------------------

F32 = np.float32
SUB = F32(2.0) ** -126                                        # the smallest normal float32
# per column n % 8: the weight scale, and the bias of the launch that has one
EDGE_WS = (F32(1.0), F32(512.0), F32(1e-40), F32(-0.37), F32(1.0), F32(0.37), F32(3.0) * SUB, F32(3.0))
EDGE_BIAS = (F32("nan"), F32("inf"), F32("-inf"), F32(-0.0), F32(0.25), F32(-1e-3), -SUB, F32(1e30))
EDGE_A_SCALE = 0.5
TIE_FORM = (1.0, 3, -128, 127)
# launch "plain": no bias, y_scale = 1 -- the ties; an int8, a uint8 and a 4-bit domain inside int8.  Launch "bias": the
# non-finite columns; zero points at either end of either domain (PARAMS of test_gpu_codes8.py), a 4-bit domain.
EDGE_FORMS = {"plain": (None, TIE_FORM, (1.0, 128, 0, 255), (1.0, 0, -8, 7)),
              "bias": (None, (0.25, -128, -128, 127), (0.2, 127, -128, 127), (0.3, 0, 0, 255), (0.0123, 255, 0, 255), (2.0, 1, -8, 7))}


@functools.lru_cache(maxsize=None)
def edge_problem(M, N, K, u8, wkind="i8"):
    """Small sums (a - za in [-3, 3], w in {-1, 0, 1}: a standard deviation of about sqrt(K) * 1.6) so that half of them land
    inside every code domain; row 0 of the activations is the zero point, so its sums are zero."""
    rng = np.random.default_rng([7, M, N, K, int(u8), ("i8", "w4", "lut").index(wkind)])
    za = 114 if u8 else -5
    a = (za + rng.integers(-3, 4, (M, K))).astype(np.uint8 if u8 else np.int8)
    a[0] = za
    w = rng.integers(-1, 2, (N, K)).astype(np.int8)
    p = dict(M=M, N=N, K=K, u8=u8, wkind=wkind, a=a, za=za, sa=EDGE_A_SCALE, w=w)
    if wkind == "lut":
        p["packed"] = pack4(np.asarray([LUT16.index(v) for v in (-1, 0, 1)], np.uint8)[w + 1])
    elif wkind == "w4":
        p["packed"] = pack4(w)
    p["rowsum"] = w.astype(np.int32).sum(1, dtype=np.int32)
    p["ws"] = np.asarray([EDGE_WS[n % 8] for n in range(N)], F32)
    p["edge_bias"] = np.asarray([EDGE_BIAS[n % 8] for n in range(N)], F32)
    p["acc"] = _exact_sums(a, za, w)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def edge_expected(M, N, K, u8, wkind, launch, fi):
    from oracle import mctq_oracle as O
    p = edge_problem(M, N, K, u8, wkind)
    out = EDGE_FORMS[launch][fi]
    y = O.qlinear_i8(p["a"], p["za"], p["sa"], p["w"], p["ws"], p["edge_bias"] if launch == "bias" else None)
    if out is None:
        return y, as_bytes(y, None)
    return y, _bytes(_want_codes(y, np.float32(out[0]), out[1], out[2], out[3]))


# (M, N, K) of the edge problem of each epilogue implementation: ragged where the kernel takes it
EDGE_SHAPES = {"packed": (33, 40, 272), "stream": (33, 40, 272), "tiled": (70, 72, 272), "whole": (256, 256, 256)}


# ------------------------------------------------------------------------------------------------
# the cases hold what they claim (no GPU)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sorted(TILED))
def test_tile_order_cases_reach_every_mapping_of_the_tiled_kernels(variant):
    bm, bn = TILED[variant][:2]
    seen = set()
    for (M, N, K, u8, band, form) in order_cases(variant):
        mbl, nbl = -(-M // bm), -(-N // bn)
        assert (mbl, nbl) in ORDER_GRIDS and 0 < bm * mbl - M < bm and 0 < bn * nbl - N < bn and K == 272
        asked, gm = tiled_gm(variant, mbl, nbl, band)
        assert 1 <= gm <= mbl and (band == 0 or asked == band)
        tiles = tile_map(mbl, nbl, gm)
        assert sorted(tiles) == [(m, n) for m in range(mbl) for n in range(nbl)]       # every tile once: what the kernel must do
        seen.add(((mbl * nbl) % 8 == 0, band_layout(mbl, asked), form, u8))
        if gm == 1 and (mbl * nbl) % 8:                                                # no remap, bands of one row: row-major
            assert tiles == [(i // nbl, i % nbl) for i in range(mbl * nbl)]
    for remap in (True, False):
        for layout in ("full", "full+short", "short"):
            for form in ("f32", "codes", "zp", "res"):
                assert {u8 for (r, l, f, u8) in seen if (r, l, f) == (remap, layout, form)}, (variant, remap, layout, form)
    for form in ("f32", "codes", "zp", "res"):
        assert {u8 for (_, _, f, u8) in seen if f == form} == {False, True}
    # the remap really permutes (block 1 is the first tile of the second XCD's share), and a shorter last band changes the order
    assert tile_map(3, 8, 1)[:3] == [(0, 0), (0, 3), (0, 6)] and tile_map(5, 3, 2)[12:] == [(4, 0), (4, 1), (4, 2)]


def test_automatic_band_is_the_launchers_formula():
    """gm = (int)(sqrt(m_blocks * n_blocks / 8 * bn / bm) + 0.5), clamped to 1 ... m_blocks: the values the GPU test requires in
    the launch note, spelled out for one variant of every tile shape."""
    assert [tiled_gm(83233, *g, 0)[1] for g in ORDER_GRIDS] == [2, 2, 1]              # 32 x 32: sqrt(3), sqrt(5), sqrt(1.875)
    assert [tiled_gm(86433, *g, 0)[1] for g in ORDER_GRIDS] == [1, 2, 1]              # 64 x 32: sqrt(1.5), sqrt(2.5), sqrt(0.94)
    assert [tiled_gm(612, *g, 0)[1] for g in ORDER_GRIDS] == [2, 3, 2]                # 64 x 128: sqrt(6), sqrt(10), sqrt(3.75)
    assert [tiled_gm(812613, *g, 0)[1] for g in ORDER_GRIDS] == [1, 2, 1]             # 128 x 64
    assert tiled_gm(662, 3, 8, 8) == (8, 3) and tiled_gm(662, 3, 2, 2) == (2, 2) and tiled_gm(662, 3, 2, 0)[1] == 1
    for variant in TILED:                                                             # the K walk's grid: 3 x 2 tiles, no remap
        M, N = walk_shape(variant)
        bm, bn = TILED[variant][:2]
        assert (-(-M // bm), -(-N // bn)) == (3, 2)


@pytest.mark.parametrize("variant", sorted(WHOLE))
def test_whole_tile_cases_reach_every_mapping(variant):
    bm, bn = WHOLE[variant][:2]
    seen = set()
    for (M, N, K, u8, form) in whole_cases(variant):
        assert M % bm == 0 and N % bn == 0 and K == 256
        mbl, nbl = M // bm, N // bn
        tiles = tile_map(mbl, nbl, WHOLE_GM)
        assert sorted(tiles) == [(m, n) for m in range(mbl) for n in range(nbl)]
        seen.add(((mbl * nbl) % 8 == 0, band_layout(mbl, WHOLE_GM), form, u8))
    assert seen == {(r, l, f, u) for r in (True, False) for l in ("full", "full+short", "short") for f in ("f32", "codes")
                    for u in (False, True)}
    assert max(M * N for (M, N, K, u8, form) in whole_cases(2560)) == 1280 * 2048 and (1536, 1024, 256, False, "f32") in whole_cases(2560)


def test_k_walk_reaches_every_tail_and_every_depth_of_the_loops():
    for variant, (bm, bn, bk, st, kg) in TILED.items():
        ks = k_tiled(variant)
        assert all(k % 16 == 0 and 16 <= k <= 32768 for k in ks)
        assert {k % bk for k in ks} == set(range(0, bk, 16))                          # every length of the ragged last tile
        assert {-(-k // bk) for k in ks} >= {1, 2, 3, 4, 5, 7, 8}                     # ring prologue, steady state, drain
        assert all(bk * c in ks and bk * c + 16 in ks for c in TILE_COUNTS)
        # a tail that leaves whole wave groups without data: group g multiplies sub-steps [g, g + 1) * bk / 64 / kg of a tile
        sub = bk // 64 // kg
        if kg > 1:
            assert {min(kg, -(-(k % bk) // (64 * sub))) for k in ks if k % bk} == set(range(1, kg + 1))
    ks = k_stream()
    assert {k % 256 for k in ks} == set(range(0, 256, 16)) and max(ks) <= 32768
    per_wave = {b: [(b - wv + STREAM_WAVES - 1) // STREAM_WAVES if b > wv else 0 for wv in range(STREAM_WAVES)] for b in STREAM_BLOCKS}
    assert {n for b in STREAM_BLOCKS if b < 41 for n in per_wave[b]} == {0, 1, 2, 3, 4, 5} and max(per_wave[41]) == 6
    assert any(len(set(per_wave[b])) > 1 for b in STREAM_BLOCKS)                      # mixed within a block
    assert {packed_mt(M) for M in STREAM_M} == {1, 2, 4} and {M <= 16 for M in STREAM_M} == {M <= 32 for M in STREAM_M} == {True, False}
    assert KEY_SETTINGS[1] == {"ql_rot": 1, "ql_band": 2} and tiled_gm(662, 3, 2, 2)[1] == 2     # the rotation needs gm > 1


def _edge_cases():
    for kind, (M, N, K) in EDGE_SHAPES.items():
        for u8 in (False, True):
            for wkind in (("w4", "lut") if kind == "packed" else ("i8",)):
                yield M, N, K, u8, wkind


def test_edge_columns_hold_what_they_claim():
    for (M, N, K, u8, wkind) in _edge_cases():
        p = edge_problem(M, N, K, u8, wkind)
        cols = np.arange(N) % 8
        # ties: v * inv = sum / 2 exactly, a tie whenever the sum is odd -- at least a quarter of the tie columns, inside the
        # domain, with the even neighbour below and above
        y, _ = edge_expected(M, N, K, u8, wkind, "plain", 0)
        tie_cols = (cols == 0) | (cols == 4)
        v = y[:, tie_cols].astype(np.float64)
        assert np.array_equal(v, p["acc"][:, tie_cols] * 0.5)
        codes = _want_codes(y, np.float32(TIE_FORM[0]), *TIE_FORM[1:])[:, tie_cols]
        inside = (codes > TIE_FORM[2]) & (codes < TIE_FORM[3])
        ties = (np.abs(v - np.floor(v) - 0.5) == 0) & inside
        assert ties.sum() * 4 >= v.size, (M, N, K, u8, wkind, int(ties.sum()), v.size)
        down, up = codes - TIE_FORM[1] == np.floor(v), codes - TIE_FORM[1] == np.floor(v) + 1
        assert (ties & down).any() and (ties & up).any() and np.all((codes[ties] - TIE_FORM[1]) % 2 == 0)
        # signed zeros in the float32 output: +0.0 from a positive scale, -0.0 from a negative one, with and without bias
        bits = y.view(np.uint32)
        assert (bits[0] == 0).any() and (bits[0] == 0x80000000).any()
        yb, _ = edge_expected(M, N, K, u8, wkind, "bias", 0)
        assert np.all(yb.view(np.uint32)[0, cols == 3] == 0x80000000)
        # a subnormal a_scale * w_scale, and a normal one whose outputs the bias cancels down to subnormals
        tiny = np.float32(np.finfo(np.float32).tiny)
        sc = np.float32(EDGE_A_SCALE) * p["ws"]
        assert np.all((sc[cols == 2] > 0) & (sc[cols == 2] < tiny)) and np.all(sc[cols == 6] >= tiny)
        for out_y, col in ((y, 2), (yb, 6)):
            sel = out_y[:, cols == col]
            assert ((sel != 0) & (np.abs(sel) < tiny)).any(), (col, M, N, K, u8, wkind)
        # NaN and both infinities reach the clamp through the bias
        assert np.isnan(yb[:, cols == 0]).all() and np.isposinf(yb[:, cols == 1]).all() and np.isneginf(yb[:, cols == 2]).all()
        for launch, forms in EDGE_FORMS.items():
            for fi, out in enumerate(forms):
                if out is None:
                    continue
                yy, raw = edge_expected(M, N, K, u8, wkind, launch, fi)
                c = _want_codes(yy, np.float32(out[0]), *out[1:])
                assert c.min() == out[2] and c.max() == out[3] and len(np.unique(c)) > 8, (launch, out, np.unique(c))
                if launch == "bias":                                                   # quant_min, quant_max, quant_min
                    assert np.all(c[:, cols == 0] == out[2]) and np.all(c[:, cols == 1] == out[3]) and np.all(c[:, cols == 2] == out[2])
                assert raw.size == M * N


def test_expected_values_of_the_forms_differ_and_fill_their_domains():
    """The shared problems: every form has its own expectation, and the codes are no saturated handful."""
    M, N, K = order_shape(64, 64, 5, 3)
    for u8 in (False, True):
        ys = {form: expected(M, N, K, u8, "i8", form) for form in ("f32", "codes", "zp", "res")}
        assert not np.array_equal(ys["f32"][0], ys["zp"][0])
        out = CODE_FORMS[u8]
        c = _want_codes(ys["f32"][0], np.float32(out[0]), *out[1:])
        assert c.min() == out[2] and c.max() == out[3] and len(np.unique(c)) > 50
        assert ys["codes"][1].size == M * N and ys["f32"][1].size == 4 * M * N
        assert (ys["res"][0] == (out[1] if u8 else 0)).any()                           # the ReLU's floor
    p = problem(17, 17, 272, True, "lut")
    lut = np.asarray(LUT16)
    assert LUT16[0] != 0 and np.array_equal(p["rowsum"], lut[p["packed"] & 15].sum(1) + lut[p["packed"] >> 4].sum(1))


# ------------------------------------------------------------------------------------------------
# the tuning keys themselves (mctq_set_tuning is host code)
# ------------------------------------------------------------------------------------------------

KEY_REFUSALS = {"ql_rot": ((-1, 2, 7), b"ql_rot must be 0 or 1"), "ql_stagger": ((-1, 2, 7), b"ql_stagger must be 0 or 1"),
                "ql_band": ((-1, 4097, 1 << 20), b"ql_band must be 0 (automatic) or the number of tile rows per band")}


def test_tuning_keys_accept_their_domain_and_refuse_the_rest():
    from mct_quantizers_amd.hip import native
    lib = native.load()
    try:
        for key, ok in (("ql_rot", (0, 1)), ("ql_stagger", (0, 1)), ("ql_band", (0, 1, 2, 4096))):
            for v in ok:
                assert lib.mctq_set_tuning(key.encode(), v) == 0, (key, v)
            bad, message = KEY_REFUSALS[key]
            for v in bad:
                assert lib.mctq_set_tuning(key.encode(), v) == E_ARG == native.MCTQ_E_ARG, (key, v)
                assert lib.mctq_last_error() == message, lib.mctq_last_error()
    finally:
        for key in KEY_REFUSALS:
            assert lib.mctq_set_tuning(key.encode(), 0) == 0
