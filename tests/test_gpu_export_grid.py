"""The export-grid kernels (mctq_grid_per_tensor_f32 / mctq_grid_per_channel_f32: GridOp on the shared launchers) on every
launch route, at misaligned pointers and at edge values, through the raw C ABI.

Expected values: oracle.mctq_oracle.export_grid (numpy, float32 throughout; anchored in the reference for these inputs by
tests/golden/export_edges.*, tests/test_export_edges.py).  Bar: equality bit for bit on EVERY element -- NaN matches NaN,
signed zeros must agree, nothing excluded, no tolerance.  Every output sits in a frame with 64 guard elements on each side
which must keep their bits, and starts as a sentinel no result can equal, so that an unwritten element shows.
GridOp is not an affine op: its route depends on shape and alignment only, so every case names the route it must take.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_VALUE = 768.0
SENTINEL = 12345.0            # no result: results lie on a grid inside [-4, 4], or are NaN / +-inf

ROUTES = ("rows_kernel<", "lastaxis_kernel<", "window_kernel<vector>", "window_kernel<scalar>", "flat_kernel<",
          "flat_scalar_kernel<")


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    return native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(got, want):
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    if got.shape != want.shape:
        return False, f"shape {got.shape} vs {want.shape}"
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if ok.all():
        return True, ""
    i = int(np.flatnonzero(~ok)[0])
    return False, f"{int((~ok).sum())} of {ok.size} mismatch, first at {i}: got={got[i]!r} want={want[i]!r}"


def _route(text):
    assert "GridOp" in text, text
    hits = [r for r in ROUTES if text.startswith(r)]
    assert len(hits) == 1, text
    return hits[0]


class _Frame:
    """x at ``xoff`` elements and y at ``yoff`` elements off a 256-byte boundary; y framed by guards."""

    def __init__(self, x_np, xoff=0, yoff=0):
        n = x_np.size
        self.n, self.yoff = n, yoff
        self.xb = torch.zeros(n + xoff, dtype=torch.float32, device="cuda")
        self.xb[xoff:] = torch.from_numpy(np.ascontiguousarray(x_np).reshape(-1)).cuda()
        self.x = self.xb[xoff:]
        self.frame = torch.full((n + yoff + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
        self.y = self.frame[GUARD + yoff:GUARD + yoff + n]
        self.y.fill_(SENTINEL)
        assert self.x.data_ptr() % 16 == (4 * xoff) % 16 and self.y.data_ptr() % 16 == (4 * yoff) % 16

    def result(self, what):
        torch.cuda.synchronize()
        f = self.frame.cpu().numpy()
        a = GUARD + self.yoff
        edge = np.concatenate([f[:a], f[a + self.n:]])
        assert np.array_equal(edge.view(np.uint32), np.full(edge.shape, GUARD_VALUE, np.float32).view(np.uint32)), \
            f"{what}: wrote outside its tensor"
        return f[a:a + self.n]


def _table(values, off):
    """Device copy of a parameter table, ``off`` elements off a 16-byte boundary."""
    buf = torch.zeros(len(values) + off, dtype=torch.float32, device="cuda")
    buf[off:] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).cuda()
    t = buf[off:]
    assert t.data_ptr() % 16 == (4 * off) % 16
    return t


def _launch_channels(lib, x_np, lo, hi, step, shifted, xoff=0, yoff=0, tab_off=(0, 0, 0)):
    from mct_quantizers_amd.hip import native
    outer, C, inner = x_np.shape
    fr = _Frame(x_np, xoff, yoff)
    tabs = [_table(v, o) for v, o in zip((lo, hi, step), tab_off)]
    rc = lib.mctq_grid_per_channel_f32(fr.x.data_ptr(), fr.y.data_ptr(), outer, C, inner, tabs[0].data_ptr(),
                                       tabs[1].data_ptr(), tabs[2].data_ptr(), int(shifted), _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    return fr.result(f"{x_np.shape} x+{xoff} y+{yoff} tables+{tab_off} shifted={shifted} [{text}]"), text


def _launch_tensor(lib, x_np, lo, hi, step, shifted, xoff=0, yoff=0):
    from mct_quantizers_amd.hip import native
    fr = _Frame(x_np, xoff, yoff)
    rc = lib.mctq_grid_per_tensor_f32(fr.x.data_ptr(), fr.y.data_ptr(), x_np.size, float(lo), float(hi), float(step),
                                      int(shifted), _stream())
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    return fr.result(f"n={x_np.size} x+{xoff} y+{yoff} shifted={shifted} [{text}]"), text


# ------------------------------------------------------------------------------------------------
# 1. per-channel geometry: (route, outer, C, inner, x offset, y offset, table offsets)
# ------------------------------------------------------------------------------------------------

def _geometry():
    g = []
    # rows_kernel: inner % 4 == 0 and inner >= 1024; a tile is 4096 elements (one variant: four lane-vectors per lane)
    for shape in ((3, 5, 1024), (2, 3, 4096), (2, 3, 4100), (1, 2, 12292), (5, 1, 2048)):
        g.append(("rows_kernel<", *shape, 0, 0, (0, 0, 0)))
    # lastaxis_kernel: inner == 1, C % 4 == 0, tables 16-byte aligned.  The outers give a full group, a short group and a
    # short second slab whatever slab height the launcher's waste search picks.
    for C in (4, 8):
        for outer in (1, 27, 2047, 4096, 5000, 6151):
            g.append(("lastaxis_kernel<", outer, C, 1, 0, 0, (0, 0, 0)))
    g.append(("lastaxis_kernel<", 700, 12, 1, 0, 0, (0, 0, 0)))      # 3 lane-vectors per row: does not divide 256
    g.append(("lastaxis_kernel<", 41, 64, 1, 0, 0, (0, 0, 0)))
    for outer in (1, 3, 37, 70):
        g.append(("lastaxis_kernel<", outer, 4096, 1, 0, 0, (0, 0, 0)))
    # lastaxis fall-back: one table 4 bytes off a 16-byte boundary -> the window route, and still exact
    for k in range(3):
        g.append(("window_kernel<vector>", 41, 64, 1, 0, 0, tuple(int(j == k) for j in range(3))))
    for shape in ((1, 1, 1), (50, 3, 1), (1, 5001, 1), (33, 5, 2), (4, 6, 5), (2, 8, 100), (4, 6, 1020), (3, 5, 1030),
                  (1, 3000, 3), (2, 300, 576)):
        g.append(("window_kernel<vector>", *shape, 0, 0, (0, 0, 0)))
    for shape in ((4, 6, 5), (3, 5, 1024), (41, 64, 1), (1, 3000, 3)):
        for xoff, yoff in ((1, 0), (0, 1), (3, 3)):
            g.append(("window_kernel<scalar>", *shape, xoff, yoff, (0, 0, 0)))
    return g


GEOMETRY = _geometry()
_OBSERVED = {}


def _geo_id(case):
    route, outer, C, inner, xoff, yoff, toff = case
    return f"{route.rstrip('<').replace('<', '_').replace('>', '')}-{outer}x{C}x{inner}-x{xoff}y{yoff}-t{''.join(map(str, toff))}"


@pytest.mark.parametrize("case", GEOMETRY, ids=_geo_id)
def test_grid_per_channel_geometry_vs_oracle(lib, case):
    from oracle import mctq_oracle as O
    from oracle.grid_inputs import grid_edge_inputs, grid_params
    route, outer, C, inner, xoff, yoff, toff = case
    rng = np.random.default_rng([outer, C, inner, xoff, yoff])
    for zero_lo in (False, True):
        lo, hi, step = grid_params(rng, C, zero_lo)
        x = grid_edge_inputs(rng, (outer, C, inner), lo, hi, step, axis=1)
        for shifted in (0, 1):
            got, text = _launch_channels(lib, x, lo, hi, step, shifted, xoff, yoff, toff)
            assert _route(text) == route, f"{case}: took {text}"
            _OBSERVED[_geo_id(case)] = _route(text)
            ok, why = _same(got, O.export_grid(x, lo, hi, step, 1, bool(shifted)))
            assert ok, f"{case} zero_lo={zero_lo} shifted={shifted} [{text}]: {why}"


# ------------------------------------------------------------------------------------------------
# 2. per tensor
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 4103, 12289, 1 << 20])
@pytest.mark.parametrize("xoff,yoff", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_grid_per_tensor_vs_oracle(lib, n, xoff, yoff):
    from oracle import mctq_oracle as O
    from oracle.grid_inputs import grid_edge_inputs, grid_params
    rng = np.random.default_rng([n, xoff, yoff])
    route = "flat_kernel<" if xoff == 0 and yoff == 0 else "flat_scalar_kernel<"
    for zero_lo in (False, True):
        lo, hi, step = (v[0] for v in grid_params(rng, 1, zero_lo))
        x = grid_edge_inputs(rng, (n,), lo, hi, step)
        for shifted in (0, 1):
            got, text = _launch_tensor(lib, x, lo, hi, step, shifted, xoff, yoff)
            assert _route(text) == route, f"n={n} x+{xoff} y+{yoff}: took {text}"
            _OBSERVED[f"flat-{n}-{xoff}-{yoff}"] = _route(text)
            ok, why = _same(got, O.export_grid(x, lo, hi, step, None, bool(shifted)))
            assert ok, f"n={n} x+{xoff} y+{yoff} zero_lo={zero_lo} shifted={shifted} [{text}]: {why}"


def test_grid_empty_tensor_launches_nothing(lib):
    from mct_quantizers_amd.hip import native
    before = native.launch_count()
    for shifted in (0, 1):
        assert lib.mctq_grid_per_tensor_f32(None, None, 0, -1.0, 1.0, 0.125, shifted, _stream()) == 0
    assert native.launch_count() == before


def test_every_grid_route_is_reached(lib):
    """After the whole list: all six routes were taken under GridOp.  Cases this process has not run yet (a selection
    with -k, another order) are launched here, so the test does not depend on the ones above having run."""
    from oracle.grid_inputs import grid_edge_inputs, grid_params
    rng = np.random.default_rng(3)
    for case in GEOMETRY:
        if _geo_id(case) not in _OBSERVED:
            route, outer, C, inner, xoff, yoff, toff = case
            lo, hi, step = grid_params(rng, C)
            _, text = _launch_channels(lib, grid_edge_inputs(rng, (outer, C, inner), lo, hi, step, 1), lo, hi, step, 0,
                                       xoff, yoff, toff)
            _OBSERVED[_geo_id(case)] = _route(text)
    for off in (0, 1):
        if f"flat-1023-{off}-{off}" not in _OBSERVED:
            lo, hi, step = (v[0] for v in grid_params(rng, 1))
            _, text = _launch_tensor(lib, grid_edge_inputs(rng, (1023,), lo, hi, step), lo, hi, step, 0, off, off)
            _OBSERVED[f"flat-1023-{off}-{off}"] = _route(text)
    assert set(_OBSERVED.values()) == set(ROUTES), sorted(set(_OBSERVED.values()))
    for case in GEOMETRY:
        assert _OBSERVED[_geo_id(case)] == case[0], case


@pytest.mark.parametrize("route,shape,off", [("rows_kernel<", (2, 3, 4100), 0), ("lastaxis_kernel<", (27, 8, 1), 0),
                                             ("window_kernel<vector>", (4, 6, 5), 0), ("window_kernel<scalar>", (4, 6, 5), 1)])
def test_constant_tables_equal_the_per_tensor_launch(lib, route, shape, off):
    from oracle.grid_inputs import grid_edge_inputs, grid_params
    rng = np.random.default_rng([7, *shape, off])
    C = shape[1]
    for zero_lo in (False, True):
        lo, hi, step = (v[0] for v in grid_params(rng, 1, zero_lo))
        x = grid_edge_inputs(rng, shape, lo, hi, step)
        full = lambda v: np.full(C, v, np.float32)                    # noqa: E731
        for shifted in (0, 1):
            a, text = _launch_channels(lib, x, full(lo), full(hi), full(step), shifted, off, off)
            assert _route(text) == route, text
            b, _ = _launch_tensor(lib, x.reshape(-1), lo, hi, step, shifted)
            ok, why = _same(a, b)
            assert ok, f"{shape} zero_lo={zero_lo} shifted={shifted} [{text}]: {why}"


# ------------------------------------------------------------------------------------------------
# 3. every 251st float32 bit pattern (both signs, every exponent, NaN payloads, denormals): what the full sweep of
#    tests/test_onnx_export.py (per tensor, unshifted, one parameter set) leaves out
# ------------------------------------------------------------------------------------------------

SWEEP_N = ((1 << 32) + 250) // 251                     # bits = 251 * i < 2^32: 17 111 424 patterns
_FACTORS = np.asarray([1, 0.5, 3, 0.7, 1.9, 0.11, 2.5, 1.3], dtype=np.float32)   # channel 0: the per-tensor set itself


def _sweep_params(name, channels):
    f = _FACTORS[:channels]
    if name == "signed":                               # the existing sweep's set
        thr = (np.float32(1.3) * f).astype(np.float32)
        step = (thr / np.float32(128)).astype(np.float32)
        return -thr, (thr - step).astype(np.float32), step
    if name == "unsigned":                             # (0, 255 s, s)
        step = (np.float32(1.3 / 128) * f).astype(np.float32)
        return np.zeros(channels, np.float32), (np.float32(255) * step).astype(np.float32), step
    lo, hi = (np.float32(-0.37) * f).astype(np.float32), (np.float32(0.91) * f).astype(np.float32)
    return lo, hi, ((hi - lo) / np.float32(255)).astype(np.float32)       # "offgrid": lo is no multiple of the step


@functools.lru_cache(maxsize=1)
def _sweep_device():
    return (torch.arange(SWEEP_N, dtype=torch.int64, device="cuda") * 251).to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=1)
def _sweep_host():
    x = (np.arange(SWEEP_N, dtype=np.uint64) * np.uint64(251)).astype(np.uint32).view(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("params", ["signed", "unsigned", "offgrid"])
@pytest.mark.parametrize("entry", ["tensor_shifted", "tensor_unshifted", "lastaxis", "rows"])
def test_grid_strided_float32_patterns_vs_oracle(lib, entry, params):
    from oracle import mctq_oracle as O
    from mct_quantizers_amd.hip import native
    xd, x = _sweep_device(), _sweep_host()
    assert (SWEEP_N - 1) * 251 < 1 << 32 <= SWEEP_N * 251
    assert np.array_equal(xd[::65537].view(torch.int32).cpu().numpy(), x[::65537].view(np.int32))
    if entry.startswith("tensor"):
        shifted = entry == "tensor_shifted"
        lo, hi, step = (v[0] for v in _sweep_params(params, 1))
        y = torch.full_like(xd, SENTINEL)
        rc = lib.mctq_grid_per_tensor_f32(xd.data_ptr(), y.data_ptr(), SWEEP_N, float(lo), float(hi), float(step), int(shifted),
                                          _stream())
        assert rc == 0, lib.mctq_last_error()
        assert _route(native.last_launch()) == "flat_kernel<"
        ok, why = _same(y.cpu().numpy(), O.export_grid(x, lo, hi, step, None, shifted))
        assert ok, f"{entry} {params}: {why}"
        return
    if entry == "lastaxis":
        shape, route = (SWEEP_N // 8, 8, 1), "lastaxis_kernel<"
    else:
        inner = SWEEP_N // 16                          # whole rows only
        shape, route = (4, 4, inner), "rows_kernel<"
        assert inner % 4 == 0
    n = shape[0] * shape[1] * shape[2]
    lo, hi, step = _sweep_params(params, shape[1])
    tabs = [_table(v, 0) for v in (lo, hi, step)]
    xs = x[:n].reshape(shape)
    for shifted in (0, 1):
        y = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
        rc = lib.mctq_grid_per_channel_f32(xd.data_ptr(), y.data_ptr(), *shape, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                           tabs[2].data_ptr(), shifted, _stream())
        assert rc == 0, lib.mctq_last_error()
        assert _route(native.last_launch()) == route, native.last_launch()
        ok, why = _same(y.cpu().numpy(), O.export_grid(xs, lo, hi, step, 1, bool(shifted)))
        assert ok, f"{entry} {params} shifted={shifted}: {why}"
