"""The float-output affine fake-quant kernels on every launch route and at edge values: mctq_fq_per_tensor, mctq_fq_per_channel
and mctq_fq_per_tensor_tqp (AffineOp of csrc/mctq_kernels.hpp on flat_kernel, flat_paced_kernel, flat_scalar_kernel, rows_kernel,
rowsteps_kernel, rows_kernel_finetail, shortrows_kernel, gather_kernel, lastaxis_kernel and window_kernel), the batched lists
(mctq_fq_batched, mctq_fq_batch_pack + mctq_fq_batch_run) and the float64 entry points, through the raw C ABI.

The cases, the replay of the launchers that predicts every launch note, and the CPU proof of what the cases reach live in
tests/test_affine_route_cases.py.

Expected values: ``want`` there -- oracle.mctq_oracle.fake_quant_affine on the values as stored with every NaN replaced by -inf
(+inf -> qmax, -inf / NaN -> qmin, y = (q - z) s), narrowed to the storage type; numpy only.  Bar: the stored bit
pattern of EVERY element -- no mask, no tolerance; 16-bit outputs as stored, the sign of an underflowed zero and float16
subnormals included.  Every output sits in a frame of 0xA5 bytes, 64 guard bytes on each side, and starts as the bit complement of
its expected value, so a store outside the tensor and an element never written both show.  Every successful single-tensor call
advances mctq_launch_count by exactly one and leaves the launch note that the replay predicts for this device's CU count; a
mismatch means the launcher changed and the replay has to follow.
"""
import numpy as np
import pytest
import torch

import test_affine_route_cases as R
from test_gpu_codes8 import (DT_CODE, _channel_sets, _dev, _Frame, _rounds, _shifted, _store, _stream, _sweep, _sweep_host,
                             _table, lib)  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _device(lib):
    """The process's first GPU call creates its context (a few tenths of a second): here, not inside whichever test runs first."""
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


@pytest.fixture
def tuning(lib):
    """set(keys): the library's tuning state becomes the defaults with ``keys`` on top; afterwards every key is a default again."""
    from mct_quantizers_amd.hip import native

    def set_(keys):
        for k, v in R.tuned(**keys).items():
            native.set_tuning(k, v)

    set_({})
    yield set_
    set_({})


def _framed(want_bits, yoff_bytes=0):
    return _Frame(inside=(~want_bits).view(np.uint8), yoff=yoff_bytes)


def _compare(fr, want_bits, x_np, what):
    got = fr.result(what).view(want_bits.dtype)
    assert got.shape == want_bits.shape, f"{what}: {got.shape} elements, expected {want_bits.shape}"
    if np.array_equal(got, want_bits):
        return got
    bad = np.flatnonzero(got != want_bits)
    i = int(bad[0])
    unwritten = int((got[bad] == ~want_bits[bad]).sum())
    raise AssertionError(f"{what}: {bad.size} of {want_bits.size} elements differ ({unwritten} of them never written), first at "
                         f"{i}: x={np.asarray(x_np).reshape(-1)[i]!r} got {int(got[i]):#x} want {int(want_bits[i]):#x}")


def _call(lib, entry, xd, fr, shape, dt_code, scales, zps, qmin, qmax, tab_off=(0, 0)):
    """One raw call.  ``zps`` None: no zero-point table (per channel).  Returns (rc, what keeps the tables alive)."""
    outer, C, inner = shape
    if entry == "tensor":
        return lib.mctq_fq_per_tensor(xd.data_ptr(), fr.ptr(), inner, dt_code, float(scales[0]), int(zps[0]), qmin, qmax,
                                      _stream()), None
    s_d = _table(scales, np.float32, tab_off[0])
    z_d = None if zps is None else _table(zps, np.int32, tab_off[1])
    if entry == "tqp":
        return lib.mctq_fq_per_tensor_tqp(xd.data_ptr(), fr.ptr(), inner, dt_code, s_d.data_ptr(), z_d.data_ptr(), qmin, qmax,
                                          _stream()), (s_d, z_d)
    return lib.mctq_fq_per_channel(xd.data_ptr(), fr.ptr(), outer, C, inner, dt_code, s_d.data_ptr(),
                                   None if z_d is None else z_d.data_ptr(), qmin, qmax, _stream()), (s_d, z_d)


def _run(lib, entry, xd, x_np, want32, dt, shape, scales, zps, qmin, qmax, note, what, yoff=0, tab_off=(0, 0)):
    """One call on the framed output: one launch counted, the whole note, every bit.  Returns the stored bit patterns."""
    from mct_quantizers_amd.hip import native
    assert not np.isnan(want32).any(), f"{what}: the expected values hold a NaN"
    want_bits = R.stored_bits(want32, dt)
    fr = _framed(want_bits, yoff * R.ESIZE[dt])
    count = native.launch_count()
    rc, keep = _call(lib, entry, xd, fr, shape, DT_CODE[dt], scales, zps, qmin, qmax, tab_off)
    assert rc == 0, lib.mctq_last_error()
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: the library took {text}, the replay of its launchers says {note}"
    got = _compare(fr, want_bits, x_np, f"{what} [{text}]")
    del keep
    return got


def _want_channels(x, scales, zps, qmin, qmax, dt):
    z = np.zeros(len(scales), np.int32) if zps is None else np.asarray(zps, np.int32)
    return R.want(x, np.asarray(scales, np.float32), z, qmin, qmax, 1, dt)


# ------------------------------------------------------------------------------------------------
# (a) value sweeps through every route: all 65 536 patterns of a 16-bit type, every float32 exponent x edge mantissas with the
#     ties and tie neighbours of every grid (_sweep of test_gpu_codes8.py), laid out so that every channel sees the whole vector.
#     Tables: one whose scales recip_exact takes in every wave, SIGNED / UNSIGNED of test_gpu_codes8.py, and SIGNED with a scale
#     above 2^100 (the IEEE-division fallback of the lane-owned reciprocals).
# ------------------------------------------------------------------------------------------------

def _sweep_tensor(dt, idx, xoff):
    """The sweep vector gathered by ``idx`` (-1: a zero) on the device, bit for bit."""
    xd1, x1 = _sweep(dt)
    L = x1.size
    src = torch.cat([xd1, torch.zeros(1, dtype=xd1.dtype, device="cuda")])
    flat = np.ascontiguousarray(np.where(idx < 0, L, idx).reshape(-1))
    xd = _shifted(src[_dev(flat.astype(np.int64))], xoff)
    bits = np.concatenate([_sweep_host(dt)[0], np.zeros(1, _sweep_host(dt)[0].dtype)])
    ints = torch.int32 if dt == "float32" else torch.int16
    assert np.array_equal(xd.view(ints).cpu().numpy().view(bits.dtype), bits[flat])       # NaN payloads and all
    return xd, flat


def _tensor_sweep(lib, tuning, route, dt, params):
    cus = _cus()
    entry, shape, idx, xoff, has_zp, keys = R.sweep_layout(route, dt, cus)
    assert entry == "tensor"
    tuning(keys)
    xd, flat = _sweep_tensor(dt, idx, xoff)
    x1 = np.concatenate([_sweep(dt)[1], np.zeros(1, np.float32)])
    note = R.expected_note(entry, dt, *shape, x_aligned=xoff == 0, cus=cus, tuning=keys)
    assert note.startswith(R.KERNEL[route]), note
    for scale, zp, qmin, qmax in params:
        w1 = R.want(x1, np.float32(scale), zp, qmin, qmax, None, dt)
        _run(lib, entry, xd, x1[flat], w1[flat], dt, shape, [scale], [zp], qmin, qmax, note, f"{route} {dt} {(scale, zp, qmin, qmax)}")


# flat_paced_kernel starts at 2048 cus lane vectors (2 ... 4 Mi elements here): one parameter pair per test
@pytest.mark.parametrize("p", range(len(R.ALL_PARAMS)), ids=[f"{p[0]:g},{p[1]},{p[2]},{p[3]}" for p in R.ALL_PARAMS])
@pytest.mark.parametrize("dt", R.DTYPES)
def test_value_sweep_paced(lib, tuning, dt, p):
    _tensor_sweep(lib, tuning, "flat_paced", dt, R.ALL_PARAMS[p:p + 1])


@pytest.mark.parametrize("route,dt", [rd for rd in R.sweep_routes() if rd[0] != "flat_paced"], ids=lambda v: str(v))
def test_value_sweep(lib, tuning, route, dt):
    if R.SWEEPS[route][0] == "tensor":
        return _tensor_sweep(lib, tuning, route, dt, R.ALL_PARAMS)
    cus = _cus()
    entry, shape, idx, xoff, has_zp, keys = R.sweep_layout(route, dt, cus)
    outer, C, inner = shape
    tuning(keys)
    xd, flat = _sweep_tensor(dt, idx, xoff)
    x1 = np.concatenate([_sweep(dt)[1], np.zeros(1, np.float32)])
    x_np = x1[flat]
    note = R.expected_note(entry, dt, outer, C, inner, x_aligned=xoff == 0, has_zp=has_zp, cus=cus, tuning=keys)
    assert note.startswith(R.KERNEL[route.split("-")[0]]), note
    chan = np.ascontiguousarray(np.broadcast_to(np.arange(C)[None, :, None], shape)).reshape(-1)
    for name, sets in R.TABLES.items():
        P = len(sets)                                         # channel c has parameter set c % P (_channel_sets)
        scales, zps, domains = _channel_sets(sets, C)
        if not has_zp:
            zps = None
        for qmin, qmax in domains:
            # the oracle on [P, L + 1]: row j is the whole vector under parameter set j; element [o, c, i] picks its value
            per_set = R.want(np.broadcast_to(x1, (P, x1.size)), np.asarray(scales[:P], np.float32),
                             np.zeros(P, np.int32) if zps is None else np.asarray(zps[:P], np.int32), qmin, qmax, 0, dt)
            _run(lib, entry, xd, x_np, per_set[chan % P, flat], dt, shape, scales, zps, qmin, qmax, note,
                 f"{route} {dt} {shape} table {name} [{qmin}, {qmax}]")


# ------------------------------------------------------------------------------------------------
# (b) launch geometry: every case of the table, inputs dense in the ties and clamp edges of the element's own channel with NaN,
#     +-inf, +-0.0, a denormal and +-3e38 on one element in 16 (_edge_values of test_gpu_codes8.py) and planted
#     (geometry_launches of tests/test_affine_route_cases.py)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(R.cases(256))), ids=[c.id for c in R.cases(256)])
def test_geometry(lib, tuning, k):
    cus = _cus()
    c = R.cases(cus)[k]
    shape = (c.outer, c.C, c.inner)
    n = c.outer * c.C * c.inner
    tuning(c.tuning)
    note = R.case_note(c, cus)
    assert note.startswith(R.KERNEL[c.route]), f"{c.id}: the table files it under {c.route}, the replay says {note}"
    launches = 0
    for x32, scales, zps, qmin, qmax in R.geometry_launches(c, k):
        xd, x = _store(x32.reshape(-1), c.dt, c.xoff)
        x = x.reshape(shape)
        want32 = R.case_want(c, x, scales, zps, qmin, qmax)
        _run(lib, c.entry, xd, x, want32, c.dt, shape, scales, zps, qmin, qmax, note, f"{c.id} {shape}", c.yoff, c.tab_off)
        launches += 1
    assert launches == _rounds(n)


# ------------------------------------------------------------------------------------------------
# (c) batched lists: an item for every branch of batched_tile in each storage type, per-tensor items and zero-point tables among
#     them, through the kernel-argument launch and through the packed table; every output framed, equal to the oracle and to the
#     single-tensor entry point's bits
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["kernarg", "table"])
def test_batched_lists(lib, tuning, source):
    from mct_quantizers_amd.hip import native
    tuning({})
    cus = _cus()
    rng = np.random.default_rng(77)
    specs = R.batch_specs()
    arr = (native.FqItem * len(specs))()
    held = []
    for k, (it, (dt, (shape, has_zp, per_tensor))) in enumerate(zip(arr, specs)):
        outer, C, inner = shape
        x32, scales, zps, qmin, qmax = R.batch_launch(rng, k, shape, has_zp)
        xd, x = _store(x32.reshape(-1), dt)
        x = x.reshape(shape)
        want32 = _want_channels(x, scales, zps, qmin, qmax, dt)
        assert not np.isnan(want32).any()
        want_bits = R.stored_bits(want32, dt)
        fr = _framed(want_bits)
        s_d = _table(scales, np.float32)
        z_d = None if zps is None else _table(zps, np.int32)
        it.x, it.y, it.outer, it.channels, it.inner = xd.data_ptr(), fr.ptr(), outer, C, inner
        it.scales, it.zero_points = s_d.data_ptr(), None if z_d is None else z_d.data_ptr()
        it.quant_min, it.quant_max, it.dtype = qmin, qmax, DT_CODE[dt]
        it.flags = native.FQ_ITEM_PER_TENSOR if per_tensor else 0
        held.append((dt, shape, per_tensor, xd, x, fr, want32, want_bits, scales, zps, qmin, qmax, s_d, z_d))
    count = native.launch_count()
    if source == "kernarg":
        assert lib.mctq_fq_batched(arr, len(specs), _stream()) == 0, lib.mctq_last_error()
        last = "batched_kernel<AffineOp,in2B,out2B,U=4,NT=2>"
    else:
        need = lib.mctq_fq_batch_pack(arr, len(specs), None, 0)
        assert need > 0, lib.mctq_last_error()
        host = np.zeros(need, np.uint8)
        assert lib.mctq_fq_batch_pack(arr, len(specs), host.ctypes.data, need) == need
        dev = _dev(host)
        assert lib.mctq_fq_batch_run(host.ctypes.data, dev.data_ptr(), _stream()) == 0, lib.mctq_last_error()
        last = "batched_kernel<table><AffineOp,in2B,out2B,U=4,NT=2>"
    # one grid per storage type (float32, float16, bfloat16 in that order), nothing launched on its own
    assert native.launch_count() == count + 3 and native.last_launch() == last, (native.launch_count() - count, native.last_launch())
    for dt, shape, per_tensor, xd, x, fr, want32, want_bits, scales, zps, qmin, qmax, s_d, z_d in held:
        what = f"{source} {dt} {shape}"
        _compare(fr, want_bits, x, what)
        # the same operands through the single-tensor entry point the item stands for: tensor qparams for a per-tensor item with
        # a zero-point pointer, mctq_fq_per_tensor for one without, mctq_fq_per_channel otherwise -- one launch, its note, its bits
        entry = "channel" if not per_tensor else "tqp" if zps is not None else "tensor"
        note = R.expected_note(entry, dt, *shape, has_zp=zps is not None, cus=cus)
        z1 = np.zeros(1, np.int32) if entry == "tensor" else zps
        _run(lib, entry, xd, x, want32, dt, shape, scales, z1, qmin, qmax, note, f"{what}: the single-tensor entry point ({entry})")


# ------------------------------------------------------------------------------------------------
# (d) float64: fq64_kernel<VEC> behind the three entry points (csrc/mctq_f64.hip).  A lane vector is two doubles, a tile 2048
#     (1024 when x or y is 8 bytes off a 16-byte boundary); odd rows make a pair straddle two rows and the channel wrap.  These
#     launches leave no launch note: results only.
# ------------------------------------------------------------------------------------------------

def _f64_inputs(rng, shape, scales, zps, qmin, qmax):
    C = shape[1]
    s = np.asarray(scales, np.float32).reshape(1, C, 1)
    z = (np.zeros(C) if zps is None else np.asarray(zps, np.float64)).reshape(1, C, 1)
    inv = (np.float32(1.0) / s).astype(np.float64)
    k = rng.integers(qmin - 2, qmax + 3, size=shape).astype(np.float64) - z
    with np.errstate(all="ignore"):
        tie = (k + 0.5) / inv                                 # an exact tie of the double product where 1 / s is a power of two
        x = rng.standard_normal(shape) * s.astype(np.float64) * 0.4 * (qmax - qmin)
        kind = rng.integers(0, 8, size=shape)
        x = np.where(kind == 0, tie, x)
        x = np.where(kind == 1, np.nextafter(tie, -np.inf), x)
        x = np.where(kind == 2, np.nextafter(tie, np.inf), x)
        x = np.where(kind == 3, k / inv, x)
    special = np.asarray([np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0, 5e-324, -1e-310], dtype=np.float64)
    pick = rng.integers(0, 12 * special.size, size=shape)
    return np.where(pick < special.size, special[pick % special.size], x).astype(np.float64)


def _run64(lib, entry, x, shape, scales, zps, qmin, qmax, xoff, yoff, what):
    from mct_quantizers_amd.hip import native
    axis = 1 if entry == "channel" else None
    z = np.zeros(len(scales), np.int32) if zps is None else np.asarray(zps, np.int32)
    want_bits = np.ascontiguousarray(R.want64(x, np.asarray(scales, np.float32), z, qmin, qmax, axis)).reshape(-1).view(np.uint64)
    assert not np.isnan(want_bits.view(np.float64)).any()
    xd = _shifted(_dev(x.reshape(-1)), xoff)
    assert xd.dtype == torch.float64 and np.array_equal(xd.cpu().numpy().view(np.uint64), x.reshape(-1).view(np.uint64))
    fr = _framed(want_bits, 8 * yoff)
    rc, keep = _call(lib, entry, xd, fr, shape, native.DT_F64, scales, zps, qmin, qmax)
    assert rc == 0, lib.mctq_last_error()
    _compare(fr, want_bits, x, what)
    del keep


@pytest.mark.parametrize("xoff,yoff", [(0, 0), (1, 0), (0, 1)], ids=["aligned", "x+8", "y+8"])
@pytest.mark.parametrize("entry", ["tensor", "tqp", "channel"])
def test_float64(lib, tuning, entry, xoff, yoff):
    tuning({})
    rng = np.random.default_rng([xoff, yoff, len(entry)])
    # (3, 5, 7): one partial tile, 105 elements (an odd count: a lone last element); (13, 5, 33): 2145 elements, a second,
    # partial tile of either width; odd rows: pairs that straddle two rows, the wrap from channel 4 to 0
    for shape in ((3, 5, 7), (13, 5, 33)):
        if entry != "channel":
            shape = (1, 1, shape[0] * shape[1] * shape[2])
        C = shape[1]
        for qmin, qmax, with_zp in ((-128, 127, True), (0, 255, True), (-8, 7, False)):
            if entry != "channel" and not with_zp:
                continue                                      # both per-tensor forms carry a zero point
            scales = rng.uniform(0.01, 0.9, size=C).astype(np.float32)
            scales[0] = np.float32(0.25)                      # 1 / s = 4: (k + 1/2) / 4 is an exact tie of the double product
            zps = rng.integers(qmin, qmax + 1, size=C).astype(np.int32) if with_zp else None
            x = _f64_inputs(rng, shape, scales, zps, qmin, qmax)
            z0 = 0 if zps is None else int(zps[0])
            x[0, 0, :3] = [(qmin + 1 - z0 + 0.5) * 0.25, np.nan, np.inf]     # channel 0: an exact tie inside the domain
            sel = x[:, 0, :]
            assert np.isnan(sel).any() and np.isinf(sel).any()
            frac = np.abs(sel[np.isfinite(sel)] * 4.0) % 1.0
            assert (frac == 0.5).any()                        # exact ties went in
            _run64(lib, entry, x, shape, scales, zps, qmin, qmax, xoff, yoff,
                   f"float64 {entry} {shape} x+{8 * xoff} y+{8 * yoff} [{qmin}, {qmax}]{'' if with_zp else ' NULL zero points'}")
