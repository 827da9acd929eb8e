"""The float-output LUT fake-quant kernels on every launch route and at edge values: mctq_lutt_* (LutTableOp), mctq_lut_*
(LutOp<registers>, LutOp<lds>) and mctq_luts_* (LutStepsOp, LutCellsOp) of csrc/mctq_kernels.hpp on flat_kernel,
flat_scalar_kernel, rows_kernel, lastaxis_kernel and window_kernel, the batched LUT launch (mctq_lutt_batch_pack +
mctq_lutt_batch_run) and the float64 entry points, through the raw C ABI.

The cases, the replay of the launchers that predicts every launch note, and the CPU proof of what the cases reach live in
tests/test_lut_route_cases.py.

Expected values: oracle.mctq_oracle.lut_quantize on the values as stored, widened (lut_quantize_f64 for float64 input); numpy
only.  Bar: the bit pattern of EVERY float32 output -- no mask, no tolerance; NaN, infinities and signed zeros in, whatever the
oracle gives out.  Every output sits in a frame of 0xA5 bytes, 64 guard bytes on each side, and starts as the bit complement of
its expected value, so a store outside the tensor and an element never written both show.  Every successful single-tensor call
advances mctq_launch_count by exactly one and leaves the launch note that the replay predicts for this device's CU count; a
refused call returns MCTQ_E_ARG, launches nothing and leaves the frame untouched.
"""
import numpy as np
import pytest
import torch

import test_lut_route_cases as R
from test_gpu_lut_index import _cus, _dev, _Frame, _shifted, _store, _stream, lib  # noqa: F401  (lib: the module-scoped fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _device(lib):
    """The process's first GPU call creates its context: here, not inside whichever test runs first."""
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


@pytest.fixture
def tuning(lib):
    """set(keys): the library's tuning state becomes the defaults with ``keys`` on top; afterwards every key is a default again."""
    from mct_quantizers_amd.hip import native

    def set_(keys):
        for k, v in R.tuned(**keys).items():
            native.set_tuning(k, v)

    try:
        set_({})
        yield set_
    finally:
        set_({})


_BOOKS = {}


def _book(name):
    """(device pointer holder, count) of a book: the decision table, the codebook or the threshold list."""
    if name not in _BOOKS:
        b = R.BOOKS[name]
        host = R.value_table(name) if b.op == "table" else np.asarray(b.lut, dtype=F32) if b.op in ("registers", "lds") \
            else R.steps_list(name)
        _BOOKS[name] = (_dev(host), R.book_count(b))
    return _BOOKS[name]


def _entry(lib, b, kind):
    stem = {"table": "mctq_lutt", "registers": "mctq_lut", "lds": "mctq_lut", "steps": "mctq_luts", "cells": "mctq_luts"}[b.op]
    return getattr(lib, f"{stem}_per_{kind}")


def _call(lib, b, dt, kind, xd, y_ptr, shape, thr, eps, step=False, toff=0, div=None):
    """One raw call -> (rc, what keeps the tables alive).  Per tensor: thr a number (``div``: the divisor, else as the classes
    form it); per channel: float32 [C]."""
    book_d, count = _book(b.name)
    mult, cmin, cmax = R.domain(b)
    if kind == "tensor":
        if div is None:
            div = float(R.tensor_divisor(thr, eps, dt if step else "float32"))
        return _entry(lib, b, "tensor")(xd.data_ptr(), y_ptr, int(np.prod(shape)), R.DT_CODE[dt], R.DT_CODE[dt] if step else 0,
                                        div, float(F32(thr)), book_d.data_ptr(), count, mult, cmin, cmax, _stream()), None
    outer, C, inner = shape
    t_d = _shifted(_dev(np.asarray(thr, dtype=F32)), toff)
    assert t_d.data_ptr() % 16 == 4 * toff
    return _entry(lib, b, "channel")(xd.data_ptr(), y_ptr, outer, C, inner, R.DT_CODE[dt], t_d.data_ptr(), eps, book_d.data_ptr(),
                                     count, mult, cmin, cmax, _stream()), t_d


def _compare(fr, want, x, what):
    want_w = np.ascontiguousarray(want, dtype=F32).reshape(-1).view(np.uint32)
    got = fr.result(what).view(np.uint32)
    assert got.shape == want_w.shape, f"{what}: {got.shape} elements, expected {want_w.shape}"
    if np.array_equal(got, want_w):
        return
    bad = np.flatnonzero(got != want_w)
    i = int(bad[0])
    unwritten = int((got[bad] == ~want_w[bad]).sum())
    raise AssertionError(f"{what}: {bad.size} of {want_w.size} elements differ ({unwritten} of them never written), first at {i}: "
                         f"x={np.asarray(x).reshape(-1)[i]!r} got {got[i:i + 1].view(F32)[0]!r} ({int(got[i]):#x}) "
                         f"want {want_w[i:i + 1].view(F32)[0]!r} ({int(want_w[i]):#x})")


def _run(lib, b, dt, kind, x, want, thr, eps, note, what, xoff=0, yoff=0, toff=0, step=False, div=None):
    """One call on the framed output: one launch counted, the whole note, every bit."""
    from mct_quantizers_amd.hip import native
    x = np.asarray(x, dtype=F32)
    xd = _store(x, dt, xoff)
    fr = _Frame(np.ascontiguousarray(want, dtype=F32), yoff=4 * yoff)
    count = native.launch_count()
    rc, keep = _call(lib, b, dt, kind, xd, fr.ptr(), x.shape, thr, eps, step, toff, div)
    assert rc == 0, (what, lib.mctq_last_error())
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    assert text == note, f"{what}: the library took {text}, the replay of its launchers says {note}"
    _compare(fr, want, x, f"{what} [{text}]")
    del keep


# ------------------------------------------------------------------------------------------------
# (a) value sweeps through every route, per book and storage type.  Per tensor: the four divisors of the index cases (1.0 and
#     1.7 divide fast, 2^70 and 2^-70 by IEEE) and a zero threshold (0 / 0, x / 0).  Per channel: every channel holds the sweep of
#     its OWN divisor and the table mixes 1.7, 2^70, 2^-70, 1.0 and 0 with eps = 0; the "waves" layout gives window_kernel's
#     ballot waves that are all fast, all IEEE and mixed, each with NaN, +inf and -inf in it.
# ------------------------------------------------------------------------------------------------

SWEEP_IDS = [(route, name, dt) for route in R.SWEEPS for name in R.sweep_books(route) for dt in R.DTYPES]


@pytest.mark.parametrize("route,name,dt", SWEEP_IDS, ids=["-".join(s) for s in SWEEP_IDS])
def test_value_sweep(lib, tuning, route, name, dt):
    tuning({})
    cus = _cus()
    b = R.BOOKS[name]
    kind, layout, xoff = R.SWEEPS[route]
    if kind == "tensor":
        for dname, thr, eps in R.TENSOR_DIVISORS:
            for step in ((False, True) if dt != "float32" and name in R.STEP_BOOKS and 0 < thr < 2 else (False,)):
                x, want, div, mul = R.tensor_sweep(name, dname, dt, step)
                note, _ = R.route(b, dt, "tensor", x.shape, xoff == 0, cus=cus)
                assert note.startswith(R.KERNEL[route]), note
                _run(lib, b, dt, "tensor", x, want, thr, eps, note, f"{route} {name} {dt} d={dname}{' step_round' if step else ''}",
                     xoff=xoff, step=step, div=div)
        return
    shape, x, want, thr = R.sweep_case(route, name, dt)
    note, info = R.route(b, dt, "channel", shape, xoff == 0, cus=cus)
    _run(lib, b, dt, "channel", x, want, thr, 0.0, note, f"{route} {name} {dt} {shape}", xoff=xoff)


# ------------------------------------------------------------------------------------------------
# (b) launch geometry: every case of the table
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(R.cases(256))), ids=[c.id for c in R.cases(256)])
def test_geometry(lib, tuning, k):
    cus = _cus()
    c = R.cases(cus)[k]
    tuning(c.tuning)
    note, info = R.case_route(c, cus)
    assert note is not None and note.startswith(R.KERNEL[c.route]), f"{c.id}: the table files it under {c.route}, the replay says {note}"
    x, thr, eps, want = R.geometry_inputs(c, cus)
    _run(lib, R.BOOKS[c.book], c.dt, c.kind, x, want, thr, eps, note, c.id, c.xoff, c.yoff, c.toff, c.step)


def test_quantizer_class_with_a_2048_centre_codebook_on_the_last_axis(lib, tuning):
    """What used to raise "parameter window exceeds 64 KiB of LDS": 1023 channels on the last axis (no multiple of four, so not the
    last-axis route) under the 49 184-byte cells book.  The class computes, through the list alone."""
    import warnings
    import mct_quantizers_amd as mq
    from mct_quantizers_amd.hip import native
    tuning({})
    b = R.BOOKS["c2048"]
    C = 1023
    rng = np.random.default_rng(1023)
    thr = rng.uniform(0.5, 3.0, size=C).astype(F32)
    x = (rng.standard_normal((3, C)) * 1.2).astype(F32)
    x[0, :3] = [np.nan, np.inf, -np.inf]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = mq.pytorch_quantizers.WeightsLUTSymmetricInferableQuantizer(11, b.lut, [float(t) for t in thr], True, 1, 2,
                                                                        lut_values_bitwidth=b.bits)
    got = q(_dev(x))
    text = native.last_launch()
    assert text == "window_kernel<vector><LutStepsOp,in4B,out4B,U=4,NT=1>", text
    want = R._oracle(x.reshape(3, C, 1), b, thr, 1e-8, per_channel=True).reshape(3, C)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# (c) refusals: MCTQ_E_ARG, nothing launched, the frame untouched
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", R.DTYPES)
def test_refused_calls_launch_nothing(lib, tuning, dt):
    from mct_quantizers_amd.hip import native
    tuning({})
    x = R.narrow(np.linspace(-2, 2, 60, dtype=F32), dt).reshape(3, 5, 4)
    xd = _store(x, dt)
    t_d = _dev(np.full(5, 1.5, F32))
    for name, bad_count, word in (("t8s", 510, b"entries"), ("s64", 131, b"steps size"), ("c256", 1540, b"steps size"), ("r16", 0, b"n_lut"),
                                  ("l17", 4097, b"n_lut")):
        b = R.BOOKS[name]
        book_d, _ = _book(name)
        mult, cmin, cmax = R.domain(b)
        for kind in ("tensor", "channel"):
            fr = _Frame(nbytes=4 * x.size)
            count = native.launch_count()
            if kind == "tensor":
                rc = _entry(lib, b, kind)(xd.data_ptr(), fr.ptr(), x.size, R.DT_CODE[dt], 0, 1.5, 1.5, book_d.data_ptr(), bad_count,
                                          mult, cmin, cmax, _stream())
            else:
                rc = _entry(lib, b, kind)(xd.data_ptr(), fr.ptr(), 3, 5, 4, R.DT_CODE[dt], t_d.data_ptr(), 1e-8, book_d.data_ptr(),
                                          bad_count, mult, cmin, cmax, _stream())
            what = f"{name} {kind} {dt} count {bad_count}"
            assert rc == native.MCTQ_E_ARG and word in lib.mctq_last_error(), (what, rc, lib.mctq_last_error())
            assert native.launch_count() == count, what
            fr.untouched(what)
        # a mult that is no power of two
        fr = _Frame(nbytes=4 * x.size)
        count = native.launch_count()
        rc = _entry(lib, b, "tensor")(xd.data_ptr(), fr.ptr(), x.size, R.DT_CODE[dt], 0, 1.5, 1.5, book_d.data_ptr(), R.book_count(b),
                                      3.0, cmin, cmax, _stream())
        assert rc == native.MCTQ_E_ARG and native.launch_count() == count, (name, rc)
        fr.untouched(name)


# ------------------------------------------------------------------------------------------------
# (d) the table-op geometry cases once more as ONE batched LUT launch (a grid per storage type); the same expected bits
# ------------------------------------------------------------------------------------------------

def test_table_op_cases_as_one_batched_launch(lib, tuning):
    from mct_quantizers_amd.hip import native
    tuning({})
    cus = _cus()
    picked = [c for c in R.cases(cus) if c.op == "table" and not (c.xoff or c.yoff or c.toff or c.tuning or c.step)
              and "second-pass" not in c.id]
    assert {c.dt for c in picked} == set(R.DTYPES) and {c.route for c in picked} == {"flat", "rows", "lastaxis", "window"}
    arr = (native.LutItem * len(picked))()
    held = []
    for it, c in zip(arr, picked):
        b = R.BOOKS[c.book]
        x, thr, eps, want = R.geometry_inputs(c, cus)
        xd = _store(x, c.dt)
        fr = _Frame(np.ascontiguousarray(want, dtype=F32))
        book_d, entries = _book(c.book)
        mult, cmin, cmax = R.domain(b)
        it.x, it.y, it.table, it.entries = xd.data_ptr(), fr.ptr(), book_d.data_ptr(), entries
        it.mult, it.clip_min, it.clip_max, it.dtype, it.step_round = mult, cmin, cmax, R.DT_CODE[c.dt], 0
        if c.kind == "tensor":
            it.outer, it.channels, it.inner, it.thresholds = 1, 1, x.size, None
            it.eps, it.thr_div, it.thr_mul = 0.0, float(R.tensor_divisor(thr, eps)), float(F32(thr))
            t_d = None
        else:
            t_d = _dev(thr)
            it.outer, it.channels, it.inner = c.shape
            it.thresholds, it.eps, it.thr_div, it.thr_mul = t_d.data_ptr(), eps, 0.0, 0.0
        held.append((c, x, want, xd, fr, t_d))
    need = lib.mctq_lutt_batch_pack(arr, len(picked), None, 0)
    assert need > 0, lib.mctq_last_error()
    host = np.zeros(need, np.uint8)
    assert lib.mctq_lutt_batch_pack(arr, len(picked), host.ctypes.data, need) == need
    dev = _dev(host)
    count = native.launch_count()
    assert lib.mctq_lutt_batch_run(host.ctypes.data, dev.data_ptr(), _stream()) == 0, lib.mctq_last_error()
    assert native.launch_count() == count + 3 and "batched_lut_kernel<table>" in native.last_launch(), \
        (native.launch_count() - count, native.last_launch())
    for c, x, want, xd, fr, t_d in held:
        _compare(fr, want, x, f"batched {c.id}")


# ------------------------------------------------------------------------------------------------
# (e) float64 input: lut64_kernel (the literal scan in double: mctq_lut_per_tensor_f64 and the float64 branch of
#     mctq_lut_per_channel; no launch note) and lut64_steps_kernel<VEC> (mctq_luts_per_tensor_f64, mctq_luts_per_channel_f64)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xoff", [0, 1], ids=["aligned", "x+8"])
@pytest.mark.parametrize("name", R.F64_BOOKS)
def test_float64(lib, tuning, name, xoff):
    from mct_quantizers_amd.hip import native
    tuning({})
    b = R.BOOKS[name]
    mult, cmin, cmax = R.domain(b)
    lut_d = _dev(np.asarray(b.lut, dtype=F32))
    blob = native.build_lut_steps_f64(b.lut, mult, cmin, cmax)
    assert blob is not None
    blob_d, P = _dev(blob[0]), blob[1]
    for shape in R.F64_SHAPES:
        x, thr, want = R.f64_inputs(name, shape)
        xd = _shifted(_dev(x.reshape(-1)), xoff)
        assert xd.dtype == torch.float64 and np.array_equal(xd.cpu().numpy().view(np.uint64), x.reshape(-1).view(np.uint64))
        for form in ("literal", "steps"):
            what = f"float64 {form} {name} {shape} x+{8 * xoff}"
            fr = _Frame(np.ascontiguousarray(want, dtype=F32))
            count = native.launch_count()
            if len(shape) == 1:
                div, mul = float(thr) + 1e-8, float(F32(thr))
                if form == "literal":
                    rc = lib.mctq_lut_per_tensor_f64(xd.data_ptr(), fr.ptr(), x.size, div, mul, lut_d.data_ptr(), len(b.lut), mult, cmin,
                                                     cmax, _stream())
                else:
                    rc = lib.mctq_luts_per_tensor_f64(xd.data_ptr(), fr.ptr(), x.size, div, mul, blob_d.data_ptr(), P, mult, cmin, cmax,
                                                      _stream())
                t_d = None
            else:
                t_d = _dev(thr)
                if form == "literal":
                    rc = lib.mctq_lut_per_channel(xd.data_ptr(), fr.ptr(), *shape, native.DT_F64, t_d.data_ptr(), 1e-8, lut_d.data_ptr(),
                                                  len(b.lut), mult, cmin, cmax, _stream())
                else:
                    rc = lib.mctq_luts_per_channel_f64(xd.data_ptr(), fr.ptr(), *shape, t_d.data_ptr(), 1e-8, blob_d.data_ptr(), P, mult,
                                                       cmin, cmax, _stream())
            assert rc == 0, (what, lib.mctq_last_error())
            if form == "steps":                                 # (the literal launcher leaves no note: results and frame only)
                assert native.launch_count() == count + 1, what
                assert native.last_launch() == "lut64_steps_kernel<LutSteps64,in8B,out4B,U=4,NT=1>", native.last_launch()
            _compare(fr, want, x, what)
            del t_d
