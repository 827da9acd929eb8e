"""The integer product on every tile order, K walk and edge value: mctq_qlinear_i8 / _codes / _zp / _res / _w4a8 / _w4a8_zp /
_lut4a8 (csrc/mctq_qlinear.hip: qlinear_i8_kernel, qlinear_i8_lds_kernel, qgemm_i8_glds_kernel, qgemm_i8_wide_kernel,
qgemm_i8_pp_kernel) through the raw C ABI, on the cases of tests/test_qlinear_route_cases.py, which proves without a GPU what they
reach.

Expected values: oracle.mctq_oracle.qlinear_i8 (zp_oracle for the zero-point forms, consumers._cpu_epilogue on the exact int32
sums for the residual form); codes are fake_quant_affine(..., return_index=True) of that float32 value on the CPU, NaN ->
quant_min -- never the GPU's own float32 output.  Bar: equality of every bit or byte of every element, no mask, no tolerance.
Every output sits in the middle of a 0xA5 frame with 64 guard bytes on each side, which must keep their value; inside, every
byte starts as the complement of its expected value, so an unwritten element shows.  Every successful call advances
mctq_launch_count by exactly one and leaves the launch note the case predicts: the kernel, the code types, the form, and U = gm
for the tiled kernels / the rows-per-pass factor MT for the streams.  Every tuning key is put back to 0 in a ``finally``.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import test_qlinear_route_cases as C

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE = 0xA5
KEYS = ("ql_variant", "ql_band", "ql_rot", "ql_stagger")
LUT_BYTES = np.asarray(C.LUT16, np.int8).tobytes()
DEVICE_FIELDS = ("a", "w", "ws", "rowsum", "bias", "edge_bias", "zw", "a_rowsum", "residual", "packed")


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


@contextlib.contextmanager
def _tuning(lib, **keys):
    try:
        for key, value in keys.items():
            assert key in KEYS and lib.mctq_set_tuning(key.encode(), value) == 0, (key, value, lib.mctq_last_error())
        yield
    finally:
        for key in KEYS:
            lib.mctq_set_tuning(key.encode(), 0)


@functools.lru_cache(maxsize=8)
def _device(edge, M, N, K, u8, wkind):
    """The operands of one problem on the GPU (16-byte aligned: fresh allocations)."""
    p = (C.edge_problem if edge else C.problem)(M, N, K, u8, wkind)
    d = {k: torch.from_numpy(np.array(p[k])).cuda() for k in DEVICE_FIELDS if p.get(k) is not None}
    assert d["a"].data_ptr() % 16 == 0 and d["w"].data_ptr() % 16 == 0 and d.get("packed", d["w"]).data_ptr() % 16 == 0
    return p, d


class _Frame:
    """The output bytes in the middle of a 0xA5 frame; inside, the complement of the bytes expected."""

    def __init__(self, want):
        self.want = want
        self.nb = want.size
        self.buf = torch.full((self.nb + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + self.nb].copy_(torch.from_numpy(~want).cuda())
        assert self.ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def check(self, what, item):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        edge = np.concatenate([b[:GUARD], b[GUARD + self.nb:]])
        assert edge.size == 2 * GUARD and np.all(edge == GUARD_BYTE), f"{what}: wrote outside its {self.nb} bytes"
        got = b[GUARD:GUARD + self.nb]
        if np.array_equal(got, self.want):
            return
        bad = np.unique(np.flatnonzero(got != self.want) // item)
        i = int(bad[0])
        show = (lambda v: repr(v[item * i:item * i + item].view(np.float32)[0])) if item == 4 else (lambda v: int(v[i]))
        unwritten = int(np.sum(np.all((got == ~self.want).reshape(-1, item), axis=1)))
        raise AssertionError(f"{what}: {bad.size} of {self.nb // item} elements differ ({unwritten} never written), first at element "
                             f"{i}: got {show(got)} want {show(self.want)}")


def _launch(lib, p, d, form, out, want, note, what, bias="own"):
    """One call of the entry point of ``form`` on the framed output: the expected bytes, one launch, the note."""
    from mct_quantizers_amd.hip import native
    fr = _Frame(want)
    item = 4 if out is None else 1
    assert want.size == p["M"] * p["N"] * item
    bias_t = d.get("bias") if bias == "own" else d["edge_bias"] if bias == "edge" else None
    head = (d["a"].data_ptr(), native.CODE_U8 if p["u8"] else native.CODE_I8, p["za"], p["sa"])
    mid = (d["ws"].data_ptr(), d["rowsum"].data_ptr(), None if bias_t is None else bias_t.data_ptr())
    f5 = (-1, 1.0, 0, 0, 0) if out is None else (native.CODE_U8 if out[2] >= 0 else native.CODE_I8, out[0], out[1], out[2], out[3])
    tail = (p["M"], p["N"], p["K"], torch.cuda.current_stream().cuda_stream)
    count = native.launch_count()
    if form == "f32":
        assert out is None
        rc = lib.mctq_qlinear_i8(*head, d["w"].data_ptr(), *mid, fr.ptr(), *tail)
    elif form == "codes":
        rc = lib.mctq_qlinear_i8_codes(*head, d["w"].data_ptr(), *mid, fr.ptr(), *f5, *tail)
    elif form == "zp":
        rc = lib.mctq_qlinear_i8_zp(*head, d["w"].data_ptr(), *mid, fr.ptr(), *f5, d["zw"].data_ptr(), d["a_rowsum"].data_ptr(), *tail)
    elif form == "res":
        rc = lib.mctq_qlinear_i8_res(*head, d["w"].data_ptr(), *mid, d["residual"].data_ptr(), native.CODE_U8, C.R_FORM[0],
                                     C.R_FORM[1], 1, fr.ptr(), *f5, *tail)
    elif form == "w4":
        rc = lib.mctq_qlinear_w4a8(*head, d["packed"].data_ptr(), *mid, fr.ptr(), *f5, *tail)
    elif form == "w4zp":
        rc = lib.mctq_qlinear_w4a8_zp(*head, d["packed"].data_ptr(), *mid, fr.ptr(), *f5, d["zw"].data_ptr(),
                                      d["a_rowsum"].data_ptr(), *tail)
    else:
        assert form == "lut"
        rc = lib.mctq_qlinear_lut4a8(*head, d["packed"].data_ptr(), LUT_BYTES, *mid, fr.ptr(), *f5, *tail)
    assert rc == 0, f"{what}: {lib.mctq_last_error()}"
    text = native.last_launch()
    assert native.launch_count() == count + 1, f"{what}: {native.launch_count() - count} launches noted [{text}]"
    if note is not None:
        assert text == note, f"{what}: took {text}, expected {note}"
    fr.check(f"{what} [{text}]", item)
    return text


def _run(lib, M, N, K, u8, wkind, form, note, what):
    """A case of the shared random problems."""
    p, d = _device(False, M, N, K, u8, wkind)
    _, want = C.expected(M, N, K, u8, wkind, form)
    return _launch(lib, p, d, form, C.out_form(form, u8), want, note, f"{what} M={M} N={N} K={K} u8={u8} {form}")


def _form_note(name, u8, u, form):
    return C.note(name, u8, u, zp=form in ("zp", "w4zp"), tail=" res(u8) relu" if form == "res" else "")


# ------------------------------------------------------------------------------------------------
# 1. tile order
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", sorted(C.TILED))
def test_tile_order_of_the_tiled_kernels(lib, variant):
    """Grids of 3 x 8, 5 x 8 (remap) and 5 x 3 (none) tiles, ragged in M and N, under ql_band = 0, 1, 2, 3 and m_blocks + 5."""
    bm, bn = C.TILED[variant][:2]
    for (M, N, K, u8, band, form) in C.order_cases(variant):
        gm = C.tiled_gm(variant, -(-M // bm), -(-N // bn), band)[1]
        with _tuning(lib, ql_variant=variant, ql_band=band):
            _run(lib, M, N, K, u8, "i8", form, _form_note(C.tiled_name(variant), u8, gm, form), f"variant {variant} ql_band={band}")


@pytest.mark.parametrize("variant", sorted(C.WHOLE))
def test_tile_order_of_the_whole_tile_kernels(lib, variant):
    """Grids (m_blocks, n_blocks) = (6, 4), (5, 8), (5, 3), (3, 8), (4, 2), (4, 3) and (3, 3) of whole tiles at K = 256, the
    largest 1536 x 1024 and 1280 x 2048 for the 256 x 256 kernel: GM = 4 gives bands of 4 + 2, 4 + 1, 4 and a single band of 3,
    each with and without the remap."""
    bm, bn, name, u = C.WHOLE[variant]
    for (M, N, K, u8, form) in C.whole_cases(variant):
        with _tuning(lib, ql_variant=variant):
            _run(lib, M, N, K, u8, "i8", form, C.note(name, u8, u), f"variant {variant} grid {M // bm} x {N // bn}")


# ------------------------------------------------------------------------------------------------
# 2. K walk
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", range(len(C.KEY_SETTINGS)), ids=["keys0", "rot_band2", "stagger"])
@pytest.mark.parametrize("variant", sorted(C.TILED))
def test_k_walk_of_the_tiled_kernels(lib, variant, setting):
    """3 x 2 ragged tiles over every tail length, K below one step and 1 ... 8 K tiles; with the K rotation (bands of 2 + 1
    rows: every block of a band starts at another tile and wraps) and with the staggered copy."""
    keys = C.KEY_SETTINGS[setting]
    M, N = C.walk_shape(variant)
    gm = C.tiled_gm(variant, 3, 2, keys.get("ql_band", 0))[1]
    assert gm == (2 if "ql_rot" in keys else 1)
    for ki, K in enumerate(C.k_tiled(variant)):
        u8 = ki % 2 == 1
        with _tuning(lib, ql_variant=variant, **keys):
            _run(lib, M, N, K, u8, "i8", "f32", C.note(C.tiled_name(variant), u8, gm), f"variant {variant} {keys}")


@pytest.mark.parametrize("M", C.STREAM_M)
@pytest.mark.parametrize("variant", sorted(C.STREAMS))
def test_k_walk_of_the_streaming_kernels(lib, variant, M):
    for ki, K in enumerate(C.k_stream()):
        u8 = ki % 2 == 1
        with _tuning(lib, ql_variant=variant):
            _run(lib, M, 17, K, u8, "i8", "f32", C.note("qlinear_stream_lds_8waves", u8, C.STREAMS[variant]), f"variant {variant}")


@pytest.mark.parametrize("M", C.STREAM_M)
@pytest.mark.parametrize("form", ["w4", "w4zp", "lut"])
def test_k_walk_of_the_packed_kernels(lib, form, M):
    """The codebook's entry 0 is -77: beyond K the activation must be the zero code, for uint8 and int8 activations."""
    name = "qlinear_stream_lut4" if form == "lut" else "qlinear_stream_w4"
    for ki, K in enumerate(C.k_stream()):
        for u8 in ((False, True) if form == "lut" else (ki % 2 == 1,)):
            _run(lib, M, 17, K, u8, "lut" if form == "lut" else "w4", form, _form_note(name, u8, C.packed_mt(M), form), form)


# ------------------------------------------------------------------------------------------------
# 3. edge values of every epilogue
# ------------------------------------------------------------------------------------------------

EDGE_IMPLS = [("packed", "w4", None), ("packed", "lut", None)] + [("stream", "i8", v) for v in sorted(C.STREAMS)] \
    + [("tiled", "i8", v) for v in (83233, 166623, 662)] + [("whole", "i8", v) for v in sorted(C.WHOLE)]


@pytest.mark.parametrize("kind,wkind,variant", EDGE_IMPLS, ids=[f"{k}-{w}-{v}" for (k, w, v) in EDGE_IMPLS])
def test_edge_values_of_the_epilogue(lib, kind, wkind, variant):
    """Rounding ties, both clamps, NaN / +inf / -inf through the bias (codes quant_min, quant_max, quant_min), signed zeros and
    subnormal scales and outputs (the oracle keeps subnormals, and it is the contract): float32 and code outputs."""
    M, N, K = C.EDGE_SHAPES[kind]
    for u8 in (False, True):
        p, d = _device(True, M, N, K, u8, wkind)
        if kind == "packed":
            name, u = ("qlinear_stream_lut4" if wkind == "lut" else "qlinear_stream_w4"), C.packed_mt(M)
        elif kind == "stream":
            name, u = "qlinear_stream_lds_8waves", C.STREAMS[variant]
        elif kind == "tiled":
            bm, bn = C.TILED[variant][:2]
            name, u = C.tiled_name(variant), C.tiled_gm(variant, -(-M // bm), -(-N // bn), 0)[1]
        else:
            name, u = C.WHOLE[variant][2:]
        for launch, forms in C.EDGE_FORMS.items():
            for fi, out in enumerate(forms):
                _, want = C.edge_expected(M, N, K, u8, wkind, launch, fi)
                form = wkind if kind == "packed" else "f32" if out is None else "codes"
                with _tuning(lib, ql_variant=variant or 0):
                    _launch(lib, p, d, form, out, want, C.note(name, u8, u), f"{kind} {wkind} {variant} u8={u8} {launch} out={out}",
                            bias="edge" if launch == "bias" else None)


# ------------------------------------------------------------------------------------------------
# 4. frames for the entry points that had none, at the small ragged shapes of the existing lists
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0] + sorted(C.STREAMS) + sorted(C.TILED))
def test_plain_codes_and_zero_point_forms_stay_inside_their_output(lib, variant):
    for (M, N, K) in ((1, 16, 16), (16, 33, 272), (130, 20, 528)):
        for u8 in (False, True):
            for form in ("f32", "codes", "zp"):
                note = None
                if variant in C.STREAMS:
                    note = _form_note("qlinear_stream_lds_8waves", u8, C.STREAMS[variant], form)
                elif variant in C.TILED:
                    bm, bn = C.TILED[variant][:2]
                    note = _form_note(C.tiled_name(variant), u8, C.tiled_gm(variant, -(-M // bm), -(-N // bn), 0)[1], form)
                with _tuning(lib, ql_variant=variant):
                    text = _run(lib, M, N, K, u8, "i8", form, note, f"variant {variant}")
                assert text.startswith("qlinear") and f"<{'u8' if u8 else 'i8'} x i8{' zp' if form == 'zp' else ''}," in text, text


@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 130])
def test_packed_forms_stay_inside_their_output(lib, M):
    for (N, K) in ((16, 16), (33, 272), (20, 528)):
        for u8 in (False, True):
            for form in ("w4", "w4zp", "lut"):
                name = "qlinear_stream_lut4" if form == "lut" else "qlinear_stream_w4"
                _run(lib, M, N, K, u8, "lut" if form == "lut" else "w4", form, _form_note(name, u8, C.packed_mt(M), form), form)


# ------------------------------------------------------------------------------------------------
# 5. a refused key leaves the previous value in force
# ------------------------------------------------------------------------------------------------

def test_a_refused_tuning_value_leaves_the_previous_one_in_force(lib):
    from mct_quantizers_amd.hip import native
    M, N, K = C.order_shape(64, 64, 5, 3)
    with _tuning(lib, ql_variant=662, ql_band=3, ql_rot=1, ql_stagger=1):
        for key, (bad, message) in C.KEY_REFUSALS.items():
            for v in bad:
                assert lib.mctq_set_tuning(key.encode(), v) == native.MCTQ_E_ARG and lib.mctq_last_error() == message
        assert C.tiled_gm(662, 5, 3, 0)[1] != 3
        _run(lib, M, N, K, True, "i8", "f32", C.note(C.tiled_name(662), True, 3), "ql_band=3 kept")
