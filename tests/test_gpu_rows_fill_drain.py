"""rows_kernel_finetail (csrc/mctq_kernels.hpp; tuning key "filldrain"): symmetric float32 per-channel rows that are a whole
number of four-vector tiles (1024 lane-vectors = 4096 elements), rows_kernel's blocks with the LAST half round of tiles of the
launch cut into four one-vector blocks each.  Default: launches of at least 9/8 rounds of resident blocks (config 2 -- 4096 x 4096
-- is two); "filldrain" = 2 takes it whenever the launch is eligible, 0 never.  Bit for bit against the oracle: config 2 at full
size, the neighbour shapes it was measured on, row counts that make the fine tail empty / partial / the whole launch, rows of
several tiles (the tail starting inside a row), outer > 1 (channel = row % channels), a seeded geometry fuzz; launches with a
zero-point table, 16-bit storage and rows that are no whole tiles keep their old routes."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import bits_equal, finite_equal, first_mismatch

pytestmark = pytest.mark.gpu
NEW = "rows_kernel_finetail"


@pytest.fixture(scope="module")
def lib():
    from mct_quantizers_amd.hip import native
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return native.load()


@pytest.fixture()
def tuning():
    """set(key, value) for the test, every touched key back to its default afterwards"""
    from mct_quantizers_amd.hip import native
    defaults = {"filldrain": 1, "paced": 1, "shortrows": 1, "rowsteps": 2}
    touched = set()

    def set_(key, value):
        touched.add(key)
        native.set_tuning(key, value)
    yield set_
    for key in touched:
        native.set_tuning(key, defaults[key])


def _round():
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count      # resident 256-thread blocks


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _input(rng, shape, s_b, zp_b, qmin, qmax):
    """normal values spread over the grid, a third of them exactly on a grid point or on a rounding tie"""
    with np.errstate(all="ignore"):
        x = rng.standard_normal(shape).astype(np.float32) * np.minimum(s_b, np.float32(1.0)) * np.float32(0.4 * (qmax - qmin))
        k = rng.integers(qmin - 2, qmax + 3, size=shape).astype(np.float32) - zp_b
        kind = rng.integers(0, 6, size=shape)
        x = np.where(kind == 0, (k + np.float32(0.5)) * s_b, x)
        x = np.where(kind == 1, k * s_b, x)
    return np.nan_to_num(x.astype(np.float32), nan=0.0, posinf=3e38, neginf=-3e38)


def _abi_case(lib, rng, outer, C, inner, dt="float32", with_zp=False, qmin=-128, qmax=127, wild_scales=False):
    """one mctq_fq_per_channel call on a seeded tensor -> (launch name, got, want, x)"""
    from mct_quantizers_amd.hip import native
    from oracle import mctq_oracle as O
    code, tdt = {"float32": 0, "float16": 1, "bfloat16": 2}[dt], getattr(torch, dt)
    scales = rng.uniform(0.01, 0.2, size=C).astype(np.float32)
    if wild_scales:                                               # divisors whose reciprocal is subnormal / huge
        scales[:: int(rng.integers(1, 40))] = np.float32(3e-33)
        scales[int(rng.integers(0, C)):: int(rng.integers(1, 90))] = np.float32(2e31)
    zps = rng.integers(-5, 6, size=C).astype(np.int32) if with_zp else np.zeros(C, dtype=np.int32)
    shape = (outer, C, inner)
    x32 = _input(rng, shape, scales.reshape(1, C, 1), zps.reshape(1, C, 1).astype(np.float32), qmin, qmax)
    xh = _dev(x32).to(tdt)
    x_np = xh.float().cpu().numpy()
    y = torch.full_like(xh, 300.0)                                # a value no grid holds: an unwritten element shows
    s_d, z_d = _dev(scales), _dev(zps)
    rc = lib.mctq_fq_per_channel(xh.data_ptr(), y.data_ptr(), outer, C, inner, code, s_d.data_ptr(),
                                 z_d.data_ptr() if with_zp else None, qmin, qmax, _stream())
    assert rc == 0, lib.mctq_last_error()
    name = native.last_launch().split("<")[0]
    want = O.narrow(O.fake_quant_affine(x_np, scales, zps, qmin, qmax, axis=1), dt)
    return name, y.float().cpu().numpy(), want, x_np


def _quantizer_setup(shape, axis, seed):
    """a symmetric per-channel weights quantizer, its input on the GPU, the oracle's output"""
    import mct_quantizers_amd as mq
    from oracle import oracle_call
    rng = np.random.default_rng(seed)
    x_np = (rng.standard_normal(shape) * 1.5).astype(np.float32)
    kw = dict(num_bits=8, threshold=[float(v) for v in rng.uniform(0.5, 4.0, shape[axis])], per_channel=True, channel_axis=axis)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = mq.pytorch_quantizers.WeightsSymmetricInferableQuantizer(**kw)
        want = oracle_call("WeightsSymmetricInferableQuantizer", kw, x_np)
    return q, torch.from_numpy(x_np).cuda(), want, x_np


def _run(q, x):
    from mct_quantizers_amd.hip import native
    y = q(x)
    return native.last_launch().split("<")[0], y.cpu().numpy()


def test_config_2_at_full_size_takes_the_route_by_default_and_equals_the_oracle():
    """bench.py's default workload itself (workloads.make_workload("cfg2"): 4096 x 4096 float32, per channel on axis 0)."""
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import workloads
    from mct_quantizers_amd.hip import native
    from oracle import oracle_call
    x_np = workloads.make_input("cfg2")
    assert x_np.shape == (4096, 4096) and x_np.dtype == np.float32
    wl = workloads.make_workload("cfg2", x_np)
    q = getattr(mq.pytorch_quantizers, wl.quantizer)(**wl.kwargs)
    y = q(torch.from_numpy(x_np).cuda())
    assert native.last_launch().startswith(NEW + "<"), native.last_launch()
    got, want = y.cpu().numpy(), oracle_call(wl.quantizer, wl.kwargs, x_np)
    assert bits_equal(got, want), first_mismatch(got, want, x_np)


@pytest.mark.parametrize("shape,default_route", [
    ((8192, 4096), NEW), ((6144, 4096), NEW), ((4096, 8192), NEW), ((3072, 4096), NEW),
    ((2048, 4096), "shortrows_kernel"),        # one round: the paced window's (tuning key "paced")
    ((16384, 1024), "gather_kernel"),          # rows of a quarter tile: never eligible
])
def test_neighbour_shapes_by_default_and_forced(shape, default_route, tuning):
    q, x, want, x_np = _quantizer_setup(shape, 0, seed=shape[0] + shape[1])
    name, got = _run(q, x)
    assert name == default_route, (shape, name)
    assert bits_equal(got, want), (shape, name, first_mismatch(got, want, x_np))
    tuning("filldrain", 2)
    tuning("paced", 0)                                            # (the paced window is asked first)
    name2, got2 = _run(q, x)
    assert name2 == (NEW if shape[1] % 4096 == 0 else default_route), (shape, name2)
    assert bits_equal(got2, want), (shape, name2, first_mismatch(got2, want, x_np))
    tuning("filldrain", 0)
    name0, got0 = _run(q, x)
    assert name0 != NEW and bits_equal(got0, want), (shape, name0)


def test_row_counts_around_the_fine_tail_and_the_round(lib, tuning):
    """R = half a round of tiles is the fine tail.  One tile per row (4096-element rows): rows = 1, R - 1, R (the whole launch is
    fine blocks), R + 1 (one bulk block), a round - 1 / + 1; the default takes the route from 9/8 rounds on and not below."""
    from mct_quantizers_amd.hip import native
    rnd = _round()
    R = rnd // 2
    rng = np.random.default_rng(77)
    tuning("filldrain", 2)
    tuning("paced", 0)
    for rows in (1, 2, R - 1, R, R + 1, rnd - 1, rnd, rnd + 1):
        name, got, want, x_np = _abi_case(lib, rng, 1, rows, 4096)
        assert name == NEW, (rows, native.last_launch())
        assert bits_equal(got, want), (rows, first_mismatch(got, want, x_np))
    tuning("filldrain", 1)
    tuning("paced", 1)
    for rows, taken in ((9 * rnd // 8 - 1, False), (9 * rnd // 8, True), (3 * rnd // 2, True), (rnd + 1, False), (R, False)):
        name, got, want, x_np = _abi_case(lib, rng, 1, rows, 4096)
        assert (name == NEW) == taken, (rows, native.last_launch())
        assert bits_equal(got, want), (rows, first_mismatch(got, want, x_np))


def test_rows_of_several_tiles_and_a_wrapped_channel_table(lib, tuning):
    """Rows of 2, 3 and 4 tiles: with three tiles per row the fine tail starts INSIDE a row.  outer > 1: channel = row % channels."""
    from mct_quantizers_amd.hip import native
    rnd = _round()
    rng = np.random.default_rng(78)
    tuning("filldrain", 2)
    tuning("paced", 0)
    cases = [(1, rnd // 4 + 3, 8192), (1, rnd // 6 + 59, 12288), (1, 5, 12288), (1, rnd // 8 + 1, 16384), (1, 1, 16384),
             (3, 700, 4096), (2, rnd // 4 + 1, 4096), (5, 3, 12288), (4, 1, 4096), (2, rnd // 2 + 7, 8192)]
    for outer, C, inner in cases:
        tiles = outer * C * (inner // 4096)
        if inner == 12288 and tiles > rnd // 2:
            assert (tiles - rnd // 2) % 3 != 0, "the case is meant to start the tail inside a row"
        name, got, want, x_np = _abi_case(lib, rng, outer, C, inner, wild_scales=C > 8)
        assert name == NEW, ((outer, C, inner), native.last_launch())
        assert finite_equal(got, want, x_np), ((outer, C, inner), first_mismatch(got, want, x_np))


def test_zero_point_tables_16_bit_storage_and_ragged_rows_keep_their_routes(lib, tuning):
    """The route takes symmetric float32 launches only (its kernel reads no zero-point table): everything else is launched as
    before even with the key forced, and still equals the oracle."""
    from mct_quantizers_amd.hip import native
    rnd = _round()
    rng = np.random.default_rng(79)
    tuning("filldrain", 2)
    tuning("paced", 0)
    for kwargs, route in ((dict(outer=1, C=rnd + 5, inner=4096, with_zp=True, qmin=0, qmax=255), "rows_kernel"),
                          (dict(outer=2, C=300, inner=8192, with_zp=True, qmin=-8, qmax=7), "rows_kernel"),
                          (dict(outer=1, C=rnd // 2 + 3, inner=8192, dt="bfloat16"), None),
                          (dict(outer=1, C=rnd // 2 + 3, inner=8192, dt="float16"), None),
                          (dict(outer=1, C=700, inner=4096 + 1024), "rows_kernel"),       # five steps: a ragged last tile
                          (dict(outer=1, C=700, inner=2048), None),
                          (dict(outer=1, C=700, inner=4100), None)):
        name, got, want, x_np = _abi_case(lib, rng, **kwargs)
        assert name != NEW and (route is None or name == route), (kwargs, native.last_launch())
        assert finite_equal(got, want, x_np), (kwargs, name, first_mismatch(got, want, x_np))


def test_fuzz_fine_tail_geometry_vs_oracle(lib, tuning):
    """Seeded fuzz of the launch geometry: tiles per row 1 ... 5, total tiles from one to 2.6 rounds (drawn densely around half a
    round, one round and 9/8 rounds, where the tail is the whole launch / the default rule starts), outer 1 ... 3, signed and
    unsigned grids, scales outside the fast reciprocal's range, the key forced or at its default -- bit for bit against the oracle.
    MCTQ_FUZZ_SEED / MCTQ_FUZZ_CASES widen it."""
    from mct_quantizers_amd.hip import native
    rng = np.random.default_rng(int(os.environ.get("MCTQ_FUZZ_SEED", "707")))
    rnd = _round()
    seen = set()
    for case in range(int(os.environ.get("MCTQ_FUZZ_CASES", "24"))):
        tpr = int(rng.integers(1, 6))
        outer = int(rng.integers(1, 4))
        centre = [rnd // 2, rnd, 9 * rnd // 8, 2 * rnd, None][case % 5]
        tiles = int(rng.integers(1, int(2.6 * rnd))) if centre is None else max(1, centre + int(rng.integers(-2 * tpr * outer, 2 * tpr * outer + 1)))
        C = max(1, tiles // (tpr * outer))
        forced = case % 3 != 2
        tuning("filldrain", 2 if forced else 1)
        tuning("paced", 0 if forced else 1)
        qmin, qmax = [(-128, 127), (0, 255), (-8, 7), (0, 15)][int(rng.integers(0, 4))]
        name, got, want, x_np = _abi_case(lib, rng, outer, C, 4096 * tpr, qmin=qmin, qmax=qmax, wild_scales=C > 8 and rng.random() < 0.4)
        total = outer * C * tpr
        if forced:
            assert name == NEW, (case, (outer, C, tpr), native.last_launch())
        else:
            assert (name == NEW) == (8 * total >= 9 * rnd), (case, (outer, C, tpr), native.last_launch())
        seen.add(name)
        assert finite_equal(got, want, x_np), (case, (outer, C, tpr), forced, native.last_launch(), first_mismatch(got, want, x_np))
    assert NEW in seen, seen


def test_the_key_takes_0_1_2_only(lib):
    from mct_quantizers_amd.hip import native
    for bad in (-1, 3, 11):
        assert lib.mctq_set_tuning(b"filldrain", bad) != 0
    native.set_tuning("filldrain", 1)
