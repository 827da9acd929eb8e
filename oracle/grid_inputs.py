"""Edge-value inputs for the export-grid arithmetic (test infrastructure only, numpy).

One generator shared by the GPU geometry tests (tests/test_gpu_export_grid.py) and by the reference
fixture ``tests/golden/export_edges.*`` (tools/gen_golden.py --export-edges), so that the values the
kernels are tested on are the values the oracle is anchored on.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32

# planted on top of the mix, each at least COPIES times where the tensor is large enough
SPECIALS = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38], dtype=F32)
COPIES = 40


def grid_params(rng, channels: int, zero_lo: bool = False):
    """``lo = -U(0.1, 4)``, ``hi = U(0.1, 4)``, ``step = (hi - lo) / 255`` in float32, one set per channel.
    ``zero_lo``: every third channel (channel 0 included) gets ``lo = 0``, where ``-0.0`` meets a zero bound."""
    lo = (-rng.uniform(0.1, 4, channels)).astype(F32)
    hi = rng.uniform(0.1, 4, channels).astype(F32)
    if zero_lo:
        lo[::3] = F32(0)
    step = ((hi - lo) / F32(255)).astype(F32)
    return lo, hi, step


def grid_edge_inputs(rng, shape, lo, hi, step, axis=None) -> np.ndarray:
    """float32 inputs dense in what the grid arithmetic can get wrong, relative to each element's OWN channel.

    One eighth of the elements each: normals x 3; exact ties of the shifted grid ``lo + (k + 0.5) * step``,
    ``k`` in [-2, 257]; ties of the unshifted grid ``(k - 128 + 0.5) * step``; exactly ``lo``; exactly ``hi``;
    the remaining three eighths uniform over the clip range widened by a tenth on each side.  Then NaN, +-inf,
    +-0.0, +-1e-45, 1e-39 and +-3e38 at random positions: COPIES of each, or as many as fit a quarter of a
    small tensor.  ``lo`` / ``hi`` / ``step``: float32 vectors along ``axis``, or scalars when ``axis`` is None.
    """
    shape = tuple(int(s) for s in shape)
    lo, hi, step = (np.asarray(v, dtype=np.float64).astype(F32) for v in (lo, hi, step))
    if axis is None:
        lo_b, hi_b, st_b = (np.broadcast_to(v.reshape(-1)[0], shape) for v in (lo, hi, step))
    else:
        bs = [1] * len(shape)
        bs[axis] = -1
        lo_b, hi_b, st_b = (np.broadcast_to(v.reshape(bs), shape) for v in (lo, hi, step))
    kind = rng.integers(0, 8, size=shape)
    k = rng.integers(-2, 258, size=shape).astype(F32)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        span = (hi_b - lo_b).astype(F32)
        x = (lo_b + (rng.uniform(-0.1, 1.1, size=shape).astype(F32) * span).astype(F32)).astype(F32)
        x = np.where(kind == 0, (rng.standard_normal(shape) * 3).astype(F32), x)
        x = np.where(kind == 1, (lo_b + ((k + half) * st_b).astype(F32)).astype(F32), x)
        x = np.where(kind == 2, ((k - F32(128) + half) * st_b).astype(F32), x)
        x = np.where(kind == 3, lo_b, x)
        x = np.where(kind == 4, hi_b, x)
    x = np.ascontiguousarray(x, dtype=F32)
    flat = x.reshape(-1)
    want = COPIES * SPECIALS.size
    m = want if flat.size >= 2 * want else flat.size // 4
    if m:
        flat[rng.choice(flat.size, size=m, replace=False)] = np.resize(SPECIALS, m)
    return x
