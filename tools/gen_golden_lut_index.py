#!/usr/bin/env python3
"""Generate tests/golden/lut_index_cases.{json,npz} from the REFERENCE implementation.

Runs only in the build container (imports sony/mct_quantizers from /root/reference, torch CPU), like tools/gen_golden.py.
For ~40 seeded cases of the three LUT quantizer classes it records the input, the reference quantizer's output and the
codebook index the reference's chain selects -- ``torch.argmin(torch.abs(t - lut))`` over the reference's own
``int_quantization_with_threshold`` result (quantizer_utils.py:126-134).  The cases cover 2 / 3 / 4 / 8 bits, codebooks
with duplicates and in shuffled order, per tensor and per channel on the first / a middle / the last axis, power-of-two
and other thresholds, and inputs with NaN, +-inf, +-0, values on and +-1 ulp around the half-integer points of the scaled
domain and values beyond the clip range.

Data only (inputs and expected outputs); the reference source never enters this repository.
Usage:  python tools/gen_golden_lut_index.py
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")

import torch  # noqa: E402
from mct_quantizers.pytorch import quantizers as refq  # noqa: E402  (the reference)
from mct_quantizers.pytorch.quantizer_utils import int_quantization_with_threshold  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
rng = np.random.default_rng(20261016)
F32 = np.float32
BITWIDTH = 8
EPS = 1e-8


def codebook(bits: int, signed: bool, kind: str):
    lo, hi = (-2 ** (BITWIDTH - 1), 2 ** (BITWIDTH - 1) - 1) if signed else (0, 2 ** BITWIDTH - 1)
    n = 2 ** bits
    vals = rng.choice(np.arange(lo, hi + 1), size=n, replace=False).astype(np.float64)
    vals.sort()
    if kind == "dup":                               # duplicates, not adjacent in the list
        k = max(1, n // 4)
        perm = rng.permutation(n)
        src, dst = perm[:k], perm[k:2 * k]
        vals[dst] = vals[src]
    if kind in ("shuffled", "dup"):
        rng.shuffle(vals)
    return [float(v) for v in vals]


def channel_values(n: int, thr: float, lut, signed: bool):
    """n inputs for one threshold: random ones and every interesting point of the scaled domain t = x / thr * mult."""
    mult = 2.0 ** (BITWIDTH - int(signed))
    cmin, cmax = (-2 ** (BITWIDTH - 1), 2 ** (BITWIDTH - 1) - 1) if signed else (0, 2 ** BITWIDTH - 1)
    cs = np.unique(np.asarray(lut))
    pts = list((cs[:-1] + cs[1:]) / 2.0)                                # decision points: midpoints of adjacent centres
    pts += list(rng.integers(cmin, cmax, size=6) + 0.5)                 # other half-integer points
    pts += [cmin, cmax, cmin - 0.5, cmax + 0.5, cmin + 0.5, cmax - 0.5]
    special = []
    for p in pts:
        x0 = F32(F32(p) / F32(mult) * F32(thr))
        special += [x0, np.nextafter(x0, F32(np.inf)), np.nextafter(x0, F32(-np.inf)),
                    np.nextafter(np.nextafter(x0, F32(np.inf)), F32(np.inf))]
    special += [F32(np.nan), F32(np.inf), F32(-np.inf), F32(0.0), F32(-0.0), F32(2.5 * thr), F32(-2.5 * thr),
                F32(1e30), F32(-1e30), F32(1e-40), F32(thr), F32(-thr)]
    special = np.asarray(special, dtype=F32)
    x = (rng.standard_normal(n) * thr * 0.6).astype(F32)
    take = rng.random(n) < 0.6
    x[take] = rng.choice(special, size=int(take.sum()))
    return x


def thresholds(n: int, pot: bool):
    if pot:
        return [float(2.0 ** int(e)) for e in rng.integers(-4, 4, size=n)]
    return [float(F32(v)) for v in rng.uniform(0.05, 6.0, size=n)]


def main():
    cases, arrays = [], {}
    total = 0
    plan = []
    for bits in (2, 3, 4, 8):
        for kind in ("sorted", "shuffled", "dup"):
            plan.append(("WeightsLUTSymmetricInferableQuantizer", bits, kind, None, (23, 32)))
            plan.append(("WeightsLUTSymmetricInferableQuantizer", bits, kind, len(plan) % 3, (6, 5, 24)))
    for bits, kind, axis, shape in ((2, "dup", 0, (8, 16)), (3, "shuffled", 1, (4, 8, 16)), (4, "dup", 2, (5, 3, 16)),
                                    (8, "shuffled", None, (17, 9)), (4, "sorted", 1, (16, 16)), (3, "dup", None, (40, 8))):
        plan.append(("WeightsLUTPOTInferableQuantizer", bits, kind, axis, shape))
    for bits, kind, signed in ((2, "dup", True), (3, "shuffled", False), (4, "dup", False), (8, "shuffled", True),
                               (4, "sorted", True), (8, "dup", False), (2, "sorted", False), (3, "dup", True),
                               (4, "shuffled", True), (8, "sorted", False)):
        plan.append(("ActivationLutPOTInferableQuantizer", bits, kind, signed, (3, 7, 16)))

    for i, (cls, bits, kind, axis_or_signed, shape) in enumerate(plan):
        cid = f"c{i:02d}"
        activation = cls.startswith("Activation")
        pot = "POT" in cls
        if activation:
            signed, axis = bool(axis_or_signed), None
        else:
            signed, axis = True, axis_or_signed
        lut = codebook(bits, signed, kind)
        n_thr = 1 if axis is None else shape[axis]
        thr = thresholds(n_thr, pot)
        x = np.empty(shape, dtype=F32)
        if axis is None:
            x[...] = channel_values(x.size, thr[0], lut, signed).reshape(shape)
        else:
            for c in range(n_thr):
                sl = [slice(None)] * len(shape)
                sl[axis] = c
                x[tuple(sl)] = channel_values(x.size // n_thr, thr[c], lut, signed).reshape(x[tuple(sl)].shape)
        if activation:
            kwargs = dict(num_bits=bits, lut_values=lut, threshold=thr, signed=signed, lut_values_bitwidth=BITWIDTH, eps=EPS)
            thr_t = thr[0]                                         # a Python float, as the class passes it
        else:
            kwargs = dict(num_bits=bits, lut_values=lut, threshold=thr, per_channel=axis is not None, channel_axis=axis,
                          input_rank=len(shape) if axis is not None else None, lut_values_bitwidth=BITWIDTH, eps=EPS)
            thr_t = torch.tensor(thr, dtype=torch.float32)
            if axis is not None:
                bs = [1] * len(shape)
                bs[axis] = -1
                thr_t = thr_t.reshape(bs)
        q = getattr(refq, cls)(**kwargs)
        xt = torch.from_numpy(x.copy())
        y = q(xt).detach().numpy().astype(F32)
        lut_t = torch.tensor(lut, dtype=torch.float32)
        t = int_quantization_with_threshold(torch.from_numpy(x.copy()), n_bits=BITWIDTH, signed=signed, threshold=thr_t, eps=EPS)
        idx = torch.argmin(torch.abs(t.unsqueeze(-1) - lut_t.reshape([1] * t.dim() + [-1])), dim=-1).numpy()
        # the index reproduces the reference's output through the two float32 operations of the chain's end
        mult = F32(2.0 ** (BITWIDTH - int(signed)))
        thr_b = np.asarray(thr, dtype=F32)
        thr_b = thr_b[0] if axis is None else thr_b.reshape([-1 if d == axis else 1 for d in range(len(shape))])
        again = (np.asarray(lut, dtype=F32)[idx] / mult) * thr_b
        assert again.astype(F32).tobytes() == y.tobytes(), cid
        assert idx.max() < len(lut)
        arrays[cid + "_x"], arrays[cid + "_y"], arrays[cid + "_idx"] = x, y, idx.astype(np.uint8)
        cases.append(dict(id=cid, cls=cls, kwargs=kwargs, axis=axis, signed=signed, kind=kind, shape=list(shape)))
        total += x.size
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "lut_index_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "lut_index_cases.npz"), **arrays)
    print(f"{len(cases)} cases, {total} elements, "
          f"{os.path.getsize(os.path.join(OUT, 'lut_index_cases.npz'))} bytes")


if __name__ == "__main__":
    main()
