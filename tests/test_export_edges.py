"""The export arithmetic on edge values, anchored in the reference.

tests/golden/export_edges.* (tools/gen_golden.py --export-edges) holds what the reference's four export functions --
quantize_sym_weights_torch, quantize_uniform_weights_torch, quantize_sym_activations_torch and
quantize_uniform_activations_torch, reached through its quantizer classes while tracing, on the CPU -- return for the
inputs of oracle/grid_inputs.py: NaN, +-inf, +-0.0 at a zero bound, denormals, ties and bounds of every channel's own
grid, on channel-last (C = 8, 12), long-row (inner = 1028) and per-tensor shapes.  The GPU grid tests
(tests/test_gpu_export_grid.py) compare the kernels with ``oracle.mctq_oracle.export_grid`` on inputs from the same
generator; here that oracle is held to the reference.  Bar: every element bit for bit, NaN matches NaN.
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _load():
    with open(os.path.join(GOLDEN, "export_edges.json")) as f:
        meta = json.load(f)
    return meta["cases"], np.load(os.path.join(GOLDEN, "export_edges.npz"))


def _same(got, want):
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False, f"shape {got.shape} vs {want.shape}"
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if ok.all():
        return True, ""
    i = tuple(np.argwhere(~ok)[0])
    return False, f"{int((~ok).sum())} mismatches, first at {i}: got={got[i]!r} want={want[i]!r}"


def _traced_call(q, x):
    box = {}

    def fn(t):
        box["y"] = q(t)
        return box["y"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.trace(fn, x, check_trace=False)
    return box["y"].detach()


def _make(case):
    import mct_quantizers_amd as mq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        q = getattr(mq.pytorch_quantizers, case["cls"])(**case["kwargs"])
    q.enable_custom_impl()
    return q


def test_fixture_covers_the_edges():
    cases, arrays = _load()
    names = {c["name"] for c in cases}
    assert len(cases) >= 12
    assert {"wsym_last8", "wsym_last12", "wsym_rows1028", "wuni_last8", "wuni_last12", "asym_u", "auni_neg", "auni_pos"} <= names
    assert {c["cls"] for c in cases} >= {"WeightsSymmetricInferableQuantizer", "WeightsUniformInferableQuantizer",
                                         "ActivationSymmetricInferableQuantizer", "ActivationUniformInferableQuantizer"}
    neg_zero_out = 0
    for c in cases:
        x, y = arrays[c["id"] + "_x"], arrays[c["id"] + "_y"]
        assert x.dtype == np.float32 and y.dtype == np.float32 and list(x.shape) == c["shape"] == list(y.shape)
        bits = x.view(np.uint32)
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any(), c["name"]
        assert (bits == 0x80000000).any() and (bits == 0).any() and (bits == 1).any() and (bits == 0x80000001).any(), c["name"]
        neg_zero_out += int((y.view(np.uint32) == 0x80000000).sum())
    assert neg_zero_out > 0                                   # the signed-zero bar is live


def test_oracle_reproduces_the_reference_on_edge_values():
    from oracle import mctq_oracle as O
    from oracle import oracle_export_call, oracle_export_params
    cases, arrays = _load()
    for c in cases:
        x, want = arrays[c["id"] + "_x"], arrays[c["id"] + "_y"]
        ok, why = _same(oracle_export_call(c["cls"], c["kwargs"], x), want)                 # the export_* wrappers
        assert ok, f'{c["id"]} {c["name"]} (wrapper): {why}'
        lo, hi, step, axis, shifted = oracle_export_params(c["cls"], c["kwargs"], x.ndim)
        ok, why = _same(O.export_grid(x, lo, hi, step, axis, shifted), want)                # export_grid itself
        assert ok, f'{c["id"]} {c["name"]} (export_grid): {why}'


def test_traced_quantizers_on_cpu_tensors_match_the_reference_on_edge_values():
    cases, arrays = _load()
    for c in cases:
        y = _traced_call(_make(c), torch.from_numpy(arrays[c["id"] + "_x"].copy()))
        ok, why = _same(y.numpy(), arrays[c["id"] + "_y"])
        assert ok, f'{c["id"]} {c["name"]}: {why}'


def test_edge_generator_inputs_oracle_equals_the_literal_torch_chain():
    """On the generator's inputs the numpy oracle and the reference's literal op chain (torch, CPU) agree bit for bit, for
    both forms and per channel, and the unshifted form yields -0.0 results."""
    from oracle import mctq_oracle as O
    from oracle.grid_inputs import grid_edge_inputs, grid_params
    rng = np.random.default_rng(11)
    neg_zero = 0
    for shape in ((3, 5, 1024), (700, 12, 1), (1, 5001, 1), (4, 6, 5)):
        for zero_lo in (False, True):
            lo, hi, step = grid_params(rng, shape[1], zero_lo)
            x = grid_edge_inputs(rng, shape, lo, hi, step, axis=1)
            xt = torch.from_numpy(x)
            lt, ht, st = (torch.from_numpy(v).reshape(1, -1, 1) for v in (lo, hi, step))
            c = torch.where(xt < lt, lt, xt)
            c = torch.where(xt > ht, ht, c)
            for shifted in (False, True):
                want = st * torch.round((c - lt) / st) + lt if shifted else torch.round(c / st) * st
                got = O.export_grid(x, lo, hi, step, 1, shifted)
                ok, why = _same(got, want.numpy())
                assert ok, f"{shape} zero_lo={zero_lo} shifted={shifted}: {why}"
                if not shifted:
                    neg_zero += int((got.view(np.uint32) == 0x80000000).sum())
    assert neg_zero > 0


@pytest.mark.gpu
def test_traced_quantizers_on_gpu_match_the_reference_on_edge_values():
    from mct_quantizers_amd.hip import native
    native.load()
    cases, arrays = _load()
    for c in cases:
        n0 = native.launch_count()
        y = _traced_call(_make(c), torch.from_numpy(arrays[c["id"] + "_x"].copy()).cuda())
        assert y.is_cuda and native.launch_count() > n0 and "GridOp" in native.last_launch(), c["name"]
        ok, why = _same(y.cpu().numpy(), arrays[c["id"] + "_y"])
        assert ok, f'{c["id"]} {c["name"]} [{native.last_launch()}]: {why}'
