"""What does folding the residual join into the product in front of it save?  (fuse_linear_consumers_fx(..., stay_on_codes=True,
fused_residuals=True); consumers.qlinear_i8(residual=..., relu=...); include/mctq_hip.h: mctq_qlinear_i8_res)

Sections, each in one process with its arms alternating round by round (median of --rounds, with least and most):
    kernel   the fused product against the product + join pair it replaces, on the SAME buffers, for the block-end products of
             ResNet-50, channels-last rows, per batch: the four downsample convolutions (float32 residual: the other branch's
             output) and the four identity shapes (codes residual: the join in front), ReLU, uint8 codes out.  Outputs are compared
             bit for bit first, and the kernel each arm's product chose is printed: where the unfused product runs on a
             register-pinned whole-tile kernel the fused one runs on the tiled kernels, and the table shows whether it is slower.
             Warm buffers: every call reads the same tensors (batch 64's do not fit the caches)
    model    workloads.wrapped_resnet50, eager forward, through fuse_linear_consumers_fx(convolutions=True, shared_holders=True,
             stay_on_codes=True, pools=True) and the same with fused_residuals=True: outputs compared bit for bit, joins and
             launches per forward counted, the kernel of every fused launch listed
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/residual_consumer_probe.py [--sections kernel model] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "model"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

native.load()
assert torch.cuda.is_available(), "the probe measures on the GPU"
dev = torch.device("cuda")

# (what, K, N, output image side, joins of this shape that the rewrite folds in ResNet-50)
PRODUCTS = [("down, f32 residual", 64, 256, 56, 1), ("down, f32 residual", 256, 512, 28, 1), ("down, f32 residual", 512, 1024, 14, 1),
            ("down, f32 residual", 1024, 2048, 7, 1), ("c3, codes residual", 64, 256, 56, 2), ("c3, codes residual", 128, 512, 28, 3),
            ("c3, codes residual", 256, 1024, 14, 5), ("c3, codes residual", 512, 2048, 7, 0)]
FORM = (8.0 / 255, 0, 0, 255)                                 # the holder behind a ReLU
R_FORM = (8.0 / 255, 0)


def timed(arms, iters=None):
    """arms: [(name, f())] -> {name: (median us, least us, most us)}, rounds alternating between the arms"""
    iters = iters or args.iters
    times = {name: [] for name, _ in arms}
    for name, f in arms:                                      # warm every arm before any timed window
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, f in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000 / iters)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in times.items()}


def cell(r, digits=2):
    return f"{r[0]:.{digits}f} ({r[1]:.{digits}f} .. {r[2]:.{digits}f})"


def kernel_of(launch):
    return launch.split("<")[0]


if "kernel" in args.sections:
    rows_md = []
    for what, K, N, side, count in PRODUCTS:
        for B in args.batches:
            M = B * side * side
            g = torch.Generator(device=dev).manual_seed(K + N)
            a = torch.randint(0, 256, (M, K), device=dev, generator=g).to(torch.uint8)
            w = torch.randint(-128, 128, (N, K), device=dev, generator=g).to(torch.int8)
            ws = ((torch.rand(N, device=dev, generator=g) + 0.5) * (4.0 / (0.02 * 5476.0 * K ** 0.5))).float()
            bias = (torch.rand(N, device=dev, generator=g) - 0.5).float()
            rowsum = w.sum(dim=1, dtype=torch.int32)
            as_codes = what.startswith("c3")
            rc = torch.randint(0, 256, (M, N), device=dev, generator=g).to(torch.uint8)
            residual, r_form = (rc, R_FORM) if as_codes else (ops.dequantize_codes(rc, *R_FORM), None)
            del rc
            operands = (a, 0, 0.02, w, ws, rowsum, bias)

            def pair():
                x = consumers.qlinear_i8(*operands)
                kw = dict(residual_codes=(residual, *r_form)) if as_codes else dict(residual=residual)
                return ops.fq_join(x, *FORM, relu=True, want_float=False, **kw)[1]

            def product_alone():
                return consumers.qlinear_i8(*operands)

            def fused():
                return consumers.qlinear_i8(*operands, FORM, residual=residual, residual_codes=r_form, relu=True)

            product_alone()
            k_pair = kernel_of(native.last_launch())
            want = pair()
            assert native.last_launch().startswith("fq_join<")
            got = fused()
            k_fused = kernel_of(native.last_launch())
            assert " res(" in native.last_launch() and torch.equal(got, want), "the fused product differs from the pair"
            del got, want
            res = timed([("pair", pair), ("product", product_alone), ("fused", fused)], iters=100)
            p, x, f = res["pair"], res["product"], res["fused"]
            print(f"{what} {M} x {N} x {K} (batch {B}, {count} in the model): pair {cell(p)} us [{k_pair} + fq_join]; its product alone "
                  f"{cell(x)} us; fused {cell(f)} us [{k_fused}]; pair / fused {p[0] / f[0]:.2f}", flush=True)
            rows_md.append(f"| {what} | {K} | {N} | {side} | {B} | {count} | {cell(p)} | {cell(x)} | {cell(f)} | {p[0] / f[0]:.2f} | "
                           f"{k_pair} | {k_fused} |")
            del a, w, residual
            torch.cuda.empty_cache()
    print("\n| product | K | N | image | batch | folded in ResNet-50 | product + join us (least .. most) | that product alone us | fused us "
          "| pair / fused | the pair's product ran on | the fused product ran on |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


def launches_per_forward(m, x, log=None):
    m(x)
    count = native.launch_count()
    hooks = []
    if log is not None:
        for name, s in m.named_modules():
            if isinstance(s, consumers.IntegerConsumer) and s.emit_residual is not None:
                hooks.append(s.register_forward_hook(lambda mod, a, out, name=name: log.append((name, tuple(out.shape), native.last_launch()))))
    m(x)
    for h in hooks:
        h.remove()
    return native.launch_count() - count


if "model" in args.sections:
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True)
    print("\nwrapped ResNet-50 (workloads.wrapped_resnet50), eager forward, NCHW float32 input; outputs of the two arms equal bit for bit")
    print("| batch | arm | wrapped layers on codes | joins | launches per forward | us per forward (least .. most) |\n|---|---|---|---|---|---|")
    with torch.no_grad():
        arms_of = {"fused_residuals=False": consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(), **switches),
                   "fused_residuals=True": consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(), fused_residuals=True, **switches)}
        chosen = {}
        for B in args.batches:
            x = torch.randn(B, 3, 224, 224, device=dev)
            first, second = (m(x) for m, _ in arms_of.values())
            assert torch.equal(first, second), "fused_residuals changed the output"
            del first, second
            res = timed([(name, (lambda m: lambda: m(x))(m)) for name, (m, _) in arms_of.items()], iters=max(1, args.iters // 5))
            for name, (m, n) in arms_of.items():
                joins = sum(isinstance(s, consumers.QuantizedJoin) for s in m.modules())
                log = [] if name.endswith("True") else None
                print(f"| {B} | {name} | {n} | {joins} | {launches_per_forward(m, x, log)} | {cell(res[name], 1)} |", flush=True)
                if log:
                    chosen[B] = log
        for B, log in chosen.items():
            print(f"\nthe fused launches at batch {B}:")
            for name, shape, launch in log:
                print(f"    {name} -> {shape}: {launch}")
