"""What does keeping the activations on codes save?  (fuse_linear_consumers_fx(..., shared_holders=True, stay_on_codes=True);
consumers.folded_clamp, QuantizedJoin(residual_codes=...); include/mctq_hip.h: mctq_fq_join_rc_f32)

Sections, each in one process with its arms alternating round by round (median of --rounds, with least and most):
    kernel   the join with its residual as codes against mctq_fq_join_f32, add + ReLU, on ResNet-50's four identity join shapes
             (channels, image side): (256, 56), (512, 28), (1024, 14), (2048, 7), channels-last, per batch.  Three arms on the same
             tensors: float32 residual with both outputs (what a residual join does without ``stay_on_codes``), codes residual with
             both outputs, codes residual with codes alone (what the join becomes in the model: the swap that really happens is
             the first arm against the third).  Outputs are compared bit for bit first.  Cold caches: every call takes the next
             set of a ring of (x, residual, residual codes) larger than 512 MiB in all (at most 64 sets: the small shapes of
             batch 1 are then warm, and at the launch floor anyway).  Bytes per element: 13, 10 and 6
    model    workloads.wrapped_resnet50, eager forward, through fuse_linear_consumers_fx(convolutions=True, shared_holders=True)
             and the same with stay_on_codes=True: outputs compared bit for bit, joins and launches per forward counted, and the
             largest difference of either to the model as built
    block    the inverted-residual block of tools/dw_consumer_probe.py (32 -> 144 -> depthwise 3x3 -> 32 on 56 x 56, ReLU6),
             through fuse_linear_consumers_fx(depthwise=True, shared_holders=True) and the same with stay_on_codes=True
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/stay_on_codes_probe.py [--sections kernel model block] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mct_quantizers_amd as mq
from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "model", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

native.load()
assert torch.cuda.is_available(), "the probe measures on the GPU"
dev = torch.device("cuda")
Q = mq.pytorch_quantizers

JOINS = [(256, 56), (512, 28), (1024, 14), (2048, 7)]
RING_BYTES, RING_MAX = 600 << 20, 64


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


def launches_per_forward(m, x):
    m(x)
    count = native.launch_count()
    m(x)
    return native.launch_count() - count


if "kernel" in args.sections:
    holder = mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False))
    form = consumers._activation_code_params(holder.activation_holder_quantizer)
    r_scale, r_zp = form[0], form[1]                          # the join in front has the same kind of holder
    rows_md = []
    for (C, side) in JOINS:
        for B in args.batches:
            n = B * C * side * side
            sets = max(1, min(RING_MAX, -(-RING_BYTES // (8 * n))))
            g = torch.Generator(device=dev).manual_seed(C + side)
            ring = []
            for _ in range(sets):
                x = (torch.randn(B, C, side, side, device=dev, generator=g) * 3).contiguous(memory_format=torch.channels_last)
                rc = torch.randint(0, 256, (B, C, side, side), device=dev, generator=g).to(torch.uint8).contiguous(memory_format=torch.channels_last)
                ring.append((x, ops.dequantize_codes(rc, r_scale, r_zp), rc))
            state = {"i": 0}

            def nxt():
                state["i"] = (state["i"] + 1) % sets
                return ring[state["i"]]

            def f32_both():
                x, r, _ = nxt()
                return ops.fq_join(x, *form, residual=r, relu=True)

            def codes_both():
                x, _, rc = nxt()
                return ops.fq_join(x, *form, residual_codes=(rc, r_scale, r_zp), relu=True)

            def codes_only():
                x, _, rc = nxt()
                return ops.fq_join(x, *form, residual_codes=(rc, r_scale, r_zp), relu=True, want_float=False)

            outs = []
            for f in (f32_both, codes_both, codes_only):
                state["i"] = -1
                outs.append(f())
                assert native.last_launch().startswith("fq_join<") and ("addc" in native.last_launch()) == (f is not f32_both)
            assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1]) and outs[1][0].stride() == outs[0][0].stride()
            assert outs[2][0] is None and torch.equal(outs[2][1], outs[0][1])
            del outs
            res = timed([("f32 both", f32_both), ("codes both", codes_both), ("codes only", codes_only)], iters=200)
            a, b, c = res["f32 both"], res["codes both"], res["codes only"]
            print(f"{C} x {side} x {side} batch {B} (ring of {sets}): float32 residual, both out {cell(a)} us; codes residual, both out "
                  f"{cell(b)} us; codes residual, codes out {cell(c)} us, {6 * n / c[0] / 1e3:.0f} GB/s", flush=True)
            rows_md.append(f"| {C} | {side} | {B} | {sets} | {cell(a)} | {cell(b)} | {cell(c)} | {6 * n / c[0] / 1e3:.0f} | "
                           f"{a[0] / b[0]:.2f} | {a[0] / c[0]:.2f} |")
            del ring
            torch.cuda.empty_cache()
    print("\n| channels | image | batch | ring sets | float32 residual, f32 + codes out us (least .. most) | codes residual, f32 + codes out us "
          "| codes residual, codes out us | its GB/s at 6 B | first / second | first / third |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


def model_rows(title, build, switches, x_of, iters):
    print(f"\n{title}")
    print("| batch | arm | wrapped layers on codes | joins | launches per forward | us per forward (least .. most) | max rel diff to as built |"
          "\n|---|---|---|---|---|---|---|")
    with torch.no_grad():
        plain = build()
        arms_of = {}
        for name, kw in (("shared_holders=True", switches), ("shared_holders=True, stay_on_codes=True", dict(switches, stay_on_codes=True))):
            arms_of[name] = consumers.fuse_linear_consumers_fx(build(), **kw)
        for B in args.batches:
            x = x_of(B)
            ref = plain(x)
            outs = {name: m(x) for name, (m, _) in arms_of.items()}
            first, second = outs.values()
            assert torch.equal(first, second), "stay_on_codes changed the output"
            diffs = {name: float((y - ref).abs().max() / ref.abs().max()) for name, y in outs.items()}
            del outs, first, second, ref
            res = timed([(name, (lambda m: lambda: m(x))(m)) for name, (m, _) in arms_of.items()], iters=iters)
            for name, (m, n) in arms_of.items():
                joins = sum(isinstance(s, consumers.QuantizedJoin) for s in m.modules())
                print(f"| {B} | {name} | {n} | {joins} | {launches_per_forward(m, x)} | {cell(res[name], 1)} | {diffs[name]:.1e} |", flush=True)


if "model" in args.sections:
    model_rows("wrapped ResNet-50 (workloads.wrapped_resnet50), eager forward, NCHW float32 input; outputs of the two arms equal bit for bit",
               workloads.wrapped_resnet50, dict(convolutions=True, shared_holders=True),
               lambda B: torch.randn(B, 3, 224, 224, device=dev), max(1, args.iters // 5))


def pair(cin, cout, k, stride, groups=1, relu=False):
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, groups=groups, bias=True).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in conv.weight.detach().abs().amax((1, 2, 3))]
        wq = Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=True, channel_axis=0)
        aq = Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False) if relu else \
            Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-4.0], max_range=[4.0])
    return [mq.PytorchActivationQuantizationHolder(aq).to(dev), mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)]


class InvertedResidual(torch.nn.Module):
    def __init__(self, C=32, E=144):
        super().__init__()
        self.h1, self.c1 = pair(C, E, 1, 1)
        self.h2, self.c2 = pair(E, E, 3, 1, groups=E, relu=True)
        self.h3, self.c3 = pair(E, C, 1, 1, relu=True)

    def forward(self, x):
        y = torch.nn.functional.relu6(self.c1(self.h1(x)))
        y = torch.nn.functional.relu6(self.c2(self.h2(y)))
        return x + self.c3(self.h3(y))


if "block" in args.sections:
    def block():
        torch.manual_seed(0)                                      # the same weights for every arm
        return InvertedResidual().to(dev)

    model_rows("inverted residual, 32 -> 144 -> 144 (depthwise 3x3) -> 32 on 56 x 56, ReLU6, eager forward; outputs of the two arms equal bit for bit",
               block, dict(depthwise=True, shared_holders=True), lambda B: torch.randn(B, 32, 56, 56, device=dev), args.iters)
