"""What does the join in front of a shared activation holder cost?  (consumers.QuantizedJoin, fuse_linear_consumers_fx(...,
shared_holders=True); include/mctq_hip.h: mctq_fq_join_f32)

Shapes: the 16 joins of ResNet-50 at 224 x 224 -- the a3 of every bottleneck, (channels, image side, how many): (256, 56, 3),
(512, 28, 4), (1024, 14, 6), (2048, 7, 3) -- channels-last, at batch 1 and 64.
Sections, each in one process with its arms alternating round by round:
    kernel   ops.fq_join (add, ReLU, float32 and codes out: one launch) against the chain it replaces -- ATen add, ATen ReLU,
             the holder, ops.fq_codes: four launches -- on the same tensors, outputs compared bit for bit first; cold caches:
             every call takes the next set of a ring of (x, residual) pairs larger than 512 MiB in all (at most 64 sets: the
             small shapes of batch 1 are then warm, and at the launch floor anyway).  Achieved bytes/s of the join counts 13 B per
             element: 8 read, 4 + 1 written
    model    workloads.wrapped_resnet50, eager forward: as built, through fuse_linear_consumers_fx(convolutions=True), and
             through fuse_linear_consumers_fx(convolutions=True, shared_holders=True); how many wrapped layers each rewrite
             took, and the largest difference to the model as built
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/join_consumer_probe.py [--sections kernel model] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mct_quantizers_amd as mq
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
Q = mq.pytorch_quantizers

JOINS = [(256, 56, 3), (512, 28, 4), (1024, 14, 6), (2048, 7, 3)]
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


if "kernel" in args.sections:
    holder = mq.PytorchActivationQuantizationHolder(Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False))
    form = consumers._activation_code_params(holder.activation_holder_quantizer)
    rows_md = []
    for (C, side, count) in JOINS:
        for B in args.batches:
            n = B * C * side * side
            sets = max(1, min(RING_MAX, -(-RING_BYTES // (8 * n))))
            g = torch.Generator(device=dev).manual_seed(C + side)
            ring = [tuple((torch.randn(B, C, side, side, device=dev, generator=g) * 3).contiguous(memory_format=torch.channels_last)
                          for _ in range(2)) for _ in range(sets)]
            state = {"i": 0}

            def nxt():
                state["i"] = (state["i"] + 1) % sets
                return ring[state["i"]]

            def chain():
                x, r = nxt()
                v = torch.relu(x + r)
                return holder(v), ops.fq_codes(v, None, None, None, form[2], form[3], form[0], form[1])

            def join():
                x, r = nxt()
                return ops.fq_join(x, *form, residual=r, relu=True)

            state["i"] = -1
            want = chain()
            state["i"] = -1
            got = join()
            assert native.last_launch().startswith("fq_join<")
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].stride() == want[0].stride()
            res = timed([("chain", chain), ("join", join)], iters=200)
            c, j = res["chain"], res["join"]
            print(f"{C} x {side} x {side} batch {B} ({count} joins, ring of {sets}): chain {c[0]:.2f} us ({c[1]:.2f} .. {c[2]:.2f}), "
                  f"join {j[0]:.2f} us ({j[1]:.2f} .. {j[2]:.2f}), {13 * n / j[0] / 1e3:.0f} GB/s", flush=True)
            rows_md.append(f"| {C} | {side} | {count} | {B} | {sets} | {c[0]:.2f} ({c[1]:.2f} .. {c[2]:.2f}) | {j[0]:.2f} ({j[1]:.2f} .. {j[2]:.2f}) | "
                           f"{13 * n / j[0] / 1e3:.0f} | {c[0] / j[0]:.2f} |")
            del ring
            torch.cuda.empty_cache()
    print("\n| channels | image | joins | batch | ring sets | add, ReLU, holder, codes us (least .. most) | join us (least .. most) | join GB/s | chain / join |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)

if "model" in args.sections:
    print("\nwrapped ResNet-50 (workloads.wrapped_resnet50), eager forward, NCHW float32 input")
    print("| batch | arm | wrapped layers on codes | joins | us per forward (least .. most) | max rel diff to as built |\n|---|---|---|---|---|---|")
    with torch.no_grad():
        plain = workloads.wrapped_resnet50()
        arms_of = {"as built": (plain, 0)}
        for name, kw in (("fx, convolutions=True", dict(convolutions=True)),
                         ("fx, convolutions=True, shared_holders=True", dict(convolutions=True, shared_holders=True))):
            arms_of[name] = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(), **kw)
        for B in args.batches:
            x = torch.randn(B, 3, 224, 224, device=dev)
            ref = plain(x)
            diffs = {name: float((m(x) - ref).abs().max() / ref.abs().max()) for name, (m, _) in arms_of.items()}
            res = timed([(name, (lambda m: lambda: m(x))(m)) for name, (m, _) in arms_of.items()], iters=max(1, args.iters // 5))
            for name, (m, n) in arms_of.items():
                r = res[name]
                joins = sum(isinstance(s, consumers.QuantizedJoin) for s in m.modules())
                print(f"| {B} | {name} | {n} | {joins} | {r[0]:.0f} ({r[1]:.0f} .. {r[2]:.0f}) | {diffs[name]:.1e} |", flush=True)
