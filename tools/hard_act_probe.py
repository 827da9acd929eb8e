"""Which float32 expression do ATen's GPU Hardswish / Hardsigmoid kernels evaluate, and what does folding them into the integer
consumers' epilogues save?  (consumers.qlinear_i8(act=...), qconv_dw_i8(act=...), fuse_linear_consumers_fx(hard_activations=True);
include/mctq_hip.h: mctq_qlinear_i8_act, mctq_qconv_dw_i8_act)

Sections:
    formula  needs only torch.  For each activation and each candidate expression, written with one torch op per IEEE operation
             on the GPU (the divisor and the reciprocal are GPU tensors: ATen turns a division by a Python number into a
             multiplication by its reciprocal), the number of float32 bit patterns, out of all 2^32 in chunks of 2^26, whose
             result differs in bits from F.hardswish / F.hardsigmoid on the GPU (a NaN equals any NaN).  Then the same count of
             ATen's CPU result against its GPU result over every 257th pattern
    sweep    every float32 bit pattern through the bias of mctq_qlinear_i8_act (K = 16, activation codes at the zero point, weights
             0: the epilogue's value is exactly bias[n]), M = 1 and N = 2^20 per launch, uint8 and int8 output forms: the number of
             codes that differ from ops.fq_codes(F.hardswish(bias)) on the GPU
    time     conv 1x1 -> Hardswish -> holder -> conv 1x1 and conv 1x1 -> Hardswish -> holder -> depthwise 3x3 -> Hardswish ->
             holder -> conv 1x1 at MobileNetV3-Large shapes (16 x 112 x 112, 72 x 56 x 56, 120 x 28 x 28, 480 x 14 x 14,
             960 x 7 x 7; channels padded up to a multiple of 16), the SE gate of tools/mul_consumer_probe.py, and one whole-tile
             product (4096 x 4096 x 256) where act sends the call to the tiled kernel, against the register-pinned launch + ATen's
             activation + the quantize launch it replaces.  Arms alternate round by round in one process; median and spread
             (least .. most) of the rounds; outputs compared with torch.equal first
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/hard_act_probe.py [--sections formula sweep time] [--iters 20] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["formula", "sweep", "time"])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

dev = torch.device("cuda")
CHUNK = 1 << 26


def patterns(start, count, step=1):
    """float32 tensor on the GPU holding the bit patterns start, start + step, ... (count of them)"""
    bits = (torch.arange(count, dtype=torch.int64, device=dev) * step + start) & 0xFFFFFFFF
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)


def differing(a, b):
    """number of elements whose bits differ, a NaN equal to any NaN"""
    return int(((a.view(torch.int32) != b.view(torch.int32)) & ~(a.isnan() & b.isnan())).sum())


if "formula" in args.sections:
    c = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)      # noqa: E731
    zero, three, six, sixth = c(0.0), c(3.0), c(6.0), torch.tensor(1.0, dtype=torch.float32) / torch.tensor(6.0, dtype=torch.float32)
    sixth = sixth.to(dev)
    ramp = lambda x: torch.minimum(torch.maximum(torch.add(x, three), zero), six)      # noqa: E731
    CANDIDATES = {
        "hardswish": [("x * min(max(x + 3, 0), 6) / 6", lambda x: torch.div(torch.mul(x, ramp(x)), six)),
                      ("x * min(max(x + 3, 0), 6) * (1 / 6)", lambda x: torch.mul(torch.mul(x, ramp(x)), sixth)),
                      ("x * (min(max(x + 3, 0), 6) / 6)", lambda x: torch.mul(x, torch.div(ramp(x), six))),
                      ("x * (min(max(x + 3, 0), 6) * (1 / 6))", lambda x: torch.mul(x, torch.mul(ramp(x), sixth))),
                      ("(x / 6) * min(max(x + 3, 0), 6)", lambda x: torch.mul(torch.div(x, six), ramp(x))),
                      ("(x * (1 / 6)) * min(max(x + 3, 0), 6)", lambda x: torch.mul(torch.mul(x, sixth), ramp(x)))],
        "hardsigmoid": [("min(max(x + 3, 0), 6) / 6", lambda x: torch.div(ramp(x), six)),
                        ("min(max(x + 3, 0), 6) * (1 / 6)", lambda x: torch.mul(ramp(x), sixth)),
                        ("min(max(x / 6 + 0.5, 0), 1)", lambda x: torch.minimum(torch.maximum(
                            torch.add(torch.div(x, six), c(0.5)), zero), c(1.0))),
                        ("min(max(x * (1 / 6) + 0.5, 0), 1)", lambda x: torch.minimum(torch.maximum(
                            torch.add(torch.mul(x, sixth), c(0.5)), zero), c(1.0)))],
    }
    ATEN = {"hardswish": F.hardswish, "hardsigmoid": F.hardsigmoid}
    print(f"\ntorch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    print("\n| activation | candidate (one torch op per operation, GPU) | bit patterns differing from ATen GPU, of 2^32 |\n|---|---|---|",
          flush=True)
    for kind, cands in CANDIDATES.items():
        miss = [0] * len(cands)
        for start in range(0, 1 << 32, CHUNK):
            x = patterns(start, CHUNK)
            want = ATEN[kind](x)
            for i, (_, f) in enumerate(cands):
                miss[i] += differing(f(x), want)
        for (name, _), m in zip(cands, miss):
            print(f"| {kind} | {name} | {m} |", flush=True)
    print("\n| activation | ATen CPU against ATen GPU, every 257th bit pattern: differing / compared |\n|---|---|", flush=True)
    for kind, f in ATEN.items():
        n = (1 << 32) // 257 + 1
        x = patterns(0, n, 257)
        print(f"| {kind} | {differing(f(x.cpu()), f(x).cpu())} / {n} |", flush=True)

if "sweep" in args.sections or "time" in args.sections:
    import mct_quantizers_amd as mq
    from mct_quantizers_amd import consumers
    from mct_quantizers_amd.hip import native, ops
    Q = mq.pytorch_quantizers
    ACTS = ("hardswish", "hardsigmoid")
    # the output forms of tests/test_hard_act_consumer.py
    OUT_FORMS = {"hardswish": {"u8": (0.02, 10, 0, 255), "i8": (0.03, -120, -128, 127)},
                 "hardsigmoid": {"u8": (1.0 / 256, 0, 0, 255), "i8": (1.0 / 256, -128, -128, 127)}}

    def chain_codes(y, act, form):
        return ops.fq_codes(getattr(F, act)(y), None, None, None, form[2], form[3], form[0], form[1])


if "sweep" in args.sections:
    N, K = 1 << 20, 16
    w = torch.zeros((N, K), dtype=torch.int8, device=dev)
    rowsum, ws = torch.zeros(N, dtype=torch.int32, device=dev), torch.ones(N, dtype=torch.float32, device=dev)
    print("\n| activation | output form | float32 bit patterns through the bias | codes differing from the GPU chain |\n|---|---|---|---|",
          flush=True)
    for kind in ("u8", "i8"):
        za = 114 if kind == "u8" else -5
        a = torch.full((1, K), za, dtype=torch.uint8 if kind == "u8" else torch.int8, device=dev)
        miss = {act: 0 for act in ACTS}
        for start in range(0, 1 << 32, N):
            bias = patterns(start, N)
            y = consumers.qlinear_i8(a, za, 0.5, w, ws, rowsum, bias)
            for act in ACTS:
                form = OUT_FORMS[act][kind]
                got = consumers.qlinear_i8(a, za, 0.5, w, ws, rowsum, bias, form, act=act)
                miss[act] += int((got != chain_codes(y, act, form)).sum())
        for act in ACTS:
            print(f"| {act} | {kind} {OUT_FORMS[act][kind]} | {1 << 32} | {miss[act]} |", flush=True)
    del w, rowsum, ws
    torch.cuda.empty_cache()


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


def fmt(r):
    return f"{r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f})"


def wrapped(cin, cout, k, groups=1):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, groups=groups, bias=False).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * cout, per_channel=True, channel_axis=0)
    return mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)


def holder(threshold=8.0, signed=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mq.PytorchActivationQuantizationHolder(
            Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=signed)).to(dev)


class Block(torch.nn.Module):
    """conv 1x1 -> Hardswish -> holder -> [depthwise 3x3 -> Hardswish -> holder ->] conv 1x1"""

    def __init__(self, C, depthwise):
        super().__init__()
        torch.manual_seed(0)
        self.h0, self.c1, self.a1, self.h1 = holder(4.0, True), wrapped(C, C, 1), torch.nn.Hardswish(), holder(4.0, True)
        self.dw = wrapped(C, C, 3, groups=C) if depthwise else None
        self.a2, self.h2, self.c2 = torch.nn.Hardswish(), holder(4.0, True), wrapped(C, C, 1)

    def forward(self, x):
        x = self.h1(self.a1(self.c1(self.h0(x))))
        if self.dw is not None:
            x = self.h2(self.a2(self.dw(x)))
        return self.c2(x)


class SEBlock(torch.nn.Module):
    """tools/mul_consumer_probe.py's SE block"""

    def __init__(self, C=144, squeezed=48):
        super().__init__()
        torch.manual_seed(0)
        self.h0, self.c, self.a = holder(), wrapped(C, C, 1), holder(8.0)
        self.b, self.fc1, self.hc, self.fc2 = holder(4.0), wrapped(C, squeezed, 1), holder(4.0), wrapped(squeezed, C, 1)
        self.gate, self.g = torch.nn.Hardsigmoid(), holder(1.0)
        self.m, self.last = holder(8.0), wrapped(C, C, 1)

    def forward(self, x):
        a = self.a(torch.relu(self.c(self.h0(x))))
        s = self.b(a.mean((2, 3), keepdim=True))
        g = self.g(self.gate(self.fc2(self.hc(torch.relu(self.fc1(s))))))
        return self.last(self.m(a * g))


if "time" in args.sections:
    switches = dict(convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True, pools=True, avg_pools=True,
                    concats=True, fused_residuals=True, muls=True)
    pad16 = lambda c: (c + 15) // 16 * 16      # noqa: E731
    models = [(f"{'depthwise' if d else 'pointwise'} {pad16(C)} x {side} x {side}", (lambda C=C, d=d: Block(pad16(C), d)), pad16(C), side)
              for d in (False, True) for C, side in ((16, 112), (72, 56), (120, 28), (480, 14), (960, 7))]
    models.append(("se block 144 x 28 x 28", SEBlock, 144, 28))
    print("\n| model | batch | library launches per forward (off / on) | hard_activations=False us (least .. most) | "
          "hard_activations=True us (least .. most) | off / on | outputs |\n|---|---|---|---|---|---|---|", flush=True)
    for name, make, C, side in models:
        for B in args.batches:
            x = (torch.randn(B, C, side, side, device=dev) * 1.5).contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                gm0, _ = consumers.fuse_linear_consumers_fx(make().eval(), **switches)
                gm, _ = consumers.fuse_linear_consumers_fx(make().eval(), hard_activations=True, **switches)
                same = "torch.equal" if torch.equal(gm(x), gm0(x)) else "DIFFERENT"
                count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
                l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
                res = timed([("off", lambda: gm0(x)), ("on", lambda: gm(x))])
            a, b = res["off"], res["on"]
            print(f"| {name} | {B} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | {same} |", flush=True)
            del gm, gm0, x
            torch.cuda.empty_cache()

    # one whole-tile product: the activation form on the tiled kernel against the register-pinned launch + ATen + quantize
    M, N, K = 4096, 4096, 256
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randint(0, 256, (M, K), generator=g, device=dev).to(torch.uint8)
    w = torch.randint(-128, 128, (N, K), generator=g, device=dev).to(torch.int8)
    ws = ((torch.rand(N, generator=g, device=dev) + 0.5) * (4.0 / (0.02 * 5476.0 * 16))).float()
    bias = ((torch.rand(N, generator=g, device=dev) - 0.5) * 4).float()
    rowsum = w.sum(dim=1, dtype=torch.int32)
    form = OUT_FORMS["hardswish"]["u8"]
    plain = lambda: consumers.qlinear_i8(a, 114, 0.02, w, ws, rowsum, bias)                             # noqa: E731
    folded = lambda: consumers.qlinear_i8(a, 114, 0.02, w, ws, rowsum, bias, form, act="hardswish")      # noqa: E731
    y = plain()
    plain_note = native.last_launch()
    got = folded()
    folded_note = native.last_launch()
    assert torch.equal(got, chain_codes(y, "hardswish", form))
    h = F.hardswish(y)
    res = timed([("folded", folded), ("plain", plain), ("aten", lambda: F.hardswish(y)), ("quantize", lambda: chain_codes(y, "hardswish", form)),
                 ("replaced", lambda: chain_codes(plain(), "hardswish", form))], iters=20)
    print("\n| product | folded launch | us (least .. most) | plain launch | us | ATen hardswish us | hardswish + quantize us | "
          "plain + hardswish + quantize us | replaced / folded |\n|---|---|---|---|---|---|---|---|---|")
    print(f"| {M} x {N} x {K} | {folded_note} | {fmt(res['folded'])} | {plain_note} | {fmt(res['plain'])} | {fmt(res['aten'])} | "
          f"{fmt(res['quantize'])} | {fmt(res['replaced'])} | {res['replaced'][0] / res['folded'][0]:.2f} |", flush=True)
    del h
