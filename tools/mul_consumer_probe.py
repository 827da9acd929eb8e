"""What does an elementwise multiply on activation codes cost, and what does it save?  (consumers.QuantizedMul,
fuse_linear_consumers_fx(muls=True); include/mctq_hip.h: mctq_codes_mul_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone on the SE shapes of EfficientNet-B0 and RegNetY (96 x 56 x 56, 144 x 28 x 28, 240 x 14 x 14,
             672 x 7 x 7, 1152 x 7 x 7), channels-last, with the gate [B, C, 1, 1] as codes ("row") and as float32 values coded in
             the kernel ("row f32"), and one same-shape case (two 144 x 28 x 28 tensors), against what it replaces: ATen's float32
             multiply of the two holder outputs, holder M (ops.fq_per_tensor) and one quantize launch of its output
             (ops.fq_codes_nhwc).  Every launch takes the next set of a ring of buffers (at most 16 sets, about 1.2 GB in all);
             outputs compared with torch.equal first
    se       one SE block (conv 1x1 -> ReLU -> A -> {mean((2, 3), keepdim) -> B -> fc1 -> ReLU -> C -> fc2 -> Hardsigmoid -> G} ->
             mul -> M -> conv 1x1, 144 channels on 28 x 28, 48 squeezed) through fuse_linear_consumers_fx with every switch, with
             and without muls=True; torch.equal where it holds, else the largest relative difference (the float32 convolution
             behind M that the consumer replaces rounds its sums); library launches per forward of both
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/mul_consumer_probe.py [--sections kernel se] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mct_quantizers_amd as mq
from mct_quantizers_amd import consumers
from mct_quantizers_amd.hip import native, ops

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "se"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers

# (name, channels, image side, gate form)
MULS = [("efficientnet-b0 se", 96, 56, "row"), ("efficientnet-b0 se", 96, 56, "row f32"), ("efficientnet-b0 se", 144, 28, "row"),
        ("efficientnet-b0 se", 144, 28, "row f32"), ("gated layer", 144, 28, "same"), ("efficientnet-b0 se", 240, 14, "row"),
        ("efficientnet-b0 se", 240, 14, "row f32"), ("efficientnet-b0 se", 672, 7, "row"), ("efficientnet-b0 se", 672, 7, "row f32"),
        ("efficientnet-b0 se", 1152, 7, "row"), ("efficientnet-b0 se", 1152, 7, "row f32")]
RING_BYTES, RING_MAX = 1200 << 20, 16
# (scale, zero point, qmin, qmax) of A (behind a ReLU), of G (behind a hardsigmoid) and of M
A_FORM, G_FORM, OUT = (8.0 / 256, 0, 0, 255), (1.0 / 256, 0, 0, 255), (0.021, 0, 0, 255)


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


class MulCase:
    """A ring of (float32 holder outputs, A's codes, the gate) sets for one multiply, and launchers that take the next set each
    time.  ``gate``: "same" (codes of a's shape), "row" (codes [B, C, 1, 1]) or "row f32" (the holder's float32 input)."""

    def __init__(self, C, side, B, gate):
        self.C, self.B, self.side, self.gate = C, B, side, gate
        self.pixels = B * side * side
        sets = max(1, min(RING_MAX, RING_BYTES // (10 * self.pixels * C)))
        gen = torch.Generator(device=dev).manual_seed(C + side)
        g_shape = (B, C, side, side) if gate == "same" else (B, C, 1, 1)
        self.a, self.g, self.a_codes, self.g_op = [], [], [], []
        for _ in range(sets):
            x = ((torch.rand(B, C, side, side, device=dev, generator=gen) - 0.2) * 9.0).contiguous(memory_format=torch.channels_last)
            v = ((torch.rand(*g_shape, device=dev, generator=gen) * 1.2) - 0.1).contiguous(memory_format=torch.channels_last)
            self.a.append(ops.fq_per_tensor(x, *A_FORM))                              # what holder A writes
            self.g.append(ops.fq_per_tensor(v, *G_FORM))                              # ... and holder G
            self.a_codes.append(ops.fq_codes_nhwc(x, A_FORM[2], A_FORM[3], A_FORM[0], A_FORM[1]))
            self.g_op.append(v.permute(0, 2, 3, 1).contiguous() if gate == "row f32"
                             else ops.fq_codes_nhwc(v, G_FORM[2], G_FORM[3], G_FORM[0], G_FORM[1]))
        self.out = torch.empty((B, side, side, C), dtype=torch.uint8, device=dev)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.a)
        return self.i

    def raw(self):
        i = self.step()
        s, z, qmin, qmax = OUT
        return lib.mctq_codes_mul_nhwc(self.a_codes[i].data_ptr(), native.CODE_U8, A_FORM[0], A_FORM[1], self.g_op[i].data_ptr(),
                                       native.CODE_U8, G_FORM[0], G_FORM[1], int(self.gate == "row f32"), G_FORM[2], G_FORM[3],
                                       0 if self.gate == "same" else self.side * self.side, self.out.data_ptr(), native.CODE_U8,
                                       self.pixels, self.C, s, z, qmin, qmax, S())

    def output(self):
        self.i = -1
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def mul(self):
        i = self.step()
        return self.a[i] * self.g[i]

    def holder(self, t):
        return ops.fq_per_tensor(t, *OUT)

    def quantize(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_codes_nhwc(t, qmin, qmax, s, z)


if "kernel" in args.sections:
    print("\n| multiply | gate | batch | ring sets | codes mul us (least .. most) | GB/s | ATen float32 mul us | holder us | quantize us | "
          "mul + holder + 1 quantize us | replaced / codes mul |")
    print("|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name, C, side, gate in MULS:
        for B in args.batches:
            c = MulCase(C, side, B, gate)
            got = c.output()
            want = c.quantize(c.holder(c.a[0] * c.g[0]))
            assert torch.equal(got, want), (name, gate)      # the launch's codes == codes of the holder behind the float32 product
            t = c.mul()
            h = c.holder(t)
            res = timed([("codes", c.raw), ("mul", c.mul), ("holder", lambda: c.holder(t)), ("quantize", lambda: c.quantize(h)),
                         ("replaced", lambda: c.quantize(c.holder(c.mul())))], iters=100)
            n = c.pixels * C
            print(f"| {name} {C} x {side} x {side} | {gate} | {B} | {len(c.a)} | {fmt(res['codes'])} | "
                  f"{(2 if gate != 'same' else 3) * n / res['codes'][0] / 1e3:.0f} | {fmt(res['mul'])} | {fmt(res['holder'])} | "
                  f"{fmt(res['quantize'])} | {fmt(res['replaced'])} | {res['replaced'][0] / res['codes'][0]:.2f} |", flush=True)
            del c, t, h
            torch.cuda.empty_cache()


def compare(y, ref):
    return "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"


def wrapped(cin, cout, k):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=False).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * cout, per_channel=True, channel_axis=0)
    return mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)


def holder(threshold=8.0, signed=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mq.PytorchActivationQuantizationHolder(
            Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=signed)).to(dev)


class SEBlock(torch.nn.Module):
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


if "se" in args.sections:
    print("\n| model | batch | layers replaced (without / with muls) | library launches per forward | muls=False us (least .. most) | "
          "muls=True us (least .. most) | without / with | outputs |\n|---|---|---|---|---|---|---|---|", flush=True)
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, avg_pools=True, concats=True,
                    fused_residuals=True)
    for B in args.batches:
        x = torch.rand(B, 144, 28, 28, device=dev).contiguous(memory_format=torch.channels_last) * 6.0
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(SEBlock().eval(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(SEBlock().eval(), muls=True, **switches)
            same = compare(gm(x), gm0(x))
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(x)), ("on", lambda: gm(x))], iters=20)
        a, b = res["off"], res["on"]
        print(f"| se block 144 x 28 x 28 | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | {same} |", flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()
