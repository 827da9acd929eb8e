"""What does a channel concatenation on activation codes cost, and what does it save?  (consumers.QuantizedConcat,
fuse_linear_consumers_fx(concats=True); include/mctq_hip.h: mctq_codes_concat_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel     the launch alone on the concatenations of an Inception 3a block (64 + 128 + 32 + 32 channels, 28 x 28), a Fire
               module's expand layers (128 + 128, 27 x 27) and a decoder stage with a skip connection (64 + 64, 112 x 112),
               channels-last, the operands in four different forms, against what it replaces: torch.cat of the float32 outputs
               of the operand holders, the holder behind it (ops.fq_per_tensor) and one quantize launch of its output
               (ops.fq_codes_nhwc).  Every launch takes the next set of a ring of buffers (at most 16 sets, about 1.2 GB in all);
               outputs compared with torch.equal first.  One more arm: every operand in the output's form (all lanes copy)
    inception  an Inception-3a-shaped block (192 channels in; 1x1 64 | 1x1 96 -> 3x3 128 | 1x1 16 -> 5x5 32 | pool -> 1x1 32;
               ReLU and a holder behind every convolution; cat; holder; the four readers of the next block: three 1x1
               convolutions and a MaxPool2d(3, 1, 1) in front of a fourth) through fuse_linear_consumers_fx(convolutions=True,
               shared_holders=True, stay_on_codes=True, pools=True) with and without concats=True; torch.equal where it holds,
               else the largest relative difference (the float32 convolutions the consumers replace round their sums)
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/concat_consumer_probe.py [--sections kernel inception] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "inception"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, operand channels, image side)
CONCATS = [("inception 3a", (64, 128, 32, 32), 28), ("fire expand", (128, 128), 27), ("decoder skip", (64, 64), 112)]
RING_BYTES, RING_MAX = 1200 << 20, 16
# (scale, zero point, qmin, qmax): the operands' forms in turn, and the form of the holder behind the concatenation
FORMS = [(8.0 / 256, 0, 0, 255), (4.0 / 256, 0, 0, 255), (0.021, 17, 0, 255), (6.0 / 128, 0, -128, 127)]
OUT = (4.0 / 256, 0, 0, 255)


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


class ConcatCase:
    """A ring of (float32 holder outputs, their codes) sets for one concatenation, and launchers that take the next set each
    time.  ``forms``: the operands' forms."""

    def __init__(self, channels, side, B, forms):
        self.channels, self.B, self.side, self.forms = channels, B, side, forms
        self.pixels, self.total = B * side * side, sum(channels)
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * self.pixels * self.total)))
        g = torch.Generator(device=dev).manual_seed(self.total + side)
        self.x, self.codes = [], []
        for _ in range(sets):
            xs, cs = [], []
            for c, (s, z, qmin, qmax) in zip(channels, forms):
                x = ((torch.rand(B, c, side, side, device=dev, generator=g) - 0.3) * 6.0).contiguous(memory_format=torch.channels_last)
                xs.append(ops.fq_per_tensor(x, s, z, qmin, qmax))                      # what the operand's holder writes
                cs.append(ops.fq_codes_nhwc(x, qmin, qmax, s, z))
            self.x.append(xs)
            self.codes.append(cs)
        self.out = torch.empty((B, side, side, self.total), dtype=torch.uint8, device=dev)
        self.items = []
        for cs in self.codes:
            items = (native.ConcatItem * len(cs))()
            for it, c, (s, z, _, _) in zip(items, cs, forms):
                it.codes, it.channels, it.code_dtype, it.zero_point, it.scale = c.data_ptr(), c.shape[-1], ops._code_of(c), z, s
            self.items.append(items)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self):
        s, z, qmin, qmax = OUT
        return lib.mctq_codes_concat_nhwc(self.items[self.step()], len(self.channels), self.out.data_ptr(), native.CODE_U8, self.pixels,
                                          s, z, qmin, qmax, S())

    def output(self):
        self.i = -1
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def cat(self):
        return torch.cat(self.x[self.step()], 1)

    def holder(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_per_tensor(t, s, z, qmin, qmax)

    def quantize(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_codes_nhwc(t, qmin, qmax, s, z)


if "kernel" in args.sections:
    print("\n| concatenation | batch | ring sets | codes concat us (least .. most) | GB/s | all operands copies us | torch.cat float32 us | "
          "holder us | quantize us | cat + holder + 1 quantize us | replaced / codes concat |")
    print("|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name, channels, side in CONCATS:
        for B in args.batches:
            c = ConcatCase(channels, side, B, [FORMS[k % len(FORMS)] for k in range(len(channels))])
            got = c.output()
            want = c.quantize(c.holder(torch.cat(c.x[0], 1)))
            assert torch.equal(got, want), name              # the launch's codes == codes of the holder behind the float32 cat
            copies = ConcatCase(channels, side, B, [OUT] * len(channels))
            assert torch.equal(copies.output(), torch.cat(copies.codes[0], -1)), name
            t = c.cat()
            h = c.holder(t)
            res = timed([("codes", c.raw), ("copies", copies.raw), ("cat", c.cat), ("holder", lambda: c.holder(t)),
                         ("quantize", lambda: c.quantize(h)), ("replaced", lambda: c.quantize(c.holder(c.cat())))], iters=100)
            n = c.pixels * c.total
            print(f"| {name} {' + '.join(map(str, channels))} x {side} x {side} | {B} | {len(c.x)} | {fmt(res['codes'])} | "
                  f"{2 * n / res['codes'][0] / 1e3:.0f} | {fmt(res['copies'])} | {fmt(res['cat'])} | {fmt(res['holder'])} | "
                  f"{fmt(res['quantize'])} | {fmt(res['replaced'])} | {res['replaced'][0] / res['codes'][0]:.2f} |", flush=True)
            del c, copies, t, h
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


class Inception3a(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.h0 = holder()
        self.b1, self.h1 = wrapped(192, 64, 1), holder(8.0)
        self.b2a, self.h2a, self.b2b, self.h2b = wrapped(192, 96, 1), holder(8.0), wrapped(96, 128, 3), holder(16.0)
        self.b3a, self.h3a, self.b3b, self.h3b = wrapped(192, 16, 1), holder(8.0), wrapped(16, 32, 5), holder(4.0)
        self.pool, self.b4, self.h4 = torch.nn.MaxPool2d(3, 1, 1), wrapped(192, 32, 1), holder(8.0)
        self.hc = holder(8.0)
        self.n1, self.n2, self.n3, self.n4 = wrapped(256, 128, 1), wrapped(256, 128, 1), wrapped(256, 32, 1), wrapped(256, 64, 1)
        self.npool = torch.nn.MaxPool2d(3, 1, 1)

    def forward(self, x):
        x = self.h0(x)
        a = self.h1(F.relu(self.b1(x)))
        b = self.h2b(F.relu(self.b2b(self.h2a(F.relu(self.b2a(x))))))
        c = self.h3b(F.relu(self.b3b(self.h3a(F.relu(self.b3a(x))))))
        d = self.h4(F.relu(self.b4(self.pool(x))))
        t = self.hc(torch.cat([a, b, c, d], 1))
        return torch.cat([self.n1(t), self.n2(t), self.n3(t), self.n4(self.npool(t))], 1)


if "inception" in args.sections:
    print("\n| model | batch | layers replaced (without / with concats) | library launches per forward | concats=False us (least .. most) | "
          "concats=True us (least .. most) | without / with | outputs |\n|---|---|---|---|---|---|---|---|", flush=True)
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True)
    for B in args.batches:
        x = torch.rand(B, 192, 28, 28, device=dev).contiguous(memory_format=torch.channels_last) * 6.0
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(Inception3a().eval(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(Inception3a().eval(), concats=True, **switches)
            same = compare(gm(x), gm0(x))
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(x)), ("on", lambda: gm(x))], iters=20)
        a, b = res["off"], res["on"]
        print(f"| inception 3a block, 28 x 28 | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | {same} |", flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()
