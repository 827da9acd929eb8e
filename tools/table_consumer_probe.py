"""What does an elementwise activation on activation codes cost as a byte table, and what does it save?
(consumers.QuantizedActivationTable, fuse_linear_consumers_fx(activation_tables=True); include/mctq_hip.h: mctq_codes_table)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone, SiLU on EfficientNet-B0's activation shapes (32 x 112 x 112, 96 x 112 x 112, 144 x 56 x 56,
             240 x 28 x 28, 672 x 14 x 14, 1152 x 7 x 7) and GELU on 3072 x 196 (a ViT-B MLP), channels-last, against what it
             replaces: ATen's f on the float32 holder output, the holder behind it (ops.fq_per_tensor) and one quantize launch of
             its output (ops.fq_codes).  Every launch takes the next set of a ring of buffers (at most 16 sets, about 1.2 GB in
             all: cold inputs); outputs compared with torch.equal first
    chunks   16-byte chunks per lane, tuning key "table_chunks" 1 / 2 / 4, on the same rows, same buffers
    block    one MBConv-style block (1x1 48 -> 144, A, SiLU, B, depthwise 3x3, A, SiLU, B, 1x1 144 -> 48, 56 x 56) through
             fuse_linear_consumers_fx with every switch, with and without activation_tables=True; the outputs must be torch.equal
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No time is fixed in advance: the condition
is that every batch-64 row of ``kernel`` is faster than the replaced chain measured next to it; the last line says whether it held.

    python tools/table_consumer_probe.py [--sections kernel chunks block] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "chunks", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, activation, shape behind the batch); 4-D shapes are channels-last
SHAPES = [("SiLU 32 x 112 x 112", torch.nn.SiLU, (32, 112, 112)), ("SiLU 96 x 112 x 112", torch.nn.SiLU, (96, 112, 112)),
          ("SiLU 144 x 56 x 56", torch.nn.SiLU, (144, 56, 56)), ("SiLU 240 x 28 x 28", torch.nn.SiLU, (240, 28, 28)),
          ("SiLU 672 x 14 x 14", torch.nn.SiLU, (672, 14, 14)), ("SiLU 1152 x 7 x 7", torch.nn.SiLU, (1152, 7, 7)),
          ("GELU 196 x 3072", torch.nn.GELU, (196, 3072))]
RING_BYTES, RING_MAX = 1200 << 20, 16
IN, OUT = (8.0 / 128, 0, -128, 127), (0.033, -119, -128, 127)  # holder A's form, holder B's: (scale, zero point, qmin, qmax)


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


class TableCase:
    """A ring of (float32 holder output, its codes) sets for one activation, and launchers that take the next set each time."""

    def __init__(self, fn, shape, B):
        self.fn = fn
        n = B * int(np.prod(shape))
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * n)))              # the input as float32 and as codes
        g = torch.Generator(device=dev).manual_seed(n % 9973)
        s, z, qmin, qmax = IN
        self.x, self.codes = [], []
        for _ in range(sets):
            x = torch.randn(B, *shape, device=dev, generator=g) * 2.0
            if x.dim() == 4:
                x = x.contiguous(memory_format=torch.channels_last)
            self.x.append(ops.fq_per_tensor(x, s, z, qmin, qmax))        # what holder A writes
            self.codes.append(ops.fq_codes(x, None, None, None, qmin, qmax, s, z))
        self.table = ops.code_table(fn, IN, OUT, dev)
        self.out = torch.empty_like(self.codes[0])
        self.n, self.i = n, 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self):
        return lib.mctq_codes_table(self.codes[self.step()].data_ptr(), native.CODE_I8, self.out.data_ptr(), native.CODE_I8, self.n,
                                    self.table.data_ptr(), S())

    def output(self):
        self.i = -1
        self.out.zero_()
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def f(self):
        return self.fn(self.x[self.step()])

    def holder(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_per_tensor(t, s, z, qmin, qmax)

    def quantize(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_codes(t, None, None, None, qmin, qmax, s, z)


def quantizer(threshold=8.0, signed=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=signed)


held = True
if "kernel" in args.sections:
    print("\n| activation | batch | ring sets | codes table us (least .. most) | GB/s | ATen f float32 us | holder us | quantize us | "
          "f + holder + 1 quantize us | replaced / codes table | with the feature |")
    print("|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    with torch.no_grad():
        for name, act, shape in SHAPES:
            for B in args.batches:
                c = TableCase(act(), shape, B)
                got = c.output()
                want = c.quantize(c.holder(c.fn(c.x[0])))
                assert torch.equal(got, want), name           # the launch's codes == codes of the holder behind ATen's f
                t = c.f()
                h = c.holder(t)
                res = timed([("codes", c.raw), ("f", c.f), ("holder", lambda: c.holder(t)), ("quantize", lambda: c.quantize(h)),
                             ("replaced", lambda: c.quantize(c.holder(c.f())))])
                ratio = res["replaced"][0] / res["codes"][0]
                if B >= 64 and ratio <= 1:
                    held = False
                print(f"| {name} | {B} | {len(c.x)} | {fmt(res['codes'])} | {2 * c.n / res['codes'][0] / 1e3:.0f} | {fmt(res['f'])} | "
                      f"{fmt(res['holder'])} | {fmt(res['quantize'])} | {fmt(res['replaced'])} | {ratio:.2f} | "
                      f"{'faster' if ratio > 1 else '**slower**'} |", flush=True)
                del c, t, h, got, want
                torch.cuda.empty_cache()
    print(f"\nevery batch-64 row faster than the replaced chain: {held}", flush=True)

if "chunks" in args.sections:
    print("\n| activation | batch | 1 chunk per lane us (least .. most) | 2 chunks us (least .. most) | 4 chunks us (least .. most) | "
          "fastest |")
    print("|---|---|---|---|---|---|", flush=True)
    try:
        with torch.no_grad():
            for name, act, shape in SHAPES:
                for B in args.batches:
                    c = TableCase(act(), shape, B)
                    outs = []
                    for chunks in (1, 2, 4):
                        native.set_tuning("table_chunks", chunks)
                        outs.append(c.output())
                        assert f"U={chunks}," in native.last_launch()
                    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), name

                    def run(chunks):
                        native.set_tuning("table_chunks", chunks)
                        return c.raw()

                    res = timed([("1", lambda: run(1)), ("2", lambda: run(2)), ("4", lambda: run(4))])
                    best = min(res, key=lambda k: res[k][0])
                    print(f"| {name} | {B} | {fmt(res['1'])} | {fmt(res['2'])} | {fmt(res['4'])} | {best} |", flush=True)
                    del c, outs
                    torch.cuda.empty_cache()
    finally:
        native.set_tuning("table_chunks", 4)


def wrapped(cin, cout, k, groups=1):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, groups=groups, bias=False).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * cout, per_channel=True, channel_axis=0)
    return mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)


def holder(threshold=8.0, signed=False):
    return mq.PytorchActivationQuantizationHolder(quantizer(threshold, signed)).to(dev)


class MBConv(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.h0 = holder(4.0, True)
        self.expand, self.a1, self.f1, self.b1 = wrapped(48, 144, 1), holder(8.0, True), torch.nn.SiLU(), holder(8.0, True)
        self.dw, self.a2, self.f2, self.b2 = wrapped(144, 144, 3, groups=144), holder(8.0, True), torch.nn.SiLU(), holder(8.0, True)
        self.project = wrapped(144, 48, 1)

    def forward(self, x):
        x = self.b1(self.f1(self.a1(self.expand(self.h0(x)))))
        x = self.b2(self.f2(self.a2(self.dw(x))))
        return self.project(x)


if "block" in args.sections:
    print("\n| model | batch | layers replaced (without / with activation_tables) | library launches per forward | "
          "activation_tables=False us (least .. most) | activation_tables=True us (least .. most) | without / with | with the feature | "
          "outputs |\n|---|---|---|---|---|---|---|---|---|", flush=True)
    switches = dict(convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True, pools=True, concats=True, muls=True)
    for B in args.batches:
        x = (torch.randn(B, 48, 56, 56, device=dev) * 1.5).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(MBConv().eval(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(MBConv().eval(), activation_tables=True, **switches)
            assert torch.equal(gm(x), gm0(x))                 # the condition: bit for bit
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(x)), ("on", lambda: gm(x))], iters=20)
        a, b = res["off"], res["on"]
        print(f"| MBConv 48 -> 144 -> 48, 56 x 56 | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | "
              f"{'faster' if a[0] > b[0] else '**slower**'} | torch.equal |", flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()
