"""What does a bilinear upsample on activation codes cost, and what does it save?  (consumers.QuantizedBilinearUpsample,
fuse_linear_consumers_fx(bilinear_upsamples=True); include/mctq_hip.h: mctq_codes_upsample_bilinear_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone (the launcher's own strip) on 2 x upsamples of 256 x 28 x 28, 128 x 56 x 56 and 64 x 112 x 112 and a
             4 x upsample of 128 x 28 x 28 (segmentation-head shapes), channels-last, against the float32 chain it replaces: A's
             fake-quant (ops.fq_per_tensor), ATen's bilinear upsample of its output, B's fake-quant.  Every launch takes the next
             set of a ring of buffers (at most 16 sets, about 1.2 GB in all: cold inputs).  The scales are powers of two and the
             weights dyadic, so the launch's codes are compared with the chain's with torch.equal first
    strips   every strip length (tuning key "bilinear_strip" 1 / 4 / 8) on the same rows, outputs compared with torch.equal
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/bilinear_consumer_probe.py [--sections kernel strips] [--iters 100] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "strips"])
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
F = torch.nn.functional

# (name, channels, image side, scale factor)
SHAPES = [("2x 256 x 28 x 28", 256, 28, 2), ("2x 128 x 56 x 56", 128, 56, 2), ("2x 64 x 112 x 112", 64, 112, 2), ("4x 128 x 28 x 28", 128, 28, 4)]
STRIPS = (1, 4, 8)
RING_BYTES, RING_MAX = 1200 << 20, 16
IN, OUT = (8.0 / 256, 0, 0, 255), (16.0 / 256, 0, 0, 255)     # holder A's form, holder B's: (scale, zero point, qmin, qmax)


def timed(arms):
    """arms: [(name, f())] -> {name: (median us, least us, most us)}, rounds alternating between the arms"""
    times = {name: [] for name, _ in arms}
    for name, f in arms:                                      # warm every arm before any timed window
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, f in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000 / args.iters)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in times.items()}


def fmt(r):
    return f"{r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f})"


class BilinearCase:
    """A ring of (float32 input of holder A, A's codes) sets for one upsample, and launchers that take the next set each time."""

    def __init__(self, channels, side, B, factor):
        self.B, self.C, self.side, self.factor = B, channels, side, factor
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            q = mq.pytorch_quantizers.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False)
        up = consumers.QuantizedBilinearUpsample(torch.nn.Upsample(scale_factor=factor, mode="bilinear"), q, q)
        self.tables = [t for axis in up.tables(side, side, dev) for t in axis]
        self.ho = self.wo = side * factor
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * B * channels * side * side)))     # the input as float32 and as codes
        g = torch.Generator(device=dev).manual_seed(channels + side)
        s, z, qmin, qmax = IN
        self.x, self.codes = [], []
        for _ in range(sets):
            x = ((torch.rand(B, channels, side, side, device=dev, generator=g) - 0.3) * 6.0).contiguous(memory_format=torch.channels_last)
            self.x.append(x)
            self.codes.append(ops.fq_codes_nhwc(x, qmin, qmax, s, z))
        self.out = torch.empty((B, self.ho, self.wo, channels), dtype=torch.uint8, device=dev)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self):
        s, z, qmin, qmax = OUT
        return lib.mctq_codes_upsample_bilinear_nhwc(self.codes[self.step()].data_ptr(), self.out.data_ptr(), native.CODE_U8, IN[1], IN[0],
                                                     self.B, self.side, self.side, self.C, self.ho, self.wo,
                                                     *(t.data_ptr() for t in self.tables), native.CODE_U8, s, z, qmin, qmax, S())

    def output(self):
        self.i = -1
        self.out.zero_()
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def chain(self):
        """What the launch replaces: A's fake-quant, ATen's bilinear upsample, B's fake-quant, all float32."""
        a = ops.fq_per_tensor(self.x[self.step()], *IN)
        return ops.fq_per_tensor(F.interpolate(a, scale_factor=self.factor, mode="bilinear"), *OUT)


def cases():
    for name, channels, side, factor in SHAPES:
        for B in args.batches:
            yield name, B, BilinearCase(channels, side, B, factor)
            torch.cuda.empty_cache()


if "kernel" in args.sections:
    print("\n| upsample | batch | ring sets | strip (auto) | codes bilinear us (least .. most) | GB/s | float32 chain A, ATen bilinear, B us | "
          "chain / codes bilinear | with the feature |")
    print("|---|---|---|---|---|---|---|---|---|", flush=True)
    for name, B, c in cases():
        got = c.output()
        strip = native.last_launch().split("strip ")[1].split(",")[0]       # the launcher's own choice (tuning key 0)
        c.i = -1
        s, z, qmin, qmax = OUT
        want = ops.fq_codes_nhwc(c.chain(), qmin, qmax, s, z)
        assert torch.equal(got, want), name                  # dyadic weights, power-of-two scales: the chain's codes bit for bit
        res = timed([("codes", c.raw), ("chain", c.chain)])
        ratio = res["chain"][0] / res["codes"][0]
        print(f"| {name} | {B} | {len(c.x)} | {strip} | {fmt(res['codes'])} | {(c.codes[0].numel() + c.out.numel()) / res['codes'][0] / 1e3:.0f} | "
              f"{fmt(res['chain'])} | {ratio:.2f} | {'faster' if ratio > 1 else 'slower'} |", flush=True)
        del c, got, want

if "strips" in args.sections:
    print("\n| upsample | batch | " + " | ".join(f"strip {r} us (least .. most)" for r in STRIPS) + " | strip 1 / strip 4 | strip 1 / strip 8 | "
          "fastest | auto |")
    print("|---|---|---|---|---|---|---|---|---|", flush=True)
    try:
        for name, B, c in cases():
            native.set_tuning("bilinear_strip", 0)
            c.output()
            auto = native.last_launch().split("strip ")[1].split(",")[0]
            outs = []
            for r in STRIPS:
                native.set_tuning("bilinear_strip", r)
                outs.append(c.output())
            assert all(torch.equal(outs[0], o) for o in outs[1:]), name

            def run(r, c=c):
                native.set_tuning("bilinear_strip", r)
                return c.raw()

            res = timed([(r, lambda r=r: run(r)) for r in STRIPS])
            best = min(STRIPS, key=lambda r: res[r][0])
            print(f"| {name} | {B} | " + " | ".join(fmt(res[r]) for r in STRIPS) + f" | {res[1][0] / res[4][0]:.2f} | "
                  f"{res[1][0] / res[8][0]:.2f} | {best} | {auto} |", flush=True)
            del c, outs
    finally:
        native.set_tuning("bilinear_strip", 0)
