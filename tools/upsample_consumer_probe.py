"""What does a nearest upsample on activation codes cost, and what does it save?  (consumers.QuantizedUpsample,
fuse_linear_consumers_fx(upsamples=True); include/mctq_hip.h: mctq_codes_upsample_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone on 2 x upsamples of 256 x 28 x 28, 128 x 56 x 56 and 64 x 112 x 112 (U-Net / YOLO-neck shapes) and
             one non-integer geometry (128 x 56 x 56 by 1.5: 84 x 84, through the maps), channels-last, against what it replaces:
             ATen's nearest upsample of the float32 holder output, the holder behind it (ops.fq_per_tensor) and one quantize
             launch of its output (ops.fq_codes_nhwc).  Every launch takes the next set of a ring of buffers (at most 16 sets,
             about 1.2 GB in all: cold inputs); outputs compared with torch.equal first
    forms    gather against replicate (tuning key "upsample_form" 1 / 2) on the integer-factor rows, and at factors 4 x 4
    decoder  one decoder stage (conv -> ReLU -> A -> up(x) -> B -> cat([B, S]) -> C -> 3x3 conv, 128 + 128 channels, 28 x 28 ->
             56 x 56) through fuse_linear_consumers_fx with every switch, with and without upsamples=True; torch.equal where it
             holds, else the largest relative difference (the float32 convolutions the consumers replace round their sums)
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/upsample_consumer_probe.py [--sections kernel forms decoder] [--iters 100] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "decoder"])
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, channels, image side, F.interpolate's arguments)
SHAPES = [("2x 256 x 28 x 28", 256, 28, dict(scale_factor=2)), ("2x 128 x 56 x 56", 128, 56, dict(scale_factor=2)),
          ("2x 64 x 112 x 112", 64, 112, dict(scale_factor=2)), ("1.5x 128 x 56 x 56", 128, 56, dict(scale_factor=1.5))]
RING_BYTES, RING_MAX = 1200 << 20, 16
IN, OUT = (8.0 / 256, 0, 0, 255), (0.021, 17, 0, 255)         # holder A's form, holder B's: (scale, zero point, qmin, qmax)


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


class UpsampleCase:
    """A ring of (float32 holder output, its codes) sets for one upsample, and launchers that take the next set each time."""

    def __init__(self, channels, side, B, geometry, factors=None):
        self.B, self.C, self.side, self.geometry = B, channels, side, geometry
        up = consumers.QuantizedUpsample(torch.nn.Upsample(**geometry), quantizer(8.0))
        rows, cols, found = up.index_maps(side, side, dev)
        self.rows, self.cols, self.factors = rows, cols, factors or found
        self.ho, self.wo = rows.numel(), cols.numel()
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * B * channels * side * side)))     # the input as float32 and as codes
        g = torch.Generator(device=dev).manual_seed(channels + side)
        s, z, qmin, qmax = IN
        self.x, self.codes = [], []
        for _ in range(sets):
            x = ((torch.rand(B, channels, side, side, device=dev, generator=g) - 0.3) * 6.0).contiguous(memory_format=torch.channels_last)
            self.x.append(ops.fq_per_tensor(x, s, z, qmin, qmax))                      # what holder A writes
            self.codes.append(ops.fq_codes_nhwc(x, qmin, qmax, s, z))
        self.out = torch.empty((B, self.ho, self.wo, channels), dtype=torch.uint8, device=dev)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self):
        s, z, qmin, qmax = OUT
        fh, fw = self.factors or (0, 0)
        maps = (None, None) if self.factors else (self.rows.data_ptr(), self.cols.data_ptr())
        return lib.mctq_codes_upsample_nhwc(self.codes[self.step()].data_ptr(), self.out.data_ptr(), native.CODE_U8, IN[1], IN[0], self.B,
                                            self.side, self.side, self.C, self.ho, self.wo, fh, fw, *maps, native.CODE_U8, s, z, qmin, qmax, S())

    def output(self):
        self.i = -1
        self.out.zero_()
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def upsample(self):
        return F.interpolate(self.x[self.step()], **self.geometry)

    def holder(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_per_tensor(t, s, z, qmin, qmax)

    def quantize(self, t):
        s, z, qmin, qmax = OUT
        return ops.fq_codes_nhwc(t, qmin, qmax, s, z)


def quantizer(threshold=8.0, signed=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=signed)


if "kernel" in args.sections:
    print("\n| upsample | batch | ring sets | form | codes upsample us (least .. most) | GB/s | ATen upsample float32 us | holder us | "
          "quantize us | upsample + holder + 1 quantize us | replaced / codes upsample | with the feature |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name, channels, side, geometry in SHAPES:
        for B in args.batches:
            c = UpsampleCase(channels, side, B, geometry)
            got = c.output()
            form = "replicate" if "replicate" in native.last_launch() else "gather"      # the launcher's own choice (tuning key 0)
            want = c.quantize(c.holder(F.interpolate(c.x[0], **geometry)))
            assert torch.equal(got, want), name              # the launch's codes == codes of the holder behind ATen's upsample
            t = c.upsample()
            h = c.holder(t)
            res = timed([("codes", c.raw), ("upsample", c.upsample), ("holder", lambda: c.holder(t)), ("quantize", lambda: c.quantize(h)),
                         ("replaced", lambda: c.quantize(c.holder(c.upsample())))])
            n_in, n_out = B * channels * side * side, c.out.numel()
            ratio = res["replaced"][0] / res["codes"][0]
            print(f"| {name} | {B} | {len(c.x)} | {form} | {fmt(res['codes'])} | "
                  f"{(n_in + n_out) / res['codes'][0] / 1e3:.0f} | {fmt(res['upsample'])} | {fmt(res['holder'])} | {fmt(res['quantize'])} | "
                  f"{fmt(res['replaced'])} | {ratio:.2f} | {'faster' if ratio > 1 else 'slower'} |", flush=True)
            del c, t, h, got, want
            torch.cuda.empty_cache()

if "forms" in args.sections:
    print("\n| upsample | batch | gather us (least .. most) | replicate us (least .. most) | gather / replicate | faster form |")
    print("|---|---|---|---|---|---|", flush=True)
    rows = [(n, c, s, g) for n, c, s, g in SHAPES if g["scale_factor"] == 2] + [("4x 128 x 28 x 28", 128, 28, dict(scale_factor=4))]
    try:
        for name, channels, side, geometry in rows:
            for B in args.batches:
                c = UpsampleCase(channels, side, B, geometry)
                assert c.factors is not None
                outs = []
                for form in (1, 2):
                    native.set_tuning("upsample_form", form)
                    outs.append(c.output())
                    assert ("gather", "replicate")[form - 1] in native.last_launch()
                assert torch.equal(*outs), name

                def run(form):
                    native.set_tuning("upsample_form", form)
                    return c.raw()

                res = timed([("gather", lambda: run(1)), ("replicate", lambda: run(2))])
                ratio = res["gather"][0] / res["replicate"][0]
                print(f"| {name} | {B} | {fmt(res['gather'])} | {fmt(res['replicate'])} | {ratio:.2f} | "
                      f"{'replicate' if ratio > 1 else 'gather'} |", flush=True)
                del c, outs
                torch.cuda.empty_cache()
    finally:
        native.set_tuning("upsample_form", 0)


def compare(y, ref):
    return "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"


def wrapped(cin, cout, k):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=False).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * cout, per_channel=True, channel_axis=0)
    return mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)


def holder(threshold=8.0, signed=False):
    return mq.PytorchActivationQuantizationHolder(quantizer(threshold, signed)).to(dev)


class DecoderStage(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.h0 = holder()
        self.first, self.ha = wrapped(256, 128, 1), holder(8.0)
        self.up, self.hb = torch.nn.Upsample(scale_factor=2), holder(16.0)
        self.hs, self.hc = holder(4.0), holder(8.0)
        self.last = wrapped(256, 128, 3)

    def forward(self, x, skip):
        b = self.hb(self.up(self.ha(F.relu(self.first(self.h0(x))))))
        return self.last(self.hc(torch.cat([b, self.hs(skip)], 1)))


if "decoder" in args.sections:
    print("\n| model | batch | layers replaced (without / with upsamples) | library launches per forward | upsamples=False us (least .. most) | "
          "upsamples=True us (least .. most) | without / with | with the feature | outputs |\n|---|---|---|---|---|---|---|---|---|", flush=True)
    switches = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, concats=True, muls=True)
    for B in args.batches:
        x = torch.rand(B, 256, 28, 28, device=dev).contiguous(memory_format=torch.channels_last) * 6.0
        skip = torch.rand(B, 128, 56, 56, device=dev).contiguous(memory_format=torch.channels_last) * 3.0
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(DecoderStage().eval(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(DecoderStage().eval(), upsamples=True, **switches)
            same = compare(gm(x, skip), gm0(x, skip))
            count = lambda g: (native.launch_count(), g(x, skip), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(x, skip)), ("on", lambda: gm(x, skip))], iters=20)
        a, b = res["off"], res["on"]
        print(f"| decoder stage 28 x 28 -> 56 x 56 | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | "
              f"{'faster' if a[0] > b[0] else 'slower'} | {same} |", flush=True)
        del gm, gm0, x, skip
        torch.cuda.empty_cache()
