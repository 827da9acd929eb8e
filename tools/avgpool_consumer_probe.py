"""What does an average pool on activation codes cost, and what does it save?  (consumers.QuantizedAvgPool2d,
fuse_linear_consumers*(avg_pools=True); include/mctq_hip.h: mctq_codes_avgpool_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel    the launch alone -- in the lane form, in the split form (tuning key "avgpool_form") and as the launcher chooses -- on
              ResNet-50's 7 x 7 x 2048 head, MobileNetV2's 7 x 7 x 1280 head, SE squeezes over 56 x 56 x 64 and 14 x 14 x 256 (all
              global) and Inception's 3 x 3 stride 1 padding 1 branch on 35 x 35 x 192, against what it replaces: ATen's float32
              average pool of the channels-last holder output, holder B on the result (ops.fq_per_tensor) and one quantize launch
              (ops.fq_codes).  Every launch takes the next set of a ring of buffers (at most 16 sets, about 1.2 GB in all); the
              forms' outputs are compared with torch.equal first, and with the codes of the float32 chain (they may differ by one
              code next to a rounding tie where the window's count is no power of two: the count of differing elements is printed)
    forms     where the launcher's rule comes from: the lane form against the split form alone, on global k x k pools (9 to 196
              taps) of 2048 and of 64 channels at batches from 1 to 4096 (1 to 2048 workgroups of the lane form), codes only
    resnet50  workloads.wrapped_resnet50(pooled_holder=True) through fuse_linear_consumers_fx with every switch, with and without
              avg_pools=True, at 224 x 224
    head      a MobileNet-style head by itself: holder -> conv 1 x 1 (320 -> 1280) -> ReLU6 -> holder -> AdaptiveAvgPool2d(1) ->
              holder -> Flatten -> Linear(1280, 1000) on 7 x 7 maps, same switches
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/avgpool_consumer_probe.py [--sections kernel forms resnet50 head] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "resnet50", "head"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, channels, image side, kernel (None: global), stride, padding)
POOLS = [("resnet50 head", 2048, 7, None, None, 0), ("mobilenetv2 head", 1280, 7, None, None, 0), ("SE squeeze", 64, 56, None, None, 0),
         ("SE squeeze", 256, 14, None, None, 0), ("inception branch", 192, 35, 3, 1, 1)]
RING_BYTES, RING_MAX = 1200 << 20, 16
FORM = (8.0 / 256, 0, 0, 255)                               # the unsigned holder behind a ReLU, in front of the pool and behind it


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


class PoolCase:
    """A ring of (float32 holder output, its codes) sets for one pool shape, and launchers that take the next set each time."""

    def __init__(self, C, side, k, s, p, B, chain=True):
        self.k, self.s, self.p, self.B, self.C, self.side = k or side, s or k or side, p, B, C, side
        self.so = ops._pool_out_size(side, self.k, self.s, p, 1, False)
        n_in = B * C * side * side
        sets = max(1, min(RING_MAX, RING_BYTES // ((5 if chain else 1) * n_in)))
        g = torch.Generator(device=dev).manual_seed(C + side)
        scale, zp, qmin, qmax = FORM
        self.out = torch.empty((B, self.so, self.so, C), dtype=torch.uint8, device=dev)
        self.i = 0
        if not chain:                                         # the codes alone
            self.codes = [torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
            self.x = self.codes
            return
        self.x = [(torch.rand(B, C, side, side, device=dev, generator=g) * 9.0 - 0.5).contiguous(memory_format=torch.channels_last)
                  for _ in range(sets)]
        self.x = [ops.fq_per_tensor(x, scale, zp, qmin, qmax) for x in self.x]        # what holder A writes
        self.codes = [ops.fq_codes_nhwc(x, qmin, qmax, scale, zp) for x in self.x]

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self):
        scale, zp, qmin, qmax = FORM
        c = self.codes[self.step()]
        return lib.mctq_codes_avgpool_nhwc(c.data_ptr(), self.out.data_ptr(), native.CODE_U8, zp, scale, self.B, self.side, self.side, self.C,
                                           self.k, self.k, self.s, self.s, self.p, self.p, 0, 1, 0, self.so, self.so,
                                           native.CODE_U8, scale, zp, qmin, qmax, S())

    def output(self, form):
        native.set_tuning("avgpool_form", form)
        self.i = -1
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        native.set_tuning("avgpool_form", 0)
        return self.out.clone(), native.last_launch()

    def float_chain(self, first=False):
        """ATen's pool of holder A's output, holder B, one quantize launch."""
        scale, zp, qmin, qmax = FORM
        pooled = F.avg_pool2d(self.x[0 if first else self.step()], self.k, self.s, self.p)
        return ops.fq_codes(ops.fq_per_tensor(pooled, scale, zp, qmin, qmax), None, None, None, qmin, qmax, scale, zp)


def forced(form, f):
    def g():
        native.set_tuning("avgpool_form", form)
        return f()
    return g


if "kernel" in args.sections:
    print("\n| pool | batch | ring sets | lane form us (least .. most) | split form us (least .. most) | as chosen us | chosen | "
          "ATen float32 pool + holder + quantize us | replaced / as chosen | elements off the float32 chain by one code |")
    print("|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for (name, C, side, k, s, p) in POOLS:
        for B in args.batches:
            c = PoolCase(C, side, k, s, p, B)
            lane, _ = c.output(1)
            split, _ = c.output(2)
            auto, chosen = c.output(0)
            assert torch.equal(lane, split) and torch.equal(lane, auto), name
            chain = c.float_chain(first=True).permute(0, 2, 3, 1)
            diff = (lane.to(torch.int16) - chain.to(torch.int16)).abs()
            assert int(diff.max()) <= 1, name
            try:
                res = timed([("lane", forced(1, c.raw)), ("split", forced(2, c.raw)), ("auto", forced(0, c.raw)), ("chain", c.float_chain)],
                            iters=100)
            finally:
                native.set_tuning("avgpool_form", 0)
            kind = "global" if k is None else f"{k}x{k}/{s}"
            print(f"| {name} {C} x {side} x {side}, {kind} | {B} | {len(c.x)} | {fmt(res['lane'])} | {fmt(res['split'])} | {fmt(res['auto'])} | "
                  f"{'split' if 'split' in chosen else 'lane'} | {fmt(res['chain'])} | {res['chain'][0] / res['auto'][0]:.2f} | "
                  f"{int((diff != 0).sum())} of {diff.numel()} |", flush=True)
            del c
            torch.cuda.empty_cache()


if "forms" in args.sections:
    print("\n| global pool | taps | batch | output chunks | lane-form workgroups | ring sets | lane form us (least .. most) | "
          "split form us (least .. most) | lane / split |")
    print("|---|---|---|---|---|---|---|---|---|", flush=True)
    for C, batches in ((2048, (1, 64, 512, 4096)), (64, (64, 4096))):
        for side in (3, 4, 5, 7, 14):
            for B in batches:
                if B * C * side * side > (600 << 20):
                    continue
                c = PoolCase(C, side, None, None, 0, B, chain=False)
                assert torch.equal(c.output(1)[0], c.output(2)[0])
                try:
                    res = timed([("lane", forced(1, c.raw)), ("split", forced(2, c.raw))], iters=100)
                finally:
                    native.set_tuning("avgpool_form", 0)
                chunks = B * C // 16
                print(f"| {C} x {side} x {side} | {side * side} | {B} | {chunks} | {(chunks + 255) // 256} | {len(c.x)} | {fmt(res['lane'])} | "
                      f"{fmt(res['split'])} | {res['lane'][0] / res['split'][0]:.2f} |", flush=True)
                del c
                torch.cuda.empty_cache()


def compare(y, ref):
    return "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"


EVERY = dict(convolutions=True, shared_holders=True, stay_on_codes=True, pools=True, fused_residuals=True)


def model_rows(name, make, make_x, batches, iters):
    for B in batches:
        x = make_x(B)
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(make(), **EVERY)
            gm, n = consumers.fuse_linear_consumers_fx(make(), avg_pools=True, **EVERY)
            same = compare(gm(x), gm0(x))
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("avg_pools=False", lambda: gm0(x)), ("avg_pools=True", lambda: gm(x))], iters=iters)
        a, b = res["avg_pools=False"], res["avg_pools=True"]
        slower = b[0] - a[0] > max(a[2] - a[1], b[2] - b[1])
        print(f"| {name} | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f}{' MORE' if slower else ''} | {same} |", flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()


HEAD = ("\n| model | batch | layers replaced (without / with avg_pools) | library launches per forward | avg_pools=False us (least .. most) | "
        "avg_pools=True us (least .. most) | without / with | outputs |\n|---|---|---|---|---|---|---|---|")

if "resnet50" in args.sections:
    print(HEAD, flush=True)
    model_rows("wrapped_resnet50(pooled_holder=True)", lambda: workloads.wrapped_resnet50(device="cuda", pooled_holder=True),
               lambda B: torch.randn(B, 3, 224, 224, device=dev), args.batches, 10)


def mobilenet_head():
    def quantized(layer):
        n = layer.weight.shape[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * n, per_channel=True, channel_axis=0)
        return mq.PytorchQuantizationWrapper(layer.to(dev), {"weight": wq}).to(dev)

    def holder(signed=False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return mq.PytorchActivationQuantizationHolder(
                Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=signed)).to(dev)

    torch.manual_seed(0)
    return torch.nn.Sequential(holder(True), quantized(torch.nn.Conv2d(320, 1280, 1, bias=False)), torch.nn.ReLU6(), holder(),
                               torch.nn.AdaptiveAvgPool2d(1), holder(), torch.nn.Flatten(),
                               quantized(torch.nn.Linear(1280, 1000, bias=False))).eval()


if "head" in args.sections:
    print(HEAD, flush=True)
    model_rows("mobilenet-style head, 320 x 7 x 7 -> 1280 -> pool -> 1000", mobilenet_head, lambda B: torch.randn(B, 320, 7, 7, device=dev),
               args.batches, 50)
