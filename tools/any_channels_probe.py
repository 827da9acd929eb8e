"""What do integer consumers for any channel count cost, and what do they save?  (the ``any_channels`` keyword of
consumers.QuantizedLinear / QuantizedConv1x1 / QuantizedConv2d and of fuse_linear_consumers*; include/mctq_hip.h:
mctq_codes_im2col_pad_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds.  Every
launch or forward takes the next set of a ring of input buffers (at most 16 sets, about 1.2 GB in all: cold inputs):
    gather   mctq_codes_im2col_pad_nhwc alone at batch 1 and 64 on the stem (3 x 224 x 224, 7 x 7 / 2, pad 3), the re-pitch of a
             pointwise layer's rows (24 x 56 x 56 and 40 x 28 x 28, 1 x 1) and a 3 x 3 patch matrix (24 x 56 x 56): time and bytes
             written per second; the bytes compared with the torch route first
    grain    4-byte against 1-byte pieces (tuning key "im2col_grain" 4 / 1) on the rows with C % 4 == 0, same bytes
    pairs    activation holder -> wrapped layer as built (fake-quantize activation and weight, float32 conv2d / linear: what runs
             without the switch) against the padded consumer: the stem, 24 -> 144 pointwise on 56 x 56, an SE fc2 (Linear 6 -> 144)
    block    MobileNetV2's block 24 -> 144 -> 144 -> 24 on 56 x 56 through fuse_linear_consumers_fx with every switch, with and
             without any_channels=True
    resnet50 workloads.wrapped_resnet50(input_holder=True, pooled_holder=True) through the same two rewrites, and how many of
             its 54 wrapped layers run on codes
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/any_channels_probe.py [--sections gather grain pairs block resnet50] [--iters 100] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["gather", "grain", "pairs", "block", "resnet50"])
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
ap.add_argument("--resnet-batch", type=int, default=64)
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, channels, image side, kernel, stride, padding)
SHAPES = [("stem 3 x 224 x 224, 7 x 7 / 2", 3, 224, 7, 2, 3), ("24 x 56 x 56, 1 x 1", 24, 56, 1, 1, 0),
          ("40 x 28 x 28, 1 x 1", 40, 28, 1, 1, 0), ("24 x 56 x 56, 3 x 3", 24, 56, 3, 1, 1)]
RING_BYTES, RING_MAX = 1200 << 20, 16
EVERY = dict(chain=True, uniform_weights=True, convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True, pools=True,
             fused_residuals=True, concats=True, avg_pools=True, muls=True, hard_activations=True, upsamples=True)


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


def ring_sets(bytes_per_set):
    return max(1, min(RING_MAX, RING_BYTES // max(1, bytes_per_set)))


class Ring:
    """``make()`` tensors, as many as fit the ring; ``next()`` hands out the following one."""

    def __init__(self, make, bytes_per_set):
        self.items, self.i = [make() for _ in range(ring_sets(bytes_per_set))], 0

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


class GatherCase:
    """A ring of NHWC codes for one geometry and the raw launch on the next set."""

    def __init__(self, C, side, k, stride, pad, B):
        self.args = (B, side, side, C, k, k, stride, stride, pad, pad, 1, 1, 114)
        so = (side + 2 * pad - k) // stride + 1
        self.K, self.Kp, self.rows = k * k * C, -(-k * k * C // 16) * 16, B * so * so
        g = torch.Generator(device=dev).manual_seed(C + side)
        self.ring = Ring(lambda: torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev, generator=g), B * side * side * C)
        self.out = torch.empty((self.rows, self.Kp), dtype=torch.uint8, device=dev)
        self.geometry = (k, stride, pad, 1)

    def raw(self):
        return lib.mctq_codes_im2col_pad_nhwc(self.ring.next().data_ptr(), self.out.data_ptr(), *self.args, S())

    def output(self):
        self.ring.i = -1
        self.out.zero_()
        assert self.raw() == 0, lib.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def torch_route(self):
        """the same matrix by torch ops on the device: the unpadded gather of a channel count the old kernel takes is not available"""
        return ops.codes_im2col(self.ring.items[0].cpu(), *self.geometry, 114, pad_to=16).to(dev)


if "gather" in args.sections:
    print("\n| gather | batch | ring sets | rows x Kp (K) | pieces | us (least .. most) | MB written | GB/s written |")
    print("|---|---|---|---|---|---|---|---|", flush=True)
    for name, C, side, k, stride, pad in SHAPES:
        for B in args.batches:
            c = GatherCase(C, side, k, stride, pad, B)
            got = c.output()
            grain = native.last_launch().split("G=")[1][0]
            assert torch.equal(got, c.torch_route()), name
            res = timed([("gather", c.raw)])
            mb = c.out.numel() / 1e6
            print(f"| {name} | {B} | {len(c.ring.items)} | {c.rows} x {c.Kp} ({c.K}) | {grain} B | {fmt(res['gather'])} | {mb:.2f} | "
                  f"{mb / res['gather'][0] * 1e3:.0f} |", flush=True)
            del c, got
            torch.cuda.empty_cache()

if "grain" in args.sections:
    print("\n| gather | batch | 4-byte pieces us (least .. most) | 1-byte pieces us (least .. most) | 1-byte / 4-byte | faster |")
    print("|---|---|---|---|---|---|", flush=True)
    try:
        for name, C, side, k, stride, pad in [s for s in SHAPES if s[1] % 4 == 0] + [("72 x 28 x 28, 3 x 3", 72, 28, 3, 1, 1)]:
            for B in args.batches:
                c = GatherCase(C, side, k, stride, pad, B)
                outs = []
                for grain in (4, 1):
                    native.set_tuning("im2col_grain", grain)
                    outs.append(c.output())
                    assert f"G={grain}" in native.last_launch()
                assert torch.equal(*outs), name

                def run(grain):
                    native.set_tuning("im2col_grain", grain)
                    return c.raw()

                res = timed([("g4", lambda: run(4)), ("g1", lambda: run(1))])
                ratio = res["g1"][0] / res["g4"][0]
                print(f"| {name} | {B} | {fmt(res['g4'])} | {fmt(res['g1'])} | {ratio:.2f} | {'4-byte' if ratio > 1 else '1-byte'} |", flush=True)
                del c, outs
                torch.cuda.empty_cache()
    finally:
        native.set_tuning("im2col_grain", 0)


def quantizer(threshold=8.0, signed=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[threshold], signed=signed)


def holder(threshold=8.0, signed=False):
    return mq.PytorchActivationQuantizationHolder(quantizer(threshold, signed)).to(dev)


def wrapped(layer):
    layer = layer.to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in layer.weight.detach().reshape(layer.weight.shape[0], -1).abs().amax(1)]
        wq = Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=True, channel_axis=0)
    return mq.PytorchQuantizationWrapper(layer, {"weight": wq}).to(dev)


def pair(make_layer, signed):
    torch.manual_seed(0)                                      # the same weights for both arms
    return torch.nn.Sequential(holder(4.0 if signed else 8.0, signed), wrapped(make_layer())).to(dev).eval()


def compare(y, ref):
    return "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"


if "pairs" in args.sections:
    print("\n| pair | batch | ring sets | as built us (least .. most) | padded consumer us (least .. most) | library launches (as built / consumer) | "
          "as built / consumer | with the feature | outputs |\n|---|---|---|---|---|---|---|---|---|", flush=True)
    PAIRS = [("stem 3 -> 64, 7 x 7 / 2, 224 x 224", lambda: torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), True,
              lambda B: (B, 3, 224, 224), dict(convolutions=True)),
             ("24 -> 144 pointwise, 56 x 56", lambda: torch.nn.Conv2d(24, 144, 1, bias=False), False, lambda B: (B, 24, 56, 56), {}),
             ("SE fc2: Linear 6 -> 144", lambda: torch.nn.Linear(6, 144), False, lambda B: (B, 6), {})]
    for name, make_layer, signed, shape, switch in PAIRS:
        plain, fused = pair(make_layer, signed), pair(make_layer, signed)
        assert consumers.fuse_linear_consumers(pair(make_layer, signed), **switch) == 0          # without the switch: left alone
        assert consumers.fuse_linear_consumers(fused, any_channels=True, **switch) == 1
        for B in args.batches:
            n = int(np.prod(shape(B)))
            g = torch.Generator(device=dev).manual_seed(n % 1000)
            make = lambda: (torch.randn(*shape(B), device=dev, generator=g) * 1.5)              # noqa: E731
            ring = Ring(make, 4 * n)                                                            # NCHW float32, as a model's input arrives
            with torch.no_grad():
                x0 = ring.items[0]
                same = compare(fused(x0), plain(x0))
                count = lambda m: (native.launch_count(), m(x0), native.launch_count())      # noqa: E731
                l0, l1 = (c[2] - c[0] for c in (count(plain), count(fused)))
                res = timed([("plain", lambda: plain(ring.next())), ("fused", lambda: fused(ring.next()))])
            a, b = res["plain"], res["fused"]
            print(f"| {name} | {B} | {len(ring.items)} | {fmt(a)} | {fmt(b)} | {l0} / {l1} | {a[0] / b[0]:.2f} | "
                  f"{'faster' if a[0] > b[0] else 'slower'} | {same} |", flush=True)
            del ring
            torch.cuda.empty_cache()


class InvertedResidual(torch.nn.Module):
    """MobileNetV2's block 24 -> 144 -> 144 -> 24 (stride 1, with its identity), a holder behind every activation and the add."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.h_in = holder(4.0, True)
        self.e, self.h1 = wrapped(torch.nn.Conv2d(24, 144, 1, bias=False)), holder(6.0)
        self.dw, self.h2 = wrapped(torch.nn.Conv2d(144, 144, 3, padding=1, groups=144, bias=False)), holder(6.0)
        self.p, self.h_out = wrapped(torch.nn.Conv2d(144, 24, 1, bias=False)), holder(4.0, True)
        self.last = wrapped(torch.nn.Conv2d(24, 144, 1, bias=False))           # the next block's expand layer reads the sum

    def forward(self, x):
        a = self.h_in(x)
        y = F.relu6(self.dw(self.h1(F.relu6(self.e(a)))))
        return self.last(self.h_out(a + self.p(self.h2(y))))


def model_rows(title, make, shape, batches, iters):
    for B in batches:
        n = int(np.prod(shape(B)))
        g = torch.Generator(device=dev).manual_seed(7)
        ring = Ring(lambda: torch.randn(*shape(B), device=dev, generator=g) * 1.5, 4 * n)         # NCHW float32
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(make(), **EVERY)
            gm, n1 = consumers.fuse_linear_consumers_fx(make(), any_channels=True, **EVERY)
            x0 = ring.items[0]
            same = compare(gm(x0), gm0(x0))
            count = lambda m: (native.launch_count(), m(x0), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(ring.next())), ("on", lambda: gm(ring.next()))], iters=iters)
        a, b = res["off"], res["on"]
        print(f"| {title} | {B} | {len(ring.items)} | {n0} / {n1} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | "
              f"{'faster' if a[0] > b[0] else 'slower'} | {same} |", flush=True)
        del gm, gm0, ring
        torch.cuda.empty_cache()


MODEL_HEADER = ("\n| model | batch | ring sets | wrapped layers on codes (without / with any_channels) | library launches per forward | "
                "any_channels=False us (least .. most) | any_channels=True us (least .. most) | without / with | with the feature | outputs |\n"
                "|---|---|---|---|---|---|---|---|---|---|")

if "block" in args.sections:
    print(MODEL_HEADER, flush=True)
    model_rows("MobileNetV2 block 24 -> 144 -> 144 -> 24 (+ the next expand), 56 x 56", lambda: InvertedResidual().eval(),
               lambda B: (B, 24, 56, 56), args.batches, 20)

if "resnet50" in args.sections:
    print(MODEL_HEADER, flush=True)
    model_rows("wrapped_resnet50(input_holder=True, pooled_holder=True), 224 x 224, 54 wrapped layers",
               lambda: workloads.wrapped_resnet50(input_holder=True, pooled_holder=True), lambda B: (B, 3, 224, 224),
               sorted({1, args.resnet_batch}), max(2, args.iters // 10))
