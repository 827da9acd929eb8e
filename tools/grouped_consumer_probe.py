"""What does a grouped convolution cost on the integer consumer?  (consumers.QuantizedGroupedConv2d,
fuse_linear_consumers*(grouped=True); include/mctq_hip.h: mctq_qconv_grouped_i8)

Shapes, all 3 x 3 with padding 1, as (channels, groups, image side, stride), at batch 1 and 64: ResNeXt-50 32x4d's four grouped layers
(128 / 32 on 56 x 56, 256 / 32 on 28 x 28, 512 / 32 on 14 x 14, 1024 / 32 on 7 x 7) with their stride-2 first-of-stage forms on
the larger image, and RegNet's group widths 8, 16, 24 and 48.
Sections, each in one process with its arms alternating round by round:
    kernel   mctq_qconv_grouped_i8 alone, float32 and codes output, cold caches: every launch takes the next set of a ring of
             (input, output) buffers larger than 512 MiB in all (at most 64 sets: the small shapes of batch 1 are then warm, and
             at the launch floor anyway); achieved bytes/s counts B * H * W * C bytes read once plus 4 or 1 byte per output element,
             achieved op/s 2 * Kg multiply-accumulates per output element
    pairs    activation holder -> wrapped grouped convolution, unfused (fake-quantize weight and activation, float32 grouped conv2d:
             what the pair runs as without the switch, as the model is built) against fused, NCHW float32 input; median and spread
             (least .. most) of the rounds
    block    one ResNeXt bottleneck at 256 channels on 56 x 56 -- 1x1 256 -> 128, ReLU, 3x3 groups=32, ReLU, 1x1 128 -> 256, plus the
             input, ReLU, a holder in front of each layer and one behind the block -- as built and through fuse_linear_consumers_fx
             with every switch, without and with grouped=True
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/grouped_consumer_probe.py [--sections kernel pairs block] [--iters 50] [--rounds 5] [--batches 1 64]
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
from mct_quantizers_amd.hip import native

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "pairs", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
Q = mq.pytorch_quantizers

# (channels, groups, image side, stride)
RESNEXT = [(128, 32, 56, 1), (256, 32, 56, 2), (256, 32, 28, 1), (512, 32, 28, 2), (512, 32, 14, 1), (1024, 32, 14, 2), (1024, 32, 7, 1)]
REGNET = [(64, 8, 56, 1), (128, 8, 28, 1), (168, 7, 28, 1), (432, 9, 14, 1)]          # group widths 8, 16, 24, 48
SHAPES = RESNEXT + REGNET
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


class RawCase:
    """Operands of mctq_qconv_grouped_i8 for one shape and a ring of (input, output) sets; call(codes_out) -> a launcher that
    takes the next set each time."""

    def __init__(self, C, G, side, stride, B):
        self.C, self.G, self.side, self.stride, self.B = C, G, side, stride, B
        self.so = (side + 2 - 3) // stride + 1
        self.kg = 9 * (C // G)
        self.n_in, self.n_out = B * side * side * C, B * self.so * self.so * C
        sets = max(1, min(RING_MAX, -(-RING_BYTES // (self.n_in + 4 * self.n_out))))
        g = torch.Generator(device=dev).manual_seed(C + side)
        self.x = [torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
        self.y = [torch.empty(self.n_out * 4, dtype=torch.uint8, device=dev) for _ in range(sets)]
        w = torch.randint(-128, 128, (C, 3, 3, C // G), dtype=torch.int8, device=dev, generator=g)
        self.w, self.rowsum = consumers.pack_grouped_weights(w, G)
        self.sc = torch.rand(C, device=dev, generator=g) * 0.01 + 0.001
        self.bias = torch.randn(C, device=dev, generator=g)
        self.i = 0

    def call(self, codes_out):
        form = (native.CODE_U8, 0.05, 114, 0, 255) if codes_out else (-1, 1.0, 0, 0, 0)

        def f():
            self.i = (self.i + 1) % len(self.x)
            return lib.mctq_qconv_grouped_i8(self.x[self.i].data_ptr(), native.CODE_U8, 114, 0.02, self.w.data_ptr(), self.sc.data_ptr(),
                                             self.rowsum.data_ptr(), None, self.bias.data_ptr(), self.y[self.i].data_ptr(), *form,
                                             self.B, self.side, self.side, self.C, self.C, self.G, 3, 3, self.stride, self.stride,
                                             1, 1, 1, 1, S())
        return f


if "kernel" in args.sections:
    print("\n| C | groups | Cg | image | stride | batch | ring sets | float32 out us | GB/s | Top/s | codes out us | GB/s | Top/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for (C, G, side, stride) in SHAPES:
        for B in args.batches:
            c = RawCase(C, G, side, stride, B)
            for codes_out in (False, True):
                assert c.call(codes_out)() == 0, lib.mctq_last_error()
            assert native.last_launch().startswith("qconv_grouped<")
            res = timed([("f32", c.call(False)), ("codes", c.call(True))], iters=200)
            gb = lambda out_bytes, us: (c.n_in + out_bytes * c.n_out) / us / 1e3            # noqa: E731
            tops = lambda us: 2.0 * c.kg * c.n_out / us / 1e6                               # noqa: E731
            print(f"| {C} | {G} | {C // G} | {side} | {stride} | {B} | {len(c.x)} | {res['f32'][0]:.2f} | {gb(4, res['f32'][0]):.0f} | "
                  f"{tops(res['f32'][0]):.2f} | {res['codes'][0]:.2f} | {gb(1, res['codes'][0]):.0f} | {tops(res['codes'][0]):.2f} |",
                  flush=True)
            del c
            torch.cuda.empty_cache()


def pair(cin, cout, k, stride, groups=1, relu=False):
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, groups=groups, bias=True).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in conv.weight.detach().abs().amax((1, 2, 3))]
        wq = Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=True, channel_axis=0)
        aq = Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False) if relu else \
            Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-4.0], max_range=[4.0])
    return [mq.PytorchActivationQuantizationHolder(aq).to(dev), mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)]


if "pairs" in args.sections:
    rows_md = []
    for (C, G, side, stride) in SHAPES:
        torch.manual_seed(0)
        plain = torch.nn.Sequential(*pair(C, C, 3, stride, groups=G, relu=True))
        torch.manual_seed(0)                                      # the same weights for both arms
        fused = torch.nn.Sequential(*pair(C, C, 3, stride, groups=G, relu=True))
        assert consumers.fuse_linear_consumers(fused, grouped=True) == 1
        for B in args.batches:
            x = torch.rand(B, C, side, side, device=dev) * 8.0
            with torch.no_grad():
                ref, y = plain(x), fused(x)
                assert native.last_launch().startswith("qconv_grouped<")
                rel = float((y - ref).abs().max() / ref.abs().max())
                res = timed([("unfused", lambda: plain(x)), ("fused", lambda: fused(x))])
            u, f = res["unfused"], res["fused"]
            print(f"{C}/{G} 3x3/{stride} {side}x{side} batch {B}: unfused {u[0]:.1f} us ({u[1]:.1f} .. {u[2]:.1f}), fused {f[0]:.1f} us "
                  f"({f[1]:.1f} .. {f[2]:.1f}), max rel diff {rel:.1e}", flush=True)
            bold = "**" if f[0] > u[0] else ""                    # the feature slower: in bold
            rows_md.append(f"| {C} | {G} | {side} | {stride} | {B} | {u[0]:.1f} ({u[1]:.1f} .. {u[2]:.1f}) | "
                           f"{bold}{f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}){bold} | {bold}{u[0] / f[0]:.2f}{bold} |")
        del plain, fused
        torch.cuda.empty_cache()
    print("\n| channels | groups | image | stride | batch | unfused pair us (least .. most) | fused pair us (least .. most) | unfused / fused |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


class Bottleneck(torch.nn.Module):
    def __init__(self, C=256, E=128, G=32):
        super().__init__()
        self.h0, self.c1 = pair(C, E, 1, 1, relu=True)
        self.h1, self.c2 = pair(E, E, 3, 1, groups=G, relu=True)
        self.h2, self.c3 = pair(E, C, 1, 1, relu=True)
        self.h3 = pair(16, 16, 1, 1, relu=True)[0]

    def forward(self, x):
        x = self.h0(x)
        y = self.h1(torch.relu(self.c1(x)))
        y = self.h2(torch.relu(self.c2(y)))
        return self.h3(torch.relu(self.c3(y) + x))


if "block" in args.sections:
    def block():
        torch.manual_seed(0)
        return Bottleneck().to(dev)

    every = dict(convolutions=True, depthwise=True, uniform_weights=True, shared_holders=True, stay_on_codes=True, fused_residuals=True,
                 pools=True, avg_pools=True, concats=True, muls=True, hard_activations=True, upsamples=True, any_channels=True,
                 activation_tables=True)
    print("\nResNeXt bottleneck, 256 -> 128 -> 128 (3x3, groups=32) -> 256 on 56 x 56, eager forward")
    print("| batch | arm | layers fused | us per forward (least .. most) | max abs diff to as built / output step |\n|---|---|---|---|---|")
    for B in args.batches:
        x = torch.rand(B, 256, 56, 56, device=dev) * 8.0
        with torch.no_grad():
            plain = block()
            ref = plain(x)
            step = consumers._activation_code_params(plain.h3.activation_holder_quantizer)[0]
            arms, meta = [("as built", lambda: plain(x))], {"as built": (0, 0.0)}
            for name, kw in (("fx, every switch, grouped=False", every), ("fx, every switch, grouped=True", dict(every, grouped=True))):
                gm, n = consumers.fuse_linear_consumers_fx(block(), **kw)
                meta[name] = (n, float((gm(x) - ref).abs().max()) / step)
                arms.append((name, (lambda g: lambda: g(x))(gm)))
            res = timed(arms)
        for name, _ in arms:
            r = res[name]
            print(f"| {B} | {name} | {meta[name][0]} | {r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f}) | {meta[name][1]:.1f} |", flush=True)
