"""What does a max pool on activation codes cost, and what does it save?  (consumers.QuantizedMaxPool2d,
fuse_linear_consumers*(pools=True); include/mctq_hip.h: mctq_codes_maxpool_nhwc)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel    the launch alone on ResNet-50's stem pool (64 channels, 112 x 112, 3 x 3 stride 2 padding 1) and VGG-16's five pools
              (2 x 2 stride 2), against what it replaces: ATen's float32 max pool of the holder's output (NCHW for the stem, whose
              producer is a wrapper; channels-last for VGG, whose producers are consumers) and one quantize launch of the pooled
              tensor (ops.fq_codes_nhwc; ResNet-50's first block issues two, c1's and the downsample's).  Every launch takes the
              next set of a ring of buffers (at most 16 sets, about 1.2 GB in all); outputs compared with torch.equal first
    forms     the shipped build beside the experiment build, if it is there (tools/build_variant.py), same ring, same check:
                  python tools/build_variant.py pool_unroll -DMCTQ_POOL_UNROLL=1 --units=mctq_codes_maxpool.hip
              (2 x 2 and 3 x 3 kernels on an instance unrolled at compile time instead of the run-time tap loops)
    resnet50  workloads.wrapped_resnet50 through fuse_linear_consumers_fx(convolutions=True, shared_holders=True,
              stay_on_codes=True) with and without pools=True.  Without it the first block's c1 and downsample are float32
              wrappers, whose accumulation rounds: the outputs are compared by their largest relative difference, not bit for bit
    vgg       conv3x3 -> ReLU -> holder -> conv3x3 -> ReLU -> holder -> MaxPool2d(2), three times over (64, 128, 256 channels, 56 x 56
              input), same switches with and without pools=True; torch.equal where it holds, else the largest relative difference
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/pool_consumer_probe.py [--sections kernel forms resnet50 vgg] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import ctypes
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
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "resnet50", "vgg"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
Q = mq.pytorch_quantizers
F = torch.nn.functional

# (name, channels, image side, kernel, stride, padding, the float32 arm's memory format)
POOLS = [("resnet50 stem", 64, 112, 3, 2, 1, torch.contiguous_format)] + \
        [(f"vgg16 pool{i + 1}", c, side, 2, 2, 0, torch.channels_last) for i, (c, side) in
         enumerate(((64, 224), (128, 112), (256, 56), (512, 28), (512, 14)))]
RING_BYTES, RING_MAX = 1200 << 20, 16
FORM = (8.0 / 256, 0, 0, 255)                               # the unsigned holder behind a ReLU


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

    def __init__(self, C, side, k, s, p, fmt_, B):
        self.k, self.s, self.p, self.B, self.C, self.side = k, s, p, B, C, side
        self.so = ops._pool_out_size(side, k, s, p, 1, False)
        n_in = B * C * side * side
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * n_in)))
        g = torch.Generator(device=dev).manual_seed(C + side)
        scale, zp, qmin, qmax = FORM
        self.x = [(torch.rand(B, C, side, side, device=dev, generator=g) * 9.0 - 0.5).contiguous(memory_format=fmt_) for _ in range(sets)]
        self.x = [mq_fq(x) for x in self.x]                   # what a holder writes
        self.codes = [ops.fq_codes_nhwc(x, qmin, qmax, scale, zp) for x in self.x]
        self.out = torch.empty((B, self.so, self.so, C), dtype=torch.uint8, device=dev)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def raw(self, L):
        def f():
            c = self.codes[self.step()]
            return L.mctq_codes_maxpool_nhwc(c.data_ptr(), self.out.data_ptr(), native.CODE_U8, self.B, self.side, self.side, self.C,
                                             self.k, self.k, self.s, self.s, self.p, self.p, 1, 1, 0, self.so, self.so, S())
        return f

    def output(self, L):
        self.i = -1
        assert self.raw(L)() == 0, L.mctq_last_error()
        torch.cuda.synchronize()
        return self.out.clone()

    def aten_pool(self):
        return F.max_pool2d(self.x[self.step()], self.k, self.s, self.p)

    def quantize(self, pooled):
        scale, zp, qmin, qmax = FORM
        return ops.fq_codes_nhwc(pooled, qmin, qmax, scale, zp)


def mq_fq(x):
    scale, zp, qmin, qmax = FORM
    return ops.fq_per_tensor(x, scale, zp, qmin, qmax)


forms = {"shipped": lib}
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ablate", "libmctq_hip_pool_unroll.so")
if os.path.exists(path):
    forms["pool_unroll"] = ctypes.CDLL(path)
    forms["pool_unroll"].mctq_codes_maxpool_nhwc.restype, forms["pool_unroll"].mctq_codes_maxpool_nhwc.argtypes = \
        native.SIGNATURES["mctq_codes_maxpool_nhwc"]
    forms["pool_unroll"].mctq_last_error.restype = ctypes.c_char_p

if "kernel" in args.sections or "forms" in args.sections:
    print("\n| pool | batch | ring sets | codes pool us (least .. most) | GB/s | ATen float32 pool us | quantize pooled us | "
          "ATen pool + 1 quantize us | ATen pool + quantize / codes pool |" + "".join(f" {n} us |" for n in list(forms)[1:]))
    print("|---|---|---|---|---|---|---|---|---|" + "---|" * (len(forms) - 1), flush=True)
    for (name, C, side, k, s, p, fmt_) in POOLS:
        for B in args.batches:
            c = PoolCase(C, side, k, s, p, fmt_, B)
            got = c.output(lib)
            want = c.quantize(F.max_pool2d(c.x[0], k, s, p))
            assert torch.equal(got, want), name            # pooled codes == codes of ATen's float32 pool
            assert all(torch.equal(c.output(L), got) for L in forms.values())
            pooled = c.aten_pool()
            arms = [("codes", c.raw(lib)), ("aten", c.aten_pool), ("quantize", lambda: c.quantize(pooled)),
                    ("aten+q", lambda: c.quantize(c.aten_pool()))]
            if "forms" in args.sections:
                arms += [(n, c.raw(L)) for n, L in list(forms.items())[1:]]
            res = timed(arms, iters=100)
            n_in, n_out = B * C * side * side, B * C * c.so * c.so
            print(f"| {name} {C} x {side} x {side}, {k}x{k}/{s} | {B} | {len(c.x)} | {fmt(res['codes'])} | "
                  f"{(n_in + n_out) / res['codes'][0] / 1e3:.0f} | {fmt(res['aten'])} | {fmt(res['quantize'])} | {fmt(res['aten+q'])} | "
                  f"{res['aten+q'][0] / res['codes'][0]:.2f} |" + "".join(f" {fmt(res[n])} |" for n in list(forms)[1:]), flush=True)
            del c, pooled
            torch.cuda.empty_cache()


def compare(y, ref):
    return "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"


def model_rows(name, make, make_x, switches, batches, iters):
    for B in batches:
        x = make_x(B)
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(make(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(make(), pools=True, **switches)
            same = compare(gm(x), gm0(x))
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("pools=False", lambda: gm0(x)), ("pools=True", lambda: gm(x))], iters=iters)
        a, b = res["pools=False"], res["pools=True"]
        print(f"| {name} | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | {same} |", flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()


HEAD = ("\n| model | batch | layers replaced (without / with pools) | library launches per forward | pools=False us (least .. most) | "
        "pools=True us (least .. most) | without / with | outputs |\n|---|---|---|---|---|---|---|---|")

if "resnet50" in args.sections:
    print(HEAD, flush=True)
    model_rows("wrapped_resnet50", lambda: workloads.wrapped_resnet50(device="cuda"), lambda B: torch.randn(B, 3, 224, 224, device=dev),
               dict(convolutions=True, shared_holders=True, stay_on_codes=True), args.batches, 10)


def vgg_stack():
    def wrapped(cin, cout):
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wq = Q.WeightsPOTInferableQuantizer(num_bits=8, threshold=[0.125] * cout, per_channel=True, channel_axis=0)
        return mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)

    def holder(signed=False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return mq.PytorchActivationQuantizationHolder(
                Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=signed)).to(dev)

    torch.manual_seed(0)
    layers, cin = [holder(True)], 16
    for c in (64, 128, 256):
        layers += [wrapped(cin, c), torch.nn.ReLU(), holder(), wrapped(c, c), torch.nn.ReLU(), holder(), torch.nn.MaxPool2d(2)]
        cin = c
    layers += [wrapped(cin, 64)]
    return torch.nn.Sequential(*layers).eval()


if "vgg" in args.sections:
    print(HEAD, flush=True)
    model_rows("vgg-style, 3 x (2 conv3x3 + pool)", vgg_stack, lambda B: torch.randn(B, 16, 56, 56, device=dev),
               dict(convolutions=True, shared_holders=True, stay_on_codes=True), args.batches, 20)
