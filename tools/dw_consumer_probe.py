"""What does a depthwise convolution cost on the integer consumer?  (consumers.QuantizedDepthwiseConv2d,
fuse_linear_consumers*(depthwise=True); include/mctq_hip.h: mctq_qconv_dw_i8)

Shapes: MobileNetV2's depthwise layers at 224 x 224 as (channels, image side, stride), all 3 x 3 with padding 1, at batch 1 and 64.
Sections, each in one process with its arms alternating round by round:
    kernel   mctq_qconv_dw_i8 alone, float32 and codes output, cold caches: every launch takes the next set of a ring of
             (input, output) buffers larger than 512 MiB in all (at most 64 sets: the small shapes of batch 1 are then warm, and
             at the launch floor anyway); achieved bytes/s counts B * H * W * C bytes read once plus 4 or 1 byte per output element
    forms    the shipped build beside the experiment builds that are there (tools/build_variant.py), same ring, outputs compared
             bit for bit:
                 python tools/build_variant.py dw_loop -DMCTQ_DW_UNROLL3=0 --units=mctq_qconv_dw.hip
             (3 x 3 kernels on the run-time tap loops instead of the instance unrolled at compile time)
    pairs    activation holder -> wrapped depthwise convolution, unfused (fake-quantize weight and activation, float32 grouped
             conv2d: what the pair ran as before) against fused, NCHW float32 input; median and spread (least .. most) of the rounds
    block    one inverted-residual block at 144 channels on 56 x 56 -- 1x1 expand (32 -> 144), ReLU6, depthwise 3x3, ReLU6, 1x1
             project (144 -> 32), a holder in front of each, plus the input -- as built, through fuse_linear_consumers_fx(...,
             depthwise=False) (the two pointwise pairs) and through fuse_linear_consumers_fx(..., depthwise=True), with and
             without chain=True (the ReLU6 between the layers keeps them from chaining: the arm shows that it costs nothing)
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/dw_consumer_probe.py [--sections kernel forms pairs block] [--iters 50] [--rounds 5] [--batches 1 64]
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
from mct_quantizers_amd import consumers
from mct_quantizers_amd.hip import native

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "pairs", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
Q = mq.pytorch_quantizers

DW3 = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1), (576, 14, 2), (960, 7, 1)]
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
    """Operands of mctq_qconv_dw_i8 for one shape and a ring of (input, output) sets; call(lib, codes_out) -> a launcher that
    takes the next set each time."""

    def __init__(self, C, side, stride, B):
        self.C, self.side, self.stride, self.B = C, side, stride, B
        self.so = (side + 2 - 3) // stride + 1
        self.n_in, self.n_out = B * side * side * C, B * self.so * self.so * C
        sets = max(1, min(RING_MAX, -(-RING_BYTES // (self.n_in + 4 * self.n_out))))
        g = torch.Generator(device=dev).manual_seed(C + side)
        self.x = [torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
        self.y = [torch.empty(self.n_out * 4, dtype=torch.uint8, device=dev) for _ in range(sets)]
        self.w = torch.randint(-128, 128, (3, 3, C), dtype=torch.int8, device=dev, generator=g)
        self.sc = torch.rand(C, device=dev, generator=g) * 0.01 + 0.001
        self.bias = torch.randn(C, device=dev, generator=g)
        self.i = 0

    def call(self, L, codes_out):
        form = (native.CODE_U8, 0.05, 114, 0, 255) if codes_out else (-1, 1.0, 0, 0, 0)

        def f():
            self.i = (self.i + 1) % len(self.x)
            return L.mctq_qconv_dw_i8(self.x[self.i].data_ptr(), native.CODE_U8, 114, 0.02, self.w.data_ptr(), self.sc.data_ptr(), None,
                                      self.bias.data_ptr(), self.y[self.i].data_ptr(), *form, self.B, self.side, self.side, self.C,
                                      3, 3, self.stride, self.stride, 1, 1, 1, 1, S())
        return f

    def output(self, L, codes_out):
        """the bytes one launch of L writes for set 0"""
        self.i = -1
        assert self.call(L, codes_out)() == 0, L.mctq_last_error()
        torch.cuda.synchronize()
        return self.y[0][:self.n_out * (1 if codes_out else 4)].clone()


forms = {"shipped": lib}
for name in ("dw_loop",):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ablate", f"libmctq_hip_{name}.so")
    if os.path.exists(path):
        forms[name] = ctypes.CDLL(path)
        forms[name].mctq_qconv_dw_i8.restype, forms[name].mctq_qconv_dw_i8.argtypes = native.SIGNATURES["mctq_qconv_dw_i8"]
        forms[name].mctq_last_error.restype = ctypes.c_char_p

if "kernel" in args.sections:
    print("\n| C | image | stride | batch | ring sets | float32 out us | GB/s | codes out us | GB/s |")
    print("|---|---|---|---|---|---|---|---|---|", flush=True)
    for (C, side, stride) in DW3:
        for B in args.batches:
            c = RawCase(C, side, stride, B)
            c.output(lib, False), c.output(lib, True)
            res = timed([("f32", c.call(lib, False)), ("codes", c.call(lib, True))], iters=200)
            gb = lambda out_bytes, us: (c.n_in + out_bytes * c.n_out) / us / 1e3            # noqa: E731
            print(f"| {C} | {side} | {stride} | {B} | {len(c.x)} | {res['f32'][0]:.2f} | {gb(4, res['f32'][0]):.0f} | "
                  f"{res['codes'][0]:.2f} | {gb(1, res['codes'][0]):.0f} |", flush=True)
            del c
            torch.cuda.empty_cache()

if "forms" in args.sections:
    if len(forms) == 1:
        print("\n(forms: no experiment build under tools/ablate/ -- not measured)")
    else:
        print("\n| C | image | stride | batch | output | " + " | ".join(f"{n} us (least .. most)" for n in forms) + " |")
        print("|---|---|---|---|---|" + "---|" * len(forms), flush=True)
        for (C, side, stride) in DW3:
            for B in args.batches:
                c = RawCase(C, side, stride, B)
                for codes_out in (False, True):
                    want = c.output(lib, codes_out)
                    assert all(torch.equal(c.output(L, codes_out), want) for L in forms.values())
                    res = timed([(n, c.call(L, codes_out)) for n, L in forms.items()], iters=200)
                    print(f"| {C} | {side} | {stride} | {B} | {'codes' if codes_out else 'float32'} | "
                          + " | ".join(f"{res[n][0]:.2f} ({res[n][1]:.2f} .. {res[n][2]:.2f})" for n in forms) + " |", flush=True)
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
    for (C, side, stride) in DW3:
        torch.manual_seed(0)
        plain = torch.nn.Sequential(*pair(C, C, 3, stride, groups=C, relu=True))
        torch.manual_seed(0)                                      # the same weights for both arms
        fused = torch.nn.Sequential(*pair(C, C, 3, stride, groups=C, relu=True))
        assert consumers.fuse_linear_consumers(fused, depthwise=True) == 1
        for B in args.batches:
            x = torch.rand(B, C, side, side, device=dev) * 8.0
            with torch.no_grad():
                ref, y = plain(x), fused(x)
                assert native.last_launch().startswith("qconv_dw<")
                rel = float((y - ref).abs().max() / ref.abs().max())
                res = timed([("unfused", lambda: plain(x)), ("fused", lambda: fused(x))])
            u, f = res["unfused"], res["fused"]
            print(f"{C} 3x3/{stride} {side}x{side} batch {B}: unfused {u[0]:.1f} us ({u[1]:.1f} .. {u[2]:.1f}), fused {f[0]:.1f} us "
                  f"({f[1]:.1f} .. {f[2]:.1f}), max rel diff {rel:.1e}", flush=True)
            rows_md.append(f"| {C} | {side} | {stride} | {B} | {u[0]:.1f} ({u[1]:.1f} .. {u[2]:.1f}) | {f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}) | "
                           f"{u[0] / f[0]:.2f} |")
        del plain, fused
        torch.cuda.empty_cache()
    print("\n| channels | image | stride | batch | unfused pair us (least .. most) | fused pair us (least .. most) | unfused / fused |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


class InvertedResidual(torch.nn.Module):
    def __init__(self, C=32, E=144):
        super().__init__()
        self.h1, self.c1 = pair(C, E, 1, 1)
        self.h2, self.c2 = pair(E, E, 3, 1, groups=E, relu=True)
        self.h3, self.c3 = pair(E, C, 1, 1, relu=True)

    def forward(self, x):
        y = torch.nn.functional.relu6(self.c1(self.h1(x)))
        y = torch.nn.functional.relu6(self.c2(self.h2(y)))
        return x + self.c3(self.h3(y))


if "block" in args.sections:
    def block():
        torch.manual_seed(0)
        return InvertedResidual().to(dev)

    print("\ninverted residual, 32 -> 144 -> 144 (depthwise 3x3) -> 32 on 56 x 56, eager forward")
    print("| batch | arm | pairs fused | us per forward (least .. most) | max rel diff to as built |\n|---|---|---|---|---|")
    for B in args.batches:
        x = torch.randn(B, 32, 56, 56, device=dev)
        with torch.no_grad():
            plain = block()
            ref = plain(x)
            arms, meta = [("as built", lambda: plain(x))], {"as built": (0, 0.0)}
            for name, kw in (("fx, depthwise=False", dict()), ("fx, depthwise=True", dict(depthwise=True)),
                             ("fx, depthwise=True, chain=True", dict(depthwise=True, chain=True))):
                gm, n = consumers.fuse_linear_consumers_fx(block(), **kw)
                meta[name] = (n, float((gm(x) - ref).abs().max() / ref.abs().max()))
                arms.append((name, (lambda g: lambda: g(x))(gm)))
            res = timed(arms)
        for name, _ in arms:
            r = res[name]
            print(f"| {B} | {name} | {meta[name][0]} | {r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f}) | {meta[name][1]:.1e} |", flush=True)
