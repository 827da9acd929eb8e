"""What does a transposed convolution cost on the integer consumer?  (consumers.QuantizedConvTranspose2d,
fuse_linear_consumers*(transposed=True); include/mctq_hip.h: mctq_qconv_transposed_i8)

Shapes, as (in channels, out channels, kernel, stride, padding, output padding, image side), at batch 1 and 64: a U-Net decoder's
2 x 2 stride-2 layers (256 -> 128 on 28 x 28, 128 -> 64 on 56 x 56, 64 -> 32 on 112 x 112), the 4 x 4 stride-2 padding-1 layers of a
segmentation head or a GAN generator (256 -> 128 on 16 x 16, 128 -> 64 on 32 x 32) and 3 x 3 stride 2 with padding 1 and output
padding 1 (128 -> 64 on 56 x 56).
Sections, each in one process with its arms alternating round by round:
    kernel   mctq_qconv_transposed_i8 alone, float32 and codes output, cold caches: every launch takes the next set of a ring of
             (input, output) buffers larger than 512 MiB in all (at most 64 sets: the small shapes of batch 1 are then warm, and
             at the launch floor anyway); achieved bytes/s counts B * H * W * C bytes read once plus 4 or 1 byte per output element,
             achieved op/s 2 * (kh * kw * C / (sh * sw)) multiply-accumulates per output element (the taps that reach it, on
             average); the launch floor is what the batch-1 rows show
    pairs    activation holder -> wrapped ConvTranspose2d, unfused (fake-quantize weight and activation, float32 conv_transpose2d:
             what the pair runs as without the switch, as the model is built) against fused, NCHW float32 input; median and spread
             (least .. most) of the rounds
    stage    one decoder stage -- conv1x1 128 -> 128, ReLU, holder A, ConvTranspose2d 128 -> 64 (2 x 2, stride 2), ReLU, holder B,
             cat([B, skip holder]), holder C, conv3x3 128 -> 64 on 56 x 56 -> 112 x 112 -- as built and through
             fuse_linear_consumers_fx with every switch, without and with transposed=True
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/transposed_consumer_probe.py [--sections kernel pairs stage] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "pairs", "stage"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
Q = mq.pytorch_quantizers

# (in channels, out channels, kernel, stride, padding, output padding, image side)
SHAPES = [(256, 128, 2, 2, 0, 0, 28), (128, 64, 2, 2, 0, 0, 56), (64, 32, 2, 2, 0, 0, 112),
          (256, 128, 4, 2, 1, 0, 16), (128, 64, 4, 2, 1, 0, 32), (128, 64, 3, 2, 1, 1, 56)]
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
    """Operands of mctq_qconv_transposed_i8 for one shape and a ring of (input, output) sets; call(codes_out) -> a launcher that
    takes the next set each time."""

    def __init__(self, C, O, k, s, p, op, side, B):
        self.geometry, self.C, self.O, self.side, self.B = (k, k, s, s, p, p, op, op), C, O, side, B
        self.so = (side - 1) * s - 2 * p + k + op
        self.macs = k * k * C / (s * s)
        self.n_in, self.n_out = B * side * side * C, B * self.so * self.so * O
        sets = max(1, min(RING_MAX, -(-RING_BYTES // (self.n_in + 4 * self.n_out))))
        g = torch.Generator(device=dev).manual_seed(C + side)
        self.x = [torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
        self.y = [torch.empty(self.n_out * 4, dtype=torch.uint8, device=dev) for _ in range(sets)]
        w = torch.randint(-128, 128, (O, k, k, C), dtype=torch.int8, device=dev, generator=g)
        self.w, self.rowsum = consumers.pack_transposed_weights(w, s)
        self.sc = torch.rand(O, device=dev, generator=g) * 0.01 + 0.001
        self.bias = torch.randn(O, device=dev, generator=g)
        self.i = 0

    def call(self, codes_out):
        form = (native.CODE_U8, 0.05, 114, 0, 255) if codes_out else (-1, 1.0, 0, 0, 0)

        def f():
            self.i = (self.i + 1) % len(self.x)
            return lib.mctq_qconv_transposed_i8(self.x[self.i].data_ptr(), native.CODE_U8, 114, 0.02, self.w.data_ptr(), self.sc.data_ptr(),
                                                self.rowsum.data_ptr(), None, self.bias.data_ptr(), self.y[self.i].data_ptr(), *form,
                                                self.B, self.side, self.side, self.C, self.O, *self.geometry, S())
        return f


if "kernel" in args.sections:
    print("\n| C -> O | kernel | stride | pad, out pad | image | batch | ring sets | float32 out us | GB/s | Top/s | codes out us | GB/s | Top/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for (C, O, k, s, p, op, side) in SHAPES:
        for B in args.batches:
            c = RawCase(C, O, k, s, p, op, side, B)
            for codes_out in (False, True):
                assert c.call(codes_out)() == 0, lib.mctq_last_error()
            assert native.last_launch().startswith("qconv_transposed<")
            res = timed([("f32", c.call(False)), ("codes", c.call(True))], iters=200)
            gb = lambda out_bytes, us: (c.n_in + out_bytes * c.n_out) / us / 1e3            # noqa: E731
            tops = lambda us: 2.0 * c.macs * c.n_out / us / 1e6                             # noqa: E731
            print(f"| {C} -> {O} | {k}x{k} | {s} | {p}, {op} | {side} | {B} | {len(c.x)} | {res['f32'][0]:.2f} | {gb(4, res['f32'][0]):.0f} | "
                  f"{tops(res['f32'][0]):.2f} | {res['codes'][0]:.2f} | {gb(1, res['codes'][0]):.0f} | {tops(res['codes'][0]):.2f} |",
                  flush=True)
            del c
            torch.cuda.empty_cache()


def _quantizers(weight, axis, relu):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in weight.detach().abs().amax(tuple(d for d in range(4) if d != axis))]
        wq = Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=True, channel_axis=axis)
        aq = Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False) if relu else \
            Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-4.0], max_range=[4.0])
    return wq, aq


def pair(cin, cout, k, relu=False):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=True).to(dev)
    wq, aq = _quantizers(conv.weight, 0, relu)
    return [mq.PytorchActivationQuantizationHolder(aq).to(dev), mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)]


def pair_t(cin, cout, k, s, p=0, op=0, relu=False):
    conv = torch.nn.ConvTranspose2d(cin, cout, k, stride=s, padding=p, output_padding=op, bias=True).to(dev)
    wq, aq = _quantizers(conv.weight, 1, relu)
    return [mq.PytorchActivationQuantizationHolder(aq).to(dev), mq.PytorchQuantizationWrapper(conv, {"weight": wq}).to(dev)]


if "pairs" in args.sections:
    rows_md = []
    for (C, O, k, s, p, op, side) in SHAPES:
        torch.manual_seed(0)
        plain = torch.nn.Sequential(*pair_t(C, O, k, s, p, op, relu=True))
        torch.manual_seed(0)                                      # the same weights for both arms
        fused = torch.nn.Sequential(*pair_t(C, O, k, s, p, op, relu=True))
        assert consumers.fuse_linear_consumers(fused, transposed=True) == 1
        for B in args.batches:
            x = torch.rand(B, C, side, side, device=dev) * 8.0
            with torch.no_grad():
                ref, y = plain(x), fused(x)
                assert native.last_launch().startswith("qconv_transposed<")
                rel = float((y - ref).abs().max() / ref.abs().max())
                res = timed([("unfused", lambda: plain(x)), ("fused", lambda: fused(x))])
            u, f = res["unfused"], res["fused"]
            print(f"{C}->{O} {k}x{k}/{s} p{p} op{op} {side}x{side} batch {B}: unfused {u[0]:.1f} us ({u[1]:.1f} .. {u[2]:.1f}), fused {f[0]:.1f} us "
                  f"({f[1]:.1f} .. {f[2]:.1f}), max rel diff {rel:.1e}", flush=True)
            bold = "**" if f[0] > u[0] else ""                    # the feature slower: in bold
            rows_md.append(f"| {C} -> {O} | {k}x{k} | {s} | {p}, {op} | {side} | {B} | {u[0]:.1f} ({u[1]:.1f} .. {u[2]:.1f}) | "
                           f"{bold}{f[0]:.1f} ({f[1]:.1f} .. {f[2]:.1f}){bold} | {bold}{u[0] / f[0]:.2f}{bold} |")
        del plain, fused
        torch.cuda.empty_cache()
    print("\n| C -> O | kernel | stride | pad, out pad | image | batch | unfused pair us (least .. most) | fused pair us (least .. most) | unfused / fused |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


class Stage(torch.nn.Module):
    def __init__(self, C=128):
        super().__init__()
        self.h0, self.first = pair(C, C, 1)
        self.ha, self.up = pair_t(C, C // 2, 2, 2, relu=True)
        self.hb, self.hs, self.hc = (pair(16, 16, 1, relu=True)[0] for _ in range(3))
        self.last = pair(C, C // 2, 3, relu=True)[1]

    def forward(self, x, skip):
        b = self.hb(torch.relu(self.up(self.ha(torch.relu(self.first(self.h0(x)))))))
        return self.last(self.hc(torch.cat([b, self.hs(skip)], 1)))


if "stage" in args.sections:
    def stage():
        torch.manual_seed(0)
        return Stage().to(dev)

    every = dict(convolutions=True, depthwise=True, grouped=True, uniform_weights=True, shared_holders=True, stay_on_codes=True,
                 fused_residuals=True, pools=True, avg_pools=True, concats=True, muls=True, hard_activations=True, upsamples=True,
                 any_channels=True, activation_tables=True)
    print("\ndecoder stage, 128 -> 128 (1x1) -> 64 (transposed 2x2 / 2) -> cat with 64 skip channels -> 64 (3x3), 56 x 56 -> 112 x 112, eager forward")
    print("| batch | arm | layers fused | us per forward (least .. most) | max abs diff to as built / largest output |\n|---|---|---|---|---|")
    for B in args.batches:
        x, skip = torch.randn(B, 128, 56, 56, device=dev) * 2.0, torch.rand(B, 64, 112, 112, device=dev) * 8.0
        with torch.no_grad():
            plain = stage()
            ref = plain(x, skip)
            unit = float(ref.abs().max())
            arms, meta = [("as built", lambda: plain(x, skip))], {"as built": (0, 0.0)}
            for name, kw in (("fx, every switch, transposed=False", every), ("fx, every switch, transposed=True", dict(every, transposed=True))):
                gm, n = consumers.fuse_linear_consumers_fx(stage(), **kw)
                meta[name] = (n, float((gm(x, skip) - ref).abs().max()) / unit)
                arms.append((name, (lambda g: lambda: g(x, skip))(gm)))
            res = timed(arms, iters=max(5, args.iters // (5 if B > 8 else 1)))
        for name, _ in arms:
            r = res[name]
            print(f"| {B} | {name} | {meta[name][0]} | {r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f}) | {meta[name][1]:.1e} |", flush=True)
        del plain, arms
        torch.cuda.empty_cache()
