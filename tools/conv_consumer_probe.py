"""What does a k x k / strided convolution cost on the integer consumer?  (consumers.QuantizedConv2d,
fuse_linear_consumers*(convolutions=True); include/mctq_hip.h: mctq_codes_im2col_nhwc)

Sections, each in one process with its arms alternating round by round:
    im2col   mctq_codes_im2col_nhwc alone on ResNet-50's 3x3 shapes (stride 1, and the stride-2 first block of a stage) at
             batch 1 and 64: the shipped build beside the experiment builds that are there (tools/build_variant.py):
                 python tools/build_variant.py im2col_nt -DMCTQ_IM2COL_NT=1 --units=mctq_codes_im2col.hip
                 python tools/build_variant.py im2col_c2048 -DMCTQ_IM2COL_BLOCK_CHUNKS=2048 --units=mctq_codes_im2col.hip
             outputs of all builds compared byte for byte
    product  the same builds' launch FOLLOWED by mctq_qlinear_i8 (the shipped library's) on the patch matrix it wrote: what the
             stores' cache policy is worth to the reader of the matrix
    pairs    activation holder -> wrapped convolution, unfused (fake-quantize weight and activation, float32 conv2d) against
             fused (codes, patch matrix, integer product): the four 3x3 shapes and the three stride-2 1x1 downsample shapes of
             ResNet-50 at batch 1 and 64, NCHW float32 input
    resnet50 workloads.wrapped_resnet50 eager: as built / fuse_linear_consumers_fx(model) (what the rewrite took before:
             the 16 pointwise pairs) / fuse_linear_consumers_fx(model, convolutions=True) (+ the 16 3x3 pairs) / the unfused
             model's whole forward replayed from one hipGraph (accelerate(model, example_inputs))
Prints one line per measurement, then markdown tables (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/conv_consumer_probe.py [--sections im2col product pairs resnet50] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["im2col", "product", "pairs", "resnet50"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
ap.add_argument("--resnet-batch", type=int, default=64)
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
Q = mq.pytorch_quantizers

# (channels, image side, stride) of ResNet-50's 3x3 convolutions at 224 x 224; (C in, C out, side) of its strided downsamples
CONV3 = [(64, 56, 1), (128, 28, 1), (256, 14, 1), (512, 7, 1), (128, 56, 2), (256, 28, 2), (512, 14, 2)]
DOWN = [(256, 512, 56), (512, 1024, 28), (1024, 2048, 14)]


def timed(arms, iters=None):
    """arms: [(name, f())] -> {name: (median us, least us)}, rounds alternating between the arms"""
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
    return {name: (float(np.median(v)), min(v)) for name, v in times.items()}


forms = {"shipped": lib}
for name in ("im2col_nt", "im2col_c2048"):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ablate", f"libmctq_hip_{name}.so")
    if os.path.exists(path):
        forms[name[7:]] = ctypes.CDLL(path)
        forms[name[7:]].mctq_codes_im2col_nhwc.argtypes = native.SIGNATURES["mctq_codes_im2col_nhwc"][1]

if "im2col" in args.sections:
    print("\n| C | image | stride | batch | patches MB | " + " | ".join(f"{n} us" for n in forms) + " | shipped GB/s written |")
    print("|---|---|---|---|---|" + "---|" * (len(forms) + 1), flush=True)
    for (C, side, stride) in CONV3:
        for B in args.batches:
            x = torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev)
            so = (side + 2 - 3) // stride + 1
            outs = {n: torch.empty(B * so * so, 9 * C, dtype=torch.uint8, device=dev) for n in forms}
            call = lambda n: (lambda: forms[n].mctq_codes_im2col_nhwc(x.data_ptr(), outs[n].data_ptr(), B, side, side, C, 3, 3,
                                                                      stride, stride, 1, 1, 1, 1, 114, S()))
            for n in forms:
                assert call(n)() == 0
            torch.cuda.synchronize()
            assert all(torch.equal(outs[n], outs["shipped"]) for n in forms)
            res = timed([(n, call(n)) for n in forms], iters=200)
            mb = outs["shipped"].numel() / 1e6
            print(f"| {C} | {side} | {stride} | {B} | {mb:.2f} | " + " | ".join(f"{res[n][0]:.2f}" for n in forms)
                  + f" | {mb / res['shipped'][0] * 1e3:.0f} |", flush=True)


if "product" in args.sections:
    print("\n| C | image | batch | M x N x K | " + " | ".join(f"{n} + product us" for n in forms) + " | product alone us | product kernel |")
    print("|---|---|---|---|" + "---|" * (len(forms) + 2), flush=True)
    for (C, side, stride) in [c for c in CONV3 if c[2] == 1]:
        for B in args.batches:
            M, K = B * side * side, 9 * C
            x = torch.randint(0, 256, (B, side, side, C), dtype=torch.uint8, device=dev)
            w = torch.randint(-128, 128, (C, K), dtype=torch.int8, device=dev)
            sc, wsum = torch.rand(C, device=dev) * 0.01, w.sum(1, dtype=torch.int32)
            y = torch.empty(M, C, dtype=torch.float32, device=dev)
            outs = {n: torch.empty(M, K, dtype=torch.uint8, device=dev) for n in forms}

            def product(n):
                return lib.mctq_qlinear_i8(outs[n].data_ptr(), native.CODE_U8, 114, 0.02, w.data_ptr(), sc.data_ptr(), wsum.data_ptr(),
                                           None, y.data_ptr(), M, C, K, S())

            def both(n):
                def f():
                    forms[n].mctq_codes_im2col_nhwc(x.data_ptr(), outs[n].data_ptr(), B, side, side, C, 3, 3, 1, 1, 1, 1, 1, 1, 114, S())
                    product(n)
                return f

            want = None
            for n in forms:
                both(n)()
                torch.cuda.synchronize()
                want = y.clone() if want is None else want
                assert torch.equal(y, want)
            kernel = native.last_launch().split("<")[0].replace("qlinear_", "")
            res = timed([(n, both(n)) for n in forms] + [("product", lambda: product("shipped"))], iters=200)
            print(f"| {C} | {side} | {B} | {M} x {C} x {K} | " + " | ".join(f"{res[n][0]:.2f}" for n in forms)
                  + f" | {res['product'][0]:.2f} | {kernel} |", flush=True)


def pair(cin, cout, k, stride):
    torch.manual_seed(0)                                      # the same weights for both arms
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = [float(v) for v in conv.weight.detach().abs().amax((1, 2, 3))]
        wq = Q.WeightsSymmetricInferableQuantizer(num_bits=8, threshold=thr, per_channel=True, channel_axis=0)
        aq = Q.ActivationSymmetricInferableQuantizer(num_bits=8, threshold=[8.0], signed=False)
    return torch.nn.Sequential(mq.PytorchActivationQuantizationHolder(aq), mq.PytorchQuantizationWrapper(conv, {"weight": wq})).to(dev)


if "pairs" in args.sections:
    rows_md = []
    shapes = [(C, C, 3, s, side) for (C, side, s) in CONV3 if s == 1] + [(ci, co, 1, 2, side) for (ci, co, side) in DOWN]
    for (cin, cout, k, stride, side) in shapes:
        plain = pair(cin, cout, k, stride)
        fused = pair(cin, cout, k, stride)
        assert consumers.fuse_linear_consumers(fused, convolutions=True) == 1
        for B in args.batches:
            x = torch.rand(B, cin, side, side, device=dev) * 8.0
            with torch.no_grad():
                ref, y = plain(x), fused(x)
                kernel = native.last_launch().split("<")[0]
                rel = float((y - ref).abs().max() / ref.abs().max())
                codes = torch.randint(0, 256, (B, side, side, cin), dtype=torch.uint8, device=dev)
                res = timed([("unfused", lambda: plain(x)), ("fused", lambda: fused(x)),
                             ("im2col", lambda: ops.codes_im2col(codes, k, stride, k // 2, 1, 0))])
            print(f"{cin}->{cout} {k}x{k}/{stride} {side}x{side} batch {B}: unfused {res['unfused'][0]:.1f} us, fused {res['fused'][0]:.1f} us "
                  f"(im2col alone {res['im2col'][0]:.1f}) [{kernel}] max rel diff {rel:.1e}", flush=True)
            rows_md.append(f"| {cin} -> {cout} | {k}x{k} / {stride} | {side} | {B} | {res['unfused'][0]:.1f} | {res['fused'][0]:.1f} | "
                           f"{res['im2col'][0]:.1f} | {kernel.replace('qlinear_', '')} | {res['unfused'][0] / res['fused'][0]:.2f} |")
        del plain, fused
        torch.cuda.empty_cache()
    print("\n| channels | kernel / stride | image | batch | unfused pair us | fused pair us | im2col alone us | product kernel | unfused / fused |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows_md), flush=True)


if "resnet50" in args.sections:
    B = args.resnet_batch
    x = torch.randn(B, 3, 224, 224, device=dev)
    with torch.no_grad():
        plain = workloads.wrapped_resnet50()
        gm1, n1 = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50())
        gm2, n2 = consumers.fuse_linear_consumers_fx(workloads.wrapped_resnet50(), convolutions=True)
        ref = plain(x)
        d1, d2 = float((gm1(x) - ref).abs().max() / ref.abs().max()), float((gm2(x) - ref).abs().max() / ref.abs().max())
        arms = [("as built", lambda: plain(x)), (f"fx ({n1} pairs)", lambda: gm1(x)), (f"fx convolutions=True ({n2} pairs)", lambda: gm2(x))]
        try:
            captured = mq.accelerate(workloads.wrapped_resnet50(), example_inputs=(x,))
            arms.append(("as built, one hipGraph", lambda: captured(x)))
        except Exception as e:  # noqa: BLE001
            print(f"(whole-forward capture not available here: {e})")
        res = timed(arms, iters=max(2, args.iters // 5))
    print(f"\nwrapped ResNet-50, batch {B}, 224 x 224, eager forward; max |diff| / max |ref| of the logits: {d1:.1e} ({n1} pairs), {d2:.1e} ({n2} pairs)")
    print("| arm | ms per forward (median) | least |\n|---|---|---|")
    for name, _ in arms:
        print(f"| {name} | {res[name][0] / 1e3:.2f} | {res[name][1] / 1e3:.2f} |", flush=True)
