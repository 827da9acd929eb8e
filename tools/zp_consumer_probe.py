"""What does a weight zero point cost on the integer consumer?  (consumers.qlinear_i8(..., w_zero_points=...))

Four arms on the same product, in one process, alternating round by round on a ring of weight copies larger than the
256 MiB Infinity Cache (every launch streams its weights from HBM, as tools/bench_consumer.py does):
    i8       mctq_qlinear_i8 (zero point 0; the baseline)
    rowsum   mctq_codes_rowsum alone (the extra launch of the zero-point form)
    zp       mctq_codes_rowsum + mctq_qlinear_i8_zp (what QuantizedLinear runs for uniform weights)
    wrapper  the path a uniform-weights layer takes without the consumer: fake-quantize the float32 weight and the
             activation, then the float32 F.linear
Prints one line per (N, K, M, arm) with the median and the least microseconds per launch over the rounds, then the
results as a markdown table (profiles/EXPERIMENTS.md).  No threshold: the figures are recorded, not judged.

    python tools/zp_consumer_probe.py [--iters 100] [--rounds 5] [--rows 1 16 64 256 1024] [--rowsum-only]
"""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import mct_quantizers_amd as mq
from mct_quantizers_amd.hip import native

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 64, 256, 1024])
ap.add_argument("--rowsum-only", action="store_true", help="the row-sum launch on both sides of its block / wave crossover")
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
Q = mq.pytorch_quantizers


def timed(arms):
    """arms: [(name, f(i))] -> {name: (median us, least us)}, rounds alternating between the arms"""
    times = {name: [] for name, _ in arms}
    for name, f in arms:                                      # warm every arm before any timed window
        for i in range(5):
            f(i)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, f in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.iters):
                f(i + r)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000 / args.iters)
    return {name: (float(np.median(v)), min(v)) for name, v in times.items()}


if args.rowsum_only:
    # the shipped dispatch beside the two forms forced (builds of tools/build_variant.py, when they are there):
    #   python tools/build_variant.py rs_block -DMCTQ_ROWSUM_BLOCK_ROWS=1073741824 --units=mctq_qlinear.hip
    #   python tools/build_variant.py rs_wave -DMCTQ_ROWSUM_BLOCK_ROWS=0 --units=mctq_qlinear.hip
    import ctypes
    forms = {"shipped": lib}
    for name in ("rs_block", "rs_wave"):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ablate", f"libmctq_hip_{name}.so")
        if os.path.exists(path):
            forms[name[3:]] = ctypes.CDLL(path)
            forms[name[3:]].mctq_codes_rowsum.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    print("| K | M | " + " | ".join(f"{n} us" for n in forms) + " | shipped form |\n|---|---|" + "---|" * (len(forms) + 1), flush=True)
    for K in (1024, 4096, 32768):
        for M in (1, 16, 32, 64, 65, 128, 256, 512, 1024, 4096):
            a = torch.randint(0, 256, (M, K), dtype=torch.uint8, device=dev)
            out = torch.empty(M, dtype=torch.int32, device=dev)
            call = lambda L: (lambda i: L.mctq_codes_rowsum(a.data_ptr(), native.CODE_U8, 114, out.data_ptr(), M, K, S()))
            assert lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_U8, 114, out.data_ptr(), M, K, S()) == 0
            form = native.last_launch().split("<")[1].split(",")[0]
            res = timed([(n, call(L)) for n, L in forms.items()])
            print(f"| {K} | {M} | " + " | ".join(f"{res[n][0]:.2f}" for n in forms) + f" | {form} |", flush=True)
    sys.exit(0)

rows_md = []
for (N, K) in [(4096, 4096), (11008, 4096)]:
    ring = max(2, int(np.ceil(400e6 / (N * K))))
    w8 = [torch.randint(-128, 128, (N, K), dtype=torch.int8, device=dev) for _ in range(ring)]
    fring = max(2, int(np.ceil(400e6 / (4 * N * K))))
    wf = [torch.randn(N, K, device=dev) * 0.4 + 0.3 for _ in range(fring)]
    sc = torch.rand(N, device=dev) * 0.01
    wsum = w8[0].sum(1, dtype=torch.int32)
    zw = torch.randint(-128, 128, (N,), dtype=torch.int32, device=dev)
    bias = torch.randn(N, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wq = Q.WeightsUniformInferableQuantizer(num_bits=8, min_range=[-0.9] * N, max_range=[1.5] * N, per_channel=True, channel_axis=0)
        aq = Q.ActivationUniformInferableQuantizer(num_bits=8, min_range=[-2.5], max_range=[3.1])
    for M in args.rows:
        a = torch.randint(0, 256, (M, K), dtype=torch.uint8, device=dev)
        x = torch.randn(M, K, device=dev)
        y = torch.empty(M, N, dtype=torch.float32, device=dev)
        ars = torch.empty(M, dtype=torch.int32, device=dev)

        def t_i8(i):
            lib.mctq_qlinear_i8(a.data_ptr(), native.CODE_U8, 114, 0.02, w8[i % ring].data_ptr(), sc.data_ptr(), wsum.data_ptr(),
                                bias.data_ptr(), y.data_ptr(), M, N, K, S())

        def t_rowsum(i):
            lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_U8, 114, ars.data_ptr(), M, K, S())

        def t_zp(i):
            lib.mctq_codes_rowsum(a.data_ptr(), native.CODE_U8, 114, ars.data_ptr(), M, K, S())
            lib.mctq_qlinear_i8_zp(a.data_ptr(), native.CODE_U8, 114, 0.02, w8[i % ring].data_ptr(), sc.data_ptr(), wsum.data_ptr(),
                                   bias.data_ptr(), y.data_ptr(), -1, 1.0, 0, 0, 0, zw.data_ptr(), ars.data_ptr(), M, N, K, S())

        def t_wrapper(i):
            torch.nn.functional.linear(aq(x), wq(wf[i % fring]), bias)

        kernel = {}
        t_i8(0); kernel["i8"] = native.last_launch().split("<")[0]
        t_zp(0); kernel["zp"] = native.last_launch().split("<")[0]
        t_rowsum(0); kernel["rowsum"] = native.last_launch().split(",")[0]
        kernel["wrapper"] = "fake-quant + F.linear"
        res = timed([("i8", t_i8), ("rowsum", t_rowsum), ("zp", t_zp), ("wrapper", t_wrapper)])
        for name in ("i8", "rowsum", "zp", "wrapper"):
            print(f"N={N} K={K} M={M} {name:7s} median {res[name][0]:9.2f} us  min {res[name][1]:9.2f} us  [{kernel[name]}]", flush=True)
        rows_md.append(f"| {M} | {N} x {K} | {res['i8'][0]:.1f} ({kernel['i8'].replace('qlinear_', '')}) | {res['rowsum'][0]:.1f} | "
                       f"{res['zp'][0]:.1f} ({kernel['zp'].replace('qlinear_', '')}) | {res['wrapper'][0]:.1f} | "
                       f"{res['zp'][0] / res['i8'][0]:.2f} | {res['wrapper'][0] / res['zp'][0]:.1f} |")
    del w8, wf
    torch.cuda.empty_cache()
print("\n| M | N x K | mctq_qlinear_i8 us | row sums us | row sums + _zp us | fake-quant + F.linear us | zp / i8 | wrapper / zp |")
print("|---|---|---|---|---|---|---|---|")
print("\n".join(rows_md), flush=True)
