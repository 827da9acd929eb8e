"""Where does streaming packed 4-bit codebook indices beat the int8 consumer?  (consumers._LUT4_MAX_ROWS)

Three arms on the same product, in one process, alternating round by round on a ring of weight copies larger than the
256 MiB Infinity Cache (every launch streams its weights from HBM):
    int8   mctq_qlinear_i8 on the expanded codebook values (1 B per weight; the baseline)
    w4     mctq_qlinear_w4a8 (0.5 B per weight, two VALU operations per 8 weights)
    lut4   mctq_qlinear_lut4a8 (0.5 B per weight, decoded index -> int8 in registers)
Prints one line per (N, K, M, arm) with the median and the least microseconds per launch over the rounds, then per (N, K)
the largest probed M up to which lut4 is faster than int8 at every smaller probed M too, and the least of those.

    python tools/lut_consumer_probe.py [--iters 200] [--rounds 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mct_quantizers_amd.hip import native
from mct_quantizers_amd import consumers

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", type=int, nargs="*", default=[1, 8, 16, 32, 48, 64, 96, 128])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")
S = lambda: torch.cuda.current_stream().cuda_stream
LUT = [-120, 77, -2, 38, -96, 3, 127, -50, 11, -33, 100, -9, 24, -70, 55, -20]
lut_bytes = consumers._lut16_bytes(LUT)
lut_dev = torch.tensor(LUT, dtype=torch.int8, device=dev)
crossover = {}
for (N, K) in [(8192, 8192), (28672, 8192), (8192, 28672), (4096, 11008)]:
    ring = max(2, int(np.ceil(600e6 / (N * K))))             # int8 copies: 600 MB; packed copies: 300 MB
    idx = [torch.randint(0, 16, (N, K), dtype=torch.uint8, device=dev) for _ in range(ring)]
    w8 = [lut_dev[i.long()] for i in idx]
    i4 = [consumers.pack_lut4(i) for i in idx]
    w4 = [consumers.pack_w4(torch.randint(-8, 8, (N, K), dtype=torch.int8, device=dev)) for _ in range(ring)]
    del idx
    sc = torch.rand(N, device=dev) * 0.01
    wsum = w8[0].sum(1, dtype=torch.int32)
    bias = torch.randn(N, device=dev)
    best = 0
    still = True
    for M in args.rows:
        a = torch.randint(0, 256, (M, K), dtype=torch.uint8, device=dev)
        y = torch.empty(M, N, dtype=torch.float32, device=dev)

        def t8(i):
            lib.mctq_qlinear_i8(a.data_ptr(), native.CODE_U8, 114, 0.02, w8[i % ring].data_ptr(), sc.data_ptr(), wsum.data_ptr(),
                                bias.data_ptr(), y.data_ptr(), M, N, K, S())

        def t4(i):
            lib.mctq_qlinear_w4a8(a.data_ptr(), native.CODE_U8, 114, 0.02, w4[i % ring].data_ptr(), sc.data_ptr(), wsum.data_ptr(),
                                  bias.data_ptr(), y.data_ptr(), -1, 1.0, 0, 0, 0, M, N, K, S())

        def tl(i):
            lib.mctq_qlinear_lut4a8(a.data_ptr(), native.CODE_U8, 114, 0.02, i4[i % ring].data_ptr(), lut_bytes, sc.data_ptr(),
                                    wsum.data_ptr(), bias.data_ptr(), y.data_ptr(), -1, 1.0, 0, 0, 0, M, N, K, S())

        arms = (("int8", t8), ("w4", t4), ("lut4", tl))
        times = {name: [] for name, _ in arms}
        kernel = {}
        for name, f in arms:                                  # warm every arm before any timed window
            for i in range(5):
                f(i)
            kernel[name] = native.last_launch().split("<")[0]
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
        med = {name: float(np.median(v)) for name, v in times.items()}
        for name, _ in arms:
            print(f"N={N} K={K} M={M} {name:5s} median {med[name]:8.2f} us  min {min(times[name]):8.2f} us  [{kernel[name]}]", flush=True)
        wins = med["lut4"] < med["int8"]
        print(f"N={N} K={K} M={M} lut4 / int8 = {med['lut4'] / med['int8']:.3f}  lut4 / w4 = {med['lut4'] / med['w4']:.3f}", flush=True)
        still = still and wins
        if still:
            best = M
    crossover[(N, K)] = best
    print(f"N={N} K={K}: lut4 faster than int8 for every probed M <= {best}", flush=True)
    del w8, i4, w4
    torch.cuda.empty_cache()
print("largest probed M at which lut4 beats int8 on every shape:", min(crossover.values()), flush=True)
