"""A / B of two BUILDS of the library on mctq_qlinear_i8, both loaded into one process and timed alternately on the same
buffers over cold weights (a ring of weight copies larger than the Infinity Cache, as tools/bench_consumer.py).  Arm A is
timed twice per round (A1, A2): the spread of a build against itself in the same run is the difference that means nothing.

    python tools/qlinear_ab_probe.py --a parent --b shipped     (A = tools/ablate/libmctq_hip_parent.so: another commit's
                                                                 library copied there; B = mct_quantizers_amd/lib/libmctq_hip.so)
    python tools/qlinear_ab_probe.py --a parent --b shipped --shapes 16,4096,4096 1024,4096,4096 [--iters 200] [--rounds 7]
"""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from mct_quantizers_amd.hip import native

U8 = native.CODE_U8
ap = argparse.ArgumentParser()
ap.add_argument("--a", default="parent")
ap.add_argument("--b", default="shipped")
ap.add_argument("--shapes", nargs="*", default=["16,4096,4096", "64,4096,4096", "256,4096,4096", "1024,4096,4096"])
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
P, I64, I32, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float


def load(name):
    path = os.path.join(REPO, "mct_quantizers_amd", "lib", "libmctq_hip.so") if name == "shipped" else \
        os.path.join(REPO, "tools", "ablate", f"libmctq_hip_{name}.so")
    lib = ctypes.CDLL(path)
    lib.mctq_qlinear_i8.argtypes = [P, I32, I32, F32, P, P, P, P, P, I64, I64, I64, P]
    lib.mctq_last_launch.restype = ctypes.c_char_p
    return lib


A, B = load(args.a), load(args.b)
dev = torch.device("cuda")
stream = torch.cuda.current_stream().cuda_stream
print(f"A = {args.a}   B = {args.b}   (median / least us per launch over {args.rounds} rounds of {args.iters}; order A1 B A2 per round)", flush=True)
for shape in args.shapes:
    M, N, K = (int(v) for v in shape.split(","))
    ring = max(2, int(np.ceil(400e6 / (N * K))))
    ws = [torch.randint(-128, 128, (N, K), dtype=torch.int8, device=dev) for _ in range(ring)]
    a = torch.randint(0, 256, (M, K), dtype=torch.uint8, device=dev)
    sc = torch.rand(N, device=dev) * 0.01
    rs = ws[0].sum(1, dtype=torch.int32)
    bias = torch.randn(N, device=dev)
    ys = {k: torch.empty(M, N, device=dev) for k in "AB"}

    def call(lib, y):
        return lambda i: lib.mctq_qlinear_i8(a.data_ptr(), U8, 114, 0.02, ws[i % ring].data_ptr(), sc.data_ptr(),
                                             rs.data_ptr(), bias.data_ptr(), y.data_ptr(), M, N, K, stream)

    arms = [("A1", call(A, ys["A"]), A), ("B", call(B, ys["B"]), B), ("A2", call(A, ys["A"]), A)]
    names = {}
    for name, f, lib in arms:
        for i in range(ring + 5):
            assert f(i) == 0
        names[name] = lib.mctq_last_launch().decode().split("<")[0]
    torch.cuda.synchronize()
    A.mctq_qlinear_i8(a.data_ptr(), U8, 114, 0.02, ws[0].data_ptr(), sc.data_ptr(), rs.data_ptr(), bias.data_ptr(), ys["A"].data_ptr(), M, N, K, stream)
    B.mctq_qlinear_i8(a.data_ptr(), U8, 114, 0.02, ws[0].data_ptr(), sc.data_ptr(), rs.data_ptr(), bias.data_ptr(), ys["B"].data_ptr(), M, N, K, stream)
    torch.cuda.synchronize()
    same = torch.equal(ys["A"].view(torch.int32), ys["B"].view(torch.int32))
    times = {name: [] for name, _, _ in arms}
    for r in range(args.rounds):
        for name, f, _ in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.iters):
                f(i + r)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000 / args.iters)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = abs(med["A1"] - med["A2"]) / min(med["A1"], med["A2"])
    a_mid = 0.5 * (med["A1"] + med["A2"])
    print(f"M={M} N={N} K={K}  A1 {med['A1']:8.2f}/{min(times['A1']):8.2f}  B {med['B']:8.2f}/{min(times['B']):8.2f}  "
          f"A2 {med['A2']:8.2f}/{min(times['A2']):8.2f}   A-vs-A spread {100 * spread:.2f} %   B vs mean(A) {100 * (med['B'] / a_mid - 1):+.2f} %  "
          f"equal={same}  [A {names['A1']} | B {names['B']}]", flush=True)
    del ws
    torch.cuda.empty_cache()
