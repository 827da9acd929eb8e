#!/usr/bin/env python3
"""Codebook-index codes of the LUT quantizers against the two things a user would otherwise do, all arms in ONE process
on the same buffers, timed alternately (two passes over the arms), with tools/ab_probe.py's protocol per arm (0.4 s
pre-warm, a ring of buffers larger than the 256 MiB Infinity Cache, HIP events around 100 launches, best / median of 5).

  A   q(w): the fused fake-quant launch mctq_lutt_per_channel / _per_tensor      8 B / element
  A'  the same launch again: the same-process spread of A, the margin the other arms are judged with
  B   the ATen chain (lut[codes.long()] / mult) * thr on the same codes           what the decode replaces
  C   decode, uint8 codes    5 B / element        D   decode, packed 4-bit codes   4.5 B / element (16 entries only)
  E   encode, uint8 codes    5 B / element        F   encode, packed 4-bit codes   4.5 B / element

    python tools/lut_codes_probe.py [--quick]

Prints microseconds per launch and algorithmic bytes / time as a fraction of 8 TB/s; C, D, E, F are checked against A
(bit-equal round trip) before anything is timed."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mct_quantizers_amd.hip import native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="one shape, 16 entries")
args = ap.parse_args()
lib = native.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
U8, U4 = native.CODE_U8, native.CODE_U4
MULT, CMIN, CMAX = 128.0, -128.0, 127.0


def timed(call, pre=0.4, n=100, reps=5):
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < pre:
        call(k)
        k += 1
        if k % 128 == 0:
            torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / n)
    out.sort()
    return out[0], out[len(out) // 2]


def codebook(n_lut):
    if n_lut == 16:
        return np.asarray([-128, -96, -64, -40, -24, -12, -5, 0, 5, 12, 24, 40, 64, 96, 120, 127], dtype=np.float32)
    return np.random.default_rng(6).permutation(np.arange(-128, 128)).astype(np.float32)


def check(rc):
    assert rc == 0, lib.mctq_last_error()


def case(rows, cols, kind, n_lut):
    n = rows * cols
    lutv = codebook(n_lut)
    lut = torch.from_numpy(lutv).to(dev)
    vtab = torch.from_numpy(native.build_lut_table(lutv, MULT, CMIN, CMAX)).to(dev)
    itab = torch.from_numpy(native.build_lut_index_table(lutv, MULT, CMIN, CMAX)).to(dev)
    entries = vtab.shape[0] - 1
    ring = min(16, max(2, -(-(512 << 20) // int(n * 4.5)) + 1))
    xs = [torch.randn(rows, cols, device=dev) * 1.5 for _ in range(ring)]
    ys = [torch.empty(rows, cols, device=dev) for _ in range(ring)]
    cs = [torch.empty(rows, cols, dtype=torch.uint8, device=dev) for _ in range(ring)]
    c4 = [torch.empty(rows, cols // 2, dtype=torch.uint8, device=dev) for _ in range(ring)]
    if kind == "pt":
        geo, C, thr_b = None, 1, None
    elif kind == "pc0":
        geo, C, thr_b = (1, rows, cols), rows, (rows, 1)
    else:
        geo, C, thr_b = (rows, cols, 1), cols, (1, cols)
    thr = torch.rand(C, device=dev) + 3.5
    thr0 = float(thr[0].item())
    div0 = float(np.float32(thr0) + np.float32(1e-8))

    def fq(i):
        x, y = xs[i % ring].data_ptr(), ys[i % ring].data_ptr()
        if geo is None:
            return lib.mctq_lutt_per_tensor(x, y, n, 0, 0, div0, thr0, vtab.data_ptr(), entries, MULT, CMIN, CMAX, stream)
        return lib.mctq_lutt_per_channel(x, y, *geo, 0, thr.data_ptr(), 1e-8, vtab.data_ptr(), entries, MULT, CMIN, CMAX, stream)

    def enc(code, outs):
        def call(i):
            x, c = xs[i % ring].data_ptr(), outs[i % ring].data_ptr()
            if geo is None:
                return lib.mctq_lut_codes_per_tensor(x, c, n, 0, code, 0, div0, lut.data_ptr(), n_lut, itab.data_ptr(), entries,
                                                     MULT, CMIN, CMAX, stream)
            return lib.mctq_lut_codes_per_channel(x, c, *geo, 0, code, thr.data_ptr(), 1e-8, lut.data_ptr(), n_lut,
                                                  itab.data_ptr(), entries, MULT, CMIN, CMAX, stream)
        return call

    def dec(code, ins):
        def call(i):
            c, y = ins[i % ring].data_ptr(), ys[i % ring].data_ptr()
            if geo is None:
                return lib.mctq_lut_decode_per_tensor(c, y, n, code, lut.data_ptr(), n_lut, MULT, thr0, stream)
            return lib.mctq_lut_decode_per_channel(c, y, *geo, code, lut.data_ptr(), n_lut, MULT, thr.data_ptr(), stream)
        return call

    thr_view = thr0 if geo is None else thr.reshape(thr_b)

    def aten(i):
        ys[i % ring] = (lut[cs[i % ring].long()] / MULT) * thr_view

    # correctness first: codes of every ring slot, round trip against the fused launch
    use4 = n_lut <= 16
    for i in range(ring):
        check(enc(U8, cs)(i))
        if use4:
            check(enc(U4, c4)(i))
    check(fq(0))
    want = ys[0].clone()
    ys[0].zero_()
    check(dec(U8, cs)(0))
    dec_name = lib.mctq_last_launch().decode()
    ok = torch.equal(want.view(torch.int32), ys[0].view(torch.int32))
    if use4:
        ys[0].zero_()
        check(dec(U4, c4)(0))
        ok = ok and torch.equal(want.view(torch.int32), ys[0].view(torch.int32))
    aten(0)
    ok = ok and torch.equal(want.view(torch.int32), ys[0].view(torch.int32))
    torch.cuda.synchronize()

    arms = [("A  q(w) fused", 8.0, fq), ("A' q(w) again", 8.0, fq), ("B  ATen chain", 5.0, aten), ("C  decode u8", 5.0, dec(U8, cs)),
            ("E  encode u8", 5.0, enc(U8, cs))]
    if use4:
        arms += [("D  decode u4", 4.5, dec(U4, c4)), ("F  encode u4", 4.5, enc(U4, c4))]
    res = {name: [] for name, _, _ in arms}
    for _ in range(2):
        for name, _, call in arms:
            res[name].append(timed(call))
    label = f"{rows}x{cols} {kind} lut{n_lut}"
    print(f"--- {label}  ring {ring}  round trip bit-equal: {ok}  [{dec_name}]", flush=True)
    med = {}
    for name, bpe, _ in arms:
        best = min(r[0] for r in res[name])
        med[name] = min(r[1] for r in res[name])
        cells = "  ".join(f"{lo:7.2f}/{m:7.2f}" for lo, m in res[name])
        print(f"{label:26s} {name:14s} {cells}   median {med[name]:7.2f} us   best {best:7.2f} us   "
              f"{n * bpe / med[name] / 8e6:.3f} of 8 TB/s", flush=True)
    a, a2 = med["A  q(w) fused"], med["A' q(w) again"]
    line = f"{label:26s} vs A ({a:.2f} us, A'/A {a2 / a:.3f}):"
    for name, _, _ in arms[2:]:
        line += f"  {name[0]} {med[name] / a:.3f}"
    line += f"   C/B {med['C  decode u8'] / med['B  ATen chain']:.4f}"
    print(line, flush=True)
    del xs, ys, cs, c4
    torch.cuda.empty_cache()


print("us per launch as best/median of 5, two passes over the arms; bytes = algorithmic bytes per element x elements", flush=True)
shapes = [(4096, 4096, "pc0")] if args.quick else [(4096, 4096, "pc0"), (4096, 4096, "pc1"), (16384, 1024, "pc0"), (11008, 4096, "pt")]
for rows, cols, kind in shapes:
    for n_lut in ((16,) if args.quick else (16, 256)):
        case(rows, cols, kind, n_lut)
