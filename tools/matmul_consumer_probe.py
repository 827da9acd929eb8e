"""What does a matrix product on activation codes cost, and what does it save?  (consumers.QuantizedMatmul,
fuse_linear_consumers_fx(matmuls=True); include/mctq_hip.h: mctq_qmatmul_i8)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone (the raw entry point on prepared operands) and consumers.qmatmul_i8 (the Python route: its checks,
             the views, a re-pitch launch where K % 16 != 0), both forms -- "NT" Q.K^T: [B, H, T, D] x [B, H, T, D] -> [B, H, T, T] float32; "NN" P.V: [B, H, T, T] x
             [B, H, T, D] -> [B, H, T, D] codes -- on ViT-B/16 (12 heads, T = 197, D = 64) and BERT-base (12 heads, D = 64, T = 128
             and 384), the operands permuted views of [B, T, H, D] storage as an attention block makes them (the probabilities
             contiguous), against what it replaces: torch.matmul of the float32 holder outputs (on contiguous [B, H, T, D] copies,
             the layout that favours it), plus for NN the holder (ops.fq_per_tensor) and one quantize launch of its output
             (ops.fq_codes).  A K that is no multiple of 16 (T = 197 in NN) includes the re-pitch launch of the probabilities.
             Every launch takes the next set of a ring of buffers (at most 16 sets, about 6 GB in all, at least 5 sets for the largest case); outputs compared
             first: torch.equal for NT where the float32 product is exact, the largest difference otherwise
    block    workloads.wrapped_attention_block (dim 768, 12 heads, T = 197) through fuse_linear_consumers_fx with every switch,
             with and without matmuls=True; the largest relative difference of the outputs; library launches per forward
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md).  No threshold: figures are recorded.

    python tools/matmul_consumer_probe.py [--sections kernel block] [--iters 50] [--rounds 5] [--batches 1 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mct_quantizers_amd import consumers, workloads
from mct_quantizers_amd.hip import native, ops

ap = argparse.ArgumentParser()
ap.add_argument("--sections", nargs="*", default=["kernel", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

lib = native.load()
dev = torch.device("cuda")

# (name, heads, tokens, head dim)
SHAPES = [("vit-b/16", 12, 197, 64), ("bert-base", 12, 128, 64), ("bert-base", 12, 384, 64)]
RING_BYTES, RING_MAX = 6 << 30, 16
# (scale, zero point, qmin, qmax): Q / K / V holders (signed), the probabilities' holder, the context's holder
QKV_FORM, P_FORM, CTX_FORM = (4.0 / 128, 0, -128, 127), (1.0 / 256, 0, 0, 255), (2.0 / 128, 0, -128, 127)


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


class MatmulCase:
    """A ring of operand sets for one product -- codes as permuted views of [B, T, H, D] storage and the float32 holder outputs
    as contiguous [B, H, T, D] tensors -- and launchers that take the next set each time."""

    def __init__(self, B, H, T, D, nt):
        self.nt = nt
        per_set = B * H * T * (2 * D * 5 if nt else (T + D) * 5)
        sets = max(1, min(RING_MAX, RING_BYTES // per_set))
        gen = torch.Generator(device=dev).manual_seed(T + D + nt)
        self.a_codes, self.b_codes, self.a_f32, self.b_f32 = [], [], [], []
        for _ in range(sets):
            if nt:
                a = torch.randn(B, T, H, D, device=dev, generator=gen).permute(0, 2, 1, 3)
                a_form = QKV_FORM
            else:
                a = torch.softmax(torch.randn(B, H, T, T, device=dev, generator=gen) * 3, dim=-1)
                a_form = P_FORM
            b = torch.randn(B, T, H, D, device=dev, generator=gen).permute(0, 2, 1, 3)
            self.a_codes.append(ops.fq_codes(a, None, None, None, a_form[2], a_form[3], a_form[0], a_form[1]))
            self.b_codes.append(ops.fq_codes(b, None, None, None, QKV_FORM[2], QKV_FORM[3], QKV_FORM[0], QKV_FORM[1]))
            self.a_f32.append(ops.fq_per_tensor(a.contiguous(), *a_form))
            self.b_f32.append(ops.fq_per_tensor(b.contiguous(), *QKV_FORM))
        self.a_form, self.out_codes = a_form, None if nt else CTX_FORM
        # the raw launch's operands: the views as the Python route hands them over (the probabilities re-pitched where T % 16 != 0)
        self.a_view = [consumers._matmul_view(t, a_form[1], True) for t in self.a_codes]
        self.b_view = [consumers._matmul_view(t, QKV_FORM[1], nt) for t in self.b_codes]
        self.tdt, *self.form = consumers._output_form(self.out_codes)
        self.dims = (B, H, T, T if nt else D, D if nt else T)
        self.out = torch.empty(self.dims[:4], dtype=self.tdt, device=dev)
        self.i = 0

    def step(self):
        self.i = (self.i + 1) % len(self.a_codes)
        return self.i

    def raw(self):
        i = self.step()
        a, b = self.a_view[i], self.b_view[i]
        return lib.mctq_qmatmul_i8(a.data_ptr(), ops._code_of(a), self.a_form[1], self.a_form[0], *consumers._matmul_strides(a),
                                   b.data_ptr(), ops._code_of(b), QKV_FORM[1], QKV_FORM[0], *consumers._matmul_strides(b), int(self.nt),
                                   self.out.data_ptr(), *self.form, *self.dims, torch.cuda.current_stream().cuda_stream)

    def codes(self):
        i = self.step()
        return consumers.qmatmul_i8(self.a_codes[i], self.a_form[:2], self.b_codes[i], QKV_FORM[:2], transposed_b=self.nt,
                                    out_codes=self.out_codes)

    def matmul(self):
        i = self.step()
        return torch.matmul(self.a_f32[i], self.b_f32[i].transpose(-1, -2) if self.nt else self.b_f32[i])

    def holder(self, t):
        return ops.fq_per_tensor(t, *CTX_FORM)

    def quantize(self, t):
        return ops.fq_codes(t, None, None, None, CTX_FORM[2], CTX_FORM[3], CTX_FORM[0], CTX_FORM[1])

    def replaced(self):
        return self.matmul() if self.nt else self.quantize(self.holder(self.matmul()))


if "kernel" in args.sections:
    print("\n| product | form | batch | M x N x K per head | ring sets | kernel alone us (least .. most) | TOP/s | qmatmul_i8 us (launches) | "
          "float32 matmul us | holder us | quantize us | replaced chain us | replaced / kernel | replaced / qmatmul_i8 | outputs |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for name, H, T, D in SHAPES:
        for nt in (True, False):
            for B in args.batches:
                c = MatmulCase(B, H, T, D, nt)
                c.i = -1
                n0 = native.launch_count()
                got = c.codes()
                launches = native.launch_count() - n0
                c.i = -1
                assert c.raw() == 0, lib.mctq_last_error()
                assert torch.equal(c.out, got)               # the raw launch == the Python route
                c.i = -1
                want = c.replaced()
                if nt:
                    same = "torch.equal" if torch.equal(got, want) else f"max diff {float((got - want).abs().max()):.1e}"
                else:
                    same = f"{float((got != want).float().mean()) * 100:.3f} % of codes differ, by at most {int((got.int() - want.int()).abs().max())}"
                t = c.matmul()
                arms = [("raw", c.raw), ("codes", c.codes), ("matmul", c.matmul), ("replaced", c.replaced)]
                if not nt:
                    h = c.holder(t)
                    arms += [("holder", lambda: c.holder(t)), ("quantize", lambda: c.quantize(h))]
                res = timed(arms)
                M, N, K = (T, T, D) if nt else (T, D, T)
                ops_count = 2.0 * B * H * M * N * K
                print(f"| {name} | {'NT' if nt else 'NN'} | {B} | {M} x {N} x {K} | {len(c.a_codes)} | {fmt(res['raw'])} | "
                      f"{ops_count / res['raw'][0] / 1e6:.2f} | {fmt(res['codes'])} ({launches}) | {fmt(res['matmul'])} | "
                      f"{fmt(res['holder']) if not nt else '-'} | {fmt(res['quantize']) if not nt else '-'} | {fmt(res['replaced'])} | "
                      f"{res['replaced'][0] / res['raw'][0]:.2f} | {res['replaced'][0] / res['codes'][0]:.2f} | {same} |", flush=True)
                del c, t
                torch.cuda.empty_cache()


if "block" in args.sections:
    print("\n| model | batch | layers replaced (without / with matmuls) | library launches per forward | matmuls=False us (least .. most) | "
          "matmuls=True us (least .. most) | without / with | outputs |\n|---|---|---|---|---|---|---|---|", flush=True)
    switches = dict(chain=True, uniform_weights=True, convolutions=True, depthwise=True, shared_holders=True, stay_on_codes=True, pools=True,
                    fused_residuals=True, concats=True, avg_pools=True, muls=True, hard_activations=True, upsamples=True, any_channels=True,
                    activation_tables=True, grouped=True, transposed=True)
    make = lambda: workloads.wrapped_attention_block(dim=768, heads=12, tokens=197, device=dev)      # noqa: E731
    for B in args.batches:
        x = torch.randn(B, 197, 768, device=dev)
        with torch.no_grad():
            gm0, n0 = consumers.fuse_linear_consumers_fx(make(), **switches)
            gm, n = consumers.fuse_linear_consumers_fx(make(), matmuls=True, **switches)
            y, ref = gm(x), gm0(x)
            same = "torch.equal" if torch.equal(y, ref) else f"max rel diff {float((y - ref).abs().max() / ref.abs().max()):.1e}"
            count = lambda g: (native.launch_count(), g(x), native.launch_count())      # noqa: E731
            l0, l1 = (c[2] - c[0] for c in (count(gm0), count(gm)))
            res = timed([("off", lambda: gm0(x)), ("on", lambda: gm(x))], iters=20)
        a, b = res["off"], res["on"]
        print(f"| attention block 768 / 12 heads / 197 tokens | {B} | {n0} / {n} | {l0} / {l1} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:.3f} | {same} |",
              flush=True)
        del gm, gm0, x
        torch.cuda.empty_cache()
