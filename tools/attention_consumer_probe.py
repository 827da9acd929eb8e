"""What does one fused launch for the core of an attention block save over the three launches it replaces?
(consumers.qattention_i8, consumers.QuantizedAttention, fuse_linear_consumers_fx(attentions=True); include/mctq_hip.h: mctq_qattention_i8)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   q, k, v codes as views of one fused [B, T, 3, H, D] tensor -> the context's codes: ``qattention_i8`` against
             ``qmatmul_i8`` -> ``ops.codes_softmax`` (the ``* D^-0.5`` prefix as a pre-table, padded pitch) -> ``qmatmul_i8``, the same
             build.  Every launch takes the next set of a ring of qkv tensors (cold inputs); outputs compared first
    block    workloads.wrapped_attention_block (dim 768, 12 heads, 197 tokens) through fuse_linear_consumers_fx with
             shared_holders, stay_on_codes, matmuls and softmaxes, with and without attentions=True
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md); every row that is slower with the feature
says so in its last column.

    python tools/attention_consumer_probe.py [--sections kernel block] [--iters 50] [--rounds 5] [--batches 1 64]
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

dev = torch.device("cuda")
SHAPES = [("ViT-B/16 12 x 197 x 197 x 64", 12, 197, 64), ("BERT 12 x 128 x 128 x 64", 12, 128, 64),
          ("BERT 12 x 384 x 384 x 64", 12, 384, 64), ("16 x 1024 x 1024 x 64", 16, 1024, 64)]
RING_BYTES, RING_MAX = 600 << 20, 16
QKV = (4.0 / 128, 0)                                                                          # the block's a_qkv
A0, A, B, C = (32.0 / 128, 0, -128, 127), (8.0 / 128, 0, -128, 127), (1.0 / 256, 0, 0, 255), (2.0 / 128, 0, -128, 127)


def timed(arms):
    """arms: [(name, f())] -> {name: (median us, least us, most us)}, rounds alternating between the arms"""
    times = {name: [] for name, _ in arms}
    for name, f in arms:                                      # warm every arm before any timed window
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, f in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000 / args.iters)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in times.items()}


def fmt(r):
    return f"{r[0]:.1f} ({r[1]:.1f} .. {r[2]:.1f})"


class Case:
    """A ring of fused qkv code tensors, and the two arms, each taking the next one every time."""

    def __init__(self, batch, heads, tokens, d):
        n = batch * tokens * 3 * heads * d
        sets = max(1, min(RING_MAX, RING_BYTES // (n + batch * heads * tokens * tokens * 2)))
        g = torch.Generator(device=dev).manual_seed(tokens)
        self.qkv = [torch.randint(-128, 128, (batch, tokens, 3, heads, d), device=dev, generator=g).to(torch.int8) for _ in range(sets)]
        self.pre = ops.code_table(lambda v: v * d ** -0.5, A0, A, dev)
        self.exp = torch.from_numpy(ops.softmax_exp_table(A[0]).view("int32")).to(dev)
        self.tokens, self.i = tokens, 0

    def views(self):
        self.i = (self.i + 1) % len(self.qkv)
        return self.qkv[self.i].permute(2, 0, 3, 1, 4)

    def fused(self):
        q, k, v = self.views()
        return consumers.qattention_i8(q, QKV, k, QKV, v, QKV, scores_form=A0, a_form=A, probs_form=B, pre_table=self.pre,
                                       exp_table=self.exp, out_codes=C)

    def three(self):
        q, k, v = self.views()
        s = consumers.qmatmul_i8(q, QKV, k, QKV, transposed_b=True, out_codes=A0)
        p = ops.codes_softmax(s, A, B, pre_table=self.pre, pad_to=16, exp_table=self.exp)
        return consumers.qmatmul_i8(p, B[:2], v, QKV, transposed_b=False, out_codes=C, a_padded_k=self.tokens)


with torch.no_grad():
    if "kernel" in args.sections:
        print("\n| heads x T x T x D | batch | ring sets | fused launch us (least .. most) | three launches us | three / fused | with the feature |")
        print("|---|---|---|---|---|---|---|", flush=True)
        for name, heads, tokens, d in SHAPES:
            for batch in args.batches:
                case = Case(batch, heads, tokens, d)
                case.i = -1
                got = case.fused()
                assert "qattention" in native.last_launch()
                case.i = -1
                assert torch.equal(got, case.three())
                r = timed([("fused", case.fused), ("three", case.three)])
                ratio = r["three"][0] / r["fused"][0]
                print(f"| {name} | {batch} | {len(case.qkv)} | {fmt(r['fused'])} | {fmt(r['three'])} | {ratio:.2f} | "
                      f"{'faster' if ratio > 1 else 'SLOWER'} |", flush=True)
                del case
                torch.cuda.empty_cache()
    if "block" in args.sections:
        print("\n| attention block 768 / 12 heads / 197 tokens | batch | matmuls + softmaxes us (least .. most) | + attentions us | ratio | with the feature |")
        print("|---|---|---|---|---|---|", flush=True)
        switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True)
        for batch in args.batches:
            base, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(768, 12, 197, device=dev), **switches)
            att, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(768, 12, 197, device=dev), attentions=True, **switches)
            x = torch.randn(batch, 197, 768, device=dev) * 1.5
            r = timed([("base", lambda: base(x)), ("att", lambda: att(x))])
            ratio = r["base"][0] / r["att"][0]
            print(f"| wrapped_attention_block | {batch} | {fmt(r['base'])} | {fmt(r['att'])} | {ratio:.2f} | {'faster' if ratio > 1 else 'SLOWER'} |",
                  flush=True)
