"""What does the softmax of an attention block cost on activation codes, and what does it save?
(consumers.QuantizedSoftmax, fuse_linear_consumers_fx(softmaxes=True); include/mctq_hip.h: mctq_codes_softmax)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone -- scores' codes in, the ``* scale`` prefix as a pre-table, probabilities' codes out at the padded
             pitch -- on ViT-B/16 (12 x 197 x 197) and BERT (12 heads, T = 128 and 384) at batch 1 and 64, against the chain it
             replaces on the float32 scores: holder, ``* scale``, holder, ATen's softmax, holder, one quantize launch and, where
             T % 16 != 0, the re-pitch launch of the product behind.  Every launch takes the next set of a ring of buffers (at
             most 16 sets, about 1.2 GB in all: cold inputs); outputs compared with the CPU route first
    forms    wave form against block form (tuning key "softmax_form") on the same rows, same buffers
    block    workloads.wrapped_attention_block (dim 768, 12 heads, 197 tokens) through fuse_linear_consumers_fx with
             shared_holders, stay_on_codes and matmuls, with and without softmaxes=True
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md); every row that is slower with the feature
says so in its last column.

    python tools/softmax_consumer_probe.py [--sections kernel forms block] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

dev = torch.device("cuda")
SHAPES = [("ViT-B/16 12 x 197 x 197", 12, 197), ("BERT 12 x 128 x 128", 12, 128), ("BERT 12 x 384 x 384", 12, 384)]
RING_BYTES, RING_MAX = 1200 << 20, 16
A0, A, B = (32.0 / 128, 0, -128, 127), (8.0 / 128, 0, -128, 127), (1.0 / 256, 0, 0, 255)     # the block's a_scores, a_scaled, a_probs
SCALE = 0.125


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
    """A ring of (float32 scores, their codes) sets, and the two arms, each taking the next set every time."""

    def __init__(self, batch, heads, tokens):
        n = batch * heads * tokens * tokens
        sets = max(1, min(RING_MAX, RING_BYTES // (5 * n)))
        g = torch.Generator(device=dev).manual_seed(tokens)
        self.x = [torch.randn(batch, heads, tokens, tokens, device=dev, generator=g) * 6.0 for _ in range(sets)]
        self.codes = [ops.fq_codes(x, None, None, None, *A0[2:], *A0[:2]) for x in self.x]
        self.pre = ops.code_table(lambda v: v * SCALE, A0, A, dev)
        self.exp = torch.from_numpy(ops.softmax_exp_table(A[0]).view("int32")).to(dev)
        self.tokens, self.n, self.i = tokens, n, 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def softmax(self):
        return ops.codes_softmax(self.codes[self.step()], A, B, pre_table=self.pre, pad_to=16, exp_table=self.exp)

    def chain(self):
        x = ops.fq_per_tensor(self.x[self.step()], *A0) * SCALE
        p = ops.fq_per_tensor(torch.softmax(ops.fq_per_tensor(x, *A), -1), *B)
        c = ops.fq_codes(p, None, None, None, *B[2:], *B[:2])
        return c if self.tokens % 16 == 0 else ops.codes_im2col(c.reshape(-1, self.tokens), 1, pad_to=16, pad_code=B[1])


with torch.no_grad():
    if "kernel" in args.sections or "forms" in args.sections:
        print("\n| scores | batch | ring sets | softmax on codes us (least .. most) | wave form us | block form us | replaced chain us | "
              "chain / codes | with the feature |")
        print("|---|---|---|---|---|---|---|---|---|", flush=True)
        for name, heads, tokens in SHAPES:
            for batch in args.batches:
                case = Case(batch, heads, tokens)
                want = ops.codes_softmax(case.codes[0].cpu(), A, B, pre_table=case.pre.cpu(), pad_to=16)
                case.i = -1
                assert torch.equal(case.softmax().cpu(), want)
                r = timed([("codes", case.softmax), ("chain", case.chain)])
                forms = {}
                for form in (1, 2) if "forms" in args.sections else ():
                    native.set_tuning("softmax_form", form)
                    try:
                        forms[form] = fmt(timed([("f", case.softmax)])["f"])
                    finally:
                        native.set_tuning("softmax_form", 0)
                ratio = r["chain"][0] / r["codes"][0]
                print(f"| {name} | {batch} | {len(case.x)} | {fmt(r['codes'])} | {forms.get(1, '-')} | {forms.get(2, '-')} | {fmt(r['chain'])} | "
                      f"{ratio:.2f} | {'faster' if ratio > 1 else 'SLOWER'} |", flush=True)
                del case
                torch.cuda.empty_cache()
    if "block" in args.sections:
        print("\n| attention block 768 / 12 heads / 197 tokens | batch | matmuls us (least .. most) | matmuls + softmaxes us | ratio | with the feature |")
        print("|---|---|---|---|---|---|", flush=True)
        switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True)
        for batch in args.batches:
            base, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(768, 12, 197, device=dev), **switches)
            soft, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_attention_block(768, 12, 197, device=dev), softmaxes=True, **switches)
            x = torch.randn(batch, 197, 768, device=dev) * 1.5
            r = timed([("base", lambda: base(x)), ("soft", lambda: soft(x))])
            ratio = r["base"][0] / r["soft"][0]
            print(f"| wrapped_attention_block | {batch} | {fmt(r['base'])} | {fmt(r['soft'])} | {ratio:.2f} | {'faster' if ratio > 1 else 'SLOWER'} |",
                  flush=True)
