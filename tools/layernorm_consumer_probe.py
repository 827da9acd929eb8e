"""What does the LayerNorm of a transformer layer cost on activation codes, and what does it save?
(consumers.QuantizedLayerNorm, fuse_linear_consumers_fx(layernorms=True); include/mctq_hip.h: mctq_codes_layernorm)

Sections, each in one process with its arms alternating round by round; median and spread (least .. most) of the rounds:
    kernel   the launch alone -- A's codes in, B's codes out -- on ViT-B / BERT-base rows ([B * 197, 768], [B * 128, 768]), ViT-L
             ([B * 197, 1024]) and one 4096-wide row set at batch 1 and 64, against the chain it replaces on holder A's float32
             output: ATen's layer norm, holder B, one quantize launch.  Every launch takes the next set of a ring of buffers
             (at most 16 sets, about 1.2 GB in all: cold inputs); outputs compared with the CPU route first
    forms    wave form against block form (tuning key "layernorm_form") where both fit, same buffers
    grids    the auto grid against 2, 4 and 8 workgroups per CU and one worker per row (tuning key "layernorm_blocks")
    block    workloads.wrapped_encoder_block (dim 768, 12 heads, 197 tokens, hidden 3072) through fuse_linear_consumers_fx with
             shared_holders, stay_on_codes, matmuls and softmaxes, with and without layernorms=True; then where the outputs of
             the two arms part: the codes in front of and behind each norm, arm against arm
Prints one line per measurement, as markdown table rows (profiles/EXPERIMENTS.md); every row that is slower with the feature
says so in its last column.

    python tools/layernorm_consumer_probe.py [--sections kernel forms grids block] [--iters 50] [--rounds 5] [--batches 1 64]
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
ap.add_argument("--sections", nargs="*", default=["kernel", "forms", "grids", "block"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
args = ap.parse_args()

dev = torch.device("cuda")
SHAPES = [("ViT-B [B * 197, 768]", 197, 768), ("BERT-base [B * 128, 768]", 128, 768), ("ViT-L [B * 197, 1024]", 197, 1024),
          ("[B * 128, 4096]", 128, 4096)]
RING_BYTES, RING_MAX = 1200 << 20, 16
A, B = (8.0 / 128, 0, -128, 127), (4.0 / 128, 0, -128, 127)             # the encoder block's a_res and a_n2
EPS = 1e-5
CUS = torch.cuda.get_device_properties(0).multi_processor_count


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


def tuned(f, **keys):
    """``timed`` of ``f`` alone under the tuning ``keys``, which are reset behind it."""
    for key, value in keys.items():
        native.set_tuning(key, value)
    try:
        return fmt(timed([("f", f)])["f"])
    finally:
        for key in keys:
            native.set_tuning(key, 0)


class Case:
    """A ring of (holder A's float32 output, its codes) sets, and the two arms, each taking the next set every time."""

    def __init__(self, rows, L):
        n = rows * L
        sets = max(1, min(RING_MAX, RING_BYTES // (10 * n)))
        g = torch.Generator(device=dev).manual_seed(L)
        self.x = [ops.fq_per_tensor(torch.randn(rows, L, device=dev, generator=g) * 2.0, *A) for _ in range(sets)]
        self.codes = [ops.fq_codes(x, None, None, None, *A[2:], *A[:2]) for x in self.x]
        self.gamma = 1.0 + 0.25 * torch.randn(L, device=dev, generator=g)
        self.beta = 0.1 * torch.randn(L, device=dev, generator=g)
        self.L, self.i = L, 0

    def step(self):
        self.i = (self.i + 1) % len(self.x)
        return self.i

    def norm(self):
        return ops.codes_layernorm(self.codes[self.step()], A, B, self.gamma, self.beta, EPS)

    def chain(self):
        y = ops.fq_per_tensor(torch.nn.functional.layer_norm(self.x[self.step()], (self.L,), self.gamma, self.beta, EPS), *B)
        return ops.fq_codes(y, None, None, None, *B[2:], *B[:2])


with torch.no_grad():
    if {"kernel", "forms", "grids"} & set(args.sections):
        print(f"\n{CUS} CUs")
        print("| rows | batch | ring sets | layernorm on codes us (least .. most) | launch | wave form us | block form us | 2 / CU us | 4 / CU us | "
              "8 / CU us | one worker per row us | replaced chain us | chain / codes | off by one code vs chain | with the feature |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
        for name, tokens, L in SHAPES:
            for batch in args.batches:
                rows = batch * tokens
                case = Case(rows, L)
                want = ops.codes_layernorm(case.codes[0].cpu(), A, B, case.gamma.cpu(), case.beta.cpu(), EPS)
                case.i = -1
                got = case.norm()
                assert torch.equal(got.cpu(), want)
                launch = native.last_launch()
                case.i = -1
                off = (got.int() - case.chain().int()).abs()
                r = timed([("codes", case.norm), ("chain", case.chain)])
                forms, grids = {}, {}
                if "forms" in args.sections and L <= 2048:
                    forms = {form: tuned(case.norm, layernorm_form=form) for form in (1, 2)}
                if "grids" in args.sections:
                    workers = rows if L > 2048 else -(-rows // 4)
                    grids = {k: tuned(case.norm, layernorm_blocks=min(k * CUS, workers)) for k in (2, 4, 8) if k * CUS < workers}
                    grids["rows"] = tuned(case.norm, layernorm_blocks=workers) if workers <= 65536 else "-"
                ratio = r["chain"][0] / r["codes"][0]
                print(f"| {name} | {batch} | {len(case.x)} | {fmt(r['codes'])} | {launch} | {forms.get(1, '-')} | {forms.get(2, '-')} | "
                      f"{grids.get(2, '-')} | {grids.get(4, '-')} | {grids.get(8, '-')} | {grids.get('rows', '-')} | {fmt(r['chain'])} | "
                      f"{ratio:.2f} | {int((off > 0).sum())} of {off.numel()} (at most {int(off.max())}) | {'faster' if ratio > 1 else 'SLOWER'} |", flush=True)
                del case
                torch.cuda.empty_cache()
    if "block" in args.sections:
        print("\n| encoder block 768 / 12 heads / 197 tokens / hidden 3072 | batch | without layernorms us (least .. most) | with layernorms us | ratio | "
              "max difference in steps of the last holder | with the feature |")
        print("|---|---|---|---|---|---|---|", flush=True)
        switches = dict(shared_holders=True, stay_on_codes=True, matmuls=True, softmaxes=True)
        stages = []
        for batch in args.batches:
            base, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(768, 12, 197, 3072, device=dev), **switches)
            norm, _ = consumers.fuse_linear_consumers_fx(workloads.wrapped_encoder_block(768, 12, 197, 3072, device=dev), layernorms=True, **switches)
            x = torch.randn(batch, 197, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(batch)) * 1.5
            # where the two arms part: each norm's input and output in the base arm (float32, coded here in the node's forms)
            # against the node's codes in the other arm
            seen, hooks = {}, []
            for name, node in (("attn.norm", "attn_a_in_layernorm"), ("norm2", "a_n2_layernorm")):
                hooks.append(base.get_submodule(name).register_forward_hook(lambda m, a, out, k=name: seen.__setitem__(k, (a[0], out))))
                hooks.append(norm.get_submodule(node).register_forward_hook(lambda m, a, out, k=node: seen.__setitem__(k, (a[0], out))))
            d = (base(x) - norm(x)).abs() / consumers._code_form(base.a_out.activation_holder_quantizer)[0]
            steps = d.max().item()
            stages.append(f"batch {batch}: output elements that differ {int((d > 0).sum())} of {d.numel()}, by at most {steps:.0f} steps")
            for name, node in (("attn.norm", "attn_a_in_layernorm"), ("norm2", "a_n2_layernorm")):
                q = norm.get_submodule(node)
                for what, form, i in (("input", q.activation_code_params(), 0), ("output", q.output_code_params(), 1)):
                    want = ops.fq_codes(seen[name][i], None, None, None, *form[2:], *form[:2])
                    off = (seen[node][i].int() - want.int()).abs()
                    stages.append(f"batch {batch}: {node} {what} codes that differ {int((off > 0).sum())} of {off.numel()}, by at most {int(off.max())}")
            for h in hooks:
                h.remove()
            r = timed([("base", lambda: base(x)), ("norm", lambda: norm(x))])
            ratio = r["base"][0] / r["norm"][0]
            print(f"| wrapped_encoder_block | {batch} | {fmt(r['base'])} | {fmt(r['norm'])} | {ratio:.2f} | {steps:.2f} | "
                  f"{'faster' if ratio > 1 else 'SLOWER'} |", flush=True)
        print("\nwhere the two arms of the block part (seeded inputs):\n" + "\n".join(stages), flush=True)
