#!/usr/bin/env python3
"""Benchmark of the inferable-quantizer hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2|...|resnet50] [--batched T] [--batch N]
                    [--dump-outputs DIR] [--full [--no-cpu] ...] ...

A *step* is one call of the configuration's quantizer (through the public class, hence through the
C ABI and the gfx950 kernel) on one device-resident synthetic tensor.  Default workload: BASELINE
config 2, WeightsSymmetricInferableQuantizer per-channel (axis 0) 8-bit on 4096x4096 float32.
``--batched T``: a step is ONE batched launch over T such tensors (the launch a wrapped model issues per forward,
pytorch/batching.py -> mctq_fq_batch_run; reference call site pytorch/quantize_wrapper.py:228-240), algorithmic bytes
T x 128 MiB per launch.  ``--config resnet50`` / ``linear16``: a step re-quantizes ALL weight tensors of that model (54
tensors, 25.5 M elements / 16 x 4096^2), each with its own per-channel quantizer, in ONE table launch.

Protocol
  * cache: the 128 MiB in+out working set of config 2 fits the 256 MiB Infinity Cache, so the steps rotate
    over RING distinct (input, output) buffer pairs whose total footprint exceeds it: every launch streams
    from/to HBM ("cold").  ``--ring 1`` measures the warm case.
  * clocks: before the W warm-up steps the same step loop runs for a FIXED, declared duration
    (``--prewarm-seconds``, default 1.0 s; reported as ``prewarm_s``) so that a 20-step run and a 1000-step run
    see the same clocks and a warm caching allocator.  It is outside the timed region.
  * timed region: exactly K steps between barrier + synchronize on both sides (at N > 1 a rank's clock stops when its
    own device has finished its K steps; the closing barrier follows and rank 0 takes the MAX over ranks).  Three clocks,
    one claim each:
      - the host wall clock gives ``value``, ``ms_per_step``, ``achieved_gbs`` and ``roofline.frac_wall``;
      - (only when there is no steady part -- hipGraph replay, several streams -- HIP events around the K launches give
        ``roofline.frac_events_whole_region``; otherwise that field repeats ``frac_wall``: every marker inside the region
        costs ~5 us of stream time, so the judged region carries two, not three);
      - the event behind the FIRST launch to the event behind the LAST gives ``roofline.kernel_us`` / ``achieved`` /
        ``frac``: the average launch period of launches 2..K, bubbles between launches included -- the figure that
        rocprofv3's average kernel duration (profiles/) must agree with.
  * ``--dump-outputs DIR``: right after the timed region the output(s) of the LAST timed step are written to DIR as .npy
    (float32; float64 for float64 tensors; a fixed seeded sample of each beyond 64 MB in all -- dump_outputs).  The
    inputs are the portable synthetic tensors, identical from run to run, so two builds can be compared output for output.
  * a plain run stops there: set-up, pre-warm, W warm-up steps, the K timed steps, the dump, the line.  Everything
    below marked --full runs only with ``--full``, after the judged region.
  * --full, per-launch evidence: >= 50 launches with an event between every two;
    median / mean / p10 / p90 of the per-launch periods are reported under ``roofline.per_launch``.
  * ``roofline.traffic`` is emitted only when profiles/pmc_traffic.json holds counters taken on the SAME kernel
    variant (``mctq_last_launch()``) of the SAME library build (``mctq_build_id()``) this run launched; otherwise null
    with the reason (``traffic_build_id_mismatch``).
  * --full, the parity check compares the output of the LAST timed step with the CPU oracle.
  * --full at N = 1 appends ``batched_16x4096``: the same tensor 16 times in one batched launch, measured
    after the judged region with the same event protocol (``--no-batched-extra`` skips it).

``--gpus N`` with N > 1 and no RANK in the environment: the script starts ``python -m torch.distributed.run`` on
itself as a child process (before anything touches the GPU) and relays its output and exit status; launched by
torch.distributed.run directly it is one rank.  Every rank runs the same per-GPU workload (weak scaling; the path
needs no collective); ``value`` is the sum over ranks divided by the slowest rank's time.  With --full, BASELINE config 5
sharded by dim 0 + ONE all-gather (RCCL) is measured outside the timed region and reported as ``sharded_cfg5`` plus the
top-level ``sharded_cfg5_*`` fields (``--gather`` runs it without --full too, and at N = 1 under torchrun).

With --full, self-verifying at every N: each rank compares the SHA-256 of the output of its last timed step with the REFERENCE's digest
(``ranks_parity_ok``), and of its config-5 shard with the reference's digest of that row block
(``sharded_cfg5.ranks_shard_digest_ok``); one mismatch -> ``parity_error`` and exit status 3.  Rank 0 runs the
``cpu_baseline`` leg at every N.  With N > 1 the job exits non-zero instead of printing a line when RCCL cannot form the
group (status 6) or the sharded config-5 leg fails (status 7) -- unless ``--allow-gloo`` is given (rehearsals on fewer GPUs
than ranks: gloo control plane, gather staged through the host; the line says so).

``--device cpu`` is a dry run of the entry path (launcher, process group over gloo, barriers, max-over-ranks, JSON)
on the config-1 plumbing workload for the CPU test-suite; its line says so and is not a measurement.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench_dist  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec (guide MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)
HBM_COPY_GBS = 6290.0
BASELINE_METRIC = "elems/s + achieved HBM GB/s, per-channel symmetric 4096×4096 fp32"
DUMP_BUDGET_BYTES = 64 * 10**6  # --dump-outputs: all .npy files together, headers included
DUMP_SEED = 0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", default="cfg2", choices=["cfg1", "cfg2", "cfg3", "cfg4", "cfg5", "resnet50", "linear16", "sym"],
                    help="cfg1..cfg5: the BASELINE configurations; resnet50 / linear16: ALL weights of that model re-quantized "
                         "in one batched launch per step (what a wrapped model does per forward); sym: WeightsSymmetric 8 bit "
                         "per channel along --axis of a tensor of --shape (the launch shapes no BASELINE configuration has: "
                         "channel-last, short and ragged rows)")
    ap.add_argument("--shape", default="4096x4096", help="--config sym: the tensor's shape, e.g. 4096x4096 or 64x56x56x256")
    ap.add_argument("--axis", type=int, default=0, help="--config sym: the channel axis")
    ap.add_argument("--per-tensor", action="store_true", help="--config sym: one threshold for the whole tensor (the per-tensor launch) instead of one per channel")
    ap.add_argument("--batched", type=int, default=0,
                    help="T > 0: a step is ONE batched launch over T tensors of the configuration (affine configs)")
    ap.add_argument("--batch", type=int, default=64, help="N of config 3")
    ap.add_argument("--ring", type=int, default=0, help="buffer pairs to rotate over (0 = enough to exceed 512 MiB)")
    ap.add_argument("--prewarm-seconds", type=float, default=1.0,
                    help="fixed-duration run of the step loop before the warm-up steps (clocks, allocator); declared in the output")
    ap.add_argument("--evidence-launches", type=int, default=200,
                    help="--full: launches of the per-launch event-pair pass after the timed region (0 = skip)")
    ap.add_argument("--nt", type=int, default=None)
    ap.add_argument("--cached-store-max-mb", type=int, default=None,
                    help="tuning key cached_store_max_mb: outputs up to this size are stored through the caches (default 32)")
    ap.add_argument("--unroll", type=int, default=None)
    ap.add_argument("--heavy-unroll", type=int, default=None)
    ap.add_argument("--rowsteps", type=int, default=None, help="tuning key rowsteps (include/mctq_hip.h): 1 = rowsteps_kernel for short whole-step rows")
    ap.add_argument("--paced", type=int, default=None, help="tuning key paced (include/mctq_hip.h): 0 = per-tensor launches never through flat_paced_kernel")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-batched-extra", action="store_true", help="skip the batched_16x4096 object of a --full run")
    ap.add_argument("--no-eager-extra", action="store_true",
                    help="config 3: skip the eager per-call figure (profiler passes: only the judged kernel's dispatches)")
    ap.add_argument("--gather", action="store_true", help="run the sharded config-5 + all-gather leg even at N = 1 (needs torchrun)")
    ap.add_argument("--no-sharded-extra", action="store_true",
                    help="N = 1 without a launcher: skip the sharded config-5 + all-gather leg (a process group of one rank formed "
                         "in-process after everything else, so that the three series of SURVEY 8(e) exist at every N)")
    ap.add_argument("--graph", action="store_true", help="replay the timed steps from one hipGraph")
    ap.add_argument("--extras", action="store_true",
                    help="after the judged region also measure: two-stream overlap, warm-cache rate, ATen's HIP operator")
    ap.add_argument("--streams", type=int, default=1,
                    help="issue independent steps round-robin on this many HIP streams (default 1: the judged protocol)")
    ap.add_argument("--stream-depth", type=int, default=0,
                    help="config 3: batches per replay of the activation stream (pytorch/graphs.py: CapturedStream; one fused "
                         "batched launch per D batches).  0 = automatic (on for --batch <= 64, D = the largest divisor of "
                         "--steps that is <= 32 and <= steps / 2), -1 = off (one eager call per batch)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16"],
                    help="STORAGE type of the tensors (arithmetic is float32 always): bf16 / f16 = SURVEY 8(f3), the affine "
                         "kernels read and write 2 B per element (4 B/el algorithmic), the LUT kernels read 2 and write 4")
    ap.add_argument("--e2e", action="store_true",
                    help="with --config resnet50: a step is one FORWARD of a wrapped ResNet-50 loaded through "
                         "pytorch_load_quantized_model (per-layer vs auto-batched vs captured; bench_e2e.py)")
    ap.add_argument("--e2e-lut", action="store_true", help="--e2e with 16-entry LUT weights quantizers")
    ap.add_argument("--e2e-side", type=int, default=224, help="--e2e: image side")
    ap.add_argument("--allow-gloo", action="store_true",
                    help="N > 1 only: accept a gloo control plane when RCCL cannot form the group (rehearsal of the entry path "
                         "on a box with fewer GPUs than ranks); without it such a run exits with status 6, and a run whose "
                         "sharded config-5 leg did not execute with status 7")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="cpu: dry run of the entry path over gloo (tests); not a measurement")
    ap.add_argument("--full", action="store_true",
                    help="after the judged region also run every side leg: the digest parity check (ranks_parity_ok), the "
                         "per-launch evidence pass, config 3's eager figure, batched_16x4096, the sharded config-5 leg and the "
                         "CPU baseline.  Without it a run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (float32, or float64 for float64 "
                         "tensors); beyond %d MB in all, a fixed seeded sample of every output" % (DUMP_BUDGET_BYTES // 10**6))
    args = ap.parse_args()
    args.batch_given = any(a == "--batch" or a.startswith("--batch=") for a in sys.argv[1:])
    return args


DTYPE_NAMES = {"f32": "fp32", "bf16": "bf16", "f16": "fp16"}


def cpu_model() -> str:
    """The host CPU's model string (BASELINE.md section 3 asks for it beside the CPU baseline): /proc/cpuinfo, else platform."""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith(("model name", "hardware", "cpu model")):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine() or "unknown"


def metric_label(config: str, wl, batched: int, dtype: str = "f32") -> str:
    if config == "cfg2" and not batched and dtype == "f32":
        return BASELINE_METRIC
    dn = DTYPE_NAMES[dtype]
    if config in ("resnet50", "linear16"):
        return f"elems/s + achieved HBM GB/s, {wl.name} {dn}, one batched launch per step"
    tail = f", {batched} tensors per launch" if batched else ""
    return f"elems/s + achieved HBM GB/s, {wl.name} {'x'.join(str(s) for s in wl.shape)} {dn}{tail}"


def graph_ok_for_calibration(args) -> bool:
    return not args.graph and args.streams == 1 and args.device == "cuda"


def per_launch_periods(step, launches: int):
    """Periods between consecutive launches, one HIP event between every two (on the current stream)."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    evs[0].record()
    for i in range(launches):
        step(i)
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(launches)]


def dump_outputs(out_dir: str, y):
    """--dump-outputs: the output(s) of the last timed step as out_dir/<name>.npy -- ``output`` for one tensor, ``output_000``,
    ``output_001``, ... for a step that returns several.  float64 tensors are written as float64, all others widened to
    float32 (exact).  When everything together would exceed DUMP_BUDGET_BYTES, each output is replaced by a sample of flat
    indices in proportion to its size, drawn once from a generator seeded with DUMP_SEED and the output's position and
    kept in index order: the same arguments give the same sample on every run and every build."""
    outs = list(y) if isinstance(y, (list, tuple)) else [y]
    names = ["output"] if len(outs) == 1 else [f"output_{i:03d}" for i in range(len(outs))]
    dtypes = [torch.float64 if t.dtype == torch.float64 else torch.float32 for t in outs]
    data = sum(t.numel() * (8 if dt == torch.float64 else 4) for t, dt in zip(outs, dtypes))
    data_budget = DUMP_BUDGET_BYTES - 128 * len(outs)     # 128 B: the .npy header of each file
    os.makedirs(out_dir, exist_ok=True)
    import numpy as np
    for i, (t, dt, name) in enumerate(zip(outs, dtypes, names)):
        a = t.detach().to(dt).cpu().numpy()
        if data > data_budget:
            keep = max(1, a.size * data_budget // data)   # this output's share of the budget, in its own elements
            idx = np.sort(np.random.default_rng([DUMP_SEED, i]).choice(a.size, size=keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def batched_plans(quantizer, x0, tensors: int, ring: int):
    """``ring`` pre-packed plans of ``tensors`` copies of x0 each (distinct input and output buffers everywhere):
    what pytorch/batching.py builds for a model with that many wrapped weights.  Returns (plans, outputs per plan)."""
    from mct_quantizers_amd.hip import native
    fast = native.fast()
    assert fast is not None, "the batched bench needs the compiled binding (lib/_mctq_torch.so)"
    plans, outs = [], []
    for _ in range(ring):
        xs = [x0.clone() for _ in range(tensors)]
        items, ys = [], []
        for x in xs:
            if hasattr(quantizer, "batch_item"):                      # affine weights quantizers
                xi, scales, zps, axis, qmin, qmax = quantizer.batch_item(x)
                y = torch.empty_like(x0)
                items.append((xi, y, scales, zps, axis, qmin, qmax))
            else:                                                     # LUT quantizers with a decision table: float32 out
                item = quantizer.batch_item_lut(x)
                assert item is not None, "this LUT configuration has no decision table: no batched launch"
                y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
                items.append(item[:2] + (y,) + item[3:])
            ys.append(y)
        plans.append(fast.BatchPlan(items))
        outs.append(ys)
    return plans, outs


def event_timed(step, steps: int):
    """(average period of launches 2..K in us, average over all K incl. the idle stream's start-up) by HIP events."""
    e0, ef, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    e0.record()
    for i in range(steps):
        step(i)
        if i == 0:
            ef.record()
    e1.record()
    torch.cuda.synchronize()
    return ef.elapsed_time(e1) * 1e3 / max(1, steps - 1), e0.elapsed_time(e1) * 1e3 / steps


def own_stdout():
    """The process's standard output carries ONE JSON line and nothing else: libraries that write to file descriptor 1 on their own
    (RCCL prints "Librccl path : ..." through C stdio, flushed at exit, i.e. BEHIND the line) are sent to stderr for the whole run --
    descriptor 1 is re-pointed at descriptor 2 and Python's sys.stdout at a private duplicate of the original."""
    try:
        sys.stdout.flush()
        real = os.dup(1)
        os.dup2(2, 1)
        sys.stdout = os.fdopen(real, "w", buffering=1)
    except OSError:
        pass


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher (child process; nothing here has touched the GPU)
        sys.exit(bench_dist.self_launch(os.path.abspath(__file__), args.gpus, sys.argv[1:]))
    own_stdout()                                     # (a rank, or the single process: never the launcher, whose children inherit)
    if args.e2e:
        if args.config != "resnet50" or args.gpus != 1:
            raise SystemExit("--e2e goes with --config resnet50 at --gpus 1")
        if args.dump_outputs:
            raise SystemExit("--dump-outputs: not with --e2e (a step there is a whole forward, not one quantizer output)")
        import bench_e2e
        sys.exit(bench_e2e.main(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    dry = args.device == "cpu"
    if dry:
        device = torch.device("cpu")
        args.config, args.batched, args.graph, args.streams, args.extras = "cfg1", 0, False, 1, False
    else:
        assert torch.cuda.is_available(), "bench.py needs a GPU"
        # fewer visible devices than LOCAL_RANK + 1: either the rehearsal of the N > 1 path on one GPU (tests set
        # MCTQ_BENCH_WRAP_DEVICES) or a launcher that gave every rank its own HIP_VISIBLE_DEVICES -- told apart below by the
        # physical identities the ranks exchange, never assumed
        implicit_wrap = local_rank >= torch.cuda.device_count()
        if os.environ.get("MCTQ_BENCH_WRAP_DEVICES") or implicit_wrap:
            local_rank %= torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    dist, control_plane = None, None
    if world > 1 or (args.gather and "RANK" in os.environ):
        dist, control_plane = bench_dist.init_process_group(
            "gloo" if dry else "nccl", device, force_gloo=bool(os.environ.get("MCTQ_BENCH_FORCE_GLOO")),
            allow_gloo=args.allow_gloo)
    ranks_seen = dist.get_world_size() if dist is not None else 1
    if ranks_seen != args.gpus:
        # a scaling line must not claim GPUs the process group did not see (one rank per GPU), whatever the control plane
        print(f"[bench] --gpus {args.gpus} but the process group has {ranks_seen} ranks", file=sys.stderr, flush=True)
        if dist is not None:
            dist.destroy_process_group()
        sys.exit(5)
    # which physical device every rank computes on (uuid | PCI address | name): a line that claims N GPUs shows N distinct ones
    wrapped = bool(os.environ.get("MCTQ_BENCH_WRAP_DEVICES")) and not dry
    rank_devs, devices_distinct = bench_dist.rank_devices(dist, control_plane, device)
    if not dry and implicit_wrap and devices_distinct is not True:
        wrapped = True                                # LOCAL_RANK beyond the visible devices and no proof of distinct ones
    if world > 1 and (wrapped or devices_distinct is False) and not args.allow_gloo:
        if rank == 0:
            print(f"[bench] --gpus {args.gpus}: the ranks do not sit on {args.gpus} distinct devices "
                  f"({'MCTQ_BENCH_WRAP_DEVICES is set; ' if wrapped else ''}rank_devices = {rank_devs}) and --allow-gloo was not "
                  f"given: exiting with status {bench_dist.EXIT_SHARED_DEVICE}", file=sys.stderr, flush=True)
        dist.destroy_process_group()
        sys.exit(bench_dist.EXIT_SHARED_DEVICE)

    import mct_quantizers_amd as mq
    from mct_quantizers_amd import workloads
    from mct_quantizers_amd.hip import native
    if not dry:
        native.load()
        for key, val in (("nt", args.nt), ("unroll", args.unroll), ("heavy_unroll", args.heavy_unroll), ("rowsteps", args.rowsteps),
                         ("cached_store_max_mb", args.cached_store_max_mb), ("paced", args.paced)):
            if val is not None:
                native.set_tuning(key, val)

    # ---- workload -------------------------------------------------------------------------
    model_mode = args.config in ("resnet50", "linear16")
    if model_mode:
        # every weight of the model, each with its own per-channel quantizer, ONE table launch per step
        assert not dry and native.fast() is not None, "the model workloads need a GPU and the compiled binding"
        weights = workloads.make_model_weights(args.config)
        quantizers = [mq.pytorch_quantizers.WeightsSymmetricInferableQuantizer(**kw) for _, kw in weights]
        total = sum(int(x.size) for x, _ in weights)
        import types
        wl = types.SimpleNamespace(name=f"{args.config}: all {len(weights)} weight tensors, WeightsSymmetric per-channel(axis0) 8b",
                                   shape=(len(weights), "tensors"), quantizer="WeightsSymmetricInferableQuantizer",
                                   numel=total, bytes_per_elem=8, kwargs=None)
        x_np, quantizer = None, quantizers[0]
        args.batched = len(weights)
    else:
        if args.config == "sym":
            x_np = workloads.make_input("sym", shape=tuple(int(d) for d in args.shape.lower().split("x")))
            wl = workloads.make_workload("sym", x_np, axis=None if args.per_tensor else args.axis)
        else:
            x_np = workloads.make_input(args.config, batch=args.batch)
            wl = workloads.make_workload(args.config, x_np)
        quantizer = getattr(mq.pytorch_quantizers, wl.quantizer)(**wl.kwargs)
    tdtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[args.dtype]
    is_lut = "LUT" in wl.quantizer or "Lut" in wl.quantizer
    if args.dtype != "f32":
        if dry or args.graph or args.streams > 1:
            raise SystemExit("--dtype bf16 / f16: eager or batched launches on the GPU only")
        # algorithmic bytes: 16-bit in; the affine kernels write the input's type, the LUT kernels float32 (the reference's
        # chain promotes once the float32 codebook enters, quantizer_utils.py:131-137)
        wl.bytes_per_elem = 2 + (4 if is_lut else 2)
    tensors = max(1, args.batched)
    per_launch = 1                               # steps served by one launch (activation stream: D batches per replay)
    stream_on = (args.config == "cfg3" and not args.batched and not dry and not args.graph and args.streams == 1
                 and (args.stream_depth > 0 or (args.stream_depth == 0 and args.batch <= 64)) and native.fast() is not None)
    if stream_on:
        cap = args.stream_depth if args.stream_depth > 0 else min(32, max(1, args.steps // 2))
        per_launch = max(d for d in range(1, cap + 1) if args.steps % d == 0)
        stream_on = per_launch > 1
    elems = wl.numel if model_mode else wl.numel * tensors
    alg_bytes = elems * wl.bytes_per_elem        # per STEP
    ring = args.ring or max(2, -(-(512 << 20) // (alg_bytes * per_launch)) + 1)
    x0 = None if model_mode else torch.from_numpy(x_np).to(device).to(tdtype)
    streams = None
    if stream_on:
        from mct_quantizers_amd.pytorch.graphs import capture_stream
        holder = mq.PytorchActivationQuantizationHolder(quantizer).to(device)
        act_streams = [capture_stream(holder, x0, depth=per_launch) for _ in range(ring)]
        xs, ys = None, None

        def step(i):                             # one LAUNCH: per_launch batches
            act_streams[i % ring].run()
    elif model_mode:
        plans, plan_outs = [], []
        for _ in range(ring):
            items, ys_ = [], []
            for (xw, _), q in zip(weights, quantizers):
                xi, scales, zps, axis, qmin, qmax = q.batch_item(torch.from_numpy(xw).to(device).to(tdtype))
                y = torch.empty_like(xi)
                items.append((xi, y, scales, zps, axis, qmin, qmax))
                ys_.append(y)
            plans.append(native.fast().BatchPlan(items))
            plan_outs.append(ys_)
        xs, ys = None, None

        def step(i):
            plans[i % ring]()
    elif args.batched:
        if not hasattr(quantizer, "batch_item") and not hasattr(quantizer, "batch_item_lut"):
            raise SystemExit(f"--batched: {wl.quantizer} has no batched launch")
        plans, plan_outs = batched_plans(quantizer, x0, tensors, ring)
        xs, ys = None, None

        def step(i):
            plans[i % ring]()
    else:
        xs = [x0] + [x0.clone() for _ in range(ring - 1)]
        ys = [None] * ring
        streams = [torch.cuda.Stream() for _ in range(args.streams)] if args.streams > 1 else None

        def step(i):
            if streams is None:
                ys[i % ring] = quantizer(xs[i % ring])
            else:
                with torch.cuda.stream(streams[i % len(streams)]):
                    ys[i % ring] = quantizer(xs[i % ring])
    n_launch = args.steps // per_launch
    launch_bytes = alg_bytes * per_launch

    def dev_sync():
        if not dry:
            torch.cuda.synchronize()

    # ---- fixed-duration pre-warm (declared; outside the timed region) --------------------------
    p0, n_pre = time.perf_counter(), 0
    while n_pre < ring or time.perf_counter() - p0 < (0.05 if dry else args.prewarm_seconds):
        step(n_pre)
        n_pre += 1
        if n_pre % 256 == 0:
            dev_sync()                        # keep the launch queue bounded
    dev_sync()
    prewarm_s = time.perf_counter() - p0

    for i in range(-(-args.warmup // per_launch)):
        step(i)
    dev_sync()
    kernel_variant = "aten cpu operator (dry run)" if dry else native.last_launch()
    build_id = None if dry else native.load().mctq_build_id().decode()
    sync_method = bench_dist.calibrate_sync(step, device) if graph_ok_for_calibration(args) else "torch.cuda.synchronize()"

    graph = None
    if args.graph:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(n_launch):
                step(i)
        torch.cuda.synchronize()

    # ---- timed region ---------------------------------------------------------------------
    steady = graph is None and streams is None and n_launch >= 2 and not dry
    if not dry:
        # two markers only inside the judged region (each costs ~5 us of stream time, tools/region_overhead_probe.py): one
        # behind the FIRST launch, one behind the last; a third in front of the first launch only when there is no steady part
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_first = torch.cuda.Event(enable_timing=True)

    def run_all(_):
        if dry:
            for i in range(n_launch):
                step(i)
            return None
        if not steady:
            ev0.record()
        if graph is not None:
            graph.replay()
        else:
            for i in range(n_launch):
                step(i)
                if i == 0 and steady:
                    ev_first.record()
        if streams is not None:
            for st in streams:
                torch.cuda.current_stream().wait_stream(st)
        ev1.record()
        return ev1                                 # the region's closing synchronize polls this event first

    wall = bench_dist.timed_region(run_all, 1, device, dist)

    # ---- the last timed step's output, kept for the dump and the parity check before anything overwrites the ring ----------
    last_slot = (n_launch - 1) % ring
    if stream_on:
        y_last = act_streams[last_slot].outputs       # persistent outputs of the last timed replay
    elif args.batched:
        y_last = plan_outs[last_slot]       # persistent outputs; later passes rewrite them with the same values
    else:
        y_last = ys[last_slot]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, y_last)

    # events on the stream the kernels were launched on; with a steady part the whole-region figure is the host wall clock
    dev_ms = wall * 1e3 if (dry or steady) else ev0.elapsed_time(ev1)
    wall, dev_ms = bench_dist.max_over_ranks([wall, dev_ms], dist, control_plane, device)

    value = elems * args.steps * world / wall
    launch_us_all = dev_ms * 1e3 / n_launch
    if steady:
        # launches 2..K, from the end of launch 1 to the end of launch K: the period without the idle stream's start-up (the
        # host's first call + launch latency, ~5-8 us once per region -- 1.5 % of a 20-step region, 0.03 % of a 1000-step one)
        own_steady_us = ev_first.elapsed_time(ev1) * 1e3 / (n_launch - 1)
        launch_us = bench_dist.max_over_ranks([own_steady_us], dist, control_plane, device)[0]
    else:
        own_steady_us = launch_us = launch_us_all
    achieved = launch_bytes / (launch_us * 1e-6) / 1e9
    wall_us = wall * 1e6 / args.steps
    achieved_wall = alg_bytes / (wall_us * 1e-6) / 1e9

    result = {
        "metric": metric_label(args.config, wl, args.batched, args.dtype),
        "value": value,
        "unit": "elems/s",
        "n_gpus": world,
        "ranks_seen": ranks_seen,
        "rank_devices": rank_devs,                            # uuid | PCI domain:bus:device | name of every rank's device
        "devices_distinct": False if wrapped else devices_distinct,   # null: the runtime reports neither a uuid nor a PCI address
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": wall * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,                                  # the tensors' STORAGE type; arithmetic is float32 (config.arithmetic)
        "data": "synthetic (portable splitmix64 generator, mct_quantizers_amd/workloads.py)",
        "config": {"workload": wl.name + (f", {tensors} tensors in one batched launch" if args.batched and not model_mode else
                                          ", one batched launch per step" if model_mode else ""),
                   "shape": list(wl.shape), "quantizer": wl.quantizer, "tensors_per_step": tensors,
                   "storage": DTYPE_NAMES[args.dtype], "arithmetic": "fp32",
                   "algorithmic_bytes_per_elem": wl.bytes_per_elem,
                   "per_gpu_elems": elems, "buffer_ring": ring, "cache_protocol": "cold" if ring > 1 else "warm",
                   "launch": ("hipGraph" if graph is not None else
                              f"fused group of {per_launch} independent batches per launch (pytorch/graphs.py CapturedStream, mode "
                              f"{act_streams[0].mode}): a THROUGHPUT mode for a producer that owns {per_launch} batches at once -- a "
                              f"batch's result is ready when its group's launch completes; NOT what a holder does inside one "
                              f"forward (reference activation_quantization_holder.py:43-53): that is eager_us_per_batch / eager_frac"
                              if stream_on else "eager (one holder / quantizer call per batch)"),
                   "steps_per_launch": per_launch, "streams": args.streams,
                   "binding": "none (dry run)" if dry else ("compiled" if native.fast() is not None else "ctypes"),
                   "library_build_id": build_id,
                   "prewarm_s": round(prewarm_s, 3), "prewarm_steps": n_pre,
                   "parallelism": f"replicated x{world} (weak, no collective)",
                   "control_plane": control_plane, "ranks_seen": ranks_seen,
                   "region_end": sync_method},
        "achieved_gbs": achieved_wall,                       # same clock as value / ms_per_step (host wall)
        "achieved_gbs_steady": achieved,                     # = roofline.achieved (event period of launches 2..K)
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "frac_of_measured_copy": achieved / HBM_COPY_GBS,
                     "frac_wall": achieved_wall / HBM_PEAK_GBS,
                     "frac_events_whole_region": launch_bytes / (launch_us_all * 1e-6) / 1e9 / HBM_PEAK_GBS,
                     "traffic": None, "kernel": kernel_variant, "kernel_us": launch_us,
                     "kernel_us_is": ("average launch PERIOD inside the timed region, launches 2..K (event behind launch 1 -> event "
                                      "behind launch K): kernel duration + the ~1.4 us bubble between back-to-back launches; "
                                      "frac_wall = the same bytes over ms_per_step (host wall clock incl. the first launch's latency "
                                      "and the closing synchronize)"
                                      if steady else "average launch PERIOD over the timed region (one event pair around K launches)"),
                     "kernel_us_incl_first_launch_latency": launch_us_all,
                     "algorithmic_bytes_per_launch": launch_bytes},
    }
    if dry:
        result["dry_run"] = "CPU dry run of the entry path (launcher, gloo process group, barriers, JSON): NOT a measurement"
        result["roofline"] = None
    if dist is not None:
        # every rank's own steady period (the headline uses the slowest)
        t = torch.tensor([own_steady_us], dtype=torch.float64, device=device if control_plane == "nccl" else "cpu")
        got = [torch.zeros_like(t) for _ in range(ranks_seen)]
        dist.all_gather(got, t)
        result["per_rank_kernel_us"] = [float(v[0]) for v in got]

    # ---- config 3 with --full: the EAGER per-call figure beside a fused-group line (outside the timed region) -------------
    if args.full and args.config == "cfg3" and not dry and not args.batched and not args.no_eager_extra:
        try:
            holder_e = mq.PytorchActivationQuantizationHolder(quantizer).to(device)
            ring_e = max(2, -(-(512 << 20) // alg_bytes) + 1)
            xs_e = [x0] + [x0.clone() for _ in range(min(ring_e, 64) - 1)]
            for i in range(20):
                holder_e(xs_e[i % len(xs_e)])
            n_e = max(200, min(2000, args.steps))
            torch.cuda.synchronize()
            ee0, ee1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            ee0.record()
            for i in range(n_e):
                holder_e(xs_e[i % len(xs_e)])
            h1 = time.perf_counter()
            ee1.record()
            torch.cuda.synchronize()
            e_us = ee0.elapsed_time(ee1) * 1e3 / n_e
            result["eager_us_per_batch"] = e_us
            result["eager_host_us_per_call"] = (h1 - h0) * 1e6 / n_e
            result["eager_frac"] = alg_bytes / e_us / 1e3 / HBM_PEAK_GBS
            result["eager_is"] = (f"{n_e} back-to-back holder(x) calls, one launch per batch, HIP events on the launch stream; "
                                  f"host-bound when eager_host_us_per_call ~= eager_us_per_batch")
            del xs_e
        except Exception as e:  # noqa: BLE001
            result["eager_us_per_batch"] = {"error": repr(e)[:200]}

    # ---- --full: per-launch evidence pass (outside the timed region) ---------------------------------------------
    if args.full and args.evidence_launches > 0 and graph is None and streams is None and not dry:
        try:
            periods = per_launch_periods(step, max(50, args.evidence_launches))[1:]     # first period: event after idle
            periods.sort()
            n = len(periods)
            med = statistics.median(periods)
            result["roofline"]["per_launch"] = {
                "launches": n, "median_us": med, "mean_us": sum(periods) / n,
                "p10_us": periods[n // 10], "p90_us": periods[(n * 9) // 10],
                "achieved_gbs_at_median": launch_bytes / med / 1e3, "frac_at_median": launch_bytes / med / 1e3 / HBM_PEAK_GBS,
                "note": "one HIP event between every two launches (the marker itself adds to the period); "
                        "outside the timed region"}
        except Exception as e:  # noqa: BLE001
            result["roofline"]["per_launch"] = {"error": repr(e)[:200]}

    # ---- measured HBM traffic per launch (rocprofv3 PMC passes committed under profiles/) ----------------
    if not dry:
        key = args.config if args.config != "cfg3" else f"cfg3_n{args.batch}"
        if args.config == "sym":
            key = f"sym_{args.shape.lower()}_" + ("pertensor" if args.per_tensor else f"axis{args.axis % len(wl.shape)}")
        if args.batched and not model_mode:
            key = f"{key}_batched{tensors}"
        if stream_on:
            key = f"{key}_stream{per_launch}"
        if args.dtype != "f32":
            key = f"{key}_{args.dtype}"
        result["roofline"].update(bench_dist.traffic_fields(os.path.join(REPO, "profiles", "pmc_traffic.json"), key,
                                                            kernel_variant, build_id))

    # ---- --full, every rank: its own last timed output against the REFERENCE's digest of this configuration ------------
    # (tests/golden/full_sha.json: SHA-256 of the reference's float32 output on the same portable input).  The verdict
    # of every rank travels to rank 0 (ranks_parity_ok); one False fails the job.  None = no digest for this workload
    # (16-bit storage, model workloads).
    if args.full:
        own_parity = None
        want_sha = None if (model_mode or args.dtype != "f32") else bench_dist.golden_output_digest(args.config, wl.shape, args.batch)
        if want_sha is not None:
            if isinstance(y_last, (list, tuple)):
                own_parity = all(bench_dist.sha256_of(y) == want_sha for y in y_last[:2]) and \
                    all(bool(torch.equal(y, y_last[0])) for y in y_last[2:])
            else:
                own_parity = bench_dist.sha256_of(y_last) == want_sha
        result["ranks_parity_ok"] = bench_dist.gather_flags(dist, own_parity, control_plane, device)
        result["ranks_parity_is"] = ("per rank: SHA-256 of the output of its LAST timed step == the reference's digest "
                                     "(tests/golden/full_sha.json); null = no digest recorded for this workload / storage type")
        if any(v is False for v in result["ranks_parity_ok"]):
            result["parity_error"] = f"ranks_parity_ok = {result['ranks_parity_ok']}: a rank's output differs from the reference's digest"

    # Extra (outside the judged region): the same K independent steps issued round-robin on two HIP streams,
    # which overlaps one kernel's tail with the next one's ramp.  Whole-job rate only; per-kernel durations
    # overlap, so this is not a roofline figure.
    if args.extras and args.streams == 1 and graph is None and not args.batched and not stream_on:
        try:
            s2 = [torch.cuda.Stream(), torch.cuda.Stream()]
            for st in s2:
                st.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            o0 = time.perf_counter()
            for i in range(args.steps):
                with torch.cuda.stream(s2[i & 1]):
                    ys[i % ring] = quantizer(xs[i % ring])
            torch.cuda.synchronize()
            o = time.perf_counter() - o0
            result["two_stream_overlap"] = {"value": elems * args.steps * world / o, "unit": "elems/s",
                                            "ms_per_step": o * 1e3 / args.steps,
                                            "achieved_gbs_whole_job": alg_bytes * args.steps / o / 1e9}
        except Exception as e:  # noqa: BLE001
            result["two_stream_overlap"] = {"error": repr(e)[:200]}

    # Extras at N = 1 (outside the judged region): warm-cache rate (one buffer pair, working set inside the
    # Infinity Cache) and what the REFERENCE would execute on this GPU for the same call -- ATen's own HIP
    # fake-quant operator (only defined for the affine configurations).
    if args.extras and world == 1 and graph is None and args.streams == 1 and not args.batched and not stream_on:
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            wsteps = min(args.steps, 300)
            for _ in range(20):
                yw = quantizer(xs[0])
            e0.record()
            for _ in range(wsteps):
                yw = quantizer(xs[0])
            e1.record()
            torch.cuda.synchronize()
            wus = e0.elapsed_time(e1) * 1e3 / wsteps
            result["warm_cache"] = {"kernel_us": wus, "achieved_gbs": alg_bytes / wus / 1e3,
                                    "note": "same tensor every launch (input + output fit the 256 MiB Infinity Cache "
                                            "for config 2); not an HBM figure"}
            aten = None
            if wl.quantizer in ("WeightsSymmetricInferableQuantizer", "WeightsPOTInferableQuantizer",
                                "WeightsUniformInferableQuantizer") and wl.kwargs.get("per_channel"):
                aten = lambda t: torch.fake_quantize_per_channel_affine(    # noqa: E731
                    t, quantizer.scales.flatten(), quantizer.zero_points.flatten(), wl.kwargs["channel_axis"],
                    quantizer.min_quantized_domain, quantizer.max_quantized_domain)
            elif wl.quantizer == "ActivationUniformInferableQuantizer":
                aten = lambda t: torch.fake_quantize_per_tensor_affine(     # noqa: E731
                    t, quantizer.scale, quantizer.zero_point, quantizer.min_quantized_domain,
                    quantizer.max_quantized_domain)
            if aten is not None:
                asteps = 60
                for i in range(5):
                    ya = aten(xs[i % ring])
                e0.record()
                for i in range(asteps):
                    ya = aten(xs[i % ring])
                e1.record()
                torch.cuda.synchronize()
                aus = e0.elapsed_time(e1) * 1e3 / asteps
                result["aten_hip_reference_path"] = {
                    "kernel_us": aus, "elems_per_s": elems / (aus * 1e-6), "speedup_of_this_package": aus / launch_us,
                    "bit_equal": bool(torch.equal(ya, quantizer(xs[(asteps - 1) % ring]))),
                    "note": "torch.fake_quantize_*_affine on the same device-resident tensors: the operator the "
                            "reference's __call__ dispatches to on a ROCm device"}
        except Exception as e:  # noqa: BLE001
            result["extras_error"] = repr(e)[:200]

    # ---- --full at N = 1: the headline tensor 16 times in ONE batched launch (outside the judged region) -------
    if (args.full and not dry and world == 1 and args.config == "cfg2" and args.dtype == "f32" and not args.batched and not args.no_batched_extra
            and graph is None and streams is None and hasattr(quantizer, "batch_item") and native.fast() is not None):
        try:
            T = 16
            bplans, bouts = batched_plans(quantizer, x0, T, 2)
            b0, i = time.perf_counter(), 0
            while i < 6 or time.perf_counter() - b0 < 0.3:            # the same kind of declared pre-warm, 0.3 s
                bplans[i % 2]()
                i += 1
                if i % 64 == 0:
                    torch.cuda.synchronize()
            bsteps = max(20, min(args.steps, 100))
            b_us, b_us_all = event_timed(lambda i: bplans[i % 2](), bsteps)
            bb = alg_bytes * T
            same = all(torch.equal(y, bouts[(bsteps - 1) % 2][0]) for y in bouts[(bsteps - 1) % 2][1:])
            result["batched_16x4096"] = {
                "what": "the headline tensor 16 times (distinct buffers, 2 GiB in + 2 GiB out per launch) in ONE batched "
                        "launch: the launch a wrapped model issues per forward (pytorch/batching.py, "
                        "mctq_fq_batch_run); outside the judged region, same event protocol",
                "kernel": native.last_launch(), "launches": bsteps, "prewarm_s": 0.3, "kernel_us": b_us, "kernel_us_per_tensor": b_us / T,
                "kernel_us_incl_first_launch_latency": b_us_all, "algorithmic_bytes_per_launch": bb,
                "achieved_gbs": bb / b_us / 1e3, "frac": bb / b_us / 1e3 / HBM_PEAK_GBS,
                "frac_of_measured_copy": bb / b_us / 1e3 / HBM_COPY_GBS,
                "all_16_outputs_equal": bool(same),
                "equal_to_single_launch_output": bool(torch.equal(bouts[(bsteps - 1) % 2][0], y_last))}
            del bplans, bouts
            torch.cuda.empty_cache()
        except Exception as e:  # noqa: BLE001
            result["batched_16x4096"] = {"error": repr(e)[:300]}

    # ---- config 5 sharded by dim 0 + ONE all-gather (three series at every N) -----------------
    # N > 1 (or --gather under torchrun): here, on the job's process group.  N = 1 without a launcher: after the CPU baseline,
    # on a group of one rank formed in-process (RCCL's all_gather_into_tensor on HIP memory; no link is crossed).
    sharded_failed = None

    def run_sharded_leg(group, control, watchdog_s, watchdog_status):
        nonlocal sharded_failed
        with bench_dist.Watchdog(watchdog_s, rank, lambda: json.dumps(result), status=watchdog_status):
            try:
                kw = dict(rows=64, cols=128, reps=3, gather_reps=2) if dry else {}
                leg = bench_dist.sharded_cfg5_leg(group, rank, world, device, control=control, **kw)
                result["sharded_cfg5"] = leg
                result["sharded_cfg5_compute_elems_per_s"] = leg["compute_elems_per_s"]
                result["sharded_cfg5_compute_plus_allgather_elems_per_s"] = leg["compute_plus_allgather_elems_per_s"]
                result["sharded_cfg5_allgather_gbs_per_link"] = leg["allgather_gbs_per_link"]     # null at N = 1: no link is crossed
                bad = [k for k in ("gathered_rows_match_local",) if leg.get(k) is not True]
                if any(v is False for v in leg["ranks_shard_digest_ok"]) or leg.get("gathered_equals_reference_digest") is False:
                    bad.append("digest")
                if bad:
                    result["parity_error"] = f"sharded config 5: {bad} -- ranks_shard_digest_ok = {leg['ranks_shard_digest_ok']}"
            except Exception as e:  # noqa: BLE001
                result["sharded_cfg5"] = {"error": repr(e)[:300]}
                sharded_failed = repr(e)[:300]

    if dist is not None and (args.gather or (world > 1 and args.full)):
        run_sharded_leg(dist, control_plane, 300.0 if control_plane == "gloo" and not dry else 120.0, 4)

    # --full, CPU baseline: on rank 0, at every N (the other ranks are done; they leave through destroy_process_group below)
    if args.full and rank == 0 and not args.no_cpu and not dry and model_mode:
        # CPU baseline of the model workloads: ATen's CPU operator on every weight in turn, oracle-derived parameters
        from oracle import torch_cpu
        fs = [torch_cpu.prepare("WeightsSymmetricInferableQuantizer", kw) for _, kw in weights]
        xcs = [torch.from_numpy(xw).to(tdtype) for xw, _ in weights]
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        wants = [f(x) for f, x in zip(fs, xcs)]
        same = all(bool(torch.equal(y.cpu(), w)) for y, w in zip(y_last, wants))
        n, c0 = 0, time.perf_counter()
        while True:
            for f, x in zip(fs, xcs):
                f(x)
            n += 1
            el = time.perf_counter() - c0
            if el >= args.cpu_seconds or n >= 2000:
                break
        result["cpu_baseline"] = {"value": elems * n / el, "unit": "elems/s", "cores": torch.get_num_threads(), "kind": "port",
                                  "cpu_model": cpu_model(), "host_threads": os.cpu_count(),
                                  "sample": f"{n} passes over all {len(weights)} weight tensors with the ATen CPU operator the "
                                            f"reference calls (oracle/torch_cpu.py parameters), {el:.1f} s",
                                  "ms_per_call": el * 1e3 / n, "gpu_output_bit_equal": same,
                                  "gpu_output_checked": f"all {len(weights)} outputs of the last timed step"}
        if not same:
            result["parity_error"] = "GPU output differs from the CPU oracle"
    elif args.full and rank == 0 and not args.no_cpu and not dry:
        from oracle import torch_cpu
        f = torch_cpu.prepare(wl.quantizer, wl.kwargs)
        x_cpu = torch.from_numpy(x_np).to(tdtype)          # the same rounding to the storage type as on the device
        y_cpu = f(x_cpu)                                   # warm-up + parity reference
        if args.batched or stream_on:
            same = all(bool(torch.equal(y.cpu(), y_cpu)) for y in y_last[:2]) and \
                all(bool(torch.equal(y, y_last[0])) for y in y_last[2:])
        else:
            same = bool(torch.equal(y_last.cpu(), y_cpu))  # the output of the LAST timed step
        # ATen's CPU kernel stops scaling (and degrades) well before all hardware threads of a big host:
        # probe a few thread counts briefly and report the best one.
        ncpu = os.cpu_count() or 1
        probe = {}
        for th in sorted({1, 8, 16, 32, 64, ncpu} & set(range(1, ncpu + 1))):
            torch.set_num_threads(th)
            f(x_cpu)
            c0, n = time.perf_counter(), 0
            while time.perf_counter() - c0 < 0.7:
                f(x_cpu)
                n += 1
            probe[th] = (time.perf_counter() - c0) / n
        best = min(probe, key=probe.get)
        torch.set_num_threads(best)
        n, c0 = 0, time.perf_counter()
        while True:
            f(x_cpu)
            n += 1
            el = time.perf_counter() - c0
            if el >= args.cpu_seconds or n >= 2000:
                break
        result["cpu_baseline"] = {"value": wl.numel * n / el, "unit": "elems/s", "cores": best, "kind": "port",
                                  "cpu_model": cpu_model(), "host_threads": ncpu,
                                  "sample": f"{n} calls on one {wl.name} tensor of the ATen CPU operator the "
                                            f"reference calls, parameters from the oracle restatement "
                                            f"(oracle/torch_cpu.py), {el:.1f} s at the best of "
                                            f"{sorted(probe)} threads on a {ncpu}-thread host",
                                  "ms_per_call": el * 1e3 / n,
                                  "ms_per_call_by_threads": {str(k): round(v * 1e3, 3) for k, v in probe.items()},
                                  "gpu_output_bit_equal": same,
                                  "gpu_output_checked": "output of the last timed step"}
        if not same:
            result["parity_error"] = "GPU output differs from the CPU oracle"

    if args.full and dist is None and world == 1 and not args.no_sharded_extra and not model_mode and "sharded_cfg5" not in result:
        # --full at N = 1, no launcher: the same leg on a process group of one rank.  A failure here (no RCCL, a stuck init) costs the
        # leg, not the line: the watchdog prints the line as it stands and leaves with status 0.
        try:
            group, own_control = bench_dist.init_single_rank_group(device)
        except Exception as e:  # noqa: BLE001
            result["sharded_cfg5"] = {"error": "process group of one rank: " + repr(e)[:260]}
        else:
            run_sharded_leg(group, own_control, 240.0, 0)
            if isinstance(result.get("sharded_cfg5"), dict) and "error" not in result["sharded_cfg5"]:
                result["sharded_cfg5"]["process_group"] = "one rank, formed in-process (tcp://127.0.0.1), backend " + own_control
            try:
                group.destroy_process_group()
            except Exception:  # noqa: BLE001
                pass

    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0 and result.get("parity_error"):
        print(f"[bench] {result['parity_error']}", file=sys.stderr, flush=True)
        sys.exit(3)
    if world > 1 and not dry and sharded_failed is not None and not args.allow_gloo:
        # a scaling line whose config-5 + all-gather leg did not execute must not look like success
        print(f"[bench] the sharded config-5 leg failed ({sharded_failed}) and --allow-gloo was not given: exiting with status "
              f"{bench_dist.EXIT_NO_SHARDED_LEG}", file=sys.stderr, flush=True)
        sys.exit(bench_dist.EXIT_NO_SHARDED_LEG)


if __name__ == "__main__":
    main()
