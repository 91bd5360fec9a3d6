"""Headline benchmark: encoded nodes/s on synthetic 60,000-node / 300,000-edge
shards (BASELINE.json configs[2]), fp16 model, inputs resident in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set-up, warm-up, the K timed steps, the
outputs if ``--dump-outputs`` is given, and the result line.  Everything else it can measure
(the repeated leg, ``roofline``, ``kernels_ms``, ``distance``, ``cpu_baseline``) runs only with
``--full``; those keys are null in a plain run.

``--dump-outputs DIR`` (rank 0): after the timed steps, the embeddings of the shard the last
timed step encoded, as the caller of the hot path receives them (60,000 x 128, fp16 widened to
float32, 30.7 MB), are written to ``DIR/embeddings.npy``.  The shards are seeded, so the same
arguments give the same inputs on every run.

``--gpus N`` with N > 1 (or ``--spawn``) outside torch.distributed.run: this process starts
the N ranks itself (``python -m torch.distributed.run --nnodes=1 --nproc-per-node N
--master-addr 127.0.0.1 ...``) before anything touches HIP, relays rank 0's line and exits
with the ranks' status.  Under torch.distributed.run it is one rank.

One step = one pass of the hot path over one shard: COO→CSR build, per-encode setup (tile
plans + input Linear, 1 launch), 4 fused GINE layer launches the last of which also runs
head + float64 L2 normalise, embeddings left on the device.  The steps are issued
``--batch`` shards at a time (default 4) through ``gfy_encode_coo_batch`` — the shards of a
batch share every launch (one graph of 240,000 nodes in global numbering; the layers run as
the windowed rounds kernel k_gine_layer_w), as ``encode_graphs`` issues the micro-batches of
one shard — with ``--streams`` batches in flight (default 2).  ``--batch 1`` is one shard per
launch sequence (the one-round kernel k_gine_layer_f16).  K and W count SHARDS either way.
Multi-GPU: shards are independent, every rank encodes its own shards, there is no data-path
collective ("weak" scaling); the only communication is the barrier and the MAX-reduction of
the elapsed time.

Before the W warm-up steps the script builds every pre-bound step the K steps use (each run
once) and runs batches untimed for 0.25 s (GFY_BENCH_SETTLE_S): set-up, so that the part has
reached its working clocks whatever K and W are.  Then W warm-up steps, barrier +
synchronize, EXACTLY K timed steps, synchronize, MAX over ranks.  With ``--full``, when those K
steps took less than 10 ms (K=20 is 1.5 ms) the same leg is repeated until 10 ms are covered and
reported beside the contract values (``timed_ms``, ``repeated``); ``value`` stays the K-step one.

Rank 0 prints ONE JSON line.  Besides the contract keys it carries, with ``--full``
  roofline      dominant kernel (k_gine_layer_w, or k_gine_layer_f16 with --batch 1):
                algorithmic bytes per launch ((512·N + 9·E) x the shards of one launch + layer
                weights) ÷ its mean duration IN THE
                TIMED CONFIGURATION (all streams in flight), taken on the device clock by
                the launches themselves (first workgroup start -> last workgroup end,
                gfy_encoder_set_timing(3): an event pair on one stream would include the
                other streams' kernels); `isolated` repeats it one batch at a time with
                HIP events around the launches; `traffic`
                = HBM bytes per launch from the committed PMC passes, only while they
                were taken from the kernel source as it is now (else null)
  distance      BASELINE configs[3]: all-pairs nearest over 1M x 128 fp16 rows, fraction
                of the dense fp16 MFMA peak (N=1 only)
  cpu_baseline  oracle/gine_torch.py (the reference's aten op sequence) timed on this
                box's host cores on the same workload, best of several thread counts —
                N=1 only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

# Every stream in flight needs its own hardware queue: ROCm maps HIP streams onto
# GPU_MAX_HW_QUEUES (default 4) queues, and torch's default stream takes one, so the fourth
# shard stream would share a queue — and serialise — with another one (measured: 546 vs
# 632 M nodes/s).  Must be set before the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NODES, EDGES = 60_000, 300_000
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s HBM3E (spec)
MFMA_PEAK_TFLOPS = 2500.0        # dense fp16
POOL = 4                         # distinct shards per rank, cycled
MIN_TIMED_S = 0.010              # the K timed steps are repeated until this much was timed

# algorithmic bytes, SURVEY §8(d):  whole shard  2,332·N + 36·E + 612,872
PIPELINE_BYTES = 2332 * NODES + 36 * EDGES + 612_872
# one GINE layer launch: h read + h write (fp16) + COO once + that layer's fp16 weights
LAYER_WEIGHT_BYTES = 2 * (256 * 128 + 128 * 256 + 10 * 128 + 256 + 4 * 256 + 128 + 2 * 128)
LAYER_BYTES = 512 * NODES + 9 * EDGES + LAYER_WEIGHT_BYTES
LAYER_FLOPS = NODES * 2 * (128 * 256 + 256 * 128)


def parse() -> argparse.Namespace:
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=1000)
    parser.add_argument("--warmup", type=int, default=100)
    parser.add_argument("--streams", type=int, default=2,
                        help="batches in flight per GPU (HIP streams)")
    parser.add_argument("--batch", type=int, default=4,
                        help="shards per launch sequence (gfy_encode_coo_batch, 1..16)")
    parser.add_argument("--full", action="store_true",
                        help="also run the repeated leg, the per-kernel roofline, the distance "
                             "leg and the CPU baseline (off: set-up, warm-up, timed steps only)")
    parser.add_argument("--dump-outputs", metavar="DIR", default=None,
                        help="write the last timed step's embeddings to DIR/embeddings.npy "
                             "(float32, rank 0)")
    parser.add_argument("--distance-rows", type=int, default=1_000_000,
                        help="with --full: rows of the all-pairs nearest leg (0 = skip it)")
    parser.add_argument("--no-cpu-baseline", action="store_true",
                        help="with --full: skip the CPU baseline")
    parser.add_argument("--cpu-seconds", type=float, default=12.0)
    parser.add_argument("--workload", choices=("encode", "cross-shard"), default="encode",
                        help="cross-shard = BASELINE configs[4] in miniature: shard-parallel "
                             "encode + chunked RCCL all-gather + cross-shard nearest")
    parser.add_argument("--shards", type=int, default=16,
                        help="cross-shard workload: synthetic 60k-node shards over all ranks")
    parser.add_argument("--chunk-rows", type=int, default=1 << 20,
                        help="cross-shard workload: rows per rank per all-gather chunk")
    parser.add_argument("--spawn", action="store_true",
                        help="go through the rank launcher even for --gpus 1 (world size 1 "
                             "under torch.distributed.run, RCCL group created)")
    return parser.parse_args()


def visible_gpus() -> int:
    """GPUs this process may use, WITHOUT starting the HIP runtime (torch.cuda.device_count()
    opens /dev/kfd unless amdsmi is importable): the KFD topology lists every node, GPUs are
    the ones with SIMDs; HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES
    narrow the list as the runtime would."""
    nodes = Path("/sys/class/kfd/kfd/topology/nodes")
    count = 0
    try:
        for node in sorted(nodes.iterdir(), key=lambda p: int(p.name)):
            text = (node / "properties").read_text()
            fields = dict(line.split() for line in text.splitlines() if len(line.split()) == 2)
            if int(fields.get("simd_count", "0")) > 0:
                count += 1
    except (OSError, ValueError):
        return torch.cuda.device_count()            # no KFD topology: ask the runtime
    for name in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        value = os.environ.get(name)
        if value is not None:
            listed = [v for v in value.split(",") if v.strip() != ""]
            count = min(count, len(listed))
    return count


def launch_ranks(args: argparse.Namespace) -> "NoReturn":
    """``python bench.py --gpus N`` outside torchrun: start N fresh rank processes and relay
    rank 0's line.  The reference's model is one process per shard under an external
    scheduler (docs/GRAPH_PIPELINE.md:22-24); here the scheduler is torch.distributed.run,
    one rank per GPU.  This process never touches HIP (the GPUs are counted from the KFD
    topology in sysfs) and never replaces itself: the ranks are children and their exit status
    is ours.  ``--standalone`` lets the launcher pick its own rendezvous port (no probed port
    that could be taken between the probe and the bind)."""
    import subprocess

    visible = visible_gpus()
    if visible < args.gpus:
        print(f"bench.py: --gpus {args.gpus} but only {visible} HIP device(s) visible; "
              "refusing to report a smaller world as if it were the requested one",
              file=sys.stderr)
        raise SystemExit(3)
    passed = [a for a in sys.argv[1:] if a != "--spawn"]
    command = [sys.executable, "-m", "torch.distributed.run", "--standalone",
               "--local-addr", "127.0.0.1", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               str(Path(__file__).resolve()), *passed]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes
    done = subprocess.run(command, env=env, stdout=subprocess.PIPE, text=True)
    lines = [line for line in done.stdout.splitlines() if line.startswith("{")]
    for line in (lines[-1:] if done.returncode == 0 else done.stdout.splitlines()):
        print(line, flush=True)
    if done.returncode == 0 and not lines:
        print("bench.py: the ranks exited 0 without a result line", file=sys.stderr)
        raise SystemExit(4)
    raise SystemExit(done.returncode)


KERNEL_SOURCES = ("ginfinity_amd/csrc/gine_layer.inc", "ginfinity_amd/csrc/gine_layer_q.inc",
                  "ginfinity_amd/csrc/gine_layer_w.inc", "ginfinity_amd/csrc/gine_block_pipe.inc",
                  "ginfinity_amd/csrc/gine_layer_x.inc", "ginfinity_amd/csrc/csr_records.inc",
                  "ginfinity_amd/csrc/gine_f16.hip", "ginfinity_amd/csrc/gfy_common.h")


def kernel_source_sha16() -> str:
    """Fingerprint of the sources the dominant kernel is compiled from."""
    import hashlib
    digest = hashlib.sha256()
    for name in KERNEL_SOURCES:
        digest.update((ROOT / name).read_bytes())
    return digest.hexdigest()[:16]


def measured_traffic(kernel: str, nodes_per_launch: int):
    """HBM bytes per launch of ``kernel`` from the committed PMC passes (rocprofv3
    FETCH_SIZE / WRITE_SIZE, gfx950 half-count correction applied; tools/profile_round.sh +
    tools/pmc_summary.py), scaled from the node count the passes ran on to this run's.  Counter
    passes cannot run inside this script, so the figure is only reported while the summary was
    taken from the kernel source as it is now."""
    newest = sorted((ROOT / "profiles").glob("r*_traffic_pmc.json"))
    for path in reversed(newest):
        try:
            summary = json.loads(path.read_text())
            if summary.get("kernel_source_sha16") != kernel_source_sha16():
                continue
            measured = summary["kernels"][kernel]["hbm_bytes_per_launch"]
            return (measured * nodes_per_launch / summary.get("nodes_per_launch", NODES),
                    f"profiles/{path.name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the "
                    "same kernel source (hash-checked), taken in a separate run — not measured "
                    "in this one")
        except (OSError, KeyError, ValueError):
            continue
    return None, ("none: no committed PMC pass matches the kernel source as it is now "
                  "(tools/profile_round.sh + tools/pmc_summary.py)")


def measured_counters(kernel: str):
    """Matrix-pipe busy share and vector / matrix co-execution share of a launch of ``kernel``
    from the committed SQ counter passes (SQ_VALU_MFMA_BUSY_CYCLES, SQ_VALU_MFMA_COEXEC_CYCLES
    and SQ_WAVE_CYCLES over tools/gfy_bench; tools/profile_round.sh + tools/pmc_summary.py),
    hash-guarded like ``measured_traffic``: ``(mfma_busy_frac, coexec_frac, source)``."""
    newest = sorted((ROOT / "profiles").glob("r*_layer_sq_pmc.json"))
    for path in reversed(newest):
        try:
            summary = json.loads(path.read_text())
            if summary.get("kernel_source_sha16") != kernel_source_sha16():
                continue
            counters = summary["kernels"][kernel]
            return (counters["mfma_busy_frac"], counters["coexec_frac"],
                    f"profiles/{path.name}: rocprofv3 --pmc passes of the same kernel source "
                    "(hash-checked), taken in a separate run; shares of the launch's cycles per "
                    "SIMD (wave lifetime from SQ_WAVE_CYCLES)")
        except (OSError, KeyError, ValueError, TypeError):
            continue
    return None, None, ("none: no committed SQ counter pass matches the kernel source as it is "
                        "now (tools/profile_round.sh + tools/pmc_summary.py)")


def cpu_baseline(seconds: float) -> dict:
    """Reference-equivalent CPU encode (same aten ops) on the same workload, at the best of
    several torch thread counts (oversubscribing a 256-cpu host is slower than 8 threads)."""
    from ginfinity_amd import synthetic
    from ginfinity_amd.weights import load_checkpoint
    from oracle import gine_torch

    params = gine_torch.prepare(load_checkpoint().state)
    shard = synthetic.roofline_shard(0)
    arrays = (shard.node_features, shard.edge_index, shard.edge_types)
    cpus = os.cpu_count() or 1
    counts = sorted({min(c, cpus) for c in (8, 16, 32, 64, cpus)})
    rates, spent = {}, 0.0
    for threads in counts:
        torch.set_num_threads(threads)
        gine_torch.encode(params, *arrays)                       # warm
        done, began = 0, time.perf_counter()
        while done < 2 or time.perf_counter() - began < seconds / len(counts):
            gine_torch.encode(params, *arrays)
            done += 1
        elapsed = time.perf_counter() - began
        spent += elapsed
        rates[threads] = done * NODES / elapsed
    best = max(rates, key=rates.get)
    listing = ", ".join(f"{t} threads {r / 1e3:.1f} k" for t, r in rates.items())
    return {"value": rates[best], "unit": "nodes/s", "cores": best, "kind": "port",
            "sample": f"encodes of the 60000-node/300000-edge synthetic shard, fp16 model, "
                      f"{spent:.1f} s in all, oracle/gine_torch.py (reference aten op "
                      f"sequence); nodes/s by torch thread count: {listing}; host has "
                      f"{cpus} cpus"}


def distance_leg(rows: int, device) -> dict:
    """BASELINE configs[3]: nearest other row of every row, N x N never materialised."""
    from ginfinity_amd import distance, synthetic
    points = torch.from_numpy(synthetic.unit_rows(0, rows)).to(device)
    # One untimed search of the full size first (workspace, code, and the clock the part settles
    # at under this load: a 4,096-row warm-up left the first full search to find it), then three
    # timed ones, all reported; `seconds` is their median.  Round 3's single timed call read
    # 0.2096 s on the driver's box and 0.1905 s on the builder's: one number cannot tell a box
    # from a ramp.
    distance.nearest(points, metric="l2", exclude_self=True)
    torch.cuda.synchronize(device)
    timed = []
    for _ in range(3):
        began, ended = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        began.record()
        distance.nearest(points, metric="l2", exclude_self=True)
        ended.record()
        torch.cuda.synchronize(device)
        timed.append(began.elapsed_time(ended) * 1e-3)
    seconds = sorted(timed)[1]
    tflops = 2.0 * rows * rows * 128 / seconds / 1e12
    return {"workload": f"all-pairs L2 nearest over {rows} x 128 fp16 unit rows "
                        "(BASELINE configs[3]); parity unpinned: the reference has no "
                        "implementation of this step",
            "seconds": seconds, "seconds_all": timed, "pairs_per_s": rows * rows / seconds,
            "roofline": {"bound": "mfma", "achieved": tflops, "peak": MFMA_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": tflops / MFMA_PEAK_TFLOPS,
                         "kernel": "k_pairwise"}}


def cross_shard(args, rank: int, local_rank: int, world: int, distributed: bool, *,
                device=None, encoder=None, search=None, make_shard=None) -> dict | None:
    """BASELINE configs[4] at a size that fits the run: every rank encodes its shards (no
    collective), the fp16 blocks are exchanged chunk by chunk (all_gather_into_tensor: RCCL
    over xGMI) while the chunks already there are searched, every rank keeps the nearest
    other row of ITS rows over all ranks' rows.  Parity unpinned.

    ``device`` / ``encoder`` / ``search`` / ``make_shard`` replace the GPU pieces (tests: the
    driver logic — shard ownership, staging, the grouped encode step, fences, MAX-reductions,
    offsets, the result line — runs under gloo on CPU tensors with the oracle as the search;
    ``encoder`` then is any object with ``stage_shards`` and ``encode_staged``)."""
    import torch.distributed as dist
    from ginfinity_amd import parallel, synthetic
    on_gpu = device is None
    if on_gpu:
        from ginfinity_amd import Ginfinity
        device = torch.device("cuda", local_rank)
        encoder = Ginfinity.load(f"cuda:{local_rank}", allow_nondeterministic_cuda=True)
    make_shard = make_shard or synthetic.roofline_shard
    owned = parallel.shard_assignment(args.shards, world, rank)
    shards = {s: make_shard(s) for s in owned}

    def fence():
        if distributed:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize(device)

    def longest(seconds: float) -> float:
        if not distributed:
            return seconds
        worst = torch.tensor([seconds], dtype=torch.float64, device=device)
        dist.all_reduce(worst, op=dist.ReduceOp.MAX)
        return float(worst.item())

    # Encode leg: this rank's shards, their micro-batches in groups of four per launch sequence,
    # two groups in flight
    # (Ginfinity.encode_staged = gfy_encode_coo_batch).  The shards are staged on the device
    # first and that upload is timed by itself: `encode` is the hot path with its inputs
    # resident in HBM, `stage` the PCIe-bound feeding of it.  A rank without
    # shards walks the same fences with an empty block.
    fence()
    t0 = time.perf_counter()
    staged, _counts = encoder.stage_shards([shards[s] for s in owned]) if owned else ([], [])
    if on_gpu:
        torch.cuda.synchronize(device)
    stage_s = longest(time.perf_counter() - t0)
    block = (encoder.encode_staged(staged) if staged else      # warm: workspace, result block
             torch.empty((0, 128), dtype=torch.float16, device=device))
    if not staged:
        encoder.encode_staged(encoder.stage_shards([make_shard(0)])[0])
    fence()
    t0 = time.perf_counter()
    if staged:
        encoder.encode_staged(staged, out=block)
    if on_gpu:
        torch.cuda.synchronize(device)
    encode_s = longest(time.perf_counter() - t0)
    # ... and the product path of a rank from HOST arrays: the uploads streamed under the
    # compute (Ginfinity.encode_shards_device), what parallel.encode_owned_shards runs
    streamed_s = None
    if on_gpu and owned:
        for _ in range(2):      # warm: the second call reaches the staging ring's other slots
            encoder.encode_shards_device([shards[s] for s in owned], out=block)   # (page-locked
                                                                                  # allocations)
        fence()
        t0 = time.perf_counter()
        encoder.encode_shards_device([shards[s] for s in owned], out=block)
        torch.cuda.synchronize(device)
        streamed_s = longest(time.perf_counter() - t0)
    fence()
    t1 = time.perf_counter()
    values, indices, offsets = parallel.cross_shard_nearest(
        block, metric="cosine", chunk_rows=args.chunk_rows, search=search)
    if on_gpu:
        torch.cuda.synchronize(device)
    search_s = longest(time.perf_counter() - t1)
    total = offsets[-1]
    line = None
    if rank == 0:
        gathered_bytes = total * 128 * 2 * max(world - 1, 0)      # received by all ranks
        line = {
            "metric": "cross-shard nearest over sharded embeddings (BASELINE configs[4] in "
                      "miniature)", "value": float(total) * total / search_s,
            "unit": "pairs/s", "n_gpus": world, "higher_is_better": True, "scaling": "strong",
            "dtype": "f16", "data": "synthetic", "vs_baseline": None,
            "config": {"workload": f"{args.shards} synthetic 60k-node shards over {world} GPU(s): "
                                   "shard-parallel encode, chunked all-gather, nearest other row "
                                   "(cosine) of every row", "rows_total": total,
                       "chunk_rows": args.chunk_rows, "rank_offsets": offsets,
                       "rccl_ranks": dist.get_world_size() if distributed else 0},
            "encode": {"seconds": encode_s, "nodes_per_s": total / encode_s,
                       "note": "inputs resident on the device, embeddings left there; the "
                               "micro-batches in groups of 4 per launch sequence, two groups in flight"},
            "stage": {"seconds": stage_s,
                      "note": "numpy shards -> device arrays of the owned shards (PCIe, pageable, "
                              "synchronous)"},
            "encode_from_host_arrays": None if streamed_s is None else {
                "seconds": streamed_s, "nodes_per_s": total / streamed_s,
                "note": "numpy shards in, device block out: pinned staging ring, H2D of group "
                        "g + 1 on a copy stream under the compute of group g "
                        "(encode_shards_device)"},
            "exchange_and_search": {"seconds": search_s,
                                    "bytes_received_all_ranks": gathered_bytes,
                                    "tflops": 2.0 * total * total * 128 / search_s / 1e12},
            "sample": [float(values[0]), int(indices[0])] if values.numel() else None}
        print(json.dumps(line))
    return line


def main() -> None:
    args = parse()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if args.dump_outputs is not None and args.workload != "encode":
        raise SystemExit("bench.py: --dump-outputs covers the encode workload only")
    if "RANK" not in os.environ and (args.gpus > 1 or args.spawn):
        launch_ranks(args)            # before anything touches the GPU; does not return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # under torch.distributed.run (RANK set) the process group is always created, so the
    # RCCL path (barrier + MAX all-reduce) is the one exercised even at world size 1
    distributed = "RANK" in os.environ
    if distributed and world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # Rehearsal switches (no multi-GPU box was ever available to this build): the ranks' control
    # flow — fences, MAX-reductions, the repeated leg, who prints — can be run with all ranks on
    # ONE GPU over gloo: GFY_BENCH_BACKEND=gloo GFY_BENCH_ONE_DEVICE=1.  The line then says so
    # (config.rehearsal) and its value is not a scaling figure.
    backend = os.environ.get("GFY_BENCH_BACKEND", "nccl")
    one_device = os.environ.get("GFY_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    if distributed:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    device = torch.device("cuda", local_rank)
    reduce_device = device if backend == "nccl" else torch.device("cpu")
    torch.cuda.set_device(device)
    if args.workload == "cross-shard":
        cross_shard(args, rank, local_rank, world, distributed)
        if distributed:
            dist.destroy_process_group()
        return

    from ginfinity_amd import Ginfinity, synthetic
    from ginfinity_amd import _native as native
    # Shards are independent (graph.py:392-395): `batch` of them go through the hot path in ONE
    # sequence of launches (gfy_encode_coo_batch: count, setup, 4 layer launches, head), and
    # `streams` such batches are in flight, each with its own encoder handle, workspace and
    # output blocks.  A step is still ONE shard: K timed steps = K shards, in ceil(K / batch)
    # calls, the last one smaller.
    lanes = max(1, args.streams)
    batch = max(1, min(args.batch, native.GFY_MAX_BATCH_SHARDS))
    encoders = [Ginfinity.load(f"cuda:{local_rank}", allow_nondeterministic_cuda=True)
                for _ in range(lanes)]
    engines = [e._engine for e in encoders]
    streams = [torch.cuda.Stream(device=device) for _ in range(lanes)]
    engine = engines[0]

    # inputs resident in HBM before the timed region
    shards = [synthetic.roofline_shard(1000 * rank + i) for i in range(POOL)]
    assert all((s.node_count, s.edge_count) == (NODES, EDGES) for s in shards)
    # ... as Ginfinity.stage_shards puts them there: the record boundaries (graph.py:268-271) ride
    # along, and the batch call turns COO into tile plans without global atomics
    # (GFY_BENCH_NO_RECORDS=1: without them, for A/B runs against the counting kernel)
    with_records = os.environ.get("GFY_BENCH_NO_RECORDS", "") in ("", "0")
    inputs = [engine.upload_arrays(s.node_features, s.edge_index, s.edge_types, None,
                                   node_ptr=s.node_ptr if with_records else None,
                                   edge_ptr=s.edge_ptr if with_records else None)[:3]
              for s in shards]
    outputs = [[torch.empty((NODES, 128), dtype=torch.float16, device=device)
                for _ in range(batch)] for _ in range(lanes)]
    handles = [s.cuda_stream for s in streams]
    prepared = {}

    def call(lane: int, first: int, count: int) -> None:
        """Shards first .. first + count - 1 (cycling through the pool) as one batch."""
        key = (lane, first % POOL, count)
        step = prepared.get(key)
        if step is None:
            step = prepared[key] = engines[lane].prepare_batch_step(
                [(*inputs[(first + k) % POOL], None, outputs[lane][k]) for k in range(count)])
        step(handles[lane])

    def run(steps: int) -> tuple[int, int]:
        """`steps` shards, batch by batch, round-robin over the lanes; returns the lane and the
        output slot of the last shard."""
        done, index, last = 0, 0, (0, 0)
        while done < steps:
            count = min(batch, steps - done)
            call(index % lanes, done, count)
            last = (index % lanes, count - 1)
            done += count
            index += 1
        return last

    def prebind(steps: int) -> None:
        """Build (and run once) every pre-bound step that `run(steps)` uses, without running
        all `steps` shards."""
        done, index, seen = 0, 0, set()
        while done < steps:
            count = min(batch, steps - done)
            key = (index % lanes, done % POOL, count)
            if key not in seen:
                seen.add(key)
                call(index % lanes, done, count)
            done += count
            index += 1

    def fence() -> None:
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(device)

    # set-up, not measurement: build every pre-bound step once and let the part reach its
    # working clocks (a cold MI355X needs tens of milliseconds of load), whatever W is
    settle = time.perf_counter() + float(os.environ.get("GFY_BENCH_SETTLE_S", "0.25"))
    prebind(args.steps)
    torch.cuda.synchronize(device)
    while time.perf_counter() < settle:
        run(batch * lanes)
        torch.cuda.synchronize(device)

    run(args.warmup)
    fence()
    began = time.perf_counter()
    last_lane, last_slot = run(args.steps)
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - began
    if distributed:
        worst = torch.tensor([elapsed], dtype=torch.float64, device=reduce_device)
        dist.all_reduce(worst, op=dist.ReduceOp.MAX)
        elapsed = float(worst.item())
    fence()
    # what the last timed step computed: the embeddings of shard (K - 1) mod POOL, read before
    # anything else writes the lane's output blocks
    if rank == 0 and args.dump_outputs is not None:
        folder = Path(args.dump_outputs)
        folder.mkdir(parents=True, exist_ok=True)
        np.save(folder / "embeddings.npy",
                outputs[last_lane][last_slot].float().cpu().numpy())
    # --full: the K timed steps may cover very little time (K = 20: under 2 ms): the
    # same K steps are repeated until at least MIN_TIMED_S have been timed, and both figures are
    # reported — `value` stays the contract's (exactly K steps)
    repeats, long_elapsed = 0, 0.0
    if args.full and (rank == 0 or distributed):
        repeats = max(1, int(np.ceil(MIN_TIMED_S / max(elapsed, 1e-6))))
        repeats = min(repeats, 4096)
        fence()
        began = time.perf_counter()
        for _ in range(repeats):
            run(args.steps)
        torch.cuda.synchronize(device)
        long_elapsed = time.perf_counter() - began
        if distributed:
            worst = torch.tensor([long_elapsed], dtype=torch.float64, device=reduce_device)
            dist.all_reduce(worst, op=dist.ReduceOp.MAX)
            long_elapsed = float(worst.item())
        fence()

    # ---- per-kernel device time, rank 0 ------------------------------------------------------
    roofline = None
    kernels = None
    if rank == 0 and args.full:
        full = min(batch, max(args.steps, 1))          # shards per launch in what follows
        launch_bytes, launch_flops = LAYER_BYTES * full, LAYER_FLOPS * full

        def layer_roofline(layer_ms: float) -> dict:
            achieved = launch_bytes / (layer_ms * 1e-3) / 1e9
            return {"achieved": achieved, "frac": achieved / HBM_PEAK_GBS, "kernel_ms": layer_ms,
                    "mfma_tflops": launch_flops / (layer_ms * 1e-3) / 1e12,
                    "mfma_frac": launch_flops / (layer_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS}

        # marks: setup | layer 1 .. layer L | stand-alone head (0 for fp16 output: the last
        # layer's launch runs head + normalise too, in the one-round kernel and in the
        # persistent-rounds kernel alike); layers 1 .. L-1 carry no head and are the ones
        # the roofline figure is about
        def plain_layers(times: list[float]) -> list[float]:
            return times[1:-2]

        # (1) the timed configuration: every lane busy.  With several streams in flight the
        # span between two HIP events of one stream contains the other streams' kernels, so
        # the layer launches time themselves on the device clock (first workgroup start ->
        # last workgroup end, gfy_encoder_set_timing(3)): the duration rocprofv3 reports
        for e in engines:
            e.set_timing(3)
        samples = []
        for _ in range(8):
            for lane in range(lanes):
                call(lane, 0, full)
            torch.cuda.synchronize(device)
            for e in engines:
                per_layer = e.kernel_times_ms()
                samples += per_layer[:-1]            # the last launch carries the head
        for e in engines:
            e.set_timing(False)
        timed_ms = sum(samples) / len(samples)

        # (2) one batch at a time on lane 0: an event pair around the layer launches (timing
        # mode 2), then the whole call without the marks
        engine.set_timing(2)
        rounds = 30
        sums = None
        for _ in range(rounds):
            call(0, 0, full)
            torch.cuda.synchronize(device)
            times = engine.kernel_times_ms()
            sums = times if sums is None else [a + b for a, b in zip(sums, times)]
        engine.set_timing(False)
        mean = [t / rounds for t in sums]
        with torch.cuda.stream(streams[0]):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(rounds):
                call(0, 0, full)
            e1.record()
        torch.cuda.synchronize(device)
        alone_call_ms = e0.elapsed_time(e1) / rounds
        plain = plain_layers(mean)
        # the kernel the encoder actually launched (a checkpoint with edge_dim > 12 or a forced
        # GFY_OPT_LAYER_KERNEL runs another one than this run's sizes suggest)
        kernel_name = {1: "k_gine_layer_f16", 3: "k_gine_layer_q", 4: "k_gine_layer_w",
                       5: "k_gine_layer_x"}.get(engine.last_layer_kernel(), "k_gine_layer_w")
        traffic, traffic_source = measured_traffic(kernel_name, full * NODES)
        mfma_busy, coexec, counter_source = measured_counters(kernel_name)
        # `frac` / `achieved` / `kernel_ms`: ONE launch by itself — what a profiler reports for
        # the kernel and what profiles/ holds.  The span of a launch while another batch's
        # kernels share the CUs is kept aside (`in_flight`): it contains the others' work.
        roofline = {
            "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "kernel": kernel_name, "shards_per_launch": full,
            "algorithmic_bytes_per_launch": launch_bytes,
            "configuration": "one batch at a time, one HIP event pair around the plain layer "
                             "launches (the kernel by itself: rocprofv3's average duration of "
                             "the same command is committed under profiles/)",
            **layer_roofline(sum(plain) / len(plain)),
            "traffic": traffic, "traffic_source": traffic_source,
            "mfma_busy_frac": mfma_busy, "coexec_frac": coexec, "counter_source": counter_source,
            "isolated": layer_roofline(sum(plain) / len(plain)),
            "in_flight": {"configuration": f"{lanes} batch(es) of {full} shard(s) in flight on "
                                           f"{lanes} stream(s), as timed; kernel_ms = device "
                                           "clock, first workgroup start to last end: with "
                                           "several streams the span contains the other "
                                           "batches' workgroups",
                          **layer_roofline(timed_ms)},
            "pipeline_frac": PIPELINE_BYTES * world * args.steps / elapsed / 1e9
                             / (HBM_PEAK_GBS * world),
            "pipeline_frac_long": (PIPELINE_BYTES * world * args.steps * repeats / long_elapsed
                                   / 1e9 / (HBM_PEAK_GBS * world)) if repeats else None,
        }
        kernels = {"configuration": f"one batch of {full} shard(s) at a time on one stream "
                                    "(gfy_encode_coo_batch: k_encode_setup_rec — or k_csr_count + "
                                    "k_encode_setup_coo without record boundaries —, 4 layer "
                                    "launches, the last with head + normalise)",
                   "whole_call_ms": alone_call_ms, "per_shard_ms": alone_call_ms / full,
                   "csr_finish_plans_input_linear_ms": mean[0], "layer_ms": plain,
                   "last_layer_with_head_normalise_ms": mean[-2]}

    distance = None
    if args.full and rank == 0 and world == 1 and args.distance_rows > 0:
        distance = distance_leg(args.distance_rows, device)

    baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        baseline = cpu_baseline(args.cpu_seconds)

    if rank == 0:
        value = world * args.steps * NODES / elapsed
        print(json.dumps({
            "metric": "encoded nodes/sec on 60k-node/300k-edge shards",
            "value": value, "unit": "nodes/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "timed_ms": 1e3 * elapsed,
            "repeated": {"repeats": repeats, "timed_ms": 1e3 * long_elapsed,
                         "value": world * args.steps * repeats * NODES / long_elapsed,
                         "note": f"the same {args.steps} steps repeated until >= "
                                 f"{1e3 * MIN_TIMED_S:.0f} ms were timed"} if repeats else None,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16", "data": "synthetic",
            "config": {"workload": "synthetic shard max_batch_nodes=60000 / "
                                   "max_batch_edges=300000 (BASELINE configs[2]), "
                                   "fp16 model, fp16 normalised output",
                       "nodes_per_step": NODES, "edges_per_step": EDGES,
                       "shards_per_rank": POOL, "streams_per_gpu": lanes,
                       "shards_per_launch": batch,
                       "rccl_ranks": dist.get_world_size() if distributed and backend == "nccl" else 0,
                       **({"rehearsal": f"{world} ranks over {backend}"
                                        + (" sharing ONE GPU" if one_device else "")}
                          if backend != "nccl" or one_device else {}),
                       "parallelism": f"shard-parallel x{world}"},
            "roofline": roofline, "cpu_baseline": baseline, "distance": distance,
            "kernels_ms": kernels,
        }))
    if distributed:
        fence()          # rank 0's extra measurements are over: the ranks leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
