"""Top-k measurement: the k nearest rows of every row over N x 128 fp16 unit rows (N x N never
materialised), against what a user had before it, all in one process on one device:

  (a) ``distance.nearest`` — one neighbour, the nearest-row kernel;
  (b) ``torch.topk`` over ``distance.pairwise`` blocks of 4,096 a-rows, the only route to k
      neighbours without this kernel: ``--dense-blocks`` blocks (at least 8) are timed and the
      whole search is extrapolated from them.

Per metric and k: ``--warmup`` untimed runs, ``--repeats`` timed runs (HIP events around one
call), min, median and max reported; the ratios use the medians.  Nothing else may run on the
device.  The document names the run: host, UTC time, device, ROCm / torch versions, the commit
(``--commit``, or ``git rev-parse HEAD`` where the tree is a checkout) and a SHA-256 over the
kernel sources that were measured.  Writes one JSON document (default
profiles/topk_bench.json) and prints it.

``--records MEAN`` adds a leg per metric and k: the same rows cut into records of about MEAN
rows (sizes uniform in 1 .. 2 MEAN - 1, seed 0), searched with ``exclude_records`` and, next
to it in the same run, with ``exclude_self``; both times and their ratio are written, no ratio
is expected in advance.

``--distinct`` (with ``--records``) adds a further leg: ``exclude_records`` together with
``distinct_records`` (at most one hit per record) next to ``exclude_records`` alone, same rows,
same run; both times and their ratio are written, no ratio is expected in advance either.

    python tools/bench_topk.py --rows 1000000
    python tools/bench_topk.py --rows 1000000 --records 300
    python tools/bench_topk.py --rows 1000000 --records 300 --distinct
"""
from __future__ import annotations

import argparse
import datetime
import hashlib
import json
import platform
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ginfinity_amd import distance, synthetic  # noqa: E402

DENSE_ROWS = 4_096
KERNEL_SOURCES = ("pairwise.hip", "pairwise_sweep.inc", "pairwise_topk.hip", "pairwise_topk.inc",
                  "pairwise_topk_ranges.hip", "pairwise_topk_distinct.hip", "gfy_common.h",
                  "gfy_api.hip")


def _commit() -> str | None:
    try:
        done = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True,
                              text=True, timeout=10)
    except (OSError, subprocess.SubprocessError):
        return None
    return done.stdout.strip() if done.returncode == 0 and done.stdout.strip() else None


def _sources_sha256() -> str:
    digest = hashlib.sha256()
    for name in KERNEL_SOURCES:
        digest.update((ROOT / "ginfinity_amd" / "csrc" / name).read_bytes())
    return digest.hexdigest()


def _timed(call, repeats: int, warmup: int) -> list[float]:
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    seconds = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        seconds.append(e0.elapsed_time(e1) * 1e-3)
    return seconds


def _span(seconds: list[float]) -> dict:
    return {"min": min(seconds), "median": statistics.median(seconds), "max": max(seconds),
            "runs": seconds}


def _record_counts(rows: int, mean: int) -> list[int]:
    """Record sizes uniform in 1 .. 2 mean - 1 that sum to ``rows`` (the last one cut short)."""
    sizes = np.random.default_rng(0).integers(1, 2 * mean, size=2 * rows // mean + 16)
    ends = np.cumsum(sizes)
    keep = int(np.searchsorted(ends, rows))
    counts = sizes[:keep + 1].copy()
    counts[keep] -= ends[keep] - rows
    assert counts.sum() == rows and counts.min() >= 0
    return [int(c) for c in counts]


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--dense-blocks", type=int, default=8)
    parser.add_argument("--ks", default="1,4,8,16")
    parser.add_argument("--records", type=int, default=0, metavar="MEAN",
                        help="also time exclude_records over records of about MEAN rows")
    parser.add_argument("--distinct", action="store_true",
                        help="with --records: also time distinct_records next to exclude_records")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "topk_bench.json"))
    args = parser.parse_args()
    if args.dense_blocks < 8:
        parser.error("--dense-blocks: at least 8")
    if args.records < 0:
        parser.error("--records: a positive mean")
    if args.distinct and not args.records:
        parser.error("--distinct needs --records MEAN")
    ks = [int(k) for k in args.ks.split(",")]
    rows = torch.from_numpy(synthetic.unit_rows(0, args.rows)).cuda()
    n = args.rows
    blocks_total = (n + DENSE_ROWS - 1) // DENSE_ROWS
    result = {"metric": "exact top-k over N x 128 fp16 embeddings, exclude_self",
              "rows": n, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "kernel_sources": list(KERNEL_SOURCES), "kernel_sources_sha256": _sources_sha256(),
              "command": "python tools/bench_topk.py " + " ".join(sys.argv[1:]),
              "repeats": args.repeats, "warmup": args.warmup, "ratios_use": "median",
              "dense_rows_per_block": DENSE_ROWS, "dense_blocks_timed": args.dense_blocks,
              "distances": {}}
    counts = _record_counts(n, args.records) if args.records else None
    if counts is not None:
        result["records"] = {"mean_rows_asked": args.records, "records": len(counts),
                             "largest": max(counts), "sizes": "uniform in 1 .. 2 mean - 1, seed 0"}
        ranges = distance.record_ranges(counts, rows.device)     # on the device: not in the times
    for metric in ("l2", "cosine"):
        nearest = _timed(lambda: distance.nearest(rows, metric=metric, exclude_self=True),
                         args.repeats, args.warmup)
        entry = {"nearest_seconds": _span(nearest), "topk": {}}
        print(f"{metric} nearest {statistics.median(nearest):.4f} s", file=sys.stderr, flush=True)
        for k in ks:
            workspace = distance.TopKWorkspace()
            topk = _timed(lambda: distance.topk(rows, k=k, metric=metric, exclude_self=True,
                                                workspace=workspace), args.repeats, args.warmup)

            def dense_route():
                # the self pair is masked the way a user would: the diagonal of every block
                for block in range(args.dense_blocks):
                    first = block * DENSE_ROWS % max(n - DENSE_ROWS, 1)
                    part = distance.pairwise(rows[first:first + DENSE_ROWS], rows, metric=metric)
                    own = torch.arange(part.shape[0], device=part.device)
                    part[own, own + first] = float("inf") if metric == "l2" else float("-inf")
                    torch.topk(part, k, dim=1, largest=metric == "cosine")

            dense = [t * blocks_total / args.dense_blocks
                     for t in _timed(dense_route, args.repeats, args.warmup)]
            mid, mid_nearest, mid_dense = (statistics.median(topk), statistics.median(nearest),
                                           statistics.median(dense))
            entry["topk"][str(k)] = {
                "seconds": _span(topk),
                "pairs_per_s": n * n / mid,
                "ratio_to_nearest": mid / mid_nearest,
                "dense_topk_seconds_extrapolated": _span(dense),
                "speedup_over_dense_topk": mid_dense / mid}
            print(f"{metric} k={k}: topk {mid:.4f} s, {mid / mid_nearest:.2f} x nearest, dense "
                  f"route {mid_dense:.2f} s = {mid_dense / mid:.1f} x topk", file=sys.stderr,
                  flush=True)
            if counts is not None:   # the same rows, the same k, one after the other in this run
                beside = _timed(lambda: distance.topk(rows, k=k, metric=metric, exclude_self=True,
                                                      workspace=workspace),
                                args.repeats, args.warmup)
                records = _timed(lambda: distance.topk(rows, k=k, metric=metric,
                                                       exclude_ranges=ranges, workspace=workspace),
                                 args.repeats, args.warmup)
                ratio = statistics.median(records) / statistics.median(beside)
                entry["topk"][str(k)]["records"] = {
                    "exclude_records_seconds": _span(records),
                    "exclude_self_seconds": _span(beside),
                    "exclude_records_over_exclude_self": ratio}
                print(f"{metric} k={k}: exclude_records {statistics.median(records):.4f} s = "
                      f"{ratio:.3f} x exclude_self", file=sys.stderr, flush=True)
            if counts is not None and args.distinct:   # counts are checked on the host per call
                beside = _timed(lambda: distance.topk(rows, k=k, metric=metric,
                                                      exclude_records=counts, workspace=workspace),
                                args.repeats, args.warmup)
                distinct = _timed(lambda: distance.topk(rows, k=k, metric=metric,
                                                        exclude_records=counts,
                                                        distinct_records=counts,
                                                        workspace=workspace),
                                  args.repeats, args.warmup)
                ratio = statistics.median(distinct) / statistics.median(beside)
                entry["topk"][str(k)]["distinct"] = {
                    "exclude_records_distinct_records_seconds": _span(distinct),
                    "exclude_records_seconds": _span(beside),
                    "distinct_over_exclude_records": ratio}
                print(f"{metric} k={k}: distinct_records {statistics.median(distinct):.4f} s = "
                      f"{ratio:.3f} x exclude_records", file=sys.stderr, flush=True)
        result["distances"][metric] = entry
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
