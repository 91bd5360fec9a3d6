"""Radius-search measurement: ``distance.count_within`` and ``distance.within`` over N x 128 fp16
unit rows against themselves (N x N never materialised), next to ``distance.nearest`` on the
same rows, all in one process on one device.

The threshold is chosen per metric from a dense block of 1,024 sampled rows so that a row has
about ``--hits`` hits besides itself; the hits per row it really gives are reported.  Per metric
and function: ``--warmup`` untimed runs, ``--repeats`` timed runs (HIP events around one call;
``within`` includes its wait for the total and the allocation of the hits), min, median and max
reported; the ratios use the medians.  Nothing else may run on the device.  The document names
the run as tools/bench_topk.py does.  Writes one JSON document (default
profiles/within_bench.json) and prints it.

    python tools/bench_within.py --rows 262144
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

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ginfinity_amd import distance, synthetic  # noqa: E402

SAMPLE_ROWS = 1_024
KERNEL_SOURCES = ("pairwise.hip", "pairwise_sweep.inc", "pairwise_within.hip", "gfy_common.h",
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


def _threshold(rows: torch.Tensor, metric: str, hits: int) -> float:
    """The median over 1,024 sampled rows of the value of the (hits + 1)-th best pair, the row
    itself being the best: about ``hits`` other rows pass it."""
    step = max(rows.shape[0] // SAMPLE_ROWS, 1)
    part = distance.pairwise(rows[::step][:SAMPLE_ROWS].contiguous(), rows, metric=metric)
    kth = torch.topk(part, hits + 1, dim=1, largest=metric == "cosine").values[:, hits]
    return float(kth.median().item())


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=262_144)
    parser.add_argument("--hits", type=int, default=10, help="hits per row the threshold aims at")
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "within_bench.json"))
    args = parser.parse_args()
    rows = torch.from_numpy(synthetic.unit_rows(0, args.rows)).cuda()
    n = args.rows
    result = {"metric": "radius search over N x 128 fp16 unit rows, exclude_self",
              "rows": n, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "kernel_sources": list(KERNEL_SOURCES), "kernel_sources_sha256": _sources_sha256(),
              "command": "python tools/bench_within.py " + " ".join(sys.argv[1:]),
              "repeats": args.repeats, "warmup": args.warmup, "ratios_use": "median",
              "distances": {}}
    for metric in ("l2", "cosine"):
        threshold = _threshold(rows, metric, args.hits)
        workspace = distance.WithinWorkspace()
        nearest = _timed(lambda: distance.nearest(rows, metric=metric, exclude_self=True),
                         args.repeats, args.warmup)
        count = _timed(lambda: distance.count_within(rows, threshold=threshold, metric=metric,
                                                     exclude_self=True, workspace=workspace),
                       args.repeats, args.warmup)
        both = _timed(lambda: distance.within(rows, threshold=threshold, metric=metric,
                                              exclude_self=True, workspace=workspace),
                      args.repeats, args.warmup)
        total = int(distance.within(rows, threshold=threshold, metric=metric, exclude_self=True,
                                    workspace=workspace).offsets[-1].item())
        mid_nearest, mid_count, mid_both = (statistics.median(x) for x in (nearest, count, both))
        result["distances"][metric] = {
            "threshold": threshold, "hits": total, "hits_per_row": total / n,
            "nearest_seconds": _span(nearest), "count_within_seconds": _span(count),
            "within_seconds": _span(both), "pairs_per_s_count": n * n / mid_count,
            "count_within_over_nearest": mid_count / mid_nearest,
            "within_over_nearest": mid_both / mid_nearest}
        print(f"{metric}: threshold {threshold:.4f}, {total / n:.2f} hits per row; nearest "
              f"{mid_nearest:.4f} s, count_within {mid_count:.4f} s = "
              f"{mid_count / mid_nearest:.2f} x, within {mid_both:.4f} s = "
              f"{mid_both / mid_nearest:.2f} x", file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
