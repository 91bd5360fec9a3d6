"""Record-score measurement: ``distance.record_scores`` over N x N rows of 128-d fp16 unit rows cut
into records of about ``--records`` rows (N x N never materialised, the N x R row-level
intermediate walked in blocks), next to ``distance.nearest`` on the same rows in the same
process on one device — the sweep does the same MFMA work with a lighter epilogue plus the
flushes at the records' ends, so the number to read is the ratio of the two.

Per metric: ``--warmup`` untimed runs, ``--repeats`` timed runs (HIP events around one call),
min, median and max reported; the ratio uses the medians.  No target is set: nobody had measured
any part of this before the first run.  Nothing else may run on the device.  The document names
the run: host, UTC time, device, ROCm / torch versions, the commit (``--commit``, or ``git
rev-parse HEAD`` where the tree is a checkout) and a SHA-256 of pairwise_records.hip.  Writes one
JSON document (default profiles/records_bench.json) and prints it.

    python tools/bench_records.py --rows 1000000 --records 200
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

KERNEL_SOURCE = "pairwise_records.hip"


def _commit() -> str | None:
    try:
        done = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True,
                              text=True, timeout=10)
    except (OSError, subprocess.SubprocessError):
        return None
    return done.stdout.strip() if done.returncode == 0 and done.stdout.strip() else None


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
    parser.add_argument("--records", type=int, default=200, metavar="MEAN",
                        help="records of about MEAN rows")
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--max-workspace-bytes", type=int, default=distance.RECORD_WORKSPACE_BYTES)
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "records_bench.json"))
    args = parser.parse_args()
    if args.records < 1:
        parser.error("--records: a positive mean")
    n = args.rows
    rows = torch.from_numpy(synthetic.unit_rows(0, n)).cuda()
    counts = _record_counts(n, args.records)
    blocks = distance.plan_record_blocks(counts, len(counts), args.max_workspace_bytes)
    source = ROOT / "ginfinity_amd" / "csrc" / KERNEL_SOURCE
    result = {"metric": "record_scores over N x N rows of 128-d fp16 embeddings, self-search",
              "rows": n, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "kernel_source": KERNEL_SOURCE,
              "kernel_source_sha256": hashlib.sha256(source.read_bytes()).hexdigest(),
              "command": "python tools/bench_records.py " + " ".join(sys.argv[1:]),
              "repeats": args.repeats, "warmup": args.warmup, "ratio_uses": "median",
              "records": {"mean_rows_asked": args.records, "records": len(counts),
                          "largest": max(counts), "sizes": "uniform in 1 .. 2 mean - 1, seed 0"},
              "max_workspace_bytes": args.max_workspace_bytes, "a_blocks": len(blocks),
              "distances": {}}
    keeper_nearest, keeper = distance.NearestWorkspace(), distance.RecordWorkspace()
    for metric in ("l2", "cosine"):
        nearest = _timed(lambda: distance.nearest(rows, metric=metric, workspace=keeper_nearest),
                         args.repeats, args.warmup)
        scores = _timed(lambda: distance.record_scores(
            rows, counts_a=counts, metric=metric, max_workspace_bytes=args.max_workspace_bytes,
            workspace=keeper), args.repeats, args.warmup)
        mid, mid_nearest = statistics.median(scores), statistics.median(nearest)
        result["distances"][metric] = {"nearest_seconds": _span(nearest),
                                       "record_scores_seconds": _span(scores),
                                       "pairs_per_s": n * n / mid,
                                       "ratio_to_nearest": mid / mid_nearest}
        print(f"{metric}: nearest {mid_nearest:.4f} s, record_scores {mid:.4f} s = "
              f"{mid / mid_nearest:.2f} x nearest ({len(blocks)} a-blocks)", file=sys.stderr,
              flush=True)
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
