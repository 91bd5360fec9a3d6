"""Seeding measurement: ``align.hit_runs`` next to the ``distance.within`` call that produced its
hits, over N x 128 fp16 unit rows against themselves in records of ``--record`` rows, all in one
process on one device.

Two cases.  ``random``: the rows of tools/bench_within.py, a cosine threshold chosen as there so
that a row has about ``--hits`` hits besides itself; nearly every run has length 1.  ``planted``:
the same rows with record 1 overwritten by a bit-identical copy of record 0, so that two runs of
``--record`` hits are in it and one lane walks each of them serially.  Per case and function:
``--warmup`` untimed runs, ``--repeats`` timed runs (HIP events around one call; both functions
include their wait for a total), min, median and max reported; the ratio ``hit_runs`` / ``within``
uses the medians.  Nothing else may run on the device.  Writes one JSON document (default
profiles/runs_bench.json) and prints it.

    python tools/bench_runs.py --rows 262144
"""
from __future__ import annotations

import argparse
import datetime
import json
import platform
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_within import _commit, _span, _threshold, _timed  # noqa: E402
from ginfinity_amd import align, distance, synthetic  # noqa: E402


def _measured_arguments() -> list[str]:
    """The command line without ``--out``: where the document goes is no part of the run."""
    kept, skip = [], False
    for argument in sys.argv[1:]:
        if skip or argument.startswith("--out="):
            skip = False
        elif argument == "--out":
            skip = True
        else:
            kept.append(argument)
    return kept


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=262_144)
    parser.add_argument("--record", type=int, default=4_096, help="rows per record")
    parser.add_argument("--hits", type=int, default=10, help="hits per row the threshold aims at")
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "runs_bench.json"))
    args = parser.parse_args()
    n, record = args.rows, args.record
    if record < 1 or n % record or n < 2 * record:
        parser.error("--rows must be a multiple of --record and hold two records at least")
    counts = [record] * (n // record)
    rows = torch.from_numpy(synthetic.unit_rows(0, n)).cuda()
    threshold = _threshold(rows, "cosine", args.hits)
    result = {"metric": "diagonal runs of the hits of a cosine radius search over N x 128 fp16 "
                        "unit rows, exclude_self",
              "rows": n, "rows_per_record": record, "threshold": threshold,
              "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "command": "python tools/bench_runs.py " + " ".join(_measured_arguments()),
              "repeats": args.repeats, "warmup": args.warmup, "ratios_use": "median",
              "cases": {}}
    for case in ("random", "planted"):
        if case == "planted":
            rows[record:2 * record] = rows[:record]
        search = distance.WithinWorkspace()

        def within():
            return distance.within(rows, threshold=threshold, metric="cosine", exclude_self=True,
                                   workspace=search)
        hits = within()
        workspace = align.RunsWorkspace()
        searched = _timed(within, args.repeats, args.warmup)
        seeded = _timed(lambda: align.hit_runs(hits, counts_a=counts, workspace=workspace),
                        args.repeats, args.warmup)
        runs = align.hit_runs(hits, counts_a=counts, workspace=workspace)
        total = int(hits.indices.numel())
        mid_within, mid_runs = statistics.median(searched), statistics.median(seeded)
        result["cases"][case] = {
            "hits": total, "hits_per_row": total / n, "runs": int(runs.lengths.numel()),
            "longest_run": int(runs.lengths.max().item()) if runs.lengths.numel() else 0,
            "within_seconds": _span(searched), "hit_runs_seconds": _span(seeded),
            "hit_runs_over_within": mid_runs / mid_within}
        print(f"{case}: {total / n:.2f} hits per row, {int(runs.lengths.numel())} runs, longest "
              f"{result['cases'][case]['longest_run']}; within {mid_within:.4f} s, hit_runs "
              f"{mid_runs:.4f} s = {mid_runs / mid_within:.3f} x", file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
