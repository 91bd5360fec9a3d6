"""Chaining measurement: ``align.chain_runs`` next to the ``distance.within`` and
``align.hit_runs`` calls that feed it, over N x 128 fp16 unit rows against themselves in records
of ``--record`` rows, all in one process on one device.

Two cases.  ``random``: the rows of tools/bench_runs.py, a cosine threshold chosen as there so
that a row has about ``--hits`` hits besides itself; the runs spread over every record pair, one
wave each.  ``thinned``: the same rows with record 1 overwritten by a copy of record 0 in which
every third row is replaced by its negative, so that the copy is about ``--record`` / 3 runs of
two hits with gaps of one in ONE record pair (and as many in the mirrored pair), which one wave
chains serially.  Per case and function: ``--warmup`` untimed runs, ``--repeats`` timed runs (HIP
events around one call; every function includes its waits for a total), min, median and max
reported; the ratios use the medians.  Nothing else may run on the device.  Writes one JSON
document (default profiles/chains_bench.json) and prints it.

    python tools/bench_chains.py --rows 262144
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
from bench_runs import _measured_arguments  # noqa: E402
from bench_within import _commit, _span, _threshold, _timed  # noqa: E402
from ginfinity_amd import align, distance, synthetic  # noqa: E402


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=262_144)
    parser.add_argument("--record", type=int, default=4_096, help="rows per record")
    parser.add_argument("--hits", type=int, default=10, help="hits per row the threshold aims at")
    parser.add_argument("--max-gap", type=int, default=8)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--out", default=str(ROOT / "profiles" / "chains_bench.json"))
    args = parser.parse_args()
    n, record = args.rows, args.record
    if record < 3 or n % record or n < 2 * record:
        parser.error("--rows must be a multiple of --record and hold two records at least")
    counts = [record] * (n // record)
    rows = torch.from_numpy(synthetic.unit_rows(0, n)).cuda()
    threshold = _threshold(rows, "cosine", args.hits)
    result = {"metric": "chains of the diagonal runs of the hits of a cosine radius search over "
                        "N x 128 fp16 unit rows, exclude_self",
              "rows": n, "rows_per_record": record, "threshold": threshold,
              "max_gap": args.max_gap, "max_shift": args.max_gap,
              "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "command": "python tools/bench_chains.py " + " ".join(_measured_arguments()),
              "repeats": args.repeats, "warmup": args.warmup, "ratios_use": "median",
              "cases": {}}
    for case in ("random", "thinned"):
        if case == "thinned":
            rows[record:2 * record] = rows[:record]
            rows[record:2 * record:3] = -rows[:record:3]
        search = distance.WithinWorkspace()

        def within():
            return distance.within(rows, threshold=threshold, metric="cosine", exclude_self=True,
                                   workspace=search)
        hits = within()
        seeds, links = align.RunsWorkspace(), align.ChainsWorkspace()
        runs = align.hit_runs(hits, counts_a=counts, workspace=seeds)
        searched = _timed(within, args.repeats, args.warmup)
        seeded = _timed(lambda: align.hit_runs(hits, counts_a=counts, workspace=seeds),
                        args.repeats, args.warmup)
        chained = _timed(lambda: align.chain_runs(runs, max_gap=args.max_gap, workspace=links),
                         args.repeats, args.warmup)
        chains = align.chain_runs(runs, max_gap=args.max_gap, workspace=links)
        pair = (runs.pairs[:, 0].to(torch.int64) << 31) | runs.pairs[:, 1].to(torch.int64)
        mid_within, mid_runs, mid_chains = (statistics.median(x)
                                            for x in (searched, seeded, chained))
        result["cases"][case] = {
            "hits": int(hits.indices.numel()), "runs": int(runs.lengths.numel()),
            "record_pairs": int(torch.unique(pair).numel()),
            "most_runs_in_a_pair": int(torch.unique(pair, return_counts=True)[1].max().item()),
            "chains": int(chains.counts.numel()),
            "most_runs_in_a_chain": int(chains.counts.max().item()),
            "within_seconds": _span(searched), "hit_runs_seconds": _span(seeded),
            "chain_runs_seconds": _span(chained),
            "chain_runs_over_hit_runs": mid_chains / mid_runs,
            "chain_runs_over_within": mid_chains / mid_within}
        print(f"{case}: {result['cases'][case]['runs']} runs in "
              f"{result['cases'][case]['record_pairs']} pairs, {result['cases'][case]['chains']} "
              f"chains, longest {result['cases'][case]['most_runs_in_a_chain']} runs; within "
              f"{mid_within:.4f} s, hit_runs {mid_runs:.4f} s, chain_runs {mid_chains:.4f} s = "
              f"{mid_chains / mid_runs:.3f} x hit_runs, {mid_chains / mid_within:.3f} x within",
              file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
