"""Local-alignment measurement: ``align.local_align`` over ``--pairs`` pairs of records of 200 to
600 rows of 128-d fp16 unit rows on one device, reported as pairs/s and cell updates/s (a cell
update is one (i, j) of a pair's ``Lq x Lr`` dynamic program, the cosine included).

``--warmup`` untimed runs, ``--repeats`` timed runs (HIP events around one call), min, median
and max reported; the rates use the median.  No target is set: nobody had measured any part of
this before the first run.  For scale only, a host numpy float32 dynamic program of the same
recurrences (anti-diagonal by anti-diagonal, from cosines the device computed) is timed on
``--host-pairs`` of the pairs.  Nothing else may run on the device.  The document names the run:
host, UTC time, device, ROCm / torch versions, the commit (``--commit``, or ``git rev-parse
HEAD`` where the tree is a checkout) and a SHA-256 of align_kernels.hip.  Writes one JSON document
(default profiles/align_bench.json) and prints it.

``--spans`` times ``align.local_spans`` (score, start and end) after ``local_align`` in the same
run, on the same pairs and with the same warm-up and repeats, and adds ``spans_seconds``,
``spans_cell_updates_per_s``, ``spans_over_local_align`` (the ratio of the two medians) and the
SHA-256 of the span kernel's sources; without the flag nothing changes.

``--paths`` times ``align.local_paths`` (score, start, end and the aligned path: the span launch,
the copy of starts and ends to the host, the trace launch on the boxes and the compaction) next
to ``align.local_spans`` on the same pairs, and adds ``paths`` to the document: both medians,
their ratio, the ops and the box cells of the run.  Random records share nothing, so their
alignments are a few cells long and the trace has next to nothing to do; the same two calls
are therefore timed a second time on every record paired with ITSELF (``paths_self``), where the
box is the whole matrix and the path its whole diagonal: the most a trace can be asked for.

``--global`` and ``--within`` time ``align.global_align`` (``within=False`` / ``True``) after
``local_align`` on the same pairs, and add ``global`` / ``within`` to the document: the seconds,
pairs/s, cell updates/s and ``over_local_align``, the ratio of the two medians.  The loop is
the local aligner's, so the ratio is information and no gate.

``--band W`` times the same pairs inside a band of ``W`` diagonals around diagonal 0 (``band =
(-(W // 2), W - 1 - W // 2)`` for every pair) next to the call without a band, and adds ``band``
to the document: ``local_align`` with the band, its seconds, pairs/s and ``over_unbanded`` (the
ratio of the two medians), the cells inside the band and the steps per strip by the
kernel's loop bounds (arithmetic, counted on the host); with ``--spans`` the same for
``local_spans``, with ``--paths`` for ``local_paths`` (on the pairs and on every record with
itself, whose diagonal 0 is the path).  Random records share nothing: the band changes which
alignment is found, and the times say what the band saves, not what it finds.

``--box MARGIN`` is a measurement of its own (nothing above runs): ``--records`` records of 4,096
rows on either side, b-record r random but for a copy of 150 rows of a-record r at another
place, and ``--pairs`` pairs ``(r, r)``.  Every pair is aligned inside the band of 9 diagonals
around its region's diagonal, once without a box and once inside the box of the region and
``MARGIN`` rows around it (what ``Chains.bands(4)`` and ``Chains.boxes(MARGIN)`` give for such a
region), by ``local_align``, ``local_spans`` and ``local_paths``.  The document (default
profiles/align_box_bench.json) holds the medians, ``boxed_over_banded`` (their ratio), the strips
of both by the kernel's loop bounds (arithmetic, counted on the host) and how many of the boxed
alignments are the banded ones bit for bit (the region is the best alignment of its band, so
all of them should be).

``--global --box MARGIN`` and ``--within --box MARGIN`` are the fill-between-anchors measurement, on
the pairs of ``--box``: ``global_paths`` (``within=False`` / ``True``) inside the box of every
region and ``MARGIN`` rows around it, next to (a) ``global_paths`` on the two whole records, the
only way without a box (on the first ``--whole-pairs`` pairs, 4,096 x 4,096 cells each, and per
pair), and (b) ``local_paths`` banded and boxed.  The document (default
profiles/align_global_box_bench.json) holds the medians, the seconds per pair, the ratios and
the strips of each by the kernel's loop bounds (arithmetic, counted on the host).

``--values --box MARGIN`` times ``align.path_values`` next to the ``local_paths`` call, banded and
boxed, that made its paths, on the pairs of ``--box``.  The document (default
profiles/path_values_bench.json) holds the two medians, their ratio, the ops and how many of the
scores are those of ``local_paths`` bit for bit (all of them should be).  No ratio is set.

``--null K --box MARGIN`` times ``align.null_scores`` (K shuffles of every pair's b-side, one launch)
on the pairs and boxes of ``--box``, with the making of its orders and with the orders given,
next to two routes that need no such call: (a) K calls of ``local_align`` on the same boxed pairs
(the same cells, nothing shuffled) and (b) a torch gather of the shuffled rows into ``pairs x K``
records of their own plus one ``local_align`` on them, the gather timed with it and its bytes
reported.  Without ``--band`` there is no band; ``--band W`` puts W diagonals around every
region's diagonal, in all routes.  The document (default profiles/align_null_bench.json) holds
the medians, their ratios to ``null_scores``, the bytes of the orders and of the gathered rows,
and how many scores of the gathered route ``null_scores`` gives bit for bit (all of them should
be).  No ratio is set.

    python tools/bench_align.py --pairs 20000
    python tools/bench_align.py --pairs 2000 --records 64 --null 20 --box 16
    python tools/bench_align.py --pairs 2000 --records 64 --values --box 16
    python tools/bench_align.py --pairs 2000 --records 64 --box 16
    python tools/bench_align.py --pairs 2000 --records 64 --global --within --box 16
    python tools/bench_align.py --pairs 20000 --spans
    python tools/bench_align.py --pairs 20000 --band 129 --spans --paths
    python tools/bench_align.py --pairs 20000 --global --within
    python tools/bench_align.py --pairs 20000 --paths
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
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ginfinity_amd import align, distance, synthetic  # noqa: E402

KERNEL_SOURCE = "align_kernels.hip"
ALIGN_SOURCES = ("align_local.inc", "align_kernels.hip")     # every alignment kernel: the shared body and its modes
VALUE_SOURCES = ("align_values.hip", "pairwise_sweep.inc")   # --values
BOX_RECORD_ROWS = 4096            # --box: rows of every record
BOX_REGION_ROWS = 150             # --box: rows of the region a pair shares


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


def _paths_against_spans(rows, counts, pairs, keeper, parameters, repeats, warmup) -> dict:
    """``local_spans`` and ``local_paths`` on the same pairs, one after the other."""
    pairs_dev = torch.from_numpy(pairs)
    spans = _timed(lambda: align.local_spans(rows, counts_a=counts, pairs=pairs_dev,
                                             workspace=keeper, **parameters), repeats, warmup)
    paths = _timed(lambda: align.local_paths(rows, counts_a=counts, pairs=pairs_dev,
                                             workspace=keeper, **parameters), repeats, warmup)
    result = align.local_paths(rows, counts_a=counts, pairs=pairs_dev, workspace=keeper,
                               **parameters)
    box = (result.ends - result.starts + 1).cpu().numpy().astype(np.int64)
    box[result.starts.cpu().numpy()[:, 0] < 0] = 0
    span_mid, path_mid = statistics.median(spans), statistics.median(paths)
    return {"pairs": int(pairs.shape[0]),
            "cells": int((counts[pairs[:, 0]].astype(np.int64) * counts[pairs[:, 1]]).sum()),
            "box_cells": int((box[:, 0] * box[:, 1]).sum()), "ops": int(result.ops.shape[0]),
            "spans_seconds": _span(spans), "paths_seconds": _span(paths),
            "paths_over_local_spans": path_mid / span_mid,
            "timed": "local_paths whole: the span launch, starts and ends to the host, the trace "
                     "launch, the compaction"}


def _band_counts(counts, pairs, lo: int, hi: int) -> dict:
    """Cells inside the band and steps of the kernel's step loop, by its bounds: per strip of 64
    rows from i0, columns c_lo = max(0, i0 + lo) .. c_hi = min(Lr - 1, i0 + rows - 1 + hi) and
    c_hi - (c_lo & ~31) + rows steps, against Lr + rows - 1 without a band.  Arithmetic."""
    cells = steps = steps_plain = 0
    for lq, lr in zip(counts[pairs[:, 0]].tolist(), counts[pairs[:, 1]].tolist()):
        i = np.arange(lq)
        cells += int(np.maximum(np.minimum(lr - 1, i + hi) - np.maximum(0, i + lo) + 1, 0).sum())
        for i0 in range(0, lq, 64):
            rows = min(64, lq - i0)
            steps_plain += lr + rows - 1
            c_lo, c_hi = max(0, i0 + lo), min(lr - 1, i0 + rows - 1 + hi)
            if c_lo <= c_hi:
                steps += c_hi - (c_lo & ~31) + rows
    return {"band_cells": cells, "steps": steps, "steps_without_band": steps_plain,
            "counted": "on the host from the loop bounds, not measured"}


def _band_against_plain(call, plain_mid: float, pairs: int, repeats: int, warmup: int) -> dict:
    seconds = _timed(call, repeats, warmup)
    mid = statistics.median(seconds)
    return {"seconds": _span(seconds), "pairs_per_s": pairs / mid, "over_unbanded": mid / plain_mid}


def _measured_arguments() -> list[str]:
    """The command line without ``--out``: where the document goes is no part of what was measured."""
    kept, skip = [], False
    for word in sys.argv[1:]:
        if skip or word.startswith("--out="):
            skip = False
        elif word == "--out":
            skip = True
        else:
            kept.append(word)
    return kept


def _box_case(args):
    """The records, pairs, bands and boxes of ``--box``: ``(a, b, counts, pairs, bands, boxes,
    first, last)``, the rows on the device and the rest on the host."""
    rng = np.random.default_rng(0)
    rows, region, margin = BOX_RECORD_ROWS, BOX_REGION_ROWS, args.box
    counts = np.full(args.records, rows)
    a = synthetic.unit_rows(0, args.records * rows)
    b = synthetic.unit_rows(1, args.records * rows)
    at = rng.integers(0, rows - region + 1, size=(args.records, 2))     # (i, j) of every region
    for r, (i, j) in enumerate(at.tolist()):
        b[r * rows + j:r * rows + j + region] = a[r * rows + i:r * rows + i + region]
    record = rng.integers(0, args.records, size=args.pairs)
    pairs = np.stack([record, record], axis=1).astype(np.int32)
    first, last = at[record], at[record] + region - 1
    diagonal = first[:, 1] - first[:, 0]
    bands = np.stack([diagonal - 4, diagonal + 4], axis=1).astype(np.int32)
    boxes = np.stack([first[:, 0] - margin, last[:, 0] + margin, first[:, 1] - margin,
                      last[:, 1] + margin], axis=1).astype(np.int32)
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), counts, pairs, bands, boxes, \
        first, last


def _global_box_bench(args) -> dict:
    """``--global`` / ``--within`` with ``--box``: ``global_paths`` in chain-sized boxes next to
    ``global_paths`` on the whole records and ``local_paths`` banded and boxed."""
    a, b, counts, pairs, bands, boxes, first, last = _box_case(args)
    rows = BOX_RECORD_ROWS
    parameters = dict(gap_open=1.0, gap_extend=0.25, match_scale=1.0, match_shift=-0.3)
    keeper = align.AlignWorkspace()
    pairs_dev, box_dev = torch.from_numpy(pairs), torch.from_numpy(boxes)
    few = min(args.whole_pairs, args.pairs)
    common = dict(counts_a=counts, counts_b=counts, workspace=keeper, **parameters)
    box_rows = np.minimum(boxes[:, 1], rows - 1) - np.maximum(boxes[:, 0], 0) + 1
    boxed_strips = int(((box_rows + 63) // 64).sum())
    source = ROOT / "ginfinity_amd" / "csrc"
    result = {"metric": "global_paths of pairs of 4,096-row records that share a 150-row region: "
                        "inside the region's box, on the whole records, and local_paths banded and "
                        "boxed",
              "pairs": args.pairs, "records": args.records, "record_rows": rows,
              "region_rows": BOX_REGION_ROWS, "margin": args.box, "whole_pairs": few,
              "parameters": parameters, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "source_sha256": {name: hashlib.sha256((source / name).read_bytes()).hexdigest()
                                for name in ALIGN_SOURCES},
              "command": "python tools/bench_align.py " + " ".join(_measured_arguments()),
              "repeats": args.repeats, "warmup": args.warmup, "rates_use": "median",
              "timed": "the whole call: host checks, the uploads, both launches, the compaction",
              "strips_per_pair": {"boxed": boxed_strips / args.pairs, "whole_records": rows // 64,
                                  "counted": "on the host from the loop bounds, not measured"}}
    local = _timed(lambda: align.local_paths(a, b, pairs=pairs_dev, band=torch.from_numpy(bands),
                                             box=box_dev, **common), args.repeats, args.warmup)
    local_mid = statistics.median(local)
    result["local_paths_banded_and_boxed"] = {"seconds": _span(local),
                                              "seconds_per_pair": local_mid / args.pairs}
    for name, wanted, within in (("global", args.whole, False), ("within", args.within, True)):
        if not wanted:
            continue
        boxed = _timed(lambda: align.global_paths(a, b, pairs=pairs_dev, within=within,
                                                  box=box_dev, **common), args.repeats, args.warmup)
        whole = _timed(lambda: align.global_paths(a, b, pairs=pairs_dev[:few], within=within,
                                                  **common), args.repeats, args.warmup)
        boxed_mid, whole_mid = statistics.median(boxed), statistics.median(whole)
        got = align.global_paths(a, b, pairs=pairs_dev, within=within, box=box_dev, **common)
        cells_first = got.starts.cpu().numpy()
        result[name] = {"call": f"align.global_paths(within={within})",
                        "boxed_seconds": _span(boxed), "whole_records_seconds": _span(whole),
                        "boxed_seconds_per_pair": boxed_mid / args.pairs,
                        "whole_records_seconds_per_pair": whole_mid / few,
                        "boxed_over_whole_records_per_pair":
                            (boxed_mid / args.pairs) / (whole_mid / few),
                        "boxed_over_local_paths_banded_and_boxed": boxed_mid / local_mid,
                        "ops": int(got.ops.shape[0]),
                        "paths_that_start_at_their_box":
                            int((cells_first[:, 0] == np.maximum(boxes[:, 0], 0)).sum())}
        print(f"global_paths(within={within}): boxed {boxed_mid:.4f} s for {args.pairs} pairs, whole "
              f"records {whole_mid:.4f} s for {few} pairs = "
              f"{result[name]['boxed_over_whole_records_per_pair']:.5f} x per pair; local_paths "
              f"banded and boxed {local_mid:.4f} s", file=sys.stderr, flush=True)
    return result


def _values_bench(args) -> dict:
    """``--values`` with ``--box``: ``path_values`` next to the ``local_paths`` call, banded and
    boxed, that made the paths."""
    a, b, counts, pairs, bands, boxes, first, last = _box_case(args)
    parameters = dict(gap_open=1.0, gap_extend=0.25, match_scale=1.0, match_shift=-0.3)
    pairs_dev = torch.from_numpy(pairs)
    common = dict(counts_a=counts, counts_b=counts, pairs=pairs_dev, **parameters)
    keeper = align.AlignWorkspace()

    def make_paths():
        return align.local_paths(a, b, band=torch.from_numpy(bands), box=torch.from_numpy(boxes),
                                 workspace=keeper, **common)
    source = ROOT / "ginfinity_amd" / "csrc"
    made = _timed(make_paths, args.repeats, args.warmup)
    paths = make_paths()
    valued = _timed(lambda: align.path_values(paths, a, b, **common), args.repeats, args.warmup)
    values = align.path_values(paths, a, b, **common)
    made_mid, valued_mid = statistics.median(made), statistics.median(valued)
    scores, mine = paths.scores.cpu().numpy(), values.scores.cpu().numpy()
    same = (scores.view(np.uint32) == mine.view(np.uint32)) | ((scores == 0) & (mine == 0))
    ops = int(paths.ops.shape[0])
    print(f"local_paths (banded, boxed) {made_mid:.6f} s, path_values {valued_mid:.6f} s = "
          f"{valued_mid / made_mid:.4f} x for {args.pairs} paths of {ops} ops", file=sys.stderr,
          flush=True)
    return {"metric": "path_values on the paths of local_paths (banded and boxed) of pairs of "
                      "4,096-row records that share a 150-row region",
            "pairs": args.pairs, "records": args.records, "record_rows": BOX_RECORD_ROWS,
            "region_rows": BOX_REGION_ROWS, "margin": args.box, "band_diagonals": 9,
            "parameters": parameters, "host": platform.node(),
            "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
            "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
            "torch": torch.__version__, "commit": args.commit or _commit(),
            "source_sha256": {name: hashlib.sha256((source / name).read_bytes()).hexdigest()
                              for name in VALUE_SOURCES},
            "command": "python tools/bench_align.py " + " ".join(_measured_arguments()),
            "repeats": args.repeats, "warmup": args.warmup, "rates_use": "median",
            "timed": "the whole call: host checks, the uploads, the launches (local_paths: its "
                     "copy to the host and the compaction as well)",
            "local_paths_seconds": _span(made), "path_values_seconds": _span(valued),
            "path_values_over_local_paths": valued_mid / made_mid,
            "ops": ops, "ops_per_path": ops / args.pairs,
            "path_values_seconds_per_op": valued_mid / max(ops, 1),
            "matches": int(values.matches.sum()), "refused": int((values.status != 0).sum()),
            "scores_equal_to_local_paths": int(same.sum())}


def _null_bench(args) -> dict:
    """``--null K`` with ``--box``: ``null_scores`` next to K calls of ``local_align`` and next to a
    gather of the shuffled rows with one ``local_align`` on them."""
    a, b, counts, pairs, bands, boxes, first, last = _box_case(args)
    rows, shuffles = BOX_RECORD_ROWS, args.null
    if args.band:       # W diagonals around the region's diagonal; without --band no band at all
        centre = (bands[:, 0] + bands[:, 1]) // 2
        bands = np.stack([centre - args.band // 2, centre + args.band - 1 - args.band // 2], axis=1)
    parameters = dict(gap_open=1.0, gap_extend=0.25, match_scale=1.0, match_shift=-0.3)
    keeper = align.AlignWorkspace()
    pairs_dev, box_dev = torch.from_numpy(pairs), torch.from_numpy(boxes)
    band_dev = torch.from_numpy(bands.astype(np.int32)) if args.band else None
    common = dict(counts_a=counts, counts_b=counts, workspace=keeper, **parameters)
    j_lo = np.maximum(boxes[:, 2], 0).astype(np.int64)
    columns = np.minimum(boxes[:, 3], rows - 1) - j_lo + 1
    box_rows = np.minimum(boxes[:, 1], rows - 1) - np.maximum(boxes[:, 0], 0) + 1
    order, order_ptr = align.shuffle_orders(columns, shuffles, 0, "cuda")

    def null():
        return align.null_scores(a, b, pairs=pairs_dev, band=band_dev, box=box_dev,
                                 shuffles=shuffles, seed=0, **common)

    def null_given():
        return align.null_scores(a, b, pairs=pairs_dev, band=band_dev, box=box_dev,
                                 shuffles=shuffles, orders=(order, order_ptr), **common)

    def repeated():                 # (a): the same cells, the rows not shuffled
        for _ in range(shuffles):
            align.local_align(a, b, pairs=pairs_dev, band=band_dev, box=box_dev, **common)

    # (b): every shuffled b-side as a record of its own
    virtual = args.pairs * shuffles
    side_first = torch.from_numpy(np.repeat(pairs[:, 1].astype(np.int64) * rows + j_lo, shuffles))
    lengths = torch.from_numpy(np.repeat(columns, shuffles))
    many_pairs = torch.from_numpy(np.stack([np.repeat(pairs[:, 0], shuffles),
                                            np.arange(virtual)], axis=1).astype(np.int32))
    many_boxes = torch.from_numpy(np.repeat(np.stack(
        [boxes[:, 0], boxes[:, 1], np.full(args.pairs, -rows), np.full(args.pairs, rows)],
        axis=1), shuffles, axis=0).astype(np.int32))
    many_bands = None if not args.band else torch.from_numpy(
        np.repeat(bands - j_lo[:, None], shuffles, axis=0).astype(np.int32))
    many_counts = np.repeat(columns, shuffles)
    gathered_bytes = int(columns.sum()) * shuffles * 256

    def gathered():
        base = torch.repeat_interleave(side_first.cuda(), lengths.cuda(),
                                       output_size=int(order.shape[0]))
        shuffled = b[base + order]
        return align.local_align(a, shuffled, counts_a=counts, counts_b=many_counts,
                                 pairs=many_pairs, band=many_bands, box=many_boxes,
                                 workspace=keeper, **parameters)[0]

    timed = {name: _timed(call, args.repeats, args.warmup)
             for name, call in (("null_scores", null), ("null_scores_given_orders", null_given),
                                ("local_align_k_times", repeated),
                                ("gather_and_local_align", gathered))}
    mids = {name: statistics.median(seconds) for name, seconds in timed.items()}
    same = (null().reshape(-1).view(torch.int32) == gathered().view(torch.int32))
    source = ROOT / "ginfinity_amd" / "csrc"
    for name, mid in mids.items():
        print(f"{name}: {mid:.4f} s = {mid / mids['null_scores']:.3f} x null_scores",
              file=sys.stderr, flush=True)
    return {"metric": "null_scores of boxed pairs of 4,096-row records that share a 150-row region: "
                      "K shuffles of every pair's b-side in one launch, next to K calls of "
                      "local_align and next to a gather of the shuffled rows with one local_align",
            "pairs": args.pairs, "records": args.records, "record_rows": rows,
            "region_rows": BOX_REGION_ROWS, "margin": args.box, "shuffles": shuffles,
            "band_diagonals": args.band or None, "parameters": parameters,
            "host": platform.node(),
            "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
            "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
            "torch": torch.__version__, "commit": args.commit or _commit(),
            "source_sha256": {name: hashlib.sha256((source / name).read_bytes()).hexdigest()
                              for name in ALIGN_SOURCES},
            "command": "python tools/bench_align.py " + " ".join(_measured_arguments()),
            "repeats": args.repeats, "warmup": args.warmup, "rates_use": "median",
            "timed": "the whole call: host checks, the uploads, the launches; null_scores with the "
                     "making of its orders, gather_and_local_align with the gather",
            "virtual_pairs": virtual, "cells": int((box_rows * columns).sum()) * shuffles,
            "order_bytes": int(order.shape[0]) * 4, "gathered_bytes": gathered_bytes,
            "seconds": {name: _span(seconds) for name, seconds in timed.items()},
            "over_null_scores": {name: mid / mids["null_scores"] for name, mid in mids.items()},
            "scores_equal_to_the_gathered_route": int(same.sum())}


def _box_bench(args) -> dict:
    """``--box``: the same pairs banded, without and with the box of the planted region."""
    a, b, counts, pairs, bands, boxes, first, last = _box_case(args)
    rows, region, margin = BOX_RECORD_ROWS, BOX_REGION_ROWS, args.box
    pairs = torch.from_numpy(pairs)
    parameters = dict(gap_open=1.0, gap_extend=0.25, match_scale=1.0, match_shift=-0.3)
    keeper = align.AlignWorkspace()
    common = dict(counts_a=counts, counts_b=counts, pairs=pairs, band=torch.from_numpy(bands),
                  workspace=keeper, **parameters)
    box_dev = torch.from_numpy(boxes)
    # strips by the loop bounds: a band of 9 diagonals meets every strip of the a-record whose
    # rows have a column, a box has ceil(its rows inside the record / 64)
    i0 = np.arange(0, rows, 64)[None, :]
    banded_strips = int(((np.maximum(i0 + bands[:, :1], 0) <=
                          np.minimum(i0 + 63 + bands[:, 1:], rows - 1))).sum())
    box_rows = np.minimum(boxes[:, 1], rows - 1) - np.maximum(boxes[:, 0], 0) + 1
    boxed_strips = int(((box_rows + 63) // 64).sum())
    source = ROOT / "ginfinity_amd" / "csrc"
    result = {"metric": "local alignment of pairs of 4,096-row records that share a 150-row region, "
                        "inside a band of 9 diagonals, without and with the region's box",
              "pairs": args.pairs, "records": args.records, "record_rows": rows,
              "region_rows": region, "margin": margin, "band_diagonals": 9,
              "parameters": parameters, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "source_sha256": {name: hashlib.sha256((source / name).read_bytes()).hexdigest()
                                for name in ALIGN_SOURCES},
              "command": "python tools/bench_align.py " + " ".join(_measured_arguments()),
              "repeats": args.repeats, "warmup": args.warmup, "rates_use": "median",
              "timed": "the whole call: host checks, the upload of pairs, bands and boxes, the "
                       "launches",
              "strips": {"banded": banded_strips, "boxed": boxed_strips,
                         "counted": "on the host from the loop bounds, not measured"}}
    for name in ("local_align", "local_spans", "local_paths"):
        function = getattr(align, name)
        banded = _timed(lambda: function(a, b, **common), args.repeats, args.warmup)
        boxed = _timed(lambda: function(a, b, box=box_dev, **common), args.repeats, args.warmup)
        banded_mid, boxed_mid = statistics.median(banded), statistics.median(boxed)
        result[name] = {"banded_seconds": _span(banded), "boxed_seconds": _span(boxed),
                        "banded_pairs_per_s": args.pairs / banded_mid,
                        "boxed_pairs_per_s": args.pairs / boxed_mid,
                        "boxed_over_banded": boxed_mid / banded_mid}
        print(f"{name}: banded {banded_mid:.4f} s, boxed {boxed_mid:.4f} s = "
              f"{boxed_mid / banded_mid:.3f} x; strips {boxed_strips} of {banded_strips} (counted)",
              file=sys.stderr, flush=True)
    one = align.local_spans(a, b, **common)
    two = align.local_spans(a, b, box=box_dev, **common)
    same = torch.stack([(x.reshape(args.pairs, -1) == y.reshape(args.pairs, -1)).all(dim=1)
                        for x, y in zip(one, two)]).all(dim=0)
    result["boxed_equal_to_banded"] = int(same.sum())
    result["region_inside_the_alignment"] = int(
        ((two[1].cpu().numpy() <= first) & (two[2].cpu().numpy() >= last)).all(axis=1).sum())
    return result


def _host_gotoh(S: np.ndarray, go: np.float32, ge: np.float32) -> np.float32:
    """max H of the recurrences in numpy float32, one anti-diagonal at a time."""
    lq, lr = S.shape
    H = np.zeros((lq + 1, lr + 1), dtype=np.float32)
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=np.float32)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=np.float32)
    for d in range(lq + lr - 1):
        i = np.arange(max(0, d - lr + 1), min(lq - 1, d) + 1) + 1
        j = d + 2 - i
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(np.maximum(np.float32(0), H[i - 1, j - 1] + S[i - 1, j - 1]),
                             np.maximum(e, f))
    return H.max()


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=20_000)
    parser.add_argument("--records", type=int, default=2_000, help="records in the library")
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--host-pairs", type=int, default=4,
                        help="pairs of the host numpy DP timed for scale (0: none)")
    parser.add_argument("--spans", action="store_true",
                        help="time align.local_spans as well, after local_align")
    parser.add_argument("--paths", action="store_true",
                        help="time align.local_paths next to align.local_spans, on the pairs and "
                             "on every record with itself")
    parser.add_argument("--global", dest="whole", action="store_true",
                        help="time align.global_align (global alignment) after local_align")
    parser.add_argument("--within", action="store_true",
                        help="time align.global_align(within=True) (query-in-target) after "
                             "local_align")
    parser.add_argument("--band", type=int, default=0, metavar="W",
                        help="time the same pairs inside a band of W diagonals around diagonal 0 "
                             "next to the calls without a band (with --spans and --paths: those "
                             "calls too)")
    parser.add_argument("--box", type=int, default=None, metavar="MARGIN",
                        help="a measurement of its own: pairs of 4,096-row records that share a "
                             "150-row region, banded, without and with the region's box of MARGIN "
                             "rows around it (default output profiles/align_box_bench.json)")
    parser.add_argument("--values", action="store_true",
                        help="with --box: time align.path_values next to the local_paths call, "
                             "banded and boxed, that made its paths (default output "
                             "profiles/path_values_bench.json)")
    parser.add_argument("--null", type=int, default=0, metavar="K",
                        help="with --box (and, if wanted, --band W): time align.null_scores with K "
                             "shuffles next to K calls of local_align and next to a gather of the "
                             "shuffled rows plus one local_align (default output "
                             "profiles/align_null_bench.json)")
    parser.add_argument("--whole-pairs", type=int, default=64,
                        help="with --global / --within and --box: the pairs on which global_paths "
                             "on the two whole records is timed")
    parser.add_argument("--commit", default=None, help="the commit measured, where git cannot say")
    parser.add_argument("--out", default=None,
                        help="default profiles/align_bench.json, with --box "
                             "profiles/align_box_bench.json")
    args = parser.parse_args()
    if args.pairs < 1 or args.records < 1:
        parser.error("--pairs, --records: positive")
    if args.band < 0:
        parser.error("--band: a positive number of diagonals")
    if args.box is not None and args.box < 0:
        parser.error("--box: a margin of 0 rows or more")
    if args.whole_pairs < 1:
        parser.error("--whole-pairs: positive")
    if args.values and (args.box is None or args.whole or args.within):
        parser.error("--values: with --box MARGIN, and without --global and --within")
    if args.null < 0 or (args.null and (args.box is None or args.values or args.whole
                                        or args.within)):
        parser.error("--null K: K positive, with --box MARGIN, and without --values, --global and "
                     "--within")
    fill = args.box is not None and (args.whole or args.within)
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("align_bench.json" if args.box is None
                                            else "align_null_bench.json" if args.null
                                            else "path_values_bench.json" if args.values
                                            else "align_global_box_bench.json" if fill
                                            else "align_box_bench.json"))
    if args.box is not None:
        result = _null_bench(args) if args.null else _values_bench(args) if args.values \
            else _global_box_bench(args) if fill else _box_bench(args)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result))
        return
    rng = np.random.default_rng(0)
    counts = rng.integers(200, 601, size=args.records)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    rows = torch.from_numpy(synthetic.unit_rows(0, int(ptr[-1]))).cuda()
    pairs = rng.integers(0, args.records, size=(args.pairs, 2)).astype(np.int32)
    cells = int((counts[pairs[:, 0]].astype(np.int64) * counts[pairs[:, 1]]).sum())
    parameters = dict(gap_open=1.0, gap_extend=0.25, match_scale=1.0, match_shift=-0.3)
    keeper = align.AlignWorkspace()
    pairs_dev = torch.from_numpy(pairs)
    seconds = _timed(lambda: align.local_align(rows, counts_a=counts, pairs=pairs_dev,
                                               workspace=keeper, **parameters),
                     args.repeats, args.warmup)
    mid = statistics.median(seconds)
    source = ROOT / "ginfinity_amd" / "csrc" / KERNEL_SOURCE
    result = {"metric": "local_align over pairs of 200- to 600-row records of 128-d fp16 embeddings",
              "pairs": args.pairs, "records": args.records, "rows": int(ptr[-1]), "cells": cells,
              "parameters": parameters, "host": platform.node(),
              "utc": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
              "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "torch": torch.__version__, "commit": args.commit or _commit(),
              "kernel_source": KERNEL_SOURCE,
              "kernel_source_sha256": hashlib.sha256(source.read_bytes()).hexdigest(),
              "command": "python tools/bench_align.py " + " ".join(sys.argv[1:]),
              "repeats": args.repeats, "warmup": args.warmup, "rates_use": "median",
              "timed": "the whole call: host checks of the pair list, its upload, one launch",
              "seconds": _span(seconds), "pairs_per_s": args.pairs / mid,
              "cell_updates_per_s": cells / mid}
    print(f"local_align: {mid:.4f} s for {args.pairs} pairs = {args.pairs / mid:.3e} pairs/s, "
          f"{cells / mid:.3e} cell updates/s", file=sys.stderr, flush=True)
    if args.spans:
        span_seconds = _timed(lambda: align.local_spans(rows, counts_a=counts, pairs=pairs_dev,
                                                        workspace=keeper, **parameters),
                              args.repeats, args.warmup)
        span_mid = statistics.median(span_seconds)
        result["spans_seconds"] = _span(span_seconds)
        result["spans_cell_updates_per_s"] = cells / span_mid
        result["spans_over_local_align"] = span_mid / mid
        result["spans_source_sha256"] = {
            name: hashlib.sha256((source.parent / name).read_bytes()).hexdigest()
            for name in ALIGN_SOURCES}
        print(f"local_spans: {span_mid:.4f} s = {cells / span_mid:.3e} cell updates/s, "
              f"{span_mid / mid:.3f} x local_align", file=sys.stderr, flush=True)
    for name, wanted, within in (("global", args.whole, False), ("within", args.within, True)):
        if not wanted:
            continue
        mode_seconds = _timed(lambda: align.global_align(rows, counts_a=counts, pairs=pairs_dev,
                                                         within=within, workspace=keeper,
                                                         **parameters), args.repeats, args.warmup)
        mode_mid = statistics.median(mode_seconds)
        result[name] = {"call": f"align.global_align(within={within})",
                        "seconds": _span(mode_seconds), "pairs_per_s": args.pairs / mode_mid,
                        "cell_updates_per_s": cells / mode_mid,
                        "over_local_align": mode_mid / mid}
        result["global_source_sha256"] = {
            source_name: hashlib.sha256((source.parent / source_name).read_bytes()).hexdigest()
            for source_name in ALIGN_SOURCES}
        print(f"global_align(within={within}): {mode_mid:.4f} s = {args.pairs / mode_mid:.3e} "
              f"pairs/s, {cells / mode_mid:.3e} cell updates/s, {mode_mid / mid:.3f} x local_align",
              file=sys.stderr, flush=True)
    if args.paths:
        result["paths"] = _paths_against_spans(rows, counts, pairs, keeper, parameters,
                                               args.repeats, args.warmup)
        own = np.repeat(np.arange(args.records, dtype=np.int32)[:, None], 2, axis=1)
        result["paths_self"] = _paths_against_spans(rows, counts, own, keeper, parameters,
                                                    args.repeats, args.warmup)
        result["paths_source_sha256"] = {
            name: hashlib.sha256((source.parent / name).read_bytes()).hexdigest()
            for name in ALIGN_SOURCES}
        for name in ("paths", "paths_self"):
            part = result[name]
            print(f"{name}: local_spans {part['spans_seconds']['median']:.4f} s, local_paths "
                  f"{part['paths_seconds']['median']:.4f} s = {part['paths_over_local_spans']:.3f} x, "
                  f"{part['ops']} ops, {part['box_cells']} box cells of {part['cells']}",
                  file=sys.stderr, flush=True)
    if args.band:
        band = (-(args.band // 2), args.band - 1 - args.band // 2)
        part = {"diagonals": args.band, "band": list(band),
                **_band_counts(counts, pairs, *band),
                "local_align": _band_against_plain(
                    lambda: align.local_align(rows, counts_a=counts, pairs=pairs_dev, band=band,
                                              workspace=keeper, **parameters),
                    mid, args.pairs, args.repeats, args.warmup)}
        if args.spans:
            part["local_spans"] = _band_against_plain(
                lambda: align.local_spans(rows, counts_a=counts, pairs=pairs_dev, band=band,
                                          workspace=keeper, **parameters),
                statistics.median(result["spans_seconds"]["runs"]), args.pairs, args.repeats,
                args.warmup)
        if args.paths:
            for name, which in (("paths", pairs), ("paths_self", own)):
                which_dev = torch.from_numpy(which)
                part["local_" + name] = _band_against_plain(
                    lambda: align.local_paths(rows, counts_a=counts, pairs=which_dev, band=band,
                                              workspace=keeper, **parameters),
                    result[name]["paths_seconds"]["median"], int(which.shape[0]), args.repeats,
                    args.warmup)
        part["source_sha256"] = {
            name: hashlib.sha256((source.parent / name).read_bytes()).hexdigest()
            for name in ALIGN_SOURCES}
        result["band"] = part
        for name, timed in part.items():
            if isinstance(timed, dict) and "over_unbanded" in timed:
                print(f"band of {args.band} diagonals, {name}: {timed['seconds']['median']:.4f} s = "
                      f"{timed['over_unbanded']:.3f} x the call without a band; steps "
                      f"{part['steps']} of {part['steps_without_band']} (counted)",
                      file=sys.stderr, flush=True)
    if args.host_pairs > 0:
        some = pairs[:args.host_pairs]
        host_seconds, host_cells = 0.0, 0
        for q, r in some:
            C = distance.pairwise(rows[ptr[q]:ptr[q + 1]], rows[ptr[r]:ptr[r + 1]],
                                  metric="cosine").cpu().numpy()
            S = (C * np.float32(parameters["match_scale"])) + np.float32(parameters["match_shift"])
            start = time.perf_counter()
            _host_gotoh(S, np.float32(parameters["gap_open"]), np.float32(parameters["gap_extend"]))
            host_seconds += time.perf_counter() - start
            host_cells += S.size
        result["host_numpy_dp"] = {"pairs": int(len(some)), "cells": host_cells,
                                   "seconds": host_seconds,
                                   "cell_updates_per_s": host_cells / host_seconds,
                                   "what": "numpy float32 anti-diagonal DP on one host thread, the "
                                           "cosines given: for scale, not a competitor"}
    text = json.dumps(result, indent=1)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
