"""Windowed records end to end: ``encode_many`` on 100-nt windows at stride 50 over the 300
longest records of tests/golden/rouskin_sample_6k.tsv (2,601 windows), numpy out, warm.

Two roads on the same box in the same process, alternating: "device" is ``encode_many`` (the
windows are built by gfy_window_select / gfy_window_emit), "host" is what ``encode_many`` did
before the device window builder existed — ``GraphBuilder.build_shard`` on the host, then
``encode_graphs``.  Three option rows; for the device road also the split into select + count,
the copy of the counts to the host, emit, and encode (each a host clock around work that ends
in a device synchronise).  Prints one JSON document.

    python tools/bench_windows.py [--repeats 7] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ginfinity_amd import RNA, Ginfinity, GraphBuilder, read_rna_table  # noqa: E402

ROWS = ((False, 1), (True, 1), (True, 3))
WINDOW, STRIDE, MOLECULES = 100, 50, 300


def window_list() -> list[RNA]:
    whole = read_rna_table(ROOT / "tests" / "golden" / "rouskin_sample_6k.tsv")
    longest = sorted(whole, key=lambda r: (-r.length, r.identifier))[:MOLECULES]
    out = []
    for record in longest:
        # every stride until the window reaches the 3' end (the last one may be shorter)
        for start in range(0, max(record.length - WINDOW, 0) + STRIDE, STRIDE):
            end = min(start + WINDOW, record.length)
            out.append(RNA(f"{record.identifier}:{start}-{end}", record.sequence,
                           record.structure, start, end))
    return out


def _summary(samples: list[float]) -> dict:
    return {"median_ms": round(statistics.median(samples) * 1e3, 3),
            "min_ms": round(min(samples) * 1e3, 3), "max_ms": round(max(samples) * 1e3, 3),
            "runs": len(samples)}


def main() -> None:
    import torch
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows.py measures on the GPU; no HIP device here")
    encoder = Ginfinity.load("cuda:0", allow_nondeterministic_cuda=True)
    engine = encoder._engine
    records = window_list()
    report = {"windows": len(records), "molecules": MOLECULES,
              "molecule_nt": sum(len(sequence) for sequence, _structure in
                                 {(r.sequence, r.structure) for r in records}), "rows": []}

    def sync() -> None:
        torch.cuda.synchronize()

    for keep, hops in ROWS:
        options = dict(keep_paired_neighbours=keep, context_hops=hops)

        def device_road():
            return encoder.encode_many(records, **options)

        def host_road():
            shard = GraphBuilder(encoder.graph_spec, **options).build_shard(records)
            return encoder.encode_graphs(shard)

        def host_build_only():
            return GraphBuilder(encoder.graph_spec, **options).build_shard(records)

        for _ in range(args.warmup):
            a, b = device_road(), host_road()
        same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)
        timings = {"device": [], "host": [], "host_build": []}
        for _ in range(args.repeats):                       # alternating
            for name, road in (("device", device_road), ("host", host_road),
                               ("host_build", host_build_only)):
                sync()
                t0 = time.perf_counter()
                road()
                sync()
                timings[name].append(time.perf_counter() - t0)

        # the split of the device road
        split = {"text_and_upload": [], "select_count": [], "counts_to_host": [], "emit": [],
                 "encode_and_download": []}
        spec = encoder.graph_spec
        from ginfinity_amd.graph import window_text
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            text = window_text(records, spec)
            tensors = encoder._uploader((text.bases, text.marks, text.mol_ptr, text.molecule,
                                         text.start, text.end, text.positional()))
            sync()
            t1 = time.perf_counter()
            windows = engine.window_select(*tensors[:6], skip2=spec.has_skip2, **options)
            sync()
            t2 = time.perf_counter()
            counts = windows.counts.cpu().numpy()
            t3 = time.perf_counter()
            node_ptr = np.concatenate(([0], np.cumsum(counts[:, 0]))).astype(np.int64)
            edge_ptr = np.concatenate(([0], np.cumsum(counts[:, 1]))).astype(np.int64)
            core_ptr = np.concatenate(([0], np.cumsum(text.core_counts))).astype(np.int64)
            pointers = encoder._uploader((node_ptr, edge_ptr, core_ptr))
            sync()
            t4 = time.perf_counter()
            engine.window_emit(windows, 0, *pointers, tensors[6], int(node_ptr[-1]),
                               int(edge_ptr[-1]), int(core_ptr[-1]),
                               struct_states=1 if spec.struct_feature == "A" else 3)
            sync()
            t5 = time.perf_counter()
            split["text_and_upload"].append(t1 - t0)
            split["select_count"].append(t2 - t1)
            split["counts_to_host"].append(t3 - t2)
            split["emit"].append(t5 - t4)
        whole = statistics.median(timings["device"])
        rest = whole - sum(statistics.median(split[k]) for k in
                           ("text_and_upload", "select_count", "counts_to_host", "emit"))
        nodes = int(node_ptr[-1])
        report["rows"].append({
            "keep_paired_neighbours": keep, "context_hops": hops, "nodes": nodes,
            "edges": int(edge_ptr[-1]), "outputs_identical": bool(same),
            "device_road": _summary(timings["device"]), "host_road": _summary(timings["host"]),
            "host_build_alone": _summary(timings["host_build"]),
            "speedup_median": round(statistics.median(timings["host"]) / whole, 2),
            "device_nodes_per_s": round(nodes / whole),
            "split_ms": {**{k: _summary(v)["median_ms"] for k, v in split.items() if v},
                         "encode_and_download_by_difference": round(rest * 1e3, 3)}})
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
