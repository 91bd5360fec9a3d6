"""Record tests/golden/windows.json from the GENUINE reference builder.

Run only where the reference is mounted read-only (never copied into this repository, never
shipped to the GPU box):

    python tests/golden/make_windows_golden.py

It imports ``ginfinity`` from /root/reference/src and lets the reference's
``GraphBuilder(...).build_shard`` build the seeded list of windows of tests/window_cases.py
over ``rouskin_sample_6k.tsv`` for every (keep_paired_neighbours, context_hops) pair of
``OPTION_PAIRS``.  Stored: SHA-256, shape and dtype of the seven shard arrays, the node and edge
totals.  Hashes and counts only.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, "/root/reference/src")
sys.path.insert(0, str(HERE.parent))

import ginfinity as ref                                       # noqa: E402  (the reference)
from window_cases import (GOLDEN_SEED, GOLDEN_WINDOWS, OPTION_PAIRS,   # noqa: E402
                          seeded_windows, shard_digest)


def main() -> None:
    whole = ref.read_rna_table(HERE / "rouskin_sample_6k.tsv")
    windows = seeded_windows(
        whole, lambda name, seq, struct, start, end: ref.RNA(name, seq, struct, start=start,
                                                             end=end))
    fixture = {"seed": GOLDEN_SEED, "windows": GOLDEN_WINDOWS, "options": {}}
    for keep, hops in OPTION_PAIRS:
        shard = ref.GraphBuilder(keep_paired_neighbours=keep,
                                 context_hops=hops).build_shard(windows)
        fixture["options"][f"keep={int(keep)},hops={hops}"] = {
            "nodes": int(shard.node_ptr[-1]), "edges": int(shard.edge_ptr[-1]),
            "arrays": shard_digest(shard)}
    (HERE / "windows.json").write_text(json.dumps(fixture, indent=1) + "\n")
    print({key: (value["nodes"], value["edges"]) for key, value in fixture["options"].items()})


if __name__ == "__main__":
    main()
