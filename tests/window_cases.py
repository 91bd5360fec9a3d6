"""Lists of windowed records shared by the window tests and the recorder of
tests/golden/windows.json (tests/golden/make_windows_golden.py): everything is rebuilt from a
seed, nothing is stored but hashes."""
from __future__ import annotations

import numpy as np

#: (keep_paired_neighbours, context_hops) pairs recorded from the reference
OPTION_PAIRS = ((False, 1), (True, 1), (True, 2), (True, 4))
GOLDEN_SEED, GOLDEN_WINDOWS = 20261016, 450
SHARD_ARRAYS = ("node_features", "edge_index", "edge_types", "node_ptr", "edge_ptr",
                "residue_index", "node_roles")


def seeded_windows(records, make, *, seed=GOLDEN_SEED, count=GOLDEN_WINDOWS):
    """``count`` windows over ``records`` (whole-molecule records of the TSV sample):
    ``make(identifier, sequence, structure, start, end)`` builds each record, so that the
    recorder can hand in the reference's RNA type and the tests this repository's."""
    rng = np.random.default_rng(seed)
    out = []
    for index in range(count):
        record = records[int(rng.integers(len(records)))]
        length = len(record.sequence)
        start = int(rng.integers(0, length))
        end = int(rng.integers(start + 1, min(length, start + 1 + int(rng.integers(1, 300))) + 1))
        out.append(make(f"w{index}:{record.identifier}", record.sequence, record.structure,
                        start, end))
    return out


def shard_digest(shard) -> dict:
    """SHA-256, shape and dtype of the seven arrays of a shard."""
    import hashlib
    out = {}
    for name in SHARD_ARRAYS:
        array = np.ascontiguousarray(getattr(shard, name))
        out[name] = {"sha256": hashlib.sha256(array.tobytes()).hexdigest(),
                     "shape": list(array.shape), "dtype": str(array.dtype)}
    return out
