"""The definition of ``align.chain_runs`` in plain Python, for test_chain_runs_host.py and
test_gpu_chain_runs.py: O(S^2) per record pair, the definition word for word; nothing here is the
code under test."""
from __future__ import annotations

import numpy as np

NAMES = ("pairs", "starts", "ends", "diagonals", "counts", "lengths", "weights", "members")


def links(s, t, max_gap: int, max_shift: int):
    """``|d_t - d_s|`` if the run s = (q, r, i, j, L) may precede the run t, else None."""
    if s[:2] != t[:2]:
        return None
    gi, gj = t[2] - (s[2] + s[4]), t[3] - (s[3] + s[4])
    if gi < 0 or gj < 0 or max(gi, gj) > max_gap or abs(gj - gi) > max_shift:
        return None
    return abs(gj - gi)


def chains(pairs, cells, lengths, weights, max_gap: int, max_shift=None):
    """The eight arrays of ``align.Chains`` by the definition."""
    max_shift = max_gap if max_shift is None else max_shift
    count = len(lengths)
    run = [(*map(int, pairs[s]), *map(int, cells[s]), int(lengths[s])) for s in range(count)]
    of_pair = {}
    for s in range(count):
        of_pair.setdefault(run[s][:2], []).append(s)
    pred, succ = [-1] * count, [-1] * count
    forward, backward = [0] * count, [0] * count
    # a link never leaves a record pair, and s -> t implies s < t in Runs order (the key ascends,
    # i_t >= i_s + L_s > i_s), so only those are tried: test_chain_runs_host.py tries the others
    for group in of_pair.values():
        for at, t in enumerate(group):               # C: ascending, so that every C[s] is there
            best = None
            for s in group[:at]:
                shift = links(run[s], run[t], max_gap, max_shift)
                if shift is not None:
                    best = max(best or (0, 0, -1), (forward[s], -shift, s))
            forward[t] = run[t][4] + (best[0] if best else 0)
            pred[t] = best[2] if best else -1
        for at in range(len(group) - 1, -1, -1):     # D: descending
            best, s = None, group[at]
            for t in group[at + 1:]:
                shift = links(run[s], run[t], max_gap, max_shift)
                if shift is not None:
                    best = max(best or (0, 0, -count), (backward[t], -shift, -t))
            backward[s] = run[s][4] + (best[0] if best else 0)
            succ[s] = -best[2] if best else -1
    kept = [succ[s] if succ[s] >= 0 and pred[succ[s]] == s else -1 for s in range(count)]
    has_before = [False] * count
    for s in range(count):
        if kept[s] >= 0:
            assert not has_before[kept[s]]
            has_before[kept[s]] = True
    out = {name: [] for name in NAMES[:7]}
    members = [-1] * count
    for head in range(count):                        # chains in the order of their first runs
        if has_before[head]:
            continue
        chain, s = len(out["pairs"]), head
        total, hits, number, diagonals = None, 0, 0, []
        while s >= 0:
            members[s] = chain
            weight = np.float64(weights[s])
            total = weight if total is None else total + weight
            hits += run[s][4]
            number += 1
            diagonals.append(run[s][3] - run[s][2])
            last, s = s, kept[s]
        out["pairs"].append(run[head][:2])
        out["starts"].append(run[head][2:4])
        out["ends"].append((run[last][2] + run[last][4] - 1, run[last][3] + run[last][4] - 1))
        out["diagonals"].append((min(diagonals), max(diagonals)))
        out["counts"].append(number)
        out["lengths"].append(hits)
        out["weights"].append(np.float32(total))
    assert -1 not in members
    return (*(np.asarray(out[name], dtype=np.int32).reshape(-1, 2) for name in NAMES[:4]),
            np.asarray(out["counts"], dtype=np.int32), np.asarray(out["lengths"], dtype=np.int32),
            np.asarray(out["weights"], dtype=np.float32), np.asarray(members, dtype=np.int32))


def assert_same(got, want) -> None:
    """Exact: integer arrays ``==``, weights as bytes."""
    got = [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in got]
    assert len(got) == len(want) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        if name == "weights":
            assert g.tobytes() == w.tobytes(), name
        else:
            assert np.array_equal(g, w), name


def assert_invariants(result, runs) -> None:
    """What holds whatever the two integers: every run in one chain, every hit counted once."""
    result = [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in result]
    counts, lengths, members = result[4], result[5], result[7]
    run_lengths = np.asarray(runs[2].cpu()) if hasattr(runs[2], "cpu") else np.asarray(runs[2])
    assert counts.sum() == run_lengths.size == members.size
    assert lengths.astype(np.int64).sum() == run_lengths.astype(np.int64).sum()
    assert np.array_equal(np.bincount(members, minlength=counts.size), counts)
