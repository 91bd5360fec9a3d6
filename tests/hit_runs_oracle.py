"""The definition of ``align.hit_runs`` in plain numpy / Python, for test_hit_runs_host.py and
test_gpu_hit_runs.py.  A set of cells per call and the definition word for word; nothing here is
the code under test."""
from __future__ import annotations

import numpy as np


def hits_of(matrix, values=None, seed: int = 0):
    """``(offsets, indices, values)`` as ``distance.within`` lays hits out, for the true cells of
    a boolean matrix (``np.nonzero``: rows ascending, then columns ascending).  Without
    ``values``: random float32 over many orders of magnitude and both signs, so that the order of
    a float64 sum shows in its bits."""
    matrix = np.asarray(matrix, dtype=bool)
    rows, cols = np.nonzero(matrix)
    offsets = np.concatenate(([0], np.cumsum(matrix.sum(axis=1)))).astype(np.int64)
    if values is None:
        rng = np.random.default_rng(seed)
        values = (rng.standard_normal(rows.size) * 10.0 ** rng.integers(-12, 13, rows.size))
    return offsets, cols.astype(np.int32), np.asarray(values, dtype=np.float32)


def record_of(row: int, ptr) -> int:
    """The record of a row: a row at a boundary belongs to the record that starts there, a record
    of zero rows owns nothing."""
    for record in range(len(ptr) - 1):
        if ptr[record] <= row < ptr[record + 1]:
            return record
    raise AssertionError(f"row {row} lies in no record")


def runs(offsets, indices, values, counts_a, counts_b=None, min_length: int = 1):
    """``(pairs int32 [S, 2], cells int32 [S, 2], lengths int32 [S], weights float32 [S])`` by
    the definition."""
    counts_b = counts_a if counts_b is None else counts_b
    ptr_a = np.concatenate(([0], np.cumsum(np.asarray(counts_a, dtype=np.int64))))
    ptr_b = np.concatenate(([0], np.cumsum(np.asarray(counts_b, dtype=np.int64))))
    n = len(offsets) - 1
    assert ptr_a[-1] == n
    where = {}                                       # the cell of every hit -> its position
    for i in range(n):
        for h in range(int(offsets[i]), int(offsets[i + 1])):
            where[(i, int(indices[h]))] = h
    pairs, cells, lengths, weights = [], [], [], []
    for (i, j), h in where.items():                  # insertion order: i ascending, j ascending
        q, r = record_of(i, ptr_a), record_of(j, ptr_b)
        if (i - 1, j - 1) in where and i - 1 >= ptr_a[q] and j - 1 >= ptr_b[r]:
            continue                                 # it has a predecessor: no head
        length, total = 0, np.float64(0.0)
        while (i + length, j + length) in where and i + length < ptr_a[q + 1] \
                and j + length < ptr_b[r + 1]:
            value = np.float64(values[where[(i + length, j + length)]])
            total = value if length == 0 else total + value
            length += 1
        if length >= min_length:
            pairs.append((q, r))
            cells.append((i - ptr_a[q], j - ptr_b[r]))
            lengths.append(length)
            weights.append(np.float32(total))
    return (np.asarray(pairs, dtype=np.int32).reshape(-1, 2),
            np.asarray(cells, dtype=np.int32).reshape(-1, 2),
            np.asarray(lengths, dtype=np.int32), np.asarray(weights, dtype=np.float32))


def assert_same(got, want) -> None:
    """Exact: integer arrays ``==``, weights as bytes."""
    names = ("pairs", "cells", "lengths", "weights")
    got = [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in got]
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
    for name, g, w in zip(names[:3], got, want):
        assert np.array_equal(g, w), name
    assert got[3].tobytes() == want[3].tobytes(), "weights"
