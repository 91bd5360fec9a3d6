"""Oracle of the values along an aligned path (align.path_values, gfy_align_path_values; the
definition is in include/gfy.h) — a checker, never the code under test.

    values_of(C, ops, start, scale, shift, go, ge)
        (cosines float32 [len], running float32 [len], score float32, counts (matches, runs of op
        1, runs of op 2), cosine_sum float64) of one path on a float32 cosine matrix ``C`` of the
        pair's two records

Every step is an explicit sequential operation in the type the definition names: the running
score is a loop of single float32 additions and subtractions, the sum of the matched cosines a
``np.cumsum`` in float64 (which adds one element at a time, in order; ``np.sum`` adds pairwise
and is not used).  The substitution scores are ``align_oracle.substitution_f32``'s, and the last
running value is ``align_path_oracle.rescore``'s (tests/test_path_values_host.py)."""
from __future__ import annotations

import numpy as np

import align_oracle as O


def values_of(C: np.ndarray, ops, start, match_scale, match_shift, gap_open, gap_extend):
    assert C.dtype == np.float32 and C.ndim == 2
    ops = np.asarray(ops, dtype=np.uint8)
    S = O.substitution_f32(np.ascontiguousarray(C), match_scale, match_shift)
    go, ge = np.float32(gap_open), np.float32(gap_extend)
    cosines = np.full(ops.size, np.nan, dtype=np.float32)
    running = np.zeros(ops.size, dtype=np.float32)
    h, i, j, before = np.float32(0), int(start[0]), int(start[1]), 0
    matches, runs = 0, {1: 0, 2: 0}
    for x, op in enumerate(ops.tolist()):
        assert op in (0, 1, 2)
        if op == 0:
            assert 0 <= i < C.shape[0] and 0 <= j < C.shape[1], "the path leaves the records"
            cosines[x] = C[i, j]
            h = np.float32(h + S[i, j])
            matches += 1
            i, j = i + 1, j + 1
        else:
            h = np.float32(h - (ge if op == before else go))
            runs[op] += op != before
            i, j = (i, j + 1) if op == 1 else (i + 1, j)
        before = op
        running[x] = h
    assert i <= C.shape[0] and j <= C.shape[1], "the path leaves the records"
    # from 0, as the definition says: 0 + (-0) is +0, where a cumsum of the cosines alone would
    # start from the first of them and keep its sign
    cosine_sum = np.cumsum(np.concatenate(([0.0], cosines[ops == 0].astype(np.float64))))[-1]
    return cosines, running, np.float32(h), (matches, runs[1], runs[2]), cosine_sum
