"""Oracle of the aligned path of the local aligner (align.local_paths, gfy_align_trace; the walk
is in include/gfy.h) — a checker, never the code under test.

    gotoh_matrices(S, go, ge, dtype)  H, E and F of the definition, index + 1 (row and column 0
                                      are outside the matrix)
    walk(S, H, E, F, go, ge, end)     the ops of the walk back from ``end``, in forward order
    path_of(S, go, ge)                (score, start, end, ops) of a float32 substitution matrix:
                                      what the device must give bit for bit
    box_path(S, go, ge)               the walk from the LAST cell of S (what gfy_align_trace gives
                                      for a box that is all of S); no ops where H there is not > 0
    rescore(S, ops, start, go, ge)    the float32 score the ops add up to

The dynamic program is ``align_span_oracle.gotoh_origins``' arithmetic, operation by operation
in the same order along anti-diagonals, so H is that function's H bit for bit; the walk compares
values that the program stored and rounds nothing."""
from __future__ import annotations

import numpy as np

import align_oracle as O


def gotoh_matrices(S: np.ndarray, gap_open, gap_extend, dtype):
    """``(H, E, F)``, each ``[Lq + 1, Lr + 1]``; S must already be of ``dtype``."""
    assert S.dtype == dtype and S.ndim == 2
    lq, lr = S.shape
    go, ge = dtype(gap_open), dtype(gap_extend)
    H = np.zeros((lq + 1, lr + 1), dtype=dtype)
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    zero = dtype(0)
    for d in range(lq + lr - 1):
        i = np.arange(max(0, d - lr + 1), min(lq - 1, d) + 1) + 1
        j = d + 2 - i
        e_ext, e_open = E[i, j - 1] - ge, H[i, j - 1] - go
        f_ext, f_open = F[i - 1, j] - ge, H[i - 1, j] - go
        match = H[i - 1, j - 1] + S[i - 1, j - 1]
        e = np.maximum(e_ext, e_open)
        f = np.maximum(f_ext, f_open)
        h = np.maximum(np.maximum(zero, match), np.maximum(e, f))
        E[i, j], F[i, j], H[i, j] = e, f, h
    return H, E, F


def walk(S, H, E, F, gap_open, gap_extend, end):
    """(ops uint8 in forward order, the cell where the walk stopped) from H at ``end`` (0-based);
    H, E, F as ``gotoh_matrices`` returns them.  At most rows + cols - 1 ops, and the walk stops
    when it leaves the matrix."""
    dtype = H.dtype.type
    go, ge = dtype(gap_open), dtype(gap_extend)
    i, j = end[0] + 1, end[1] + 1
    state, ops, stopped = "H", [], (-1, -1)
    limit = end[0] + end[1] + 1
    while len(ops) < limit and i >= 1 and j >= 1:
        if state == "H":
            if H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
                ops.append(0)
                stopped = (i - 1, j - 1)
                if not H[i - 1, j - 1] > 0:
                    break
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                state = "F"
        elif state == "E":
            ops.append(1)
            state = "H" if H[i, j - 1] - go >= E[i, j - 1] - ge else "E"
            j -= 1
        else:
            ops.append(2)
            state = "H" if H[i - 1, j] - go >= F[i - 1, j] - ge else "F"
            i -= 1
    return np.array(ops[::-1], dtype=np.uint8), stopped


def path_of(S: np.ndarray, gap_open, gap_extend):
    """(score float32, start, end, ops) of a float32 substitution matrix; a score of 0 has start =
    end = (-1, -1) and no ops."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    H, E, F = gotoh_matrices(S, gap_open, gap_extend, np.float32)
    score, end = O.end_of(H[1:, 1:])
    if end == (-1, -1):
        return score, (-1, -1), end, np.zeros(0, dtype=np.uint8)
    ops, start = walk(S, H, E, F, gap_open, gap_extend, end)
    return score, start, end, ops


def box_path(S: np.ndarray, gap_open, gap_extend):
    """The ops of the walk from the last cell of S; none where H there is not positive."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    H, E, F = gotoh_matrices(S, gap_open, gap_extend, np.float32)
    if S.size == 0 or not H[-1, -1] > 0:
        return np.zeros(0, dtype=np.uint8)
    return walk(S, H, E, F, gap_open, gap_extend, (S.shape[0] - 1, S.shape[1] - 1))[0]


def rescore(S: np.ndarray, ops, start, gap_open, gap_extend) -> np.float32:
    """h = 0; op 0: h = fl32(h + s[i][j]); the first op of a run of equal gap ops: g = fl32(h -
    gap_open), every further one g = fl32(g - gap_extend); after the run h = g."""
    go, ge = np.float32(gap_open), np.float32(gap_extend)
    h, i, j, before = np.float32(0), start[0], start[1], 0
    for op in ops:
        if op == 0:
            h = np.float32(h + S[i, j])
            i, j = i + 1, j + 1
        else:
            h = np.float32(h - (ge if op == before else go))
            i, j = (i, j + 1) if op == 1 else (i + 1, j)
        before = op
    return h
