"""Oracle of the global and query-in-target modes (align.global_align, align.global_paths,
gfy_align_global, gfy_align_global_trace; the definition is in include/gfy.h) — a checker, never
the code under test.

    matrices(S, go, ge, dtype, within)   H, E and F with their borders, index + 1: row 0 and column
                                         0 are row -1 and column -1 of the definition, iterated
    score_of(S, go, ge, within)          (score, end) of a float32 substitution matrix
    path_of(S, go, ge, within)           (score, start, end, ops): what the device must give bit
                                         for bit
    rescore(S, ops, start, go, ge)       the float32 score the ops add up to (the local rule)
    enumerate_alignments(S, go, ge, within)   the best sum over every alignment of a tiny matrix,
                                         one by one

``within`` False is global alignment, True query-in-target.  The borders are iterated cell by
cell exactly as the definition iterates them; the inside runs along anti-diagonals, whose cells
do not depend on each other, so each numpy operation is the one rounded operation per cell of a
cell-by-cell loop.  The walk follows the general rules on the bordered matrices and only the
exits are special; it compares values the program stored and rounds nothing."""
from __future__ import annotations

import numpy as np

import align_path_oracle as PO

rescore = PO.rescore


def matrices(S: np.ndarray, gap_open, gap_extend, dtype, within: bool):
    """``(H, E, F)``, each ``[Lq + 1, Lr + 1]``; S must already be of ``dtype``."""
    assert S.dtype == dtype and S.ndim == 2
    lq, lr = S.shape
    go, ge = dtype(gap_open), dtype(gap_extend)
    H = np.zeros((lq + 1, lr + 1), dtype=dtype)
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    with np.errstate(invalid="raise"):
        for i in range(1, lq + 1):                      # the left border, both modes
            F[i, 0] = max(dtype(F[i - 1, 0] - ge), dtype(H[i - 1, 0] - go))
            H[i, 0] = F[i, 0]
        if not within:                                  # the top border: charged, or free
            for j in range(1, lr + 1):
                E[0, j] = max(dtype(E[0, j - 1] - ge), dtype(H[0, j - 1] - go))
                H[0, j] = E[0, j]
        for d in range(lq + lr - 1):
            i = np.arange(max(0, d - lr + 1), min(lq - 1, d) + 1) + 1
            j = d + 2 - i
            e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
            f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
            h = np.maximum(H[i - 1, j - 1] + S[i - 1, j - 1], np.maximum(e, f))
            E[i, j], F[i, j], H[i, j] = e, f, h
    return H, E, F


def end_of(H: np.ndarray, within: bool):
    """(score, (i, j)) from the bordered H: the last cell, or the first best cell of the last
    row; (0, (-1, -1)) where a side has no row."""
    lq, lr = H.shape[0] - 1, H.shape[1] - 1
    if lq == 0 or lr == 0:
        return H.dtype.type(0), (-1, -1)
    if not within:
        return H[lq, lr], (lq - 1, lr - 1)
    j = int(np.argmax(H[lq, 1:]))          # first occurrence
    return H[lq, 1 + j], (lq - 1, j)


def walk(S, H, E, F, gap_open, gap_extend, end, within: bool):
    """(ops uint8 in forward order, start) of the walk back from H at ``end`` (0-based)."""
    dtype = H.dtype.type
    go, ge = dtype(gap_open), dtype(gap_extend)
    i, j = end[0] + 1, end[1] + 1
    state, ops, start_j = "H", [], 0
    while True:
        if state == "H":
            if i == 0 and j == 0:
                break
            if j == 0:                       # (i - 1, -1): the left border is a charged gap
                ops += [2] * i
                break
            if i == 0:                       # (-1, j - 1): charged (global) or free (within)
                if within:
                    start_j = j
                else:
                    ops += [1] * j
                break
            if H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
                ops.append(0)
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            ops.append(1)
            state = "H" if H[i, j - 1] - go >= E[i, j - 1] - ge else "E"
            j -= 1
        else:
            ops.append(2)
            state = "H" if H[i - 1, j] - go >= F[i - 1, j] - ge else "F"
            i -= 1
    return np.array(ops[::-1], dtype=np.uint8), (0, start_j)


def score_of(S: np.ndarray, gap_open, gap_extend, within: bool, dtype=np.float32):
    S = np.ascontiguousarray(S, dtype=dtype)
    return end_of(matrices(S, gap_open, gap_extend, dtype, within)[0], within)


def path_of(S: np.ndarray, gap_open, gap_extend, within: bool, dtype=np.float32):
    """(score, start, end, ops); a pair with nothing to align has score 0, start = end =
    (-1, -1) and no ops."""
    S = np.ascontiguousarray(S, dtype=dtype)
    H, E, F = matrices(S, gap_open, gap_extend, dtype, within)
    score, end = end_of(H, within)
    if end == (-1, -1):
        return score, (-1, -1), end, np.zeros(0, dtype=np.uint8)
    ops, start = walk(S, H, E, F, gap_open, gap_extend, end, within)
    return score, start, end, ops


def enumerate_alignments(S: np.ndarray, gap_open: float, gap_extend: float, within: bool) -> float:
    """The best sum over every alignment, by walking each: a path moves between the corners of
    the cells, diagonally (a match, + S[i][j]), right (a row of B faces a gap) or down (a row of
    A faces a gap); a gap position costs gap_extend after a move of the same kind and gap_open
    after anything else.  Global: from corner (0, 0) to corner (Lq, Lr).  Within: from any corner
    of the top edge — along which nothing moves right, those rows are free — to any corner (Lq,
    j + 1), 0 <= j < Lr.  Exponential: for matrices of up to 4 x 4.  Float64; feed it values that
    add exactly."""
    lq, lr = S.shape
    best = [-np.inf]

    def go_on(gi, gj, last, total):
        if gi == lq and (gj == lr or (within and gj >= 1)):
            best[0] = max(best[0], total)
        if gi < lq and gj < lr:
            go_on(gi + 1, gj + 1, "m", total + float(S[gi, gj]))
        if gj < lr and not (within and gi == 0):
            go_on(gi, gj + 1, "r", total - (gap_extend if last == "r" else gap_open))
        if gi < lq:
            go_on(gi + 1, gj, "d", total - (gap_extend if last == "d" else gap_open))

    for gj in range(lr + 1 if within else 1):
        go_on(0, gj, None, 0.0)
    return best[0]
