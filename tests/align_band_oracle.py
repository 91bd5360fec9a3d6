"""Oracle of local alignment inside a band of diagonals (the ``band`` of align.local_align,
local_spans and local_paths; gfy_align_local_band, gfy_align_local_span_band,
gfy_align_trace_band; the rules are in include/gfy.h) — a checker, never the code under test.

    band_matrices(S, go, ge, lo, hi, dtype)   H, E and F (index + 1) and the origins of H under
                                              the band lo <= j - i <= hi
    band_span_of(S, go, ge, lo, hi)           (score, start, end) of a float32 substitution matrix
    band_walk(S, H, E, F, go, ge, end)        the ops of the walk back from ``end``
    band_path_of(S, go, ge, lo, hi)           (score, start, end, ops): what the device must give
                                              bit for bit
    band_box_path(S, go, ge, lo, hi)          the walk from the LAST cell of S under the band: what
                                              gfy_align_trace_band gives for a box that is all of
                                              S (the band already in the box's coordinates)
    covering(lq, lr)                          the narrowest band that covers an lq x lr matrix

The band is the matrix: the program is ``align_span_oracle.gotoh_origins``' anti-diagonal
program, operation by operation in the same order, and after each anti-diagonal the cells
outside the band are set to what lies outside the matrix, H = 0, E = F = -inf, origin -1.  The
walk is ``align_path_oracle.walk``'s, comparing values this program stored; it rounds nothing."""
from __future__ import annotations

import numpy as np

import align_oracle as O
import align_path_oracle as PO


def covering(lq: int, lr: int):
    return -(lq - 1), lr - 1


def band_matrices(S: np.ndarray, gap_open, gap_extend, lo: int, hi: int, dtype):
    """``(H, E, F, start_i, start_j)``: H, E, F ``[Lq + 1, Lr + 1]`` (row and column 0 are outside
    the matrix), the origins ``[Lq, Lr]``; S must already be of ``dtype``."""
    assert S.dtype == dtype and S.ndim == 2 and lo <= hi
    lq, lr = S.shape
    go, ge = dtype(gap_open), dtype(gap_extend)
    H = np.zeros((lq + 1, lr + 1), dtype=dtype)
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    OH = np.full((lq + 1, lr + 1, 2), -1, dtype=np.int64)
    OE = np.full((lq + 1, lr + 1, 2), -1, dtype=np.int64)
    OF = np.full((lq + 1, lr + 1, 2), -1, dtype=np.int64)
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
        oe = np.where((e_open >= e_ext)[:, None], OH[i, j - 1], OE[i, j - 1])
        of = np.where((f_open >= f_ext)[:, None], OH[i - 1, j], OF[i - 1, j])
        here = np.stack([i - 1, j - 1], axis=1)
        od = np.where((H[i - 1, j - 1] > 0)[:, None], OH[i - 1, j - 1], here)
        oh = np.where((h == match)[:, None], od, np.where((h == e)[:, None], oe, of))
        oh = np.where((h > 0)[:, None], oh, -1)
        E[i, j], F[i, j], H[i, j] = e, f, h
        OE[i, j], OF[i, j], OH[i, j] = oe, of, oh
        # the band is the matrix: what is outside it holds what lies outside the matrix
        out = ((j - i) < lo) | ((j - i) > hi)
        io, jo = i[out], j[out]
        H[io, jo], E[io, jo], F[io, jo] = zero, -np.inf, -np.inf
        OE[io, jo], OF[io, jo], OH[io, jo] = -1, -1, -1
    return H, E, F, OH[1:, 1:, 0], OH[1:, 1:, 1]


def band_span_of(S: np.ndarray, gap_open, gap_extend, lo: int, hi: int):
    """(score float32, (i0, j0), (i, j)) under the band; a score of 0 has start = end = (-1, -1)."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    H, _, _, start_i, start_j = band_matrices(S, gap_open, gap_extend, lo, hi, np.float32)
    score, end = O.end_of(H[1:, 1:])
    if end == (-1, -1):
        return score, (-1, -1), end
    return score, (int(start_i[end]), int(start_j[end])), end


def band_walk(S, H, E, F, gap_open, gap_extend, end):
    """(ops uint8 in forward order, the cell where the walk stopped) from H at ``end``: the walk of
    ``align_path_oracle`` on the banded matrices.  A cell outside the band reads as outside the
    matrix, and the walk never enters one: a cell it visits has a positive value."""
    return PO.walk(S, H, E, F, gap_open, gap_extend, end)


def band_path_of(S: np.ndarray, gap_open, gap_extend, lo: int, hi: int):
    """(score float32, start, end, ops) under the band; a score of 0 has start = end = (-1, -1)
    and no ops."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    H, E, F, start_i, start_j = band_matrices(S, gap_open, gap_extend, lo, hi, np.float32)
    score, end = O.end_of(H[1:, 1:])
    if end == (-1, -1):
        return score, (-1, -1), end, np.zeros(0, dtype=np.uint8)
    ops, start = band_walk(S, H, E, F, gap_open, gap_extend, end)
    assert start == (int(start_i[end]), int(start_j[end]))      # the walk ends at the origin
    return score, start, end, ops


def band_box_path(S: np.ndarray, gap_open, gap_extend, lo: int, hi: int):
    """(H of the last cell, ops of the walk from it) of S under the band; no ops where that H is
    not positive (a last cell outside the band holds 0)."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    if S.size == 0:
        return np.float32(0), np.zeros(0, dtype=np.uint8)
    H, E, F, _, _ = band_matrices(S, gap_open, gap_extend, lo, hi, np.float32)
    if not H[-1, -1] > 0:
        return H[-1, -1], np.zeros(0, dtype=np.uint8)
    return H[-1, -1], band_walk(S, H, E, F, gap_open, gap_extend,
                                (S.shape[0] - 1, S.shape[1] - 1))[0]
