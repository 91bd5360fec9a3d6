"""Oracle of the start cells of the local aligner (align.local_spans, gfy_align_local_span;
the rules are in include/gfy.h) — a checker, never the code under test.

    gotoh_origins(S, go, ge, dtype)   H of the definition and, per cell, the origin (i0, j0) of
                                      H by the tie rules; -1 where H is not positive
    span_of(S, go, ge)                (score, start, end) of a float32 substitution matrix: what
                                      the device must give bit for bit

The dynamic program runs along anti-diagonals like ``align_oracle._gotoh``, with the same
operations in the same order, so H is that function's H bit for bit; the origins are chosen by
comparing the operands of each maximum, which rounds nothing."""
from __future__ import annotations

import numpy as np

import align_oracle as O


def gotoh_origins(S: np.ndarray, gap_open, gap_extend, dtype):
    """``(H, start_i, start_j)``, each ``[Lq, Lr]``; S must already be of ``dtype``."""
    assert S.dtype == dtype and S.ndim == 2
    lq, lr = S.shape
    go, ge = dtype(gap_open), dtype(gap_extend)
    H = np.zeros((lq + 1, lr + 1), dtype=dtype)           # index + 1: row / column 0 is outside
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    # origins as (i0, j0) in the last axis; what a value <= 0 holds is never used
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
    return H[1:, 1:], OH[1:, 1:, 0], OH[1:, 1:, 1]


def span_of(S: np.ndarray, gap_open, gap_extend):
    """(score float32, (i0, j0), (i, j)) of a float32 substitution matrix; a score of 0 has
    start = end = (-1, -1)."""
    H, start_i, start_j = gotoh_origins(np.ascontiguousarray(S, dtype=np.float32), gap_open,
                                        gap_extend, np.float32)
    score, end = O.end_of(H)
    if end == (-1, -1):
        return score, (-1, -1), end
    return score, (int(start_i[end]), int(start_j[end])), end
