"""Oracles of the local aligner (ginfinity_amd/align.py, include/gfy.h) — checkers, never the
code under test.

    gotoh_f32(S, go, ge)            the recurrences and the end rule on a float32 substitution
                                    matrix, every operation one float32 rounding: what the device
                                    must give bit for bit
    gotoh_f64(A, B, ...)            the definition in float64, from float64 cosines of the rows
    enumerate_paths(S, go, ge)      every local alignment path of a tiny matrix, one by one

The dynamic programs run along anti-diagonals, whose cells do not depend on each other: each
numpy operation is then the same single rounded operation per cell that a cell-by-cell loop
would perform, so the order changes no bit."""
from __future__ import annotations

import numpy as np


def _gotoh(S: np.ndarray, gap_open, gap_extend, dtype) -> np.ndarray:
    """H of the definition, ``[Lq, Lr]`` in ``dtype``; S must already be of ``dtype``."""
    assert S.dtype == dtype and S.ndim == 2
    lq, lr = S.shape
    go, ge = dtype(gap_open), dtype(gap_extend)
    H = np.zeros((lq + 1, lr + 1), dtype=dtype)           # index + 1: row / column 0 is outside
    E = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    F = np.full((lq + 1, lr + 1), -np.inf, dtype=dtype)
    zero = dtype(0)
    for d in range(lq + lr - 1):
        i = np.arange(max(0, d - lr + 1), min(lq - 1, d) + 1) + 1
        j = d + 2 - i
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        h = np.maximum(np.maximum(zero, H[i - 1, j - 1] + S[i - 1, j - 1]), np.maximum(e, f))
        E[i, j], F[i, j], H[i, j] = e, f, h
    return H[1:, 1:]


def end_of(H: np.ndarray):
    """(score, (i, j)) by the end rule: the first cell, i ascending then j ascending, that holds
    the maximum; (0, (-1, -1)) when nothing is positive (or there is no cell)."""
    if H.size == 0 or not H.max() > 0:
        return H.dtype.type(0), (-1, -1)
    flat = int(np.argmax(H))          # row-major, first occurrence
    return H.max(), (flat // H.shape[1], flat % H.shape[1])


def substitution_f32(C: np.ndarray, match_scale, match_shift) -> np.ndarray:
    """s = fl32(fl32(C * scale) + shift) for a float32 cosine matrix."""
    assert C.dtype == np.float32
    return (C * np.float32(match_scale)).astype(np.float32) + np.float32(match_shift)


def gotoh_f32(S: np.ndarray, gap_open, gap_extend):
    """(score float32, (i, j)) of a float32 substitution matrix."""
    return end_of(_gotoh(np.ascontiguousarray(S, dtype=np.float32), gap_open, gap_extend,
                         np.float32))


def cosine_f64(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    A, B = A.astype(np.float64), B.astype(np.float64)
    na = np.maximum(np.linalg.norm(A, axis=1), 1e-12)
    nb = np.maximum(np.linalg.norm(B, axis=1), 1e-12)
    return (A @ B.T) / (na[:, None] * nb[None, :])


def gotoh_f64(A, B, gap_open, gap_extend, match_scale=1.0, match_shift=0.0):
    """(score, (i, j), H) of the float64 definition on rows ``A`` and ``B``; the four parameters
    are taken at their float32 values, which is what the device receives."""
    scale, shift = float(np.float32(match_scale)), float(np.float32(match_shift))
    S = cosine_f64(A, B) * scale + shift
    H = _gotoh(S, float(np.float32(gap_open)), float(np.float32(gap_extend)), np.float64)
    score, end = end_of(H)
    return float(score), end, H


def enumerate_paths(S: np.ndarray, gap_open: float, gap_extend: float) -> np.ndarray:
    """max(0, best path ending in cell (i, j)) for every cell, by walking every path: a path
    starts at any corner between cells and moves diagonally (a match, + S[i][j]), right or down
    (a gap position: gap_open after anything else, gap_extend after a move of the same kind).
    Exponential: for matrices of up to 4 x 4.  Float64; feed it values that add exactly."""
    lq, lr = S.shape
    best = np.zeros((lq, lr), dtype=np.float64)

    def walk(gi, gj, last, total):
        if gi >= 1 and gj >= 1 and last is not None:
            best[gi - 1, gj - 1] = max(best[gi - 1, gj - 1], total)
        if gi < lq and gj < lr:
            walk(gi + 1, gj + 1, "m", total + float(S[gi, gj]))
        if gj < lr:
            walk(gi, gj + 1, "r", total - (gap_extend if last == "r" else gap_open))
        if gi < lq:
            walk(gi + 1, gj, "d", total - (gap_extend if last == "d" else gap_open))

    for gi in range(lq + 1):
        for gj in range(lr + 1):
            walk(gi, gj, None, 0.0)
    return best
