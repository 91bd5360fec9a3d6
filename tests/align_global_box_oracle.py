"""Oracle of global and query-in-target alignment inside a box of rows (the ``box`` of
align.global_align and global_paths; gfy_align_global_box, gfy_align_global_trace_box; the rules
are in include/gfy.h) — a checker, never the code under test.

    box_path_of(S, go, ge, box, within)    (score, start, end, ops) in the coordinates of S: what
                                           the device must give bit for bit
    box_score_of(S, go, ge, box, within)   (score, end) of the same

The box is the matrix, so the oracle is the global oracle (align_global_oracle) on the sliced
substitution matrix ``S[i_lo:i_hi + 1, j_lo:j_hi + 1]`` with the cells shifted back by ``(i_lo,
j_lo)``: the second consequence of the contract, taken as the definition.  It computes nothing
of its own."""
from __future__ import annotations

import numpy as np

import align_box_oracle as XO
import align_global_oracle as GO

NOTHING = XO.NOTHING


def _sliced(S: np.ndarray, box):
    S = np.ascontiguousarray(S, dtype=np.float32)
    inside = XO.clipped(box, *S.shape)
    if inside is None:
        return None, (0, 0)
    i_lo, i_hi, j_lo, j_hi = inside
    return S[i_lo:i_hi + 1, j_lo:j_hi + 1], (i_lo, j_lo)


def box_score_of(S: np.ndarray, gap_open, gap_extend, box, within: bool):
    """(score float32, end); a box that holds no cell has score 0 and end (-1, -1)."""
    part, (i_lo, j_lo) = _sliced(S, box)
    if part is None:
        return NOTHING[0], NOTHING[2]
    score, end = GO.score_of(part, gap_open, gap_extend, within)
    return score, (end[0] + i_lo, end[1] + j_lo)


def box_path_of(S: np.ndarray, gap_open, gap_extend, box, within: bool):
    """(score float32, start, end, ops); a box that holds no cell has score 0, start = end =
    (-1, -1) and no ops."""
    part, (i_lo, j_lo) = _sliced(S, box)
    if part is None:
        return NOTHING
    score, start, end, ops = GO.path_of(part, gap_open, gap_extend, within)
    return score, (start[0] + i_lo, start[1] + j_lo), (end[0] + i_lo, end[1] + j_lo), ops
