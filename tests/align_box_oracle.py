"""Oracle of local alignment inside a box of rows (the ``box`` of align.local_align, local_spans
and local_paths; gfy_align_local_box, gfy_align_local_span_box; the rules are in include/gfy.h) —
a checker, never the code under test.

    clipped(box, lq, lr)                       the box clipped into an lq x lr matrix, or None
                                               where it holds no cell
    covering(lq, lr)                           the smallest box that covers an lq x lr matrix
    box_path_of(S, go, ge, box, band=None)     (score, start, end, ops) in the coordinates of S:
                                               what the device must give bit for bit
    two_regions()                              the pair of records with two planted regions on
                                               one diagonal, shared by the host and the GPU test

The box is the matrix, so the oracle is the band oracle (align_band_oracle) on the sliced
substitution matrix ``S[i_lo:i_hi + 1, j_lo:j_hi + 1]``, the band shifted by ``-(j_lo - i_lo)``
and the cells shifted back by ``(i_lo, j_lo)``: the second consequence of the contract, taken as
the definition.  It computes nothing of its own."""
from __future__ import annotations

import functools

import numpy as np

import align_band_oracle as BO
import align_cases as Z
import align_oracle as O

NOTHING = (np.float32(0), (-1, -1), (-1, -1), np.zeros(0, dtype=np.uint8))
ROWS_MAX = 4096


def clipped(box, lq: int, lr: int):
    """``(i_lo, i_hi, j_lo, j_hi)`` inside ``0 .. lq - 1`` and ``0 .. lr - 1``, or None."""
    i_lo, i_hi, j_lo, j_hi = (int(x) for x in box)
    assert i_lo <= i_hi and j_lo <= j_hi
    i_lo, j_lo, i_hi, j_hi = max(i_lo, 0), max(j_lo, 0), min(i_hi, lq - 1), min(j_hi, lr - 1)
    return (i_lo, i_hi, j_lo, j_hi) if i_lo <= i_hi and j_lo <= j_hi else None


def covering(lq: int, lr: int):
    return 0, lq - 1, 0, lr - 1


def box_path_of(S: np.ndarray, gap_open, gap_extend, box, band=None):
    """(score float32, start, end, ops) of ``S`` inside ``box`` and, where one is given, the band
    ``(lo, hi)`` of diagonals of S; a score of 0 has start = end = (-1, -1) and no ops."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    inside = clipped(box, *S.shape)
    if inside is None:
        return NOTHING
    i_lo, i_hi, j_lo, j_hi = inside
    lo, hi = (-ROWS_MAX, ROWS_MAX) if band is None else (int(band[0]), int(band[1]))
    shift = j_lo - i_lo
    score, start, end, ops = BO.band_path_of(S[i_lo:i_hi + 1, j_lo:j_hi + 1], gap_open, gap_extend,
                                             lo - shift, hi - shift)
    if end == (-1, -1):
        return score, start, end, ops
    return score, (start[0] + i_lo, start[1] + j_lo), (end[0] + i_lo, end[1] + j_lo), ops


#: the two-region pair: (match_scale, match_shift, gap_open, gap_extend).  A match scores 0.25, two
#: unrelated letters -0.75 or -1.75, so the linker costs more than the weaker region brings
REGION_PARAMETERS = (1.0, -0.75, 2.0, 1.0)
REGION_ROWS = (200, 190)          # rows of the a-record and of the b-record
REGION_SHIFT = 7                  # both regions lie on the diagonal j - i = 7
#: (first row of A, rows): the stronger region, a linker of 45 unrelated rows, the weaker region
REGIONS = ((20, 48), (113, 26))


@functools.lru_cache(maxsize=None)
def two_regions() -> dict:
    """Two records of letters that share two regions at one offset: rows ``at .. at + rows - 1``
    of the a-record are rows ``at + REGION_SHIFT ..`` of the b-record, bit for bit, for both
    entries of REGIONS; everything else is unrelated.  ``a`` / ``b`` are the fp16 rows (read-only),
    ``S`` the exact float32 substitution matrix under REGION_PARAMETERS, ``plants`` the planted
    cells ``[rows, 2]`` of each region."""
    rng = np.random.default_rng(20261021)
    a, b = Z.letters(rng, REGION_ROWS[0]), Z.letters(rng, REGION_ROWS[1])
    plants = []
    for at, rows in REGIONS:
        b[at + REGION_SHIFT:at + REGION_SHIFT + rows] = a[at:at + rows]
        plants.append(np.stack([np.arange(at, at + rows),
                                np.arange(at, at + rows) + REGION_SHIFT], axis=1))
    S = O.substitution_f32(a.astype(np.float32) @ b.astype(np.float32).T, *REGION_PARAMETERS[:2])
    for array in (a, b, S, *plants):
        array.setflags(write=False)
    return dict(a=a, b=b, S=S, plants=plants)


def holds(cells: np.ndarray, plant: np.ndarray) -> bool:
    """Every planted cell is a matched cell of the path ``cells`` (``align.path_cells``)."""
    matched = {tuple(cell) for cell in cells.tolist() if cell[0] >= 0 and cell[1] >= 0}
    return all(tuple(cell) in matched for cell in plant.tolist())
