"""Inputs on which the aligners' tie rules decide the answer — shared by test_align_ties_host.py,
test_gpu_align_ties.py and test_gpu_align_crowd.py.  Deterministic, host only: no device is
touched here, and nothing here is the code under test.

    letters(rng, n)            n fp16 rows, each one of 4 signed basis vectors: every cosine of two
                               rows is exactly 0, +1 or -1
    related(rng, rows, ...)    a copy with a few substitutions, short insertions and deletions
    zoo()                      the tie zoo: 6 a-records and 6 b-records of letters, some b-records
                               related to a-records, lengths on the edges of the loop
    TIE_PARAMETERS             four dyadic parameter sets: every sum is exact in float32
    bands_of(q, r, k)          the five bands a pair is aligned under
    local(...), span(...), path(...), within(...), banded(...)
                               the oracles' answers per (pair, parameter set), computed once

With a substitution matrix of three dyadic values and dyadic gap costs nothing is ever rounded,
so two candidates of a maximum are equal in a large share of the cells (test_align_ties_host.py
counts them) where random float rows make them equal essentially never: which candidate the
device names — diagonal, then E, then F; opening before extending; the first cell in (i, j)
order — then shows in every start, end and op."""
from __future__ import annotations

import functools

import numpy as np

import align_band_oracle as BO
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import align_span_oracle as SO

#: (match_scale, match_shift, gap_open, gap_extend)
TIE_PARAMETERS = ((1.0, -0.25, 1.0, 0.25), (2.0, -0.5, 0.75, 0.0), (1.0, -0.25, 0.0, 0.0),
                  (-1.0, 0.25, 1.0, 0.5))
#: one to three strips of 64 a-rows; the 32-column block edge, and 97 + 64 > 128 wraps the ring
ROWS_A = (0, 1, 63, 64, 65, 130)
ROWS_B = (0, 1, 31, 33, 97, 129)
#: (dimension, sign) of the four letters; the dimensions lie in different 8-element pieces of a row
ALPHABET = ((3, 1.0), (3, -1.0), (70, 1.0), (70, -1.0))
#: b-record r is ``related`` to a-record RELATIVES[r] (its first rows, where it is shorter)
RELATIVES = {2: 3, 3: 2, 4: 4, 5: 5}
SEED = 20261019


def letters(rng, n: int) -> np.ndarray:
    """``n`` fp16 rows ``[n, 128]``, each one of the four letters of ALPHABET."""
    chosen = rng.integers(0, len(ALPHABET), size=n)
    rows = np.zeros((n, 128), dtype=np.float16)
    for letter, (dimension, sign) in enumerate(ALPHABET):
        rows[chosen == letter, dimension] = sign
    return rows


def related(rng, rows: np.ndarray, substitutions: int = 4, insertions: int = 2,
            deletions: int = 2, longest: int = 3) -> np.ndarray:
    """A copy of ``rows`` with ``substitutions`` rows replaced by letters, ``insertions`` runs of 1
    to ``longest`` letters put in and ``deletions`` runs of 1 to ``longest`` rows taken out, at
    random places: long homology that more than one path explains."""
    rows = rows.copy()
    if rows.shape[0] == 0:
        return rows
    for at in rng.integers(0, rows.shape[0], size=substitutions):
        rows[at] = letters(rng, 1)[0]
    for _ in range(insertions):
        at = int(rng.integers(0, rows.shape[0] + 1))
        rows = np.concatenate([rows[:at], letters(rng, int(rng.integers(1, longest + 1))), rows[at:]])
    for _ in range(deletions):
        run = int(rng.integers(1, longest + 1))
        if rows.shape[0] > run:
            at = int(rng.integers(0, rows.shape[0] - run + 1))
            rows = np.concatenate([rows[:at], rows[at + run:]])
    return rows


def _fitted(rng, rows: np.ndarray, n: int) -> np.ndarray:
    """``rows`` cut, or continued with letters, to ``n`` rows."""
    return np.concatenate([rows, letters(rng, max(n - rows.shape[0], 0))])[:n]


@functools.lru_cache(maxsize=None)
def zoo() -> dict:
    """``rec_a`` and ``rec_b`` (lists of read-only fp16 arrays of ROWS_A and ROWS_B rows), ``a``
    and ``b`` (the records one after the other) and ``pairs`` (int32 [36, 2], every a-record with
    every b-record, a-record major)."""
    rng = np.random.default_rng(SEED)
    rec_a = [letters(rng, n) for n in ROWS_A]
    rec_b = [_fitted(rng, related(rng, rec_a[RELATIVES[r]][:n + 2]), n) if r in RELATIVES
             else letters(rng, n) for r, n in enumerate(ROWS_B)]
    for record in rec_a + rec_b:
        record.setflags(write=False)
    pairs = np.array([(q, r) for q in range(len(ROWS_A)) for r in range(len(ROWS_B))], dtype=np.int32)
    pairs.setflags(write=False)
    return dict(rec_a=rec_a, rec_b=rec_b, a=np.concatenate(rec_a), b=np.concatenate(rec_b),
                pairs=pairs)


def pair_index(q: int, r: int) -> int:
    return q * len(ROWS_B) + r


def values_of(k: int) -> set:
    """The three values a substitution score of two letters can have under TIE_PARAMETERS[k]."""
    scale, shift = TIE_PARAMETERS[k][:2]
    return {shift - abs(scale), shift, shift + abs(scale)}


@functools.lru_cache(maxsize=None)
def substitution(q: int, r: int, k: int, transposed: bool = False) -> np.ndarray:
    """The float32 substitution matrix of a-record q and b-record r under TIE_PARAMETERS[k], from
    the letters themselves (exact); ``transposed``: of b-record r against a-record q."""
    case = zoo()
    A, B = case["rec_a"][q].astype(np.float32), case["rec_b"][r].astype(np.float32)
    S = O.substitution_f32(B @ A.T if transposed else A @ B.T, *TIE_PARAMETERS[k][:2])
    S.setflags(write=False)
    return S


def _frozen(result: tuple) -> tuple:
    for part in result:
        if isinstance(part, np.ndarray):
            part.setflags(write=False)
    return result


@functools.lru_cache(maxsize=None)
def local(q: int, r: int, k: int, transposed: bool = False):
    """``align_oracle.gotoh_f32``: (score, end)."""
    return O.gotoh_f32(substitution(q, r, k, transposed), *TIE_PARAMETERS[k][2:])


@functools.lru_cache(maxsize=None)
def span(q: int, r: int, k: int, transposed: bool = False):
    """``align_span_oracle.span_of``: (score, start, end)."""
    return SO.span_of(substitution(q, r, k, transposed), *TIE_PARAMETERS[k][2:])


@functools.lru_cache(maxsize=None)
def path(q: int, r: int, k: int, transposed: bool = False):
    """``align_path_oracle.path_of``: (score, start, end, ops)."""
    return _frozen(PO.path_of(substitution(q, r, k, transposed), *TIE_PARAMETERS[k][2:]))


@functools.lru_cache(maxsize=None)
def within(q: int, r: int, k: int, mode: bool):
    """``align_global_oracle.path_of``: (score, start, end, ops); ``mode`` False is global."""
    return _frozen(GO.path_of(substitution(q, r, k), *TIE_PARAMETERS[k][2:], mode))


@functools.lru_cache(maxsize=None)
def bands_of(q: int, r: int, k: int) -> tuple:
    """The bands (lo, hi) of a pair with a row on both sides under TIE_PARAMETERS[k]:

    0  the narrowest band that covers the matrix;
    1  the one diagonal through the start of the pair's alignment (a homologous stretch);
    2  8 diagonals on either side of it, nested between 1 and 0;
    3  9 diagonals from lo = 37 (lo = 5 against fewer than 48 columns): lo is no multiple of 32,
       so the first 32-column block of every strip that has band cells is cut inside;
    4  the diagonals -129 and -128 of a record of more than 128 rows, which leave its first
       two strips without a band cell (skipped) before the third; -40 .. -33 for a shorter one.

    Bands 1 to 3 are made as ``align.band_around`` makes them; the import is local so that the
    module itself needs nothing of the package."""
    from ginfinity_amd import align
    lq, lr = ROWS_A[q], ROWS_B[r]
    start = path(q, r, k)[1]
    seed = np.array([start if start != (-1, -1) else (0, 0)])
    lo = 5 if lr < 48 else 37
    return (BO.covering(lq, lr),
            tuple(int(x) for x in align.band_around(seed, 0)[0]),
            tuple(int(x) for x in align.band_around(seed, 8)[0]),
            tuple(int(x) for x in align.band_around(np.array([[0, lo + 4]]), 4)[0]),
            (-129, -128) if lq > 128 else (-40, -33))


@functools.lru_cache(maxsize=None)
def banded(q: int, r: int, k: int, band: tuple):
    """``align_band_oracle.band_path_of``: (score, start, end, ops)."""
    return _frozen(BO.band_path_of(substitution(q, r, k), *TIE_PARAMETERS[k][2:], *band))


def with_rows() -> list:
    """The pairs (q, r) of the zoo with a row on both sides."""
    return [(q, r) for q in range(1, len(ROWS_A)) for r in range(1, len(ROWS_B))]
