"""Batched local alignment of record pairs on the device: the step behind ``record_scores``.

``distance.record_scores`` ranks pairs of records; ``local_align`` aligns the pairs a caller
picks from that ranking, without the embeddings leaving the device:

    scores = distance.record_scores(rows, counts_a=counts, metric="cosine")
    pairs = align.top_pairs(scores, 8, largest=True)
    score, end = align.local_align(rows, counts_a=counts, pairs=pairs, gap_open=1.0, gap_extend=0.25)

The sparse chain needs no dense ``[Q, R]`` matrix: the radius search, its hits collapsed into
diagonal runs, the runs linked into chains, the best chains as seeds, alignment inside a band
around each seed's diagonals and a box around its rows:

    hits = distance.within(rows, threshold=0.9, metric="cosine", exclude_records=counts)
    runs = align.hit_runs(hits, counts_a=counts, min_length=8)
    chains = align.chain_runs(runs, max_gap=8)
    best = chains.best(64)                                  # host indices: most hits, then heaviest
    paths = align.local_paths(rows, counts_a=counts, pairs=chains.pairs[best],
                              band=chains.bands(4)[best], box=chains.boxes(16)[best],
                              gap_open=1.0, gap_extend=0.25)

A chain is a list of anchors, and the step after it is to fill between them: the stretch from a
chain's first cell to its last aligned end to end, unrelated linkers included (a local
alignment keeps the best piece and drops the rest), or a window of the query placed inside a
region of the target:

    paths = align.global_paths(rows, counts_a=counts, pairs=chains.pairs[best],
                               box=chains.boxes(0)[best], gap_open=1.0, gap_extend=0.25)
    where = align.global_paths(rows, counts_a=counts, pairs=chains.pairs[best], within=True,
                               box=chains.boxes(0)[best] + [0, 0, -32, 32],   # 32 b-rows of slack
                               gap_open=1.0, gap_extend=0.25)

**This is not ``ginfinity-sw``.**  The reference delegates alignment to that external package,
which is not in its tree; it holds the names of eight scoring parameters and no formula.  The
semantics below are defined here and in include/gfy.h, as the whole distance path's are.
Nothing here reproduces that package's scores, none of ``default_alignment_parameters()``'s
entries maps onto an argument of ``local_align`` (that function stays a pass-through and is not
wired in), and ``gap_open`` / ``gap_extend`` are ordinary arguments without a default.

Definition.  A pair ``(q, r)`` aligns ``A`` = the ``Lq`` rows of record q of ``a`` with ``B`` =
the ``Lr`` rows of record r of ``b``: Smith-Waterman with affine gaps (Gotoh), all in float32,
every addition and subtraction one rounded operation, ``max`` exact:

    C[i][j] = distance.pairwise(A, B, metric="cosine")[i, j]           (bit for bit)
    s[i][j] = fl32(fl32(C[i][j] * match_scale) + match_shift)
    E[i][j] = max(E[i][j-1] - gap_extend, H[i][j-1] - gap_open)
    F[i][j] = max(F[i-1][j] - gap_extend, H[i-1][j] - gap_open)
    H[i][j] = max(0, H[i-1][j-1] + s[i][j], E[i][j], F[i][j])

with ``H = 0`` and ``E = F = -inf`` outside the matrix; ``gap_open`` is the cost of a gap's
first position.  ``score = max H``; ``end = (i, j)`` is the first cell in the order (i
ascending, then j ascending) with ``H == score``, 0-based inside the two records; a score of 0
(no positive cell, a record of zero rows) gives ``end = (-1, -1)``, and only a zero keeps no
promise of its sign.  Every cell is a fixed expression of its three predecessors, so a pair's
result depends neither on the other pairs of the call nor on the run, bit for bit.

Start cells.  ``local_spans`` returns, next to score and end, the cell where each alignment
starts.  Every E, F and H that is positive has an origin ``(i0, j0)``, the first matched cell of
the path that produced it, carried through the same recurrences (the matrix is still never
written):

    H[i][j]   the origin of the first candidate, in the order diagonal, then E, then F, whose
              value equals H[i][j]; the diagonal candidate ``H[i-1][j-1] + s[i][j]`` carries the
              origin of ``H[i-1][j-1]`` if that value is > 0 and ``(i, j)`` itself otherwise (a
              predecessor that is 0 of either sign or outside the matrix: the alignment starts
              here)
    E[i][j]   the origin of ``H[i][j-1]`` if ``H[i][j-1] - gap_open >= E[i][j-1] - gap_extend``
              (opening wins a tie), else that of ``E[i][j-1]``
    F[i][j]   the same rule with the row above

A value <= 0 has no origin, and none is needed: a positive E or F descends from a positive H.
``start`` is the origin of H at ``end``; a score of 0 gives ``(-1, -1)``.  An origin is a fixed
function of the three predecessors, so a start is as independent of company and run as a score.
It follows that ``start <= end`` in both coordinates, that ``s[start] == H[start] > 0``, and that
the same recurrences run on the box ``start..end`` alone reach exactly ``score`` at the box's last
cell, bit for bit: the traceback only has to revisit that box.

The aligned path.  ``local_paths`` returns, next to score, start and end, the path itself: the
walk back from ``end`` by the origin rules above, nothing new.  A state is one of H, E or F at a
cell, and the walk starts in H at ``end``:

    H at (i, j)   if ``H == H[i-1][j-1] + s[i][j]``: op ``0`` (row i of A matched with row j of B);
                  then, if ``H[i-1][j-1] > 0``, on in H at (i-1, j-1), otherwise stop (this cell
                  is ``start``).  If H is not the diagonal candidate but ``H == E[i][j]``: E at
                  the same cell.  Otherwise F at the same cell.
    E at (i, j)   op ``1`` (row j of B faces a gap); on at (i, j-1), in H if ``H[i][j-1] -
                  gap_open >= E[i][j-1] - gap_extend`` (opening wins a tie), otherwise in E
    F at (i, j)   op ``2`` (row i of A faces a gap); on at (i-1, j) by the same rule with the
                  row above

The ops are reported in forward order, ``start`` to ``end``.  The first and the last op are
``0``; the ops ``0`` and ``2`` number ``end_i - start_i + 1``, the ops ``0`` and ``1`` ``end_j -
start_j + 1``; a score of 0 has an empty path.  Re-scoring the ops (``h = 0``; op 0: ``h = fl32(h
+ s[i][j])``; the first op of a run of equal gap ops ``g = fl32(h - gap_open)``, each further one
``g = fl32(g - gap_extend)``, and ``h = g`` after the run) gives ``score`` bit for bit.  The
device walks the box ``start..end`` alone, which gives the same ops as the full matrix
(include/gfy.h has the argument), and keeps 4 bits per cell of the box in scratch memory: the
only thing proportional to ``Lq x Lr`` that is ever written.

Global and query-in-target alignment.  ``global_align`` and ``global_paths`` answer two other
questions with the same recurrences, substitution scores and parameters.  ``within=False`` is
global alignment (Needleman-Wunsch with affine gaps): how similar are two whole records — both
take part end to end, and unrelated flanks are charged for.  ``within=True`` is query-in-target
("fit") alignment: where does all of the a-record lie inside the b-record — the b-record's rows
in front of and behind the alignment are free, so a window cannot take part with a piece of
itself as it may in a local alignment:

    E[i][j] = max(E[i][j-1] - gap_extend, H[i][j-1] - gap_open)
    F[i][j] = max(F[i-1][j] - gap_extend, H[i-1][j] - gap_open)
    H[i][j] = max(H[i-1][j-1] + s[i][j], E[i][j], F[i][j])              (no 0 candidate)

The borders are the same recurrences carried onto row -1 and column -1, so a border is an
iterated sum and not a closed form.  ``H[-1][-1] = 0``.  Left border, both modes: ``F[i][-1] =
max(F[i-1][-1] - gap_extend, H[i-1][-1] - gap_open)``, ``H[i][-1] = F[i][-1]``, ``E[i][-1] =
-inf``, with ``F[-1][-1] = -inf``; that is ``H[0][-1] = fl32(0 - gap_open)`` and ``H[i][-1] =
fl32(H[i-1][-1] - gap_extend)``.  Top border, global: the mirror image, ``H[-1][j] = E[-1][j]``
iterated along j and ``F[-1][j] = -inf``.  Top border, ``within``: ``H[-1][j] = 0`` and ``E[-1][j]
= F[-1][j] = -inf`` for every j.

Global: ``score = H[Lq-1][Lr-1]`` and ``end = (Lq-1, Lr-1)``.  ``within``: ``score = max_j
H[Lq-1][j]`` over ``0 <= j < Lr`` and ``end = (Lq-1, j)`` for the first such j.  Scores may be
negative.  A pair with a record of zero rows on either side is "nothing to align": score 0, end
``(-1, -1)`` and an empty path, as in the local mode (not the cost of a gap).  Because every
operation is monotone in its inputs and the modes differ only in the candidates they add,
``global score <= within score <= local score`` holds exactly, in float32 comparison, for any
pair and parameters.

The path of these modes is the walk back from ``end``, starting in H, by the tie rules above (in
H the diagonal first, then E, then F; in E and F opening wins a tie), with the same ops in
forward order.  There is no "starts here" rule: the walk ends on a border.  At ``(-1, -1)`` it
stops; at ``(i, -1)`` it emits ``i + 1`` ops ``2`` (the left border is a charged gap); at ``(-1,
j)`` global emits ``j + 1`` ops ``1`` and ``within`` stops (those rows are free).  A path has at
most ``Lq + Lr`` ops, one more than the local bound.  ``start`` is (first row of A consumed, first
row of B consumed): ``start_i`` is always 0, ``start_j`` is 0 for global and ``end_j + 1 - #(ops
!= 2)`` for ``within``, which is ``end_j + 1`` when no row of B is consumed; ``path_cells(ops,
start)`` gives the cells.  Re-scoring the ops by the rule above gives ``score`` bit for bit,
which is why the borders are iterated.

Alignment inside a band (seed and extend).  ``local_align``, ``local_spans`` and ``local_paths``
take ``band``: per pair two integers ``(lo, hi)`` with ``lo <= hi``, diagonals ``d = j - i`` in
the coordinates of the two records, both ends inclusive.  **The band is the matrix**: a cell
whose diagonal lies outside ``[lo, hi]`` is outside the matrix in the sense above, ``H = 0``, ``E
= F = -inf``, no origin.  Nothing else changes: the substitution scores, the recurrences, every
rounded operation, the order that names ``end``, the origin rules, the tie rules of the walk and
the op codes stay as they are.  "The best local alignment near this seed" is another question
than the best one anywhere in the pair: eight seeds in one target get eight answers.  It
follows that

* a band that covers the matrix (``lo <= -(Lq - 1)`` and ``hi >= Lr - 1``) gives the results of
  the call without a band bit for bit;
* every operation is monotone and an outside cell holds the least values a cell can have, so
  widening a band never lowers a pair's score, exactly, in float32 comparison;
* a band that meets no cell of the matrix gives score 0, start and end ``(-1, -1)`` and an empty
  path;
* ``lo == hi`` is gapless extension along one diagonal;
* the span property survives with the band shifted: the recurrences run on the box
  ``start..end`` alone, under the band ``(lo - (start_j - start_i), hi - (start_j - start_i))``,
  reach exactly ``score`` at the box's last cell, and the path is the walk inside that box; a
  path cell always has a positive value, so the walk never leaves the band;
* re-scoring the ops gives ``score`` bit for bit, as without a band.

Seeds and their bands come from ``seeds.py``, whose names this module exports: ``band_around``
makes bands from seed cells, ``hit_cells`` gives one seed per hit of ``distance.topk`` or
``within``, ``hit_runs`` one per maximal diagonal run of ``within`` hits, and ``chain_runs``
links the runs that an inserted or deleted row cut apart into one band (``chains.pairs`` and
``chains.bands(4)`` in the recipe above; ``runs.pairs`` and ``runs.bands(16)`` seed from the runs
themselves).  Their definitions are at the
head of that module.  The device does not do the work outside the band: a strip of 64 rows from row ``i0`` holds band cells in the
columns ``c_lo = max(0, i0 + lo) .. c_hi = min(Lr - 1, i0 + rows - 1 + hi)`` only, a strip
without any is skipped, and a strip takes ``c_hi - (c_lo & ~31) + rows`` steps against ``Lr + rows
- 1`` (arithmetic, not a measurement; two records of 4,096 rows and a band of 129 diagonals:
about 290 steps per strip against about 4,160).

Alignment inside a box (one answer per chain).  A band says on which diagonals a seed lies, not
where on them: two conserved regions of one record pair at the same offset, an unrelated linker
between them, share their band, and a banded call returns the stronger region for both.
``local_align``, ``local_spans`` and ``local_paths`` take ``box``: per pair four integers ``(i_lo,
i_hi, j_lo, j_hi)``, rows of the a-record and of the b-record, 0-based inside the two records,
both ends inclusive.  **The box is the matrix**, exactly as the band is: a cell outside the box
is outside the matrix, ``H = 0``, ``E = F = -inf``, no origin.  Nothing else changes: the
substitution scores, the recurrences, every rounded operation, the order that names ``end``, the
origin rules, the tie rules of the walk and the op codes stay as they are.  ``band`` keeps its
meaning, diagonals ``j - i`` in the records' coordinates, and combines with the box by
intersection.  ``starts``, ``ends`` and ``path_cells`` stay in the records' coordinates.  The
box is clipped into the record; a box that holds no cell after clipping gives what a band that
meets no cell gives: score 0, start and end ``(-1, -1)`` and an empty path.  ``i_lo > i_hi`` or
``j_lo > j_hi`` as given is a ``ValueError`` (the kernel refuses it like a band with ``lo >
hi``).  It follows that

* a box that covers both records gives the results of the call without a box bit for bit:
  scores, starts, ends and ops;
* a boxed call equals, bit for bit, the call without a box on rows ``i_lo..i_hi`` of A and
  ``j_lo..j_hi`` of B taken as two records of their own, with the band shifted by ``-(j_lo -
  i_lo)`` and the cells shifted back by ``(i_lo, j_lo)``;
* enlarging a box never lowers a score, exactly, in float32 comparison (the band's argument);
* re-scoring the ops gives ``score`` bit for bit;
* a pair's result depends neither on the other pairs of the call nor on the run.

``Runs.boxes(margin)`` and ``Chains.boxes(margin)`` make the boxes of seeds, ``margin`` rows
around each on all four sides; with ``band=chains.bands(4)[best], box=chains.boxes(16)[best]``
eight seeds in one target get eight answers also where they share their diagonals.  The device
does not do the work outside the box: the strips start at the box's first row, ``ceil(box rows /
64)`` of them, so a 150-row chain with a margin of 16 in two 4,096-row records takes 3 strips
where a band of 9 diagonals alone meets all 64 of the a-record (arithmetic, not a measurement),
and the carry workspace is sized by the widest box of the call.  The path needs no boxed trace:
``start..end`` lies inside the box, so the trace on ``start..end`` walks the same path
(include/gfy.h has the argument).

Global and query-in-target alignment inside a box (fill between anchors).  ``global_align`` and
``global_paths`` take ``box`` exactly as the local functions do: the same form, the same
clipping, the same checks and ``ValueError`` texts.  **The box is the matrix**: a boxed global
alignment is by definition the global alignment of rows ``i_lo..i_hi`` of A and ``j_lo..j_hi`` of
B taken as two records of their own.  Row -1 and column -1 of the definition are the rows just
outside the box; the left border is the charged gap iterated in float32, the top border is
charged (global) or free (``within``), exactly as without a box; substitution scores,
recurrences, rounded operations, tie rules and op codes do not change.  With ``within=True`` the
a-side of the box is the window, the b-side the region, and the b-rows of the region in front
of and behind the alignment are free.  Results stay in the records' coordinates: global has
``end = (i_hi, j_hi)`` of the clipped box and ``start = (i_lo, j_lo)``; ``within`` has ``end =
(i_hi, j)`` for the first best ``j`` in ``j_lo..j_hi`` and ``start = (i_lo, start_j)``, ``start_j =
end_j + 1`` where no b-row is consumed.  A box that holds no cell after clipping is "nothing to
align", like a record of zero rows: score 0, start and end ``(-1, -1)``, an empty path.  It
follows that

* a covering box gives the results of the call without a box bit for bit: scores, starts, ends
  and ops;
* a boxed call equals, bit for bit, the call without a box on the sliced rows as two records of
  their own, with the cells shifted back by ``(i_lo, j_lo)``;
* re-scoring the ops gives ``score`` bit for bit;
* in one and the same box ``global <= within <= local`` holds exactly;
* a pair's result depends neither on the other pairs of the call, nor on the run, nor on the
  workspace;
* for ``within``, widening the box on the b-side (a lower ``j_lo``, a higher ``j_hi``, the same
  a-rows) never lowers the score, exactly, in float32 comparison: a real cell of a column is
  never below the charged left border it replaces, and every operation is monotone
  (include/gfy.h has the induction).  Global has no such property: a wider box must pay for the
  rows it adds.

The device does not do the work outside the box: ``ceil(box rows / 64)`` strips from the box's
first row, 3 for a 150-row chain where ``global_paths`` on two whole 4,096-row records takes 64
and charges the flanks as well, so that its path is not even the same one (arithmetic, not a
measurement).  ``global_paths`` stays two launches with no copy to the host between them: slots
and the largest box come from the boxes clipped on the host.

Limits: a record has at most ``GFY_ALIGN_ROWS_MAX`` = 4096 rows (``records.MAXIMUM_LENGTH_NT``),
``0 <= gap_extend <= gap_open``, the four parameters finite.  Out of scope: a band on the
global and ``within`` modes (borders that leave the band, pairs with no admissible path at all;
a box has neither, and is built),
band-only or box-only storage of the direction words, boxes that are not rectangles, a span-only kernel for the global and ``within`` modes,
free ends on the a-side, a ``device="cpu"`` path, and, of what tells a score's meaning: nulls
for the global and ``within`` modes, shuffling the a-side, and an E-value calibrated over a whole
database search (``null_scores`` and ``significance`` below judge one pair against its own
shuffled target).  Measured cost: DESIGN.md §4.

Values along a path.  ``path_values`` takes the paths of any of the functions above (or a
caller's own) and returns, per op, the cosine of its cell — the dense kernel's, bit for bit,
from the same eight MFMA steps on the path's 32 row pairs at a time, not from a dense ``Lq x Lr``
matrix — and the running score behind it, and per path the score (the aligner's, bit for bit),
the matches, the gap runs and the float64 sum of the matched cosines.

Null scores and significance.  A raw local score cannot rank hits across pairs: it grows with
the two lengths, depends on ``match_scale / match_shift / gap_*`` and on how ordinary the two
records' rows are, and this aligner has no scoring matrix to look a λ and a K up for.  The answer
is empirical: align the pair against **the same target with its rows in random order**, K times,
and state the real score against those K.  ``null_scores`` does that in one launch and without
writing a shuffled row: in run k column j of pair p's matrix holds row ``order[j]`` of the pair's
b-side (the b-record, or with a ``box`` the b-rows of the box, so entries are relative to the
box: ``0 .. columns - 1``), 4 bytes per shuffled row in place of 256.  Nothing else changes — the
a-side, the cosine (its ``1/|b|`` taken from the row the column holds), the recurrences, the band
and the box — so ``null_scores(...)[p, k]`` equals, bit for bit, ``local_align`` of the pair with
the b-side replaced by the rows ``order[...]`` copied out in that order.  Entries need not be a
permutation: a reversal, or a bootstrap with repeats, is an order like any other.

``shuffle_orders(columns, shuffles, seed)`` makes the orders, and they are a fixed function of
``(seed, v, j)`` that anything with 64-bit integers reproduces (no ``torch.Generator``): with
``v = p * shuffles + k`` the virtual pair, all arithmetic modulo 2^64 and ``>>`` logical,

    mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;
             z ^= z >> 31
    G = 0x9E3779B97F4A7C15
    key(seed, v, j) = mix(mix(seed + (v + 1) * G) + (j + 1) * G) >> 32

and the order of virtual pair v is ``0 .. columns - 1`` stably sorted by ``(key, j)``; the whole
array is one stable sort by (virtual pair, key, j).  The same bytes come out on a CPU tensor and
on the device.  ``significance(scores, null)`` turns ``[P, K]`` null scores into a z-score and an
extreme-value p-value per pair; its docstring has the formulas.  They are estimates from K
samples: K decides their resolution.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _native as native
from .distance import (_checked, _checked_integer, _grown, _host_array, _prepare, _record_ptr,
                       _scratch_tail)
from .seeds import (Chains, ChainsWorkspace, Runs, RunsWorkspace, band_around, chain_runs,
                    hit_cells, hit_runs)


class AlignWorkspace:
    """Scratch memory of ``local_align``, ``local_spans``, ``local_paths``, ``global_align`` and
    ``global_paths`` kept across calls, as ``distance.RecordWorkspace`` keeps that of ``record_scores`` (the results are always new
    tensors)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None

    def buffer(self, device, scratch_bytes: int) -> torch.Tensor:
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        return self.scratch


def _checked_pairs(pairs, records_a: int, records_b: int) -> np.ndarray:
    """``pairs`` as an int32 ``[P, 2]`` host array with every index inside its side's records."""
    pairs = _host_array(pairs)
    if pairs.size == 0 and pairs.ndim in (1, 2):
        pairs = np.zeros((0, 2), dtype=np.int64)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be an integer array of shape (P, 2)")
    pairs = pairs.astype(np.int64)
    if pairs.shape[0] >= 2 ** 31:
        raise ValueError("pairs must hold fewer than 2^31 pairs")
    if pairs.shape[0] and (pairs.min() < 0 or pairs[:, 0].max() >= records_a
                           or pairs[:, 1].max() >= records_b):
        bad = int(np.flatnonzero((pairs[:, 0] < 0) | (pairs[:, 0] >= records_a)
                                 | (pairs[:, 1] < 0) | (pairs[:, 1] >= records_b))[0])
        raise ValueError(f"pair {bad} = ({int(pairs[bad, 0])}, {int(pairs[bad, 1])}) is out of "
                         f"range: a has {records_a} records, b has {records_b}")
    return np.ascontiguousarray(pairs.astype(np.int32))


def _checked_band(band, count: int) -> np.ndarray | None:
    """``band`` as an int32 ``[count, 2]`` host array of ``(lo, hi)`` with ``lo <= hi``, clipped
    into ``[-GFY_ALIGN_ROWS_MAX, GFY_ALIGN_ROWS_MAX]``; ``None`` stays ``None`` (no band)."""
    if band is None:
        return None
    if isinstance(band, (tuple, list)) and any(isinstance(x, (bool, np.bool_)) for x in band):
        raise ValueError("band must hold integers (lo, hi)")
    band = _host_array(band)
    if band.size == 0 and count == 0 and band.ndim in (1, 2):
        band = np.zeros((0, 2), dtype=np.int64)
    if band.dtype.kind not in "iu":
        raise ValueError("band must be an integer array of shape (P, 2) or one (lo, hi)")
    if band.shape == (2,):
        band = np.broadcast_to(band, (count, 2))
    if band.ndim != 2 or band.shape != (count, 2):
        raise ValueError(f"band must be one (lo, hi) or an integer array of shape (P, 2) = "
                         f"({count}, 2), one (lo, hi) per pair")
    if np.any(band[:, 0] > band[:, 1]):
        bad = int(np.argmax(band[:, 0] > band[:, 1]))
        raise ValueError(f"band of pair {bad} = ({int(band[bad, 0])}, {int(band[bad, 1])}): "
                         "lo <= hi is required")
    limit = native.GFY_ALIGN_ROWS_MAX
    return np.ascontiguousarray(np.clip(band, -limit, limit).astype(np.int32))


def _checked_box(box, count: int) -> np.ndarray | None:
    """``box`` as an int32 ``[count, 4]`` host array of ``(i_lo, i_hi, j_lo, j_hi)`` with ``i_lo <=
    i_hi`` and ``j_lo <= j_hi``, clipped into ``[-GFY_ALIGN_ROWS_MAX, GFY_ALIGN_ROWS_MAX]``; ``None``
    stays ``None`` (no box)."""
    if box is None:
        return None
    if isinstance(box, (tuple, list)) and any(isinstance(x, (bool, np.bool_)) for x in box):
        raise ValueError("box must hold integers (i_lo, i_hi, j_lo, j_hi)")
    box = _host_array(box)
    if box.size == 0 and count == 0 and box.ndim in (1, 2):
        box = np.zeros((0, 4), dtype=np.int64)
    if box.dtype.kind not in "iu":
        raise ValueError("box must be an integer array of shape (P, 4) or one (i_lo, i_hi, j_lo, "
                         "j_hi)")
    if box.shape == (4,):
        box = np.broadcast_to(box, (count, 4))
    if box.ndim != 2 or box.shape != (count, 4):
        raise ValueError(f"box must be one (i_lo, i_hi, j_lo, j_hi) or an integer array of shape "
                         f"(P, 4) = ({count}, 4), one box per pair")
    wrong = (box[:, 0] > box[:, 1]) | (box[:, 2] > box[:, 3])
    if np.any(wrong):
        bad = int(np.argmax(wrong))
        raise ValueError(f"box of pair {bad} = ({', '.join(str(int(x)) for x in box[bad])}): "
                         "i_lo <= i_hi and j_lo <= j_hi are required")
    limit = native.GFY_ALIGN_ROWS_MAX
    return np.ascontiguousarray(np.clip(box, -limit, limit).astype(np.int32))


def _checked_parameter(value, name: str) -> float:
    if value is None:
        raise ValueError(f"{name} is required: it has no default")
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(value)):
        raise ValueError(f"{name} must be a finite number")
    value = float(value)
    if abs(value) > float(np.finfo(np.float32).max):
        raise ValueError(f"{name} must be finite in float32")
    return value


class _Call(NamedTuple):
    """A checked call: the rows (``b`` is ``a`` where it was omitted), the records and pairs on
    both sides and the band and the box of every pair, or None; ``on_device`` adds the device
    arrays."""
    a: torch.Tensor
    b: torch.Tensor
    ptr_a: np.ndarray
    ptr_b: np.ndarray
    pairs: np.ndarray
    rows_b: np.ndarray
    parameters: tuple          # match_scale, match_shift, gap_open, gap_extend
    ptr_a_dev: torch.Tensor | None = None
    ptr_b_dev: torch.Tensor | None = None
    pairs_dev: torch.Tensor | None = None
    band: np.ndarray | None = None       # int32 [P, 2] of (lo, hi), clipped
    band_dev: torch.Tensor | None = None
    box: np.ndarray | None = None        # int32 [P, 4] of (i_lo, i_hi, j_lo, j_hi), clipped
    box_dev: torch.Tensor | None = None

    @property
    def box_columns(self) -> np.ndarray:
        """The columns of every pair's matrix: those of its box clipped into the b-record, or
        with no box the b-record's rows.  This is what a carry buffer has to hold."""
        if self.box is None:
            return self.rows_b
        columns = np.minimum(self.box[:, 3], self.rows_b - 1) - np.maximum(self.box[:, 2], 0) + 1
        return np.maximum(columns, 0)

    @property
    def box_rows(self) -> np.ndarray:
        """The rows of every pair's matrix: those of its box clipped into the a-record, or with
        no box the a-record's rows."""
        rows_a = np.diff(self.ptr_a)[self.pairs[:, 0]]
        if self.box is None:
            return rows_a
        return np.maximum(np.minimum(self.box[:, 1], rows_a - 1) - np.maximum(self.box[:, 0], 0) + 1, 0)

    @property
    def empty(self) -> bool:
        """No pair, or no pair with a row on both sides: nothing is launched."""
        return self.pairs.shape[0] == 0 or self.a.shape[0] == 0 or self.b.shape[0] == 0

    def on_device(self) -> "_Call":
        """The call with its rows on the device and, unless it is empty, its arrays next to
        them."""
        a = _prepare(self.a, None)
        b = a if self.b is self.a else _prepare(self.b, a.device)
        if self.empty:
            return self._replace(a=a, b=b)
        return self._replace(a=a, b=b,
                             ptr_a_dev=torch.from_numpy(self.ptr_a.astype(np.int32)).to(a.device),
                             ptr_b_dev=torch.from_numpy(self.ptr_b.astype(np.int32)).to(a.device),
                             pairs_dev=torch.from_numpy(self.pairs).to(a.device),
                             band_dev=None if self.band is None
                             else torch.from_numpy(self.band).to(a.device),
                             box_dev=None if self.box is None
                             else torch.from_numpy(self.box).to(a.device))

    def values(self) -> tuple:
        """The 14 values every alignment call of the C ABI starts with."""
        return (self.a.data_ptr(), self.a.shape[0], self.ptr_a_dev.data_ptr(), self.ptr_a.size - 1,
                self.b.data_ptr(), self.b.shape[0], self.ptr_b_dev.data_ptr(), self.ptr_b.size - 1,
                self.pairs_dev.data_ptr(), self.pairs.shape[0], *self.parameters)


#: the kinds of call and the symbol of each without a band or a box
_SYMBOLS = {"score": "gfy_align_local", "span": "gfy_align_local_span", "trace": "gfy_align_trace",
            "global": "gfy_align_global", "global_trace": "gfy_align_global_trace",
            "null": "gfy_align_local_null"}


def _symbol(call: _Call, kind: str, within: bool | None = None) -> tuple:
    """``(symbol, what it takes between gap_extend and its outputs)`` of a call of ``kind``, a key
    of ``_SYMBOLS``.  The local symbols take the band where the call has one (``*_band``), and
    with a box (``*_box``) the band or NULL and then the box; the trace of a local path takes no
    box (``start..end`` lies inside it).  The global symbols have no band: they take ``within``
    and behind it the box where the call has one.  The null scores have one symbol, which takes
    the band or NULL and the box or NULL."""
    name = _SYMBOLS[kind]
    # an empty call is never launched and has no device arrays: its pointers are None
    band, box = (None if x is None else x.data_ptr() for x in (call.band_dev, call.box_dev))
    boxed = call.box is not None and kind != "trace"
    if kind == "null":
        return name, (band, box)
    if kind in ("global", "global_trace"):
        return (name + "_box", (int(within), box)) if boxed else (name, (int(within),))
    if boxed:
        return name + "_box", (band, box)
    return (name, ()) if call.band is None else (name + "_band", (band,))


def _checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend, match_scale,
                  match_shift, band=None, box=None) -> _Call:
    """Every check the alignment functions share: the call, or the ``ValueError``.  No device is
    touched."""
    gap_open = _checked_parameter(gap_open, "gap_open")
    gap_extend = _checked_parameter(gap_extend, "gap_extend")
    match_scale = _checked_parameter(match_scale, "match_scale")
    match_shift = _checked_parameter(match_shift, "match_shift")
    if not 0.0 <= gap_extend <= gap_open:
        raise ValueError("0 <= gap_extend <= gap_open is required")
    a = _checked(a)
    if b is None:
        b, counts_b = a, counts_a if counts_b is None else counts_b
    else:
        b = _checked(b)
        if counts_b is None:
            raise ValueError("counts_b is required with b: record counts of b's rows")
    ptr_a = _record_ptr(counts_a, a.shape[0], "counts_a", "a")
    ptr_b = _record_ptr(counts_b, b.shape[0], "counts_b", "b")
    pairs = _checked_pairs(pairs, ptr_a.size - 1, ptr_b.size - 1)
    rows_a = np.diff(ptr_a)[pairs[:, 0]]
    rows_b = np.diff(ptr_b)[pairs[:, 1]]
    for side, rows, column in (("a", rows_a, 0), ("b", rows_b, 1)):
        if rows.size and rows.max() > native.GFY_ALIGN_ROWS_MAX:
            bad = int(np.argmax(rows > native.GFY_ALIGN_ROWS_MAX))
            raise ValueError(f"pair {bad}: record {int(pairs[bad, column])} of {side} has "
                             f"{int(rows[bad])} rows, more than {native.GFY_ALIGN_ROWS_MAX}")
    return _Call(a, b, ptr_a, ptr_b, pairs, rows_b,
                 (match_scale, match_shift, gap_open, gap_extend),
                 band=_checked_band(band, pairs.shape[0]), box=_checked_box(box, pairs.shape[0]))


def _launch(call: _Call, kind: str, within, workspace) -> tuple:
    """The one score launch of a call that is ``on_device``: the symbol of ``kind`` ("score",
    "span" or "global", the last with ``within``) with the call's arguments in front of the
    outputs, its workspace sized for the widest matrix of the call.  "span" gives ``(scores,
    starts, ends)``, the others ``(scores, ends)``; an empty call gives its results without a
    launch."""
    device, count, span = call.a.device, call.pairs.shape[0], kind == "span"
    sizer = "gfy_align_span_workspace_bytes" if span else "gfy_align_workspace_bytes"
    with torch.cuda.device(device):
        scores = torch.zeros(count, dtype=torch.float32, device=device)
        ends = torch.full((count, 2), -1, dtype=torch.int32, device=device)
        starts = torch.full((count, 2), -1, dtype=torch.int32, device=device) if span else None
        outputs = (scores, starts, ends) if span else (scores, ends)
        if not call.empty:
            lib, (name, front) = native.library(), _symbol(call, kind, within)
            need = getattr(lib, sizer)(count, int(call.box_columns.max()))
            scratch = (workspace or AlignWorkspace()).buffer(device, need)
            native.check(getattr(lib, name)(
                *call.values(), *front, *(out.data_ptr() for out in outputs),
                *_scratch_tail(scratch, device)), name)
    return outputs


def local_align(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                match_scale=1.0, match_shift=0.0, band=None, box=None,
                workspace: AlignWorkspace | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Local alignment of the record pairs ``pairs``: ``(scores float32 [P], ends int32 [P, 2])``
    on the device, exact, the ``Lq x Lr`` matrix of a pair never written (the definition is at
    the head of this module; it is this project's own and not ``ginfinity-sw``'s).

    ``a`` / ``b`` are fp16 ``[rows, 128]`` embeddings as ``distance.pairwise`` takes them,
    ``counts_a`` / ``counts_b`` the row counts of their contiguous records.  With ``b`` omitted
    ``a`` is aligned against itself and ``counts_b`` defaults to ``counts_a``; nothing is
    excluded, ``(q, q)`` aligns a record with itself.  ``pairs`` is an integer ``[P, 2]`` array
    (numpy or torch, on any device) of (record of ``a``, record of ``b``); ``top_pairs`` makes
    one from ``distance.record_scores``.  The substitution score of two rows is
    ``cosine * match_scale + match_shift`` (two rounded float32 operations); ``gap_open`` (the
    cost of a gap's first position) and ``gap_extend`` are required, ``0 <= gap_extend <=
    gap_open``.

    ``band=None`` aligns in the whole matrix.  Otherwise ``band`` is an integer array ``[P, 2]``
    (numpy or torch, on any device) of ``(lo, hi)`` per pair, or one ``(lo, hi)`` for every pair:
    only cells on the diagonals ``lo <= j - i <= hi`` exist (the head of this module says what
    that means, ``band_around`` makes bands from seeds), and the columns of a strip outside the
    band cost nothing.  Values are clipped into ``+-GFY_ALIGN_ROWS_MAX``, which covers any matrix.

    ``box=None`` aligns the two whole records.  Otherwise ``box`` is an integer array ``[P, 4]``
    (numpy or torch, on any device) of ``(i_lo, i_hi, j_lo, j_hi)`` per pair, or one such tuple for
    every pair: only the cells of rows ``i_lo .. i_hi`` of the a-record and ``j_lo .. j_hi`` of the
    b-record exist, both ends inclusive (the head of this module says what that means,
    ``Runs.boxes`` and ``Chains.boxes`` make boxes from seeds), and the strips outside the box
    cost nothing.  Values are clipped into ``+-GFY_ALIGN_ROWS_MAX`` and the box into the two
    records; a box that then holds no cell gives score 0 and ``(-1, -1)``.  ``band`` keeps its
    meaning with a box, and ``ends`` stay in the records' coordinates.

    Every argument error is a ``ValueError`` before a device is touched: a pair out of range, a
    record named by a pair with more than ``GFY_ALIGN_ROWS_MAX`` rows, a parameter that is not
    finite or out of order, a band that is not integer, of another shape, or with ``lo > hi``,
    a box that is not integer, of another shape, or with ``i_lo > i_hi`` or ``j_lo > j_hi``.
    ``P == 0`` returns empty tensors without a launch."""
    return _launch(_checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend,
                                 match_scale, match_shift, band, box).on_device(), "score", None,
                   workspace)


def local_spans(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                match_scale=1.0, match_shift=0.0, band=None, box=None,
                workspace: AlignWorkspace | None = None
                ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``local_align`` with the start cell of every alignment: ``(scores float32 [P], starts
    int32 [P, 2], ends int32 [P, 2])`` on the device.  Rows ``starts[p, 0] .. ends[p, 0]`` of the
    a-record and ``starts[p, 1] .. ends[p, 1]`` of the b-record are the stretch that takes part
    (the origin rules are at the head of this module).  Scores and ends are those of
    ``local_align`` bit for bit; a score of 0 gives a start of ``(-1, -1)``.

    The arguments (``band`` and ``box`` among them; ``starts`` too stay in the records'
    coordinates), their checks and the ``ValueError``s are those of
    ``local_align``; an ``AlignWorkspace`` serves both functions (this one needs twice the
    bytes)."""
    return _launch(_checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend,
                                 match_scale, match_shift, band, box).on_device(), "span", None,
                   workspace)


class AlignedPaths(NamedTuple):
    """What ``local_paths`` returns, all on the device: pair p's path is
    ``ops[offsets[p]:offsets[p + 1]]``."""
    scores: torch.Tensor    # float32 [P]
    starts: torch.Tensor    # int32 [P, 2]
    ends: torch.Tensor      # int32 [P, 2]
    ops: torch.Tensor       # uint8 [offsets[P]]: 0 match, 1 gap facing a row of b, 2 facing one of a
    offsets: torch.Tensor   # int64 [P + 1]


def local_paths(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                match_scale=1.0, match_shift=0.0, band=None, box=None,
                workspace: AlignWorkspace | None = None,
                max_workspace_bytes: int = 2 << 30) -> AlignedPaths:
    """``local_spans`` with the aligned path of every pair: ``AlignedPaths(scores, starts, ends,
    ops, offsets)`` on the device.  ``ops`` (uint8, all pairs one after the other) holds each
    path in forward order, ``start`` to ``end``: ``0`` a row of the a-record matched with a row of
    the b-record, ``1`` a row of the b-record facing a gap, ``2`` a row of the a-record facing a
    gap (the walk is at the head of this module); ``offsets`` (int64 ``[P + 1]``) says where a
    pair's ops lie, and ``path_cells`` turns them into row pairs.  Scores, starts and ends are
    those of ``local_spans`` bit for bit; a score of 0 has an empty path.

    Two launches with a copy to the host between them: the ``local_spans`` launch, then
    ``starts`` and ``ends`` (``P x 4`` integers) come to the host — which waits for the device —
    to size each pair's slot and the largest box, then the trace launch on the boxes.  The trace
    keeps 4 bits per cell of a box per wave in flight (8 MB for a 4096 x 4096 box); it is given
    ``min(what all waves need, max_workspace_bytes)`` bytes and fewer waves share the work where
    that is less.  The default, 2 GiB, is a choice: a quarter of what the widest launch needs in
    the worst case, and still a wave per compute unit.  A ``max_workspace_bytes`` below one wave's
    need for the largest box of the call is refused by the library (``NativeLibraryError``).

    The other arguments, their checks and the ``ValueError``s are those of ``local_spans``;
    with a ``band`` both launches get the same array (the trace shifts it into each box itself).
    A ``box`` goes to the span launch alone: ``start..end`` lies inside it, so the trace on
    ``start..end`` walks the same path without it.
    An ``AlignWorkspace`` serves all three functions.  ``P == 0``, or a call with no rows, returns
    empty tensors without a launch."""
    max_workspace_bytes = _checked_cap(max_workspace_bytes)
    call = _checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend, match_scale,
                         match_shift, band, box).on_device()
    scores, starts, ends = _launch(call, "span", None, workspace)
    with torch.cuda.device(scores.device):
        box = (ends - starts + 1).cpu().numpy().astype(np.int64)    # waits for the span launch
        box[starts.cpu().numpy()[:, 0] < 0] = 0                     # nothing aligned: no box
        slots = np.maximum(box.sum(axis=1) - 1, 0)                  # rows + cols - 1 ops at most
        name, front = _symbol(call, "trace")

        def trace(lib, slot_ptr, slot_ops, lengths, *rest):   # rest: box, workspace, stream
            return getattr(lib, name)(*call.values(), *front, starts.data_ptr(), ends.data_ptr(),
                                      slot_ptr, slot_ops, lengths, *rest)
        return _traced(call, name, trace, "gfy_align_trace_workspace_bytes",
                       f"{name} refused a box of its span call", scores, starts, ends, slots, box,
                       max_workspace_bytes, workspace)


def _traced(call: _Call, name: str, trace, sizer: str, refusal: str, scores, starts, ends,
            slots: np.ndarray, boxes: np.ndarray, cap: int, workspace) -> AlignedPaths:
    """The trace launch behind ``local_paths`` and ``global_paths`` and what it returns.  Pair p
    owns ``slots[p]`` ops and has a box of ``boxes[p]`` (rows, columns); ``trace(lib, slot_ptr,
    slot_ops, lengths, box_rows, box_cols, scratch, bytes, stream)`` calls the symbol ``name``
    with the call site's own arguments in front, on ``min(what the symbol sizer asks for, cap)``
    bytes.  A negative length is ``refusal``."""
    device, count = scores.device, scores.shape[0]
    slot_ptr = np.concatenate(([0], np.cumsum(slots)))
    if call.empty or slot_ptr[-1] == 0:                             # every path is empty
        return AlignedPaths(scores, starts, ends,
                            torch.zeros(0, dtype=torch.uint8, device=device),
                            torch.zeros(count + 1, dtype=torch.int64, device=device))
    lib = native.library()
    box_rows, box_cols = int(boxes[:, 0].max()), int(boxes[:, 1].max())
    need = min(getattr(lib, sizer)(count, box_rows, box_cols), cap)
    scratch = (workspace or AlignWorkspace()).buffer(device, need)
    slot_ptr_dev = torch.from_numpy(slot_ptr).to(device)
    slot_ops = torch.empty(int(slot_ptr[-1]), dtype=torch.uint8, device=device)
    lengths = torch.zeros(count, dtype=torch.int32, device=device)
    native.check(trace(lib, slot_ptr_dev.data_ptr(), slot_ops.data_ptr(), lengths.data_ptr(),
                       box_rows, box_cols, *_scratch_tail(scratch[:need], device)), name)
    if bool((lengths < 0).any()):
        raise native.NativeLibraryError(refusal)
    return AlignedPaths(scores, starts, ends, *_compacted(slot_ops, slot_ptr_dev, slots, lengths))


def _compacted(slot_ops, slot_ptr_dev, slots: np.ndarray, lengths) -> tuple:
    """``(ops, offsets)`` of traced slots: the front ``lengths[p]`` of every slot, one after the
    other.  Not the hot path."""
    device, count = slot_ops.device, lengths.shape[0]
    lengths = lengths.to(torch.int64)
    offsets = torch.cat([lengths.new_zeros(1), torch.cumsum(lengths, 0)])
    owner = torch.repeat_interleave(torch.arange(count, device=device),
                                    torch.from_numpy(slots).to(device))
    inside = torch.arange(slot_ops.shape[0], device=device) - slot_ptr_dev[owner]
    return slot_ops[inside < lengths[owner]], offsets


def _checked_within(within) -> bool:
    if not isinstance(within, (bool, np.bool_)):
        raise ValueError("within must be True (query-in-target) or False (global)")
    return bool(within)


def _checked_cap(max_workspace_bytes) -> int:
    return _checked_integer(max_workspace_bytes, "max_workspace_bytes", 1)


def global_align(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                 match_scale=1.0, match_shift=0.0, within: bool = False, box=None,
                 workspace: AlignWorkspace | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Global (``within=False``) or query-in-target (``within=True``) alignment of the record
    pairs ``pairs``: ``(scores float32 [P], ends int32 [P, 2])`` on the device, exact, the ``Lq x
    Lr`` matrix of a pair never written (the definition is at the head of this module).  Global:
    both records take part end to end and ``end`` is ``(Lq - 1, Lr - 1)``.  ``within``: all of the
    a-record is aligned inside the b-record, whose rows in front of and behind the alignment are
    free; ``end`` is ``(Lq - 1, j)`` for the first best j.  Scores may be negative; a pair with a
    record of zero rows on either side has nothing to align and gives 0 and ``(-1, -1)``.
    ``global <= within <= local_align`` holds for the scores of any pair, exactly.

    ``box=None`` aligns the two whole records.  Otherwise ``box`` is what ``local_align`` takes,
    an integer array ``[P, 4]`` of ``(i_lo, i_hi, j_lo, j_hi)`` per pair or one such tuple for every
    pair, and **the box is the matrix**: rows ``i_lo .. i_hi`` of the a-record and ``j_lo .. j_hi``
    of the b-record are aligned as two records of their own (the head of this module says what
    follows from that; ``Chains.boxes(0)`` is the stretch from a chain's first cell to its
    last), and the strips outside the box cost nothing.  ``ends`` stay in the records'
    coordinates: ``(i_hi, j_hi)`` of the box clipped into the records, or with ``within`` ``(i_hi,
    j)`` for the first best j in ``j_lo .. j_hi``.  A box that holds no cell after clipping has
    nothing to align: 0 and ``(-1, -1)``.  There is no ``band`` on these modes.

    The other arguments, their checks and the ``ValueError``s are those of ``local_align``
    (``box`` and its texts included); ``within`` must be a bool.  An ``AlignWorkspace`` serves
    this function too."""
    within = _checked_within(within)
    return _launch(_checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend,
                                 match_scale, match_shift, None, box).on_device(), "global", within,
                   workspace)


def global_paths(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                 match_scale=1.0, match_shift=0.0, within: bool = False, box=None,
                 workspace: AlignWorkspace | None = None,
                 max_workspace_bytes: int = 2 << 30) -> AlignedPaths:
    """``global_align`` with the aligned path of every pair: ``AlignedPaths(scores, starts, ends,
    ops, offsets)`` on the device, ops and offsets as ``local_paths`` returns them.  The path
    takes in every row of the a-record, and of the b-record every row (global) or rows ``start_j
    .. end_j`` (``within``); the border it ends on is part of it (the walk is at the head of this
    module), so a path has up to ``Lq + Lr`` ops and may consist of gaps alone.  ``starts[p]`` is
    ``(0, 0)`` for global and ``(0, start_j)`` for ``within``, where ``start_j = end_j + 1`` if no
    row of the b-record is consumed; ``path_cells(ops, start)`` gives the cells.  Scores and ends
    are those of ``global_align`` bit for bit; a pair with nothing to align has start and end
    ``(-1, -1)`` and an empty path.

    Two launches and no copy to the host between them: every slot (``Lq + Lr`` ops) and the
    largest box are known from the counts, and the trace launch reads the ends of the first one
    on the device.  The workspace of the trace and ``max_workspace_bytes`` are those of
    ``local_paths``, the boxes being the records' own sizes.

    With a ``box`` (``global_align`` says what it is) the path is that of the box's rows taken as
    two records of their own, in the records' coordinates: ``starts[p]`` is ``(i_lo, j_lo)`` of the
    clipped box for global and ``(i_lo, start_j)`` for ``within``, a path has up to ``box rows +
    box columns`` ops, and both launches get the same boxes.  Slots and the largest box come from
    the boxes clipped on the host, so there is still no copy between the launches.

    The other arguments, their checks and the ``ValueError``s are those of ``global_align``."""
    within = _checked_within(within)
    cap = _checked_cap(max_workspace_bytes)
    call = _checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend, match_scale,
                         match_shift, None, box).on_device()
    scores, ends = _launch(call, "global", within, workspace)
    device, count = scores.device, scores.shape[0]
    with torch.cuda.device(device):
        starts = torch.full((count, 2), -1, dtype=torch.int32, device=device)
        rows_a, rows_b = call.box_rows.astype(np.int64), call.box_columns.astype(np.int64)
        both = (rows_a > 0) & (rows_b > 0)
        slots = np.where(both, rows_a + rows_b, 0)           # rows + columns ops at most
        name, front = _symbol(call, "global_trace", within)

        def trace(lib, slot_ptr, slot_ops, lengths, *rest):   # rest: box, workspace, stream
            return getattr(lib, name)(*call.values(), *front, ends.data_ptr(), slot_ptr, slot_ops,
                                      lengths, starts.data_ptr(), *rest)
        return _traced(call, name, trace, "gfy_align_global_trace_workspace_bytes",
                       f"{name} refused an end of its score call", scores, starts, ends, slots,
                       np.stack([rows_a, rows_b], axis=1), cap, workspace)


class PathValues(NamedTuple):
    """What ``path_values`` returns, all on the device: the per-op values of pair p are
    ``cosines[offsets[p]:offsets[p + 1]]`` and ``running[offsets[p]:offsets[p + 1]]``."""
    cosines: torch.Tensor       # float32 [offsets[P]]: the cosine of a matched cell, NaN at a gap op
    running: torch.Tensor       # float32 [offsets[P]]: the score behind every op
    scores: torch.Tensor        # float32 [P]: the last running value, 0 for an empty path
    matches: torch.Tensor       # int32 [P]: ops 0
    gap_runs: torch.Tensor      # int32 [P, 2]: runs of op 1, runs of op 2
    cosine_sums: torch.Tensor   # float64 [P]: the matched cosines added in path order
    status: torch.Tensor        # int32 [P]: 0, or -2 for a path that was refused
    offsets: torch.Tensor       # int64 [P + 1]: the offsets of the paths

    def mean_cosine(self) -> torch.Tensor:
        """``cosine_sums / matches`` in float64 ``[P]``, NaN where nothing matched (and for a
        path that was refused)."""
        matched = self.matches > 0
        return torch.where(matched, self.cosine_sums / self.matches.clamp(min=1).to(torch.float64),
                           torch.full_like(self.cosine_sums, float("nan")))

    def of(self, p: int) -> tuple[torch.Tensor, torch.Tensor]:
        """``(cosines, running)`` of pair p: the two per-op slices (reads two offsets, which
        waits for the device)."""
        lo, hi = (int(x) for x in self.offsets[p:p + 2].tolist())
        return self.cosines[lo:hi], self.running[lo:hi]


def _checked_paths(paths, count: int) -> tuple:
    """``(starts, ops, offsets)`` of ``paths`` as tensors wherever they live, or the
    ``ValueError``.  No device is touched: of arrays on a device only type and shape are looked
    at, and what they hold is the kernel's to check."""
    tensors = []
    for name in ("starts", "ops", "offsets"):
        try:
            values = getattr(paths, name)
        except AttributeError:
            raise ValueError("paths must have starts, ops and offsets (an AlignedPaths, or any "
                             "object with these three)") from None
        if isinstance(values, np.ndarray):
            values = torch.from_numpy(np.ascontiguousarray(values))
        if not isinstance(values, torch.Tensor):
            raise ValueError(f"paths.{name} must be a numpy array or a torch tensor")
        tensors.append(values)
    starts, ops, offsets = tensors
    if ops.dtype != torch.uint8 or ops.dim() != 1:
        raise ValueError("paths.ops must be a one-dimensional uint8 array of 0, 1 and 2")
    if offsets.dtype != torch.int64 or offsets.shape != (count + 1,):
        raise ValueError(f"paths.offsets must be an int64 array of shape (P + 1,) = ({count + 1},)")
    if offsets.device.type == "cpu" and (int(offsets[0]) != 0 or int(offsets[-1]) != ops.shape[0]):
        raise ValueError(f"paths.offsets must start at 0 and end at ops.shape[0] = {ops.shape[0]}, "
                         f"not run from {int(offsets[0])} to {int(offsets[-1])}")
    if starts.dtype != torch.int32 or starts.shape != (count, 2):
        raise ValueError(f"paths.starts must be an int32 array of shape (P, 2) = ({count}, 2)")
    return starts, ops, offsets


def path_values(paths, a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                match_scale=1.0, match_shift=0.0, max_waves: int | None = None) -> PathValues:
    """The values along aligned paths, without leaving the device: ``PathValues(cosines, running,
    scores, matches, gap_runs, cosine_sums, status, offsets)``.

    ``paths`` is what ``local_paths`` or ``global_paths`` returned for the same rows, counts,
    pairs and parameters, or any object with ``starts`` (int32 ``[P, 2]``, the cell where each path
    starts, in the records' coordinates), ``ops`` (uint8, all paths one after the other) and
    ``offsets`` (int64 ``[P + 1]``), numpy or torch, on any device: a caller may hand in paths of
    their own.  Op ``0`` consumes cell ``(i, j)`` and moves to ``(i + 1, j + 1)``, op ``1`` moves to
    ``(i, j + 1)``, op ``2`` to ``(i + 1, j)``, as ``path_cells`` reads them.  There is no ``band`` and
    no ``box``: the starts already are in the records' coordinates.

    * ``cosines``: at an op ``0`` at ``(i, j)`` the cosine ``distance.pairwise(A, B,
      metric="cosine")[i, j]`` of the pair's two records, bit for bit, and NaN at a gap op.  The
      dense ``Lq x Lr`` matrix is not written.
    * ``running``: the score behind every op under the re-scoring rule at the head of this module
      (``h = 0``; op 0 adds ``s[i][j]``; the first op of a run of equal gap ops takes ``gap_open``,
      each further one ``gap_extend``), every operation one rounded float32 operation.
    * ``scores``: the last running value, 0 for an empty path.  For a path that one of the
      aligners returned this is that aligner's score bit for bit (only a zero keeps no promise
      of its sign).
    * ``matches``, ``gap_runs``: the ops ``0``, and the runs of op ``1`` and of op ``2`` (op ``1``
      behind op ``2`` starts a new run).
    * ``cosine_sums``: the matched cosines added one at a time in float64 in path order;
      ``values.mean_cosine()`` divides it by ``matches``.  Matched counts, gap runs and cosine sums
      are what a normalisation of scores starts from.

    A path is REFUSED where the kernel cannot follow it: a start with a negative coordinate other
    than ``(-1, -1)`` (where only an empty path may start), an op byte above 2, a path that names
    a cell outside its two records, offsets on the device that decrease or leave ``ops``.  A
    refused path has ``status`` -2, NaN in all its per-op values, in its score and in its sum.
    This is reported through ``status`` and NOT raised: reading it back would make the call wait
    for the device.  The other paths of the call are not affected, and a path's values depend
    neither on its company, nor on the order of the paths, nor on ``max_waves``.

    ``max_waves=None`` leaves the number of waves to the library (one per path, up to 4,096); a
    positive integer bounds it, and the waves take the paths in turn.

    Every argument error is a ``ValueError`` before a device is touched: those of
    ``local_align`` (without ``band`` and ``box``), ``ops`` that is not one-dimensional uint8,
    ``offsets`` that is not int64 ``[P + 1]`` — or, where it lives on the host, does not start at 0
    or end at ``ops.shape[0]`` —, ``starts`` that is not int32 ``[P, 2]``.  ``P == 0``, or every
    path empty, returns empty or zero tensors without a launch."""
    if max_waves is not None:
        max_waves = _checked_integer(max_waves, "max_waves", 1)
    call = _checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend, match_scale,
                         match_shift)
    count = call.pairs.shape[0]
    starts, ops, offsets = _checked_paths(paths, count)
    call = call.on_device()
    device, total = call.a.device, ops.shape[0]
    with torch.cuda.device(device):
        starts, ops, offsets = (x.to(device).contiguous() for x in (starts, ops, offsets))
        # NaN where the kernel writes nothing: the ops of a slot that it refuses
        cosines = torch.full((total,), float("nan"), dtype=torch.float32, device=device)
        running = torch.full((total,), float("nan"), dtype=torch.float32, device=device)
        scores = torch.zeros(count, dtype=torch.float32, device=device)
        counts = torch.zeros((count, 4), dtype=torch.int32, device=device)
        sums = torch.zeros(count, dtype=torch.float64, device=device)
        if call.empty and total and count:
            # no row to align with: a path with ops names cells that do not exist.  torch.where,
            # not an assignment under a mask, which would wait for the device
            refused = offsets[1:] > offsets[:-1]
            scores = torch.where(refused, torch.full_like(scores, float("nan")), scores)
            sums = torch.where(refused, torch.full_like(sums, float("nan")), sums)
            counts[:, 3] = torch.where(refused, -2, 0).to(torch.int32)
        elif total and count:
            name = "gfy_align_path_values"
            native.check(getattr(native.library(), name)(
                *call.values(), starts.data_ptr(), offsets.data_ptr(), ops.data_ptr(), total,
                cosines.data_ptr(), running.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                sums.data_ptr(), max_waves or 0, torch.cuda.current_stream(device).cuda_stream),
                name)
    return PathValues(cosines, running, scores, counts[:, 0], counts[:, 1:3], sums, counts[:, 3],
                      offsets)


_WORD = 1 << 64
_GOLDEN = 0x9E3779B97F4A7C15
_MIX_1, _MIX_2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _signed(word: int) -> int:
    """The int64 with the bits of ``word`` modulo 2^64: torch has no uint64 arithmetic, and int64
    products and sums wrap to the same bits."""
    word %= _WORD
    return word - _WORD if word >= 1 << 63 else word


def _shifted(z: torch.Tensor, bits: int) -> torch.Tensor:
    """``z >> bits`` of the 64-bit pattern, logical: int64's own shift copies the sign."""
    return (z >> bits) & ((1 << (64 - bits)) - 1)


def _mixed(z: torch.Tensor) -> torch.Tensor:
    """``mix`` of the head of this module on int64 tensors, bit for bit what uint64 gives."""
    z = (z ^ _shifted(z, 30)) * _signed(_MIX_1)
    z = (z ^ _shifted(z, 27)) * _signed(_MIX_2)
    return z ^ _shifted(z, 31)


def _checked_columns(columns) -> np.ndarray:
    columns = _host_array(columns)
    if columns.size == 0 and columns.ndim == 1:
        columns = np.zeros(0, dtype=np.int64)
    if columns.ndim != 1 or columns.dtype.kind not in "iu" or (columns.size and columns.min() < 0):
        raise ValueError("columns must be a one-dimensional array of non-negative integers, the "
                         "rows of every pair's b-side")
    return columns.astype(np.int64)


def shuffle_orders(columns, shuffles, seed, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """The orders of a null: for every pair p ``shuffles`` uniform-looking permutations of ``0 ..
    columns[p] - 1``, as ``(order int32, order_ptr int64 [P + 1])`` the way ``null_scores`` and
    ``gfy_align_local_null`` take them: pair p's orders lie back to back from ``order_ptr[p]``,
    ``columns[p]`` entries each, ``order_ptr[p] = shuffles * sum(columns[:p])``.

    The result is a fixed function of ``(seed, v, j)``, ``v = p * shuffles + k`` (the formula is
    at the head of this module and in include/gfy.h): the entries of virtual pair v are ``0 ..
    columns[p] - 1`` stably sorted by ``(key(seed, v, j), j)``, so a segment depends on its own
    ``(seed, v)`` and length alone, not on what stands before or behind it, and numpy ``uint64``
    reproduces it.  No ``torch.Generator`` is used.  ``seed`` is any integer, taken modulo 2^64.

    ``device=None`` gives CPU tensors; on a device the scans and the one stable sort run there,
    and the bytes are the same.  ``columns`` is a host array (a list, numpy, or a torch tensor,
    which is copied to the host); ``P * shuffles`` must stay below 2^31."""
    columns = _checked_columns(columns)
    shuffles = _checked_integer(shuffles, "shuffles", 1)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("seed must be an integer")
    virtual = columns.size * shuffles
    if virtual >= 2 ** 31:
        raise ValueError(f"P * shuffles = {columns.size} * {shuffles} must stay below 2^31")
    device = torch.device("cpu" if device is None else device)
    total = int(columns.sum()) * shuffles
    order_ptr = torch.from_numpy(np.concatenate(([0], np.cumsum(columns) * shuffles))).to(device)
    if total == 0:
        return torch.zeros(0, dtype=torch.int32, device=device), order_ptr
    lengths = torch.from_numpy(np.repeat(columns, shuffles)).to(device)          # [P * shuffles]
    first = torch.cumsum(lengths, 0) - lengths
    v = torch.repeat_interleave(torch.arange(virtual, device=device), lengths, output_size=total)
    j = torch.arange(total, device=device) - first[v]
    keys = _mixed(_mixed((v + 1) * _signed(_GOLDEN) + _signed(int(seed)))
                  + (j + 1) * _signed(_GOLDEN))
    # one stable sort by (virtual pair, key, j): the elements stand in (virtual pair, j) order
    where = torch.sort((v << 32) | _shifted(keys, 32), stable=True).indices
    return j[where].to(torch.int32), order_ptr


def _checked_orders(orders, columns: np.ndarray, shuffles: int) -> tuple:
    """``orders`` as ``(order, order_ptr)`` tensors wherever they live, or the ``ValueError``.  Of
    arrays only type and shape are looked at: what they hold is the kernel's to check."""
    if not isinstance(orders, (tuple, list)) or len(orders) != 2:
        raise ValueError("orders must be a pair (order, order_ptr), as shuffle_orders returns it")
    tensors = []
    for values, name in zip(orders, ("order", "order_ptr")):
        if isinstance(values, np.ndarray):
            values = torch.from_numpy(np.ascontiguousarray(values))
        if not isinstance(values, torch.Tensor):
            raise ValueError(f"orders: {name} must be a numpy array or a torch tensor")
        tensors.append(values)
    order, order_ptr = tensors
    total = int(columns.sum()) * shuffles
    if order.dtype != torch.int32 or order.shape != (total,):
        raise ValueError(f"orders: order must be an int32 array of shape (shuffles * the columns "
                         f"of all pairs,) = ({total},)")
    if order_ptr.dtype != torch.int64 or order_ptr.shape != (columns.size + 1,):
        raise ValueError(f"orders: order_ptr must be an int64 array of shape (P + 1,) = "
                         f"({columns.size + 1},)")
    return order, order_ptr


def null_scores(a, b=None, *, counts_a, counts_b=None, pairs, gap_open, gap_extend,
                match_scale=1.0, match_shift=0.0, band=None, box=None, shuffles=None, seed=0,
                orders=None, workspace: AlignWorkspace | None = None) -> torch.Tensor:
    """The null of ``local_align``: every pair aligned ``shuffles`` times against its own b-side
    with the rows in another order each time, ``float32 [P, shuffles]`` on the device, in one
    launch and without a shuffled row being written (the head of this module says why and how).

    The arguments of ``local_align`` keep their meaning, ``band`` and ``box`` included: the
    b-side of a pair is its b-record, or with a ``box`` rows ``j_lo .. j_hi`` of it (clipped), and
    only those are shuffled, among themselves.  ``shuffles`` is required and has no default
    worth having: it decides the resolution of everything ``significance`` makes of the result.
    ``seed`` names the orders (``shuffle_orders(call's columns, shuffles, seed)``, made on the
    device).  ``orders=(order, order_ptr)`` replaces them with the caller's own, in the layout
    ``shuffle_orders`` documents: a reversal, a bootstrap with repeats, or the identity, under
    which the result is ``local_align``'s score.  Result ``[p, k]`` equals, bit for bit,
    ``local_align`` of pair p with its b-side replaced by the rows ``order[...]`` copied out in
    the order of run k, and depends neither on the other pairs or runs of the call nor on the
    workspace.

    Every argument error is a ``ValueError`` before a device is touched: those of
    ``local_align``, a ``shuffles`` that is missing or no positive integer, ``P * shuffles`` of
    2^31 or more, a ``seed`` that is no integer, ``orders`` that is no pair of an int32 array of
    ``shuffles * sum(columns)`` entries and an int64 array of ``P + 1``.  What ``orders`` HOLDS is
    not read here, because that would wait for the device: a pair whose ``order_ptr`` does not
    step by ``shuffles * columns`` gets NaN in all its runs, a run with an entry outside ``0 ..
    columns - 1`` gets NaN, and nothing outside the arrays is read for either.  ``P == 0``
    returns ``[0, shuffles]`` without a launch; an ``AlignWorkspace`` serves this function too."""
    if shuffles is None:
        raise ValueError("shuffles is required: it has no default")
    shuffles = _checked_integer(shuffles, "shuffles", 1)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("seed must be an integer")
    call = _checked_call(a, b, counts_a, counts_b, pairs, gap_open, gap_extend, match_scale,
                         match_shift, band, box)
    count = call.pairs.shape[0]
    if count * shuffles >= 2 ** 31:
        raise ValueError(f"P * shuffles = {count} * {shuffles} must stay below 2^31")
    columns = call.box_columns.astype(np.int64)
    if orders is not None:
        orders = _checked_orders(orders, columns, shuffles)
    call = call.on_device()
    device = call.a.device
    with torch.cuda.device(device):
        scores = torch.zeros((count, shuffles), dtype=torch.float32, device=device)
        if call.empty:
            return scores
        order, order_ptr = orders if orders is not None else \
            shuffle_orders(columns, shuffles, seed, device)
        order, order_ptr = order.to(device).contiguous(), order_ptr.to(device).contiguous()
        if order.numel() == 0:                   # no b-side has a row: NULL is no array
            order = torch.zeros(1, dtype=torch.int32, device=device)
        lib, (name, front) = native.library(), _symbol(call, "null")
        need = lib.gfy_align_workspace_bytes(count * shuffles, int(columns.max()))
        scratch = (workspace or AlignWorkspace()).buffer(device, need)
        native.check(getattr(lib, name)(
            *call.values(), *front,
            shuffles, order.data_ptr(), order_ptr.data_ptr(), scores.data_ptr(),
            *_scratch_tail(scratch, device)), name)
    return scores


class Significance(NamedTuple):
    """What ``significance`` returns: float64 ``[P]`` tensors on the device of ``null``."""
    z: torch.Tensor          # (score - mean) / std
    mean: torch.Tensor       # of the pair's null scores
    std: torch.Tensor        # their K - 1 standard deviation
    p_value: torch.Tensor    # P(a null score >= score) under the fitted Gumbel distribution
    lam: torch.Tensor        # the Gumbel scale parameter lambda
    mu: torch.Tensor         # the Gumbel location


_EULER_GAMMA = 0.5772156649015329


def significance(scores, null) -> Significance:
    """The real ``scores`` (``[P]``) against their ``null`` scores (``[P, K]``, ``K >= 2``, what
    ``null_scores`` returned): ``Significance(z, mean, std, p_value, lam, mu)``, float64 ``[P]``
    tensors on the device of ``null``.  All in float64, per row of ``null``:

        mean    = sum(null) / K
        std     = sqrt(sum((null - mean)^2) / (K - 1))
        z       = (score - mean) / std
        lam     = pi / (std * sqrt(6))                   the Gumbel fit by moments
        mu      = mean - gamma / lam                     gamma = 0.5772156649015329
        p_value = -expm1(-exp(-lam * (score - mu)))      = 1 - exp(-exp(-lam (score - mu)))

    The best local score of unrelated sequences follows an extreme-value (Gumbel) distribution,
    which is why the p-value is read off a Gumbel fitted to the null and not off a normal one;
    ``z`` is the plain distance in standard deviations.  These are ESTIMATES FROM K SAMPLES, and K
    decides their resolution: the mean and the deviation carry a relative error of about
    ``1 / sqrt(K)`` and ``1 / sqrt(2 K)``, and a p-value far below ``1 / K`` is an extrapolation
    of the fitted tail that no sample has seen.

    Nothing is raised for what the numbers hold.  Where ``std == 0`` (a constant row) the
    results are the plain IEEE ones: ``z`` is ``+-inf`` or NaN, ``lam`` is ``inf``, ``mu == mean``,
    ``p_value`` is 0 above the mean, 1 below it and NaN on it.  A NaN in a row of ``null`` (a
    refused pair) makes all six NaN for that row; a NaN score makes its ``z`` and ``p_value`` NaN.
    ``K < 2``, or shapes that do not match, are a ``ValueError``."""
    if isinstance(null, np.ndarray):
        null = torch.from_numpy(np.ascontiguousarray(null))
    if not isinstance(null, torch.Tensor) or null.dim() != 2 or not null.dtype.is_floating_point:
        raise ValueError("null must be a floating-point array of shape (P, K)")
    if null.shape[1] < 2:
        raise ValueError(f"null must hold at least 2 scores per pair, not K = {null.shape[1]}: "
                         "one sample has no deviation")
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(np.ascontiguousarray(scores))
    if not isinstance(scores, torch.Tensor) or scores.shape != (null.shape[0],) \
            or not scores.dtype.is_floating_point:
        raise ValueError(f"scores must be a floating-point array of shape (P,) = "
                         f"({null.shape[0]},), one score per row of null")
    null = null.to(torch.float64)
    scores = scores.to(device=null.device, dtype=torch.float64)
    count = null.shape[1]
    mean = null.sum(dim=1) / count
    std = torch.sqrt(((null - mean[:, None]) ** 2).sum(dim=1) / (count - 1))
    z = (scores - mean) / std
    lam = math.pi / (std * math.sqrt(6.0))
    mu = mean - _EULER_GAMMA / lam
    p_value = -torch.expm1(-torch.exp(-lam * (scores - mu)))
    return Significance(z, mean, std, p_value, lam, mu)


def path_cells(ops, start) -> np.ndarray:
    """The rows a path pairs up: int32 ``[len, 2]`` of (row of the a-record, row of the b-record)
    for the ops of one pair (``ops[offsets[p]:offsets[p + 1]]`` of ``local_paths``) from its
    ``start``, with ``-1`` on the gap side (op ``1``: ``(-1, j)``, op ``2``: ``(i, -1)``).  A pure
    function of its arguments: no device is needed."""
    ops = _host_array(ops)
    if ops.size == 0 and ops.ndim == 1:
        return np.zeros((0, 2), dtype=np.int32)
    if ops.ndim != 1 or ops.dtype.kind not in "iu" or ops.min() < 0 or ops.max() > 2:
        raise ValueError("ops must be a one-dimensional integer array of 0, 1 and 2")
    start = _host_array(start)
    if start.shape != (2,) or start.dtype.kind not in "iu" or start.min() < 0:
        raise ValueError("start must be a cell (i, j) with both coordinates >= 0")
    in_a, in_b = ops != 1, ops != 2
    cells = np.stack([np.where(in_a, int(start[0]) - 1 + np.cumsum(in_a), -1),
                      np.where(in_b, int(start[1]) - 1 + np.cumsum(in_b), -1)], axis=1)
    return cells.astype(np.int32)


def top_pairs(scores, k: int, *, largest: bool) -> np.ndarray:
    """The candidate pairs of a ``distance.record_scores`` matrix ``[Q, R]``: for every row q its
    ``k`` best columns r, as an int32 ``[Q * min(k, R), 2]`` host array of ``[q, r]``, rows in
    order and inside a row the best column first.  ``largest`` says which end is good (True for
    cosine scores, False for L2).  Ties go to the lowest r; NaN (a record of zero rows) ranks
    behind every number.  A pure function of its arguments: no device is needed."""
    k = _checked_integer(k, "k", 1)
    if not isinstance(largest, (bool, np.bool_)):
        raise ValueError("largest must be True (large scores are good) or False")
    scores = _host_array(scores)
    if scores.ndim != 2 or scores.dtype.kind != "f":
        raise ValueError("scores must be a floating-point matrix [Q, R]")
    missing = np.isnan(scores)
    keys = np.where(missing, 0, -scores if largest else scores)
    # by (NaN or not, key, column): lexsort is stable and takes its last key first
    order = np.lexsort((keys, missing), axis=1)[:, :min(int(k), scores.shape[1])]
    rows = np.repeat(np.arange(scores.shape[0]), order.shape[1])
    return np.stack([rows, order.reshape(-1)], axis=1).astype(np.int32)


__all__ = ["local_align", "local_spans", "local_paths", "global_align", "global_paths",
           "path_cells", "AlignedPaths", "AlignWorkspace", "top_pairs", "band_around",
           "hit_cells", "hit_runs", "Runs", "RunsWorkspace", "chain_runs", "Chains",
           "ChainsWorkspace"]
