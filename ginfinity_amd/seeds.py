"""Seeds for the banded aligners: hits as cells, diagonal runs of hits, chains of runs, bands.

The sparse search chain is ``distance.within`` -> ``hit_runs`` -> ``chain_runs`` ->
``align.local_paths``; ``align`` exports every name of this module, so ``align.hit_runs`` is
``seeds.hit_runs``:

    hits = distance.within(rows, threshold=0.9, metric="cosine", exclude_records=counts)
    runs = align.hit_runs(hits, counts_a=counts, min_length=8)
    chains = align.chain_runs(runs, max_gap=8)              # max_shift defaults to max_gap
    best = chains.best(64)                                  # most hits, then heaviest
    paths = align.local_paths(rows, counts_a=counts, pairs=chains.pairs[best],
                              band=chains.bands(4)[best], box=chains.boxes(16)[best],
                              gap_open=1.0, gap_extend=0.25)

The definitions below stand here once in Python; include/gfy.h has them as the C contract.

Runs (``hit_runs``).  ``hits = Hits(offsets int64 [n + 1], indices int32 [H], values float32
[H])``: row i's hits are ``indices[offsets[i]:offsets[i + 1]]``, strictly ascending, the contract
of ``within``.  ``counts_a`` are the rows of ``a`` in contiguous records (``sum == n``, zero counts
allowed), ``counts_b`` those of ``b`` (``sum == m``; default ``counts_a``, the self-search form),
``ptr_a`` / ``ptr_b`` their running sums.  A row at a boundary belongs to the record that starts
there, a record of zero rows owns nothing (``distance.record_of``).  For a hit ``(i, j)`` let
``q``, ``r`` be the records of ``i`` and ``j``.  Its predecessor is ``(i - 1, j - 1)``; it counts
only if it is a hit, ``i - 1 >= ptr_a[q]`` and ``j - 1 >= ptr_b[r]``, so that it lies in the same
two records.  A hit without a predecessor is a head; the run of a head is the hits ``(i + t, j +
t)``, ``t = 0 .. L - 1``, for the largest ``L`` for which all of them are hits inside records
``q`` and ``r``.  Every hit belongs to exactly one run, and a run never crosses a record boundary
on either side.  Run s has ``pairs[s] = (q, r)``, ``cells[s] = (i - ptr_a[q], j - ptr_b[r])`` (its
head inside the two records), ``lengths[s] = L`` and ``weights[s]`` = the sum of its ``L`` values,
accumulated in float64 in ascending ``t``, each addition one rounded operation, and rounded to
float32 once (the rule of ``record_scores``).  Runs come in the order of their heads inside
``hits``: ``i`` ascending, then ``j`` ascending.  ``min_length`` (an integer >= 1) drops the
shorter runs and keeps the order of the rest.

A run is a function of the hits and the counts alone, bit for bit.  So the lengths sum to ``H``
at ``min_length=1``; ``min_length=k`` is that result filtered by length; and a record that is a
bit-identical copy of another gives, under a threshold its rows pass, exactly one run ``(q, r,
(0, 0), rows of the record)`` on the pair's main diagonal, whatever else hits.

Chains of runs (``chain_runs``).  A run is a gapless stretch on one diagonal, so two records that
share a region with one inserted or deleted row give two runs on two diagonals.  ``chain_runs``
links such pieces and returns, per chain, the band of diagonals that holds all of it.  It is a
fixed function of the ``Runs`` and two integers, bit for bit, and needs no counts.

Inputs.  ``runs = Runs(pairs int32 [S, 2], cells int32 [S, 2], lengths int32 [S], weights float32
[S])``, in the order ``hit_runs`` emits them: the key ``(q, cell_i, r, cell_j)`` is strictly
ascending lexicographically from run to run (this follows from "i ascending, then j ascending"
over contiguous records).  A boolean-mask subset of a ``Runs`` keeps this order; a ``best()``
permutation does not.

Terms.  Run s has pair ``(q_s, r_s)``, head ``(i_s, j_s)``, length ``L_s >= 1`` and diagonal ``d_s
= j_s - i_s``.  Its tail is the cell ``(i_s + L_s - 1, j_s + L_s - 1)``.

Linking rule.  s may precede t (``s -> t``) if and only if all of these hold: the pairs are equal;
``gi = i_t - (i_s + L_s) >= 0``; ``gj = j_t - (j_s + L_s) >= 0``; ``max(gi, gj) <= max_gap``;
``|d_t - d_s| = |gj - gi| <= max_shift``.  ``max_shift=None`` means ``max_gap``.  There is no
overlap in either coordinate, and ``s -> t`` implies ``s < t`` in Runs order.

Forward pass.  ``C[t] = L_t + max(0, max over s -> t of C[s])``, computed in int64.  ``pred[t]`` is
the s that attains the maximum; ties go to the smallest ``|d_t - d_s|``, then to the largest s;
``pred[t] = -1`` when no s precedes t.

Backward pass.  The mirror image: ``D[s] = L_s + max(0, max over s -> t of D[t])``.  ``succ[s]`` is
the t that attains the maximum; ties go to the smallest ``|d_t - d_s|``, then to the smallest t.

Links and chains.  A link ``s - t`` is kept if and only if ``pred[t] == s`` and ``succ[s] == t``:
both ends must choose each other.  Every run therefore has at most one kept predecessor and at
most one kept successor.  The chains are the maximal paths; every run belongs to exactly one
chain, and a chain lies in one record pair.  The rule was chosen because it is symmetric (the
runs read backwards give the same chains) and needs no serial "take the best chain, remove its
runs, repeat" step: two passes and a comparison decide every link.  What it guarantees: where a
record pair's maximum-hit chain is unique, including all its prefixes and suffixes, that chain is
one of the chains returned.

Output.  ``Chains`` is a NamedTuple of device tensors; chains come in the order of their first
runs.  ``pairs`` int32 ``[K, 2]``; ``starts`` int32 ``[K, 2]``, the head of the first run; ``ends``
int32 ``[K, 2]``, the tail of the last run; ``diagonals`` int32 ``[K, 2]``, ``(min d, max d)`` over
the chain's runs; ``counts`` int32 ``[K]``, the number of runs; ``lengths`` int32 ``[K]``, the sum
of ``L``, which is the number of hits; ``weights`` float32 ``[K]``, the runs' float32 weights
added in float64 in chain order, each addition one rounded operation, rounded to float32 once;
``members`` int32 ``[S]``, the chain of every run: a chain's runs are ``flatnonzero(members ==
c)``, ascending.  ``Chains.bands(half_width)`` gives ``(diagonals[:, 0] - half_width,
diagonals[:, 1] + half_width)`` as an int32 host array, which is what ``local_align`` /
``local_spans`` / ``local_paths`` take with ``pairs=chains.pairs``, and ``Chains.boxes(margin)``
gives ``(starts_i - margin, ends_i + margin, starts_j - margin, ends_j + margin)``, what they take
as ``box`` (``Runs.boxes(margin)`` is the same from a run's head and tail); ``Chains.best(k)`` is the rule
of ``Runs.best``: lengths descending, then weights descending with NaN last, then position.

Consequences.  ``max_gap=0`` links nothing, because two such runs would have been one maximal
run: then ``K == S``, ``starts == cells``, ``lengths`` are equal, ``weights`` are the same bytes
and ``members == arange(S)``.  ``counts.sum() == S`` and ``lengths.sum() == runs.lengths.sum()``,
whatever the two integers.

Out of scope for ``hit_runs``: a cross-shard form in ``parallel.py``, runs from ``topk`` results
(a ``[n, k]`` block is not sorted by b-row), and a ``device="cpu"`` path.  Out of scope for
``chain_runs``: overlapping runs (two runs that share a row or a column never link), a gap or
shift penalty in the chain score (``C`` counts hits alone), chains across record pairs or
shards, and a ``device="cpu"`` path.  Measured cost: DESIGN.md §4.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _native as native
from .distance import (_checked_counts, _checked_integer, _grown, _host_array, _record_ptr,
                       _scratch_tail, record_of)


def _widened(lo, hi, half_width) -> np.ndarray:
    """The bands ``(lo - half_width, hi + half_width)`` of int64 diagonals ``lo <= hi`` as an int32
    ``[P, 2]`` array.  ``half_width`` is a non-negative integer, cut at twice
    ``GFY_ALIGN_ROWS_MAX``, which is wider than any matrix; the bounds are clipped into int32."""
    width = min(_checked_integer(half_width, "half_width", 0), 2 * native.GFY_ALIGN_ROWS_MAX)
    limit = np.iinfo(np.int32)
    return np.clip(np.stack([lo - width, hi + width], axis=1), limit.min,
                   limit.max).astype(np.int32)


def _boxed(first, last, margin) -> np.ndarray:
    """The boxes ``(first_i - margin, last_i + margin, first_j - margin, last_j + margin)`` of
    int64 cells ``first <= last`` (``[P, 2]`` each) as an int32 ``[P, 4]`` array.  ``margin`` is a
    non-negative integer, cut like a ``half_width`` at twice ``GFY_ALIGN_ROWS_MAX``; the bounds are
    clipped into int32 and not into any record: the call that takes the boxes does that."""
    margin = min(_checked_integer(margin, "margin", 0), 2 * native.GFY_ALIGN_ROWS_MAX)
    limit = np.iinfo(np.int32)
    return np.clip(np.stack([first[:, 0] - margin, last[:, 0] + margin, first[:, 1] - margin,
                             last[:, 1] + margin], axis=1), limit.min, limit.max).astype(np.int32)


def band_around(seeds, half_width: int) -> np.ndarray:
    """The bands of ``half_width`` diagonals on either side of seed cells: int32 ``[P, 2]`` of
    ``(j - i - half_width, j - i + half_width)`` for ``seeds``, an integer ``[P, 2]`` array (numpy
    or torch) of cells ``(i, j)`` inside the two records of each pair; ``half_width`` is a
    non-negative integer, 0 the seed's diagonal alone.  A pure function of its arguments: no
    device is needed.  ``hit_cells`` turns the hits of ``distance.topk`` / ``within`` into seeds
    (one per hit, by taking away each record's first row) and the ``pairs`` that go with them;
    ``hit_runs`` makes one seed per diagonal run of ``within`` hits, and ``Runs.bands`` is this
    function on them.
    """
    seeds = _host_array(seeds)
    if seeds.size == 0 and seeds.ndim in (1, 2):
        seeds = np.zeros((0, 2), dtype=np.int64)
    if seeds.ndim != 2 or seeds.shape[1] != 2 or seeds.dtype.kind not in "iu":
        raise ValueError("seeds must be an integer array of shape (P, 2) of cells (i, j)")
    seeds = seeds.astype(np.int64)
    if seeds.size and (seeds.min() < 0 or seeds.max() >= native.GFY_ALIGN_ROWS_MAX):
        raise ValueError(f"seeds must be cells inside records: 0 <= i, j < "
                         f"{native.GFY_ALIGN_ROWS_MAX}")
    diagonal = seeds[:, 1] - seeds[:, 0]
    return _widened(diagonal, diagonal, half_width)


def hit_cells(rows, indices, counts_a, counts_b=None) -> tuple:
    """Hits as seed cells: ``(q, r, cells)`` for the hits (row ``rows[x]`` of ``a``, row
    ``indices[x]`` of ``b``) of ``distance.topk`` / ``nearest`` / ``within`` — ``q`` and ``r`` the
    records of the two rows (``distance.record_of``: a row at a boundary belongs to the record
    that starts there) and ``cells`` ``[P, 2]`` the rows minus each record's first row, which is
    what ``band_around`` takes as seeds and ``stack([q, r], 1)`` what the aligners take as
    ``pairs``.  One seed per hit; ``hit_runs`` makes one per stretch of collinear hits.

    ``rows`` and ``indices`` are integer arrays of one shape and one library: torch tensors (on
    one device; the results stay there, ``q`` and ``r`` int32, ``cells`` int64) or numpy arrays
    (numpy results).  ``counts_a`` / ``counts_b`` are the row counts of the records of ``a`` /
    ``b`` (any integer sequence, checked as ``record_of`` checks them; ``counts_b`` defaults to
    ``counts_a``).  An index outside every record, ``-1`` included, gives record ``-1`` and a
    cell coordinate of ``-1``."""
    counts_a = _checked_counts(counts_a)
    counts_b = counts_a if counts_b is None else _checked_counts(counts_b)
    as_torch = isinstance(rows, torch.Tensor)
    if as_torch != isinstance(indices, torch.Tensor):
        raise ValueError("rows and indices must both be torch tensors or both numpy arrays")
    if not as_torch:
        rows, indices = (torch.from_numpy(np.ascontiguousarray(x)) for x in (rows, indices))
    if rows.shape != indices.shape or rows.dim() != 1 or rows.device != indices.device or \
            rows.dtype.is_floating_point or indices.dtype.is_floating_point or \
            torch.bool in (rows.dtype, indices.dtype):
        raise ValueError("rows and indices must be one-dimensional integer arrays of one length "
                         "(torch: on one device)")
    found, inside = [], []
    for index, counts in ((rows, counts_a), (indices, counts_b)):
        record = record_of(index, counts)
        first = torch.from_numpy(np.concatenate(([0], np.cumsum(counts)))).to(index.device)
        outside = record < 0
        start = first[torch.where(outside, torch.zeros_like(record), record).to(torch.int64)]
        found.append(record)
        inside.append(torch.where(outside, torch.full_like(start, -1),
                                  index.to(torch.int64) - start))
    cells = torch.stack(inside, dim=1)
    if as_torch:
        return found[0], found[1], cells
    return found[0].numpy(), found[1].numpy(), cells.numpy()


def _best(lengths, weights, k) -> np.ndarray:
    """The rule of ``Runs.best`` and ``Chains.best``: the first ``k`` positions in the order
    ``lengths`` descending, then ``weights`` descending with NaN last, then position."""
    k = _checked_integer(k, "k", 1)
    lengths, weights = _host_array(lengths), _host_array(weights)
    missing = np.isnan(weights)
    # by (length, NaN or not, weight, position): lexsort is stable and takes its last key first
    order = np.lexsort((np.where(missing, 0, -weights.astype(np.float64)), missing,
                        -lengths.astype(np.int64)))
    return order[:k].astype(np.int64)


class Runs(NamedTuple):
    """What ``hit_runs`` returns, all on the device: run s lies in the record pair ``pairs[s]``,
    starts at the cell ``cells[s]`` inside the two records, and is ``lengths[s]`` hits long on
    the diagonal ``cells[s, 1] - cells[s, 0]``; ``weights[s]`` is the sum of its values."""
    pairs: torch.Tensor     # int32 [S, 2] of (record of a, record of b)
    cells: torch.Tensor     # int32 [S, 2] of the head (i, j) inside the two records
    lengths: torch.Tensor   # int32 [S]
    weights: torch.Tensor   # float32 [S]

    def bands(self, half_width: int) -> np.ndarray:
        """``band_around(self.cells, half_width)``: the band of every run's diagonal for
        ``local_align`` / ``local_spans`` / ``local_paths`` with ``pairs=self.pairs``."""
        return band_around(self.cells, half_width)

    def boxes(self, margin: int) -> np.ndarray:
        """The box of every run with ``margin`` rows around it on all four sides, as an int32
        ``[S, 4]`` host array of ``(i_lo, i_hi, j_lo, j_hi)``: from the head ``cells`` minus
        ``margin`` to the tail ``cells + lengths - 1`` plus ``margin``, for the ``box`` of
        ``local_align`` / ``local_spans`` / ``local_paths`` with ``pairs=self.pairs``.  ``margin``
        is a non-negative integer, cut like ``half_width``.  A pure function of ``cells`` and
        ``lengths``; the boxes are not clipped at the records' ends, the call does that."""
        cells = _host_array(self.cells).astype(np.int64).reshape(-1, 2)
        lengths = _host_array(self.lengths).astype(np.int64).reshape(-1, 1)
        return _boxed(cells, cells + lengths - 1, margin)

    def best(self, k: int) -> np.ndarray:
        """The indices (int64 host array, at most ``k``) of the ``k`` runs that come first in the
        order ``lengths`` descending, then ``weights`` descending, then position ascending; a NaN
        weight ranks behind every number of its length.  A pure function of ``lengths`` and
        ``weights``, which come to the host for it."""
        return _best(self.lengths, self.weights, k)


class Chains(NamedTuple):
    """What ``chain_runs`` returns, all on the device: chain c lies in the record pair
    ``pairs[c]``, reaches from the cell ``starts[c]`` (the head of its first run) to the cell
    ``ends[c]`` (the tail of its last run) on the diagonals ``diagonals[c, 0] .. diagonals[c, 1]``,
    and is ``counts[c]`` runs of ``lengths[c]`` hits in all; ``weights[c]`` is the sum of their
    weights.  ``members[s]`` is the chain of run s: a chain's runs are
    ``flatnonzero(members == c)``, ascending."""
    pairs: torch.Tensor       # int32 [K, 2] of (record of a, record of b)
    starts: torch.Tensor      # int32 [K, 2]
    ends: torch.Tensor        # int32 [K, 2]
    diagonals: torch.Tensor   # int32 [K, 2] of (min d, max d)
    counts: torch.Tensor      # int32 [K]
    lengths: torch.Tensor     # int32 [K]
    weights: torch.Tensor     # float32 [K]
    members: torch.Tensor     # int32 [S]

    def bands(self, half_width: int) -> np.ndarray:
        """``(diagonals[:, 0] - half_width, diagonals[:, 1] + half_width)`` as an int32 ``[K, 2]``
        host array: the band that holds every run of a chain, for ``local_align`` /
        ``local_spans`` / ``local_paths`` with ``pairs=self.pairs``.  ``half_width`` is a
        non-negative integer, 0 the chain's own diagonals alone; like ``band_around`` it is cut
        at twice ``GFY_ALIGN_ROWS_MAX``, wider than any matrix."""
        diagonals = _host_array(self.diagonals).astype(np.int64).reshape(-1, 2)
        return _widened(diagonals[:, 0], diagonals[:, 1], half_width)

    def boxes(self, margin: int) -> np.ndarray:
        """The box of every chain with ``margin`` rows around it on all four sides, as an int32
        ``[K, 4]`` host array of ``(starts_i - margin, ends_i + margin, starts_j - margin, ends_j +
        margin)``, for the ``box`` of ``local_align`` / ``local_spans`` / ``local_paths`` next to
        ``band=self.bands(...)``: two chains on the same diagonals of one record pair then get two
        answers.  ``margin`` is a non-negative integer, cut like ``half_width``.  A pure function
        of ``starts`` and ``ends``; the boxes are not clipped at the records' ends, the call does
        that."""
        return _boxed(_host_array(self.starts).astype(np.int64).reshape(-1, 2),
                      _host_array(self.ends).astype(np.int64).reshape(-1, 2), margin)

    def best(self, k: int) -> np.ndarray:
        """The indices (int64 host array, at most ``k``) of the ``k`` chains that come first by
        the rule of ``Runs.best``: ``lengths`` (hits) descending, then ``weights`` descending with
        NaN last, then position ascending."""
        return _best(self.lengths, self.weights, k)


#: a result's fields as (dtype, axis, columns...): axis K counts what the emit launch writes
#: (runs, chains), axis S what the call was given
_RUNS_LAYOUT = ((torch.int32, "K", 2), (torch.int32, "K", 2), (torch.int32, "K"),
                (torch.float32, "K"))
_CHAINS_LAYOUT = ((torch.int32, "K", 2),) * 4 + ((torch.int32, "K"), (torch.int32, "K"),
                                                 (torch.float32, "K"), (torch.int32, "S"))


class _SeedWorkspace:
    """Scratch memory, marks and slots of a two-pass seed maker kept across calls (the results
    are always new tensors)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.marks: torch.Tensor | None = None
        self.slots: torch.Tensor | None = None

    def buffers(self, device, count: int, scratch_bytes: int):
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        self.marks = _grown(self.marks, device, count, torch.int32)
        self.slots = _grown(self.slots, device, count, torch.int64)
        return self.scratch, self.marks[:count], self.slots[:count]


class RunsWorkspace(_SeedWorkspace):
    """The workspace of ``hit_runs``: one mark and one slot per hit."""


class ChainsWorkspace(_SeedWorkspace):
    """The workspace of ``chain_runs``: one mark and one slot per run.  ``plain_scan=True`` makes
    the link kernel look at every earlier (later) run of a pair instead of stopping at the first
    one too far away to link; the chains are the same bytes, which is what the switch is there
    to show."""

    def __init__(self, plain_scan: bool = False) -> None:
        if not isinstance(plain_scan, (bool, np.bool_)):
            raise ValueError("plain_scan must be a bool")
        super().__init__()
        self.plain_scan = bool(plain_scan)


def _on_one_device(parts, what: str) -> tuple:
    """``parts`` contiguous on the one cuda device that holds any of them, else on ``cuda``;
    parts on two cuda devices are a ``ValueError``."""
    devices = {part.device for part in parts if part.device.type == "cuda"}
    if len(devices) > 1:
        raise ValueError(f"{what} must live on one device")
    device = devices.pop() if devices else torch.device("cuda")
    return tuple(part.to(device).contiguous() for part in parts)


def _fresh(kind, layout, device, kept: int, given: int):
    """An uninitialised result ``kind`` on ``device`` whose fields have the shapes of ``layout``
    with K = ``kept`` and S = ``given``."""
    rows = {"K": kept, "S": given}
    return kind(*(torch.empty((rows[axis], *columns), dtype=dtype, device=device)
                  for dtype, axis, *columns in layout))


def _two_pass(*, symbols, leading, middle, emit_middle, keep, kind, layout, count: int, device,
              workspace: _SeedWorkspace, error: str):
    """The two launches of ``hit_runs`` and ``chain_runs`` on ``count`` checked entries of
    ``device``, and their result.  ``symbols`` names the workspace sizer and the two calls:

        first(*leading, *middle, marks, status, scratch, bytes, stream)
        second(*leading, marks, slots, *emit_middle, K, *outputs, status, scratch, bytes, stream)

    The first writes one int32 mark per entry, ``slots`` is the running sum of ``keep(marks)``,
    and its last entry K comes to the host, which waits for the device.  The second fills a new
    ``kind`` of the shapes of ``layout`` and is left out when K is 0.  Either call may set its
    word of ``status``: what it was given contradicted itself, a ``NativeLibraryError`` of the
    text ``error`` once both are through (the second wait)."""
    sizer, first, second = symbols
    lib = native.library()
    scratch, marks, slots = workspace.buffers(device, count, getattr(lib, sizer)(count))
    status = torch.zeros(2, dtype=torch.int32, device=device)
    back = _scratch_tail(scratch, device)
    native.check(getattr(lib, first)(*leading, *middle, marks.data_ptr(),
                                     status[0:].data_ptr(), *back), first)
    torch.cumsum(keep(marks), 0, dtype=torch.int64, out=slots)
    kept = int(slots[-1].item())   # waits for the device
    result = _fresh(kind, layout, device, kept, count)
    if kept:
        native.check(getattr(lib, second)(
            *leading, marks.data_ptr(), slots.data_ptr(), *emit_middle, kept,
            *(out.data_ptr() for out in result), status[1:].data_ptr(), *back), second)
    if bool(status.any().item()):
        raise native.NativeLibraryError(error)
    return result


def _checked_hits(hits) -> tuple:
    """``(offsets, indices, values)`` of a ``distance.Hits`` (or any triple of torch tensors or
    numpy arrays) with the dtypes and shapes of ``within``'s result, wherever they live."""
    if not isinstance(hits, tuple) or len(hits) != 3:
        raise ValueError("hits must be a distance.Hits (offsets, indices, values)")
    parts = []
    for part, name, dtype in zip(hits, ("offsets", "indices", "values"),
                                 (torch.int64, torch.int32, torch.float32)):
        if isinstance(part, np.ndarray):
            part = torch.from_numpy(np.ascontiguousarray(part))
        if not isinstance(part, torch.Tensor) or part.dtype != dtype or part.dim() != 1:
            raise ValueError(f"hits.{name} must be a one-dimensional "
                             f"{str(dtype).replace('torch.', '')} array")
        parts.append(part)
    offsets, indices, values = parts
    if offsets.numel() < 1:
        raise ValueError("hits.offsets must hold n + 1 entries")
    if indices.numel() != values.numel():
        raise ValueError(f"hits.indices has {indices.numel()} entries, hits.values "
                         f"{values.numel()}")
    if indices.numel() >= 2 ** 31 - 1:
        raise ValueError("hits must hold fewer than 2^31 - 1 hits")
    return offsets, indices, values


def hit_runs(hits, *, counts_a, counts_b=None, min_length: int = 1,
             workspace: RunsWorkspace | None = None) -> Runs:
    """The maximal diagonal runs of the hits of ``distance.within``: ``Runs(pairs int32 [S, 2],
    cells int32 [S, 2], lengths int32 [S], weights float32 [S])`` on the device.  A stretch that
    two records share is one hit per row on one diagonal; this collapses each into one seed with
    the evidence behind it, and ``pairs`` says which records are worth aligning at all without a
    dense ``record_scores``.  The definition of a run, of its four fields and of ``min_length``
    is at the head of this module.

    Every argument error is a ``ValueError`` before a device is touched: dtypes, shapes,
    ``min_length``, the counts (checked as ``record_scores`` checks them), ``offsets.numel() ==
    sum(counts_a) + 1``.  Three more need the data and are made on the device in front of the
    launch — ``offsets[0] == 0``; ``offsets`` non-decreasing with ``offsets[-1] == H``; ``0 <=
    indices < sum(counts_b)`` — so that no hand-made ``Hits`` makes a kernel read outside its
    arrays.  Ascending order inside a row is a precondition and is not checked.  Hits on the
    host are moved to the device, as rows are; there is no CPU path.

    Two launches with a running sum between them (``torch.cumsum``: plumbing, as in ``within``),
    whose total comes to the host, which waits for the device as ``within`` does.  One lane per
    hit; a head walks its run serially, so a run of ``L`` hits is ``L`` steps of one lane
    (DESIGN.md §4).  ``H == 0`` or ``n == 0`` returns four empty tensors without a launch."""
    offsets, indices, values = _checked_hits(hits)
    min_length = _checked_integer(min_length, "min_length", 1)
    if workspace is not None and not isinstance(workspace, RunsWorkspace):
        raise ValueError("workspace must be a RunsWorkspace")
    n, total = offsets.numel() - 1, indices.numel()
    ptr_a = _record_ptr(counts_a, n, "counts_a", "hits")
    if counts_b is None:
        ptr_b = ptr_a
    else:
        ptr_b = _record_ptr(counts_b, int(_checked_counts(counts_b).sum()), "counts_b", "b")
    m = int(ptr_b[-1])
    offsets, indices, values = _on_one_device((offsets, indices, values), "hits")
    device = offsets.device
    with torch.cuda.device(device):
        # every entry at or above its predecessor, the first 0, the last H; every index a row of b
        sound = (offsets[0] == 0) & (offsets[-1] == total) & \
            (offsets[1:] >= offsets[:-1]).all()
        if total:
            sound = sound & (indices.min() >= 0) & (indices.max() < m)
        if not bool(sound.item()):
            raise ValueError(
                "hits are not those of a search: offsets must start at 0, never decrease and end "
                f"at {total} = the number of hits, and indices must lie in 0..{m - 1}")
        if total == 0 or n == 0:
            return _fresh(Runs, _RUNS_LAYOUT, device, 0, 0)
        ptr_a_dev = torch.from_numpy(ptr_a.astype(np.int32)).to(device)
        ptr_b_dev = ptr_a_dev if ptr_b is ptr_a else \
            torch.from_numpy(ptr_b.astype(np.int32)).to(device)
        return _two_pass(
            symbols=("gfy_hit_runs_workspace_bytes", "gfy_hit_runs_mark", "gfy_hit_runs_emit"),
            leading=(offsets.data_ptr(), n, indices.data_ptr(), values.data_ptr(), total,
                     ptr_a_dev.data_ptr(), ptr_a.size - 1, ptr_b_dev.data_ptr(), ptr_b.size - 1,
                     m),
            middle=(), emit_middle=(min(min_length, 2 ** 31 - 1),),
            keep=lambda marks: marks >= min_length, kind=Runs, layout=_RUNS_LAYOUT, count=total,
            device=device, workspace=workspace or RunsWorkspace(),
            error="gfy_hit_runs: the hits contradicted the sizes of the call")


def _checked_runs(runs) -> tuple:
    """``(pairs, cells, lengths, weights)`` of a ``Runs`` (or any 4-tuple of torch tensors or
    numpy arrays) with the dtypes and shapes of ``hit_runs``' result, wherever they live."""
    if not isinstance(runs, tuple) or len(runs) != 4:
        raise ValueError("runs must be an align.Runs (pairs, cells, lengths, weights)")
    parts = []
    for part, name, dtype, dim in zip(runs, Runs._fields, (torch.int32, torch.int32, torch.int32,
                                                           torch.float32), (2, 2, 1, 1)):
        if isinstance(part, np.ndarray):
            part = torch.from_numpy(np.ascontiguousarray(part))
        if not isinstance(part, torch.Tensor) or part.dtype != dtype or part.dim() != dim or \
                (dim == 2 and part.shape[1] != 2):
            raise ValueError(f"runs.{name} must be a {str(dtype).replace('torch.', '')} array "
                             f"of shape {'(S, 2)' if dim == 2 else '(S,)'}")
        parts.append(part)
    count = parts[2].shape[0]
    for part, name in zip(parts, Runs._fields):
        if part.shape[0] != count:
            raise ValueError(f"runs.{name} has {part.shape[0]} entries, runs.lengths {count}")
    if count >= 2 ** 31 - 1:
        raise ValueError("runs must hold fewer than 2^31 - 1 runs")
    return tuple(parts)


def _checked_reach(value, name: str) -> int:
    # coordinates are int32: nothing lies farther apart
    return min(_checked_integer(value, name, 0), 2 ** 31 - 1)


def chain_runs(runs, *, max_gap: int, max_shift: int | None = None,
               workspace: ChainsWorkspace | None = None) -> Chains:
    """The runs of ``hit_runs`` linked across neighbouring diagonals: ``Chains(pairs, starts,
    ends, diagonals, counts, lengths, weights, members)`` on the device.  An inserted or deleted
    row cuts a shared region into two runs on two diagonals; a chain is the region again, with
    the band ``Chains.bands`` that holds all of it.  A fixed function of the ``Runs`` and two
    integers, bit for bit; it needs no counts.  The linking rule, the two passes, the fields of
    the result and what follows from them are at the head of this module.

    Every argument error is a ``ValueError`` before a device is touched: ``runs`` that is not a
    4-tuple of tensors or arrays with ``Runs``' dtypes and shapes, ``S >= 2^31 - 1``, a
    ``max_gap`` or ``max_shift`` that is not a non-negative integer (a bool is none), a
    ``workspace`` that is not a ``ChainsWorkspace``.  The checks that need the data are made on
    the device in front of the launch, as ``hit_runs`` makes its own, and raise ``ValueError``
    "runs are not those of hit_runs": ``lengths >= 1``, ``cells >= 0``, ``pairs >= 0``,
    ``lengths.sum() < 2^31``, no tail beyond int32, the key strictly ascending.  Runs on the host
    are moved to the device; there is no CPU path.  ``S == 0`` returns empty tensors without a
    launch.

    Two launches with torch plumbing around them, as in ``hit_runs``: a stable sort of the runs
    by the key ``q * 2^31 + r`` in int64 and the group boundaries in front of the link launch (one
    wave per record pair; include/gfy.h says what it does), the running sum of chain-head marks
    behind it, whose total K comes to the host, then the emit launch.  Not built: overlapping
    runs, a gap or shift penalty in the chain score, chains across record pairs or shards, a CPU
    path."""
    pairs, cells, lengths, weights = _checked_runs(runs)
    max_gap = _checked_reach(max_gap, "max_gap")
    max_shift = max_gap if max_shift is None else _checked_reach(max_shift, "max_shift")
    if workspace is not None and not isinstance(workspace, ChainsWorkspace):
        raise ValueError("workspace must be a ChainsWorkspace")
    count = lengths.shape[0]
    pairs, cells, lengths, weights = _on_one_device((pairs, cells, lengths, weights), "runs")
    device = pairs.device
    with torch.cuda.device(device):
        if count == 0:
            return _fresh(Chains, _CHAINS_LAYOUT, device, 0, 0)
        # (q, i, r, j) strictly ascending from run to run, in lexicographic order
        keys = torch.stack([pairs[:, 0], cells[:, 0], pairs[:, 1], cells[:, 1]], dim=1)
        below, equal = keys[:-1] < keys[1:], keys[:-1] == keys[1:]
        ascending = below[:, 3]
        for column in (2, 1, 0):
            ascending = below[:, column] | (equal[:, column] & ascending)
        sound = (lengths >= 1).all() & (cells >= 0).all() & (pairs >= 0).all() & \
            (lengths.sum(dtype=torch.int64) < 2 ** 31) & ascending.all() & \
            ((cells.to(torch.int64) + lengths[:, None]).max() <= 2 ** 31)
        if not bool(sound.item()):
            raise ValueError(
                "runs are not those of hit_runs: lengths must be >= 1 and sum to less than 2^31, "
                "cells and pairs must be >= 0, and (q, cell_i, r, cell_j) must ascend strictly "
                "from run to run (a best() permutation does not)")
        # the runs of one record pair side by side, in their own order: plumbing, as the scan is
        key, order = torch.sort((pairs[:, 0].to(torch.int64) << 31) | pairs[:, 1].to(torch.int64),
                                stable=True)
        edge = torch.ones(count + 1, dtype=torch.bool, device=device)
        edge[1:-1] = key[1:] != key[:-1]
        bounds = torch.nonzero(edge).flatten()      # waits for the device
        workspace = workspace or ChainsWorkspace()
        chains = _two_pass(
            symbols=("gfy_chain_runs_workspace_bytes", "gfy_chain_runs_link",
                     "gfy_chain_runs_emit"),
            leading=(pairs.data_ptr(), cells.data_ptr(), lengths.data_ptr(), weights.data_ptr(),
                     count),
            middle=(order.data_ptr(), bounds.data_ptr(), bounds.numel() - 1, max_gap, max_shift,
                    int(workspace.plain_scan)),
            emit_middle=(), keep=lambda marks: marks > 0, kind=Chains, layout=_CHAINS_LAYOUT,
            count=count, device=device, workspace=workspace,
            error="gfy_chain_runs: the sorted order contradicted the sizes of the call")
        if chains.counts.shape[0] == 0:
            raise native.NativeLibraryError("gfy_chain_runs_link: no run starts a chain")
        return chains


__all__ = ["band_around", "hit_cells", "hit_runs", "Runs", "RunsWorkspace", "chain_runs",
           "Chains", "ChainsWorkspace"]
