"""All-pairs L2 / cosine distance over 128-d fp16 embeddings on the matrix cores.

The reference has no implementation of this step (its aligner is the external
``ginfinity-sw`` package; src/ginfinity/api.py:47-50 only exports scoring
parameters), so the semantics are defined here and in include/gfy.h:

    L2      D_ij = sqrt(max(|a_i|² + |b_j|² − 2 a_i·b_j, 0))
    cosine  S_ij = a_i·b_j / (max(|a_i|, 1e-12) · max(|b_j|, 1e-12))

Inputs are fp16 device tensors as produced by ``Ginfinity.encode_graphs_device``;
products are exact, accumulation is fp32 (MFMA).  ``nearest`` and ``topk`` never
materialise the N×M matrix.  ``topk`` and ``nearest`` can leave out a range of rows per row
(``exclude_ranges``) — in a search over a library of records, each row's own record
(``exclude_records``, ``record_ranges``) — and can return at most one row per record
(``distinct_records``, ``record_of``).

Record-to-record best-match scores (``record_best``, ``record_scores``; also include/gfy.h).
The rows of ``b`` are grouped in contiguous records of ``counts_b`` rows and the rows of ``a`` in
records of ``counts_a`` rows (non-negative integers, checked as ``record_ranges`` checks them,
``sum(counts_b) == m``, ``sum(counts_a) == n``).  The key and the value of a pair are those of
``nearest`` / ``topk``, computed the same way.

    row level     best[i, r]  = the value of the best pair (i, j) with j in record r (smallest
                                L2 distance / largest cosine); a record of zero rows gives
                                +inf (l2) / -inf (cosine)
    record level  score[q, r] = the mean over the rows i of record q of best[i, r], summed in
                                float64 in ascending row order, divided by |q| and rounded to
                                float32 once; an a-record of zero rows gives a row of NaN, a
                                b-record of zero rows +inf / -inf through the mean

``best[:, r]`` equals ``nearest(a, b[ptr[r]:ptr[r + 1]])`` values bit for bit; an entry of
``best`` or ``score`` depends neither on the other records and rows of the call nor on how the
call is cut into blocks, chunks or workgroups, and is the same from run to run bit for bit.  The
score is directional (``a`` onto ``b``): the symmetric form is two calls.  Nothing is excluded:
in a self-search the pairs (i, i) are simply the best ones.

Radius search (``count_within``, ``within``; also include/gfy.h): every row of ``b`` that is at
least as close as ``threshold`` to each row of ``a`` — a result whose length varies per row.  The
key and the value of a pair are those of ``nearest`` / ``topk``, computed the same way;
``threshold`` is rounded to float32 once on the host and compared in float32:

    l2      the pair (i, j) is a hit iff value_ij <= threshold
    cosine  the pair (i, j) is a hit iff value_ij >= threshold

``value_ij`` is bit for bit what ``topk`` reports for the pair.  So the hit set of a row depends
neither on the other rows of the call nor on how the call is cut into blocks and chunks, is the
same from run to run bit for bit, is for ``m <= 16`` the entries of ``topk(k=m)`` that pass the
comparison (same value bits), and is nested in a monotone threshold: raising an l2 threshold
never loses a hit.  An excluded pair (``exclude_self``, ``exclude_ranges``, ``exclude_records``:
one skipped range ``lo[i] <= j < hi[i]`` per row, as in ``topk``) is never a hit and never
counted.  ``within`` sweeps twice (count, then fill) and waits for the device in between to
learn the total.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _native as native

_METRICS = {"l2": native.GFY_L2, "cosine": native.GFY_COSINE}


def _checked(rows) -> torch.Tensor:
    """``rows`` as a tensor of the accepted dtype and shape, wherever it lives."""
    if isinstance(rows, np.ndarray):
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float16))
    if rows.dtype != torch.float16:
        raise ValueError("embeddings must be float16")
    if rows.dim() != 2 or rows.shape[1] != 128:
        raise ValueError("embeddings must have shape (rows, 128)")
    return rows


def _checked_integer(value, name: str, least: int) -> int:
    """``value`` as an int; ``ValueError`` unless it is an ``int`` or ``np.integer`` of at least
    ``least`` (1 or 0).  A bool is no integer here, and ``np.bool_`` is neither of the two."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"{name} must be a {'positive' if least else 'non-negative'} integer")
    return int(value)


def _host_array(values) -> np.ndarray:
    """``values`` as a host numpy array: a torch tensor from wherever it lives, anything else as
    ``np.asarray`` takes it."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    return np.asarray(values)


def _scratch_tail(scratch, device) -> tuple:
    """What every call of the C ABI ends with: the scratch memory, its size and the current
    stream of ``device``."""
    return scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(device).cuda_stream


def _prepare(rows, device: torch.device | None) -> torch.Tensor:
    rows = _checked(rows)
    if rows.device.type != "cuda":
        rows = rows.to(device if device is not None else "cuda")
    return rows.contiguous()


def _metric(name: str) -> int:
    try:
        return _METRICS[name]
    except KeyError:
        raise ValueError(f"metric must be one of {sorted(_METRICS)}") from None


def pairwise(a, b=None, *, metric: str = "l2") -> torch.Tensor:
    """Dense [n, m] float32 distance (l2) or similarity (cosine) block.
    Meant for blocks that fit comfortably in memory (n·m·4 bytes)."""
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
    lib = native.library()
    n, m = a.shape[0], b.shape[0]
    with torch.cuda.device(a.device):
        out = torch.empty((n, m), dtype=torch.float32, device=a.device)
        scratch = torch.empty(lib.gfy_pairwise_workspace_bytes(n, m),
                              dtype=torch.uint8, device=a.device)
        native.check(lib.gfy_pairwise_dense(
            a.data_ptr(), n, b.data_ptr(), m, _metric(metric), out.data_ptr(),
            *_scratch_tail(scratch, a.device)), "gfy_pairwise_dense")
    return out


def _grown(kept: torch.Tensor | None, device, count: int, dtype) -> torch.Tensor:
    """The grow rule of every workspace: ``kept`` where it lives on ``device`` and holds ``count``
    elements, a new tensor of ``max(count, 1)`` otherwise."""
    if kept is None or kept.numel() < count or kept.device != device:
        return torch.empty(max(count, 1), dtype=dtype, device=device)
    return kept


class NearestWorkspace:
    """Scratch memory and result arrays of ``nearest`` kept across calls (the chunked
    cross-shard search calls it once per rank's piece and chunk: allocating per call costs
    more than small searches)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.values: torch.Tensor | None = None
        self.indices: torch.Tensor | None = None

    def buffers(self, device, rows: int, scratch_bytes: int):
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        self.values = _grown(self.values, device, rows, torch.float32)
        self.indices = _grown(self.indices, device, rows, torch.int32)
        return self.scratch, self.values[:rows], self.indices[:rows]


def _checked_counts(counts) -> np.ndarray:
    """Record sizes as a non-negative int64 array; ``ValueError`` ("record counts ...") else."""
    counts = _host_array(counts)
    if counts.size == 0:
        counts = np.zeros(0, dtype=np.int64)
    if counts.ndim != 1 or counts.dtype.kind not in "iu":
        raise ValueError("record counts must be a sequence of integers")
    counts = counts.astype(np.int64)
    if np.any(counts < 0):
        raise ValueError("record counts must not be negative")
    return counts


def record_ranges(counts, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """The rows of every row's own record, for rows grouped in records of ``counts`` rows each
    (what ``Ginfinity.encode_graphs_device`` returns next to the embeddings): ``(lo, hi)``, int32
    tensors of length ``sum(counts)`` on ``device`` (default: the host), where row r of record q
    gets ``[ptr[q], ptr[q + 1])`` and ``ptr`` is the running sum of ``counts``.  Zero counts are
    allowed; a negative or non-integer count is a ``ValueError``.  The pair is what
    ``topk(..., exclude_ranges=...)`` takes."""
    counts = _checked_counts(counts)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    if ptr[-1] >= 2 ** 31 - 1:
        raise ValueError("record counts must sum to fewer than 2^31 - 1 rows")
    lo = torch.from_numpy(np.repeat(ptr[:-1], counts).astype(np.int32))
    hi = torch.from_numpy(np.repeat(ptr[1:], counts).astype(np.int32))
    if device is not None:
        lo, hi = lo.to(device), hi.to(device)
    return lo, hi


def record_of(indices, counts) -> torch.Tensor:
    """The record number of every index that ``topk`` / ``nearest`` returned, for rows grouped in
    records of ``counts`` rows each: an int32 tensor of the shape of ``indices`` on its device
    (a numpy array gives a host tensor), -1 where the index is -1.  A row at a boundary belongs
    to the record that starts there; a record of zero rows owns nothing.  ``counts`` is checked
    as ``record_ranges`` checks it."""
    counts = _checked_counts(counts)
    if not isinstance(indices, torch.Tensor):
        indices = torch.from_numpy(np.ascontiguousarray(indices))
    ends = torch.from_numpy(np.cumsum(counts)).to(indices.device)
    # the first record whose end lies behind the row: empty records end where they start
    found = torch.searchsorted(ends, indices.to(torch.int64), right=True)
    outside = (indices < 0) | (found >= ends.numel())
    return torch.where(outside, torch.full_like(found, -1), found).to(torch.int32)


def _checked_ranges(n: int, b_rows: int | None, exclude_ranges, exclude_records, others: bool):
    """``(lo, hi)`` int32 tensors of length n, wherever they live, from ``exclude_ranges`` or
    ``exclude_records``; None when neither is given.  ``others``: one of the single-pair
    exclusions was given too.  No device is touched."""
    if exclude_ranges is None and exclude_records is None:
        return None
    if others or (exclude_ranges is not None and exclude_records is not None):
        raise ValueError("exclude_ranges, exclude_records, exclude_self, exclude_offset and "
                         "window_first exclude each other")
    if exclude_records is not None:
        if b_rows is not None and b_rows != n:
            raise ValueError("exclude_records is for self-search: b omitted, or as many rows as a")
        lo, hi = record_ranges(exclude_records)
        if lo.numel() != n:
            raise ValueError(f"exclude_records sums to {lo.numel()} rows, a has {n}")
        return lo, hi
    try:
        lo, hi = exclude_ranges
    except (TypeError, ValueError):
        raise ValueError("exclude_ranges must be a pair (lo, hi) of int32 arrays") from None
    bounds = []
    for bound in (lo, hi):
        if isinstance(bound, np.ndarray):
            if bound.dtype != np.int32:
                raise ValueError("exclude_ranges must be int32")
            bound = torch.from_numpy(np.ascontiguousarray(bound))
        if not isinstance(bound, torch.Tensor) or bound.dtype != torch.int32:
            raise ValueError("exclude_ranges must be a pair (lo, hi) of int32 arrays")
        if bound.dim() != 1 or bound.shape[0] != n:
            raise ValueError(f"exclude_ranges must have shape ({n},): one range per row of a")
        bounds.append(bound)
    return tuple(bounds)


def _pair_ranges(n: int, exclude_self: bool, exclude_offset: int | None,
                 window_first: int | None) -> tuple[torch.Tensor, torch.Tensor]:
    """The single-pair exclusions of ``nearest`` / ``topk`` as ``(lo, hi)`` int32 host tensors of
    length n, the form of ``exclude_ranges``: a range of one row per row of ``a``, or of none
    (without an exclusion, and for a negative ``exclude_offset``, which excludes nothing).
    A search times this on the host, so the usual case is two passes over int32.  ``lo`` and
    ``hi`` may be one tensor (ranges of no row): callers read them and never write."""
    if window_first is not None:
        skip = -int(window_first)
    else:
        skip = 0 if exclude_self and exclude_offset is None else exclude_offset
    first = 0 if skip is None else int(skip)
    width = 0 if skip is None or (window_first is None and skip < 0) else 1
    if first >= -1 and first + n + width < 2 ** 31:      # every bound fits int32 as it is
        lo = torch.arange(first, first + n, dtype=torch.int32)
        return lo, (lo + width if width else lo)
    # a pair outside b excludes nothing; clamped so that the bounds fit int32
    lo = torch.arange(n, dtype=torch.int64) + first
    return tuple(bound.clamp(-1, 2 ** 31 - 1).to(torch.int32) for bound in (lo, lo + width))


def _results(values, indices, scratch) -> tuple:
    """What a ``nearest`` / ``topk`` call of the C ABI ends with: the two results, the scratch
    memory and its size, the current stream of their device."""
    return values.data_ptr(), indices.data_ptr(), *_scratch_tail(scratch, values.device)


def nearest(a, b=None, *, metric: str = "l2", exclude_self: bool = False,
            exclude_offset: int | None = None, window_first: int | None = None,
            exclude_ranges=None, exclude_records=None,
            workspace: NearestWorkspace | None = None
            ) -> tuple[torch.Tensor, torch.Tensor]:
    """For every row of ``a`` the closest row of ``b`` (smallest L2 distance /
    largest cosine): ``(values float32 [n], indices int32 [n])``; ties go to
    the lowest index.  ``exclude_self`` (with ``b`` omitted or identical to
    ``a``) skips the pair (i, i); ``exclude_offset=k`` skips (i, i+k) — ``a`` is a
    row block of ``b`` starting at row k; ``window_first=k`` is the opposite case:
    ``b`` is rows [k, k + m) of ``a`` and every row skips itself (the cross-shard
    search of a rank's own piece, one call).  A row with every candidate excluded
    gets index -1 and value ``+inf`` (l2) / ``-inf`` (cosine).  With ``workspace`` the returned
    tensors are views of its buffers, valid until its next use.

    ``exclude_ranges`` / ``exclude_records`` (see ``topk``) skip a range of rows per row, each
    row's own record: that search is ``topk`` at k = 1, whose column 0 is returned as ``[n]``
    views; it takes no ``NearestWorkspace`` (``ValueError``)."""
    if exclude_ranges is not None or exclude_records is not None:
        if workspace is not None:
            raise ValueError("exclude_ranges / exclude_records are served by topk: "
                             "no NearestWorkspace")
        values, indices = topk(a, b, k=1, metric=metric, exclude_self=exclude_self,
                               exclude_offset=exclude_offset, window_first=window_first,
                               exclude_ranges=exclude_ranges, exclude_records=exclude_records)
        return values[:, 0], indices[:, 0]
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
    if window_first is not None and (exclude_self or exclude_offset is not None):
        raise ValueError("window_first excludes the other exclusion arguments")
    if exclude_offset is None:
        exclude_offset = 0 if exclude_self else -1
    lib = native.library()
    n, m = a.shape[0], b.shape[0]
    with torch.cuda.device(a.device):
        need = lib.gfy_pairwise_workspace_bytes(n, m)
        if workspace is None:
            values = torch.empty(n, dtype=torch.float32, device=a.device)
            indices = torch.empty(n, dtype=torch.int32, device=a.device)
            scratch = torch.empty(need, dtype=torch.uint8, device=a.device)
        else:
            scratch, values, indices = workspace.buffers(a.device, n, need)
        if window_first is None:
            name, middle = "gfy_pairwise_nearest", (int(exclude_offset),)
        else:
            name, middle = "gfy_pairwise_nearest_window", (int(window_first),)
        native.check(getattr(lib, name)(
            a.data_ptr(), n, b.data_ptr(), m, _metric(metric), *middle,
            *_results(values, indices, scratch)), name)
    return values, indices


class TopKWorkspace:
    """Scratch memory and ``[n][k]`` result arrays of ``topk`` kept across calls, as
    ``NearestWorkspace`` keeps those of ``nearest``."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.values: torch.Tensor | None = None
        self.indices: torch.Tensor | None = None

    def buffers(self, device, rows: int, k: int, scratch_bytes: int):
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        self.values = _grown(self.values, device, rows * k, torch.float32)
        self.indices = _grown(self.indices, device, rows * k, torch.int32)
        return (self.scratch, self.values[:rows * k].view(rows, k),
                self.indices[:rows * k].view(rows, k))


def checked_k(k) -> int:
    """``k`` of a top-k search as an int; ``ValueError`` unless it is an integer (a numpy
    integer included, no bool) in 1..GFY_PAIRWISE_TOPK_MAX.  The one check of ``topk`` and of
    ``parallel.cross_shard_topk``."""
    try:
        if _checked_integer(k, "k", 1) <= native.GFY_PAIRWISE_TOPK_MAX:
            return int(k)
    except ValueError:
        pass
    raise ValueError(f"k must be an integer in 1..{native.GFY_PAIRWISE_TOPK_MAX}")


def topk(a, b=None, *, k: int, metric: str = "l2", exclude_self: bool = False,
         exclude_offset: int | None = None, window_first: int | None = None,
         exclude_ranges=None, exclude_records=None, distinct_records=None,
         workspace: TopKWorkspace | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """For every row of ``a`` the ``k`` best rows of ``b``, smallest L2 distance / largest
    cosine first: ``(values float32 [n, k], indices int32 [n, k])``, exact, the N×M matrix
    never written.  ``1 <= k <= 16``.

    A row's columns are ordered by (the kernel's fp32 key of the pair, b-row index): among equal
    keys the lowest index comes first, and no index appears twice.  The key is the one
    ``nearest`` minimises, computed the same way: column 0 equals ``nearest(...)`` bit for bit,
    ``topk(k=j)`` equals the first ``j`` columns of any call with a larger ``k`` bit for bit, and
    a row's result does not depend on the other rows of the call.  ``exclude_self``,
    ``exclude_offset`` and ``window_first`` are those of ``nearest``; an excluded pair appears
    in no column.  A row with fewer than ``k`` candidates fills its trailing columns with index
    -1 and value ``+inf`` (l2) / ``-inf`` (cosine).  With ``workspace`` the returned tensors
    are views of its buffers, valid until its next use.

    ``exclude_ranges=(lo, hi)``, two int32 arrays of length n (numpy or torch, on any device):
    row i skips the rows ``lo[i] <= j < hi[i]`` of ``b``.  The bounds may hold any value
    (``lo >= hi`` skips nothing, the comparison clips them to ``b``), rows are independent of each
    other, and everything above holds unchanged.  ``exclude_records=counts`` is the self-search
    form (``b`` omitted, or with n rows): the rows are grouped in records of ``counts`` rows, as
    ``Ginfinity.encode_graphs_device`` returns them, ``sum(counts) == n``, and every row skips its
    own record, itself included — ``exclude_ranges=record_ranges(counts)``.  The two exclude
    each other and the three single-pair arguments.  A search whose rows are sorted by record
    pays for the ranges only under each block's own records; arbitrary ranges are correct and
    not meant to be fast (include/gfy.h).

    ``distinct_records=counts_b``: the rows of ``b`` are grouped in contiguous records of
    ``counts_b`` rows (integers, ``sum(counts_b) == m``), and at most one row per record is
    returned: the ``k`` best rows that lie in ``k`` different records.  A record's representative
    for row i is its non-excluded row that is first in the order (key, b-row index); the result
    is the ``k`` best representatives in that order; a record with every row excluded has none.
    Keys, values, the -1 / ``inf`` columns behind the last record that has a representative, the
    prefix property and the independence of rows are as above, and with records of one row each
    the result is the one without the argument bit for bit.  It combines with every exclusion
    (the single-pair ones become ranges on the host); the search for the molecules that resemble
    each position is ``topk(rows, k=8, exclude_records=counts, distinct_records=counts)``, and
    ``record_of(indices, counts)`` names the records found.  ``k`` is at most
    ``GFY_PAIRWISE_TOPK_DISTINCT_MAX`` (16)."""
    k = checked_k(k)
    if distinct_records is not None and k > native.GFY_PAIRWISE_TOPK_DISTINCT_MAX:
        raise ValueError("k must be an integer in 1.."
                         f"{native.GFY_PAIRWISE_TOPK_DISTINCT_MAX} with distinct_records")
    if window_first is not None and (exclude_self or exclude_offset is not None):
        raise ValueError("window_first excludes the other exclusion arguments")
    code = _metric(metric)
    a = _checked(a)
    b = None if b is None else _checked(b)   # every argument error before a device is touched
    ranges = _checked_ranges(a.shape[0], None if b is None else b.shape[0], exclude_ranges,
                             exclude_records,
                             exclude_self or exclude_offset is not None or window_first is not None)
    groups = None
    if distinct_records is not None:
        n, m = a.shape[0], a.shape[0] if b is None else b.shape[0]
        groups = record_ranges(distinct_records)
        if groups[0].numel() != m:
            raise ValueError(f"distinct_records sums to {groups[0].numel()} rows, b has {m}")
        if ranges is None:   # the single-pair exclusions (or none) as ranges of one row (or none)
            ranges = _pair_ranges(n, exclude_self, exclude_offset, window_first)
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
    if ranges is not None:
        ranges = tuple(bound.to(a.device).contiguous() for bound in ranges)
    if groups is not None:
        groups = tuple(bound.to(a.device) for bound in groups)
    if exclude_offset is None:
        exclude_offset = 0 if exclude_self else -1
    lib = native.library()
    n, m = a.shape[0], b.shape[0]
    with torch.cuda.device(a.device):
        need = lib.gfy_pairwise_topk_workspace_bytes(n, m, k)
        if workspace is None:
            values = torch.empty((n, k), dtype=torch.float32, device=a.device)
            indices = torch.empty((n, k), dtype=torch.int32, device=a.device)
            scratch = torch.empty(need, dtype=torch.uint8, device=a.device)
        else:
            scratch, values, indices = workspace.buffers(a.device, n, k, need)
        if n == 0:
            return values, indices
        if groups is not None:
            name = "gfy_pairwise_topk_distinct"
            middle = tuple(bound.data_ptr() for bound in (*ranges, *groups))
        elif ranges is not None:
            name, middle = "gfy_pairwise_topk_ranges", tuple(bound.data_ptr() for bound in ranges)
        elif window_first is None:
            name, middle = "gfy_pairwise_topk", (int(exclude_offset),)
        else:
            name, middle = "gfy_pairwise_topk_window", (int(window_first),)
        native.check(getattr(lib, name)(
            a.data_ptr(), n, b.data_ptr(), m, code, k, *middle,
            *_results(values, indices, scratch)), name)
    return values, indices


class RecordWorkspace:
    """Scratch memory of ``record_best`` / ``record_scores`` kept across calls, as
    ``TopKWorkspace`` keeps that of ``topk`` (the results are always new tensors)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None

    def buffer(self, device, scratch_bytes: int) -> torch.Tensor:
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        return self.scratch


#: default ``max_workspace_bytes`` of ``record_scores``: the row-level intermediate of one block
RECORD_WORKSPACE_BYTES = 1 << 30


def _record_ptr(counts, rows: int, name: str, side: str) -> np.ndarray:
    """The running sums (int64, records + 1 entries) of ``counts``, which must sum to ``rows``."""
    counts = _checked_counts(counts)
    ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    if ptr[-1] != rows:
        raise ValueError(f"{name} sums to {int(ptr[-1])} rows, {side} has {rows}")
    if rows >= 2 ** 31 - 1:
        raise ValueError("record counts must sum to fewer than 2^31 - 1 rows")
    if counts.size > native.GFY_PAIRWISE_RECORDS_MAX:
        raise ValueError(f"{name} must hold at most {native.GFY_PAIRWISE_RECORDS_MAX} records")
    return ptr


def plan_record_blocks(counts_a, records_b: int, max_workspace_bytes: int) -> list[tuple[int, int]]:
    """How ``record_scores`` walks ``a``: half-open ranges ``(first, last)`` of records of ``a``,
    in order, that cover every record once.  A block is whole records, as many as fit: its rows
    times ``records_b`` words — the row-level intermediate of its native call — are at most
    ``max_workspace_bytes``.  A pure function of its arguments; a single record that alone
    exceeds the budget is a ``ValueError`` that names the bytes it needs."""
    counts = _checked_counts(counts_a)
    per_row = 4 * max(int(records_b), 0)
    budget = int(max_workspace_bytes)
    blocks, first, rows = [], 0, 0
    for q, count in enumerate(counts.tolist()):
        if count * per_row > budget:
            raise ValueError(f"record {q} of a has {count} rows and needs {count * per_row} bytes "
                             f"of workspace against {records_b} records of b: "
                             f"max_workspace_bytes is {budget}")
        if (rows + count) * per_row > budget:
            blocks.append((first, q))
            first, rows = q, 0
        rows += count
    if first < counts.size:
        blocks.append((first, int(counts.size)))
    return blocks


def _worst(code: int) -> float:
    """What a record of zero rows gives: no pair at all."""
    return float("inf") if code == native.GFY_L2 else float("-inf")


def record_best(a, b=None, *, counts_b, metric: str = "l2",
                workspace: RecordWorkspace | None = None) -> torch.Tensor:
    """For every row of ``a`` the best pair inside every record of ``b``: float32 ``[n, R]``,
    ``best[i, r]`` the smallest L2 distance / largest cosine between row i and the rows of
    record r, exact, the N×M matrix never written (the definitions are at the head of this
    module).  ``counts_b`` are the row counts of ``b``'s contiguous records, ``sum(counts_b) ==
    m``; a record of zero rows gives ``+inf`` (l2) / ``-inf`` (cosine).  Column r equals
    ``nearest(a, b[ptr[r]:ptr[r + 1]])`` values bit for bit.  Meant for blocks that fit in
    memory (n·R·4 bytes twice: the result and its transposed intermediate), as ``pairwise`` is.
    With ``b`` omitted ``a`` is searched against itself."""
    code = _metric(metric)
    a = _checked(a)
    b = None if b is None else _checked(b)   # every argument error before a device is touched
    n, m = a.shape[0], a.shape[0] if b is None else b.shape[0]
    ptr_b = _record_ptr(counts_b, m, "counts_b", "b")
    records = ptr_b.size - 1
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
    with torch.cuda.device(a.device):
        if n == 0 or records == 0 or m == 0:
            return torch.full((n, records), _worst(code), dtype=torch.float32, device=a.device)
        lib = native.library()
        best = torch.empty((n, records), dtype=torch.float32, device=a.device)
        need = lib.gfy_pairwise_record_workspace_bytes(n, m, 0, records)
        scratch = (workspace or RecordWorkspace()).buffer(a.device, need)
        ptr = torch.from_numpy(ptr_b.astype(np.int32)).to(a.device)
        native.check(lib.gfy_pairwise_record_best(
            a.data_ptr(), n, b.data_ptr(), m, code, ptr.data_ptr(), records, best.data_ptr(),
            *_scratch_tail(scratch, a.device)), "gfy_pairwise_record_best")
    return best


def record_scores(a, b=None, *, counts_a, counts_b=None, metric: str = "l2",
                  max_workspace_bytes: int = RECORD_WORKSPACE_BYTES,
                  workspace: RecordWorkspace | None = None) -> torch.Tensor:
    """How well every record of ``a`` matches every record of ``b``: float32 ``[Q, R]``,
    ``score[q, r]`` the mean over the rows i of record q of ``record_best(a, b)[i, r]`` — the
    float64 sum in ascending row order, divided by the record's rows, rounded to float32 once
    (the definitions are at the head of this module).  Exact and dense: the ranking by which to
    decide which pairs of records to align at all.  Small L2 scores / large cosine scores are
    good matches.  An a-record of zero rows gives a row of NaN, a b-record of zero rows a column
    of ``+inf`` (l2) / ``-inf`` (cosine).

    ``counts_a`` / ``counts_b`` are the row counts of the contiguous records of ``a`` / ``b``.
    With ``b`` omitted it is a self-search and ``counts_b`` defaults to ``counts_a``; nothing is
    excluded, so the diagonal holds 0 (l2) / 1 (cosine, up to rounding).  The score is
    directional, ``a`` onto ``b``: ``score(a, b)[q, r]`` and ``score(b, a)[r, q]`` differ, and
    a symmetric score is two calls combined by the caller.

    Neither the N×M matrix nor the n × R row-level intermediate is ever whole in memory: ``a``
    is walked in blocks of whole records (``plan_record_blocks``) whose intermediates take at
    most ``max_workspace_bytes`` each, one native call per block into the rows of the one
    result; the blocking does not change a bit of it.  A single record of ``a`` that alone
    exceeds the budget is a ``ValueError`` that names the bytes it needs."""
    code = _metric(metric)
    a = _checked(a)
    if b is None:
        counts_b = counts_a if counts_b is None else counts_b
    else:
        b = _checked(b)
        if counts_b is None:
            raise ValueError("counts_b is required with b: record counts of b's rows")
    n, m = a.shape[0], a.shape[0] if b is None else b.shape[0]
    ptr_a = _record_ptr(counts_a, n, "counts_a", "a")
    ptr_b = _record_ptr(counts_b, m, "counts_b", "b")
    queries, records = ptr_a.size - 1, ptr_b.size - 1
    max_workspace_bytes = _checked_integer(max_workspace_bytes, "max_workspace_bytes", 0)
    blocks = plan_record_blocks(np.diff(ptr_a), records, max_workspace_bytes)
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
    with torch.cuda.device(a.device):
        scores = torch.empty((queries, records), dtype=torch.float32, device=a.device)
        if queries == 0 or records == 0:
            return scores
        if n == 0 or m == 0:   # no pair at all: NaN for a record without rows, else the worst
            scores.fill_(_worst(code))
            empty = torch.from_numpy(np.diff(ptr_a) == 0).to(a.device)
            scores[empty] = float("nan")
            return scores
        lib = native.library()
        ptr_b_dev = torch.from_numpy(ptr_b.astype(np.int32)).to(a.device)
        # every block's running sums, counted from the block's first row: one upload
        relative = [ptr_a[first:last + 1] - ptr_a[first] for first, last in blocks]
        starts = np.concatenate(([0], np.cumsum([piece.size for piece in relative])))
        ptr_a_dev = torch.from_numpy(np.concatenate(relative).astype(np.int32)).to(a.device)
        keeper = workspace or RecordWorkspace()
        for (first, last), at in zip(blocks, starts.tolist()):
            row_lo, row_hi = int(ptr_a[first]), int(ptr_a[last])
            if row_hi == row_lo:   # records of zero rows only
                scores[first:last] = float("nan")
                continue
            rows = row_hi - row_lo
            need = lib.gfy_pairwise_record_workspace_bytes(rows, m, last - first, records)
            scratch = keeper.buffer(a.device, need)
            native.check(lib.gfy_pairwise_record_scores(
                a[row_lo:row_hi].data_ptr(), rows, b.data_ptr(), m, code,
                ptr_a_dev[at:].data_ptr(), last - first, ptr_b_dev.data_ptr(), records,
                scores[first:last].data_ptr(), *_scratch_tail(scratch, a.device)),
                "gfy_pairwise_record_scores")
    return scores


class Hits(NamedTuple):
    """What ``within`` returns: row i's hits are ``indices[offsets[i]:offsets[i + 1]]`` (rows of
    ``b``, ascending) with ``values`` next to them."""
    offsets: torch.Tensor   # int64 [n + 1]
    indices: torch.Tensor   # int32 [H]
    values: torch.Tensor    # float32 [H]

    def rows(self) -> torch.Tensor:
        """The a-row of every hit: int64 ``[H]``, row i repeated once per hit of its."""
        counts = self.offsets[1:] - self.offsets[:-1]
        return torch.repeat_interleave(
            torch.arange(counts.numel(), dtype=torch.int64, device=counts.device), counts)


class TooManyHits(RuntimeError):
    """``within(..., max_hits=...)`` found more hits than that; ``total`` is how many."""

    def __init__(self, total: int, max_hits: int) -> None:
        super().__init__(f"within: {total} hits, max_hits is {max_hits}")
        self.total = total
        self.max_hits = max_hits


class WithinWorkspace:
    """Scratch memory and the ``[n]`` counts of ``count_within`` / ``within`` kept across calls,
    as ``TopKWorkspace`` keeps those of ``topk`` (the hits are always new tensors)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.counts: torch.Tensor | None = None

    def buffers(self, device, rows: int, scratch_bytes: int):
        self.scratch = _grown(self.scratch, device, scratch_bytes, torch.uint8)
        self.counts = _grown(self.counts, device, rows, torch.int32)
        return self.scratch, self.counts[:rows]


def _checked_threshold(threshold) -> float:
    """``threshold`` rounded to float32 once; ``ValueError`` unless it is a real number (no bool)
    that is finite in float32."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer,
                                                                 np.floating)):
        raise ValueError("threshold must be a real number")
    with np.errstate(over="ignore"):
        rounded = float(np.float32(threshold))
    if not np.isfinite(rounded):
        raise ValueError("threshold must be finite in float32")
    return rounded


class _WithinCall:
    """The checked arguments of ``count_within`` / ``within`` (every argument error is raised
    here, before a device is touched), then the two native calls on them."""

    def __init__(self, a, b, threshold, metric, exclude_self, exclude_ranges, exclude_records,
                 workspace) -> None:
        self.threshold = _checked_threshold(threshold)
        self.code = _metric(metric)
        a = _checked(a)
        b = None if b is None else _checked(b)
        n = a.shape[0]
        ranges = _checked_ranges(n, None if b is None else b.shape[0], exclude_ranges,
                                 exclude_records, bool(exclude_self))
        if ranges is None and exclude_self:   # the pair (i, i) as a range of one row
            ranges = _pair_ranges(n, True, None, None)
        if workspace is not None and not isinstance(workspace, WithinWorkspace):
            raise ValueError("workspace must be a WithinWorkspace")
        self.keeper = workspace or WithinWorkspace()
        self.a = _prepare(a, None)
        self.b = self.a if b is None else _prepare(b, self.a.device)
        self.device = self.a.device
        self.n, self.m = self.a.shape[0], self.b.shape[0]
        self.ranges = None if ranges is None else tuple(
            bound.to(self.device).contiguous() for bound in ranges)

    def _front(self) -> tuple:
        skip = (None, None) if self.ranges is None else tuple(
            bound.data_ptr() for bound in self.ranges)
        return (self.a.data_ptr(), self.n, self.b.data_ptr(), self.m, self.code, self.threshold,
                *skip)

    def _back(self, scratch) -> tuple:
        return _scratch_tail(scratch, self.device)

    def buffers(self):
        need = native.library().gfy_pairwise_within_workspace_bytes(self.n, self.m)
        return self.keeper.buffers(self.device, self.n, need)

    def count(self) -> torch.Tensor:
        """int32 [n], a view of the workspace's buffer"""
        scratch, counts = self.buffers()
        if self.n == 0 or self.m == 0:
            return counts.zero_()
        native.check(native.library().gfy_pairwise_within_count(
            *self._front(), counts.data_ptr(), *self._back(scratch)),
            "gfy_pairwise_within_count")
        return counts

    def fill(self, offsets, total: int) -> tuple[torch.Tensor, torch.Tensor]:
        scratch, _ = self.buffers()
        indices = torch.empty(total, dtype=torch.int32, device=self.device)
        values = torch.empty(total, dtype=torch.float32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        native.check(native.library().gfy_pairwise_within_fill(
            *self._front(), offsets.data_ptr(), indices.data_ptr(), values.data_ptr(),
            status.data_ptr(), *self._back(scratch)), "gfy_pairwise_within_fill")
        if int(status.item()) != 0:
            raise native.NativeLibraryError(
                "gfy_pairwise_within_fill: the hits did not match the counted segments")
        return indices, values


def count_within(a, b=None, *, threshold=None, metric: str = "l2", exclude_self: bool = False,
                 exclude_ranges=None, exclude_records=None,
                 workspace: WithinWorkspace | None = None) -> torch.Tensor:
    """For every row of ``a`` the number of rows of ``b`` within ``threshold``: int32 ``[n]``,
    exact, the N×M matrix never written.  A pair is a hit iff its value — the one ``topk``
    reports, bit for bit — is ``<= threshold`` (l2) / ``>= threshold`` (cosine); ``threshold`` is
    required and rounded to float32 once (the definitions are at the head of this module).

    ``exclude_self`` (with ``b`` omitted or identical to ``a``) skips the pair (i, i);
    ``exclude_ranges=(lo, hi)`` and ``exclude_records=counts`` are those of ``topk``.  The three
    exclude each other; an excluded pair is not counted.  One sweep: the matrix-core work of
    ``nearest`` with a lighter epilogue.  With ``workspace`` the returned tensor is a view of its
    buffer, valid until its next use."""
    call = _WithinCall(a, b, threshold, metric, exclude_self, exclude_ranges, exclude_records,
                       workspace)
    with torch.cuda.device(call.device):
        return call.count()


def within(a, b=None, *, threshold=None, metric: str = "l2", exclude_self: bool = False,
           exclude_ranges=None, exclude_records=None, max_hits: int | None = None,
           workspace: WithinWorkspace | None = None) -> Hits:
    """For every row of ``a`` every row of ``b`` within ``threshold``: ``Hits(offsets int64
    [n + 1], indices int32 [H], values float32 [H])``; row i's hits are
    ``indices[offsets[i]:offsets[i + 1]]`` in ascending order of the row of ``b``, ``values``
    next to them (a ``torch.sort`` of a segment orders it by value).  Hits, values, exclusions
    and ``threshold`` are those of ``count_within``, whose result is ``offsets.diff()``.

    Two sweeps and a wait: the count, its running sum, the total copied to the host (which waits
    for the device), then the fill into exactly that many entries and the ordering of every
    row's segment.  ``max_hits``: a positive integer; a total above it raises ``TooManyHits``
    (which carries ``total``) before anything is allocated for the hits.  No rows, or no hit,
    returns empty ``indices`` / ``values`` without the second sweep."""
    if max_hits is not None:
        max_hits = _checked_integer(max_hits, "max_hits", 1)
    call = _WithinCall(a, b, threshold, metric, exclude_self, exclude_ranges, exclude_records,
                       workspace)
    with torch.cuda.device(call.device):
        offsets = torch.zeros(call.n + 1, dtype=torch.int64, device=call.device)
        total = 0
        if call.n > 0 and call.m > 0:
            torch.cumsum(call.count(), 0, dtype=torch.int64, out=offsets[1:])
            total = int(offsets[-1].item())   # waits for the device
        if max_hits is not None and total > max_hits:
            raise TooManyHits(total, max_hits)
        if total == 0:
            return Hits(offsets, torch.empty(0, dtype=torch.int32, device=call.device),
                        torch.empty(0, dtype=torch.float32, device=call.device))
        return Hits(offsets, *call.fill(offsets, total))


__all__ = ["pairwise", "nearest", "NearestWorkspace", "topk", "TopKWorkspace", "record_ranges",
           "record_of", "record_best", "record_scores", "RecordWorkspace", "plan_record_blocks",
           "count_within", "within", "Hits", "TooManyHits", "WithinWorkspace"]
