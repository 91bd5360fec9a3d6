"""Multi-GPU operation: one process per GPU, ``torch.distributed`` over RCCL.

The reference has no distributed code — it delegates to an external scheduler
running one process per shard (docs/GRAPH_PIPELINE.md:22-24).  On an 8-GPU
MI355X node the same decomposition maps to ranks:

* **encode is shard-parallel and needs no collective** — graphs never share
  edges across records (graph.py:392-395), weights (0.6 MB) are replicated,
  rank r encodes shards r, r+W, r+2W, …;
* **the one exchange step** is the cross-shard nearest-neighbour search (one neighbour:
  ``cross_shard_nearest``, the k nearest: ``cross_shard_topk``): the fp16
  embedding blocks are all-gathered in chunks (``all_gather_into_tensor`` per chunk into
  one of two staging buffers — RCCL over xGMI on GPUs, gloo on CPU tensors in the tests)
  and every chunk is searched against the rank's own rows while the next one is in
  flight; per row the best (value, global row) is merged on the device.  Row reductions
  stay on the rank that owns the row: no second collective.

With world size 1 (or no process group) every function degenerates to the
single-GPU path without touching ``torch.distributed``.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.distributed as dist


def world(group=None) -> tuple[int, int]:
    """(rank, world_size); (0, 1) when no process group is initialised."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def shard_assignment(n_shards: int, world_size: int, rank: int) -> list[int]:
    """Round-robin shard ownership: shard s belongs to rank s mod W."""
    if not 0 <= rank < world_size:
        raise ValueError("rank outside the world")
    return list(range(rank, n_shards, world_size))


def encode_owned_shards(encoder, shards: Sequence, *, group=None,
                        max_batch_nodes: int = 60_000,
                        max_batch_edges: int = 300_000
                        ) -> tuple[torch.Tensor, list[int], list[tuple[int, ...]]]:
    """Encode this rank's share of ``shards`` (no communication).

    Returns (fp16 device block of all owned core rows, owned shard indices,
    per-shard per-record row counts)."""
    rank, size = world(group)
    owned = shard_assignment(len(shards), size, rank)
    if owned:   # all owned shards in one call: their micro-batches share launches in groups
        merged, counts = encoder.encode_shards_device(
            [shards[index] for index in owned], max_batch_nodes=max_batch_nodes,
            max_batch_edges=max_batch_edges)
    else:
        counts = []
        merged = torch.empty((0, 128), dtype=torch.float16,
                             device=encoder._engine.device)
    return merged, owned, counts


def all_gather_rows(block: torch.Tensor, group=None
                    ) -> tuple[torch.Tensor, list[int]]:
    """Gather ``[rows_r, 128]`` blocks of all ranks into one ``[sum rows, 128]``
    tensor in rank order; returns it with the row offset of every rank's block
    (length W+1).  Blocks may differ in size: they are padded to the largest
    for one equal-count ``all_gather_into_tensor`` and compacted afterwards.
    For SMALL exchanges (manifests, tests): the search path, ``cross_shard_nearest``,
    gathers in chunks and never holds all rows at once."""
    rank, size = world(group)
    rows = int(block.shape[0])
    if size == 1:
        return block, [0, rows]
    counts = torch.tensor([rows], dtype=torch.int64, device=block.device)
    all_counts = torch.empty(size, dtype=torch.int64, device=block.device)
    dist.all_gather_into_tensor(all_counts, counts, group=group)
    sizes = [int(v) for v in all_counts.tolist()]
    widest = max(sizes)
    padded = block
    if rows < widest:
        padded = torch.zeros((widest, block.shape[1]), dtype=block.dtype,
                             device=block.device)
        padded[:rows] = block
    gathered = torch.empty((size * widest, block.shape[1]), dtype=block.dtype,
                           device=block.device)
    dist.all_gather_into_tensor(gathered, padded.contiguous(), group=group)
    offsets = [0]
    for value in sizes:
        offsets.append(offsets[-1] + value)
    if all(value == widest for value in sizes):
        return gathered, offsets
    pieces = [gathered[r * widest:r * widest + sizes[r]] for r in range(size)]
    return torch.cat(pieces, dim=0), offsets


def _exchange(block: torch.Tensor, group, chunk_rows: int):
    """The chunked exchange of ``cross_shard_nearest`` and ``cross_shard_topk``: returns
    ``(rank, offsets, pieces)``.  ``offsets`` is the row offset of every rank's block (W + 1
    entries, from one small ``all_gather_into_tensor`` of the sizes, done here).  ``pieces`` is a
    generator of ``(other_rank, first, piece)``: ``piece`` is rows ``[first, first + len(piece))``
    of ``other_rank``'s block, every non-empty piece of every rank once, chunk by chunk, and
    nothing when this rank has no rows (it still takes part in every collective).  A chunk is one
    equal-count ``all_gather_into_tensor`` of at most ``chunk_rows`` rows per rank into one of two
    staging buffers; chunk c+1 is started before chunk c's pieces are handed out, so it is in
    flight under whatever the caller does with them, and a piece is valid until the caller asks
    for the first piece of the next chunk.  The collectives of the chunks run as the generator is
    advanced: every rank must exhaust it (a rank that stops early leaves the others waiting in
    an ``all_gather``).  With world size 1 the pieces are slices of ``block`` and
    ``torch.distributed`` is not touched."""
    rank, size = world(group)
    rows = int(block.shape[0])
    device = block.device
    if size > 1:
        mine = torch.tensor([rows], dtype=torch.int64, device=device)
        everyone = torch.empty(size, dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(everyone, mine, group=group)
        sizes = [int(v) for v in everyone.tolist()]
    else:
        sizes = [rows]
    offsets = [0]
    for value in sizes:
        offsets.append(offsets[-1] + value)
    widest = max(sizes)
    chunk_rows = max(1, min(int(chunk_rows), max(widest, 1)))
    chunks = (widest + chunk_rows - 1) // chunk_rows
    if size > 1:
        staging = [torch.empty((size, chunk_rows, block.shape[1]), dtype=block.dtype, device=device)
                   for _ in range(min(2, max(chunks, 1)))]
        outgoing = [torch.zeros((chunk_rows, block.shape[1]), dtype=block.dtype, device=device)
                    for _ in range(len(staging))]

    def start(chunk: int):
        first = chunk * chunk_rows
        have = max(0, min(rows - first, chunk_rows))
        buffer = outgoing[chunk % len(outgoing)]
        if have:
            buffer[:have] = block[first:first + have]
        return dist.all_gather_into_tensor(
            staging[chunk % len(staging)].view(size * chunk_rows, block.shape[1]), buffer,
            group=group, async_op=True)

    def pieces():
        pending = start(0) if size > 1 and chunks else None
        for chunk in range(chunks):
            first = chunk * chunk_rows
            if size > 1:
                arriving = pending
                pending = start(chunk + 1) if chunk + 1 < chunks else None   # under the search
                arriving.wait()
            for other in range(size):
                valid = max(0, min(sizes[other] - first, chunk_rows))
                if valid == 0 or rows == 0:
                    continue
                yield other, first, (staging[chunk % len(staging)][other, :valid] if size > 1
                                     else block[first:first + valid])

    return rank, offsets, pieces()


def _search_block(search, local: torch.Tensor, other: torch.Tensor, metric: str,
                  own_first: int | None, workspace=None) -> tuple[torch.Tensor, torch.Tensor]:
    """``search(local, other)``; when ``other`` is rows [own_first, own_first + len(other)) of
    ``local`` itself, every row skips itself (``window_first``: one call for the rows in front
    of the window, inside it and behind it)."""
    extra = {} if workspace is None else {"workspace": workspace}
    if own_first is None:
        return search(local, other, metric=metric, **extra)
    return search(local, other, metric=metric, window_first=own_first, **extra)


def cross_shard_nearest(block: torch.Tensor, *, metric: str = "l2", group=None,
                        chunk_rows: int = 1 << 20, search=None
                        ) -> tuple[torch.Tensor, torch.Tensor, list[int]]:
    """Nearest other embedding, over ALL ranks' rows, of every local row.

    The blocks are exchanged in chunks of ``chunk_rows`` rows per rank — one equal-count
    ``all_gather_into_tensor`` per chunk into one of two staging buffers (RCCL over xGMI;
    the gathered 15.7 GB of BASELINE configs[4] never exist at once, nothing is compacted
    or copied a second time) — and chunk k is searched (``distance.nearest`` on the matrix
    cores, one call per rank's piece) while chunk k+1 is in flight.  Per local row the
    best (value, global row) is merged on the device; ties go to the lowest global row.
    Rows of other ranks never leave the rank that owns the query row, so there is no second
    collective.  A rank without rows takes part in the collectives and returns empty
    results.  With world size 1 the same code runs without ``torch.distributed``.

    Returns (values float32 [rows_r], global row indices int64 [rows_r], rank offsets W+1).
    ``search`` (tests) replaces ``distance.nearest``."""
    workspace = None
    if search is None:
        from . import distance
        search = distance.nearest
        workspace = distance.NearestWorkspace()     # one set of buffers for every piece
    if metric not in ("l2", "cosine"):
        raise ValueError("metric must be 'l2' or 'cosine'")
    rank, offsets, pieces = _exchange(block, group, chunk_rows)
    rows = int(block.shape[0])
    worse = float("inf") if metric == "l2" else float("-inf")
    best_value = torch.full((rows,), worse, dtype=torch.float32, device=block.device)
    best_index = torch.full((rows,), -1, dtype=torch.int64, device=block.device)
    for other, first, piece in pieces:
        values, indices = _search_block(search, block, piece, metric,
                                        first if other == rank else None, workspace)
        indices = indices.to(torch.int64) + (offsets[other] + first)
        better = (values < best_value) if metric == "l2" else (values > best_value)
        better |= (values == best_value) & (indices < best_index)
        best_value = torch.where(better, values, best_value)
        best_index = torch.where(better, indices, best_index)
    return best_value, best_index, offsets


_NO_ROW = torch.iinfo(torch.int64).max   # an empty slot while lists are merged: behind every row


def _merge_topk(best_value, best_index, values, indices, k: int, metric: str):
    """The k best of two [rows][k] lists by (value, global row): smallest value first for l2,
    largest for cosine, ties to the lowest global row; empty slots (row _NO_ROW) go last.
    Two stable sorts: by row, then by value."""
    value = torch.cat([best_value, values], dim=1)
    index = torch.cat([best_index, indices], dim=1)
    by_row = torch.argsort(index, dim=1, stable=True)
    value, index = value.gather(1, by_row), index.gather(1, by_row)
    by_value = torch.argsort(value if metric == "l2" else -value, dim=1, stable=True)[:, :k]
    return value.gather(1, by_value), index.gather(1, by_value)


def cross_shard_topk(block: torch.Tensor, k: int, *, metric: str = "l2", group=None,
                     chunk_rows: int = 1 << 20, search=None, record_counts=None
                     ) -> tuple[torch.Tensor, torch.Tensor, list[int]]:
    """The ``k`` nearest other embeddings, over ALL ranks' rows, of every local row.

    The exchange is ``cross_shard_nearest``'s (``_exchange``): chunks of ``chunk_rows`` rows per
    rank, one equal-count ``all_gather_into_tensor`` per chunk into one of two staging buffers, chunk
    c searched while chunk c+1 is in flight.  Per piece one ``distance.topk`` call (the rank's
    own piece with ``window_first``), whose ``[rows][k]`` lists are merged into the running
    ones on the device by (value, global row), keeping ``k``; ties go to the lowest global
    row.  A row with fewer than ``k`` other rows in the whole world fills its trailing columns
    with row -1 and value ``+inf`` (l2) / ``-inf`` (cosine).  A rank without rows takes part
    in the collectives and returns empty results.

    ``record_counts``: the rank's own rows are grouped in records of that many rows each (the
    counts ``encode_owned_shards`` returns, flattened; they sum to the rank's rows, and a record
    never spans ranks since shards are whole), and every row skips its whole own record, itself
    included, instead of itself alone: the rank's own pieces are searched with
    ``exclude_ranges`` (``distance.record_ranges``, built once per call and shifted to the piece)
    instead of ``window_first``; the other ranks' pieces as before.

    The merged order is that of the VALUES, not of the kernel's keys.  ``distance.topk`` orders
    a row by (fp32 key, row), and two pairs with different keys can round to the same fp32 value
    (the l2 value is ``sqrt(max(|a|² + key, 0))``; keys within about 3e-7 of each other for unit
    rows).  Two such neighbours stand here in row order, in a plain ``distance.topk`` call over
    the same rows in key order: the same rows and the same values, two adjacent columns
    exchanged — for random unit rows about one row in 10^4 at k = 8.  So this function equals
    ``distance.topk`` bit for bit only on data without such a pair; what it guarantees on any
    data is the order (value, global row) stated above.

    Returns (values float32 [rows_r][k], global rows int64 [rows_r][k], rank offsets W+1).
    ``search`` (tests) replaces ``distance.topk``."""
    from . import distance
    workspace = None
    if search is None:
        search = distance.topk
        workspace = distance.TopKWorkspace()     # one set of buffers for every piece
    if metric not in ("l2", "cosine"):
        raise ValueError("metric must be 'l2' or 'cosine'")
    k = distance.checked_k(k)                    # the check of distance.topk
    rows = int(block.shape[0])
    own = None
    if record_counts is not None:
        own = distance.record_ranges(record_counts, block.device)   # once: own pieces shift it
        if own[0].numel() != rows:
            raise ValueError(f"record_counts sums to {own[0].numel()} rows, the block has {rows}")
    rank, offsets, pieces = _exchange(block, group, chunk_rows)
    worse = float("inf") if metric == "l2" else float("-inf")
    best_value = torch.full((rows, k), worse, dtype=torch.float32, device=block.device)
    best_index = torch.full((rows, k), _NO_ROW, dtype=torch.int64, device=block.device)
    for other, first, piece in pieces:
        extra = {} if workspace is None else {"workspace": workspace}
        if other == rank and own is None:
            extra["window_first"] = first
        elif other == rank:      # in the piece's row numbers; subsumes the self-exclusion
            extra["exclude_ranges"] = (own[0] - first, own[1] - first)
        values, indices = search(block, piece, k=k, metric=metric, **extra)
        indices = indices.to(torch.int64)
        indices = torch.where(indices < 0, _NO_ROW, indices + (offsets[other] + first))
        best_value, best_index = _merge_topk(best_value, best_index, values, indices, k, metric)
    best_index = torch.where(best_index == _NO_ROW, -1, best_index)
    return best_value, best_index, offsets


__all__ = ["world", "shard_assignment", "encode_owned_shards",
           "all_gather_rows", "cross_shard_nearest", "cross_shard_topk"]
