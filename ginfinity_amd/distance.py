"""All-pairs L2 / cosine distance over 128-d fp16 embeddings on the matrix cores.

The reference has no implementation of this step (its aligner is the external
``ginfinity-sw`` package; src/ginfinity/api.py:47-50 only exports scoring
parameters), so the semantics are defined here and in include/gfy.h:

    L2      D_ij = sqrt(max(|a_i|² + |b_j|² − 2 a_i·b_j, 0))
    cosine  S_ij = a_i·b_j / (max(|a_i|, 1e-12) · max(|b_j|, 1e-12))

Inputs are fp16 device tensors as produced by ``Ginfinity.encode_graphs_device``;
products are exact, accumulation is fp32 (MFMA).  ``nearest`` and ``topk`` never
materialise the N×M matrix.
"""
from __future__ import annotations

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
            scratch.data_ptr(), scratch.numel(),
            torch.cuda.current_stream(a.device).cuda_stream),
            "gfy_pairwise_dense")
    return out


class NearestWorkspace:
    """Scratch memory and result arrays of ``nearest`` kept across calls (the chunked
    cross-shard search calls it once per rank's piece and chunk: allocating per call costs
    more than small searches)."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.values: torch.Tensor | None = None
        self.indices: torch.Tensor | None = None

    def buffers(self, device, rows: int, scratch_bytes: int):
        if self.scratch is None or self.scratch.numel() < scratch_bytes or \
                self.scratch.device != device:
            self.scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device=device)
        if self.values is None or self.values.numel() < rows or self.values.device != device:
            self.values = torch.empty(max(rows, 1), dtype=torch.float32, device=device)
            self.indices = torch.empty(max(rows, 1), dtype=torch.int32, device=device)
        return self.scratch, self.values[:rows], self.indices[:rows]


def nearest(a, b=None, *, metric: str = "l2", exclude_self: bool = False,
            exclude_offset: int | None = None, window_first: int | None = None,
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
    tensors are views of its buffers, valid until its next use."""
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
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if window_first is None:
            native.check(lib.gfy_pairwise_nearest(
                a.data_ptr(), n, b.data_ptr(), m, _metric(metric),
                int(exclude_offset), values.data_ptr(), indices.data_ptr(),
                scratch.data_ptr(), scratch.numel(), stream), "gfy_pairwise_nearest")
        else:
            native.check(lib.gfy_pairwise_nearest_window(
                a.data_ptr(), n, b.data_ptr(), m, _metric(metric), int(window_first),
                values.data_ptr(), indices.data_ptr(), scratch.data_ptr(), scratch.numel(),
                stream), "gfy_pairwise_nearest_window")
    return values, indices


class TopKWorkspace:
    """Scratch memory and ``[n][k]`` result arrays of ``topk`` kept across calls, as
    ``NearestWorkspace`` keeps those of ``nearest``."""

    def __init__(self) -> None:
        self.scratch: torch.Tensor | None = None
        self.values: torch.Tensor | None = None
        self.indices: torch.Tensor | None = None

    def buffers(self, device, rows: int, k: int, scratch_bytes: int):
        if self.scratch is None or self.scratch.numel() < scratch_bytes or \
                self.scratch.device != device:
            self.scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device=device)
        if self.values is None or self.values.numel() < rows * k or self.values.device != device:
            self.values = torch.empty(max(rows * k, 1), dtype=torch.float32, device=device)
            self.indices = torch.empty(max(rows * k, 1), dtype=torch.int32, device=device)
        return (self.scratch, self.values[:rows * k].view(rows, k),
                self.indices[:rows * k].view(rows, k))


def checked_k(k) -> int:
    """``k`` of a top-k search as an int; ``ValueError`` unless it is an integer (a numpy
    integer included, no bool) in 1..GFY_PAIRWISE_TOPK_MAX.  The one check of ``topk`` and of
    ``parallel.cross_shard_topk``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or \
            not 1 <= k <= native.GFY_PAIRWISE_TOPK_MAX:
        raise ValueError(f"k must be an integer in 1..{native.GFY_PAIRWISE_TOPK_MAX}")
    return int(k)


def topk(a, b=None, *, k: int, metric: str = "l2", exclude_self: bool = False,
         exclude_offset: int | None = None, window_first: int | None = None,
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
    are views of its buffers, valid until its next use."""
    k = checked_k(k)
    if window_first is not None and (exclude_self or exclude_offset is not None):
        raise ValueError("window_first excludes the other exclusion arguments")
    code = _metric(metric)
    a = _checked(a)
    b = None if b is None else _checked(b)   # every argument error before a device is touched
    a = _prepare(a, None)
    b = a if b is None else _prepare(b, a.device)
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
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if n == 0:
            return values, indices
        if window_first is None:
            native.check(lib.gfy_pairwise_topk(
                a.data_ptr(), n, b.data_ptr(), m, code, k, int(exclude_offset),
                values.data_ptr(), indices.data_ptr(), scratch.data_ptr(), scratch.numel(),
                stream), "gfy_pairwise_topk")
        else:
            native.check(lib.gfy_pairwise_topk_window(
                a.data_ptr(), n, b.data_ptr(), m, code, k, int(window_first),
                values.data_ptr(), indices.data_ptr(), scratch.data_ptr(), scratch.numel(),
                stream), "gfy_pairwise_topk_window")
    return values, indices


__all__ = ["pairwise", "nearest", "NearestWorkspace", "topk", "TopKWorkspace"]
