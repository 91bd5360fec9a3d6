"""Oracles of the null scores (ginfinity_amd/align.py: shuffle_orders, null_scores; include/gfy.h:
gfy_align_local_null) — checkers, never the code under test.

    shuffle_orders(columns, shuffles, seed)   the numpy twin of align.shuffle_orders: the formula
                                              of include/gfy.h in uint64, one virtual pair at a
                                              time
    side_of(record_b, box)                    the rows of a pair's b-side: the b-record, or the
                                              b-rows of the box clipped into it
    gathered(side, order)                     the b-side's rows copied out in the order of one
                                              run, as a record of its own: what null_scores must
                                              equal local_align on, bit for bit
    segment(order, order_ptr, columns, shuffles, p, k)
                                              the entries of run k of pair p
"""
from __future__ import annotations

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MIX_1, MIX_2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * MIX_1
        z = (z ^ (z >> np.uint64(27))) * MIX_2
    return z ^ (z >> np.uint64(31))


def keys(seed: int, v: int, count: int) -> np.ndarray:
    """key(seed, v, j) for j = 0 .. count - 1: uint64 values below 2^32."""
    with np.errstate(over="ignore"):
        head = mix(np.array([(int(seed) + (v + 1) * int(GOLDEN)) % (1 << 64)], dtype=np.uint64))
        j = np.arange(1, count + 1, dtype=np.uint64)
        return mix(head + j * GOLDEN) >> np.uint64(32)


def shuffle_orders(columns, shuffles: int, seed: int):
    """(order int32, order_ptr int64 [P + 1]) of align.shuffle_orders, by the formula."""
    columns = np.asarray(columns, dtype=np.int64)
    parts = []
    for p, count in enumerate(columns):
        for k in range(shuffles):
            parts.append(np.argsort(keys(seed, p * shuffles + k, int(count)), kind="stable"))
    order = np.concatenate(parts) if parts else np.zeros(0)
    return order.astype(np.int32), np.concatenate(([0], np.cumsum(columns) * shuffles)).astype(np.int64)


def side_of(record_b: np.ndarray, box=None) -> np.ndarray:
    if box is None:
        return record_b
    j_lo, j_hi = max(int(box[2]), 0), min(int(box[3]), record_b.shape[0] - 1)
    return record_b[j_lo:j_hi + 1] if j_lo <= j_hi else record_b[:0]


def gathered(side: np.ndarray, order: np.ndarray) -> np.ndarray:
    return side[np.asarray(order, dtype=np.int64)] if len(order) else side[:0]


def segment(order, order_ptr, columns, shuffles: int, p: int, k: int) -> np.ndarray:
    lo = int(order_ptr[p]) + k * int(columns[p])
    return np.asarray(order[lo:lo + int(columns[p])])
