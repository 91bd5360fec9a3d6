"""Hand-written runs and the chains ``align.chain_runs`` must make of them, written out literally:
test_chain_runs_host.py holds the oracle to them, test_gpu_chain_runs.py the device.

A run is ``(q, r, i, j, L)``; run s weighs ``2 ** s``, so that a chain's weight names its members.
A case is ``(runs, max_gap, max_shift, chains)`` with ``chains`` = ``(pairs, starts, ends,
diagonals, counts, lengths, weights, members)``."""
from __future__ import annotations

import numpy as np

INDEL = [(0, 0, 0, 10, 30), (0, 0, 30, 43, 27)]            # gi = 0, gj = 3
ONE = ([(0, 0)], [(0, 10)], [(56, 69)], [(10, 13)], [2], [57], [3.0], [0, 0])
APART = ([(0, 0)] * 2, [(0, 10), (30, 43)], [(29, 39), (56, 69)], [(10, 10), (13, 13)], [1, 1],
         [30, 27], [1.0, 2.0], [0, 1])

GAP = [(0, 0, 0, 0, 5), (0, 0, 8, 8, 4)]                   # gi = gj = 3
SHIFT = [(0, 0, 0, 0, 5), (0, 0, 5, 7, 4)]                 # gi = 0, gj = 2
# s -> t1 and s -> t2; t2 is longer, so s chooses it and t1, which chose s, starts its own chain
FORK = [(0, 0, 0, 0, 5), (0, 0, 6, 6, 3), (0, 0, 6, 8, 10)]
# both s1 and s2 precede t with C = 4: |dd| is 0 from s1 and 2 from s2, the larger index loses
TIE_SHIFT = [(0, 0, 0, 0, 4), (0, 0, 1, 3, 4), (0, 0, 7, 7, 5)]
# both precede t with C = 4 and |dd| = 1: the larger index wins
TIE_INDEX = [(0, 0, 0, 1, 4), (0, 0, 1, 0, 4), (0, 0, 6, 6, 5)]
# s precedes t1 and t2 with D = 3 and |dd| = 1: the smaller index wins
TIE_INDEX_BACK = [(0, 0, 0, 0, 4), (0, 0, 5, 6, 3), (0, 0, 6, 5, 3)]
# two record pairs interleaved in Runs order: run 0 would link to run 3 but for the pair
TWO_PAIRS = [(0, 0, 0, 0, 3), (0, 1, 0, 0, 3), (0, 0, 4, 4, 3), (0, 1, 4, 4, 3)]
# t starts in the last row of s: gi = -1
OVERLAP = [(0, 0, 0, 0, 5), (0, 0, 4, 6, 3)]

CASES = {
    "two runs link": (INDEL, 4, None, ONE),
    "two runs link, shift at max_shift": (INDEL, 4, 3, ONE),
    "two runs, shift at max_shift + 1": (INDEL, 4, 2, APART),
    "two runs, gap at max_gap": (INDEL, 3, None, ONE),
    "two runs, gap at max_gap + 1": (INDEL, 2, None, APART),
    "gap at max_gap": (GAP, 3, 0, ([(0, 0)], [(0, 0)], [(11, 11)], [(0, 0)], [2], [9], [3.0],
                                   [0, 0])),
    "gap at max_gap + 1": (GAP, 2, 2, ([(0, 0)] * 2, [(0, 0), (8, 8)], [(4, 4), (11, 11)],
                                       [(0, 0), (0, 0)], [1, 1], [5, 4], [1.0, 2.0], [0, 1])),
    "shift at max_shift": (SHIFT, 5, 2, ([(0, 0)], [(0, 0)], [(8, 10)], [(0, 2)], [2], [9], [3.0],
                                         [0, 0])),
    "shift at max_shift + 1": (SHIFT, 5, 1, ([(0, 0)] * 2, [(0, 0), (5, 7)], [(4, 4), (8, 10)],
                                             [(0, 0), (2, 2)], [1, 1], [5, 4], [1.0, 2.0],
                                             [0, 1])),
    "fork": (FORK, 3, None, ([(0, 0)] * 2, [(0, 0), (6, 6)], [(15, 17), (8, 8)],
                             [(0, 2), (0, 0)], [2, 1], [15, 3], [5.0, 2.0], [0, 1, 0])),
    "tie in C decided by |dd|": (TIE_SHIFT, 3, None,
                                 ([(0, 0)] * 2, [(0, 0), (1, 3)], [(11, 11), (4, 6)],
                                  [(0, 0), (2, 2)], [2, 1], [9, 4], [5.0, 2.0], [0, 1, 0])),
    "tie in C decided by index": (TIE_INDEX, 2, None,
                                  ([(0, 0)] * 2, [(0, 1), (1, 0)], [(3, 4), (10, 10)],
                                   [(1, 1), (-1, 0)], [1, 2], [4, 9], [1.0, 6.0], [0, 1, 1])),
    "tie in D decided by index": (TIE_INDEX_BACK, 2, None,
                                  ([(0, 0)] * 2, [(0, 0), (6, 5)], [(7, 8), (8, 7)],
                                   [(0, 1), (-1, -1)], [2, 1], [7, 3], [3.0, 4.0], [0, 0, 1])),
    "two pairs interleaved": (TWO_PAIRS, 1, None,
                              ([(0, 0), (0, 1)], [(0, 0), (0, 0)], [(6, 6), (6, 6)],
                               [(0, 0), (0, 0)], [2, 2], [6, 6], [5.0, 10.0], [0, 1, 0, 1])),
    "overlap in i only": (OVERLAP, 5, None,
                          ([(0, 0)] * 2, [(0, 0), (4, 6)], [(4, 4), (6, 8)], [(0, 0), (2, 2)],
                           [1, 1], [5, 3], [1.0, 2.0], [0, 1])),
}


def runs_of(entries):
    """``(pairs, cells, lengths, weights)`` of a case's runs, with ``hit_runs``' dtypes."""
    entries = np.asarray(entries, dtype=np.int32).reshape(-1, 5)
    return (entries[:, :2].copy(), entries[:, 2:4].copy(), entries[:, 4].copy(),
            (2.0 ** np.arange(len(entries))).astype(np.float32))


def chains_of(expected):
    """A case's chains as the eight arrays of ``align.Chains``."""
    pairs, starts, ends, diagonals, counts, lengths, weights, members = expected
    return (*(np.asarray(x, dtype=np.int32).reshape(-1, 2)
              for x in (pairs, starts, ends, diagonals)),
            np.asarray(counts, dtype=np.int32), np.asarray(lengths, dtype=np.int32),
            np.asarray(weights, dtype=np.float32), np.asarray(members, dtype=np.int32))
