"""One small library of records with known relations, for the tests that run the search chain on
encoder output — shared by test_search_chain_host.py and test_gpu_search_chain.py.  Nothing here
is the code under test, and nothing is computed at import.

    library()                  the 27 records: records 0..23 of tests/golden/rouskin_sample_6k.tsv
                               whole (47 to 341 nt), then JOIN, COPY and WINDOW
    JOIN    (record 24)        records 1 and 7 (91 and 75 nt) as one molecule: sequence + sequence,
                               structure + structure, balanced because both parts are
    COPY    (record 25)        record 0 again under another identifier: the last whole record
    WINDOW  (record 26)        record 8 (289 nt) as the window [WINDOW_START, WINDOW_END), which
                               cuts the stem that closes the molecule's first domain; encoded with
                               ``keep_paired_neighbours=True, context_hops=2``
    encode_library(encoder)    (rows, counts): on a GPU the whole records through
                               ``encode_graphs_device`` (``encode_whole``) and WINDOW through
                               ``encode_many`` behind them (``append_window``), one device block;
                               on ``device="cpu"`` one numpy block
    seeds_from_hits(...)       the recipe of ``align.band_around``'s docstring, as typed there
    planted()                  the pairs whose relation says what an alignment must give
    FLANKED                    (4, 5), (4, 9), (5, 9): see below
    PARAMETERS                 two dyadic-gap parameter sets
    bound(...), relation(...)  the score bound of tests/test_gpu_align.py, and whether the
                               float64 definition gives a planted pair's relation and by how much

The sample table holds no molecule twice (``duplicate_groups`` finds none in its 5,840 records,
and the host test asserts it): records 4, 5 and 9 have 177 nt each but different inserts.  What
they share, with records 14 and 23, are the two adapters of their library — the first 26 nt of
the sequence and the last 21 nt, sequence and structure — and rows inside an adapter are
bit-identical from record to record.  That is where the groups of identical rows among the sample
records come from.  The three pairs therefore have no full diagonal to find; they take part in
every comparison with an oracle, which needs no relation, and the host test states what does
hold for them."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
SAMPLE = 24
JOINED = (1, 7)
JOIN, COPY, WINDOW = 24, 25, 26
RECORDS = 27
WINDOWED = 8
#: [34, 197) of record 8: position 34 lies inside the arm ``(((((`` 33..37 (47, the partner of 33,
#: is in the window), the rows 70..82 are paired with 0..12 in front of the window and the rows
#: 181..188 and 191..194 with 221..235 behind it: stems cut on both sides
WINDOW_START, WINDOW_END = 34, 197
WINDOW_OPTIONS = dict(keep_paired_neighbours=True, context_hops=2)    # test_gpu_call_pipeline.py
FLANKED = ((4, 5), (4, 9), (5, 9))
#: (match_scale, match_shift, gap_open, gap_extend), the gap costs dyadic.  A record's rows
#: inside JOIN are not its rows alone: the cosines along the planted diagonals go down to 0.268
#: for record 1 and 0.471 for record 7.  A diagonal is found whole only under a shift above minus
#: its weakest cosine, and -0.25 and -0.125 are dyadic ones: PARAMETERS.  The shift -0.3 of
#: tests/test_gpu_align.py scores the last cells of (1, JOIN) below 0 and a shift of -0.5 the
#: first cells of (7, JOIN) too, by the float64 definition itself: STEEPER_SHIFTS do not find the
#: JOIN diagonals whole, which the host test asserts.
STEEPER_SHIFTS = ((1.0, -0.3, 1.0, 0.25), (1.0, -0.5, 1.0, 0.5))
PARAMETERS = ((1.0, -0.25, 1.0, 0.25), (1.0, -0.125, 1.0, 0.5))
COSINE_TOL = 2e-6        # tests/test_gpu_distance_ranges.py


@functools.lru_cache(maxsize=None)
def sample_records() -> tuple:
    from ginfinity_amd import read_rna_table
    return tuple(read_rna_table(GOLDEN / "rouskin_sample_6k.tsv"))


def duplicate_groups(records) -> list:
    """The groups of two or more ``records`` with equal sequence and structure, as indices."""
    groups: dict = {}
    for index, record in enumerate(records):
        groups.setdefault((record.sequence, record.structure), []).append(index)
    return [group for group in groups.values() if len(group) > 1]


@functools.lru_cache(maxsize=None)
def library() -> tuple:
    """The 27 records; WINDOW, the only sliced one, is the last."""
    from ginfinity_amd import RNA
    sample = sample_records()[:SAMPLE]
    first, second = (sample[index] for index in JOINED)
    join = RNA("join_1_7", first.sequence + second.sequence, first.structure + second.structure)
    copy = RNA("copy_of_0", sample[0].sequence, sample[0].structure)
    whole = sample[WINDOWED]
    window = RNA("window_of_8", whole.sequence, whole.structure, WINDOW_START, WINDOW_END)
    records = (*sample, join, copy, window)
    assert len(records) == RECORDS and records[JOIN] is join and records[COPY] is copy
    assert not any(record.sliced for record in records[:WINDOW]) and records[WINDOW].sliced
    return records


def lengths() -> tuple:
    return tuple(record.core_length for record in library())


def encode_whole(encoder):
    """``(block, counts)`` of the 26 whole records on a GPU, as ``encode_graphs_device`` returns
    them: nothing is copied or waited for here."""
    from ginfinity_amd import GraphBuilder
    return encoder.encode_graphs_device(GraphBuilder().build_shard(list(library()[:WINDOW])))


def append_window(encoder, block, counts):
    """``(rows, counts)`` of the library from ``encode_whole``'s results: WINDOW's array of
    ``encode_many`` uploaded behind the block and counted behind the counts."""
    import torch
    tail = encoder.encode_many([library()[WINDOW]], **WINDOW_OPTIONS)[0]
    rows = torch.cat([block, torch.from_numpy(np.ascontiguousarray(tail)).to(block.device)])
    return rows, (*counts, tail.shape[0])


def encode_library(encoder):
    """``(rows, counts)`` of the library under ``encoder``, a ``Ginfinity``.  On a GPU:
    ``append_window`` of ``encode_whole``, one device block.  On ``device="cpu"`` everything comes
    from ``encode_many``: one float16 numpy block."""
    if encoder.device != "cpu":
        return append_window(encoder, *encode_whole(encoder))
    records = library()
    arrays = encoder.encode_many(list(records[:WINDOW])) + \
        encoder.encode_many([records[WINDOW]], **WINDOW_OPTIONS)
    return np.concatenate(arrays), tuple(array.shape[0] for array in arrays)


def seeds_from_hits(rows, idx_column, counts_a, counts_b):
    """``(q, r, seeds)`` of the hits (row ``rows[x]`` of a, row ``idx_column[x]`` of b): the recipe
    in the docstring of ``align.band_around``, with ``idx_column`` for its ``idx[rows, k]``.
    Torch or numpy, whichever ``rows`` is; the counts are arrays of the same library, on the
    device of ``rows``, as the docstring says they must be."""
    import torch
    from ginfinity_amd import distance
    if isinstance(rows, torch.Tensor):
        stack, cumsum = torch.stack, functools.partial(torch.cumsum, dim=0)
    else:
        stack, cumsum = np.stack, np.cumsum
    q, r = distance.record_of(rows, counts_a), distance.record_of(idx_column, counts_b)
    seeds = stack([rows - cumsum(counts_a)[q] + counts_a[q],          # minus the record's
                   idx_column - cumsum(counts_b)[r] + counts_b[r]], 1)    # first row
    return q, r, seeds


class Planted:
    """A pair (a-record, b-record) and what its relation says: ``mode`` is "local", "global" or
    "within"; the alignment is the diagonal of ``length`` matches from ``start`` to ``end``."""

    def __init__(self, pair, mode, start, length):
        self.pair, self.mode, self.start, self.length = pair, mode, start, length
        self.end = (start[0] + length - 1, start[1] + length - 1)

    def __repr__(self):
        return f"Planted({self.pair}, {self.mode}, {self.start}..{self.end})"


@functools.lru_cache(maxsize=None)
def planted() -> tuple:
    n = lengths()
    first, second = JOINED
    return (Planted((0, COPY), "local", (0, 0), n[0]),
            Planted((0, COPY), "global", (0, 0), n[0]),
            Planted((first, JOIN), "local", (0, 0), n[first]),
            Planted((second, JOIN), "local", (0, n[first]), n[second]),
            Planted((WINDOW, WINDOWED), "within", (0, WINDOW_START), n[WINDOW]))


def whole_record_pairs() -> tuple:
    """The planted pairs of two whole records, both ways round where both hold a full copy."""
    return ((0, COPY), (COPY, 0), (JOINED[0], JOIN), (JOINED[1], JOIN))


def pointers(counts) -> np.ndarray:
    return np.concatenate(([0], np.cumsum(np.asarray(counts, dtype=np.int64))))


def record_rows(rows: np.ndarray, counts, record: int) -> np.ndarray:
    ptr = pointers(counts)
    return rows[ptr[record]:ptr[record + 1]]


def twin_rows(rows: np.ndarray, counts):
    """``(twins, groups, largest)``: how many rows are bit-identical to a row of another record,
    in how many groups of identical rows, and the most copies a group has."""
    inverse = row_groups(rows)
    sizes = np.bincount(inverse)
    record = np.repeat(np.arange(len(counts)), counts)
    low = np.full(sizes.size, len(counts))
    high = np.full(sizes.size, -1)
    np.minimum.at(low, inverse, record)
    np.maximum.at(high, inverse, record)
    spans = high > low                             # the group has rows of two records or more
    return int(spans[inverse].sum()), int(spans.sum()), int(sizes[spans].max(initial=0))


def row_groups(rows: np.ndarray) -> np.ndarray:
    """For every row the number of its group of bit-identical rows (equal numbers: equal bytes)."""
    keys = np.ascontiguousarray(rows).view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1])))
    return np.unique(keys.ravel(), return_inverse=True)[1]


def tied_tops(cosine: np.ndarray, rows: np.ndarray, counts):
    """``(tied, by_twins)`` for the float64 cosine matrix of ``rows`` with every row's own record
    masked: the rows whose best cosine is attained by two columns or more, and those among them
    where a column that attains it has a bit-identical row at another column outside the record
    (then the tie is exact whatever the arithmetic).  Two boolean arrays."""
    masked = masked_cosine(cosine, counts)
    best = masked.max(axis=1)
    tied = (masked == best[:, None]).sum(axis=1) >= 2
    groups = row_groups(rows)
    record = np.repeat(np.arange(len(counts)), counts)
    top = masked.argmax(axis=1)
    by_twins = np.array([np.count_nonzero((groups == groups[top[x]]) & (record != record[x])) >= 2
                         for x in range(rows.shape[0])])
    return tied, by_twins


def masked_cosine(cosine: np.ndarray, counts) -> np.ndarray:
    """``cosine`` (square, of the library's rows) with every row's own record at -inf."""
    ptr = pointers(counts)
    masked = cosine.copy()
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        masked[lo:hi, lo:hi] = -np.inf
    return masked


def bound(lq: int, lr: int, scale: float, score64: float) -> float:
    """The score bound of tests/test_gpu_align.py."""
    return min(lq, lr) * abs(scale) * COSINE_TOL + (lq + lr) * 2.0 ** -24 * max(score64, 1.0)


def record_scores_f64(cosine: np.ndarray, counts) -> np.ndarray:
    """The float64 definition of ``distance.record_scores`` (cosine, self-search) from the float64
    cosine matrix of the rows: the mean over a record's rows of the best cosine in every record."""
    ptr = pointers(counts)
    best = np.stack([cosine[:, lo:hi].max(axis=1) for lo, hi in zip(ptr[:-1], ptr[1:])], axis=1)
    return np.stack([best[lo:hi].mean(axis=0) for lo, hi in zip(ptr[:-1], ptr[1:])])


def relation(A: np.ndarray, B: np.ndarray, plant: Planted, parameters):
    """What the float64 definition gives for the rows ``A`` and ``B`` of a planted pair, and by
    how much: ``(score64, holds, margin, bound)``.

    ``holds``: the float64 alignment is the planted diagonal — end, start and ops (all 0).
    ``margin`` is the smaller of two gaps.  The end: how far the best cell lies above every
    other cell that could be named instead (local: all cells; within: the last row; global: the
    end is fixed, no gap).  The path: over the cells of the diagonal, how far the diagonal
    candidate lies above E, F and (local) 0 at that cell, which is what the walk compares.
    ``bound`` is the score bound of tests/test_gpu_align.py for this pair; a float32 value of a
    cell lies within it of the float64 one, so two of them cannot change order across a margin
    of more than twice the bound."""
    import align_global_oracle as GO
    import align_oracle as O
    import align_path_oracle as PO
    scale, shift, go, ge = (float(np.float32(x)) for x in parameters)
    S = O.cosine_f64(A, B) * scale + shift
    lq, lr = S.shape
    if plant.mode == "local":
        H, E, F = PO.gotoh_matrices(S, go, ge, np.float64)
        score, end = O.end_of(H[1:, 1:])
        ops, start = PO.walk(S, H, E, F, go, ge, end)
        others = H[1:, 1:].copy()
    else:
        within = plant.mode == "within"
        H, E, F = GO.matrices(S, go, ge, np.float64, within)
        score, end = GO.end_of(H, within)
        ops, start = GO.walk(S, H, E, F, go, ge, end, within)
        others = H[lq:, 1:].copy() if within else np.full((1, lr), -np.inf)
    holds = end == plant.end and tuple(start) == plant.start and ops.size == plant.length \
        and not ops.any()
    others[-1 if plant.mode != "local" else end[0], end[1]] = -np.inf
    end_margin = float(score) - float(others.max()) if others.size > 1 else np.inf
    step = np.arange(plant.length)
    i, j = plant.start[0] + step + 1, plant.start[1] + step + 1
    rivals = np.maximum(E[i, j], F[i, j])
    if plant.mode == "local":
        rivals = np.maximum(rivals, 0.0)
    path_margin = float((H[i - 1, j - 1] + S[i - 1, j - 1] - rivals).min())
    return float(score), bool(holds), min(end_margin, path_margin), \
        bound(lq, lr, scale, float(score))


def cosine_f64(rows: np.ndarray) -> np.ndarray:
    """``oracle.gine_numpy.pairwise_cosine`` of the library's rows with itself, taken on the
    distinct rows and spread out again: bit-identical rows get bit-identical entries whatever
    order the matrix product adds in, so the ties of the rows are ties of the reference."""
    from oracle import gine_numpy
    groups = row_groups(rows)
    first = np.zeros(groups.max() + 1, dtype=np.int64)
    first[groups[::-1]] = np.arange(rows.shape[0])[::-1]
    distinct = rows[first]
    return gine_numpy.pairwise_cosine(distinct, distinct)[groups][:, groups]


def top1_f64(cosine: np.ndarray, counts) -> np.ndarray:
    """For every row the lowest index that attains its best cosine outside its own record."""
    return masked_cosine(cosine, counts).argmax(axis=1)


def chosen_hits(q, r, wanted=None, most: int = 3) -> list:
    """Which hits go on to the aligners: for every pair of records ``wanted`` (default: the
    planted pairs and FLANKED) up to ``most`` of the hits (x: record q[x] -> record r[x]) that
    join it, the first, the middle one and the last; indices into q and r."""
    if wanted is None:
        wanted = list(dict.fromkeys([plant.pair for plant in planted()] + [(COPY, 0)]
                                    + list(FLANKED)))
    q, r = np.asarray(q), np.asarray(r)
    chosen = []
    for a, b in wanted:
        hits = np.flatnonzero((q == a) & (r == b))
        if hits.size:
            chosen += sorted({int(hits[0]), int(hits[hits.size // 2]), int(hits[-1])})[:most]
    return chosen
