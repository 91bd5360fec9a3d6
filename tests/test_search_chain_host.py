"""The library of tests/search_cases.py on the ``device="cpu"`` path: that the case bites, from
references alone.  No GPU: ``Ginfinity.load("cpu")`` with the float16 model, float64 numpy
(oracle.gine_numpy.pairwise_cosine, the float64 Gotoh programs of the align oracles) and the two
pure functions ``align.top_pairs`` and ``align.band_around``.  tests/test_gpu_search_chain.py
runs the same library through the device and re-asserts the conditions on the device's rows.

Measured on this path (3,537 rows in 27 records; every test prints its figures with -s):

    row norms                          0.99990 to 1.00011
    twin rows                          600 rows are bit-identical to a row of another record, in
                                       264 groups of up to 5 copies (record 0 and COPY give 102
                                       pairs, the adapters of records 4, 5, 9, 14 and 23 and
                                       WINDOW inside record 8 the rest)
    tied tops                          368 rows attain their best cosine outside their own record
                                       at two rows or more, each of them through twin rows
    smallest margin / bound            26.8 ((1, JOIN) under shift -0.25: its last cell adds
                                       0.268 - 0.25); every other pair is above 170
    steeper shifts                     -0.3 fails (1, JOIN), -0.5 (1, JOIN) and (7, JOIN):
                                       search_cases.STEEPER_SHIFTS says why
    broken recipe, ptr[q + 1]          every seed is negative and ``band_around`` refuses them; a
                                       band of half-width 8 made by hand loses score on 3 of the
                                       5 planted pairs of records: the diagonal moves by Lq - Lr,
                                       which is 0 for (0, COPY) and (COPY, 0)
    broken recipe, q and r swapped     loses score on 5 of 5

The sample table holds no molecule twice, so (4, 5), (4, 9) and (5, 9) are not copies of each
other: search_cases says what they share."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import align_band_oracle as BO
import align_oracle as O
import search_cases as SC
from ginfinity_amd import align

FACTOR = 4.0          # the GPU's rows may differ in last places: it re-asserts 2 on its own rows
HALF_WIDTH = 8


@functools.lru_cache(maxsize=None)
def _case():
    from ginfinity_amd import Ginfinity
    rows, counts = SC.encode_library(Ginfinity.load("cpu"))
    rows.setflags(write=False)
    cosine = SC.cosine_f64(rows)
    cosine.setflags(write=False)
    return dict(rows=rows, counts=counts, cosine=cosine, ptr=SC.pointers(counts))


def _record(case, record):
    return SC.record_rows(case["rows"], case["counts"], record)


def test_the_library_is_what_search_cases_says():
    records, counts = SC.library(), _case()["counts"]
    assert counts == SC.lengths() and sum(counts) == _case()["rows"].shape[0]
    assert counts[1] == 91 and counts[7] == 75 and counts[SC.JOIN] == 166
    assert counts[SC.WINDOWED] == 289 and counts[SC.WINDOW] == SC.WINDOW_END - SC.WINDOW_START
    assert [counts[x] for x in (4, 5, 9)] == [177] * 3
    # no molecule is in the table twice, the three of 177 nt included
    assert SC.duplicate_groups(SC.sample_records()) == []
    for a, b in SC.FLANKED:
        assert records[a].sequence != records[b].sequence
        assert records[a].sequence[:26] == records[b].sequence[:26]
        assert records[a].structure[-21:] == records[b].structure[-21:]


def test_ties_at_the_top():
    case = _case()
    rows, counts = case["rows"], case["counts"]
    norms = np.linalg.norm(rows.astype(np.float64), axis=1)
    twins, groups, largest = SC.twin_rows(rows, counts)
    tied, by_twins = SC.tied_tops(case["cosine"], rows, counts)
    print(f"norms {norms.min():.5f} to {norms.max():.5f}; {twins} twin rows in {groups} groups of "
          f"up to {largest}; {tied.sum()} tied tops, {(tied & by_twins).sum()} through twin rows")
    assert twins >= 100
    assert _record(case, 0).tobytes() == _record(case, SC.COPY).tobytes()
    assert (tied & by_twins).sum() >= 100
    # the shared adapters: any two of the three records of 177 nt have rows that are the same bits
    groups, ptr = SC.row_groups(rows), case["ptr"]
    for a, b in SC.FLANKED:
        shared = np.intersect1d(groups[ptr[a]:ptr[a + 1]], groups[ptr[b]:ptr[b + 1]]).size
        print(f"records {a} and {b} share {shared} distinct rows")
        assert shared >= 1, (a, b)


@pytest.mark.parametrize("parameters", SC.PARAMETERS)
def test_every_planted_relation_holds_with_a_margin(parameters):
    case = _case()
    smallest = np.inf
    for plant in SC.planted():
        score, holds, margin, bound = SC.relation(_record(case, plant.pair[0]),
                                                  _record(case, plant.pair[1]), plant, parameters)
        print(f"{plant} score64 {score:.4f} margin {margin:.4f} bound {bound:.2e} "
              f"ratio {margin / bound:.1f}")
        assert holds, (plant, parameters)
        assert margin > FACTOR * bound, (plant, parameters, margin, bound)
        smallest = min(smallest, margin / bound)
    print(f"smallest margin / bound {smallest:.1f}")


def test_steeper_shifts_do_not_find_the_join_diagonals_whole():
    """Why PARAMETERS have milder shifts than the sets of tests/test_gpu_align.py: by the float64
    definition a shift of -0.3 or -0.5 cuts a JOIN diagonal short or leaves it less than FACTOR
    bounds of margin, and nothing else fails under them."""
    case = _case()
    for parameters in SC.STEEPER_SHIFTS:
        failed = []
        for plant in SC.planted():
            _, holds, margin, bound = SC.relation(_record(case, plant.pair[0]),
                                                  _record(case, plant.pair[1]), plant, parameters)
            if not (holds and margin > FACTOR * bound):
                failed.append(plant.pair)
        print(parameters, "fails", failed)
        assert failed and all(pair[1] == SC.JOIN for pair in failed), (parameters, failed)


def _banded_score(case, pair, parameters, diagonal):
    scale, shift, go, ge = (float(np.float32(x)) for x in parameters)
    S = O.cosine_f64(_record(case, pair[0]), _record(case, pair[1])) * scale + shift
    H = BO.band_matrices(S, go, ge, int(diagonal) - HALF_WIDTH, int(diagonal) + HALF_WIDTH,
                         np.float64)[0]
    return float(O.end_of(H[1:, 1:])[0]), SC.bound(*S.shape, scale, float(H.max()))


def test_the_recipe_gives_the_cells_and_a_broken_one_loses_score():
    case = _case()
    counts, ptr = np.asarray(case["counts"]), case["ptr"]
    rows = np.arange(case["rows"].shape[0])
    top = SC.top1_f64(case["cosine"], case["counts"])
    q, r, seeds = SC.seeds_from_hits(rows, top, counts, counts)
    q, r = q.numpy().astype(np.int64), r.numpy().astype(np.int64)
    # independently: the record by a scan of the boundaries, the cell by the record's first row
    owner = np.array([max(k for k in range(len(counts)) if ptr[k] <= x) for x in rows])
    assert (q == owner).all() and (r == owner[top]).all() and (q != r).all()
    assert (seeds == np.stack([rows - ptr[q], top - ptr[r]], axis=1)).all()
    assert (seeds >= 0).all() and (seeds[:, 0] < counts[q]).all() and (seeds[:, 1] < counts[r]).all()
    # the recipe's precondition: the counts as arrays; the tuple that ``encode_graphs_device``
    # returns cannot be indexed by the records
    with pytest.raises(TypeError):
        SC.seeds_from_hits(rows, top, case["counts"], case["counts"])
    chosen = SC.chosen_hits(q, r, [plant.pair for plant in SC.planted()] + [(SC.COPY, 0)])
    pairs = sorted({(int(q[x]), int(r[x])) for x in chosen})
    assert len(pairs) == 5       # every planted pair of records is found by some row's top hit
    # broken once: the end of the record for its first row; broken twice: q and r swapped
    late = np.stack([rows - ptr[q + 1], top - ptr[r + 1]], axis=1)
    swapped = np.stack([rows - ptr[r], top - ptr[q]], axis=1)
    assert (late < 0).all()
    with pytest.raises(ValueError, match="seeds must be cells inside records"):
        align.band_around(late, HALF_WIDTH)
    parameters = SC.PARAMETERS[0]
    lost = {"late": set(), "swapped": set()}
    for x in chosen:
        pair = (int(q[x]), int(r[x]))
        right = align.band_around(seeds[x:x + 1], HALF_WIDTH)[0]
        diagonal = int(seeds[x, 1] - seeds[x, 0])
        assert tuple(right) == (diagonal - HALF_WIDTH, diagonal + HALF_WIDTH)
        good, bound = _banded_score(case, pair, parameters, diagonal)
        for name, broken in (("late", late), ("swapped", swapped)):
            bad, _ = _banded_score(case, pair, parameters, broken[x, 1] - broken[x, 0])
            if good - bad > FACTOR * bound:
                lost[name].add(pair)
    print({name: sorted(found) for name, found in lost.items()}, "of", pairs)
    assert lost["late"] and lost["swapped"]
    # records of equal length hide the first break: the diagonal moves by Lq - Lr
    assert (0, SC.COPY) not in lost["late"] and (0, SC.COPY) in lost["swapped"]


def test_top_pairs_on_the_float64_record_scores():
    case = _case()
    scores = SC.record_scores_f64(case["cosine"], case["counts"])
    assert scores[0, 0] == scores[0, SC.COPY] == scores[SC.COPY, 0] == scores[SC.COPY, SC.COPY]
    assert (scores.max(axis=1) == np.diag(scores)).all()
    pairs = align.top_pairs(scores, 3, largest=True)
    assert pairs.shape == (3 * SC.RECORDS, 2) and pairs.dtype == np.int32
    assert (pairs[:, 0] == np.repeat(np.arange(SC.RECORDS), 3)).all()
    best = pairs.reshape(SC.RECORDS, 3, 2)[:, :, 1]
    # ties go to the lowest r: record 0 before COPY in both rows
    assert best[0, :2].tolist() == [0, SC.COPY] and best[SC.COPY, :2].tolist() == [0, SC.COPY]
    listed = {tuple(pair) for pair in pairs.tolist()}
    assert set(SC.whole_record_pairs()) <= listed and (SC.WINDOW, SC.WINDOWED) in listed
    for q in (1, 7, SC.WINDOW):                        # itself, then the record that holds it
        assert best[q, 0] == q and best[q, 1] == {1: SC.JOIN, 7: SC.JOIN, SC.WINDOW: SC.WINDOWED}[q]
