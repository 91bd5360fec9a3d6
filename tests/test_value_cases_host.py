"""The value families of tests/value_cases.py are what they say they are, ``scaled`` is exact,
the float64 definition is finite on every pair of families, and the cap the device tests rely on
holds: on every search placement at least 90 % of the a-rows have a nearest row that no kernel
within the value tolerance can miss (``value_cases.certain``), so that an exact-index assertion
there is an assertion on most rows.  No device."""
from __future__ import annotations

import numpy as np
import pytest

import value_cases as V


def _wide(rows):
    return rows.astype(np.float64)


@pytest.mark.parametrize("name", V.FAMILIES)
def test_family_is_what_it_says(name):
    rows = V.family(name, 45, seed=3)
    wide = _wide(rows)
    assert rows.dtype == np.float16 and rows.shape == (45, 128) and np.all(np.isfinite(wide))
    assert np.array_equal(rows, V.family(name, 45, seed=3))            # a function of the seed
    size = np.abs(wide)
    if name == "zero":
        assert np.all(wide == 0)
        assert not np.signbit(rows[0]).any() and np.signbit(rows[1]).all()
    elif name == "subnormal":
        assert np.all(size < V.F16_TINY) and np.all(size * 2.0 ** 24 == np.round(size * 2.0 ** 24))
        assert np.all(size[[0] + list(range(2, 45))] > 0)              # subnormal throughout
        assert np.count_nonzero(wide[1]) == 1 and wide[1].max() == 2.0 ** -24
        assert (wide < 0).any() and (wide > 0).any()
    elif name == "tiny":
        assert size.min() >= V.F16_TINY and size.max() <= 2.0 ** -10
    elif name == "huge":
        assert size.min() >= 16384 and size.max() == V.F16_MAX and np.all(wide[1] == V.F16_MAX)
        assert (wide[0] < 0).any() and (wide[0] > 0).any()
    elif name == "onehot":
        assert np.all(np.count_nonzero(wide, axis=1) == 1)
        seen = {(int(np.flatnonzero(row)[0]), float(row[np.flatnonzero(row)[0]])) for row in wide}
        assert seen == {(c, v) for c in V.ONEHOT_COLUMNS for v in V.ONEHOT_VALUES}
    elif name == "clustered":
        assert wide.min() >= 0
        unit = wide / np.linalg.norm(wide, axis=1, keepdims=True)
        assert (unit @ unit.T).min() >= 0.999
        assert np.array_equal(rows[2], rows[0]) and np.array_equal(rows[5], rows[3])
    elif name == "mixed":
        norms = np.linalg.norm(wide, axis=1)
        assert norms.min() < 2.0 ** -17 and norms.max() > 2.0 ** 7       # ten orders of magnitude
        assert norms.max() / norms.min() > 1e7 and np.all(norms > 0)
    else:
        norms = np.linalg.norm(wide, axis=1)
        assert norms.min() > 0.79 and norms.max() < 1.26


def _cosines(a, b):
    a, b = _wide(a), _wide(b)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T


def test_both_sides_of_a_clustered_call_lie_in_one_cluster():
    """The case is d² as pure cancellation BETWEEN a and b: the dense call, the family rows of a
    search placement and the whole-family records of the aligners, as the device tests draw them."""
    assert _cosines(V.family("clustered", 257, seed=1), V.family("clustered", 385, seed=2)).min() >= 0.999
    for n, m in V.SEARCH_SHAPES:
        a, b = V.search_rows("clustered", "both", n, m)
        assert _cosines(a[V.positions(n, "a")], b[V.positions(m, "b")]).min() >= 0.999
        rows, _ = V.self_rows("clustered", n)
        assert _cosines(rows[V.positions(n, "self")], rows[V.positions(n, "self")]).min() >= 0.999
    a, counts_a, b, counts_b, pairs = V.align_records("clustered")
    assert (3, 1) in {tuple(pair) for pair in pairs.tolist()}
    whole_a = a[sum(counts_a[:3]):sum(counts_a[:4])]
    whole_b = b[counts_b[0]:counts_b[0] + counts_b[1]]
    assert _cosines(whole_a, whole_b).min() >= 0.999
    spots = a[[0, counts_a[0] + 96, 2 * 97 + 63, 2 * 97 + 64]]      # the rows inside the records
    assert _cosines(spots, np.concatenate([whole_b, b[[0, 31, 32, 129]]])).min() >= 0.999


@pytest.mark.parametrize("side,count", [("a", 257), ("b", 385), ("self", 513)])
def test_the_few_rows_of_a_placement_span_their_family(side, count):
    rows, where = V.placed("mixed", count, seed=11, side=side, twins=257)
    norms = np.linalg.norm(_wide(rows[where]), axis=1)
    assert norms.min() < 2.0 ** -17 and norms.max() > 2.0 ** 7 and norms.max() / norms.min() > 1e7
    assert np.sum((norms > 2.0 ** -10) & (norms < 2.0 ** 4)) >= 1       # and something in between
    rows, where = V.placed("onehot", count, seed=11, side=side, twins=257)
    wide = _wide(rows[where])
    assert np.all(np.count_nonzero(wide, axis=1) == 1)
    assert {int(np.flatnonzero(row)[0]) for row in wide} == set(V.ONEHOT_COLUMNS)
    assert {float(row[np.flatnonzero(row)[0]]) for row in wide} == set(V.ONEHOT_VALUES)


@pytest.mark.parametrize("side,count", [("a", 257), ("a", 513), ("b", 385), ("b", 641), ("self", 257)])
def test_placed_puts_the_family_at_the_seams(side, count):
    rows, where = V.placed("huge", count, seed=5, side=side, twins=257 if side == "b" else None)
    assert rows.shape == (count, 128) and {0, 127, 128, 256, count - 1} <= set(where)
    assert (255 in where) == (side != "b")
    big = np.abs(_wide(rows)).max(axis=1) >= 16384
    assert np.array_equal(np.flatnonzero(big), where)
    if side == "b":                                    # the last row is alone in a ragged tile
        assert count % 128 == 1


def test_scaled_is_exact_and_refuses_what_is_not():
    rows = V.in_normal_range(V.family("gauss", 30, seed=1))
    for p in (-6, 5):
        out = V.scaled(rows, p)
        assert np.array_equal(_wide(out), _wide(rows) * 2.0 ** p)
    assert np.array_equal(V.scaled(V.scaled(rows, 5), -5), rows)
    with pytest.raises(AssertionError):
        V.scaled(V.family("huge", 4), 1)               # overflow
    with pytest.raises(AssertionError):
        V.scaled(V.family("tiny", 4), -1)              # a new subnormal
    with pytest.raises(AssertionError):
        V.scaled(V.family("subnormal", 4), -1)         # bits lost
    for name in ("gauss", "clustered"):
        kept = V.in_normal_range(V.family(name, 60, seed=2))
        assert np.count_nonzero(kept) >= 0.9 * kept.size       # still the family
    ones = V.family("onehot", 20)[[0, 3, 4, 7]]
    assert np.array_equal(V.in_normal_range(ones), ones)


@pytest.mark.parametrize("metric", V.METRICS)
def test_the_float64_definition_is_finite_on_every_pair_of_families(metric):
    for one in V.FAMILIES:
        for two in V.FAMILIES:
            full, tolerance = V.reference(V.family(one, 9, 1), V.family(two, 7, 2), metric)
            assert full.shape == (9, 7) and np.all(np.isfinite(full)), (one, two)
            assert np.all(np.isfinite(tolerance)) and np.all(tolerance >= 0)
            if metric == "cosine":
                assert np.abs(full).max() <= 1 + 1e-12
                if "zero" in (one, two):
                    assert np.all(full == 0)           # zero against zero included
            elif one == "zero":                        # d² = |b_j|²
                assert np.allclose(full, (_wide(V.family(two, 7, 2)) ** 2).sum(1)[None, :],
                                   rtol=1e-15, atol=0)


def test_equal_rows_get_equal_columns():
    b = np.concatenate([V.family("clustered", 9), V.family("zero", 4)])
    first, group = V.unique_rows(b)
    assert group.tolist() == [0, 1, 0, 3, 4, 3, 6, 7, 6, 9, 9, 9, 9] and first.tolist() == [0, 1, 3, 4, 6, 7, 9]
    full, _ = V.reference(V.family("gauss", 5), b, "l2")
    assert np.array_equal(full[:, 2], full[:, 0]) and np.array_equal(full[:, 12], full[:, 9])


def test_certain_and_nearest_expected_on_a_matrix_worked_by_hand():
    cost = np.array([[1.0, 1.0, 3.0, 1.0 + 1e-9], [2.0, 2.0, 2.0, np.inf]])
    tolerance = np.full(cost.shape, 1e-6)
    group = np.array([0, 0, 2, 3])                     # rows 0 and 1 of b are copies
    index, sure = V.nearest_expected(cost, tolerance, group)
    assert index.tolist() == [0, 0] and sure.tolist() == [False, False]   # 1 + 1e-9; a tie of strangers
    cost[0, 3], cost[1, 2] = 1.1, 2.5
    index, sure = V.nearest_expected(cost, tolerance, group)
    assert index.tolist() == [0, 0] and sure.tolist() == [True, True]
    cost[0, 0] = np.inf                                # the first copy excluded: the second one
    index, sure = V.nearest_expected(cost, tolerance, group)
    assert index.tolist() == [1, 0] and sure.tolist() == [True, True]
    cost[1] = np.inf                                   # nothing left
    index, sure = V.nearest_expected(cost, tolerance, group)
    assert index.tolist() == [1, -1] and sure.tolist() == [True, False]
    cost[1] = [5.0, 5.0, 2.0, np.inf]
    columns = np.array([[2, 3], [0, -1]])
    assert V.certain(cost, tolerance, columns).tolist() == [[True, True], [False, False]]


@pytest.mark.parametrize("metric", V.METRICS)
def test_the_margin_cap_holds_on_every_search_placement(metric):
    """What the exact-index assertions of tests/test_gpu_distance_values.py stand on: per
    placement, the share of a-rows whose float64 nearest row is certain.  ``zero``, ``clustered``
    and the copies need no exemption: a placement holds at most six family rows."""
    worst = 1.0
    for name, role, n, m in V.search_cases():
        a, b = V.search_rows(name, role, n, m)
        full, tolerance = V.reference(a, b, metric)
        _, group = V.unique_rows(b)
        _, sure = V.nearest_expected(V.ranking(full, metric), tolerance, group)
        share = sure.mean()
        worst = min(worst, share)
        assert share >= V.MARGIN_CAP, (name, role, n, m, share)
    for name in V.FAMILIES:
        for n, _ in V.SEARCH_SHAPES:
            rows, counts = V.self_rows(name, n)
            assert counts.sum() == n and (counts == 0).sum() == 1
            full, tolerance = V.reference(rows, rows, metric)
            _, group = V.unique_rows(rows)
            cost = V.ranking(full, metric, V.excluded_mask(n, n, counts))
            _, sure = V.nearest_expected(cost, tolerance, group)
            worst = min(worst, sure.mean())
            assert sure.mean() >= V.MARGIN_CAP, (name, n, sure.mean())
    print(f"{metric}: smallest share of certain rows {worst:.3f}")


@pytest.mark.parametrize("name", V.FAMILIES)
def test_align_records_hold_the_family_where_they_say(name):
    a, counts_a, b, counts_b, pairs = V.align_records(name)
    assert a.shape[0] == sum(counts_a) and b.shape[0] == sum(counts_b)
    assert max(counts_a + counts_b) <= 200 and len(pairs) <= 12
    assert {int(q) for q, _ in pairs} == set(range(5)) and {int(r) for _, r in pairs} == set(range(3))
    assert np.all(np.isfinite(_wide(a))) and np.all(np.isfinite(_wide(b)))
    if name == "zero":
        ptr = np.concatenate(([0], np.cumsum(counts_a)))
        zero = np.flatnonzero(~_wide(a).any(axis=1))
        want = [0, ptr[1] + 96, ptr[2] + 63, ptr[2] + 64] + list(range(ptr[3], ptr[4]))
        assert zero.tolist() == want
        zero = np.flatnonzero(~_wide(b).any(axis=1))
        assert zero.tolist() == [0, 31, 32, 129] + list(range(130, 167))
