"""The all-pairs distance path on the VALUE range of its inputs: zero rows (the 1e-12 clamp of
``inverse_norm``), fp16 subnormals, rows near the fp16 maximum (|b|² about 5e11 in the folded L2
key), one-hot rows at the ends of the 16-byte pieces, clustered non-negative rows (a and b in ONE
cluster, every cosine >= 0.999: d² is pure cancellation), norms ten orders of magnitude apart in
one call — tests/value_cases.py.  Every other device test of this path draws Gaussian directions
of norm about 1.

The reference is the float64 definition (oracle.gine_numpy) and the tolerances are the project's
own (tests/test_gpu_distance.py), applied PER PAIR:

    cosine   |S - S64| <= 2e-6
    L2       |d² - d64²| <= 4e-6 (|a_i|² + |b_j|²)

Indices are asserted exactly where no kernel within those tolerances could answer otherwise
(``value_cases.certain``; tests/test_value_cases_host.py asserts that this is at least 90 % of
the rows of every placement), values everywhere.  Equal rows have equal keys, so among the
copies of a row the lowest index is asserted as well.

At these sizes (n in {257, 513}, m in {385, 641}) every 128-row tile of b is a sweep chunk of its
own (``test_every_tile_is_a_chunk_of_its_own`` reads it off the workspace size): the merges of
the chunks' results are all in play; sweeps of several tiles per workgroup need n >= 65,536 and
are tests/test_gpu_distance_sweeps.py's.

Which assertion catches what: with the clamp of ``inverse_norm`` removed a zero row has 1 / |row| =
inf and its cosines are 0 * inf = NaN (``test_zero_rows_exactly``, and every case of
``test_dense_matches_float64_per_pair`` with ``zero``); with the unfolded key in ONE of the L2
search kernels — fma(dot, -2, |b|²) against -2 (dot - |b|² / 2) summed from -|b|² / 2 — its keys
round differently from the others' and the byte comparisons of
``test_searches_and_their_identities`` between ``nearest``, ``topk`` and ``record_best`` fail.
That detection does not depend on |b|² = 5e11: the two forms differ in the last bit at norm 1 as
well, on the ``gauss`` control as on ``huge``, whose rows win a search only against each other.
What the ``huge`` cases add is that the identities, the values and the indices hold where the
folded key starts its sums from -2.7e11.

The dense test prints, per pair of families and metric, the worst error over its tolerance
(-s); DESIGN.md §4 holds the table of one run on an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import value_cases as V

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KS = (1, 8, 16)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def _host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _same(one, two):
    """Byte-equal, a NaN standing for any NaN (an a-record of zero rows)."""
    one, two = np.ascontiguousarray(one), np.ascontiguousarray(two)
    holes = np.isnan(one) if one.dtype.kind == "f" else np.zeros(one.shape, dtype=bool)
    return bool(one.shape == two.shape and one.dtype == two.dtype
                and np.array_equal(holes, np.isnan(two) if two.dtype.kind == "f" else holes)
                and one[~holes].tobytes() == two[~holes].tobytes())


def _as_cost(values, metric):
    """Device values in the unit of ``value_cases.ranking``: d², or -S."""
    wide = values.astype(np.float64)
    return wide ** 2 if metric == "l2" else -wide


# ---- 1. dense against float64, per pair -----------------------------------------------------------

@pytest.mark.parametrize("family_b", V.FAMILIES)
@pytest.mark.parametrize("family_a", V.FAMILIES)
def test_dense_matches_float64_per_pair(family_a, family_b):
    from ginfinity_amd import distance
    a, b = V.family(family_a, 257, seed=1), V.family(family_b, 385, seed=2)
    a_dev, b_dev = _device(a), _device(b)
    for metric in V.METRICS:
        got, = _host(distance.pairwise(a_dev, b_dev, metric=metric))
        assert got.shape == (257, 385) and not np.isnan(got).any(), metric
        full, tolerance = V.reference(a, b, metric)
        error = np.abs(_as_cost(got, metric) - V.ranking(full, metric))
        scale = tolerance / (V.COSINE_TOL if metric == "cosine" else V.D2_TOL)
        with np.errstate(invalid="ignore", divide="ignore"):
            relative = np.where(scale > 0, error / scale, 0.0)
        print(f"VALUE-ERROR dense a={family_a} b={family_b} {metric}: worst error / scale "
              f"{relative.max():.3e} (tolerance {V.COSINE_TOL if metric == 'cosine' else V.D2_TOL})")
        assert np.all(error <= tolerance), (metric, float((error - tolerance).max()))


def _row_square_sum(rows):
    """fl32 |row|² the way ``row_square_sum`` (csrc/pairwise_sweep.inc) adds it: per 16-byte piece
    eight fused multiply-adds in order (the squares of float16 values are exact in float32, so
    each is one rounded addition), then a butterfly over the 16 partial sums."""
    wide = rows.astype(np.float64).reshape(rows.shape[0], 16, 8)
    part = np.zeros(wide.shape[:2], dtype=np.float32)
    for j in range(8):
        part = (part.astype(np.float64) + wide[:, :, j] ** 2).astype(np.float32)
    for step in (1, 2, 4, 8):
        part = part + part[:, np.arange(16) ^ step]
    assert np.all(part == part[:, :1])
    return part[:, 0]


@pytest.mark.parametrize("family_b", V.FAMILIES)
def test_zero_rows_exactly(family_b):
    """A zero row: cosine 0 of either sign with anything, L2 of a zero a-row sqrt(fl32 |b_j|²),
    nothing NaN; under cosine it ties every b-row, so the searches name the first candidates in
    row order."""
    from ginfinity_amd import distance
    n, m = 257, 385
    a, zero_a = V.placed("zero", n, seed=31, side="a")
    b, where_b = V.placed(family_b, m, seed=31, side="b", twins=n)
    a_dev, b_dev = _device(a), _device(b)
    zero_b = np.flatnonzero(~b.astype(np.float64).any(axis=1))
    assert (family_b == "zero") == (zero_b.size > 0)

    S, = _host(distance.pairwise(a_dev, b_dev, metric="cosine"))
    D, = _host(distance.pairwise(a_dev, b_dev, metric="l2"))
    assert not np.isnan(S).any() and not np.isnan(D).any()
    assert np.all(S[zero_a] == 0) and np.all(S[:, zero_b] == 0)
    assert D[zero_a].tobytes() == np.tile(np.sqrt(_row_square_sum(b)), (len(zero_a), 1)).tobytes()
    assert np.all(D[:, zero_b] == np.sqrt(_row_square_sum(a))[:, None])

    values, indices = _host(*distance.nearest(a_dev, b_dev, metric="cosine"))
    assert np.all(indices[zero_a] == 0) and np.all(values[zero_a] == 0) and not np.isnan(values).any()
    counts_b = V.records(m, 31)
    firsts = np.concatenate(([0], np.cumsum(counts_b)))[:-1][counts_b > 0]
    for k in KS:
        values, indices = _host(*distance.topk(a_dev, b_dev, k=k, metric="cosine"))
        assert np.all(indices[zero_a] == np.arange(k)) and np.all(values[zero_a] == 0)
        values, indices = _host(*distance.topk(a_dev, b_dev, k=k, metric="cosine",
                                               distinct_records=counts_b))
        assert firsts.size >= k
        assert np.all(indices[zero_a] == firsts[:k]) and np.all(values[zero_a] == 0)
    best, = _host(distance.record_best(a_dev, b_dev, counts_b=counts_b, metric="cosine"))
    assert np.all(best[zero_a][:, counts_b > 0] == 0) and not np.isnan(best).any()

    # against itself, every row skipping its own record: the first row of another record
    rows, counts = V.self_rows("zero", n)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    zero = np.flatnonzero(~rows.astype(np.float64).any(axis=1))
    first_free = np.array([0 if ptr[np.searchsorted(ptr, i, side="right") - 1] > 0
                           else ptr[np.searchsorted(ptr, i, side="right")] for i in zero])
    dev = _device(rows)
    values, indices = _host(*distance.nearest(dev, metric="cosine", exclude_records=counts))
    assert np.array_equal(indices[zero], first_free) and np.all(values[zero] == 0)
    assert not np.isnan(values).any()
    values, indices = _host(*distance.nearest(dev, metric="cosine", exclude_self=True))
    assert np.array_equal(indices[zero], np.where(zero == 0, 1, 0)) and np.all(values[zero] == 0)


# ---- 2. the searches ------------------------------------------------------------------------------

def _chunks(lib, n, m):
    """The sweep chunks of nearest(n, m), from the workspace size (the layout of carve(),
    csrc/pairwise.hip, as tests/test_gpu_distance_sweeps.py reads it)."""
    def align(size):
        return (size + 255) // 256 * 256
    tiles_b = (m + 127) // 128
    partial, odd = divmod(lib.gfy_pairwise_workspace_bytes(n, m)
                          - 2 * align(tiles_b * 128 * 4) - align(n * 4), 2)
    fits = [c for c in range(1, tiles_b + 1) if align(c * n * 4) == partial]
    assert odd == 0 and len(fits) == 1
    return fits[0]


def test_every_tile_is_a_chunk_of_its_own(gpu):
    for n, m in V.SEARCH_SHAPES:
        assert _chunks(gpu, n, m) == (m + 127) // 128 >= 4
        assert all(128 * c in V.positions(m, "b") for c in (1, 2))   # first rows of later chunks


def _check_columns(values, indices, cost, tolerance, metric, record=None):
    """``values`` / ``indices`` ``[n, k]`` of a search against ``cost`` (value_cases.ranking: excluded
    pairs at +inf) and the per-pair ``tolerance``; ``record[j]``: the record of b-row j of a
    search that returns one row per record."""
    n, k = indices.shape
    rows = np.arange(n)[:, None]
    assert values.dtype == np.float32 and indices.dtype == np.int32 and not np.isnan(values).any()
    if record is None:
        order = np.argsort(cost, axis=1, kind="stable")[:, :k]
        want = cost[rows, order]
    else:                                  # every record's best row, the records by that row
        count = int(record.max()) + 1
        best = np.full((n, count), np.inf)
        best_at = np.zeros((n, count), dtype=np.int64)
        for r in range(count):
            columns = np.flatnonzero(record == r)
            if columns.size == 0:
                continue
            at = np.argmin(cost[:, columns], axis=1)
            best[:, r], best_at[:, r] = cost[rows[:, 0], columns[at]], columns[at]
        chosen = np.argsort(best, axis=1, kind="stable")[:, :k]
        order, want = best_at[rows, chosen], best[rows, chosen]
    if order.shape[1] < k:                 # fewer candidates than k
        short = ((0, 0), (0, k - order.shape[1]))
        order, want = np.pad(order, short), np.pad(want, short, constant_values=np.inf)
    has = np.isfinite(want)
    order = np.where(has, order, -1)
    empty = np.float32(np.inf if metric == "l2" else -np.inf)
    assert np.all(indices[~has] == -1) and np.all(values[~has] == empty)
    assert np.all(indices[has] >= 0) and indices.max() < cost.shape[1]
    at = np.where(has, indices, 0)
    picked = cost[rows, at]
    assert np.all(np.isfinite(picked[has]))                    # never an excluded pair
    for name, keys in (("index", indices), ("record", None if record is None else record[at])):
        if keys is not None:                                   # nothing twice
            lined = np.sort(np.where(has, keys, -1 - np.arange(k)[None, :]), axis=1)
            assert np.all(np.diff(lined, axis=1) != 0), name
    allowed = tolerance[rows, at]
    with np.errstate(invalid="ignore"):                        # inf - inf in the empty columns
        behind = np.abs(picked - want)
        error = np.abs(_as_cost(values, metric) - picked)
    assert np.all(behind[has] <= allowed[has])                 # as good as the float64 choice
    assert np.all(error[has] <= allowed[has])                  # and its value is that pair's
    sure = V.certain(cost, tolerance, order)
    assert np.array_equal(indices[sure], order[sure])


def _searches(a, b, metric, counts_a, counts_b, gone=None, exclude=None):
    """Every search of one placement: checked against float64, and the project's identities
    byte for byte.  ``exclude``: the record counts of a self-search (``b`` is ``a``)."""
    from ginfinity_amd import distance
    n, m = a.shape[0], b.shape[0]
    full, tolerance = V.reference(a, b, metric)
    cost = V.ranking(full, metric, gone)
    _, group = V.unique_rows(b)
    a_dev = _device(a)
    b_dev = None if exclude is not None else _device(b)
    more = {} if exclude is None else {"exclude_records": exclude}
    record = np.repeat(np.arange(len(counts_b)), counts_b)

    near_values, near_indices = _host(*distance.nearest(a_dev, b_dev, metric=metric, **more))
    _check_columns(near_values[:, None], near_indices[:, None], cost, tolerance, metric)
    expected, sure = V.nearest_expected(cost, tolerance, group)
    assert np.array_equal(near_indices[sure], expected[sure])  # the lowest copy of the best row
    assert sure.mean() >= V.MARGIN_CAP
    for k in KS:
        values, indices = _host(*distance.topk(a_dev, b_dev, k=k, metric=metric, **more))
        _check_columns(values, indices, cost, tolerance, metric)
        assert values[:, 0].tobytes() == near_values.tobytes(), (metric, k)
        assert indices[:, 0].tobytes() == near_indices.tobytes(), (metric, k)
        values, indices = _host(*distance.topk(a_dev, b_dev, k=k, metric=metric,
                                               distinct_records=counts_b, **more))
        _check_columns(values, indices, cost, tolerance, metric, record)
    if exclude is not None:
        return
    # record_best[:, r] is nearest on record r; record_scores the float64 mean of record_best
    best, = _host(distance.record_best(a_dev, b_dev, counts_b=counts_b, metric=metric))
    ptr_b = np.concatenate(([0], np.cumsum(counts_b)))
    keeper = distance.NearestWorkspace()
    for r, count in enumerate(counts_b):
        if count == 0:
            assert np.all(best[:, r] == np.float32(np.inf if metric == "l2" else -np.inf))
            continue
        values, _ = distance.nearest(a_dev, b_dev[int(ptr_b[r]):int(ptr_b[r + 1])], metric=metric,
                                     workspace=keeper)
        assert values.cpu().numpy().tobytes() == np.ascontiguousarray(best[:, r]).tobytes(), r
    scores, = _host(distance.record_scores(a_dev, b_dev, counts_a=counts_a, counts_b=counts_b,
                                           metric=metric))
    ptr_a = np.concatenate(([0], np.cumsum(counts_a)))
    mean = np.full(scores.shape, np.nan, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for q in range(len(counts_a)):
            part = best[ptr_a[q]:ptr_a[q + 1]].astype(np.float64)
            if part.shape[0]:                      # cumsum adds in sequence, as the definition does
                mean[q] = (np.cumsum(part, axis=0)[-1] / part.shape[0]).astype(np.float32)
    # a zero a-row alone in its record: the mean of one -0 is a zero of either sign
    assert _same(scores + np.float32(0), mean + np.float32(0))


SEARCHES = sorted({(name, role) for name, role, _, _ in V.search_cases()})


@pytest.mark.parametrize("metric", V.METRICS)
@pytest.mark.parametrize("name,role", SEARCHES)
def test_searches_and_their_identities(name, role, metric):
    for n, m in V.SEARCH_SHAPES:
        a, b = V.search_rows(name, role, n, m)
        _searches(a, b, metric, V.records(n, 41), V.records(m, 42))


@pytest.mark.parametrize("metric", V.METRICS)
@pytest.mark.parametrize("name", V.FAMILIES)
def test_self_search_that_skips_each_row_s_own_record(name, metric):
    for n, _ in V.SEARCH_SHAPES:
        rows, counts = V.self_rows(name, n)
        _searches(rows, rows, metric, counts, counts, gone=V.excluded_mask(n, n, counts),
                  exclude=counts)


# ---- 3. power-of-two invariance -------------------------------------------------------------------

def _scalable(name):
    """A placement of SEARCH_SHAPES[0] whose elements all stay normal under 2^-6 and 2^5: the
    family rows that cannot (one-hot 65504 and 2^-24) are left out, elements below 2^-8 are set
    to zero."""
    n, m = V.SEARCH_SHAPES[0]
    a, b = V.search_rows("gauss", "both", n, m)
    pool = V.family(name, 60, seed=5)
    size = np.abs(pool.astype(np.float64)).max(axis=1)
    pool = pool[(size <= 2.0) & (size >= 2.0 ** -8)]
    assert pool.shape[0] >= 12
    where_a, where_b = V.positions(n, "a"), V.positions(m, "b")
    a[where_a] = pool[:len(where_a)]
    b[where_b] = pool[6:6 + len(where_b)]
    return V.in_normal_range(a), V.in_normal_range(b)


def _outputs(a, b, metric, counts_a, counts_b):
    from ginfinity_amd import distance
    a_dev, b_dev = _device(a), _device(b)
    out = list(_host(distance.pairwise(a_dev, b_dev, metric=metric)))
    out += _host(*distance.nearest(a_dev, b_dev, metric=metric))
    out += _host(*distance.topk(a_dev, b_dev, k=8, metric=metric))
    out += _host(distance.record_scores(a_dev, b_dev, counts_a=counts_a, counts_b=counts_b,
                                        metric=metric))
    return out


@pytest.mark.parametrize("name", ("gauss", "clustered", "onehot"))
def test_power_of_two_scaling_changes_no_bit(name):
    """Derived, not measured: a power of two scales every product, every partial sum, |row|², its
    square root and its reciprocal exactly (nothing leaves the normal range of float32), so the
    cosine outputs do not change and the L2 outputs scale, byte for byte.  A hidden absolute
    constant or a flush breaks it."""
    a, b = _scalable(name)
    counts_a, counts_b = V.records(a.shape[0], 41), V.records(b.shape[0], 42)
    cosine = _outputs(a, b, "cosine", counts_a, counts_b)
    l2 = _outputs(a, b, "l2", counts_a, counts_b)
    for p in (-6, 5):
        for q in (-6, 5):
            got = _outputs(V.scaled(a, p), V.scaled(b, q), "cosine", counts_a, counts_b)
            for one, two in zip(got, cosine):
                assert _same(one, two), (p, q)
        got = _outputs(V.scaled(a, p), V.scaled(b, p), "l2", counts_a, counts_b)
        for one, two in zip(got, l2):
            want = two * np.float32(2.0 ** p) if two.dtype == np.float32 else two
            assert _same(one, want), p
