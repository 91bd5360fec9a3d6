"""Record-to-record best-match scores (gfy_pairwise_record_best, gfy_pairwise_record_scores;
distance.record_best, distance.record_scores; csrc/pairwise_records.hip).

Inputs, record sizes and tolerances are those of tests/test_gpu_distance_ranges.py.  The row
level is compared bit for bit with ``nearest`` on every record's rows, the record level with the
float64 definition of oracle.gine_numpy taken per record and, bit for bit, with the stated mean
of the returned row level; independence of the rest of the call, of the blocking and of the run
are byte comparisons.

Tolerances.  A score is a mean of values that are each within the tolerance of the row level
(cosine 2e-6; L2 2e-5 on d >= 0.1, asserted on the reference), so it is within the same
tolerance, plus one rounding of the result to float32 (2^-24 relative).  The float64 sum adds
nothing that shows at these sizes.  On the diagonal of an L2 self-search d = 0 lies below 0.1:
there the bound of test_gpu_distance_ranges.py on d² applies, 4e-6 (|a|² + |b|²), i.e.
d <= sqrt(4e-6 * 2 |x|²) per row and so for their mean."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_ranges.py
L2_TOL = 2e-5            # on an L2 distance d >= 0.1
D2_TOL = 4e-6            # on d², times (|a_i|² + |b_j|²)
ROUNDING = 2.0 ** -24    # one rounding to float32, relative
TILE = 128               # a-rows per workgroup, b-rows per tile (pairwise_records.hip)
RECORD_SIZES = (1, 2, 37, 100, 128, 129, 300)
LEAD = (128, 0, 0, 600)  # ends on a tile end; two of zero rows; longer than the ring of four
METRICS = ("l2", "cosine")
ROWS_A = (257, 385)
ROWS_B = (385, 1_000, 8_269)
SELF_SEARCH = 8_269


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


@functools.lru_cache(maxsize=None)
def _pool():
    from ginfinity_amd import synthetic
    data = synthetic.unit_rows(101, 20_480)
    data.setflags(write=False)
    return data


def _a_rows(n):
    return _pool()[:n]


def _b_rows(m):
    """Disjoint from every _a_rows(n), n <= 8,269."""
    return _pool()[10_240:10_240 + m]


@functools.lru_cache(maxsize=None)
def _device_pool():
    return torch.from_numpy(np.array(_pool())).cuda()


def _device(rows):
    return torch.from_numpy(np.array(rows)).cuda()           # a copy: shared inputs are read-only


def _records(rows, lead=()):
    """Record sizes: ``lead``, then RECORD_SIZES over and over until ``rows`` rows are used up
    (whichever record gets there is cut short: the last record ends at ``rows``).  Returns
    (counts, ptr)."""
    counts, at = [], 0
    for size in lead:
        counts.append(min(size, rows - sum(counts)))
    while sum(counts) < rows:
        counts.append(min(RECORD_SIZES[at % len(RECORD_SIZES)], rows - sum(counts)))
        at += 1
    ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    assert ptr[-1] == rows
    return counts, ptr


def _best(a, b, counts_b, metric):
    from ginfinity_amd import distance
    return distance.record_best(a, b, counts_b=counts_b, metric=metric).cpu().numpy()


def _scores(a, b=None, **arguments):
    from ginfinity_amd import distance
    return distance.record_scores(a, b, **arguments).cpu().numpy()


def _empty(metric):
    return np.float32(np.inf if metric == "l2" else -np.inf)


def _same(one, two):
    """Byte-equal, a NaN standing for any NaN."""
    one, two = np.ascontiguousarray(one), np.ascontiguousarray(two)
    if one.shape != two.shape or one.dtype != two.dtype:
        return False
    holes = np.isnan(one)
    return bool(np.array_equal(holes, np.isnan(two))
                and one[~holes].tobytes() == two[~holes].tobytes())


def _assert_columns_are_nearest(a, b, counts, ptr, metric, best):
    """best[:, r] is nearest(a, the rows of record r) byte for byte; a record of zero rows has
    no nearest row and holds +inf / -inf."""
    from ginfinity_amd import distance
    keeper = distance.NearestWorkspace()
    assert best.shape == (a.shape[0], len(counts)) and best.dtype == np.float32
    for r, count in enumerate(counts):
        if count == 0:
            assert np.all(best[:, r] == _empty(metric)), r
            continue
        values, _ = distance.nearest(a, b[int(ptr[r]):int(ptr[r + 1])], metric=metric,
                                     workspace=keeper)
        assert values.cpu().numpy().tobytes() == np.ascontiguousarray(best[:, r]).tobytes(), \
            (metric, r, count, int(ptr[r]))


def _reference(n, m, metric):
    """The float64 definition: the matrix [n, m] of oracle.gine_numpy."""
    from oracle import gine_numpy
    full = (gine_numpy.pairwise_l2 if metric == "l2" else gine_numpy.pairwise_cosine)(
        _a_rows(n), _b_rows(m))
    return full


def _reference_best(full, ptr_b, metric):
    pick = np.min if metric == "l2" else np.max
    best = np.full((full.shape[0], len(ptr_b) - 1), float(_empty(metric)))
    for r in range(len(ptr_b) - 1):
        if ptr_b[r + 1] > ptr_b[r]:
            best[:, r] = pick(full[:, ptr_b[r]:ptr_b[r + 1]], axis=1)
    return best


def _mean_of_rows(best, ptr_a):
    """The stated mean: float64 sum in ascending row order (cumsum adds in sequence; np.sum would
    add pairwise), divided by the rows, rounded to float32 once."""
    out = np.full((len(ptr_a) - 1, best.shape[1]), np.nan, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for q in range(len(ptr_a) - 1):
            rows = best[ptr_a[q]:ptr_a[q + 1]].astype(np.float64)
            if rows.shape[0]:
                out[q] = (np.cumsum(rows, axis=0)[-1] / rows.shape[0]).astype(np.float32)
    return out


# ---- 1. the row level against nearest, bit for bit ----------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", ROWS_B)
@pytest.mark.parametrize("n", ROWS_A)
def test_every_column_is_nearest_on_that_record(n, m, metric):
    """Lead records: 128 rows that end exactly on a tile end, two of zero rows, 600 rows (longer
    than the ring of four tiles; cut short at m = 385); then the cycle of sizes; a record of
    zero rows at the very end.  m is no multiple of 128 and the last record with rows ends at
    m, in the ragged tile."""
    assert m % TILE
    counts, ptr = _records(m, LEAD)
    counts, ptr = counts + [0], np.append(ptr, m)
    assert counts[:3] == [128, 0, 0] and (m < 728 or counts[3] == 600)
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    _assert_columns_are_nearest(a, b, counts, ptr, metric, _best(a, b, counts, metric))


@pytest.mark.parametrize("metric", METRICS)
def test_records_of_one_row_are_the_dense_block(metric):
    n, m = 257, 385
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    counts = [1] * m
    best = _best(a, b, counts, metric)
    _assert_columns_are_nearest(a, b, counts, np.arange(m + 1), metric, best)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", ROWS_B)
def test_one_record_of_all_rows_is_nearest(m, metric):
    from ginfinity_amd import distance
    a, b = _device(_a_rows(385)), _device(_b_rows(m))
    best = _best(a, b, [m], metric)
    values, _ = distance.nearest(a, b, metric=metric)
    assert best.shape == (385, 1)
    assert best[:, 0].tobytes() == values.cpu().numpy().tobytes()


# ---- 2. chunks ----------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_records_across_chunk_and_tile_pair_cuts(gpu, metric):
    """The self-search of 8,269 rows: the library reports how many chunks it cuts b into, the
    test derives the cuts, finds a record across a chunk cut and one across a cut between two
    tile pairs inside a chunk, and the row level is nearest on every record all the same."""
    n = m = SELF_SEARCH
    chunks = gpu.gfy_pairwise_record_chunks(n, m)
    tiles = -(-m // TILE)
    assert 2 <= chunks < tiles, chunks
    per = [size for size in range(1, tiles + 1) if -(-tiles // size) == chunks]
    assert len(per) == 1 and per[0] >= 3, (chunks, per)     # the cuts follow from the count
    chunk_rows = per[0] * TILE
    counts, ptr = _records(m, LEAD)
    inside = lambda cut: bool(np.any((ptr[:-1] < cut) & (cut < ptr[1:])))
    chunk_cuts = [c * chunk_rows for c in range(1, chunks)]
    pair_cuts = [c * chunk_rows + 2 * TILE for c in range(chunks) if c * chunk_rows + 2 * TILE < m]
    assert any(inside(cut) for cut in chunk_cuts) and any(inside(cut) for cut in pair_cuts)
    x = _device_pool()[:n]
    _assert_columns_are_nearest(x, x, counts, ptr, metric, _best(x, None, counts, metric))


# ---- 3. the record level against float64 --------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", ROWS_B)
@pytest.mark.parametrize("n", ROWS_A)
def test_scores_against_the_float64_definition(n, m, metric):
    counts_b, ptr_b = _records(m, LEAD)                      # two b-records of zero rows
    counts_a, ptr_a = _records(n, (37, 0, 129))              # one a-record of zero rows
    want_best = _reference_best(_reference(n, m, metric), ptr_b, metric)
    filled = np.array(counts_b) > 0
    if metric == "l2":
        assert want_best[:, filled].min() >= 0.1             # the tolerance on d applies
    with np.errstate(invalid="ignore"):
        want = np.stack([want_best[ptr_a[q]:ptr_a[q + 1]].mean(axis=0) if counts_a[q]
                         else np.full(len(counts_b), np.nan) for q in range(len(counts_a))])
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    tol = L2_TOL if metric == "l2" else COSINE_TOL
    best = _best(a, b, counts_b, metric)
    print(metric, n, m, "row level, worst:", np.abs(best[:, filled] - want_best[:, filled]).max())
    assert np.all(np.abs(best[:, filled] - want_best[:, filled])
                  <= tol + ROUNDING * np.abs(want_best[:, filled]))
    got = _scores(a, b, counts_a=counts_a, counts_b=counts_b, metric=metric)
    assert got.shape == (len(counts_a), len(counts_b)) and got.dtype == np.float32
    rows = np.array(counts_a) > 0
    assert np.all(np.isnan(got[~rows])) and (~rows).sum() == 1
    assert np.all(got[rows][:, ~filled] == _empty(metric)) and (~filled).sum() == 2
    error = np.abs(got[rows][:, filled] - want[rows][:, filled])
    print(metric, n, m, "record level, worst:", error.max())
    assert np.all(error <= tol + ROUNDING * np.abs(want[rows][:, filled]))


# ---- 4. the score is the stated mean of best, bit for bit ---------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,m", [(257, 1_000), (385, 8_269)])
def test_score_is_the_float64_mean_of_the_row_level(n, m, metric):
    counts_b, _ = _records(m, LEAD)
    counts_a, ptr_a = _records(n, (37, 0, 129))
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    best = _best(a, b, counts_b, metric)
    got = _scores(a, b, counts_a=counts_a, counts_b=counts_b, metric=metric)
    assert _same(got, _mean_of_rows(best, ptr_a))


# ---- 5. independence and blocking, bit for bit --------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_entries_do_not_depend_on_the_rest_of_the_call(metric):
    n, m = 385, 1_000
    counts_b, ptr_b = _records(m, LEAD)
    counts_a, ptr_a = _records(n, (37, 0, 129))
    a, b = _a_rows(n), _b_rows(m)
    whole_best = _best(_device(a), _device(b), counts_b, metric)
    whole = _scores(_device(a), _device(b), counts_a=counts_a, counts_b=counts_b, metric=metric)
    keep_a = [q for q in range(len(counts_a)) if q % 3 != 2]
    keep_b = [r for r in range(len(counts_b)) if r % 4 != 0 or r == 1]
    assert len(keep_a) < len(counts_a) and len(keep_b) < len(counts_b)
    part_a = np.concatenate([a[ptr_a[q]:ptr_a[q + 1]] for q in keep_a])
    part_b = np.concatenate([b[ptr_b[r]:ptr_b[r + 1]] for r in keep_b])
    rows_a = np.concatenate([np.arange(ptr_a[q], ptr_a[q + 1]) for q in keep_a])
    part_counts_a = [counts_a[q] for q in keep_a]
    part_counts_b = [counts_b[r] for r in keep_b]
    got_best = _best(_device(part_a), _device(part_b), part_counts_b, metric)
    assert _same(got_best, whole_best[rows_a][:, keep_b])
    got = _scores(_device(part_a), _device(part_b), counts_a=part_counts_a,
                  counts_b=part_counts_b, metric=metric)
    assert _same(got, whole[keep_a][:, keep_b])


@pytest.mark.parametrize("metric", METRICS)
def test_blocking_and_repetition_change_no_bit(metric):
    from ginfinity_amd import distance
    n, m = 385, 1_000
    counts_b, _ = _records(m, LEAD)
    counts_a, _ = _records(n, (37, 0, 129))
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    arguments = dict(counts_a=counts_a, counts_b=counts_b, metric=metric)
    whole = _scores(a, b, **arguments)
    assert len(distance.plan_record_blocks(counts_a, len(counts_b),
                                           distance.RECORD_WORKSPACE_BYTES)) == 1
    budget = 130 * len(counts_b) * 4
    assert len(distance.plan_record_blocks(counts_a, len(counts_b), budget)) >= 3
    keeper = distance.RecordWorkspace()
    assert _same(_scores(a, b, max_workspace_bytes=budget, workspace=keeper, **arguments), whole)
    assert _same(_scores(a, b, workspace=keeper, **arguments), whole)
    assert _same(_scores(a, b, **arguments), whole)
    with pytest.raises(ValueError, match="needs"):
        _scores(a, b, max_workspace_bytes=128 * len(counts_b) * 4, **arguments)


# ---- 6. self-search -----------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_self_search_has_the_best_score_on_its_diagonal(metric):
    """Nothing is excluded: every row finds itself.  Cosine: within 2e-6 of 1.  L2: 0 up to the
    bound on d² (the head of this file); the kernel's d² of a row against itself is
    |x|² + (-2)(x.x - |x|²/2) with the two sums rounded in different orders, a few 1e-7, and
    only its negative half is clamped to 0."""
    n = 1_000
    counts, ptr = _records(n, (37, 0, 129))
    x = _device_pool()[:n]
    got = _scores(x, counts_a=counts, metric=metric)
    assert _same(got, _scores(x, x, counts_a=counts, counts_b=counts, metric=metric))
    assert _same(got, _scores(x, x.clone(), counts_a=counts, counts_b=counts, metric=metric))
    rows = np.flatnonzero(np.array(counts) > 0)
    diagonal = got[rows, rows]
    print(metric, "diagonal:", diagonal.min(), diagonal.max())
    if metric == "l2":
        scale = 2.0 * (_pool()[:n].astype(np.float64) ** 2).sum(1).max()
        assert np.all(diagonal >= 0) and np.all(diagonal <= np.sqrt(D2_TOL * scale))
        assert np.all(got[rows][:, rows].argmin(axis=1) == np.arange(len(rows)))
    else:
        assert np.all(np.abs(diagonal - 1.0) <= COSINE_TOL)
        assert np.all(got[rows][:, rows].argmax(axis=1) == np.arange(len(rows)))
    assert np.all(np.isnan(got[1])) and np.all(got[rows][:, 1] == _empty(metric))


# ---- 7. a planted answer ------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_a_planted_record_is_found(metric):
    """Record r of b holds exact copies of the rows of a-record q (in another order, among other
    rows): score[q, r] is 0 (l2, up to the bound on d²) or the maximum (cosine), and r is the
    argmin / argmax of row q."""
    n, m = 385, 1_000
    counts_a, ptr_a = _records(n, (37, 0, 129))
    counts_b, ptr_b = _records(m, LEAD)
    q, r = 5, 8
    assert 0 < counts_a[q] <= counts_b[r]
    a, b = np.array(_a_rows(n)), np.array(_b_rows(m))
    copies = a[ptr_a[q]:ptr_a[q + 1]][::-1]
    b[ptr_b[r + 1] - len(copies):ptr_b[r + 1]] = copies
    got = _scores(_device(a), _device(b), counts_a=counts_a, counts_b=counts_b, metric=metric)
    print(metric, "planted:", got[q, r], "next:", np.sort(got[q])[:2], np.sort(got[q])[-4:])
    if metric == "l2":
        scale = 2.0 * (a.astype(np.float64) ** 2).sum(1).max()
        assert 0 <= got[q, r] <= np.sqrt(D2_TOL * scale)
        assert np.argmin(got[q]) == r
    else:
        assert abs(got[q, r] - 1.0) <= COSINE_TOL
        assert got[q, r] == got[q][np.isfinite(got[q])].max() and np.argmax(got[q]) == r
