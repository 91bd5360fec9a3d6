"""Radius search on the GPU (distance.count_within, distance.within; gfy_pairwise_within_count,
gfy_pairwise_within_fill): every row of b whose value passes the threshold, per row of a.

The first oracle is the library's own dense values: ``record_best(a, b, counts_b=ones(m))`` is
``[n, m]`` with column j equal to ``nearest(a, b[j:j + 1])`` bit for bit, so ``within`` must
return exactly ``{j : dense[i, j] passes}`` per row in ascending j with the same value bits — an
entry equal to the threshold is a hit by definition, so no pair is ambiguous and none is left
out.  The second is the float64 definition (oracle/gine_numpy.py) on inputs whose hits are
planted so that no float64 value lies within 100 tolerances of the threshold: the share of
pairs the comparison may leave undecided is zero, which is asserted on the CPU first."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_topk.py
L2_TOL = 2e-5            # on an L2 distance d >= 0.1
BLOCK_A = 128            # a-rows per workgroup (pairwise_within.hip)
ORDER_LDS = 2_048        # entries k_within_order sorts in LDS; longer segments in global memory
METRICS = ("l2", "cosine")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


# --------------------------------------------------------------------------------------------
# inputs and the comparison against a dense block

def _mixed_rows(seed, count, unit):
    """The recipe of tests/test_gpu_distance_topk.py: unit rows, or norms in [0.2, 3)."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((count, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    if not unit:
        data *= rng.uniform(0.2, 3.0, size=(count, 1))
    return data.astype(np.float16)


def _device(rows):
    return torch.from_numpy(np.array(rows, order="C")).cuda()      # a copy: cached rows are read-only


def _dense(a, b, metric):
    """[n, m] float32: the library's own value of every pair (module docstring)."""
    from ginfinity_amd import distance
    return distance.record_best(a, b, counts_b=np.ones(b.shape[0], dtype=np.int64),
                                metric=metric).cpu().numpy()


def _within(a, b=None, **arguments):
    from ginfinity_amd import distance
    hits = distance.within(a, b, **arguments)
    assert hits.offsets.dtype == torch.int64 and hits.indices.dtype == torch.int32
    assert hits.values.dtype == torch.float32
    assert hits.rows().shape == hits.indices.shape
    return hits.offsets.cpu().numpy(), hits.indices.cpu().numpy(), hits.values.cpu().numpy()


def _count(a, b=None, **arguments):
    from ginfinity_amd import distance
    counts = distance.count_within(a, b, **arguments)
    assert counts.dtype == torch.int32
    return counts.cpu().numpy()


def _passes(dense, threshold, metric):
    threshold = np.float32(threshold)
    return dense <= threshold if metric == "l2" else dense >= threshold


def _bits(values):
    """The bits of float32 values, a zero without its sign (a maximum does not tell +0 from -0:
    include/gfy.h on gfy_pairwise_record_best)."""
    return (np.asarray(values, dtype=np.float32) + np.float32(0.0)).view(np.uint32)


def _assert_is(got, counts, dense, mask):
    """``got`` = (offsets, indices, values) is exactly the set ``mask`` of the dense block."""
    offsets, indices, values = got
    want = np.concatenate(([0], np.cumsum(mask.sum(1, dtype=np.int64))))
    assert offsets.shape == want.shape and np.array_equal(offsets, want)
    assert np.array_equal(counts.astype(np.int64), np.diff(offsets))
    rows, columns = np.nonzero(mask)          # row-major: ascending j inside a row
    assert np.array_equal(indices, columns.astype(np.int32))
    assert np.array_equal(_bits(values), _bits(dense[rows, columns]))


def _thresholds(dense, metric):
    """Three thresholds from the dense values themselves: below every value, at a value that
    occurs, and the 2 % (cosine: 98 %) quantile."""
    flat = np.sort(dense.ravel())
    below = np.nextafter(flat[0], np.float32(-np.inf), dtype=np.float32)
    occurs = flat[flat.size // 3]
    quantile = np.float32(np.quantile(flat.astype(np.float64), 0.02 if metric == "l2" else 0.98))
    return float(below), float(occurs), float(quantile)


# --------------------------------------------------------------------------------------------
# 1. bit-exact against the library's own dense values

SHAPES = ((1, 1), (129, 127), (255, 129), (257, 385), (130, 1_000), (300, 500))


def test_the_multi_chunk_shape_is_multi_chunk(gpu):
    assert gpu.gfy_pairwise_within_chunks(130, 1_000) > 1


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("unit", (True, False), ids=("unit", "mixed"))
@pytest.mark.parametrize("metric", METRICS)
def test_hits_are_the_dense_values_that_pass_bit_for_bit(gpu, metric, unit, n, m):
    a, b = _mixed_rows(3 * n + m, n, unit), _mixed_rows(5 * m + n, m, unit)
    a_dev, b_dev = _device(a), _device(b)
    dense = _dense(a_dev, b_dev, metric)
    assert dense.shape == (n, m)
    below, occurs, quantile = _thresholds(dense, metric)
    for threshold in (below, occurs, quantile):
        mask = _passes(dense, threshold, metric)
        if threshold == below:
            assert mask.sum() == (0 if metric == "l2" else n * m)
        if threshold == occurs:
            assert np.any(dense == np.float32(threshold))     # equality is exercised
        got = _within(a_dev, b_dev, threshold=threshold, metric=metric)
        counts = _count(a_dev, b_dev, threshold=threshold, metric=metric)
        _assert_is(got, counts, dense, mask)


# --------------------------------------------------------------------------------------------
# 2. m <= 16 against topk(k = m)

@pytest.mark.parametrize("m", (1, 3, 15, 16))
@pytest.mark.parametrize("metric", METRICS)
def test_small_m_is_topk_restricted_to_the_entries_that_pass(gpu, metric, m):
    from ginfinity_amd import distance
    n = 200
    a_dev, b_dev = _device(_mixed_rows(7 * m, n, False)), _device(_mixed_rows(11 * m, m, False))
    top_val, top_idx = distance.topk(a_dev, b_dev, k=m, metric=metric)
    top_val, top_idx = top_val.cpu().numpy(), top_idx.cpu().numpy()
    assert top_idx.min() >= 0
    threshold = float(np.sort(top_val.ravel())[top_val.size // 2])
    offsets, indices, values = _within(a_dev, b_dev, threshold=threshold, metric=metric)
    keep = _passes(top_val, threshold, metric)
    assert 0 < keep.sum() < n * m or m == 1
    assert np.array_equal(np.diff(offsets), keep.sum(1))
    for i in range(n):
        order = np.argsort(top_idx[i][keep[i]])
        assert np.array_equal(indices[offsets[i]:offsets[i + 1]], top_idx[i][keep[i]][order])
        assert np.array_equal(_bits(values[offsets[i]:offsets[i + 1]]),
                              _bits(top_val[i][keep[i]][order]))


# --------------------------------------------------------------------------------------------
# 3. against the float64 definition on multi-tile sweeps, hits planted

PLANTED = ((1_000, 3_000), (64, 20_000), (70_000, 2_560))
COSINE_THRESHOLD = 0.8
L2_THRESHOLD = float(np.sqrt(2.0 - 1.6))      # the same pairs on unit rows
MOST_PLANTED = 40


def _sample(n, seed):
    """Both sides of 64 workgroup seams, the first and the last 300 rows, random rows: 2,000."""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.arange(1, n // BLOCK_A), size=64, replace=False)
    fixed = np.unique(np.concatenate([BLOCK_A * blocks - 1, BLOCK_A * blocks, np.arange(300),
                                      np.arange(n - 300, n)]))
    others = np.setdiff1d(np.arange(n), fixed)
    rows = np.sort(np.concatenate([fixed, rng.choice(others, 2_000 - fixed.size, replace=False)]))
    assert np.isin(BLOCK_A * blocks - 1, rows).all() and np.isin(BLOCK_A * blocks, rows).all()
    return rows


@functools.lru_cache(maxsize=None)
def _planted_case(n, m):
    """(a, b, rows, oracle): unit rows whose hits are planted.  ``a`` repeats G = min(n, m // 24)
    random centres (row i is centre i mod G, so that m rows of b can serve every row of a);
    centre g owns 0..40 rows of b, each its fp16 row turned by an angle whose cosine lies in
    [0.94, 0.99] and rounded to fp16, at columns of a random permutation; every other row of b
    is random.  ``rows`` are the checked a-rows (all, or 2,000 with both sides of block seams)
    and ``oracle[metric]`` their float64 values [rows][m]."""
    from oracle import gine_numpy as G
    rng = np.random.default_rng(1_000 * n + m)
    groups = min(n, m // 24)
    centres = rng.standard_normal((groups, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    centres = centres.astype(np.float16)
    owned = rng.integers(0, MOST_PLANTED + 1, size=groups)
    owned[:2] = (0, MOST_PLANTED)
    assert owned.sum() <= m
    b = rng.standard_normal((m, 128))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    columns = rng.permutation(m)[:owned.sum()]
    owner = np.repeat(np.arange(groups), owned)
    centre = centres[owner].astype(np.float64)
    centre /= np.linalg.norm(centre, axis=1, keepdims=True)
    noise = rng.standard_normal((owner.size, 128))
    noise -= (noise * centre).sum(1, keepdims=True) * centre
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cosine = rng.uniform(0.94, 0.99, size=(owner.size, 1))
    b[columns] = cosine * centre + np.sqrt(1.0 - cosine ** 2) * noise
    b = b.astype(np.float16)
    a = centres[np.arange(n) % groups]
    assert np.unique(columns % 128).size == 128           # every residue mod 128 holds a hit
    rows = np.arange(n) if n <= 2_000 else _sample(n, n + m)
    oracle = {"cosine": G.pairwise_cosine(a[rows], b), "l2": G.pairwise_l2(a[rows], b)}
    # the recipe: hits at cosine >= 0.93, everything else below 0.6, nothing near the threshold
    planted = np.zeros((groups, m), dtype=bool)
    planted[owner, columns] = True
    planted = planted[rows % groups]
    assert oracle["cosine"][planted].min() >= 0.93 and oracle["cosine"][~planted].max() < 0.6
    assert np.abs(oracle["cosine"] - COSINE_THRESHOLD).min() > 100 * COSINE_TOL
    assert np.abs(oracle["l2"] - L2_THRESHOLD).min() > 100 * L2_TOL
    assert np.array_equal(oracle["l2"] <= L2_THRESHOLD, planted)
    assert np.array_equal(oracle["cosine"] >= COSINE_THRESHOLD, planted)
    assert oracle["l2"][planted].min() >= 0.1              # where L2_TOL is stated
    per_row = planted.sum(1)
    assert per_row.min() == 0 and per_row.max() == MOST_PLANTED
    for array in (a, b, rows, oracle["cosine"], oracle["l2"]):
        array.setflags(write=False)
    return a, b, rows, oracle


@pytest.mark.parametrize("n,m", PLANTED)
@pytest.mark.parametrize("metric", METRICS)
def test_planted_hits_against_the_float64_definition(gpu, metric, n, m):
    a, b, rows, oracle = _planted_case(n, m)      # asserts the gap on the CPU first
    full = oracle[metric]
    threshold = L2_THRESHOLD if metric == "l2" else COSINE_THRESHOLD
    want = full <= threshold if metric == "l2" else full >= threshold
    a_dev, b_dev = _device(a), _device(b)
    offsets, indices, values = _within(a_dev, b_dev, threshold=threshold, metric=metric)
    counts = _count(a_dev, b_dev, threshold=threshold, metric=metric)
    assert np.array_equal(counts.astype(np.int64), np.diff(offsets))
    assert np.array_equal(counts[rows], want.sum(1))
    tolerance = L2_TOL if metric == "l2" else COSINE_TOL
    worst = 0.0
    for at, i in enumerate(rows):
        segment = slice(offsets[i], offsets[i + 1])
        columns = np.nonzero(want[at])[0]
        assert np.array_equal(indices[segment], columns), i
        if columns.size:
            worst = max(worst, float(np.abs(values[segment] - full[at, columns]).max()))
    print(f"within {metric} {n} x {m}: worst deviation {worst:.3g} (tolerance {tolerance:g})")
    assert worst <= tolerance


# --------------------------------------------------------------------------------------------
# 4. exclusions

RECORDS = (1, 63, 64, 65, 200, 7)


@functools.lru_cache(maxsize=None)
def _self_search(metric):
    a = _mixed_rows(77, sum(RECORDS), False)
    a_dev = _device(a)
    dense = _dense(a_dev, a_dev, metric)
    dense.setflags(write=False)
    return a_dev, dense, _thresholds(dense, metric)[2]


@pytest.mark.parametrize("metric", METRICS)
def test_exclude_self_drops_the_best_pair_of_every_row(gpu, metric):
    a_dev, dense, threshold = _self_search(metric)
    n = dense.shape[0]
    mask = _passes(dense, threshold, metric)
    assert mask[np.arange(n), np.arange(n)].all()         # (i, i) is a hit, and the best one
    best = dense.min(1) if metric == "l2" else dense.max(1)
    assert np.array_equal(_bits(best), _bits(dense[np.arange(n), np.arange(n)]))
    mask = mask & ~np.eye(n, dtype=bool)
    got = _within(a_dev, threshold=threshold, metric=metric, exclude_self=True)
    counts = _count(a_dev, threshold=threshold, metric=metric, exclude_self=True)
    _assert_is(got, counts, dense, mask)
    assert not np.any(got[1] == np.repeat(np.arange(n), np.diff(got[0])))


@pytest.mark.parametrize("metric", METRICS)
def test_exclude_records_drops_the_row_s_own_record(gpu, metric):
    a_dev, dense, threshold = _self_search(metric)
    n = dense.shape[0]
    ptr = np.concatenate(([0], np.cumsum(RECORDS)))
    record = np.repeat(np.arange(len(RECORDS)), RECORDS)
    own = record[:, None] == record[None, :]
    mask = _passes(dense, threshold, metric)
    assert (mask & own).sum() > n                          # more than the diagonal is dropped
    got = _within(a_dev, threshold=threshold, metric=metric, exclude_records=RECORDS)
    counts = _count(a_dev, threshold=threshold, metric=metric, exclude_records=RECORDS)
    _assert_is(got, counts, dense, mask & ~own)
    rows = np.repeat(np.arange(n), np.diff(got[0]))
    assert not np.any((got[1] >= ptr[record[rows]]) & (got[1] < ptr[record[rows] + 1]))


@pytest.mark.parametrize("metric", METRICS)
def test_exclude_ranges_any_bounds_and_empty_ranges(gpu, metric):
    a_dev, dense, threshold = _self_search(metric)
    n = dense.shape[0]
    mask = _passes(dense, threshold, metric)
    rng = np.random.default_rng(5)
    # lo >= hi excludes nothing
    lo = rng.integers(-50, n + 50, n).astype(np.int32)
    hi = (lo - rng.integers(0, 30, n)).astype(np.int32)
    got = _within(a_dev, threshold=threshold, metric=metric, exclude_ranges=(lo, hi))
    counts = _count(a_dev, threshold=threshold, metric=metric, exclude_ranges=(lo, hi))
    _assert_is(got, counts, dense, mask)
    # unsorted, overlapping ranges that reach past both ends of b are clipped by the comparison
    hi = (lo + rng.integers(0, 120, n)).astype(np.int32)
    columns = np.arange(n)[None, :]
    gone = (columns >= lo[:, None]) & (columns < hi[:, None])
    assert (mask & gone).any()
    got = _within(a_dev, threshold=threshold, metric=metric, exclude_ranges=(lo, hi))
    counts = _count(a_dev, threshold=threshold, metric=metric, exclude_ranges=(lo, hi))
    _assert_is(got, counts, dense, mask & ~gone)


# --------------------------------------------------------------------------------------------
# 5. independence and reproducibility

BIG = 131_072


@functools.lru_cache(maxsize=None)
def _big():
    from ginfinity_amd import synthetic
    return _device(synthetic.unit_rows(101, BIG)), _device(synthetic.unit_rows(202, 1_000))


def _loose(metric):
    """About two hits per row among 1,000 random unit rows (cosine 0.25 is 2.8 sigma)."""
    return float(np.sqrt(2.0 - 0.5)) if metric == "l2" else 0.25


@pytest.mark.parametrize("metric", METRICS)
def test_a_row_s_segment_does_not_depend_on_the_call_it_is_in(gpu, metric):
    a_dev, b_dev = _big()
    threshold = _loose(metric)
    offsets, indices, values = _within(a_dev, b_dev, threshold=threshold, metric=metric)
    assert offsets[-1] > BIG
    picked = np.array([0, 127, 128, 5_000, 65_535, 65_536, 100_001, BIG - 1])
    assert gpu.gfy_pairwise_within_chunks(picked.size, 1_000) > 1 == \
        gpu.gfy_pairwise_within_chunks(BIG, 1_000)        # cut differently, too
    alone = _within(a_dev[torch.from_numpy(picked).cuda()], b_dev, threshold=threshold,
                    metric=metric)
    assert alone[0][-1] > 0
    for at, i in enumerate(picked):
        there = slice(offsets[i], offsets[i + 1])
        here = slice(alone[0][at], alone[0][at + 1])
        assert np.array_equal(indices[there], alone[1][here])
        assert np.array_equal(values[there].view(np.uint32), alone[2][here].view(np.uint32))


def test_two_runs_give_the_same_bytes_and_a_grown_workspace_changes_nothing(gpu):
    from ginfinity_amd import distance
    a_dev, b_dev = _big()
    small = a_dev[:4_097]
    first = _within(small, b_dev, threshold=0.25, metric="cosine")
    second = _within(small, b_dev, threshold=0.25, metric="cosine")
    keeper = distance.WithinWorkspace()
    grown = _within(a_dev[:20_000], b_dev, threshold=0.3, metric="cosine", workspace=keeper)
    assert grown[0][-1] > 0
    bytes_kept = keeper.scratch.numel()
    third = _within(small, b_dev, threshold=0.25, metric="cosine", workspace=keeper)
    assert keeper.scratch.numel() == bytes_kept
    counts = _count(small, b_dev, threshold=0.25, metric="cosine", workspace=keeper)
    for other in (second, third):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    assert np.array_equal(counts.astype(np.int64), np.diff(first[0]))


# --------------------------------------------------------------------------------------------
# 6. nesting

def test_l2_hit_sets_are_nested_in_the_threshold(gpu):
    a_dev, b_dev = _device(_mixed_rows(1, 257, False)), _device(_mixed_rows(2, 385, False))
    dense = _dense(a_dev, b_dev, "l2")
    t1, t2 = (float(np.float32(np.quantile(dense, q))) for q in (0.05, 0.2))
    assert t1 < t2
    inner = _within(a_dev, b_dev, threshold=t1)
    outer = _within(a_dev, b_dev, threshold=t2)
    assert 0 < inner[0][-1] < outer[0][-1]
    for i in range(257):
        small = inner[1][inner[0][i]:inner[0][i + 1]]
        large = outer[1][outer[0][i]:outer[0][i + 1]]
        assert np.isin(small, large).all()


# --------------------------------------------------------------------------------------------
# 7. max_hits

def test_too_many_hits_is_raised_before_the_fill(gpu, monkeypatch):
    from ginfinity_amd import distance
    a_dev, b_dev = _device(_mixed_rows(1, 257, True)), _device(_mixed_rows(2, 385, True))
    total = int(_count(a_dev, b_dev, threshold=0.1, metric="cosine").sum())
    assert total > 1
    want = _within(a_dev, b_dev, threshold=0.1, metric="cosine")

    def no_fill(self, offsets, count):
        raise AssertionError("the fill was started")
    with monkeypatch.context() as patch:
        patch.setattr(distance._WithinCall, "fill", no_fill)
        for max_hits in (1, total - 1):
            with pytest.raises(distance.TooManyHits) as caught:
                distance.within(a_dev, b_dev, threshold=0.1, metric="cosine", max_hits=max_hits)
            assert caught.value.total == total
    got = _within(a_dev, b_dev, threshold=0.1, metric="cosine", max_hits=total)
    for x, y in zip(want, got):
        assert x.tobytes() == y.tobytes()


def test_no_rows_and_no_hit_return_empty_tensors(gpu, monkeypatch):
    from ginfinity_amd import distance

    def no_fill(self, offsets, count):
        raise AssertionError("the fill was started")
    monkeypatch.setattr(distance._WithinCall, "fill", no_fill)
    rows = _device(_mixed_rows(1, 5, True))
    none = rows[:0]
    for a, b, n in ((none, rows, 0), (rows, none, 5), (rows, rows, 5)):
        hits = distance.within(a, b, threshold=-1.0, metric="l2")
        assert hits.offsets.tolist() == [0] * (n + 1)
        assert hits.indices.numel() == hits.values.numel() == 0
        assert distance.count_within(a, b, threshold=-1.0, metric="l2").tolist() == [0] * n


# --------------------------------------------------------------------------------------------
# 8. the segment guard: offsets that are valid, in bounds and one slot short for one row

def test_a_segment_one_slot_short_is_reported_and_nothing_is_stored_outside_it(gpu):
    from ginfinity_amd import _native as native
    n, m, threshold = 129, 127, 0.05
    a_dev, b_dev = _device(_mixed_rows(3, n, True)), _device(_mixed_rows(4, m, True))
    offsets, indices, values = _within(a_dev, b_dev, threshold=threshold, metric="cosine")
    counts = np.diff(offsets)
    row = int(np.nonzero((counts[:-1] >= 2) & (counts[1:] >= 1))[0][0])
    total = int(offsets[-1])
    short = offsets.copy()
    short[row + 1:] -= 1              # row's segment loses its last slot; the total is total - 1
    short_dev = torch.from_numpy(short).cuda()
    got_idx = torch.full((total,), -7, dtype=torch.int32, device="cuda")    # total entries are
    got_val = torch.full((total,), -7.0, dtype=torch.float32, device="cuda")  # allocated
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(gpu.gfy_pairwise_within_workspace_bytes(n, m), dtype=torch.uint8,
                          device="cuda")
    native.check(gpu.gfy_pairwise_within_fill(
        a_dev.data_ptr(), n, b_dev.data_ptr(), m, native.GFY_COSINE, threshold, None, None,
        short_dev.data_ptr(), got_idx.data_ptr(), got_val.data_ptr(), status.data_ptr(),
        scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream),
        "gfy_pairwise_within_fill")
    torch.cuda.synchronize()
    assert int(status.item()) != 0
    got_idx, got_val = got_idx.cpu().numpy(), got_val.cpu().numpy()
    # the word behind the row's segment belongs to the next row and is that row's first hit
    assert got_idx[short[row + 1]] == indices[offsets[row + 1]]
    assert got_idx[total - 1] == -7 and got_val[total - 1] == -7.0      # behind offsets[n]: untouched
    for i in range(n):
        mine = got_idx[short[i]:short[i + 1]]
        true = indices[offsets[i]:offsets[i + 1]]
        if i == row:                  # one hit was dropped, whichever; the others are in order
            assert mine.size == true.size - 1 and np.isin(mine, true).all()
            assert np.all(np.diff(mine) > 0)
        else:
            assert np.array_equal(mine, true)
            assert np.array_equal(got_val[short[i]:short[i + 1]].view(np.uint32),
                                  values[offsets[i]:offsets[i + 1]].view(np.uint32))


# --------------------------------------------------------------------------------------------
# 9. segments longer than the ordering kernel's LDS

@pytest.mark.parametrize("metric", METRICS)
def test_segments_longer_than_the_lds_sort_holds(gpu, metric):
    n, m = 4, 6_000
    assert m > ORDER_LDS
    a_dev, b_dev = _device(_mixed_rows(8, n, False)), _device(_mixed_rows(9, m, False))
    dense = _dense(a_dev, b_dev, metric)
    # every pair is a hit: below everything (cosine), above everything (l2)
    threshold = float(np.nextafter(dense.min(), np.float32(-np.inf), dtype=np.float32)) \
        if metric == "cosine" else float(dense.max())
    mask = _passes(dense, threshold, metric)
    assert mask.all()
    got = _within(a_dev, b_dev, threshold=threshold, metric=metric)
    counts = _count(a_dev, b_dev, threshold=threshold, metric=metric)
    _assert_is(got, counts, dense, mask)
