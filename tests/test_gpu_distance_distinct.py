"""Top-k search with at most one hit per record of b (gfy_pairwise_topk_distinct;
distance.topk(distinct_records=...), distance.record_of; csrc/pairwise_topk_distinct.hip).

Inputs, record sizes and tolerances are those of tests/test_gpu_distance_ranges.py.  The result
is compared bit for bit with what the plain search gives where the two must agree (records of one
row; the de-duplicated plain k = 16 list), rank-wise with the float64 definition of
oracle.gine_numpy taken per record, and on planted neighbours and ties whose answer is known."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_ranges.py
L2_TOL = 2e-5            # on an L2 distance d >= 0.1
D2_TOL = 4e-6            # on d², times (|a_i|² + |b_j|²)
BLOCK_A = 128            # a-rows per workgroup, b-rows per tile (pairwise_topk.inc)
RECORD_SIZES = (1, 2, 37, 100, 128, 129, 300)
METRICS = ("l2", "cosine")
SELF_SEARCHES = (1_000, 8_269)


def _kmax():
    from ginfinity_amd import _native
    return _native.GFY_PAIRWISE_TOPK_DISTINCT_MAX


KMAX = _kmax()


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


@functools.lru_cache(maxsize=None)
def _pool(seed, rows):
    from ginfinity_amd import synthetic
    data = synthetic.unit_rows(seed, rows)
    data.setflags(write=False)
    return data


def _rows(n):
    return _pool(101, 20_480)[:n].copy()


def _device(rows):
    return torch.from_numpy(np.array(rows)).cuda()           # a copy: shared inputs are read-only


def _topk(a, b=None, **arguments):
    from ginfinity_amd import distance
    values, indices = distance.topk(a, b, **arguments)
    return values.cpu().numpy(), indices.cpu().numpy()


def _same(one, two):
    return (np.ascontiguousarray(one[0]).tobytes() == np.ascontiguousarray(two[0]).tobytes()
            and np.ascontiguousarray(one[1]).tobytes() == np.ascontiguousarray(two[1]).tobytes())


def _records(n, lead=()):
    """Record sizes: ``lead``, then RECORD_SIZES over and over until n rows are used up (the last
    one cut short).  Returns (counts, ptr)."""
    counts, at = list(lead), 0
    while sum(counts) < n:
        counts.append(min(RECORD_SIZES[at % len(RECORD_SIZES)], n - sum(counts)))
        at += 1
    ptr = np.concatenate(([0], np.cumsum(counts)))
    assert ptr[-1] == n and min(counts) > 0
    return counts, ptr


def _record_of(indices, ptr):
    """Record number per index for non-empty records, -1 for -1 (a numpy loop-free stand-in that
    does not go through distance.record_of)."""
    found = np.searchsorted(ptr, indices, side="right") - 1
    return np.where(indices < 0, -1, found)


def _align(size):
    return (size + 255) // 256 * 256


def _sweep(lib, n, m, k=8):
    """(chunks, tiles per workgroup, tiles of the last chunk) of topk(n, m), recovered from the
    workspace size as tests/test_gpu_distance_ranges.py does."""
    tiles_b = (m + 127) // 128
    partial, odd = divmod(lib.gfy_pairwise_topk_workspace_bytes(n, m, k)
                          - 2 * _align(tiles_b * 128 * 4) - _align(n * 4), 2)
    assert odd == 0 and n * k * 4 >= 256
    fits = [c for c in range(1, tiles_b + 1) if _align(c * n * k * 4) == partial]
    assert len(fits) == 1, (n, m, fits)
    chunks = fits[0]
    per = -(-tiles_b // chunks)
    return chunks, per, tiles_b - (chunks - 1) * per


def _empty(metric):
    return np.float32(np.inf if metric == "l2" else -np.inf)


# --------------------------------------------------------------------------------------------
# 1. records of one row: the plain search bit for bit

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,m", [(257, 385), (513, 640), (8_000, 8_269)])
def test_records_of_one_row_are_the_plain_search_bit_for_bit(gpu, n, m, metric):
    pool = _device(_rows(m + 7))
    b = pool[:m]
    ones = [1] * m
    rng = np.random.default_rng(n)
    lo = rng.integers(-20, m, size=n).astype(np.int32)
    hi = (lo + rng.integers(-3, 200, size=n)).astype(np.int32)
    cases = [
        (pool[5:5 + n], b, {}),
        (pool[5:5 + n], b, dict(exclude_offset=5)),          # a is rows [5, 5 + n) of b
        (pool, b[7:], dict(window_first=7)),                 # b is rows [7, ...) of a
        (pool[5:5 + n], b, dict(exclude_ranges=(lo, hi))),
    ]
    for k in (1, 5, KMAX):
        for a_rows, b_rows, arguments in cases:
            counts = ones[:b_rows.shape[0]]
            plain = _topk(a_rows, b_rows, k=k, metric=metric, **arguments)
            distinct = _topk(a_rows, b_rows, k=k, metric=metric, distinct_records=counts,
                             **arguments)
            assert _same(plain, distinct), (k, sorted(arguments))
    plain = _topk(b, k=5, metric=metric, exclude_self=True)
    assert _same(plain, _topk(b, k=5, metric=metric, exclude_self=True, distinct_records=ones))


# --------------------------------------------------------------------------------------------
# the self-searches over records that tests 2, 3 and 7 share

@functools.lru_cache(maxsize=None)
def _self_search(n, metric):
    """(rows, counts, ptr, plain k = 16 result, distinct k = KMAX result), every row's own
    record excluded.  Computed once; nobody writes to it."""
    rows = _rows(n)
    counts, ptr = _records(n)
    device = _device(rows)
    plain = _topk(device, k=16, metric=metric, exclude_records=counts)
    distinct = _topk(device, k=KMAX, metric=metric, exclude_records=counts,
                     distinct_records=counts)
    for array in (rows, *plain, *distinct):
        array.setflags(write=False)
    return rows, counts, ptr, plain, distinct


def test_the_geometry_the_cases_rely_on(gpu):
    chunks, per, last = _sweep(gpu, 8_269, 8_269)
    print(f"topk(8269, 8269): {chunks} chunks of {per} tiles, the last of {last}")
    assert chunks > 1 and per == 4 and 8_269 % BLOCK_A != 0
    chunks, per, last = _sweep(gpu, 1_000, 1_000)
    assert chunks == 8 and per == 1


# 2. what the plain k = 16 list determines (property 3), and property 4

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", SELF_SEARCHES)
def test_first_columns_are_the_deduplicated_plain_list_bit_for_bit(gpu, n, metric):
    rows, counts, ptr, plain, whole = _self_search(n, metric)
    plain_val, plain_idx = plain
    record = _record_of(plain_idx, ptr)
    first = np.ones(plain_idx.shape, dtype=bool)          # the first entry of its record in the row
    for c in range(1, 16):
        first[:, c] = (plain_idx[:, c] >= 0) & ~np.any(record[:, :c] == record[:, c:c + 1], axis=1)
    first[:, 0] = plain_idx[:, 0] >= 0
    kept = first.sum(axis=1)
    assert kept.min() >= 1 and kept.max() > kept.min()
    order = np.argsort(~first, axis=1, kind="stable")     # the kept columns in front, in order
    want_val = np.take_along_axis(plain_val, order, axis=1)
    want_idx = np.take_along_axis(plain_idx, order, axis=1)
    device = _device(rows)
    own = _record_of(np.arange(n), ptr)
    for k in (4, 8, KMAX):
        values, indices = whole if k == KMAX else _topk(
            device, k=k, metric=metric, exclude_records=counts, distinct_records=counts)
        valid = np.arange(k)[None, :] < np.minimum(kept, k)[:, None]
        assert np.array_equal(indices[valid], want_idx[:, :k][valid]), k
        assert values[valid].tobytes() == want_val[:, :k][valid].tobytes(), k
        found = _record_of(indices, ptr)
        for c in range(1, k):                              # property 4
            assert not np.any((found[:, c] >= 0) & np.any(found[:, :c] == found[:, c:c + 1], axis=1))
        assert not np.any(found == own[:, None]), "a column inside the row's own record"
        assert np.all((indices >= 0) == np.isfinite(values))


# 3. rank-wise against the float64 definition taken per record

def _sample(n, per_chunk_rows):
    edges = [e for e in range(BLOCK_A, n, BLOCK_A)] + [per_chunk_rows]
    fixed = {r for e in edges for r in (e - 1, e) if 0 <= r < n} | {0, n - 1}
    rng = np.random.default_rng(n)
    rest = [r for r in rng.permutation(n) if r not in fixed][:512 - len(fixed)]
    sample = np.array(sorted(fixed | set(int(r) for r in rest)))
    assert sample.size == 512
    return sample


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", SELF_SEARCHES)
def test_against_the_float64_definition_per_record(gpu, n, metric):
    from oracle import gine_numpy as G
    rows, counts, ptr, _, (values, indices) = _self_search(n, metric)
    chunks, per, _ = _sweep(gpu, n, n)
    sample = _sample(n, per * BLOCK_A)
    a = rows[sample]
    full = G.pairwise_l2(a, rows) if metric == "l2" else G.pairwise_cosine(a, rows)
    if metric == "cosine":
        full = -full                                       # smaller is better for both
    own = _record_of(sample, ptr)
    optimum = np.minimum.reduceat(full, ptr[:-1], axis=1)  # [512][records]
    optimum[np.arange(sample.size), own] = np.inf          # the own record has no representative
    best = np.sort(optimum, axis=1)[:, :KMAX]
    if best.shape[1] < KMAX:
        best = np.pad(best, ((0, 0), (0, KMAX - best.shape[1])), constant_values=np.inf)
    got = values[sample].astype(np.float64) * (-1.0 if metric == "cosine" else 1.0)
    idx = indices[sample]
    valid = idx >= 0
    assert np.array_equal(valid, np.isfinite(best)), "columns and records with a representative"
    assert np.all(np.isinf(values[sample][~valid]))
    found = _record_of(idx, ptr)
    mine = np.where(valid, np.take_along_axis(optimum, np.maximum(found, 0), axis=1), np.inf)
    picked = np.where(valid, np.take_along_axis(full, np.maximum(idx, 0), axis=1), np.inf)
    worst = 0.0
    for name, one, two in (("rank", got, best), ("record", got, mine), ("row", got, picked)):
        x, y = one[valid], two[valid]
        if metric == "cosine":
            error = np.abs(x - y)
            assert error.max() <= COSINE_TOL, (name, error.max())
            worst = max(worst, float(error.max()))
        else:
            scale = ((a.astype(np.float64) ** 2).sum(1)[:, None]
                     + (rows[np.maximum(idx, 0)].astype(np.float64) ** 2).sum(2))[valid]
            error = np.abs(x ** 2 - y ** 2) / scale
            assert error.max() <= D2_TOL, (name, error.max())
            far = y >= 0.1
            assert np.all(np.abs(x - y)[far] <= L2_TOL), name
            worst = max(worst, float(error.max()))
    print(f"n = {n} {metric}: worst deviation {worst:.3g}")


# 4. planted neighbours

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", SELF_SEARCHES)
def test_planted_copies_one_column_per_record(gpu, n, metric):
    from ginfinity_amd import distance
    from oracle import gine_numpy as G
    rows = _rows(n)
    # the big record is rows [400, 700): across the tile boundaries 512 and 640, and 512 is a
    # chunk boundary of both searches (chunks of 1 and of 4 tiles)
    counts, ptr = _records(n, lead=[100] * 4 + [300] + [20] * 8)
    query, big = 50, 4
    copies = 400 + 19 * np.arange(16)
    assert copies[5] < 512 < copies[6] and copies[-1] < 700
    base = rows[query].astype(np.float32)
    for c, at in enumerate(copies):
        row = base.copy()
        row[c] += 0.01 * (c + 1)
        rows[at] = row.astype(np.float16)
    singles = 700 + 20 * np.arange(8) + 3
    shuffle = np.array([5, 2, 7, 0, 3, 6, 1, 4])           # distance order is not row order
    for s, at in enumerate(singles):
        row = base.copy()
        row[20 + s] += 0.2 + 0.02 * shuffle[s]
        rows[at] = row.astype(np.float16)
    a = rows[query:query + 1]
    planted = np.concatenate((copies, singles))
    exact = (G.pairwise_l2(a, rows[planted]) if metric == "l2"
             else -G.pairwise_cosine(a, rows[planted]))[0]
    assert exact[:16].max() < exact[16:].min() - 1e-3      # every copy beats every single
    others = np.setdiff1d(np.arange(n), np.concatenate((planted, np.arange(0, 100))))
    rest = (G.pairwise_l2(a, rows[others]) if metric == "l2" else -G.pairwise_cosine(a, rows[others]))
    assert exact.max() < rest.min() - 1e-3                  # and every planted row the others
    device = _device(rows)
    _, plain = _topk(device, k=8, metric=metric, exclude_records=counts)
    assert np.all(_record_of(plain[query], ptr) == big), "the case does not bite"
    want = [big] + [5 + int(s) for s in np.argsort(exact[16:])]
    for k in (4, 8, KMAX):
        _, indices = distance.topk(device, k=k, metric=metric, exclude_records=counts,
                                   distinct_records=counts)
        found = distance.record_of(indices, counts)
        assert found.shape == indices.shape and found.device == indices.device
        assert found.dtype == torch.int32
        assert found[query].tolist()[:9] == want[:k], k
        assert int(indices[query, 0]) == copies[int(np.argmin(exact[:16]))]


# 5. ties

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("first,second", [(1, 9),            # one lane's 16 values of a tile
                                          (5, 70),           # two waves' 32-row slices
                                          (10, 10 + 3 * 512)])   # two chunks
def test_ties_inside_a_record_and_between_records(gpu, first, second, metric):
    n, query = 8_269, 7_000
    rows = _rows(n)
    twin = rows[query].astype(np.float32)
    twin[3] += 0.02
    rows[first] = rows[second] = twin.astype(np.float16)
    device = _device(rows)
    skip = (np.array([query], dtype=np.int32), np.array([query + 1], dtype=np.int32))
    together = [1_600] + [100] * 66 + [69]                  # both rows in the first record
    apart = [1] * n
    _, same = _topk(device[query:query + 1], device, k=4, metric=metric, exclude_ranges=skip,
                    distinct_records=together)
    assert same[0, 0] == first and second not in same[0]
    assert np.all(same[0, 1:] >= 1_600)
    _, both = _topk(device[query:query + 1], device, k=4, metric=metric, exclude_ranges=skip,
                    distinct_records=apart)
    assert both[0, :2].tolist() == [first, second]


# 6. fewer records than k

@pytest.mark.parametrize("metric", METRICS)
def test_fewer_records_than_k(gpu, metric):
    rows = _device(_rows(300))
    counts = [100, 1, 199]
    values, indices = _topk(rows[:130], rows, k=8, metric=metric, distinct_records=counts)
    assert np.all(indices[:, :3] >= 0) and np.all(indices[:, 3:] == -1)
    assert np.all(values[:, 3:] == _empty(metric)) and np.all(np.isfinite(values[:, :3]))
    assert np.array_equal(np.sort(_record_of(indices[:, :3], np.array([0, 100, 101, 300])), axis=1),
                          np.tile(np.arange(3), (130, 1)))
    values, indices = _topk(rows, k=8, metric=metric, exclude_records=counts,
                            distinct_records=counts)
    assert np.all(indices[:, :2] >= 0) and np.all(indices[:, 2:] == -1)
    assert np.all(values[:, 2:] == _empty(metric)) and np.all(np.isfinite(values[:, :2]))


# 7. prefix and block independence

@pytest.mark.parametrize("metric", METRICS)
def test_prefix_and_row_block_independence(gpu, metric):
    n = 8_269
    rows, counts, ptr, _, whole = _self_search(n, metric)
    device = _device(rows)
    for j in (1, 3, 8):
        part = _topk(device, k=j, metric=metric, exclude_records=counts, distinct_records=counts)
        assert _same(part, (whole[0][:, :j], whole[1][:, :j])), j
    own = _record_of(np.arange(n), ptr)
    for start, stop in ((1_000, 1_300), (8_100, n)):
        skip = (ptr[own[start:stop]].astype(np.int32), ptr[own[start:stop] + 1].astype(np.int32))
        block = _topk(device[start:stop], device, k=KMAX, metric=metric, exclude_ranges=skip,
                      distinct_records=counts)
        assert _same(block, (whole[0][start:stop], whole[1][start:stop])), start


# 8. no rows; a kept workspace

def test_no_rows_and_workspace_reuse(gpu):
    from ginfinity_amd import distance
    rows = _device(_rows(700))
    counts, _ = _records(700)
    values, indices = distance.topk(rows[:0], rows, k=5, distinct_records=counts)
    assert values.shape == (0, 5) and indices.shape == (0, 5)
    keep = distance.TopKWorkspace()
    for n, k in ((700, 8), (300, 3)):
        sizes, _ = _records(n)
        fresh = _topk(rows[:n], k=k, exclude_records=sizes, distinct_records=sizes)
        kept = _topk(rows[:n], k=k, exclude_records=sizes, distinct_records=sizes, workspace=keep)
        assert _same(fresh, kept), (n, k)
