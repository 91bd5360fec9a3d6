"""Top-k search that skips a half-open range of b-rows per a-row (gfy_pairwise_topk_ranges;
distance.topk / nearest with exclude_ranges / exclude_records; csrc/pairwise_topk.inc, kRanges)
against the float64 definition (oracle.gine_numpy.pairwise_l2 / pairwise_cosine with the excluded
columns set to the value that never wins) and, where a range is a single row, against the
single-pair modes bit for bit.

The comparison with the oracle is rank-wise, as in tests/test_gpu_distance_topk.py: the oracle
value at the returned index is within tolerance of the r-th entry of the oracle's sorted row, the
returned value is within tolerance of the oracle value at the returned index, indices are
distinct, inside [0, m) and outside the row's range, values are monotone along a row.
Tolerances are those of tests/test_gpu_distance_sweeps.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_sweeps.py
L2_TOL = 2e-5            # on an L2 distance d >= 0.1
D2_TOL = 4e-6            # on d², times (|a_i|² + |b_j|²)
BLOCK_A = 128            # a-rows per workgroup, b-rows per tile (pairwise_topk.inc)
RECORD_SIZES = (1, 2, 37, 100, 128, 129, 300)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


# --------------------------------------------------------------------------------------------
# inputs and the oracle comparison

@functools.lru_cache(maxsize=None)
def _pool(seed, rows):
    from ginfinity_amd import synthetic
    data = synthetic.unit_rows(seed, rows)
    data.setflags(write=False)
    return data


def _a_rows(n):
    return _pool(101, 20_480)[:n].copy()


def _b_rows(m):
    return _pool(202, 20_480)[:m].copy()


def _mixed_rows(seed, count, unit):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((count, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    if not unit:
        data *= rng.uniform(0.2, 3.0, size=(count, 1))
    return data.astype(np.float16)


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def _pair(lo, hi):
    return (np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32))


def _topk(a, b, **arguments):
    from ginfinity_amd import distance
    values, indices = distance.topk(a, b, **arguments)
    return values.cpu().numpy(), indices.cpu().numpy()


def _same(one, two):
    return (np.ascontiguousarray(one[0]).tobytes() == np.ascontiguousarray(two[0]).tobytes()
            and np.ascontiguousarray(one[1]).tobytes() == np.ascontiguousarray(two[1]).tobytes())


def _records(n, lead=()):
    """Record sizes: ``lead``, then RECORD_SIZES over and over until n rows are used up (the
    last record cut short).  Returns (counts, lo, hi) with lo / hi the int64 range of every row."""
    counts, at = list(lead), 0
    while sum(counts) < n:
        counts.append(min(RECORD_SIZES[at % len(RECORD_SIZES)], n - sum(counts)))
        at += 1
    ptr = np.concatenate(([0], np.cumsum(counts)))
    assert ptr[-1] == n
    return counts, np.repeat(ptr[:-1], counts), np.repeat(ptr[1:], counts)


def _masked_oracle(a_block, b, metric, lo, hi):
    """float64 [rows][m], the columns lo <= j < hi of every row set to the value that never wins."""
    from oracle import gine_numpy as G
    full = G.pairwise_l2(a_block, b) if metric == "l2" else G.pairwise_cosine(a_block, b)
    columns = np.arange(b.shape[0])[None, :]
    full[(columns >= lo[:, None]) & (columns < hi[:, None])] = np.inf if metric == "l2" else -np.inf
    return full


def _against_oracle(a, b, rows, values, indices, metric, lo, hi):
    """``values`` / ``indices`` [n][k] of the a-rows ``rows``, rank-wise against the float64
    definition (module docstring).  ``lo`` / ``hi`` int64 [n].  Every checked row must have at
    least k candidates.  Returns the worst deviation seen (cosine: absolute; l2: of d² relative
    to |a|² + |b|²)."""
    m, k = b.shape[0], values.shape[1]
    worst = 0.0
    for start in range(0, rows.size, 512):
        block = rows[start:start + 512]
        count = np.arange(block.size)
        idx = indices[block]
        got = values[block].astype(np.float64)
        assert idx.min() >= 0 and idx.max() < m
        ordered = np.sort(idx, axis=1)
        assert np.all(ordered[:, 1:] != ordered[:, :-1]), "an index twice in a row"
        assert not np.any((idx >= lo[block][:, None]) & (idx < hi[block][:, None])), \
            "an index inside the row's excluded range"
        assert np.all(got[:, 1:] >= got[:, :-1]) if metric == "l2" else np.all(got[:, 1:] <= got[:, :-1])
        full = _masked_oracle(a[block], b, metric, lo[block], hi[block])
        picked = full[count[:, None], idx]                      # before the partition reorders
        if metric == "cosine":
            full *= -1.0
        full.partition(k - 1, axis=1)
        best = np.sort(full[:, :k], axis=1)
        if metric == "cosine":
            best = -best
        assert np.all(np.isfinite(best)), "a checked row with fewer than k candidates"
        if metric == "cosine":
            assert np.abs(picked - best).max() <= COSINE_TOL
            assert np.abs(got - picked).max() <= COSINE_TOL
            worst = max(worst, float(np.abs(got - best).max()))
        else:
            scale = ((a[block].astype(np.float64) ** 2).sum(1)[:, None]
                     + (b[idx.ravel()].astype(np.float64) ** 2).sum(1).reshape(idx.shape))
            assert np.all(np.abs(picked ** 2 - best ** 2) <= D2_TOL * scale)
            assert np.all(np.abs(got ** 2 - picked ** 2) <= D2_TOL * scale)
            far = best >= 0.1
            assert np.all(np.abs(picked - best)[far] <= L2_TOL)
            assert np.all(np.abs(got - picked)[far] <= L2_TOL)
            worst = max(worst, float((np.abs(got ** 2 - best ** 2) / scale).max()))
    return worst


def _align(size):
    return (size + 255) // 256 * 256


def _sweep(lib, n, m, k=8):
    """(chunks, tiles per workgroup, tiles of the last chunk) of topk(n, m), recovered from the
    workspace size: carve_topk() lays out s and t (tiles_b * 128 floats each), a_term (n floats)
    and the two [chunks][n][k] partial arrays, each rounded up to 256 bytes."""
    tiles_b = (m + 127) // 128
    partial, odd = divmod(lib.gfy_pairwise_topk_workspace_bytes(n, m, k)
                          - 2 * _align(tiles_b * 128 * 4) - _align(n * 4), 2)
    assert odd == 0 and n * k * 4 >= 256
    fits = [c for c in range(1, tiles_b + 1) if _align(c * n * k * 4) == partial]
    assert len(fits) == 1, (n, m, fits)
    chunks = fits[0]
    per = -(-tiles_b // chunks)
    return chunks, per, tiles_b - (chunks - 1) * per


#: n = m whose workgroups sweep 4 tiles (the last chunk 1) and 5 tiles (the last chunk 4), both
#: with a ragged last tile — what carve_topk() chooses today, asserted where they are used
MULTI_TILE = (8_269, 10_000)


# --------------------------------------------------------------------------------------------
# 1. a range of one row is the single-pair mode, bit for bit

@pytest.mark.parametrize("n,m", [(257, 385), (513, 640), (8_000, 8_269)])
def test_single_row_ranges_are_the_single_pair_modes_bit_for_bit(gpu, n, m):
    """Rows as slices of one pool.  Empty ranges == the plain call; lo = i + off, hi = lo + 1 ==
    exclude_offset = off; lo = i - first, hi = lo + 1 == window_first = first (a is the longer
    side there); values and indices, k = 1, 5, 16, both metrics; nearest(exclude_ranges=...) is
    column 0."""
    from ginfinity_amd import distance
    if m > 1_000:
        assert _sweep(gpu, n, m)[1] >= 4 and _sweep(gpu, m, n)[1] >= 4      # multi-tile sweeps
    assert n <= m
    both = _a_rows(m)
    offset, first = min(129, m - n), min(77, m - n)
    cases = [(_a_rows(n), _b_rows(m), {}, np.zeros(n), np.zeros(n)),
             (both[offset:offset + n], both[:m], {"exclude_offset": offset},
              np.arange(n) + offset, np.arange(n) + offset + 1),
             (both[:n], both[:n], {"exclude_self": True}, np.arange(n), np.arange(n) + 1),
             (both[:m], both[first:first + n], {"window_first": first},
              np.arange(m) - first, np.arange(m) - first + 1)]
    for a, b, arguments, lo, hi in cases:
        device_a, device_b = _device(a), _device(b)
        ranges = _pair(lo, hi)
        for metric in ("l2", "cosine"):
            for k in (1, 5, 16):
                want = _topk(device_a, device_b, k=k, metric=metric, **arguments)
                got = _topk(device_a, device_b, k=k, metric=metric, exclude_ranges=ranges)
                assert _same(want, got), (arguments, metric, k)
            near_values, near_indices = distance.nearest(device_a, device_b, metric=metric,
                                                         exclude_ranges=ranges)
            assert near_values.shape == (a.shape[0],) and near_indices.dtype == torch.int32
            assert _same((near_values.cpu().numpy(), near_indices.cpu().numpy()),
                         (got[0][:, 0], got[1][:, 0]))
            was = distance.nearest(device_a, device_b, metric=metric, **arguments)
            assert _same((near_values.cpu().numpy(), near_indices.cpu().numpy()),
                         (was[0].cpu().numpy(), was[1].cpu().numpy()))


# --------------------------------------------------------------------------------------------
# 2. self-search with records, every row

@pytest.mark.parametrize("n", [300, 1_000])
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_row_against_the_oracle_with_records(gpu, metric, unit, n):
    counts, lo, hi = _records(n)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    inner = [(s, e) for s, e in zip(ptr[:-1], ptr[1:]) if s // BLOCK_A != (e - 1) // BLOCK_A]
    assert inner, "no record straddles a 128-row seam"
    if n == 1_000:      # one record covers a whole tile and more
        assert any(s <= t * BLOCK_A and (t + 1) * BLOCK_A <= e for s, e in inner for t in range(8))
        assert set(RECORD_SIZES) <= set(counts)
    rows = _mixed_rows(7 * n, n, unit)
    device_rows = _device(rows)
    for k in (1, 8, 16):
        values, indices = _topk(device_rows, None, k=k, metric=metric, exclude_records=counts)
        assert values.shape == (n, k) and indices.dtype == np.int32
        worst = _against_oracle(rows, rows, np.arange(n), values, indices, metric, lo, hi)
        again = _topk(device_rows, device_rows, k=k, metric=metric, exclude_ranges=_pair(lo, hi))
        assert _same((values, indices), again)
        print(f"records({n}, k={k}) {metric} unit={unit}: worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 3. multi-tile sweeps

@functools.lru_cache(maxsize=None)
def _multi_tile_case(n):
    """(rows, counts, lo, hi, sample): a 700-row record first (more than a chunk of either shape:
    its range crosses a chunk boundary and two ring pairs), the sample holds both sides of every
    record boundary and of every block seam under the big record, and 1,000 random rows."""
    counts, lo, hi = _records(n, lead=(5, 700))
    ptr = np.concatenate(([0], np.cumsum(counts)))
    rng = np.random.default_rng(n)
    edges = ptr[1:-1]
    seams = BLOCK_A * np.arange(1, n // BLOCK_A + 1)
    seams = seams[seams < n]
    sample = np.unique(np.concatenate([edges - 1, edges, seams - 1, seams, [0, n - 1],
                                       rng.integers(0, n, 1_000)]))
    return _a_rows(n), counts, lo, hi, sample


def test_multi_tile_geometry_is_what_the_tests_assume(gpu):
    lengths = set()
    for n in MULTI_TILE:
        chunks, per, last = _sweep(gpu, n, n)
        print(f"topk({n}, {n}): {chunks} chunks of {per} tiles, the last of {last}")
        assert chunks > 1 and n % BLOCK_A != 0 and n <= 20_000
        assert 700 > per * BLOCK_A - 5                      # the big record leaves its chunk
        lengths |= {per, last}
    assert any(length >= 4 and length % 2 == 0 for length in lengths)
    assert any(length >= 3 and length % 2 == 1 for length in lengths)


@pytest.mark.parametrize("n", MULTI_TILE)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_multi_tile_sweeps_with_records_against_the_oracle(gpu, metric, n):
    assert _sweep(gpu, n, n)[1] >= 4
    rows, counts, lo, hi, sample = _multi_tile_case(n)
    device_rows = _device(rows)
    for k in (8, 16):
        values, indices = _topk(device_rows, None, k=k, metric=metric, exclude_records=counts)
        assert indices.min() >= 0 and indices.max() < n
        assert not np.any((indices >= lo[:, None]) & (indices < hi[:, None]))
        worst = _against_oracle(rows, rows, sample, values, indices, metric, lo, hi)
        print(f"records({n}, k={k}) {metric}: {sample.size} rows, worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 4. the excluded range hides the true nearest

PLANT_K = 16


def _planted_copies(row, rng):
    """16 copies of ``row`` at distances 0.10, 0.12, ... 0.40 (before fp16 rounding)."""
    out = np.empty((PLANT_K, 128), dtype=np.float16)
    for j in range(PLANT_K):
        direction = rng.standard_normal(128)
        direction -= direction.dot(row) / row.dot(row) * row
        direction /= np.linalg.norm(direction)
        out[j] = (row + (0.10 + 0.02 * j) * direction).astype(np.float16)
    return out


@pytest.mark.parametrize("n", [1_000, 8_269])
def test_planted_neighbours_inside_the_record_are_hidden(gpu, n):
    """For 24 rows 16 perturbed copies, the farther the later: the even ones inside the row's
    own record, the odd ones outside every chosen record.  The row itself and the eight inside
    copies are nearer than anything returned; the list is exactly the eight outside ones in
    planted order, and the ninth column lies outside the record too."""
    rng = np.random.default_rng(n)
    rows = _a_rows(n)
    counts, lo, hi = _records(n)
    ptr = np.concatenate(([0], np.cumsum(counts)))
    roomy = [q for q, count in enumerate(counts) if count >= 100][:3]    # 100, 128, 129 rows
    assert len(roomy) == 3
    chosen, inside = [], []
    taken = np.zeros(n, dtype=bool)
    for slot in range(24):                      # 8 rows in each of the three records, 9 rows each
        q = roomy[slot % len(roomy)]
        free = np.nonzero(~taken[ptr[q]:ptr[q + 1]])[0] + ptr[q]
        assert free.size >= 9
        picked = rng.permutation(free)[:9]
        taken[picked] = True
        chosen.append(picked[0])
        inside.append(picked[1:])
    chosen, inside = np.array(chosen), np.array(inside)
    in_chosen_record = np.zeros(n, dtype=bool)
    for q in roomy:
        in_chosen_record[ptr[q]:ptr[q + 1]] = True
    outside = rng.permutation(np.nonzero(~in_chosen_record)[0])[:24 * 8].reshape(24, 8)
    assert outside.size == 24 * 8
    for row, near, far in zip(chosen, inside, outside):
        copies = _planted_copies(rows[row].astype(np.float64), rng)
        rows[near] = copies[0::2]
        rows[far] = copies[1::2]
    assert np.all((inside >= lo[chosen][:, None]) & (inside < hi[chosen][:, None]))
    assert not np.any((outside >= lo[chosen][:, None]) & (outside < hi[chosen][:, None]))
    for metric in ("l2", "cosine"):             # the oracle agrees with the construction
        plain = _masked_oracle(rows[chosen], rows, metric, np.zeros(24), np.zeros(24))
        order = np.argsort(plain if metric == "l2" else -plain, axis=1, kind="stable")
        assert all(set(order[i, :9]) == {chosen[i], *inside[i, :4], *outside[i, :4]}
                   for i in range(24))
        full = _masked_oracle(rows[chosen], rows, metric, lo[chosen], hi[chosen])
        order = np.argsort(full if metric == "l2" else -full, axis=1, kind="stable")[:, :9]
        assert np.array_equal(order[:, :8], outside), metric
        top = np.take_along_axis(full, order, axis=1)
        gaps = np.abs(np.diff(top, axis=1))
        assert np.all(gaps >= 100 * (L2_TOL if metric == "l2" else COSINE_TOL))
    device_rows = _device(rows)
    for metric in ("l2", "cosine"):
        for k in (8, 3, 1):
            _, indices = _topk(device_rows, None, k=k, metric=metric, exclude_records=counts)
            np.testing.assert_array_equal(indices[chosen], outside[:, :k])
        _, indices = _topk(device_rows, None, k=9, metric=metric, exclude_records=counts)
        np.testing.assert_array_equal(indices[chosen, :8], outside)
        ninth = indices[chosen, 8]
        assert not np.any((ninth >= lo[chosen]) & (ninth < hi[chosen]))
        _, plain = _topk(device_rows, None, k=1, metric=metric, exclude_self=True)
        np.testing.assert_array_equal(plain[chosen, 0], inside[:, 0])     # what the range hides


# --------------------------------------------------------------------------------------------
# 5. arbitrary ranges, b != a

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_arbitrary_ranges_against_the_oracle(gpu, metric):
    """Row i skips [(i % 7) * 400, (i % 7) * 400 + 50 * (i % 5)): neighbouring rows of one block
    disagree, every fifth range is empty.  Further rows carry lo < 0, hi > m, lo > hi, the int32
    extremes, and ranges that cover all of b: those return -1 and +-inf in every column."""
    n, m = 300, 3_000
    a, b = _mixed_rows(11, n, False), _mixed_rows(13, m, False)
    i = np.arange(n)
    lo = (i % 7) * 400
    hi = lo + 50 * (i % 5)
    special = {10: (-5, 40), 11: (2_990, m + 100), 12: (500, 100), 140: (-2 ** 31, 17),
               141: (2_900, 2 ** 31 - 1), 142: (2 ** 31 - 1, -2 ** 31), 143: (m, m + 5),
               144: (-9, 0), 13: (-7, m + 7), 150: (0, m), 299: (-2 ** 31, 2 ** 31 - 1)}
    for row, (low, high) in special.items():
        lo[row], hi[row] = low, high
    everything = np.array([13, 150, 299])
    others = np.setdiff1d(i, everything)
    assert np.any(lo >= hi) and np.any(hi - lo == 200)
    nothing = np.inf if metric == "l2" else -np.inf
    device_a, device_b = _device(a), _device(b)
    for k in (16, 5, 1):
        values, indices = _topk(device_a, device_b, k=k, metric=metric, exclude_ranges=_pair(lo, hi))
        assert np.all(indices[everything] == -1) and np.all(values[everything] == nothing)
        worst = _against_oracle(a, b, others, values, indices, metric, lo, hi)
        print(f"arbitrary ranges k={k} {metric}: worst {worst:.2e}")
    # rows without a range are the rows of the plain call, bit for bit
    free = np.nonzero(lo >= hi)[0]
    plain = _topk(device_a, device_b, k=16, metric=metric)
    ranged = _topk(device_a, device_b, k=16, metric=metric, exclude_ranges=_pair(lo, hi))
    assert _same((ranged[0][free], ranged[1][free]), (plain[0][free], plain[1][free]))
    # torch bounds on the device are taken as they are
    on_device = tuple(torch.from_numpy(bound).cuda() for bound in _pair(lo, hi))
    assert _same(ranged, _topk(device_a, device_b, k=16, metric=metric, exclude_ranges=on_device))


# --------------------------------------------------------------------------------------------
# 6. fewer than k candidates

@pytest.mark.parametrize("n", [300, 700])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_fewer_candidates_than_k(gpu, metric, n):
    """One record holds all rows but 3: its rows return the 3 others and then -1 / +-inf; the 3
    others (records of 2 and 1 rows) have n - 2 and n - 1 candidates."""
    from ginfinity_amd import distance
    counts = [2, n - 3, 1]
    lo, hi = (bound.numpy().astype(np.int64) for bound in distance.record_ranges(counts))
    rows = _a_rows(n)
    big, small = np.arange(2, n - 1), np.array([0, 1, n - 1])
    nothing = np.inf if metric == "l2" else -np.inf
    device_rows = _device(rows)
    for k in (16, 4, 3, 2):
        values, indices = _topk(device_rows, None, k=k, metric=metric, exclude_records=counts)
        have = min(k, 3)
        assert np.all(indices[big, have:] == -1) and np.all(values[big, have:] == nothing)
        assert np.all(np.isin(indices[big, :have], small))
        _against_oracle(rows, rows, big, values[:, :have], indices[:, :have], metric, lo, hi)
        _against_oracle(rows, rows, small, values, indices, metric, lo, hi)
    values, indices = distance.nearest(device_rows, metric=metric, exclude_records=[n])
    assert torch.all(indices == -1) and torch.all(values == nothing) and values.shape == (n,)


# --------------------------------------------------------------------------------------------
# 7. prefix and block independence

@pytest.mark.parametrize("n", [1_000, 8_269])
def test_prefix_and_block_independence(gpu, n):
    """k = 4 is the prefix of k = 16; the rows [s, e) searched alone (s no multiple of 128: other
    lanes, waves, workgroups and chunks) give the same bytes; the ranges of the rows outside
    [s, e) do not matter inside."""
    from ginfinity_amd import distance
    rows = _a_rows(n)
    counts, lo, hi = _records(n, lead=(5, 700))
    device_rows = _device(rows)
    start, stop = 77, n - 301
    assert start % BLOCK_A != 0 and (stop - start) % BLOCK_A != 0
    rng = np.random.default_rng(n)
    other_lo, other_hi = lo.copy(), hi.copy()
    outside = np.concatenate([np.arange(start), np.arange(stop, n)])
    other_lo[outside] = rng.integers(-100, n, outside.size)
    other_hi[outside] = other_lo[outside] + rng.integers(-50, 900, outside.size)
    workspace = distance.TopKWorkspace()
    for metric in ("l2", "cosine"):
        full = _topk(device_rows, None, k=16, metric=metric, exclude_ranges=_pair(lo, hi))
        short = _topk(device_rows, None, k=4, metric=metric, exclude_ranges=_pair(lo, hi))
        assert _same(short, (full[0][:, :4], full[1][:, :4]))
        part = _topk(device_rows[start:stop], device_rows, k=16, metric=metric,
                     exclude_ranges=_pair(lo[start:stop], hi[start:stop]))
        assert _same(part, (full[0][start:stop], full[1][start:stop]))
        other = _topk(device_rows, None, k=16, metric=metric,
                      exclude_ranges=_pair(other_lo, other_hi), workspace=workspace)
        assert _same((other[0][start:stop], other[1][start:stop]), part)
        assert not _same(other, full)


def test_no_rows_give_empty_results(gpu):
    empty = torch.zeros((0, 128), dtype=torch.float16, device="cuda")
    values, indices = _topk(empty, None, k=5, exclude_records=[])
    assert values.shape == (0, 5) and indices.shape == (0, 5)
    nobody = np.zeros(0, dtype=np.int32)
    values, indices = _topk(empty, _device(_b_rows(10)), k=5, exclude_ranges=(nobody, nobody))
    assert values.shape == (0, 5) and indices.shape == (0, 5)


# --------------------------------------------------------------------------------------------
# 8. real embeddings

def test_real_embeddings_top8_outside_the_own_record(gpu, gpu_encoder, rouskin_shard):
    from ginfinity_amd import distance
    block, counts = gpu_encoder.encode_graphs_device(rouskin_shard.slice(0, 40))
    assert block.shape[0] == sum(counts) and block.shape[0] >= 512
    host = block.cpu().numpy()
    lo, hi = (bound.numpy().astype(np.int64) for bound in distance.record_ranges(counts))
    for metric in ("cosine", "l2"):
        values, indices = _topk(block, None, k=8, metric=metric, exclude_records=counts)
        assert not np.any((indices >= lo[:, None]) & (indices < hi[:, None]))
        worst = _against_oracle(host, host, np.arange(512), values, indices, metric, lo, hi)
        print(f"real embeddings ({host.shape[0]} rows, {len(counts)} records) {metric}: "
              f"worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 9. cross-shard, world size 1

def test_cross_shard_topk_with_records_world_size_one(gpu):
    """No process group: the values are those of distance.topk(exclude_records=...) bit for bit
    and every row holds the same rows, whatever the chunking (records are cut by the chunks).
    The ORDER of the rows is not compared: the merge orders by value and the kernel by key
    (parallel.cross_shard_topk states the caveat)."""
    from ginfinity_amd import distance, parallel
    n = 1_200
    block = _device(_a_rows(n))
    counts, _, _ = _records(n)
    for metric in ("l2", "cosine"):
        want_values, want_indices = distance.topk(block, k=8, metric=metric, exclude_records=counts)
        want_values = want_values.clone()
        want_rows = torch.sort(want_indices.to(torch.int64), dim=1).values
        for chunk_rows in (1 << 20, 1_000, 257):
            values, indices, offsets = parallel.cross_shard_topk(
                block, 8, metric=metric, chunk_rows=chunk_rows, record_counts=counts)
            assert offsets == [0, n] and indices.dtype == torch.int64
            assert torch.equal(values.view(torch.int32), want_values.view(torch.int32))
            assert torch.equal(torch.sort(indices, dim=1).values, want_rows)
