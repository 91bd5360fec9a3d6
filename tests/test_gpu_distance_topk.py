"""Exact top-k nearest-row search (csrc/pairwise_topk.hip, distance.topk) against the float64
definition (oracle.gine_numpy.pairwise_l2 / pairwise_cosine; the top-k oracle is their stable
argsort, written here) and against the nearest-row kernel, whose answer column 0 has to be bit
for bit.  The reference has no implementation of this step: parity is unpinned.

The comparison with the oracle is rank-wise, so that two neighbours closer than the tolerance
may swap: the oracle value at the returned index is within tolerance of the r-th entry of the
oracle's sorted row, the returned value is within tolerance of the oracle value at the returned
index, indices are distinct and inside [0, m), values are monotone along a row.  Tolerances are
those of tests/test_gpu_distance_sweeps.py.

A workgroup of the top-k kernel owns 128 a-rows and sweeps more than one 128-row b-tile only when
(n / 128) * (m / 128) exceeds about 1,024 (carve_topk() in pairwise_topk.hip), so the multi-tile
tests take their shapes from SWEEPS, whose sweep lengths
``test_sweep_geometry_is_what_the_tests_assume`` asserts."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_sweeps.py
L2_TOL = 2e-5            # on an L2 distance d >= 0.1
D2_TOL = 4e-6            # on d², times (|a_i|² + |b_j|²)
BLOCK_A = 128            # a-rows per workgroup (pairwise_topk.hip)
RING = 4                 # b-tile buffers of its ring


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
    return _pool(101, 262_400)[:n].copy()


def _b_rows(m):
    return _pool(202, 66_560)[:m].copy()


def _mixed_rows(seed, count, unit):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((count, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    if not unit:
        data *= rng.uniform(0.2, 3.0, size=(count, 1))
    return data.astype(np.float16)


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def _topk(a, b, **arguments):
    from ginfinity_amd import distance
    values, indices = distance.topk(a, b, **arguments)
    return values.cpu().numpy(), indices.cpu().numpy()


def _nearest(a, b, **arguments):
    from ginfinity_amd import distance
    values, indices = distance.nearest(a, b, **arguments)
    return values.cpu().numpy(), indices.cpu().numpy()


def _oracle_block(a_block, b, metric, gone=None):
    """float64 [rows][m] with the excluded column of every row (``gone``, where it is a row of
    b) set to the value that never wins."""
    from oracle import gine_numpy as G
    full = G.pairwise_l2(a_block, b) if metric == "l2" else G.pairwise_cosine(a_block, b)
    if gone is not None:
        has = (gone >= 0) & (gone < b.shape[0])
        full[np.nonzero(has)[0], gone[has]] = np.inf if metric == "l2" else -np.inf
    return full


def _against_oracle(a, b, rows, values, indices, metric, excluded=None):
    """``values`` / ``indices`` [n][k] of the a-rows ``rows``, rank-wise against the float64
    definition (module docstring).  Every checked row must have at least k candidates.  Returns
    the worst deviation seen (cosine: absolute; l2: of d² relative to |a|² + |b|²)."""
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
        if excluded is not None:
            assert not np.any(idx == excluded[block][:, None])
        assert np.all(got[:, 1:] >= got[:, :-1]) if metric == "l2" else np.all(got[:, 1:] <= got[:, :-1])
        full = _oracle_block(a[block], b, metric, None if excluded is None else excluded[block])
        picked = full[count[:, None], idx]                      # before the partition reorders
        if metric == "cosine":
            full *= -1.0
        full.partition(k - 1, axis=1)                               # in place: 512 x 1M is 4 GB
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


def _sample(n, seed, extra=()):
    """Both sides of 64 workgroup seams, the first and the last 300 rows, 1,400 random rows."""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.arange(1, n // BLOCK_A), size=64, replace=False)
    rows = np.unique(np.concatenate([
        BLOCK_A * blocks - 1, BLOCK_A * blocks, np.arange(300), np.arange(n - 300, n),
        rng.integers(0, n, 1_400), np.asarray(extra, dtype=np.int64)]))
    assert np.isin(BLOCK_A * blocks - 1, rows).all() and np.isin(BLOCK_A * blocks, rows).all()
    return rows


# --------------------------------------------------------------------------------------------
# 1. small and seam shapes, every row

SMALL = ((1, 1), (130, 257), (300, 500), (1_000, 3_000), (64, 20_000), (129, 127), (255, 129),
         (257, 385), (513, 640), (770, 1))
KS = (1, 2, 3, 5, 8, 16)


@pytest.mark.parametrize("n,m", SMALL)
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_row_against_the_oracle_small_and_seam_shapes(gpu, metric, unit, n, m):
    """All rows, k = 1, 2, 3, 5, 8, 16.  Where m < k the leading min(k, m) columns are checked
    rank-wise and the trailing ones are exactly -1 / +-inf."""
    a, b = _mixed_rows(3 * n + m, n, unit), _mixed_rows(5 * m + n, m, unit)
    device_a, device_b = _device(a), _device(b)
    nothing = np.inf if metric == "l2" else -np.inf
    for k in KS:
        values, indices = _topk(device_a, device_b, k=k, metric=metric)
        assert values.shape == (n, k) and indices.shape == (n, k)
        assert values.dtype == np.float32 and indices.dtype == np.int32
        have = min(k, m)
        assert np.all(indices[:, have:] == -1) and np.all(values[:, have:] == nothing)
        worst = _against_oracle(a, b, np.arange(n), values[:, :have], indices[:, :have], metric)
        print(f"topk({n}, {m}, k={k}) {metric} unit={unit}: worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 2. fewer candidates than k

@pytest.mark.parametrize("m", [1, 3, 15])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_fewer_candidates_than_k(gpu, metric, m):
    """k = 16 against m = 1, 3, 15 rows: plain (m candidates), with exclude_offset and with
    window_first (m - 1 candidates for the rows that have a partner in b).  The trailing slots
    are exactly -1 / +-inf, the leading ones are the oracle's."""
    n, k = 700, 16
    nothing = np.inf if metric == "l2" else -np.inf
    a = _a_rows(n)
    device_a = _device(a)
    for first in (0, 5, 300):
        b = a[first:first + m]
        cases = (({}, None),
                 ({"exclude_offset": 0}, np.arange(n)),                  # pair (i, i)
                 ({"window_first": first}, np.arange(n) - first))         # pair (first + j, j)
        for arguments, excluded in cases:
            values, indices = _topk(device_a, _device(b), k=k, metric=metric, **arguments)
            candidates = np.full(n, m)
            if excluded is not None:
                candidates -= (excluded >= 0) & (excluded < m)
            for count in np.unique(candidates):
                rows = np.nonzero(candidates == count)[0]
                assert np.all(indices[rows, count:] == -1), (m, first, arguments, count)
                assert np.all(values[rows, count:] == nothing)
                if count:
                    _against_oracle(a, b, rows, values[:, :count], indices[:, :count], metric,
                                    excluded)
            assert candidates.min() == (m - 1 if excluded is not None else m)


# --------------------------------------------------------------------------------------------
# 3. sweep geometry

#: (n, m, chunks, tiles per workgroup, tiles of the last chunk) — what carve_topk() chooses today.
#: A retune of its heuristic fails test_sweep_geometry_is_what_the_tests_assume and has to bring
#: new shapes: nothing below may fall back to one tile per workgroup unnoticed.
SWEEPS = (
    (65_536, 256, 2, 1, 1),
    (65_536, 512, 2, 2, 2),
    (65_536, 641, 2, 3, 3),            # 128 * 5 + 1
    (65_536, 1_024, 2, 4, 4),
    (65_536, 1_153, 2, 5, 5),          # 128 * 9 + 1
    (65_536, 1_536, 2, 6, 6),
    (65_536, 1_700, 2, 7, 7),
    (65_536, 1_920, 2, 8, 7),
    (65_536, 2_304, 2, 9, 9),
    (65_536, 4_607, 2, 18, 18),        # 128 * 35 + 127
    (70_000, 2_560, 7, 3, 2),
    (262_400, 4_096, 5, 7, 4),
    # a is a block of b (section 5): m >= n, long sweeps
    (65_536, 65_536, 2, 256, 256),
    (65_536, 65_663, 2, 257, 256),     # 127 + n
    (65_536, 65_805, 2, 258, 257),
)
GEOMETRY = {(n, m): (chunks, per, last) for n, m, chunks, per, last in SWEEPS}


def _align(size):
    return (size + 255) // 256 * 256


def _sweep(lib, n, m, k=8):
    """(chunks, tiles per workgroup, tiles of the last chunk) of topk(n, m), recovered from the
    workspace size: carve_topk() lays out s and t (tiles_b * 128 floats each), a_term (n floats)
    and the two [chunks][n][k] partial arrays, each rounded up to 256 bytes.  The chunk count does
    not depend on k."""
    tiles_b = (m + 127) // 128
    partial, odd = divmod(lib.gfy_pairwise_topk_workspace_bytes(n, m, k)
                          - 2 * _align(tiles_b * 128 * 4) - _align(n * 4), 2)
    assert odd == 0 and n * k * 4 >= 256
    fits = [c for c in range(1, tiles_b + 1) if _align(c * n * k * 4) == partial]
    assert len(fits) == 1, (n, m, fits)
    chunks = fits[0]
    per = -(-tiles_b // chunks)
    return chunks, per, tiles_b - (chunks - 1) * per


def test_sweep_geometry_is_what_the_tests_assume(gpu):
    reached, short_last, odd_tail = set(), False, False
    for n, m, *want in SWEEPS:
        chunks, per, last = _sweep(gpu, n, m)
        assert (chunks, per, last) == _sweep(gpu, n, m, k=16) == _sweep(gpu, n, m, k=1)
        print(f"topk({n}, {m}): {chunks} chunks of {per} tiles, the last of {last}")
        assert (chunks, per, last) == tuple(want), (n, m)
        assert 1 <= last <= per and (chunks - 1) * per + last == (m + 127) // 128
        assert chunks > 1                                   # more than one chunk, everywhere
        reached |= {per, last}
        short_last |= last < per
        odd_tail |= per % 2 == 1 and per > 1                # two tiles per barrier, then one
    print("sweep lengths reached:", sorted(reached))
    assert set(range(1, 10)) <= reached                     # 1 through 9 tiles
    assert any(length >= RING + 2 for length in reached)    # past the ring depth plus one
    assert max(reached) >= 16
    assert short_last and odd_tail
    assert len({n for n, *_ in SWEEPS}) >= 3


@pytest.mark.parametrize("n,m", [(n, m) for n, m, *_ in SWEEPS if m <= 4_607])
def test_multi_tile_sweeps_against_the_oracle(gpu, n, m):
    """Every sweep length of SWEEPS, ragged ends included: every 7th a-row is b[m - 1] (whose
    padding rows re-read it with a term that never wins), k = 8 and 16."""
    assert GEOMETRY[(n, m)] == _sweep(gpu, n, m)
    a, b = _a_rows(n), _b_rows(m)
    at_end = np.arange(n) % 7 == 0
    a[at_end] = b[m - 1]
    device_a, device_b = _device(a), _device(b)
    rows = _sample(n, seed=m)[::3]
    for metric in ("l2", "cosine"):
        for k in (8, 16):
            values, indices = _topk(device_a, device_b, k=k, metric=metric)
            assert indices.min() >= 0 and indices.max() < m
            assert np.all(indices[at_end, 0] == m - 1)
            worst = _against_oracle(a, b, rows, values, indices, metric)
            print(f"topk({n}, {m}, k={k}) {metric}: {rows.size} rows, worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 4. exact ties at every merge level

#: copies of one row, as distances from its first copy.  With the first copy on a row 8 q of a
#: tile: 1-3 are further registers of the same lane (and 8, 16, 24: its other register groups),
#: 4 and 5 the other lane half of the same wave, 32 / 64 / 96 the other three waves; 128 is the
#: next tile (the second of a pair when the first copy is in an even tile of the sweep, the next
#: pair otherwise), 256 two tiles on, 512 the same ring buffer again; FAR (added per shape) lands
#: 37 rows into the tile one whole sweep later: another chunk.
TIE_OFFSETS = (0, 1, 2, 3, 4, 5, 8, 16, 24, 32, 64, 96, 128, 132, 256, 512, 516)
TIE_SHAPES = ((65_536, 4_607), (65_536, 2_304), (70_000, 2_560), (262_400, 4_096))


def _lane(position):
    """(tile, wave of the tile's four b-waves, lane half) that holds b-row ``position``."""
    inside = position % 128
    return position // 128, inside // 32, (inside % 8) // 4


def _place_tied_copies(m, chunks, per, offsets):
    """First-copy positions such that no two rows' copies collide: first copies on rows 0, 8, 16
    and 24 of the first tiles of a sweep (even and odd), of its last two tiles (the copies 128 and
    more rows on are in the NEXT chunk) and of the tiles in between."""
    used = np.zeros(m, dtype=bool)
    firsts = []
    tiles = sorted({t for c in range(chunks) for t in (c * per, c * per + 1, c * per + 2,
                                                       c * per + per - 2, c * per + per - 1)
                    if 0 <= t})
    for tile in tiles:
        for inside in (0, 8, 16, 24):
            at = tile * 128 + inside + np.array(offsets)
            if at.max() < m and not used[at].any():
                used[at] = True
                firsts.append(tile * 128 + inside)
    return np.array(firsts)


@pytest.mark.parametrize("n,m", TIE_SHAPES)
def test_exact_ties_keep_the_lowest_copies_at_every_merge_level(gpu, n, m):
    """a: R rows repeated over all n rows.  b: filler rows scaled by 0.5 with c = 19 >= k + 1
    exact copies of every one of the R rows.  Every a-row must return the k LOWEST copy positions
    in ascending order (k = 16, and 5 and 8 for the shallower lists).  Nothing else can win: a
    copy is at distance 0 / cosine 1, another unit row has |a - c|² ~ 2 and cosine ~ 0 +- 0.4, a
    filler row |a - f|² ~ 1.25.  Cosine also with the copies scaled by 2, 1, 0.5, 0.25 in turn:
    exact in fp16 and fp32 (elements below 2^-12 are flushed to zero first), so the ties stay
    exact in the kernel's arithmetic and in the oracle's."""
    from oracle import gine_numpy as G
    chunks, per, last = _sweep(gpu, n, m)
    assert (chunks, per, last) == GEOMETRY[(n, m)] and chunks > 1
    far = per * 128 + 37
    offsets = np.unique(np.array(TIE_OFFSETS + (far, far + 4)))      # ascending
    assert offsets.size == len(TIE_OFFSETS) + 2 >= 16 + 1
    column_of = {int(offset): at for at, offset in enumerate(offsets)}
    firsts = _place_tied_copies(m, chunks, per, offsets)
    count = firsts.size
    assert count >= 5
    positions = firsts[:, None] + offsets[None, :]                  # [R][c], ascending along a row
    assert np.unique(positions).size == positions.size and positions.max() < m
    # the placement reaches every level it names
    tile, wave, half = _lane(positions)
    same_tile = tile == tile[:, :1]
    assert np.all(same_tile[:, :12]) and not np.any(same_tile[:, 12:])
    for column in (1, 2, 3):                                       # the first copy's own lane
        assert np.all((wave[:, column] == wave[:, 0]) & (half[:, column] == half[:, 0]))
    for column in (6, 7, 8):                                       # its other register groups
        assert np.all(half[:, column] == half[:, 0]) and np.any(wave[:, column] == wave[:, 0])
    for column in (4, 5):                                           # the other lane half
        assert np.all((wave[:, column] == wave[:, 0]) & (half[:, column] != half[:, 0]))
    assert np.all(wave[:, 9:12] != wave[:, :1])                     # the other waves
    in_sweep = tile % per
    starts_pair = in_sweep[:, 0] % 2 == 0
    chunk = tile // per
    stays = chunk[:, column_of[128]] == chunk[:, 0]
    assert np.any(starts_pair & stays) and np.any(~starts_pair & stays)   # in a pair / across pairs
    assert np.any(chunk[:, column_of[512]] == chunk[:, 0]) == (per > 4)      # the same ring buffer again
    assert np.any(~stays)                                                 # copy 128 in the next chunk
    assert np.all(chunk[:, column_of[far]] != chunk[:, 0])                   # FAR: always another chunk
    print(f"topk({n}, {m}): sweeps of {per} tiles; {count} rows with {offsets.size} copies each")

    base = _pool(303, 512)[:count].copy()
    base[np.abs(base) < 2.0 ** -12] = 0
    filler = _pool(404, 8_192)[:m] * np.float16(0.5)
    b = filler.copy()
    scaled = filler.copy()
    factors = np.float16([2, 1, 0.5, 0.25])
    for column in range(offsets.size):
        b[positions[:, column]] = base
        scaled[positions[:, column]] = base * factors[column % 4]
        assert np.array_equal(scaled[positions[:, column]].astype(np.float64),
                              float(factors[column % 4]) * base.astype(np.float64))
    # the oracle agrees with the construction: the copies are its best, exactly tied
    for rows, metric in ((b, "l2"), (b, "cosine"), (scaled, "cosine")):
        full = G.pairwise_l2(base, rows) if metric == "l2" else -G.pairwise_cosine(base, rows)
        order = np.argsort(full, axis=1, kind="stable")[:, :offsets.size]
        assert np.array_equal(order, positions), metric
        tied = np.take_along_axis(full, order, axis=1)
        assert np.all(tied == tied[:, :1]), metric

    a = _device(np.tile(base, (-(-n // count), 1))[:n])
    which = np.arange(n) % count
    for name, rows, metric in (("l2", b, "l2"), ("cosine", b, "cosine"),
                               ("cosine, copies scaled by powers of two", scaled, "cosine")):
        device_b = _device(rows)
        for k in (16, 8, 5):
            values, indices = _topk(a, device_b, k=k, metric=metric)
            wrong = np.nonzero(np.any(indices != positions[which, :k], axis=1))[0]
            assert wrong.size == 0, (name, k, wrong[:4], indices[wrong[:4]],
                                     positions[which[wrong[:4]], :k])
            assert np.all(values == values[:, :1])


@pytest.mark.parametrize("n,m", [(300, 1_600), (65_536, 2_304), (70_000, 2_560)])
def test_a_better_row_arriving_later_keeps_the_order_of_tied_ones(gpu, n, m):
    """Seven exact copies of a row c at distance ~0.2 of the a-row (tied among themselves: one
    lane's registers, the other lane half, another wave, the next tile), then — at HIGHER
    indices, so that every list already holds the tied group when they arrive — the a-row itself
    and a row at distance ~0.1.  The two late rows go in front and the tied group behind them
    keeps its ascending order, at every list depth."""
    from oracle import gine_numpy as G
    rng = np.random.default_rng(m)
    tied_at, better_at = np.array([0, 1, 2, 3, 4, 32, 128]), np.array([8, 130])
    firsts = 256 * np.arange(6) + 16
    base = _pool(303, 512)[:firsts.size].copy()
    b = _pool(404, 8_192)[:m] * np.float16(0.5)
    want = []
    for row, first in zip(base, firsts):
        near = _planted_copies(row.astype(np.float64), rng)
        b[first + tied_at] = near[5]                 # 0.20 away
        b[first + better_at[0]] = row
        b[first + better_at[1]] = near[0]            # 0.10 away
        want.append(np.concatenate([first + better_at, first + tied_at]))
    want = np.array(want)
    for metric in ("l2", "cosine"):
        full = G.pairwise_l2(base, b) if metric == "l2" else -G.pairwise_cosine(base, b)
        order = np.argsort(full, axis=1, kind="stable")[:, :want.shape[1]]
        assert np.array_equal(order, want), metric
        tied = np.take_along_axis(full, order[:, 2:], axis=1)
        assert np.all(tied == tied[:, :1]) and np.all(full[np.arange(6), order[:, 1]] < tied[:, 0])
    a = _device(np.tile(base, (-(-n // 6), 1))[:n])
    device_b = _device(b)
    which = np.arange(n) % 6
    for metric in ("l2", "cosine"):
        for k in (9, 8, 5, 4, 3):
            _, indices = _topk(a, device_b, k=k, metric=metric)
            wrong = np.nonzero(np.any(indices != want[which, :k], axis=1))[0]
            assert wrong.size == 0, (metric, k, wrong[:4], indices[wrong[:4]])


# --------------------------------------------------------------------------------------------
# 5. planted neighbours: exact index lists

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


def _assert_gaps(a_rows, b, metric, want, excluded):
    """The planted lists are the oracle's first 16, every gap between consecutive entries and to
    the 17th at least 100 times the tolerance."""
    full = _oracle_block(a_rows, b, metric, excluded)
    scale = (a_rows.astype(np.float64) ** 2).sum(1)[:, None] + (b.astype(np.float64) ** 2).sum(1)[None, :]
    order = np.argsort(full if metric == "l2" else -full, axis=1, kind="stable")[:, :PLANT_K + 1]
    assert np.array_equal(order[:, :PLANT_K], want)
    top = np.take_along_axis(full, order, axis=1)
    if metric == "cosine":
        assert np.all(top[:, :-1] - top[:, 1:] >= 100 * COSINE_TOL)
    else:
        assert np.all(top[:, 1:] - top[:, :-1] >= 100 * L2_TOL) and np.all(top >= 0.1 - 1e-3)
        top_scale = np.take_along_axis(scale, order, axis=1)
        assert np.all(top[:, 1:] ** 2 - top[:, :-1] ** 2
                      >= 100 * D2_TOL * np.maximum(top_scale[:, 1:], top_scale[:, :-1]))


@pytest.mark.parametrize("n,m", [(300, 500), (65_536, 4_607), (70_000, 2_560)])
def test_planted_neighbours_come_back_in_the_planted_order(gpu, n, m):
    """For 24 a-rows, 16 perturbed copies in b at shuffled positions (all over b: every chunk,
    tile and wave), the farther the later.  The index list must be the planted order, for k = 16
    and, as its prefix, k = 1, 3, 8."""
    rng = np.random.default_rng(n + m)
    a, b = _a_rows(n), _b_rows(m)
    chosen = np.sort(rng.choice(n, size=24, replace=False))
    spots = rng.permutation(m)[:24 * PLANT_K].reshape(24, PLANT_K)
    for row, where in zip(chosen, spots):
        b[where] = _planted_copies(a[row].astype(np.float64), rng)
    for metric in ("l2", "cosine"):
        _assert_gaps(a[chosen], b, metric, spots, None)
    device_a, device_b = _device(a), _device(b)
    for metric in ("l2", "cosine"):
        for k in (16, 8, 3, 1):
            _, indices = _topk(device_a, device_b, k=k, metric=metric)
            np.testing.assert_array_equal(indices[chosen], spots[:, :k])


#: (k0, m): a = b[k0 : k0 + n] with n = 65,536; k0 % 128 puts the start of every a-block's
#: excluded band of 128 b-rows at the start (0), the middle (64) or the end (127) of a tile
BLOCK_OF_B = ((0, 65_536), (192, 65_805), (127, 65_663))
N_BLOCK = 65_536


@pytest.mark.parametrize("k0,m", BLOCK_OF_B)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_excluded_pair_is_the_true_nearest_and_appears_in_no_column(gpu, metric, k0, m):
    """a = b[k0 : k0 + n], exclude_offset = k0: the excluded pair is the exact copy of every row.
    For 24 of them 16 perturbed copies are planted in b outside the block's own rows' partners;
    their list is the planted order, and no row returns its own copy in any column."""
    n = N_BLOCK
    assert GEOMETRY[(n, m)] == _sweep(gpu, n, m) and m >= k0 + n
    assert k0 % 128 in (0, 64, 127)
    rng = np.random.default_rng(k0 + m)
    b = _b_rows(m)
    chosen = np.sort(rng.choice(n, size=24, replace=False))
    free = np.setdiff1d(np.arange(m), chosen + k0)
    spots = rng.permutation(free)[:24 * PLANT_K].reshape(24, PLANT_K)
    for row, where in zip(chosen, spots):
        b[where] = _planted_copies(b[k0 + row].astype(np.float64), rng)
    a = b[k0:k0 + n]
    _assert_gaps(a[chosen], b, metric, spots, chosen + k0)
    device_a, device_b = _device(a), _device(b)
    for k in (16, 4):
        values, indices = _topk(device_a, device_b, k=k, metric=metric, exclude_offset=k0)
        assert indices.min() >= 0 and indices.max() < m
        assert not np.any(indices == (np.arange(n) + k0)[:, None])
        np.testing.assert_array_equal(indices[chosen], spots[:, :k])
    sample = _sample(n, seed=k0, extra=chosen)[::4]
    worst = _against_oracle(a, b, sample, values, indices, metric, excluded=np.arange(n) + k0)
    print(f"exclude_offset={k0}, m={m}, {metric}: {sample.size} rows, worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 6. column 0 is `nearest`, bit for bit

def _pin_cases(n, m):
    """(a, b, arguments) for plain, exclude_self, exclude_offset and window_first at (n, m)."""
    a, b = _a_rows(n), _b_rows(m)
    both = _a_rows(max(n, m))
    cases = [(a, b, {})]
    if n <= m:
        offset = min(129, m - n)
        cases.append((both[offset:offset + n], both[:m], {"exclude_offset": offset}))
    else:
        first = min(777, n - m)
        cases.append((a, a[first:first + m], {"window_first": first}))
    cases.append((both[:n], both[:n], {"exclude_self": True}))
    if n > 1:
        cases.append((both[:n], both[n // 3:n // 3 + max(1, n // 2)], {"window_first": n // 3}))
        cases.append((both[5:5 + n // 2], both[:n], {"exclude_offset": 5}))
    return cases


@pytest.mark.parametrize("n,m", [(1, 1), (129, 127), (255, 129), (257, 385), (513, 640),
                                 (770, 1), (1_000, 3_000), (65_536, 4_607)])
def test_column_zero_is_nearest_bit_for_bit(gpu, n, m):
    modes = set()
    for a, b, arguments in _pin_cases(n, m):
        modes |= set(arguments) or {"plain"}
        device_a, device_b = _device(a), _device(b)
        for metric in ("l2", "cosine"):
            want_values, want_indices = _nearest(device_a, device_b, metric=metric, **arguments)
            for k in (1, 4, 16):
                values, indices = _topk(device_a, device_b, k=k, metric=metric, **arguments)
                assert values[:, 0].tobytes() == want_values.tobytes(), (arguments, metric, k)
                assert indices[:, 0].tobytes() == want_indices.tobytes(), (arguments, metric, k)
    assert modes >= ({"plain", "exclude_self"} if n == 1 else
                     {"plain", "exclude_self", "exclude_offset", "window_first"})


# --------------------------------------------------------------------------------------------
# 7. prefix, block independence, determinism, workspace reuse

@pytest.mark.parametrize("n,m", [(513, 640), (65_536, 4_607), (70_000, 2_560)])
def test_a_shorter_list_is_the_prefix_of_a_longer_one(gpu, n, m):
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    for metric in ("l2", "cosine"):
        for arguments in ({}, {"exclude_offset": 3}):
            for short, long in ((3, 5), (4, 16), (1, 2), (8, 9)):
                one = _topk(a, b, k=short, metric=metric, **arguments)
                two = _topk(a, b, k=long, metric=metric, **arguments)
                assert one[0].tobytes() == np.ascontiguousarray(two[0][:, :short]).tobytes()
                assert one[1].tobytes() == np.ascontiguousarray(two[1][:, :short]).tobytes()


@pytest.mark.parametrize("n,m", [(131_072, 1_281), (65_536, 4_607)])
def test_a_row_s_result_does_not_depend_on_its_block(gpu, n, m):
    """topk(a[s:e], b) == topk(a, b)[s:e] bit for bit, s not a multiple of 128: the rows land on
    other lanes, waves and workgroups, and the shorter call splits b into other chunks."""
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    start, stop = 777, 777 + 65_536 + 1_000 if n > 70_000 else 777 + 30_001
    assert start % BLOCK_A != 0
    for metric in ("l2", "cosine"):
        for k in (5, 16):
            values, indices = _topk(a, b, k=k, metric=metric)
            part_values, part_indices = _topk(a[start:stop], b, k=k, metric=metric)
            assert np.ascontiguousarray(values[start:stop]).tobytes() == part_values.tobytes()
            assert np.ascontiguousarray(indices[start:stop]).tobytes() == part_indices.tobytes()


def test_two_runs_give_the_same_bytes(gpu):
    n, m = 65_536, 4_607
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    for metric in ("l2", "cosine"):
        for k in (1, 8, 16):
            one, two = _topk(a, b, k=k, metric=metric), _topk(a, b, k=k, metric=metric)
            assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()


def test_workspace_of_a_larger_call_changes_nothing(gpu):
    from ginfinity_amd import distance
    n, m = 65_536, 2_304
    a, b = _device(_a_rows(131_072)), _device(_b_rows(8_192))
    workspace = distance.TopKWorkspace()
    for metric in ("l2", "cosine"):
        fresh = _topk(a[:n], b[:m], k=5, metric=metric, exclude_offset=129)
        distance.topk(a, b, k=16, metric=metric, workspace=workspace)    # leaves its lists behind
        again = _topk(a[:n], b[:m], k=5, metric=metric, exclude_offset=129, workspace=workspace)
        assert fresh[0].tobytes() == again[0].tobytes()
        assert fresh[1].tobytes() == again[1].tobytes()


# --------------------------------------------------------------------------------------------
# 8. full size

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_million_by_million_top8_sampled_against_the_oracle(gpu, metric):
    """1,000,000 unit rows against themselves, exclude_self, k = 8: at least 2,048 sampled rows
    — both sides of 96 workgroup seams, the first and the last rows (the ragged last tile: 10^6
    = 128 * 7,812 + 64) — rank-wise against the float64 definition, in 512-row blocks."""
    from ginfinity_amd import synthetic
    rows = 1_000_000
    points = synthetic.unit_rows(0, rows)
    values, indices = _topk(_device(points), None, k=8, metric=metric, exclude_self=True)
    assert values.shape == (rows, 8) and indices.min() >= 0 and indices.max() < rows
    assert not np.any(indices == np.arange(rows)[:, None])
    rng = np.random.default_rng(7)
    seams = np.concatenate([np.array([BLOCK_A * s - 1, BLOCK_A * s])
                            for s in rng.choice(np.arange(1, rows // BLOCK_A), 96, replace=False)])
    sample = np.unique(np.concatenate([
        np.arange(0, 260), np.arange(rows - 300, rows), seams, rng.integers(0, rows, 1_400)]))
    assert sample.size >= 2_048 and np.isin(seams, sample).all() and seams.size >= 2 * 64
    assert rows % 128 != 0 and rows - 1 in sample and 0 in sample
    worst = _against_oracle(points, points, sample, values, indices, metric,
                            excluded=np.arange(rows))
    print(f"1M x 1M top-8 ({metric}): {sample.size} sampled rows, worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 9. real embeddings

def test_real_embeddings_top8_cosine(gpu, gpu_encoder, rouskin_shard):
    block, counts = gpu_encoder.encode_graphs_device(rouskin_shard.slice(0, 40))
    assert block.shape[0] == sum(counts) and block.shape[0] >= 512
    host = block.cpu().numpy()
    values, indices = _topk(block, None, k=8, metric="cosine", exclude_self=True)
    rows = np.arange(512)
    worst = _against_oracle(host, host, rows, values, indices, "cosine",
                            excluded=np.arange(host.shape[0]))
    print(f"real embeddings ({host.shape[0]} rows): worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 10. cross-shard, world size 1

def test_cross_shard_topk_world_size_one_is_topk(gpu):
    """No process group: cross_shard_topk(block, 8) is distance.topk(block, k=8,
    exclude_self=True) bit for bit, whatever the chunking; an empty block gives empty results.
    The equality holds for THIS fixed block only, not for every input: the merge orders by
    (value, row) and the kernel by (key, row), and the two disagree where two of a row's eight
    neighbours have different keys and the same fp32 value, i.e. lie within ~3e-7 of each other
    in d² — about one row in 10^4 for random unit rows, none among these 1,200 (the seed is
    fixed; `cross_shard_topk` states the caveat).  On other data the two calls return the same
    rows and values with such a pair of columns exchanged."""
    from ginfinity_amd import distance, parallel
    block = _device(_a_rows(1_200))
    for metric in ("l2", "cosine"):
        want_values, want_indices = distance.topk(block, k=8, metric=metric, exclude_self=True)
        want_values, want_indices = want_values.clone(), want_indices.clone()
        for chunk_rows in (1 << 20, 1_000, 257):
            values, indices, offsets = parallel.cross_shard_topk(block, 8, metric=metric,
                                                                 chunk_rows=chunk_rows)
            assert offsets == [0, 1_200] and indices.dtype == torch.int64
            assert torch.equal(values.view(torch.int32), want_values.view(torch.int32))
            assert torch.equal(indices, want_indices.to(torch.int64))
    values, indices, offsets = parallel.cross_shard_topk(block[:0], 8)
    assert values.shape == (0, 8) and indices.shape == (0, 8) and offsets == [0, 0]
