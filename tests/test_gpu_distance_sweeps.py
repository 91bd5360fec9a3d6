"""The nearest-row kernel (csrc/pairwise.hip) where its machinery is: sweeps of more than one
128-row b-tile per workgroup (the ring of four LDS buffers, two tiles per barrier and the odd
tail, the reduce that waves 4-7 carry across the barrier), exact ties at every merge level,
excluded pairs that are the true nearest, ragged ends inside a sweep, rows with nothing left,
and the dense kernel at its seams.  The oracle is the float64 definition (oracle.gine_numpy):
the reference has no implementation of this step.

A workgroup sweeps more than one tile only when (n / 256) * (m / 128) exceeds about 1,024
(carve() in pairwise.hip), so every multi-tile test here has n >= 65,536 and takes its shape
from SWEEPS, whose sweep lengths ``test_sweep_geometry_is_what_the_tests_assume`` asserts."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance.py: unit rows against the float64 oracle
L2_TOL = 2e-5            # the same, on an L2 distance
D2_TOL = 4e-6            # on d², times (|a_i|² + |b_j|²): cancellation for near-duplicates


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


# --------------------------------------------------------------------------------------------
# 1. sweep geometry

#: (n, m, chunks, tiles per workgroup, tiles of the last chunk) — what carve() chooses today.
#: A retune of its heuristic fails test_sweep_geometry_is_what_the_tests_assume and has to
#: bring new shapes: nothing below may fall back to one tile per workgroup unnoticed.
SWEEPS = (
    (65_536, 512, 4, 1, 1),
    (65_536, 1_024, 4, 2, 2),
    (65_536, 1_153, 4, 3, 1),          # 128 * 9 + 1
    (65_536, 2_047, 4, 4, 4),          # 128 * 15 + 127
    (65_536, 2_560, 4, 5, 5),
    (65_536, 3_073, 4, 7, 4),          # 128 * 24 + 1
    (65_536, 4_096, 4, 8, 8),
    (65_536, 4_607, 4, 9, 9),          # 128 * 35 + 127
    (65_536, 8_192, 4, 16, 16),
    (70_000, 2_560, 7, 3, 2),
    (131_072, 1_281, 2, 6, 5),         # 128 * 10 + 1
    (131_072, 2_304, 2, 9, 9),
    (262_400, 4_096, 5, 7, 4),
    (262_400, 8_192, 5, 13, 12),
    # a is a block of b (section 3): m >= n, long sweeps
    (65_536, 65_536, 4, 128, 128),
    (65_536, 65_663, 4, 129, 126),     # 127 + n = 128 * 512 + 127
    (65_536, 65_805, 4, 129, 128),
    (65_536, 66_369, 4, 130, 129),
)
GEOMETRY = {(n, m): (chunks, per, last) for n, m, chunks, per, last in SWEEPS}


def _align(size):
    return (size + 255) // 256 * 256


def _sweep(lib, n, m):
    """(chunks, tiles per workgroup, tiles of the last chunk) of nearest(n, m), recovered from
    the workspace size: carve() lays out s and t (tiles_b * 128 floats each), a_term (n floats)
    and the two [chunks][n] partial arrays, each rounded up to 256 bytes."""
    tiles_b = (m + 127) // 128
    partial, odd = divmod(lib.gfy_pairwise_workspace_bytes(n, m)
                          - 2 * _align(tiles_b * 128 * 4) - _align(n * 4), 2)
    assert odd == 0 and n * 4 >= 256           # below 64 rows two counts could share a size
    fits = [c for c in range(1, tiles_b + 1) if _align(c * n * 4) == partial]
    assert len(fits) == 1, (n, m, fits)
    chunks = fits[0]
    per = -(-tiles_b // chunks)
    return chunks, per, tiles_b - (chunks - 1) * per


def test_sweep_geometry_is_what_the_tests_assume(gpu):
    reached, short_last = set(), False
    for n, m, *want in SWEEPS:
        chunks, per, last = _sweep(gpu, n, m)
        print(f"nearest({n}, {m}): {chunks} chunks of {per} tiles, the last of {last}")
        assert (chunks, per, last) == tuple(want), (n, m)
        assert 1 <= last <= per and (chunks - 1) * per + last == (m + 127) // 128
        reached |= {per, last}
        short_last |= chunks > 1 and last < per
    print("sweep lengths reached:", sorted(reached))
    assert set(range(1, 10)) <= reached
    assert max(reached) >= 16
    assert short_last
    assert len({n for n, *_ in SWEEPS}) >= 3 and max(n for n, *_ in SWEEPS) > 262_144


# --------------------------------------------------------------------------------------------
# inputs, samples, the oracle comparison

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


def _near_copy(row):
    """``row`` with its largest element moved away from zero by one fp16 ulp."""
    out = row.copy()
    out.view(np.uint16)[np.argmax(np.abs(row))] += 1
    assert np.count_nonzero(out != row) == 1 and np.all(np.isfinite(out))
    return out


def _sample(n, seed, extra=()):
    """The a-rows the oracle is evaluated on: both sides of 40 workgroup seams, the first and
    the last 300 rows, 2,200 random rows, and ``extra``."""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.arange(1, n // 256), size=40, replace=False)
    rows = np.unique(np.concatenate([
        256 * blocks - 1, 256 * blocks, np.arange(300), np.arange(n - 300, n),
        rng.integers(0, n, 2_200), np.asarray(extra, dtype=np.int64)]))
    assert np.isin(256 * blocks - 1, rows).all() and np.isin(256 * blocks, rows).all()
    assert blocks.size >= 32 and rows.size >= 2_000 + 600 + 64
    return rows


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def _nearest(a, b, **arguments):
    from ginfinity_amd import distance
    values, indices = distance.nearest(a, b, **arguments)
    return values.cpu().numpy(), indices.cpu().numpy()


def _against_oracle(a, b, rows, values, indices, metric, excluded=None):
    """``values`` / ``indices`` [n] of the a-rows ``rows`` against the float64 definition with
    the pair (i, excluded[i]) removed (where that is a row of b).  Cosine: 2e-6.  L2: d² within
    4e-6 (|a_i|² + |b_j|²) — the form that holds next to a near-duplicate, where d itself is the
    square root of cancellation noise — and 2e-5 on d wherever d >= 0.1."""
    from oracle import gine_numpy as G
    m = b.shape[0]
    assert indices.min() >= 0 and indices.max() < m
    worst = 0.0
    for start in range(0, rows.size, 512):
        block = rows[start:start + 512]
        full = G.pairwise_l2(a[block], b) if metric == "l2" else G.pairwise_cosine(a[block], b)
        if excluded is not None:
            gone = excluded[block]
            has = (gone >= 0) & (gone < m)
            full[np.nonzero(has)[0], gone[has]] = np.inf if metric == "l2" else -np.inf
        best = full.min(axis=1) if metric == "l2" else full.max(axis=1)
        assert np.all(np.isfinite(best))
        got = values[block].astype(np.float64)
        picked = full[np.arange(block.size), indices[block]]
        if metric == "cosine":
            assert np.abs(picked - best).max() <= COSINE_TOL
            assert np.abs(got - picked).max() <= COSINE_TOL
            worst = max(worst, float(np.abs(got - best).max()))
        else:
            scale = ((a[block].astype(np.float64) ** 2).sum(1)
                     + (b[indices[block]].astype(np.float64) ** 2).sum(1))
            assert np.all(np.abs(picked ** 2 - best ** 2) <= D2_TOL * scale)
            assert np.all(np.abs(got ** 2 - picked ** 2) <= D2_TOL * scale)
            far = best >= 0.1
            assert np.all(np.abs(picked - best)[far] <= L2_TOL)
            assert np.all(np.abs(got - picked)[far] <= L2_TOL)
            worst = max(worst, float((np.abs(got ** 2 - best ** 2) / scale).max()))
    return worst


# --------------------------------------------------------------------------------------------
# 2. exact ties at every merge level

#: two copies this far apart inside one tile: two registers of a lane (1-3, 8, 16, 24), the two
#: lane halves merged by __shfl_xor (4), two waves merged through LDS (32, 64, 96)
IN_TILE = (1, 2, 3, 4, 8, 16, 24, 32, 64, 96)
#: the second tile of a pair, the next pair, the same ring buffer again
TILES_APART = (128, 256, 512)
#: into the next tile / the one after it, 37 rows EARLIER in the tile: the later copy is held by
#: a lower lane half or wave than the earlier one, so a merge that forgets the index keeps it
BACK_IN_TILE = {91: 1, 219: 2}
TIE_SHAPES = [(n, m) for n, m, *_ in SWEEPS if m <= 8_192]


def _place_copies(m, chunks, per, seed):
    """Positions of first copies and the distance to their second copy, every position used
    once: {distance: [first, ...]}.  In-tile distances stay inside one tile; 128 starts in the
    first tile of a pair and 128 / 256 / 512 stay inside one workgroup's sweep (where it is long
    enough); 91 and 219 land one and two tiles later on an earlier row of the tile, inside the
    sweep; the last distance reaches past the sweep of a chunk, into another chunk."""
    rng = np.random.default_rng(seed)
    tiles_b = (m + 127) // 128
    used = np.zeros(m, dtype=bool)
    quota = max(2, min(16, m // (8 * (len(IN_TILE) + len(TILES_APART) + len(BACK_IN_TILE) + 1))))
    placed = {}

    def put(distance, candidates):
        """Half of the quota from first copies in rows 64-127 of a tile — the waves that carry
        their reduce across the barrier — where there are such candidates."""
        candidates = rng.permutation(candidates)
        upper = candidates[candidates % 128 >= 64]
        lower = candidates[candidates % 128 < 64]
        taken = []
        for group, count in ((upper, quota // 2), (lower, quota), (upper, quota)):
            for first in group:
                if len(taken) >= count:
                    break
                if not used[first] and not used[first + distance]:
                    used[first] = used[first + distance] = True
                    taken.append(int(first))
        if taken:
            placed[distance] = taken

    position = np.arange(m)
    tile = position // 128
    in_chunk = tile % per                                       # tile of its workgroup's sweep
    sweep = np.minimum(per, tiles_b - (tile // per) * per)       # length of that sweep
    for distance in IN_TILE:
        put(distance, position[(position % 128 + distance < 128) & (position + distance < m)])
    for distance in TILES_APART:
        inside = (in_chunk + distance // 128 < sweep) & (position + distance < m)
        if distance == 128:
            inside &= in_chunk % 2 == 0
        put(distance, position[inside])
    for distance, tiles in BACK_IN_TILE.items():
        put(distance, position[(position % 128 >= 37) & (in_chunk + tiles < sweep)
                               & (position + distance < m)])
    if chunks > 1:
        far = per * 128 + 37
        put(far, position[position + far < m])
    return placed


@pytest.mark.parametrize("n,m", TIE_SHAPES)
def test_exact_ties_keep_the_first_copy_at_every_merge_level(gpu, n, m):
    """a: R unit rows repeated over all n rows.  b: filler rows scaled by 0.5 with two exact
    copies of every one of the R rows at a controlled distance.  Every a-row must return its
    FIRST copy.  Nothing else can win: a copy is at distance 0 / cosine 1, another unit row c
    has |a - c|² ~ 2 and cosine ~ 0 +- 0.4, a filler row f has |a - f|² ~ 1.25.
    Cosine also with the first copy scaled by 2 and the second by 0.5: scaling by a power of two
    is exact in fp16 and fp32 (elements below 2^-12 are flushed to zero first, so nothing goes
    subnormal), so the tie stays exact in the kernel's arithmetic and in the oracle's."""
    from oracle import gine_numpy as G
    chunks, per, last = _sweep(gpu, n, m)
    assert (chunks, per, last) == GEOMETRY[(n, m)]
    placed = _place_copies(m, chunks, per, seed=m)
    # the placement reached what the shape allows
    for distance in IN_TILE:
        firsts = np.array(placed[distance])
        assert np.all(firsts // 128 == (firsts + distance) // 128)
        assert np.any(firsts % 128 < 64)
        assert distance >= 64 or np.any(firsts % 128 >= 64)
    for distance in TILES_APART:
        assert (distance in placed) == (per > distance // 128), (distance, per)
        if distance in placed:
            firsts = np.array(placed[distance])
            assert np.all(firsts // 128 // per == (firsts + distance) // 128 // per)
            assert np.any(firsts % 128 >= 64)
    for distance, tiles in BACK_IN_TILE.items():
        assert (distance in placed) == (per > tiles), (distance, per)
        if distance in placed:
            firsts = np.array(placed[distance])
            assert np.all(firsts // 128 + tiles == (firsts + distance) // 128)
            assert np.all(firsts // 128 // per == (firsts + distance) // 128 // per)
    far = per * 128 + 37
    assert (far in placed) == (chunks > 1 and far < m)
    print(f"nearest({n}, {m}): sweeps of {per} tiles (last {last}); copies at distances "
          f"{sorted(placed)}")

    first = np.concatenate([placed[d] for d in sorted(placed)])
    second = np.concatenate([np.array(placed[d]) + d for d in sorted(placed)])
    count = first.size
    base = _pool(303, 512)[:count].copy()
    base[np.abs(base) < 2.0 ** -12] = 0
    filler = _pool(404, 8_192)[:m] * np.float16(0.5)
    b = filler.copy()
    b[first], b[second] = base, base
    scaled = filler.copy()
    scaled[first], scaled[second] = base * np.float16(2), base * np.float16(0.5)
    assert np.array_equal(scaled[first].astype(np.float64), 2.0 * base.astype(np.float64))
    assert np.array_equal(scaled[second].astype(np.float64), 0.5 * base.astype(np.float64))
    # the oracle agrees with the construction (its argmin / argmax keep the first of equals)
    assert np.array_equal(G.pairwise_l2(base, b).argmin(axis=1), first)
    assert np.array_equal(G.pairwise_cosine(base, b).argmax(axis=1), first)
    assert np.array_equal(G.pairwise_cosine(base, scaled).argmax(axis=1), first)
    assert np.array_equal(G.pairwise_cosine(base, scaled)[np.arange(count), first],
                          G.pairwise_cosine(base, scaled)[np.arange(count), second])

    a = _device(np.tile(base, (-(-n // count), 1))[:n])
    want = first[np.arange(n) % count]
    for name, rows, metric in (("l2", b, "l2"), ("cosine", b, "cosine"),
                               ("cosine, copies scaled by 2 and 0.5", scaled, "cosine")):
        _, indices = _nearest(a, _device(rows), metric=metric)
        wrong = np.nonzero(indices != want)[0]
        assert wrong.size == 0, (name, wrong[:8], indices[wrong[:8]], want[wrong[:8]])


# --------------------------------------------------------------------------------------------
# 3. exclusion where it matters

#: (k, m): a = b[k : k + n] with n = 65,536.  k % 128 puts the start of every a-block's excluded
#: band of 256 b-rows at the start (0), the middle (64) or the end (127) of a tile; a band that
#: starts at a tile's first row covers the two tiles of one pair (k = 0: tiles 2j, 2j + 1), any
#: other covers three tiles and so crosses a pair boundary too.
BLOCK_OF_B = ((0, 65_536), (192, 65_805), (127, 65_663), (333, 66_369))
N_BLOCK = 65_536


def test_exclusion_offsets_reach_every_place(gpu):
    starts, crosses_chunk, ragged_end = set(), False, False
    for k, m in BLOCK_OF_B:
        chunks, per, last = _sweep(gpu, N_BLOCK, m)
        assert (chunks, per, last) == GEOMETRY[(N_BLOCK, m)] and m >= k + N_BLOCK
        starts.add(k % 128)
        # a chunk boundary strictly inside some a-block's band [256 j + k, 256 j + k + 256)
        edges = np.arange(1, chunks) * per * 128
        crosses_chunk |= bool(np.any((edges > k) & (edges < k + N_BLOCK) & ((edges - k) % 256 != 0)))
        ragged_end |= m == k + N_BLOCK and m % 128 != 0      # the last partners: the ragged tile
    assert {0, 64, 127} <= starts and crosses_chunk and ragged_end
    assert any(k % 128 == 0 and (k // 128) % 2 == 0 for k, _ in BLOCK_OF_B)   # one pair exactly
    assert any(k % 128 != 0 for k, _ in BLOCK_OF_B)                           # a pair boundary


@pytest.mark.parametrize("k,m", BLOCK_OF_B)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_excluded_pair_is_the_true_nearest_of_every_row(gpu, metric, k, m):
    """a = b[k : k + n]: the excluded pair (i, i + k) is the exact copy of every row, so a
    missed exclusion changes every answer.  Some rows have a near-copy (one element moved by
    one fp16 ulp) in the slot next to the excluded one, others 300 rows further or earlier —
    another tile — or on the next row that is a wave's first of its tile: their answer after the exclusion is known by construction."""
    n = N_BLOCK
    b = _b_rows(m)
    want = {}                                  # a-row -> its b-row by construction
    for t in range(64):
        r = k + 997 * t + 5                    # 997 is prime: every position inside a tile
        other = (r + 1, r + 300, r - 300, r - r % 32 + 32)[t % 4]   # the last: a wave's first b-row
        if not (0 <= other < m and r < k + n):
            continue
        b[other] = _near_copy(b[r])
        want[r - k] = other
        if k <= other < k + n:
            want[other - k] = r
    assert len(want) >= 100
    a = b[k:k + n]
    values, indices = _nearest(_device(a), _device(b), metric=metric, exclude_offset=k)
    assert indices.min() >= 0 and indices.max() < m
    assert not np.any(indices == np.arange(n) + k)
    rows = np.array(sorted(want))
    np.testing.assert_array_equal(indices[rows], np.array([want[r] for r in rows]))
    sample = _sample(n, seed=k, extra=rows)
    worst = _against_oracle(a, b, sample, values, indices, metric, excluded=np.arange(n) + k)
    print(f"exclude_offset={k}, m={m}, {metric}: {sample.size} rows, worst {worst:.2e}")


@pytest.mark.parametrize("m,first", [(1_153, 0), (1_153, 64_383), (2_560, 4_429),
                                     (4_607, 31_000), (4_607, 60_929)])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_window_of_a_excludes_every_row_s_own_copy_multi_tile(gpu, metric, m, first):
    """b = a[first : first + m] through ``window_first`` on sweeps of 3 (last chunk 1), 5 and 9
    tiles (ragged): the rows inside the window have their exact copy excluded — the window at
    the front, in the middle and at the very end of a — and near-copies one slot or 300 rows
    away give the answer by construction."""
    n = 65_536
    assert GEOMETRY[(n, m)] == _sweep(gpu, n, m) and first + m <= n
    a = _a_rows(n)
    want = {}
    for t in range(m // 401):
        r = first + 401 * t + 3
        other = r + (1, 300, -300)[t % 3]
        if not first <= other < first + m:
            continue
        a[other] = _near_copy(a[r])
        want[r], want[other] = other - first, r - first
    assert len(want) >= 2
    b = a[first:first + m]
    values, indices = _nearest(_device(a), _device(b), metric=metric, window_first=first)
    assert indices.min() >= 0 and indices.max() < m
    assert not np.any(indices == np.arange(n) - first)
    rows = np.array(sorted(want))
    np.testing.assert_array_equal(indices[rows], np.array([want[r] for r in rows]))
    sample = _sample(n, seed=first + m, extra=np.arange(first, first + m))
    worst = _against_oracle(a, b, sample, values, indices, metric, excluded=np.arange(n) - first)
    print(f"window_first={first}, m={m}, {metric}: {sample.size} rows, worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 4. ragged ends inside a sweep

@pytest.mark.parametrize("n,m", [(n, m) for n, m, *_ in SWEEPS
                                 if m % 128 in (1, 127) and m <= 8_192])
def test_ragged_last_tile_inside_a_sweep(gpu, n, m):
    """m = 128 q + 1 and 128 q + 127: every 7th a-row is b[m - 1], whose padding rows re-read it
    with t = +-inf (a wrong pad term is an index >= m or a wrong winner), other rows are b[0]."""
    assert GEOMETRY[(n, m)] == _sweep(gpu, n, m)
    a, b = _a_rows(n), _b_rows(m)
    at_end = np.arange(n) % 7 == 0
    at_start = (np.arange(n) % 11 == 3) & ~at_end
    a[at_end], a[at_start] = b[m - 1], b[0]
    device_a, device_b = _device(a), _device(b)
    for metric in ("l2", "cosine"):
        values, indices = _nearest(device_a, device_b, metric=metric)
        assert indices.min() >= 0 and indices.max() < m
        assert np.all(indices[at_end] == m - 1) and np.all(indices[at_start] == 0)
        worst = _against_oracle(a, b, _sample(n, seed=m), values, indices, metric)
        print(f"nearest({n}, {m}) {metric}: worst {worst:.2e}")


# --------------------------------------------------------------------------------------------
# 5. everything excluded

@pytest.mark.parametrize("metric,nothing", [("l2", np.inf), ("cosine", -np.inf)])
def test_a_row_with_every_candidate_excluded(gpu, metric, nothing):
    """Index -1 and value +inf (L2) / -inf (cosine), as include/gfy.h defines it."""
    rows = _a_rows(700)
    values, indices = _nearest(rows[:1], rows[:1], metric=metric, exclude_self=True)
    assert indices[0] == -1 and values[0] == nothing
    # one b-row: only the a-row that is that row has nothing left
    for k in (0, 5, 300):
        values, indices = _nearest(rows[:1], rows[k:k + 1], metric=metric, exclude_offset=0)
        assert indices[0] == -1 and values[0] == nothing
        values, indices = _nearest(rows, rows[k:k + 1], metric=metric, window_first=k)
        others = np.arange(700) != k
        assert indices[k] == -1 and values[k] == nothing
        assert np.all(indices[others] == 0) and np.all(np.isfinite(values[others]))


# --------------------------------------------------------------------------------------------
# 6. the dense kernel at its seams

DENSE_M = (127, 128, 129, 256, 384, 511, 513, 641, 1_153, 2_560)
PATTERN = 0x7FA5A5A5          # a NaN with a payload: the kernel writes sqrt(max(x, 0)) or a product
GUARD = 4_096                 # floats in front of and behind [n][m]


def _mixed_rows(seed, count, unit):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((count, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    if not unit:
        data *= rng.uniform(0.2, 3.0, size=(count, 1))
    return data.astype(np.float16)


@pytest.mark.parametrize("n", [255, 256, 257, 513])
@pytest.mark.parametrize("unit", [True, False])
def test_dense_block_at_workgroup_and_tile_seams(gpu, unit, n):
    """Every element against the oracle, through the C ABI into a buffer with guard rows: the
    guards keep their bit pattern and no element of [n][m] does."""
    from ginfinity_amd import _native as native
    from oracle import gine_numpy as G
    a = _mixed_rows(7 * n, n, unit)
    device_a = _device(a)
    a2 = (a.astype(np.float64) ** 2).sum(1)
    stream = torch.cuda.current_stream().cuda_stream
    for m in DENSE_M:
        b = _mixed_rows(11 * m + 1, m, unit)
        device_b = _device(b)
        scale = a2[:, None] + (b.astype(np.float64) ** 2).sum(1)[None, :]
        scratch = torch.empty(gpu.gfy_pairwise_workspace_bytes(n, m), dtype=torch.uint8,
                              device="cuda")
        for metric in ("l2", "cosine"):
            buffer = torch.full((GUARD + n * m + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
            native.check(gpu.gfy_pairwise_dense(
                device_a.data_ptr(), n, device_b.data_ptr(), m,
                native.GFY_L2 if metric == "l2" else native.GFY_COSINE,
                buffer.data_ptr() + 4 * GUARD, scratch.data_ptr(), scratch.numel(), stream),
                "gfy_pairwise_dense")
            bits = buffer.cpu().numpy()
            assert np.all(bits[:GUARD] == PATTERN) and np.all(bits[GUARD + n * m:] == PATTERN)
            inside = bits[GUARD:GUARD + n * m]
            assert not np.any(inside == PATTERN), (n, m, metric)
            got = inside.view(np.float32).reshape(n, m).astype(np.float64)
            if metric == "cosine":
                assert np.abs(got - G.pairwise_cosine(a, b)).max() <= COSINE_TOL, (n, m)
            else:
                want = G.pairwise_l2(a, b)
                assert np.all(np.abs(got ** 2 - want ** 2) <= D2_TOL * scale), (n, m)
                if unit:
                    assert np.abs(got - want).max() <= L2_TOL, (n, m)


# --------------------------------------------------------------------------------------------
# 7. checks that need no oracle

def test_two_runs_give_the_same_bytes(gpu):
    from ginfinity_amd import distance
    n, m = 65_536, 4_607
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    for metric in ("l2", "cosine"):
        one, two = _nearest(a, b, metric=metric), _nearest(a, b, metric=metric)
        assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
        one = distance.pairwise(a[:513], b, metric=metric)
        two = distance.pairwise(a[:513], b, metric=metric)
        assert torch.equal(one.view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("n,m", [(131_072, 1_281), (65_536, 4_607)])
def test_a_row_s_result_does_not_depend_on_its_block(gpu, n, m):
    """nearest(a[s:e], b) == nearest(a, b)[s:e] bit for bit, s not a multiple of 256: the rows
    land on other lanes, waves and workgroups, and the shorter call splits b into other chunks."""
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    start, stop = 777, 777 + 65_536 + 1_000 if n > 70_000 else 777 + 30_001
    for metric in ("l2", "cosine"):
        values, indices = _nearest(a, b, metric=metric)
        part_values, part_indices = _nearest(a[start:stop], b, metric=metric)
        assert values[start:stop].tobytes() == part_values.tobytes()
        assert indices[start:stop].tobytes() == part_indices.tobytes()


def test_nearest_and_dense_agree(gpu):
    """Cosine: both paths compute -fma(dot, s, 0) * (1 / |a|) per pair (k_pairwise<true> and
    k_pairwise<false> + k_nearest_finish), and negation and the product with a positive
    number are monotone, so the nearest value IS the row maximum of the dense block, bit for
    bit.  L2: nearest folds -|b|²/2 into the accumulator's start — other arithmetic — so the
    dense distance at the returned index is within the tolerance of the row minimum."""
    from ginfinity_amd import distance
    n, m = 65_536, 2_560
    assert GEOMETRY[(n, m)] == _sweep(gpu, n, m)
    a, b = _device(_a_rows(n)), _device(_b_rows(m))
    rows = torch.arange(n, device="cuda")
    for metric in ("cosine", "l2"):
        values, indices = distance.nearest(a, b, metric=metric)
        assert int(indices.min()) >= 0 and int(indices.max()) < m      # before they index
        dense = distance.pairwise(a, b, metric=metric)
        at_index = dense[rows, indices.long()]
        if metric == "cosine":
            assert torch.equal(values.view(torch.int32), dense.max(dim=1).values.view(torch.int32))
            assert torch.equal(values.view(torch.int32), at_index.view(torch.int32))
        else:
            assert float((at_index - dense.min(dim=1).values).abs().max()) <= L2_TOL
            assert float((values - at_index).abs().max()) <= L2_TOL


def test_workspace_of_a_larger_call_changes_nothing(gpu):
    from ginfinity_amd import distance
    n, m = 65_536, 3_073
    a, b = _device(_a_rows(131_072)), _device(_b_rows(8_192))
    workspace = distance.NearestWorkspace()
    for metric in ("l2", "cosine"):
        fresh = _nearest(a[:n], b[:m], metric=metric, exclude_offset=129)
        distance.nearest(a, b, metric=metric, workspace=workspace)       # leaves its partials behind
        again = _nearest(a[:n], b[:m], metric=metric, exclude_offset=129, workspace=workspace)
        assert fresh[0].tobytes() == again[0].tobytes()
        assert fresh[1].tobytes() == again[1].tobytes()
