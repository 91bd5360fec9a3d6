"""Rows that cover the VALUE range of the distance and alignment inputs — zero, fp16 subnormal,
tiny, near the fp16 maximum, one-hot, clustered, norms ten orders of magnitude apart — and the
float64 side of the tests that use them (tests/test_value_cases_host.py, test_gpu_distance_values.py,
test_gpu_align_values.py).  numpy only: everything here runs without a device.

Every family is ``[count, 128]`` float16, built from a seed; nothing is stored.

    family(name, count, seed)        the rows of one family
    placed(name, count, ...)         family rows among Gaussian filler at the rows where the kernels
                                     change path (block, tile and chunk seams, the ragged end)
    scaled(rows, p)                  rows * 2^p, asserted exact
    reference(a, b, metric)          the float64 definition per pair (cosine S, L2 d²) and the
                                     per-pair tolerance
    certain(...)                     the pairs whose place in a row's ranking no kernel within the
                                     tolerance can change: where indices are asserted exactly

The filler of a search is not independent: every a-row has a noisy copy among the b-rows (cosine
about 0.96), so that the nearest row of a filler row is a filler row by a wide margin whatever
the family rows next to it hold — under L2 a zero or tiny b-row is otherwise the nearest row of
every row of norm about 1, all of them within the tolerance of each other.
"""
from __future__ import annotations

import numpy as np

DIM = 128
FAMILIES = ("zero", "subnormal", "tiny", "huge", "onehot", "clustered", "mixed", "gauss")
ONEHOT_VALUES = (1.0, 65504.0, 2.0 ** -24, -1.0)
#: the first and last element of a 16-byte piece, the first and last piece of the swizzle
ONEHOT_COLUMNS = (0, 7, 8, 120, 127)
SEARCH_SHAPES = ((257, 385), (513, 641))
METRICS = ("l2", "cosine")

COSINE_TOL = 2e-6        # tests/test_gpu_distance.py: |S - S64| per pair, scale-free
D2_TOL = 4e-6            # the same file: |d² - d64²| <= D2_TOL * (|a_i|² + |b_j|²) per pair
F16_TINY = 2.0 ** -14    # the smallest normal float16
F16_MAX = 65504.0
MARGIN_CAP = 0.9         # the share of a placement's rows whose nearest row must be certain


def _rng(name: str, seed: int, salt: int = 0):
    return np.random.default_rng([FAMILIES.index(name), int(seed), salt])


def _f16(data) -> np.ndarray:
    out = np.asarray(data, dtype=np.float64).astype(np.float16)
    assert out.ndim == 2 and out.shape[1] == DIM and np.all(np.isfinite(out))
    return out


def _directions(rng, count: int) -> np.ndarray:
    data = rng.standard_normal((count, DIM))
    return data / np.linalg.norm(data, axis=1, keepdims=True)


def _signs(rng, shape) -> np.ndarray:
    return rng.integers(0, 2, size=shape) * 2.0 - 1.0


def family(name: str, count: int, seed: int = 0) -> np.ndarray:
    """``count`` rows of family ``name`` (FAMILIES), float16 ``[count, 128]``.  The special rows of
    a family come first, so that any ``count >= 2`` holds them."""
    rng = _rng(name, seed)
    if name == "zero":                    # even rows +0, odd rows -0
        rows = np.zeros((count, DIM))
        rows[1::2] = -0.0
    elif name == "subnormal":             # k * 2^-24, 1 <= |k| <= 1023; row 1: one 2^-24 alone
        rows = rng.integers(1, 1024, size=(count, DIM)) * _signs(rng, (count, DIM)) * 2.0 ** -24
        if count > 1:
            rows[1] = 0.0
            rows[1, int(rng.integers(0, DIM))] = 2.0 ** -24
    elif name == "tiny":                  # 2^-14 <= |x| < 2^-10
        rows = 2.0 ** rng.uniform(-14.0, -10.0, size=(count, DIM)) * _signs(rng, (count, DIM))
        rows = np.sign(rows) * np.clip(np.abs(rows), F16_TINY, 2.0 ** -10)
    elif name == "huge":                  # 16384 <= |x| <= 65504; row 1: 65504 everywhere
        rows = rng.uniform(16384.0, F16_MAX, size=(count, DIM)) * _signs(rng, (count, DIM))
        if count > 1:
            rows[1] = F16_MAX
    elif name == "onehot":                # row r: ONEHOT_VALUES[r % 4] at ONEHOT_COLUMNS[r % 5]:
        rows = np.zeros((count, DIM))     # five rows hold every column and value, twenty every pair
        for r in range(count):
            rows[r, ONEHOT_COLUMNS[r % 5]] = ONEHOT_VALUES[r % 4]
    elif name == "clustered":             # a non-negative base plus noise; rows 2, 5, 8 .. copies
        # ONE base for every seed: the a side and the b side of a call lie in the same cluster
        base = _rng(name, 0, salt=1).uniform(0.25, 1.0, size=DIM)
        rows = np.maximum(base + 0.012 * rng.standard_normal((count, DIM)), 0.0)
        for r in range(2, count, 3):
            rows[r] = rows[r - 2]
    elif name == "mixed":                 # Gaussian directions of norm 2^-18 .. 2^8, shuffled
        # a few rows still span the range: -18 and 8 are among any count >= 2
        exponents = (np.resize(np.arange(-18, 9), count) if count >= 27
                     else np.round(np.linspace(-18, 8, count)).astype(np.int64))
        rng.shuffle(exponents)
        rows = _directions(rng, count) * 2.0 ** exponents[:, None]
    elif name == "gauss":                 # the kind every other device test draws
        rows = _directions(rng, count) * rng.uniform(0.8, 1.25, size=(count, 1))
    else:
        raise ValueError(f"no family {name!r}")
    return _f16(rows)


def positions(count: int, side: str) -> list[int]:
    """Where ``placed`` puts family rows.  a: both sides of the 128- and 256-row block seams
    (top-k / record sweeps and nearest) and the last row.  b: the first tile's ends, the first
    row of the second and third tile — at these sizes every tile is a chunk of its own, so both
    are first rows of later chunks — and the last row, which the shapes of SEARCH_SHAPES leave
    alone in a ragged tile."""
    wanted = (0, 127, 128, 255, 256, count - 1) if side != "b" else (0, 127, 128, 256, count - 1)
    return sorted({p for p in wanted if 0 <= p < count})


def _filler(count: int, seed: int, side: str, twins: int) -> np.ndarray:
    """Gaussian filler whose rows find each other: side a is centre r, side b a noisy copy of
    centre (5 j + 2) % twins (every centre once before any comes twice: 5 divides neither 257
    nor 513), side self a noisy copy of centre r % (count // 2)."""
    centres = _directions(np.random.default_rng([99, int(seed)]), max(twins, count))
    rng = np.random.default_rng([98, int(seed), ("a", "b", "self").index(side)])
    norms = rng.uniform(0.8, 1.25, size=(count, 1))
    if side == "a":
        return centres[:count] * norms
    which = (5 * np.arange(count) + 2) % twins if side == "b" else np.arange(count) % max(count // 2, 1)
    rows = centres[which] + 0.3 * _directions(rng, count)
    return rows / np.linalg.norm(rows, axis=1, keepdims=True) * norms


def placed(name: str, count: int, seed: int = 0, side: str = "a", twins: int | None = None):
    """``(rows, where)``: ``count`` filler rows with rows of family ``name`` at ``positions(count,
    side)``.  ``side`` is "a", "b" (``twins``: the rows of the a side it is searched from) or
    "self" (a matrix searched against itself)."""
    rows = _f16(_filler(count, seed, side, count if twins is None else twins))
    where = positions(count, side)
    rows[where] = family(name, len(where), seed + 1 + ("a", "b", "self").index(side))
    return rows, where


def scaled(rows: np.ndarray, p: int) -> np.ndarray:
    """``rows * 2^p``, exact in float16: no overflow, and no element leaves the normal range."""
    assert rows.dtype == np.float16
    wide = rows.astype(np.float64) * 2.0 ** p
    with np.errstate(over="ignore"):
        out = wide.astype(np.float16)
    assert np.all(np.isfinite(out)) and np.array_equal(out.astype(np.float64), wide)
    assert np.all((out == 0) | (np.abs(wide) >= F16_TINY)), "a new subnormal"
    return out


def in_normal_range(rows: np.ndarray, low: int = -6, high: int = 5) -> np.ndarray:
    """``rows`` with every element that ``scaled(., low)`` or ``scaled(., high)`` could not take
    set to zero (elements below 2^(-14 - low)) — there must be none above."""
    out = rows.copy()
    out[np.abs(out.astype(np.float64)) < F16_TINY * 2.0 ** -low] = 0
    assert np.abs(out.astype(np.float64)).max() * 2.0 ** high <= F16_MAX
    return out


def records(total: int, seed: int, largest: int = 40) -> np.ndarray:
    """Record sizes that sum to ``total``: 1 .. ``largest`` rows, and one record of zero rows."""
    rng = np.random.default_rng([97, int(seed), int(total)])
    counts = []
    while sum(counts) < total:
        counts.append(int(min(rng.integers(1, largest + 1), total - sum(counts))))
    counts.insert(len(counts) // 2, 0)
    return np.asarray(counts, dtype=np.int64)


# ---- the float64 side ----------------------------------------------------------------------------

def unique_rows(b: np.ndarray):
    """``(first, group)``: ``group[j]`` is the lowest index of a row equal to row j element by
    element (+0 equals -0), ``first`` the sorted distinct values of ``group``."""
    canon = (b.astype(np.float32) + 0.0).astype(np.float16)      # -0 + 0 = +0
    seen, group = {}, np.empty(b.shape[0], dtype=np.int64)
    for j in range(b.shape[0]):
        group[j] = seen.setdefault(canon[j].tobytes(), j)
    return np.unique(group), group


def reference(a: np.ndarray, b: np.ndarray, metric: str):
    """``(full, tolerance)``, float64 ``[n, m]`` each: the definition of oracle.gine_numpy per
    pair — cosine S, or the SQUARED L2 distance — and what a device value may differ from it by.
    Equal rows of b get the same column, computed once: no BLAS blocking tells them apart."""
    from oracle import gine_numpy as G
    first, group = unique_rows(b)
    if metric == "cosine":
        full = G.pairwise_cosine(a, b[first])
        tolerance = np.full(full.shape, COSINE_TOL)
    else:
        full = G.pairwise_l2(a, b[first]) ** 2
        tolerance = D2_TOL * ((a.astype(np.float64) ** 2).sum(1)[:, None]
                              + (b[first].astype(np.float64) ** 2).sum(1)[None, :])
    at = np.searchsorted(first, group)
    return np.ascontiguousarray(full[:, at]), np.ascontiguousarray(tolerance[:, at])


def excluded_mask(n: int, m: int, counts=None) -> np.ndarray:
    """bool ``[n, m]``: the pairs a self-search with ``exclude_records=counts`` leaves out."""
    mask = np.zeros((n, m), dtype=bool)
    if counts is not None:
        ptr = np.concatenate(([0], np.cumsum(counts)))
        for lo, hi in zip(ptr[:-1], ptr[1:]):
            mask[lo:hi, lo:hi] = True
    return mask


def ranking(full: np.ndarray, metric: str, gone: np.ndarray | None = None) -> np.ndarray:
    """``full`` as a cost to minimise (cosine negated), excluded pairs at +inf."""
    cost = full.copy() if metric == "l2" else -full
    if gone is not None:
        cost[gone] = np.inf
    return cost


def certain(cost: np.ndarray, tolerance: np.ndarray, columns: np.ndarray, group=None) -> np.ndarray:
    """bool like ``columns`` (int ``[n, k]``, b-rows per a-row, -1 for none): pair (i, columns[i,
    c]) differs from EVERY other candidate pair of row i by more than the two pairs' tolerances
    together, so that no kernel whose values are within the tolerance can rank the two the other
    way round.  With ``group`` (unique_rows) the equal copies of a row count as one candidate."""
    n, k = columns.shape
    out = np.zeros((n, k), dtype=bool)
    rows = np.arange(n)
    for c in range(k):
        j = columns[:, c]
        has = j >= 0
        jj = np.where(has, j, 0)
        with np.errstate(invalid="ignore"):            # inf - inf: an excluded pair, masked below
            gap = np.abs(cost - cost[rows, jj][:, None])
        need = tolerance + tolerance[rows, jj][:, None]
        other = np.isfinite(cost)
        if group is None:
            other[rows, jj] = False
        else:
            other &= group[None, :] != group[jj][:, None]
        out[:, c] = has & np.isfinite(cost[rows, jj]) & np.all((gap > need) | ~other, axis=1)
    return out


def nearest_expected(cost: np.ndarray, tolerance: np.ndarray, group: np.ndarray):
    """``(index, sure)`` per a-row: the lowest index among the copies of its float64 best row, and
    whether that row beats every row that is not a copy of it by more than the tolerances (the
    tie rule names the copy: equal rows have equal keys)."""
    rows = np.arange(cost.shape[0])
    best = np.argmin(cost, axis=1)
    reachable = np.isfinite(cost[rows, best])
    # the lowest copy of the best row that is a candidate (a copy in the row's own record is not)
    copies = (group[None, :] == group[best][:, None]) & np.isfinite(cost)
    index = np.where(reachable, np.argmax(copies, axis=1), best)
    sure = certain(cost, tolerance, index[:, None], group)[:, 0]
    return np.where(reachable, index, -1), sure & reachable


def search_cases():
    """``(name, role, n, m)`` of every search placement: each family as a, as b and as both (the
    control as both), at both SEARCH_SHAPES."""
    for name in FAMILIES:
        for role in (("both",) if name == "gauss" else ("a", "b", "both")):
            for n, m in SEARCH_SHAPES:
                yield name, role, n, m


def search_rows(name: str, role: str, n: int, m: int):
    """``(a, b)`` of a search case: seeds fixed so that MARGIN_CAP holds (asserted on the host)."""
    a, _ = placed(name if role in ("a", "both") else "gauss", n, seed=11, side="a")
    b, _ = placed(name if role in ("b", "both") else "gauss", m, seed=11, side="b", twins=n)
    return a, b


def self_rows(name: str, n: int):
    """``(rows, counts)`` of a self-search case: a placement searched against itself, every row
    skipping its own record."""
    rows, _ = placed(name, n, seed=23, side="self")
    return rows, records(n, 23)


# ---- records for the aligners --------------------------------------------------------------------

#: where zero rows go inside a record of ALIGN_ROWS rows: the first row, the last row, both sides
#: of the 64-row strip seam
ALIGN_ROWS = 97
ZERO_SPOTS = {"first": (0,), "last": (ALIGN_ROWS - 1,), "seam": (63, 64)}
ALIGN_PAIRS = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (2, 1), (3, 1), (4, 1), (2, 2),
               (3, 2), (4, 2))


def align_records(name: str, seed: int = 0):
    """``(rows_a, counts_a, rows_b, counts_b, pairs)``: records for the aligners with rows of
    family ``name`` inside.  Both sides share a 40-row segment (noisy copies), so that there is
    something to align; the family rows sit in it and around it.

    a: three records of ALIGN_ROWS rows with family rows at each of ZERO_SPOTS, one record made
    of family rows only (33 rows), one plain record of 70 rows.  b: a record of 130 rows with
    family rows at its first, its last and rows 31 / 32 (the 32-column block seam), a record of
    family rows only (37 rows), one plain record of 66 rows.  ALIGN_PAIRS: 12 pairs, every
    record in at least one, whole-family against whole-family among them."""
    rng = np.random.default_rng([96, FAMILIES.index(name), int(seed)])
    segment = family("gauss", 40, seed + 50).astype(np.float64)

    def plain(size):
        rows = family("gauss", size, int(rng.integers(1 << 30))).astype(np.float64)
        at = int(rng.integers(0, size - 40 + 1))
        rows[at:at + 40] = segment + 0.02 * rng.standard_normal((40, DIM))
        return _f16(rows)

    def with_family(size, spots):
        rows = plain(size)
        rows[list(spots)] = family(name, len(spots), int(rng.integers(1 << 30)))
        return rows

    rec_a = [with_family(ALIGN_ROWS, ZERO_SPOTS[key]) for key in ("first", "last", "seam")]
    rec_a += [family(name, 33, seed + 7), plain(70)]
    rec_b = [with_family(130, (0, 31, 32, 129)), family(name, 37, seed + 8), plain(66)]
    return (np.concatenate(rec_a), [len(r) for r in rec_a],
            np.concatenate(rec_b), [len(r) for r in rec_b], np.asarray(ALIGN_PAIRS, dtype=np.int32))
