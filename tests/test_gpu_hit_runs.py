"""Seeds from radius-search hits on the GPU (align.hit_runs; gfy_hit_runs_mark,
gfy_hit_runs_emit): the maximal diagonal runs of a ``Hits``, against the plain-Python definition
of tests/hit_runs_oracle.py.  Every comparison is exact: integer arrays ``==``, weights as bytes.

Hand-made hits are the true cells of a boolean matrix (``np.nonzero``), their values random
float32 over many orders of magnitude and both signs, so that a float64 sum added in another
order, or in float32, has other bits."""
from __future__ import annotations

import numpy as np
import pytest

import hit_runs_oracle as oracle
import search_cases

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COUNTS_A = (0, 33, 0, 1, 36)       # 70 rows: empty records in front, in the middle, by a 1-row one
COUNTS_B = (50, 0, 40)             # 90 rows
SELF_COUNTS = (0, 33, 0, 1, 36)    # 70 x 70: the main diagonal meets both boundaries in one step


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


def _upload(hits):
    from ginfinity_amd import distance
    return distance.Hits(*(torch.from_numpy(np.ascontiguousarray(part)).cuda() for part in hits))


def _runs(hits, **arguments):
    """``align.hit_runs`` of host hits, with the dtypes and shapes of its result checked."""
    from ginfinity_amd import align
    runs = align.hit_runs(_upload(hits), **arguments)
    assert isinstance(runs, align.Runs) and all(part.is_cuda for part in runs)
    assert runs.pairs.dtype == runs.cells.dtype == runs.lengths.dtype == torch.int32
    assert runs.weights.dtype == torch.float32
    count = runs.lengths.shape[0]
    assert runs.pairs.shape == runs.cells.shape == (count, 2) and runs.weights.shape == (count,)
    return runs


def _check(hits, counts_a, counts_b=None, min_length=1):
    """The device against the oracle; the oracle's result."""
    want = oracle.runs(*hits, counts_a, counts_b, min_length)
    oracle.assert_same(_runs(hits, counts_a=counts_a, counts_b=counts_b, min_length=min_length),
                       want)
    return want


def _dense(seed, rows, cols, diagonal=False):
    matrix = np.random.default_rng(seed).random((rows, cols)) < 0.5
    if diagonal:
        matrix |= np.eye(rows, cols, dtype=bool)
    return oracle.hits_of(matrix, seed=seed)


@pytest.fixture(scope="module")
def boundary_hits():
    return _dense(11, 70, 90)


# --------------------------------------------------------------------------------------------
# 1. boundaries

@pytest.mark.parametrize("seed", (11, 12, 13))
def test_runs_split_at_every_record_boundary(seed):
    hits = _dense(seed, 70, 90)
    pairs, cells, lengths, _ = _check(hits, COUNTS_A, COUNTS_B)
    assert lengths.sum() == hits[1].size
    rows_a, rows_b = np.asarray(COUNTS_A)[pairs[:, 0]], np.asarray(COUNTS_B)[pairs[:, 1]]
    assert np.all(cells >= 0) and np.all(cells[:, 0] + lengths <= rows_a)
    assert np.all(cells[:, 1] + lengths <= rows_b)            # no run leaves its two records
    assert not np.isin(pairs[:, 0], (0, 2)).any() and not (pairs[:, 1] == 1).any()
    assert {1, 3, 4} == set(pairs[:, 0].tolist()) and {0, 2} == set(pairs[:, 1].tolist())
    # a row on a boundary belongs to the record that starts there: rows 33 and 34 of a, 50 of b
    assert ((pairs[:, 0] == 3) & (cells[:, 0] == 0)).any()
    assert ((pairs[:, 1] == 2) & (cells[:, 1] == 0)).any()
    # the one-row record splits every diagonal through it: its runs have length 1
    assert np.all(lengths[pairs[:, 0] == 3] == 1)


def test_self_search_shape_diagonal_crosses_both_boundaries_in_one_step():
    hits = _dense(21, 70, 70, diagonal=True)
    pairs, cells, lengths, _ = _check(hits, SELF_COUNTS)
    main = (pairs[:, 0] == pairs[:, 1]) & (cells[:, 0] == 0) & (cells[:, 1] == 0)
    assert pairs[main, 0].tolist() == [1, 3, 4] and lengths[main].tolist() == [33, 1, 36]
    # counts_b omitted is counts_b = counts_a
    oracle.assert_same(_runs(hits, counts_a=SELF_COUNTS, counts_b=SELF_COUNTS),
                       oracle.runs(*hits, SELF_COUNTS, SELF_COUNTS))


# --------------------------------------------------------------------------------------------
# 2. every cell a hit

def test_every_cell_a_hit():
    hits = oracle.hits_of(np.ones((300, 300), dtype=bool), seed=2)
    pairs, cells, lengths, _ = _check(hits, (300,))
    assert lengths.size == 599 and lengths.max() == 300 and lengths.sum() == 90_000
    assert np.all((cells[:, 0] == 0) | (cells[:, 1] == 0))    # heads: the first row and column
    pairs, cells, lengths, _ = _check(hits, (130, 170), (64, 236))
    assert lengths.sum() == 90_000
    assert lengths.size == (130 + 64 - 1) + (130 + 236 - 1) + (170 + 64 - 1) + (170 + 236 - 1)
    assert lengths.max() == 170


# --------------------------------------------------------------------------------------------
# 3. the longest walk

def test_the_longest_walk():
    size = 4_096
    hits = oracle.hits_of(np.eye(size, dtype=bool), seed=3)
    pairs, cells, lengths, _ = _check(hits, (size,))
    assert pairs.tolist() == [[0, 0]] and cells.tolist() == [[0, 0]] and lengths.tolist() == [size]
    pairs, cells, lengths, _ = _check(hits, (size - 1, 1), (size,))
    assert pairs.tolist() == [[0, 0], [1, 0]] and cells.tolist() == [[0, 0], [0, size - 1]]
    assert lengths.tolist() == [size - 1, 1]
    thinned = np.eye(size, dtype=bool)
    thinned[np.arange(0, size, 3), np.arange(0, size, 3)] = False
    hits = oracle.hits_of(thinned, seed=4)
    pairs, cells, lengths, _ = _check(hits, (size,))
    assert lengths.size == size // 3 and np.all(lengths == 2)
    assert np.array_equal(cells[:, 0], np.arange(1, size - 1, 3))


# --------------------------------------------------------------------------------------------
# 4. empty segments

def test_rows_without_hits_first_last_and_inside_a_diagonal():
    matrix = np.random.default_rng(41).random((9, 9)) < 0.5
    matrix[[3, 5], [3, 5]] = True
    matrix[[1, 2, 6, 7], [1, 2, 6, 7]] = False
    matrix[[0, 4, 8]] = False
    hits = oracle.hits_of(matrix, seed=41)
    assert hits[0][1] == 0 and hits[0][4] == hits[0][5] and hits[0][8] == hits[0][9]
    pairs, cells, lengths, _ = _check(hits, (9,))
    on_main = cells[:, 0] == cells[:, 1]
    assert cells[on_main, 0].tolist() == [3, 5] and lengths[on_main].tolist() == [1, 1]
    _check(hits, (2, 3, 4), (5, 4))


def test_no_hits_and_no_rows():
    from ginfinity_amd import align
    none = (np.zeros(8, dtype=np.int64), np.zeros(0, dtype=np.int32),
            np.zeros(0, dtype=np.float32))
    empty = oracle.runs(*none, (3, 4))
    assert all(part.shape[0] == 0 for part in empty)
    oracle.assert_same(_runs(none, counts_a=(3, 4)), empty)
    oracle.assert_same(_runs(none, counts_a=(3, 4), counts_b=(5,), min_length=3), empty)
    rowless = (np.zeros(1, dtype=np.int64), none[1], none[2])
    oracle.assert_same(_runs(rowless, counts_a=()), empty)
    oracle.assert_same(_runs(rowless, counts_a=(0, 0), counts_b=(4,)), empty)
    # hits on the host are moved to the device
    host = oracle.hits_of(np.eye(3, dtype=bool), seed=5)
    moved = align.hit_runs(tuple(host), counts_a=(3,))
    assert all(part.is_cuda for part in moved)
    oracle.assert_same(moved, oracle.runs(*host, (3,)))


# --------------------------------------------------------------------------------------------
# 5. min_length

def test_min_length_filters_the_runs_of_min_length_one(boundary_hits):
    from ginfinity_amd import align
    full = oracle.runs(*boundary_hits, COUNTS_A, COUNTS_B)
    longest = int(full[2].max())
    assert longest >= 5
    workspace = align.RunsWorkspace()
    for min_length in (1, 2, 5, longest + 1):
        keep = full[2] >= min_length
        want = tuple(part[keep] for part in full)
        oracle.assert_same(_runs(boundary_hits, counts_a=COUNTS_A, counts_b=COUNTS_B,
                                 min_length=min_length, workspace=workspace), want)
        oracle.assert_same(oracle.runs(*boundary_hits, COUNTS_A, COUNTS_B, min_length), want)
    assert not keep.any()


def test_one_workspace_on_a_large_a_small_and_a_large_input(boundary_hits):
    """The second call uses nine entries of buffers that hold some 3,000 marks and slots of the
    first: anything read beyond the call's own length would show there, anything left behind by
    it in the third."""
    from ginfinity_amd import align
    from test_hit_runs_host import PATTERN, VALUES
    large = (boundary_hits, COUNTS_A, COUNTS_B, oracle.runs(*boundary_hits, COUNTS_A, COUNTS_B))
    small_hits = oracle.hits_of(PATTERN, VALUES)
    small = (small_hits, (7,), None, oracle.runs(*small_hits, (7,)))
    assert small_hits[1].size == 9 and boundary_hits[1].size > 2_000
    workspace = align.RunsWorkspace()
    for hits, counts_a, counts_b, want in (large, small, large):
        kept = _runs(hits, counts_a=counts_a, counts_b=counts_b, workspace=workspace)
        fresh = _runs(hits, counts_a=counts_a, counts_b=counts_b)
        for first, second in zip(kept, fresh):
            assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
        oracle.assert_same(kept, want)
        assert workspace.marks.numel() >= boundary_hits[1].size     # grown once, never shrunk


# --------------------------------------------------------------------------------------------
# 6. behind the real searcher

def test_behind_the_real_searcher():
    from ginfinity_amd import align, distance
    counts = (120, 80, 40)
    data = np.random.default_rng(6).standard_normal((200, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    rows = data.astype(np.float16)
    rows = torch.from_numpy(np.concatenate([rows, rows[10:50]])).cuda()
    hits = distance.within(rows, threshold=0.99, metric="cosine", exclude_records=counts)
    host = tuple(part.cpu().numpy() for part in hits)
    runs = align.hit_runs(hits, counts_a=counts)
    oracle.assert_same(runs, oracle.runs(*host, counts))
    found = [(*pair, *cell, length) for pair, cell, length in
             zip(runs.pairs.tolist(), runs.cells.tolist(), runs.lengths.tolist())]
    assert (2, 0, 0, 10, 40) in found and (0, 2, 10, 0, 40) in found
    assert sum(entry[:2] == (2, 0) for entry in found) == 1
    # the run as a seed: alignment on its diagonal alone finds the score of the whole matrix
    at = found.index((2, 0, 0, 10, 40))
    scale, shift, gap_open, gap_extend = search_cases.PARAMETERS[0]
    gaps = dict(counts_a=counts, pairs=runs.pairs[at:at + 1], gap_open=gap_open,
                gap_extend=gap_extend, match_scale=scale, match_shift=shift)
    band = runs.bands(0)[at:at + 1]
    assert band.tolist() == [[10, 10]]
    banded, banded_end = align.local_align(rows, band=band, **gaps)
    whole, whole_end = align.local_align(rows, **gaps)
    assert banded.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    assert banded_end.tolist() == whole_end.tolist() == [[39, 49]] and float(whole) > 20.0
    assert runs.best(2).tolist() == sorted(
        range(len(found)), key=lambda s: (-found[s][4], -float(runs.weights[s]), s))[:2]
    # the same bytes from call to call and from another stream
    again = align.hit_runs(hits, counts_a=counts)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = align.hit_runs(hits, counts_a=counts)
    stream.synchronize()
    for repeat in (again, other):
        for first, second in zip(runs, repeat):
            assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()


# --------------------------------------------------------------------------------------------
# 7. refusals that need the data

def test_refusals_that_need_the_data_launch_nothing(monkeypatch, boundary_hits):
    from ginfinity_amd import align
    offsets, indices, values = boundary_hits

    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)

    def changed(array, position, value):
        array = array.copy()
        array[position] = value
        return array
    swapped = offsets.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    bad = {"offsets[0] != 0": (changed(offsets, 0, 1), indices),
           "offsets[0] < 0": (changed(offsets, 0, -1), indices),
           "offsets decrease": (swapped, indices),
           "offsets[-1] < H": (changed(offsets, -1, offsets[-1] - 1), indices),
           "offsets[-1] > H": (changed(offsets, -1, offsets[-1] + 1), indices),
           "an index < 0": (offsets, changed(indices, 7, -1)),
           "an index == m": (offsets, changed(indices, indices.size - 1, 90)),
           "an index far out": (offsets, changed(indices, 100, 2 ** 31 - 1))}
    assert offsets[10] != offsets[11]
    for name, (bad_offsets, bad_indices) in bad.items():
        with pytest.raises(ValueError, match="not those of a search"):
            align.hit_runs(_upload((bad_offsets, bad_indices, values)), counts_a=COUNTS_A,
                           counts_b=COUNTS_B)
    # m comes from counts_b: hits of 90 columns against 89 rows of b
    with pytest.raises(ValueError, match="not those of a search"):
        align.hit_runs(_upload(boundary_hits), counts_a=COUNTS_A, counts_b=(50, 0, 39))
    monkeypatch.undo()
    oracle.assert_same(align.hit_runs(_upload(boundary_hits), counts_a=COUNTS_A,
                                      counts_b=COUNTS_B),
                       oracle.runs(*boundary_hits, COUNTS_A, COUNTS_B))
