"""Chains of diagonal runs on the GPU (align.chain_runs; gfy_chain_runs_link,
gfy_chain_runs_emit) against the plain-Python definition of tests/chain_runs_oracle.py.  Every
comparison is exact: integer arrays ``==``, weights as bytes.

Hand-made runs are those of tests/hit_runs_oracle.py on the true cells of a boolean matrix, their
values random float32 over many orders of magnitude and both signs, so that a float64 sum added
in another order, or in float32, has other bits."""
from __future__ import annotations

import numpy as np
import pytest

import chain_runs_cases as cases
import chain_runs_oracle as oracle
import hit_runs_oracle
import search_cases

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COUNTS_A = (0, 33, 0, 1, 36)       # 70 rows: the runs of a record's pairs interleave in Runs order
COUNTS_B = (50, 0, 40)             # 90 rows
REACHES = ((0, 0), (1, 1), (3, 1), (8, 8))
LDS_RUNS = 1024                    # kChainLdsRuns: up to here a group's arrays live in LDS


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import _native
    return _native.library()


def _upload(runs):
    from ginfinity_amd import align
    return align.Runs(*(torch.from_numpy(np.ascontiguousarray(part)).cuda() for part in runs))


def _chains(runs, max_gap, max_shift=None, **arguments):
    """``align.chain_runs`` of host runs, with the dtypes and shapes of its result checked."""
    from ginfinity_amd import align
    chains = align.chain_runs(_upload(runs), max_gap=max_gap, max_shift=max_shift, **arguments)
    assert isinstance(chains, align.Chains) and all(part.is_cuda for part in chains)
    assert all(part.dtype == torch.int32 for part in chains[:6] + chains[7:])
    assert chains.weights.dtype == torch.float32
    count = chains.counts.shape[0]
    assert all(part.shape == (count, 2) for part in chains[:4])
    assert chains.lengths.shape == chains.weights.shape == (count,)
    assert chains.members.shape == (runs[2].shape[0],)
    return chains


def _check(runs, max_gap, max_shift=None, want=None):
    """The device, with the early stop and with the plain scan, against the oracle; the
    oracle's result."""
    from ginfinity_amd import align
    want = oracle.chains(*runs, max_gap, max_shift) if want is None else want
    for workspace in (None, align.ChainsWorkspace(plain_scan=True)):
        got = _chains(runs, max_gap, max_shift, workspace=workspace)
        oracle.assert_same(got, want)
        oracle.assert_invariants(got, runs)
    return want


def _runs_of(matrix, counts_a, counts_b=None, min_length=1, seed=0):
    return hit_runs_oracle.runs(*hit_runs_oracle.hits_of(matrix, seed=seed), counts_a, counts_b,
                                min_length)


@pytest.fixture(scope="module")
def one_pair_runs():
    """About 1,270 runs of one record pair, with forks and ties: more than LDS_RUNS."""
    runs = _runs_of(np.random.default_rng(31).random((60, 80)) < 0.5, (60,), (80,), seed=31)
    assert runs[2].size > LDS_RUNS + 1
    return runs


# --------------------------------------------------------------------------------------------
# 1. grouping across pairs

@pytest.mark.parametrize("seed", (11, 12, 13))
def test_runs_of_interleaved_pairs_are_grouped(seed):
    matrix = np.random.default_rng(seed).random((70, 90)) < 0.5
    for min_length in (1, 2):
        runs = _runs_of(matrix, COUNTS_A, COUNTS_B, min_length, seed)
        pairs = runs[0].astype(np.int64)
        key = pairs[:, 0] * 3 + pairs[:, 1]
        # six pairs, interleaved; the one-row record's runs have length 1
        assert np.unique(key).size == (6 if min_length == 1 else 4) and np.any(np.diff(key) < 0)
        for max_gap, max_shift in REACHES:
            got = _check(runs, max_gap, max_shift)
            assert np.array_equal(got[0], runs[0][np.unique(got[7], return_index=True)[1]])
            if max_gap == 0:
                assert got[4].size == runs[2].size
            else:
                assert got[4].max() > 1 and got[4].size < runs[2].size


# --------------------------------------------------------------------------------------------
# 2. more than one stride of the lanes, a long serial chain, both homes of a group's arrays

def test_every_cell_a_hit_links_nothing():
    """599 runs of one pair, each to the matrix's edge: nothing can follow any of them."""
    runs = _runs_of(np.ones((300, 300), dtype=bool), (300,), seed=2)
    assert runs[2].size == 599
    for max_gap, max_shift in ((1, 1), (8, 8)):
        got = _check(runs, max_gap, max_shift)
        assert got[4].size == 599 and np.array_equal(got[7], np.arange(599))


def test_one_chain_of_1365_runs():
    size = 4_096
    thinned = np.eye(size, dtype=bool)
    thinned[np.arange(0, size, 3), np.arange(0, size, 3)] = False
    runs = _runs_of(thinned, (size,), seed=4)
    assert runs[2].size == 1_365 and np.all(runs[2] == 2)
    pairs, starts, ends, diagonals, counts, lengths, _, members = _check(runs, 1)
    assert pairs.tolist() == [[0, 0]] and starts.tolist() == [[1, 1]]
    # cells 0, 3, .., 4095 are gone: the first run is (1, 2), the last (4093, 4094)
    assert ends.tolist() == [[size - 2, size - 2]] and diagonals.tolist() == [[0, 0]]
    assert counts.tolist() == [1_365] and lengths.tolist() == [2_730] and not members.any()
    apart = _check(runs, 0)
    assert apart[4].size == 1_365 and np.array_equal(apart[1], runs[1])
    assert apart[6].tobytes() == runs[3].tobytes()


@pytest.mark.parametrize("count", (LDS_RUNS, LDS_RUNS + 1, None))
def test_a_group_just_under_and_just_over_the_lds_limit(one_pair_runs, count):
    """A subset of a ``Runs`` in its order is a ``Runs``: the first 1,024 runs of the pair live
    in LDS, the first 1,025 and all of them in the workspace."""
    runs = tuple(part[:count] for part in one_pair_runs)
    got = _check(runs, 3, 2)
    assert got[4].max() > 2 and (got[3][:, 0] != got[3][:, 1]).any()


# --------------------------------------------------------------------------------------------
# 3. limits exactly

@pytest.mark.parametrize("name", cases.CASES)
def test_hand_written_limits_forks_and_ties(name):
    entries, max_gap, max_shift, expected = cases.CASES[name]
    _check(cases.runs_of(entries), max_gap, max_shift, want=cases.chains_of(expected))


def test_no_runs_and_runs_on_the_host():
    from ginfinity_amd import align
    none = cases.runs_of([])
    empty = oracle.chains(*none, 3)
    assert all(part.shape[0] == 0 for part in empty)
    oracle.assert_same(_chains(none, 3), empty)
    host = cases.runs_of(cases.FORK)
    moved = align.chain_runs(host, max_gap=3)
    assert all(part.is_cuda for part in moved)
    oracle.assert_same(moved, cases.chains_of(cases.CASES["fork"][3]))
    # a reach beyond int32 is the widest reach
    oracle.assert_same(align.chain_runs(host, max_gap=2 ** 40, max_shift=2 ** 35),
                       oracle.chains(*host, 2 ** 40, 2 ** 35))


# --------------------------------------------------------------------------------------------
# 4. refusals that need the data

def test_refusals_that_need_the_data_launch_nothing(monkeypatch):
    from ginfinity_amd import align
    matrix = np.random.default_rng(11).random((70, 90)) < 0.5
    runs = _runs_of(matrix, COUNTS_A, COUNTS_B, seed=11)

    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)

    def changed(which, position, value):
        parts = [part.copy() for part in runs]
        parts[which][position] = value
        return tuple(parts)
    swapped = tuple(part.copy() for part in runs)
    for part in swapped:
        part[[10, 11]] = part[[11, 10]]
    best = align.Runs(*map(torch.from_numpy, runs)).best(runs[2].size)
    assert not np.array_equal(best, np.arange(runs[2].size))
    huge = cases.runs_of([(0, 0, 0, 0, 2 ** 30), (0, 0, 2 ** 30, 2 ** 30, 2 ** 30)])
    bad = {"a length of 0": changed(2, 7, 0),
           "a negative length": changed(2, 7, -3),
           "a negative cell": changed(1, (5, 1), -1),
           "a negative pair": changed(0, (0, 0), -1),
           "two runs swapped": swapped,
           "a run twice": tuple(np.concatenate([part[:5], part[4:]]) for part in runs),
           "a best() permutation": tuple(part[best] for part in runs),
           "lengths that sum to 2^31": huge}
    assert int(huge[2].astype(np.int64).sum()) == 2 ** 31
    for name, parts in bad.items():
        with pytest.raises(ValueError, match="not those of hit_runs"):
            align.chain_runs(_upload(parts), max_gap=2)
    monkeypatch.undo()
    oracle.assert_same(align.chain_runs(_upload(runs), max_gap=2), oracle.chains(*runs, 2))
    # one hit fewer and the same two runs pass
    fits = cases.runs_of([(0, 0, 0, 0, 2 ** 30), (0, 0, 2 ** 30, 2 ** 30, 2 ** 30 - 1)])
    got = _check(fits, 0)
    assert got[5].tolist() == [2 ** 31 - 1] and got[2].tolist() == [[2 ** 31 - 2, 2 ** 31 - 2]]


# --------------------------------------------------------------------------------------------
# 5. behind the real chain: search, runs, chains, banded alignment

def test_behind_the_real_chain():
    """Record 2 is record 0's rows 10..69 without rows 40..42: a deletion of three rows cuts the
    shared region into two runs three diagonals apart, and the chain is the region again."""
    from ginfinity_amd import align, distance
    counts = (120, 80, 57)
    data = np.random.default_rng(7).standard_normal((200, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    rows = data.astype(np.float16)
    rows = torch.from_numpy(np.concatenate([rows, rows[10:40], rows[43:70]])).cuda()
    hits = distance.within(rows, threshold=0.99, metric="cosine", exclude_records=counts)
    runs = align.hit_runs(hits, counts_a=counts)
    host = tuple(part.cpu().numpy() for part in runs)
    found = [(*pair, *cell, length) for pair, cell, length in
             zip(host[0].tolist(), host[1].tolist(), host[2].tolist())]
    assert [entry for entry in found if entry[:2] == (2, 0)] == [(2, 0, 0, 10, 30),
                                                                 (2, 0, 30, 43, 27)]
    chains = align.chain_runs(runs, max_gap=4)
    oracle.assert_same(chains, oracle.chains(*host, 4))
    oracle.assert_invariants(chains, host)
    there = [c for c, pair in enumerate(chains.pairs.tolist()) if pair == [2, 0]]
    assert len(there) == 1
    at = there[0]
    assert chains.counts[at].item() == 2 and chains.lengths[at].item() == 57
    assert chains.starts[at].tolist() == [0, 10] and chains.ends[at].tolist() == [56, 69]
    assert chains.diagonals[at].tolist() == [10, 13]
    members = np.flatnonzero(chains.members.cpu().numpy() == at)
    assert [found[s] for s in members] == [(2, 0, 0, 10, 30), (2, 0, 30, 43, 27)]
    assert at in chains.best(2).tolist() and chains.bands(0)[at].tolist() == [10, 13]
    # with max_gap = 2 the deletion of three rows is out of reach
    assert (align.chain_runs(runs, max_gap=2).counts == 1).all()
    # the chain as a seed: alignment inside its band alone finds the score of the whole matrix,
    # inside either run's diagonal alone a strictly lower one
    scale, shift, gap_open, gap_extend = search_cases.PARAMETERS[0]
    gaps = dict(counts_a=counts, pairs=chains.pairs[at:at + 1], gap_open=gap_open,
                gap_extend=gap_extend, match_scale=scale, match_shift=shift)
    banded, banded_end = align.local_align(rows, band=chains.bands(0)[at:at + 1], **gaps)
    whole, whole_end = align.local_align(rows, **gaps)
    assert banded.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    assert banded_end.tolist() == whole_end.tolist() == [[56, 69]]
    for s in members:
        single, _ = align.local_align(rows, band=runs.bands(0)[s:s + 1], **gaps)
        assert float(single) < float(whole)


# --------------------------------------------------------------------------------------------
# 6. determinism

def test_the_same_bytes_from_call_to_call(one_pair_runs):
    from ginfinity_amd import align
    matrix = np.random.default_rng(12).random((70, 90)) < 0.5
    small = _upload(_runs_of(matrix, COUNTS_A, COUNTS_B, seed=12))
    large = _upload(one_pair_runs)
    workspace = align.ChainsWorkspace()
    for runs in (large, small, large):               # a reused workspace grows and is reused
        first = align.chain_runs(runs, max_gap=3, max_shift=2)
        again = align.chain_runs(runs, max_gap=3, max_shift=2)
        kept = align.chain_runs(runs, max_gap=3, max_shift=2, workspace=workspace)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            other = align.chain_runs(runs, max_gap=3, max_shift=2, workspace=workspace)
        stream.synchronize()
        torch.cuda.current_stream().wait_stream(stream)
        for repeat in (again, kept, other):
            for one, two in zip(first, repeat):
                assert one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes()
