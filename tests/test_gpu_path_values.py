"""The values along aligned paths on the device (align.path_values, gfy_align_path_values)
against the dense kernel and the oracle of tests/path_values_oracle.py, byte for byte.

The contract: at an op 0 at cell (i, j) ``cosines`` holds ``distance.pairwise(A, B, "cosine")[i, j]``
of the pair's two records bit for bit, and everything else is the oracle's sequential float32 /
float64 arithmetic on those cosines.  So every test takes the device's own dense ``C`` of a pair
(computed once per case, read-only), runs the oracle on it and compares bytes.

    1  hand-made paths inside two records of 140 rows, several records per side: lengths on the
       edges of the 32-op product and the 64-op block, gap runs across both seams, a leading gap
       run, the last cell of both records, a trailing gap run behind the last row of A
    2  paths of every aligner on planted pairs: ``scores`` is the aligner's score
    3  a path's values do not depend on its company, on the order, or on ``max_waves``
    4  zero rows, fp16 subnormals and rows near the fp16 maximum (tests/value_cases.py)
    5  refusals: one path per kind among good ones
    6  the cosines against the float64 definition, within the tolerance of tests/test_gpu_align.py

The grid is given fewer waves than paths (``max_waves``) so that waves take paths in turn."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import align_oracle as O
import path_values_oracle as VO
import value_cases as V
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_align.py
#: (match_scale, match_shift, gap_open, gap_extend)
PARAMETERS = ((1.0, -0.3, 1.0, 0.25), (1.5, 0.2, 0.75, 0.75))
ROWS = 140
COUNTS_A = (17, ROWS, 5)
COUNTS_B = (9, ROWS, 3)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


def _bits(value) -> bytes:
    return np.ascontiguousarray(value).tobytes()


class _Case:
    """Rows, records and pairs on the device, and the device's own dense C of every pair."""

    def __init__(self, a, counts_a, b, counts_b):
        self.a, self.b = a, b
        self.counts_a, self.counts_b = list(counts_a), list(counts_b)
        self.a_dev, self.b_dev = _device(a), _device(b)
        self.ptr_a = np.concatenate(([0], np.cumsum(counts_a)))
        self.ptr_b = np.concatenate(([0], np.cumsum(counts_b)))
        self._dense = {}

    def rows(self, q, r):
        return (self.a[self.ptr_a[q]:self.ptr_a[q + 1]], self.b[self.ptr_b[r]:self.ptr_b[r + 1]])

    def dense(self, q, r):
        if (q, r) not in self._dense:
            C = distance.pairwise(self.a_dev[self.ptr_a[q]:self.ptr_a[q + 1]],
                                  self.b_dev[self.ptr_b[r]:self.ptr_b[r + 1]],
                                  metric="cosine").cpu().numpy()
            C.setflags(write=False)
            self._dense[(q, r)] = C
        return self._dense[(q, r)]

    def call(self, function, parameters, pairs, *front, **more):
        scale, shift, go, ge = parameters
        return function(*front, self.a_dev, self.b_dev, counts_a=self.counts_a,
                        counts_b=self.counts_b, pairs=pairs, gap_open=go, gap_extend=ge,
                        match_scale=scale, match_shift=shift, **more)


def _as_paths(paths):
    """``(pair, start, ops)`` per path as the object ``path_values`` takes, host arrays."""
    lengths = [len(ops) for _, _, ops in paths]
    return (np.array([pair for pair, _, _ in paths], dtype=np.int32).reshape(-1, 2),
            SimpleNamespace(starts=np.array([start for _, start, _ in paths], dtype=np.int32).reshape(-1, 2),
                            ops=np.array([op for _, _, ops in paths for op in ops], dtype=np.uint8),
                            offsets=np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)))


def _host(values):
    return align.PathValues(*(t.cpu().numpy() for t in values))


def _assert_path(case, got, p, pair, start, ops, parameters, where=None):
    """Path p of ``got`` (host arrays) is the oracle's on the device's dense C, byte for byte."""
    cosines, running, score, counts, total = VO.values_of(case.dense(*pair), ops, start, *parameters)
    lo, hi = int(got.offsets[p]), int(got.offsets[p + 1])
    where = (where, p, pair, start, len(ops))
    assert hi - lo == len(ops), where
    assert got.status[p] == 0, where
    assert _bits(got.cosines[lo:hi]) == _bits(cosines), where
    assert np.array_equal(np.isnan(got.cosines[lo:hi]), np.asarray(ops) != 0), where
    assert _bits(got.running[lo:hi]) == _bits(running), where
    assert _bits(got.scores[p]) == _bits(score), where
    assert (int(got.matches[p]), *got.gap_runs[p].tolist()) == counts, where
    assert got.cosine_sums.dtype == np.float64 and _bits(got.cosine_sums[p]) == _bits(total), where


@functools.lru_cache(maxsize=None)
def _hand_case():
    rng = np.random.default_rng(20261021)

    def unit(count):
        rows = rng.standard_normal((count, 128))
        return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float16)
    return _Case(unit(sum(COUNTS_A)), COUNTS_A, unit(sum(COUNTS_B)), COUNTS_B)


def _hand_paths():
    big, small = (1, 1), (2, 0)
    paths = [(big, (3 + n % 5, 5 + n % 3), [0] * n) for n in (1, 31, 32, 33, 63, 64, 65, 129)]
    paths += [
        (big, (2, 7), [0] * 30 + [1] * 4 + [0] * 10),                 # a gap run across op 31 | 32
        (big, (9, 1), [0] * 61 + [2] * 5 + [0] * 20),                 # a gap run across op 63 | 64
        (big, (0, 0), [2] * 3 + [0] * 20 + [1] * 2),                  # starts in a gap run (global)
        (big, (ROWS - 40, ROWS - 40), [0] * 40),                      # ends at the last cell of both
        (big, (130, 120), [0] * 10 + [1] * 10),                       # gaps behind the last row of A
        (big, (120, 135), [0] * 5 + [2] * 15),                        # gaps behind the last row of B
        (big, (5, 5), [1, 2, 1, 2, 2, 1, 0, 2, 1] * 8),               # every gap op a new run
        (big, (40, 2), [0, 0, 1, 0, 2, 2, 0, 1, 1, 1] * 9),           # 90 ops, all kinds mixed
        (big, (-1, -1), []),                                          # nothing aligned
        (big, (7, 7), []),
        (small, (0, 0), [0] * 3),                                     # records 5 x 9
        (small, (1, 2), [0, 1, 0, 2, 0, 1, 1]),
        ((0, 1), (16, 139), [0]),                                     # the last cell of 17 x 140
    ]
    return paths


@pytest.mark.parametrize("waves", (None, 3))
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_hand_made_paths_equal_the_dense_kernel_and_the_oracle(parameters, waves):
    case, paths = _hand_case(), _hand_paths()
    assert {len(ops) for _, _, ops in paths} >= {1, 31, 32, 33, 63, 64, 65, 129}
    pairs, given = _as_paths(paths)
    got = _host(case.call(align.path_values, parameters, pairs, given, max_waves=waves))
    assert _bits(got.offsets) == _bits(given.offsets)
    for p, (pair, start, ops) in enumerate(paths):
        _assert_path(case, got, p, pair, start, ops, parameters, waves)


# ---- 2: the paths of every aligner -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _family_case(name):
    a, counts_a, b, counts_b, pairs = V.align_records(name)
    return _Case(a, counts_a, b, counts_b), pairs


def _aligners(case, pairs, parameters):
    """(name, AlignedPaths) of the six calls that return paths."""
    _, ends = case.call(align.local_align, parameters, pairs)
    band = align.band_around(np.maximum(ends.cpu().numpy(), 0), 8)
    box = (10, 80, 5, 100)
    yield "local", case.call(align.local_paths, parameters, pairs)
    yield "band", case.call(align.local_paths, parameters, pairs, band=band)
    yield "box", case.call(align.local_paths, parameters, pairs, box=box)
    yield "global", case.call(align.global_paths, parameters, pairs, within=False)
    yield "within", case.call(align.global_paths, parameters, pairs, within=True)
    yield "global box", case.call(align.global_paths, parameters, pairs, within=False, box=box)
    yield "within box", case.call(align.global_paths, parameters, pairs, within=True, box=box)


@pytest.mark.parametrize("name", ("gauss", "zero"))
def test_the_score_of_every_aligners_path_is_the_aligners_score(name):
    case, pairs = _family_case(name)
    parameters = PARAMETERS[0]
    empty = walked = 0
    for which, paths in _aligners(case, pairs, parameters):
        got = _host(case.call(align.path_values, parameters, pairs, paths, max_waves=5))
        scores, ops, offsets = (t.cpu().numpy() for t in (paths.scores, paths.ops, paths.offsets))
        assert got.offsets.tolist() == offsets.tolist() and not got.status.any(), which
        for p in range(len(pairs)):
            mine = ops[offsets[p]:offsets[p + 1]]
            where = (name, which, tuple(pairs[p]))
            # byte for byte; where both are zero the sign is free (tests/test_gpu_align_ties.py)
            assert _bits(got.scores[p]) == _bits(scores[p]) or (got.scores[p] == 0 and scores[p] == 0), where
            assert got.matches[p] + np.count_nonzero(mine) == mine.size, where
            if mine.size == 0:
                assert scores[p] == 0 and _bits(got.scores[p]) == _bits(np.float32(0)), where
                assert got.matches[p] == 0 and not got.gap_runs[p].any(), where
                assert got.cosine_sums[p] == 0, where
                empty += 1
            elif which in ("local", "within"):
                start = tuple(paths.starts[p].tolist())
                _assert_path(case, got, p, tuple(pairs[p]), start, mine, parameters, which)
                walked += 1
    assert walked >= 12 and (name != "zero" or empty > 0)


# ---- 3: independence of company ----------------------------------------------------------------

def test_a_paths_values_do_not_depend_on_company_order_or_waves():
    case = _hand_case()
    parameters = PARAMETERS[0]
    rng = np.random.default_rng(3)
    chosen = ((1, 1), (9, 1), [0] * 61 + [2] * 5 + [0] * 20)
    crowd = []
    for _ in range(300):
        length = int(rng.integers(1, 41))
        kinds = rng.choice([0, 0, 0, 1, 2], size=length).tolist()
        crowd.append(((1, 1), (int(rng.integers(0, 60)), int(rng.integers(0, 60))), kinds))

    def values_at(paths, at, waves):
        pairs, given = _as_paths(paths)
        got = _host(case.call(align.path_values, parameters, pairs, given, max_waves=waves))
        assert not got.status.any()
        lo, hi = int(got.offsets[at]), int(got.offsets[at + 1])
        return (_bits(got.cosines[lo:hi]), _bits(got.running[lo:hi]), _bits(got.scores[at]),
                int(got.matches[at]), got.gap_runs[at].tolist(), _bits(got.cosine_sums[at]))

    alone = values_at([chosen], 0, None)
    assert alone[3:5] == (81, [0, 1])
    middle = crowd[:150] + [chosen] + crowd[150:]
    assert values_at(middle, 150, None) == alone
    assert values_at(middle, 150, 7) == alone              # 301 paths on 7 waves: 43 turns
    assert values_at(middle[::-1], 150, 64) == alone
    assert values_at([chosen] + crowd, 0, 1) == alone      # one wave walks them all
    # and the crowd itself is right: a few of its paths against the oracle
    pairs, given = _as_paths(middle)
    got = _host(case.call(align.path_values, parameters, pairs, given, max_waves=7))
    for p in (0, 1, 149, 151, 299, 300):
        _assert_path(case, got, p, *middle[p], parameters)


# ---- 4: the value range ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("zero", "subnormal", "huge"))
def test_zero_tiny_and_huge_rows_still_give_the_dense_kernels_bytes(name):
    case, pairs = _family_case(name)
    parameters = PARAMETERS[0]
    matched_family = 0
    for within in (False, True):
        paths = case.call(align.global_paths, parameters, pairs, within=within)
        got = _host(case.call(align.path_values, parameters, pairs, paths))
        starts, ops, offsets = (t.cpu().numpy() for t in (paths.starts, paths.ops, paths.offsets))
        for p in range(len(pairs)):
            mine = ops[offsets[p]:offsets[p + 1]]
            _assert_path(case, got, p, tuple(pairs[p]), tuple(starts[p]), mine, parameters, within)
        # the whole-family records against each other: every matched cell holds family rows
        whole = [p for p in range(len(pairs)) if tuple(pairs[p]) == (3, 1)]
        assert len(whole) == 1
        matched_family += int(got.matches[whole[0]])
        if name == "zero":
            lo, hi = offsets[whole[0]], offsets[whole[0] + 1]
            kept = got.cosines[lo:hi][ops[lo:hi] == 0]
            assert np.all(kept == 0) and got.cosine_sums[whole[0]] == 0
    assert matched_family > 0


# ---- 5: refusals -------------------------------------------------------------------------------

def test_refused_paths_get_nan_and_leave_their_neighbours_alone():
    case = _hand_case()
    parameters = PARAMETERS[0]
    big = (1, 1)
    good = [(big, (3, 5), [0] * 33), (big, (2, 7), [0] * 30 + [1] * 4 + [0] * 10),
            (big, (130, 120), [0] * 10 + [1] * 10), (big, (0, 0), [0] * 70), (big, (-1, -1), []),
            (big, (9, 9), [0, 2, 0])]
    bad = [(big, (130, 0), [0] * 11),                      # one row past the a-record
           (big, (0, 130), [0] * 11),                      # one row past the b-record
           (big, (4, 4), [0] * 40 + [3] + [0] * 40),       # an op byte of 3
           (big, (-3, 0), [0] * 5),                        # a negative start
           (big, (-1, -1), [0]),                           # only an empty path may start there
           (big, (139, 0), [2, 2]),                        # gaps that leave the a-record
           # a start whose sum with the path's rows wraps around in 32 bits
           (big, (2 ** 31 - 1, 0), [0, 0]),
           (big, (0, 2 ** 31 - 1), [0, 0]),
           (big, (2 ** 31 - 1, 2 ** 31 - 1), [0] * 70),
           (big, (2 ** 31 - 64, 2 ** 31 - 129), [0, 1, 2] * 43)]
    paths = [path for k, wrong in enumerate(bad) for path in (good[k % len(good)], wrong)]
    pairs, given = _as_paths(paths)
    got = _host(case.call(align.path_values, parameters, pairs, given, max_waves=2))   # it returned
    for p, (pair, start, ops) in enumerate(paths):
        lo, hi = int(got.offsets[p]), int(got.offsets[p + 1])
        if p % 2 == 0:
            _assert_path(case, got, p, pair, start, ops, parameters)
            continue
        assert got.status[p] == -2, p
        assert hi - lo == len(ops) and np.isnan(got.cosines[lo:hi]).all(), p
        assert np.isnan(got.running[lo:hi]).all(), p
        assert np.isnan(got.scores[p]) and np.isnan(got.cosine_sums[p]), p
        assert got.matches[p] == 0 and not got.gap_runs[p].any(), p
    mean = align.PathValues(*(torch.from_numpy(np.ascontiguousarray(x)) for x in got)).mean_cosine()
    assert bool(torch.isnan(mean[1])) and bool(torch.isnan(mean[8]))
    assert float(mean[0]) == float(got.cosine_sums[0]) / 33


def test_offsets_on_the_device_that_leave_ops_refuse_the_slot_and_leave_nan():
    """Offsets that live on the device are the kernel's to check: a slot that runs past ``ops`` or
    backwards is refused, none of its per-op values is written, and they read NaN."""
    case = _hand_case()
    parameters = PARAMETERS[0]
    pairs, given = _as_paths([((1, 1), (3, 5), [0, 0, 0]), ((1, 1), (0, 0), [0] * 5),
                              ((1, 1), (0, 0), [])])
    given.offsets = torch.tensor([0, 3, 9, 8], dtype=torch.int64).cuda()     # ops has 8 bytes
    got = _host(case.call(align.path_values, parameters, pairs, given))
    assert got.status.tolist() == [0, -2, -2]
    assert np.isnan(got.cosines[3:]).all() and np.isnan(got.running[3:]).all()
    assert np.isnan(got.scores[1:]).all() and np.isnan(got.cosine_sums[1:]).all()
    _assert_path(case, got, 0, (1, 1), (3, 5), [0, 0, 0], parameters)


def test_paths_with_ops_on_a_call_without_rows_are_refused():
    rows = _hand_case().a_dev
    none = rows[:0]
    pairs, given = _as_paths([((0, 0), (0, 0), [0, 1]), ((0, 0), (-1, -1), []),
                              ((0, 0), (1, 1), [2])])
    got = _host(align.path_values(given, none, rows, counts_a=[0], counts_b=[rows.shape[0]],
                                  pairs=pairs, gap_open=1.0, gap_extend=0.5))
    assert got.status.tolist() == [-2, 0, -2] and got.matches.tolist() == [0, 0, 0]
    assert np.isnan(got.cosines).all() and np.isnan(got.running).all() and got.cosines.shape == (3,)
    assert np.isnan(got.scores[[0, 2]]).all() and got.scores[1] == 0
    assert np.isnan(got.cosine_sums[[0, 2]]).all() and got.cosine_sums[1] == 0


def test_an_empty_call_and_empty_paths_need_no_launch():
    case = _hand_case()
    none = SimpleNamespace(starts=np.zeros((0, 2), dtype=np.int32), ops=np.zeros(0, dtype=np.uint8),
                           offsets=np.zeros(1, dtype=np.int64))
    got = case.call(align.path_values, PARAMETERS[0], np.zeros((0, 2), dtype=np.int32), none)
    assert got.scores.shape == (0,) and got.gap_runs.shape == (0, 2) and got.cosines.shape == (0,)
    assert got.cosine_sums.dtype == torch.float64 and got.scores.is_cuda
    pairs, given = _as_paths([((1, 1), (-1, -1), []), ((0, 0), (-1, -1), [])])
    got = _host(case.call(align.path_values, PARAMETERS[0], pairs, given))
    assert got.scores.tolist() == [0, 0] and got.status.tolist() == [0, 0]
    assert got.matches.tolist() == [0, 0] and got.cosine_sums.tolist() == [0, 0]


# ---- 6: the float64 definition -----------------------------------------------------------------

def test_the_cosines_agree_with_the_float64_definition():
    case, paths = _hand_case(), _hand_paths()
    pairs, given = _as_paths(paths)
    got = _host(case.call(align.path_values, PARAMETERS[0], pairs, given))
    checked = 0
    for p, (pair, start, ops) in enumerate(paths):
        C64 = O.cosine_f64(*case.rows(*pair))
        cells = align.path_cells(np.array(ops, dtype=np.uint8), np.array(start)) if ops else \
            np.zeros((0, 2), dtype=np.int32)
        mine = got.cosines[got.offsets[p]:got.offsets[p + 1]]
        for x, (i, j) in enumerate(cells):
            if i >= 0 and j >= 0:
                assert abs(float(mine[x]) - C64[i, j]) <= COSINE_TOL, (p, x)
                checked += 1
    assert checked > 500
