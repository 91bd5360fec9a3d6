"""The aligners on the VALUE range of their inputs (tests/value_cases.py): records that hold zero
rows — C = 0, s = match_shift — at their first row, their last row, both sides of the 64-row
strip seam and all through, on either side; fp16 subnormal rows, rows near the fp16 maximum, norms
ten orders of magnitude apart, and clustered rows, where every s is nearly the same and the fixed
tie rules decide the path.

The chain is closed here: the aligners' contract is C[i][j] == distance.pairwise(A, B, "cosine")[i,
j] bit for bit, tests/test_gpu_distance_values.py checks that ``pairwise`` against float64 on these
families, and this file feeds the float32 oracles (align_oracle, align_span_oracle,
align_path_oracle, align_global_oracle, align_band_oracle) with the device's C and asserts scores,
ends, starts and ops exactly; C itself is checked against float64 once more, per pair of records.
An aligner whose own cosine differed from ``pairwise`` on a zero row (the clamp of
``inverse_norm`` is taken in ``a_inv`` and ``b_s`` of csrc/align_local.inc separately from
k_row_terms) fails every test of ``zero`` below."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import align_span_oracle as SO
import value_cases as V
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

#: (match_scale, match_shift, gap_open, gap_extend): a zero row scores match_shift against every
#: row — below zero, where it breaks a local alignment, and above, where it joins any
PARAMETERS = ((1.0, -0.3, 1.0, 0.25), (1.5, 0.2, 0.75, 0.5))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


class _Case:
    def __init__(self, a, counts_a, b, counts_b, pairs):
        self.a, self.b, self.counts_a, self.counts_b, self.pairs = a, b, counts_a, counts_b, pairs
        self.a_dev, self.b_dev = _device(a), _device(b)
        self.ptr_a = np.concatenate(([0], np.cumsum(counts_a)))
        self.ptr_b = np.concatenate(([0], np.cumsum(counts_b)))
        self.cosines = []                  # the device's own C of every pair, read-only
        for q, r in pairs:
            C = distance.pairwise(self.a_dev[self.ptr_a[q]:self.ptr_a[q + 1]],
                                  self.b_dev[self.ptr_b[r]:self.ptr_b[r + 1]],
                                  metric="cosine").cpu().numpy()
            C.setflags(write=False)
            self.cosines.append(C)

    def rows(self, p):
        q, r = self.pairs[p]
        return (self.a[self.ptr_a[q]:self.ptr_a[q + 1]], self.b[self.ptr_b[r]:self.ptr_b[r + 1]])

    def call(self, function, parameters, **more):
        scale, shift, go, ge = parameters
        return function(self.a_dev, self.b_dev, counts_a=self.counts_a, counts_b=self.counts_b,
                        pairs=self.pairs, gap_open=go, gap_extend=ge, match_scale=scale,
                        match_shift=shift, **more)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(*V.align_records(name))


def _host(result):
    return tuple(t.cpu().numpy() for t in result)


def _equal_score(got, want):
    return got.tobytes() == np.float32(want).tobytes() or (want == 0 and got == 0)


def _paths_of(result, p):
    scores, starts, ends, ops, offsets = result
    return scores[p], tuple(starts[p]), tuple(ends[p]), ops[offsets[p]:offsets[p + 1]]


@pytest.mark.parametrize("name", V.FAMILIES)
def test_the_device_cosines_of_the_records_match_float64(name):
    case = _case(name)
    assert len(case.pairs) <= 12 and max(case.counts_a + case.counts_b) <= 200
    for p in range(len(case.pairs)):
        rows_a, rows_b = case.rows(p)
        C = case.cosines[p]
        assert not np.isnan(C).any()
        assert np.abs(C.astype(np.float64) - O.cosine_f64(rows_a, rows_b)).max() <= V.COSINE_TOL
        gone_a = ~rows_a.astype(np.float64).any(axis=1)
        gone_b = ~rows_b.astype(np.float64).any(axis=1)
        assert np.all(C[gone_a] == 0) and np.all(C[:, gone_b] == 0)      # a zero row: C = 0
    if name == "zero":
        assert any(np.all(C == 0) for C in case.cosines)


@pytest.mark.parametrize("parameters", PARAMETERS)
@pytest.mark.parametrize("name", V.FAMILIES)
def test_local_scores_spans_and_paths_equal_the_oracles(name, parameters):
    case = _case(name)
    scale, shift, go, ge = parameters
    scores, ends = _host(case.call(align.local_align, parameters))
    span = _host(case.call(align.local_spans, parameters))
    paths = _host(case.call(align.local_paths, parameters))
    positive = 0
    for p in range(len(case.pairs)):
        S = O.substitution_f32(case.cosines[p], scale, shift)
        rows_a, rows_b = case.rows(p)
        if not rows_a.astype(np.float64).any() or not rows_b.astype(np.float64).any():
            assert np.all(S == np.float32(shift))                         # s = match_shift
        score, start, end, ops = PO.path_of(S, go, ge)
        assert (score, start, end) == SO.span_of(S, go, ge)
        assert O.gotoh_f32(S, go, ge) == (score, end)
        where = (name, tuple(case.pairs[p]), parameters)
        assert _equal_score(scores[p], score) and tuple(ends[p]) == end, where
        assert _equal_score(span[0][p], score), where
        assert (tuple(span[1][p]), tuple(span[2][p])) == (start, end), where
        got = _paths_of(paths, p)
        assert _equal_score(got[0], score) and got[1:3] == (start, end), where
        assert got[3].tobytes() == ops.tobytes(), where
        positive += bool(score > 0)
    assert positive >= 6                       # the shared segment is found: something to walk


@pytest.mark.parametrize("within", (False, True))
@pytest.mark.parametrize("parameters", PARAMETERS)
@pytest.mark.parametrize("name", V.FAMILIES)
def test_global_scores_and_paths_equal_the_oracle(name, parameters, within):
    case = _case(name)
    scale, shift, go, ge = parameters
    scores, ends = _host(case.call(align.global_align, parameters, within=within))
    paths = _host(case.call(align.global_paths, parameters, within=within))
    for p in range(len(case.pairs)):
        S = O.substitution_f32(case.cosines[p], scale, shift)
        score, start, end, ops = GO.path_of(S, go, ge, within)
        assert GO.score_of(S, go, ge, within) == (score, end)
        where = (name, tuple(case.pairs[p]), parameters, within)
        assert scores[p].tobytes() == np.float32(score).tobytes(), where
        assert tuple(ends[p]) == end, where
        got = _paths_of(paths, p)
        assert got[0].tobytes() == np.float32(score).tobytes() and got[1:3] == (start, end), where
        assert got[3].tobytes() == ops.tobytes(), where


def _bands(case, parameters):
    """A band of 8 diagonals on either side of every pair's unbanded end cell (the first cell of
    a pair without one)."""
    _, ends = _host(case.call(align.local_align, parameters))
    return align.band_around(np.maximum(ends, 0), 8)


@pytest.mark.parametrize("name", ("zero", "huge", "clustered"))
def test_banded_spans_equal_the_oracle(name):
    case = _case(name)
    parameters = PARAMETERS[0]
    scale, shift, go, ge = parameters
    band = _bands(case, parameters)
    span = _host(case.call(align.local_spans, parameters, band=band))
    for p in range(len(case.pairs)):
        S = O.substitution_f32(case.cosines[p], scale, shift)
        score, start, end = BO.band_span_of(S, go, ge, int(band[p, 0]), int(band[p, 1]))
        where = (name, tuple(case.pairs[p]))
        assert _equal_score(span[0][p], score), where
        assert (tuple(span[1][p]), tuple(span[2][p])) == (start, end), where


def _scalable_records(name):
    """``align_records`` with every element inside the range that 2^-6 and 2^5 keep normal: one-hot
    values outside it become +-1 in place, other elements below 2^-8 zero."""
    a, counts_a, b, counts_b, pairs = V.align_records(name)
    out = []
    for rows in (a, b):
        wide = rows.astype(np.float64)
        if name == "onehot":
            odd = (np.abs(wide) > 2) | ((wide != 0) & (np.abs(wide) < 2.0 ** -8))
            rows = np.where(odd, np.sign(wide), wide).astype(np.float16)
        out.append(V.in_normal_range(rows))
    return out[0], counts_a, out[1], counts_b, pairs


def _every_output(case, parameters, band):
    """Every output of every entry point the tests above call, and one banded call."""
    out = []
    for function in (align.local_align, align.local_spans, align.local_paths):
        out += _host(case.call(function, parameters))
    out += _host(case.call(align.local_spans, parameters, band=band))
    for within in (False, True):
        out += _host(case.call(align.global_align, parameters, within=within))
        out += _host(case.call(align.global_paths, parameters, within=within))
    return out


@pytest.mark.parametrize("name", ("gauss", "clustered", "onehot"))
def test_power_of_two_scaling_changes_no_bit(name):
    """The aligners see rows only through cosines, and a power of two scales every product, sum,
    |row|², root and reciprocal exactly: every output is the same byte for byte."""
    a, counts_a, b, counts_b, pairs = _scalable_records(name)
    parameters = PARAMETERS[0]
    base = _Case(a, counts_a, b, counts_b, pairs)
    band = _bands(base, parameters)
    want = _every_output(base, parameters, band)
    assert want[0].max() > 0
    for p, q in ((-6, -6), (-6, 5), (5, -6), (5, 5)):
        moved = _Case(V.scaled(a, p), counts_a, V.scaled(b, q), counts_b, pairs)
        for C, C0 in zip(moved.cosines, base.cosines):
            assert C.tobytes() == C0.tobytes(), (p, q)
        for got, expected in zip(_every_output(moved, parameters, band), want):
            assert got.dtype == expected.dtype and got.tobytes() == expected.tobytes(), (p, q)
