"""Start cells of the local aligner on the device (align.local_spans, gfy_align_local_span).

Bit for bit against tests/align_span_oracle.py: the substitution matrix of a pair is taken from
the device itself (``distance.pairwise(A, B, metric="cosine")``), scaled and shifted in numpy
float32, and the oracle runs the recurrences and the origin rules of include/gfy.h in float32 —
scores, starts and ends must be equal, and scores and ends equal ``local_align``'s.  A second
check needs no new oracle: ``align_oracle._gotoh`` on the box start..end of S alone must end at
exactly the device's score.  The records, the planted copies and the four parameter sets are
those of tests/test_gpu_align.py, whose cached case is shared."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_oracle as O
import align_span_oracle as SO
import test_gpu_align as G
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, PARAMETERS, WAVES = G.ROWS_A, G.ROWS_B, G.PARAMETERS, G.WAVES


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _spans(case, pairs, parameters, **more):
    scale, shift, go, ge = parameters
    scores, starts, ends = align.local_spans(
        case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs, gap_open=go,
        gap_extend=ge, match_scale=scale, match_shift=shift, **more)
    assert scores.dtype == torch.float32 and scores.is_cuda and scores.shape == (len(pairs),)
    for cells in (starts, ends):
        assert cells.dtype == torch.int32 and cells.is_cuda and cells.shape == (len(pairs), 2)
    return scores.cpu().numpy(), starts.cpu().numpy(), ends.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _grid(parameters):
    """The device's spans of the 6 x 6 pairs under one parameter set, computed once."""
    case = G._case()
    result = _spans(case, case["pairs"], parameters)
    for array in result:
        array.setflags(write=False)
    return result


def _single(A, B, parameters, function=None):
    scale, shift, go, ge = parameters
    result = (function or align.local_spans)(
        A, B, counts_a=[A.shape[0]], counts_b=[B.shape[0]], pairs=[[0, 0]], gap_open=go,
        gap_extend=ge, match_scale=scale, match_shift=shift)
    return tuple(x.cpu().numpy()[0] for x in result)


def _substitution(A, B, parameters):
    C = distance.pairwise(A, B, metric="cosine").cpu().numpy()
    return O.substitution_f32(C, parameters[0], parameters[1])


def _same_span(got, want, where=None):
    """Device (score, start, end) against the oracle's, bit for bit (a zero of either sign)."""
    score, start, end = want
    assert got[0].tobytes() == np.float32(score).tobytes() or (score == 0 and got[0] == 0), \
        (where, got, want)
    assert tuple(got[1]) == start and tuple(got[2]) == end, (where, got, want)


# 1
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_scores_starts_and_ends_equal_the_oracle_bit_for_bit(parameters):
    case = G._case()
    scale, shift, go, ge = parameters
    scores, starts, ends = _grid(parameters)
    for p, (q, r) in enumerate(case["pairs"]):
        S = O.substitution_f32(case["cosines"][p], scale, shift)
        _same_span((scores[p], starts[p], ends[p]), SO.span_of(S, go, ge),
                   (ROWS_A[q], ROWS_B[r], parameters))
    assert scores[case["planted"]].min() > 10     # the planted copies are found: far from 0
    local_scores, local_ends = G._align(case, case["pairs"], parameters)
    assert G._same_bits(scores, local_scores) and G._same_bits(ends, local_ends)


# 2
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_the_box_between_start_and_end_reaches_the_score(parameters):
    """No use of the span oracle: the existing H on the box alone."""
    case = G._case()
    scale, shift, go, ge = parameters
    scores, starts, ends = _grid(parameters)
    positive = 0
    for p, (q, r) in enumerate(case["pairs"]):
        if not scores[p] > 0:
            assert tuple(starts[p]) == (-1, -1) == tuple(ends[p])
            continue
        S = O.substitution_f32(case["cosines"][p], scale, shift)
        (i0, j0), (i1, j1) = starts[p], ends[p]
        assert 0 <= i0 <= i1 < ROWS_A[q] and 0 <= j0 <= j1 < ROWS_B[r], (starts[p], ends[p])
        assert S[i0, j0] > 0
        box = O._gotoh(np.ascontiguousarray(S[i0:i1 + 1, j0:j1 + 1]), go, ge, np.float32)
        assert box[-1, -1].tobytes() == scores[p].tobytes(), (ROWS_A[q], ROWS_B[r], parameters)
        positive += 1
    assert positive >= case["planted"].sum()


# 3
def _basis_rows(indices, signs):
    rows = np.zeros((len(indices), 128), dtype=np.float16)
    rows[np.arange(len(indices)), indices] = signs
    return rows


@pytest.mark.parametrize("transposed", (False, True))
def test_origins_cross_the_strip_edge_inside_a_gap(transposed):
    """Signed basis vectors: every cosine is 0 or +-1 and every sum exact.  The long record is the
    short one with 8 foreign rows after its 60th: the best path is 60 matches, a gap of 8 over
    positions 60..67 (across the edge at 64) and 40 matches, 100 * 0.75 - 1 - 7 * 0.25 = 72.25."""
    rng = np.random.default_rng(64)
    signs = rng.choice([-1.0, 1.0], 100)
    short = _basis_rows(np.arange(100), signs)
    foreign = _basis_rows(np.arange(100, 108), np.ones(8))
    long = np.concatenate([short[:60], foreign, short[60:]])
    A, B = (short, long) if transposed else (long, short)
    A, B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    parameters = (1.0, -0.25, 1.0, 0.25)
    S = _substitution(A, B, parameters)
    assert set(np.unique(S)) <= {-1.25, -0.25, 0.75}
    want = SO.span_of(S, 1.0, 0.25)
    assert want == (np.float32(72.25), (0, 0), (99, 107) if transposed else (107, 99))
    _same_span(_single(A, B, parameters), want)


def test_origins_cross_two_strip_edges():
    rng = np.random.default_rng(128)
    segment = G._unitish(rng, 100)
    rows = G._unitish(rng, 200)
    rows[30:130] = segment + 0.02 * rng.standard_normal((100, 128))
    A = torch.from_numpy(rows.astype(np.float16)).cuda()
    B = torch.from_numpy(segment.astype(np.float16)).cuda()
    for parameters in (PARAMETERS[0], PARAMETERS[2]):
        want = SO.span_of(_substitution(A, B, parameters), parameters[2], parameters[3])
        assert want[0] > 40 and want[1][0] < 64 and want[2][0] >= 128    # strips 0, 1 and 2
        _same_span(_single(A, B, parameters), want)


# 4
@pytest.mark.parametrize("transposed", (False, True))
def test_ties_name_the_first_copy_and_its_start(transposed):
    X, doubled = G._tie_rows()
    A, B = (doubled, X) if transposed else (X, doubled)
    A, B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    parameters = (1.0, -0.5, 1.0, 0.5)
    want = SO.span_of(_substitution(A, B, parameters), 1.0, 0.5)
    assert want[0] > 15 and want[1:] == ((0, 0), (39, 39))
    _same_span(_single(A, B, parameters), want)


# 5
def test_a_span_does_not_depend_on_its_company_or_the_run():
    case = G._case()
    parameters = PARAMETERS[0]
    pair = [5, 5]                                   # 200 x 330: four strips, eleven b-tiles
    alone = _spans(case, [pair], parameters)
    assert alone[0][0] > 10

    def same(one, two):
        return all(G._same_bits(x, y) for x, y in zip(one, two))

    for count in (WAVES - 1, WAVES, WAVES + 1):     # the pairs of one workgroup, one more
        got = _spans(case, [pair] * count, parameters)
        for p in range(count):
            assert same([x[p:p + 1] for x in got], alone)
    rng = np.random.default_rng(3)
    crowd = rng.integers(0, 6, size=(300, 2)).astype(np.int32)
    for seat in (0, 150, 299):
        crowd[seat] = pair
    keeper = align.AlignWorkspace()
    first = _spans(case, crowd, parameters, workspace=keeper)
    again = _spans(case, crowd, parameters, workspace=keeper)
    assert same(first, again)
    order = rng.permutation(300)
    assert same(_spans(case, crowd[order], parameters), [x[order] for x in first])
    for seat in (0, 150, 299):
        assert same([x[seat:seat + 1] for x in first], alone)
    index = crowd[:, 0] * 6 + crowd[:, 1]
    assert same(first, [x[index] for x in _grid(parameters)])
    # the workspace serves local_align as well, before and after
    scores, ends = G._align(case, crowd, parameters, workspace=keeper)
    assert G._same_bits(scores, first[0]) and G._same_bits(ends, first[2])


# 6
def test_edges_empty_records_nothing_positive_self_alignment():
    rng = np.random.default_rng(9)
    rows = G._unitish(rng, 129 + 40).astype(np.float16)
    dev = torch.from_numpy(rows).cuda()
    counts_a, counts_b = [0, 129, 40, 0], [129, 0, 40]
    common = dict(counts_a=counts_a, counts_b=counts_b, gap_open=1.0, gap_extend=0.5)
    pairs = [[0, 0], [1, 1], [0, 1], [3, 2], [1, 0], [2, 2]]
    scores, starts, ends = (x.cpu().numpy() for x in align.local_spans(dev, dev, pairs=pairs, **common))
    for p in range(4):                              # a record of zero rows on either side
        assert scores[p] == 0 and tuple(starts[p]) == (-1, -1) == tuple(ends[p]), p
    assert tuple(ends[4]) == (128, 128) and tuple(ends[5]) == (39, 39)
    assert tuple(starts[4]) == (0, 0) == tuple(starts[5])
    # nothing positive: cosine - 2 <= 0 everywhere
    scores, starts, ends = align.local_spans(dev, dev, pairs=pairs, match_shift=-2.0, **common)
    assert np.all(scores.cpu().numpy() == 0)
    assert np.all(starts.cpu().numpy() == -1) and np.all(ends.cpu().numpy() == -1)
    # b omitted: a record with itself starts at (0, 0)
    scores, starts, ends = (x.cpu().numpy() for x in align.local_spans(
        dev, counts_a=[129, 40], pairs=[[0, 0], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5))
    for p, (lo, hi) in enumerate(((0, 129), (129, 169))):
        want = SO.span_of(_substitution(dev[lo:hi], dev[lo:hi], (1.0, 0.0)), 1.0, 0.5)
        assert want[1:] == ((0, 0), (hi - lo - 1, hi - lo - 1))
        _same_span((scores[p], starts[p], ends[p]), want)
    # no pair at all
    scores, starts, ends = align.local_spans(dev, counts_a=[129, 40],
                                             pairs=np.zeros((0, 2), dtype=np.int64),
                                             gap_open=1.0, gap_extend=0.5)
    assert scores.shape == (0,) and starts.shape == (0, 2) and ends.shape == (0, 2)
    assert scores.is_cuda and starts.is_cuda and ends.is_cuda


# 7
def test_coordinates_at_the_packing_limit():
    """4096 rows against 64 and the other way round: the copy sits in the long record's last 40
    rows, so both coordinates of an origin word come close to their 12 bits."""
    rng = np.random.default_rng(4095)
    long = G._unitish(rng, 4096)
    short = G._unitish(rng, 64)
    short[10:50] = long[4056:4096] + 0.02 * rng.standard_normal((40, 128))
    long_dev = torch.from_numpy(long.astype(np.float16)).cuda()
    short_dev = torch.from_numpy(short.astype(np.float16)).cuda()
    parameters = (1.0, -0.3, 1.0, 0.25)
    for side, (A, B) in enumerate(((long_dev, short_dev), (short_dev, long_dev))):
        want = SO.span_of(_substitution(A, B, parameters), 1.0, 0.25)
        assert want[0] > 10 and want[2][side] == 4095 and want[1][side] >= 4050, want
        got = _single(A, B, parameters)
        _same_span(got, want)
        local = _single(A, B, parameters, align.local_align)
        assert local[0].tobytes() == got[0].tobytes() and tuple(local[1]) == tuple(got[2])


# 8
def test_raw_call_clips_pairs_it_cannot_serve(gpu):
    """The bad pairs of test_gpu_align.test_raw_call_clips_pairs_it_cannot_serve: NaN and (-2, -2)
    in starts and ends, their neighbours what they get without them.  The kernel compares and
    clips what it reads from the device arrays and never follows an index it has not checked."""
    rng = np.random.default_rng(12)
    a = torch.from_numpy(G._unitish(rng, 4097 + 70).astype(np.float16)).cuda()
    b = torch.from_numpy(G._unitish(rng, 90).astype(np.float16)).cuda()
    ptr_a = torch.tensor([0, 4097, 4167], dtype=torch.int32).cuda()
    ptr_b = torch.tensor([0, 90], dtype=torch.int32).cuda()
    pair_list = [[1, 0], [0, 0], [2, 0], [1, 0], [-1, 0], [1, 1], [1, -5], [1, 0], [2 ** 31 - 1, 0]]
    bad = [1, 2, 4, 5, 6, 8]

    def call(pairs, rows_b=4096):
        pairs = torch.tensor(pairs, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_span_workspace_bytes(count, rows_b)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        native.check(gpu.gfy_align_local_span(
            a.data_ptr(), a.shape[0], ptr_a.data_ptr(), 2, b.data_ptr(), b.shape[0],
            ptr_b.data_ptr(), 1, pairs.data_ptr(), count, 1.0, 0.0, 1.0, 0.5, scores.data_ptr(),
            starts.data_ptr(), ends.data_ptr(), scratch.data_ptr(), need,
            torch.cuda.current_stream().cuda_stream), "gfy_align_local_span")
        torch.cuda.synchronize()
        return scores.cpu().numpy(), starts.cpu().numpy(), ends.cpu().numpy()

    scores, starts, ends = call(pair_list)
    clean = call([[1, 0]])
    assert clean[0][0] > 0 and np.all(clean[1] >= 0) and np.all(clean[1] <= clean[2])
    for p in range(len(pair_list)):
        if p in bad:
            assert np.isnan(scores[p]) and tuple(starts[p]) == (-2, -2) == tuple(ends[p]), p
        else:
            for got, want in zip((scores, starts, ends), clean):
                assert G._same_bits(got[p:p + 1], want), p
    # a workspace sized for shorter b-records than a pair names: that pair is refused the same way
    scores, starts, ends = call([[1, 0]], rows_b=32)
    assert np.isnan(scores[0]) and starts.tolist() == [[-2, -2]] == ends.tolist()
