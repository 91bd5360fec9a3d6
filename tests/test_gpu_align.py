"""The local aligner on the device (align.local_align, gfy_align_local) against the two oracles of
tests/align_oracle.py.

Bit for bit: the substitution matrix of a pair is taken from the device itself
(``distance.pairwise(A, B, metric="cosine")``, existing code), scaled and shifted in numpy
float32, and oracle (a) runs the recurrences in float32 — scores and ends must be equal, on
record lengths around the strip edge (64 a-rows) and the b-tile edges (32 / 128 b-rows).

Against the float64 definition (oracle (b)) the score may differ by
    min(Lq, Lr) * |match_scale| * COSINE_TOL + (Lq + Lr) * 2^-24 * max(score64, 1):
the first term bounds the substitution errors along any path (a path has at most min(Lq, Lr)
matches, each cosine is within COSINE_TOL), the second the float32 roundings (one per cell of a
path, at most Lq + Lr cells, each half an ulp of a value no larger than the score); the optimum
is 1-Lipschitz in both.  Ends are compared where the float64 best cell beats EVERY other cell by
more than twice that bound (then no cell's float32 value can overtake it); every planted pair
must qualify, which is asserted on the host before the device is asked.
The test prints every pair's error next to its bound and the largest ratio of the two (-s).  On
an MI355X: largest error / bound 0.0104, ends compared on 25 of the 36 pairs."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import align_oracle as O
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

COSINE_TOL = 2e-6        # tests/test_gpu_distance_ranges.py
ROWS_A = (1, 63, 64, 65, 129, 200)      # strip edge 64
ROWS_B = (1, 127, 128, 129, 257, 330)   # b-tile edges 32 and 128
WAVES = 4                               # pairs per workgroup (align_local.inc)
#: (match_scale, match_shift, gap_open, gap_extend)
PARAMETERS = ((1.0, -0.3, 1.0, 0.25), (2.0, -0.5, 0.75, 0.0), (1.5, -0.4, 0.5, 0.5),
              (1.0, 0.0, 1.0, 0.5))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _unitish(rng, count):
    data = rng.standard_normal((count, 128))
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    return data * rng.uniform(0.8, 1.25, size=(count, 1))


def _records(rng, sizes, segment):
    """Records of ``sizes`` rows; every record of 63 rows or more carries a noisy copy of the
    first 30 to 50 rows of ``segment`` somewhere."""
    records = []
    for size in sizes:
        rows = _unitish(rng, size)
        if size >= 63:
            length = int(rng.integers(30, 51))
            at = int(rng.integers(0, size - length + 1))
            rows[at:at + length] = segment[:length] + 0.02 * rng.standard_normal((length, 128))
        records.append(rows.astype(np.float16))
    return records


@functools.lru_cache(maxsize=None)
def _case():
    """The 6 x 6 pairs of ROWS_A x ROWS_B, their device tensors and, per pair, the device's own
    cosine matrix (float32, read-only) — computed once for the module."""
    rng = np.random.default_rng(20251018)
    segment = _unitish(rng, 50)
    rec_a, rec_b = _records(rng, ROWS_A, segment), _records(rng, ROWS_B, segment)
    a, b = np.concatenate(rec_a), np.concatenate(rec_b)
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    pairs = np.array([(q, r) for q in range(len(ROWS_A)) for r in range(len(ROWS_B))], dtype=np.int32)
    cosines = []
    for q, r in pairs:
        C = distance.pairwise(torch.from_numpy(rec_a[q]).cuda(), torch.from_numpy(rec_b[r]).cuda(),
                              metric="cosine").cpu().numpy()
        C.setflags(write=False)
        cosines.append(C)
    planted = np.array([ROWS_A[q] >= 63 and ROWS_B[r] >= 63 for q, r in pairs])
    assert 2 * planted.sum() >= len(pairs)
    return dict(rec_a=rec_a, rec_b=rec_b, a=a_dev, b=b_dev, pairs=pairs, cosines=cosines,
                planted=planted)


def _align(case, pairs, parameters, **more):
    scale, shift, go, ge = parameters
    scores, ends = align.local_align(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B,
                                     pairs=pairs, gap_open=go, gap_extend=ge, match_scale=scale,
                                     match_shift=shift, **more)
    assert scores.dtype == torch.float32 and ends.dtype == torch.int32 and scores.is_cuda
    return scores.cpu().numpy(), ends.cpu().numpy()


def _same_bits(one, two):
    return one.dtype == two.dtype and one.shape == two.shape and one.tobytes() == two.tobytes()


@pytest.mark.parametrize("parameters", PARAMETERS)
def test_scores_and_ends_equal_the_float32_oracle_bit_for_bit(parameters):
    case = _case()
    scale, shift, go, ge = parameters
    scores, ends = _align(case, case["pairs"], parameters)
    for p, (q, r) in enumerate(case["pairs"]):
        S = O.substitution_f32(case["cosines"][p], scale, shift)
        score, end = O.gotoh_f32(S, go, ge)
        where = (ROWS_A[q], ROWS_B[r], parameters)
        assert scores[p].tobytes() == np.float32(score).tobytes() or \
            (score == 0 and scores[p] == 0), (where, scores[p], score)
        assert tuple(ends[p]) == end, (where, ends[p], end)
    assert scores[case["planted"]].min() > 10     # the planted copies are found: far from 0


def test_scores_and_ends_against_the_float64_definition():
    case = _case()
    parameters = PARAMETERS[0]
    scale, shift, go, ge = parameters
    expected, compared = [], []
    for p, (q, r) in enumerate(case["pairs"]):
        score64, end64, H = O.gotoh_f64(case["rec_a"][q], case["rec_b"][r], go, ge, scale, shift)
        lq, lr = H.shape
        bound = min(lq, lr) * abs(scale) * COSINE_TOL + (lq + lr) * 2.0 ** -24 * max(score64, 1.0)
        others = H.copy()
        if end64 != (-1, -1):
            others[end64] = -np.inf
        clear = end64 != (-1, -1) and score64 - others.max() > 2 * bound
        assert clear or not case["planted"][p], (ROWS_A[q], ROWS_B[r], score64 - others.max(), bound)
        expected.append((score64, end64, bound))
        compared.append(clear)
    assert sum(compared) >= case["planted"].sum()      # host only up to here
    scores, ends = _align(case, case["pairs"], parameters)
    worst = 0.0
    for p, (score64, end64, bound) in enumerate(expected):
        error = abs(float(scores[p]) - score64)
        worst = max(worst, error / bound)
        print(f"Lq {ROWS_A[case['pairs'][p][0]]:4d} Lr {ROWS_B[case['pairs'][p][1]]:4d} "
              f"score64 {score64:10.6f} error {error:.3e} bound {bound:.3e}")
        assert error <= bound, (case["pairs"][p], float(scores[p]), score64, bound)
        if compared[p]:
            assert tuple(ends[p]) == end64, (case["pairs"][p], ends[p], end64)
    print(f"largest error / bound: {worst:.4f}; ends compared on {sum(compared)} of {len(expected)}")


def _tie_rows():
    rng = np.random.default_rng(77)
    X = _unitish(rng, 40).astype(np.float16)
    junk = _unitish(rng, 70).astype(np.float16)
    return X, np.concatenate([X, junk, X])


@pytest.mark.parametrize("transposed", (False, True))
def test_ties_go_to_the_first_copy(transposed):
    """B = [X, junk, X] against A = X (and the transposed case): both copies end with bit-equal
    scores — shown with oracle (a) on the device's own cosines — and the first one is named."""
    X, doubled = _tie_rows()
    A, B = (doubled, X) if transposed else (X, doubled)
    a_dev, b_dev = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    scale, shift, go, ge = 1.0, -0.5, 1.0, 0.5
    S = O.substitution_f32(distance.pairwise(a_dev, b_dev, metric="cosine").cpu().numpy(),
                           scale, shift)
    H = O._gotoh(S, go, ge, np.float32)
    first, second = ((39, 39), (149, 39)) if transposed else ((39, 39), (39, 149))
    assert H[first] == H[second] == H.max() and H.max() > 15
    assert O.end_of(H)[1] == first
    scores, ends = align.local_align(a_dev, b_dev, counts_a=[len(A)], counts_b=[len(B)],
                                     pairs=[[0, 0]], gap_open=go, gap_extend=ge,
                                     match_scale=scale, match_shift=shift)
    assert scores.cpu().numpy()[0].tobytes() == H.max().tobytes()
    assert tuple(ends.cpu().numpy()[0]) == first


def test_a_pair_does_not_depend_on_its_company_or_the_run():
    case = _case()
    parameters = PARAMETERS[0]
    pair = [5, 5]                                   # 200 x 330: four strips, eleven b-tiles
    alone = _align(case, [pair], parameters)
    assert alone[0][0] > 10
    for count in (WAVES - 1, WAVES, WAVES + 1):     # the pairs of one workgroup, one more
        scores, ends = _align(case, [pair] * count, parameters)
        for p in range(count):
            assert _same_bits(scores[p:p + 1], alone[0]) and _same_bits(ends[p:p + 1], alone[1])
    rng = np.random.default_rng(3)
    crowd = rng.integers(0, 6, size=(300, 2)).astype(np.int32)
    for seat in (0, 150, 299):
        crowd[seat] = pair
    keeper = align.AlignWorkspace()
    first = _align(case, crowd, parameters, workspace=keeper)
    again = _align(case, crowd, parameters, workspace=keeper)
    assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1])
    order = rng.permutation(300)
    shuffled = _align(case, crowd[order], parameters)
    assert _same_bits(shuffled[0], first[0][order]) and _same_bits(shuffled[1], first[1][order])
    for seat in (0, 150, 299):
        assert _same_bits(first[0][seat:seat + 1], alone[0])
        assert _same_bits(first[1][seat:seat + 1], alone[1])
    # every pair of the crowd equals the same pair of the 6 x 6 call
    grid = _align(case, case["pairs"], parameters)
    index = crowd[:, 0] * 6 + crowd[:, 1]
    assert _same_bits(first[0], grid[0][index]) and _same_bits(first[1], grid[1][index])


def test_edges_empty_records_nothing_positive_self_alignment():
    rng = np.random.default_rng(9)
    rows = _unitish(rng, 129 + 40).astype(np.float16)
    dev = torch.from_numpy(rows).cuda()
    counts_a, counts_b = [0, 129, 40, 0], [129, 0, 40]
    common = dict(counts_a=counts_a, counts_b=counts_b, gap_open=1.0, gap_extend=0.5)
    pairs = [[0, 0], [1, 1], [0, 1], [3, 2], [1, 0], [2, 2]]
    scores, ends = align.local_align(dev, dev, pairs=pairs, **common)
    scores, ends = scores.cpu().numpy(), ends.cpu().numpy()
    for p in range(4):                              # a record of zero rows on either side
        assert scores[p] == 0 and tuple(ends[p]) == (-1, -1), p
    assert tuple(ends[4]) == (128, 128) and tuple(ends[5]) == (39, 39)
    # nothing positive: cosine - 2 <= 0 everywhere
    scores, ends = align.local_align(dev, dev, pairs=pairs, match_shift=-2.0, **common)
    assert np.all(scores.cpu().numpy() == 0) and np.all(ends.cpu().numpy() == -1)
    # b omitted: a record with itself, bit-equal to oracle (a) on the device's cosines
    scores, ends = align.local_align(dev, counts_a=[129, 40], pairs=[[0, 0], [1, 1], [1, 0]],
                                     gap_open=1.0, gap_extend=0.5)
    scores, ends = scores.cpu().numpy(), ends.cpu().numpy()
    for p, (lo, hi) in enumerate(((0, 129), (129, 169))):
        C = distance.pairwise(dev[lo:hi], dev[lo:hi], metric="cosine").cpu().numpy()
        score, end = O.gotoh_f32(O.substitution_f32(C, 1.0, 0.0), 1.0, 0.5)
        assert end == (hi - lo - 1, hi - lo - 1) == tuple(ends[p])
        assert scores[p].tobytes() == np.float32(score).tobytes()
    # no pair at all
    scores, ends = align.local_align(dev, counts_a=[129, 40], pairs=np.zeros((0, 2), dtype=np.int64),
                                     gap_open=1.0, gap_extend=0.5)
    assert scores.shape == (0,) and ends.shape == (0, 2) and scores.is_cuda


def test_the_longest_record_against_one_strip():
    """4096 rows (the limit, 64 strips) against 64 rows, and the other way round (one strip, 128
    b-tiles): single pairs."""
    rng = np.random.default_rng(4096)
    long = _unitish(rng, 4096)
    short = _unitish(rng, 64)
    short[10:50] = long[3000:3040] + 0.02 * rng.standard_normal((40, 128))
    long_dev = torch.from_numpy(long.astype(np.float16)).cuda()
    short_dev = torch.from_numpy(short.astype(np.float16)).cuda()
    for A, B in ((long_dev, short_dev), (short_dev, long_dev)):
        C = distance.pairwise(A, B, metric="cosine").cpu().numpy()
        score, end = O.gotoh_f32(O.substitution_f32(C, 1.0, -0.3), 1.0, 0.25)
        scores, ends = align.local_align(A, B, counts_a=[A.shape[0]], counts_b=[B.shape[0]],
                                         pairs=[[0, 0]], gap_open=1.0, gap_extend=0.25,
                                         match_shift=-0.3)
        assert score > 10
        assert scores.cpu().numpy()[0].tobytes() == np.float32(score).tobytes()
        assert tuple(ends.cpu().numpy()[0]) == end


def test_raw_call_clips_pairs_it_cannot_serve(gpu):
    """The C call with pair indices out of range and a record of 4097 rows: those pairs get NaN
    and (-2, -2), their neighbours what they get without them.  The kernel compares and clips
    what it reads from the device arrays and never follows an index it has not checked."""
    rng = np.random.default_rng(12)
    a = torch.from_numpy(_unitish(rng, 4097 + 70).astype(np.float16)).cuda()
    b = torch.from_numpy(_unitish(rng, 90).astype(np.float16)).cuda()
    ptr_a = torch.tensor([0, 4097, 4167], dtype=torch.int32).cuda()
    ptr_b = torch.tensor([0, 90], dtype=torch.int32).cuda()
    pair_list = [[1, 0], [0, 0], [2, 0], [1, 0], [-1, 0], [1, 1], [1, -5], [1, 0], [2 ** 31 - 1, 0]]
    bad = [1, 2, 4, 5, 6, 8]

    def call(pairs):
        pairs = torch.tensor(pairs, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_workspace_bytes(count, 4096)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        native.check(gpu.gfy_align_local(
            a.data_ptr(), a.shape[0], ptr_a.data_ptr(), 2, b.data_ptr(), b.shape[0],
            ptr_b.data_ptr(), 1, pairs.data_ptr(), count, 1.0, 0.0, 1.0, 0.5, scores.data_ptr(),
            ends.data_ptr(), scratch.data_ptr(), need,
            torch.cuda.current_stream().cuda_stream), "gfy_align_local")
        torch.cuda.synchronize()
        return scores.cpu().numpy(), ends.cpu().numpy()

    scores, ends = call(pair_list)
    clean_scores, clean_ends = call([[1, 0]])
    assert clean_scores[0] > 0
    for p in range(len(pair_list)):
        if p in bad:
            assert np.isnan(scores[p]) and tuple(ends[p]) == (-2, -2), (p, scores[p], ends[p])
        else:
            assert _same_bits(scores[p:p + 1], clean_scores) and _same_bits(ends[p:p + 1], clean_ends)
    # a workspace sized for shorter b-records than a pair names: that pair is refused the same way
    pairs = torch.tensor([[1, 0]], dtype=torch.int32).cuda()
    out_s = torch.zeros(1, dtype=torch.float32).cuda()
    out_e = torch.zeros((1, 2), dtype=torch.int32).cuda()
    need = gpu.gfy_align_workspace_bytes(1, 32)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    native.check(gpu.gfy_align_local(
        a.data_ptr(), a.shape[0], ptr_a.data_ptr(), 2, b.data_ptr(), b.shape[0], ptr_b.data_ptr(),
        1, pairs.data_ptr(), 1, 1.0, 0.0, 1.0, 0.5, out_s.data_ptr(), out_e.data_ptr(),
        scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "gfy_align_local")
    torch.cuda.synchronize()
    assert np.isnan(out_s.cpu().numpy()[0]) and out_e.cpu().numpy().tolist() == [[-2, -2]]


def test_record_scores_to_pairs_to_alignments():
    """The two-call pipeline: the planted copies rank first and align far from 0."""
    case = _case()
    ranking = distance.record_scores(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B,
                                     metric="cosine")
    pairs = align.top_pairs(ranking, 2, largest=True)
    assert pairs.shape == (12, 2) and pairs[:, 0].tolist() == [q for q in range(6) for _ in (0, 1)]
    scores, ends = _align(case, pairs, PARAMETERS[0])
    grid = _align(case, case["pairs"], PARAMETERS[0])
    index = pairs[:, 0] * 6 + pairs[:, 1]
    assert _same_bits(scores, grid[0][index]) and _same_bits(ends, grid[1][index])
