"""Global and query-in-target alignment on the device (align.global_align, align.global_paths,
gfy_align_global, gfy_align_global_trace) against the oracle of tests/align_global_oracle.py.

Bit for bit: as in test_gpu_align, a pair's substitution matrix is the device's own cosine
matrix scaled and shifted in numpy float32, and the oracle runs the recurrences, the iterated
borders and the walk in float32 — scores, starts, ends, ops and offsets must be equal, on record
lengths around the strip edge (64 a-rows) and the b-tile edges (32 / 128 b-rows).

Against the float64 definition a score may differ by
    min(Lq, Lr) * (|scale| * COSINE_TOL + 2 * 2^-24 * (|scale| + |shift|))
        + 2^-24 * c * L * (L + 1) / 2,     L = Lq + Lr,  c = max(gap_open, |scale| + |shift|).
Both scores are maxima over the same set of alignments (rounded + and max are monotone), so they
differ by no more than one alignment's two evaluations do.  An alignment has at most min(Lq, Lr)
matches, each substitution score off by the cosine's tolerance times the scale and by two
roundings of values no larger than |scale| + |shift| (first term); and at most L ops, border
included — the border is where the magnitudes come from: every op moves the running value by at
most c, so after k ops it is at most k * c (gap_open + k * gap_extend on a border) and its
rounding at most 2^-24 of that (second term).  Nothing in the bound comes from the device.  The
test prints every pair's error next to its bound (-s).  On an MI355X: largest error / bound
0.0070 (global) and 0.0056 (within)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import align_global_oracle as GO
import align_oracle as O
import test_gpu_align as G
import test_gpu_align_span as GS
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, PARAMETERS, WAVES = G.ROWS_A, G.ROWS_B, G.PARAMETERS, G.WAVES
MODES = (False, True)          # within


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _host(result):
    """(scores, starts, ends, [ops of pair p], offsets) as numpy."""
    offsets = result.offsets.cpu().numpy()
    ops = result.ops.cpu().numpy()
    assert result.ops.dtype == torch.uint8 and result.offsets.dtype == torch.int64
    assert result.scores.dtype == torch.float32 and result.starts.dtype == torch.int32
    assert offsets[0] == 0 and offsets[-1] == ops.size and result.ops.is_cuda
    return (result.scores.cpu().numpy(), result.starts.cpu().numpy(), result.ends.cpu().numpy(),
            [ops[offsets[p]:offsets[p + 1]] for p in range(offsets.size - 1)], offsets)


def _keywords(parameters):
    scale, shift, go, ge = parameters
    return dict(gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift)


def _paths(case, pairs, parameters, within, **more):
    return _host(align.global_paths(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B,
                                    pairs=pairs, within=within, **_keywords(parameters), **more))


def _scores(case, pairs, parameters, within, **more):
    scores, ends = align.global_align(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B,
                                      pairs=pairs, within=within, **_keywords(parameters), **more)
    assert scores.dtype == torch.float32 and ends.dtype == torch.int32 and scores.is_cuda
    return scores.cpu().numpy(), ends.cpu().numpy()


def _single(A, B, parameters, within):
    """global_align and global_paths of one pair of device tensors; the two agree."""
    common = dict(counts_a=[A.shape[0]], counts_b=[B.shape[0]], pairs=[[0, 0]], within=within,
                  **_keywords(parameters))
    scores, starts, ends, paths, _ = _host(align.global_paths(A, B, **common))
    score, end = align.global_align(A, B, **common)
    assert G._same_bits(score.cpu().numpy(), scores) and G._same_bits(end.cpu().numpy(), ends)
    return scores[0], starts[0], ends[0], paths[0]


def _same_score(got, want):
    return np.float32(got).tobytes() == np.float32(want).tobytes() or (got == 0 and want == 0)


def _same_path(got, want, where=None):
    score, start, end, ops = want
    assert _same_score(got[0], score), (where, got[0], score)
    assert tuple(got[1]) == start and tuple(got[2]) == end, (where, got[1:3], want[1:3])
    assert got[3].tobytes() == ops.tobytes(), (where, got[3], ops)


def _same_paths(one, two):
    return all(G._same_bits(x, y) for x, y in zip(one[:3], two[:3])) and \
        len(one[3]) == len(two[3]) and all(x.tobytes() == y.tobytes() for x, y in zip(one[3], two[3]))


def _pick(result, index):
    scores, starts, ends, paths = result[:4]
    return scores[index], starts[index], ends[index], [paths[p] for p in index]


# 1
@pytest.mark.parametrize("within", MODES)
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_scores_ends_and_paths_equal_the_oracle_bit_for_bit(parameters, within):
    case = G._case()
    scale, shift, go, ge = parameters
    scores, starts, ends, paths, offsets = _paths(case, case["pairs"], parameters, within)
    plain = _scores(case, case["pairs"], parameters, within)
    assert G._same_bits(plain[0], scores) and G._same_bits(plain[1], ends)
    total, bordered = 0, 0
    for p, (q, r) in enumerate(case["pairs"]):
        S = O.substitution_f32(case["cosines"][p], scale, shift)
        want = GO.path_of(S, go, ge, within)
        _same_path((scores[p], starts[p], ends[p], paths[p]), want,
                   (ROWS_A[q], ROWS_B[r], parameters, within))
        assert offsets[p] == total
        total += want[3].size
        bordered += int(want[3][0] != 0)
    assert offsets[-1] == total and bordered >= 4        # paths that end on a charged border


# 2
@pytest.mark.parametrize("within", MODES)
def test_scores_against_the_float64_definition(within):
    case = G._case()
    parameters = PARAMETERS[0]
    scale, shift, go, ge = (float(np.float32(x)) for x in parameters)
    scores, _ = _scores(case, case["pairs"], parameters, within)
    worst = 0.0
    for p, (q, r) in enumerate(case["pairs"]):
        S = O.cosine_f64(case["rec_a"][q], case["rec_b"][r]) * scale + shift
        score64 = float(GO.score_of(S, go, ge, within, np.float64)[0])
        lq, lr = S.shape
        length, step = lq + lr, max(go, abs(scale) + abs(shift))
        bound = min(lq, lr) * (abs(scale) * G.COSINE_TOL + 2 * 2.0 ** -24 * (abs(scale) + abs(shift))) \
            + 2.0 ** -24 * step * length * (length + 1) / 2
        error = abs(float(scores[p]) - score64)
        worst = max(worst, error / bound)
        print(f"Lq {lq:4d} Lr {lr:4d} score64 {score64:11.6f} error {error:.3e} bound {bound:.3e}")
        assert error <= bound, (within, lq, lr, float(scores[p]), score64, bound)
    print(f"within {within}: largest error / bound {worst:.4f}")


# 3
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_global_within_local_ordering(parameters):
    case = G._case()
    whole = _scores(case, case["pairs"], parameters, False)[0]
    inside = _scores(case, case["pairs"], parameters, True)[0]
    local = G._align(case, case["pairs"], parameters)[0]
    assert np.all(whole <= inside) and np.all(inside <= local), (whole, inside, local)
    assert np.any(whole < inside) and np.any(inside < local)


# 4
def _flanked():
    """Signed basis vectors (every cosine 0 or +-1, every sum exact): a core of 50 rows, and the
    core behind 70 rows (across the strip edge at 64) or 140 rows (across the b-tile edges at 32
    and 128) that are orthogonal to it."""
    rng = np.random.default_rng(70)
    core = GS._basis_rows(np.arange(50), rng.choice([-1.0, 1.0], 50))
    flank = GS._basis_rows(50 + np.arange(140) % 78, np.ones(140))
    return core, flank


@pytest.mark.parametrize("within", MODES)
def test_the_left_border_across_the_strip_edge(within):
    core, flank = _flanked()
    A = torch.from_numpy(np.concatenate([flank[:70], core])).cuda()
    B = torch.from_numpy(core).cuda()
    parameters = (1.0, -0.5, 1.0, 0.25)
    want = GO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25, within)
    assert want[3].tolist() == [2] * 70 + [0] * 50 and want[1:3] == ((0, 0), (119, 49))
    assert want[0] == np.float32(50 * 0.5 - 1.0 - 69 * 0.25)
    _same_path(_single(A, B, parameters, within), want)


@pytest.mark.parametrize("within", MODES)
def test_the_top_border_across_the_tile_edges(within):
    core, flank = _flanked()
    A = torch.from_numpy(core).cuda()
    B = torch.from_numpy(np.concatenate([flank, core])).cuda()
    parameters = (1.0, -0.5, 1.0, 0.25)
    want = GO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25, within)
    if within:           # the 140 leading rows of B are free
        assert want[3].tolist() == [0] * 50 and want[1:3] == ((0, 140), (49, 189))
        assert want[0] == np.float32(25)
    else:
        assert want[3].tolist() == [1] * 140 + [0] * 50 and want[1:3] == ((0, 0), (49, 189))
        assert want[0] == np.float32(25 - 1.0 - 139 * 0.25)
    _same_path(_single(A, B, parameters, within), want)


@pytest.mark.parametrize("within", MODES)
@pytest.mark.parametrize("transposed", (False, True))
def test_a_gap_across_the_strip_edge(transposed, within):
    """The case of test_gpu_align_path: 60 matches, a gap of 8 over positions 60..67 of the long
    record (in F across the strip edge at 64; transposed, in E) and 40 matches."""
    rng = np.random.default_rng(64)
    short = GS._basis_rows(np.arange(100), rng.choice([-1.0, 1.0], 100))
    foreign = GS._basis_rows(np.arange(100, 108), np.ones(8))
    long = np.concatenate([short[:60], foreign, short[60:]])
    A, B = (short, long) if transposed else (long, short)
    A, B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    parameters = (1.0, -0.25, 1.0, 0.25)
    want = GO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25, within)
    assert want[3].tolist() == [0] * 60 + [1 if transposed else 2] * 8 + [0] * 40
    assert want[:3] == (np.float32(72.25), (0, 0), (99, 107) if transposed else (107, 99))
    _same_path(_single(A, B, parameters, within), want)


# 5
def test_within_finds_a_window_where_it_was_cut():
    case = G._case()
    whole = case["rec_b"][5]                       # 330 rows
    offset = 131                                   # no multiple of 8
    A = torch.from_numpy(np.ascontiguousarray(whole[offset:offset + 100])).cuda()
    B = torch.from_numpy(whole).cuda()
    parameters = (1.0, -0.3, 1.0, 0.25)
    S = GS._substitution(A, B, parameters)
    score, start, end, ops = _single(A, B, parameters, True)
    assert tuple(start) == (0, offset) and tuple(end) == (99, offset + 99)
    assert ops.tolist() == [0] * 100
    total = np.float32(0)
    for i in range(100):
        total = np.float32(total + S[i, offset + i])
    assert score.tobytes() == total.tobytes() and score > 60
    _same_path((score, start, end, ops), GO.path_of(S, 1.0, 0.25, True))
    local = align.local_spans(A, B, counts_a=[100], counts_b=[330], pairs=[[0, 0]],
                              **_keywords(parameters))
    assert local[0].cpu().numpy()[0].tobytes() == score.tobytes()
    assert local[1].cpu().numpy()[0].tolist() == [0, offset]
    assert local[2].cpu().numpy()[0].tolist() == [99, offset + 99]


# 6
@pytest.mark.parametrize("within", MODES)
def test_a_pair_does_not_depend_on_its_company_the_run_or_the_workspace(gpu, within):
    case = G._case()
    parameters = PARAMETERS[0]
    grid = _paths(case, case["pairs"], parameters, within)
    rng = np.random.default_rng(6)
    crowd = np.concatenate([rng.permutation(36), rng.integers(0, 36, size=64)])   # with repeats
    pairs = case["pairs"][crowd]
    keeper = align.AlignWorkspace()
    first = _paths(case, pairs, parameters, within, workspace=keeper)
    again = _paths(case, pairs, parameters, within, workspace=keeper)
    assert _same_paths(first, again) and G._same_bits(first[4], again[4])
    assert _same_paths(first, _pick(grid, crowd))
    # exactly one wave's need: a single wave serves all 100 pairs in turn
    one_wave = gpu.gfy_align_global_trace_workspace_bytes(1, max(ROWS_A), max(ROWS_B)) // WAVES
    narrow = _paths(case, pairs, parameters, within, max_workspace_bytes=one_wave)
    assert _same_paths(first, narrow) and G._same_bits(first[4], narrow[4])
    plain = _scores(case, pairs, parameters, within, workspace=keeper)
    assert G._same_bits(plain[0], first[0]) and G._same_bits(plain[1], first[2])
    for count in (WAVES - 1, WAVES + 1):            # the pairs of one workgroup, one more
        got = _paths(case, [[5, 5]] * count, parameters, within)
        assert _same_paths(got, _pick(grid, [35] * count))


# 7
@pytest.mark.parametrize("within", MODES)
def test_edges_empty_records_one_cell_self_alignment_no_pair(within):
    rng = np.random.default_rng(9)
    rows = G._unitish(rng, 129 + 40 + 1).astype(np.float16)
    dev = torch.from_numpy(rows).cuda()
    counts_a, counts_b = [0, 129, 40, 1, 0], [129, 0, 40, 1]
    common = dict(counts_a=counts_a, counts_b=counts_b, gap_open=1.0, gap_extend=0.5, within=within)
    pairs = [[0, 0], [1, 1], [0, 1], [4, 2], [3, 3], [1, 0], [2, 2]]
    scores, starts, ends, paths, _ = _host(align.global_paths(dev, dev, pairs=pairs, **common))
    for p in range(4):                              # a record of zero rows on either side
        assert scores[p] == 0 and tuple(starts[p]) == tuple(ends[p]) == (-1, -1), p
        assert paths[p].size == 0
    # 1 x 1: the row with itself
    C = distance.pairwise(dev[169:170], dev[169:170], metric="cosine").cpu().numpy()
    _same_path((scores[4], starts[4], ends[4], paths[4]),
               GO.path_of(O.substitution_f32(C, 1.0, 0.0), 1.0, 0.5, within))
    assert paths[4].tolist() == [0] and tuple(ends[4]) == (0, 0)
    # a record with itself: the diagonal
    for p, size in ((5, 129), (6, 40)):
        assert paths[p].tolist() == [0] * size and tuple(starts[p]) == (0, 0)
        assert tuple(ends[p]) == (size - 1, size - 1) and abs(scores[p] - size) < 0.01
    # b omitted
    scores, ends = align.global_align(dev, counts_a=[129, 40, 1], pairs=[[1, 1]], gap_open=1.0,
                                      gap_extend=0.5, within=within)
    assert ends.cpu().numpy().tolist() == [[39, 39]]
    # no pair at all
    none = np.zeros((0, 2), dtype=np.int64)
    scores, ends = align.global_align(dev, dev, pairs=none, **common)
    assert scores.shape == (0,) and ends.shape == (0, 2) and scores.is_cuda
    empty = align.global_paths(dev, dev, pairs=none, **common)
    assert empty.scores.shape == (0,) and empty.starts.shape == (0, 2) and empty.ops.shape == (0,)
    assert empty.offsets.tolist() == [0] and empty.ops.dtype == torch.uint8 and empty.ops.is_cuda


@pytest.mark.parametrize("within", MODES)
def test_the_longest_record_against_a_short_one(within):
    """4096 rows (the limit, 64 strips; a border iterated 4096 times) against 40 rows, and the
    other way round (one strip, 128 b-tiles)."""
    rng = np.random.default_rng(4096)
    long = G._unitish(rng, 4096)
    short = G._unitish(rng, 40)
    short[5:35] = long[3000:3030] + 0.02 * rng.standard_normal((30, 128))
    long_dev = torch.from_numpy(long.astype(np.float16)).cuda()
    short_dev = torch.from_numpy(short.astype(np.float16)).cuda()
    parameters = (1.0, -0.3, 1.0, 0.25)
    for A, B in ((long_dev, short_dev), (short_dev, long_dev)):
        want = GO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25, within)
        assert want[3].size >= 4096 or (within and A is short_dev)
        _same_path(_single(A, B, parameters, within), want)


# 8
def test_raw_calls_refuse_what_they_cannot_serve(gpu):
    rng = np.random.default_rng(12)
    a = torch.from_numpy(G._unitish(rng, 4097 + 70).astype(np.float16)).cuda()
    b = torch.from_numpy(G._unitish(rng, 90).astype(np.float16)).cuda()
    ptr_a = torch.tensor([0, 4097, 4167], dtype=torch.int32).cuda()
    ptr_b = torch.tensor([0, 90], dtype=torch.int32).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def head(pairs):
        return (a.data_ptr(), a.shape[0], ptr_a.data_ptr(), 2, b.data_ptr(), b.shape[0],
                ptr_b.data_ptr(), 1, pairs.data_ptr(), pairs.shape[0], 1.0, 0.0, 1.0, 0.5)

    def score_call(pair_list, within, columns=4096):
        pairs = torch.tensor(pair_list, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_workspace_bytes(count, columns)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        native.check(gpu.gfy_align_global(*head(pairs), within, scores.data_ptr(), ends.data_ptr(),
                                          scratch.data_ptr(), need, stream), "gfy_align_global")
        torch.cuda.synchronize()
        return scores.cpu().numpy(), ends.cpu().numpy()

    def trace_call(pair_list, within, end_list, slot_sizes, rows=70, cols=90):
        pairs = torch.tensor(pair_list, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        ends = torch.tensor(end_list, dtype=torch.int32).cuda()
        op_ptr = torch.tensor(np.concatenate(([0], np.cumsum(slot_sizes))), dtype=torch.int64).cuda()
        ops = torch.full((int(sum(slot_sizes)),), 9, dtype=torch.uint8).cuda()      # the sentinel
        lengths = torch.full((count,), 7, dtype=torch.int32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_global_trace_workspace_bytes(count, rows, cols)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        native.check(gpu.gfy_align_global_trace(
            *head(pairs), within, ends.data_ptr(), op_ptr.data_ptr(), ops.data_ptr(),
            lengths.data_ptr(), starts.data_ptr(), rows, cols, scratch.data_ptr(), need, stream),
            "gfy_align_global_trace")
        torch.cuda.synchronize()
        bounds = op_ptr.cpu().numpy()
        ops = ops.cpu().numpy()
        return (lengths.cpu().numpy(), starts.cpu().numpy(),
                [ops[bounds[p]:bounds[p + 1]] for p in range(count)])

    pair_list = [[1, 0], [0, 0], [2, 0], [1, 0], [-1, 0], [1, 1], [1, -5], [1, 0], [2 ** 31 - 1, 0]]
    bad = [1, 2, 4, 5, 6, 8]
    for within in (0, 1):
        scores, ends = score_call(pair_list, within)
        clean_scores, clean_ends = score_call([[1, 0]], within)
        assert tuple(clean_ends[0]) == (69, 89) or within
        for p in range(len(pair_list)):
            if p in bad:
                assert np.isnan(scores[p]) and tuple(ends[p]) == (-2, -2), (p, scores[p], ends[p])
            else:
                assert G._same_bits(scores[p:p + 1], clean_scores)
                assert G._same_bits(ends[p:p + 1], clean_ends)
        # a carry sized for shorter b-records than the pair names
        scores, ends = score_call([[1, 0]], within, columns=32)
        assert np.isnan(scores[0]) and ends.tolist() == [[-2, -2]]
        # the trace: a good pair between pairs it has to refuse; a slot of Lq + Lr - 1 bytes
        # where Lq + Lr are needed; an end the score call cannot have named
        end = clean_ends[0].tolist()
        need = 70 + end[1] + 1
        lengths, starts, slots = trace_call(
            [[1, 0], [0, 0], [1, 0], [5, 0], [1, 0], [1, 0]], within,
            [end, end, end, end, [68, end[1]], [69, 90]], [need, need, need - 1, need, need, need])
        assert lengths[0] > 0 and starts[0].tolist() == [0, need - 70 - np.count_nonzero(slots[0][:lengths[0]] != 2)]
        assert np.all(slots[0][:lengths[0]] <= 2) and np.all(slots[0][lengths[0]:] == 9)
        for p in range(1, 6):
            assert lengths[p] == -2 and starts[p].tolist() == [-2, -2], (p, lengths, starts)
            assert np.all(slots[p] == 9), p
        if not within:                              # global: only the last cell is an end
            lengths, starts, slots = trace_call([[1, 0]], within, [[69, 88]], [160])
            assert lengths[0] == -2 and np.all(slots[0] == 9)
        # a region too small for the box: the workspace cut for 70 x 64 boxes, or for 69 rows
        for rows, cols in ((70, 64), (69, 90)):
            lengths, starts, slots = trace_call([[1, 0]], 0, [[69, 89]], [160], rows=rows, cols=cols)
            assert lengths[0] == -2 and starts[0].tolist() == [-2, -2] and np.all(slots[0] == 9)
        # (-1, -1): nothing to align, an empty path
        lengths, starts, slots = trace_call([[1, 0]], within, [[-1, -1]], [160])
        assert lengths[0] == 0 and starts[0].tolist() == [-1, -1] and np.all(slots[0] == 9)
