"""The aligned path of the local aligner on the device (align.local_paths, gfy_align_trace).

Bit for bit and element for element against tests/align_path_oracle.py: the substitution matrix
of a pair is taken from the device itself (``distance.pairwise(A, B, metric="cosine")``), scaled
and shifted in numpy float32, and the oracle runs the recurrences and the walk of include/gfy.h
on the FULL matrix in float32, while the device walks the box start..end alone.  Ops, offsets,
scores, starts and ends must be equal, and scores, starts and ends equal ``local_spans``'.  The
records, the planted copies and the four parameter sets are those of tests/test_gpu_align.py,
whose cached case is shared."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_oracle as O
import align_path_oracle as PO
import test_gpu_align as G
import test_gpu_align_span as GS
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, PARAMETERS, WAVES = G.ROWS_A, G.ROWS_B, G.PARAMETERS, G.WAVES


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _host(result):
    """AlignedPaths on the host: (scores, starts, ends, [ops of pair 0, ...], offsets)."""
    assert isinstance(result, align.AlignedPaths)
    count = result.scores.shape[0]
    assert result.scores.dtype == torch.float32 and result.scores.shape == (count,)
    assert result.starts.dtype == torch.int32 and result.starts.shape == (count, 2)
    assert result.ends.dtype == torch.int32 and result.ends.shape == (count, 2)
    assert result.ops.dtype == torch.uint8 and result.ops.dim() == 1
    assert result.offsets.dtype == torch.int64 and result.offsets.shape == (count + 1,)
    assert all(x.is_cuda for x in result)
    offsets, ops = result.offsets.cpu().numpy(), result.ops.cpu().numpy()
    assert offsets[0] == 0 and offsets[-1] == ops.size and np.all(np.diff(offsets) >= 0)
    paths = [ops[offsets[p]:offsets[p + 1]] for p in range(count)]
    return (result.scores.cpu().numpy(), result.starts.cpu().numpy(), result.ends.cpu().numpy(),
            paths, offsets)


def _paths(case, pairs, parameters, **more):
    scale, shift, go, ge = parameters
    return _host(align.local_paths(
        case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs, gap_open=go,
        gap_extend=ge, match_scale=scale, match_shift=shift, **more))


def _single(A, B, parameters):
    scale, shift, go, ge = parameters
    scores, starts, ends, paths, _ = _host(align.local_paths(
        A, B, counts_a=[A.shape[0]], counts_b=[B.shape[0]], pairs=[[0, 0]], gap_open=go,
        gap_extend=ge, match_scale=scale, match_shift=shift))
    return scores[0], starts[0], ends[0], paths[0]


def _same_path(got, want, where=None):
    """Device (score, start, end, ops) against the oracle's, bit for bit."""
    GS._same_span(got[:3], want[:3], where)
    assert got[3].dtype == np.uint8 and got[3].tobytes() == want[3].tobytes(), \
        (where, got[3].tolist(), want[3].tolist())


def _same_paths(one, two):
    return all(G._same_bits(x, y) for x, y in zip(one[:3], two[:3])) and \
        len(one[3]) == len(two[3]) and all(G._same_bits(x, y) for x, y in zip(one[3], two[3]))


def _pick(result, index):
    scores, starts, ends, paths, _ = result
    return scores[index], starts[index], ends[index], [paths[p] for p in index]


@functools.lru_cache(maxsize=None)
def _grid(parameters):
    """The device's paths of the 6 x 6 pairs under one parameter set, computed once."""
    case = G._case()
    return _paths(case, case["pairs"], parameters)


# 1
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_paths_equal_the_oracle_bit_for_bit(parameters):
    case = G._case()
    scale, shift, go, ge = parameters
    scores, starts, ends, paths, offsets = _grid(parameters)
    total, unaligned = 0, set()
    for p, (q, r) in enumerate(case["pairs"]):
        S = O.substitution_f32(case["cosines"][p], scale, shift)
        want = PO.path_of(S, go, ge)
        _same_path((scores[p], starts[p], ends[p], paths[p]), want,
                   (ROWS_A[q], ROWS_B[r], parameters))
        assert offsets[p] == total
        total += want[3].size
        if case["planted"][p]:
            assert paths[p].size >= 30, (ROWS_A[q], ROWS_B[r], paths[p].size)
            unaligned.add((int(starts[p][1]) % 8 != 0, int(ends[p][1] - starts[p][1] + 1) % 8 != 0))
    assert offsets[-1] == total
    assert (True, True) in unaligned      # boxes begin off a word's edge and end inside a word
    span = GS._grid(parameters)
    assert all(G._same_bits(x, y) for x, y in zip((scores, starts, ends), span))


# 2
@pytest.mark.parametrize("transposed", (False, True))
def test_a_gap_across_the_strip_edge(transposed):
    """The signed-basis case of test_gpu_align_span: 60 matches, a gap of 8 over positions 60..67
    of the long record (across the edge at 64) and 40 matches."""
    rng = np.random.default_rng(64)
    signs = rng.choice([-1.0, 1.0], 100)
    short = GS._basis_rows(np.arange(100), signs)
    foreign = GS._basis_rows(np.arange(100, 108), np.ones(8))
    long = np.concatenate([short[:60], foreign, short[60:]])
    A, B = (short, long) if transposed else (long, short)
    A, B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    parameters = (1.0, -0.25, 1.0, 0.25)
    want = PO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25)
    gap = 1 if transposed else 2
    assert want[3].tolist() == [0] * 60 + [gap] * 8 + [0] * 40
    assert want[:3] == (np.float32(72.25), (0, 0), (99, 107) if transposed else (107, 99))
    _same_path(_single(A, B, parameters), want)


# 3
def test_a_path_over_two_strip_edges():
    rng = np.random.default_rng(128)
    segment = G._unitish(rng, 100)
    rows = G._unitish(rng, 200)
    rows[30:130] = segment + 0.02 * rng.standard_normal((100, 128))
    A = torch.from_numpy(rows.astype(np.float16)).cuda()
    B = torch.from_numpy(segment.astype(np.float16)).cuda()
    for parameters in (PARAMETERS[0], PARAMETERS[2]):
        want = PO.path_of(GS._substitution(A, B, parameters), parameters[2], parameters[3])
        assert want[0] > 40 and want[1][0] < 64 and want[2][0] >= 128    # strips 0, 1 and 2
        assert want[3].size >= 100
        _same_path(_single(A, B, parameters), want)


# 4
@pytest.mark.parametrize("transposed", (False, True))
def test_ties_walk_the_first_copy(transposed):
    X, doubled = G._tie_rows()
    A, B = (doubled, X) if transposed else (X, doubled)
    A, B = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    parameters = (1.0, -0.5, 1.0, 1.0)                  # gap_open == gap_extend
    want = PO.path_of(GS._substitution(A, B, parameters), 1.0, 1.0)
    assert want[0] > 15 and want[1:3] == ((0, 0), (39, 39)) and want[3].tolist() == [0] * 40
    _same_path(_single(A, B, parameters), want)


# 5
def test_a_path_does_not_depend_on_its_company_the_run_or_the_workspace(gpu):
    case = G._case()
    parameters = PARAMETERS[0]
    pair = [5, 5]                                   # 200 x 330: four strips, eleven b-tiles
    alone = _paths(case, [pair], parameters)
    assert alone[0][0] > 10 and alone[3][0].size >= 30
    for count in (WAVES - 1, WAVES, WAVES + 1):     # the pairs of one workgroup, one more
        got = _paths(case, [pair] * count, parameters)
        for p in range(count):
            assert _same_paths(_pick(got, [p]), alone)
    rng = np.random.default_rng(3)
    crowd = rng.integers(0, 6, size=(300, 2)).astype(np.int32)
    for seat in (0, 150, 299):
        crowd[seat] = pair
    keeper = align.AlignWorkspace()
    first = _paths(case, crowd, parameters, workspace=keeper)
    again = _paths(case, crowd, parameters, workspace=keeper)
    assert _same_paths(first, again) and G._same_bits(first[4], again[4])
    # exactly one wave's need: a single wave serves all 300 pairs in turn
    boxes = np.where(first[1] < 0, 0, first[2] - first[1] + 1)
    one_wave = gpu.gfy_align_trace_workspace_bytes(1, int(boxes[:, 0].max()),
                                                   int(boxes[:, 1].max())) // WAVES
    narrow = _paths(case, crowd, parameters, max_workspace_bytes=one_wave)
    assert _same_paths(first, narrow) and G._same_bits(first[4], narrow[4])
    for seat in (0, 150, 299):
        assert _same_paths(_pick(first, [seat]), alone)
    index = crowd[:, 0] * 6 + crowd[:, 1]
    assert _same_paths(first, _pick(_grid(parameters), index))
    # the workspace serves local_spans as well, after the paths
    spans = GS._spans(case, crowd, parameters, workspace=keeper)
    assert all(G._same_bits(x, y) for x, y in zip(spans, first[:3]))


# 6
def test_edges_empty_records_nothing_positive_self_alignment():
    rng = np.random.default_rng(9)
    rows = G._unitish(rng, 129 + 40).astype(np.float16)
    dev = torch.from_numpy(rows).cuda()
    counts_a, counts_b = [0, 129, 40, 0], [129, 0, 40]
    common = dict(counts_a=counts_a, counts_b=counts_b, gap_open=1.0, gap_extend=0.5)
    pairs = [[0, 0], [1, 1], [0, 1], [3, 2], [1, 0], [2, 2]]
    scores, starts, ends, paths, offsets = _host(align.local_paths(dev, dev, pairs=pairs, **common))
    for p in range(4):                              # a record of zero rows on either side
        assert scores[p] == 0 and tuple(starts[p]) == (-1, -1) == tuple(ends[p]), p
        assert paths[p].size == 0
    assert paths[4].tolist() == [0] * 129 and paths[5].tolist() == [0] * 40
    assert offsets.tolist() == [0, 0, 0, 0, 0, 129, 169]
    # nothing positive: cosine - 2 <= 0 everywhere
    scores, starts, ends, paths, offsets = _host(align.local_paths(dev, dev, pairs=pairs,
                                                                  match_shift=-2.0, **common))
    assert np.all(scores == 0) and np.all(starts == -1) and np.all(ends == -1)
    assert all(path.size == 0 for path in paths) and offsets.tolist() == [0] * 7
    # b omitted: a record with itself is all matches, as long as the record
    scores, starts, ends, paths, offsets = _host(align.local_paths(
        dev, counts_a=[129, 40], pairs=[[0, 0], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5))
    for p, (lo, hi) in enumerate(((0, 129), (129, 169))):
        want = PO.path_of(GS._substitution(dev[lo:hi], dev[lo:hi], (1.0, 0.0)), 1.0, 0.5)
        assert want[3].tolist() == [0] * (hi - lo)
        _same_path((scores[p], starts[p], ends[p], paths[p]), want)
    want = PO.path_of(GS._substitution(dev[129:169], dev[0:129], (1.0, 0.0)), 1.0, 0.5)
    _same_path((scores[2], starts[2], ends[2], paths[2]), want)
    # no pair at all
    result = align.local_paths(dev, counts_a=[129, 40], pairs=np.zeros((0, 2), dtype=np.int64),
                               gap_open=1.0, gap_extend=0.5)
    scores, starts, ends, paths, offsets = _host(result)
    assert scores.shape == (0,) and starts.shape == (0, 2) and ends.shape == (0, 2)
    assert result.ops.shape == (0,) and offsets.tolist() == [0]


# 7
def test_a_box_far_from_the_origin():
    """4096 rows against 64 and the other way round, the copy in the long record's last 40 rows
    (test_gpu_align_span.test_coordinates_at_the_packing_limit): the box lies far from (0, 0)."""
    rng = np.random.default_rng(4095)
    long = G._unitish(rng, 4096)
    short = G._unitish(rng, 64)
    short[10:50] = long[4056:4096] + 0.02 * rng.standard_normal((40, 128))
    long_dev = torch.from_numpy(long.astype(np.float16)).cuda()
    short_dev = torch.from_numpy(short.astype(np.float16)).cuda()
    parameters = (1.0, -0.3, 1.0, 0.25)
    for side, (A, B) in enumerate(((long_dev, short_dev), (short_dev, long_dev))):
        want = PO.path_of(GS._substitution(A, B, parameters), 1.0, 0.25)
        assert want[0] > 10 and want[2][side] == 4095 and want[1][side] >= 4050, want[:3]
        assert want[3].size >= 30
        _same_path(_single(A, B, parameters), want)


# 8
def test_raw_call_refuses_boxes_it_cannot_serve(gpu):
    """The C call with boxes that are no box of their records, a slot one byte short, a workspace
    cut for a smaller box and a bad record index: those pairs get out_len = -2 and their slots
    stay as they were, their neighbours get what they get alone.  A box that is valid but not an
    alignment's own returns the walk of the recurrences on that box."""
    rng = np.random.default_rng(21)
    segment = G._unitish(rng, 60)
    rows_a, rows_b = G._unitish(rng, 90), G._unitish(rng, 130)
    rows_a[20:80] = segment + 0.02 * rng.standard_normal((60, 128))
    rows_b[50:110] = segment + 0.02 * rng.standard_normal((60, 128))
    a = torch.from_numpy(rows_a.astype(np.float16)).cuda()
    b = torch.from_numpy(rows_b.astype(np.float16)).cuda()
    ptr_a = torch.tensor([0, 90], dtype=torch.int32).cuda()
    ptr_b = torch.tensor([0, 130], dtype=torch.int32).cuda()
    parameters = (1.0, -0.3, 1.0, 0.25)
    S = GS._substitution(a, b, parameters)
    score, start, end, ops = PO.path_of(S, 1.0, 0.25)
    assert score > 10 and ops.size >= 50 and start[0] > 0 and start[1] > 0
    rows, cols = end[0] - start[0] + 1, end[1] - start[1] + 1
    full = rows + cols - 1
    corner = PO.box_path(np.ascontiguousarray(S[:20, :20]), 1.0, 0.25)
    inner = (start[0] + 5, start[1] + 5), (end[0] - 5, end[1] - 5)    # valid, not an alignment's own
    inner_ops = PO.box_path(np.ascontiguousarray(
        S[inner[0][0]:inner[1][0] + 1, inner[0][1]:inner[1][1] + 1]), 1.0, 0.25)
    assert inner_ops.size >= 30
    #        pair    start           end             slot bytes   refused
    cases = [((0, 0), start, end, full, False),
             ((0, 0), end, start, full, True),                         # a start after the end
             ((0, 0), start, (90, end[1]), full + 90, True),           # an end past the a-record
             ((0, 0), start, (end[0], 130), full + 130, True),         # ... past the b-record
             ((0, 0), start, end, full, False),
             ((0, 0), (-1, start[1]), end, full + 90, True),           # a negative start
             ((0, 0), (start[0], -3), end, full + 130, True),
             ((0, 0), (-1, -1), (-1, -1), 5, False),                   # the empty alignment
             ((0, 0), start, end, full - 1, True),                     # a slot one byte short
             ((1, 0), start, end, full, True),                         # a bad record index
             ((0, -1), start, end, full, True),
             ((0, 0), (0, 0), (19, 19), 39, False),                    # the top-left 20 x 20
             ((0, 0), inner[0], inner[1], full, False),
             ((0, 0), start, end, full + 7, False)]

    def call(chosen, box_rows=rows, box_cols=cols, waves=None):
        pairs = torch.tensor([c[0] for c in chosen], dtype=torch.int32).cuda()
        starts = torch.tensor([c[1] for c in chosen], dtype=torch.int32).cuda()
        ends = torch.tensor([c[2] for c in chosen], dtype=torch.int32).cuda()
        op_ptr = np.concatenate(([0], np.cumsum([c[3] for c in chosen]))).astype(np.int64)
        count = len(chosen)
        slots = torch.full((int(op_ptr[-1]),), 9, dtype=torch.uint8).cuda()
        lengths = torch.full((count,), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_trace_workspace_bytes(count, box_rows, box_cols)
        if waves is not None:
            need = need // (WAVES * ((count + WAVES - 1) // WAVES)) * waves
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        op_ptr_dev = torch.from_numpy(op_ptr).cuda()
        native.check(gpu.gfy_align_trace(
            a.data_ptr(), 90, ptr_a.data_ptr(), 1, b.data_ptr(), 130, ptr_b.data_ptr(), 1,
            pairs.data_ptr(), count, *parameters, starts.data_ptr(), ends.data_ptr(),
            op_ptr_dev.data_ptr(), slots.data_ptr(), lengths.data_ptr(), box_rows, box_cols,
            scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "gfy_align_trace")
        torch.cuda.synchronize()
        slots = slots.cpu().numpy()
        return lengths.cpu().numpy(), [slots[op_ptr[p]:op_ptr[p + 1]] for p in range(count)]

    wanted = {0: ops, 4: ops, 7: np.zeros(0, dtype=np.uint8), 11: corner, 12: inner_ops, 13: ops}
    for waves in (None, 1):          # every wave of the grid; one wave for all the pairs
        lengths, slots = call(cases, waves=waves)
        for p, case in enumerate(cases):
            if case[4]:
                assert lengths[p] == -2 and np.all(slots[p] == 9), (p, lengths[p])
            else:
                assert lengths[p] == wanted[p].size, (p, lengths[p], wanted[p].size)
                assert slots[p][:lengths[p]].tobytes() == wanted[p].tobytes(), p
                assert np.all(slots[p][lengths[p]:] == 9), p      # the rest of the slot is untouched
    alone = call([cases[0]])
    assert alone[0][0] == ops.size and alone[1][0][:ops.size].tobytes() == ops.tobytes()
    # a workspace cut for a smaller box: the pair whose box does not fit is refused, the corner
    # (20 x 20) is served
    lengths, slots = call([cases[0], cases[11], cases[4]], box_rows=20, box_cols=24)
    assert lengths.tolist() == [-2, corner.size, -2]
    assert np.all(slots[0] == 9) and np.all(slots[2] == 9)
    assert slots[1][:corner.size].tobytes() == corner.tobytes()
