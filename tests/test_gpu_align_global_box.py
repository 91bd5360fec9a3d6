"""Global and query-in-target alignment inside a box of rows per pair on the device (the ``box``
of align.global_align and global_paths; gfy_align_global_box, gfy_align_global_trace_box).

Everything is bit for bit, for both ``within`` values and with no tolerance anywhere: against
tests/align_global_box_oracle.py (the global oracle on the sliced substitution matrix, the cells
shifted back), against the calls without a box on the gathered slices (rows ``i_lo..i_hi`` and
``j_lo..j_hi`` copied out as records of their own), and between ``global_align`` and
``global_paths``.  The records are those of tests/test_gpu_align_box.py, letters of
tests/align_cases.py: every cosine is exactly 0, +1 or -1, so the substitution matrix is known
exactly on the host and the tie rules decide most cells; one test takes the random rows of
tests/test_gpu_align.py and the device's own cosines, where every sum is rounded.  The boxes put
every edge of the loop (strip 64, b-tile 32, the 128-diagonal ring, the two carry buffers, the
direction word 8) at the start, the end and the inside of a box."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_box_oracle as XO
import align_cases as Z
import align_global_box_oracle as GXO
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import test_gpu_align as G
import test_gpu_align_box as GB
import test_gpu_align_global as GG
from ginfinity_amd import _native as native
from ginfinity_amd import align

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, PARAMETERS = GB.ROWS_A, GB.ROWS_B, GB.PARAMETERS     # 130 200 0 150 x 140 170 131 0
MODES = (False, True)                                                # within
PAIRS = GB.PAIRS


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _bytes(value) -> bytes:
    return np.float32(value).tobytes()


def _call(function, pairs, boxes, within, parameters=PARAMETERS, **more):
    case = GB._case()
    return function(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs,
                    within=within, box=boxes, **GG._keywords(parameters), **more)


def _device(pairs, boxes, within, parameters=PARAMETERS, **more):
    """``global_paths`` on the host, after ``global_align`` gave the same scores and ends."""
    paths = GG._host(_call(align.global_paths, pairs, boxes, within, parameters, **more))
    scores, ends = (x.cpu().numpy() for x in _call(align.global_align, pairs, boxes, within, parameters))
    assert G._same_bits(scores, paths[0]) and G._same_bits(ends, paths[2])
    return paths


def _gathered(pairs, boxes, within, parameters=PARAMETERS):
    """The calls WITHOUT a box on the rows of every box copied out as two records of their own,
    the cells shifted back: (scores, starts, ends, paths)."""
    case = GB._case()
    rows_a, rows_b, corners = [], [], []
    for (q, r), box in zip(pairs, boxes):
        inside = XO.clipped(box, ROWS_A[q], ROWS_B[r])
        i_lo, i_hi, j_lo, j_hi = inside if inside else (0, -1, 0, -1)
        rows_a.append(case["rec_a"][q][i_lo:i_hi + 1])
        rows_b.append(case["rec_b"][r][j_lo:j_hi + 1])
        corners.append((i_lo, j_lo))
    count = len(rows_a)
    scores, starts, ends, paths, _ = GG._host(align.global_paths(
        torch.from_numpy(np.concatenate(rows_a)).cuda(), torch.from_numpy(np.concatenate(rows_b)).cuda(),
        counts_a=[x.shape[0] for x in rows_a], counts_b=[x.shape[0] for x in rows_b],
        pairs=np.stack([np.arange(count), np.arange(count)], axis=1), within=within,
        **GG._keywords(parameters)))
    back = np.array(corners, dtype=np.int32)
    found = starts[:, 0] >= 0
    starts, ends = starts.copy(), ends.copy()
    starts[found] += back[found]
    ends[found] += back[found]
    return scores, starts, ends, paths


def _check(pairs, boxes, within, parameters=PARAMETERS, substitution=GB._substitution):
    """The device under ``boxes`` against the oracle and against the gathered slices; returns
    the oracle's answers."""
    go, ge = parameters[2:]
    got = _device(pairs, boxes, within, parameters)
    assert GG._same_paths(got[:4], _gathered(pairs, boxes, within, parameters))
    wanted = []
    for p, ((q, r), box) in enumerate(zip(pairs, boxes)):
        S = substitution(q, r, parameters)
        want = GXO.box_path_of(S, go, ge, box, within)
        where = ((q, r), tuple(box), within)
        GG._same_path((got[0][p], got[1][p], got[2][p], got[3][p]), want, where)
        if want[2] != (-1, -1):
            assert _bytes(PO.rescore(S, got[3][p], want[1], go, ge)) == _bytes(got[0][p]), where
        wanted.append(want)
    return wanted


# the places where the loop changes: every first row with every number of rows, every first
# column with every number of columns, the other side taken in turn
EDGE_ROWS = [(i_lo, rows) for i_lo in (0, 1, 63, 64, 65) for rows in (1, 63, 64, 65, 129)]
EDGE_COLS = [(j_lo, cols) for j_lo in (0, 1, 31, 32, 33) for cols in (1, 31, 32, 33, 65, 130)]


def _edge_boxes():
    boxes = []
    for n, (i_lo, rows) in enumerate(EDGE_ROWS):
        j_lo, cols = EDGE_COLS[(7 * n) % len(EDGE_COLS)]
        boxes.append((i_lo, i_lo + rows - 1, j_lo, j_lo + cols - 1))
    for n, (j_lo, cols) in enumerate(EDGE_COLS):
        i_lo, rows = EDGE_ROWS[(11 * n + 3) % len(EDGE_ROWS)]
        boxes.append((i_lo, i_lo + rows - 1, j_lo, j_lo + cols - 1))
    return boxes


# box edges
@pytest.mark.parametrize("within", MODES)
def test_boxes_at_the_places_where_the_loop_changes(within):
    boxes = _edge_boxes()
    assert {(b[0], b[1] - b[0] + 1) for b in boxes} == set(EDGE_ROWS)
    assert {(b[2], b[3] - b[2] + 1) for b in boxes} == set(EDGE_COLS)
    assert max(b[1] for b in boxes) < ROWS_A[1] and max(b[3] for b in boxes) < ROWS_B[1]
    wanted = _check([(1, 1)] * len(boxes), boxes, within)
    assert max(want[0] for want in wanted) > 10 and min(want[0] for want in wanted) < -10
    if within:
        assert len({want[2][1] - box[3] for want, box in zip(wanted, boxes)}) > 5    # ends inside
    # the same boxes of the other related pair, whose a-record ends inside its third strip
    other = [(i_lo, min(i_hi, ROWS_A[0] + 3), j_lo, min(j_hi, ROWS_B[0] + 3))
             for i_lo, i_hi, j_lo, j_hi in boxes[::3]]
    _check([(0, 0)] * len(other), other, within)


# clipping
@pytest.mark.parametrize("within", MODES)
def test_a_box_hanging_over_a_record_edge_equals_its_clipped_self(within):
    lq, lr = ROWS_A[1], ROWS_B[1]
    hanging = [(-5, 70, 10, 90), (120, lq + 7, 10, 90), (30, 100, -2, 60), (30, 100, 100, lr + 9),
               (-4096, 4096, 100, 5000), (150, 5000, -4096, 60), (-10 ** 6, 3, -10 ** 6, 3)]
    inside = [XO.clipped(box, lq, lr) for box in hanging]
    assert all(one != tuple(two) for one, two in zip(inside, hanging))
    pairs = [(1, 1)] * len(hanging)
    wanted = _check(pairs, hanging, within)
    got = _device(pairs, inside, within)
    for p, want in enumerate(wanted):
        GG._same_path((got[0][p], got[1][p], got[2][p], got[3][p]), want, hanging[p])
        assert want[1][0] == inside[p][0] and want[2][0] == inside[p][1]


# consequence 1
@pytest.mark.parametrize("within", MODES)
@pytest.mark.parametrize("parameters", Z.TIE_PARAMETERS[:2])
def test_a_covering_box_equals_the_calls_without_a_box(parameters, within):
    pairs = PAIRS + [(2, 1), (1, 3)]                         # and a record of zero rows on either side
    exact = [XO.covering(max(ROWS_A[q], 1), max(ROWS_B[r], 1)) for q, r in pairs]
    plain = GG._host(_call(align.global_paths, pairs, None, within, parameters))
    assert plain[0].max() > 10 and np.count_nonzero(plain[2][:, 0] == -1) == 2
    for boxes in (exact, np.array(exact) + np.array([-3, 5, -1, 2]), (0, 4095, 0, 4095),
                  (-10 ** 6, 10 ** 6, -10 ** 6, 10 ** 6)):
        got = _device(pairs, boxes, within, parameters)
        assert GG._same_paths(got, plain) and G._same_bits(got[4], plain[4])


@functools.lru_cache(maxsize=None)
def _bordered():
    """A record of 140 letters and one of 60 whose rows 10 .. 39 are rows 90 .. 119 of the first:
    in the box (20, 119, 10, 39), 100 rows by 30 columns, the best path is a gap of 70 a-rows down
    the left border, over the strip edge, and then the diagonal."""
    rng = np.random.default_rng(20261022)
    A, B = Z.letters(rng, 140), Z.letters(rng, 60)
    B[10:40] = A[90:120]
    S = O.substitution_f32(A.astype(np.float32) @ B.astype(np.float32).T, *PARAMETERS[:2])
    return torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), S


def _bordered_paths(box, within, parameters=PARAMETERS):
    A, B, _ = _bordered()
    common = dict(counts_a=[140], counts_b=[60], pairs=[[0, 0]], within=within, box=box,
                  **GG._keywords(parameters))
    scores, starts, ends, paths, _ = GG._host(align.global_paths(A, B, **common))
    score, end = align.global_align(A, B, **common)
    assert G._same_bits(score.cpu().numpy(), scores) and G._same_bits(end.cpu().numpy(), ends)
    return scores[0], starts[0], ends[0], paths[0]


# borders at the box's edge
@pytest.mark.parametrize("within", MODES)
def test_the_borders_lie_at_the_edges_of_the_box(within):
    go, ge = PARAMETERS[2:]
    S = _bordered()[2]
    # a left border of more than 64 rows: 70 ops 2, then 30 matches
    box = (20, 119, 10, 39)
    want = GXO.box_path_of(S, go, ge, box, within)
    assert want[3].tolist() == [2] * 70 + [0] * 30 and want[1] == (20, 10) and want[2] == (119, 39)
    assert _bytes(want[0]) == _bytes(30 * 0.75 - (go + 69 * ge))
    GG._same_path(_bordered_paths(box, within), want)
    # the mirror image: a top border of 10 columns in front of the diagonal, charged or free
    box = (90, 119, 0, 39)
    want = GXO.box_path_of(S, go, ge, box, within)
    assert want[2] == (119, 39) and want[3].tolist()[-30:] == [0] * 30
    assert want[1] == ((90, 10) if within else (90, 0)) and want[3].size == (30 if within else 40)
    GG._same_path(_bordered_paths(box, within), want)
    # a path that is all gaps: a match is worth less than the two gap positions that avoid it
    dear = (1.0, -3.0, 0.5, 0.25)
    S = O.substitution_f32(np.asarray(S) - np.float32(PARAMETERS[1]), 1.0, -3.0)
    for box in ((20, 119, 10, 39), (64, 64 + 65 - 1, 5, 5 + 33 - 1), (7, 7, 3, 3)):
        rows, cols = box[1] - box[0] + 1, box[3] - box[2] + 1
        want = GXO.box_path_of(S, *dear[2:], box, within)
        assert not np.any(want[3] == 0)
        if within:       # no b-row is consumed: start_j = end_j + 1, and the first best j is j_lo
            assert want[3].tolist() == [2] * rows and want[2] == (box[1], box[2])
            assert want[1] == (box[0], box[2] + 1)
        else:
            assert want[3].size == rows + cols and want[1] == (box[0], box[2])
        GG._same_path(_bordered_paths(box, within, dear), want, box)


def _random_box(rng, lq, lr):
    """A box that meets an lq x lr matrix and may reach over its ends."""
    i_lo, j_lo = int(rng.integers(-10, lq)), int(rng.integers(-10, lr))
    return (i_lo, max(i_lo, 0) + int(rng.integers(0, lq)), j_lo, max(j_lo, 0) + int(rng.integers(0, lr)))


# consequence 4
def test_global_within_local_are_ordered_in_the_same_boxes():
    rng = np.random.default_rng(4)
    pairs = [PAIRS[n % len(PAIRS)] for n in range(60)]
    boxes = [_random_box(rng, max(ROWS_A[q], 1), max(ROWS_B[r], 1)) for q, r in pairs]
    for parameters in Z.TIE_PARAMETERS[:2]:
        keywords = GG._keywords(parameters)
        case = GB._case()
        common = dict(counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs, box=boxes, **keywords)
        whole = align.global_align(case["a"], case["b"], within=False, **common)[0].cpu().numpy()
        fit = align.global_align(case["a"], case["b"], within=True, **common)[0].cpu().numpy()
        local = align.local_align(case["a"], case["b"], **common)[0].cpu().numpy()
        assert not np.isnan(whole).any() and not np.isnan(fit).any()
        assert np.all(whole <= fit) and np.all(fit <= local), (whole, fit, local)
        assert np.count_nonzero(whole < fit) > 20 and np.count_nonzero(fit < local) > 20


# consequence 6
def test_widening_the_b_side_never_lowers_a_within_score():
    pairs = [(1, 1), (0, 0), (3, 2), (1, 0)]
    rows = [(40, 160), (0, 129), (70, 70 + 64), (63, 128)]
    lo, hi, before, raised = 80, 80, None, 0
    for grow in (0, 1, 7, 24, 31, 32, 33, 64, 100, 4096):
        boxes = [(i_lo, i_hi, lo - grow, hi + grow // 2) for i_lo, i_hi in rows]
        scores = _call(align.global_align, pairs, boxes, True)[0].cpu().numpy()
        assert not np.isnan(scores).any()
        if before is not None:
            assert np.all(scores >= before), (grow, scores, before)
            raised += np.count_nonzero(scores > before)
        before = scores
    assert raised > 10
    whole = _call(align.global_align, pairs, [(i_lo, i_hi, 0, 4095) for i_lo, i_hi in rows], True)
    assert G._same_bits(before, whole[0].cpu().numpy())             # the last one covers the b-side


# consequence 5
@pytest.mark.parametrize("within", MODES)
def test_a_crowd_of_boxes_equals_the_same_pairs_one_at_a_time(gpu, within):
    """320 seats of 40 different (pair, box), more than one pair per wave of the workgroups in
    flight with the narrow workspace: a wave's next pair finds the carry, the ring and the
    direction words its last pair left, and a box of other sizes.  Each seat equals the same
    pair in a call of its own, whatever the workspace."""
    rng = np.random.default_rng(20261021)
    kinds = []
    for number in range(40):
        q, r = PAIRS[number % len(PAIRS)]
        kinds.append(((q, r), _random_box(rng, max(ROWS_A[q], 1), max(ROWS_B[r], 1))))
    kinds[7] = ((2, 1), (0, 10, 0, 10))                      # a record of zero rows
    kinds[8] = ((1, 1), (300, 400, 0, 10))                   # a box outside the record
    kinds[9] = ((1, 1), (0, 199, 0, 169))                    # the largest box of the call
    seats = np.concatenate([rng.permutation(len(kinds)), rng.integers(0, len(kinds), 280)])
    pairs, boxes = [kinds[k][0] for k in seats], [kinds[k][1] for k in seats]
    crowd = _device(pairs, boxes, within)
    assert crowd[0].max() > 10 and crowd[0].min() < -10
    alone = [GG._host(_call(align.global_paths, [pair], [box], within)) for pair, box in kinds]
    for seat, k in enumerate(seats):
        assert GG._same_paths(GG._pick(crowd, [seat]), GG._pick(alone[k], [0])), (seat, kinds[k])
    # a workspace kept across calls, and one of two waves' need: the waves share the work
    keeper = align.AlignWorkspace()
    for _ in range(2):
        kept = _device(pairs, boxes, within, workspace=keeper)
        assert GG._same_paths(kept, crowd) and G._same_bits(kept[4], crowd[4])
    two_waves = gpu.gfy_align_global_trace_workspace_bytes(1, 200, 170) // G.WAVES * 2
    narrow = _device(pairs, boxes, within, max_workspace_bytes=two_waves)
    assert GG._same_paths(narrow, crowd) and G._same_bits(narrow[4], crowd[4])
    # a sample of the kinds against the oracle
    _check([kind[0] for kind in kinds[::4]], [kind[1] for kind in kinds[::4]], within)


# degenerate inputs
@pytest.mark.parametrize("within", MODES)
def test_an_empty_box_a_record_of_zero_rows_and_no_pair(within):
    pairs = [(1, 1), (2, 1), (1, 3), (2, 3), (0, 0), (1, 1), (1, 1), (1, 1)]
    boxes = [(10, 100, 10, 100), (0, 10, 0, 10), (0, 10, 0, 10), (-5, 5, -5, 5), (20, 90, 20, 90),
             (200, 210, 0, 10), (0, 10, -9, -1), (90, 90, 77, 77)]
    wanted = _check(pairs, boxes, within)
    for index in (1, 2, 3, 5, 6):
        assert _bytes(wanted[index][0]) == _bytes(0) and wanted[index][3].size == 0
        assert wanted[index][1] == wanted[index][2] == (-1, -1)
    assert wanted[7][1][0] == wanted[7][2][0] == 90 and wanted[7][3].size in (1, 2)   # one cell
    # every box of the call is empty: no path at all, and no trace launch
    got = _device(pairs[1:4], boxes[1:4], within)
    assert got[0].tolist() == [0, 0, 0] and got[4].tolist() == [0, 0, 0, 0]
    # no pair at all
    empty = _call(align.global_paths, [], [], within)
    assert empty.scores.shape == (0,) and empty.ops.shape == (0,) and empty.offsets.tolist() == [0]
    scores, ends = _call(align.global_align, np.zeros((0, 2), dtype=np.int32),
                         np.zeros((0, 4), dtype=np.int32), within)
    assert scores.shape == (0,) and ends.shape == (0, 2) and scores.is_cuda


# rounded sums: the random rows of test_gpu_align and the device's own cosines
@pytest.mark.parametrize("within", MODES)
def test_boxes_of_records_whose_sums_are_rounded(within):
    case = G._case()
    parameters = G.PARAMETERS[0]
    go, ge = parameters[2:]
    rng = np.random.default_rng(8)
    chosen = [35, 35, 35, 28, 28, 34, 23, 20]                # 200 x 330, 129 x 257, 200 x 257, ...
    pairs = case["pairs"][chosen]
    boxes = [_random_box(rng, G.ROWS_A[q], G.ROWS_B[r]) for q, r in pairs]
    boxes[0] = (64, 199, 97, 97 + 160)                       # columns wrap the ring of 128
    common = dict(counts_a=G.ROWS_A, counts_b=G.ROWS_B, pairs=pairs, within=within, box=boxes,
                  **GG._keywords(parameters))
    got = GG._host(align.global_paths(case["a"], case["b"], **common))
    scores, ends = align.global_align(case["a"], case["b"], **common)
    assert G._same_bits(scores.cpu().numpy(), got[0]) and G._same_bits(ends.cpu().numpy(), got[2])
    for p, index in enumerate(chosen):
        S = O.substitution_f32(case["cosines"][index], *parameters[:2])
        want = GXO.box_path_of(S, go, ge, boxes[p], within)
        GG._same_path((got[0][p], got[1][p], got[2][p], got[3][p]), want, (index, boxes[p]))
        assert _bytes(PO.rescore(S, got[3][p], want[1], go, ge)) == _bytes(got[0][p])


# two regions
def test_one_box_from_the_first_anchor_to_the_last_holds_both_regions():
    """The premise is proved on the host in tests/test_align_global_box_host.py: in the box from
    the first planted cell to the last the global and the ``within`` path hold both regions and
    the linker between them, the local path only the stronger region."""
    region = XO.two_regions()
    rng = np.random.default_rng(11)
    counts_a, counts_b = [70, XO.REGION_ROWS[0]], [XO.REGION_ROWS[1], 40]
    a = torch.from_numpy(np.concatenate([Z.letters(rng, 70), region["a"]])).cuda()
    b = torch.from_numpy(np.concatenate([region["b"], Z.letters(rng, 40)])).cuda()
    scale, shift, go, ge = XO.REGION_PARAMETERS
    box = (20, 138, 27, 145)
    common = dict(counts_a=counts_a, counts_b=counts_b, pairs=[[1, 0]], box=box, gap_open=go,
                  gap_extend=ge, match_scale=scale, match_shift=shift)
    first, second = region["plants"]
    for within in MODES:
        scores, starts, ends, paths, _ = GG._host(align.global_paths(a, b, within=within, **common))
        want = GXO.box_path_of(region["S"], go, ge, box, within)
        GG._same_path((scores[0], starts[0], ends[0], paths[0]), want, within)
        cells = align.path_cells(paths[0], starts[0])
        assert XO.holds(cells, first) and XO.holds(cells, second)
        assert _bytes(scores[0]) == _bytes(-6.75) and paths[0].size == 121
    scores, starts, ends, paths, _ = GG._host(align.local_paths(a, b, **common))
    cells = align.path_cells(paths[0], starts[0])
    assert XO.holds(cells, first) and not XO.holds(cells, second)
    assert _bytes(scores[0]) == _bytes(12.5) and tuple(ends[0]) == (69, 76)
    # the whole records charge the flanks as well: not the same path
    whole = GG._host(align.global_paths(a, b, **{**common, "box": None}))
    assert whole[0][0] < -6.75 and whole[3][0].size > 190


# raw calls
def test_raw_calls_refuse_a_box_the_wrong_way_round_and_an_end_they_cannot_have_named(gpu):
    """Argument checks: the kernel compares and clips what it is given, the refused pair gets
    NaN, (-2, -2) and length -2, its slot stays untouched and its neighbours are served."""
    case = GB._case()
    ptr_a = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_A))), dtype=torch.int32).cuda()
    ptr_b = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_B))), dtype=torch.int32).cuda()
    pair_list = [(1, 1), (0, 0), (1, 1), (3, 2), (1, 1), (0, 1), (1, 1)]
    box_list = [(10, 150, 5, 160), (0, 129, 0, 139), (5, 4, 0, 10), (0, 10, 2 ** 31 - 1, -2 ** 31),
                (10, 150, 5, 160), (64, 129, 32, 100), (300, 310, 0, 9)]
    bad = (2, 3)
    rows, cols = 150 - 10 + 1, 160 - 5 + 1                   # the largest box of the call
    stream = torch.cuda.current_stream().cuda_stream
    go, ge = PARAMETERS[2:]

    def head(pairs):
        return (case["a"].data_ptr(), case["a"].shape[0], ptr_a.data_ptr(), len(ROWS_A),
                case["b"].data_ptr(), case["b"].shape[0], ptr_b.data_ptr(), len(ROWS_B),
                pairs.data_ptr(), pairs.shape[0], *PARAMETERS)

    def score_call(pair_list, box_list, within, columns=cols, null=False):
        pairs = torch.tensor(pair_list, dtype=torch.int32).cuda()
        boxes = torch.tensor(box_list, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_workspace_bytes(count, columns)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        code = gpu.gfy_align_global_box(*head(pairs), within, None if null else boxes.data_ptr(),
                                        scores.data_ptr(), ends.data_ptr(), scratch.data_ptr(),
                                        need, stream)
        torch.cuda.synchronize()
        return code, scores.cpu().numpy(), ends.cpu().numpy()

    def trace_call(pair_list, box_list, within, end_list, slot_sizes, rows=rows, cols=cols):
        pairs = torch.tensor(pair_list, dtype=torch.int32).cuda()
        boxes = torch.tensor(box_list, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        ends = torch.tensor(end_list, dtype=torch.int32).cuda()
        op_ptr = torch.tensor(np.concatenate(([0], np.cumsum(slot_sizes))), dtype=torch.int64).cuda()
        ops = torch.full((int(sum(slot_sizes)),), 9, dtype=torch.uint8).cuda()      # the sentinel
        lengths = torch.full((count,), 7, dtype=torch.int32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        need = gpu.gfy_align_global_trace_workspace_bytes(count, rows, cols)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        native.check(gpu.gfy_align_global_trace_box(
            *head(pairs), within, boxes.data_ptr(), ends.data_ptr(), op_ptr.data_ptr(),
            ops.data_ptr(), lengths.data_ptr(), starts.data_ptr(), rows, cols, scratch.data_ptr(),
            need, stream), "gfy_align_global_trace_box")
        torch.cuda.synchronize()
        bounds = op_ptr.cpu().numpy()
        ops = ops.cpu().numpy()
        return (lengths.cpu().numpy(), starts.cpu().numpy(),
                [ops[bounds[p]:bounds[p + 1]] for p in range(count)])

    code, scores, _ = score_call(pair_list, box_list, 0, null=True)
    assert code == native.GFY_ERR_INVALID and b"boxes is NULL" in gpu.gfy_last_error()
    assert scores.tolist() == [7.0] * len(pair_list)                 # nothing was launched
    for within in (0, 1):
        code, scores, ends = score_call(pair_list, box_list, within)
        assert code == native.GFY_OK
        wanted = []
        for p, (pair, box) in enumerate(zip(pair_list, box_list)):
            if p in bad:
                assert np.isnan(scores[p]) and tuple(ends[p]) == (-2, -2), (p, scores[p], ends[p])
                wanted.append(None)
                continue
            want = GXO.box_path_of(GB._substitution(*pair), go, ge, box, bool(within))
            assert _bytes(scores[p]) == _bytes(want[0]) and tuple(ends[p]) == want[2], p
            wanted.append(want)
        assert wanted[6][2] == (-1, -1)                              # a box outside the record
        # the trace on the same boxes and the ends of the score call, each slot rows + cols
        sizes = [(box[1] - box[0] + 1) + (box[3] - box[2] + 1) if p not in bad else 16
                 for p, box in enumerate(box_list)]
        lengths, starts, slots = trace_call(pair_list, box_list, within, ends.tolist(), sizes)
        for p, want in enumerate(wanted):
            if want is None:
                assert lengths[p] == -2 and starts[p].tolist() == [-2, -2] and np.all(slots[p] == 9)
                continue
            assert lengths[p] == want[3].size and tuple(starts[p]) == want[1], p
            assert slots[p][:lengths[p]].tobytes() == want[3].tobytes(), p
            assert np.all(slots[p][lengths[p]:] == 9), p
        # ends the score call cannot have named for the box (10, 150, 5, 160), between good ones
        good = ends[0].tolist()
        named = [good, [149, good[1]], [151, good[1]], [150, 4], [150, 161], [140, 155], [-1, 0],
                 good]
        if not within:
            named[5] = [150, 159]                                    # global: only the last cell
        lengths, starts, slots = trace_call([(1, 1)] * len(named), [box_list[0]] * len(named),
                                            within, named, [rows + cols] * len(named))
        for p in (0, len(named) - 1):
            assert lengths[p] == wanted[0][3].size and tuple(starts[p]) == wanted[0][1]
            assert slots[p][:lengths[p]].tobytes() == wanted[0][3].tobytes()
        for p in range(1, len(named) - 1):
            assert lengths[p] == -2 and starts[p].tolist() == [-2, -2], (p, named[p], lengths)
            assert np.all(slots[p] == 9), p
        # the end of the covering call is no end of the box, and a slot one byte short is none
        lengths, starts, slots = trace_call([(1, 1)] * 2, [box_list[0]] * 2, within,
                                            [[199, 169], good], [rows + cols, rows + good[1] - 5])
        assert lengths.tolist() == [-2, -2] and np.all(slots[0] == 9) and np.all(slots[1] == 9)
        # (-1, -1): nothing to align, an empty path
        lengths, starts, slots = trace_call([(1, 1)], [box_list[0]], within, [[-1, -1]], [16])
        assert lengths[0] == 0 and starts[0].tolist() == [-1, -1] and np.all(slots[0] == 9)
    # a workspace for fewer columns than a box has: that pair is refused, the others are served
    code, scores, ends = score_call([(1, 1), (1, 1)], [(10, 150, 5, 160), (0, 50, 0, 20)], 0, columns=21)
    assert code == native.GFY_OK and np.isnan(scores[0]) and ends[0].tolist() == [-2, -2]
    want = GXO.box_score_of(GB._substitution(1, 1), go, ge, (0, 50, 0, 20), False)
    assert _bytes(scores[1]) == _bytes(want[0]) and tuple(ends[1]) == want[1]
