"""Local alignment inside a box of rows per pair on the device (the ``box`` of align.local_align,
local_spans and local_paths; gfy_align_local_box, gfy_align_local_span_box).

Everything is bit for bit, three ways: against tests/align_box_oracle.py (the band oracle on the
sliced substitution matrix), against the calls without a box on the gathered slices (rows
``i_lo..i_hi`` and ``j_lo..j_hi`` copied out as records of their own, the band shifted, the
cells shifted back), and among ``local_align``, ``local_spans`` and ``local_paths`` themselves.
The records are letters (tests/align_cases.py): every cosine is exactly 0, +1 or -1, so the
substitution matrix is known exactly on the host and the tie rules decide most cells.  130 to
200 rows against 131 to 170: two to four strips of the a-record, five or six b-tiles, and the
boxes put every edge of the loop (strip 64, b-tile 32, the direction word 8) at the start, the
end and the inside of a box."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_box_oracle as XO
import align_cases as Z
import align_oracle as O
import align_path_oracle as PO
import test_gpu_align as G
import test_gpu_align_path as GP
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

ROWS_A = (130, 200, 0, 150)
ROWS_B = (140, 170, 131, 0)
PARAMETERS = Z.TIE_PARAMETERS[0]
WAVES_OF_THE_GRID = 256 * G.WAVES        # kAlignGroupsMax workgroups (align_local.inc)
WIDE = (-4096, 4096)                     # the covering band


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _fitted(rng, rows, n):
    return np.concatenate([rows, Z.letters(rng, max(n - rows.shape[0], 0))])[:n]


@functools.lru_cache(maxsize=None)
def _case():
    """Four a-records and four b-records of letters, b-records 0 and 1 related to a-records 0
    and 1; a record of zero rows on either side."""
    rng = np.random.default_rng(20261021)
    rec_a = [Z.letters(rng, n) for n in ROWS_A]
    rec_b = [_fitted(rng, Z.related(rng, rec_a[r], 12, 5, 5), n) if r < 2 else Z.letters(rng, n)
             for r, n in enumerate(ROWS_B)]
    for record in rec_a + rec_b:
        record.setflags(write=False)
    return dict(rec_a=rec_a, rec_b=rec_b, a=torch.from_numpy(np.concatenate(rec_a)).cuda(),
                b=torch.from_numpy(np.concatenate(rec_b)).cuda())


@functools.lru_cache(maxsize=None)
def _substitution(q, r, parameters=PARAMETERS):
    case = _case()
    A, B = case["rec_a"][q].astype(np.float32), case["rec_b"][r].astype(np.float32)
    S = O.substitution_f32(A @ B.T, *parameters[:2])
    S.setflags(write=False)
    return S


def _call(function, pairs, boxes, bands, parameters=PARAMETERS, **more):
    case = _case()
    scale, shift, go, ge = parameters
    return function(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs,
                    gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift, band=bands,
                    box=boxes, **more)


def _device(pairs, boxes, bands, parameters=PARAMETERS):
    """``local_paths`` on the host, after ``local_align`` and ``local_spans`` gave the same bits."""
    paths = GP._host(_call(align.local_paths, pairs, boxes, bands, parameters))
    scores, ends = (x.cpu().numpy() for x in _call(align.local_align, pairs, boxes, bands, parameters))
    span = tuple(x.cpu().numpy() for x in _call(align.local_spans, pairs, boxes, bands, parameters))
    assert G._same_bits(scores, paths[0]) and G._same_bits(ends, paths[2])
    assert all(G._same_bits(x, y) for x, y in zip(span, paths[:3]))
    return paths


def _gathered(pairs, boxes, bands, parameters=PARAMETERS):
    """The calls WITHOUT a box on the rows of every box copied out as two records of their own,
    the band shifted into them and the cells shifted back: (scores, starts, ends, paths)."""
    case = _case()
    scale, shift, go, ge = parameters
    rows_a, rows_b, shifted, corners = [], [], [], []
    for p, ((q, r), box) in enumerate(zip(pairs, boxes)):
        inside = XO.clipped(box, ROWS_A[q], ROWS_B[r])
        i_lo, i_hi, j_lo, j_hi = inside if inside else (0, -1, 0, -1)
        rows_a.append(case["rec_a"][q][i_lo:i_hi + 1])
        rows_b.append(case["rec_b"][r][j_lo:j_hi + 1])
        corners.append((i_lo, j_lo))
        if bands is not None:
            shifted.append((int(bands[p][0]) - (j_lo - i_lo), int(bands[p][1]) - (j_lo - i_lo)))
    count = len(rows_a)
    result = GP._host(align.local_paths(
        torch.from_numpy(np.concatenate(rows_a)).cuda(), torch.from_numpy(np.concatenate(rows_b)).cuda(),
        counts_a=[x.shape[0] for x in rows_a], counts_b=[x.shape[0] for x in rows_b],
        pairs=np.stack([np.arange(count), np.arange(count)], axis=1), gap_open=go, gap_extend=ge,
        match_scale=scale, match_shift=shift, band=shifted if bands is not None else None))
    scores, starts, ends, paths, _ = result
    back = np.array(corners, dtype=np.int32)
    found = starts[:, 0] >= 0
    starts, ends = starts.copy(), ends.copy()
    starts[found] += back[found]
    ends[found] += back[found]
    return scores, starts, ends, paths


def _check(pairs, boxes, bands, parameters=PARAMETERS):
    """The device under ``boxes`` (and ``bands``, or None) against the oracle and against the
    gathered slices; returns the oracle's answers."""
    go, ge = parameters[2:]
    got = _device(pairs, boxes, bands, parameters)
    assert GP._same_paths(got[:4], _gathered(pairs, boxes, bands, parameters))
    wanted = []
    for p, ((q, r), box) in enumerate(zip(pairs, boxes)):
        S = _substitution(q, r, parameters)
        want = XO.box_path_of(S, go, ge, box, None if bands is None else bands[p])
        where = ((q, r), tuple(box), None if bands is None else tuple(bands[p]))
        GP._same_path((got[0][p], got[1][p], got[2][p], got[3][p]), want, where)
        if want[2] != (-1, -1):
            assert PO.rescore(S, got[3][p], want[1], go, ge).tobytes() == got[0][p].tobytes(), where
            cells = align.path_cells(got[3][p], got[1][p])
            both = cells[(cells >= 0).all(axis=1)]
            assert both[:, 0].min() >= box[0] and both[:, 0].max() <= box[1], where
            assert both[:, 1].min() >= box[2] and both[:, 1].max() <= box[3], where
        wanted.append(want)
    return wanted


PAIRS = [(q, r) for q in (0, 1, 3) for r in (0, 1, 2)]


# 1
@pytest.mark.parametrize("parameters", Z.TIE_PARAMETERS[:2])
def test_a_covering_box_equals_the_calls_without_a_box(parameters):
    exact = [XO.covering(ROWS_A[q], ROWS_B[r]) for q, r in PAIRS]
    diagonals = [r * 7 - q * 5 for q, r in PAIRS]
    for bands in (None, [(d - 9, d + 9) for d in diagonals]):
        plain = GP._host(_call(align.local_paths, PAIRS, None, bands, parameters))
        assert plain[0].max() > 10
        for boxes in (exact, np.array(exact) + np.array([-3, 5, -1, 2]), (0, 4095, 0, 4095),
                      (-10 ** 6, 10 ** 6, -10 ** 6, 10 ** 6)):
            got = _device(PAIRS, boxes, bands, parameters)
            assert GP._same_paths(got, plain) and G._same_bits(got[4], plain[4])


# 2
def test_boxes_at_the_places_where_the_loop_changes():
    lq, lr = ROWS_A[1], ROWS_B[1]            # 200 x 170: four strips, six b-tiles
    cases = [(90, 90, 77, 77),               # a single cell
             (0, 0, 0, lr - 1), (0, lq - 1, 5, 5)]        # a single row, a single column
    cases += [(i_lo, 150, 10, 120) for i_lo in (1, 63, 64, 65)]
    cases += [(3, i_hi, 10, 120) for i_hi in (63, 64, lq - 1)]
    cases += [(40, 160, j_lo, 140) for j_lo in (31, 32, 33)]
    cases += [(40, 160, 20, lr - 1), (100, lq - 1, 90, lr - 1),
              (70, 70 + 64, 50, 50 + 32),    # 65 x 33: a second strip and a second b-tile of one
              (63, 63 + 64, 31, 31 + 32),    # the same across the record's own edges
              (-5, lq + 7, -2, lr + 9),      # larger than the record: clipped
              (150, 5000, -4096, 60),
              (lq, lq + 10, 0, lr - 1),      # wholly outside: empty
              (0, lq - 1, lr, 4096), (-9, -1, 0, 10), (0, 10, -4096, -1)]
    pairs = [(1, 1)] * len(cases)
    wanted = _check(pairs, cases, None)
    assert _bytes(wanted[0][0]) in (_bytes(0), _bytes(0.75)) and len(wanted[0][3]) <= 1
    assert all(want[2] == (-1, -1) and want[3].size == 0 for want in wanted[-4:])
    assert max(want[0] for want in wanted) > 20
    # the same boxes of the other related pair, whose a-record ends inside its third strip
    lq, lr = ROWS_A[0], ROWS_B[0]
    other = [(i_lo, min(i_hi, lq + 3), j_lo, min(j_hi, lr + 3)) for i_lo, i_hi, j_lo, j_hi in cases
             if i_lo <= lq + 3 and j_lo <= lr + 3]
    _check([(0, 0)] * len(other), other, None)


def _bytes(value) -> bytes:
    return np.float32(value).tobytes()


@functools.lru_cache(maxsize=None)
def _seed():
    """Start and end of the alignment of the related pair (1, 1) in the whole matrix."""
    _, start, end, _ = PO.path_of(_substitution(1, 1), *PARAMETERS[2:])
    assert end[0] - start[0] > 100
    return start, end


# 3
def test_a_box_with_a_band():
    start, end = _seed()
    d = start[1] - start[0]
    box = (70, 140, 70 + d - 10, 140 + d + 10)       # around the middle of the alignment
    far = d + 120
    cases = [(box, (d - 6, d + 6)),                  # a band through the box
             (box, (d - 1, d + 1)), (box, (d, d)),   # lo == hi: gapless
             (box, (d + 3, d + 3)),
             (box, (far, far + 10)),                 # a band that misses the box: score 0
             (box, (-4096, box[2] - box[1] - 1)),
             (box, WIDE),
             ((65, 190, 33, 160), (d - 6, d + 6)),
             ((-4096, 4096, -4096, 4096), (d - 6, d + 6)),   # the banded call
             ((90, 90, 90 + d, 90 + d), (d, d)),             # one cell on the band
             ((90, 90, 90 + d, 90 + d), (d + 1, d + 2))]     # one cell off it
    pairs = [(1, 1)] * len(cases)
    wanted = _check(pairs, [c[0] for c in cases], [c[1] for c in cases])
    assert wanted[0][0] > 10 and wanted[2][0] > 0 and not wanted[2][3].any()
    for index in (4, 5, 10):
        assert _bytes(wanted[index][0]) == _bytes(0) and wanted[index][2] == (-1, -1)
    banded = GP._host(_call(align.local_paths, [(1, 1)], None, [(d - 6, d + 6)]))
    GP._same_path((banded[0][0], banded[1][0], banded[2][0], banded[3][0]), wanted[8])
    # the other pairs and parameter sets, a band around each box's own diagonal
    rng = np.random.default_rng(3)
    for parameters in Z.TIE_PARAMETERS[1:]:
        boxes, bands = [], []
        for q, r in PAIRS:
            boxes.append(_random_box(rng, ROWS_A[q], ROWS_B[r]))
            centre = boxes[-1][2] - boxes[-1][0] + int(rng.integers(-20, 21))
            bands.append((centre - int(rng.integers(0, 12)), centre + int(rng.integers(0, 12))))
        _check(PAIRS, boxes, bands, parameters)
        _check(PAIRS, boxes, None, parameters)


def _random_box(rng, lq, lr):
    """A box that meets an lq x lr matrix and may reach over its ends."""
    i_lo, j_lo = int(rng.integers(-10, lq)), int(rng.integers(-10, lr))
    return (i_lo, max(i_lo, 0) + int(rng.integers(0, lq)), j_lo, max(j_lo, 0) + int(rng.integers(0, lr)))


# 4
def test_scores_in_nested_boxes_never_decrease():
    start, end = _seed()
    mid = ((start[0] + end[0]) // 2, (start[1] + end[1]) // 2)
    pairs = [(1, 1), (0, 0), (3, 2)]
    for bands in (None, [WIDE, (0, 20), (-30, 30)]):
        before = None
        for grow in (0, 1, 7, 31, 32, 33, 64, 100, 4096):
            boxes = [(mid[0] - grow, mid[0] + grow, mid[1] - grow, mid[1] + grow)] * len(pairs)
            scores = _call(align.local_align, pairs, boxes, bands)[0].cpu().numpy()
            assert not np.isnan(scores).any()
            if before is not None:
                assert np.all(scores >= before), (grow, scores, before)
            before = scores
        whole = _call(align.local_align, pairs, None, bands)[0].cpu().numpy()
        assert G._same_bits(before, whole)                       # the last one covers
    assert before[0] > 20


# 5
def test_a_pair_with_a_record_of_zero_rows():
    pairs = [(1, 1), (2, 1), (1, 3), (2, 3), (0, 0)]
    boxes = [(10, 100, 10, 100), (0, 10, 0, 10), (0, 10, 0, 10), (-5, 5, -5, 5), (20, 90, 20, 90)]
    for bands in (None, [(-10, 10)] * len(pairs)):
        wanted = _check(pairs, boxes, bands)
        for index in (1, 2, 3):
            assert _bytes(wanted[index][0]) == _bytes(0) and wanted[index][2] == (-1, -1)
        assert wanted[0][0] > 5 and wanted[4][0] > 5
    # no pair at all
    empty = _call(align.local_paths, [], [], None)
    assert empty.scores.shape == (0,) and empty.ops.shape == (0,) and empty.offsets.tolist() == [0]
    scores, starts, ends = _call(align.local_spans, np.zeros((0, 2), dtype=np.int32),
                                 np.zeros((0, 4), dtype=np.int32), (0, 1))
    assert scores.shape == (0,) and starts.shape == ends.shape == (0, 2)


# 6
def test_a_crowd_of_boxes_equals_the_same_pairs_one_at_a_time():
    """300 different (pair, box, band) and a call of more pairs than the grid has waves: every
    wave's second pair finds the carry, the ring and the band its first pair left, and a box
    of other sizes.  Each seat equals the same pair in a call of its own."""
    rng = np.random.default_rng(20261021)
    kinds = []
    for number in range(300):
        q, r = PAIRS[number % len(PAIRS)]
        box = _random_box(rng, ROWS_A[q], ROWS_B[r])
        centre = box[2] - box[0] + int(rng.integers(-30, 31))
        band = WIDE if number % 3 == 0 else \
            (centre - int(rng.integers(0, 15)), centre + int(rng.integers(0, 15)))
        kinds.append(((q, r), box, band))
    kinds[7] = ((2, 1), (0, 10, 0, 10), WIDE)                # a record of zero rows
    kinds[8] = ((1, 1), (300, 400, 0, 10), (-5, 5))          # a box outside the record
    seats = np.concatenate([rng.integers(0, len(kinds), WAVES_OF_THE_GRID), rng.permutation(len(kinds))])
    crowd = _device([kinds[k][0] for k in seats], [kinds[k][1] for k in seats],
                    [kinds[k][2] for k in seats])
    assert crowd[0].max() > 20 and np.count_nonzero(crowd[0] > 0) > len(seats) // 2
    alone = [GP._host(_call(align.local_paths, [pair], [box], [band])) for pair, box, band in kinds]
    for seat, k in enumerate(seats):
        assert GP._same_paths(GP._pick(crowd, [seat]), GP._pick(alone[k], [0])), (seat, kinds[k])
    # a sample of the kinds against the oracle
    sample = list(range(0, len(kinds), 10))
    _check([kinds[k][0] for k in sample], [kinds[k][1] for k in sample], [kinds[k][2] for k in sample])


# 7
def test_two_regions_on_one_diagonal_get_two_answers():
    """within -> hit_runs -> chain_runs -> local_paths on a pair of records that share two
    regions at one offset: the band of the two chains is the same, and only their boxes tell
    them apart (the premise is proved on the host in tests/test_align_box_host.py)."""
    region = XO.two_regions()
    rng = np.random.default_rng(11)
    counts_a, counts_b = [70, XO.REGION_ROWS[0]], [XO.REGION_ROWS[1], 40]
    a = torch.from_numpy(np.concatenate([Z.letters(rng, 70), region["a"]])).cuda()
    b = torch.from_numpy(np.concatenate([region["b"], Z.letters(rng, 40)])).cuda()
    scale, shift, go, ge = XO.REGION_PARAMETERS
    hits = distance.within(a, b, threshold=0.9, metric="cosine")
    runs = align.hit_runs(hits, counts_a=counts_a, counts_b=counts_b, min_length=12)
    chains = align.chain_runs(runs, max_gap=8)               # the linker has 45 rows
    first, second = region["plants"]
    assert chains.pairs.tolist() == [[1, 0], [1, 0]]
    assert chains.diagonals.tolist() == [[XO.REGION_SHIFT] * 2] * 2
    starts, ends = chains.starts.cpu().numpy(), chains.ends.cpu().numpy()
    for c, plant in enumerate((first, second)):
        assert np.all(starts[c] <= plant[0]) and np.all(ends[c] >= plant[-1])
    bands, boxes = chains.bands(4), chains.boxes(8)
    assert bands.tolist() == [[XO.REGION_SHIFT - 4, XO.REGION_SHIFT + 4]] * 2
    assert boxes.shape == (2, 4) and boxes[0, 1] < boxes[1, 0] and boxes[0, 3] < boxes[1, 2]

    def paths(**more):
        return GP._host(align.local_paths(a, b, counts_a=counts_a, counts_b=counts_b,
                                          pairs=chains.pairs, gap_open=go, gap_extend=ge,
                                          match_scale=scale, match_shift=shift, **more))

    def cells(result, p):
        return align.path_cells(result[3][p], result[1][p])

    # the premise: the band alone returns the same path twice, the stronger region's
    banded = paths(band=bands)
    assert GP._same_paths(GP._pick(banded, [0]), GP._pick(banded, [1]))
    assert XO.holds(cells(banded, 0), first) and not XO.holds(cells(banded, 1), second)
    # with the boxes: two paths, and each covers its plant
    boxed = paths(band=bands, box=boxes)
    assert not G._same_bits(boxed[1][0], boxed[1][1]) and not G._same_bits(boxed[2][0], boxed[2][1])
    for p, plant in enumerate((first, second)):
        assert XO.holds(cells(boxed, p), plant), p
        want = XO.box_path_of(region["S"], go, ge, boxes[p], bands[p])
        GP._same_path((boxed[0][p], boxed[1][p], boxed[2][p], boxed[3][p]), want, p)
    # the stronger region is the band's own answer, the weaker one is new
    assert GP._same_paths(GP._pick(boxed, [0]), GP._pick(banded, [0]))
    assert boxed[0][1] > 0 and boxed[0][1] < boxed[0][0]


# 8
def test_raw_call_refuses_null_boxes_and_a_box_the_wrong_way_round(gpu):
    case = _case()
    ptr_a = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_A))), dtype=torch.int32).cuda()
    ptr_b = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_B))), dtype=torch.int32).cuda()
    pair_list = [(1, 1), (0, 0), (1, 1), (3, 2), (1, 1), (0, 1)]
    box_list = [(10, 150, 5, 160), (0, 129, 0, 139), (5, 4, 0, 10), (0, 10, 2 ** 31 - 1, -2 ** 31),
                (10, 150, 5, 160), (64, 129, 32, 100)]
    band_list = [(-30, 60), (0, 40), (-30, 60), (0, 40), (-30, 60), (-4096, 4096)]
    bad = (2, 3)
    columns = 160 - 5 + 1                                    # the widest box of the call
    stream = torch.cuda.current_stream().cuda_stream

    def call(pairs, boxes, bands, span, null=False):
        pairs = torch.tensor(pairs, dtype=torch.int32).cuda()
        boxes = torch.tensor(boxes, dtype=torch.int32).cuda()
        bands = None if bands is None else torch.tensor(bands, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        sizer = gpu.gfy_align_span_workspace_bytes if span else gpu.gfy_align_workspace_bytes
        need = sizer(count, columns)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        outputs = (scores, starts, ends) if span else (scores, ends)
        function = gpu.gfy_align_local_span_box if span else gpu.gfy_align_local_box
        code = function(case["a"].data_ptr(), case["a"].shape[0], ptr_a.data_ptr(), len(ROWS_A),
                        case["b"].data_ptr(), case["b"].shape[0], ptr_b.data_ptr(), len(ROWS_B),
                        pairs.data_ptr(), count, *PARAMETERS,
                        None if bands is None else bands.data_ptr(),
                        None if null else boxes.data_ptr(), *(x.data_ptr() for x in outputs),
                        scratch.data_ptr(), need, stream)
        torch.cuda.synchronize()
        return code, tuple(x.cpu().numpy() for x in outputs)

    for span in (False, True):
        code, untouched = call(pair_list, box_list, band_list, span, null=True)
        assert code == native.GFY_ERR_INVALID and b"boxes is NULL" in gpu.gfy_last_error()
        assert untouched[0].tolist() == [7.0] * len(pair_list)       # nothing was launched
        for bands in (band_list, None):
            code, got = call(pair_list, box_list, bands, span)
            assert code == native.GFY_OK
            for p in range(len(pair_list)):
                if p in bad:
                    assert np.isnan(got[0][p]), (p, got[0][p])
                    assert all(tuple(x[p]) == (-2, -2) for x in got[1:]), (p, got[1:])
                    continue
                code, clean = call([pair_list[p]], [box_list[p]],
                                   None if bands is None else [bands[p]], span)
                assert code == native.GFY_OK and not np.isnan(clean[0][0])
                assert all(G._same_bits(x[p:p + 1], y) for x, y in zip(got, clean)), p
                want = XO.box_path_of(_substitution(*pair_list[p]), *PARAMETERS[2:], box_list[p],
                                      None if bands is None else bands[p])
                assert _bytes(got[0][p]) == _bytes(want[0]) and tuple(got[-1][p]) == want[2], p
                if span:
                    assert tuple(got[1][p]) == want[1], p
    # a workspace for fewer columns than a box has: that pair is refused, the others are served
    narrow = [(10, 150, 5, 160), (0, 50, 0, 20)]
    pairs = torch.tensor([(1, 1), (1, 1)], dtype=torch.int32).cuda()
    boxes = torch.tensor(narrow, dtype=torch.int32).cuda()
    scores = torch.full((2,), 7.0, dtype=torch.float32).cuda()
    ends = torch.full((2, 2), 7, dtype=torch.int32).cuda()
    need = gpu.gfy_align_workspace_bytes(2, 21)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    code = gpu.gfy_align_local_box(
        case["a"].data_ptr(), case["a"].shape[0], ptr_a.data_ptr(), len(ROWS_A),
        case["b"].data_ptr(), case["b"].shape[0], ptr_b.data_ptr(), len(ROWS_B), pairs.data_ptr(), 2,
        *PARAMETERS, None, boxes.data_ptr(), scores.data_ptr(), ends.data_ptr(), scratch.data_ptr(),
        need, stream)
    torch.cuda.synchronize()
    assert code == native.GFY_OK
    assert np.isnan(scores[0].item()) and ends[0].tolist() == [-2, -2]
    want = XO.box_path_of(_substitution(1, 1), *PARAMETERS[2:], narrow[1])
    assert _bytes(scores[1].item()) == _bytes(want[0]) and tuple(ends[1].tolist()) == want[2]
