"""Local alignment inside a band of diagonals on the device (the ``band`` of align.local_align,
local_spans and local_paths; gfy_align_local_band, gfy_align_local_span_band,
gfy_align_trace_band).

Everything is bit for bit, against the unbanded calls (a covering band) and against
tests/align_band_oracle.py, which runs the recurrences of include/gfy.h in float32 on the
device's own cosines with the cells outside the band held at the outside values.  The records,
the planted copies and the parameter sets are those of tests/test_gpu_align.py, whose cached
case is shared: 1 to 200 rows against 1 to 330, three full strips and a ragged fourth, b-tile
edges at 32 and 128.  The cases of ``test_places_where_the_loop_changes`` are the ones the
header of csrc/align_local.inc names: a first and a last strip without a band cell, a step loop
that starts at a multiple of 32 other than 0, a band that meets nothing, a single diagonal, and
direction words begun and ended mid-way."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_oracle as O
import align_path_oracle as PO
import test_gpu_align as G
import test_gpu_align_path as GP
import test_gpu_align_span as GS
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B, PARAMETERS, WAVES = G.ROWS_A, G.ROWS_B, G.PARAMETERS, G.WAVES
LONG = (5, 5)          # 200 x 330: four strips, eleven b-tiles


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _call(function, case, pairs, parameters, band, b=None, counts_b=ROWS_B):
    scale, shift, go, ge = parameters
    return function(case["a"], case["b"] if b is None else b, counts_a=ROWS_A, counts_b=counts_b,
                    pairs=pairs, gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift,
                    band=band)


def _scores(case, pairs, parameters, band, **more):
    scores, ends = _call(align.local_align, case, pairs, parameters, band, **more)
    return scores.cpu().numpy(), ends.cpu().numpy()


def _spans(case, pairs, parameters, band, **more):
    return tuple(x.cpu().numpy()
                 for x in _call(align.local_spans, case, pairs, parameters, band, **more))


def _paths(case, pairs, parameters, band, **more):
    return GP._host(_call(align.local_paths, case, pairs, parameters, band, **more))


def _substitution(case, p, parameters):
    return O.substitution_f32(case["cosines"][p], parameters[0], parameters[1])


def _index(pair):
    return pair[0] * len(ROWS_B) + pair[1]


@functools.lru_cache(maxsize=None)
def _seeds():
    """The diagonal start_j - start_i of every pair's unbanded alignment under PARAMETERS[0]
    (0 where nothing aligns), and the planted pairs."""
    case = G._case()
    _, starts, _ = GS._grid(PARAMETERS[0])
    diagonals = np.where(starts[:, 0] >= 0, starts[:, 1] - starts[:, 0], 0).astype(np.int64)
    return diagonals, np.flatnonzero(case["planted"])


def _against_the_oracle(case, pairs, bands, parameters, **more):
    """Scores, starts, ends and ops of ``pairs`` under ``bands`` from all three functions against
    the banded oracle; ``more`` may name another b side, then ``cosines`` come with it."""
    cosines = more.pop("cosines", None)
    go, ge = parameters[2:]
    scores, starts, ends, ops, _ = _paths(case, pairs, parameters, bands, **more)
    plain = _scores(case, pairs, parameters, bands, **more)
    span = _spans(case, pairs, parameters, bands, **more)
    assert G._same_bits(plain[0], scores) and G._same_bits(plain[1], ends)
    assert all(G._same_bits(x, y) for x, y in zip(span, (scores, starts, ends)))
    wanted = []
    for p, (pair, (lo, hi)) in enumerate(zip(pairs, bands)):
        S = O.substitution_f32(cosines[p], parameters[0], parameters[1]) if cosines else \
            _substitution(case, _index(pair), parameters)
        want = BO.band_path_of(S, go, ge, int(lo), int(hi))
        GP._same_path((scores[p], starts[p], ends[p], ops[p]), want, (tuple(pair), int(lo), int(hi)))
        if want[2] != (-1, -1):
            assert PO.rescore(S, ops[p], want[1], go, ge).tobytes() == scores[p].tobytes()
        wanted.append(want)
    return wanted


# 1
@pytest.mark.parametrize("parameters", PARAMETERS)
def test_a_covering_band_equals_the_calls_without_a_band(parameters):
    case = G._case()
    pairs = case["pairs"]
    exact = np.array([BO.covering(ROWS_A[q], ROWS_B[r]) for q, r in pairs], dtype=np.int64)
    span, paths = GS._grid(parameters), GP._grid(parameters)
    for bands in (exact, exact + np.array([-3, 5]), (-4096, 4096), (-10 ** 6, 10 ** 6)):
        got = _scores(case, pairs, parameters, bands)
        assert G._same_bits(got[0], span[0]) and G._same_bits(got[1], span[2])
        got = _spans(case, pairs, parameters, bands)
        assert all(G._same_bits(x, y) for x, y in zip(got, span))
    for bands in (exact, (-4096, 4096)):
        got = _paths(case, pairs, parameters, bands)
        assert GP._same_paths(got, paths) and G._same_bits(got[4], paths[4])


# 2
@pytest.mark.parametrize("shift", (0, 25))
@pytest.mark.parametrize("half_width", (0, 3, 17, 40))
def test_band_shapes_against_the_oracle(half_width, shift):
    """Bands around the seed diagonal of every planted pair, and the same bands 25 diagonals
    further so that the planted stretch is cut."""
    case = G._case()
    parameters = PARAMETERS[0]
    diagonals, planted = _seeds()
    pairs = case["pairs"][planted]
    bands = np.stack([diagonals[planted] + shift - half_width,
                      diagonals[planted] + shift + half_width], axis=1)
    if half_width == 40 and shift == 0:      # host only: the band recovers the planted copy
        for p, (lo, hi) in zip(planted, bands):
            S = _substitution(case, p, parameters)
            assert BO.band_span_of(S, *parameters[2:], int(lo), int(hi))[0] > 10, case["pairs"][p]
    wanted = _against_the_oracle(case, pairs, bands, parameters)
    if half_width == 0:
        assert all(not want[3].any() for want in wanted)


# 3
def test_places_where_the_loop_changes():
    case = G._case()
    parameters = PARAMETERS[0]
    diagonals, _ = _seeds()
    seed = int(diagonals[_index(LONG)])
    cases = [(LONG, (-150, -70)),           # strip 0 holds no band cell
             (LONG, (-4096, -70)),
             (LONG, (64, 64 + 30)),         # strip 0 starts at column 64, strip 1 at 128
             (LONG, (400, 500)),            # meets no cell
             (LONG, (-500, -400)),
             (LONG, (seed, seed)),          # one diagonal
             (LONG, (seed - 5, seed + 5)),  # 11 columns a row: first at j & 7 == 3, last at 5
             (LONG, (seed - 1, seed + 1))]  # 3 columns a row: 3 .. 5 of one word
    wanted = _against_the_oracle(case, [pair for pair, _ in cases], [band for _, band in cases],
                                 parameters)
    for index in (3, 4):
        assert wanted[index][1:3] == ((-1, -1), (-1, -1)) and wanted[index][3].size == 0
    assert wanted[0][2] == (-1, -1) or wanted[0][1][0] >= 70       # no cell above row 70
    assert wanted[5][0] > 10 and not wanted[5][3].any()
    for index, half in ((6, 5), (7, 1)):
        score, start, end, ops = wanted[index]
        assert score > 10
        # in the box the trace walks, rows of the path whose band begins at j & 7 == 3 and ends
        # at j & 7 == 5: direction words begun and ended mid-way, and walked
        rows = np.arange(end[0] - start[0] + 1)
        first = rows + (seed - half) - (start[1] - start[0])
        assert np.any((first >= 0) & (first % 8 == 3) & ((first + 2 * half) % 8 == 5) &
                      (first + 2 * half <= end[1] - start[1]))
    # the 200-row record against the 65-row one with lo = -10: rows 75 on hold no band cell, the
    # last strip none at all
    short = 3
    assert ROWS_A[5] == 200 and ROWS_A[short] == 65
    C = distance.pairwise(torch.from_numpy(case["rec_a"][5]).cuda(),
                          torch.from_numpy(case["rec_a"][short]).cuda(), metric="cosine")
    more = dict(b=case["a"], counts_b=ROWS_A, cosines=[C.cpu().numpy()] * 2)
    _against_the_oracle(case, [(5, short)] * 2, [(-10, 4096), (-10, 3)], parameters, **more)


# 4
def test_a_pair_under_a_band_does_not_depend_on_its_company():
    """4 x WAVES + 3 pairs, a few pairs under different bands in shuffled order: a wave must not
    carry a band, a column range or outside values over from its previous pair."""
    case = G._case()
    parameters = PARAMETERS[0]
    diagonals, _ = _seeds()
    kinds = []
    for pair in (LONG, (5, 2), (3, 5), (1, 1)):
        seed = int(diagonals[_index(pair)])
        kinds += [(pair, (seed - 8, seed + 8)), (pair, (seed, seed)), (pair, (seed + 20, seed + 90)),
                  (pair, (-4096, -70)), (pair, BO.covering(ROWS_A[pair[0]], ROWS_B[pair[1]]))]
    rng = np.random.default_rng(19)
    count = 4 * WAVES + 3
    order = np.concatenate([rng.permutation(len(kinds)), rng.integers(0, len(kinds), count)])[:count]
    pairs = [kinds[k][0] for k in order]
    bands = [kinds[k][1] for k in order]
    crowd = _paths(case, pairs, parameters, bands)
    crowd_scores = _scores(case, pairs, parameters, bands)
    alone = {}
    for seat, k in enumerate(order):
        if k not in alone:
            alone[k] = (_paths(case, [kinds[k][0]], parameters, [kinds[k][1]]),
                        _scores(case, [kinds[k][0]], parameters, [kinds[k][1]]))
        single, single_scores = alone[k]
        assert GP._same_paths(GP._pick(crowd, [seat]), GP._pick(single, [0])), (seat, kinds[k])
        assert G._same_bits(crowd_scores[0][seat:seat + 1], single_scores[0])
        assert G._same_bits(crowd_scores[1][seat:seat + 1], single_scores[1])


# 5
def test_scores_under_nested_bands_never_decrease():
    case = G._case()
    parameters = PARAMETERS[0]
    diagonals, planted = _seeds()
    pairs = case["pairs"]
    before = None
    for width in (0, 8, 64, 4096 + 330):
        bands = np.stack([diagonals - width, diagonals + width], axis=1)
        scores = _scores(case, pairs, parameters, bands)[0]
        assert not np.isnan(scores).any()
        if before is not None:
            assert np.all(scores >= before), (width, np.flatnonzero(scores < before))
        before = scores
    assert G._same_bits(before, GS._grid(parameters)[0])     # the last one covers
    assert before[planted].min() > 10


# 6
def test_tensor_and_tuple_forms_of_the_band():
    case = G._case()
    parameters = PARAMETERS[1]
    pairs = case["pairs"]
    one = (-20, 35)
    as_numpy = np.tile(np.array(one, dtype=np.int64), (len(pairs), 1))
    want = _paths(case, pairs, parameters, as_numpy)
    want_scores = _scores(case, pairs, parameters, as_numpy)
    forms = (torch.from_numpy(as_numpy).cuda(), torch.from_numpy(as_numpy.astype(np.int32)),
             as_numpy.astype(np.int16), one, list(one), as_numpy.tolist())
    for band in forms:
        got = _paths(case, pairs, parameters, band)
        assert GP._same_paths(got, want) and G._same_bits(got[4], want[4])
        got = _scores(case, pairs, parameters, band)
        assert G._same_bits(got[0], want_scores[0]) and G._same_bits(got[1], want_scores[1])
    assert want[0][case["planted"]].max() > 0


# 7
def test_raw_call_refuses_a_null_band_and_a_band_the_wrong_way_round(gpu):
    case = G._case()
    ptr_a = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_A))), dtype=torch.int32).cuda()
    ptr_b = torch.tensor(np.concatenate(([0], np.cumsum(ROWS_B))), dtype=torch.int32).cuda()
    pair_list = [LONG, (3, 4), LONG, (4, 3), LONG]
    band_list = [(-30, 60), (0, 40), (5, 4), (2 ** 31 - 1, -2 ** 31), (-30, 60)]
    bad = (2, 3)
    stream = torch.cuda.current_stream().cuda_stream

    def call(pairs, bands, span, null=False):
        pairs = torch.tensor(pairs, dtype=torch.int32).cuda()
        bands = torch.tensor(bands, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        sizer = gpu.gfy_align_span_workspace_bytes if span else gpu.gfy_align_workspace_bytes
        need = sizer(count, max(ROWS_B))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        outputs = (scores, starts, ends) if span else (scores, ends)
        function = gpu.gfy_align_local_span_band if span else gpu.gfy_align_local_band
        code = function(case["a"].data_ptr(), case["a"].shape[0], ptr_a.data_ptr(), len(ROWS_A),
                        case["b"].data_ptr(), case["b"].shape[0], ptr_b.data_ptr(), len(ROWS_B),
                        pairs.data_ptr(), count, 1.0, -0.3, 1.0, 0.25,
                        None if null else bands.data_ptr(), *(x.data_ptr() for x in outputs),
                        scratch.data_ptr(), need, stream)
        torch.cuda.synchronize()
        return code, tuple(x.cpu().numpy() for x in outputs)

    for span in (False, True):
        code, untouched = call(pair_list, band_list, span, null=True)
        assert code == native.GFY_ERR_INVALID and b"bands is NULL" in gpu.gfy_last_error()
        assert untouched[0].tolist() == [7.0] * 5                    # nothing was launched
        code, got = call(pair_list, band_list, span)
        assert code == native.GFY_OK
        for p in range(len(pair_list)):
            if p in bad:
                assert np.isnan(got[0][p]), (p, got[0][p])
                assert all(tuple(x[p]) == (-2, -2) for x in got[1:]), (p, got[1:])
            else:
                code, clean = call([pair_list[p]], [band_list[p]], span)
                assert code == native.GFY_OK and not np.isnan(clean[0][0])
                assert all(G._same_bits(x[p:p + 1], y) for x, y in zip(got, clean)), p
