"""The eight alignment kernels where ties decide the answer, and on rows and parameters at the
corners of what align.py allows.

The tie zoo of tests/align_cases.py (letters: every cosine exactly 0 or +-1; dyadic parameters:
no sum is ever rounded) goes through every entry point, each held bit for bit against its own
oracle: ``local_align`` (align_oracle), ``local_spans`` (align_span_oracle), ``local_paths``
(align_path_oracle), ``global_align`` / ``global_paths`` in both modes (align_global_oracle), the
three calls under five bands per pair (align_band_oracle), and the local calls on the transposed
zoo, where E and F change roles.  tests/test_align_ties_host.py shows what these inputs are worth:
13 to 47 % of the positive cells have two or more equal candidates, more than half of the cases
have their maximum in several cells, and without gap costs opening equals extending in nine cells
of ten — a ``>`` for a ``>=``, E before the diagonal or F before E, a wrong origin on a tie moves
a start, an end or an op here.

As everywhere in the alignment tests the substitution matrix is formed from the device's own
``distance.pairwise(..., metric="cosine")``; on letters it must have three exact values, which
makes it the matrix align_cases forms from the letters, so the oracles' answers are computed
once per (pair, parameters) and shared with the host test.

The corner records (``_corners``) hold rows of all zeros (the 1e-12 clamp of the norm), rows of
fp16 subnormal entries and rows with entries near the fp16 maximum: scores bit for bit against
the float32 oracles on the device's dense cosine, and against the float64 definition within the
bound of tests/test_gpu_align.py, unchanged.  On an MI355X the dense cosine of every kind of row
is within 2.4e-7 of float64 (subnormal rows 1.4e-7, large rows 1.8e-7, zero rows exactly 0), and
the largest error / bound of a score is 0.0637 (scale 1.0) and 0.0034 (scale -1.0)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_cases as Z
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import align_span_oracle as SO
import test_gpu_align as G
import test_gpu_align_path as GP
import test_gpu_align_span as GS
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

PARAMETER_SETS = range(len(Z.TIE_PARAMETERS))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


@functools.lru_cache(maxsize=None)
def _device():
    """The zoo's rows on the device and, per pair with rows, the device's own cosine matrix of
    the pair and of the transposed pair (float32, read-only)."""
    case = Z.zoo()
    records_a = [torch.from_numpy(x.copy()).cuda() for x in case["rec_a"]]
    records_b = [torch.from_numpy(x.copy()).cuda() for x in case["rec_b"]]
    cosines = {}
    for q, r in Z.with_rows():
        for transposed in (False, True):
            A, B = (records_b[r], records_a[q]) if transposed else (records_a[q], records_b[r])
            C = distance.pairwise(A, B, metric="cosine").cpu().numpy()
            C.setflags(write=False)
            cosines[q, r, transposed] = C
    return dict(a=torch.from_numpy(case["a"]).cuda(), b=torch.from_numpy(case["b"]).cuda(),
                cosines=cosines)


@functools.lru_cache(maxsize=None)
def _substitution(q, r, k, transposed=False):
    """The pair's substitution matrix from the device's cosines: three exact values, hence the
    matrix of align_cases bit for bit — asserted before anything uses it."""
    C = _device()["cosines"][q, r, transposed]
    assert C.dtype == np.float32 and set(np.unique(C)) <= {-1.0, 0.0, 1.0}, np.unique(C)
    S = O.substitution_f32(C, *Z.TIE_PARAMETERS[k][:2])
    assert set(np.unique(S)) <= Z.values_of(k), (q, r, k, np.unique(S))
    assert S.tobytes() == Z.substitution(q, r, k, transposed).tobytes()
    return S


def _keywords(k, transposed=False):
    scale, shift, go, ge = Z.TIE_PARAMETERS[k]
    device = _device()
    a, b, counts_a, counts_b = device["a"], device["b"], Z.ROWS_A, Z.ROWS_B
    if transposed:
        a, b, counts_a, counts_b = b, a, counts_b, counts_a
    return (a, b), dict(counts_a=counts_a, counts_b=counts_b, gap_open=go, gap_extend=ge,
                        match_scale=scale, match_shift=shift)


def _numpy(result):
    return tuple(x.cpu().numpy() for x in result)


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


def _empty_path(want_of_three):
    return (*want_of_three, np.zeros(0, dtype=np.uint8))


def _three_local_calls(k, pairs, transposed=False, band=None):
    """``local_align``, ``local_spans`` and ``local_paths`` of ``pairs``; the cross-checks on the
    device's results alone; returns the paths on the host."""
    rows, keywords = _keywords(k, transposed)
    more = {} if band is None else dict(band=band)
    scores, ends = _numpy(align.local_align(*rows, pairs=pairs, **keywords, **more))
    span = _numpy(align.local_spans(*rows, pairs=pairs, **keywords, **more))
    paths = GP._host(align.local_paths(*rows, pairs=pairs, **keywords, **more))
    # the three calls agree: one score, one end, the span's start is the path's
    assert G._same_bits(scores, span[0]) and G._same_bits(ends, span[2])
    assert all(G._same_bits(x, y) for x, y in zip(span, paths[:3]))
    return (scores, ends), span, paths


def _rescored(S, path, p, k):
    """The device's ops of pair p add up to the device's score, bit for bit."""
    scores, starts, ends, ops, _ = path
    go, ge = Z.TIE_PARAMETERS[k][2:]
    if tuple(ends[p]) == (-1, -1):
        assert ops[p].size == 0 and scores[p] == 0 and tuple(starts[p]) == (-1, -1)
        return
    assert ops[p][0] == 0 and ops[p][-1] == 0
    assert PO.rescore(S, ops[p], tuple(starts[p]), go, ge).tobytes() == scores[p].tobytes(), p


NOTHING = (np.float32(0), (-1, -1), (-1, -1))


# 1
@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_local_scores_spans_and_paths_equal_their_oracles(k, transposed):
    """All 36 pairs of the zoo, the pairs with an empty record among them; transposed, the
    b-records are aligned against the a-records, so what was a tie in E is one in F."""
    pairs = Z.zoo()["pairs"][:, ::-1] if transposed else Z.zoo()["pairs"]
    (scores, ends), span, paths = _three_local_calls(k, np.ascontiguousarray(pairs), transposed)
    several = 0
    for p, (q, r) in enumerate(Z.zoo()["pairs"]):
        q, r = int(q), int(r)
        where = (Z.ROWS_A[q], Z.ROWS_B[r], k, transposed)
        if Z.ROWS_A[q] == 0 or Z.ROWS_B[r] == 0:
            GP._same_path((paths[0][p], paths[1][p], paths[2][p], paths[3][p]),
                          _empty_path(NOTHING), where)
            continue
        S = _substitution(q, r, k, transposed)
        score, end = Z.local(q, r, k, transposed)
        assert scores[p].tobytes() == _bits(score) or (score == 0 and scores[p] == 0), where
        assert tuple(ends[p]) == end, (where, ends[p], end)
        GS._same_span((span[0][p], span[1][p], span[2][p]), Z.span(q, r, k, transposed), where)
        want = Z.path(q, r, k, transposed)
        GP._same_path((paths[0][p], paths[1][p], paths[2][p], paths[3][p]), want, where)
        _rescored(S, paths, p, k)
        several += int(np.count_nonzero(want[3]) > 0)
    assert several >= 8       # paths with gaps, not diagonals alone


# 2
@pytest.mark.parametrize("mode", (False, True))
@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_global_and_within_scores_and_paths_equal_the_oracle(k, mode):
    rows, keywords = _keywords(k)
    pairs = Z.zoo()["pairs"]
    scores, ends = _numpy(align.global_align(*rows, pairs=pairs, within=mode, **keywords))
    paths = GP._host(align.global_paths(*rows, pairs=pairs, within=mode, **keywords))
    assert G._same_bits(scores, paths[0]) and G._same_bits(ends, paths[2])
    local = align.local_align(*rows, pairs=pairs, **keywords)[0].cpu().numpy()
    other = align.global_align(*rows, pairs=pairs, within=not mode, **keywords)[0].cpu().numpy()
    whole, inside = (other, scores) if mode else (scores, other)
    assert np.all(whole <= inside) and np.all(inside <= local)
    bordered = 0
    go, ge = Z.TIE_PARAMETERS[k][2:]
    for p, (q, r) in enumerate(pairs):
        q, r = int(q), int(r)
        where = (Z.ROWS_A[q], Z.ROWS_B[r], k, mode)
        got = (paths[0][p], paths[1][p], paths[2][p], paths[3][p])
        if Z.ROWS_A[q] == 0 or Z.ROWS_B[r] == 0:
            GP._same_path(got, _empty_path(NOTHING), where)
            continue
        S = _substitution(q, r, k)
        want = Z.within(q, r, k, mode)
        assert got[0].tobytes() == _bits(want[0]) or (want[0] == 0 and got[0] == 0), \
            (where, got[0], want[0])
        assert tuple(got[1]) == want[1] and tuple(got[2]) == want[2], (where, got[1:3], want[1:3])
        assert got[3].tobytes() == want[3].tobytes(), (where, got[3].tolist(), want[3].tolist())
        rescored = GO.rescore(S, got[3], tuple(got[1]), go, ge)
        assert rescored.tobytes() == got[0].tobytes() or (rescored == 0 and got[0] == 0), where
        bordered += int(want[3][0] != 0)
    assert bordered >= 4      # walks that leave over a charged border


# 3
@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_the_three_calls_under_a_band_equal_the_banded_oracle(k, kind):
    """Band ``kind`` of ``align_cases.bands_of`` for every pair with rows: covering, one diagonal,
    17 diagonals, a band that cuts the first block of a strip, a band that skips strips."""
    pairs = np.array(Z.with_rows(), dtype=np.int32)
    bands = np.array([Z.bands_of(int(q), int(r), k)[kind] for q, r in pairs], dtype=np.int64)
    (scores, ends), span, paths = _three_local_calls(k, pairs, band=bands)
    positive = 0
    for p, (q, r) in enumerate(pairs):
        q, r = int(q), int(r)
        band = tuple(int(x) for x in bands[p])
        where = (Z.ROWS_A[q], Z.ROWS_B[r], k, band)
        want = Z.banded(q, r, k, band)
        GP._same_path((paths[0][p], paths[1][p], paths[2][p], paths[3][p]), want, where)
        _rescored(_substitution(q, r, k), paths, p, k)
        positive += int(want[2] != (-1, -1))
        if kind == 0:         # a covering band: the call without a band
            plain = Z.path(q, r, k)
            assert (_bits(want[0]), want[1], want[2]) == (_bits(plain[0]), plain[1], plain[2])
        if kind == 1:
            assert not paths[3][p].any()
    assert positive >= (4 if kind == 4 else 12), positive


# 4
def _corners():
    """An a-record of 70 and a b-record of 72 rows, a noisy copy of a-rows 10 .. 49 at b-rows 20
    .. 59; every 7th (5th) row is all zeros, another is scaled to fp16 subnormal entries (the
    largest 2^-15), another to a largest entry of 60000.  Returns the two records and the kind of
    every row (0 plain, 1 zero, 2 subnormal, 3 large)."""
    rng = np.random.default_rng(355)
    base_a, base_b = G._unitish(rng, 70), G._unitish(rng, 72)
    base_b[20:60] = base_a[10:50] + 0.02 * rng.standard_normal((40, 128))
    kind_a = np.select([np.arange(70) % 7 == 3, np.arange(70) % 7 == 5, np.arange(70) % 7 == 1],
                       [1, 2, 3], 0)
    kind_b = np.select([np.arange(72) % 5 == 2, np.arange(72) % 5 == 4, np.arange(72) % 5 == 0],
                       [1, 2, 3], 0)
    records = []
    for base, kinds in ((base_a, kind_a), (base_b, kind_b)):
        largest = np.abs(base).max(axis=1, keepdims=True)
        factor = np.select([kinds == 1, kinds == 2, kinds == 3],
                           [0.0, 2.0 ** -15 / largest[:, 0], 60000.0 / largest[:, 0]], 1.0)
        rows = (base * factor[:, None]).astype(np.float16)
        tiny = np.float64(np.finfo(np.float16).tiny)
        assert np.isfinite(rows).all() and not rows[kinds == 1].any()
        assert np.abs(rows[kinds == 2].astype(np.float64)).max() < tiny       # subnormal, not zero
        assert np.count_nonzero(rows[kinds == 2], axis=1).min() >= 100
        assert np.abs(rows[kinds == 3].astype(np.float64)).max(axis=1).min() > 50000
        records.append(rows)
    return records[0], records[1], kind_a, kind_b


CORNER_PARAMETERS = (G.PARAMETERS[0], Z.TIE_PARAMETERS[3])     # the second: a negative scale


@functools.lru_cache(maxsize=None)
def _corner_case():
    rec_a, rec_b, kind_a, kind_b = _corners()
    records, kinds = (rec_a, rec_b), (kind_a, kind_b)
    rows = torch.from_numpy(np.concatenate(records)).cuda()
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]          # b omitted: the two records among themselves
    cosines = []
    for q, r in pairs:
        C = distance.pairwise(torch.from_numpy(records[q]).cuda(),
                              torch.from_numpy(records[r]).cuda(), metric="cosine").cpu().numpy()
        C.setflags(write=False)
        cosines.append(C)
    return dict(rows=rows, counts=[70, 72], pairs=pairs, cosines=cosines, records=records,
                kinds=kinds)


def test_a_zero_row_has_cosine_zero_against_everything():
    case = _corner_case()
    for (q, r), C in zip(case["pairs"], case["cosines"]):
        assert not np.isnan(C).any() and np.isfinite(C).all()
        assert np.all(C[case["kinds"][q] == 1, :] == 0) and np.all(C[:, case["kinds"][r] == 1] == 0)
        # what the dense kernel makes of each kind of row, against float64 (-s)
        exact = O.cosine_f64(case["records"][q], case["records"][r])
        for name, kind in (("plain", 0), ("zero", 1), ("subnormal", 2), ("large", 3)):
            rows, cols = case["kinds"][q] == kind, case["kinds"][r] == kind
            worst = max(np.abs(C[rows, :] - exact[rows, :]).max(),
                        np.abs(C[:, cols] - exact[:, cols]).max())
            print(f"pair {(q, r)} {name:9s} rows: largest |cosine - float64| {worst:.3e}")


@pytest.mark.parametrize("parameters", CORNER_PARAMETERS)
def test_corner_rows_scores_equal_the_float32_oracles_bit_for_bit(parameters):
    case = _corner_case()
    scale, shift, go, ge = parameters
    common = dict(counts_a=case["counts"], pairs=case["pairs"], gap_open=go, gap_extend=ge,
                  match_scale=scale, match_shift=shift)
    scores, ends = _numpy(align.local_align(case["rows"], **common))
    span = _numpy(align.local_spans(case["rows"], **common))
    whole = _numpy(align.global_align(case["rows"], within=False, **common))
    inside = _numpy(align.global_align(case["rows"], within=True, **common))
    for result in (scores, span[0], whole[0], inside[0]):
        assert not np.isnan(result).any() and np.isfinite(result).all()
    for p, C in enumerate(case["cosines"]):
        S = O.substitution_f32(C, scale, shift)
        score, end = O.gotoh_f32(S, go, ge)
        assert scores[p].tobytes() == _bits(score) and tuple(ends[p]) == end, (p, scores[p], score)
        GS._same_span((span[0][p], span[1][p], span[2][p]), SO.span_of(S, go, ge), p)
        for got, mode in ((whole, False), (inside, True)):
            want = GO.score_of(S, go, ge, mode)
            assert got[0][p].tobytes() == _bits(want[0]) and tuple(got[1][p]) == want[1], \
                (p, mode, got[0][p], want)
    if scale > 0:
        assert scores[1] > 10 and scores[2] > 10      # the planted copy, through rows of every kind


@pytest.mark.parametrize("parameters", CORNER_PARAMETERS)
def test_corner_rows_scores_against_the_float64_definition(parameters):
    """The bound of test_gpu_align.test_scores_and_ends_against_the_float64_definition, as it
    stands there."""
    case = _corner_case()
    scale, shift, go, ge = parameters
    scores = align.local_align(case["rows"], counts_a=case["counts"], pairs=case["pairs"],
                               gap_open=go, gap_extend=ge, match_scale=scale,
                               match_shift=shift)[0].cpu().numpy()
    worst = 0.0
    for p, (q, r) in enumerate(case["pairs"]):
        score64, _, H = O.gotoh_f64(case["records"][q], case["records"][r], go, ge, scale, shift)
        lq, lr = H.shape
        bound = min(lq, lr) * abs(scale) * G.COSINE_TOL + (lq + lr) * 2.0 ** -24 * max(score64, 1.0)
        error = abs(float(scores[p]) - score64)
        worst = max(worst, error / bound)
        print(f"pair {(q, r)} Lq {lq:3d} Lr {lr:3d} score64 {score64:10.6f} error {error:.3e} "
              f"bound {bound:.3e}")
        assert error <= bound, ((q, r), float(scores[p]), score64, bound)
    print(f"scale {scale}: largest error / bound {worst:.4f}")
