"""The tie zoo of tests/align_cases.py does what it is for: what needs no GPU.

These are conditions on the INPUTS of test_gpu_align_ties.py and test_gpu_align_crowd.py, shown
with the oracles alone, never measurements of a kernel: the substitution scores take three exact
values, equal candidates of a maximum are common (so the order diagonal, E, F and "opening wins"
decide starts and ops), the maximum itself often lies in several cells (so the end rule decides),
and on all of it the oracles agree with each other, which is what lets the device tests hold each
entry point against its own oracle.

Measured on the zoo (seed ``align_cases.SEED``), with the thresholds asserted below in brackets:
positive cells whose H equals two or more of (diagonal, E, F), per pair of 33 rows or more on
both sides: 13.0 % the lowest, 14 to 22 % typical, 29 to 47 % with gap_open = gap_extend = 0
[10 %]; cases whose maximum H lies in two or more cells: 54 of 100, 18 of the 48 with 33 rows or
more on both sides [a quarter of each]; with gap_open = gap_extend = 0 the cells where opening
equals extending, in E or in F: 91.7 % the lowest [half].  What that buys: walking the oracle's
matrices with ``>`` for ``>=`` in the opening test changes the ops of 32 of the 97 cases with an
alignment (the start of 9), F before E changes 24 (6), and naming the last best cell for the
first changes the end of 54."""
from __future__ import annotations

import numpy as np
import pytest

import align_cases as Z
import align_path_oracle as PO

PARAMETER_SETS = range(len(Z.TIE_PARAMETERS))
LARGE = [(q, r) for q, r in Z.with_rows() if Z.ROWS_A[q] >= 33 and Z.ROWS_B[r] >= 33]


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


def _candidates(q, r, k):
    """H of the pair and, per cell, how many of (diagonal, E, F) equal it; then the cells where
    E's, and where F's, two candidates (opening, extending) are equal."""
    go, ge = (np.float32(x) for x in Z.TIE_PARAMETERS[k][2:])
    S = np.ascontiguousarray(Z.substitution(q, r, k))
    H, E, F = PO.gotoh_matrices(S, go, ge, np.float32)
    inner = H[1:, 1:]
    equal = (inner == H[:-1, :-1] + S).astype(int) + (inner == E[1:, 1:]) + (inner == F[1:, 1:])
    return inner, equal, H[1:, :-1] - go == E[1:, :-1] - ge, H[:-1, 1:] - go == F[:-1, 1:] - ge


def test_the_zoo_has_the_lengths_and_the_letters_it_promises():
    case = Z.zoo()
    assert tuple(len(x) for x in case["rec_a"]) == Z.ROWS_A == (0, 1, 63, 64, 65, 130)
    assert tuple(len(x) for x in case["rec_b"]) == Z.ROWS_B == (0, 1, 31, 33, 97, 129)
    assert case["a"].shape == (sum(Z.ROWS_A), 128) and case["a"].dtype == np.float16
    assert case["b"].shape == (sum(Z.ROWS_B), 128) and case["pairs"].shape == (36, 2)
    for rows in (case["a"], case["b"]):
        assert np.all(np.count_nonzero(rows, axis=1) == 1) and set(np.unique(rows)) == {-1, 0, 1}
        assert {int(np.flatnonzero(row)[0]) for row in rows} == {d for d, _ in Z.ALPHABET}
    again = Z.letters(np.random.default_rng(1), 50)
    assert again.tobytes() == Z.letters(np.random.default_rng(1), 50).tobytes()
    # a relative is neither a copy nor unrelated
    rng = np.random.default_rng(2)
    edited = Z.related(rng, case["rec_a"][5])
    assert abs(len(edited) - 130) <= 6 and edited.tobytes() != case["rec_a"][5].tobytes()
    assert Z.related(rng, case["rec_a"][0]).shape == (0, 128)


@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_substitution_scores_take_three_exact_values(k):
    scale, shift, go, ge = Z.TIE_PARAMETERS[k]
    for value in (scale, shift, go, ge):            # dyadic: a multiple of 1/4 of small size
        assert float(value) * 4 == int(value * 4) and abs(value) <= 2
    assert 0 <= ge <= go
    for q, r in Z.with_rows():
        for transposed in (False, True):
            S = Z.substitution(q, r, k, transposed)
            assert S.dtype == np.float32 and set(np.unique(S)) <= Z.values_of(k)
            assert S.shape == ((Z.ROWS_B[r], Z.ROWS_A[q]) if transposed else (Z.ROWS_A[q], Z.ROWS_B[r]))
        if (q, r) in LARGE:
            assert set(np.unique(Z.substitution(q, r, k))) == Z.values_of(k)


@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_equal_candidates_are_common(k):
    lowest = 1.0
    for q, r in LARGE:
        H, equal, _, _ = _candidates(q, r, k)
        positive = H > 0
        assert positive.sum() > 100
        share = float((equal[positive] >= 2).mean())
        assert np.all(equal[positive] >= 1)
        lowest = min(lowest, share)
        assert share >= 0.10, (Z.ROWS_A[q], Z.ROWS_B[r], k, share)
    print(f"parameters {k}: lowest share of tied positive cells {lowest:.3f}")


def test_the_maximum_often_lies_in_several_cells():
    cases = [(q, r, k) for q, r in Z.with_rows() for k in PARAMETER_SETS]
    several = [(q, r, k) for q, r, k in cases
               if (lambda H: H.max() > 0 and (H == H.max()).sum() >= 2)(_candidates(q, r, k)[0])]
    large = [case for case in several if case[:2] in LARGE]
    print(f"maximum in two or more cells: {len(several)} of {len(cases)} cases, "
          f"{len(large)} of {len(LARGE) * len(PARAMETER_SETS)} large ones")
    assert 4 * len(several) >= len(cases)
    assert 4 * len(large) >= len(LARGE) * len(PARAMETER_SETS)


def test_without_gap_costs_opening_equals_extending_in_half_of_the_cells():
    k = 2
    assert Z.TIE_PARAMETERS[k][2:] == (0.0, 0.0)
    lowest = 1.0
    for q, r in LARGE:
        _, _, in_e, in_f = _candidates(q, r, k)
        share = float((in_e | in_f).mean())
        lowest = min(lowest, share)
        assert share >= 0.5, (Z.ROWS_A[q], Z.ROWS_B[r], share, in_e.mean(), in_f.mean())
    print(f"opening equals extending, lowest share of cells: {lowest:.3f}")


@pytest.mark.parametrize("k", PARAMETER_SETS)
def test_the_oracles_agree_with_each_other(k):
    go, ge = Z.TIE_PARAMETERS[k][2:]
    for q, r in Z.with_rows():
        where = (Z.ROWS_A[q], Z.ROWS_B[r], k)
        for transposed in (False, True):
            S = Z.substitution(q, r, k, transposed)
            score, start, end, ops = Z.path(q, r, k, transposed)
            assert (_bits(score), end) == (lambda x: (_bits(x[0]), x[1]))(Z.local(q, r, k, transposed))
            assert (_bits(score), start, end) == \
                (lambda x: (_bits(x[0]), x[1], x[2]))(Z.span(q, r, k, transposed)), where
            if end != (-1, -1):
                assert _bits(PO.rescore(S, ops, start, go, ge)) == _bits(score), where
            else:
                assert ops.size == 0 and start == (-1, -1) and _bits(score) == _bits(0)
        S = Z.substitution(q, r, k)
        score, start, end, ops = Z.path(q, r, k)
        whole, inside = Z.within(q, r, k, False), Z.within(q, r, k, True)
        assert whole[0] <= inside[0] <= score, where
        for mode in (whole, inside):
            assert _bits(PO.rescore(S, mode[3], mode[1], go, ge)) == _bits(mode[0]), where
        bands = Z.bands_of(q, r, k)
        covered, one, some = (Z.banded(q, r, k, band) for band in bands[:3])
        assert (_bits(covered[0]), covered[1], covered[2]) == (_bits(score), start, end), where
        assert covered[3].tobytes() == ops.tobytes()
        assert bands[2][0] <= bands[1][0] == bands[1][1] <= bands[2][1]
        assert one[0] <= some[0] <= covered[0], where      # widening never lowers the score
        assert not one[3].any()                            # one diagonal: no gap
        for band in bands[3:]:
            cut = Z.banded(q, r, k, band)
            assert cut[0] <= covered[0], where
            if cut[2] != (-1, -1):
                assert _bits(PO.rescore(S, cut[3], cut[1], go, ge)) == _bits(cut[0]), where


def test_the_bands_cut_where_they_are_meant_to():
    for k in PARAMETER_SETS:
        for q, r in Z.with_rows():
            lq, lr = Z.ROWS_A[q], Z.ROWS_B[r]
            bands = Z.bands_of(q, r, k)
            assert bands[0] == (-(lq - 1), lr - 1)
            lo, hi = bands[3]
            assert lo % 32 != 0 and hi - lo == 8 and (lo < lr or lr < 6)
            lo, hi = bands[4]
            if lq > 128:      # rows 0 .. 127 hold no band cell: two strips skipped, the third works
                assert hi + 127 < 0 <= hi + lq - 1
                assert Z.banded(q, r, k, bands[4])[2][0] in (-1, 128, 129)
    # on the long related pair the homologous band finds most of the alignment
    assert Z.banded(5, 5, 0, Z.bands_of(5, 5, 0)[2])[0] > 40
