"""Every variant of the alignment call reaches its own kernel: one call of five records on each
side, aligned by every public function with and without a band, a box and ``within``, and every
result equal to the numpy oracles under tests/ bit for bit.

The records have 1, 64, 65, 130 and 200 rows (one to four strips of the a-record, with and
without a partial last strip) and are letters (tests/align_cases.py): every cosine is exactly 0,
+1 or -1, so the substitution matrix is known exactly on the host.  The band and the box are the
same for every pair and do not cover the records.  The b-record of 200 rows holds four stretches
of its a-record, placed so that the answer without a band and a box, with the band, with the box
and with both is a different stretch each time: a call that reached a neighbouring kernel (the
banded one for a boxed call, the plain one for a banded call, global for ``within``) cannot
give the right score.  The first test asserts that premise on the oracles alone."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_box_oracle as XO
import align_cases as Z
import align_global_box_oracle as GXO
import align_null_oracle as NO
import align_oracle as O
from ginfinity_amd import _native as native
from ginfinity_amd import align

ROWS = (1, 64, 65, 130, 200)
PAIRS = [(k, k) for k in range(5)] + [(k, 4 - k) for k in range(5)]
BAND, BOX = (-3, 40), (2, 100, 1, 70)
WAYS = ((None, None), (BAND, None), (None, BOX), (BAND, BOX))
COVERING = (-4096, 4096, -4096, 4096)
SCALE, SHIFT, GAP_OPEN, GAP_EXTEND = PARAMETERS = Z.TIE_PARAMETERS[0]
SHUFFLES, SEED = 3, 5
PLANTED = PAIRS.index((4, 4))


@functools.lru_cache(maxsize=None)
def _records():
    """b-record k is a-record k with a few substitutions, insertions and deletions; b-record 4
    holds four stretches of a-record 4 instead (rows of A at rows of B):
        50 .. 99 at 5 .. 54      diagonal -45: inside the box, outside the band
        40 .. 59 at 56 .. 75     diagonal 16: inside the band, 15 of its rows inside the box
        101 .. 127 at 100 .. 126 diagonal -1: inside the band, outside the box
        80 .. 149 at 130 .. 199  diagonal 50: outside both, the longest"""
    rng = np.random.default_rng(20261021)
    rec_a = [Z.letters(rng, n) for n in ROWS]
    rec_b = [Z._fitted(rng, Z.related(rng, rec_a[k]), n) for k, n in enumerate(ROWS)]
    a = rec_a[4]
    rec_b[4] = np.concatenate([Z.letters(rng, 5), a[50:100], Z.letters(rng, 1), a[40:60],
                               Z.letters(rng, 24), a[101:128], Z.letters(rng, 3), a[80:150]])
    assert [x.shape[0] for x in rec_b] == list(ROWS)
    for record in rec_a + rec_b:
        record.setflags(write=False)
    return rec_a, rec_b


@functools.lru_cache(maxsize=None)
def _substitution(q, r):
    rec_a, rec_b = _records()
    S = O.substitution_f32(rec_a[q].astype(np.float32) @ rec_b[r].astype(np.float32).T, SCALE, SHIFT)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def _local(p, band, box):
    """The oracle's (score, start, end, ops) of pair p."""
    return XO.box_path_of(_substitution(*PAIRS[p]), GAP_OPEN, GAP_EXTEND, box or COVERING, band)


@functools.lru_cache(maxsize=None)
def _global(p, within, box):
    return GXO.box_path_of(_substitution(*PAIRS[p]), GAP_OPEN, GAP_EXTEND, box or COVERING, within)


def _null(p, k, band, box, orders, columns):
    """The oracle's score of run k of pair p: the b-side's columns in the run's order, the band in
    the b-side's coordinates and the box's a-rows."""
    S = _substitution(*PAIRS[p])
    j_lo = 0 if box is None else max(box[2], 0)
    side = S[:, j_lo:j_lo + int(columns[p])]
    shuffled = side[:, NO.segment(*orders, columns, SHUFFLES, p, k).astype(np.int64)]
    rows = COVERING if box is None else (box[0], box[1], -4096, 4096)
    return XO.box_path_of(shuffled, GAP_OPEN, GAP_EXTEND, rows,
                          None if band is None else (band[0] - j_lo, band[1] - j_lo))[0]


def test_the_oracles_answers_differ_between_every_two_variants():
    """On the oracles alone: the planted pair has four different local scores and four different
    global ones, so no variant can stand in for another."""
    local = [_local(PLANTED, band, box) for band, box in WAYS]
    assert len({x[0].tobytes() for x in local}) == 4, [x[0] for x in local]
    assert len({(x[1], x[2]) for x in local}) == 4
    assert local[0][0] == max(x[0] for x in local) and local[3][0] > 0     # the whole matrix wins
    whole = [_global(PLANTED, within, box) for within in (False, True) for box in (None, BOX)]
    assert len({x[0].tobytes() for x in whole}) == 4, [x[0] for x in whole]
    # neither the band nor the box covers a record of more than one row; every strip count occurs
    assert BOX[0] > 0 and BOX[2] > 0 and BAND[0] > -(ROWS[1] - 1) and BAND[1] < ROWS[1] - 1
    assert sorted({(ROWS[q] + 63) // 64 for q, _ in PAIRS}) == [1, 2, 3, 4]


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    native.library()
    rec_a, rec_b = _records()
    return dict(a=torch.from_numpy(np.concatenate(rec_a)).cuda(),
                b=torch.from_numpy(np.concatenate(rec_b)).cuda())


def _call(function, device, **more):
    return function(device["a"], device["b"], counts_a=ROWS, counts_b=ROWS, pairs=PAIRS,
                    gap_open=GAP_OPEN, gap_extend=GAP_EXTEND, match_scale=SCALE, match_shift=SHIFT,
                    **more)


def _same(got, want, where):
    """Device tensors (scores, then cells) or AlignedPaths against the oracle's tuples."""
    scores = got[0].cpu().numpy()
    cells = [x.cpu().numpy() for x in got[1:3]]
    for p, answer in enumerate(want):
        assert scores[p].tobytes() == np.float32(answer[0]).tobytes(), (where, p, scores[p], answer[0])
        for mine, theirs in zip(cells, answer[1:]):
            assert tuple(mine[p]) == theirs, (where, p, tuple(mine[p]), theirs)
    if isinstance(got, align.AlignedPaths):
        ops, offsets = got.ops.cpu().numpy(), got.offsets.cpu().numpy()
        for p, answer in enumerate(want):
            assert ops[offsets[p]:offsets[p + 1]].tobytes() == answer[3].tobytes(), (where, p)


@pytest.mark.gpu
@pytest.mark.parametrize("band, box", WAYS)
def test_the_local_calls_give_the_oracles_answer_of_their_band_and_box(device, band, box):
    want = [_local(p, band, box) for p in range(len(PAIRS))]
    where = (band, box)
    _same(_call(align.local_align, device, band=band, box=box), [(s, e) for s, _, e, _ in want], where)
    _same(_call(align.local_spans, device, band=band, box=box), [x[:3] for x in want], where)
    _same(_call(align.local_paths, device, band=band, box=box), want, where)


@pytest.mark.gpu
@pytest.mark.parametrize("band, box", WAYS)
def test_the_null_scores_give_the_oracles_answer_of_their_band_and_box(device, band, box):
    rows_b = np.array([ROWS[r] for _, r in PAIRS])
    columns = rows_b if box is None else np.maximum(np.minimum(box[3], rows_b - 1) - max(box[2], 0) + 1, 0)
    orders = NO.shuffle_orders(columns, SHUFFLES, SEED)
    got = _call(align.null_scores, device, band=band, box=box, shuffles=SHUFFLES, seed=SEED)
    got = got.cpu().numpy()
    assert got.shape == (len(PAIRS), SHUFFLES) and got.dtype == np.float32
    for p in range(len(PAIRS)):
        for k in range(SHUFFLES):
            want = _null(p, k, band, box, orders, columns)
            assert got[p, k].tobytes() == np.float32(want).tobytes(), (band, box, p, k, got[p, k], want)


@pytest.mark.gpu
@pytest.mark.parametrize("within", (False, True))
@pytest.mark.parametrize("box", (None, BOX))
def test_the_global_calls_give_the_oracles_answer_of_their_mode_and_box(device, within, box):
    want = [_global(p, within, box) for p in range(len(PAIRS))]
    where = (within, box)
    _same(_call(align.global_align, device, within=within, box=box), [(s, e) for s, _, e, _ in want],
          where)
    _same(_call(align.global_paths, device, within=within, box=box), want, where)
