"""Null scores of local alignment on the device (align.null_scores, align.shuffle_orders,
align.significance; gfy_align_local_null).

Everything is bit for bit against the EXISTING calls on MATERIALISED rows: the b-side of every
pair copied out in the order of every run as a record of its own (tests/align_null_oracle.py),
and ``local_align`` on those records.  Two kinds of records: letters (tests/align_cases.py),
where every cosine is exactly 0 or +-1 and ties decide cells, and random fp16 rows of unequal
norms, which notice a ``1/|b|`` taken from the wrong row where letters cannot.  The sizes sit on
the edges of the loop: a-records of 1, 63, 65 and 130 rows (strips of 64), b-records of 1, 31, 33
and 70 rows (tiles of 32), and a record of zero rows on either side."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_cases as Z
import align_null_oracle as NO
import align_oracle as O
import test_gpu_align as G
from ginfinity_amd import _native as native
from ginfinity_amd import align

pytestmark = pytest.mark.gpu

ROWS_A = (1, 63, 65, 130, 0)
ROWS_B = (1, 31, 33, 70, 0)
PAIRS = [(q, r) for q in range(len(ROWS_A)) for r in range(len(ROWS_B))]
KINDS = ("letters", "random")
#: (match_scale, match_shift, gap_open, gap_extend) per kind
PARAMETERS = {"letters": Z.TIE_PARAMETERS[0], "random": (1.0, -0.3, 1.0, 0.25)}
WAVES_OF_THE_GRID = 256 * G.WAVES        # kAlignGroupsMax workgroups (align_local.inc)
BANDS = [(3 * r - 2 * q - 12, 3 * r - 2 * q + 12) for q, r in PAIRS]
#: a box that starts and ends inside a strip and a tile where the records are long enough, one
#: that covers the small records, and one whose a-rows miss the record while its b-rows do not
BOXES = [(5, 100, 7, 60) if ROWS_A[q] >= 63 and ROWS_B[r] >= 31 else (-3, 4096, 0, 4096)
         for q, r in PAIRS]
BOXES[PAIRS.index((1, 2))] = (200, 300, 0, 10)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


def _uneven(rng, rows):
    """fp16 rows whose norms run from a quarter to four."""
    rows = rows / np.maximum(np.linalg.norm(rows, axis=1, keepdims=True), 1e-6)
    return (rows * rng.uniform(0.25, 4.0, size=(rows.shape[0], 1))).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """Five a-records and five b-records; b-records 2 and 3 are related to a-records 2 and 3."""
    rng = np.random.default_rng(20261021 + KINDS.index(kind))
    if kind == "letters":
        rec_a = [Z.letters(rng, n) for n in ROWS_A]
        rec_b = [Z._fitted(rng, Z.related(rng, rec_a[r][:n + 2]), n) if r in (2, 3)
                 else Z.letters(rng, n) for r, n in enumerate(ROWS_B)]
    else:
        rec_a = [_uneven(rng, rng.standard_normal((n, 128))) for n in ROWS_A]
        rec_b = []
        for r, n in enumerate(ROWS_B):
            rows = rng.standard_normal((n, 128))
            if r in (2, 3):          # a noisy copy of the a-record's first rows, from row 3 on
                rows[3:] = rec_a[r][:n - 3].astype(np.float64) * 4 + 0.4 * rows[3:]
            rec_b.append(_uneven(rng, rows))
    for record in rec_a + rec_b:
        record.setflags(write=False)
    return dict(kind=kind, rec_a=rec_a, rec_b=rec_b,
                a=torch.from_numpy(np.concatenate(rec_a)).cuda(),
                b=torch.from_numpy(np.concatenate(rec_b)).cuda())


def _keywords(kind):
    scale, shift, go, ge = PARAMETERS[kind]
    return dict(gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift)


def _null(case, pairs, shuffles, band=None, box=None, **more):
    scores = align.null_scores(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs,
                               band=band, box=box, shuffles=shuffles, **_keywords(case["kind"]),
                               **more)
    assert scores.is_cuda and scores.dtype == torch.float32
    assert scores.shape == (len(pairs), shuffles)
    return scores.cpu().numpy()


def _local(case, pairs, band=None, box=None):
    return align.local_align(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=pairs,
                             band=band, box=box, **_keywords(case["kind"]))[0].cpu().numpy()


def _columns(pairs, box=None):
    sides = [NO.side_of(np.zeros((ROWS_B[r], 1)), None if box is None else box[p])
             for p, (q, r) in enumerate(pairs)]
    return np.array([side.shape[0] for side in sides], dtype=np.int64)


def _materialised(case, pairs, orders, shuffles, band=None, box=None):
    """``local_align`` on the b-side of every pair copied out in the order of every run, as P *
    shuffles records of their own: float32 [P, shuffles].  The band goes into the b-side's
    coordinates (j_lo is the side's first row) and the box keeps its a-rows."""
    order, order_ptr = (np.asarray(x) for x in orders)
    columns = _columns(pairs, box)
    records, virtual, bands, boxes = [], [], [], []
    for p, (q, r) in enumerate(pairs):
        side = NO.side_of(case["rec_b"][r], None if box is None else box[p])
        j_lo = 0 if box is None else max(int(box[p][2]), 0)
        for k in range(shuffles):
            records.append(NO.gathered(side, NO.segment(order, order_ptr, columns, shuffles, p, k)))
            virtual.append((q, len(virtual)))
            if band is not None:
                bands.append((int(band[p][0]) - j_lo, int(band[p][1]) - j_lo))
            if box is not None:
                boxes.append((int(box[p][0]), int(box[p][1]), -4096, 4096))
    scores = align.local_align(case["a"], torch.from_numpy(np.concatenate(records)).cuda(),
                               counts_a=ROWS_A, counts_b=[x.shape[0] for x in records],
                               pairs=virtual, band=bands or None, box=boxes or None,
                               **_keywords(case["kind"]))[0]
    return scores.cpu().numpy().reshape(len(pairs), shuffles)


def _identity(columns, shuffles=1):
    order = np.concatenate([np.tile(np.arange(n), shuffles) for n in columns] or [np.zeros(0)])
    return order.astype(np.int32), np.concatenate(([0], np.cumsum(columns) * shuffles)).astype(np.int64)


WAYS = [(None, None), (BANDS, None), (None, BOXES), (BANDS, BOXES)]


@pytest.mark.parametrize("kind", KINDS)
def test_the_identity_order_is_local_align(kind):
    case = _case(kind)
    for band, box in WAYS:
        got = _null(case, PAIRS, 1, band, box, orders=_identity(_columns(PAIRS, box)))
        want = _local(case, PAIRS, band, box)
        assert G._same_bits(got[:, 0], want), (band is not None, box is not None)
        assert not np.isnan(got).any()
    assert want.max() > 3 and _local(case, PAIRS).max() > 5


@pytest.mark.parametrize("kind", KINDS)
def test_generated_orders_equal_local_align_on_the_gathered_rows(kind):
    case = _case(kind)
    plain = None
    for band, box in WAYS:
        columns = _columns(PAIRS, box)
        orders = NO.shuffle_orders(columns, 3, 11)
        got = _null(case, PAIRS, 3, band, box, seed=11)
        assert G._same_bits(got, _materialised(case, PAIRS, orders, 3, band, box)), \
            (band is not None, box is not None)
        assert G._same_bits(got, _null(case, PAIRS, 3, band, box, orders=orders))
        plain = got if plain is None else plain
    # the runs differ from each other and from the real score: something was shuffled
    real = _local(case, PAIRS)
    related = PAIRS.index((3, 3))
    assert real[related] > plain[related].max()
    if kind == "random":                     # letters' scores are multiples of 0.25 and may meet
        assert len({x.tobytes() for x in plain[related]}) == 3
    # a pair with a record of zero rows, and the box that holds no cell, score 0 in every run
    for p, (q, r) in enumerate(PAIRS):
        if ROWS_A[q] == 0 or ROWS_B[r] == 0:
            assert plain[p].tobytes() == np.zeros(3, dtype=np.float32).tobytes(), (q, r)
    assert got[PAIRS.index((1, 2))].tobytes() == np.zeros(3, dtype=np.float32).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_reversal_and_a_bootstrap_are_orders_like_any_other(kind):
    case = _case(kind)
    rng = np.random.default_rng(5)
    for band, box in ((None, None), (BANDS, BOXES)):
        columns = _columns(PAIRS, box)
        order = np.concatenate([np.concatenate([np.arange(n)[::-1], rng.integers(0, max(n, 1), n)])
                                for n in columns]).astype(np.int32)
        orders = (order, _identity(columns, 2)[1])
        got = _null(case, PAIRS, 2, band, box, orders=orders)
        assert G._same_bits(got, _materialised(case, PAIRS, orders, 2, band, box))
    # the reversal of a whole record is the flipped record, and a bootstrap repeats rows
    p = PAIRS.index((3, 3))
    reversal = NO.segment(order, orders[1], columns, 2, p, 0)
    side = NO.side_of(case["rec_b"][3], BOXES[p])
    assert np.array_equal(NO.gathered(side, reversal), side[::-1])
    assert len(set(NO.segment(order, orders[1], columns, 2, p, 1).tolist())) < columns[p]
    flipped = torch.from_numpy(np.ascontiguousarray(case["rec_b"][3][::-1])).cuda()
    whole = _null(case, [(3, 3)], 1, orders=(np.arange(ROWS_B[3], dtype=np.int32)[::-1].copy(),
                                             np.array([0, ROWS_B[3]])))
    alone = align.local_align(case["a"], flipped, counts_a=ROWS_A, counts_b=[ROWS_B[3]],
                              pairs=[(3, 0)], **_keywords(kind))[0].cpu().numpy()
    assert G._same_bits(whole[0], alone)


def test_a_crowd_of_virtual_pairs_equals_each_of_them_alone(gpu):
    """Tiny records and more than twice as many virtual pairs as the largest grid has waves: every
    wave takes several virtual pairs and finds the carry, the ring and the order its last one
    left.  Each virtual pair equals the same one in a launch of its own (P = 1, shuffles = 1,
    the same entries)."""
    rng = np.random.default_rng(20261021)
    sizes_a, sizes_b = rng.integers(5, 41, 32), rng.integers(5, 41, 32)
    base = _uneven(rng, rng.standard_normal((40, 128))).astype(np.float64)
    rec_a = [_uneven(rng, base[:n] * 3 + 0.5 * rng.standard_normal((n, 128))) for n in sizes_a]
    rec_b = [_uneven(rng, base[:n] * 3 + 0.5 * rng.standard_normal((n, 128))) for n in sizes_b]
    a, b = (torch.from_numpy(np.concatenate(x)).cuda() for x in (rec_a, rec_b))
    pairs = np.stack([np.arange(32), rng.permutation(32)], axis=1).astype(np.int32)
    shuffles = 80
    assert len(pairs) * shuffles > 2 * WAVES_OF_THE_GRID
    columns = sizes_b[pairs[:, 1]].astype(np.int64)
    order, order_ptr = align.shuffle_orders(columns, shuffles, 3, "cuda")
    parameters = PARAMETERS["random"]
    crowd = align.null_scores(a, b, counts_a=sizes_a, counts_b=sizes_b, pairs=pairs,
                              gap_open=parameters[2], gap_extend=parameters[3],
                              match_scale=parameters[0], match_shift=parameters[1],
                              shuffles=shuffles, orders=(order, order_ptr)).cpu().numpy()
    assert not np.isnan(crowd).any() and np.count_nonzero(crowd > 0) > crowd.size // 2
    # alone: the raw call on one pair and one order at a time, nothing allocated in between
    ptr_a = torch.tensor(np.concatenate(([0], np.cumsum(sizes_a))), dtype=torch.int32).cuda()
    ptr_b = torch.tensor(np.concatenate(([0], np.cumsum(sizes_b))), dtype=torch.int32).cuda()
    pairs_dev = torch.from_numpy(pairs).cuda()
    alone = torch.full((len(pairs), shuffles), 7.0, dtype=torch.float32).cuda()
    steps = {int(n): torch.tensor([0, int(n)], dtype=torch.int64).cuda() for n in set(columns)}
    need = gpu.gfy_align_workspace_bytes(1, 40)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    starts = order_ptr.cpu().numpy()
    for p in range(len(pairs)):
        for k in range(shuffles):
            code = gpu.gfy_align_local_null(
                a.data_ptr(), a.shape[0], ptr_a.data_ptr(), 32, b.data_ptr(), b.shape[0],
                ptr_b.data_ptr(), 32, pairs_dev.data_ptr() + 8 * p, 1, *parameters, None, None, 1,
                order.data_ptr() + 4 * (int(starts[p]) + k * int(columns[p])),
                steps[int(columns[p])].data_ptr(), alone.data_ptr() + 4 * (p * shuffles + k),
                scratch.data_ptr(), need, stream)
            assert code == native.GFY_OK
    torch.cuda.synchronize()
    assert G._same_bits(crowd, alone.cpu().numpy())


def test_refused_orders_give_nan_and_leave_the_others_alone():
    case = _case("random")
    pairs = [(3, 3), (2, 2), (1, 1), (3, 2), (2, 3)]
    columns = _columns(pairs)
    order, order_ptr = NO.shuffle_orders(columns, 3, 4)
    clean = _null(case, pairs, 3, orders=(order, order_ptr))
    assert not np.isnan(clean).any()
    for p, k, at, value in ((0, 1, 0, 70), (1, 2, 32, -1), (3, 0, 5, 2 ** 31 - 1),
                            (4, 1, 69, -2 ** 31), (2, 0, 30, 31)):
        broken = order.copy()
        broken[int(order_ptr[p]) + k * int(columns[p]) + at] = value
        got = _null(case, pairs, 3, orders=(broken, order_ptr))
        assert np.isnan(got[p, k]), (p, k)
        keep = np.ones(got.shape, dtype=bool)
        keep[p, k] = False
        assert got[keep].tobytes() == clean[keep].tobytes(), (p, k)
    # an order_ptr that does not step by shuffles * columns: that pair's runs, all of them
    for p, change in ((4, -1), (4, 1), (0, -1)):
        steps = order_ptr.copy()
        steps[p + 1:] += change
        got = _null(case, pairs, 3, orders=(order, steps))
        assert np.isnan(got[p]).all(), p
        # the pairs behind it read other entries of `order` now, each served or refused by the
        # range test; the pairs in front of it are untouched
        assert got[:p].tobytes() == clean[:p].tobytes(), p
    negative = order_ptr.copy()
    negative[0] = -3
    got = _null(case, pairs, 3, orders=(order, negative))
    assert np.isnan(got[0]).all() and got[1:].tobytes() == clean[1:].tobytes()


def test_two_runs_give_the_same_bytes_and_the_device_makes_the_cpus_orders():
    case = _case("letters")
    columns = _columns(PAIRS, BOXES)
    for shuffles, seed in ((3, 0), (7, 2 ** 64 - 5)):
        on_cpu = align.shuffle_orders(columns, shuffles, seed)
        on_device = align.shuffle_orders(columns, shuffles, seed, "cuda")
        assert all(x.is_cuda for x in on_device) and not any(x.is_cuda for x in on_cpu)
        for one, two, twin in zip(on_cpu, on_device, NO.shuffle_orders(columns, shuffles, seed)):
            assert one.dtype == two.dtype
            assert one.numpy().tobytes() == two.cpu().numpy().tobytes() == twin.tobytes()
    first = _null(case, PAIRS, 7, BANDS, BOXES, seed=2 ** 64 - 5)
    again = _null(case, PAIRS, 7, BANDS, BOXES, seed=2 ** 64 - 5)
    given = _null(case, PAIRS, 7, BANDS, BOXES, orders=on_cpu)
    assert G._same_bits(first, again) and G._same_bits(first, given)
    kept = align.AlignWorkspace()
    assert G._same_bits(first, _null(case, PAIRS, 7, BANDS, BOXES, seed=-5, workspace=kept))
    empty = align.null_scores(case["a"], case["b"], counts_a=ROWS_A, counts_b=ROWS_B, pairs=[],
                              shuffles=4, **_keywords("letters"))
    assert empty.shape == (0, 4) and empty.dtype == torch.float32 and empty.is_cuda


# ---- end to end -----------------------------------------------------------------------------------
PLANT_SHUFFLES, PLANT_SEED = 20, 2026
#: a match scores 1, two other letters -1 and opposite ones -3, a gap 2 and 1 per further row: the
#: drift of unrelated letters is negative, so a null score is the best of many short chance runs
PLANT_PARAMETERS = (2.0, -1.0, 2.0, 1.0)
PLANT_ROWS_A, PLANT_ROWS_B = (90, 90), (150, 150)


@functools.lru_cache(maxsize=None)
def planted():
    """a-record 0 carries, in rows 30 .. 69, a copy of rows 50 .. 89 of b-record 0; a-record 1
    and b-record 1 are unrelated letters.  Returns the records and, from tests/align_oracle.py on
    the exact substitution matrices, the real scores [2] and the null scores [2, K]."""
    rng = np.random.default_rng(20261021)
    rec_b = [Z.letters(rng, n) for n in PLANT_ROWS_B]
    rec_a = [Z.letters(rng, n) for n in PLANT_ROWS_A]
    rec_a[0][30:70] = rec_b[0][50:90]
    scale, shift, go, ge = PLANT_PARAMETERS
    order, order_ptr = NO.shuffle_orders(PLANT_ROWS_B, PLANT_SHUFFLES, PLANT_SEED)

    def score(A, B):
        S = O.substitution_f32(A.astype(np.float32) @ B.astype(np.float32).T, scale, shift)
        return O.gotoh_f32(S, go, ge)[0]

    real = np.array([score(rec_a[p], rec_b[p]) for p in range(2)], dtype=np.float32)
    null = np.array([[score(rec_a[p], NO.gathered(rec_b[p], NO.segment(
        order, order_ptr, PLANT_ROWS_B, PLANT_SHUFFLES, p, k))) for k in range(PLANT_SHUFFLES)]
        for p in range(2)], dtype=np.float32)
    return rec_a, rec_b, real, null


def _judged(real, null):
    found = align.significance(torch.as_tensor(real), torch.as_tensor(null))
    assert all(x.dtype == torch.float64 and x.device == torch.as_tensor(null).device for x in found)
    assert real[0] > null[0].max()                       # above every null score of its own
    assert found.z[0] > found.z[1] and found.z[0] > 10
    assert found.p_value[0] < found.p_value[1] and found.p_value[0] < 1e-6
    assert not real[1] > null[1].max() + 3 * float(found.std[1])   # the unrelated pair is ordinary
    return found


def test_a_planted_copy_stands_out_of_its_null_and_an_unrelated_pair_does_not():
    rec_a, rec_b, real, null = planted()
    assert real[0] >= 40                                 # 40 matches of 1 at the least
    on_host = _judged(real, null)                        # the premise, on the CPU, first
    a, b = (torch.from_numpy(np.concatenate(x)).cuda() for x in (rec_a, rec_b))
    scale, shift, go, ge = PLANT_PARAMETERS
    call = dict(counts_a=PLANT_ROWS_A, counts_b=PLANT_ROWS_B, pairs=[(0, 0), (1, 1)],
                gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift)
    scores = align.local_align(a, b, **call)[0]
    got = align.null_scores(a, b, shuffles=PLANT_SHUFFLES, seed=PLANT_SEED, **call)
    assert G._same_bits(scores.cpu().numpy(), real) and G._same_bits(got.cpu().numpy(), null)
    on_device = _judged(scores, got)
    for one, two in zip(on_host, on_device):
        assert two.is_cuda and np.allclose(one.numpy(), two.cpu().numpy(), rtol=1e-12, atol=0)
