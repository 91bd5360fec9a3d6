"""The per-wave pair loop of the alignment kernels: more pairs than the grid has waves.

A wave takes the pairs ``slot, slot + slots, ...`` and the grid is capped at 256 workgroups of 4
waves, so a wave meets a second pair only in a call of more than 1024 pairs.  Here P = 1024 +
300: waves 0 .. 299 serve two pairs each, and everything a wave keeps between them — its best
cell, the last H of its lanes, the running borders, the two carry buffers, the ring, and under a
band the column range and the outside values after a skipped strip — must come from the second
pair alone.  The pairs are the tie zoo of tests/align_cases.py (exact arithmetic, answers full
of ties) and the float records of tests/test_gpu_align.py up to 129 x 129, in one call; the
seats are arranged so that on one wave a long pair (three strips, 129 columns) is followed by a
1 x 1 pair and by a pair with an empty record, a short pair by a long one, a pair by itself, and
tie data by float data and back.

Every result must equal, bit for bit, the same pair's result from a call of at most 36 pairs, in
which each pair has a wave of its own, and those are held against the oracles first.  A second
launch on the same ``AlignWorkspace`` and a launch in shuffled order must give the same bits."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_cases as Z
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import test_gpu_align as G
import test_gpu_align_path as GP
import test_gpu_align_ties as T
from ginfinity_amd import _native as native
from ginfinity_amd import align

pytestmark = pytest.mark.gpu

K = 0                                   # TIE_PARAMETERS[0] for every pair of the call
PARAMETERS = Z.TIE_PARAMETERS[K]
WAVES_OF_THE_GRID = 256 * G.WAVES       # kAlignGroupsMax workgroups (align_local.inc)
P = WAVES_OF_THE_GRID + 300
SMALL = 36                              # pairs of a small call: a wave each
FLOAT_A = (0, 1, 2, 3, 4)               # G.ROWS_A 1, 63, 64, 65, 129
FLOAT_B = (0, 1, 2, 3)                  # G.ROWS_B 1, 127, 128, 129
CALLS = ("local_align", "local_spans", "global", "within", "local_align_band",
         "local_spans_band", "local_paths")
NOTHING = (np.float32(0), (-1, -1), (-1, -1), np.zeros(0, dtype=np.uint8))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return native.library()


@functools.lru_cache(maxsize=None)
def _crowd():
    """The zoo's and the float case's records in one pair of tensors, the kinds of pair (record
    of a, record of b, substitution matrix, band) and the seat of every kind in the call."""
    zoo, case = T._device(), G._case()
    scale, shift, go, ge = PARAMETERS
    kinds = []
    for q, r in Z.zoo()["pairs"]:
        q, r = int(q), int(r)
        if Z.ROWS_A[q] == 0 or Z.ROWS_B[r] == 0:
            kinds.append(dict(pair=(q, r), S=None, band=(-3, 3), zoo=(q, r)))
        else:
            band = Z.bands_of(q, r, K)[4 if (q, r) == (5, 5) else (q + r) % 4]
            kinds.append(dict(pair=(q, r), S=T._substitution(q, r, K), band=band, zoo=(q, r)))
    long = len(kinds) - 1                                   # 130 x 129 under the band that skips
    assert kinds[long]["pair"] == (5, 5) and kinds[long]["band"] == (-129, -128)
    for kind in (2, 3):                                     # the same pair under two more bands
        kinds.append(dict(kinds[long], band=Z.bands_of(5, 5, K)[kind]))
    for q in FLOAT_A:
        for r in FLOAT_B:
            S = O.substitution_f32(case["cosines"][q * len(G.ROWS_B) + r], scale, shift)
            start = PO.path_of(S, go, ge)[1]
            seed = start[1] - start[0] if start != (-1, -1) else 0
            kinds.append(dict(pair=(len(Z.ROWS_A) + q, len(Z.ROWS_B) + r), S=S,
                              band=(seed - 8, seed + 8), zoo=None))
    float_long = len(kinds) - 1                             # 129 x 129: three strips
    assert kinds[float_long]["S"].shape == (129, 129)
    kinds.append(dict(kinds[float_long], band=(-128, -128)))   # rows 0 .. 127 hold no band cell
    one = Z.pair_index(1, 1)
    rng = np.random.default_rng(P)
    seats = rng.integers(0, len(kinds), size=P)
    seats[400:400 + len(kinds)] = rng.permutation(len(kinds))     # every kind is there
    pairs_of_a_wave = [(long, one), (long, Z.pair_index(5, 0)), (one, long),
                       (Z.pair_index(0, 5), long), (long, long), (float_long, one),
                       (one, float_long), (float_long, float_long), (long, float_long),
                       (float_long, long), (float_long + 1, float_long), (long + 1, long + 2)]
    for wave, (first, second) in enumerate(pairs_of_a_wave):
        seats[wave], seats[wave + WAVES_OF_THE_GRID] = first, second
    assert set(seats.tolist()) == set(range(len(kinds)))
    return dict(a=torch.cat([zoo["a"], case["a"]]), b=torch.cat([zoo["b"], case["b"]]),
                counts_a=Z.ROWS_A + G.ROWS_A, counts_b=Z.ROWS_B + G.ROWS_B, kinds=kinds,
                seats=seats, order=rng.permutation(P))


def _run(call, pairs, bands, workspace=None):
    """One call of ``pairs`` (and ``bands`` where the call has one): the arrays on the host, in
    the order (scores, [starts,] ends), and the ops of every pair or None."""
    crowd = _crowd()
    scale, shift, go, ge = PARAMETERS
    common = dict(counts_a=crowd["counts_a"], counts_b=crowd["counts_b"], pairs=pairs,
                  gap_open=go, gap_extend=ge, match_scale=scale, match_shift=shift,
                  workspace=workspace)
    rows = (crowd["a"], crowd["b"])
    if call == "local_paths":
        scores, starts, ends, ops, _ = GP._host(align.local_paths(*rows, **common))
        return (scores, starts, ends), ops
    if call in ("global", "within"):
        result = align.global_align(*rows, within=call == "within", **common)
    elif call.startswith("local_align"):
        result = align.local_align(*rows, band=bands if call.endswith("_band") else None, **common)
    else:
        result = align.local_spans(*rows, band=bands if call.endswith("_band") else None, **common)
    return tuple(x.cpu().numpy() for x in result), None


def _records(arrays, ops):
    """Per pair the bytes of everything the call returned for it."""
    return [tuple(x[p].tobytes() for x in arrays) + ((ops[p].tobytes(),) if ops else ())
            for p in range(arrays[0].shape[0])]


@functools.lru_cache(maxsize=None)
def _oracle(what, number):
    kind = _crowd()["kinds"][number]
    go, ge = PARAMETERS[2:]
    if kind["S"] is None:
        return NOTHING
    if what in ("global", "within"):
        score, end = GO.score_of(kind["S"], go, ge, what == "within")
        return score, None, end, None
    if what == "band":
        return Z.banded(*kind["zoo"], K, kind["band"]) if kind["zoo"] else \
            BO.band_path_of(kind["S"], go, ge, *kind["band"])
    return Z.path(*kind["zoo"], K) if kind["zoo"] else PO.path_of(kind["S"], go, ge)


def _wanted(call, number):
    """The oracle's (score, start, end, ops) of kind ``number`` for ``call``, computed once per
    oracle; start and ops are None where the call's oracle has none."""
    return _oracle("band" if call.endswith("_band") else call if call in ("global", "within")
                   else "local", number)


def _small_calls(call):
    """Every kind in calls of at most SMALL pairs, held against the oracle: its records."""
    kinds = _crowd()["kinds"]
    records = []
    for first in range(0, len(kinds), SMALL):
        chunk = kinds[first:first + SMALL]
        arrays, ops = _run(call, np.array([kind["pair"] for kind in chunk], dtype=np.int32),
                           np.array([kind["band"] for kind in chunk], dtype=np.int32))
        for p in range(len(chunk)):
            score, start, end, path = _wanted(call, first + p)
            where = (call, chunk[p]["pair"], chunk[p]["band"])
            assert arrays[0][p].tobytes() == np.float32(score).tobytes() or \
                (score == 0 and arrays[0][p] == 0), (where, arrays[0][p], score)
            assert tuple(arrays[-1][p]) == end, (where, arrays[-1][p], end)
            if len(arrays) == 3:
                assert tuple(arrays[1][p]) == start, (where, arrays[1][p], start)
            if ops:
                assert ops[p].tobytes() == path.tobytes(), (where, ops[p].tolist(), path.tolist())
        records += _records(arrays, ops)
    return records


def _first_difference(got, want):
    for seat, (one, two) in enumerate(zip(got, want)):
        if one != two:
            return seat
    return None if len(got) == len(want) else min(len(got), len(want))


@pytest.mark.parametrize("call", CALLS)
def test_the_second_pair_of_a_wave_equals_the_pair_in_a_small_call(call):
    crowd = _crowd()
    kinds, seats, order = crowd["kinds"], crowd["seats"], crowd["order"]
    small = _small_calls(call)
    assert sum(record[0] != np.float32(0).tobytes() for record in small) >= len(small) // 4
    pairs = np.array([kinds[k]["pair"] for k in seats], dtype=np.int32)
    bands = np.array([kinds[k]["band"] for k in seats], dtype=np.int32)
    keeper = align.AlignWorkspace()
    first = _records(*_run(call, pairs, bands, keeper))
    seat = _first_difference(first, [small[k] for k in seats])
    assert seat is None, (call, seat, kinds[seats[seat]]["pair"], kinds[seats[seat]]["band"],
                          "behind", kinds[seats[seat - WAVES_OF_THE_GRID]]["pair"]
                          if seat >= WAVES_OF_THE_GRID else None)
    again = _records(*_run(call, pairs, bands, keeper))
    assert _first_difference(again, first) is None, (call, _first_difference(again, first))
    shuffled = _records(*_run(call, pairs[order], bands[order]))
    seat = _first_difference(shuffled, [first[p] for p in order])
    assert seat is None, (call, seat)


def test_raw_calls_a_refused_pair_does_not_touch_the_waves_next_pair(gpu):
    """The C calls with P = 1025: pair 0 names a record that does not exist and is refused (NaN,
    (-2, -2)); pair 1024 comes to the same wave behind it and must equal its result alone.  And
    the other way round, the refused pair behind the good one."""
    crowd = _crowd()
    kinds, seats = crowd["kinds"], crowd["seats"]
    long = kinds[Z.pair_index(5, 5)]["pair"]
    bad = (len(crowd["counts_a"]), 0)
    ptr_a = torch.tensor(np.concatenate(([0], np.cumsum(crowd["counts_a"]))), dtype=torch.int32).cuda()
    ptr_b = torch.tensor(np.concatenate(([0], np.cumsum(crowd["counts_b"]))), dtype=torch.int32).cuda()
    most_b = max(crowd["counts_b"][:len(Z.ROWS_B) + len(FLOAT_B)])
    stream = torch.cuda.current_stream().cuda_stream
    a, b = crowd["a"], crowd["b"]

    def call(name, pair_list):
        pairs = torch.tensor(pair_list, dtype=torch.int32).cuda()
        count = pairs.shape[0]
        scores = torch.full((count,), 7.0, dtype=torch.float32).cuda()
        starts = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        ends = torch.full((count, 2), 7, dtype=torch.int32).cuda()
        span = name == "gfy_align_local_span"
        sizer = gpu.gfy_align_span_workspace_bytes if span else gpu.gfy_align_workspace_bytes
        need = sizer(count, most_b)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        head = (a.data_ptr(), a.shape[0], ptr_a.data_ptr(), len(crowd["counts_a"]), b.data_ptr(),
                b.shape[0], ptr_b.data_ptr(), len(crowd["counts_b"]), pairs.data_ptr(), count,
                *PARAMETERS)
        tail = (scratch.data_ptr(), need, stream)
        if name == "gfy_align_local":
            code = gpu.gfy_align_local(*head, scores.data_ptr(), ends.data_ptr(), *tail)
        elif span:
            code = gpu.gfy_align_local_span(*head, scores.data_ptr(), starts.data_ptr(),
                                            ends.data_ptr(), *tail)
        else:
            code = gpu.gfy_align_global(*head, int(name == "within"), scores.data_ptr(),
                                        ends.data_ptr(), *tail)
        native.check(code, name)
        torch.cuda.synchronize()
        outputs = (scores, starts, ends) if span else (scores, ends)
        return tuple(x.cpu().numpy() for x in outputs)

    # pairs that fit the carry of this call: the float records of more than 129 rows stay out
    fitting = [kinds[k]["pair"] for k in seats[:WAVES_OF_THE_GRID + 1]]
    for name in ("gfy_align_local", "gfy_align_local_span", "global", "within"):
        alone = call(name, [long])
        assert alone[0][0] > 10         # local 84.5, global and within a little less
        for refused, served in ((0, WAVES_OF_THE_GRID), (WAVES_OF_THE_GRID, 0)):
            pair_list = list(fitting)
            pair_list[refused], pair_list[served] = bad, long
            got = call(name, pair_list)
            assert np.isnan(got[0][refused]), (name, refused, got[0][refused])
            assert all(tuple(x[refused]) == (-2, -2) for x in got[1:]), (name, refused)
            assert all(G._same_bits(x[served:served + 1], y) for x, y in zip(got, alone)), \
                (name, served, [x[served] for x in got], alone)
            assert not np.isnan(np.delete(got[0], refused)).any()
