"""The search chain on the device, fed by the encoder: ``encode_graphs_device`` ->
``record_scores`` -> ``top_pairs``; ``topk`` (``exclude_records``, ``distinct_records``) ->
``record_of`` -> the seed recipe of ``band_around`` -> banded and unbanded ``local_align`` /
``local_spans`` / ``local_paths``; ``global_paths``.  Every stage is compared with its reference
on that stage's actual input: the float64 definitions on the downloaded rows
(oracle.gine_numpy.pairwise_cosine, the float64 Gotoh programs), and bit for bit the float32
oracles (align_path_oracle, align_band_oracle, align_global_oracle) on the device's own dense
cosines of each pair, as tests/test_gpu_align_band.py does.  The library, its planted relations,
the recipe and the parameter sets are those of tests/search_cases.py; tests/test_search_chain_host.py
shows on the CPU path that the case bites.

One module-scoped case: the library is encoded once and the block downloaded once.  The first
searches and then the whole chain (``_chain``) are queued straight behind the encoder, before
anything of the test's waits for the device or copies the block; the chain runs once more on
another stream.

Measured on an MI355X (every test prints its figures with -s as "measured: ..."):

    twin rows                      600 rows are bit-identical to a row of another record, in 264
                                   groups of up to 5 copies: the figures of the CPU path
    tied tops                      368 rows attain their best cosine outside their own record at
                                   two rows or more, each through twin rows
    record_scores                  largest error 1.19e-07 against the tolerance of 2e-06
    topk / distinct_records        3,187 / 3,181 returned hits have a bit-identical row at a lower
                                   index outside the row's record: each stands in an earlier column
    smallest margin / bound        26.9 ((1, JOIN) under shift -0.25), every other pair above 170
    largest error / bound          0.0041 under PARAMETERS[0], 0.0059 under PARAMETERS[1] (the
                                   window of 163 rows inside record 8)
    broken recipes                 counted on the CPU path (tests/test_search_chain_host.py): 3 of
                                   5 and 5 of 5 planted pairs of records lose score
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_global_oracle as GO
import align_oracle as O
import align_path_oracle as PO
import search_cases as SC
import test_gpu_align_path as GP
from ginfinity_amd import align, distance

pytestmark = pytest.mark.gpu

COSINE_TOL = SC.COSINE_TOL
ROUNDING = 2.0 ** -24        # tests/test_gpu_record_scores.py
K = 8
HALF_WIDTHS = (8, 64)
FACTOR = 2.0                 # tests/test_gpu_align.py; the host file asks for 4 on the CPU path
#: the a-records whose rows' top hits become seeds
SEEDED = (0, 1, 4, 5, 7, SC.COPY, SC.WINDOW)
LOCAL_PAIRS = ((0, SC.COPY), (SC.COPY, 0), (1, SC.JOIN), (7, SC.JOIN)) + SC.FLANKED


def _keywords(parameters):
    scale, shift, go, ge = parameters
    return dict(match_scale=scale, match_shift=shift, gap_open=go, gap_extend=ge)


def _bytes(value):
    """A result as something ``==`` compares byte for byte."""
    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    if isinstance(value, np.ndarray):
        return (value.dtype.str, value.shape, value.tobytes())
    if isinstance(value, (tuple, list)):
        return tuple(_bytes(x) for x in value)
    return value


def _first_calls(block, counts):
    """``record_scores``, ``topk`` and ``record_of`` queued on the current stream; the results stay
    on the device and nothing is waited for."""
    scores = distance.record_scores(block, counts_a=counts, metric="cosine")
    values, indices = distance.topk(block, k=K, metric="cosine", exclude_records=counts)
    return scores, values, indices, distance.record_of(indices, counts)


def _chain(block, counts):
    """Steps 2 to 5 on the current stream, under tuples that name the results.  The block and the
    counts go into every call as ``encode_library`` returned them.  Every stage is queued behind
    the one before it and the results come to the host at the end, with two exceptions that the
    library itself makes: which hits go on (``chosen_hits``) is decided on the host from ``q`` and
    ``r``, and ``local_paths`` brings its spans to the host to size the trace."""
    dev = {}
    scores = distance.record_scores(block, counts_a=counts, metric="cosine")
    dev["record_scores",] = scores
    for name, more in (("topk", {}), ("distinct", dict(distinct_records=counts))):
        values, indices = distance.topk(block, k=K, metric="cosine", exclude_records=counts, **more)
        records = distance.record_of(indices, counts)
        assert records.is_cuda and records.dtype == torch.int32 and records.shape == indices.shape
        dev[name,] = (values, indices, records)
    hits = dev["topk",][1]
    ptr = SC.pointers(counts)
    rows = torch.cat([torch.arange(int(ptr[a]), int(ptr[a + 1])) for a in SEEDED]).to(block.device)
    counts_dev = torch.as_tensor(counts, device=block.device)
    q, r, seeds = SC.seeds_from_hits(rows, hits[rows, 0], counts_dev, counts_dev)
    assert seeds.is_cuda and seeds.shape == (rows.shape[0], 2)
    dev["seeds",] = (rows, q, r, seeds)
    chosen = torch.as_tensor(SC.chosen_hits(q.cpu().numpy(), r.cpu().numpy()), device=block.device)
    pairs, cells = torch.stack([q, r], 1)[chosen], seeds[chosen]
    dev["chosen",] = (pairs, cells)
    common = dict(counts_a=counts, pairs=pairs, **_keywords(SC.PARAMETERS[0]))
    bands = {width: None if width is None else align.band_around(cells, width)
             for width in (None,) + HALF_WIDTHS}
    for width, band in bands.items():
        dev["local_align", width] = align.local_align(block, band=band, **common)
        dev["local_spans", width] = align.local_spans(block, band=band, **common)
    for k, parameters in enumerate(SC.PARAMETERS):
        common = dict(counts_a=counts, **_keywords(parameters))
        dev["planted_global", k] = align.global_paths(block, pairs=[(0, SC.COPY)], within=False,
                                                      **common)
        dev["planted_within", k] = align.global_paths(block, pairs=[(SC.WINDOW, SC.WINDOWED)],
                                                      within=True, **common)
        dev["planted_local", k] = align.local_paths(block, pairs=LOCAL_PAIRS, **common)
    common = dict(counts_a=counts, pairs=pairs, **_keywords(SC.PARAMETERS[0]))
    for width, band in bands.items():
        dev["local_paths", width] = align.local_paths(block, band=band, **common)
    # everything is queued: now the host
    out = {("band", width): band for width, band in bands.items()}
    out["top_pairs",] = align.top_pairs(scores, 3, largest=True)
    for name, value in dev.items():
        if isinstance(value, align.AlignedPaths):
            out[name] = GP._host(value)
        elif name[0] in ("local_align", "local_spans"):
            out[name] = _bytes(value)
        elif isinstance(value, tuple):
            out[name] = tuple(x.cpu().numpy() for x in value)
        else:
            out[name] = value.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def case(gpu_encoder):
    """The searches are queued straight behind the encoder: the first calls on the block of the
    whole records before WINDOW is even encoded, the chain on the library as soon as it is
    whole.  Only then does the block come to the host (once) for the references, and the first
    calls run again on the rows that have settled."""
    whole, whole_counts = SC.encode_whole(gpu_encoder)
    early = _first_calls(whole, whole_counts)
    block, counts = SC.append_window(gpu_encoder, whole, whole_counts)
    chain = _chain(block, counts)
    host = block.cpu().numpy()                      # the one download
    host.setflags(write=False)
    cosine = SC.cosine_f64(host)
    cosine.setflags(write=False)
    settled = _first_calls(whole, whole_counts)
    return dict(block=block, counts=counts, host=host, cosine=cosine, ptr=SC.pointers(counts),
                dense={}, chain=chain, early=_bytes(early), settled=_bytes(settled),
                whole=(whole, whole_counts))


def _rows(case, record):
    return SC.record_rows(case["host"], case["counts"], record)


def _substitution(case, pair, parameters):
    """The float32 substitution matrix of a pair from the device's own dense cosines (computed
    once per pair)."""
    pair = tuple(int(x) for x in pair)
    if pair not in case["dense"]:
        a, b = (case["block"][int(case["ptr"][x]):int(case["ptr"][x + 1])] for x in pair)
        case["dense"][pair] = distance.pairwise(a, b, metric="cosine").cpu().numpy()
    return O.substitution_f32(case["dense"][pair], parameters[0], parameters[1])


def _path(result, p):
    scores, starts, ends, paths, _ = result
    return scores[p], starts[p], ends[p], paths[p]


# 1
def test_hand_off(case):
    block, counts, host = case["block"], case["counts"], case["host"]
    assert block.is_cuda and block.dtype == torch.float16 and block.is_contiguous()
    assert isinstance(counts, tuple) and all(isinstance(x, int) for x in counts)
    assert len(counts) == SC.RECORDS and counts == SC.lengths()
    assert sum(counts) == block.shape[0]
    assert _rows(case, 0).tobytes() == _rows(case, SC.COPY).tobytes()
    twins, groups, largest = SC.twin_rows(host, counts)
    tied, by_twins = SC.tied_tops(case["cosine"], host, counts)
    print(f"measured: {twins} twin rows in {groups} groups of up to {largest}; {tied.sum()} tied "
          f"tops, {(tied & by_twins).sum()} through twin rows")
    assert twins >= 100 and (tied & by_twins).sum() >= 100


def test_searches_queued_behind_the_encoder_see_its_rows(case):
    """What ran straight behind ``encode_graphs_device``, before anything of the test's waited
    for the device, against the same calls on the settled rows: the same bytes.  The early
    ``record_scores`` is also the corner of the chain's, whose rows of WINDOW it never saw (an
    entry does not depend on the other records), and the block of the whole records is the
    front of the library's."""
    whole, whole_counts = case["whole"]
    assert whole.is_cuda and whole_counts == case["counts"][:SC.WINDOW]
    assert whole.cpu().numpy().tobytes() == case["host"][:whole.shape[0]].tobytes()
    assert case["early"] == case["settled"]
    corner = np.ascontiguousarray(case["chain"]["record_scores",][:SC.WINDOW, :SC.WINDOW])
    assert case["early"][0] == _bytes(corner)
    # and the early top-k is the float64 top-k of those rows
    values = np.frombuffer(case["early"][1][2], dtype=np.float32).reshape(-1, K)
    masked = SC.masked_cosine(case["cosine"][:whole.shape[0], :whole.shape[0]], whole_counts)
    assert np.all(np.abs(values - -np.sort(-masked, axis=1)[:, :K]) <= COSINE_TOL)


# 2
def test_record_scores_and_top_pairs(case):
    counts, got = case["counts"], case["chain"]["record_scores",]
    want = SC.record_scores_f64(case["cosine"], counts)
    assert got.shape == want.shape == (SC.RECORDS, SC.RECORDS) and got.dtype == np.float32
    error = np.abs(got.astype(np.float64) - want)
    print(f"measured: record_scores largest error {error.max():.2e} against {COSINE_TOL:.0e}")
    assert np.all(error <= COSINE_TOL + ROUNDING * np.abs(want))
    assert np.all(got.max(axis=1) == np.diag(got))
    same = [got[a, b].tobytes() for a in (0, SC.COPY) for b in (0, SC.COPY)]
    assert len(set(same)) == 1, same
    pairs = case["chain"]["top_pairs",]
    assert pairs.tobytes() == align.top_pairs(got, 3, largest=True).tobytes()
    listed = {tuple(pair) for pair in pairs.tolist()}
    assert set(SC.whole_record_pairs()) <= listed and (SC.WINDOW, SC.WINDOWED) in listed
    best = pairs.reshape(SC.RECORDS, 3, 2)[:, :, 1]
    assert best[0, :2].tolist() == [0, SC.COPY] and best[SC.COPY, :2].tolist() == [0, SC.COPY]


# 3
@pytest.mark.parametrize("name", ("topk", "distinct"))
def test_topk_on_encoder_rows(case, name):
    counts, ptr, cosine = case["counts"], case["ptr"], case["cosine"]
    values, indices, records = case["chain"][name,]
    n = case["host"].shape[0]
    assert values.shape == indices.shape == records.shape == (n, K) and (indices >= 0).all()
    own = np.repeat(np.arange(SC.RECORDS), counts)
    masked = SC.masked_cosine(cosine, counts)
    at_index = np.take_along_axis(masked, indices.astype(np.int64), axis=1)
    assert np.all(np.abs(values - at_index) <= COSINE_TOL)       # -inf inside the own record
    if name == "topk":
        want = -np.sort(-masked, axis=1)[:, :K]
    else:
        per_record = np.stack([masked[:, lo:hi].max(axis=1) for lo, hi in zip(ptr[:-1], ptr[1:])], 1)
        want = -np.sort(-per_record, axis=1)[:, :K]
    assert np.all(np.abs(values - want) <= COSINE_TOL)
    assert np.all(np.diff(values, axis=1) <= 0)
    # record_of on the device against searchsorted on the host, and no hit in the own record
    assert (records == np.searchsorted(ptr[1:], indices, side="right")).all()
    assert (records != own[:, None]).all()
    if name == "distinct":
        assert all(np.unique(row).size == K for row in records)
    # exact ties (twin rows): the lowest index first.  A bit-identical row with a lower index,
    # outside the own record, stands in an earlier column (distinct: its record does)
    groups = SC.row_groups(case["host"])
    members = {}
    for index in np.argsort(groups, kind="stable"):
        members.setdefault(int(groups[index]), []).append(int(index))
    ties = 0
    for x in range(n):
        for k in range(K):
            hit = int(indices[x, k])
            for twin in members[int(groups[hit])]:
                if twin >= hit:
                    break
                if own[twin] == own[x]:
                    continue
                ties += 1
                if name == "topk":
                    assert twin in indices[x, :k], (x, k, hit, twin)
                else:
                    assert own[twin] != own[hit] and own[twin] in records[x, :k], (x, k, hit, twin)
    print(f"measured: {name}: {ties} returned hits have a bit-identical row at a lower index")
    assert ties >= 100


def test_record_of_next_to_the_boundaries_of_copy(case):
    counts, ptr = case["counts"], case["ptr"]
    edge = [int(ptr[SC.COPY]) - 1, int(ptr[SC.COPY]), int(ptr[SC.COPY + 1]) - 1,
            int(ptr[SC.COPY + 1]), 0, int(ptr[-1]) - 1, -1]
    want = [SC.JOIN, SC.COPY, SC.COPY, SC.WINDOW, 0, SC.WINDOW, -1]
    for dtype in (torch.int32, torch.int64):
        got = distance.record_of(torch.tensor(edge, dtype=dtype, device=case["block"].device), counts)
        assert got.is_cuda and got.dtype == torch.int32 and got.cpu().tolist() == want
    # the hits that land there: the rows of record 0 find COPY's, zero distance apart
    _, indices, records = case["chain"]["topk",]
    first = indices[:counts[0]]
    assert ((first >= ptr[SC.COPY]) & (first < ptr[SC.COPY + 1])).any(axis=1).all()
    assert (records[:counts[0]][(first >= ptr[SC.COPY]) & (first < ptr[SC.COPY + 1])] == SC.COPY).all()


# 4
def test_seeds_from_device_hits_lie_inside_both_records(case):
    counts, ptr = np.asarray(case["counts"]), case["ptr"]
    rows, q, r, seeds = case["chain"]["seeds",]
    hit = case["chain"]["topk",][1][rows, 0]
    assert seeds.dtype == np.int64 and q.dtype == r.dtype == np.int32
    assert (q == np.repeat(SEEDED, counts[list(SEEDED)])).all()
    assert (seeds == np.stack([rows - ptr[q], hit - ptr[r]], axis=1)).all()
    assert (seeds >= 0).all() and (seeds[:, 0] < counts[q]).all() and (seeds[:, 1] < counts[r]).all()
    pairs, cells = case["chain"]["chosen",]
    found = {tuple(pair) for pair in pairs.tolist()}
    assert {plant.pair for plant in SC.planted()} | {(SC.COPY, 0)} <= found, found
    assert cells.shape == (len(pairs), 2)


@pytest.mark.parametrize("width", (None,) + HALF_WIDTHS)
def test_alignments_of_the_seeded_pairs_against_the_oracles(case, width):
    parameters = SC.PARAMETERS[0]
    go, ge = parameters[2:]
    chain = case["chain"]
    pairs, cells = chain["chosen",]
    result = chain["local_paths", width]
    scores, starts, ends, paths, _ = result
    assert chain["local_align", width] == _bytes((scores, ends))
    assert chain["local_spans", width] == _bytes((scores, starts, ends))
    bands = chain["band", width]
    for p, pair in enumerate(pairs.tolist()):
        S = _substitution(case, pair, parameters)
        if width is None:
            want = PO.path_of(S, go, ge)
        else:
            diagonal = int(cells[p, 1] - cells[p, 0])
            assert tuple(bands[p]) == (diagonal - width, diagonal + width)
            want = BO.band_path_of(S, go, ge, int(bands[p, 0]), int(bands[p, 1]))
        GP._same_path(_path(result, p), want, (pair, width))
        if want[2] != (-1, -1):
            assert PO.rescore(S, paths[p], want[1], go, ge).tobytes() == scores[p].tobytes()


def test_a_seed_on_the_planted_diagonal_gives_the_unbanded_score(case):
    chain = case["chain"]
    pairs, cells = chain["chosen",]
    diagonal = {plant.pair: plant.start[1] - plant.start[0] for plant in SC.planted()
                if plant.mode != "global"}
    diagonal[SC.COPY, 0] = 0
    on = [p for p, pair in enumerate(pairs.tolist())
          if diagonal.get(tuple(pair)) == cells[p, 1] - cells[p, 0] and pair[0] != SC.WINDOW]
    assert {tuple(pairs[p]) for p in on} == set(SC.whole_record_pairs())
    free = chain["local_paths", None]
    for width in HALF_WIDTHS:
        banded = chain["local_paths", width]
        for p in on:
            assert GP._same_paths(GP._pick(banded, [p]), GP._pick(free, [p])), (pairs[p], width)
            assert free[0][p] > 10


# 5
def _checked_relation(case, plant, parameters, got):
    """The margin on the device's rows first, then the device's answer against the relation and
    the float64 score; returns error / bound."""
    score64, holds, margin, bound = SC.relation(_rows(case, plant.pair[0]),
                                                _rows(case, plant.pair[1]), plant, parameters)
    assert holds and margin > FACTOR * bound, (plant, parameters, margin, bound)
    score, start, end, ops = got
    assert tuple(start) == plant.start and tuple(end) == plant.end, (plant, start, end)
    assert ops.size == plant.length and not ops.any(), (plant, ops.tolist())
    S = _substitution(case, plant.pair, parameters)
    assert PO.rescore(S, ops, plant.start, *parameters[2:]).tobytes() == score.tobytes()
    error = abs(float(score) - score64)
    print(f"measured: {plant} score64 {score64:.4f} error {error:.2e} bound {bound:.2e} "
          f"margin / bound {margin / bound:.1f}")
    assert error <= bound, (plant, float(score), score64, bound)
    return error / bound


@pytest.mark.parametrize("k", range(len(SC.PARAMETERS)))
def test_planted_relations(case, k):
    parameters, chain = SC.PARAMETERS[k], case["chain"]
    go, ge = parameters[2:]
    local = chain["planted_local", k]
    worst = 0.0
    for plant in SC.planted():
        if plant.mode == "local":
            got = _path(local, LOCAL_PAIRS.index(plant.pair))
        else:
            got = _path(chain["planted_" + plant.mode, k], 0)
        worst = max(worst, _checked_relation(case, plant, parameters, got))
    print(f"measured: largest error / bound {worst:.4f}")
    _, start, end, ops = _path(chain["planted_within", k], 0)
    assert tuple(end) == (ops.size - 1, SC.WINDOW_END - 1) and tuple(start) == (0, SC.WINDOW_START)
    # (COPY, 0) mirrors (0, COPY); every local pair, the flanked ones included, bit for bit
    mirror = _path(local, LOCAL_PAIRS.index((SC.COPY, 0)))
    assert GP._same_paths(GP._pick(local, [1]), GP._pick(local, [0])) and not mirror[3].any()
    for p, pair in enumerate(LOCAL_PAIRS):
        GP._same_path(_path(local, p), PO.path_of(_substitution(case, pair, parameters), go, ge), pair)
    for mode, pair in (("global", (0, SC.COPY)), ("within", (SC.WINDOW, SC.WINDOWED))):
        want = GO.path_of(_substitution(case, pair, parameters), go, ge, mode == "within")
        GP._same_path(_path(chain["planted_" + mode, k], 0), want, (mode, pair))


# 6
def test_a_pair_alone_gives_the_bytes_of_the_chain_call(case):
    block, ptr, chain = case["block"], case["ptr"], case["chain"]
    parameters = SC.PARAMETERS[0]

    def alone(function, pair, **more):
        a, b = (block[int(ptr[x]):int(ptr[x + 1])] for x in pair)
        return GP._host(function(torch.cat([a, b]), counts_a=[a.shape[0], b.shape[0]],
                                 pairs=[[0, 1]], **_keywords(parameters), **more))

    local = chain["planted_local", 0]
    for p, pair in enumerate(LOCAL_PAIRS):
        assert GP._same_paths(alone(align.local_paths, pair), GP._pick(local, [p])), pair
    assert GP._same_paths(alone(align.global_paths, (0, SC.COPY), within=False),
                          chain["planted_global", 0])
    assert GP._same_paths(alone(align.global_paths, (SC.WINDOW, SC.WINDOWED), within=True),
                          chain["planted_within", 0])


def _same_results(one, two):
    assert one.keys() == two.keys()
    for name in one:
        assert _bytes(one[name]) == _bytes(two[name]), name


def test_the_chain_on_another_stream_gives_the_same_bytes(case):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = _chain(case["block"], case["counts"])
    side.synchronize()
    _same_results(again, case["chain"])


def test_tensor_and_numpy_forms_of_pairs_and_band(case):
    block, counts, chain = case["block"], case["counts"], case["chain"]
    pairs, _ = chain["chosen",]
    band = chain["band", 8]
    common = dict(counts_a=counts, **_keywords(SC.PARAMETERS[0]))
    forms = ((torch.from_numpy(pairs).to(block.device), torch.from_numpy(band).to(block.device)),
             (torch.from_numpy(pairs.astype(np.int64)), torch.from_numpy(band.astype(np.int64))),
             (pairs.astype(np.int64), band.astype(np.int64)), (pairs.tolist(), band.tolist()))
    for some_pairs, some_band in forms:
        got = GP._host(align.local_paths(block, pairs=some_pairs, band=some_band, **common))
        assert GP._same_paths(got, chain["local_paths", 8])
        assert _bytes(align.local_align(block, pairs=some_pairs, band=some_band, **common)) == \
            chain["local_align", 8]
