"""An edge that joins two records of a micro-batch, through every public path.

The reference accepts such a shard (``GraphShard.__post_init__`` and ``slice`` check the node range
of the shard / the micro-batch only, graph.py:318-321, 414-444; the per-record check is the opt-in
``validate_values``) and hands the micro-batch's whole ``edge_index`` to message passing: the edge
counts.  The record-range set-up (csrc/csr_records.inc) looks for a row's in-edges in the edge
ranges of the records that overlap the workgroup's rows, so an edge whose destination lies in
another record is dropped unless both records overlap one 256 / 512 / 768-row range — and whether
record boundaries travel with a micro-batch is the API's choice, not the caller's.  Every path
must give the embeddings of the honoured edge, all of them the same bytes, while clean shards keep
the record-range set-up.

The expectation is the float64-checked numpy oracle (oracle/gine_numpy.py) run micro-batch by
micro-batch on that micro-batch's arrays.  Every case first proves, with numpy and the oracle
alone, that it can pin something: the crossing edges do cross (and the "far" ones cannot be kept
by accident, whatever the range size), and honouring an edge moves its destination row by at
least 10 x the tolerance.

The second half of the module is the guard for staging-slot reuse between
``encode_shards_device`` and the calls that share its uploader (the proof of the ordering is
tests/test_host_layer.py::test_a_staging_slot_is_acquired_before_it_is_written_or_replaced).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from ginfinity_amd import synthetic
from ginfinity_amd.graph import GraphShard

F16_TOL, F32_TOL = 1e-3, 1e-6          # BASELINE.json north_star tolerances
#: float16 output of the fp32 model (the device-block paths write nothing else): round to nearest
#: of a component of a unit row, |x| <= 1, is off by at most half the spacing below 1.0 = 2^-12
F16_ROUNDING = 2.0 ** -12
RANGE_ROWS = (256, 512, 768)           # gfy_common.h: kRecRowsSmall / kRecRowsLone / kRecRowsLarge

gpu = pytest.mark.gpu


# -- shards ---------------------------------------------------------------------------------------
def _lone(name: str, spec) -> GraphShard:
    """A one-node record without edges."""
    features = np.zeros((1, spec.node_feature_dim), np.float32)
    features[0, [0, 4, 6]] = 1
    return GraphShard(identifiers=(name,), sequences=("A",), structures=(".",),
                      node_features=features, edge_index=np.zeros((2, 0), np.int32),
                      edge_types=np.zeros(0, np.uint8), node_ptr=np.array([0, 1], np.int64),
                      edge_ptr=np.array([0, 0], np.int64), spec=spec,
                      residue_index=np.zeros(1, np.int32), node_roles=np.zeros(1, np.uint8))


def _join(shards) -> GraphShard:
    """The records of several shards as one shard (what ``GraphShard.from_graphs`` does)."""
    node_ptr = np.concatenate([[0]] + [s.node_ptr[1:] + sum(t.node_count for t in shards[:i])
                                       for i, s in enumerate(shards)]).astype(np.int64)
    edge_ptr = np.concatenate([[0]] + [s.edge_ptr[1:] + sum(t.edge_count for t in shards[:i])
                                       for i, s in enumerate(shards)]).astype(np.int64)
    bases = np.cumsum([0] + [s.node_count for s in shards[:-1]])

    def joined(name):
        return np.ascontiguousarray(np.concatenate([getattr(s, name) for s in shards]))
    return GraphShard(
        identifiers=sum((s.identifiers for s in shards), ()),
        sequences=sum((s.sequences for s in shards), ()),
        structures=sum((s.structures for s in shards), ()),
        node_features=joined("node_features"),
        edge_index=np.ascontiguousarray(np.concatenate(
            [s.edge_index + np.int32(b) for s, b in zip(shards, bases)], axis=1)),
        edge_types=joined("edge_types"), node_ptr=node_ptr, edge_ptr=edge_ptr,
        spec=shards[0].spec, residue_index=joined("residue_index"),
        node_roles=joined("node_roles"))


@dataclasses.dataclass
class Case:
    name: str
    clean: GraphShard
    crossed: GraphShard
    #: (edge id, source, destination, far): ``far`` = the destination lies in another record and
    #: in no row range, of any size, that the owning record overlaps
    edges: list
    limits: dict                    # max_batch_nodes / max_batch_edges of every call
    expected: dict = dataclasses.field(default_factory=dict)


def _owner(shard: GraphShard, edge: int) -> int:
    return int(np.searchsorted(shard.edge_ptr, edge, side="right")) - 1


def _record_of(shard: GraphShard, node: int) -> int:
    return int(np.searchsorted(shard.node_ptr, node, side="right")) - 1


def _cross(name: str, clean: GraphShard, changes, **limits) -> Case:
    """``changes``: (record, position in the record's edge list, source or None, destination or
    None) — the edge keeps its list position and so the record that owns it.  The new shard is
    built through ``GraphShard``'s own validation: it is legal input."""
    edges = clean.edge_index.copy()
    listed = []
    for record, position, source, destination in changes:
        edge = int(clean.edge_ptr[record]) + position
        assert edge < int(clean.edge_ptr[record + 1])
        if source is not None:
            edges[0, edge] = source
        if destination is not None:
            edges[1, edge] = destination
        listed.append([edge, int(edges[0, edge]), int(edges[1, edge]), False])
    crossed = dataclasses.replace(clean, edge_index=edges)
    return Case(name, clean, crossed, listed, limits)


def _first_core(shard: GraphShard, record: int, at_least: int) -> int:
    rows = np.flatnonzero(shard.node_roles == 0)
    rows = rows[(rows >= max(at_least, int(shard.node_ptr[record]))) & (rows < shard.node_ptr[record + 1])]
    return int(rows[0])


def _cases() -> list[Case]:
    spec = synthetic.roofline_shard(0, records=1, length=2).spec
    # 1. four 700-node records: a destination 2,490 rows away, a source in another record, and a
    #    pair of rows on both sides of the boundary at 700, inside the aligned range 512..767
    far = _cross("far", synthetic.roofline_shard(1, records=4, length=700), [
        (0, 5, 10, 2500),            # record 0 -> record 3: the destination is elsewhere
        (3, 2500, 20, None),         # record 3's edge, its source in record 0
        (0, 9, 690, 710),            # record 0 -> record 1, 20 rows apart
        (2, 3499, 1405, 5),          # the LAST edge of record 2 -> record 0
    ])
    # 2. one-node records without edges in front of, between and behind the records that the
    #    edges join (two records apart), and a destination that IS such a record
    parts = [_lone("l0", spec), synthetic.roofline_shard(11, records=1, length=600),
             _lone("l1", spec), _lone("l2", spec), synthetic.roofline_shard(12, records=1, length=600),
             _lone("l3", spec), synthetic.roofline_shard(13, records=1, length=600), _lone("l4", spec)]
    gaps = _cross("gaps", _join(parts), [
        (1, 0, 7, 1500),             # record 1 (rows 1..600) -> record 6 (rows 1204..1803)
        (6, 33, 1300, 100),          # record 6 -> record 1
        (6, 34, 1301, 0),            # record 6 -> the one-node record 0
        (4, 2999, 700, 602),         # record 4's last edge -> the one-node record 3 next to it
    ])
    # 3. context rows (node_roles) and all ten edge types, hubs: the destination is a core row
    arbitrary = synthetic.arbitrary_shard(2, nodes=3000, edges=12000, records=4)
    assert arbitrary.node_roles.any()
    target = _first_core(arbitrary, 3, int(arbitrary.node_ptr[1] // 768 + 2) * 768)
    back = _first_core(arbitrary, 0, 3)
    roles = _cross("roles", arbitrary, [
        (0, 17, None, target),       # record 0 -> a core row of record 3, far
        (3, 40, None, back),         # record 3 -> a core row of record 0
    ])
    # 4. twelve 500-node records in micro-batches of two: the edges join the two records of the
    #    second micro-batch, in both directions; every other micro-batch is clean
    many = synthetic.roofline_shard(5, records=12, length=500)
    multi = _cross("multi", many, [
        (2, 11, 1003, 1900),         # record 2 -> record 3, rows 3 and 900 of the micro-batch
        (3, 0, 1990, 1010),          # record 3 -> record 2
        (3, 2499, 1100, None),       # record 3's last edge: its source in record 2
    ], max_batch_nodes=1000)
    return [far, gaps, roles, multi]


def _bounds(case: Case):
    from ginfinity_amd import api
    shard = case.crossed
    return api.microbatch_bounds(
        shard.lengths, shard.edge_counts, case.limits.get("max_batch_nodes", 60_000),
        case.limits.get("max_batch_edges", 300_000))


def _microbatch_arrays(shard: GraphShard, start: int, stop: int):
    n0, n1 = int(shard.node_ptr[start]), int(shard.node_ptr[stop])
    e0, e1 = int(shard.edge_ptr[start]), int(shard.edge_ptr[stop])
    return (shard.node_features[n0:n1], shard.edge_index[:, e0:e1] - np.int32(n0),
            shard.edge_types[e0:e1], shard.node_roles[n0:n1] == 0)


def _oracle(weights, shard: GraphShard, bounds, **options) -> np.ndarray:
    """``G.encode`` micro-batch by micro-batch, the core rows of all of them."""
    from oracle import gine_numpy as G
    blocks = []
    for start, stop in bounds:
        features, edges, types, core = _microbatch_arrays(shard, start, stop)
        blocks.append(G.encode(weights, features, edges, types, **options)[core])
    return np.concatenate(blocks)


def _prove(case: Case, weights) -> None:
    """The two conditions on the INPUT, from numpy and the oracle alone (module docstring)."""
    from oracle import gine_numpy as G
    shard, bounds = case.crossed, _bounds(case)
    assert len(bounds) == (6 if case.name == "multi" else 1)
    crossing = 0
    for entry in case.edges:
        edge, source, destination, _far = entry
        owner = _owner(shard, edge)
        inside = [(a, b) for a, b in bounds if a <= owner < b]
        (start, stop), = inside
        first, last = int(shard.node_ptr[start]), int(shard.node_ptr[stop])
        # the edge stays inside its micro-batch: legal there, too
        assert first <= source < last and first <= destination < last, entry
        assert owner != _record_of(shard, destination) or owner != _record_of(shard, source), entry
        if owner == _record_of(shard, destination):
            continue                                  # only the source is elsewhere
        crossing += 1
        own_rows = np.arange(int(shard.node_ptr[owner]), int(shard.node_ptr[owner + 1])) - first
        entry[3] = all((destination - first) // size not in set((own_rows // size).tolist())
                       for size in RANGE_ROWS)
        if not entry[3]:
            continue
        # honoured against removed, at the destination row, on the micro-batch's arrays
        features, edges, types, _core = _microbatch_arrays(shard, start, stop)
        local = edge - int(shard.edge_ptr[start])
        honoured = G.encode(weights, features, edges, types)
        removed = G.encode(weights, features, np.delete(edges, local, axis=1),
                           np.delete(types, local))
        row = destination - first
        moved = float(np.abs(honoured[row].astype(np.float64)
                             - removed[row].astype(np.float64)).max())
        print(f"{case.name}: edge {edge} ({source} -> {destination}) moves its row by {moved:.4f}")
        assert moved >= 10 * F16_TOL, (case.name, entry, moved)
        assert bool(shard.node_roles[destination] == 0), entry     # ... a row that is returned
    assert crossing >= 2 and sum(1 for entry in case.edges if entry[3]) >= 1, case.edges
    # the clean twin really is clean, the crossed one is not
    from ginfinity_amd.engine import records_pay
    assert records_pay(shard.node_ptr, shard.edge_ptr)
    case.clean.validate_values()
    from ginfinity_amd.spec import GraphValidationError
    with pytest.raises(GraphValidationError):
        shard.validate_values()


@pytest.fixture(scope="module")
def cases(oracle_weights):
    built = {}
    for case in _cases():
        _prove(case, oracle_weights)
        bounds = _bounds(case)
        for label, shard in (("crossed", case.crossed), ("clean", case.clean)):
            case.expected[label] = _oracle(oracle_weights, shard, bounds)
        case.expected["crossed32"] = _oracle(oracle_weights, case.crossed, bounds,
                                             full_precision=True, embedding_dtype=np.float32)
        built[case.name] = case
    return built


CASES = ("far", "gaps", "roles", "multi")


def test_the_cases_contain_what_they_should(cases):
    """The helper gives every kind of edge the paths have to survive (and ``cases`` has proved
    each of them against the oracle): destinations in another record, sources in another record,
    records two apart with one-node zero-edge records around them, rows more than 768 apart and
    rows inside one aligned 256-row range, context rows, several micro-batches."""
    far = cases["far"]
    by_edge = {(s, d): is_far for _e, s, d, is_far in far.edges}
    assert by_edge[(10, 2500)] and 2500 - 10 > 768
    assert 690 // 256 == 710 // 256 and not by_edge[(690, 710)]
    assert _record_of(far.crossed, 690) != _record_of(far.crossed, 710)
    source_only = [e for e in far.edges if _owner(far.crossed, e[0]) == _record_of(far.crossed, e[2])]
    assert source_only and all(_owner(far.crossed, e[0]) != _record_of(far.crossed, e[1])
                               for e in source_only)
    gaps = cases["gaps"].crossed
    assert gaps.lengths == (1, 600, 1, 1, 600, 1, 600, 1)
    assert gaps.edge_counts[0] == gaps.edge_counts[2] == gaps.edge_counts[3] == 0
    pairs = {(_owner(gaps, e), _record_of(gaps, d)) for e, _s, d, _f in cases["gaps"].edges}
    assert {(1, 6), (6, 1), (6, 0), (4, 3)} <= pairs
    # (why no reduceat over edge ranges: an empty segment answers with its neighbour's element)
    assert np.minimum.reduceat(np.array([5, 1, 7, 9, 2]), [0, 3, 3]).tolist() == [1, 9, 2]
    assert cases["roles"].crossed.node_roles.any()
    multi = cases["multi"]
    assert len(_bounds(multi)) == 6
    assert {_owner(multi.crossed, e) for e, *_rest in multi.edges} == {2, 3}


# -- the paths ------------------------------------------------------------------------------------
def _rows(arrays) -> np.ndarray:
    return np.concatenate([np.asarray(a) for a in arrays])


def _encode_graphs(encoder, shard, limits, dtype, **switches):
    saved = (encoder.pinned_outputs, encoder.independent_outputs)
    try:
        for name, value in switches.items():
            setattr(encoder, name, value)
        return _rows(encoder.encode_graphs(shard, embedding_dtype=dtype, **limits))
    finally:
        encoder.pinned_outputs, encoder.independent_outputs = saved


def _shards_device(native_packer: bool, lanes: int):
    def run(encoder, shard, limits, dtype, monkeypatch):
        from ginfinity_amd import api
        monkeypatch.setattr(api, "NATIVE_PACKER", native_packer)
        monkeypatch.setattr(api, "HOST_FEED_LANES", lanes)
        block, counts = encoder.encode_shards_device([shard], **limits)
        assert counts == [shard.core_counts]
        return block.cpu().numpy()
    return run


def _staged(encoder, shard, limits, dtype, monkeypatch):
    staged, counts = encoder.stage_shards(shard, **limits)
    assert counts == [shard.core_counts]
    return encoder.encode_staged(staged).cpu().numpy()


#: name -> (run(encoder, shard, limits, dtype, monkeypatch), returns host arrays of ``dtype``)
PATHS = {
    "encode_graphs": (lambda e, s, l, d, m: _encode_graphs(e, s, l, d), True),
    "encode_graphs-pageable": (
        lambda e, s, l, d, m: _encode_graphs(e, s, l, d, pinned_outputs=False), True),
    "encode_graphs-independent": (
        lambda e, s, l, d, m: _encode_graphs(e, s, l, d, independent_outputs=True), True),
    "encode_graphs_device": (
        lambda e, s, l, d, m: e.encode_graphs_device(s, **l)[0].cpu().numpy(), False),
    "encode_shards_device-native-1": (_shards_device(True, 1), False),
    "encode_shards_device-native-2": (_shards_device(True, 2), False),
    "encode_shards_device-numpy-1": (_shards_device(False, 1), False),
    "encode_shards_device-numpy-2": (_shards_device(False, 2), False),
    "stage_shards+encode_staged": (_staged, False),
}


def _worst(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())


@gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", CASES)
def test_a_cross_record_edge_is_honoured_on_every_path(gpu_encoder, cases, monkeypatch, name, path):
    """fp16 model: the crossed shard within ``F16_TOL`` of the oracle with the edges honoured;
    then the clean twin through the same path, within tolerance too and on the same layer kernel
    (the launch sizes did not change)."""
    case, (run, _host_dtype) = cases[name], PATHS[path]
    got = run(gpu_encoder, case.crossed, case.limits, np.float16, monkeypatch)
    assert got.dtype == np.float16
    kernel = gpu_encoder._engine.last_layer_kernel()
    worst = _worst(got, case.expected["crossed"])
    print(f"{name} / {path}: max |hip - oracle| = {worst:.3e}")
    assert worst <= F16_TOL, (name, path, worst)
    clean = run(gpu_encoder, case.clean, case.limits, np.float16, monkeypatch)
    assert _worst(clean, case.expected["clean"]) <= F16_TOL, (name, path)
    assert gpu_encoder._engine.last_layer_kernel() == kernel != 0


def _batch_calls(encoder) -> np.ndarray:
    """(record-range, counting) batch calls so far, over the encoder's lanes."""
    engines = [encoder._engine]
    if encoder._lanes is not None:
        engines = [engine for engine, _stream in encoder._lanes]
    return np.array([sum(e.ranged_batch_calls for e in engines),
                     sum(e.counting_batch_calls for e in engines)])


@gpu
@pytest.mark.parametrize("name", CASES)
def test_all_paths_give_the_same_bytes_and_clean_shards_keep_the_record_ranges(
        gpu_encoder, cases, monkeypatch, name):
    """Every path returns the SAME bytes for the crossed shard, and for the clean one.  The
    counters of ``DeviceEncoder`` say which set-up the batch calls took: a clean shard's take the
    record-range set-up wherever boundaries travel (everywhere but the mapped inputs of
    ``encode_graphs``' default and a shard that ``encode_graphs`` runs as one micro-batch through
    ``gfy_encode_coo``); of the crossed shard's only the group with the crossed micro-batch
    counts."""
    from ginfinity_amd import api
    case = cases[name]
    micro = len(_bounds(case))
    crossed_at = 1 if name == "multi" else 0          # the micro-batch with the crossing edges
    outputs = {"crossed": {}, "clean": {}}
    for path, (run, _host_dtype) in PATHS.items():
        if path.startswith("encode_graphs") and not path.endswith("device"):
            groups = api._groups(micro, ramp=True) if micro > 1 else []
            boundaries = path != "encode_graphs"      # the default reads mapped inputs: counting
        else:
            groups, boundaries = api._groups(micro), True
        hit = sum(1 for group in groups if crossed_at in group)
        for label, shard in (("crossed", case.crossed), ("clean", case.clean)):
            before = _batch_calls(gpu_encoder)
            outputs[label][path] = run(gpu_encoder, shard, case.limits, np.float16, monkeypatch)
            ranged, counting = (_batch_calls(gpu_encoder) - before).tolist()
            if not boundaries:
                want = (0, len(groups))
            elif label == "clean":
                want = (len(groups), 0)
            else:
                want = (len(groups) - hit, hit)
            assert (ranged, counting) == want, (name, path, label)
    for label, by_path in outputs.items():
        first = by_path["encode_graphs"]
        assert _worst(first, case.expected[label]) <= F16_TOL
        for path, got in by_path.items():
            assert got.tobytes() == first.tobytes(), (name, label, path)
    assert outputs["crossed"]["encode_graphs"].tobytes() != outputs["clean"]["encode_graphs"].tobytes()


@gpu
@pytest.mark.parametrize("name", CASES)
def test_a_cross_record_edge_with_the_fp32_model(gpu_encoder_fp32, cases, monkeypatch, name):
    """fp32 model: the paths that return host arrays, asked for float32, within ``F32_TOL``; the
    device-block paths write float16 and are held to ``F32_TOL`` plus the rounding of that
    format (``F16_ROUNDING``).  (The fp32 model has no record-range set-up: this pins the paths'
    packing, not a set-up.)"""
    case = cases[name]
    want = case.expected["crossed32"]
    for path, (run, host_dtype) in PATHS.items():
        dtype = np.float32 if host_dtype else np.float16
        got = run(gpu_encoder_fp32, case.crossed, case.limits, dtype, monkeypatch)
        assert got.dtype == dtype
        worst = _worst(got, want)
        print(f"{name} / {path} (fp32 model, {np.dtype(dtype).name}): {worst:.3e}")
        assert worst <= (F32_TOL if host_dtype else F32_TOL + F16_ROUNDING), (name, path, worst)


@pytest.mark.parametrize("name", CASES)
def test_a_cross_record_edge_on_the_cpu_device(cases, name):
    """``Ginfinity.load("cpu")`` (csrc/gine_host.cpp) honours the edge as well: the expectation
    of the GPU paths is the expectation of the host path."""
    from ginfinity_amd import Ginfinity
    case = cases[name]
    got = _rows(Ginfinity.load("cpu").encode_graphs(case.crossed, **case.limits))
    assert _worst(got, case.expected["crossed"]) <= F16_TOL
    full = _rows(Ginfinity.load("cpu", full_precision=True).encode_graphs(
        case.crossed, embedding_dtype=np.float32, **case.limits))
    assert _worst(full, case.expected["crossed32"]) <= F32_TOL


# -- staging-slot reuse behind encode_shards_device ----------------------------------------------------
def _fresh():
    from ginfinity_amd import Ginfinity
    return Ginfinity.load("cuda", allow_nondeterministic_cuda=True)


def _shard_bytes(shard: GraphShard) -> list[bytes]:
    return [np.ascontiguousarray(getattr(shard, name)).tobytes()
            for name in ("node_features", "edge_index", "edge_types", "node_ptr", "edge_ptr",
                         "residue_index", "node_roles")]


@gpu
def test_calls_that_share_the_uploader_do_not_disturb_uploads_in_flight(rouskin_records,
                                                                        rouskin_shard):
    """``encode_shards_device`` returns with its last uploads (``gfy_upload_async``: guarded by the
    native ring's events only) possibly still reading the staging slots; ``encode_graphs``,
    ``encode_many`` and ``build_graphs_device`` write the same slots through ``_Uploader.pack``.
    Called one right behind the other on one encoder, both calls must give, bit for bit, what the
    same calls give on fresh encoders with a device synchronisation between them.  Round 2: the
    follower needs LARGER slots than ``encode_shards_device`` left (6,000-node micro-batches
    against 60,000-node ones), so every slot it takes is reallocated.  Once each, no loop, no
    sleep: this is the guard — it can pass by luck where the ordering is wrong; the proof of the
    ordering is the host-layer test named in the module docstring."""
    from ginfinity_amd import RNA
    feed = [rouskin_shard, synthetic.roofline_shard(5)]        # 16 micro-batches: 4 groups
    small = dict(max_batch_nodes=6_000)                        # ~40 micro-batches of the slice below
    part = rouskin_shard.slice(0, 1500)                        # ~230,000 nodes: 4 micro-batches
    records = rouskin_records[:1500]
    windows = [RNA(r.identifier, r.sequence, r.structure, start=2, end=min(40, r.length))
               if r.length > 12 and i % 2 else r for i, r in enumerate(rouskin_records[:400])]
    followers = {
        "encode_graphs": lambda e: [_rows(e.encode_graphs(part)).tobytes()],
        "encode_graphs-pageable": lambda e: [_rows(_pageable(e).encode_graphs(part)).tobytes()],
        "encode_many": lambda e: [_rows(e.encode_many(records)).tobytes()],
        "build_graphs_device": lambda e: _shard_bytes(e.build_graphs_device(windows)),
    }

    def _pageable(encoder):
        encoder.pinned_outputs = False
        return encoder

    rounds = (("same slots", feed, {}), ("larger slots", [part], small))
    # the expectation: fresh encoders, everything finished before the next call starts
    want = {}
    for label, shards, limits in rounds:
        for name, follow in followers.items():
            encoder = _fresh()
            block, counts = encoder.encode_shards_device(shards, **limits)
            torch.cuda.synchronize()
            first = block.cpu().numpy().tobytes()
            want[label, name] = (first, counts, follow(encoder))
            torch.cuda.synchronize()
    for label, shards, limits in rounds:
        for name, follow in followers.items():
            encoder = _fresh()
            block, counts = encoder.encode_shards_device(shards, **limits)
            behind = follow(encoder)                   # at once: no synchronisation in between
            first = block.cpu().numpy().tobytes()
            assert counts == want[label, name][1]
            assert first == want[label, name][0], (label, name, "encode_shards_device's own result")
            assert behind == want[label, name][2], (label, name, "the call behind it")
            if label == "larger slots" and name.startswith("encode_graphs"):
                grown = [s.numel() for s in encoder._uploader._staging if s is not None]
                assert max(grown) > 3 << 20, grown       # (a 60,000-node micro-batch: 4.4 MB)
