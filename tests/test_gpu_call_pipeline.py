"""The grouped host pipeline behind ``encode_graphs`` and both ``encode_many`` roads (graphs
built on the device from whole records, windows built on the device): ramped groups of
micro-batches, one launch sequence and one copy back per group, per-record views cut at the end
— at the smallest shapes that have every group size, in every result-memory mode, against the
same road issued micro-batch by micro-batch."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#: max_batch_nodes → the group sizes the ramp gives for the micro-batches that limit makes
WHOLE_LIMITS = {200: [1, 1, 2, 2], 130: [1, 1, 2, 4, 1]}
SLICED_LIMITS = {150: [1, 1, 2, 2], 96: [1, 1, 2, 4, 1]}
WINDOW_OPTIONS = dict(keep_paired_neighbours=True, context_hops=2)
MODES = {"pinned": dict(pinned_outputs=True, independent_outputs=False),
         "pageable": dict(pinned_outputs=False, independent_outputs=False),
         "independent": dict(pinned_outputs=None, independent_outputs=True)}


def _whole_records():
    """24 hairpins of 30 to 53 nucleotides, each ending in unpaired bases."""
    from ginfinity_amd import RNA
    rng = np.random.default_rng(41)
    records = []
    for index in range(24):
        stem, loop, tail = 8 + index % 5, 4 + index % 7, 1 + (index * 5) % 9
        length = 2 * stem + loop + tail + 9
        sequence = "".join(rng.choice(list("ACGU"), size=length))
        structure = "." * 9 + "(" * stem + "." * loop + ")" * stem + "." * tail
        records.append(RNA(f"hairpin{index}", sequence, structure))
    return records


def _sliced_records():
    """The same molecules, three of four as a window that cuts through the stem (its paired
    neighbours and their neighbours come along as context rows), every fourth one whole."""
    from ginfinity_amd import RNA
    records = []
    for index, record in enumerate(_whole_records()):
        if index % 4 == 3:
            records.append(record)
        else:
            records.append(RNA(f"window{index}", record.sequence, record.structure,
                               3 + index % 4, 14 + index % 6))
    return records


def _rows(record) -> int:
    return record.end - record.start if record.sliced else record.length


def _sliced_shard():
    from ginfinity_amd import GraphBuilder
    return GraphBuilder(**WINDOW_OPTIONS).build_shard(_sliced_records())


def _roads(encoder):
    """road → (records, limits, call(max_batch_nodes) → per-record arrays)."""
    whole, sliced, shard = _whole_records(), _sliced_records(), _sliced_shard()
    return {
        "graphs": (sliced, SLICED_LIMITS,
                   lambda limit: encoder.encode_graphs(shard, max_batch_nodes=limit)),
        "whole": (whole, WHOLE_LIMITS,
                  lambda limit: encoder.encode_many(whole, max_batch_nodes=limit)),
        "sliced": (sliced, SLICED_LIMITS,
                   lambda limit: encoder.encode_many(sliced, max_batch_nodes=limit,
                                                     **WINDOW_OPTIONS)),
    }


def test_the_limits_give_the_groups_the_tests_are_about():
    """(No device needed, but it belongs to the cases below.)  The micro-batches the limits make
    of both lists fall into groups of 1, 1, 2, 2 and of 1, 1, 2, 4, 1, and the windows do
    draw context rows in, so that ``out_rows`` travels."""
    from ginfinity_amd import GraphBuilder
    from ginfinity_amd.api import MICROBATCH_GROUP, _groups, microbatch_bounds
    assert MICROBATCH_GROUP == 4
    whole, sliced = GraphBuilder().build_shard(_whole_records()), _sliced_shard()
    assert sliced.node_roles.any() and sliced.node_count > sum(map(_rows, _sliced_records()))
    for shard, limits in ((whole, WHOLE_LIMITS), (sliced, SLICED_LIMITS)):
        for limit, sizes in limits.items():
            bounds = microbatch_bounds(shard.lengths, shard.edge_counts, limit, 300_000)
            assert [len(group) for group in _groups(len(bounds), ramp=True)] == sizes, \
                (limit, len(bounds))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("road", ["graphs", "whole", "sliced"])
def test_groups_give_the_bytes_of_lone_micro_batches(gpu_encoder, road, mode, monkeypatch):
    from ginfinity_amd import api
    for name, value in MODES[mode].items():
        monkeypatch.setattr(gpu_encoder, name, value)
    records, limits, call = _roads(gpu_encoder)[road]
    for limit in limits:
        grouped = call(limit)
        assert len(grouped) == len(records)
        for array, record in zip(grouped, records):
            assert array.shape == (_rows(record), 128) and array.dtype == np.float16, \
                record.identifier
            assert array.flags.owndata == (mode == "independent")
        with monkeypatch.context() as patch:
            patch.setattr(api, "MICROBATCH_GROUP", 1)
            single = call(limit)
        assert len(single) == len(grouped)
        for a, b, record in zip(grouped, single, records):
            assert a.tobytes() == b.tobytes(), (limit, record.identifier)
        assert np.abs(np.concatenate(grouped).astype(np.float32)).max() > 0


@pytest.mark.parametrize("mode", list(MODES))
def test_a_refused_call_leaves_nothing_behind(gpu_encoder, mode, monkeypatch):
    """A record with unbalanced brackets (put past ``RNA``'s own validation) in the fifth
    micro-batch: ``encode_many`` names it, and the next call on the same encoder — same staging
    slots, same downloader — returns what it returned before."""
    from ginfinity_amd import RNA, GraphBuilder
    from ginfinity_amd.api import microbatch_bounds
    from ginfinity_amd.spec import GraphValidationError
    for name, value in MODES[mode].items():
        monkeypatch.setattr(gpu_encoder, name, value)
    roads = _roads(gpu_encoder)
    for road, options in (("whole", {}), ("sliced", WINDOW_OPTIONS)):
        records, limits, call = roads[road]
        limit = min(limits)                                    # nine micro-batches
        shard = GraphBuilder(**options).build_shard(records)
        bounds = microbatch_bounds(shard.lengths, shard.edge_counts, limit, 300_000)
        position = bounds[4][0] + 1
        victim = records[position]
        assert victim.structure.endswith(".")
        # a ')' nothing opened, at the end: same length, same number of '(' — the same
        # micro-batches, and every edge the offsets promise is still written
        window = (victim.start, victim.end) if victim.sliced else ()
        damaged = RNA("damaged", victim.sequence, victim.structure, *window)
        object.__setattr__(damaged, "structure", victim.structure[:-1] + ")")
        before = [array.tobytes() for array in call(limit)]
        broken = records[:position] + [damaged] + records[position + 1:]
        with pytest.raises(GraphValidationError, match="record 'damaged'"):
            gpu_encoder.encode_many(broken, max_batch_nodes=limit, **options)
        assert [array.tobytes() for array in call(limit)] == before
