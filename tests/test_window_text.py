"""Host side of the device window builder: ``window_text`` (what crosses PCIe for a list with
sliced records) and the fixture tests/golden/windows.json, recorded from the genuine reference
(tests/golden/make_windows_golden.py), which the host builder must reproduce — that pins the
expected side of tests/test_gpu_windows.py to the reference.  CPU only."""
from __future__ import annotations

import numpy as np
import pytest

import window_cases as W
from ginfinity_amd import RNA, GraphBuilder, GraphSpec
from ginfinity_amd.graph import GraphValidationError, window_text


def test_windows_of_one_molecule_share_one_entry():
    sequence, structure = "GGGAAACCCUUUUGGG", "......(((....)))"
    records = [RNA("t:0-4", sequence, structure, 0, 4), RNA("other", "ACGU", "(..)"),
               RNA("t:9-16", sequence, structure, 9, 16), RNA("whole", sequence, structure),
               RNA("same text, other name", "ACGU", "(..)", 1, 3),
               RNA("same sequence, other structure", "ACGU", "....")]
    text = window_text(records, GraphSpec.bundled())
    assert text.molecule_count == 3 and text.record_count == 6
    assert text.mol_ptr.tolist() == [0, 16, 20, 24] and text.mol_ptr.dtype == np.int64
    assert text.molecule.tolist() == [0, 1, 0, 0, 1, 2]          # order of the records kept
    assert text.start.tolist() == [0, 0, 9, 0, 1, 0]
    assert text.end.tolist() == [4, 4, 16, 16, 3, 4]             # unsliced: [0, L)
    assert text.molecule.dtype == text.start.dtype == text.end.dtype == np.int32
    assert text.bases.tobytes() == (sequence + "ACGU" + "ACGU").encode()
    assert text.marks.tobytes() == (structure + "(..)" + "....").encode()
    assert text.core_counts.tolist() == [4, 4, 7, 16, 2, 4]


def test_positional_columns_are_the_whole_molecule_s():
    spec = GraphSpec.bundled()
    records = [RNA("a", "GGGAAACCC", "(((...)))", 2, 5), RNA("b", "AC", "..")]
    columns = window_text(records, spec).positional()
    whole = GraphBuilder(spec).build_shard([RNA("a", "GGGAAACCC", "(((...)))"), records[1]])
    assert columns.dtype == np.float32 and columns.shape == (11, 2)
    assert columns.tobytes() == np.ascontiguousarray(whole.node_features[:, 5:7]).tobytes()
    plain = GraphSpec(struct_feature="A", positional=False, edge_dim=10, extra_edges=("skip2",))
    assert window_text(records, plain).positional() is None


def test_window_text_refuses_what_a_shard_refuses():
    with pytest.raises(GraphValidationError, match="cannot be empty"):
        window_text([], GraphSpec.bundled())
    twice = [RNA("a", "ACGU", "(..)", 0, 2), RNA("a", "ACGU", "(..)", 1, 3)]
    with pytest.raises(GraphValidationError, match="duplicate identifiers"):
        window_text(twice, GraphSpec.bundled())


def test_host_builder_reproduces_the_reference_s_window_hashes(golden, rouskin_records):
    fixture = golden("windows.json")
    assert (fixture["seed"], fixture["windows"]) == (W.GOLDEN_SEED, W.GOLDEN_WINDOWS)
    windows = W.seeded_windows(rouskin_records, RNA)
    assert len(windows) == fixture["windows"] and all(record.sliced for record in windows)
    assert len(fixture["options"]) == len(W.OPTION_PAIRS)
    for keep, hops in W.OPTION_PAIRS:
        want = fixture["options"][f"keep={int(keep)},hops={hops}"]
        shard = GraphBuilder(keep_paired_neighbours=keep, context_hops=hops).build_shard(windows)
        assert (int(shard.node_ptr[-1]), int(shard.edge_ptr[-1])) == (want["nodes"],
                                                                     want["edges"])
        assert W.shard_digest(shard) == want["arrays"], (keep, hops)
