"""The device window builder (gfy_window_select + gfy_window_emit: sliced records built on the
GPU without building any whole molecule) against the host builder bit for bit — itself pinned
to the genuine reference by tests/golden/windows.json (tests/test_window_text.py) — and the
``encode_many`` road that uses it against ``encode_graphs`` on host-built shards."""
from __future__ import annotations

import json

import numpy as np
import pytest

import window_cases as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_graph_build import _records as _whole_records   # noqa: E402  (the same molecules)

F16_TOL = 1e-3            # tests/test_gpu_parity.py::test_degenerate_and_sliced_graphs
ARRAYS = W.SHARD_ARRAYS
OPTIONS = W.OPTION_PAIRS + ((True, 50),)          # 50 hops: runs to an empty frontier


def _specs():
    from ginfinity_amd import GraphSpec
    return {"bundled": GraphSpec.bundled(),
            "three_state_no_skip": GraphSpec(struct_feature="B", positional=True,
                                             edge_dim=10, extra_edges=()),
            "flag_only": GraphSpec(struct_feature="A", positional=False, edge_dim=10,
                                   extra_edges=("skip2",))}


def _window_list(rng):
    """Every hand-made molecule of the unsliced build test under the windows that stress the
    64-bit words of the chosen map, unsliced records among them, and 300 random windows."""
    from ginfinity_amd import RNA
    from ginfinity_amd.graph import pair_table
    whole = _whole_records(rng)
    hand = sorted((r for r in whole if r.identifier.startswith("hand")),
                  key=lambda r: r.identifier)
    random_ones = [r for r in whole if r.identifier.startswith("rand")]
    out, serial = [], 0

    def add(record, start, end):
        nonlocal serial
        if 0 <= start < end <= record.length:
            serial += 1
            out.append(RNA(f"{record.identifier}#{serial}:{start}-{end}", record.sequence,
                           record.structure, start, end))

    for record in hand:
        length = record.length
        partners = pair_table(record.structure)
        out.append(record)                                            # unsliced
        add(record, 0, 1); add(record, length - 1, length); add(record, 0, length)
        for start, end in ((60, 70), (63, 65), (64, 128), (0, 64), (1, 64), (63, 64), (64, 65),
                           (120, 200), (127, 129), (1000, 1100), (2047, 2049), (2040, 2060),
                           (4032, 4096), (4095, 4096), (1, length - 1), (length // 2, length)):
            add(record, start, end)
        dots = np.flatnonzero(partners < 0)
        if dots.size:                      # a window of unpaired bases only: the longest run
            runs = np.split(dots, np.flatnonzero(np.diff(dots) > 1) + 1)
            run = max(runs, key=len)
            add(record, int(run[0]), int(run[-1]) + 1)
        opens = np.flatnonzero(partners > np.arange(length))
        if opens.size:                     # windows whose partners all lie inside them
            inner = int(opens[np.argmin(partners[opens] - opens)])
            add(record, inner, int(partners[inner]) + 1)
            outer = int(opens[0])
            add(record, outer, int(partners[outer]) + 1)
            add(record, outer, outer + 1)          # one paired base, its partner far away
    for index in range(300):
        record = random_ones[int(rng.integers(len(random_ones)))]
        start = int(rng.integers(0, record.length))
        end = int(rng.integers(start + 1, record.length + 1))
        if index % 7 == 0:
            out.append(RNA(f"whole{index}", record.sequence, record.structure))
        add(record, start, end)
    assert sum(not r.sliced for r in out) >= 12 and len(out) > 500
    return out


def _assert_same_shard(got, want):
    """All seven arrays: dtype, shape and bytes; the offsets make it every record, whole."""
    for name in ARRAYS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype, name
        assert a.shape == b.shape, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            where = np.flatnonzero(np.ravel(a != b))[:8]
            raise AssertionError((name, where.tolist(), np.ravel(a)[where].tolist(),
                                  np.ravel(b)[where].tolist()))
    assert got.identifiers == want.identifiers and got.sequences == want.sequences
    assert got.structures == want.structures


@pytest.mark.parametrize("keep,hops", OPTIONS)
@pytest.mark.parametrize("variant", ["bundled", "three_state_no_skip", "flag_only"])
def test_device_windows_equal_the_host_builder(gpu_encoder, variant, keep, hops):
    from ginfinity_amd import GraphBuilder
    spec = _specs()[variant]
    records = _window_list(np.random.default_rng(23))
    want = GraphBuilder(spec, keep_paired_neighbours=keep, context_hops=hops).build_shard(records)
    got = gpu_encoder.build_graphs_device(records, keep_paired_neighbours=keep,
                                          context_hops=hops, spec=spec)
    _assert_same_shard(got, want)


def test_unsliced_records_in_a_mixed_list_come_out_as_gfy_build_graphs_writes_them(gpu_encoder):
    from ginfinity_amd import RNA, GraphBuilder
    whole = [r for r in _whole_records(np.random.default_rng(3))][:80]
    want = GraphBuilder().build_shard(whole)
    # one sliced record at the end sends the list down the window road; cut it off again
    mixed = whole + [RNA("tail", "ACGUACGU", "((....))", 2, 5)]
    got = gpu_encoder.build_graphs_device(mixed, keep_paired_neighbours=True, context_hops=3)
    _assert_same_shard(got.slice(0, len(whole)), want)


def test_device_windows_reproduce_the_reference_s_hashes(gpu_encoder, golden, rouskin_records):
    from ginfinity_amd import RNA
    fixture = golden("windows.json")
    windows = W.seeded_windows(rouskin_records, RNA)
    for keep, hops in W.OPTION_PAIRS:
        want = fixture["options"][f"keep={int(keep)},hops={hops}"]
        shard = gpu_encoder.build_graphs_device(windows, keep_paired_neighbours=keep,
                                                context_hops=hops)
        assert (int(shard.node_ptr[-1]), int(shard.edge_ptr[-1])) == (want["nodes"],
                                                                     want["edges"])
        assert W.shard_digest(shard) == want["arrays"], (keep, hops)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("keep,hops", [(False, 1), (True, 1), (True, 3)])
def test_encode_many_on_device_built_windows_equals_encode_graphs(gpu_encoder, rouskin_records,
                                                                  dtype, keep, hops):
    from ginfinity_amd import RNA, GraphBuilder
    from ginfinity_amd.api import MICROBATCH_GROUP, microbatch_bounds
    records = W.seeded_windows(rouskin_records, RNA, seed=77, count=260)
    records[5:5] = rouskin_records[:6]                     # unsliced ones among them
    shard = GraphBuilder(keep_paired_neighbours=keep, context_hops=hops).build_shard(records)
    limits = dict(max_batch_nodes=1000, max_batch_edges=5000)
    bounds = microbatch_bounds(np.diff(shard.node_ptr), np.diff(shard.edge_ptr), 1000, 5000)
    assert len(bounds) > 4 + MICROBATCH_GROUP              # the ramp and more than one group
    want = gpu_encoder.encode_graphs(shard, embedding_dtype=dtype, **limits)
    got = gpu_encoder.encode_many(records, keep_paired_neighbours=keep, context_hops=hops,
                                  embedding_dtype=dtype, **limits)
    assert len(got) == len(want) == len(records)
    for a, b, record in zip(got, want, records):
        rows = record.end - record.start if record.sliced else record.length
        assert a.dtype == b.dtype == np.dtype(dtype) and a.shape == b.shape == (rows, 128)
        assert a.tobytes() == b.tobytes(), record.identifier
    # one micro-batch (the default limits) gives the same rows
    default = gpu_encoder.encode_many(records, keep_paired_neighbours=keep, context_hops=hops,
                                      embedding_dtype=dtype)
    whole = gpu_encoder.encode_graphs(shard, embedding_dtype=dtype)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(default, whole))


def test_the_stem_record_matches_its_recorded_reference_rows(gpu_encoder, golden):
    from ginfinity_amd import RNA
    s = golden("sliced.npz")
    record = RNA("stem", "GGGAAACCCUUUUGGG", "......(((....)))", start=9, end=16)
    for hops in (1, 2, 3):
        out = gpu_encoder.encode_many([record], keep_paired_neighbours=True,
                                      context_hops=hops)[0]
        assert out.shape == (7, 128) and out.dtype == np.float16
        worst = np.abs(out.astype(np.float64) - s[f"hops{hops}.out.m16"].astype(np.float64)).max()
        assert worst <= F16_TOL, (hops, worst)
        shard = gpu_encoder.build_graphs_device([record], keep_paired_neighbours=True,
                                                context_hops=hops)
        for name in ("node_features", "edge_index", "edge_types", "residue_index", "node_roles"):
            np.testing.assert_array_equal(getattr(shard, name), s[f"hops{hops}.{name}"])
    plain = gpu_encoder.encode_many([record])[0]
    assert np.abs(plain.astype(np.float64)
                  - s["nokeep.out.m16"].astype(np.float64)).max() <= F16_TOL


def test_limits_apply_to_the_sliced_counts(gpu_encoder):
    from ginfinity_amd import RNA
    sequence = "G" * 300 + "A" * 100 + "C" * 300
    structure = "(" * 300 + "." * 100 + ")" * 300
    records = [RNA("left", sequence, structure, 0, 120), RNA("loop", sequence, structure, 310, 390)]
    # off: 120 and 80 nodes; on: the left window draws in its 120 partners
    assert [len(a) for a in gpu_encoder.encode_many(records, max_batch_nodes=120)] == [120, 80]
    with pytest.raises(ValueError, match="max_batch_nodes is smaller than the longest graph"):
        gpu_encoder.encode_many(records, max_batch_nodes=119)
    with pytest.raises(ValueError, match="max_batch_nodes is smaller than the longest graph"):
        gpu_encoder.encode_many(records, max_batch_nodes=239, keep_paired_neighbours=True)
    out = gpu_encoder.encode_many(records, max_batch_nodes=240, keep_paired_neighbours=True)
    assert [len(a) for a in out] == [120, 80]
    with pytest.raises(ValueError, match="max_batch_edges is smaller than the largest graph"):
        gpu_encoder.encode_many(records, max_batch_edges=100)
    with pytest.raises(ValueError, match="limits must be positive"):
        gpu_encoder.encode_many(records, max_batch_nodes=0)
    with pytest.raises(ValueError, match="context_hops"):
        gpu_encoder.encode_many(records, keep_paired_neighbours=True, context_hops=0)


def test_a_corrupted_text_is_reported_by_name_not_built(gpu_encoder):
    """Text that RNA() would have refused, put into records past its validation: the device
    reports the first record that uses it and writes nothing out of bounds."""
    from ginfinity_amd import RNA
    from ginfinity_amd.graph import GraphValidationError
    good = RNA("good", "GGGAAACCC", "(((...)))", 2, 7)
    for field, text in (("structure", "((....)))"), ("structure", "(((...))("),
                        ("structure", "(((.x.)))"), ("sequence", "GGGANACCC")):
        damaged = RNA("damaged", "GGGAAACCC", "(((...)))", 1, 4)
        object.__setattr__(damaged, field, text)
        later = RNA("later", "GGGAAACCC", "(((...)))", 0, 3)
        object.__setattr__(later, field, text)
        with pytest.raises(GraphValidationError, match="record 'damaged'"):
            gpu_encoder.encode_many([good, RNA("whole", "ACGU", "(..)"), damaged, later],
                                    keep_paired_neighbours=True, context_hops=2)
    # a window outside its molecule (RNA() refuses it)
    outside = RNA("outside", "GGGAAACCC", "(((...)))", 1, 4)
    object.__setattr__(outside, "end", 12)
    with pytest.raises(GraphValidationError, match="record 'outside'"):
        gpu_encoder.encode_many([good, outside])
    assert len(gpu_encoder.encode_many([good])[0]) == 5          # the encoder is still usable


def test_engine_entry_points_range_check_their_inputs(gpu_encoder):
    """The C ABI by itself: a bad molecule index, a window outside its molecule and pointers
    that disagree with the counts come back through first_invalid."""
    from ginfinity_amd import RNA
    from ginfinity_amd.graph import window_text
    engine, device = gpu_encoder._engine, gpu_encoder._engine.device
    records = [RNA("a", "GGGAAACCC", "(((...)))", 2, 7), RNA("b", "ACGU", "(..)"),
               RNA("c", "GGGAAACCC", "(((...)))", 0, 3)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731

    def select(text):
        return engine.window_select(up(text.bases), up(text.marks), up(text.mol_ptr),
                                    up(text.molecule), up(text.start), up(text.end),
                                    keep_paired_neighbours=True, context_hops=2, skip2=True)

    text = window_text(records, gpu_encoder.graph_spec)
    windows = select(text)
    assert int(windows.first_invalid.item()) == -1
    counts = windows.counts.cpu().numpy()
    assert (counts[:, 0] > 0).all()
    for name, index, value, expect in (("molecule", 1, 2, 1), ("molecule", 0, -1, 0),
                                       ("end", 2, 10, 2), ("start", 1, -1, 1),
                                       ("start", 0, 7, 0)):
        broken = window_text(records, gpu_encoder.graph_spec)
        getattr(broken, name)[index] = value
        verdict = select(broken)
        assert int(verdict.first_invalid.item()) == expect, (name, index)
        assert verdict.counts.cpu().numpy()[expect].tolist() == [0, 0]
    node_ptr = np.concatenate(([0], np.cumsum(counts[:, 0]))).astype(np.int64)
    edge_ptr = np.concatenate(([0], np.cumsum(counts[:, 1]))).astype(np.int64)
    positional = up(text.positional())

    def emit(nodes, edges):
        return engine.window_emit(windows, 0, up(nodes), up(edges), None, positional,
                                  int(node_ptr[-1]), int(edge_ptr[-1]), 0, struct_states=1)

    assert int(emit(node_ptr, edge_ptr)[-1].item()) == -1
    wrong = node_ptr.copy(); wrong[2:] += 1                 # record 1 claims one node too many
    assert int(emit(wrong, edge_ptr)[-1].item()) == 1
    wrong = edge_ptr.copy(); wrong[1] -= 2                  # record 0 one pair short
    assert int(emit(node_ptr, wrong)[-1].item()) == 0
    with pytest.raises(Exception, match="workspace"):
        small = type(windows)(**{**windows.__dict__, "workspace": windows.workspace[:64]})
        engine.window_emit(small, 0, up(node_ptr), up(edge_ptr), None, positional,
                           int(node_ptr[-1]), int(edge_ptr[-1]), 0, struct_states=1)


def test_a_list_without_sliced_records_keeps_its_road(gpu_encoder, rouskin_records, monkeypatch):
    from ginfinity_amd import RNA
    from ginfinity_amd.engine import DeviceEncoder
    calls = {"build_graphs": 0, "window_select": 0, "window_emit": 0}
    for name in calls:
        original = getattr(DeviceEncoder, name)

        def counted(self, *args, _name=name, _original=original, **kwargs):
            calls[_name] += 1
            return _original(self, *args, **kwargs)
        monkeypatch.setattr(DeviceEncoder, name, counted)
    whole = rouskin_records[:40]
    gpu_encoder.encode_many(whole, keep_paired_neighbours=True, context_hops=3)
    assert calls == {"build_graphs": 1, "window_select": 0, "window_emit": 0}
    window = RNA("w", whole[0].sequence, whole[0].structure, 3, 30)
    gpu_encoder.encode_many(whole + [window])
    assert calls == {"build_graphs": 1, "window_select": 1, "window_emit": 1}
    gpu_encoder.encode(window, keep_paired_neighbours=True)
    assert calls == {"build_graphs": 1, "window_select": 2, "window_emit": 2}


def test_cli_embed_on_a_windowed_table_takes_the_device_road(tmp_path, capsys, rouskin_records,
                                                             monkeypatch):
    """``ginfinity embed --device cuda`` on a table with start / end columns: same members and
    manifest entries as ``--device cpu`` (different arithmetic: values within 1e-3), through
    gfy_window_select / gfy_window_emit and not through the host builder."""
    from ginfinity_amd import cli
    from ginfinity_amd.engine import DeviceEncoder
    from ginfinity_amd.graph import GraphBuilder
    rows = ["transcript_id\tsequence\tsecondary_structure\tstart\tend"]
    rng = np.random.default_rng(9)
    for index, record in enumerate(rouskin_records[:60]):
        if index % 5 == 4:
            rows.append(f"{record.identifier}\t{record.sequence}\t{record.structure}\t\t")
            continue
        start = int(rng.integers(0, record.length))
        end = int(rng.integers(start + 1, record.length + 1))
        rows.append(f"{record.identifier}\t{record.sequence}\t{record.structure}\t{start}\t{end}")
    table = tmp_path / "windowed.tsv"
    table.write_text("\n".join(rows) + "\n")
    flags = ["--keep-paired-neighbours", "--context-hops", "2"]
    on_cpu = tmp_path / "cpu.npz"
    assert cli.main(["embed", "--input", str(table), "--output", str(on_cpu), *flags]) == 0
    selects = []
    original = DeviceEncoder.window_select
    monkeypatch.setattr(DeviceEncoder, "window_select",
                        lambda self, *a, **k: selects.append(1) or original(self, *a, **k))

    def refuse(self, records):
        raise AssertionError("the host builder ran on the cuda road")
    monkeypatch.setattr(GraphBuilder, "build_shard", refuse)
    on_gpu = tmp_path / "gpu.npz"
    assert cli.main(["embed", "--input", str(table), "--output", str(on_gpu), *flags,
                     "--device", "cuda", "--allow-nondeterministic-cuda"]) == 0
    capsys.readouterr()
    assert selects
    with np.load(on_gpu) as ours, np.load(on_cpu) as theirs:
        assert list(ours.files) == list(theirs.files) and len(ours.files) == 60
        for key in theirs.files:
            assert ours[key].shape == theirs[key].shape and ours[key].dtype == theirs[key].dtype
            worst = np.abs(ours[key].astype(np.float64) - theirs[key].astype(np.float64)).max()
            assert worst <= 1e-3, (key, worst)
    mine = json.loads(on_gpu.with_suffix(".manifest.json").read_text())
    reference = json.loads(on_cpu.with_suffix(".manifest.json").read_text())
    assert set(mine) == set(reference) and mine["device"] == "cuda"
    assert mine["status"] == reference["status"] == "complete"
    for a, b in zip(mine["records"], reference["records"]):
        assert ({k: a[k] for k in a if "sha256" not in k}
                == {k: b[k] for k in b if "sha256" not in k})
