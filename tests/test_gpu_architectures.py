"""The GPU encoder on every kind of architecture the library accepts (tests/arch_models.py):
one layer (the fused head in the FIRST layer launch, on the set-up's spent scratch), eight
layers (kMaxLayers), no residual (every RES=false instantiation), 4 / 12 / 13 / 16 edge types
(the windowed kernel's plan-head slots next to live table rows; its fallback above 12 types; the
-inf idle row next to a full table) and structure feature B without positions — loaded through
the public ``Ginfinity.load("cuda", model_dir=...)`` with seeded random weights.

Checked against what the genuine reference returned for the same model directories
(tests/golden/architectures.npz), against the oracle, and path against path byte for byte: every
layer kernel, fused and stand-alone head, the three set-up paths, one shard against a batch that
takes the multi-round kernels, and the output dtypes."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import arch_models as A
from ginfinity_amd import _native as native

pytestmark = pytest.mark.gpu

F16_TOL = 1e-3
F32_TOL = 1e-6
NAMES = list(A.VARIANTS)


def _maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def check_margins(name, got, want, layers):
    """test_gpu_parity._record_margin's regression bounds against the reference's own rows:
    max 1.5 ulp of [0.25, 0.5), p99.9 one ulp, mean, share of identical elements — measured on
    four layers.  Every layer adds its own one-ulp flips (the MFMA's summation order against the
    reference's BLAS, test_hidden_state_after_every_layer_against_the_oracle), so the eight-layer
    model gets a p99.9, mean and share of its own: measured 2.4-2.7e-4, 5.7-6.0e-5 and 0.26-0.27
    (1 to 3 layers: at most 2.3e-4, 1.5e-5, at least 0.70)."""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    same = float(np.mean(got.view(np.uint16) == want.view(np.uint16)))
    print(f"{name}: max {diff.max():.2e} p99.9 {np.quantile(diff, 0.999):.2e} "
          f"mean {diff.mean():.2e} identical {same:.3f}")
    p999_bound, mean_bound, same_bound = (2.6e-4, 5.5e-5, 0.29) if layers <= 4 else \
        (3.7e-4, 7e-5, 0.22)
    assert diff.max() <= 7.4e-4, (name, diff.max())
    assert np.quantile(diff, 0.999) <= p999_bound, (name, np.quantile(diff, 0.999))
    assert diff.mean() <= mean_bound, (name, diff.mean())
    assert same >= same_bound, (name, same)


@pytest.fixture(scope="module")
def arch(golden):
    return golden("architectures.npz")


@pytest.fixture(scope="module")
def encoders(tmp_path_factory):
    """name -> (fp16-model Ginfinity, fp32-model Ginfinity) on cuda:0."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ginfinity_amd import Ginfinity
    root = tmp_path_factory.mktemp("architectures")
    loaded = {}
    for name in NAMES:
        directory = A.write_model_dir(root / name, *A.variant(name))
        loaded[name] = tuple(Ginfinity.load("cuda", allow_nondeterministic_cuda=True,
                                            model_dir=directory, full_precision=full)
                             for full in (False, True))
    yield loaded
    for pair in loaded.values():
        for encoder in pair:
            encoder._engine.close()


@pytest.fixture(scope="module")
def inputs(rouskin_records):
    """name -> (rouskin records, their graphs under the architecture's spec, arbitrary shard)."""
    from ginfinity_amd import GraphBuilder
    records = rouskin_records[:A.ROUSKIN_RECORDS]
    out = {}
    for name in NAMES:
        config, _seed = A.variant(name)
        out[name] = (records, GraphBuilder(A.spec_of(config)).build_shard(records),
                     A.arbitrary_input(config))
    return out


def _oracle_weights(name):
    from oracle import gine_numpy as G
    from ginfinity_amd.weights import random_state
    config, seed = A.variant(name)
    return G.Weights.from_state_dict(random_state(config, seed), layers=config.layers,
                                     residual=config.residual)


def _device(engine, shard, records=False):
    from ginfinity_amd.engine import attach_records
    dev = engine.device
    rows, kept = None, None
    if shard.node_roles.any():
        core = shard.node_roles == 0
        kept = int(core.sum())
        table = np.cumsum(core, dtype=np.int32) - np.int32(1)
        table[~core] = -1
        rows = torch.from_numpy(table).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(shard.node_features)).to(dev)
    ei = torch.from_numpy(np.ascontiguousarray(shard.edge_index)).to(dev)
    et = torch.from_numpy(np.ascontiguousarray(shard.edge_types)).to(dev)
    if records:
        attach_records(ei, torch.from_numpy(shard.node_ptr.astype(np.int64)).to(dev),
                       torch.from_numpy(shard.edge_ptr.astype(np.int64)).to(dev))
    return x, ei, et, rows, kept


def _small_batches(shard):
    """Limits that put one or two records in a micro-batch: several micro-batches, issued in
    groups (``gfy_encode_coo_batch`` with record boundaries)."""
    return dict(max_batch_nodes=max(shard.lengths) + 1, max_batch_edges=max(shard.edge_counts) + 1)


# ---- against the reference ------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_public_paths_match_the_reference_fixture(encoders, inputs, arch, name):
    """``encode_many`` (graphs built on the device with the architecture's spec),
    ``encode_graphs`` in one micro-batch and in grouped small micro-batches (the record-range
    set-up), fp16 and fp32 model, against the reference's rows; every row against the oracle."""
    from oracle import gine_numpy as G
    enc16, enc32 = encoders[name]
    config, _seed = A.variant(name)
    records, graphs, arbitrary = inputs[name]
    rs, ars = int(arch["rouskin.stride"]), int(arch["arbitrary.stride"])
    assert enc16.graph_spec.sha256 == graphs.spec.sha256
    many = enc16.encode_many(records)
    assert [o.shape[0] for o in many] == [r.length for r in records]
    many = np.concatenate(many)
    whole = np.concatenate(enc16.encode_graphs(graphs))
    grouped = np.concatenate(enc16.encode_graphs(graphs, **_small_batches(graphs)))
    assert many.tobytes() == whole.tobytes() == grouped.tobytes()
    want = arch[f"{name}.rouskin.m16.float16"]
    assert _maxabs(many[::rs], want) <= F16_TOL
    check_margins(f"{name} rouskin", many[::rs], want, config.layers)
    weights = _oracle_weights(name)
    assert _maxabs(many, G.encode(weights, graphs.node_features, graphs.edge_index,
                                  graphs.edge_types)) <= F16_TOL
    got = np.concatenate(enc16.encode_graphs(arbitrary))
    grouped = np.concatenate(enc16.encode_graphs(arbitrary, **_small_batches(arbitrary)))
    assert got.tobytes() == grouped.tobytes()
    want = arch[f"{name}.arbitrary.m16.float16"]
    assert _maxabs(got[::ars], want) <= F16_TOL
    check_margins(f"{name} arbitrary", got[::ars], want, config.layers)
    core = arbitrary.node_roles == 0
    assert _maxabs(got, G.encode(weights, arbitrary.node_features, arbitrary.edge_index,
                                 arbitrary.edge_types)[core]) <= F16_TOL
    # fp32 model, fp32 output
    for label, rows in (
            ("rouskin", np.concatenate(enc32.encode_many(records, embedding_dtype="float32"))),
            ("arbitrary", np.concatenate(enc32.encode_graphs(arbitrary,
                                                             embedding_dtype="float32")))):
        stride = rs if label == "rouskin" else ars
        assert rows.dtype == np.float32
        worst = _maxabs(rows[::stride], arch[f"{name}.{label}.m32.float32"])
        print(f"{name} fp32 model {label}: {worst:.2e}")
        assert worst <= F32_TOL, (label, worst)
    grouped32 = np.concatenate(enc32.encode_graphs(graphs, **_small_batches(graphs),
                                                   embedding_dtype="float32"))
    assert _maxabs(grouped32[::rs], arch[f"{name}.rouskin.m32.float32"]) <= F32_TOL


# ---- path against path ----------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_every_kernel_head_and_set_up_gives_the_same_bytes(encoders, inputs, name):
    """Shard by shard, the bytes of ``gfy_encode_coo`` on the shard alone (default kernel) from:
    a batch on every layer kernel, with the counting set-up and with record boundaries (the
    record-range set-up), the caller's CSR (``gfy_encode``), and the stand-alone head behind the
    multi-round kernels."""
    engine = encoders[name][0]._engine
    _records, graphs, arbitrary = inputs[name]
    shards = [graphs, arbitrary, graphs.slice(3, 4)]
    want = []
    for shard in shards:
        x, ei, et, rows, kept = _device(engine, shard)
        want.append(engine.encode_coo(x, ei, et, out_rows=rows, n_out=kept).cpu().numpy())
        csr = engine.build_csr(ei, et, shard.node_count)
        via_csr = engine.encode(x, csr, out_rows=rows, n_out=kept).cpu().numpy()
        assert via_csr.tobytes() == want[-1].tobytes(), name
    try:
        for kernel in (-1, 1, 3, 4, 5):
            engine.set_option(native.GFY_OPT_LAYER_KERNEL, kernel)
            for records in (False, True):
                got = engine.encode_coo_batch([_device(engine, s, records) for s in shards])
                for shard, a, b in zip(shards, got, want):
                    assert a.cpu().numpy().tobytes() == b.tobytes(), (kernel, records,
                                                                      shard.node_count)
            if kernel in (3, 4, 5):
                engine.set_option(native.GFY_OPT_SEPARATE_HEAD, 1)
                got = engine.encode_coo_batch([_device(engine, s) for s in shards])
                engine.set_option(native.GFY_OPT_SEPARATE_HEAD, 0)
                for a, b in zip(got, want):
                    assert a.cpu().numpy().tobytes() == b.tobytes(), (kernel, "separate head")
    finally:
        engine.set_option(native.GFY_OPT_SEPARATE_HEAD, 0)
        engine.set_option(native.GFY_OPT_LAYER_KERNEL, -1)


@pytest.mark.parametrize("name", NAMES)
def test_fused_head_against_the_stand_alone_head_and_output_dtypes(encoders, inputs, name):
    """The one-round kernel's fused head (for ``layers=1`` inside the first launch) against the
    stand-alone head: last-bit flips of o only, as for the bundled model
    (test_gpu_parity.test_fused_head_equals_standalone_head).  The stand-alone head writes the
    float64 quotient rounded ONCE: its f16 and f32 outputs are its f64 output rounded, for both
    model dtypes."""
    enc16, enc32 = encoders[name]
    engine = enc16._engine
    _records, _graphs, arbitrary = inputs[name]
    x, ei, et, rows, kept = _device(engine, arbitrary)
    out = {}
    try:
        engine.set_option(native.GFY_OPT_LAYER_KERNEL, 1)
        fused = engine.encode_coo(x, ei, et, out_rows=rows, n_out=kept).cpu().numpy()
        assert engine.last_layer_kernel() == 1
        engine.set_option(native.GFY_OPT_SEPARATE_HEAD, 1)
        for dtype in (torch.float16, torch.float32, torch.float64):
            out[dtype] = engine.encode_coo(x, ei, et, out_rows=rows, n_out=kept,
                                           out_dtype=dtype).cpu().numpy()
    finally:
        engine.set_option(native.GFY_OPT_SEPARATE_HEAD, 0)
        engine.set_option(native.GFY_OPT_LAYER_KERNEL, -1)
    alone = out[torch.float16]
    flips = float(np.mean(fused.view(np.uint16) != alone.view(np.uint16)))
    print(f"{name}: fused vs stand-alone head {flips:.2e} of elements, max {_maxabs(fused, alone):.2e}")
    assert flips < 2e-3 and _maxabs(fused, alone) <= 2.5e-4
    wide = out[torch.float64]
    assert wide.astype(np.float16).tobytes() == alone.tobytes()
    assert wide.astype(np.float32).tobytes() == out[torch.float32].tobytes()
    np.testing.assert_allclose(np.linalg.norm(wide, axis=1), 1.0, atol=1e-12)
    engine32 = enc32._engine
    x, ei, et, rows, kept = _device(engine32, arbitrary)
    wide = engine32.encode_coo(x, ei, et, out_rows=rows, n_out=kept,
                               out_dtype=torch.float64).cpu().numpy()
    narrow = engine32.encode_coo(x, ei, et, out_rows=rows, n_out=kept,
                                 out_dtype=torch.float32).cpu().numpy()
    assert wide.astype(np.float32).tobytes() == narrow.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_on_the_multi_round_kernels_equals_single_shards(encoders, name):
    """Three 40,000-node interchange shards in one batch give every CU more than one round of
    tiles: the default picks the windowed rounds (<= 12 edge types) or the persistent rounds
    (13..16) — each shard's bytes equal the one-round kernel's on that shard alone."""
    from ginfinity_amd import synthetic
    engine = encoders[name][0]._engine
    config, _seed = A.variant(name)
    shards = [synthetic.arbitrary_shard(40 + i, nodes=40_000, edges=200_000, records=6,
                                        spec=A.spec_of(config)) for i in range(3)]
    want = []
    for shard in shards:
        x, ei, et, rows, kept = _device(engine, shard)
        want.append(engine.encode_coo(x, ei, et, out_rows=rows, n_out=kept).cpu().numpy())
        assert engine.last_layer_kernel() == 1
    got = engine.encode_coo_batch([_device(engine, s, True) for s in shards])
    assert engine.last_layer_kernel() == (4 if config.edge_dim <= 12 else 3)
    for a, b in zip(got, want):
        assert a.cpu().numpy().tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_forced_windowed_kernels_report_their_fallback(encoders, inputs, name):
    """Kernels 4 and 5 keep their plan-head slots in table rows 12..15: with more than 12 edge
    types they cannot run, and a forced 4 or 5 runs the persistent rounds (3) — reported by
    ``last_layer_kernel``, never silently; at 12 types and below they run as asked."""
    engine = encoders[name][0]._engine
    config, _seed = A.variant(name)
    _records, graphs, _arbitrary = inputs[name]
    try:
        for kernel in (4, 5):
            engine.set_option(native.GFY_OPT_LAYER_KERNEL, kernel)
            engine.encode_coo_batch([_device(engine, graphs)])
            torch.cuda.synchronize()
            assert engine.last_layer_kernel() == (kernel if config.edge_dim <= 12 else 3), kernel
    finally:
        engine.set_option(native.GFY_OPT_LAYER_KERNEL, -1)


# ---- per-layer state, taps, timing ----------------------------------------------------------

@pytest.mark.parametrize("name", ["v1", "v2"])
def test_hidden_state_after_every_layer_against_the_oracle(encoders, inputs, name):
    """``gfy_encode_hidden`` at every stage 0..layers (one layer without residual; eight with)
    against the oracle's per-layer trace: the input Linear bit for bit; behind it only the
    MFMA's summation order differs from the oracle's — one-ulp flips of u / w that the norms pass
    on and the layers compound: no element further off than two ulps of the stage's largest
    binade (three after eight layers: measured 2.5), and the share of differing elements within what was measured (v1: 0.006; v2: 0.003,
    0.030, 0.10, 0.22, 0.34, 0.43, 0.51, 0.57 after layers 1..8) + 25 %, as
    test_gpu_parity.test_hidden_stages_match_oracle bounds the bundled model."""
    from oracle import gine_numpy as G
    engine = encoders[name][0]._engine
    config, _seed = A.variant(name)
    _records, graphs, _arbitrary = inputs[name]
    shares = {"v1": (0.0075,),
              "v2": (0.004, 0.038, 0.13, 0.28, 0.43, 0.54, 0.64, 0.72)}[name]
    assert len(shares) == config.layers
    trace = {}
    G.forward_f16(_oracle_weights(name).half(), graphs.node_features, graphs.edge_index,
                  graphs.edge_types, trace)
    x = torch.from_numpy(graphs.node_features).to(engine.device)
    ei = torch.from_numpy(graphs.edge_index).to(engine.device)
    et = torch.from_numpy(graphs.edge_types).to(engine.device)
    csr = engine.build_csr(ei, et, graphs.node_count)
    h0 = engine.hidden(x, csr, 0).cpu().numpy()
    assert h0.tobytes() == trace["h0"].tobytes()
    for stage in range(1, config.layers + 1):
        got = engine.hidden(x, csr, stage).cpu().numpy()
        want = trace[f"l{stage - 1}.h"]
        share = float(np.mean(got.view(np.uint16) != want.view(np.uint16)))
        limit = (2 if stage < 8 else 3) * float(np.spacing(np.abs(want).max()))
        print(f"{name} stage {stage}: {share:.4f} differ, max|d| {_maxabs(got, want):.4f} "
              f"(limit {limit:.4f})")
        assert np.isfinite(got.astype(np.float32)).all()
        assert share <= shares[stage - 1], (stage, share)
        assert _maxabs(got, want) <= limit, (stage, _maxabs(got, want), limit)


def test_taps_need_the_residual_architecture_and_timing_covers_every_layer(encoders, inputs):
    """include/gfy.h: ``gfy_debug_layer`` has tap instantiations of the residual architecture
    only — GFY_ERR_UNSUPPORTED otherwise; ``gfy_encoder_get_timing`` reports set-up, every layer
    and the stand-alone head: layers + 2 entries (8 layers: the event array's full length)."""
    lib = native.library()
    for name in NAMES:
        engine = encoders[name][0]._engine
        config, _seed = A.variant(name)
        _records, graphs, _arbitrary = inputs[name]
        x = torch.from_numpy(graphs.node_features).to(engine.device)
        ei = torch.from_numpy(graphs.edge_index).to(engine.device)
        et = torch.from_numpy(graphs.edge_types).to(engine.device)
        csr = engine.build_csr(ei, et, graphs.node_count)
        hidden = engine.hidden(x, csr, 0)
        if not config.residual:
            out = torch.empty((graphs.node_count, 128), dtype=torch.float16, device=engine.device)
            need = lib.gfy_debug_layer_workspace_bytes(engine._handle, graphs.node_count,
                                                       graphs.edge_count)
            scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=engine.device)
            status = lib.gfy_debug_layer(engine._handle, 0, hidden.data_ptr(),
                                         csr.row_ptr.data_ptr(), csr.col.data_ptr(),
                                         csr.typ.data_ptr(), graphs.node_count, graphs.edge_count,
                                         native.GFY_TAP_H, out.data_ptr(), scratch.data_ptr(),
                                         scratch.numel(), None)
            assert status == native.GFY_ERR_UNSUPPORTED, name
            assert b"residual" in lib.gfy_last_error()
            with pytest.raises(native.NativeLibraryError, match="residual"):
                engine.debug_layer(hidden, csr, 0)
        try:
            engine.set_timing(1)
            engine.encode(x, csr, out_dtype=torch.float32)
            torch.cuda.synchronize()
            times = engine.kernel_times_ms()
        finally:
            engine.set_timing(0)
        assert len(times) == config.layers + 2, (name, times)
        assert all(t >= 0 for t in times) and sum(times[1:-1]) > 0, (name, times)


# ---- refusals -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(A.REFUSED))
def test_unsupported_architectures_are_refused_by_the_gpu_loader(tmp_path, name):
    from ginfinity_amd import Ginfinity
    from ginfinity_amd.weights import load_checkpoint
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    directory = A.write_model_dir(tmp_path / name, A.config_of(A.REFUSED[name]), 1)
    checkpoint = load_checkpoint(directory)
    for full_precision in (False, True):
        with pytest.raises(native.NativeLibraryError, match="gfy_encoder_create: "):
            Ginfinity.load("cuda", allow_nondeterministic_cuda=True, model_dir=directory,
                           full_precision=full_precision)
    lib = native.library()
    handle = ctypes.c_void_p()
    with torch.cuda.device(0):
        status = lib.gfy_encoder_create(checkpoint.weight_pack, len(checkpoint.weight_pack),
                                        native.GFY_F16, 0, ctypes.byref(handle))
    assert status == native.GFY_ERR_UNSUPPORTED and handle.value is None
