"""device="cpu" on the architectures the library accepts besides the bundled one
(tests/arch_models.py: one layer, eight layers, no residual, 4 / 12 / 13 / 16 edge types,
structure feature B without positions), loaded through the public ``Ginfinity.load(model_dir=)``:
against what the genuine reference returned for the same model directories
(tests/golden/architectures.npz, make_golden.py F8), and bit for bit against the oracle.  The
architectures the kernels are not built for are refused at load."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

import arch_models as A

F16_TOL = 1e-3
F32_TOL = 1e-6


def check_margins(name, got, want):
    """The regression bounds of test_gpu_parity._record_margin (fp16 model against the
    reference's own rows): max, p99.9 and mean |difference|, share of identical elements."""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    same = float(np.mean(got.view(np.uint16) == want.view(np.uint16)))
    assert diff.max() <= 7.4e-4, (name, diff.max())
    assert np.quantile(diff, 0.999) <= 2.6e-4, (name, np.quantile(diff, 0.999))
    assert diff.mean() <= 5.5e-5, (name, diff.mean())
    assert same >= 0.29, (name, same)


@pytest.fixture(scope="module")
def arch(golden):
    return golden("architectures.npz")


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("architectures")
    return {name: A.write_model_dir(root / name, *A.variant(name)) for name in A.VARIANTS}


def _maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("name", list(A.VARIANTS))
def test_fixture_records_these_architectures_and_weights(arch, name):
    """The fixture was recorded for exactly the configuration, seed and weight pack the tests
    rebuild: a change of ``random_state`` or of a variant fails here, not as a parity miss."""
    config, seed = A.variant(name)
    assert int(arch[f"{name}.seed"]) == seed
    recorded = json.loads(str(arch[f"{name}.config"]))
    assert recorded == {**{f: getattr(config, f) for f in config.__dataclass_fields__},
                        "extra_edges": list(config.extra_edges)}
    assert str(arch[f"{name}.pack_sha256"]) == A.pack_sha256(config, seed)
    shard = A.arbitrary_input(config)
    assert set(np.unique(shard.edge_types).tolist()) == set(range(config.edge_dim))
    assert np.bincount(shard.edge_index[1]).max() > 8


@pytest.mark.parametrize("name", list(A.VARIANTS))
def test_host_path_matches_the_reference_on_every_architecture(arch, model_dirs, rouskin_records,
                                                               name):
    from ginfinity_amd import Ginfinity
    config, _seed = A.variant(name)
    records = rouskin_records[:int(arch["rouskin.records"])]
    shard = A.arbitrary_input(config)
    rs, ars = int(arch["rouskin.stride"]), int(arch["arbitrary.stride"])
    enc16 = Ginfinity.load("cpu", model_dir=model_dirs[name])
    assert enc16.graph_spec.sha256 == A.spec_of(config).sha256
    assert enc16.info()["encoder_config"]["layers"] == config.layers
    outputs = enc16.encode_many(records)
    assert [o.shape[0] for o in outputs] == [r.length for r in records]
    for label, got in (("rouskin", np.concatenate(outputs)[::rs]),
                       ("arbitrary", np.concatenate(enc16.encode_graphs(shard))[::ars])):
        want = arch[f"{name}.{label}.m16.float16"]
        assert got.shape == want.shape and got.dtype == np.float16
        assert _maxabs(got, want) <= F16_TOL, (name, label)
        check_margins(f"{name} {label}", got, want)
    enc32 = Ginfinity.load("cpu", model_dir=model_dirs[name], full_precision=True)
    for label, got in (
            ("rouskin", np.concatenate(enc32.encode_many(records, embedding_dtype="float32"))[::rs]),
            ("arbitrary", np.concatenate(enc32.encode_graphs(
                shard, embedding_dtype="float32"))[::ars])):
        want = arch[f"{name}.{label}.m32.float32"]
        assert got.shape == want.shape and got.dtype == np.float32
        assert _maxabs(got, want) <= F32_TOL, (name, label)


@pytest.mark.parametrize("name", list(A.VARIANTS))
def test_host_path_equals_the_oracle_bit_for_bit(model_dirs, rouskin_records, name):
    """The host implementation keeps the oracle's rounding points: every row of both inputs,
    the records' graphs built with the architecture's own spec."""
    from ginfinity_amd import Ginfinity, GraphBuilder
    from ginfinity_amd.weights import random_state
    from oracle import gine_numpy as G
    config, seed = A.variant(name)
    weights = G.Weights.from_state_dict(random_state(config, seed), layers=config.layers,
                                        residual=config.residual)
    encoder = Ginfinity.load("cpu", model_dir=model_dirs[name])
    records = GraphBuilder(A.spec_of(config)).build_shard(rouskin_records[:24])
    for shard in (records, A.arbitrary_input(config)):
        got = np.concatenate(encoder.encode_graphs(shard))
        want = G.encode(weights, shard.node_features, shard.edge_index,
                        shard.edge_types)[shard.node_roles == 0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), name


@pytest.mark.parametrize("name", list(A.REFUSED))
def test_unsupported_architectures_are_refused_at_load(tmp_path, name):
    """Self-consistent checkpoints the kernels are not built for: ``load`` raises the library's
    error naming the limit, and the C ABI hands back no encoder."""
    from ginfinity_amd import Ginfinity, _native as native
    from ginfinity_amd.weights import load_checkpoint
    config = A.config_of(A.REFUSED[name])
    directory = A.write_model_dir(tmp_path / name, config, 1)
    checkpoint = load_checkpoint(directory)          # the checkpoint itself is well-formed
    for full_precision in (False, True):
        with pytest.raises(native.NativeLibraryError, match="gfy_host_encoder_create: built for"):
            Ginfinity.load("cpu", model_dir=directory, full_precision=full_precision)
    lib = native.host_library()
    handle = ctypes.c_void_p()
    status = lib.gfy_host_encoder_create(checkpoint.weight_pack, len(checkpoint.weight_pack),
                                         native.GFY_F16, ctypes.byref(handle))
    assert status == native.GFY_ERR_UNSUPPORTED and handle.value is None
