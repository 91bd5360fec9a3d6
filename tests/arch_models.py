"""Model directories of architectures other than the bundled one (not a test module).

``Ginfinity.load(model_dir=...)`` accepts any self-consistent checkpoint, and the C ABI more
depths, edge vocabularies and residual settings than the bundled model uses (include/gfy.h,
``gfy_encoder_create``).  ``VARIANTS`` are the architectures the suites run besides the bundled
one, with seeded ``random_state`` weights; ``REFUSED`` are architectures every loader must turn
away.  ``write_model_dir`` writes ``encoder.pt`` + ``model.json`` in the reference's layout
(checksum, graph spec, parameter count), so tests go through the public loader, and
tests/golden/make_golden.py hands the same directories to the genuine reference.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
from pathlib import Path

import torch

from ginfinity_amd.spec import DATA_DIRECTORY, GraphSpec
from ginfinity_amd.weights import (EncoderConfig, build_weight_pack, parameter_count,
                                   random_state, tensor_order)

#: name -> (changes to the bundled architecture, random_state seed)
VARIANTS: dict[str, tuple[dict, int]] = {
    # one layer: the fused head sits in the FIRST layer launch; 13 edge types: no windowed kernel
    "v1": (dict(layers=1, residual=False, edge_dim=13), 101),
    # kMaxLayers deep; the smallest vocabulary a spec without skip2 allows
    "v2": (dict(layers=8, edge_dim=4, extra_edges=()), 102),
    # structure feature B without positions (still 7 inputs); 12 types: the windowed kernel's limit
    "v3": (dict(struct_feature="B", positional=False, layers=3, edge_dim=12), 103),
    # every table row live (kMaxEdgeTypes), next to the -inf idle row
    "v4": (dict(layers=2, residual=False, edge_dim=16), 104),
}

#: architectures the kernels are not built for: refused at load, by the host and the GPU loader
REFUSED: dict[str, dict] = {
    "layers9": dict(layers=9),
    "edge_dim17": dict(edge_dim=17),
    "struct_b_positional": dict(struct_feature="B", positional=True),
    "hidden64": dict(hidden=64),
}


def bundled_metadata() -> dict:
    return json.loads((DATA_DIRECTORY / "model.json").read_text())


def config_of(changes: dict) -> EncoderConfig:
    """The bundled architecture with ``changes`` applied."""
    return dataclasses.replace(
        EncoderConfig.from_dict(bundled_metadata()["encoder_config"]),
        **{k: tuple(v) if k == "extra_edges" else v for k, v in changes.items()})


def variant(name: str) -> tuple[EncoderConfig, int]:
    changes, seed = VARIANTS[name]
    return config_of(changes), seed


def spec_of(config: EncoderConfig) -> GraphSpec:
    return GraphSpec.from_encoder_config(config)


def pack_sha256(config: EncoderConfig, seed: int) -> str:
    """SHA-256 of the weight pack of ``random_state(config, seed)``: the fixture stores it, so
    a change of ``random_state`` fails loudly instead of comparing other weights."""
    return hashlib.sha256(build_weight_pack(random_state(config, seed), config)).hexdigest()


def write_model_dir(directory: str | Path, config: EncoderConfig, seed: int) -> Path:
    """``encoder.pt`` (``{"cfg", "state_dict"}``, BatchNorm counters included, as the reference
    saves a model) and ``model.json`` (the bundled metadata with this architecture, its graph
    spec and fingerprint, parameter count and checkpoint SHA-256) under ``directory``."""
    root = Path(directory)
    root.mkdir(parents=True, exist_ok=True)
    state = random_state(config, seed)
    tensors = {name: torch.from_numpy(state[name]) for name in tensor_order(config.layers)}
    for layer in range(config.layers):
        tensors[f"convs.{layer}.mlp.1.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    cfg = {**dataclasses.asdict(config), "extra_edges": list(config.extra_edges)}
    torch.save({"cfg": cfg, "state_dict": tensors}, root / "encoder.pt")
    spec = spec_of(config)
    metadata = bundled_metadata()
    metadata.update({
        "checkpoint_sha256": hashlib.sha256((root / "encoder.pt").read_bytes()).hexdigest(),
        "parameter_count": parameter_count(state),
        "embedding_dimension": config.out_dim,
        "encoder_config": cfg,
        "graph_spec": spec.to_dict(),
        "graph_spec_sha256": spec.sha256,
    })
    (root / "model.json").write_text(json.dumps(metadata, indent=2) + "\n")
    return root


def arbitrary_input(config: EncoderConfig):
    """The fixture's interchange shard for an architecture: 2,000 nodes in 4 records, edge
    types drawn from every ``0..edge_dim-1``, a hub of in-degree 40 per record (the direct
    path), ~10 % context nodes."""
    from ginfinity_amd import synthetic
    return synthetic.arbitrary_shard(5, nodes=2000, edges=10_000, spec=spec_of(config))


#: records of tests/golden/rouskin_sample_6k.tsv the fixture encodes with ``encode_many``
ROUSKIN_RECORDS = 24
#: every STRIDE-th output row is recorded (rouskin input, arbitrary input)
STRIDES = (23, 13)
