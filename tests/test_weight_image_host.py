"""The device blob of an encoder, built on the host by tools/weight_image_dump.cpp (no HIP, no
GPU) through the library's own pack reader and derivation (csrc/weight_pack.h, weight_image.h):
byte for byte what ``gfy_encoder_create`` uploaded before the derivation was split into parts
(tests/golden/weight_image_sha256.json), and laid out as csrc/layer_image.h says.  Needs the
ROCm clang (``_Float16`` on the host); skipped where it is absent."""
from __future__ import annotations

import hashlib
import json
import subprocess
from pathlib import Path

import pytest

import arch_models as A
from ginfinity_amd import build
from ginfinity_amd.weights import build_weight_pack, random_state

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "weight_image_sha256.json").read_text())
CONFIGURATIONS = ("bundled", *A.VARIANTS)

#: csrc/layer_image.h, byte offsets from an image's start
IMAGE_FIGURES = {"image.table": 0, "image.alpha": 4352, "image.shift": 5376, "image.b0": 6400,
                 "image.b1": 6912, "image.gamma": 7168, "image.beta": 7424, "image.bytes": 7680,
                 "head_image.ba": 0, "head_image.bb": 256, "head_image.bytes": 512}


def _host_clang() -> Path | None:
    hipcc = build._hipcc()
    if hipcc is None:
        return None
    rocm = Path(hipcc).resolve().parents[1]
    for candidate in (rocm / "llvm" / "bin" / "clang++", rocm / "lib" / "llvm" / "bin" / "clang++"):
        if candidate.exists():
            return candidate
    return None


@pytest.fixture(scope="module")
def dump_tool(tmp_path_factory) -> Path:
    """tools/weight_image_dump built with the library's own floating-point flags."""
    clang = _host_clang()
    if clang is None:
        pytest.skip("no ROCm clang (hipcc's llvm/bin/clang++) on this machine")
    binary = tmp_path_factory.mktemp("weight_image") / "weight_image_dump"
    flags = [flag for flag in build.FLAGS if not flag.startswith("--offload-arch")]
    sources = [ROOT / "tools" / "weight_image_dump.cpp", build.CSRC / "weight_image.cpp",
               build.CSRC / "gfy_base.cpp"]
    done = subprocess.run([str(clang), *flags, *map(str, sources), "-o", str(binary)],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return binary


@pytest.fixture(scope="module")
def packs(checkpoint, tmp_path_factory) -> dict[str, Path]:
    folder = tmp_path_factory.mktemp("weight_packs")
    written = {}
    for name in CONFIGURATIONS:
        pack = (checkpoint.weight_pack if name == "bundled"
                else build_weight_pack(random_state(*A.variant(name)), A.variant(name)[0]))
        # the images were recorded for exactly these weights
        assert hashlib.sha256(pack).hexdigest() == GOLDEN[name]["pack_sha256"], name
        written[name] = folder / f"{name}.pack"
        written[name].write_bytes(pack)
    return written


def _dump(tool: Path, pack: Path, dtype: str, out: Path) -> dict[str, int]:
    done = subprocess.run([str(tool), str(pack), dtype, str(out)], capture_output=True, text=True,
                          timeout=60)
    assert done.returncode == 0, done.stderr[-2000:]
    return {name: int(value) for name, value in (line.split() for line in done.stdout.splitlines())}


@pytest.mark.parametrize("dtype", ("f16", "f32"))
@pytest.mark.parametrize("name", CONFIGURATIONS)
def test_image_is_byte_for_byte_the_recorded_one(dump_tool, packs, tmp_path, name, dtype):
    table = _dump(dump_tool, packs[name], dtype, tmp_path / "image.bin")
    image = (tmp_path / "image.bin").read_bytes()
    assert table["blob.bytes"] == len(image) == GOLDEN[name][dtype]["bytes"]
    assert hashlib.sha256(image).hexdigest() == GOLDEN[name][dtype]["sha256"]


def test_offset_table_is_layer_image_h(dump_tool, packs, tmp_path):
    """The figures the program prints are layer_image.h's, and the fp16 blob holds a whole
    per-layer image at every ``layerN.image`` and the head's at ``head.image``: 256-byte
    aligned, inside the blob, the -inf row of idle slots where ``image.table`` says."""
    table = _dump(dump_tool, packs["bundled"], "f16", tmp_path / "image.bin")
    image = (tmp_path / "image.bin").read_bytes()
    assert {name: table[name] for name in IMAGE_FIGURES} == IMAGE_FIGURES
    header = (build.CSRC / "layer_image.h").read_text()
    for name in ("kImageTable", "kImageAlpha", "kImageShift", "kImageB0", "kImageB1", "kImageGamma",
                 "kImageBeta", "kImageBytes", "kHeadImageBa", "kHeadImageBb", "kHeadImageBytes"):
        assert f"constexpr int {name} =" in header, name
    layers = [table[f"layer{l}.image"] for l in range(4)]
    for start in layers:
        assert start % 256 == 0 and start + table["image.bytes"] <= len(image)
        idle = start + table["image.table"] + 16 * 256          # row kMaxEdgeTypes of 17
        assert image[idle:idle + 256] == bytes.fromhex("00fc") * 128   # fp16 -inf
    assert table["head.image"] % 256 == 0
    assert table["head.image"] + table["head_image.bytes"] == len(image) == table["blob.bytes"]
