"""The host C++ (csrc/gfy_base.cpp, gine_host.cpp, weight_image.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer, from stand-alone programs: results that
are only compared through ``ctypes`` stay right after a read past a buffer, a misaligned
store, a signed overflow or a data race.  tools/host_sanitize.cpp is built three times (ASan +
UBSan, TSan, no sanitizer: a byte mismatch can then be told from a sanitizer effect), runs the
cases of tests/host_sanitize_cases.py — sizes on both sides of every path switch of the copy
loops and of the node blocks, hostile weight packs, refusals — and compares every result with
bytes worked out without the library.  tools/weight_image_dump.cpp, built the same way, puts
the image derivation under the sanitizers against the recorded SHA-256.

Host only: no ``gpu`` marker, no device, nothing preloaded, and nothing built here is loaded
into the interpreter — the programs are started directly.  The last two tests run the same
micro-batch and encode cases through the built library, where no sanitizer is needed."""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import time
from pathlib import Path

import pytest

import arch_models as A
import host_sanitize_cases as C
from ginfinity_amd import build
from test_weight_image_host import CONFIGURATIONS, GOLDEN, _dump, _host_clang

ROOT = Path(__file__).resolve().parents[1]
#: after build.FLAGS (the library's floating-point flags; the later -O wins)
BUILDS = {
    "asan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
    "plain": [],
}
SUBCOMMANDS = ("pack", "microbatch", "encode", "threads")
REPORTS = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: ThreadSanitizer")
ENVIRONMENT = {"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


def _compilers() -> list[str]:
    """The ROCm clang where it exists, then $CXX / g++ (host_sanitize needs no ``_Float16``)."""
    found = [str(_host_clang())] if _host_clang() else []
    other = shutil.which(os.environ.get("CXX", "g++"))
    return found + ([other] if other else [])


def _compile(compiler: str, flags: list[str], sources: list[Path], binary: Path):
    library = [flag for flag in build.FLAGS if not flag.startswith("--offload-arch")]
    started = time.perf_counter()
    done = subprocess.run([compiler, *library, *flags, "-pthread", *map(str, sources), "-o", str(binary)],
                          capture_output=True, text=True, timeout=600)
    return done, time.perf_counter() - started


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """``programs(kind, name)`` → the program ``name`` (host_sanitize, weight_image_dump) of
    build ``kind``, built on first use; skips where no compiler links the sanitizer's runtime."""
    folder = tmp_path_factory.mktemp("host_sanitize_bin")
    probe = folder / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    sources = {
        "host_sanitize": [ROOT / "tools" / "host_sanitize.cpp", build.CSRC / "gfy_base.cpp",
                          build.CSRC / "gine_host.cpp"],
        "weight_image_dump": [ROOT / "tools" / "weight_image_dump.cpp", build.CSRC / "weight_image.cpp",
                              build.CSRC / "gfy_base.cpp"],
    }
    built: dict[tuple[str, str], Path | str] = {}

    def make(kind: str, name: str) -> Path | str:
        compilers = _compilers() if name == "host_sanitize" else [str(c) for c in [_host_clang()] if c]
        if not compilers:
            return "no ROCm clang (hipcc's llvm/bin/clang++) on this machine" \
                if name == "weight_image_dump" else "no C++ compiler on this machine"
        reasons = []
        for compiler in compilers:
            trial = folder / f"probe_{kind}"
            done, _ = _compile(compiler, BUILDS[kind], [probe], trial)
            if done.returncode != 0 or subprocess.run([str(trial)], timeout=60).returncode != 0:
                reasons.append(f"{compiler} cannot link or run {' '.join(BUILDS[kind])}: "
                               + done.stderr.strip()[-300:])
                continue
            binary = folder / f"{name}_{kind}"
            done, seconds = _compile(compiler, BUILDS[kind], sources[name], binary)
            assert done.returncode == 0, done.stderr[-3000:]
            print(f"built {name} [{kind}] with {compiler} in {seconds:.1f} s")
            return binary
        return "; ".join(reasons)

    def get(kind: str, name: str = "host_sanitize") -> Path:
        if (kind, name) not in built:
            built[kind, name] = make(kind, name)
        if isinstance(built[kind, name], str):
            print(f"skipped: {built[kind, name]}")
            pytest.skip(built[kind, name])
        return built[kind, name]

    return get


@pytest.fixture(scope="module")
def packs(checkpoint) -> dict[str, bytes]:
    from ginfinity_amd.weights import build_weight_pack, random_state
    made = {"bundled": checkpoint.weight_pack}
    for name in A.VARIANTS:
        made[name] = build_weight_pack(random_state(*A.variant(name)), A.variant(name)[0])
    for name, pack in made.items():      # the weights the recorded images were built from
        assert hashlib.sha256(pack).hexdigest() == GOLDEN[name]["pack_sha256"], name
    return made


@pytest.fixture(scope="module")
def models(packs, oracle_weights):
    """The bundled model and ``v1`` (one layer, 13 edge types, no residual):
    ``{label: (pack, oracle weights, edge types)}``."""
    from ginfinity_amd.weights import random_state
    from oracle import gine_numpy as G
    config, seed = A.variant("v1")
    other = G.Weights.from_state_dict(random_state(config, seed), layers=config.layers,
                                      residual=config.residual)
    return {"bundled": (packs["bundled"], oracle_weights, 10), "v1": (packs["v1"], other, config.edge_dim)}


@pytest.fixture(scope="module")
def cases(packs, models):
    pack, weights, edge_dim = models["bundled"]
    return {"pack": C.pack_cases(packs), "microbatch": C.microbatch_cases(),
            "encode": C.encode_cases(models), "threads": C.threads_cases(pack, weights, edge_dim)}


@pytest.fixture(scope="module")
def case_directories(cases, tmp_path_factory):
    """``{sub-command: (directory, case names)}``, written once for all builds."""
    root = tmp_path_factory.mktemp("host_sanitize_cases")
    return {name: (root / name, C.write_cases(root / name, listed)) for name, listed in cases.items()}


def _clean(done: subprocess.CompletedProcess) -> None:
    assert done.returncode == 0, (done.stdout[-1500:], done.stderr[-3000:])
    for report in REPORTS:
        assert report not in done.stderr, done.stderr[-3000:]


def _environment() -> dict[str, str]:
    env = {**os.environ, **ENVIRONMENT}
    env.pop("GFY_PACK_STREAM", None)      # the program sets and unsets it per case
    return env


@pytest.mark.parametrize("command", SUBCOMMANDS)
@pytest.mark.parametrize("kind", list(BUILDS))
def test_host_code_is_clean_and_right(programs, case_directories, kind, command):
    """Exit status 0, one ``ok`` line for every case of the manifest — none can drop out
    silently — and no sanitizer report on stderr."""
    program = programs(kind)
    directory, names = case_directories[command]
    started = time.perf_counter()
    done = subprocess.run([str(program), command, str(directory)], capture_output=True, text=True,
                          timeout=900, env=_environment())
    print(f"{command} [{kind}]: {len(names)} cases in {time.perf_counter() - started:.1f} s")
    _clean(done)
    assert done.stdout.splitlines() == [f"ok {command} {name}" for name in names]


@pytest.mark.parametrize("dtype", ("f16", "f32"))
@pytest.mark.parametrize("kind", ("asan", "plain"))
def test_image_derivation_is_clean_and_the_recorded_one(programs, packs, tmp_path, kind, dtype,
                                                        monkeypatch):
    """``build_image_f16`` / ``build_image_f32`` of every pack: the blob's size and SHA-256 are
    those of tests/golden/weight_image_sha256.json, with the index formulas of weight_image.cpp
    under ASan + UBSan (single-threaded: no TSan build).  Needs the ROCm clang."""
    program = programs(kind, "weight_image_dump")
    for name, value in ENVIRONMENT.items():
        monkeypatch.setenv(name, value)
    for name in CONFIGURATIONS:
        (tmp_path / f"{name}.pack").write_bytes(packs[name])
        table = _dump(program, tmp_path / f"{name}.pack", dtype, tmp_path / "image.bin")
        image = (tmp_path / "image.bin").read_bytes()
        assert table["blob.bytes"] == len(image) == GOLDEN[name][dtype]["bytes"], name
        assert hashlib.sha256(image).hexdigest() == GOLDEN[name][dtype]["sha256"], name


def test_a_case_that_fails_is_reported(programs, case_directories, tmp_path):
    """The program's own check: one wrong expected byte, status or thread count away from a
    case, it exits 1 with a ``FAIL`` line naming the case, after the ``ok`` lines before it."""
    program = programs("plain")
    listed = [("right", {"pack": b"\0" * 40, "dtype": C.F16, "status": C.INVALID, "error": "magic/version"}),
              ("wrong", {"pack": b"\0" * 40, "dtype": C.F16, "status": C.OK, "error": ""})]
    C.write_cases(tmp_path / "pack", listed)
    done = subprocess.run([str(program), "pack", str(tmp_path / "pack")], capture_output=True,
                          text=True, timeout=60, env=_environment())
    assert done.returncode == 1
    assert done.stdout.splitlines()[0] == "ok pack right"
    assert done.stdout.splitlines()[1].startswith("FAIL pack wrong: status 1, expected 0")


# ---- the same cases through the built library (no sanitizer, ctypes) -----------------------------

def test_microbatch_cases_through_the_library(cases):
    from ginfinity_amd import _native as native
    lib = native.host_library()
    for name, fields in cases["microbatch"]:
        try:
            C.run_microbatch(lib, fields)
        except AssertionError as error:
            raise AssertionError(f"{name}: {error}") from error


def test_encode_cases_through_the_library(cases):
    from ginfinity_amd import _native as native
    lib = native.host_library()
    encoders: dict = {}
    try:
        for name, fields in cases["encode"]:
            try:
                C.run_encode(lib, encoders, fields)
            except AssertionError as error:
                raise AssertionError(f"{name}: {error}") from error
    finally:
        for handle in encoders.values():
            lib.gfy_host_encoder_destroy(handle)
