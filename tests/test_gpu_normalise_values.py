"""The float64 normalise of every device implementation, bit for bit, on head outputs that sit on
its edges (tests/normalise_cases.py): fp16 subnormals in, the subnormal grid out, the tie at half
the smallest subnormal, the 1e-12 clamp, -0.0, rows near 65504, rows of one element.

Each family is a model of its own (only head.2 differs); the raw head output is the device's own
``normalise=False`` run with the same settings, so a mismatch is the normalise step's and nothing
else's.  Both small shards of test_layernorm_with_a_large_row_mean_on_every_layer_kernel run as
one batch: 1,500 core rows, and 2,500 rows with context rows beside storing lanes and a ragged
last tile.  What ran, and how many values were compared, is printed (``pytest -s``)."""
from __future__ import annotations

import numpy as np
import pytest

import normalise_cases as N

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RANDOM = tuple(N.RANDOM_FAMILIES)


@pytest.fixture(scope="module")
def gpu_encoder():
    from ginfinity_amd import Ginfinity
    return Ginfinity.load("cuda:0", allow_nondeterministic_cuda=True)


@pytest.fixture(scope="module")
def config():
    from ginfinity_amd.weights import load_checkpoint
    return load_checkpoint().config


@pytest.fixture(scope="module")
def states(config):
    return N.head_families(config)


@pytest.fixture(scope="module")
def shards():
    from ginfinity_amd import synthetic
    return [synthetic.roofline_shard(9, records=3, length=500),
            synthetic.arbitrary_shard(4, nodes=2500, edges=12000)]


def _note(name: str, key: str, value) -> None:
    print(f"{name}: {key}: {value}")


class _Model:
    """One family's DeviceEncoder with both shards uploaded; ``run`` is ONE encode_coo_batch."""

    def __init__(self, gpu_encoder, state, config, shards, *, full_precision=False):
        from ginfinity_amd.engine import DeviceEncoder
        from ginfinity_amd.weights import build_weight_pack
        assert sum(shard.node_count for shard in shards) <= 4000
        self.engine = DeviceEncoder(build_weight_pack(state, config),
                                    full_precision=full_precision,
                                    device=gpu_encoder._engine.device)
        self.inputs = [self.engine.upload_arrays(shard.node_features, shard.edge_index,
                                                 shard.edge_types, shard.node_roles)
                       for shard in shards]
        self.rows = sum(int((shard.node_roles == 0).sum()) for shard in shards)

    def run(self, dtype, normalise: bool) -> np.ndarray:
        outs = self.engine.encode_coo_batch(self.inputs, out_dtype=dtype, normalise=normalise)
        out = np.concatenate([o.cpu().numpy() for o in outs])
        assert out.shape == (self.rows, N.DIM)
        return out

    def options(self, kernel: int, separate: int) -> None:
        from ginfinity_amd import _native as native
        self.engine.set_option(native.GFY_OPT_LAYER_KERNEL, kernel)
        self.engine.set_option(native.GFY_OPT_SEPARATE_HEAD, separate)

    def close(self) -> None:
        try:
            self.options(-1, 0)
        finally:
            self.engine.close()


def _same(got, want):
    return N._bytes(np.ascontiguousarray(got)) == N._bytes(np.ascontiguousarray(want))


def _check_constant_outputs(name: str, got: np.ndarray) -> None:
    """What a constant family's rows must be, written out: ``got`` in any output dtype."""
    dtype = got.dtype.type
    row = np.zeros(N.DIM, dtype=got.dtype)        # "zero": 0 / 1e-12, 128 x +0
    if name == "one_tiny":
        row[77] = 1.0
    elif name == "one_huge":
        row[8] = -1.0
    elif name == "three_four":
        row[[0, 127]] = (dtype(0.6), dtype(0.8))
    elif name == "below_tie":
        # |o| = 2 + 2^-50: the ones give 0.5 (1 - 2^-51), the 2^-24 a quotient just below the
        # tie at 2^-25 — 0 in fp16, not 2^-24; fp32 and float64 can hold it
        row[[1, 40, 64, 126]] = dtype(0.5 * (1.0 - 2.0 ** -51))
        row[15] = 0.0 if got.dtype == np.float16 else dtype(2.0 ** -25 * (1.0 - 2.0 ** -51))
    elif name == "all_max":
        row[:] = dtype(1.0 / np.sqrt(128.0))
        if got.dtype == np.float64:     # 65504 / sqrt(2^17 2047^2): the same to an ulp, every column
            assert np.all(np.abs(got - row) <= 2.0 ** -52 * row), name
            row[:] = got[0, 0]
    assert np.all(_same(got, np.broadcast_to(row, got.shape))), name
    assert not np.signbit(got[got == 0]).any(), name


def _check_edges_are_there(name: str, raw: np.ndarray) -> dict:
    """The caps of tests/test_normalise_cases_host.py on the DEVICE's raw output: a head that
    flushed its subnormals would otherwise pass every comparison below on nothing."""
    seen = N.counts(raw)
    if name in ("plain", "tiny14", "tiny20", "huge12"):
        assert seen["bracket_redo"] >= 100, (name, seen)
    if name == "ladder":
        assert seen["bracket_redo"] >= 50 and seen["subnormal_outputs"] >= 10_000, seen
    if name in ("tiny14", "tiny20", "ladder"):
        assert seen["subnormal_inputs"] >= 10_000 and seen["negative_zero_inputs"] >= 10, (name, seen)
    if name == "huge12":
        assert 2.0 ** 14 <= np.abs(raw.astype(np.float64)).max() < N.F16_MAX
    if name == "tiny24":
        norms = np.sqrt((raw.astype(np.float64) ** 2).sum(axis=1))
        assert np.all(norms > 0) and np.all(norms < 1e-6)
    if name in N.CONSTANT_FAMILIES:
        row = N.constant_rows()[name]
        assert np.all(_same(raw, np.broadcast_to(row, raw.shape))), name
    return seen


@pytest.mark.parametrize("name", N.FAMILIES)
def test_fp16_output_of_every_layer_kernel_fused_and_separate_head(name, gpu_encoder, states,
                                                                   config, shards):
    """fp16 model, fp16 output: the fused head of k_gine_layer_f16 / _q / _w / _x
    (GFY_OPT_LAYER_KERNEL 1, 3, 4, 5), and behind GFY_OPT_SEPARATE_HEAD k_head_f16<f16>
    (kernel 1) and k_head_d (3, 4, 5) — every value equals ``expected`` of the same settings'
    raw output, and the four kernels and k_head_d give the same bytes.  The constant families run
    kernels 1 and 4."""
    kernels = (1, 3, 4, 5) if name in RANDOM else (1, 4)
    model = _Model(gpu_encoder, states[name], config, shards)
    try:
        compared, first = {}, {}
        for separate in (0, 1):
            for kernel in kernels:
                model.options(kernel, separate)
                raw = model.run(torch.float16, False)
                assert model.engine.last_layer_kernel() == kernel
                got = model.run(torch.float16, True)
                assert model.engine.last_layer_kernel() == kernel
                assert raw.dtype == got.dtype == np.float16
                # the fused heads and k_head_d are one pipeline on the same registers' worth of
                # data; k_head_f16 deals the 16 channels of a k-step differently inside the MFMA
                # (last-bit flips of o on a few elements: test_fused_head_equals_standalone_head)
                head = "k_head_f16" if separate and kernel == 1 else "head_pipeline"
                if head not in first:
                    first[head] = (raw, got)
                    seen = _check_edges_are_there(name, raw)
                    assert N.robust_mask(raw, np.float16).all()
                    _note(name, f"fp16 model, {head}, raw", seen)
                else:
                    assert raw.tobytes() == first[head][0].tobytes(), (kernel, separate, "raw")
                    assert got.tobytes() == first[head][1].tobytes(), (kernel, separate)
                want = N.expected(raw, np.float16)
                wrong = ~_same(got, want)
                assert not wrong.any(), (name, kernel, separate, int(wrong.sum()),
                                         raw[wrong][:4], got[wrong][:4], want[wrong][:4])
                if name in N.CONSTANT_FAMILIES:
                    _check_constant_outputs(name, got)
                compared[f"kernel {kernel}, {'separate' if separate else 'fused'} head"] = got.size
        _note(name, "fp16 model, fp16 output, values compared", compared)
    finally:
        model.close()


def _check_wide_outputs(name, model, raw, label):
    """float32 output bit for bit on ``robust_mask``; float64 output bit for bit on
    ``exact_sum_rows`` and to a relative 2^-45 on the other rows (128 additions of relative
    error 2^-53 bound the sum of squares to 2^-46, hence the denominator to 2^-47)."""
    compared = {}
    got = model.run(torch.float32, True)
    keep = N.robust_mask(raw, np.float32)
    want = N.expected(raw, np.float32)
    wrong = ~_same(got, want)
    assert got.dtype == np.float32 and not (wrong & keep).any(), (name, int((wrong & keep).sum()))
    compared["float32"] = int(keep.sum())
    compared["float32 dropped by robust_mask"] = int((~keep).sum())
    compared["float32 dropped and different"] = int((wrong & ~keep).sum())
    if name in N.CONSTANT_FAMILIES:
        _check_constant_outputs(name, got)
    got = model.run(torch.float64, True)
    want = N.expected(raw, np.float64)
    exact = N.exact_sum_rows(raw)
    assert got.dtype == np.float64 and np.all(_same(got, want)[exact]), (name, "exact rows")
    assert np.all(np.abs(got - want) <= 2.0 ** -45 * np.abs(want)), name
    assert np.array_equal(np.signbit(got), np.signbit(want)), name
    compared["float64, rows bit for bit"] = int(exact.sum())
    compared["float64, rows to 2^-45"] = int((~exact).sum())
    if name in N.CONSTANT_FAMILIES:
        _check_constant_outputs(name, got)
    _note(name, label, compared)


@pytest.mark.parametrize("name", N.FAMILIES)
def test_float32_and_float64_output_of_the_fp16_model(name, gpu_encoder, states, config, shards):
    """k_head_f16<float> (``o * (1 / den)``, one cast) and k_head_f16<double> (true division)
    against ``expected`` of the fp16 raw output — read back through the same kernels'
    ``normalise=False`` output, which holds fp16 values."""
    model = _Model(gpu_encoder, states[name], config, shards)
    try:
        wide = model.run(torch.float32, False)
        raw = wide.astype(np.float16)
        assert np.array_equal(raw.astype(np.float32), wide)
        assert np.all(_same(wide, model.run(torch.float64, False).astype(np.float32)))
        _check_edges_are_there(name, raw)
        _check_wide_outputs(name, model, raw, "fp16 model, wide output, values compared")
    finally:
        model.close()


@pytest.mark.parametrize("name", N.FAMILIES)
def test_every_output_dtype_of_the_full_precision_model(name, gpu_encoder, states, config, shards):
    """csrc/gine_f32.hip (kEpiOutput: true division, one rounding): fp16, fp32 and float64 output
    against ``expected`` of the model's own float32 raw output."""
    model = _Model(gpu_encoder, states[name], config, shards, full_precision=True)
    try:
        raw = model.run(torch.float32, False)
        assert raw.dtype == np.float32 and np.isfinite(raw).all()
        assert np.array_equal(model.run(torch.float64, False), raw.astype(np.float64))
        if name in N.CONSTANT_FAMILIES:
            row = N.constant_rows()[name].astype(np.float32)
            assert np.all(_same(raw, np.broadcast_to(row, raw.shape))), name
        got = model.run(torch.float16, True)
        keep = N.robust_mask(raw, np.float16)
        wrong = ~_same(got, N.expected(raw, np.float16))
        assert got.dtype == np.float16 and not (wrong & keep).any(), (name, int((wrong & keep).sum()))
        out = np.abs(got.astype(np.float64))
        _note(name, "full-precision model, fp16 output",
              {"values compared": int(keep.sum()), "dropped by robust_mask": int((~keep).sum()),
               "dropped and different": int((wrong & ~keep).sum()),
               "outputs on the subnormal grid": int(((out > 0) & (out < N.F16_TINY)).sum())})
        if name == "ladder":
            assert ((out > 0) & (out < N.F16_TINY)).sum() >= 10_000
        if name in N.CONSTANT_FAMILIES:
            _check_constant_outputs(name, got)
        _check_wide_outputs(name, model, raw, "full-precision model, wide output, values compared")
    finally:
        model.close()
