"""The head families of tests/normalise_cases.py sit on the edges they are named after, both
fp16 shortcuts of the kernels — emulated in numpy — give the reference's bytes there, and the CPU
device (csrc/gine_host.cpp) does.  The caps are conditions the device tests of
tests/test_gpu_normalise_values.py rely on, not measurements.  No device."""
from __future__ import annotations

import numpy as np
import pytest

import normalise_cases as N

RANDOM = tuple(N.RANDOM_FAMILIES)


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


@pytest.fixture(scope="module")
def raws(states, config, shards):
    """The oracle's raw fp16 head output of every family on the 1,500 rows of the first shard."""
    return N.head_outputs(states, config, shards[0])


def _same(got, want):
    return N._bytes(np.ascontiguousarray(got)) == N._bytes(np.ascontiguousarray(want))


# ---- the helpers themselves, on rows worked by hand ----------------------------------------------

def test_expected_on_rows_worked_by_hand():
    rows = N.constant_rows()
    raw = np.stack([rows[name] for name in N.CONSTANT_FAMILIES])
    for dtype in (np.float16, np.float32, np.float64):
        out = N.expected(raw, dtype)
        assert out.dtype == dtype
        zero, one_tiny, one_huge, three_four, below_tie, all_max = out
        assert not zero.any() and not np.signbit(zero).any()            # 0 / 1e-12 = +0
        assert one_tiny[77] == 1.0 and np.count_nonzero(one_tiny) == 1
        assert one_huge[8] == -1.0 and np.count_nonzero(one_huge) == 1
        assert three_four[0] == dtype(0.6) and three_four[127] == dtype(0.8)
        if dtype != np.float64:
            assert np.all(all_max == dtype(1.0 / np.sqrt(128.0)))
        else:                                            # two float64 roundings against two
            assert np.all(np.abs(all_max - 1.0 / np.sqrt(128.0)) <= 2.0 ** -52 * all_max)
        assert np.all(below_tie[[1, 40, 64, 126]] == dtype(0.5 * (1.0 - 2.0 ** -51)))
    # 2^-24 / (2 + 2^-50): a float64 just below 2^-25, the tie between 0 and 2^-24
    assert N.denominator(raw)[4] == 2.0 + 2.0 ** -50
    assert N.expected(raw, np.float64)[4, 15] == 2.0 ** -25 * (1.0 - 2.0 ** -51)
    assert N.expected(raw, np.float16)[4, 15] == 0.0
    assert N.expected(raw, np.float32)[4, 15] == np.float32(2.0 ** -25)


def test_moving_the_denominator_moves_exactly_the_values_on_an_edge():
    rows = N.constant_rows()
    raw = np.stack([rows["one_tiny"], rows["below_tie"], rows["three_four"]])
    assert N.denominator(raw, 1)[2] == np.nextafter(5.0, 6.0)
    assert N.denominator(raw, -2)[1] == 2.0                # the tie itself: still 0 (to even)
    assert N.robust_mask(raw, np.float16).all()
    assert N.robust_mask(raw, np.float32).all()            # 24 bits: 2^29 ulps of room
    # float64 output has no room at all: 2^-24 / (2^-24 (1 + 2^-51)) is not 1, 3 / (5 + 2 ulps)
    # not 0.6; a zero stays a zero
    assert np.array_equal(N.robust_mask(raw[[0, 2]], np.float64), raw[[0, 2]] == 0)


def test_exact_sum_rows_on_rows_worked_by_hand():
    raw = np.zeros((5, N.DIM), dtype=np.float16)
    raw[1, :] = 65504.0                                   # 2^17 2047^2: 39 bits
    raw[2, 0], raw[2, 1] = 65504.0, 2.0 ** -24            # 2^32 against 2^-48: 80 bits apart
    raw[3, 0], raw[3, 1] = 1.0, 2.0 ** -24                # 1 + 2^-48: 49 bits
    raw[4, 0], raw[4, 1] = 8.0, 2.0 ** -24                # 64 + 2^-48: 55 bits
    assert N.exact_sum_rows(raw).tolist() == [True, True, False, True, False]
    wide = raw.astype(np.float32)
    assert N.exact_sum_rows(wide).tolist() == [True, True, False, True, False]
    wide[3, 2] = np.float32(1.0 + 2.0 ** -23)             # a square of 47 bits below 2^1
    assert N.exact_sum_rows(wide).tolist() == [True, True, False, True, False]
    wide[3, 1] = np.float32(2.0 ** -4 * (1.0 + 2.0 ** -23))    # lowest bit 2^-54, sum above 2
    assert N.exact_sum_rows(wide).tolist() == [True, True, False, False, False]


def test_the_emulations_take_their_float64_path_where_the_kernels_do():
    rows = N.constant_rows()
    raw = np.stack([rows["below_tie"], rows["three_four"], rows["one_tiny"], rows["zero"]])
    for emulate in (N.emulate_bracket, N.emulate_window):
        redo, fast = emulate(raw)
        assert fast.dtype == np.float16 and redo.dtype == bool
        assert redo[0, 15] and not redo[1:].any()          # only the value at the tie
        assert not redo[0, [1, 40, 64, 126]].any()         # 0.5 (1 - 2^-51): nowhere near one
        assert fast[1, 0] == np.float16(0.6) and fast[2, 77] == 1.0 and not fast[3].any()
    assert N.emulate_bracket(raw)[1][0, 15] == np.float16(2.0 ** -24)   # the upper product's
    negative = (-raw[3:]).astype(np.float16)
    for emulate in (N.emulate_bracket, N.emulate_window):
        assert np.signbit(emulate(negative)[1]).all()      # -0 in, -0 out: numpy's own answer
    assert np.signbit(N.expected(negative, np.float16)).all()


# ---- the generator sits on its edges -------------------------------------------------------------

def test_families_are_seeded_and_differ_in_head_2_only(states, config):
    again = N.head_families(config)
    assert tuple(states) == N.FAMILIES
    for name, state in states.items():
        for key, value in state.items():
            assert value.dtype == np.float32 and np.array_equal(value, again[name][key])
            if not key.startswith("head.2."):
                assert value is states["plain"][key] or np.array_equal(value, states["plain"][key])
    for name in N.CONSTANT_FAMILIES:
        assert not states[name]["head.2.weight"].any()
        assert np.array_equal(states[name]["head.2.bias"],
                              N.constant_rows()[name].astype(np.float32))


def test_constant_families_give_their_row_at_every_node(raws):
    for name, row in N.constant_rows().items():
        assert raws[name].shape == (1500, N.DIM)
        assert np.all(_same(raws[name], np.broadcast_to(row, raws[name].shape))), name


def test_every_family_sits_on_its_edges(raws):
    for name in N.FAMILIES:
        raw = raws[name]
        assert raw.dtype == np.float16 and np.isfinite(raw.astype(np.float32)).all(), name
        seen = N.counts(raw)
        dropped = int((~N.robust_mask(raw, np.float32)).sum())
        print(f"{name}: {seen}, float32 values robust_mask drops: {dropped}, "
              f"rows with an exact sum: {int(N.exact_sum_rows(raw).sum())} of {raw.shape[0]}")
        if name in ("plain", "tiny14", "tiny20", "huge12"):
            assert seen["bracket_redo"] >= 100, (name, seen)
        if name == "ladder":
            assert seen["bracket_redo"] >= 50 and seen["subnormal_outputs"] >= 10_000, seen
        if name in ("tiny14", "tiny20", "ladder"):
            assert seen["subnormal_inputs"] >= 10_000, (name, seen)
            assert seen["negative_zero_inputs"] >= 10, (name, seen)
        if name == "huge12":
            assert 2.0 ** 14 <= np.abs(raw.astype(np.float64)).max() < N.F16_MAX
        if name == "tiny24":
            norms = np.sqrt((raw.astype(np.float64) ** 2).sum(axis=1))
            assert np.all(norms > 0) and np.all(norms < 1e-6)
        assert N.robust_mask(raw, np.float16).all(), name
        assert dropped <= 1e-5 * raw.size, (name, dropped)
    # both sides of exact_sum_rows are there
    exact = N.exact_sum_rows(raws["plain"])
    assert exact.any() and not exact.all()


# ---- both emulated shortcuts are the reference's function ----------------------------------------

@pytest.mark.parametrize("shortcut", ["bracket", "window"])
def test_emulated_shortcut_equals_expected_on_every_value(raws, shortcut):
    emulate = {"bracket": N.emulate_bracket, "window": N.emulate_window}[shortcut]
    for name in N.FAMILIES:
        raw = raws[name]
        want = N.expected(raw, np.float16)
        redo, fast = emulate(raw)
        assert np.all(_same(fast, want)[~redo]), (name, "fast path")
        assert np.all(_same(N.float64_path(raw), want)), (name, "float64 path")
        assert np.all(_same(N.through_shortcut(raw, emulate), want)), name


def test_the_float64_path_is_needed_and_two_roundings_are_wrong(raws):
    """The edges are sharp enough to tell the variants apart: the bracket's upper product alone,
    and float64 -> fp32 -> fp16, each miss ``expected`` on values of the random families."""
    for name in ("plain", "tiny14", "tiny20", "huge12", "ladder"):
        raw = raws[name]
        want = N.expected(raw, np.float16)
        redo, fast = N.emulate_bracket(raw)
        assert (~_same(fast, want))[redo].sum() >= 10, name
    twice = lambda raw: N.expected(raw, np.float32).astype(np.float16)
    missed = {name: int((~_same(twice(raws[name]), N.expected(raws[name], np.float16))).sum())
              for name in RANDOM}
    print(f"values that rounding twice gets wrong: {missed}")
    assert sum(missed.values()) >= 10, missed


# ---- the CPU device ------------------------------------------------------------------------------

def _host_encode(encoder, shard, dtype, normalise):
    return encoder.encode_arrays(shard.node_features, shard.edge_index, shard.edge_types,
                                 shard.node_roles, embedding_dtype=np.dtype(dtype),
                                 normalise=normalise)


@pytest.mark.parametrize("full_precision", [False, True], ids=["half", "full"])
def test_cpu_device_normalise_is_the_float64_quotient_rounded_once(states, config, shards,
                                                                   full_precision):
    """csrc/gine_host.cpp: ``normalise=True`` against ``expected`` of the encoder's own
    ``normalise=False`` output — fp16 and fp32 output bit for bit on ``robust_mask``, float64
    output bit for bit on ``exact_sum_rows`` and to a relative 2^-45 elsewhere (128 additions of
    relative error 2^-53 bound the sum of squares to 2^-46, the denominator to 2^-47).  Every
    random family on the 1,500 rows whose edges the caps above hold for, ``ladder`` on the shard
    with context rows as well; a constant family, one row at every node, on 100 rows."""
    from ginfinity_amd import synthetic
    from ginfinity_amd.host import HostEncoder
    from ginfinity_amd.weights import build_weight_pack
    raw_dtype = np.float32 if full_precision else np.float16
    few = synthetic.roofline_shard(9, records=1, length=100)
    for name, state in states.items():
        encoder = HostEncoder(build_weight_pack(state, config), full_precision=full_precision)
        try:
            compared = {}
            for shard in (shards if name == "ladder" else [few] if name in N.CONSTANT_FAMILIES
                          else shards[:1]):
                raw = _host_encode(encoder, shard, raw_dtype, False)
                assert raw.shape == (int((shard.node_roles == 0).sum()), N.DIM)
                if name == "ladder" and not full_precision:
                    # the fp16 model's o IS fp16: float32 output holds the same values
                    assert np.array_equal(_host_encode(encoder, shard, np.float32, False),
                                          raw.astype(np.float32))
                if name in N.CONSTANT_FAMILIES:
                    row = N.constant_rows()[name].astype(raw_dtype)
                    assert np.all(_same(raw, np.broadcast_to(row, raw.shape))), name
                for dtype in (np.float16, np.float32):
                    got = _host_encode(encoder, shard, dtype, True)
                    keep = N.robust_mask(raw, dtype)
                    assert got.dtype == dtype
                    assert np.all(_same(got, N.expected(raw, dtype))[keep]), (name, dtype)
                    key = np.dtype(dtype).name
                    compared[key] = compared.get(key, 0) + int(keep.sum())
                    compared[key + " dropped"] = compared.get(key + " dropped", 0) + int((~keep).sum())
                got = _host_encode(encoder, shard, np.float64, True)
                want = N.expected(raw, np.float64)
                exact = N.exact_sum_rows(raw)
                assert np.all(_same(got, want)[exact]), (name, "float64, exact rows")
                assert np.all(np.abs(got - want) <= 2.0 ** -45 * np.abs(want)), (name, "float64")
                assert np.array_equal(np.signbit(got), np.signbit(want)), name
                compared["float64 exact rows"] = compared.get("float64 exact rows", 0) + int(exact.sum())
            print(f"{name} ({'full' if full_precision else 'half'}): {compared}")
        finally:
            encoder.close()
