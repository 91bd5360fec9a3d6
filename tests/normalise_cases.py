"""Models whose head output sits where the float64 normalise can go wrong — fp16 subnormals, the
subnormal grid of the output, the tie at half the smallest subnormal, the 1e-12 clamp, -0.0, rows
near 65504, rows with one element — and the float64 side of the tests that use them
(tests/test_normalise_cases_host.py, tests/test_gpu_normalise_values.py).  numpy only.

The contract: an embedding row is ``o / max(|o|, 1e-12)`` in float64, rounded ONCE to the output
dtype.  Seven implementations serve it ("The value range of the normalise"), five of
them through an fp32 shortcut with a float64 path behind it.

    head_families(config)     seeded state dicts, only head.2.weight / head.2.bias transformed
    head_outputs(...)         the oracle's raw head output of every family on one shard
    expected(raw, dtype)      the reference's recipe on raw head outputs
    robust_mask(raw, dtype)   the values whose bytes do not depend on the last ulps of the norm
    exact_sum_rows(raw)       the rows whose sum of squares is exact in float64 in any order
    emulate_bracket(raw)      the fp16 shortcut of the layer kernels' fused head and of k_head_d
    emulate_window(raw)       the fp16 shortcut of the stand-alone head (scale_to_f16)
"""
from __future__ import annotations

import numpy as np

DIM = 128
SEED = 11
NORM_FLOOR = 1e-12
F16_TINY = 2.0 ** -14    # the smallest normal float16
F16_MAX = 65504.0

#: seeded random head.2, weight and bias scaled by a power of two (``ladder``: column c by
#: 2^-(c mod 27)) — a transformed weight is an exact fp32
RANDOM_FAMILIES = {"plain": 0, "tiny14": -14, "tiny20": -20, "tiny24": -24, "huge12": 12,
                   "ladder": None}
LADDER_PERIOD = 27


def constant_rows() -> dict[str, np.ndarray]:
    """The rows of the constant families, float16 ``[128]``: head.2.weight = 0 and this row as
    the bias make every node's head output this row exactly."""
    rows = {name: np.zeros(DIM, dtype=np.float64) for name in
            ("zero", "one_tiny", "one_huge", "three_four", "below_tie", "all_max")}
    rows["one_tiny"][77] = 2.0 ** -24            # the quotient is exactly 1
    rows["one_huge"][8] = -F16_MAX               # ... exactly -1
    rows["three_four"][[0, 127]] = (3.0, 4.0)    # 0.6 and 0.8
    rows["below_tie"][[1, 40, 64, 126]] = 1.0    # |o| = 2 (1 + 2^-51): 2^-24 / |o| lies just
    rows["below_tie"][15] = 2.0 ** -24           # below the tie at 2^-25 and rounds to 0
    rows["all_max"][:] = F16_MAX                 # |o|^2 = 2^17 2047^2 is exact, 1 / sqrt(128)
    out = {name: row.astype(np.float16) for name, row in rows.items()}
    assert all(np.array_equal(out[name].astype(np.float64), rows[name]) for name in rows)
    return out


CONSTANT_FAMILIES = tuple(constant_rows())
FAMILIES = tuple(RANDOM_FAMILIES) + CONSTANT_FAMILIES


def head_families(config, seed: int = SEED) -> dict[str, dict[str, np.ndarray]]:
    """``{family: state dict}``: ``weights.random_state(config, seed)`` with head.2.weight and
    head.2.bias transformed, every other tensor shared."""
    from ginfinity_amd.weights import random_state
    base = random_state(config, seed=seed)
    weight, bias = base["head.2.weight"], base["head.2.bias"]
    assert weight.shape == (DIM, config.hidden) and bias.shape == (DIM,)

    def with_head(new_weight, new_bias):
        state = dict(base)
        state["head.2.weight"] = np.ascontiguousarray(new_weight, dtype=np.float32)
        state["head.2.bias"] = np.ascontiguousarray(new_bias, dtype=np.float32)
        return state

    out = {}
    for name, power in RANDOM_FAMILIES.items():
        factor = (2.0 ** -(np.arange(DIM) % LADDER_PERIOD) if power is None
                  else np.full(DIM, 2.0 ** power))
        state = with_head(weight * factor[:, None].astype(np.float32),
                          bias * factor.astype(np.float32))
        assert np.array_equal(state["head.2.weight"].astype(np.float64),
                              weight.astype(np.float64) * factor[:, None]), name
        assert np.array_equal(state["head.2.bias"].astype(np.float64),
                              bias.astype(np.float64) * factor), name
        out[name] = state
    for name, row in constant_rows().items():
        out[name] = with_head(np.zeros_like(weight), row.astype(np.float32))
    return out


def head_outputs(states, config, shard) -> dict[str, np.ndarray]:
    """``{family: raw}``: the oracle's fp16-model head output ``o`` (float16 ``[nodes, 128]``) of
    every state dict on ``shard``.  The families share everything below head.2, so the forward
    runs once."""
    from oracle import gine_numpy as G
    first = next(iter(states.values()))
    weights = G.Weights.from_state_dict(first, layers=config.layers,
                                        residual=config.residual).half()
    trace: dict = {}
    G.forward_f16(weights, shard.node_features, shard.edge_index, shard.edge_types, trace)
    hidden = G.up(trace["head.t"])
    out = {}
    for name, state in states.items():
        weight = state["head.2.weight"].astype(np.float16).astype(np.float32)
        bias = state["head.2.bias"].astype(np.float16).astype(np.float32)
        out[name] = G.R(hidden @ weight.T + bias)
    return out


# ---- the float64 side ----------------------------------------------------------------------------

def _wide(raw: np.ndarray) -> np.ndarray:
    raw = np.asarray(raw)
    assert raw.dtype in (np.float16, np.float32) and raw.ndim == 2
    return raw.astype(np.float32).astype(np.float64)


def denominator(raw: np.ndarray, ulps: int = 0) -> np.ndarray:
    """``max(|o|, 1e-12)`` per row in float64, moved by ``ulps`` float64 steps."""
    e = _wide(raw)
    den = np.maximum(np.sqrt((e * e).sum(axis=1)), NORM_FLOOR)
    return (den.view(np.int64) + np.int64(ulps)).view(np.float64)       # den > 0


def expected(raw: np.ndarray, dtype, ulps: int = 0) -> np.ndarray:
    """The reference's recipe: raw rows through fp32 to float64, ``sqrt((e * e).sum(axis=1))``
    clamped at 1e-12, one division, ONE ``astype``."""
    return (_wide(raw) / denominator(raw, ulps)[:, None]).astype(dtype)


def _bytes(values: np.ndarray) -> np.ndarray:
    return values.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[values.dtype.itemsize])


def robust_mask(raw: np.ndarray, dtype) -> np.ndarray:
    """bool like ``raw``: the values whose bytes stay the same when the denominator moves by
    -2 .. +2 float64 ulps — what does not depend on things the reference leaves open (the order
    of the sum of squares, ``o * (1 / den)`` against ``o / den``)."""
    want = _bytes(expected(raw, dtype))
    keep = np.ones(want.shape, dtype=bool)
    for ulps in (-2, -1, 1, 2):
        keep &= _bytes(expected(raw, dtype, ulps)) == want
    return keep


def exact_sum_rows(raw: np.ndarray) -> np.ndarray:
    """bool per row: the sum of squares is exact in float64 whatever the order of the additions.
    Python integers: every element is an integer k times one power of two per row (2^-24 for
    float16); with u the lowest set bit of any k, every square is a multiple of u^2, so every
    partial sum is one too, and all of them are exact when the whole sum is below 2^53 u^2."""
    e = _wide(raw)
    mantissa, exponent = np.frexp(e)
    digits = 11 if np.asarray(raw).dtype == np.float16 else 24
    whole = np.round(mantissa * 2.0 ** digits).astype(np.int64)          # |whole| <= 2^digits
    low = np.where(e != 0, exponent - digits, np.iinfo(np.int32).max).min(axis=1)
    shift = np.where(e != 0, exponent - digits - low[:, None], 0)
    out = np.ones(e.shape[0], dtype=bool)
    for r, (ints, shifts) in enumerate(zip(whole.tolist(), shift.tolist())):
        total, union = 0, 0
        for k, s in zip(ints, shifts):
            k <<= s
            total += k * k
            union |= abs(k)
        if total:
            unit = union & -union
            out[r] = total < (unit * unit) << 53
    return out


def float64_path(raw: np.ndarray) -> np.ndarray:
    """What both shortcuts fall back to: ``(double) o * inv`` with ``inv = 1 / den``, rounded once
    to float16 (csrc/gine_f16.hip, f64_to_f16_rne)."""
    inv = 1.0 / denominator(raw)
    return (_wide(raw) * inv[:, None]).astype(np.float16)


def _inv32(raw: np.ndarray) -> np.ndarray:
    return (1.0 / denominator(raw)).astype(np.float32).astype(np.float64)[:, None]


def emulate_bracket(raw: np.ndarray):
    """``(redo, fast)``: the shortcut of the fused head of every layer kernel and of k_head_d
    (csrc/gine_layer.inc).  Two fp32 products with ``inv (1 + 2^-22)`` and ``inv (1 - 2^-22)``
    bracket the float64 product; where their float16 roundings differ (``redo``) the value goes
    to the float64 path, elsewhere ``fast`` is the answer.  A float64 product rounded to fp32 is
    ONE rounding: 11 bits times 24 bits, and 24 bits times 1 + 2^-22, are exact in float64."""
    assert np.asarray(raw).dtype == np.float16
    e, inv = _wide(raw), _inv32(raw)
    inv_up = (inv * (1.0 + 2.0 ** -22)).astype(np.float32).astype(np.float64)    # fmaf
    inv_dn = (inv * (1.0 - 2.0 ** -22)).astype(np.float32).astype(np.float64)
    up = (e * inv_up).astype(np.float32).astype(np.float16)     # v_fma_mix_f32, v_cvt_pk_f16_f32
    dn = (e * inv_dn).astype(np.float32).astype(np.float16)
    return _bytes(up) != _bytes(dn), up


def emulate_window(raw: np.ndarray):
    """``(redo, fast)``: the shortcut of the stand-alone head for fp16 output (csrc/gine_f16.hip,
    scale_to_f16).  One fp32 product; a value within 4 fp32 ulps of a float16 rounding tie, or
    with ``0 < |q| < 2^-14``, goes to the float64 path."""
    assert np.asarray(raw).dtype == np.float16
    q = (_wide(raw) * _inv32(raw)).astype(np.float32)
    bits = q.view(np.uint32)
    near_tie = ((bits & np.uint32(0x1FFF)) - np.uint32(0xFFC)) <= np.uint32(8)
    below_normal = ((bits & np.uint32(0x7FFFFFFF)) - np.uint32(1)) < np.uint32(0x387FFFFF)
    return near_tie | below_normal, q.astype(np.float16)


def through_shortcut(raw: np.ndarray, emulate) -> np.ndarray:
    """The float16 rows an emulated shortcut gives: its fast answer, the float64 path on redo."""
    redo, fast = emulate(raw)
    return np.where(redo, float64_path(raw), fast)


def counts(raw: np.ndarray) -> dict[str, int]:
    """What a float16 raw head output holds of the edges: values on the bracket's redo path and
    in the window, fp16-subnormal inputs, outputs on the subnormal grid, -0.0 inputs."""
    size, out = np.abs(_wide(raw)), np.abs(expected(raw, np.float16).astype(np.float64))
    return {"bracket_redo": int(emulate_bracket(raw)[0].sum()),
            "window_redo": int(emulate_window(raw)[0].sum()),
            "subnormal_inputs": int(((size > 0) & (size < F16_TINY)).sum()),
            "subnormal_outputs": int(((out > 0) & (out < F16_TINY)).sum()),
            "negative_zero_inputs": int((np.signbit(raw) & (size == 0)).sum())}
