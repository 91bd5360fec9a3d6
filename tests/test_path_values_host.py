"""The values along aligned paths (align.path_values, gfy_align_path_values): what needs no GPU.
The oracle of tests/path_values_oracle.py on hand-made matrices whose every number is checkable
by eye, its agreement with ``align_path_oracle.rescore``, every ``ValueError`` of the Python
function before a device is touched, and the symbol of the C ABI: every NULL pointer named, every
count out of range and ``gap_extend > gap_open`` refused without a device, the ABI still 4."""
from __future__ import annotations

import ctypes
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import align_path_oracle as PO
import path_values_oracle as VO
from ginfinity_amd import _native as native
from ginfinity_amd import align


def _bits(value) -> bytes:
    return np.asarray(value).tobytes()


def _f32(*values) -> np.ndarray:
    return np.array(values, dtype=np.float32)


#: C[i][j] = (8 i + j) / 64: dyadic, so that every sum below is exact and can be read off
C_EYE = (np.arange(5)[:, None] * 8 + np.arange(6)[None, :]).astype(np.float32) / np.float32(64)
NAN = np.float32(np.nan)


def test_a_path_whose_every_number_is_checkable_by_eye():
    # from (1, 0): match (1, 0), match (2, 1), two ops 1 (columns 2 and 3), match (3, 4)
    ops = [0, 0, 1, 1, 0]
    cosines, running, score, counts, total = VO.values_of(C_EYE, ops, (1, 0), 2.0, -0.25, 1.0, 0.5)
    assert _bits(cosines) == _bits(_f32(8 / 64, 17 / 64, NAN, NAN, 28 / 64))
    # s = 2 C - 0.25: 0, 0.28125, 0.625
    assert _bits(running) == _bits(_f32(0.0, 0.28125, -0.71875, -1.21875, -0.59375))
    assert _bits(score) == _bits(np.float32(-0.59375))
    assert counts == (3, 1, 0)
    assert total.dtype == np.float64 and total == (8 + 17 + 28) / 64


def test_a_gap_run_of_one_op_and_equal_open_and_extend():
    ops = [0, 2, 0, 1, 0]
    cosines, running, score, counts, _ = VO.values_of(C_EYE, ops, (0, 0), 1.0, 0.0, 0.75, 0.25)
    # cells (0, 0), then row 1 faces a gap, (2, 1), then column 2 faces a gap, (3, 3)
    assert _bits(cosines) == _bits(_f32(0.0, NAN, 17 / 64, NAN, 27 / 64))
    assert _bits(running) == _bits(_f32(0.0, -0.75, -0.75 + 17 / 64, -1.5 + 17 / 64,
                                        -1.5 + 44 / 64))
    assert counts == (3, 1, 1)
    # gap_open == gap_extend: a run of three costs three times the same
    _, running, score, counts, _ = VO.values_of(C_EYE, [0, 1, 1, 1], (0, 0), 1.0, 0.0, 0.5, 0.5)
    assert _bits(running) == _bits(_f32(0.0, -0.5, -1.0, -1.5)) and counts == (1, 1, 0)
    assert _bits(score) == _bits(np.float32(-1.5))


def test_alternating_gap_ops_are_each_a_new_run():
    ops = [1, 2, 1, 2, 2, 1]
    cosines, running, score, counts, total = VO.values_of(C_EYE, ops, (0, 0), 1.0, 0.0, 1.0, 0.25)
    assert np.isnan(cosines).all() and total == 0 and total.dtype == np.float64
    assert _bits(running) == _bits(_f32(-1.0, -2.0, -3.0, -4.0, -4.25, -5.25))
    assert counts == (0, 3, 2) and _bits(score) == _bits(np.float32(-5.25))


def test_an_empty_path():
    for start in ((-1, -1), (0, 0), (4, 5)):
        cosines, running, score, counts, total = VO.values_of(C_EYE, [], start, 1.0, 0.0, 1.0, 0.5)
        assert cosines.shape == running.shape == (0,)
        assert cosines.dtype == running.dtype == np.float32
        assert _bits(score) == _bits(np.float32(0)) and counts == (0, 0, 0)
        assert total == 0 and total.dtype == np.float64


def test_the_sum_starts_from_zero():
    """0 + (-0) is +0: a path of cosines that are all -0 (zero rows) sums to +0."""
    C = np.full((3, 3), -0.0, dtype=np.float32)
    cosines, _, _, counts, total = VO.values_of(C, [0, 0, 0], (0, 0), 1.0, -0.3, 1.0, 0.5)
    assert _bits(cosines) == _bits(_f32(-0.0, -0.0, -0.0)) and counts == (3, 0, 0)
    assert total.dtype == np.float64 and _bits(total) == _bits(np.float64(0.0))


def test_the_oracle_refuses_a_path_that_leaves_the_records():
    with pytest.raises(AssertionError, match="leaves the records"):
        VO.values_of(C_EYE, [0, 0], (4, 0), 1.0, 0.0, 1.0, 0.5)         # one row past A
    with pytest.raises(AssertionError, match="leaves the records"):
        VO.values_of(C_EYE, [0, 1, 1], (0, 4), 1.0, 0.0, 1.0, 0.5)      # one row past B


def test_the_last_running_value_is_rescore_and_the_sum_is_sequential():
    rng = np.random.default_rng(7)
    for number in range(60):
        lq, lr = int(rng.integers(1, 40)), int(rng.integers(1, 50))
        C = rng.uniform(-1, 1, size=(lq, lr)).astype(np.float32)
        scale, shift, go, ge = ((1.0, -0.3, 1.0, 0.25), (1.5, 0.2, 0.75, 0.5), (1.0, 0.0, 0.5, 0.5),
                                (-1.0, 0.25, 0.7, 0.0))[number % 4]
        S = (C * np.float32(scale)).astype(np.float32) + np.float32(shift)
        # a random walk down and right from a random start, gaps first on odd numbers
        i, j = int(rng.integers(0, lq)), int(rng.integers(0, lr))
        start, ops = (i, j), []
        while True:
            allowed = ([0] if i < lq and j < lr else []) + ([1] if j < lr else []) + \
                ([2] if i < lq else [])
            if not allowed or len(ops) == 70:
                break
            op = int(rng.choice(allowed))
            ops.append(op)
            i, j = i + (op != 1), j + (op != 2)
        cosines, running, score, counts, total = VO.values_of(C, ops, start, scale, shift, go, ge)
        assert _bits(score) == _bits(PO.rescore(S, ops, start, go, ge))
        assert _bits(score) == _bits(running[-1])
        cells = align.path_cells(np.array(ops), np.array(start))
        both = cells[(cells >= 0).all(axis=1)]
        assert _bits(cosines[np.array(ops) == 0]) == _bits(C[both[:, 0], both[:, 1]])
        by_hand = np.float64(0)
        for value in C[both[:, 0], both[:, 1]]:
            by_hand = by_hand + np.float64(value)
        assert _bits(total) == _bits(by_hand) and counts[0] == both.shape[0]
        kinds = np.array(ops)
        for op, got in ((1, counts[1]), (2, counts[2])):
            firsts = (kinds == op) & (np.concatenate(([0], kinds[:-1])) != op)
            assert got == int(firsts.sum())


# ---- the Python function, before a device is touched ---------------------------------------------

def _rows_f16(count):
    rng = np.random.default_rng(count)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


BASE = dict(counts_a=[2, 4], pairs=[[0, 1], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5)


def _paths(**changes):
    good = dict(starts=torch.tensor([[0, 0], [1, 1], [-1, -1]], dtype=torch.int32),
                ops=torch.tensor([0, 0, 0, 1, 0], dtype=torch.uint8),
                offsets=torch.tensor([0, 2, 5, 5], dtype=torch.int64))
    return SimpleNamespace(**{**good, **changes})


def test_every_value_error_is_raised_before_any_device_is_touched(monkeypatch):
    def no_device(*_):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(native, "library", no_device)
    monkeypatch.setattr(align, "_prepare", no_device)
    good = _rows_f16(6)
    bad = (
        ("ops", _paths(ops=torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32))),
        ("ops", _paths(ops=np.zeros(5, dtype=np.int8))),
        ("ops", _paths(ops=torch.zeros((5, 1), dtype=torch.uint8))),
        ("offsets", _paths(offsets=torch.tensor([0, 2, 5, 5], dtype=torch.int32))),
        ("offsets", _paths(offsets=torch.tensor([0, 2, 5], dtype=torch.int64))),
        ("offsets", _paths(offsets=torch.tensor([[0, 2, 5, 5]], dtype=torch.int64))),
        ("offsets must start at 0", _paths(offsets=torch.tensor([1, 2, 5, 5]))),
        ("end at ops.shape", _paths(offsets=torch.tensor([0, 2, 4, 4]))),
        ("end at ops.shape", _paths(offsets=np.array([0, 2, 5, 6], dtype=np.int64))),
        ("starts", _paths(starts=torch.zeros((3, 2), dtype=torch.int64))),
        ("starts", _paths(starts=torch.zeros((2, 2), dtype=torch.int32))),
        ("starts", _paths(starts=torch.zeros(6, dtype=torch.int32))),
        ("starts, ops and offsets", SimpleNamespace(ops=_paths().ops, offsets=_paths().offsets)),
        ("numpy array or a torch tensor", _paths(ops=[0, 0, 0, 1, 0])),
    )
    for text, paths in bad:
        with pytest.raises(ValueError, match=text):
            align.path_values(paths, good, **BASE)
    # the checks of the alignment calls come first and are the same texts
    for changes, text in (({"pairs": [[0, 2]]}, "out of range"),
                          ({"gap_extend": 1.5}, "gap_extend <= gap_open"),
                          ({"gap_open": float("inf")}, "gap_open must be a finite number"),
                          ({"match_scale": float("nan")}, "match_scale must be a finite number"),
                          ({"counts_a": [2, 5]}, "counts_a")):
        with pytest.raises(ValueError, match=text):
            align.path_values(_paths(), good, **{**BASE, **changes})
    for waves in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_waves"):
            align.path_values(_paths(), good, max_waves=waves, **BASE)
    with pytest.raises(TypeError):                                   # neither a band nor a box
        align.path_values(_paths(), good, band=(0, 1), **BASE)
    with pytest.raises(TypeError):
        align.path_values(_paths(), good, box=(0, 1, 0, 1), **BASE)


def test_good_paths_pass_the_checks(monkeypatch):
    """Good arguments get as far as the device: the first thing asked of it is the rows' copy,
    which stands in for it here."""
    class Reached(Exception):
        pass

    def reached(*_):
        raise Reached()
    monkeypatch.setattr(align, "_prepare", reached)
    monkeypatch.setattr(native, "library", reached)
    good = _rows_f16(6)
    as_numpy = SimpleNamespace(**{name: getattr(_paths(), name).numpy()
                                  for name in ("starts", "ops", "offsets")})
    aligned = align.AlignedPaths(torch.zeros(3), _paths().starts, _paths().starts, _paths().ops,
                                 _paths().offsets)
    for paths in (_paths(), as_numpy, aligned):
        with pytest.raises(Reached):
            align.path_values(paths, good, **BASE)
    assert callable(align.path_values) and align.path_values.__module__ == align.__name__
    assert align.PathValues._fields == ("cosines", "running", "scores", "matches", "gap_runs",
                                        "cosine_sums", "status", "offsets")


def test_mean_cosine_and_of_on_host_tensors():
    values = align.PathValues(torch.tensor([0.5, float("nan"), 0.25, 1.0]),
                              torch.tensor([0.5, -0.5, -0.25, 1.0]),
                              torch.tensor([-0.25, 1.0, 0.0]),
                              torch.tensor([2, 1, 0], dtype=torch.int32),
                              torch.tensor([[1, 0], [0, 0], [0, 0]], dtype=torch.int32),
                              torch.tensor([0.75, 1.0, 0.0], dtype=torch.float64),
                              torch.zeros(3, dtype=torch.int32),
                              torch.tensor([0, 3, 4, 4]))
    mean = values.mean_cosine()
    assert mean.dtype == torch.float64 and mean[:2].tolist() == [0.375, 1.0]
    assert bool(torch.isnan(mean[2]))
    cosines, running = values.of(1)
    assert cosines.tolist() == [1.0] and running.tolist() == [1.0]
    assert values.of(2)[0].shape == (0,) and values.of(0)[1].tolist() == [0.5, -0.5, -0.25]


# ---- the C ABI, without a device ---------------------------------------------------------------

def test_c_abi_declares_the_symbol_and_names_what_it_refuses():
    lib = native.library()
    void, i64 = ctypes.c_void_p, ctypes.c_int64
    header = (Path(__file__).resolve().parents[1] / "include" / "gfy.h").read_text()
    result, declared = native.SIGNATURES["gfy_align_path_values"]
    assert result is ctypes.c_int and lib.gfy_align_path_values is not None
    # what every alignment call starts with, then starts, op_ptr, ops, n_ops, the five outputs,
    # max_waves and the stream: no workspace
    assert list(declared) == list(native.SIGNATURES["gfy_align_local"][1])[:14] + \
        [void, void, void, i64] + [void] * 5 + [i64, void]
    assert "gfy_align_path_values(" in header and "No workspace" in header
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    assert "#define GFY_ABI_VERSION 4" in header
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced

    def call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p, P=10,
             scale=1.0, shift=0.0, go=1.0, ge=0.5, starts=p, op_ptr=p, ops=p, n_ops=100, cosine=p,
             running=p, score=p, counts=p, total=p, waves=0):
        return lib.gfy_align_path_values(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P,
                                         scale, shift, go, ge, starts, op_ptr, ops, n_ops, cosine,
                                         running, score, counts, total, waves, None)

    def refusal(text, **changes):
        assert call(**changes) == native.GFY_ERR_INVALID, changes
        message = lib.gfy_last_error()
        assert message.startswith(b"gfy_align_path_values: ") and text in message, (changes, message)

    for hole, text in {"a": b"a is NULL", "b": b"b is NULL", "ptr_a": b"ptr_a is NULL",
                       "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL",
                       "starts": b"starts is NULL", "op_ptr": b"op_ptr is NULL",
                       "ops": b"ops is NULL", "cosine": b"out_cosine is NULL",
                       "running": b"out_running is NULL", "score": b"out_score is NULL",
                       "counts": b"out_counts is NULL",
                       "total": b"out_cosine_sum is NULL"}.items():
        refusal(text, **{hole: None})
    for count in (0, -1, 2 ** 31 - 1, 2 ** 40):
        refusal(b"n = ", n=count)
        refusal(b"m = ", m=count)
        refusal(b"records_a = ", records_a=count)
        refusal(b"records_b = ", records_b=count)
    for count in (0, -1, 2 ** 31, 2 ** 40):
        refusal(b"P = ", P=count)
    refusal(b"n_ops = -1", n_ops=-1)
    refusal(b"max_waves = -1", waves=-1)
    refusal(b"gap_extend", go=1.0, ge=1.5)
    refusal(b"gap_extend", go=1.0, ge=-0.5)
    for name in ("scale", "shift", "go", "ge"):
        for value in (float("inf"), float("nan")):
            refusal(b"must be finite", **{name: value})
