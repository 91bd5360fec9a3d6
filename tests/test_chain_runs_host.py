"""Chains of diagonal runs (gfy_chain_runs_link, gfy_chain_runs_emit; align.chain_runs,
align.Chains): what needs no GPU.  The oracle of test_gpu_chain_runs.py on hand-written runs whose
chains are written out in chain_runs_cases.py, every argument error of ``chain_runs`` and of the C
ABI before a device is touched, ``Chains.bands`` and ``Chains.best`` against literal expectations,
and the three symbols declared where the others are."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import chain_runs_cases as cases
import chain_runs_oracle as oracle
import hit_runs_oracle
from ginfinity_amd import _native as native
from ginfinity_amd import align
from ginfinity_amd import build as builder

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("gfy_chain_runs_workspace_bytes", "gfy_chain_runs_link", "gfy_chain_runs_emit")


@pytest.mark.parametrize("name", cases.CASES)
def test_oracle_on_hand_written_runs(name):
    entries, max_gap, max_shift, expected = cases.CASES[name]
    runs = cases.runs_of(entries)
    got = oracle.chains(*runs, max_gap, max_shift)
    oracle.assert_same(got, cases.chains_of(expected))
    oracle.assert_invariants(got, runs)
    # the key ascends strictly, and no run may precede itself or an earlier one
    keys = [(q, i, r, j) for q, r, i, j, _ in entries]
    assert keys == sorted(set(keys))
    reach = max_gap if max_shift is None else max_shift
    for t in range(len(entries)):
        for s in range(t, len(entries)):
            assert oracle.links(tuple(entries[s]), tuple(entries[t]), max_gap, reach) is None


def test_oracle_max_gap_zero_is_the_identity():
    matrix = np.random.default_rng(5).random((40, 50)) < 0.5
    runs = hit_runs_oracle.runs(*hit_runs_oracle.hits_of(matrix, seed=5), (0, 17, 23), (30, 0, 20))
    count = runs[2].size
    assert count > 100 and len({tuple(pair) for pair in runs[0].tolist()}) == 4
    pairs, starts, ends, diagonals, counts, lengths, weights, members = \
        oracle.chains(*runs, 0)
    assert np.array_equal(pairs, runs[0]) and np.array_equal(starts, runs[1])
    assert np.array_equal(ends, runs[1] + runs[2][:, None] - 1)
    assert np.array_equal(diagonals[:, 0], runs[1][:, 1] - runs[1][:, 0])
    assert np.array_equal(diagonals[:, 0], diagonals[:, 1])
    assert np.all(counts == 1) and np.array_equal(lengths, runs[2])
    assert weights.tobytes() == runs[3].tobytes()
    assert np.array_equal(members, np.arange(count))
    # a max_shift without a max_gap to use it changes nothing
    oracle.assert_same(oracle.chains(*runs, 0, 5), oracle.chains(*runs, 0))
    linked = oracle.chains(*runs, 2)
    assert linked[4].size < count
    oracle.assert_invariants(linked, runs)


def test_oracle_sums_in_float64_in_chain_order():
    """1e8 + 1 - 1e8: float64 keeps the 1, float32 accumulation would lose it; the other order of
    a longer sum gives other bits; a lone -0.0 keeps its sign."""
    entries = [(0, 0, 0, 0, 2), (0, 0, 3, 3, 2), (0, 0, 6, 6, 2), (0, 0, 9, 9, 2)]
    pairs, cells, lengths, _ = cases.runs_of(entries[:3])
    got = oracle.chains(pairs, cells, lengths, np.array([1e8, 1.0, -1e8], dtype=np.float32), 1)
    assert got[4].tolist() == [3] and got[6].tolist() == [1.0]
    values = np.array([1e16, 1.0, 1.0, -1e16], dtype=np.float32)
    got = oracle.chains(*cases.runs_of(entries)[:3], values, 1)
    assert got[6].tolist() == [float(np.float32((np.float64(values[0]) + 1.0 + 1.0)
                                                + np.float64(values[3])))]
    got = oracle.chains(pairs[:1], cells[:1], lengths[:1], np.array([-0.0], dtype=np.float32), 1)
    assert got[6].tobytes() == np.array([-0.0], dtype=np.float32).tobytes()


def test_symbols_are_declared_loaded_and_exported():
    header = (ROOT / "include" / "gfy.h").read_text()
    lib = native.library()
    for name in SYMBOLS:
        assert f"{name}(" in header and name in native.SIGNATURES
        assert getattr(lib, name) is not None
    for name in ("chain_runs", "Chains", "ChainsWorkspace"):
        assert name in align.__all__ and hasattr(align, name)
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()
    assert "#define GFY_ABI_VERSION 4" in header
    assert "chain_runs.hip" in builder.SOURCES


def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_chain_runs_workspace_bytes(1000)
    assert 64 * 1000 <= need <= 64 * 1000 + 256
    assert lib.gfy_chain_runs_workspace_bytes(0) >= 64

    def link(pairs=p, cells=p, lengths=p, weights=p, runs=1000, order=p, bounds=p, groups=7,
             max_gap=3, max_shift=3, plain=0, marks=p, status=p, ws=p, size=need):
        return lib.gfy_chain_runs_link(pairs, cells, lengths, weights, runs, order, bounds, groups,
                                       max_gap, max_shift, plain, marks, status, ws, size, None)

    def emit(pairs=p, cells=p, lengths=p, weights=p, runs=1000, marks=p, slots=p, chains=10,
             out_pairs=p, starts=p, ends=p, diagonals=p, counts=p, out_lengths=p, out_weights=p,
             members=p, status=p, ws=p, size=need):
        return lib.gfy_chain_runs_emit(pairs, cells, lengths, weights, runs, marks, slots, chains,
                                       out_pairs, starts, ends, diagonals, counts, out_lengths,
                                       out_weights, members, status, ws, size, None)

    shared = ("pairs", "cells", "lengths", "weights", "marks", "status", "ws")
    for call, holes in ((link, shared + ("order", "bounds")),
                        (emit, shared + ("slots", "out_pairs", "starts", "ends", "diagonals",
                                         "counts", "out_lengths", "out_weights", "members"))):
        for hole in holes:
            assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
            assert b"NULL" in lib.gfy_last_error()
        for runs in (0, -1, (1 << 31) - 1, 1 << 31):
            assert call(size=1 << 50, runs=runs) == native.GFY_ERR_INVALID, runs
            assert b"runs" in lib.gfy_last_error()
        for short in (0, 1, need - 1):
            assert call(size=short) == native.GFY_ERR_WORKSPACE, short
            assert b"workspace" in lib.gfy_last_error()
    for groups in (0, -1, 1001):
        assert link(groups=groups) == native.GFY_ERR_INVALID
        assert b"groups" in lib.gfy_last_error()
    for reach in (dict(max_gap=-1), dict(max_shift=-1), dict(max_gap=1 << 31),
                  dict(max_shift=1 << 40)):
        assert link(**reach) == native.GFY_ERR_INVALID, reach
        assert b"max_gap" in lib.gfy_last_error()
    for chains in (0, -1, 1001):
        assert emit(chains=chains) == native.GFY_ERR_INVALID
        assert b"chains" in lib.gfy_last_error()


def _runs(count=3):
    return align.Runs(torch.zeros((count, 2), dtype=torch.int32),
                      torch.stack([torch.arange(count, dtype=torch.int32) * 4] * 2, dim=1),
                      torch.full((count,), 2, dtype=torch.int32),
                      torch.ones(count, dtype=torch.float32))


def test_python_refuses_bad_arguments_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = _runs()
    # not a 4-tuple
    for runs in (None, good.pairs, list(good), good[:3], (*good, good.lengths)):
        with pytest.raises(ValueError, match="align.Runs"):
            align.chain_runs(runs, max_gap=1)
    # dtypes and shapes
    with pytest.raises(ValueError, match=r"pairs must be a int32 array of shape \(S, 2\)"):
        align.chain_runs(good._replace(pairs=good.pairs.to(torch.int64)), max_gap=1)
    with pytest.raises(ValueError, match=r"pairs must be a int32 array of shape \(S, 2\)"):
        align.chain_runs(good._replace(pairs=good.pairs.reshape(2, 3)), max_gap=1)
    with pytest.raises(ValueError, match=r"cells must be a int32 array of shape \(S, 2\)"):
        align.chain_runs(good._replace(cells=good.cells[:, 0]), max_gap=1)
    with pytest.raises(ValueError, match=r"cells must be a int32 array of shape \(S, 2\)"):
        align.chain_runs(good._replace(cells=good.cells.tolist()), max_gap=1)
    with pytest.raises(ValueError, match=r"lengths must be a int32 array of shape \(S,\)"):
        align.chain_runs(good._replace(lengths=good.lengths.to(torch.int16)), max_gap=1)
    with pytest.raises(ValueError, match=r"lengths must be a int32 array of shape \(S,\)"):
        align.chain_runs(good._replace(lengths=good.lengths.reshape(-1, 1)), max_gap=1)
    with pytest.raises(ValueError, match=r"weights must be a float32 array of shape \(S,\)"):
        align.chain_runs(good._replace(weights=good.weights.double()), max_gap=1)
    with pytest.raises(ValueError, match=r"weights must be a float32 array of shape \(S,\)"):
        align.chain_runs(good._replace(weights=np.ones(3, dtype=np.float16)), max_gap=1)
    with pytest.raises(ValueError, match="runs.weights has 2 entries, runs.lengths 3"):
        align.chain_runs(good._replace(weights=good.weights[:2]), max_gap=1)
    with pytest.raises(ValueError, match="runs.pairs has 4 entries, runs.lengths 3"):
        align.chain_runs(good._replace(pairs=_runs(4).pairs), max_gap=1)
    # S >= 2^31 - 1: a view of one element, no memory behind it
    huge = (torch.zeros(1, dtype=torch.int32).expand(2 ** 31 - 1, 2),) * 2 + \
        (torch.zeros(1, dtype=torch.int32).expand(2 ** 31 - 1),
         torch.zeros(1, dtype=torch.float32).expand(2 ** 31 - 1))
    with pytest.raises(ValueError, match="fewer than 2\\^31 - 1 runs"):
        align.chain_runs(huge, max_gap=1)
    # the two integers
    for reach in (-1, True, False, 1.0, "2", None, np.float32(2)):
        with pytest.raises(ValueError, match="max_gap must be a non-negative integer"):
            align.chain_runs(good, max_gap=reach)
        if reach is not None:
            with pytest.raises(ValueError, match="max_shift must be a non-negative integer"):
                align.chain_runs(good, max_gap=1, max_shift=reach)
    with pytest.raises(TypeError):
        align.chain_runs(good)                       # max_gap has no default
    for workspace in (align.RunsWorkspace(), align.AlignWorkspace(), object()):
        with pytest.raises(ValueError, match="ChainsWorkspace"):
            align.chain_runs(good, max_gap=1, workspace=workspace)
    with pytest.raises(ValueError, match="plain_scan"):
        align.ChainsWorkspace(plain_scan=1)
    # a sound call reaches the device, which this machine may not have: never a ValueError
    if not torch.cuda.is_available():
        for reach in (0, 1, np.int64(3), 2 ** 40):
            with pytest.raises(RuntimeError):
                align.chain_runs(good, max_gap=reach)


def _chains(diagonals, lengths, weights):
    count = len(lengths)
    zeros = torch.zeros((count, 2), dtype=torch.int32)
    return align.Chains(zeros, zeros, zeros,
                        torch.tensor(diagonals, dtype=torch.int32).reshape(-1, 2),
                        torch.ones(count, dtype=torch.int32),
                        torch.tensor(lengths, dtype=torch.int32),
                        torch.tensor(weights, dtype=torch.float32),
                        torch.arange(count, dtype=torch.int32))


def test_chains_bands_widen_the_diagonals_of_a_chain():
    chains = _chains([(10, 13), (-5, -5), (-2, 7)], [1, 1, 1], [1.0, 1.0, 1.0])
    assert chains.bands(0).tolist() == [[10, 13], [-5, -5], [-2, 7]]
    assert chains.bands(4).tolist() == [[6, 17], [-9, -1], [-6, 11]]
    assert chains.bands(4).dtype == np.int32 and chains.bands(np.int64(1)).shape == (3, 2)
    # what the aligners take: integers (lo, hi) with lo <= hi
    assert np.array_equal(align._checked_band(chains.bands(2), 3), chains.bands(2))
    wide = chains.bands(10 ** 12)
    assert np.all(wide[:, 0] <= -native.GFY_ALIGN_ROWS_MAX)
    assert np.all(wide[:, 1] >= native.GFY_ALIGN_ROWS_MAX)
    assert _chains([], [], []).bands(3).shape == (0, 2)
    for half_width in (-1, True, 1.5, None):
        with pytest.raises(ValueError, match="half_width"):
            chains.bands(half_width)


def test_chains_best_is_the_rule_of_runs_best():
    lengths, weights = [3, 5, 5, 1, 5, 3], [9.0, 2.0, 7.0, 100.0, 2.0, 9.0]
    chains = _chains([(0, 0)] * 6, lengths, weights)
    assert chains.best(6).tolist() == [2, 1, 4, 0, 5, 3]
    assert chains.best(2).tolist() == [2, 1] and chains.best(100).tolist() == [2, 1, 4, 0, 5, 3]
    assert chains.best(1).dtype == np.int64
    with_nan = _chains([(0, 0)] * 6, lengths, [9.0, np.nan, 7.0, 100.0, -np.inf, 9.0])
    assert with_nan.best(3).tolist() == [2, 4, 1]
    runs = align.Runs(chains.pairs, chains.starts, chains.lengths, with_nan.weights)
    assert runs.best(6).tolist() == with_nan.best(6).tolist()        # one rule, one code
    assert _chains([], [], []).best(3).tolist() == []
    for k in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="k must be"):
            chains.best(k)
