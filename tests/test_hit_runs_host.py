"""Seeds from radius-search hits (gfy_hit_runs_mark, gfy_hit_runs_emit; align.hit_runs,
align.hit_cells, align.Runs): what needs no GPU.  The oracle of test_gpu_hit_runs.py on
hand-written patterns whose runs are listed here, every argument error of ``hit_runs`` and of the
C ABI before a device is touched, ``Runs.best`` and ``hit_cells`` against literal expectations,
and the three symbols declared where the others are."""
from __future__ import annotations

import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import hit_runs_oracle as oracle
import search_cases
from ginfinity_amd import _native as native
from ginfinity_amd import align, distance, seeds

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("gfy_hit_runs_workspace_bytes", "gfy_hit_runs_mark", "gfy_hit_runs_emit")

#: nine hits; in position order (0,0) (0,3) (1,1) (1,4) (2,2) (3,6) (5,0) (6,1) (6,6)
PATTERN = np.array([[1, 0, 0, 1, 0, 0, 0],
                    [0, 1, 0, 0, 1, 0, 0],
                    [0, 0, 1, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 1],
                    [0, 0, 0, 0, 0, 0, 0],
                    [1, 0, 0, 0, 0, 0, 0],
                    [0, 1, 0, 0, 0, 0, 1]], dtype=bool)
VALUES = np.arange(1, 10, dtype=np.float32)          # a hit's value: its position + 1


def _expect(pairs, cells, lengths, weights):
    return (np.array(pairs, dtype=np.int32).reshape(-1, 2),
            np.array(cells, dtype=np.int32).reshape(-1, 2),
            np.array(lengths, dtype=np.int32), np.array(weights, dtype=np.float32))


def test_oracle_on_one_record_a_side():
    hits = oracle.hits_of(PATTERN, VALUES)
    assert hits[0].tolist() == [0, 2, 4, 5, 6, 6, 7, 9]
    assert hits[1].tolist() == [0, 3, 1, 4, 2, 6, 0, 1, 6]
    want = _expect([(0, 0)] * 5, [(0, 0), (0, 3), (3, 6), (5, 0), (6, 6)], [3, 2, 1, 2, 1],
                   [1 + 3 + 5, 2 + 4, 6, 7 + 8, 9])
    oracle.assert_same(oracle.runs(*hits, (7,)), want)
    oracle.assert_same(oracle.runs(*hits, (7,), (7,)), want)
    oracle.assert_same(oracle.runs(*hits, (7,), min_length=2),
                       _expect([(0, 0)] * 3, [(0, 0), (0, 3), (5, 0)], [3, 2, 2], [9, 6, 15]))
    assert oracle.runs(*hits, (7,), min_length=4)[2].size == 0


def test_oracle_splits_runs_at_record_boundaries():
    """a: rows 0 | - | 1 2 | 3..6 (an empty record second); b: columns 0..3 | 4..6.  The run
    (0,0) (1,1) (2,2) breaks behind row 0; (0,3) (1,4) breaks between columns 3 and 4."""
    hits = oracle.hits_of(PATTERN, VALUES)
    want = _expect([(0, 0), (0, 0), (2, 0), (2, 1), (3, 1), (3, 0), (3, 1)],
                   [(0, 0), (0, 3), (0, 1), (0, 0), (0, 2), (2, 0), (3, 2)],
                   [1, 1, 2, 1, 1, 2, 1], [1, 2, 3 + 5, 4, 6, 7 + 8, 9])
    got = oracle.runs(*hits, (1, 0, 2, 4), (4, 3))
    oracle.assert_same(got, want)
    assert got[2].sum() == 9


def test_oracle_sums_in_float64_in_ascending_order():
    """1e8 + 1 - 1e8: float64 keeps the 1, float32 accumulation would lose it; the other order of
    a longer sum gives other bits."""
    hits = oracle.hits_of(np.eye(3, dtype=bool), np.array([1e8, 1.0, -1e8], dtype=np.float32))
    assert oracle.runs(*hits, (3,))[3].tolist() == [1.0]
    values = np.array([1e16, 1.0, 1.0, -1e16], dtype=np.float32)
    forward = oracle.runs(*oracle.hits_of(np.eye(4, dtype=bool), values), (4,))[3]
    assert forward.tolist() == [float(np.float32((np.float64(values[0]) + 1.0 + 1.0)
                                                 + np.float64(values[3])))]


def test_symbols_are_declared_loaded_and_exported():
    header = (ROOT / "include" / "gfy.h").read_text()
    lib = native.library()
    for name in SYMBOLS:
        assert f"{name}(" in header and name in native.SIGNATURES
        assert getattr(lib, name) is not None
    for name in ("hit_runs", "hit_cells", "Runs", "RunsWorkspace"):
        assert name in align.__all__ and hasattr(align, name)
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()
    assert "#define GFY_ABI_VERSION 4" in header


def test_seed_names_are_those_of_align_and_seeds_imports_no_align():
    moved = ("band_around", "hit_cells", "hit_runs", "Runs", "RunsWorkspace", "chain_runs",
             "Chains", "ChainsWorkspace")
    for name in moved:
        assert getattr(align, name) is getattr(seeds, name), name
    assert sorted(seeds.__all__) == sorted(moved)
    assert align.__all__ == [
        "local_align", "local_spans", "local_paths", "global_align", "global_paths",
        "path_cells", "AlignedPaths", "AlignWorkspace", "top_pairs", "band_around",
        "hit_cells", "hit_runs", "Runs", "RunsWorkspace", "chain_runs", "Chains",
        "ChainsWorkspace"]
    assert seeds.native is align.native is native      # what the refusal tests replace
    # a fresh interpreter; the package itself imports align, so seeds is loaded under a bare
    # package object: what sys.modules then holds is what seeds and its own imports ask for
    code = ("import sys, types; package = types.ModuleType('ginfinity_amd'); "
            "package.__path__ = ['ginfinity_amd']; sys.modules['ginfinity_amd'] = package; "
            "import ginfinity_amd.seeds; loaded = sorted(m for m in sys.modules "
            "if m.startswith('ginfinity_amd.')); print(*loaded)")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split() == ["ginfinity_amd._native", "ginfinity_amd.distance",
                                   "ginfinity_amd.seeds"]


def test_checked_integer_takes_integers_from_least_up_and_no_bool():
    refused = (0, -1, True, np.True_, 1.5, "2", None, np.float32(2))
    for value in refused:
        with pytest.raises(ValueError, match="^size must be a positive integer$"):
            distance._checked_integer(value, "size", 1)
    for value in refused[1:]:
        with pytest.raises(ValueError, match="^size must be a non-negative integer$"):
            distance._checked_integer(value, "size", 0)
    assert distance._checked_integer(0, "size", 0) == 0
    for least in (0, 1):
        for value, want in ((3, 3), (np.int64(3), 3), (2 ** 40, 2 ** 40)):
            got = distance._checked_integer(value, "size", least)
            assert type(got) is int and got == want


def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_hit_runs_workspace_bytes(1000)
    assert 8 * 1000 <= need <= 8 * 1000 + 256
    assert lib.gfy_hit_runs_workspace_bytes(0) >= 8

    def mark(offsets=p, n=70, indices=p, values=p, hits=1000, ptr_a=p, records_a=3, ptr_b=p,
             records_b=2, m=90, marks=p, status=p, ws=p, size=need):
        return lib.gfy_hit_runs_mark(offsets, n, indices, values, hits, ptr_a, records_a, ptr_b,
                                     records_b, m, marks, status, ws, size, None)

    def emit(offsets=p, n=70, indices=p, values=p, hits=1000, ptr_a=p, records_a=3, ptr_b=p,
             records_b=2, m=90, marks=p, slots=p, min_length=1, runs=10, pairs=p, cells=p,
             lengths=p, weights=p, status=p, ws=p, size=need):
        return lib.gfy_hit_runs_emit(offsets, n, indices, values, hits, ptr_a, records_a, ptr_b,
                                     records_b, m, marks, slots, min_length, runs, pairs, cells,
                                     lengths, weights, status, ws, size, None)

    shared = ("offsets", "indices", "values", "ptr_a", "ptr_b", "marks", "status", "ws")
    for call, holes in ((mark, shared),
                        (emit, shared + ("slots", "pairs", "cells", "lengths", "weights"))):
        for hole in holes:
            assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
            assert b"NULL" in lib.gfy_last_error()
        for sizes in (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(m=0), dict(m=1 << 31),
                      dict(hits=0), dict(hits=-5), dict(hits=1 << 31), dict(records_a=0),
                      dict(records_b=0), dict(records_a=native.GFY_PAIRWISE_RECORDS_MAX + 1),
                      dict(records_b=native.GFY_PAIRWISE_RECORDS_MAX + 1)):
            assert call(size=1 << 50, **sizes) == native.GFY_ERR_INVALID, sizes
        for short in (0, 1, need - 1):
            assert call(size=short) == native.GFY_ERR_WORKSPACE, short
            assert b"workspace" in lib.gfy_last_error()
    for min_length in (0, -1):
        assert emit(min_length=min_length) == native.GFY_ERR_INVALID
        assert b"min_length" in lib.gfy_last_error()
    for runs in (0, -1, 1001):
        assert emit(runs=runs) == native.GFY_ERR_INVALID
        assert b"runs" in lib.gfy_last_error()


def _hits(n=4, count=3):
    return distance.Hits(torch.tensor([0] + [count] * n, dtype=torch.int64),
                         torch.arange(count, dtype=torch.int32),
                         torch.zeros(count, dtype=torch.float32))


def test_python_refuses_bad_arguments_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = _hits()
    # not a triple
    for hits in (None, good.offsets, [good.offsets, good.indices, good.values], good[:2]):
        with pytest.raises(ValueError, match="distance.Hits"):
            align.hit_runs(hits, counts_a=[4])
    # dtypes and shapes
    with pytest.raises(ValueError, match="offsets must be a one-dimensional int64"):
        align.hit_runs(good._replace(offsets=good.offsets.to(torch.int32)), counts_a=[4])
    with pytest.raises(ValueError, match="offsets must be a one-dimensional int64"):
        align.hit_runs(good._replace(offsets=good.offsets.reshape(1, -1)), counts_a=[4])
    with pytest.raises(ValueError, match="indices must be a one-dimensional int32"):
        align.hit_runs(good._replace(indices=good.indices.to(torch.int64)), counts_a=[4])
    with pytest.raises(ValueError, match="indices must be a one-dimensional int32"):
        align.hit_runs(good._replace(indices=[0, 1, 2]), counts_a=[4])
    with pytest.raises(ValueError, match="values must be a one-dimensional float32"):
        align.hit_runs(good._replace(values=good.values.double()), counts_a=[4])
    with pytest.raises(ValueError, match="values must be a one-dimensional float32"):
        align.hit_runs(good._replace(values=np.zeros(3, dtype=np.float16)), counts_a=[4])
    with pytest.raises(ValueError, match="hits.indices has 3 entries, hits.values 2"):
        align.hit_runs(good._replace(values=good.values[:2]), counts_a=[4])
    with pytest.raises(ValueError, match="n \\+ 1 entries"):
        align.hit_runs(good._replace(offsets=good.offsets[:0]), counts_a=[])
    # min_length
    for min_length in (0, -1, True, 1.5, "2", None):
        with pytest.raises(ValueError, match="min_length"):
            align.hit_runs(good, counts_a=[4], min_length=min_length)
    # the counts: offsets.numel() == sum(counts_a) + 1, and the checks of record_scores
    for counts in ([2, 1], [2, 3], []):
        with pytest.raises(ValueError, match=r"counts_a sums to \d+ rows, hits has 4"):
            align.hit_runs(good, counts_a=counts)
    with pytest.raises(ValueError, match="record counts"):
        align.hit_runs(good, counts_a=[2, -2, 4])
    with pytest.raises(ValueError, match="record counts"):
        align.hit_runs(good, counts_a=[2.0, 2.0])
    with pytest.raises(ValueError, match="record counts"):
        align.hit_runs(good, counts_a=[4], counts_b=[5, -1])
    with pytest.raises(ValueError, match="record counts"):
        align.hit_runs(good, counts_a=[4], counts_b=[[5]])
    with pytest.raises(ValueError, match="at most"):
        align.hit_runs(good, counts_a=[4],
                       counts_b=np.ones(native.GFY_PAIRWISE_RECORDS_MAX + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="RunsWorkspace"):
        align.hit_runs(good, counts_a=[4], workspace=align.AlignWorkspace())
    # a sound call reaches the device, which this machine may not have: never a ValueError
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            align.hit_runs(good, counts_a=[4])


def test_runs_best_orders_by_length_then_weight_then_position():
    runs = align.Runs(torch.zeros((6, 2), dtype=torch.int32),
                      torch.zeros((6, 2), dtype=torch.int32),
                      torch.tensor([3, 5, 5, 1, 5, 3], dtype=torch.int32),
                      torch.tensor([9.0, 2.0, 7.0, 100.0, 2.0, 9.0], dtype=torch.float32))
    assert runs.best(6).tolist() == [2, 1, 4, 0, 5, 3]
    assert runs.best(2).tolist() == [2, 1] and runs.best(100).tolist() == [2, 1, 4, 0, 5, 3]
    assert runs.best(1).dtype == np.int64
    with_nan = runs._replace(weights=np.array([9.0, np.nan, 7.0, 100.0, -np.inf, 9.0],
                                              dtype=np.float32),
                             lengths=np.array([3, 5, 5, 1, 5, 3], dtype=np.int32))
    assert with_nan.best(3).tolist() == [2, 4, 1]
    empty = align.Runs(*(torch.zeros(shape, dtype=torch.int32) for shape in ((0, 2), (0, 2), 0)),
                       torch.zeros(0, dtype=torch.float32))
    assert empty.best(3).tolist() == []
    for k in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="k must be"):
            runs.best(k)


def test_runs_bands_is_band_around_of_the_cells():
    cells = torch.tensor([[0, 10], [7, 2], [3, 3]], dtype=torch.int32)
    runs = align.Runs(torch.zeros((3, 2), dtype=torch.int32), cells,
                      torch.ones(3, dtype=torch.int32), torch.ones(3, dtype=torch.float32))
    assert runs.bands(0).tolist() == [[10, 10], [-5, -5], [0, 0]]
    assert np.array_equal(runs.bands(4), align.band_around(cells, 4))
    assert runs.bands(4).tolist() == [[6, 14], [-9, -1], [-4, 4]]
    with pytest.raises(ValueError, match="half_width"):
        runs.bands(-1)


def test_hit_cells_against_literal_cells_and_the_docstring_recipe():
    counts_a, counts_b = [0, 4, 0, 6], [3, 4, 5]
    rows = np.array([0, 3, 4, 5, 9, 9])
    indices = np.array([2, 3, 0, 6, 7, 11], dtype=np.int32)
    q, r, cells = align.hit_cells(rows, indices, counts_a, counts_b)
    assert q.tolist() == [1, 1, 3, 3, 3, 3] and r.tolist() == [0, 1, 0, 1, 2, 2]
    assert cells.tolist() == [[0, 2], [3, 0], [0, 0], [1, 3], [5, 0], [5, 4]]
    for wrap in (lambda x: x, torch.from_numpy):
        q, r, cells = align.hit_cells(wrap(rows), wrap(indices.astype(np.int64)), counts_a,
                                      counts_b)
        want = search_cases.seeds_from_hits(wrap(rows), wrap(indices.astype(np.int64)),
                                            wrap(np.array(counts_a)), wrap(np.array(counts_b)))
        assert isinstance(cells, type(wrap(rows)))
        for got, expected in zip((q, r, cells), want):
            assert np.array_equal(np.asarray(got), np.asarray(expected))
    # counts_b defaults to counts_a; an index outside every record is -1 everywhere
    q, r, cells = align.hit_cells(np.array([1, 10, -1]), np.array([9, 2, 2]), [0, 4, 0, 6])
    assert q.tolist() == [1, -1, -1] and r.tolist() == [3, 1, 1]
    assert cells.tolist() == [[1, 5], [-1, 2], [-1, 2]]
    with pytest.raises(ValueError, match="both"):
        align.hit_cells(rows, torch.from_numpy(indices), counts_a)
    with pytest.raises(ValueError, match="one length"):
        align.hit_cells(rows, indices[:3], counts_a)
    with pytest.raises(ValueError, match="integer"):
        align.hit_cells(rows.astype(np.float32), indices, counts_a)
    with pytest.raises(ValueError, match="record counts"):
        align.hit_cells(rows, indices, [4, -1])
