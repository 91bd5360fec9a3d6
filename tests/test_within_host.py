"""Radius search (gfy_pairwise_within_count, gfy_pairwise_within_fill; distance.count_within,
distance.within): what needs no GPU.  The two functions and the C ABI refuse bad arguments
before a device is touched, the four symbols are declared where the others are, and
``Hits.rows`` is checked on hand-made offsets."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from ginfinity_amd import _native as native
from ginfinity_amd import distance

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("gfy_pairwise_within_workspace_bytes", "gfy_pairwise_within_chunks",
           "gfy_pairwise_within_count", "gfy_pairwise_within_fill")


def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_symbols_are_declared_loaded_and_exported():
    header = (ROOT / "include" / "gfy.h").read_text()
    lib = native.library()
    for name in SYMBOLS:
        assert name in native.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(lib, name) is not None
    for name in ("count_within", "within", "Hits", "TooManyHits", "WithinWorkspace"):
        assert name in distance.__all__ and hasattr(distance, name)
    assert issubclass(distance.TooManyHits, RuntimeError)
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_pairwise_within_workspace_bytes(300, 500)
    assert need >= 2 * 512 * 4 + 3 * 300 * 4    # (s, t), the a-terms, the bounds, the cursors
    assert lib.gfy_pairwise_within_chunks(257, 385) >= 1
    assert lib.gfy_pairwise_within_chunks(130, 1000) > 1

    def count(a=p, n=300, b=p, m=500, metric=native.GFY_L2, threshold=1.0, lo=None, hi=None,
              counts=p, ws=p, size=need):
        return lib.gfy_pairwise_within_count(a, n, b, m, metric, threshold, lo, hi, counts, ws,
                                             size, None)

    def fill(a=p, n=300, b=p, m=500, metric=native.GFY_COSINE, threshold=0.5, lo=None, hi=None,
             offsets=p, indices=p, values=p, status=p, ws=p, size=need):
        return lib.gfy_pairwise_within_fill(a, n, b, m, metric, threshold, lo, hi, offsets,
                                            indices, values, status, ws, size, None)

    for call, holes in ((count, ("a", "b", "counts", "ws")),
                        (fill, ("a", "b", "offsets", "indices", "values", "status", "ws"))):
        for hole in holes:
            assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
        assert call(metric=7) == native.GFY_ERR_INVALID
        assert b"metric" in lib.gfy_last_error()
        for n, m in ((0, 5), (5, 0), (-1, 5), (5, -1), (5, 1 << 31), (1 << 31, 5)):
            assert call(n=n, m=m, size=1 << 50) == native.GFY_ERR_INVALID, (n, m)
        for threshold in (float("nan"), float("inf"), float("-inf")):
            assert call(threshold=threshold) == native.GFY_ERR_INVALID, threshold
            assert b"threshold" in lib.gfy_last_error()
        for lo, hi in ((p, None), (None, p)):
            assert call(lo=lo, hi=hi) == native.GFY_ERR_INVALID
            assert b"skip_lo and skip_hi" in lib.gfy_last_error()
        for short in (0, 1, need - 1):
            assert call(size=short) == native.GFY_ERR_WORKSPACE, short
            assert b"workspace" in lib.gfy_last_error()


def test_python_refuses_bad_arguments_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(distance.native, "library", no_library)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good, other = _rows_f16(4), _rows_f16(5)
    lo = np.zeros(4, dtype=np.int32)
    for function in (distance.count_within, distance.within):
        # threshold: missing, bool, not a number, not finite in float32
        with pytest.raises(ValueError, match="threshold"):
            function(good)
        for threshold in (None, True, False, "1", [1.0], float("nan"), float("inf"),
                          float("-inf"), 1e39, -1e39, np.float64(1e300)):
            with pytest.raises(ValueError, match="threshold"):
                function(good, threshold=threshold)
        # the exclusion arguments exclude each other
        for combined in (dict(exclude_self=True, exclude_ranges=(lo, lo)),
                         dict(exclude_self=True, exclude_records=[4]),
                         dict(exclude_ranges=(lo, lo), exclude_records=[4])):
            with pytest.raises(ValueError, match="exclude each other"):
                function(good, threshold=1.0, **combined)
        # ranges of the wrong length, dtype or form
        with pytest.raises(ValueError, match=r"shape \(4,\)"):
            function(good, threshold=1.0, exclude_ranges=(lo[:3], lo[:3]))
        with pytest.raises(ValueError, match="int32"):
            function(good, threshold=1.0, exclude_ranges=(lo.astype(np.int64), lo))
        with pytest.raises(ValueError, match="pair"):
            function(good, threshold=1.0, exclude_ranges=lo)
        # counts that do not sum to n, or that are none; with a b of another size
        for counts in ([2, 1], [2, 3], []):
            with pytest.raises(ValueError, match=r"exclude_records sums to \d+ rows, a has 4"):
                function(good, threshold=1.0, exclude_records=counts)
        with pytest.raises(ValueError, match="record counts"):
            function(good, threshold=1.0, exclude_records=[2, -2, 4])
        with pytest.raises(ValueError, match="self-search"):
            function(good, other, threshold=1.0, exclude_records=[4])
        # dtype, shape, metric, workspace
        with pytest.raises(ValueError, match="float16"):
            function(good.float(), threshold=1.0)
        with pytest.raises(ValueError, match="float16"):
            function(good, good.float(), threshold=1.0)
        with pytest.raises(ValueError, match="128"):
            function(torch.zeros((4, 64), dtype=torch.float16), threshold=1.0)
        with pytest.raises(ValueError, match="metric"):
            function(good, threshold=1.0, metric="dot")
        with pytest.raises(ValueError, match="WithinWorkspace"):
            function(good, threshold=1.0, workspace=distance.TopKWorkspace())
    for max_hits in (0, -1, True, 1.5, "3"):
        with pytest.raises(ValueError, match="max_hits"):
            distance.within(good, threshold=1.0, max_hits=max_hits)


def test_threshold_is_rounded_to_float32_once():
    assert distance._checked_threshold(0.1) == float(np.float32(0.1))
    assert distance._checked_threshold(np.float32(0.3)) == float(np.float32(0.3))
    assert distance._checked_threshold(3) == 3.0
    assert distance._checked_threshold(-0.0) == 0.0


def test_hits_rows_on_hand_made_offsets():
    offsets = torch.tensor([0, 2, 2, 5, 6], dtype=torch.int64)
    hits = distance.Hits(offsets, torch.arange(6, dtype=torch.int32),
                         torch.zeros(6, dtype=torch.float32))
    rows = hits.rows()
    assert rows.dtype == torch.int64
    assert rows.tolist() == [0, 0, 2, 2, 2, 3]
    assert hits.offsets is offsets and hits.indices.numel() == hits.values.numel() == 6
    empty = distance.Hits(torch.zeros(4, dtype=torch.int64), torch.empty(0, dtype=torch.int32),
                          torch.empty(0, dtype=torch.float32))
    assert empty.rows().tolist() == [] and empty.rows().dtype == torch.int64
    none = distance.Hits(torch.zeros(1, dtype=torch.int64), torch.empty(0, dtype=torch.int32),
                         torch.empty(0, dtype=torch.float32))
    assert none.rows().numel() == 0


def test_too_many_hits_carries_the_total():
    error = distance.TooManyHits(12345, 100)
    assert error.total == 12345 and error.max_hits == 100
    assert "12345" in str(error)
