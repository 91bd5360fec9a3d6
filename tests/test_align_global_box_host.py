"""Global and query-in-target alignment inside a box of rows per pair (the ``box`` of
align.global_align and global_paths; gfy_align_global_box, gfy_align_global_trace_box): what needs
no GPU.  The oracle of tests/align_global_box_oracle.py against itself on random small matrices
(a covering box is the call without one, re-scoring the ops gives the score, global <= within <=
local in one box, widening the b-side never lowers a ``within`` score), an empty box and a single
cell, the premise of the two-region case of tests/test_gpu_align_global_box.py, every
``ValueError`` of the box before a device is touched, and the two symbols of the C ABI."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import align_box_oracle as XO
import align_global_box_oracle as GXO
import align_global_oracle as GO
import align_path_oracle as PO
from ginfinity_amd import _native as native
from ginfinity_amd import align

MODES = (False, True)
#: (gap_open, gap_extend): dyadic and not, linear (open == extend), free extension, free gaps
GAPS = ((1.0, 0.25), (1.3, 0.7), (0.5, 0.5), (0.75, 0.0), (0.0, 0.0))
REGION_BOX = (20, 138, 27, 145)        # from the first planted cell of XO.two_regions to the last


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


def _same(got, want, where=None):
    assert (_bits(got[0]), tuple(got[1]), tuple(got[2])) == \
        (_bits(want[0]), tuple(want[1]), tuple(want[2])), (where, got[:3], want[:3])
    assert got[3].tobytes() == want[3].tobytes(), where


def _matrices(seed, count, most_q, most_r):
    """Random float32 substitution matrices, rounding in every sum, some with a planted diagonal."""
    rng = np.random.default_rng(seed)
    for number in range(count):
        lq, lr = int(rng.integers(1, most_q + 1)), int(rng.integers(1, most_r + 1))
        S = rng.standard_normal((lq, lr)).astype(np.float32) - np.float32(0.3)
        if number % 2:
            shift = int(rng.integers(0, lr))
            for i in range(lq):
                if i + shift < lr:
                    S[i, i + shift] += np.float32(1.5)
        yield rng, S, GAPS[number % len(GAPS)]


def _random_box(rng, lq, lr):
    i_lo, j_lo = int(rng.integers(0, lq)), int(rng.integers(0, lr))
    return i_lo, int(rng.integers(i_lo, lq)), j_lo, int(rng.integers(j_lo, lr))


# consequence 1
def test_a_covering_box_equals_the_oracle_without_a_box():
    for rng, S, gaps in _matrices(1, 40, 40, 60):
        lq, lr = S.shape
        for within in MODES:
            want = GO.path_of(S, *gaps, within)
            for box in (XO.covering(lq, lr), (-3, lq + 5, -1, lr), (-4096, 4096, -4096, 4096)):
                _same(GXO.box_path_of(S, *gaps, box, within), want, (S.shape, gaps, box, within))
                score, end = GXO.box_score_of(S, *gaps, box, within)
                assert (_bits(score), end) == (_bits(want[0]), want[2])


# consequences 3 and 4, and the table of results
def test_the_ops_add_up_to_the_score_and_global_within_local_are_ordered_in_one_box():
    checked = 0
    for rng, S, gaps in _matrices(2, 60, 40, 60):
        lq, lr = S.shape
        box = _random_box(rng, lq, lr)
        i_lo, i_hi, j_lo, j_hi = box
        found = {}
        for within in MODES:
            score, start, end, ops = found[within] = GXO.box_path_of(S, *gaps, box, within)
            where = (S.shape, gaps, box, within)
            assert _bits(PO.rescore(S, ops, start, *gaps)) == _bits(score), where
            assert start[0] == i_lo and end[0] == i_hi and j_lo <= end[1] <= j_hi, where
            assert np.count_nonzero(ops != 1) == i_hi - i_lo + 1, where
            assert np.count_nonzero(ops != 2) == end[1] - start[1] + 1, where
            if not within:
                assert start == (i_lo, j_lo) and end == (i_hi, j_hi), where
            elif not np.any(ops != 2):
                assert start[1] == end[1] + 1, where               # no b-row is consumed
            cells = align.path_cells(ops, np.array(start))
            both = cells[(cells >= 0).all(axis=1)]
            if both.size:
                assert both[:, 0].min() >= i_lo and both[:, 0].max() <= i_hi, where
                assert both[:, 1].min() >= j_lo and both[:, 1].max() <= j_hi, where
            checked += 1
        local = XO.box_path_of(S, *gaps, box)[0]
        assert found[False][0] <= found[True][0] <= local, (S.shape, gaps, box)
    assert checked == 120


# consequence 6
def test_widening_the_b_side_never_lowers_a_within_score():
    steps = strict = 0
    for rng, S, gaps in _matrices(3, 60, 40, 60):
        lq, lr = S.shape
        i_lo, i_hi, j_lo, j_hi = _random_box(rng, lq, lr)
        before = None
        while True:
            score = GXO.box_score_of(S, *gaps, (i_lo, i_hi, j_lo, j_hi), True)[0]
            assert before is None or score >= before, (S.shape, gaps, (i_lo, i_hi, j_lo, j_hi))
            strict += before is not None and score > before
            steps += before is not None
            before = score
            if (j_lo, j_hi) == (0, lr - 1):
                break
            j_lo = max(j_lo - int(rng.integers(0, 9)), 0)
            j_hi = min(j_hi + int(rng.integers(0, 9)), lr - 1)
        assert _bits(before) == _bits(GXO.box_score_of(S, *gaps, (i_lo, i_hi, 0, lr - 1), True)[0])
    assert steps > 200 and strict > 50, (steps, strict)


def test_a_box_that_holds_no_cell_and_a_single_cell():
    S = np.full((5, 7), 0.5, dtype=np.float32)
    for within in MODES:
        for box in ((5, 9, 0, 6), (-9, -1, 0, 6), (0, 4, 7, 7), (0, 4, -4096, -1), (4096, 4096, 0, 0)):
            score, start, end, ops = GXO.box_path_of(S, 1.0, 0.5, box, within)
            assert _bits(score) == _bits(0) and start == end == (-1, -1) and ops.size == 0
            assert GXO.box_score_of(S, 1.0, 0.5, box, within)[1] == (-1, -1)
        score, start, end, ops = GXO.box_path_of(S, 1.0, 0.5, (3, 3, 2, 2), within)
        assert _bits(score) == _bits(0.5) and start == end == (3, 2) and ops.tolist() == [0]
    # a cell that is worth less than its gaps: global pays for both rows, within only for A's
    S = np.full((5, 7), -4.0, dtype=np.float32)
    score, start, end, ops = GXO.box_path_of(S, 1.0, 0.5, (3, 3, 2, 2), False)
    assert _bits(score) == _bits(-2.0) and start == end == (3, 2) and sorted(ops.tolist()) == [1, 2]
    score, start, end, ops = GXO.box_path_of(S, 1.0, 0.5, (3, 3, 2, 2), True)
    assert _bits(score) == _bits(-1.0) and ops.tolist() == [2] and end == (3, 2)
    assert start == (3, 3)                                          # end_j + 1: no b-row consumed


def test_the_premise_of_the_two_region_pair():
    """In the box from the first planted cell to the last, the global and the ``within`` path hold
    BOTH planted regions, linker included, and the local one only the stronger."""
    case = XO.two_regions()
    S, (first, second) = case["S"], case["plants"]
    go, ge = XO.REGION_PARAMETERS[2:]
    assert REGION_BOX == (int(first[0, 0]), int(second[-1, 0]), int(first[0, 1]), int(second[-1, 1]))
    for within in MODES:
        score, start, end, ops = GXO.box_path_of(S, go, ge, REGION_BOX, within)
        cells = align.path_cells(ops, np.array(start))
        assert XO.holds(cells, first) and XO.holds(cells, second), within
        assert _bits(score) == _bits(-6.75) and ops.size == 121 and np.count_nonzero(ops) == 4
        assert start == (20, 27) and end == (138, 145)
        assert _bits(PO.rescore(S, ops, start, go, ge)) == _bits(score)
    score, start, end, ops = XO.box_path_of(S, go, ge, REGION_BOX)
    cells = align.path_cells(ops, np.array(start))
    assert _bits(score) == _bits(12.5) and end == (69, 76)
    assert XO.holds(cells, first[:50 - 20 + 1]) and not XO.holds(cells, second)
    # the whole records charge the flanks as well: another path, not this one shifted
    whole = GO.path_of(S, go, ge, False)
    assert whole[0] < np.float32(-6.75) and whole[3].size != 121


def _rows_f16(count):
    rng = np.random.default_rng(count)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


BASE = dict(counts_a=[2, 4], pairs=[[0, 1], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5)


@pytest.mark.parametrize("name", ("global_align", "global_paths"))
def test_a_bad_box_is_the_value_error_of_local_align_before_any_device_is_touched(name, monkeypatch):
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(native, "library", no_library)
    function = getattr(align, name)
    good = _rows_f16(6)
    bad = ([[0.0, 1.0, 0.0, 1.0]] * 3, np.zeros((3, 4)), (0.0, 1.0, 0.0, 1.0), "0101",
           (0, 1, True, 1), np.zeros((3, 4), dtype=bool), [[0, 1, 0, 1]] * 2, [[0, 1]] * 3,
           [0, 1, 2], 5, [], [[0, 1, 0, 1], [3, 2, 0, 0], [9, 1, 0, 0]], (0, 5, 1, 0),
           torch.tensor([[0, 0, 0, 0], [-1, 1, -1, 1], [5000, 4999, 0, 0]]))
    for box in bad:
        with pytest.raises(ValueError) as wanted:
            align.local_align(good, box=box, **BASE)
        assert "box" in str(wanted.value)
        for within in MODES:
            with pytest.raises(ValueError) as got:
                function(good, box=box, within=within, **BASE)
            assert str(got.value) == str(wanted.value)
    with pytest.raises(ValueError, match=r"box of pair 1 = \(3, 2, 0, 0\): i_lo <= i_hi and j_lo"):
        function(good, box=[[0, 1, 0, 1], [3, 2, 0, 0], [9, 1, 0, 0]], **BASE)
    # the other checks come first and are unchanged by a box
    with pytest.raises(ValueError, match="out of range"):
        function(good, box=(0, 1, 0, 1), **{**BASE, "pairs": [[0, 2]]})
    with pytest.raises(ValueError, match="within must be"):
        function(good, box=(0, 1, 0, 1), within=1, **BASE)
    with pytest.raises(TypeError):                                  # a band stays unavailable
        function(good, band=(0, 1), **BASE)


@pytest.mark.parametrize("name", ("global_align", "global_paths"))
def test_none_an_array_and_one_tuple_pass_the_checks(name, monkeypatch):
    """Good arguments get as far as the device: the first thing asked of it is the rows' copy,
    which stands in for it here."""
    class Reached(Exception):
        pass

    def reached(*_):
        raise Reached()
    monkeypatch.setattr(align, "_prepare", reached)
    monkeypatch.setattr(native, "library", reached)
    good = _rows_f16(6)
    for box in (None, (0, 1, 0, 3), [-7, 7, 1, 2], np.array([[0, 1, 0, 1]] * 3, dtype=np.int16),
                torch.tensor([[-3, 4, 0, 0], [-4097, 4097, -9999, 9999], [0, 0, 1, 3]]),
                [[0, 0, 9, 12]] * 3):
        for within in MODES:
            with pytest.raises(Reached):
                getattr(align, name)(good, box=box, within=within, **BASE)


def test_an_empty_call_with_a_box_needs_no_device(monkeypatch):
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(native, "library", no_library)
    good = _rows_f16(6)
    for pairs, box in (([], (0, 1, 0, 1)), ([], []), (np.zeros((0, 2), dtype=np.int32),
                                                      np.zeros((0, 4), dtype=np.int64))):
        call = align._checked_call(good, None, [2, 4], None, pairs, 1.0, 0.5, 1.0, 0.0, None, box)
        assert call.empty and call.box.shape == (0, 4)
        assert call.box_rows.shape == call.box_columns.shape == (0,)
    call = align._checked_call(good, good[:0], [2, 4], [0], [[0, 0], [1, 0]], 1.0, 0.5, 1.0, 0.0,
                               None, (0, 3, 0, 3))
    assert call.empty and call.box_rows.tolist() == [2, 4] and call.box_columns.tolist() == [0, 0]


def test_the_call_record_sizes_slots_by_the_clipped_box_and_puts_the_box_behind_within():
    good = _rows_f16(6)
    arguments = (good, None, [2, 4], None, [[0, 1], [1, 1], [1, 0]], 1.0, 0.5, 1.0, 0.0, None)
    call = align._checked_call(*arguments, None)
    assert call.box_rows.tolist() == [2, 4, 4] and call.box_columns.tolist() == [4, 4, 2]
    call = align._checked_call(*arguments, [[-3, 0, 1, 9], [1, 2, 0, 0], [4, 9, 0, 1]])
    assert call.box_rows.tolist() == [1, 2, 0] and call.box_columns.tolist() == [3, 1, 2]

    class Pointer:
        def __init__(self, value):
            self.value, self.shape = value, (6, 128)

        def data_ptr(self):
            return self.value

    plain = align._Call(Pointer(1), Pointer(2), np.array([0, 2, 6]), np.array([0, 2, 6]),
                        np.zeros((3, 2), dtype=np.int32), np.array([4, 4, 2]), (1.0, 0.0, 1.0, 0.5),
                        Pointer(3), Pointer(4), Pointer(5))
    boxed = plain._replace(box=np.zeros((3, 4), dtype=np.int32), box_dev=Pointer(7))
    assert boxed.values() == plain.values() and len(plain.values()) == 14
    for kind, name in (("global", "gfy_align_global"), ("global_trace", "gfy_align_global_trace")):
        assert align._symbol(plain, kind, False) == (name, (0,))
        assert align._symbol(plain, kind, True) == (name, (1,))
        assert align._symbol(boxed, kind, True) == (name + "_box", (1, 7))
    assert align._symbol(boxed, "span") == ("gfy_align_local_span_box", (None, 7))   # the local order


def test_c_abi_declares_the_two_symbols_and_names_what_they_refuse():
    lib = native.library()
    void, size, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    header = (Path(__file__).resolve().parents[1] / "include" / "gfy.h").read_text()
    for name in ("gfy_align_global_box", "gfy_align_global_trace_box"):
        result, declared = native.SIGNATURES[name]
        assert result is ctypes.c_int and getattr(lib, name) is not None
        # the twin's list with `boxes` behind `within`
        twin = list(native.SIGNATURES[name[:-len("_box")]][1])
        assert twin[14] is ctypes.c_int and list(declared) == twin[:15] + [void] + twin[15:], name
        assert f"{name}(" in header
    assert list(native.SIGNATURES["gfy_align_global_trace_box"][1])[-5:] == [i64, i64, void, size, void]
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    wave = lib.gfy_align_global_trace_workspace_bytes(1, 100, 200) // 4

    def score_call(a=p, b=p, ptr_a=p, ptr_b=p, pairs=p, P=10, go=1.0, ge=0.5, within=0, boxes=p,
                   score=p, end=p, ws=p, size=lib.gfy_align_workspace_bytes(10, 0)):
        return lib.gfy_align_global_box(a, 300, ptr_a, 3, b, 500, ptr_b, 7, pairs, P, 1.0, 0.0, go,
                                        ge, within, boxes, score, end, ws, size, None)

    def trace_call(a=p, b=p, ptr_a=p, ptr_b=p, pairs=p, P=10, go=1.0, ge=0.5, within=0, boxes=p,
                   ends=p, op_ptr=p, ops=p, length=p, start=p, rows=100, cols=200, ws=p, size=wave):
        return lib.gfy_align_global_trace_box(a, 300, ptr_a, 3, b, 500, ptr_b, 7, pairs, P, 1.0, 0.0,
                                              go, ge, within, boxes, ends, op_ptr, ops, length,
                                              start, rows, cols, ws, size, None)

    def refusal(call, who, code, text, **changes):
        assert call(**changes) == code, (who, changes)
        message = lib.gfy_last_error()
        assert message.startswith(who + b": ") and text in message, (changes, message)

    shared = {"a": b"a is NULL", "b": b"b is NULL", "ptr_a": b"ptr_a is NULL",
              "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL", "ws": b"workspace is NULL"}
    holes = {score_call: {**shared, "score": b"out_score is NULL", "end": b"out_end is NULL"},
             trace_call: {**shared, "ends": b"ends is NULL", "op_ptr": b"op_ptr is NULL",
                          "ops": b"out_ops is NULL", "length": b"out_len is NULL",
                          "start": b"out_start is NULL"}}
    for call, who, plain in ((score_call, b"gfy_align_global_box", b"gfy_align_global "),
                             (trace_call, b"gfy_align_global_trace_box", b"gfy_align_global_trace ")):
        refusal(call, who, native.GFY_ERR_INVALID, b"boxes is NULL", boxes=None)
        assert plain + b"is the call without a box" in lib.gfy_last_error()
        refusal(call, who, native.GFY_ERR_INVALID, b"boxes is NULL", boxes=None, a=None)
        for hole, text in holes[call].items():
            refusal(call, who, native.GFY_ERR_INVALID, text, **{hole: None})
        refusal(call, who, native.GFY_ERR_INVALID, b"P = ", P=0)
        refusal(call, who, native.GFY_ERR_INVALID, b"gap_extend", go=1.0, ge=1.5)
        for within in (2, -1):
            refusal(call, who, native.GFY_ERR_INVALID, b"within = ", within=within)
        for short in (0, 1):
            refusal(call, who, native.GFY_ERR_WORKSPACE, b"workspace", size=short)
    refusal(trace_call, b"gfy_align_global_trace_box", native.GFY_ERR_INVALID, b"are negative",
            rows=-1)
    refusal(trace_call, b"gfy_align_global_trace_box", native.GFY_ERR_WORKSPACE, b"of one wave",
            size=wave - 1)
