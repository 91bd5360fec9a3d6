"""Local alignment inside a box of rows per pair (the ``box`` of align.local_align, local_spans
and local_paths, ``Runs.boxes`` and ``Chains.boxes``; gfy_align_local_box,
gfy_align_local_span_box): what needs no GPU.  The oracle of tests/align_box_oracle.py on the tie
zoo (a covering box is the call without one, enlarging a box never lowers a score, re-scoring
the ops gives the score), every ``ValueError`` of the box before a device is touched, the boxes
of runs and chains on hand-made tuples, the two symbols of the C ABI, and the premise of the
two-region case of tests/test_gpu_align_box.py."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_box_oracle as XO
import align_cases as Z
import align_path_oracle as PO
from ginfinity_amd import _native as native
from ginfinity_amd import align, seeds

K = 0                                   # Z.TIE_PARAMETERS[0]
GAPS = Z.TIE_PARAMETERS[K][2:]


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


def _same(got, want, where=None):
    assert (_bits(got[0]), tuple(got[1]), tuple(got[2])) == \
        (_bits(want[0]), tuple(want[1]), tuple(want[2])), (where, got[:3], want[:3])
    assert got[3].tobytes() == want[3].tobytes(), where


# consequence 1
def test_a_covering_box_equals_the_oracles_without_a_box():
    for q, r in Z.with_rows():
        lq, lr = Z.ROWS_A[q], Z.ROWS_B[r]
        S = Z.substitution(q, r, K)
        for box in (XO.covering(lq, lr), (-3, lq + 5, -1, lr), (-4096, 4096, -4096, 4096)):
            _same(XO.box_path_of(S, *GAPS, box), Z.path(q, r, K), (q, r, box))
            for band in Z.bands_of(q, r, K):
                _same(XO.box_path_of(S, *GAPS, box, band), Z.banded(q, r, K, band), (q, r, box, band))


def _nested(rng, lq, lr):
    """Boxes of an lq x lr matrix, every one inside the next, the last one covering."""
    i, j = int(rng.integers(0, lq)), int(rng.integers(0, lr))
    box = [i, i, j, j]
    yield tuple(box)
    while tuple(box) != XO.covering(lq, lr):
        grow = rng.integers(0, 40, size=4)
        box = [max(box[0] - grow[0], 0), min(box[1] + grow[1], lq - 1),
               max(box[2] - grow[2], 0), min(box[3] + grow[3], lr - 1)]
        yield tuple(int(x) for x in box)


# consequences 3 and 4
def test_enlarging_a_box_never_lowers_the_score_and_the_ops_add_up_to_it():
    rng = np.random.default_rng(20261021)
    checked = 0
    for q, r in Z.with_rows():
        lq, lr = Z.ROWS_A[q], Z.ROWS_B[r]
        S = Z.substitution(q, r, K)
        for band in (None, Z.bands_of(q, r, K)[2]):
            before = None
            for box in _nested(rng, lq, lr):
                score, start, end, ops = XO.box_path_of(S, *GAPS, box, band)
                assert before is None or score >= before, (q, r, box, band)
                before = score
                if end == (-1, -1):
                    assert _bits(score) == _bits(0) and ops.size == 0
                    continue
                assert _bits(PO.rescore(S, ops, start, *GAPS)) == _bits(score), (q, r, box, band)
                cells = align.path_cells(ops, np.array(start))
                assert tuple(cells[0]) == start and tuple(cells[-1]) == end
                both = cells[(cells >= 0).all(axis=1)]
                assert both[:, 0].min() >= box[0] and both[:, 0].max() <= box[1]
                assert both[:, 1].min() >= box[2] and both[:, 1].max() <= box[3]
                checked += 1
            want = Z.path(q, r, K) if band is None else Z.banded(q, r, K, band)
            assert _bits(before) == _bits(want[0])                  # the last one covers
    assert checked >= 100, checked


def test_a_box_that_holds_no_cell_and_a_single_cell():
    S = np.full((5, 7), 0.5, dtype=np.float32)
    for box in ((5, 9, 0, 6), (-9, -1, 0, 6), (0, 4, 7, 7), (0, 4, -4096, -1), (4096, 4096, 0, 0)):
        score, start, end, ops = XO.box_path_of(S, 1.0, 0.5, box)
        assert _bits(score) == _bits(0) and start == end == (-1, -1) and ops.size == 0
    assert XO.box_path_of(S, 1.0, 0.5, (0, 4, 0, 6), (7, 9))[2] == (-1, -1)     # the band misses
    score, start, end, ops = XO.box_path_of(S, 1.0, 0.5, (3, 3, 2, 2))
    assert _bits(score) == _bits(0.5) and start == end == (3, 2) and ops.tolist() == [0]
    assert XO.box_path_of(S, 1.0, 0.5, (3, 3, 2, 2), (0, 5))[2] == (-1, -1)      # d = -1 is outside


def _rows_f16(count):
    rng = np.random.default_rng(count)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


BASE = dict(counts_a=[2, 4], pairs=[[0, 1], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5)


@pytest.mark.parametrize("name", ("local_align", "local_spans", "local_paths"))
def test_a_bad_box_is_a_value_error_before_any_device_is_touched(name, monkeypatch):
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(native, "library", no_library)
    function = getattr(align, name)
    good = _rows_f16(6)
    for box in ([[0.0, 1.0, 0.0, 1.0]] * 3, np.zeros((3, 4)), torch.zeros((3, 4)),
                (0.0, 1.0, 0.0, 1.0), "0101", (0, 1, True, 1), [[None, 1, 0, 1]] * 3,
                np.zeros((3, 4), dtype=bool), torch.zeros((3, 4), dtype=torch.bool)):
        with pytest.raises(ValueError, match="box must"):
            function(good, box=box, **BASE)
    for box in ([[0, 1, 0, 1]] * 2, [[0, 1, 0, 1]] * 4, [[0, 1]] * 3, [[0, 1, 2, 3, 4]] * 3,
                [0, 1, 2], (0, 1), 5, [[[0, 1, 0, 1]]] * 3, np.zeros((3, 4, 1), dtype=np.int32), []):
        with pytest.raises(ValueError, match=r"shape \(P, 4\)"):
            function(good, box=box, **BASE)
    with pytest.raises(ValueError, match=r"box of pair 1 = \(3, 2, 0, 0\): i_lo <= i_hi and j_lo"):
        function(good, box=[[0, 1, 0, 1], [3, 2, 0, 0], [9, 1, 0, 0]], **BASE)
    with pytest.raises(ValueError, match=r"box of pair 2 = \(0, 0, 1, 0\)"):
        function(good, box=[[0, 1, 0, 1], [2, 2, 0, 0], [0, 0, 1, 0]], **BASE)
    with pytest.raises(ValueError, match=r"box of pair 0 = \(0, 5, 1, 0\)"):
        function(good, box=(0, 5, 1, 0), **BASE)
    with pytest.raises(ValueError, match=r"box of pair 2 = \(5000, 4999, 0, 0\)"):   # before clipping
        function(good, box=torch.tensor([[0, 0, 0, 0], [-1, 1, -1, 1], [5000, 4999, 0, 0]]), **BASE)
    # the other checks come first and are unchanged by a box; a bad band next to a good box
    with pytest.raises(ValueError, match="out of range"):
        function(good, box=(0, 1, 0, 1), **{**BASE, "pairs": [[0, 2]]})
    with pytest.raises(ValueError, match="lo <= hi"):
        function(good, box=(0, 1, 0, 1), band=(1, 0), **BASE)


def test_none_a_box_and_one_tuple_pass_the_checks_with_no_device_touched():
    good = _rows_f16(6)
    arguments = (good, None, [2, 4], None, [[0, 1], [1, 1], [1, 0]], 1.0, 0.5, 1.0, 0.0)
    call = align._checked_call(*arguments)
    assert call.box is None and call.box_dev is None and not call.a.is_cuda
    assert call.box_columns.tolist() == [4, 4, 2]
    assert align._checked_call(*arguments, None, None).box is None
    wanted = [[-3, 4, 0, 0], [-4096, 4096, -4096, 4096], [0, 0, 1, 3]]
    for box in ([[-3, 4, 0, 0], [-10 ** 9, 2 ** 40, -2 ** 31, 2 ** 31], [0, 0, 1, 3]],
                np.array([[-3, 4, 0, 0], [-5000, 5000, -4097, 4097], [0, 0, 1, 3]], dtype=np.int16),
                torch.tensor([[-3, 4, 0, 0], [-4097, 4097, -9999, 9999], [0, 0, 1, 3]])):
        call = align._checked_call(*arguments, None, box)
        assert call.box.dtype == np.int32 and call.box.flags.c_contiguous
        assert call.box.tolist() == wanted and call.box_dev is None and call.band is None
        # the columns a carry buffer has to hold: those of the box inside the b-record
        assert call.box_columns.tolist() == [1, 4, 1]
    for one in ((-7, 7, 1, 2), [-7, 7, 1, 2], np.array([-7, 7, 1, 2]), torch.tensor([-7, 7, 1, 2])):
        call = align._checked_call(*arguments, (-1, 1), one)
        assert call.box.tolist() == [[-7, 7, 1, 2]] * 3 and call.band.tolist() == [[-1, 1]] * 3
        assert call.box_columns.tolist() == [2, 2, 1]
    assert align._checked_call(*arguments, None, (0, 0, 9, 12)).box_columns.tolist() == [0, 0, 0]
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        for name in ("local_align", "local_spans", "local_paths"):
            with pytest.raises((RuntimeError, AssertionError)):
                getattr(align, name)(good, counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0,
                                     gap_extend=0.5, box=(0, 1, 0, 1))


def test_an_empty_call_with_a_box_is_known_to_be_empty_without_a_device(monkeypatch):
    """``_launch`` asks the library for nothing where ``call.empty`` holds, and that is decided
    on the host, box or not."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(native, "library", no_library)
    good = _rows_f16(6)
    for pairs, box in (([], (0, 1, 0, 1)), ([], []), (np.zeros((0, 2), dtype=np.int32),
                                                      np.zeros((0, 4), dtype=np.int64))):
        call = align._checked_call(good, None, [2, 4], None, pairs, 1.0, 0.5, 1.0, 0.0, None, box)
        assert call.empty and call.box.shape == (0, 4) and call.box.dtype == np.int32
        assert call.box_dev is None and call.box_columns.shape == (0,)
    # rows on one side only: every pair is empty, whatever its box
    call = align._checked_call(good, good[:0], [2, 4], [0], [[0, 0], [1, 0]], 1.0, 0.5, 1.0, 0.0,
                               None, (0, 3, 0, 3))
    assert call.empty and call.box.shape == (2, 4)


def test_the_call_record_appends_the_band_and_the_box_to_the_arguments():
    """With a box the ``*_box`` symbols take the band (or NULL) and the box behind gap_extend."""

    class Pointer:
        def __init__(self, value):
            self.value, self.shape = value, (6, 128)

        def data_ptr(self):
            return self.value

    plain = align._Call(Pointer(1), Pointer(2), np.array([0, 2, 6]), np.array([0, 2, 6]),
                        np.zeros((3, 2), dtype=np.int32), np.array([4, 4, 2]), (1.0, 0.0, 1.0, 0.5),
                        Pointer(3), Pointer(4), Pointer(5))
    banded = plain._replace(band=np.zeros((3, 2), dtype=np.int32), band_dev=Pointer(6))
    boxed = plain._replace(box=np.zeros((3, 4), dtype=np.int32), box_dev=Pointer(7))
    both = banded._replace(box=np.zeros((3, 4), dtype=np.int32), box_dev=Pointer(7))
    assert boxed.values() == both.values() == banded.values() == plain.values()
    for kind, name in (("score", "gfy_align_local"), ("span", "gfy_align_local_span")):
        assert align._symbol(boxed, kind) == (name + "_box", (None, 7))
        assert align._symbol(both, kind) == (name + "_box", (6, 7))
        assert align._symbol(banded, kind) == (name + "_band", (6,))
    # the trace of a local path takes the band and never the box
    assert align._symbol(boxed, "trace") == ("gfy_align_trace", ())
    assert align._symbol(both, "trace") == ("gfy_align_trace_band", (6,))


def _runs(cells, lengths):
    count = len(lengths)
    return seeds.Runs(torch.zeros((count, 2), dtype=torch.int32),
                      torch.tensor(cells, dtype=torch.int32).reshape(count, 2),
                      torch.tensor(lengths, dtype=torch.int32), torch.zeros(count))


def _chains(starts, ends):
    count = len(starts)
    empty = torch.zeros(count, dtype=torch.int32)
    return seeds.Chains(torch.zeros((count, 2), dtype=torch.int32),
                        torch.tensor(starts, dtype=torch.int32).reshape(count, 2),
                        torch.tensor(ends, dtype=torch.int32).reshape(count, 2),
                        torch.zeros((count, 2), dtype=torch.int32), empty, empty,
                        torch.zeros(count), torch.zeros(0, dtype=torch.int32))


def test_the_boxes_of_runs_and_chains():
    runs = _runs([[3, 10], [0, 0], [4095, 4000]], [5, 1, 1])
    boxes = runs.boxes(0)
    assert boxes.dtype == np.int32 and boxes.shape == (3, 4)
    assert boxes.tolist() == [[3, 7, 10, 14], [0, 0, 0, 0], [4095, 4095, 4000, 4000]]
    assert runs.boxes(2).tolist() == [[1, 9, 8, 16], [-2, 2, -2, 2], [4093, 4097, 3998, 4002]]
    assert runs.boxes(np.int64(1)).tolist()[0] == [2, 8, 9, 15]
    # a margin beyond the cut: twice GFY_ALIGN_ROWS_MAX, and the call clips the rest
    assert runs.boxes(10 ** 12).tolist() == runs.boxes(8192).tolist()
    assert runs.boxes(10 ** 12).tolist()[0] == [3 - 8192, 7 + 8192, 10 - 8192, 14 + 8192]
    chains = _chains([[3, 10], [100, 90]], [[40, 52], [100, 90]])
    boxes = chains.boxes(0)
    assert boxes.dtype == np.int32 and boxes.tolist() == [[3, 40, 10, 52], [100, 100, 90, 90]]
    assert chains.boxes(16).tolist() == [[-13, 56, -6, 68], [84, 116, 74, 106]]
    assert chains.boxes(10 ** 12).tolist() == chains.boxes(8192).tolist()
    assert _runs([], []).boxes(3).shape == (0, 4) and _chains([], []).boxes(3).shape == (0, 4)
    assert _chains([], []).boxes(3).dtype == np.int32
    for margin in (-1, 1.0, "2", None, True, np.bool_(False)):
        for made in (runs, chains):
            with pytest.raises(ValueError, match="margin must be a non-negative integer"):
                made.boxes(margin)
    # what the makers give is what the call takes
    call = align._checked_call(_rows_f16(6), None, [2, 4], None, [[0, 1], [1, 1]], 1.0, 0.5, 1.0,
                               0.0, chains.bands(4), chains.boxes(10 ** 12))
    assert call.box.tolist() == [[-4096, 4096, -4096, 4096]] * 2


def test_c_abi_declares_the_two_symbols_and_names_what_they_refuse():
    lib = native.library()
    void, size = ctypes.c_void_p, ctypes.c_size_t
    call = [void, ctypes.c_int64] * 5 + [ctypes.c_float] * 4
    wanted = {"gfy_align_local_box": call + [void, void, void, void, void, size, void],
              "gfy_align_local_span_box": call + [void, void, void, void, void, void, size, void]}
    header = (Path(__file__).resolve().parents[1] / "include" / "gfy.h").read_text()
    for name, arguments in wanted.items():
        result, declared = native.SIGNATURES[name]
        assert result is ctypes.c_int and list(declared) == arguments, name
        assert getattr(lib, name) is not None
        # the banded twin's list with `boxes` behind `bands`
        twin = list(native.SIGNATURES[name[:-len("_box")] + "_band"][1])
        assert arguments == twin[:15] + [void] + twin[15:], name
        assert f"{name}(" in header
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced

    def score_call(a=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, boxes=p, score=p, end=p, ws=p,
                   size=lib.gfy_align_workspace_bytes(10, 0)):
        return lib.gfy_align_local_box(a, 300, p, 3, p, 500, p, 7, pairs, P, 1.0, 0.0, go, ge,
                                       bands, boxes, score, end, ws, size, None)

    def span_call(a=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, boxes=p, score=p, start=p, end=p,
                  ws=p, size=lib.gfy_align_span_workspace_bytes(10, 0)):
        return lib.gfy_align_local_span_box(a, 300, p, 3, p, 500, p, 7, pairs, P, 1.0, 0.0, go,
                                            ge, bands, boxes, score, start, end, ws, size, None)

    def refusal(call, who, code, text, **changes):
        assert call(**changes) == code, (who, changes)
        message = lib.gfy_last_error()
        assert message.startswith(who + b": ") and text in message, (changes, message)

    holes = {score_call: {"score": b"out_score is NULL", "end": b"out_end is NULL"},
             span_call: {"score": b"out_score is NULL", "start": b"out_start is NULL",
                         "end": b"out_end is NULL"}}
    for call, who, plain in ((score_call, b"gfy_align_local_box", b"gfy_align_local_band "),
                             (span_call, b"gfy_align_local_span_box",
                              b"gfy_align_local_span_band ")):
        refusal(call, who, native.GFY_ERR_INVALID, b"boxes is NULL", boxes=None)
        assert plain + b"is the call without a box" in lib.gfy_last_error()
        refusal(call, who, native.GFY_ERR_INVALID, b"boxes is NULL", boxes=None, bands=None)
        for hole, text in {"a": b"a is NULL", "pairs": b"pairs is NULL", "ws": b"workspace is NULL",
                           **holes[call]}.items():
            refusal(call, who, native.GFY_ERR_INVALID, text, **{hole: None})
            refusal(call, who, native.GFY_ERR_INVALID, text, bands=None, **{hole: None})
        refusal(call, who, native.GFY_ERR_INVALID, b"P = ", P=0)
        refusal(call, who, native.GFY_ERR_INVALID, b"gap_extend", go=1.0, ge=1.5)
        for short in (0, 1):
            # a NULL bands is no refusal: the next check speaks
            refusal(call, who, native.GFY_ERR_WORKSPACE, b"workspace", size=short, bands=None)


def test_the_premise_of_the_two_region_pair():
    """Two regions on one diagonal with an unrelated linker between them: the band alone gives
    both seeds the stronger region, a box around each seed gives each its own."""
    case = XO.two_regions()
    S, (first, second) = case["S"], case["plants"]
    go, ge = XO.REGION_PARAMETERS[2:]
    band = (XO.REGION_SHIFT - 4, XO.REGION_SHIFT + 4)
    boxes = [(int(plant[0, 0]) - 8, int(plant[-1, 0]) + 8, int(plant[0, 1]) - 8,
              int(plant[-1, 1]) + 8) for plant in (first, second)]
    assert boxes[0][1] < boxes[1][0] and boxes[0][3] < boxes[1][2]      # the boxes do not meet
    # both seeds have the same pair and the same band: one alignment, the stronger region's
    score, start, end, ops = BO.band_path_of(S, go, ge, *band)
    cells = align.path_cells(ops, np.array(start))
    assert XO.holds(cells, first) and not XO.holds(cells, second)
    assert end[0] < second[0, 0] and end[1] < second[0, 1]              # the weaker one is not met
    found = [XO.box_path_of(S, go, ge, box, band) for box in boxes]
    _same(found[0], (score, start, end, ops))
    assert found[1][0] > 0 and _bits(found[1][0]) != _bits(found[0][0])
    assert found[1][1] != found[0][1] and found[1][2] != found[0][2]
    for (score, start, end, ops), plant in zip(found, (first, second)):
        assert XO.holds(align.path_cells(ops, np.array(start)), plant)
        assert _bits(PO.rescore(S, ops, start, go, ge)) == _bits(score)
        assert score >= np.float32(0.25) * plant.shape[0]          # a match scores 0.25
