"""The aligned path of the local aligner (gfy_align_trace, align.local_paths): what needs no GPU.
The oracle of tests/align_path_oracle.py names the start, end and score of the span oracle, walks
the box start..end alone to the same ops, re-scores its ops to the score bit for bit and keeps
the count identities of include/gfy.h — the CPU check of the claims the kernel rests on;
``path_cells`` on hand-written ops; the Python function refuses what ``local_spans`` refuses and
the C ABI names what it refuses, both before a device is touched."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import align_path_oracle as PO
import align_span_oracle as SO
import test_gpu_align as G
from ginfinity_amd import _native as native
from ginfinity_amd import align


# ---- the oracle and the claims ------------------------------------------------------------------

def _quarter_matrices():
    """Random float32 matrices of up to 40 x 60 whose values are multiples of 1/4 (ties occur), a
    noisy diagonal planted with holes so the best path needs gaps and mismatches."""
    rng = np.random.default_rng(424242)
    for case in range(75):
        lq, lr = int(rng.integers(1, 41)), int(rng.integers(1, 61))
        S = rng.integers(-6, 3, size=(lq, lr)) / 4.0
        length = min(lq, lr)
        at_i, at_j = int(rng.integers(0, lq - length + 1)), int(rng.integers(0, lr - length + 1))
        keep = rng.random(length) < 0.8
        steps = np.arange(length)[keep]
        S[at_i + steps, at_j + steps] = rng.integers(1, 5, size=steps.size) / 4.0
        if case % 3 == 0 and lr > 8:          # a shifted second stretch: a gap joins the two
            shift = int(rng.integers(1, 4))
            late = steps[(steps >= length // 2) & (at_j + steps + shift < lr)]
            S[at_i + late, at_j + late] = -1.5
            S[at_i + late, at_j + late + shift] = 1.0
        yield S.astype(np.float32)


def test_the_walk_agrees_with_the_span_oracle_the_box_and_the_score():
    cases = gapped = tied = 0
    for S in _quarter_matrices():
        for _, _, go, ge in G.PARAMETERS:
            score, start, end, ops = PO.path_of(S, go, ge)
            want = SO.span_of(S, go, ge)
            where = (S.shape, go, ge)
            assert np.float32(score).tobytes() == np.float32(want[0]).tobytes(), where
            assert (start, end) == want[1:], (where, start, end, want)
            cases += 1
            if end == (-1, -1):
                assert ops.size == 0
                continue
            # the count identities
            assert ops[0] == 0 and ops[-1] == 0, where
            assert np.count_nonzero(ops != 1) == end[0] - start[0] + 1, where
            assert np.count_nonzero(ops != 2) == end[1] - start[1] + 1, where
            assert ops.size <= (end[0] - start[0] + 1) + (end[1] - start[1] + 1) - 1
            # the box alone gives the same ops
            box = np.ascontiguousarray(S[start[0]:end[0] + 1, start[1]:end[1] + 1])
            inside = PO.box_path(box, go, ge)
            assert inside.tobytes() == ops.tobytes(), (where, inside, ops)
            # re-scoring gives the score bit for bit
            again = PO.rescore(S, ops, start, go, ge)
            assert np.float32(again).tobytes() == np.float32(score).tobytes(), (where, again, score)
            cells = align.path_cells(ops, start)
            assert tuple(cells[0]) == start and tuple(cells[-1]) == end
            gapped += bool(np.any(ops != 0))
            H = PO.gotoh_matrices(S, go, ge, np.float32)[0][1:, 1:]
            tied += int(np.count_nonzero(H == H.max()) > 1)
    assert cases == 300 and gapped >= 60 and tied >= 10, (cases, gapped, tied)


def test_the_walk_on_hand_made_matrices():
    def matrix(shape, cells):
        S = np.full(shape, -9.0, dtype=np.float32)
        for cell, value in cells.items():
            S[cell] = value
        return S

    # the matrices of test_align_span_host.test_tie_rules_on_hand_made_matrices: diagonal, E and F
    # tie at H[1][1]; the diagonal goes first, then E, then F
    S = matrix((3, 3), {(0, 0): 1, (0, 1): 3, (1, 0): 3, (1, 1): 1, (2, 2): 5})
    assert PO.path_of(S, 1.0, 1.0)[1:3] == ((0, 0), (2, 2))
    assert PO.path_of(S, 1.0, 1.0)[3].tolist() == [0, 0, 0]
    S[1, 1] = 0.5                     # E and F tie: E, a gap along row 1 from (1, 0)
    assert PO.path_of(S, 1.0, 1.0)[1] == (1, 0)
    assert PO.path_of(S, 1.0, 1.0)[3].tolist() == [0, 1, 0]
    S[1, 0] = 2.5                     # F alone
    assert PO.path_of(S, 1.0, 1.0)[1] == (0, 1)
    assert PO.path_of(S, 1.0, 1.0)[3].tolist() == [0, 2, 0]
    # gap_open == gap_extend: E[1][2] is 3 both ways and opening wins, so the run of two gap ops
    # re-opens inside and the path comes from (0, 0) by the diagonal
    S = matrix((3, 4), {(0, 0): 1, (1, 0): 4, (1, 1): 2.5, (2, 3): 5})
    score, start, end, ops = PO.path_of(S, 0.5, 0.5)
    assert (score, start, end) == (np.float32(8), (0, 0), (2, 3)) and ops.tolist() == [0, 0, 1, 0]
    assert PO.rescore(S, ops, start, 0.5, 0.5) == np.float32(8)
    # nothing positive, no cell at all
    assert PO.path_of(np.full((3, 3), -0.5, dtype=np.float32), 1.0, 0.5)[3].size == 0
    assert PO.path_of(np.zeros((0, 3), dtype=np.float32), 1.0, 0.5)[1:3] == ((-1, -1), (-1, -1))
    assert PO.box_path(matrix((2, 2), {(0, 0): 1}), 1.0, 0.5).size == 0     # H of the last cell is 0


# ---- align.path_cells ---------------------------------------------------------------------------

def test_path_cells_on_hand_written_ops():
    cells = align.path_cells([0, 0, 1, 1, 0, 2, 0], (3, 5))
    assert cells.dtype == np.int32 and cells.shape == (7, 2)
    assert cells.tolist() == [[3, 5], [4, 6], [-1, 7], [-1, 8], [5, 9], [6, -1], [7, 10]]
    assert align.path_cells(np.array([0], dtype=np.uint8), np.array([0, 0])).tolist() == [[0, 0]]
    assert align.path_cells(torch.tensor([0, 2, 2, 0], dtype=torch.uint8),
                            torch.tensor([10, 4], dtype=torch.int32)).tolist() == \
        [[10, 4], [11, -1], [12, -1], [13, 5]]
    empty = align.path_cells(np.zeros(0, dtype=np.uint8), (-1, -1))
    assert empty.shape == (0, 2) and empty.dtype == np.int32
    for ops in ([0, 3], [-1, 0], [[0, 0]], [0.0, 1.0]):
        with pytest.raises(ValueError, match="ops must be"):
            align.path_cells(ops, (0, 0))
    for start in ((-1, -1), (0,), (0, 0, 0), (0.0, 1.0)):
        with pytest.raises(ValueError, match="start must be"):
            align.path_cells([0, 0], start)


# ---- align.local_paths: errors before a device is touched ---------------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_python_refuses_what_local_spans_refuses(monkeypatch):
    """Every bad call raises from ``local_paths`` the ValueError, text included, that it raises
    from ``local_spans``; the library is never asked for."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    for name in ("local_paths", "path_cells", "AlignedPaths"):
        assert name in align.__all__
    assert align.AlignedPaths._fields == ("scores", "starts", "ends", "ops", "offsets")
    good, other, long = _rows_f16(6), _rows_f16(5), _rows_f16(4100)
    base = dict(counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0, gap_extend=0.5)
    refused = 0

    def same_error(*rows, **changes):
        nonlocal refused
        arguments = {**base, **changes}
        with pytest.raises(ValueError) as wanted:
            align.local_spans(*(rows or (good,)), **arguments)
        with pytest.raises(ValueError) as got:
            align.local_paths(*(rows or (good,)), **arguments)
        assert str(got.value) == str(wanted.value)
        refused += 1
        return str(got.value)

    for missing in ("gap_open", "gap_extend", "pairs"):
        with pytest.raises(TypeError):
            align.local_paths(good, **{k: v for k, v in base.items() if k != missing})
    for missing in ("gap_open", "gap_extend"):
        assert f"{missing} is required" in same_error(**{missing: None})
    for name in ("gap_open", "gap_extend", "match_scale", "match_shift"):
        for value in (float("inf"), float("nan"), "1", True, 1e39):
            assert f"{name} must be" in same_error(**{name: value})
    assert "gap_extend <= gap_open" in same_error(gap_open=0.5, gap_extend=1.0)
    assert "gap_extend <= gap_open" in same_error(gap_open=1.0, gap_extend=-0.25)
    for pairs in ([[0, 2]], [[2, 0]], [[-1, 0]], [[0, 0], [1, 5]]):
        assert "out of range" in same_error(pairs=pairs)
    assert "out of range" in same_error(good, other, counts_b=[5], pairs=[[0, 1]])
    for pairs in ([0, 1], [[0.0, 1.0]], [[0, 1, 1]], [[[0, 1]]], "01"):
        assert "shape (P, 2)" in same_error(pairs=pairs)
    assert "counts_a sums to 5 rows, a has 6" in same_error(counts_a=[2, 3])
    assert "counts_b sums to 4 rows, b has 5" in same_error(good, other, counts_b=[4])
    assert "counts_b is required" in same_error(good, other)
    assert "record counts" in same_error(counts_a=[2.0, 4.0])
    assert "pair 1: record 1 of a has 4097 rows, more than 4096" in same_error(
        long, counts_a=[3, 4097], pairs=[[0, 0], [1, 0]])
    assert "pair 0: record 1 of b has 4097 rows, more than 4096" in same_error(
        good, long, counts_b=[3, 4097], pairs=[[0, 1]])
    assert "float16" in same_error(good.float())
    assert "float16" in same_error(good, other.float(), counts_b=[5])
    assert "shape (rows, 128)" in same_error(torch.zeros((6, 64), dtype=torch.float16))
    assert refused == 43
    for cap in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            align.local_paths(good, max_workspace_bytes=cap, **base)
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            align.local_paths(good, **base)


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_names_what_it_refuses_without_a_gpu():
    lib = native.library()
    for name in ("gfy_align_trace", "gfy_align_trace_workspace_bytes"):
        assert name in native.SIGNATURES and getattr(lib, name) is not None
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    sizer = lib.gfy_align_trace_workspace_bytes
    one = sizer(1, 100, 200)       # a workgroup of four waves
    assert one % 1024 == 0 and one // 4 >= 100 * 25 * 4 + 2 * 200 * 8
    assert sizer(4, 100, 200) == one and sizer(5, 100, 200) == 2 * one and sizer(0, 100, 200) == one
    assert sizer(10 ** 9, 100, 200) == sizer(10 ** 8, 100, 200) == 256 * one      # the full grid
    assert sizer(1, 10 ** 9, 10 ** 9) == sizer(1, 4096, 4096)                     # clipped
    assert 8 * 2 ** 20 <= sizer(1, 4096, 4096) // 4 <= 8 * 2 ** 20 + 2 * 4096 * 8 + 256
    assert sizer(1, 100, 201) > one > sizer(1, 100, 192) and sizer(1, -5, -5) == sizer(1, 0, 0)
    wave = one // 4

    def call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p, P=10,
             scale=1.0, shift=0.0, go=1.0, ge=0.5, starts=p, ends=p, op_ptr=p, ops=p, length=p,
             rows=100, cols=200, ws=p, size=wave):
        return lib.gfy_align_trace(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P, scale,
                                   shift, go, ge, starts, ends, op_ptr, ops, length, rows, cols,
                                   ws, size, None)

    def refusal(code, text, **changes):
        assert call(**changes) == code, changes
        message = lib.gfy_last_error()
        assert message.startswith(b"gfy_align_trace: ") and text in message, (changes, message)

    for hole, text in {"a": b"a is NULL", "b": b"b is NULL", "ptr_a": b"ptr_a is NULL",
                       "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL",
                       "starts": b"starts is NULL", "ends": b"ends is NULL",
                       "op_ptr": b"op_ptr is NULL", "ops": b"out_ops is NULL",
                       "length": b"out_len is NULL", "ws": b"workspace is NULL"}.items():
        refusal(native.GFY_ERR_INVALID, text, **{hole: None})
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, 1 << 31)):
        refusal(native.GFY_ERR_INVALID, b"bad arguments", n=n, m=m)
    for name in ("records_a", "records_b"):
        for count in (0, -1, 1 << 31):
            refusal(native.GFY_ERR_INVALID, name.encode(), **{name: count})
    for P in (0, -1, 1 << 31):
        refusal(native.GFY_ERR_INVALID, b"P = ", P=P)
    for name in ("scale", "shift", "go", "ge"):
        for value in (float("inf"), float("nan")):
            refusal(native.GFY_ERR_INVALID, b"finite", **{name: value})
    for go, ge in ((1.0, 1.5), (1.0, -0.5)):
        refusal(native.GFY_ERR_INVALID, b"gap_extend", go=go, ge=ge)
    refusal(native.GFY_ERR_INVALID, b"negative", rows=-1)
    refusal(native.GFY_ERR_INVALID, b"negative", cols=-1)
    # a workspace below one wave's part is refused; one wave's part is all a call needs, which
    # only a device can show
    for short in (0, 1, wave - 1):
        refusal(native.GFY_ERR_WORKSPACE, b"workspace", size=short)
    refusal(native.GFY_ERR_WORKSPACE, b"workspace", rows=110)
    assert native.ABI_VERSION == lib.gfy_abi_version()
