"""Global and query-in-target alignment (align.global_align, align.global_paths, gfy_align_global,
gfy_align_global_trace): what needs no GPU.  The oracle of tests/align_global_oracle.py against
an explicit enumeration of every alignment of tiny matrices, its tie rules and border exits on
hand-made matrices, the re-scoring, path_cells and ordering claims of include/gfy.h on random
matrices with forced ties; the Python functions refuse what ``local_align`` refuses (and a
``within`` that is no bool) before a device is touched; the C ABI binds and names what it
refuses; the two new kernels keep the registers and instruction counts of their local twins."""
from __future__ import annotations

import ctypes
import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import align_global_oracle as GO
import align_oracle as O
from ginfinity_amd import _native as native
from ginfinity_amd import align

ROOT = Path(__file__).resolve().parents[1]
MODES = (False, True)          # within
#: (gap_open, gap_extend), multiples of 1/8; one set with gap_open == gap_extend, one free extension
GAPS = ((1.0, 0.25), (0.5, 0.5), (0.75, 0.0), (2.0, 1.0))


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


# ---- the oracle against every alignment ---------------------------------------------------------

def _tiny_matrices():
    """Every shape up to 4 x 4 over the values -5/8, 1/8 and 7/8 (sums of them and of the gap
    costs are exact in float32): every matrix of up to 6 cells, 30 random ones of each larger
    shape."""
    values = np.array([-0.625, 0.125, 0.875], dtype=np.float32)
    rng = np.random.default_rng(2718)
    for lq, lr in itertools.product((1, 2, 3, 4), repeat=2):
        if lq * lr <= 6:
            for picks in itertools.product(range(3), repeat=lq * lr):
                yield values[list(picks)].reshape(lq, lr)
        else:
            for _ in range(30):
                yield values[rng.integers(0, 3, size=(lq, lr))]


def test_the_oracle_agrees_with_every_alignment_of_tiny_matrices():
    cases = 0
    for number, S in enumerate(_tiny_matrices()):
        go, ge = GAPS[number % len(GAPS)]
        for within in MODES:
            best = GO.enumerate_alignments(S.astype(np.float64), go, ge, within)
            score, start, end, ops = GO.path_of(S, go, ge, within)
            where = (S.tolist(), go, ge, within)
            assert float(score) == best, where
            assert float(GO.score_of(S.astype(np.float64), go, ge, within, np.float64)[0]) == best
            # the path is one of the maximisers: its own sum is the maximum, and it is an
            # alignment of the mode (all of A; all of B, or rows start_j .. end_j of it)
            assert float(GO.rescore(S, ops, start, go, ge)) == best, where
            assert np.count_nonzero(ops != 1) == S.shape[0], where
            assert np.count_nonzero(ops != 2) == end[1] + 1 - start[1], where
            assert start[0] == 0 and end[0] == S.shape[0] - 1
            assert (start[1] == 0 and end[1] == S.shape[1] - 1) or within
            cases += 1
    assert cases == 2 * (1776 + 6 * 30), cases


# ---- tie rules and border exits -----------------------------------------------------------------

def _matrix(shape, cells, fill=-9.0):
    S = np.full(shape, fill, dtype=np.float32)
    for cell, value in cells.items():
        S[cell] = value
    return S


def test_tie_rules_on_hand_made_matrices():
    # H[1][1]: the diagonal (1 + 1), E (from H[1][0] = 3 by a gap of 1) and F (from H[0][1] = 3)
    # tie at 2; H[0][1] has the top border on its diagonal, -1 (global) or 0 (within)
    for within in MODES:
        S = _matrix((2, 2), {(0, 0): 1, (1, 1): 1, (0, 1): 3 if within else 4, (1, 0): 4})
        H, E, F = GO.matrices(S, 1.0, 1.0, np.float32, within)
        assert H[1, 1] == 1 and H[2, 1] == 3 and H[1, 2] == 3
        assert H[2, 2] == 2 == E[2, 2] == F[2, 2] == H[1, 1] + S[1, 1]
        # diagonal first (walked from that cell: within ends on H[1][0] = 3)
        assert GO.walk(S, H, E, F, 1.0, 1.0, (1, 1), within)[0].tolist() == [0, 0]
    S = _matrix((2, 2), {(0, 0): 1, (1, 1): 1, (0, 1): 4, (1, 0): 4})
    S[1, 1] = 0.5                                  # E and F tie at 2 and beat the diagonal: E
    assert GO.path_of(S, 1.0, 1.0, False)[3].tolist() == [2, 0, 1]            # (1, 0) then a gap in E
    S[1, 0] = 3.5                                  # F alone
    assert GO.path_of(S, 1.0, 1.0, False)[3].tolist() == [1, 0, 2]
    # opening wins a tie in E: with gap_open == gap_extend, E[0][2] is -1.5 from H[0][1] = -1 and
    # from E[0][1] = -1 alike; the walk opens, and finds H[0][1] to be E as well
    S = _matrix((1, 3), {(0, 0): -0.5, (0, 1): -9, (0, 2): -9})
    score, start, end, ops = GO.path_of(S, 0.5, 0.5, False)
    assert ops.tolist() == [0, 1, 1] and _bits(score) == _bits(-1.5)
    assert _bits(GO.rescore(S, ops, start, 0.5, 0.5)) == _bits(score)
    # ... and in F, transposed
    score, start, end, ops = GO.path_of(np.ascontiguousarray(S.T), 0.5, 0.5, False)
    assert ops.tolist() == [0, 2, 2] and _bits(score) == _bits(-1.5)
    # within: two columns tie on the last row, the first is the end
    S = _matrix((1, 4), {(0, 1): 2, (0, 3): 2})
    assert GO.path_of(S, 1.0, 0.5, True)[1:3] == ((0, 1), (0, 1))


def test_border_exits_on_hand_made_matrices():
    go, ge = 1.0, 0.25
    # (i, -1): A = two rows nothing likes, then B.  The left border is a charged gap of two rows
    S = _matrix((4, 2), {(2, 0): 3, (3, 1): 3})
    for within in MODES:
        score, start, end, ops = GO.path_of(S, go, ge, within)
        assert ops.tolist() == [2, 2, 0, 0] and start == (0, 0) and end == (3, 1)
        assert _bits(score) == _bits(np.float32(np.float32(-1.0) - np.float32(0.25)) + 6)
    # (-1, j): the transposed case.  Global pays for the two leading rows of B; within does not
    S = np.ascontiguousarray(S.T)
    score, start, end, ops = GO.path_of(S, go, ge, False)
    assert ops.tolist() == [1, 1, 0, 0] and start == (0, 0) and end == (1, 3) and score == 4.75
    score, start, end, ops = GO.path_of(S, go, ge, True)
    assert ops.tolist() == [0, 0] and start == (0, 2) and end == (1, 3) and score == 6
    assert align.path_cells(ops, start).tolist() == [[0, 2], [1, 3]]
    # (-1, -1): a plain diagonal
    S = _matrix((2, 2), {(0, 0): 1, (1, 1): 1})
    for within in MODES:
        assert GO.path_of(S, go, ge, within)[1:] [0:2] == ((0, 0), (1, 1))
        assert GO.path_of(S, go, ge, within)[3].tolist() == [0, 0]
    # the all-gap path of Lq + Lr ops: nothing is worth a match; B first (E at the last cell
    # loses to F only where F is better: with equal costs the diagonal is out and E goes first)
    S = _matrix((2, 3), {}, fill=-50.0)
    score, start, end, ops = GO.path_of(S, go, ge, False)
    assert ops.size == 5 == sum(S.shape) and sorted(ops.tolist()) == [1, 1, 1, 2, 2]
    assert start == (0, 0) and end == (1, 2)
    assert _bits(score) == _bits(GO.rescore(S, ops, start, go, ge))
    assert float(score) == -(1.0 + 0.25) - (1.0 + 2 * 0.25)
    cells = align.path_cells(ops, start)
    assert sorted(cells[:, 0].tolist()) == [-1, -1, -1, 0, 1]
    # a within path that consumes no row of B: every row of A faces a gap, behind column j
    score, start, end, ops = GO.path_of(S, go, ge, True)
    assert ops.tolist() == [2, 2] and end == (1, 0) and start == (0, 1)
    assert start[1] == end[1] + 1 - np.count_nonzero(ops != 2)
    assert float(score) == -1.25 and _bits(GO.rescore(S, ops, start, go, ge)) == _bits(score)
    assert align.path_cells(ops, start).tolist() == [[0, -1], [1, -1]]
    # ... even behind the last column: start_j = Lr, which no op ever indexes
    S = _matrix((2, 1), {}, fill=-50.0)
    assert GO.path_of(S, go, ge, True)[1:3] == ((0, 1), (1, 0))
    # a side without rows: nothing to align
    for shape in ((0, 3), (3, 0), (0, 0)):
        for within in MODES:
            score, start, end, ops = GO.path_of(np.zeros(shape, dtype=np.float32), go, ge, within)
            assert score == 0 and start == end == (-1, -1) and ops.size == 0


# ---- the claims on random matrices with forced ties ---------------------------------------------

def _coarse_matrices():
    """300 float32 matrices of up to 40 x 60 on a grid of 1/4 (ties occur), a diagonal planted
    with holes, and in every third a shifted second stretch that a gap has to join."""
    rng = np.random.default_rng(161803)
    for case in range(300):
        lq, lr = int(rng.integers(1, 41)), int(rng.integers(1, 61))
        S = rng.integers(-6, 3, size=(lq, lr)) / 4.0
        length = min(lq, lr)
        at_i, at_j = int(rng.integers(0, lq - length + 1)), int(rng.integers(0, lr - length + 1))
        steps = np.arange(length)[rng.random(length) < 0.8]
        S[at_i + steps, at_j + steps] = rng.integers(1, 5, size=steps.size) / 4.0
        if case % 3 == 0 and lr > 8:
            shift = int(rng.integers(1, 4))
            late = steps[(steps >= length // 2) & (at_j + steps + shift < lr)]
            S[at_i + late, at_j + late] = -1.5
            S[at_i + late, at_j + late + shift] = 1.0
        yield S.astype(np.float32)


def test_rescoring_cells_and_ordering_on_random_matrices():
    parameters = ((1.0, 0.25), (0.75, 0.0), (0.5, 0.5), (1.0, 0.5))      # one with open == extend
    cases = gapped = bordered = tied = 0
    for number, S in enumerate(_coarse_matrices()):
        go, ge = parameters[number % len(parameters)]
        local = O.gotoh_f32(S, go, ge)[0]
        scores = {}
        for within in MODES:
            score, start, end, ops = GO.path_of(S, go, ge, within)
            where = (number, S.shape, go, ge, within)
            assert _bits(GO.rescore(S, ops, start, go, ge)) == _bits(score), where
            cells = align.path_cells(ops, start)
            consumed_a, consumed_b = cells[cells[:, 0] >= 0, 0], cells[cells[:, 1] >= 0, 1]
            assert consumed_a.tolist() == list(range(S.shape[0])), where
            assert consumed_b.tolist() == list(range(start[1], end[1] + 1)), where
            assert tuple(cells[-1]) == end or ops[-1] != 0, where
            assert (consumed_a[-1], max(consumed_b.tolist() + [end[1]])) == end, where
            assert start[1] == end[1] + 1 - np.count_nonzero(ops != 2), where
            assert ops.size <= sum(S.shape)
            scores[within] = score
            gapped += bool(np.any(ops != 0))
            bordered += bool(ops[0] != 0)
            H = GO.matrices(S, go, ge, np.float32, within)[0]
            tied += int(within and np.count_nonzero(H[-1, 1:] == H[-1, 1:].max()) > 1)
            cases += 1
        assert scores[False] <= scores[True] <= local, (number, scores, local)
    assert cases == 600 and gapped >= 300 and bordered >= 100 and tied >= 5, \
        (cases, gapped, bordered, tied)


def test_float64_runs_the_same_program():
    """The dtype parameter: on values that add exactly both precisions give the same numbers."""
    S = next(iter(_coarse_matrices()))
    for within in MODES:
        one = GO.path_of(S, 1.0, 0.25, within)
        two = GO.path_of(S.astype(np.float64), 1.0, 0.25, within, np.float64)
        assert float(one[0]) == float(two[0]) and one[1:3] == two[1:3]
        assert one[3].tolist() == two[3].tolist()


# ---- the Python functions: errors before a device is touched ------------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


@pytest.mark.parametrize("name", ("global_align", "global_paths"))
def test_python_refuses_what_local_align_refuses(monkeypatch, name):
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    assert name in align.__all__
    function = getattr(align, name)
    good, other, long = _rows_f16(6), _rows_f16(5), _rows_f16(4100)
    base = dict(counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0, gap_extend=0.5)
    refused = 0

    def same_error(*rows, **changes):
        nonlocal refused
        arguments = {**base, **changes}
        with pytest.raises(ValueError) as wanted:
            align.local_align(*(rows or (good,)), **arguments)
        for within in MODES:
            with pytest.raises(ValueError) as got:
                function(*(rows or (good,)), within=within, **arguments)
            assert str(got.value) == str(wanted.value)
        refused += 1
        return str(wanted.value)

    for missing in ("gap_open", "gap_extend", "pairs"):
        with pytest.raises(TypeError):
            function(good, **{k: v for k, v in base.items() if k != missing})
    for missing in ("gap_open", "gap_extend"):
        assert f"{missing} is required" in same_error(**{missing: None})
    for parameter in ("gap_open", "gap_extend", "match_scale", "match_shift"):
        for value in (float("inf"), float("nan"), "1", True, 1e39):
            assert f"{parameter} must be" in same_error(**{parameter: value})
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
    for within in (None, 0, 1, "yes", 1.0, np.int32(1)):
        with pytest.raises(ValueError, match="within must be"):
            function(good, within=within, **base)
    if name == "global_paths":
        for cap in (0, -1, 1.5, True, None):
            with pytest.raises(ValueError, match="max_workspace_bytes"):
                function(good, max_workspace_bytes=cap, **base)
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            function(good, **base)
        with pytest.raises((RuntimeError, AssertionError)):      # P == 0 returns device tensors
            function(good, **{**base, "pairs": []})


def test_global_paths_copies_nothing_to_the_host_between_its_launches():
    """By construction, read and not timed: up to the trace launch the function's source names no
    way to the host, and the slots and boxes come from the counts."""
    import inspect
    source = inspect.getsource(align.global_paths)
    before, after = source.split("return _traced(", 1)
    body = before.split('"""', 2)[2]
    for word in (".cpu(", ".numpy(", ".item(", ".tolist(", "bool(", "synchronize"):
        assert word not in body, word
    assert '_launch(call, "global", within' in body and "rows_a + rows_b" in body
    launch = inspect.getsource(align._launch) + inspect.getsource(align._symbol)
    for word in (".cpu(", ".numpy(", ".item(", ".tolist(", "bool(", "synchronize"):
        assert word not in launch, word


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_binds_and_names_what_it_refuses_without_a_gpu():
    lib = native.library()
    for name in ("gfy_align_global", "gfy_align_global_trace",
                 "gfy_align_global_trace_workspace_bytes"):
        assert name in native.SIGNATURES and getattr(lib, name) is not None
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    sizer = lib.gfy_align_global_trace_workspace_bytes
    assert sizer(1, 100, 200) == lib.gfy_align_trace_workspace_bytes(1, 100, 200)
    assert sizer(10 ** 9, 10 ** 9, 10 ** 9) == lib.gfy_align_trace_workspace_bytes(10 ** 9, 4096, 4096)
    wave = sizer(1, 100, 200) // 4

    def score_call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p,
                   P=10, scale=1.0, shift=0.0, go=1.0, ge=0.5, within=0, score=p, end=p, ws=p,
                   size=lib.gfy_align_workspace_bytes(10, 0)):
        return lib.gfy_align_global(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P,
                                    scale, shift, go, ge, within, score, end, ws, size, None)

    def trace_call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p,
                   P=10, scale=1.0, shift=0.0, go=1.0, ge=0.5, within=0, ends=p, op_ptr=p, ops=p,
                   length=p, start=p, rows=100, cols=200, ws=p, size=wave):
        return lib.gfy_align_global_trace(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs,
                                          P, scale, shift, go, ge, within, ends, op_ptr, ops,
                                          length, start, rows, cols, ws, size, None)

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
    for call, who in ((score_call, b"gfy_align_global"), (trace_call, b"gfy_align_global_trace")):
        for hole, text in holes[call].items():
            refusal(call, who, native.GFY_ERR_INVALID, text, **{hole: None})
        for n, m in ((0, 5), (5, 0), (-1, 5), (5, 1 << 31)):
            refusal(call, who, native.GFY_ERR_INVALID, b"bad arguments", n=n, m=m)
        for name in ("records_a", "records_b"):
            for count in (0, -1, 1 << 31):
                refusal(call, who, native.GFY_ERR_INVALID, name.encode(), **{name: count})
        for P in (0, -1, 1 << 31):
            refusal(call, who, native.GFY_ERR_INVALID, b"P = ", P=P)
        for name in ("scale", "shift", "go", "ge"):
            for value in (float("inf"), float("nan")):
                refusal(call, who, native.GFY_ERR_INVALID, b"finite", **{name: value})
        for go, ge in ((1.0, 1.5), (1.0, -0.5)):
            refusal(call, who, native.GFY_ERR_INVALID, b"gap_extend", go=go, ge=ge)
        for within in (2, -1):
            refusal(call, who, native.GFY_ERR_INVALID, b"within", within=within)
        for short in (0, 1):
            refusal(call, who, native.GFY_ERR_WORKSPACE, b"workspace", size=short)
    refusal(trace_call, b"gfy_align_global_trace", native.GFY_ERR_INVALID, b"negative", rows=-1)
    refusal(trace_call, b"gfy_align_global_trace", native.GFY_ERR_INVALID, b"negative", cols=-1)
    refusal(trace_call, b"gfy_align_global_trace", native.GFY_ERR_WORKSPACE, b"workspace",
            size=wave - 1)
    refusal(trace_call, b"gfy_align_global_trace", native.GFY_ERR_WORKSPACE, b"workspace", rows=110)


# ---- registers ----------------------------------------------------------------------------------

def _resource_line(tmp_path, source, kernel):
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE=source,
               GFY_ASM_OUT=str(tmp_path / (source + ".s")))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    lines = [line for line in done.stdout.splitlines() if kernel + "E" in line]   # E: the name's end
    assert len(lines) == 1, done.stdout          # one kernel of that name
    fields = lines[0].split()
    return lines[0], {word: int(fields[fields.index(word) + 1])
                      for word in ("vgpr", "spilled", "scratch", "barrier", "mfma", "ds128")}


@pytest.mark.parametrize("source, kernel, twin, twin_kernel", (
    ("align_kernels.hip", "k_align_global", "align_kernels.hip", "k_align_local"),
    ("align_kernels.hip", "k_align_global_trace", "align_kernels.hip", "k_align_trace")))
def test_the_global_kernels_keep_out_of_scratch(tmp_path, source, kernel, twin, twin_kernel):
    """No spill, no scratch, no workgroup barrier, at most the 512 registers of a SIMD's one
    wave, and the multiply of the local twin: the same MFMA and 16-byte LDS read counts."""
    line, mine = _resource_line(tmp_path, source, kernel)
    twin_line, theirs = _resource_line(tmp_path, twin, twin_kernel)
    assert kernel in line and twin_kernel in twin_line
    assert mine["vgpr"] <= 512 and mine["spilled"] == 0 and mine["scratch"] == 0, line
    assert mine["barrier"] == 0, line
    assert (mine["mfma"], mine["ds128"]) == (theirs["mfma"], theirs["ds128"]), (line, twin_line)
