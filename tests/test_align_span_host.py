"""Start cells of the local aligner (gfy_align_local_span, align.local_spans): what needs no GPU.
The oracle of tests/align_span_oracle.py keeps H of ``align_oracle._gotoh`` to the bit, names a
start that a walk over every path of tiny matrices confirms, follows each tie rule of
include/gfy.h on hand-made matrices and satisfies the box property; the C ABI and the Python
function refuse what ``gfy_align_local`` and ``local_align`` refuse, before a device is touched;
the span kernel fits the register file without scratch as hipcc allocates it."""
from __future__ import annotations

import ctypes
import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import align_oracle as O
import align_span_oracle as SO
from ginfinity_amd import _native as native
from ginfinity_amd import align

ROOT = Path(__file__).resolve().parents[1]
GAPS = ((1.0, 0.25), (0.5, 0.5), (0.75, 0.0), (2.0, 1.0))


# ---- the oracle ---------------------------------------------------------------------------------

def _tiny_matrices():
    """The matrices of test_align_host.test_oracles_agree_with_every_path_of_tiny_matrices: the
    same generator, the same order of draws."""
    rng = np.random.default_rng(11)
    for lq, lr in itertools.product((1, 2, 3, 4), repeat=2):
        for go, ge in GAPS:
            yield (rng.integers(-6, 9, size=(lq, lr)) / 4.0).astype(np.float32), go, ge


def test_h_of_the_span_oracle_is_h_of_the_align_oracle():
    cases = 0
    for S, go, ge in _tiny_matrices():
        H, start_i, start_j = SO.gotoh_origins(S, go, ge, np.float32)
        want = O._gotoh(S, go, ge, np.float32)
        assert H.tobytes() == want.tobytes() and H.shape == want.shape, (S.shape, go, ge)
        assert np.array_equal(start_i >= 0, H > 0) and np.array_equal(start_j >= 0, H > 0)
        cases += 1
    assert cases == 64
    rng = np.random.default_rng(5)
    for go, ge in GAPS:
        S = rng.uniform(-1.3, 0.7, size=(40, 50)).astype(np.float32)
        S[np.arange(5, 35), np.arange(12, 42)] += np.float32(0.9)
        H, _, _ = SO.gotoh_origins(S, go, ge, np.float32)
        assert H.tobytes() == O._gotoh(S, go, ge, np.float32).tobytes()
        assert H.max() > 3
        score, start, end = SO.span_of(S, go, ge)
        assert (score, end) == O.gotoh_f32(S, go, ge)
    assert SO.span_of(np.zeros((0, 3), dtype=np.float32), 1.0, 0.5) == (np.float32(0), (-1, -1), (-1, -1))
    assert SO.span_of(np.full((3, 3), -0.5, dtype=np.float32), 1.0, 0.5)[1:] == ((-1, -1), (-1, -1))


def _first_cells_of_best_paths(S: np.ndarray, gap_open: float, gap_extend: float, end):
    """``align_oracle.enumerate_paths`` extended by what a path remembers: the first matched
    cell.  (best total of a path ending in cell ``end`` whose first move is a match, the set of
    first cells of the paths that reach it.)  Exponential; values that add exactly."""
    lq, lr = S.shape
    best, firsts = [-np.inf], [set()]

    def walk(gi, gj, last, total, first):
        if (gi - 1, gj - 1) == end and last is not None:
            if total > best[0]:
                best[0], firsts[0] = total, set()
            if total == best[0]:
                firsts[0].add(first)
        if gi > end[0] + 1 or gj > end[1] + 1:
            return
        if gi < lq and gj < lr:
            walk(gi + 1, gj + 1, "m", total + float(S[gi, gj]),
                 (gi, gj) if first is None else first)
        if first is None:
            return            # a path of positive total starts with a match
        if gj < lr:
            walk(gi, gj + 1, "r", total - (gap_extend if last == "r" else gap_open), first)
        if gi < lq:
            walk(gi + 1, gj, "d", total - (gap_extend if last == "d" else gap_open), first)

    for gi in range(lq):
        for gj in range(lr):
            walk(gi, gj, None, 0.0, None)
    return best[0], firsts[0]


def test_starts_are_first_cells_of_best_paths_of_tiny_matrices():
    """Values are multiples of 1/4 and gap costs of 1/8: every sum is exact, so the walk's best
    total is the oracle's score and its best paths are the candidates for the start."""
    positive = 0
    for S, go, ge in _tiny_matrices():
        score, start, end = SO.span_of(S, go, ge)
        if end == (-1, -1):
            assert start == (-1, -1)
            continue
        total, firsts = _first_cells_of_best_paths(S.astype(np.float64), go, ge, end)
        assert total == float(score), (S, go, ge)
        assert start in firsts, (S, go, ge, start, firsts)
        positive += 1
    assert positive >= 48


def test_tie_rules_on_hand_made_matrices():
    def matrix(shape, cells):
        S = np.full(shape, -9.0, dtype=np.float32)
        for cell, value in cells.items():
            S[cell] = value
        return S

    # diagonal, E and F all give H[1][1] = 2, from (0, 0), (1, 0) and (0, 1); (2, 2) makes that
    # cell's origin the start
    S = matrix((3, 3), {(0, 0): 1, (0, 1): 3, (1, 0): 3, (1, 1): 1, (2, 2): 5})
    H, start_i, start_j = SO.gotoh_origins(S, 1.0, 1.0, np.float32)
    assert H[1, 1] == 2 and H[0, 1] == 3 and H[1, 0] == 3
    assert SO.span_of(S, 1.0, 1.0) == (np.float32(7), (0, 0), (2, 2))
    S[1, 1] = 0.5                     # the diagonal gives 1.5: E and F tie at 2, E goes first
    assert SO.span_of(S, 1.0, 1.0) == (np.float32(7), (1, 0), (2, 2))
    S[1, 0] = 2.5                     # E gives 1.5 as well: F alone holds 2
    assert SO.span_of(S, 1.0, 1.0) == (np.float32(7), (0, 1), (2, 2))
    # open over extend with gap_open == gap_extend: H[1][1] = 3.5 from (0, 0) by the diagonal
    # (which also beats E = 3.5 from (1, 0)), E[1][1] = 3.5 from (1, 0); E[1][2] = 3 both ways,
    # and opening names (0, 0)
    S = matrix((3, 4), {(0, 0): 1, (1, 0): 4, (1, 1): 2.5, (2, 3): 5})
    H, start_i, start_j = SO.gotoh_origins(S, 0.5, 0.5, np.float32)
    assert H[1, 0] == 4 and H[1, 1] == 3.5 and H[1, 2] == 3
    assert (start_i[1, 0], start_j[1, 0]) == (1, 0) and (start_i[1, 1], start_j[1, 1]) == (0, 0)
    assert SO.span_of(S, 0.5, 0.5) == (np.float32(8), (0, 0), (2, 3))
    S[1, 1] = 2.25                    # no tie left: E = 3.5 from (1, 0) makes H[1][1], all of it
    assert SO.span_of(S, 0.5, 0.5) == (np.float32(8), (1, 0), (2, 3))
    # a predecessor of exactly 0 carries nothing: the alignment starts behind it
    S = matrix((3, 3), {(0, 0): 1, (1, 1): -1, (2, 2): 3})
    H, _, _ = SO.gotoh_origins(S, 1.0, 0.5, np.float32)
    assert H[0, 0] == 1 and H[1, 1] == 0
    assert SO.span_of(S, 1.0, 0.5) == (np.float32(3), (2, 2), (2, 2))
    S[1, 1] = -0.5                    # 0.5 is left: the path goes on
    assert SO.span_of(S, 1.0, 0.5) == (np.float32(3.5), (0, 0), (2, 2))


def test_box_property_on_random_matrices():
    """The recurrences on the box start..end alone end at exactly the score; start <= end; the
    start is a match that begins at 0."""
    rng = np.random.default_rng(2025)
    for lq, lr in ((30, 45), (64, 64), (70, 33), (5, 90)):
        for go, ge in GAPS:
            S = rng.uniform(-1.2, 0.5, size=(lq, lr)).astype(np.float32)
            length = min(lq, lr) - 3
            at_i, at_j = int(rng.integers(0, lq - length + 1)), int(rng.integers(0, lr - length + 1))
            keep = rng.random(length) < 0.85     # holes: the path needs gaps or mismatches
            S[at_i + np.arange(length)[keep], at_j + np.arange(length)[keep]] = \
                rng.uniform(0.5, 1.0, size=int(keep.sum())).astype(np.float32)
            H = O._gotoh(S, go, ge, np.float32)
            score, start, end = SO.span_of(S, go, ge)
            assert score > 1 and start[0] <= end[0] and start[1] <= end[1]
            assert S[start] == H[start] > 0
            box = np.ascontiguousarray(S[start[0]:end[0] + 1, start[1]:end[1] + 1])
            inside = O._gotoh(box, go, ge, np.float32)
            assert inside[-1, -1].tobytes() == np.float32(score).tobytes(), (lq, lr, go, ge)
            assert inside.max() == inside[-1, -1]


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_refuses_what_gfy_align_local_refuses():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    for P, L in ((10, 300), (1, 0), (1, 1), (1000, 4096), (10 ** 9, 4096), (3, 17)):
        need = lib.gfy_align_span_workspace_bytes(P, L)
        assert need >= 2 * lib.gfy_align_workspace_bytes(P, L) - 512 and need % 256 == 0, (P, L)
    assert lib.gfy_align_span_workspace_bytes(10, 300) >= 10 * 300 * 16
    assert lib.gfy_align_span_workspace_bytes(10 ** 9, 4096) == \
        lib.gfy_align_span_workspace_bytes(10 ** 8, 4096)
    assert lib.gfy_align_span_workspace_bytes(10 ** 9, 10 ** 9) == \
        lib.gfy_align_span_workspace_bytes(10 ** 9, 4096)
    need = lib.gfy_align_span_workspace_bytes(10, 300)

    def call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p, P=10,
             scale=1.0, shift=0.0, go=1.0, ge=0.5, score=p, start=p, end=p, ws=p, size=need):
        return lib.gfy_align_local_span(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P,
                                        scale, shift, go, ge, score, start, end, ws, size, None)

    def call_local(**changes):
        changes.pop("start", None)
        arguments = dict(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7,
                         pairs=p, P=10, scale=1.0, shift=0.0, go=1.0, ge=0.5, score=p, end=p,
                         ws=p, size=lib.gfy_align_workspace_bytes(10, 300))
        arguments.update(changes)
        return lib.gfy_align_local(*arguments.values(), None)

    def same_refusal(code, **changes):
        """Both calls refuse with ``code`` and, behind their own names, the same text."""
        assert call_local(**changes) == code, changes
        text = lib.gfy_last_error()
        assert text.startswith(b"gfy_align_local: ")
        assert call(**changes) == code, changes
        assert lib.gfy_last_error() == b"gfy_align_local_span: " + text[len(b"gfy_align_local: "):]
        return text

    for hole, message in {"a": b"a is NULL", "b": b"b is NULL", "ptr_a": b"ptr_a is NULL",
                          "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL",
                          "score": b"out_score is NULL", "end": b"out_end is NULL",
                          "ws": b"workspace is NULL"}.items():
        assert message in same_refusal(native.GFY_ERR_INVALID, **{hole: None}), hole
    assert call(start=None) == native.GFY_ERR_INVALID
    assert b"gfy_align_local_span: out_start is NULL" in lib.gfy_last_error()
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, -1), (5, 1 << 31), (1 << 31, 5)):
        same_refusal(native.GFY_ERR_INVALID, n=n, m=m)
    for name in ("records_a", "records_b"):
        for count in (0, -1, 1 << 31):
            assert name.encode() in same_refusal(native.GFY_ERR_INVALID, **{name: count})
    for P in (0, -1, 1 << 31):
        assert b"P = " in same_refusal(native.GFY_ERR_INVALID, P=P)
    for name in ("scale", "shift", "go", "ge"):
        for value in (float("inf"), float("-inf"), float("nan")):
            assert b"finite" in same_refusal(native.GFY_ERR_INVALID, **{name: value})
    for go, ge in ((1.0, 1.5), (1.0, -0.5), (-1.0, -2.0)):
        assert b"gap_extend" in same_refusal(native.GFY_ERR_INVALID, go=go, ge=ge)
    for short in (0, 1, 255):
        assert call(size=short) == native.GFY_ERR_WORKSPACE, short
        assert b"gfy_align_local_span: workspace" in lib.gfy_last_error()
        assert call_local(size=short) == native.GFY_ERR_WORKSPACE
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


# ---- align.local_spans: errors before a device is touched ---------------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_python_refuses_what_local_align_refuses(monkeypatch):
    """Every bad call raises from ``local_spans`` the ValueError, text included, that it raises
    from ``local_align``; the library is never asked for."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    assert "local_spans" in align.__all__ and "local_align" in align.__all__
    good, other, long = _rows_f16(6), _rows_f16(5), _rows_f16(4100)
    base = dict(counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0, gap_extend=0.5)
    refused = 0

    def same_error(*rows, **changes):
        nonlocal refused
        arguments = {**base, **changes}
        with pytest.raises(ValueError) as wanted:
            align.local_align(*(rows or (good,)), **arguments)
        with pytest.raises(ValueError) as got:
            align.local_spans(*(rows or (good,)), **arguments)
        assert str(got.value) == str(wanted.value)
        refused += 1
        return str(got.value)

    for missing in ("gap_open", "gap_extend", "pairs"):
        with pytest.raises(TypeError):
            align.local_spans(good, **{k: v for k, v in base.items() if k != missing})
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
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            align.local_spans(good, **base)


# ---- registers ----------------------------------------------------------------------------------

def test_the_span_kernel_keeps_out_of_scratch(tmp_path):
    """k_align_span of align_kernels.hip: no spill, no scratch, no workgroup barrier,
    and a wave within the 512 registers of its SIMD."""
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE="align_kernels.hip",
               GFY_ASM_OUT=str(tmp_path / "align_span.s"))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    lines = [line for line in done.stdout.splitlines() if "k_align_spanE" in line]   # E: the name's end
    assert len(lines) == 1, done.stdout
    fields = lines[0].split()
    vgprs, spilled, scratch, barriers = (int(fields[fields.index(word) + 1])
                                         for word in ("vgpr", "spilled", "scratch", "barrier"))
    assert vgprs <= 512 and spilled == 0 and scratch == 0 and barriers == 0, lines[0]
