"""The local aligner (gfy_align_local, align.local_align, align.top_pairs): what needs no GPU.
The two oracles of tests/align_oracle.py agree with a walk over every path of tiny matrices and
keep the end rule; the C ABI and the Python functions refuse bad arguments before a device is
touched; ``top_pairs`` is checked as the pure function it is; the kernel fits the register file
without scratch as hipcc allocates it."""
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
from ginfinity_amd import _native as native
from ginfinity_amd import align

ROOT = Path(__file__).resolve().parents[1]


# ---- the oracles --------------------------------------------------------------------------------

def test_oracles_agree_with_every_path_of_tiny_matrices():
    """Scores are multiples of 1/4 and gap costs of 1/8, so float32, float64 and the path sums
    are all exact and must agree to the bit; the float64 oracle is fed rows whose cosines are
    exactly 0 or 1 (signed unit vectors), scaled and shifted."""
    rng = np.random.default_rng(11)
    cases = 0
    for lq, lr in itertools.product((1, 2, 3, 4), repeat=2):
        for go, ge in ((1.0, 0.25), (0.5, 0.5), (0.75, 0.0), (2.0, 1.0)):
            S = (rng.integers(-6, 9, size=(lq, lr)) / 4.0).astype(np.float32)
            walked = O.enumerate_paths(S.astype(np.float64), go, ge)
            H32 = O._gotoh(S, go, ge, np.float32)
            H64 = O._gotoh(S.astype(np.float64), go, ge, np.float64)
            assert np.array_equal(H32.astype(np.float64), walked), (lq, lr, go, ge)
            assert np.array_equal(H64, walked), (lq, lr, go, ge)
            score, end = O.gotoh_f32(S, go, ge)
            walked_score, walked_end = O.end_of(walked)
            assert float(score) == float(walked_score) and end == walked_end, (lq, lr, go, ge)
            cases += 1
    assert cases == 64
    # float64 from rows: unit vectors e_k with signs, cosines in {-1, 0, 1}
    for lq, lr in ((2, 3), (4, 4), (3, 1)):
        A = np.zeros((lq, 128), dtype=np.float16)
        B = np.zeros((lr, 128), dtype=np.float16)
        A[np.arange(lq), rng.integers(0, 3, lq)] = rng.choice([-1.0, 1.0], lq)
        B[np.arange(lr), rng.integers(0, 3, lr)] = rng.choice([-1.0, 1.0], lr)
        S = O.cosine_f64(A, B) * 1.5 - 0.25
        assert set(np.unique(S)) <= {-1.75, -0.25, 1.25}
        score, end, H = O.gotoh_f64(A, B, 1.0, 0.25, match_scale=1.5, match_shift=-0.25)
        assert np.array_equal(H, O.enumerate_paths(S, 1.0, 0.25))
        assert (score, end) == O.end_of(H)


def test_end_rule_on_a_hand_made_tie():
    """Two diagonals of the same score: the end is the first cell by (i, then j); a matrix with
    nothing positive ends nowhere."""
    S = np.full((4, 5), -1.0, dtype=np.float32)
    S[0, 3] = S[1, 4] = 1.0          # ends at (1, 4) with 2
    S[1, 0] = S[2, 1] = 1.0          # ends at (2, 1) with 2
    assert O.gotoh_f32(S, 1.0, 0.5) == (np.float32(2.0), (1, 4))
    S[2, 1] = -1.0
    S[1, 1] = 1.0
    S[0, 0] = 1.0                    # now (1, 1) holds 2 as well: same row, lower j
    assert O.gotoh_f32(S, 1.0, 0.5) == (np.float32(2.0), (1, 1))
    assert O.gotoh_f32(np.full((3, 3), -0.5, dtype=np.float32), 1.0, 0.5) == (np.float32(0), (-1, -1))
    assert O.gotoh_f32(np.zeros((3, 3), dtype=np.float32), 1.0, 0.5) == (np.float32(0), (-1, -1))
    assert O.gotoh_f32(np.zeros((0, 3), dtype=np.float32), 1.0, 0.5) == (np.float32(0), (-1, -1))
    # a gap is opened where it pays: 3 + 3 - 1 over one skipped column
    S = np.full((2, 3), -4.0, dtype=np.float32)
    S[0, 0] = S[1, 2] = 3.0
    assert O.gotoh_f32(S, 1.0, 0.5) == (np.float32(5.0), (1, 2))
    assert O.gotoh_f32(S, 3.5, 0.5) == (np.float32(3.0), (0, 0))


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    assert native.GFY_ALIGN_ROWS_MAX == 4096
    need = lib.gfy_align_workspace_bytes(10, 300)
    assert need >= 10 * 300 * 8 and need % 256 == 0
    assert lib.gfy_align_workspace_bytes(10 ** 9, 4096) == lib.gfy_align_workspace_bytes(10 ** 8, 4096)
    assert lib.gfy_align_workspace_bytes(10 ** 9, 10 ** 9) == lib.gfy_align_workspace_bytes(10 ** 9, 4096)

    def call(a=p, n=300, ptr_a=p, records_a=3, b=p, m=500, ptr_b=p, records_b=7, pairs=p, P=10,
             scale=1.0, shift=0.0, go=1.0, ge=0.5, score=p, end=p, ws=p, size=need):
        return lib.gfy_align_local(a, n, ptr_a, records_a, b, m, ptr_b, records_b, pairs, P, scale,
                                   shift, go, ge, score, end, ws, size, None)

    for hole, message in {"a": b"a is NULL", "b": b"b is NULL", "ptr_a": b"ptr_a is NULL",
                          "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL",
                          "score": b"out_score is NULL", "end": b"out_end is NULL",
                          "ws": b"workspace is NULL"}.items():
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
        assert message in lib.gfy_last_error(), (hole, lib.gfy_last_error())
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, -1), (5, 1 << 31), (1 << 31, 5)):
        assert call(n=n, m=m) == native.GFY_ERR_INVALID, (n, m)
    for name in ("records_a", "records_b"):
        for count in (0, -1, 1 << 31):
            assert call(**{name: count}) == native.GFY_ERR_INVALID, (name, count)
            assert name.encode() in lib.gfy_last_error()
    for P in (0, -1, 1 << 31):
        assert call(P=P) == native.GFY_ERR_INVALID, P
        assert b"P = " in lib.gfy_last_error()
    for name in ("scale", "shift", "go", "ge"):
        for value in (float("inf"), float("-inf"), float("nan")):
            assert call(**{name: value}) == native.GFY_ERR_INVALID, (name, value)
            assert b"finite" in lib.gfy_last_error()
    for go, ge in ((1.0, 1.5), (1.0, -0.5), (-1.0, -2.0)):
        assert call(go=go, ge=ge) == native.GFY_ERR_INVALID, (go, ge)
        assert b"gap_extend" in lib.gfy_last_error()
    for short in (0, 1, 255):
        assert call(size=short) == native.GFY_ERR_WORKSPACE, short
        assert b"workspace" in lib.gfy_last_error()
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


# ---- align.local_align / top_pairs: errors before a device is touched -------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_python_refuses_bad_arguments_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(align.native, "library", no_library)
    import ginfinity_amd
    assert ginfinity_amd.align is align
    for name in ("local_align", "AlignWorkspace", "top_pairs"):
        assert name in align.__all__
    good, other = _rows_f16(6), _rows_f16(5)
    base = dict(counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0, gap_extend=0.5)

    def refused(match, *rows, **changes):
        arguments = {**base, **changes}
        with pytest.raises(ValueError, match=match):
            align.local_align(*(rows or (good,)), **arguments)

    # the gap costs have no default, and None is none
    for missing in ("gap_open", "gap_extend"):
        with pytest.raises(TypeError):
            align.local_align(good, **{k: v for k, v in base.items() if k != missing})
        refused(f"{missing} is required", **{missing: None})
    with pytest.raises(TypeError):
        align.local_align(good, **{k: v for k, v in base.items() if k != "pairs"})
    # parameters
    for name in ("gap_open", "gap_extend", "match_scale", "match_shift"):
        for value in (float("inf"), float("nan"), "1", True, 1e39):
            refused(f"{name} must be", **{name: value})
    refused("gap_extend <= gap_open", gap_open=0.5, gap_extend=1.0)
    refused("gap_extend <= gap_open", gap_open=1.0, gap_extend=-0.25)
    # pairs
    for pairs in ([[0, 2]], [[2, 0]], [[-1, 0]], [[0, 0], [1, 5]]):
        refused("out of range", pairs=pairs)
    refused("out of range", good, other, counts_b=[5], pairs=[[0, 1]])
    for pairs in ([0, 1], [[0.0, 1.0]], [[0, 1, 1]], [[[0, 1]]], "01"):
        refused(r"shape \(P, 2\)", pairs=pairs)
    # counts
    refused(r"counts_a sums to 5 rows, a has 6", counts_a=[2, 3])
    refused(r"counts_b sums to 4 rows, b has 5", good, other, counts_b=[4])
    refused("counts_b is required", good, other)
    refused("record counts", counts_a=[2.0, 4.0])
    # a record over the limit, on either side, only where a pair names it
    long = _rows_f16(4100)
    refused(r"pair 1: record 1 of a has 4097 rows, more than 4096", long, counts_a=[3, 4097],
            pairs=[[0, 0], [1, 0]])
    refused(r"pair 0: record 1 of b has 4097 rows, more than 4096", good, long, counts_b=[3, 4097],
            pairs=[[0, 1]])
    # dtype and shape
    refused("float16", good.float())
    refused("float16", good, other.float(), counts_b=[5])
    refused(r"shape \(rows, 128\)", torch.zeros((6, 64), dtype=torch.float16))
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            align.local_align(good, **base)
        with pytest.raises((RuntimeError, AssertionError)):
            align.local_align(long, counts_a=[3, 4097], pairs=np.array([[0, 0]]), gap_open=1,
                              gap_extend=0)


def test_top_pairs_orders_and_breaks_ties():
    scores = np.array([[0.5, 0.9, 0.9, 0.1],
                       [0.2, 0.2, 0.2, 0.2],
                       [np.nan, 0.3, -np.inf, 0.7]], dtype=np.float32)
    got = align.top_pairs(scores, 2, largest=True)
    assert got.dtype == np.int32 and got.shape == (6, 2)
    assert got.tolist() == [[0, 1], [0, 2], [1, 0], [1, 1], [2, 3], [2, 1]]
    assert align.top_pairs(scores, 2, largest=False).tolist() == \
        [[0, 3], [0, 0], [1, 0], [1, 1], [2, 2], [2, 1]]
    # k beyond the columns: every column, NaN last
    assert align.top_pairs(scores, 9, largest=True)[8:].tolist() == \
        [[2, 3], [2, 1], [2, 2], [2, 0]]
    assert align.top_pairs(torch.from_numpy(scores), 1, largest=True).tolist() == \
        [[0, 1], [1, 0], [2, 3]]
    assert align.top_pairs(np.zeros((0, 4), dtype=np.float32), 2, largest=True).shape == (0, 2)
    assert align.top_pairs(np.zeros((3, 0), dtype=np.float32), 2, largest=True).shape == (0, 2)
    for k in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="k must be"):
            align.top_pairs(scores, k, largest=True)
    for largest in (None, 1, "yes"):
        with pytest.raises(ValueError, match="largest"):
            align.top_pairs(scores, 1, largest=largest)
    for matrix in (np.zeros(4, dtype=np.float32), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match="matrix"):
            align.top_pairs(matrix, 1, largest=True)
    with pytest.raises(TypeError):
        align.top_pairs(scores, 1)          # largest has no default: it depends on the metric


# ---- registers ----------------------------------------------------------------------------------

def test_the_align_kernel_keeps_out_of_scratch(tmp_path):
    """One 256-thread workgroup per CU (its LDS holds one): a wave may take the 512 registers of
    its SIMD, nothing is spilled, there is no scratch, and no workgroup barrier at all."""
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE="align_kernels.hip",
               GFY_ASM_OUT=str(tmp_path / "align_local.s"))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    lines = [line for line in done.stdout.splitlines() if "k_align_localE" in line]   # E: the name's end
    assert len(lines) == 1, done.stdout
    fields = lines[0].split()
    vgprs, spilled, scratch, barriers = (int(fields[fields.index(word) + 1])
                                         for word in ("vgpr", "spilled", "scratch", "barrier"))
    assert vgprs <= 512 and spilled == 0 and scratch == 0 and barriers == 0, lines[0]
