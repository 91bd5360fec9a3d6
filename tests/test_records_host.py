"""Record-to-record best-match scores (gfy_pairwise_record_best, gfy_pairwise_record_scores;
distance.record_best, distance.record_scores): what needs no GPU.  The C ABI and the two
functions refuse bad arguments before a device is touched, the planner that cuts ``a`` into
blocks of whole records is checked as the pure function it is, and the kernels of
pairwise_records.hip fit the register file as hipcc allocates them."""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from ginfinity_amd import _native as native
from ginfinity_amd import distance

ROOT = Path(__file__).resolve().parents[1]


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_pairwise_record_workspace_bytes(300, 500, 3, 7)
    assert need >= 300 * 7 * 4 + 2 * 512 * 4 + 300 * 4    # the intermediate, (s, t), the a-terms
    assert need == lib.gfy_pairwise_record_workspace_bytes(300, 500, 0, 7)

    def best(a=p, n=300, b=p, m=500, metric=native.GFY_L2, ptr_b=p, records_b=7, out=p, ws=p,
             size=need):
        return lib.gfy_pairwise_record_best(a, n, b, m, metric, ptr_b, records_b, out, ws, size,
                                            None)

    def scores(a=p, n=300, b=p, m=500, metric=native.GFY_COSINE, ptr_a=p, records_a=3, ptr_b=p,
               records_b=7, out=p, ws=p, size=need):
        return lib.gfy_pairwise_record_scores(a, n, b, m, metric, ptr_a, records_a, ptr_b,
                                              records_b, out, ws, size, None)

    names = {"a": b"a is NULL", "b": b"b is NULL", "ptr_b": b"ptr_b is NULL",
             "ws": b"workspace is NULL"}
    for call, out_name, extra in ((best, b"out_best is NULL", {}),
                                  (scores, b"out_scores is NULL", {"ptr_a": b"ptr_a is NULL"})):
        for hole, message in {**names, "out": out_name, **extra}.items():
            assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
            assert message in lib.gfy_last_error(), (hole, lib.gfy_last_error())
        assert call(metric=7) == native.GFY_ERR_INVALID
        assert b"metric" in lib.gfy_last_error()
        for n, m in ((0, 5), (5, 0), (-1, 5), (5, -1), (5, 1 << 31), (1 << 31, 5)):
            assert call(n=n, m=m, size=1 << 50) == native.GFY_ERR_INVALID, (n, m)
        for records_b in (0, -1, native.GFY_PAIRWISE_RECORDS_MAX + 1):
            assert call(records_b=records_b, size=1 << 50) == native.GFY_ERR_INVALID, records_b
            assert b"records_b" in lib.gfy_last_error()
        for short in (0, 1, need - 1):
            assert call(size=short) == native.GFY_ERR_WORKSPACE, short
            assert b"workspace" in lib.gfy_last_error()
    for records_a in (0, -1):
        assert scores(records_a=records_a) == native.GFY_ERR_INVALID, records_a
        assert b"records_a" in lib.gfy_last_error()
    assert lib.gfy_pairwise_record_chunks(257, 385) >= 1
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


# ---- distance.record_best / record_scores: errors before a device is touched --------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_python_refuses_bad_arguments_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(distance.native, "library", no_library)
    good, other = _rows_f16(4), _rows_f16(5)
    for name in ("record_best", "record_scores", "RecordWorkspace"):
        assert name in distance.__all__
    # counts that do not sum to the rows
    for counts in ([2, 1], [2, 3], []):
        with pytest.raises(ValueError, match=r"counts_b sums to \d+ rows, b has 4"):
            distance.record_best(good, counts_b=counts)
        with pytest.raises(ValueError, match=r"counts_b sums to \d+ rows, b has 4"):
            distance.record_scores(good, counts_a=[4], counts_b=counts)
        with pytest.raises(ValueError, match=r"counts_a sums to \d+ rows, a has 4"):
            distance.record_scores(good, other, counts_a=counts, counts_b=[5])
    with pytest.raises(ValueError, match="counts_b sums to 4 rows, b has 5"):
        distance.record_best(good, other, counts_b=[2, 2])
    with pytest.raises(ValueError, match="counts_b sums to 4 rows, b has 5"):
        distance.record_scores(good, other, counts_a=[4], counts_b=[4])
    with pytest.raises(ValueError, match="counts_b is required"):
        distance.record_scores(good, other, counts_a=[4])
    # counts that are none
    for counts in ([2, -2, 4], [2.0, 2.0], [[2, 2]], ["4"], [True, True, True, True]):
        with pytest.raises(ValueError, match="record counts"):
            distance.record_best(good, counts_b=counts)
        with pytest.raises(ValueError, match="record counts"):
            distance.record_scores(good, counts_a=counts)
        with pytest.raises(ValueError, match="record counts"):
            distance.record_scores(good, counts_a=[4], counts_b=counts)
    # dtype, shape, metric
    for function, arguments in ((distance.record_best, dict(counts_b=[4])),
                                (distance.record_scores, dict(counts_a=[4]))):
        with pytest.raises(ValueError, match="float16"):
            function(good.float(), **arguments)
        with pytest.raises(ValueError, match="float16"):
            function(good, good.float(), **arguments, **({} if "counts_b" in arguments
                                                         else {"counts_b": [4]}))
        with pytest.raises(ValueError, match=r"shape \(rows, 128\)"):
            function(torch.zeros((4, 64), dtype=torch.float16), **arguments)
        with pytest.raises(ValueError, match="metric"):
            function(good, metric="dot", **arguments)
    with pytest.raises(TypeError):
        distance.record_best(good)                      # counts_b is required
    with pytest.raises(TypeError):
        distance.record_scores(good)                    # counts_a is required
    # the budget
    for budget in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            distance.record_scores(good, counts_a=[1, 3], max_workspace_bytes=budget)
    with pytest.raises(ValueError, match=r"record 1 of a has 3 rows and needs 24 bytes"):
        distance.record_scores(good, counts_a=[1, 3], max_workspace_bytes=23)
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            distance.record_scores(good, counts_a=np.array([1, 3]))
        with pytest.raises((RuntimeError, AssertionError)):
            distance.record_best(good, counts_b=torch.tensor([1, 0, 3]))


# ---- the a-block planner ------------------------------------------------------------------------

def _check_plan(counts, records_b, budget):
    blocks = distance.plan_record_blocks(counts, records_b, budget)
    assert blocks == distance.plan_record_blocks(list(counts), records_b, budget)   # pure
    ptr = np.concatenate(([0], np.cumsum(np.asarray(counts, dtype=np.int64))))
    if not len(counts):
        assert blocks == []
        return blocks
    # whole records, every record once, in order
    assert [first for first, _ in blocks] == [0] + [last for _, last in blocks[:-1]]
    assert all(first < last for first, last in blocks)
    assert (blocks[-1][1] if blocks else 0) == len(counts)
    for first, last in blocks:
        assert (ptr[last] - ptr[first]) * records_b * 4 <= budget, (first, last)
    # as many as fit: the next block's first record with rows would not have fitted
    for (first, last), (_, after) in zip(blocks, blocks[1:]):
        grown = next(q for q in range(last, after) if counts[q] > 0)
        assert (ptr[grown + 1] - ptr[first]) * records_b * 4 > budget
    return blocks


def test_record_blocks_are_whole_records_within_the_budget():
    sizes = (1, 2, 37, 100, 128, 129, 300)
    counts = [sizes[q % 7] for q in range(40)]
    for records_b in (1, 7, 90):
        for rows in (300, 301, 697, 1_000, 10 ** 6):
            _check_plan(counts, records_b, rows * records_b * 4)
    assert _check_plan(counts, 7, 10 ** 9) == [(0, 40)]
    assert len(_check_plan(counts, 7, 300 * 7 * 4)) >= 10
    # records of zero rows ride along and never open a block of their own at the end
    holes = [0, 0, 5, 0, 5, 0, 0, 5, 0]
    assert _check_plan(holes, 3, 5 * 3 * 4) == [(0, 4), (4, 7), (7, 9)]
    assert _check_plan([0, 0, 0], 3, 0) == [(0, 3)]
    assert _check_plan([], 3, 100) == []
    assert _check_plan([4, 4], 0, 0) == [(0, 2)]           # no records of b: nothing to hold
    rng = np.random.default_rng(7)
    for _ in range(20):
        counts = rng.integers(0, 50, size=rng.integers(1, 60)).tolist()
        _check_plan(counts, int(rng.integers(1, 9)), int(rng.integers(49, 400)) * 8 * 4)


def test_an_oversize_record_is_refused_with_its_bytes():
    with pytest.raises(ValueError, match=r"record 2 of a has 301 rows and needs 8428 bytes"):
        distance.plan_record_blocks([300, 1, 301, 5], 7, 300 * 7 * 4)
    with pytest.raises(ValueError, match="max_workspace_bytes is 0"):
        distance.plan_record_blocks([1], 1, 0)
    with pytest.raises(ValueError, match="record counts"):
        distance.plan_record_blocks([1, -1], 1, 100)


# ---- workspaces ---------------------------------------------------------------------------------

def _split_b(n, m, block_a):
    """(blocks_a, chunks, chunk_rows) of a sweep of n a-rows in blocks of ``block_a`` against m
    b-rows in 128-row tiles: at least 1,024 workgroups, of the next five chunk counts a later one
    only where its grid ends in 1 % fewer sweeps over 256 CUs, at most one chunk per tile, and the
    chunks evened out to whole tiles."""
    blocks_a, tiles_b = -(-n // block_a), -(-m // 128)
    least = -(-1024 // blocks_a)
    best, chunks = 1e300, least
    for c in range(least, least + 6):
        sweeps = -(-blocks_a * c // 256) / c
        if sweeps < best * 0.99:
            best, chunks = sweeps, c
    chunks = max(1, min(chunks, tiles_b))
    tiles_per_chunk = -(-tiles_b // chunks)
    return blocks_a, -(-tiles_b // tiles_per_chunk), tiles_per_chunk * 128


def _workspace(n, m, *arrays):
    """s and t of b padded to whole tiles, the a-side term, then ``arrays`` (bytes each): every
    array rounded up to 256 bytes."""
    padded = -(-m // 128) * 128 * 4
    return sum(-(-size // 256) * 256 for size in (padded, padded, n * 4, *arrays))


def test_workspace_sizes_follow_the_layout_rule():
    """The three workspace functions and gfy_pairwise_record_chunks against the rule stated
    above: 256 a-rows per workgroup for nearest, 128 for top-k and the records."""
    lib = native.library()
    for n, m in ((1, 1), (130, 257), (300, 700), (65_536, 4_607), (1_000_000, 1_000_000)):
        chunks = _split_b(n, m, 256)[1]
        assert lib.gfy_pairwise_workspace_bytes(n, m) == \
            _workspace(n, m, chunks * n * 4, chunks * n * 4), (n, m)
        chunks = _split_b(n, m, 128)[1]
        assert lib.gfy_pairwise_record_chunks(n, m) == chunks, (n, m)
        for k in (1, 4, 8, 16):
            assert lib.gfy_pairwise_topk_workspace_bytes(n, m, k) == \
                _workspace(n, m, chunks * n * k * 4, chunks * n * k * 4), (n, m, k)
        for records_b in (1, 7):
            assert lib.gfy_pairwise_record_workspace_bytes(n, m, 3, records_b) == \
                _workspace(n, m, records_b * n * 4), (n, m, records_b)
    assert _split_b(300, 700, 128) == (3, 6, 128) and _split_b(300, 700, 256) == (2, 6, 128)
    assert _split_b(1_000_000, 1_000_000, 256)[:2] == (3907, 3)


# ---- registers ----------------------------------------------------------------------------------

def test_every_record_kernel_fits_the_register_file(tmp_path):
    """pairwise_records.hip holds the sweep, folded (l2) and not (cosine), and the two finish
    kernels: each at most 256 VGPRs (two waves per SIMD is what one 512-thread workgroup per CU
    needs), nothing spilled, no scratch."""
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE="pairwise_records.hip",
               GFY_ASM_OUT=str(tmp_path / "pairwise_records.s"))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    found = {}
    for line in done.stdout.splitlines():
        fields = line.split()
        budget = tuple(int(fields[fields.index(word) + 1]) for word in ("vgpr", "spilled", "scratch"))
        for name in ("k_record_sweepILb1E", "k_record_sweepILb0E", "k_record_finish_best",
                     "k_record_finish_scores"):
            if name in line:
                assert name not in found, line
                found[name] = budget
                break
        else:
            raise AssertionError(f"a kernel nobody expected: {line}")
    assert len(found) == 4, found
    for name, (vgprs, spilled, scratch) in found.items():
        assert vgprs <= 256 and spilled == 0 and scratch == 0, (name, vgprs, spilled, scratch)
