"""Top-k nearest-row search (csrc/pairwise_topk.hip, distance.topk, parallel.cross_shard_topk):
what needs no GPU.  Argument errors through the C ABI and through Python are raised before a
device is touched, the sweep kernels keep their register budget as hipcc allocates them, and
the chunked cross-shard merge is run over gloo with a float64 stand-in for the kernel."""
from __future__ import annotations

import ctypes
import os
import socket
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ginfinity_amd import _native as native
from ginfinity_amd import parallel

ROOT = Path(__file__).resolve().parents[1]


# ---- C ABI --------------------------------------------------------------------------------------

def _fake(address=0x1000):
    """A non-null pointer value: every check below fails before anything is dereferenced."""
    return ctypes.c_void_p(address)


def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = _fake()
    need = lib.gfy_pairwise_topk_workspace_bytes(300, 500, 8)
    for k in (0, 17, -1, -16, 1 << 20):
        assert lib.gfy_pairwise_topk(p, 300, p, 500, native.GFY_L2, k, -1, p, p, p, need,
                                     None) == native.GFY_ERR_INVALID, k
        assert b"k = " in lib.gfy_last_error()
        assert lib.gfy_pairwise_topk_window(p, 500, p, 300, native.GFY_COSINE, k, 0, p, p, p,
                                            need, None) == native.GFY_ERR_INVALID, k
    for hole in range(5):          # a, b, top_val, top_idx, workspace
        args = [p] * 5
        args[hole] = None
        a, b, val, idx, ws = args
        assert lib.gfy_pairwise_topk(a, 300, b, 500, native.GFY_L2, 8, -1, val, idx, ws, need,
                                     None) == native.GFY_ERR_INVALID, hole
        assert lib.gfy_pairwise_topk_window(a, 500, b, 300, native.GFY_L2, 8, 0, val, idx, ws,
                                            need, None) == native.GFY_ERR_INVALID, hole
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, 1 << 31)):
        assert lib.gfy_pairwise_topk(p, n, p, m, native.GFY_L2, 8, -1, p, p, p, 1 << 40,
                                     None) == native.GFY_ERR_INVALID, (n, m)
    assert lib.gfy_pairwise_topk(p, 300, p, 500, 7, 8, -1, p, p, p, need,
                                 None) == native.GFY_ERR_INVALID            # unknown metric
    # a window that is not inside a
    assert lib.gfy_pairwise_topk_window(p, 300, p, 200, native.GFY_L2, 8, 101, p, p, p, 1 << 40,
                                        None) == native.GFY_ERR_INVALID
    for short in (0, 1, need - 1):
        assert lib.gfy_pairwise_topk(p, 300, p, 500, native.GFY_L2, 8, -1, p, p, p, short,
                                     None) == native.GFY_ERR_WORKSPACE, short
        assert b"workspace" in lib.gfy_last_error()
        assert lib.gfy_pairwise_topk_window(p, 500, p, 300, native.GFY_L2, 8, 100, p, p, p, short,
                                            None) == native.GFY_ERR_WORKSPACE, short


def test_workspace_size_is_positive_and_grows_with_k():
    lib = native.library()
    assert native.GFY_PAIRWISE_TOPK_MAX == 16
    for n, m in ((1, 1), (130, 257), (65_536, 4_607), (1_000_000, 1_000_000)):
        sizes = [lib.gfy_pairwise_topk_workspace_bytes(n, m, k) for k in range(1, 17)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (n, m, sizes)
        assert n < 64 or sizes[-1] > sizes[0]        # below 256 bytes the arrays' rounding hides k
    # the nearest-row workspace keeps its own size function
    assert lib.gfy_pairwise_workspace_bytes(65_536, 4_607) > 0


# ---- distance.topk: errors before a device is touched -------------------------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


@pytest.mark.parametrize("k", [0, 17, -1, 2.5, None, True, "8"])
def test_topk_refuses_a_bad_k(k):
    from ginfinity_amd import distance
    with pytest.raises(ValueError, match="k must be"):
        distance.topk(_rows_f16(4), k=k)


def test_topk_refuses_bad_rows_and_conflicting_exclusions():
    """On a machine without a GPU a touched device is a RuntimeError, not the ValueError asked for."""
    from ginfinity_amd import distance
    good = _rows_f16(4)
    with pytest.raises(ValueError, match="float16"):
        distance.topk(good.float(), k=2)
    with pytest.raises(ValueError, match="float16"):
        distance.topk(good, good.float(), k=2)
    with pytest.raises(ValueError, match="shape"):
        distance.topk(torch.zeros((4, 64), dtype=torch.float16), k=2)
    with pytest.raises(ValueError, match="shape"):
        distance.topk(good, torch.zeros(128, dtype=torch.float16), k=2)
    with pytest.raises(ValueError, match="window_first"):
        distance.topk(good, good[1:3], k=2, window_first=1, exclude_self=True)
    with pytest.raises(ValueError, match="window_first"):
        distance.topk(good, good[1:3], k=2, window_first=1, exclude_offset=0)
    with pytest.raises(ValueError, match="metric"):
        distance.topk(good, k=2, metric="dot")
    assert "topk" in distance.__all__


# ---- registers ----------------------------------------------------------------------------------

def test_topk_kernels_keep_their_register_and_scratch_budget(tmp_path):
    """Every instantiation of the sweep (list depths 4 / 8 / 16, both key forms): at most 256
    VGPRs (two waves per SIMD is what one 512-thread workgroup per CU needs), nothing spilled, no
    scratch — a scratch reload is a vmcnt(0) wait that drains the LDS-DMA look-ahead."""
    script = ROOT / "tools" / "pairwise_resources.sh"
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE="pairwise_topk.hip",
               GFY_ASM_OUT=str(tmp_path / "pairwise_topk.s"))
    done = subprocess.run(["bash", str(script)], capture_output=True, text=True, timeout=900,
                          env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    sweeps = [line for line in done.stdout.splitlines() if "k_pairwise_topk" in line]
    assert len(sweeps) == 6, done.stdout            # <4 | 8 | 16, folded | (s, t)>
    kernels = [line for line in done.stdout.splitlines() if " vgpr " in line]
    assert len(kernels) == 7, done.stdout           # ... and k_topk_finish
    for line in kernels:
        fields = line.split()
        vgprs = int(fields[fields.index("vgpr") + 1])
        spilled = int(fields[fields.index("spilled") + 1])
        scratch = int(fields[fields.index("scratch") + 1])
        assert vgprs <= 256 and spilled == 0 and scratch == 0, line


# ---- cross_shard_topk over gloo -----------------------------------------------------------------

def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(rank: int, count: int, ties: bool) -> torch.Tensor:
    """Random rows.  ``ties``: rows 1 and 4 of EVERY rank are the same two rows, so every rank's
    copies tie and the lowest global row has to come first.  (For cosine, where the float64
    oracle gives 1 +- 1e-16 for a copy, which is exactly 1 in float32; its L2 distance of a copy
    is the square root of rounding noise, no tie.)"""
    rng = np.random.default_rng(100 + rank)
    rows = rng.standard_normal((count, 128)).astype(np.float16)
    shared = np.random.default_rng(99).standard_normal((2, 128)).astype(np.float16)
    for slot, at in enumerate((1, 4)):
        if ties and at < count:
            rows[at] = shared[slot]
    return torch.from_numpy(rows)


def _ranked(full: np.ndarray, k: int, metric: str):
    """The k best columns of every row of a float32 matrix by (value, column), stable; a column
    that holds +-inf (excluded) is no candidate: index -1."""
    order = np.argsort(full if metric == "l2" else -full, axis=1, kind="stable")[:, :k]
    values = np.take_along_axis(full, order, axis=1)
    order = np.where(np.isinf(values), -1, order)
    nothing = np.float32(np.inf if metric == "l2" else -np.inf)
    short = k - order.shape[1]
    if short > 0:
        values = np.pad(values, ((0, 0), (0, short)), constant_values=nothing)
        order = np.pad(order, ((0, 0), (0, short)), constant_values=-1)
    return values.astype(np.float32), order


def _oracle_topk(a, b, *, k, metric="l2", exclude_offset=None, window_first=None):
    """The semantics of distance.topk on CPU tensors with the float64 definition
    (oracle/gine_numpy.py) rounded to float32: the stand-in for the kernel."""
    from oracle import gine_numpy as G
    an, bn = a.numpy(), b.numpy()
    full = (G.pairwise_l2(an, bn) if metric == "l2" else G.pairwise_cosine(an, bn))
    full = full.astype(np.float32)
    if window_first is not None:           # b = rows [window_first, ...) of a: skip (k + j, j)
        exclude_offset = -int(window_first)
    if exclude_offset is not None and (exclude_offset >= 0 or window_first is not None):
        for i in range(an.shape[0]):
            if 0 <= i + exclude_offset < bn.shape[0]:
                full[i, i + exclude_offset] = np.inf if metric == "l2" else -np.inf
    values, order = _ranked(full, k, metric)
    return torch.from_numpy(values), torch.from_numpy(order.astype(np.int32))


def _topk_worker(rank: int, size: int, port: int, sizes: list[int], metric: str, k: int,
                 chunk_rows: int, queue) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        block = _rows(rank, sizes[rank], metric == "cosine")
        values, indices, offsets = parallel.cross_shard_topk(
            block, k, metric=metric, chunk_rows=chunk_rows, search=_oracle_topk)
        queue.put((rank, values.numpy(), indices.numpy(), offsets))
    except BaseException as error:       # the parent must not wait out its timeout for a dead rank
        queue.put((rank, repr(error), None, None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("sizes,chunk_rows,k", [([7, 7], 3, 4), ([5, 11], 4, 8), ([0, 6], 4, 3),
                                                ([9, 0, 4], 5, 16), ([3, 8, 5], 100, 5),
                                                ([2, 1], 1, 8)])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_cross_shard_topk_chunked_gloo(sizes, chunk_rows, k, metric):
    """Unequal and empty blocks, chunks smaller and larger than the blocks, two and three ranks,
    fewer rows in the world than k: every rank's rows get the single-process answer over the
    concatenated rows — the k best OTHER rows by (value, global row)."""
    from oracle import gine_numpy as G
    size = len(sizes)
    assert hasattr(parallel, "cross_shard_topk")          # before any rank is started
    context = mp.get_context("spawn")      # fresh children, as tests/test_parallel_cpu.py starts them
    queue = context.Queue()
    port = _free_port()
    procs = [context.Process(target=_topk_worker,
                             args=(r, size, port, sizes, metric, k, chunk_rows, queue))
             for r in range(size)]
    for p in procs:
        p.start()
    results = sorted((queue.get(timeout=180) for _ in procs), key=lambda item: item[0])
    for p in procs:
        p.join(timeout=60)
    assert not [item[1] for item in results if isinstance(item[1], str)]
    for p in procs:
        assert p.exitcode == 0
    everything = np.concatenate([_rows(r, sizes[r], metric == "cosine").numpy()
                                 for r in range(size)])
    full = (G.pairwise_l2(everything, everything) if metric == "l2"
            else G.pairwise_cosine(everything, everything)).astype(np.float32)
    np.fill_diagonal(full, np.inf if metric == "l2" else -np.inf)
    want_values, want = _ranked(full, k, metric)
    starts = np.concatenate(([0], np.cumsum(sizes)))
    # the shared rows do tie across ranks, and the lowest global row is in front
    copies = [starts[r] + 1 for r in range(size) if sizes[r] > 1]
    if len(copies) >= 2 and k >= len(copies) - 1 and metric == "cosine":
        assert list(want[copies[-1], :len(copies) - 1]) == copies[:-1]
        assert np.all(want_values[copies[-1], :len(copies) - 1] == 1)
    for rank, values, indices, offsets in results:
        assert offsets == list(starts)
        lo, hi = starts[rank], starts[rank + 1]
        assert indices.shape == (hi - lo, k) and indices.dtype == np.int64
        assert values.shape == (hi - lo, k) and values.dtype == np.float32
        np.testing.assert_array_equal(indices, want[lo:hi])
        np.testing.assert_array_equal(values, want_values[lo:hi])


def test_cross_shard_topk_world_size_one_needs_no_process_group():
    block = _rows(3, 13, False)
    for chunk_rows in (4, 13, 1 << 20):
        values, indices, offsets = parallel.cross_shard_topk(
            block, 5, metric="cosine", chunk_rows=chunk_rows, search=_oracle_topk)
        direct_v, direct_i = _oracle_topk(block, block, k=5, metric="cosine", exclude_offset=0)
        assert offsets == [0, 13]
        np.testing.assert_array_equal(indices.numpy(), direct_i.numpy().astype(np.int64))
        np.testing.assert_array_equal(values.numpy(), direct_v.numpy())
    empty = torch.zeros((0, 128), dtype=torch.float16)
    values, indices, offsets = parallel.cross_shard_topk(empty, 5, search=_oracle_topk)
    assert values.shape == (0, 5) and indices.shape == (0, 5) and offsets == [0, 0]
    assert values.dtype == torch.float32 and indices.dtype == torch.int64
    with pytest.raises(ValueError):
        parallel.cross_shard_topk(block, 17, search=_oracle_topk)
    with pytest.raises(ValueError):
        parallel.cross_shard_topk(block, 4, metric="dot", search=_oracle_topk)
