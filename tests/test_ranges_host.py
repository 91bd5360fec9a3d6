"""Top-k search that skips a range of rows per row (gfy_pairwise_topk_ranges, distance.topk /
nearest with exclude_ranges / exclude_records, distance.record_ranges,
parallel.cross_shard_topk(record_counts=...)): what needs no GPU.  Argument errors are raised
before a device is touched, record_ranges is a numpy loop, the cross-shard search is run over
gloo with a float64 stand-in for the kernel, and the sweep kernels — those that were there and
the range ones — keep their register budget as hipcc allocates them."""
from __future__ import annotations

import ctypes
import os
import re
import socket
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ginfinity_amd import _native as native
from ginfinity_amd import distance, parallel

ROOT = Path(__file__).resolve().parents[1]


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_pairwise_topk_workspace_bytes(300, 500, 8)

    def call(a=p, n=300, b=p, m=500, metric=native.GFY_L2, k=8, lo=p, hi=p, val=p, idx=p, ws=p,
             size=need):
        return lib.gfy_pairwise_topk_ranges(a, n, b, m, metric, k, lo, hi, val, idx, ws, size, None)

    for hole in ("lo", "hi"):
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
        assert b"skip_lo or skip_hi" in lib.gfy_last_error()
    for hole in ("a", "b", "val", "idx", "ws"):
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
    for k in (0, 17, -1, 1 << 20):
        assert call(k=k) == native.GFY_ERR_INVALID, k
        assert b"k = " in lib.gfy_last_error()
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, 1 << 31)):
        assert call(n=n, m=m, size=1 << 40) == native.GFY_ERR_INVALID, (n, m)
    assert call(metric=7) == native.GFY_ERR_INVALID
    for short in (0, 1, need - 1):      # the workspace is that of gfy_pairwise_topk
        assert call(size=short) == native.GFY_ERR_WORKSPACE, short
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


# ---- record_ranges ------------------------------------------------------------------------------

@pytest.mark.parametrize("counts", [[], [0], [1], [3, 1, 4], [0, 2, 0, 0, 5, 1, 0], [128, 129, 1],
                                    (2, 2), np.array([4, 0, 3], dtype=np.int32),
                                    torch.tensor([1, 0, 7])])
def test_record_ranges_against_a_loop(counts):
    lo, hi = distance.record_ranges(counts)
    want_lo, want_hi, first = [], [], 0
    for count in [int(c) for c in counts]:
        for _ in range(count):
            want_lo.append(first)
            want_hi.append(first + count)
        first += count
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32
    assert lo.device.type == "cpu" and lo.shape == hi.shape == (first,)
    assert lo.tolist() == want_lo and hi.tolist() == want_hi
    assert "record_ranges" in distance.__all__


@pytest.mark.parametrize("counts", [[3, -1], [2.5, 1], [1.0, 2.0], ["3"], [[1, 2]], [True, False],
                                    [2 ** 31]])
def test_record_ranges_refuses_bad_counts(counts):
    with pytest.raises(ValueError, match="record counts"):
        distance.record_ranges(counts)


# ---- distance.topk / nearest: errors before a device is touched --------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def _i32(*values):
    return torch.tensor(values, dtype=torch.int32)


def test_topk_and_nearest_refuse_bad_ranges_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(distance.native, "library", no_library)
    good = _rows_f16(4)
    lo, hi = _i32(0, 0, 2, 2), _i32(2, 2, 4, 4)

    def each(**arguments):
        yield lambda: distance.topk(good, k=2, **arguments)
        yield lambda: distance.nearest(good, **arguments)

    conflicts = [dict(exclude_ranges=(lo, hi), exclude_records=[2, 2]),
                 dict(exclude_ranges=(lo, hi), exclude_self=True),
                 dict(exclude_ranges=(lo, hi), exclude_offset=0),
                 dict(exclude_records=[2, 2], exclude_self=True),
                 dict(exclude_records=[2, 2], exclude_offset=1)]
    for arguments in conflicts:
        for call in each(**arguments):
            with pytest.raises(ValueError, match="exclude each other"):
                call()
    for arguments in (dict(exclude_ranges=(lo[:2], hi[:2])), dict(exclude_records=[1, 1])):
        with pytest.raises(ValueError, match="exclude each other"):
            distance.topk(good, good[1:3], k=2, window_first=1, **arguments)
        with pytest.raises(ValueError, match="exclude each other"):
            distance.nearest(good, good[1:3], window_first=1, **arguments)
    shapes = [(lo[:3], hi[:3]), (lo, hi[:3]), (lo.view(2, 2), hi.view(2, 2)), (lo, hi, lo), (lo,),
              lo, 5, (lo.long(), hi.long()), (lo.float(), hi.float()), (lo.numpy().astype(np.int64),
                                                                        hi.numpy()),
              ([0, 0, 2, 2], [2, 2, 4, 4]), (None, hi)]
    for pair in shapes:
        for call in each(exclude_ranges=pair):
            with pytest.raises(ValueError, match="exclude_ranges"):
                call()
    for counts in ([2, 1], [2, 3], []):             # do not sum to the 4 rows
        for call in each(exclude_records=counts):
            with pytest.raises(ValueError, match="exclude_records sums"):
                call()
    for counts in ([2, -2, 4], [2.0, 2.0], [[2, 2]]):
        for call in each(exclude_records=counts):
            with pytest.raises(ValueError, match="record counts"):
                call()
    with pytest.raises(ValueError, match="self-search"):          # b with other rows than a
        distance.topk(good, _rows_f16(5), k=2, exclude_records=[2, 2])
    with pytest.raises(ValueError, match="self-search"):
        distance.nearest(good, _rows_f16(3), exclude_records=[2, 2])
    # the checks that were there come first and stay
    with pytest.raises(ValueError, match="k must be"):
        distance.topk(good, k=17, exclude_ranges=(lo, hi))
    with pytest.raises(ValueError, match="float16"):
        distance.topk(good.float(), k=2, exclude_ranges=(lo, hi))
    with pytest.raises(ValueError, match="metric"):
        distance.topk(good, k=2, metric="dot", exclude_records=[4])
    # nearest: served by the top-k kernel, which has its own workspace type
    for arguments in (dict(exclude_ranges=(lo, hi)), dict(exclude_records=[2, 2])):
        with pytest.raises(ValueError, match="NearestWorkspace"):
            distance.nearest(good, workspace=distance.NearestWorkspace(), **arguments)
    # numpy bounds and bounds with b != a pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        for arguments in (dict(exclude_ranges=(lo.numpy(), hi.numpy())),
                          dict(exclude_records=np.array([1, 3]))):
            with pytest.raises((RuntimeError, AssertionError)):
                distance.topk(good, k=2, **arguments)


def test_cross_shard_topk_refuses_bad_record_counts():
    block = _rows_f16(6)
    for counts, text in (([2, 3], "record_counts sums"), ([7], "record_counts sums"),
                         ([3, -3, 6], "record counts"), ([3.0, 3.0], "record counts")):
        with pytest.raises(ValueError, match=text):
            parallel.cross_shard_topk(block, 2, record_counts=counts, search=_oracle_topk)


# ---- registers ----------------------------------------------------------------------------------

#: VGPRs of the instantiations that were there before the range mode, <depth, folded>: they
#: must not move (hipcc of ROCm as cross-compiled for gfx950 on the commit before this file)
VGPRS_BEFORE = {(4, True): 149, (4, False): 160, (8, True): 181, (8, False): 190,
                (16, True): 245, (16, False): 245}


def _resources(source: str, tmp_path: Path) -> dict:
    """{(depth, folded, ranges): (vgprs, spilled, scratch)} of the k_pairwise_topk
    instantiations of one translation unit, from hipcc's kernel metadata."""
    stem = source.removesuffix(".hip")
    work = tmp_path / stem
    work.mkdir()
    env = dict(os.environ, TMPDIR=str(work), GFY_SOURCE=source, GFY_ASM_OUT=str(work / (stem + ".s")))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    found = {}
    for line in done.stdout.splitlines():
        name = re.search(r"k_pairwise_topkILi(\d+)ELb([01])ELb([01])E", line)
        if name:
            fields = line.split()
            found[(int(name.group(1)), name.group(2) == "1", name.group(3) == "1")] = tuple(
                int(fields[fields.index(word) + 1]) for word in ("vgpr", "spilled", "scratch"))
    return found


def test_every_sweep_instantiation_keeps_its_register_and_scratch_budget(tmp_path):
    """pairwise_topk.hip holds the six instantiations it held, at the VGPR counts they had;
    pairwise_topk_ranges.hip holds the six range ones; all twelve at most 256 VGPRs (two waves
    per SIMD is what one 512-thread workgroup per CU needs), nothing spilled, no scratch."""
    with ThreadPoolExecutor(max_workers=2) as pool:
        plain, ranged = pool.map(lambda source: _resources(source, tmp_path),
                                 ("pairwise_topk.hip", "pairwise_topk_ranges.hip"))
    assert set(plain) == {(d, f, False) for d in (4, 8, 16) for f in (True, False)}, plain
    assert set(ranged) == {(d, f, True) for d in (4, 8, 16) for f in (True, False)}, ranged
    for key, (vgprs, spilled, scratch) in {**plain, **ranged}.items():
        assert vgprs <= 256 and spilled == 0 and scratch == 0, (key, vgprs, spilled, scratch)
    assert {key[:2]: value[0] for key, value in plain.items()} == VGPRS_BEFORE


# ---- cross_shard_topk(record_counts=...) over gloo ----------------------------------------------

def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(rank: int, count: int) -> torch.Tensor:
    rng = np.random.default_rng(500 + rank)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


def _counts(rank: int, rows: int) -> list[int]:
    """Records of 1, 3, 0, 2, 5, 0, 4 rows in turn (starting at another place per rank) until
    ``rows`` rows are used up, the last one cut short."""
    sizes, out, at = (1, 3, 0, 2, 5, 0, 4), [], rank
    while sum(out) < rows:
        out.append(min(sizes[at % len(sizes)], rows - sum(out)))
        at += 1
    return out + [0]


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


def _matrix(a: np.ndarray, b: np.ndarray, metric: str) -> np.ndarray:
    from oracle import gine_numpy as G
    full = G.pairwise_l2(a, b) if metric == "l2" else G.pairwise_cosine(a, b)
    return full.astype(np.float32)


def _oracle_topk(a, b, *, k, metric="l2", window_first=None, exclude_ranges=None):
    """The semantics of distance.topk on CPU tensors with the float64 definition rounded to
    float32, honouring ``window_first`` and ``exclude_ranges``: the stand-in for the kernel."""
    full = _matrix(a.numpy(), b.numpy(), metric)
    n, m = full.shape
    nothing = np.inf if metric == "l2" else -np.inf
    assert window_first is None or exclude_ranges is None
    if window_first is not None:            # b = rows [window_first, ...) of a: skip (first + j, j)
        for j in range(m):
            full[window_first + j, j] = nothing
    if exclude_ranges is not None:
        lo, hi = (bound.numpy().astype(np.int64) for bound in exclude_ranges)
        assert lo.shape == hi.shape == (n,) and exclude_ranges[0].dtype == torch.int32
        columns = np.arange(m)[None, :]
        full[(columns >= lo[:, None]) & (columns < hi[:, None])] = nothing
    values, order = _ranked(full, k, metric)
    return torch.from_numpy(values), torch.from_numpy(order.astype(np.int32))


def _want(sizes, metric, k):
    """The single-process answer over the concatenated rows: every row's whole record is no
    candidate."""
    everything = np.concatenate([_rows(r, sizes[r]).numpy() for r in range(len(sizes))])
    counts = [c for r in range(len(sizes)) for c in _counts(r, sizes[r])]
    full = _matrix(everything, everything, metric)
    first = 0
    for count in counts:
        full[first:first + count, first:first + count] = np.inf if metric == "l2" else -np.inf
        first += count
    assert first == everything.shape[0]
    return _ranked(full, k, metric)


def _worker(rank: int, size: int, port: int, sizes: list[int], metric: str, k: int,
            chunk_rows: int, queue) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        values, indices, offsets = parallel.cross_shard_topk(
            _rows(rank, sizes[rank]), k, metric=metric, chunk_rows=chunk_rows,
            search=_oracle_topk, record_counts=_counts(rank, sizes[rank]))
        queue.put((rank, values.numpy(), indices.numpy(), offsets))
    except BaseException as error:       # the parent must not wait out its timeout for a dead rank
        queue.put((rank, repr(error), None, None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("sizes,chunk_rows,k", [([7, 7], 3, 4), ([5, 11], 4, 8), ([0, 6], 4, 3),
                                                ([9, 0, 4], 5, 16), ([13, 8, 5], 100, 5)])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_cross_shard_topk_with_records_chunked_gloo(sizes, chunk_rows, k, metric):
    """Two and three ranks, unequal and empty blocks, chunks that cut records: every rank's rows
    get the k best rows of the world OUTSIDE their own record, by (value, global row)."""
    size = len(sizes)
    context = mp.get_context("spawn")      # fresh children, as tests/test_parallel_cpu.py starts them
    queue = context.Queue()
    port = _free_port()
    procs = [context.Process(target=_worker,
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
    want_values, want = _want(sizes, metric, k)
    starts = np.concatenate(([0], np.cumsum(sizes)))
    for rank, values, indices, offsets in results:
        assert offsets == list(starts)
        lo, hi = starts[rank], starts[rank + 1]
        assert indices.shape == (hi - lo, k) and indices.dtype == np.int64
        np.testing.assert_array_equal(indices, want[lo:hi])
        np.testing.assert_array_equal(values, want_values[lo:hi])


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_cross_shard_topk_with_records_world_size_one(metric):
    sizes = [23]
    block, counts = _rows(0, 23), _counts(0, 23)
    assert 0 in counts and max(counts) == 5
    want_values, want = _want(sizes, metric, 6)
    for chunk_rows in (4, 7, 23, 1 << 20):
        values, indices, offsets = parallel.cross_shard_topk(
            block, 6, metric=metric, chunk_rows=chunk_rows, search=_oracle_topk,
            record_counts=counts)
        assert offsets == [0, 23]
        np.testing.assert_array_equal(indices.numpy(), want)
        np.testing.assert_array_equal(values.numpy(), want_values)
    # without record_counts the call is what it was: only the row itself is skipped
    values, indices, _ = parallel.cross_shard_topk(block, 6, metric=metric, chunk_rows=7,
                                                   search=_oracle_topk)
    full = _matrix(block.numpy(), block.numpy(), metric)
    np.fill_diagonal(full, np.inf if metric == "l2" else -np.inf)
    np.testing.assert_array_equal(indices.numpy(), _ranked(full, 6, metric)[1])
    empty = torch.zeros((0, 128), dtype=torch.float16)
    values, indices, offsets = parallel.cross_shard_topk(empty, 5, search=_oracle_topk,
                                                         record_counts=[])
    assert values.shape == (0, 5) and indices.shape == (0, 5) and offsets == [0, 0]
