"""Top-k search with at most one hit per record (gfy_pairwise_topk_distinct,
distance.topk(distinct_records=...), distance.record_of): what needs no GPU.  The C ABI and
``topk`` refuse bad arguments before a device is touched, ``record_of`` is compared with a loop,
and the distinct sweep kernels fit the register file as hipcc allocates them."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from ginfinity_amd import _native as native
from ginfinity_amd import distance

ROOT = Path(__file__).resolve().parents[1]
KMAX = native.GFY_PAIRWISE_TOPK_DISTINCT_MAX


# ---- C ABI --------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_without_a_device():
    lib = native.library()
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    need = lib.gfy_pairwise_topk_workspace_bytes(300, 500, 8)

    def call(a=p, n=300, b=p, m=500, metric=native.GFY_L2, k=8, lo=p, hi=p, glo=p, ghi=p, val=p,
             idx=p, ws=p, size=need):
        return lib.gfy_pairwise_topk_distinct(a, n, b, m, metric, k, lo, hi, glo, ghi, val, idx,
                                              ws, size, None)

    for hole in ("lo", "hi"):
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
        assert b"skip_lo or skip_hi" in lib.gfy_last_error()
    for hole in ("glo", "ghi"):
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
        assert b"group_lo or group_hi" in lib.gfy_last_error()
    for hole in ("a", "b", "val", "idx", "ws"):
        assert call(**{hole: None}) == native.GFY_ERR_INVALID, hole
    assert KMAX in (8, 16)
    for k in (0, KMAX + 1, -1, 1 << 20):
        assert call(k=k) == native.GFY_ERR_INVALID, k
        assert b"k = " in lib.gfy_last_error()
        assert b"1..%d" % KMAX in lib.gfy_last_error()
    for n, m in ((0, 5), (5, 0), (-1, 5), (5, 1 << 31)):
        assert call(n=n, m=m, size=1 << 40) == native.GFY_ERR_INVALID, (n, m)
    assert call(metric=7) == native.GFY_ERR_INVALID
    for short in (0, 1, need - 1):      # the workspace is that of gfy_pairwise_topk
        assert call(size=short) == native.GFY_ERR_WORKSPACE, short
    assert native.ABI_VERSION == 4 == lib.gfy_abi_version()


# ---- record_of ----------------------------------------------------------------------------------

@pytest.mark.parametrize("counts", [[1], [3, 1, 4], [0, 2, 0, 0, 5, 1, 0], [128, 129, 1], (2, 2),
                                    np.array([4, 0, 3], dtype=np.int32), torch.tensor([1, 0, 7])])
def test_record_of_against_a_loop(counts):
    owner = [q for q, count in enumerate(int(c) for c in counts) for _ in range(count)]
    rows = len(owner)
    rng = np.random.default_rng(rows)
    indices = rng.integers(-1, rows, size=(9, 5)).astype(np.int32)
    indices[0, :] = -1
    indices[1, 0], indices[1, 1] = 0, rows - 1
    want = [[-1 if j < 0 else owner[j] for j in row] for row in indices.tolist()]
    for given in (indices, torch.from_numpy(indices), torch.from_numpy(indices).long(),
                  indices[:, 0]):
        found = distance.record_of(given, counts)
        assert isinstance(found, torch.Tensor) and found.dtype == torch.int32
        assert found.device.type == "cpu" and tuple(found.shape) == tuple(given.shape)
        assert found.tolist() == (want if found.dim() == 2 else [row[0] for row in want])
    assert distance.record_of(np.zeros((0, 3), dtype=np.int32), counts).shape == (0, 3)
    assert "record_of" in distance.__all__


@pytest.mark.parametrize("counts", [[3, -1], [2.5, 1], [1.0, 2.0], ["3"], [[1, 2]], [True, False]])
def test_record_of_refuses_bad_counts(counts):
    with pytest.raises(ValueError, match="record counts"):
        distance.record_of(np.array([0, 1], dtype=np.int32), counts)


# ---- distance.topk: errors before a device is touched -------------------------------------------

def _rows_f16(count):
    return torch.zeros((count, 128), dtype=torch.float16)


def test_topk_refuses_bad_distinct_records_without_a_device(monkeypatch):
    """On a machine without a GPU a touched device is a RuntimeError, and the library is never
    asked for: both would show instead of the ValueError."""
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(distance.native, "library", no_library)
    good = _rows_f16(4)
    others = [dict(), dict(exclude_self=True), dict(exclude_offset=1), dict(exclude_records=[2, 2]),
              dict(exclude_ranges=(torch.zeros(4, dtype=torch.int32),) * 2)]
    for arguments in others:
        for counts in ([2, 1], [2, 3], []):             # do not sum to the 4 rows of b
            with pytest.raises(ValueError, match=r"distinct_records sums to \d+ rows, b has 4"):
                distance.topk(good, k=2, distinct_records=counts, **arguments)
        for counts in ([2, -2, 4], [2.0, 2.0], [[2, 2]]):
            with pytest.raises(ValueError, match="record counts"):
                distance.topk(good, k=2, distinct_records=counts, **arguments)
    with pytest.raises(ValueError, match="distinct_records sums to 4 rows, b has 5"):
        distance.topk(good, _rows_f16(5), k=2, distinct_records=[2, 2])
    with pytest.raises(ValueError, match="distinct_records sums"):
        distance.topk(good, good[1:3], k=2, window_first=1, distinct_records=[2, 2])
    with pytest.raises(TypeError, match="distinct_records"):
        distance.nearest(good, distinct_records=[4])
    # the checks that were there come first and stay
    with pytest.raises(ValueError, match="k must be"):
        distance.topk(good, k=17, distinct_records=[3])
    if KMAX < native.GFY_PAIRWISE_TOPK_MAX:
        with pytest.raises(ValueError, match=f"1..{KMAX} with distinct_records"):
            distance.topk(good, k=KMAX + 1, distinct_records=[4])
    with pytest.raises(ValueError, match="float16"):
        distance.topk(good.float(), k=2, distinct_records=[3])
    with pytest.raises(ValueError, match="metric"):
        distance.topk(good, k=2, metric="dot", distinct_records=[3])
    with pytest.raises(ValueError, match="exclude each other"):
        distance.topk(good, k=2, exclude_records=[4], exclude_self=True, distinct_records=[4])
    # good counts pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            distance.topk(good, k=2, distinct_records=np.array([1, 3]))


# ---- registers ----------------------------------------------------------------------------------

def test_every_distinct_sweep_fits_the_register_file(tmp_path):
    """pairwise_topk_distinct.hip holds the sweep at depth 4, 8 and 16 (up to KMAX), folded and
    not, each at most 256 VGPRs (two waves per SIMD is what one 512-thread workgroup per CU
    needs), nothing spilled, no scratch; its finish kernel likewise."""
    env = dict(os.environ, TMPDIR=str(tmp_path), GFY_SOURCE="pairwise_topk_distinct.hip",
               GFY_ASM_OUT=str(tmp_path / "pairwise_topk_distinct.s"))
    done = subprocess.run(["bash", str(ROOT / "tools" / "pairwise_resources.sh")],
                          capture_output=True, text=True, timeout=900, env=env)
    assert done.returncode == 0, done.stderr[-2000:]
    print(done.stdout)
    found, finish = {}, None
    for line in done.stdout.splitlines():
        fields = line.split()
        budget = tuple(int(fields[fields.index(word) + 1]) for word in ("vgpr", "spilled", "scratch"))
        name = re.search(r"k_pairwise_topkILi(\d+)ELb([01])ELb([01])ELb([01])E", line)
        if name:
            found[(int(name.group(1)), *(name.group(g) == "1" for g in (2, 3, 4)))] = budget
        elif "k_topk_finish_distinct" in line:
            finish = budget
        else:
            raise AssertionError(f"a kernel nobody expected: {line}")
    depths = [d for d in (4, 8, 16) if d <= KMAX]
    assert set(found) == {(d, f, True, True) for d in depths for f in (True, False)}, found
    for key, (vgprs, spilled, scratch) in {**found, "finish": finish}.items():
        assert vgprs <= 256 and spilled == 0 and scratch == 0, (key, vgprs, spilled, scratch)
