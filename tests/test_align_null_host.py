"""Null scores and significance of local alignment (align.shuffle_orders, align.null_scores,
align.significance; gfy_align_local_null): what needs no GPU.  The orders against the numpy twin
of tests/align_null_oracle.py byte for byte, the formulas of ``significance`` against numpy
float64 on hand-made rows, every ``ValueError`` before a device is touched, the no-device errors
of the C entry, the declaration of the symbol, and the resources of the cross-compiled kernel."""
from __future__ import annotations

import ctypes
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import align_null_oracle as NO
from ginfinity_amd import _native as native
from ginfinity_amd import align, build

ROOT = Path(__file__).resolve().parents[1]


# ---- shuffle_orders ---------------------------------------------------------------------------------
CASES = (([5, 0, 7, 1], 3, 0), ([33, 70, 1, 31], 4, 2 ** 63 + 12345), ([200], 25, 7),
         ([0, 0], 2, 5), ([], 2, 1), ([64, 32, 4096], 2, 2 ** 64 - 1))


@pytest.mark.parametrize("columns, shuffles, seed", CASES)
def test_orders_equal_the_numpy_twin_and_every_segment_is_a_permutation(columns, shuffles, seed):
    order, order_ptr = align.shuffle_orders(columns, shuffles, seed)
    twin, twin_ptr = NO.shuffle_orders(columns, shuffles, seed)
    assert order.dtype == torch.int32 and order_ptr.dtype == torch.int64
    assert not order.is_cuda and not order_ptr.is_cuda
    assert order.numpy().tobytes() == twin.tobytes()
    assert order_ptr.numpy().tobytes() == twin_ptr.tobytes()
    assert order_ptr.tolist() == [0] + (np.cumsum(columns, dtype=np.int64) * shuffles).tolist()
    assert order.shape == (int(order_ptr[-1]),)
    for p, count in enumerate(columns):
        for k in range(shuffles):
            part = NO.segment(order.numpy(), order_ptr.numpy(), columns, shuffles, p, k)
            assert sorted(part.tolist()) == list(range(count)), (p, k)
    # other ways to say the same columns
    for same in (np.array(columns, dtype=np.int32), torch.tensor(columns, dtype=torch.int64)):
        again = align.shuffle_orders(same, np.int64(shuffles), seed - 2 ** 64)
        assert again[0].numpy().tobytes() == twin.tobytes()


def test_orders_depend_on_the_seed_and_on_nothing_behind_them():
    columns, shuffles = [40, 17, 90], 3
    one = align.shuffle_orders(columns, shuffles, 1)[0].numpy()
    two = align.shuffle_orders(columns, shuffles, 2)[0].numpy()
    assert one.tobytes() != two.tobytes()
    ptr = NO.shuffle_orders(columns, shuffles, 1)[1]
    # the runs of one pair differ from each other, and look shuffled
    runs = [NO.segment(one, ptr, columns, shuffles, 2, k) for k in range(shuffles)]
    assert len({run.tobytes() for run in runs}) == shuffles
    assert all(np.count_nonzero(run == np.arange(90)) < 10 for run in runs)
    # the same (seed, v) gives the same segment whatever follows it, and whatever stands in front
    # of it as long as v is the same
    front = align.shuffle_orders(columns[:2] + [5, 1000], shuffles, 1)[0].numpy()
    assert front[:shuffles * 57].tobytes() == one[:shuffles * 57].tobytes()
    other = align.shuffle_orders([3, 99, 90], shuffles, 1)[0].numpy()
    assert other[-shuffles * 90:].tobytes() == one[-shuffles * 90:].tobytes()
    # a segment is the stable sort of the formula's keys
    keys = NO.keys(1, 2 * shuffles + 1, 90)
    assert keys.max() < 2 ** 32 and len(set(keys.tolist())) > 80
    assert runs[1].tolist() == sorted(range(90), key=lambda j: (int(keys[j]), j))


def test_what_shuffle_orders_refuses():
    for columns in ([[1, 2]], [1.0, 2.0], [-1, 3], "12", 5):
        with pytest.raises(ValueError, match="columns must be"):
            align.shuffle_orders(columns, 2, 0)
    for shuffles in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="shuffles must be a positive integer"):
            align.shuffle_orders([3], shuffles, 0)
    for seed in (1.0, None, "7", True):
        with pytest.raises(ValueError, match="seed must be an integer"):
            align.shuffle_orders([3], 2, seed)
    with pytest.raises(ValueError, match="below 2\\^31"):
        align.shuffle_orders(np.zeros(2 ** 16, dtype=np.int64), 2 ** 15, 0)


# ---- significance -----------------------------------------------------------------------------------
GAMMA = 0.5772156649015329


def _by_hand(score, row):
    row = np.asarray(row, dtype=np.float64)
    count = row.size
    mean = row.sum() / count
    std = math.sqrt(((row - mean) ** 2).sum() / (count - 1))
    z = (score - mean) / std
    lam = math.pi / (std * math.sqrt(6.0))
    mu = mean - GAMMA / lam
    return z, mean, std, -math.expm1(-math.exp(-lam * (score - mu))), lam, mu


def test_significance_against_numpy_float64_on_hand_made_rows():
    null = np.array([[1.0, 2.0, 3.0, 4.0], [7.25, 7.5, 6.0, 9.75], [0.0, 0.0, 0.0, 0.5],
                     [10.0, 12.0, 11.0, 30.0]], dtype=np.float32)
    scores = np.array([10.0, 7.0, 0.25, 2.0], dtype=np.float32)
    found = align.significance(torch.from_numpy(scores), torch.from_numpy(null))
    assert isinstance(found, align.Significance)
    assert found._fields == ("z", "mean", "std", "p_value", "lam", "mu")
    for values in found:
        assert values.dtype == torch.float64 and values.shape == (4,) and not values.is_cuda
    for p in range(4):
        want = _by_hand(float(scores[p]), null[p])
        got = [float(values[p]) for values in found]
        assert np.allclose(got, want, rtol=1e-12, atol=0), (p, got, want)
    assert found.p_value[0] < 1e-3 < 0.5 < found.p_value[3] <= 1.0
    assert found.std[0] == math.sqrt(5.0 / 3.0) and found.mean[0] == 2.5
    # numpy arrays and float64 are taken as well
    again = align.significance(scores.astype(np.float64), null.astype(np.float64))
    assert all(torch.equal(x, y) for x, y in zip(found, again))


def test_significance_of_constant_rows_and_of_a_refused_pair():
    nan = float("nan")
    null = torch.tensor([[2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [1.0, nan, 3.0],
                         [1.0, 2.0, 3.0]])
    scores = torch.tensor([3.0, 1.0, 2.0, 2.0, nan])
    found = align.significance(scores, null)          # nothing is raised
    assert found.std[:3].tolist() == [0.0] * 3 and found.mean[:3].tolist() == [2.0] * 3
    assert found.z[0] == math.inf and found.z[1] == -math.inf and math.isnan(found.z[2])
    assert found.lam[:3].tolist() == [math.inf] * 3 and found.mu[:3].tolist() == [2.0] * 3
    assert found.p_value[0] == 0.0 and found.p_value[1] == 1.0 and math.isnan(found.p_value[2])
    assert all(math.isnan(values[3]) for values in found)       # a NaN in the row: the row is NaN
    assert math.isnan(found.z[4]) and math.isnan(found.p_value[4])
    assert found.mean[4] == 2.0 and found.std[4] == 1.0


def test_what_significance_refuses():
    for null in (torch.zeros((3, 1)), np.zeros((3, 0)), torch.zeros(3), torch.zeros((3, 2, 2)),
                 [[1.0, 2.0]], torch.zeros((3, 4), dtype=torch.int32)):
        with pytest.raises(ValueError, match="null must"):
            align.significance(torch.zeros(3), null)
    with pytest.raises(ValueError, match="at least 2 scores per pair, not K = 1"):
        align.significance(torch.zeros(3), torch.zeros((3, 1)))
    for scores in (torch.zeros(2), torch.zeros((3, 1)), [0.0] * 3, torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="scores must"):
            align.significance(scores, torch.zeros((3, 4)))


# ---- null_scores: every error before a device is touched ---------------------------------------------
def _rows_f16(count):
    rng = np.random.default_rng(count)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


BASE = dict(counts_a=[2, 4], pairs=[[0, 1], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5)
COLUMNS = [4, 4, 2]


def test_a_bad_call_is_a_value_error_before_any_device_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(native, "library", no_library)
    good = _rows_f16(6)
    with pytest.raises(ValueError, match="shuffles is required: it has no default"):
        align.null_scores(good, **BASE)
    with pytest.raises(ValueError, match="shuffles is required"):
        align.null_scores(good, shuffles=None, **BASE)
    for shuffles in (0, -3, 2.0, "4", True, np.bool_(True)):
        with pytest.raises(ValueError, match="shuffles must be a positive integer"):
            align.null_scores(good, shuffles=shuffles, **BASE)
    with pytest.raises(ValueError, match=r"P \* shuffles = 3 \* 1000000000 must stay below 2\^31"):
        align.null_scores(good, shuffles=10 ** 9, **BASE)
    for seed in (0.5, None, "1", False):
        with pytest.raises(ValueError, match="seed must be an integer"):
            align.null_scores(good, shuffles=2, seed=seed, **BASE)
    order, order_ptr = align.shuffle_orders(COLUMNS, 2, 0)
    for orders in (order, (order,), (order, order_ptr, order), "ab", 5):
        with pytest.raises(ValueError, match=r"orders must be a pair \(order, order_ptr\)"):
            align.null_scores(good, shuffles=2, orders=orders, **BASE)
    for bad in (order.to(torch.int64), order.to(torch.float32), order[:-1], order.reshape(2, -1),
                torch.cat([order, order]), order.numpy().astype(np.uint32)):
        with pytest.raises(ValueError, match=r"order must be an int32 array of shape .* = \(20,\)"):
            align.null_scores(good, shuffles=2, orders=(bad, order_ptr), **BASE)
    for bad in (order_ptr.to(torch.int32), order_ptr[:-1], order_ptr.reshape(2, 2),
                order_ptr.numpy().astype(np.float64)):
        with pytest.raises(ValueError, match=r"order_ptr must be an int64 array of shape \(P \+ 1,\) "
                                             r"= \(4,\)"):
            align.null_scores(good, shuffles=2, orders=(order, bad), **BASE)
    for bad in ([0, 1], None):
        with pytest.raises(ValueError, match="must be a numpy array or a torch tensor"):
            align.null_scores(good, shuffles=2, orders=(bad, order_ptr), **BASE)
    # the orders of a box are those of its columns: 20 entries fit no box of one column
    with pytest.raises(ValueError, match=r"= \(6,\)"):
        align.null_scores(good, shuffles=2, orders=(order, order_ptr), box=(0, 9, 1, 1), **BASE)
    # the inherited errors, unchanged
    with pytest.raises(ValueError, match="out of range"):
        align.null_scores(good, shuffles=2, **{**BASE, "pairs": [[0, 2]]})
    with pytest.raises(ValueError, match="0 <= gap_extend <= gap_open"):
        align.null_scores(good, shuffles=2, **{**BASE, "gap_extend": 2.0})
    with pytest.raises(ValueError, match="gap_open is required"):
        align.null_scores(good, shuffles=2, **{**BASE, "gap_open": None})
    with pytest.raises(ValueError, match="lo <= hi"):
        align.null_scores(good, shuffles=2, band=(1, 0), **BASE)
    with pytest.raises(ValueError, match="i_lo <= i_hi and j_lo"):
        align.null_scores(good, shuffles=2, box=(3, 2, 0, 0), **BASE)
    with pytest.raises(ValueError, match="counts_b is required"):
        align.null_scores(good, good, shuffles=2, **BASE)


def test_good_arguments_pass_the_checks_and_only_then_ask_for_a_device():
    if torch.cuda.is_available():
        pytest.skip("what follows the checks is the GPU tests' business")
    order, order_ptr = align.shuffle_orders(COLUMNS, 2, 0)
    for more in (dict(), dict(orders=(order, order_ptr)), dict(orders=[order.numpy(), order_ptr.numpy()]),
                 dict(band=(-1, 1), box=(0, 9, 0, 9), seed=2 ** 70)):
        with pytest.raises((RuntimeError, AssertionError)):
            align.null_scores(_rows_f16(6), shuffles=2, **more, **BASE)


# ---- the C entry ------------------------------------------------------------------------------------
def test_c_abi_declares_the_symbol_and_names_what_it_refuses():
    lib = native.library()
    void, size, i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64
    call = [void, i64] * 5 + [ctypes.c_float] * 4
    result, declared = native.SIGNATURES["gfy_align_local_null"]
    assert result is ctypes.c_int
    assert list(declared) == call + [void, void, i64, void, void, void, void, size, void]
    # gfy_align_local_box's list with shuffles, order and order_ptr behind boxes, and no out_end
    box = list(native.SIGNATURES["gfy_align_local_box"][1])
    assert list(declared) == box[:16] + [i64, void, void] + box[16:17] + box[18:]
    assert lib.gfy_align_local_null is not None
    header = (ROOT / "include" / "gfy.h").read_text()
    assert "gfy_align_local_null(" in header and "#define GFY_ABI_VERSION 4" in header
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    assert "no normalisation" not in header
    for word in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15"):
        assert word in header and word in align.__doc__, word
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    who = b"gfy_align_local_null"

    def null_call(a=p, ptr_b=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, boxes=p, shuffles=8,
                  order=p, order_ptr=p, score=p, ws=p, size=None):
        if size is None:
            size = lib.gfy_align_workspace_bytes(10 * 8, 0)
        return lib.gfy_align_local_null(a, 300, p, 3, p, 500, ptr_b, 7, pairs, P, 1.0, 0.0, go, ge,
                                        bands, boxes, shuffles, order, order_ptr, score, ws, size,
                                        None)

    def refusal(code, text, **changes):
        assert null_call(**changes) == code, changes
        message = lib.gfy_last_error()
        assert message.startswith(who + b": ") and text in message, (changes, message)

    for hole, text in {"a": b"a is NULL", "ptr_b": b"ptr_b is NULL", "pairs": b"pairs is NULL",
                       "order": b"order is NULL", "order_ptr": b"order_ptr is NULL",
                       "score": b"out_score is NULL", "ws": b"workspace is NULL"}.items():
        refusal(native.GFY_ERR_INVALID, text, **{hole: None})
        refusal(native.GFY_ERR_INVALID, text, bands=None, boxes=None, **{hole: None})
    for shuffles in (0, -1, -2 ** 40):
        refusal(native.GFY_ERR_INVALID, b"shuffles = ", shuffles=shuffles)
    refusal(native.GFY_ERR_INVALID, b"P = ", P=0)
    refusal(native.GFY_ERR_INVALID, b"P * shuffles", P=2 ** 16, shuffles=2 ** 15)
    refusal(native.GFY_ERR_INVALID, b"P * shuffles", P=3, shuffles=2 ** 62)
    refusal(native.GFY_ERR_INVALID, b"gap_extend", go=1.0, ge=1.5)
    # NULL bands and NULL boxes are no refusal: the next check speaks
    for short in (0, 1, lib.gfy_align_workspace_bytes(10 * 8, 0) - 1):
        refusal(native.GFY_ERR_WORKSPACE, b"workspace", size=short, bands=None, boxes=None)
        refusal(native.GFY_ERR_WORKSPACE, b"workspace", size=short)
    # P * shuffles = 2^31 - 1 passes that check (and the workspace is then too short)
    refusal(native.GFY_ERR_WORKSPACE, b"workspace", P=2 ** 31 - 1, shuffles=1, size=8)


# ---- the kernel's resources -------------------------------------------------------------------------
def _resources(source: str) -> dict:
    """{kernel: {field: value}} of the remarks of -Rpass-analysis=kernel-resource-usage."""
    hipcc = build._hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: nothing to cross-compile with")
    done = subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-c", str(build.CSRC / source),
                           "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    kernels, current = {}, None
    for line in done.stderr.splitlines():
        found = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not found:
            continue
        if found.group(1):
            current = kernels.setdefault(found.group(1), {})
        elif current is not None:
            current[found.group(2).strip()] = int(found.group(3))
    return kernels


def test_the_null_kernel_does_not_spill_and_keeps_the_box_kernels_occupancy():
    kernels = _resources("align_kernels.hip")
    null = {name: values for name, values in kernels.items() if "k_align_local_null" in name}
    box = {name: values for name, values in kernels.items() if "k_align_local_box" in name}
    assert len(null) == 1 and len(box) == 1
    (null,), (box,) = null.values(), box.values()
    assert null["SGPRs Spill"] == 0 and null["VGPRs Spill"] == 0 and null["ScratchSize"] == 0
    assert null["Occupancy"] >= box["Occupancy"] >= 1
