"""Local alignment inside a band of diagonals (the ``band`` of align.local_align, local_spans and
local_paths, align.band_around; gfy_align_local_band, gfy_align_local_span_band,
gfy_align_trace_band): what needs no GPU.  The oracle of tests/align_band_oracle.py under a
covering band against the span and path oracles, the claims of include/gfy.h about a band
(widening never lowers a score, the box property under the shifted band, re-scoring) on random
float32 matrices, ``band_around`` and every ``ValueError`` of the band before a device is
touched, and the three symbols of the C ABI."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import align_band_oracle as BO
import align_path_oracle as PO
import align_span_oracle as SO
from ginfinity_amd import _native as native
from ginfinity_amd import align

SHAPES = ((1, 1), (1, 9), (9, 1), (7, 5), (64, 65), (70, 40))
#: (gap_open, gap_extend)
GAPS = ((1.0, 0.25), (0.5, 0.5), (0.75, 0.0))


def _bits(value) -> bytes:
    return np.float32(value).tobytes()


def _matrix(rng, lq, lr):
    """Scores in the range of a shifted cosine, with a diagonal stretch that aligns and a few
    values repeated so that ties occur."""
    S = rng.uniform(-0.9, 0.4, size=(lq, lr)).astype(np.float32)
    shift = int(rng.integers(-(lq - 1), lr))
    for i in range(lq):
        if 0 <= i + shift < lr and rng.random() < 0.8:
            S[i, i + shift] = np.float32(rng.choice([0.5, 0.625, 0.75]))
    return S


def _cases():
    rng = np.random.default_rng(20261019)
    for number, (lq, lr) in enumerate(SHAPES):
        for repeat in range(3):
            yield _matrix(rng, lq, lr), GAPS[(number + repeat) % len(GAPS)]


def _bands(rng, lq, lr, count):
    """Random bands that meet the matrix, and their (lo, hi)."""
    for _ in range(count):
        lo = int(rng.integers(-(lq - 1) - 2, lr + 1))
        yield lo, lo + int(rng.integers(0, max(lq, lr)))


def test_a_covering_band_equals_the_span_and_path_oracles():
    for S, (go, ge) in _cases():
        lq, lr = S.shape
        for lo, hi in (BO.covering(lq, lr), (-(lq - 1) - 3, lr + 4), (-4096, 4096)):
            score, start, end = BO.band_span_of(S, go, ge, lo, hi)
            want = SO.span_of(S, go, ge)
            assert (_bits(score), start, end) == (_bits(want[0]), want[1], want[2]), (S.shape, lo)
            score, start, end, ops = BO.band_path_of(S, go, ge, lo, hi)
            want = PO.path_of(S, go, ge)
            assert (_bits(score), start, end) == (_bits(want[0]), want[1], want[2])
            assert ops.tobytes() == want[3].tobytes()
            assert BO.band_box_path(S, go, ge, lo, hi)[1].tobytes() == \
                PO.box_path(S, go, ge).tobytes()


def test_widening_a_band_never_lowers_the_score():
    rng = np.random.default_rng(5)
    for S, (go, ge) in _cases():
        lq, lr = S.shape
        for lo, hi in _bands(rng, lq, lr, 4):
            before = BO.band_span_of(S, go, ge, lo, hi)[0]
            for more_lo, more_hi in ((1, 0), (0, 1), (3, 5), (lq + lr, lq + lr)):
                lo, hi = lo - more_lo, hi + more_hi                 # nested: wider every time
                after = BO.band_span_of(S, go, ge, lo, hi)[0]
                assert after >= before, (S.shape, lo, hi)
                before = after
            assert _bits(before) == _bits(SO.span_of(S, go, ge)[0])    # the last one covers


def test_a_band_that_meets_no_cell_and_a_single_diagonal():
    S = np.full((5, 7), 0.5, dtype=np.float32)
    for lo, hi in ((7, 9), (-9, -5), (4096, 4096), (-4096, -4000)):
        score, start, end, ops = BO.band_path_of(S, 1.0, 0.5, lo, hi)
        assert _bits(score) == _bits(0) and start == end == (-1, -1) and ops.size == 0
    for S, (go, ge) in _cases():
        lq, lr = S.shape
        for d in {-(lq - 1), 0, lr - 1, (lr - lq) // 2}:
            score, start, end, ops = BO.band_path_of(S, go, ge, d, d)
            assert not ops.any()                                    # gapless: matches alone
            if end != (-1, -1):
                assert end[1] - end[0] == d == start[1] - start[0]
                assert ops.size == end[0] - start[0] + 1


def test_the_box_property_holds_under_the_shifted_band_and_the_ops_add_up_to_the_score():
    rng = np.random.default_rng(6)
    checked = 0
    for S, (go, ge) in _cases():
        lq, lr = S.shape
        for lo, hi in _bands(rng, lq, lr, 4):
            score, start, end, ops = BO.band_path_of(S, go, ge, lo, hi)
            if end == (-1, -1):
                continue
            shift = start[1] - start[0]
            assert lo <= shift <= hi and lo <= end[1] - end[0] <= hi
            box = S[start[0]:end[0] + 1, start[1]:end[1] + 1]
            corner, box_ops = BO.band_box_path(box, go, ge, lo - shift, hi - shift)
            assert _bits(corner) == _bits(score), (S.shape, lo, hi)
            assert box_ops.tobytes() == ops.tobytes()
            assert _bits(PO.rescore(S, ops, start, go, ge)) == _bits(score)
            assert ops[0] == 0 and ops[-1] == 0
            assert np.count_nonzero(ops != 1) == end[0] - start[0] + 1
            assert np.count_nonzero(ops != 2) == end[1] - start[1] + 1
            cells = align.path_cells(ops, np.array(start))          # the path stays in the band
            both = cells[(cells >= 0).all(axis=1)]
            assert ((both[:, 1] - both[:, 0] >= lo) & (both[:, 1] - both[:, 0] <= hi)).all()
            checked += 1
    assert checked >= 40, checked


def test_band_around():
    bands = align.band_around([[3, 10], [10, 3], [0, 0], [4095, 0]], 5)
    assert bands.dtype == np.int32 and bands.tolist() == [[2, 12], [-12, -2], [-5, 5], [-4100, -4090]]
    assert align.band_around(torch.tensor([[7, 9]]), 0).tolist() == [[2, 2]]
    assert align.band_around(np.array([[7, 9]], dtype=np.uint16), np.int64(1)).tolist() == [[1, 3]]
    assert align.band_around([[0, 4095]], 10 ** 12).tolist() == [[4095 - 8192, 4095 + 8192]]
    assert align.band_around([], 3).shape == (0, 2)
    assert align.band_around(np.zeros((0, 2), dtype=np.int64), 3).dtype == np.int32
    for half_width in (-1, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="half_width must be a non-negative integer"):
            align.band_around([[1, 2]], half_width)
    for seeds in ([1, 2], [[1.0, 2.0]], [[1, 2, 3]], [[[1, 2]]], "12"):
        with pytest.raises(ValueError, match=r"shape \(P, 2\)"):
            align.band_around(seeds, 1)
    for seeds in ([[-1, 2]], [[0, 4096]]):
        with pytest.raises(ValueError, match="inside records"):
            align.band_around(seeds, 1)


def _rows_f16(count):
    rng = np.random.default_rng(count)
    return torch.from_numpy(rng.standard_normal((count, 128)).astype(np.float16))


@pytest.mark.parametrize("name", ("local_align", "local_spans", "local_paths"))
def test_a_bad_band_is_a_value_error_before_any_device_is_touched(name):
    function = getattr(align, name)
    good = _rows_f16(6)
    base = dict(counts_a=[2, 4], pairs=[[0, 1], [1, 1], [1, 0]], gap_open=1.0, gap_extend=0.5)
    for band in ([[0.0, 1.0]] * 3, np.zeros((3, 2)), torch.zeros((3, 2)), (0.0, 1.0), "01",
                 (True, False), [[None, 1]] * 3):
        with pytest.raises(ValueError, match="band must"):
            function(good, band=band, **base)
    for band in ([[0, 1]] * 2, [[0, 1]] * 4, [[0, 1, 2]] * 3, [0, 1, 2], 5, [[[0, 1]]] * 3,
                 np.zeros((3, 2, 1), dtype=np.int32), []):
        with pytest.raises(ValueError, match=r"shape \(P, 2\)"):
            function(good, band=band, **base)
    with pytest.raises(ValueError, match=r"band of pair 1 = \(3, 2\): lo <= hi"):
        function(good, band=[[0, 1], [3, 2], [9, 1]], **base)
    with pytest.raises(ValueError, match=r"band of pair 0 = \(1, 0\): lo <= hi"):
        function(good, band=(1, 0), **base)
    with pytest.raises(ValueError, match=r"band of pair 2 = \(5000, 4999\)"):    # before clipping
        function(good, band=torch.tensor([[0, 0], [-1, 1], [5000, 4999]]), **base)
    # the other checks come first and are unchanged by a band
    with pytest.raises(ValueError, match="out of range"):
        function(good, band=(0, 1), **{**base, "pairs": [[0, 2]]})


def test_none_and_a_band_pass_the_checks_with_no_device_touched():
    good = _rows_f16(6)
    arguments = (good, None, [2, 4], None, [[0, 1], [1, 1], [1, 0]], 1.0, 0.5, 1.0, 0.0)
    call = align._checked_call(*arguments)
    assert call.band is None and call.band_dev is None and not call.a.is_cuda
    assert align._checked_call(*arguments, None).band is None
    wanted = [[-3, 4], [-4096, 4096], [0, 0]]
    for band in ([[-3, 4], [-10 ** 9, 2 ** 40], [0, 0]],
                 np.array([[-3, 4], [-5000, 5000], [0, 0]], dtype=np.int16),
                 torch.tensor([[-3, 4], [-4097, 4097], [0, 0]], dtype=torch.int64)):
        call = align._checked_call(*arguments, band)
        assert call.band.dtype == np.int32 and call.band.flags.c_contiguous
        assert call.band.tolist() == wanted and call.band_dev is None
    for one in ((-7, 7), [-7, 7], np.array([-7, 7]), torch.tensor([-7, 7])):
        assert align._checked_call(*arguments, one).band.tolist() == [[-7, 7]] * 3
    assert align._checked_call(*arguments[:4], [], *arguments[5:], (0, 1)).band.shape == (0, 2)
    assert align._checked_call(*arguments[:4], [], *arguments[5:], []).band.shape == (0, 2)
    # good arguments pass the checks: what follows touches the device
    if not torch.cuda.is_available():
        for name in ("local_align", "local_spans", "local_paths"):
            with pytest.raises((RuntimeError, AssertionError)):
                getattr(align, name)(good, counts_a=[2, 4], pairs=[[0, 1]], gap_open=1.0,
                                     gap_extend=0.5, band=(-1, 1))


def test_the_call_record_appends_the_band_to_the_arguments():
    """``values()`` is what every symbol starts with; with a band its device pointer follows
    gap_extend, where the ``*_band`` symbols take it."""

    class Pointer:
        def __init__(self, value):
            self.value, self.shape = value, (6, 128)

        def data_ptr(self):
            return self.value

    plain = align._Call(Pointer(1), Pointer(2), np.array([0, 2, 6]), np.array([0, 2, 6]),
                        np.zeros((3, 2), dtype=np.int32), np.array([4, 4, 2]), (1.0, 0.0, 1.0, 0.5),
                        Pointer(3), Pointer(4), Pointer(5))
    banded = plain._replace(band=np.zeros((3, 2), dtype=np.int32), band_dev=Pointer(6))
    assert plain.values() == banded.values() == (1, 6, 3, 2, 2, 6, 4, 2, 5, 3, 1.0, 0.0, 1.0, 0.5)
    for kind, name in (("score", "gfy_align_local"), ("span", "gfy_align_local_span"),
                       ("trace", "gfy_align_trace")):
        assert align._symbol(plain, kind) == (name, ())
        assert align._symbol(banded, kind) == (name + "_band", (6,))


def test_c_abi_declares_the_three_symbols_and_names_what_they_refuse():
    lib = native.library()
    void, size = ctypes.c_void_p, ctypes.c_size_t
    call = [void, ctypes.c_int64] * 5 + [ctypes.c_float] * 4
    wanted = {
        "gfy_align_local_band": call + [void, void, void, void, size, void],
        "gfy_align_local_span_band": call + [void, void, void, void, void, size, void],
        "gfy_align_trace_band": call + [void, void, void, void, void, void, ctypes.c_int64,
                                        ctypes.c_int64, void, size, void]}
    for name, arguments in wanted.items():
        result, declared = native.SIGNATURES[name]
        assert result is ctypes.c_int and list(declared) == arguments, name
        assert getattr(lib, name) is not None
        # the counterpart's list with `bands` behind gap_extend
        twin = list(native.SIGNATURES[name[:-len("_band")]][1])
        assert arguments == twin[:14] + [void] + twin[14:], name
    assert native.ABI_VERSION == lib.gfy_abi_version() == 4
    p = ctypes.c_void_p(0x1000)    # non-null: every check fails before anything is dereferenced
    wave = lib.gfy_align_trace_workspace_bytes(1, 100, 200) // 4

    def score_call(a=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, score=p, end=p, ws=p,
                   size=lib.gfy_align_workspace_bytes(10, 0)):
        return lib.gfy_align_local_band(a, 300, p, 3, p, 500, p, 7, pairs, P, 1.0, 0.0, go, ge,
                                        bands, score, end, ws, size, None)

    def span_call(a=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, score=p, start=p, end=p, ws=p,
                  size=lib.gfy_align_span_workspace_bytes(10, 0)):
        return lib.gfy_align_local_span_band(a, 300, p, 3, p, 500, p, 7, pairs, P, 1.0, 0.0, go,
                                             ge, bands, score, start, end, ws, size, None)

    def trace_call(a=p, pairs=p, P=10, go=1.0, ge=0.5, bands=p, starts=p, ends=p, op_ptr=p, ops=p,
                   length=p, rows=100, cols=200, ws=p, size=wave):
        return lib.gfy_align_trace_band(a, 300, p, 3, p, 500, p, 7, pairs, P, 1.0, 0.0, go, ge,
                                        bands, starts, ends, op_ptr, ops, length, rows, cols, ws,
                                        size, None)

    def refusal(call, who, code, text, **changes):
        assert call(**changes) == code, (who, changes)
        message = lib.gfy_last_error()
        assert message.startswith(who + b": ") and text in message, (changes, message)

    holes = {score_call: {"score": b"out_score is NULL", "end": b"out_end is NULL"},
             span_call: {"score": b"out_score is NULL", "start": b"out_start is NULL",
                         "end": b"out_end is NULL"},
             trace_call: {"starts": b"starts is NULL", "ends": b"ends is NULL",
                          "op_ptr": b"op_ptr is NULL", "ops": b"out_ops is NULL",
                          "length": b"out_len is NULL"}}
    for call, who, plain in ((score_call, b"gfy_align_local_band", b"gfy_align_local "),
                             (span_call, b"gfy_align_local_span_band", b"gfy_align_local_span "),
                             (trace_call, b"gfy_align_trace_band", b"gfy_align_trace ")):
        refusal(call, who, native.GFY_ERR_INVALID, b"bands is NULL", bands=None)
        assert plain + b"is the call without a band" in lib.gfy_last_error()
        for hole, text in {"a": b"a is NULL", "pairs": b"pairs is NULL", "ws": b"workspace is NULL",
                           **holes[call]}.items():
            refusal(call, who, native.GFY_ERR_INVALID, text, **{hole: None})
        refusal(call, who, native.GFY_ERR_INVALID, b"P = ", P=0)
        refusal(call, who, native.GFY_ERR_INVALID, b"gap_extend", go=1.0, ge=1.5)
        for short in (0, 1):
            refusal(call, who, native.GFY_ERR_WORKSPACE, b"workspace", size=short)
    refusal(trace_call, b"gfy_align_trace_band", native.GFY_ERR_INVALID, b"negative", rows=-1)
    refusal(trace_call, b"gfy_align_trace_band", native.GFY_ERR_WORKSPACE, b"workspace",
            size=wave - 1)
