"""Every refusal of the alignment entry points of the C ABI, code and text, byte for byte: a fixed
list of bad calls against the twelve launch entry points, gfy_align_path_values and the four size
functions, replayed against the built library and compared with tests/golden/align_refusals.json.
The golden file was written by the library as it stood before the entry points were folded into
one shared check, so the order of the checks, the codes and the texts are pinned as they were.

No device is touched: every call of the list is refused before a launch (the pointers are the
non-null 0x1000, which nothing dereferences).  ``python tests/test_align_refusals_host.py --write``
regenerates the golden file from the library that GFY_LIBRARY names (default: the in-tree build)."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "align_refusals.json"
POINTER = 0x1000
NAN = float("nan")

#: what every alignment call starts with, and a good value of each
LEAD = dict(a=POINTER, n=300, ptr_a=POINTER, records_a=3, b=POINTER, m=500, ptr_b=POINTER,
            records_b=7, pairs=POINTER, P=10, match_scale=1.0, match_shift=0.0, gap_open=1.0,
            gap_extend=0.5)
SCORE = ("out_score", "out_end")
SPAN = ("out_score", "out_start", "out_end")
TRACE = ("starts", "ends", "op_ptr", "out_ops", "out_len", "max_box_rows", "max_box_cols")
GLOBAL_TRACE = ("ends", "op_ptr", "out_ops", "out_len", "out_start", "max_rows_a", "max_rows_b")
WORKSPACE = ("ws", "ws_bytes", "stream")
#: symbol: the arguments behind gap_extend, in the order of include/gfy.h
ENTRIES = {
    "gfy_align_local": (*SCORE, *WORKSPACE),
    "gfy_align_local_span": (*SPAN, *WORKSPACE),
    "gfy_align_trace": (*TRACE, *WORKSPACE),
    "gfy_align_local_band": ("bands", *SCORE, *WORKSPACE),
    "gfy_align_local_span_band": ("bands", *SPAN, *WORKSPACE),
    "gfy_align_trace_band": ("bands", *TRACE, *WORKSPACE),
    "gfy_align_local_box": ("bands", "boxes", *SCORE, *WORKSPACE),
    "gfy_align_local_span_box": ("bands", "boxes", *SPAN, *WORKSPACE),
    "gfy_align_local_null": ("bands", "boxes", "shuffles", "order", "order_ptr", "out_score",
                             *WORKSPACE),
    "gfy_align_global": ("within", *SCORE, *WORKSPACE),
    "gfy_align_global_trace": ("within", *GLOBAL_TRACE, *WORKSPACE),
    "gfy_align_global_box": ("within", "boxes", *SCORE, *WORKSPACE),
    "gfy_align_global_trace_box": ("within", "boxes", *GLOBAL_TRACE, *WORKSPACE),
    "gfy_align_path_values": ("starts", "op_ptr", "ops", "n_ops", "out_cosine", "out_running",
                              "out_score", "out_counts", "out_cosine_sum", "max_waves", "stream"),
}
#: good values of what is no pointer
NUMBERS = dict(within=0, shuffles=8, max_box_rows=100, max_box_cols=200, max_rows_a=100,
               max_rows_b=200, n_ops=50, max_waves=0, stream=None)
#: pointers that may be NULL: alone they are no refusal, so the workspace is one byte short too
OPTIONAL = {"gfy_align_local_box": ("bands",), "gfy_align_local_span_box": ("bands",),
            "gfy_align_local_null": ("bands", "boxes")}
SIZES = (("gfy_align_workspace_bytes", (10, 0)), ("gfy_align_workspace_bytes", (10, 333)),
         ("gfy_align_workspace_bytes", (0, 5000)), ("gfy_align_workspace_bytes", (-3, -1)),
         ("gfy_align_workspace_bytes", (10 ** 9, 4096)),
         ("gfy_align_span_workspace_bytes", (10, 0)), ("gfy_align_span_workspace_bytes", (10, 333)),
         ("gfy_align_span_workspace_bytes", (0, 5000)), ("gfy_align_span_workspace_bytes", (-3, -1)),
         ("gfy_align_span_workspace_bytes", (10 ** 9, 4096)),
         ("gfy_align_trace_workspace_bytes", (1, 100, 200)),
         ("gfy_align_trace_workspace_bytes", (10, 0, 0)),
         ("gfy_align_trace_workspace_bytes", (0, -1, 9)),
         ("gfy_align_trace_workspace_bytes", (10 ** 9, 10 ** 9, 10 ** 9)),
         ("gfy_align_trace_workspace_bytes", (5, 4096, 1)),
         ("gfy_align_global_trace_workspace_bytes", (1, 100, 200)),
         ("gfy_align_global_trace_workspace_bytes", (10, 0, 0)),
         ("gfy_align_global_trace_workspace_bytes", (0, -1, 9)),
         ("gfy_align_global_trace_workspace_bytes", (10 ** 9, 10 ** 9, 10 ** 9)),
         ("gfy_align_global_trace_workspace_bytes", (5, 4096, 1)))


def _good(lib, symbol: str) -> dict:
    """A call of ``symbol`` that passes every check: each case changes it so that one fails."""
    names = ENTRIES[symbol]
    call = dict(LEAD)
    for name in names:
        call[name] = NUMBERS.get(name, POINTER)
    if "max_box_rows" in names or "max_rows_a" in names:       # a trace call: one wave's bytes
        call["ws_bytes"] = lib.gfy_align_trace_workspace_bytes(1, 100, 200) // 4
    elif symbol == "gfy_align_local_null":
        call["ws_bytes"] = lib.gfy_align_workspace_bytes(LEAD["P"] * NUMBERS["shuffles"], 0)
    elif "out_start" in names:
        call["ws_bytes"] = lib.gfy_align_span_workspace_bytes(LEAD["P"], 0)
    elif "ws_bytes" in names:
        call["ws_bytes"] = lib.gfy_align_workspace_bytes(LEAD["P"], 0)
    return call


def cases(lib, symbol: str):
    """(case, the changed arguments) of every bad call of ``symbol``, in a fixed order."""
    good = _good(lib, symbol)
    short = {"ws_bytes": good["ws_bytes"] - 1} if "ws_bytes" in good else None
    optional = OPTIONAL.get(symbol, ())
    for name, value in good.items():
        if value != POINTER:
            continue
        also = short if name in optional else {}
        yield f"{name} NULL", {name: None, **also}
        if name != "a":
            yield f"{name} and a NULL", {name: None, "a": None, **also}
    for change in (dict(n=0), dict(m=0), dict(n=2 ** 31 - 1), dict(m=2 ** 40), dict(records_a=0),
                   dict(records_b=2 ** 31 - 1), dict(P=0), dict(P=2 ** 31)):
        yield " ".join(f"{key} = {value}" for key, value in change.items()), change
    for name in ("match_scale", "match_shift", "gap_open", "gap_extend"):
        yield f"{name} NaN", {name: NAN}
    yield "gap_extend > gap_open", dict(gap_open=1.0, gap_extend=1.5)
    for name in ("within", "max_box_rows", "max_box_cols", "max_rows_a", "max_rows_b", "n_ops",
                 "max_waves"):
        if name in good:
            value = 2 if name == "within" else -1
            yield f"{name} = {value}", {name: value}
    if "shuffles" in good:
        yield "shuffles = 0", dict(shuffles=0)
        yield "P * shuffles = 2^16 * 2^15", dict(P=2 ** 16, shuffles=2 ** 15)
        yield "P * shuffles = 3 * 2^62", dict(P=3, shuffles=2 ** 62)
    if short:
        yield "workspace one byte short", short
        yield "workspace of 0 bytes", dict(ws_bytes=0)


def replay(lib) -> dict:
    refusals = []
    for symbol in ENTRIES:
        for case, change in cases(lib, symbol):
            code = getattr(lib, symbol)(*{**_good(lib, symbol), **change}.values())
            refusals.append(dict(symbol=symbol, case=case, code=code,
                                 text=lib.gfy_last_error().decode()))
    sizes = [dict(symbol=symbol, arguments=list(arguments), bytes=getattr(lib, symbol)(*arguments))
             for symbol, arguments in SIZES]
    return dict(refusals=refusals, sizes=sizes)


def _library():
    from ginfinity_amd import _native as native
    return native, native.library()


def test_the_list_covers_every_alignment_entry_point_and_never_reaches_a_launch():
    native, _ = _library()
    declared = {name for name in native.SIGNATURES if name.startswith("gfy_align")}
    assert declared == set(ENTRIES) | {symbol for symbol, _ in SIZES}
    for symbol, names in ENTRIES.items():
        assert len(native.SIGNATURES[symbol][1]) == len(LEAD) + len(names), symbol
    golden = json.loads(GOLDEN.read_text())
    assert 300 <= len(golden["refusals"]) <= 900 and GOLDEN.stat().st_size < 100 * 1024
    for entry in golden["refusals"]:                  # a refusal of the arguments, never of HIP
        assert entry["code"] in (native.GFY_ERR_INVALID, native.GFY_ERR_WORKSPACE), entry
        assert entry["text"].startswith(entry["symbol"] + ": "), entry


def test_every_refusal_keeps_its_code_and_its_text():
    _, lib = _library()
    golden, got = json.loads(GOLDEN.read_text()), replay(lib)
    assert [(e["symbol"], e["case"]) for e in got["refusals"]] == \
        [(e["symbol"], e["case"]) for e in golden["refusals"]]
    wrong = [(mine, theirs) for mine, theirs in zip(got["refusals"], golden["refusals"])
             if mine != theirs]
    assert not wrong, wrong[:5]
    assert got["sizes"] == golden["sizes"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_align_refusals_host.py --write")
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    found = replay(_library()[1])
    bad = [entry for entry in found["refusals"] if entry["code"] not in (1, 4)]
    if bad:
        sys.exit(f"not refused before the launch: {bad[:5]}")
    lines = [json.dumps(entry) for entry in found["refusals"]]
    sizes = [json.dumps(entry) for entry in found["sizes"]]
    GOLDEN.write_text('{"refusals": [\n' + ",\n".join(lines) + '\n],\n"sizes": [\n'
                      + ",\n".join(sizes) + "\n]}\n")
    print(f"{GOLDEN}: {len(lines)} refusals, {len(sizes)} sizes, {GOLDEN.stat().st_size} bytes")
