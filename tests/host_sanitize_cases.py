"""Cases for tools/host_sanitize.cpp (not a test module): inputs at the seams of the host C++
and what each call must return, worked out WITHOUT the library — the statuses of a weight pack
from the rules of csrc/weight_pack.h, a micro-batch's staging bytes from the numpy twin
(``api.Ginfinity._microbatch_arrays`` + ``_Uploader.pack_at``), encoder rows from
``oracle.gine_numpy``.

A case is ``(name, fields)``; a field is an int, a list of ints, a string or an array.
``write_cases`` puts a list of them into ``data.bin`` + ``manifest.txt`` as the program reads
them; ``run_microbatch`` / ``run_encode`` hand the same fields to the built library through
``ctypes``, so the seam sizes are covered where no sanitizer can be built.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import struct
from pathlib import Path
from types import SimpleNamespace

import numpy as np

OK, INVALID, UNSUPPORTED = 0, 1, 2            # include/gfy.h, gfy_status
F16, F32, F64 = 0, 1, 2                        # include/gfy.h, gfy_dtype
DTYPES = {F16: np.float16, F32: np.float32, F64: np.float64}


# ---- the case files -----------------------------------------------------------------------

def write_cases(directory: Path, cases) -> list[str]:
    """``cases`` → ``directory``; the case names, in order.  Equal arrays are stored once."""
    directory.mkdir(parents=True, exist_ok=True)
    stored: dict[bytes, int] = {}
    lines, names = [], []
    with open(directory / "data.bin", "wb") as data:
        for name, fields in cases:
            assert " " not in name and name not in names, name
            names.append(name)
            lines.append(f"case {name}")
            for key, value in fields.items():
                if value is None:
                    continue
                if isinstance(value, (bool, int, np.integer)):
                    lines.append(f"int {key} {int(value)}")
                elif isinstance(value, (list, tuple)):
                    lines.append(f"ints {key} {len(value)} " + " ".join(str(int(v)) for v in value))
                elif isinstance(value, str):
                    lines.append(f"text {key} {value}")
                else:
                    payload = value if isinstance(value, bytes) else np.ascontiguousarray(value).tobytes()
                    digest = hashlib.sha1(payload).digest() + len(payload).to_bytes(8, "little")
                    if digest not in stored:
                        stored[digest] = data.tell()
                        data.write(payload)
                    lines.append(f"array {key} {stored[digest]} {len(payload)}")
            lines.append("end")
    (directory / "manifest.txt").write_text("\n".join(lines) + "\n")
    return names


# ---- pack ---------------------------------------------------------------------------------

#: weight_pack.h: header words in order, and the largest value a loader accepts for each
HEADER = ("magic", "version", "in_dim", "hidden", "layers", "edge_dim", "out_dim", "flags")
LEGAL_MAXIMUM = {"magic": 0x31594647, "version": 1, "in_dim": 7, "hidden": 128, "layers": 8,
                 "edge_dim": 16, "out_dim": 128, "flags": 1}


def pack_bytes_of(layers: int, edge_dim: int, in_dim: int = 7, h: int = 128, out_dim: int = 128) -> int:
    """include/gfy.h's pack layout counted here: 32 header bytes, then fp32 tensors."""
    m = 2 * h
    layer = 1 + h * edge_dim + h + m * h + m + 4 * m + h * m + h + 2 * h
    return 32 + 4 * (h * in_dim + h + layers * layer + h * h + h + out_dim * h + out_dim)


def pack_verdict(pack: bytes | None, dtype: int) -> tuple[int, str]:
    """Status and words of the error text for a pack, by the rules of weight_pack.h in the order
    it states them: missing / truncated, magic and version, architecture, byte count, dtype."""
    if pack is None or len(pack) < 32:
        return INVALID, "missing or truncated"
    word = dict(zip(HEADER, struct.unpack("<8I", pack[:32])))
    if word["magic"] != 0x31594647 or word["version"] != 1:
        return INVALID, "magic/version"
    if (word["in_dim"] != 7 or word["hidden"] != 128 or word["out_dim"] != 128
            or not 1 <= word["layers"] <= 8 or not 1 <= word["edge_dim"] <= 16):
        return UNSUPPORTED, "built for"
    if len(pack) != pack_bytes_of(word["layers"], word["edge_dim"]):
        return INVALID, "bytes, expected"
    if dtype not in (F16, F32):
        return INVALID, "model_dtype"
    return OK, ""


def pack_cases(packs: dict[str, bytes]):
    """Every valid pack whole, cut and extended, and with every header word off; NULL pack,
    NULL ``out``, a model dtype that is none.  ``length`` / ``word`` / ``value`` tell the
    program what to do to the stored pack; the verdict is worked out here on the same bytes."""
    cases = []

    def add(name, pack, dtype, **fields):
        length = fields.get("length", len(pack))
        changed = bytearray(pack[:length].ljust(length, b"\0"))
        if "word" in fields and length >= 4 * fields["word"] + 4:
            struct.pack_into("<I", changed, 4 * fields["word"], fields["value"])
        status, text = pack_verdict(bytes(changed), dtype)
        cases.append((name, {"pack": pack, "dtype": dtype, "status": status, "error": text, **fields}))

    for label, pack in packs.items():
        expected = len(pack)
        assert expected == pack_bytes_of(*struct.unpack("<8I", pack[:32])[4:6])
        for dtype in (F16, F32):
            tag = f"{label}.m{16 if dtype == F16 else 32}"
            add(f"{tag}.valid", pack, dtype)
            assert cases[-1][1]["status"] == OK
            for length in (0, 1, 31, 32, 33, expected - 4, expected - 1, expected + 1, expected + 4):
                add(f"{tag}.length{length}", pack, dtype, length=length)
                assert cases[-1][1]["status"] == INVALID
            for index, word in enumerate(HEADER):
                for value in (0, 1, LEGAL_MAXIMUM[word] + 1, 0xFFFFFFFF):
                    add(f"{tag}.{word}={value}", pack, dtype, word=index, value=value)
            add(f"{tag}.valid_again", pack, dtype)          # a success clears the error text
    pack = packs["bundled"]
    cases.append(("null_pack", {"pack": pack, "dtype": F16, "null_pack": 1, "length": len(pack),
                                "status": INVALID, "error": "missing or truncated"}))
    cases.append(("null_out", {"pack": pack, "dtype": F16, "null_out": 1, "status": INVALID,
                               "error": "out is NULL"}))
    for dtype in (F64, -1, 7):
        add(f"model_dtype={dtype}", pack, dtype)
        assert cases[-1][1]["status"] == INVALID
    add("bundled.valid_last", pack, F32)
    return cases


# ---- microbatch -----------------------------------------------------------------------------

def make_shard(seed: int, nodes, edges, feature_dim: int = 7, context: bool = False):
    """A shard of ``len(nodes)`` records in the interchange format's arrays: random features,
    random edges inside each record, all ten edge types; ``context``: every third node of a
    record but its first is a context node."""
    rng = np.random.default_rng(seed)
    node_ptr = np.concatenate(([0], np.cumsum(nodes))).astype(np.int64)
    edge_ptr = np.concatenate(([0], np.cumsum(edges))).astype(np.int64)
    blocks = [rng.integers(node_ptr[r], max(node_ptr[r + 1], node_ptr[r] + 1), size=(2, edges[r]))
              for r in range(len(nodes))]
    roles = np.zeros(int(node_ptr[-1]), np.uint8)
    if context:
        inside = np.arange(len(roles)) - np.repeat(node_ptr[:-1], nodes)
        roles[(inside % 3) == 2] = 1
    return SimpleNamespace(
        node_features=rng.standard_normal((int(node_ptr[-1]), feature_dim)).astype(np.float32),
        edge_index=np.ascontiguousarray(np.concatenate(blocks, axis=1).astype(np.int32)),
        edge_types=rng.integers(0, 10, size=int(edge_ptr[-1])).astype(np.uint8),
        node_roles=roles, node_ptr=node_ptr, edge_ptr=edge_ptr)


def twin_layout(shard, start: int, stop: int, with_records: int, base: int):
    """The numpy twin's six entries for records [start, stop) and the bytes of a slot that
    holds them from ``base``: every present entry padded to 256."""
    from ginfinity_amd import api
    arrays, kept = api.Ginfinity._microbatch_arrays(shard, start, stop, bool(with_records))
    plain = [item[0] if isinstance(item, tuple) else item for item in arrays]
    size = base + sum(api._Uploader.padded(a.nbytes) for a in plain if a is not None)
    return arrays, plain, kept, size


def twin_pack(shard, start: int, stop: int, with_records: int, base: int):
    """``(slot bytes, offsets[6], counts[4], slot image)`` from ``_Uploader.pack_at`` over a
    zeroed slot of exactly the layout's size; raises what the twin raises."""
    import torch
    from ginfinity_amd import api
    arrays, plain, kept, size = twin_layout(shard, start, stop, with_records, base)

    class Slot(api._Uploader):
        def __init__(self):
            self._staging = [torch.zeros(size, dtype=torch.uint8)]

    slot = Slot()
    offsets = slot.pack_at(0, base, arrays)
    offsets = [-1 if array is None else offset for offset, array in zip(offsets, plain)]
    counts = [len(plain[0]), plain[1].shape[1], stop - start if plain[4] is not None else 0, kept]
    return size, offsets, counts, slot._staging[0].numpy().tobytes()


def _microbatch_fields(shard, start, stop, with_records=1, base=0, misalign=0, **changes):
    fields = {"node_features": shard.node_features, "feature_dim": shard.node_features.shape[1],
              "edge_index": shard.edge_index, "edges_total": shard.edge_index.shape[1],
              "edge_types": shard.edge_types, "node_roles": shard.node_roles,
              "node_ptr": shard.node_ptr, "edge_ptr": shard.edge_ptr, "start": start,
              "stop": stop, "with_records": with_records, "base": base, "misalign": misalign}
    fields.update(changes)
    return fields


def _accepted(shard, start, stop, with_records=1, base=0, misalign=0, **changes):
    size, offsets, counts, image = twin_pack(shard, start, stop, with_records, base)
    return _microbatch_fields(shard, start, stop, with_records, base, misalign, status=OK,
                              slot_bytes=size, offsets=offsets, counts=counts, want_slot=image,
                              **changes)


def _refused(shard, start, stop, text, base=0, **changes):
    """A call that must fail; the slot is as large as the twin's layout of the range, so what
    the call writes before it refuses stays inside."""
    try:
        size = twin_layout(shard, max(start, 0), max(stop, start, 0), 1, max(base, 0) & ~255)[3]
    except Exception:                       # (pointer arrays the twin cannot cut either)
        size = 4096
    return _microbatch_fields(shard, start, stop, 1, base, 0, status=INVALID, error=text,
                              slot_bytes=size, **changes)


EDGE_COUNTS = (0, 1, 3, 4, 15, 16, 17, 31, 33, 64)      # head, 16-wide body and tail of copy_rebased
#: bytes on both sides of copy_bytes' 4,096-byte switch-over, and its 64-byte body and tail;
#: float rows are multiples of 4 bytes, so the node rows take 4,096 + 60 where the edge types
#: take 4,096 + 63
COPY_SIZES = ((4092, 4092), (4096, 4096), (4100, 4100), (4096 + 60, 4096 + 63))
MISALIGN = (0, 4, 12)


def microbatch_cases():
    from ginfinity_amd.spec import GraphValidationError
    cases = []
    # edge counts: 12 records of 5 nodes; record 0 and record 5 hold E edges (start = 0: no
    # rebasing; start = 5: n0 = 25, e0 > 0), records [4, 7) hold E in their middle record, and
    # the last record holds E, so that both rows of its edges, its types and its node rows end
    # where their arrays end
    for count in EDGE_COUNTS:
        edges = [2] * 12
        edges[0] = edges[5] = edges[11] = count
        for context in (False, True):
            shard = make_shard(100 + count, [5] * 12, edges, context=context)
            for start, stop in ((0, 1), (5, 6), (4, 7), (11, 12)):
                for misalign in MISALIGN:
                    for with_records in (1, 0):
                        fields = _accepted(shard, start, stop, with_records, 256 * (misalign // 4),
                                           misalign)
                        n = 5 * (stop - start)
                        assert fields["counts"][2] == (stop - start if with_records else 0)
                        assert (fields["offsets"][3] == -1) == (not context)
                        assert (fields["counts"][3] < n) == context
                        if start:
                            assert shard.node_ptr[start] > 0 and (shard.edge_ptr[start] > 0 or count == 0)
                        cases.append((f"edges{count}.{'context' if context else 'core'}.r{start}-{stop}"
                                      f".a{misalign}.rec{with_records}", fields))
    # copy sizes: one float per node, so n nodes are 4 n bytes; three records in the range, the
    # first three of the shard and its last three (the copies end where the arrays end)
    for node_bytes, type_bytes in COPY_SIZES:
        n, e = node_bytes // 4, type_bytes
        nodes, edges = [7] * 12, [9] * 12
        for first in (0, 9):
            nodes[first:first + 3] = [n // 3, n // 3, n - 2 * (n // 3)]
            edges[first:first + 3] = [e // 3, e // 3, e - 2 * (e // 3)]
        shard = make_shard(200 + n, nodes, edges, feature_dim=1, context=True)
        for start in (0, 9):
            for misalign in MISALIGN:
                fields = _accepted(shard, start, start + 3, 1, 512, misalign)
                assert fields["counts"][:3] == [n, e, 3]
                cases.append((f"copy{node_bytes}+{type_bytes}.r{start}-{start + 3}.a{misalign}", fields))
    # records: one of 65,537 edges, and an edge that joins two records: no boundaries travel
    long = make_shard(300, [40] * 12, [6, 6, 65537] + [6] * 9)
    for start, stop, misalign in ((1, 4, 0), (2, 3, 4)):
        fields = _accepted(long, start, stop, 1, 0, misalign)
        assert fields["counts"][2] == 0 and fields["offsets"][4] == fields["offsets"][5] == -1
        cases.append((f"record65537.r{start}-{stop}.a{misalign}", fields))
    for row, position in ((0, 0), (1, 16), (1, 33)):
        joined = make_shard(301, [5] * 12, [17] * 12)
        joined.edge_index[row, int(joined.edge_ptr[3]) + position % 17] = int(joined.node_ptr[4]) + 2
        for misalign in MISALIGN:
            fields = _accepted(joined, 2, 5, 1, 256, misalign)
            assert fields["counts"][2] == 0 and fields["offsets"][4] == fields["offsets"][5] == -1
            cases.append((f"joined.row{row}.at{position}.a{misalign}", fields))
            fields = _accepted(joined, 0, 3, 1, 256, misalign)     # a range without that edge
            assert fields["counts"][2] == 3
            cases.append((f"closed.row{row}.at{position}.a{misalign}", fields))
    # no records at all, and no edges at all
    plain = make_shard(302, [5] * 12, [17] * 12, context=True)
    cases.append(("empty_range", _accepted(plain, 4, 4, 1, 0, 0)))
    bare = make_shard(303, [3] * 12, [0] * 12)
    for start, stop in ((0, 12), (5, 7)):
        cases.append((f"no_edges.null_index.r{start}-{stop}",
                      _accepted(bare, start, stop, 1, 0, 4, edge_index=None, edge_types=None)))
    quiet = make_shard(304, [5] * 12, [17, 17, 17, 0, 0, 17, 17, 17, 17, 17, 17, 17])
    cases.append(("no_edges_in_range.null_index",       # (e == 0 is all the call asks for)
                  _accepted(quiet, 3, 5, 1, 0, 0, edge_index=None, edge_types=None)))
    # refusals
    n0, n1 = int(plain.node_ptr[5]), int(plain.node_ptr[7])
    e0 = int(plain.edge_ptr[5])
    for row in (0, 1):
        for label, value in (("below", n0 - 1), ("above", n1)):
            for position in (0, 16, 33):
                broken = make_shard(302, [5] * 12, [17] * 12, context=True)
                broken.edge_index[row, e0 + position] = value
                try:
                    twin_pack(broken, 5, 7, 1, 0)
                except GraphValidationError as error:
                    assert "edge index outside" in str(error)
                else:
                    raise AssertionError("the twin accepted an edge that leaves the range")
                cases.append((f"refused.index_{label}.row{row}.at{position}",
                              _refused(broken, 5, 7, "edge index outside shard node range")))
    total = plain.edge_index.shape[1]
    cases.append(("refused.edge_ptr_beyond_edges_total", _refused(
        plain, 10, 12, "no valid node / edge range", edges_total=total - 1,
        edge_index=np.ascontiguousarray(plain.edge_index[:, :total - 1]),
        edge_types=plain.edge_types[:total - 1])))
    descending = plain.node_ptr.copy()
    descending[7] = descending[5] - 1
    cases.append(("refused.descending_node_ptr",
                  _refused(plain, 5, 7, "no valid node / edge range", node_ptr=descending)))
    descending = plain.edge_ptr.copy()
    descending[7] = descending[5] - 1
    cases.append(("refused.descending_edge_ptr",
                  _refused(plain, 5, 7, "no valid node / edge range", edge_ptr=descending)))
    cases.append(("refused.stop_below_start", _refused(plain, 7, 5, "unaligned base")))
    cases.append(("refused.negative_start", _refused(plain, -1, 5, "unaligned base")))
    for base in (128, 4, -256):
        cases.append((f"refused.base{base}", _refused(plain, 5, 7, "unaligned base", base=base)))
    cases.append(("refused.null_edge_index", _refused(plain, 5, 7, "no valid node / edge range",
                                                      edge_index=None)))
    cases.append(("refused.null_edge_types", _refused(plain, 5, 7, "no valid node / edge range",
                                                      edge_types=None)))
    cases.append(("accepted_after_refusals", _accepted(plain, 5, 7, 1, 0, 12)))
    return cases


def _pointer(value):
    return None if value is None else np.ascontiguousarray(value).ctypes.data


def run_microbatch(lib, fields) -> None:
    """One micro-batch case through the built library (``ctypes``), both copy paths."""
    arrays = {key: None if fields.get(key) is None else np.ascontiguousarray(fields[key])
              for key in ("node_features", "edge_index", "edge_types", "node_roles", "node_ptr",
                          "edge_ptr")}
    size, lead = fields["slot_bytes"], fields["misalign"]
    for stream in (None, "0"):
        if stream is None:
            os.environ.pop("GFY_PACK_STREAM", None)
        else:
            os.environ["GFY_PACK_STREAM"] = stream
        try:
            block = np.zeros(size + lead + 16 + 64, np.uint8)
            first = (-block.ctypes.data) % 16 + lead
            offsets, counts = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 4)()
            status = lib.gfy_pack_microbatch(
                _pointer(arrays["node_features"]), fields["feature_dim"],
                _pointer(arrays["edge_index"]), fields["edges_total"],
                _pointer(arrays["edge_types"]), _pointer(arrays["node_roles"]),
                _pointer(arrays["node_ptr"]), _pointer(arrays["edge_ptr"]), fields["start"],
                fields["stop"], fields["with_records"], block.ctypes.data + first, fields["base"],
                offsets, counts)
        finally:
            os.environ.pop("GFY_PACK_STREAM", None)
        text = lib.gfy_last_error().decode()
        assert status == fields["status"], (stream, status, text)
        assert not block[:first].any() and not block[first + size:].any(), "a byte outside the slot changed"
        if status != OK:
            assert fields["error"] in text
            continue
        assert text == ""
        assert list(offsets) == fields["offsets"] and list(counts) == fields["counts"], stream
        assert block[first:first + size].tobytes() == fields["want_slot"], stream


# ---- encode ---------------------------------------------------------------------------------

NODE_COUNTS = (1, 2, 63, 64, 65, 128, 129, 200)          # parallel_nodes cuts at 64
THREADS = (0, 1, 2, 3, 16, 1000)
#: the suite's bound for fp32-model rows against the reference (test_architectures_host.F32_TOL:
#: twice the reference's own fp32-against-float64 error of 4.96e-7 on normalised rows)
F32_TOL = 1e-6


def make_graph(seed: int, n: int, edge_dim: int, shape: str = "random"):
    """``(x, edge_index, edge_types)``: ``random`` 3 n edges; ``bare`` none; ``hub`` also 70
    in-edges of node n // 2; ``isolated`` no edge touches the last node."""
    rng = np.random.default_rng(seed)
    reach = n - 1 if shape == "isolated" else n
    e = 0 if shape == "bare" else 3 * n
    edges = rng.integers(0, max(reach, 1), size=(2, e))
    if shape == "hub":
        edges = np.concatenate((edges, np.stack((rng.integers(0, n, size=70), np.full(70, n // 2)))),
                               axis=1)[:, rng.permutation(e + 70)]
        assert np.bincount(edges[1]).max() > 64
    if shape == "isolated":
        assert n >= 2 and edges.max() < n - 1
    types = rng.integers(0, edge_dim, size=edges.shape[1]).astype(np.uint8)
    return (rng.standard_normal((n, 7)).astype(np.float32),
            np.ascontiguousarray(edges.astype(np.int32)), types)


def _linear_f16_ascending(x16, w, b):
    """``oracle.gine_numpy._linear_f16`` with the fp32 sum written out in ascending k, one
    rounding per product and per add: what the oracle's ``@`` computes on batches of five rows
    and more, where numpy's matrix product takes the blocked kernel.  On fewer rows (n = 1, 3,
    4 here) it takes another kernel with another summation order, and the oracle's rows then
    differ from its own rows for the same graph inside a larger batch."""
    x = np.asarray(x16).astype(np.float32)
    wt = np.ascontiguousarray(np.asarray(w, np.float32).T)
    acc = np.zeros((x.shape[0], wt.shape[1]), np.float32)
    for k in range(wt.shape[0]):
        acc = acc + x[:, k:k + 1] * wt[k][None, :]
    return (acc + np.asarray(b, np.float32)).astype(np.float16)


def forward_f16_ascending(weights, x, edge_index, edge_types):
    """``oracle.gine_numpy.forward_f16`` independent of the batch's row count (above)."""
    from oracle import gine_numpy as G
    blas = G._linear_f16
    G._linear_f16 = _linear_f16_ascending
    try:
        return G.forward_f16(weights, x, edge_index, edge_types)
    finally:
        G._linear_f16 = blas


def oracle_rows(weights, model_dtype, graph, out_dtype, normalise):
    """fp16 model: ``{"want": rows}`` bit for bit (oracle.gine_numpy keeps the rounding points;
    its matrix products summed as ``_linear_f16_ascending`` says, for graphs of any size).
    fp32 model: the float64 evaluation of the same module and, per element, the suite's bound
    on normalised rows (times the row's norm for raw rows) plus half an ulp of the output
    dtype at the expected value."""
    from oracle import gine_numpy as G
    x, edge_index, edge_types = graph
    numpy_dtype = DTYPES[out_dtype]
    if model_dtype == F16:
        raw = forward_f16_ascending(weights.half(), x, edge_index, edge_types)
        if len(x) >= 63:                  # ... and is the oracle as it stands on a real batch
            assert raw.tobytes() == G.forward_f16(weights.half(), x, edge_index, edge_types).tobytes()
        rows = G.normalise(raw, numpy_dtype) if normalise else raw.astype(numpy_dtype)
        return {"want": rows}
    raw = G.forward_f32(weights, x, edge_index, edge_types, dtype=np.float64)
    norms = np.maximum(np.linalg.norm(raw, axis=1, keepdims=True), 1e-12)
    want = raw / norms if normalise else raw
    scale = np.ones_like(norms) if normalise else norms
    half_ulp = {F16: 2.0 ** -11, F32: 2.0 ** -24, F64: 0.0}[out_dtype]
    floor = 2.0 ** -25 if out_dtype == F16 else 0.0        # half the fp16 subnormal spacing
    tol = F32_TOL * scale + half_ulp * np.abs(want) + floor
    return {"want64": want.astype(np.float64), "tol64": np.broadcast_to(tol, want.shape).astype(np.float64)}


def _encode_fields(pack, model_dtype, graph, out_dtype, normalise, threads, rows=None, **changes):
    x, edge_index, edge_types = graph
    fields = {"pack": pack, "model_dtype": model_dtype, "x": x, "edge_index": edge_index,
              "edge_types": edge_types, "n": len(x), "e": edge_index.shape[1], "out_rows": rows,
              "out_dtype": out_dtype, "normalise": normalise, "threads": list(threads),
              "out_count": len(x) if rows is None else int((rows >= 0).sum()), "status": OK}
    fields.update(changes)
    return fields


def dropped_rows(n: int, seed: int = 0) -> np.ndarray:
    """``out_rows`` with -1 entries: first and last row, and about one row in four between."""
    keep = np.random.default_rng(seed).random(n) >= 0.25
    keep[[0, -1]] = False
    keep[n // 2] = True
    rows = (np.cumsum(keep) - 1).astype(np.int32)
    rows[~keep] = -1
    return rows


def encode_cases(models):
    """``models``: ``{label: (pack bytes, oracle Weights, edge types)}``, the bundled model and a
    variant.  Every node count with every thread count (fp16 model; 1, 3 and 1,000 for the
    fp32 model, whose float64 sums are the slow ones), three graph shapes, and on the 129-node
    hub graph every output dtype with and without normalise and dropped rows."""
    cases = []
    for label, (pack, weights, edge_dim) in models.items():
        graphs = [(f"n{n}", make_graph(400 + n, n, edge_dim)) for n in NODE_COUNTS]
        graphs += [("n65.bare", make_graph(470, 65, edge_dim, "bare")),
                   ("n1.bare", make_graph(471, 1, edge_dim, "bare")),
                   ("n129.hub", make_graph(472, 129, edge_dim, "hub")),
                   ("n64.isolated", make_graph(473, 64, edge_dim, "isolated")),
                   ("n65.isolated", make_graph(474, 65, edge_dim, "isolated"))]
        for model_dtype in (F16, F32):
            tag = f"{label}.m{16 if model_dtype == F16 else 32}"
            threads = THREADS if model_dtype == F16 else (1, 3, 1000)
            for name, graph in graphs:
                out_dtype = F16 if model_dtype == F16 else F32
                cases.append((f"{tag}.{name}", _encode_fields(
                    pack, model_dtype, graph, out_dtype, 1, threads,
                    **oracle_rows(weights, model_dtype, graph, out_dtype, 1))))
            hub = graphs[-3][1]
            rows = dropped_rows(129)
            for out_dtype in (F16, F32, F64):
                for normalise in (1, 0):
                    want = oracle_rows(weights, model_dtype, hub, out_dtype, normalise)
                    for kind, out_rows in (("all", None), ("dropped", rows)):
                        kept = want if out_rows is None else {k: v[out_rows >= 0] for k, v in want.items()}
                        cases.append((f"{tag}.n129.hub.out{out_dtype}.norm{normalise}.{kind}",
                                      _encode_fields(pack, model_dtype, hub, out_dtype, normalise,
                                                     (3, 1), out_rows, **kept)))
    # refusals (gine_host.cpp): nothing is written, the text says which
    label, (pack, weights, edge_dim) = next(iter(models.items()))
    graph = make_graph(480, 65, edge_dim)
    x, edge_index, edge_types = graph

    def refused(name, text, graph=graph, **changes):
        cases.append((f"refused.{name}", _encode_fields(
            pack, F16, graph, changes.pop("out_dtype", F16), 1, (1, 3),
            **{"status": INVALID, "error": text, **changes})))

    refused("null_encoder", "bad arguments", null_encoder=1)
    refused("negative_n", "bad arguments", n=-1)
    refused("zero_n", "bad arguments", n=0)
    refused("negative_e", "bad arguments", e=-1)
    refused("null_edge_index", "bad arguments", edge_index=None)
    refused("out_dtype3", "unsupported out_dtype", out_dtype=3, out_count=0)
    for row, value, what in ((0, 65, "source_above"), (0, -1, "source_below"), (1, 65, "destination_above"),
                             (1, -1, "destination_below")):
        for position in (0, edge_index.shape[1] - 1):
            broken = edge_index.copy()
            broken[row, position] = value
            refused(f"{what}.at{position}", "outside the shard", graph=(x, broken, edge_types))
    outside = edge_types.copy()
    outside[7] = edge_dim
    refused("edge_type", "outside the shard", graph=(x, edge_index, outside))
    cases.append(("accepted_after_refusals", _encode_fields(
        pack, F16, graph, F16, 1, (2,), **oracle_rows(weights, F16, graph, F16, 1))))
    return cases


def run_encode(lib, encoders, fields) -> None:
    """One encode case through the built library (``ctypes``); ``encoders`` caches handles by
    (pack, model dtype)."""
    handle = None
    if not fields.get("null_encoder"):
        key = (id(fields["pack"]), fields["model_dtype"])
        if key not in encoders:
            made = ctypes.c_void_p()
            assert lib.gfy_host_encoder_create(fields["pack"], len(fields["pack"]),
                                               fields["model_dtype"], ctypes.byref(made)) == OK
            encoders[key] = made
        handle = encoders[key]
    x, edge_index, edge_types, rows = (None if fields.get(k) is None else np.ascontiguousarray(fields[k])
                                       for k in ("x", "edge_index", "edge_types", "out_rows"))
    dtype = DTYPES.get(fields["out_dtype"], np.uint8)
    first = None
    for threads in fields["threads"]:
        out = np.full((fields["out_count"], 128), 0xAB, np.uint8).repeat(np.dtype(dtype).itemsize, axis=1)
        status = lib.gfy_host_encode(handle, _pointer(x), _pointer(edge_index), _pointer(edge_types),
                                     fields["n"], fields["e"], _pointer(rows), out.ctypes.data,
                                     fields["out_dtype"], fields["normalise"], threads)
        text = lib.gfy_last_error().decode()
        assert status == fields["status"], (threads, status, text)
        if status != OK:
            assert fields["error"] in text and (out == 0xAB).all()
            continue
        assert text == ""
        got = out.view(dtype)
        if "want" in fields:
            assert got.tobytes() == fields["want"].tobytes(), threads
        else:
            off = np.abs(got.astype(np.float64) - fields["want64"])
            assert (off <= fields["tol64"]).all(), (threads, float(off.max()))
        first = got.tobytes() if first is None else first
        assert got.tobytes() == first, threads


# ---- threads ----------------------------------------------------------------------------------

def threads_cases(pack, weights, edge_dim):
    """Two threads with an encoder each (20 encodes of the 129-node graph, three workers) next to
    a thread whose packs are refused; then one const encoder under two encoding threads."""
    graph = make_graph(472, 129, edge_dim, "hub")
    x, edge_index, edge_types = graph
    common = {"pack": pack, "x": x, "edge_index": edge_index, "edge_types": edge_types,
              "n": len(x), "e": edge_index.shape[1], "rounds": 20,
              "want": oracle_rows(weights, F16, graph, F16, 1)["want"]}
    verdict = pack_verdict(pack[:len(pack) - 4], F16)
    assert verdict[0] == INVALID
    return [("own_encoders", {**common, "bad_length": len(pack) - 4, "error": verdict[1]}),
            ("shared_encoder", {**common, "shared": 1})]
