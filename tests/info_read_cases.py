"""Constructed pe_info / st_info texts for the device reader (vs_links_from_info) and its host twin (vs_info_read_host), each
with the outcome it must have, written down by hand from the rule of process_pe_info (utils/VStrains_IO.py:603-612) and the
library's contract (include/vstrains_hip.h, vs_info_parse).  Shared by test_info_read_cpu.py and test_info_read_gpu.py.

The header's hash (csrc/vs_info_read_core.h) is restated here so that names that land on one slot of the name table, and a
string with the hash of a listed name, can be found by search -- as seed_index_model.colliding_seeds does for seeds."""
import ctypes as C
from itertools import count

import numpy as np

NAMES = ["1", "2", "3"]


# ---- the header's hash, restated -------------------------------------------------------------------------------------------
def ir_hash(name: bytes) -> int:
    h = 0
    for b in name:
        h = (h * 31 + b) & 0xFFFFFFFF
    return h


def ir_table_bits(n: int) -> int:
    bits = 1
    while bits < 31 and (1 << bits) < 2 * n:
        bits += 1
    return bits


def ir_first_slot(h: int, bits: int) -> int:
    return ((h * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)


def names_on_one_slot(k: int, n_total: int):
    """k decimal names of two digits or more whose first slot in a table for n_total names is the same"""
    bits = ir_table_bits(n_total)
    by_slot = {}
    for i in count(10):
        s = str(i)
        got = by_slot.setdefault(ir_first_slot(ir_hash(s.encode()), bits), [])
        got.append(s)
        if len(got) == k:
            return got


def same_hash(name: str) -> str:
    """another string with the hash of ``name``: h * 31 + b is kept when the last two bytes go (a - 1, b + 31)"""
    other = name[:-2] + chr(ord(name[-2]) - 1) + chr(ord(name[-1]) + 31)
    assert other != name and ir_hash(other.encode()) == ir_hash(name.encode()) and ":" not in other and other.isascii() and other.isprintable()
    return other


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class InfoCase:
    def __init__(self, name, text, kind, cells=(), skipped=0, bad_at=None, quoted=None, names=None):
        """kind: "ok" (cells: (row, column, count) in text order, zero counts included; skipped: lines with an unknown id),
        "python" (a carriage return or a byte >= 0x80 anywhere) or "error" (bad_at: text offset of the first malformed line,
        quoted: what the message quotes of it)."""
        self.name, self.text, self.kind = name, text, kind
        self.cells, self.skipped, self.bad_at, self.quoted = list(cells), skipped, bad_at, quoted
        self.names = list(NAMES if names is None else names)

    def message(self, path):
        return "%s: malformed line at byte %d: '%s' (expected id:id:count)" % (path, self.bad_at, self.quoted)

    def matrix(self):
        """the table of this text alone: every cell adds to [r][c] and, off the diagonal, to [c][r] (int64, wrapping)"""
        n = len(self.names)
        m = np.zeros((n, n), dtype=np.uint64)
        for r, c, v in self.cells:
            m[r, c] += np.uint64(v & 0xFFFFFFFFFFFFFFFF)
            if r != c:
                m[c, r] += np.uint64(v & 0xFFFFFFFFFFFFFFFF)
        return m.view(np.int64)

    def fits(self, window):
        """False when a line that has to be parsed -- one up to the empty line, and up to the first malformed one -- does not
        fit a buffer of ``window`` bytes together with its newline: the file is then the host reader's."""
        parts = self.text.split(b"\n")
        at = 0
        for line in [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else []):
            if line == b"\n":
                return True
            if len(line) > window:
                return False
            if self.kind == "error" and at == self.bad_at:
                return True
            at += len(line)
        return True


def _slot_case():
    a, b, c = names_on_one_slot(3, 3)
    x = same_hash(a)
    text = "%s:%s:1\n%s:%s:2\n%s:%s:3\n%s:%s:4\n%s:%s:5\n" % (a, b, b, c, c, a, x, a, a, x)
    return InfoCase("three_names_on_one_slot", text.encode(), "ok", [(0, 1, 1), (1, 2, 2), (2, 0, 3)], skipped=2, names=[a, b, c])


MAX64, MIN64 = 9223372036854775807, -9223372036854775808

CASES = [
    InfoCase("empty_file", b"", "ok"),
    InfoCase("newline_alone", b"\n", "ok"),
    InfoCase("last_line_without_newline", b"7&8*0:9:57", "ok", [(0, 1, 5)], names=["7&8*0", "9"]),
    InfoCase("last_line_of_one_character", b"1:2:3\nx", "error", bad_at=6, quoted="x"),
    InfoCase("empty_line_then_malformed_text", b"1:2:3\n\nthis is not a line\n1:2:4\n", "ok", [(0, 1, 3)]),
    InfoCase("four_and_more_fields", b"1:2:3:4\n1:3:5:x:y\n2:3:6:\n", "ok", [(0, 1, 3), (0, 2, 5), (1, 2, 6)]),
    InfoCase("signs", b"1:2:+5\n2:3:-5\n", "ok", [(0, 1, 5), (1, 2, -5)]),
    InfoCase("sign_alone", b"1:2:+\n", "error", bad_at=0, quoted="1:2:+"),
    InfoCase("count_missing", b"1:2:5\n1:2:\n", "error", bad_at=6, quoted="1:2:"),
    InfoCase("int64_extremes", b"1:2:9223372036854775807\n1:3:-9223372036854775808\n", "ok", [(0, 1, MAX64), (0, 2, MIN64)]),
    InfoCase("beyond_int64_max", b"1:2:1\n1:2:9223372036854775808\n", "error", bad_at=6, quoted="1:2:9223372036854775808"),
    InfoCase("beyond_int64_min", b"1:2:-9223372036854775809\n", "error", bad_at=0, quoted="1:2:-9223372036854775809"),
    InfoCase("unknown_id_good_count", b"1:9:5\n9:1:5\n1:2:1\n", "ok", [(0, 1, 1)], skipped=2),
    InfoCase("unknown_id_bad_count", b"1:2:1\n1:9:x\n", "error", bad_at=6, quoted="1:9:x"),
    InfoCase("duplicate_lines_add", b"1:2:3\n1:2:4\n2:1:5\n", "ok", [(0, 1, 3), (0, 1, 4), (1, 0, 5)]),
    InfoCase("diagonal_added_once", b"2:2:7\n", "ok", [(1, 1, 7)]),
    InfoCase("zero_counts", b"1:2:0\n2:3:0\n3:3:1\n", "ok", [(0, 1, 0), (1, 2, 0), (2, 2, 1)]),
    InfoCase("name_listed_twice", b"1:2:3\n", "ok", [(2, 1, 3)], names=["1", "2", "1"]),
    InfoCase("names_that_are_prefixes", b"1:12:1\n12:1&2*0:2\n1&2*0:1:3\n1&2:1:4\n", "ok", [(0, 1, 1), (1, 2, 2), (2, 0, 3)], skipped=1,
             names=["1", "12", "1&2*0"]),
    InfoCase("empty_id_field", b":1:5\n1::5\n1:2:1\n", "ok", [(0, 1, 1)], skipped=2),
    InfoCase("two_malformed_lines", b"1:2:3\n1:2\n1:2:x\n", "error", bad_at=6, quoted="1:2"),
    InfoCase("malformed_line_of_75_bytes", b"1:2:" + b"9" * 70 + b"\n", "error", bad_at=0, quoted="1:2:" + "9" * 56),
    InfoCase("carriage_return", b"1:2:3\r\n2:3:4\r\n", "python"),
    InfoCase("byte_0x80", b"1:2:3\n1:\x80:4\n", "python"),
    InfoCase("carriage_return_behind_the_empty_line", b"1:2:3\n\n1:2:4\r\n", "python"),
    _slot_case(),
]
CASE_IDS = [c.name for c in CASES]


def name_arrays(names):
    """(blob uint8, offsets uint64) as the library takes a name list"""
    enc = [s.encode("ascii") for s in names]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8), off


OUTCOMES = {0: "ok", 1: "python", 2: "error", 3: "does_not_fit"}


def read_host(text: bytes, names, window_bytes=0):
    """vs_info_read_host: (outcome word, cells [(r, c, v)], info dict)"""
    from vstrains_amd import _native as nat

    blob, off = name_arrays(names)
    cap = text.count(b"\n") + 1
    rows, cols = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    vals = np.zeros(cap, dtype=np.int64)
    info = (C.c_uint64 * 8)()
    buf = np.frombuffer(text or b"\0", dtype=np.uint8)
    rc = nat.lib().vs_info_read_host(buf.ctypes.data, len(text), blob.ctypes.data, off.ctypes.data, len(names), window_bytes, rows.ctypes.data,
                                     cols.ctypes.data, vals.ctypes.data, cap, info)
    assert rc == 0, nat.lib().vs_last_error(None)
    keys = ("outcome", "lines", "skipped", "cells", "bad_at", "windows", "flags", "text_bytes")
    rec = {k: int(info[i]) for i, k in enumerate(keys)}
    k = rec["cells"]
    return OUTCOMES[rec["outcome"]], list(zip(rows[:k].tolist(), cols[:k].tolist(), vals[:k].tolist())), rec
