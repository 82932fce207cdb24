"""The plain model of two FASTQ files paired by read name (``pe.PairedNameStream``, csrc/vs_pair_names.hip).

Records, the name token and ``mates(a, b)`` are those of tests/interleaved_model.py; ``a`` is the header line of the file-1
record and ``b`` that of the file-2 record.

Key of a record: its token, without a trailing ``/1`` on a file-1 record and without a trailing ``/2`` on a file-2 record.  Two
records are a pair iff they are of different files, their keys are non-empty and equal, and ``mates`` says so.

An input is valid when (V1) within one file no non-empty key occurs twice and (V2) the file-1 records that have a mate, in
file order, have their mates in increasing file-2 order.  For a valid input the pairs are exactly the records whose key is in
both files (and ``mates``), in file-1 order; every other complete record is a single of its file.

``join`` is that definition by dict on two whole texts -- or on two windows, where it also says what a round of the window
protocol decides: every record up to the last match, and every record of the other window when a file is at its end.
``drive`` runs the window protocol on any join (the host twin, the kernels) over two texts cut into chunks."""
from interleaved_model import mates, records, token


def key(header: bytes, file: int) -> bytes:
    t = token(header)
    return t[:-2] if t.endswith(b"/2" if file else b"/1") else t


def pn_hash(k: bytes, bits: int = 64) -> int:
    """FNV-1a over the key bytes, then the finaliser of MurmurHash3"""
    m = (1 << 64) - 1
    h = 0xCBF29CE484222325
    for c in k:
        h = ((h ^ c) * 0x100000001B3) & m
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & m
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & m
    h ^= h >> 33
    return h & ((1 << bits) - 1)


def join(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True):
    """(pairs [(i, j)], info) of two texts or windows.  info: ``records``, ``decided`` (a pair of counts each),
    ``duplicate`` = (file, the smallest record of that file whose key occurs twice in it) or None -- file 1 first --,
    ``order`` = the first pair whose file-2 record does not lie behind that of the pair before, or None (also with a
    duplicate).  With either set there are no pairs and nothing is decided."""
    heads = [[r[0] for r in records(text0, eof0)], [r[0] for r in records(text1, eof1)]]
    keys = [[key(h, f) for h in heads[f]] for f in (0, 1)]
    dup = None
    index = [{}, {}]
    for f in (0, 1):
        twice = []
        for r, k in enumerate(keys[f]):
            if not k:
                continue
            if k in index[f]:
                twice += [index[f][k], r]
            else:
                index[f][k] = r
        if twice and dup is None:
            dup = (f, min(twice))
    pairs = []
    for i, k in enumerate(keys[0]):
        j = index[1].get(k) if k else None
        if j is not None and mates(heads[0][i], heads[1][j]):
            pairs.append((i, j))
    order = None if dup else next((p for p in range(1, len(pairs)) if pairs[p][1] <= pairs[p - 1][1]), None)  # (a key twice: no pairs, no order)
    n = (len(heads[0]), len(heads[1]))
    info = dict(pairs=len(pairs), records=n, decided=(0, 0), duplicate=dup, order=order, first_bad=None)
    if dup is not None or order is not None:
        info["pairs"] = 0
        return [], info
    dec = [pairs[-1][0] + 1, pairs[-1][1] + 1] if pairs else [0, 0]
    if eof1:
        dec[0] = n[0]
    if eof0:
        dec[1] = n[1]
    info["decided"] = tuple(dec)
    return pairs, info


def strict(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True):
    """the strict mode on two texts or windows: pair p is record p of either; (pairs, info with ``first_bad``)"""
    heads = [[r[0] for r in records(text0, eof0)], [r[0] for r in records(text1, eof1)]]
    n = min(len(heads[0]), len(heads[1]))
    bad = next((p for p in range(n) if not mates(heads[0][p], heads[1][p])), None)
    return [(p, p) for p in range(n)], dict(pairs=n, records=(len(heads[0]), len(heads[1])), decided=(n, n), duplicate=None, order=None, first_bad=bad)


def filtered(text0: bytes, text1: bytes):
    """the two files repaired: (R1 bytes, R2 bytes, singles of file 1, singles of file 2) of a valid input"""
    pairs, info = join(text0, text1)
    assert info["duplicate"] is None and info["order"] is None
    recs = [records(text0), records(text1)]
    out = [b"".join(b"\n".join(recs[f][p[f]]) + b"\n" for p in pairs) for f in (0, 1)]
    return out[0], out[1], info["records"][0] - len(pairs), info["records"][1] - len(pairs)


def end_of_record(text: bytes, n: int) -> int:
    """one past the line end that closes record n - 1 (the end of the text when its last line has none)"""
    at = 0
    for _ in range(4 * n):
        nl = text.find(b"\n", at)
        if nl < 0:
            return len(text)
        at = nl + 1
    return at


def chunks_after_every_record(text: bytes):
    """chunk ends: one past every record (and the end of the text)"""
    ends = [end_of_record(text, r + 1) for r in range(len(records(text)))]
    return sorted(set(ends + [len(text)]))


def drive(join_fn, text0: bytes, text1: bytes, ends0, ends1, pick=None):
    """The window protocol over two texts that arrive in chunks (``ends*``: rising chunk ends, the last one the text's
    length).  ``join_fn(w0, w1, eof0, eof1)`` -> (pairs, info) joins one pair of windows.  ``pick(round, sizes, eof)`` says
    which files get their next chunk (a pair of bools; at least one file that is not at its end is always served); default:
    the smaller window, both when they are equal.  Returns (pairs with file-wide record numbers, singles per file, rounds,
    the largest window)."""
    text, ends = (text0, text1), (list(ends0), list(ends1))
    for f in (0, 1):
        assert ends[f] and ends[f][-1] == len(text[f]) and ends[f] == sorted(ends[f])
    win, at, nxt, base = [b"", b""], [0, 0], [0, 0], [0, 0]
    eof = [False, False]
    pairs, singles, rounds, largest = [], [0, 0], 0, 0
    while True:
        want = pick(rounds, (len(win[0]), len(win[1])), tuple(eof)) if pick else (len(win[0]) <= len(win[1]), len(win[1]) <= len(win[0]))
        want = [bool(want[f]) and not eof[f] for f in (0, 1)]
        if not any(want):
            want = [not eof[0], not eof[1]]
        for f in (0, 1):
            if want[f]:
                win[f] += text[f][at[f]:ends[f][nxt[f]]]
                at[f] = ends[f][nxt[f]]
                nxt[f] += 1
                eof[f] = nxt[f] == len(ends[f])
        got, info = join_fn(win[0], win[1], eof[0], eof[1])
        rounds += 1
        largest = max(largest, len(win[0]), len(win[1]))
        if info["duplicate"] is not None:
            raise ValueError("duplicate %r" % (info["duplicate"],))
        if info["order"] is not None:
            raise ValueError("order %d" % info["order"])
        pairs += [(base[0] + int(i), base[1] + int(j)) for i, j in got]
        for f in (0, 1):
            dec = info["decided"][f]
            singles[f] += dec - len(got)
            win[f] = win[f][end_of_record(win[f], dec):]
            base[f] += dec
        if eof[0] and eof[1]:
            return pairs, tuple(singles), rounds, largest
