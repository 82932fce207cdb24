"""The plain model of the interleaved FASTQ ingest (``pe.InterleavedStream``, csrc/vs_interleaved.hip), and the constructed
cases its tests share.

A record is four lines: complete records = lines // 4, a final line without a newline counts at the end of the file, a
trailing group of fewer than four lines is ignored.  (The model splits at ``\\n`` only: text mode -- ``\\r``, bytes >= 0x80 --
is the two-file stream's, applied before names are compared, and the tests compare such files with their plain form.)

Name token of a record: its first line from its first byte up to (not including) the first space, tab or the line's end.
``mates(a, b)``: take both tokens; if a's ends in ``/1`` AND b's in ``/2`` drop those two bytes from both; true iff both are
non-empty, of equal length and equal byte for byte.

Pairing is greedy from the front, as ``bwa mem -p`` pairs::

    i = 0
    while i < R:
        if i + 1 < R and mates(i, i + 1):  pair (i, i + 1);  i += 2
        else:                              single i;         i += 1

With ``eof`` false the window's last complete record has no successor yet: it is held back (neither a single nor a pair)
unless it is the second of a pair."""


def records(text: bytes, eof: bool = True):
    """the complete records of the text, each a list of its four lines (without line ends)"""
    lines = text.split(b"\n")
    last = lines.pop()  # (what follows the last newline: a line only at the end of the file, and only if it has bytes)
    if eof and last:
        lines.append(last)
    return [lines[4 * r:4 * r + 4] for r in range(len(lines) // 4)]


def token(header: bytes) -> bytes:
    for k, c in enumerate(header):
        if c in (0x20, 0x09):
            return header[:k]
    return header


def mates(a: bytes, b: bytes) -> bool:
    """a, b: the header lines of two adjacent records"""
    ta, tb = token(a), token(b)
    if ta.endswith(b"/1") and tb.endswith(b"/2"):
        ta, tb = ta[:-2], tb[:-2]
    return len(ta) > 0 and ta == tb


def pairing(text: bytes, eof: bool = True):
    """(pairs [(i, i + 1)], singles [i], the record held back or None, complete records)"""
    recs = records(text, eof)
    n = len(recs)
    pairs, singles, held = [], [], None
    i = 0
    while i < n:
        if i + 1 < n and mates(recs[i][0], recs[i + 1][0]):
            pairs.append((i, i + 1))
            i += 2
        else:
            if i + 1 == n and not eof:
                held = i
            else:
                singles.append(i)
            i += 1
    return pairs, singles, held, n


def deinterleave(text: bytes, singles: bool):
    """(R1 bytes, R2 bytes, single indices): the two files the interleaved text stands for.  ``singles`` false is the strict
    mode: ValueError naming the first single record."""
    recs = records(text, True)
    pairs, single, _, _ = pairing(text, True)
    if single and not singles:
        raise ValueError("record %d has no mate" % single[0])
    r1 = b"".join(b"\n".join(recs[a]) + b"\n" for a, _ in pairs)
    r2 = b"".join(b"\n".join(recs[b]) + b"\n" for _, b in pairs)
    return r1, r2, single


def interleave(r1: bytes, r2: bytes) -> bytes:
    """two FASTQ texts of equally many records, record by record"""
    a, b = records(r1), records(r2)
    assert len(a) == len(b)
    return b"".join(b"\n".join(x) + b"\n" + b"\n".join(y) + b"\n" for x, y in zip(a, b))


# ---- constructed cases ---------------------------------------------------------------------------------------------------
def record(header: bytes, k: int = 0) -> bytes:
    seq = b"ACGTTGCA"[: 1 + k % 8] * (1 + k % 3)
    return header + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"


def from_headers(headers) -> bytes:
    return b"".join(record(h, k) for k, h in enumerate(headers))


def by_runs(headers):
    """(pairs, singles) of records whose header lines are bare tokens without /1, /2, spaces or tabs, stated by RUNS, not
    by the greedy walk: a maximal run of L equal non-empty names is L // 2 pairs from its start and, if L is odd, a single
    at its end."""
    pairs, singles = [], []
    i = 0
    while i < len(headers):
        j = i
        while j + 1 < len(headers) and headers[j + 1] == headers[i] and headers[i]:
            j += 1
        run = j - i + 1
        pairs += [(i + 2 * p, i + 2 * p + 1) for p in range(run // 2)]
        if run % 2:
            singles.append(j)
        i = j + 1
    return pairs, singles


def filler(n: int):
    """n records in front of a run: unique pairs, led by one single if n is odd"""
    out = [b"@lead"] if n % 2 else []
    for p in range(n // 2):
        out += [b"@f%d" % p] * 2
    return out


RUN_OFFSETS = list(range(61, 67)) + list(range(253, 259))  # the wavefront edge 63|64, the workgroup edge 255|256


def name_cases():
    """(name, header lines): records named by bare tokens; ``by_runs`` says what they pair to"""
    A, B = b"@A", b"@B"
    out = [
        ("one_record", [A]),
        ("one_pair", [A, A]),
        ("two_singles", [A, B]),
        ("three_records", [A, A, B]),
        ("run2", [A, A, B, B]),
        ("run3_then_pair", [A, A, A, B, B]),
        ("run4", [A, A, A, A]),
        ("run5", [A, A, A, A, A]),
        ("run1000", [A] * 1000),
        ("run1001", [A] * 1001),
        ("alternating_pair_single", sum(([b"@p%d" % k] * 2 + [b"@s%d" % k] for k in range(40)), [])),
        ("singles_only", [b"@s%d" % k for k in range(70)]),
        ("single_first_and_last", [b"@x", A, A, B, B, b"@y"]),
        ("two_adjacent_singles", [A, A, b"@x", b"@y", B, B]),
        ("empty_header_lines", [b"", b"", A, A]),
    ]
    for run in (2, 3, 4, 5):
        for off in RUN_OFFSETS:
            out.append(("run%d_at_%d" % (run, off), filler(off) + [b"@R"] * run + [b"@tail"] * 2))
    return out


def differing_names():
    """name lengths 1..40, the two tokens differing at each byte position in turn (two singles), each followed by a pair of
    that length: (text, pairs, singles)"""
    headers, pairs, singles = [], [], []
    for length in range(1, 41):
        for pos in range(length):
            x = bytes(97 + k % 7 for k in range(length))
            y = x[:pos] + b"Z" + x[pos + 1:]
            q = b"q" * length
            at = len(headers)
            headers += [x, y, q, q]
            singles += [at, at + 1]
            pairs.append((at + 2, at + 3))
    return from_headers(headers), pairs, singles


def cases():
    """(name, text, pairs, singles) at the end of the file; pairs / singles stated independently of ``pairing``"""
    out = []
    for name, headers in name_cases():
        out.append((name, from_headers(headers)) + by_runs(headers))
    two = from_headers([b"@A", b"@A"])
    out += [
        ("empty", b"", [], []),
        ("three_lines_only", b"@A\nAC\n+\n", [], []),
        ("no_final_newline", two[:-1], [(0, 1)], []),
        ("last_line_missing_at_eof", from_headers([b"@A"]) + b"@A\nAC\n+", [], [0]),  # (three lines: no record)
        ("quality_line_without_newline", from_headers([b"@A"]) + b"@A\nAC\n+\nII", [(0, 1)], []),
    ]
    for extra in (1, 2, 3):
        out.append(("trailing_%d_lines" % extra, two + b"\n".join([b"@A", b"AC", b"+"][:extra]) + b"\n", [(0, 1)], []))
    text, pairs, singles = differing_names()
    out.append(("names_differ_at_each_byte", text, pairs, singles))
    h = from_headers
    out += [
        ("prefix_short_first", h([b"@abc", b"@abcd"]), [], [0, 1]),
        ("prefix_long_first", h([b"@abcd", b"@abc"]), [], [0, 1]),
        ("slash_1_2", h([b"@a/1", b"@a/2"]), [(0, 1)], []),
        ("slash_2_1", h([b"@a/2", b"@a/1"]), [], [0, 1]),
        ("slash_1_1", h([b"@a/1", b"@a/1"]), [(0, 1)], []),
        ("slash_2_2", h([b"@a/2", b"@a/2"]), [(0, 1)], []),
        ("slash_1_2_other_name", h([b"@a/1", b"@b/2"]), [], [0, 1]),
        ("slash_1_and_bare", h([b"@a/1", b"@a"]), [], [0, 1]),
        ("only_slash_1_2", h([b"/1", b"/2"]), [], [0, 1]),  # (nothing is left of either token)
        ("only_slash_1_1", h([b"/1", b"/1"]), [(0, 1)], []),  # (identical tokens, nothing dropped)
        ("comment_after_space", h([b"@a 1:N:0:x", b"@a 2:N:0:x"]), [(0, 1)], []),
        ("comment_after_tab", h([b"@a\t1:N:0:x", b"@a\tother"]), [(0, 1)], []),
        ("space_ends_the_token", h([b"@a b", b"@a c", b"@ab", b"@a"]), [(0, 1)], [2, 3]),
        ("header_starts_with_space", h([b" x", b" x"]), [], [0, 1]),  # (an empty token never matches)
        ("slash_after_comment_is_no_suffix", h([b"@a /1", b"@a /2"]), [(0, 1)], []),
    ]
    return out


def with_singles(r1: bytes, r2: bytes) -> bytes:
    """the pairs of two FASTQ texts interleaved, with single records among them as `samtools fastq x.bam` writes them: one at
    record 0, one at the last record, two adjacent ones, and one behind every 37th pair"""
    a, b = records(r1), records(r2)
    assert len(a) == len(b) and len(a) > 100
    single = lambda k: record(b"@single%d extra" % k, k)
    out = [single(0)]
    for p, (x, y) in enumerate(zip(a, b)):
        out.append(b"\n".join(x) + b"\n" + b"\n".join(y) + b"\n")
        if p % 37 == 5:
            out.append(single(p))
        if p == 50:
            out += [single(10 ** 6), single(10 ** 6 + 1)]
    out.append(single(10 ** 7))
    return b"".join(out)
