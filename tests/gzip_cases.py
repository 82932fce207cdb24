"""Constructed plain gzip streams for the parallel decoder (vs_gzip_core.h): the CPU suite runs them through the one-lane
host twin ``vs_gzip_inflate_host``, the GPU suite through the kernels (``vs_gzip_inflate``).  zlib is the oracle: a good
case is what ``zlib_text`` turns back into the text, a bad case is what it refuses.  Streams come from Python's zlib with
its knobs (level, memLevel, strategy, flush modes); where zlib cannot be made to write a block -- a distance beyond its
own 32 506, a stored block around deflate bytes, a match in front of a member -- the block is written by hand."""
import functools
import os
import struct
import zlib

import numpy as np

import bgzf_util as bu
from conftest import GOLDEN

EVERY = 0      # granularity "every candidate"
COARSE = 4096  # compressed bytes per selected start


def golden_fastq(case="hiv_like_k55") -> bytes:
    with open(os.path.join(GOLDEN, "pe", case, "fwd.fq"), "rb") as fh:
        fwd = fh.read()
    with open(os.path.join(GOLDEN, "pe", case, "rve.fq"), "rb") as fh:
        return fwd + fh.read()


def fastq_with_edits(n: int, seed=5, every=50) -> bytes:
    """n bytes: the golden reads again and again, every copy with one base in `every` replaced by a random base and one
    quality in `every` by a random quality (every = 6 leaves matches of a few bytes, so that a block's symbols cover
    little text)"""
    base = np.frombuffer(golden_fastq(), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < n:
        part = base.copy()
        for old, new in ((b"ACGT", b"ACGT"), (b"I", b"FFFFFFF:,#I")):
            at = rng.integers(0, part.size, size=part.size // every)
            at = at[np.isin(part[at], np.frombuffer(old, dtype=np.uint8))]
            part[at] = np.frombuffer(new, dtype=np.uint8)[rng.integers(0, len(new), size=at.size)]
        parts.append(part)
        have += part.size
    return np.concatenate(parts)[:n].tobytes()


def raw(text: bytes, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=(), end=zlib.Z_FINISH) -> bytes:
    """raw deflate of text; flushes = ((position, mode), ...); end = the last flush (Z_FINISH ends the stream, Z_FULL_FLUSH
    and Z_SYNC_FLUSH leave it open and byte-aligned behind an empty stored block)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = [], 0
    for pos, mode in flushes:
        out.append(c.compress(text[at:pos]))
        out.append(c.flush(mode))
        at = pos
    out.append(c.compress(text[at:]))
    out.append(c.flush(end))
    return b"".join(out)


FHCRC, FEXTRA, FNAME, FCOMMENT = 2, 4, 8, 16


def member(raw_bytes: bytes, text: bytes, flags=0, extra=b"", name=b"", comment=b"", crc=None, isize=None) -> bytes:
    head = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\x00\xff")
    if flags & FEXTRA:
        head += struct.pack("<H", len(extra)) + extra
    if flags & FNAME:
        head += name + b"\0"
    if flags & FCOMMENT:
        head += comment + b"\0"
    if flags & FHCRC:
        head += struct.pack("<H", zlib.crc32(bytes(head)) & 0xFFFF)
    crc = zlib.crc32(text) if crc is None else crc
    isize = len(text) if isize is None else isize
    return bytes(head) + raw_bytes + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def zlib_text(data: bytes):
    """what zlib makes of a whole gzip file of one or more members: the text, or None when it refuses"""
    out = []
    try:
        while data:
            d = zlib.decompressobj(31)
            out.append(d.decompress(data))
            out.append(d.flush())
            if not d.eof:
                return None
            data = d.unused_data
    except zlib.error:
        return None
    return b"".join(out)


def stored_block(payload: bytes, final=0) -> bytes:
    """a stored block at a byte boundary"""
    assert len(payload) <= 0xFFFF
    return bytes([final]) + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload


def _match(w, length, dist):
    """one match of the fixed code, for the lengths and distances the cases use"""
    if length == 258:
        w.fixed(285)
    elif length == 3:
        w.fixed(257)
    else:
        assert 99 <= length <= 114
        w.fixed(279)
        w.bits(length - 99, 4)
    if dist <= 4:
        w.code(dist - 1, 5)
    else:
        assert 24577 <= dist <= 32768
        w.code(29, 5)
        w.bits(dist - 24577, 13)


def _apply(text: bytearray, length, dist):
    for _ in range(length):
        text.append(text[-dist])


def far_fixed_block(before: bytes):
    """(a final fixed block, the text it adds behind `before`): matches at distance exactly 32 768, 32 767 and 1, and a
    match of length 258 at distance 1 whose source is itself a far copy -- a marker, when the run starts late enough"""
    assert len(before) >= 32768
    w = bu.fixed_start(final=1)
    text = bytearray(before)
    for length, dist in ((258, 32768), (100, 32767), (3, 32768), (258, 1)):
        _match(w, length, dist)
        _apply(text, length, dist)
    w.fixed(ord("Q"))
    text.append(ord("Q"))
    for length, dist in ((258, 1), (3, 32768), (258, 1), (110, 32767)):
        _match(w, length, dist)
        _apply(text, length, dist)
    w.fixed(256)
    return w.done(), bytes(text[len(before):])


def _repeated_string(runs=150):
    """one marked string per kilobyte between reads: with memLevel 1 a block holds about a kilobyte, so every copy of the
    string is a match whose source is the copy of the run before: the marker chain is as deep as the chain of runs"""
    fq = fastq_with_edits(runs * 960, seed=9)
    mark = b"<the-same-forty-bytes-in-every-run-0123>"
    return b"".join(mark + fq[960 * i: 960 * (i + 1)] for i in range(runs))


@functools.lru_cache(maxsize=None)
def good_cases():
    """[(name, gzip bytes, text)]"""
    fq200 = fastq_with_edits(200_000, every=6)
    fq1m = fastq_with_edits(1_000_000, seed=6, every=6)
    fq40 = fq200[:40_000]
    out = []

    def add(name, data, text):
        assert zlib_text(data) == text, name
        out.append((name, data, text))

    add("small_blocks", member(raw(fq200, 6, 1), fq200), fq200)
    add("default_blocks", member(raw(fq1m, 6, 8), fq1m), fq1m)
    add("level1", member(raw(fq200, 1, 8), fq200), fq200)
    add("level9_mem3", member(raw(fq200, 9, 3), fq200), fq200)
    # far copies
    head = raw(fq40, 6, 1, end=zlib.Z_SYNC_FLUSH)
    block, more = far_fixed_block(fq40)
    add("far_copies", member(head + block, fq40 + more), fq40 + more)
    one = b"A" * 100_000
    add("one_byte_100k", member(raw(one, 6, 1), one), one)
    rep = _repeated_string()
    add("repeated_string", member(raw(rep, 6, 1), rep), rep)
    # block kinds
    a, b, c = fq200[:30_000], fq200[30_000:50_000], fq200[50_000:90_000]
    mixed = raw(a, 6, 1, end=zlib.Z_FULL_FLUSH) + raw(b, 6, 8, zlib.Z_FIXED, end=zlib.Z_FULL_FLUSH) + raw(c, 6, 1)
    add("fixed_between_dynamic", member(mixed, a + b + c), a + b + c)
    mixed = raw(a, 6, 1, end=zlib.Z_FULL_FLUSH) + raw(b, 0, 8, flushes=((7000, zlib.Z_SYNC_FLUSH),), end=zlib.Z_FULL_FLUSH) + raw(c, 6, 1)
    add("stored_between_dynamic", member(mixed, a + b + c), a + b + c)
    # a run longer than the span of input a counted run may read (64 finder spans: 128 KiB at "every candidate", 256 KiB at
    # COARSE): 300 KB of stored blocks between dynamic ones; the chain reaches it, so it is counted a second time
    long_b = fq1m[100_000:400_000]
    mixed = raw(a, 6, 1, end=zlib.Z_FULL_FLUSH) + raw(long_b, 0, 8, end=zlib.Z_FULL_FLUSH) + raw(c, 6, 1)
    add("long_stored_between_dynamic", member(mixed, a + long_b + c), a + long_b + c)
    add("stored_only", member(raw(fq200, 0, 8, flushes=((70_000, zlib.Z_SYNC_FLUSH),)), fq200), fq200)
    add("fixed_only", member(raw(fq40, 6, 8, zlib.Z_FIXED), fq40), fq40)
    add("empty_text", member(raw(b""), b""), b"")
    # a false candidate: a stored block whose payload is a valid dynamic block, byte-aligned
    inner = raw(b, 6, 1, end=zlib.Z_FULL_FLUSH)
    assert (inner[0] & 7) == 4 and len(inner) < 0xFFFF  # BFINAL 0, BTYPE 2
    text = a + inner + c
    add("false_candidate", member(raw(a, 6, 1, end=zlib.Z_FULL_FLUSH) + stored_block(inner) + raw(c, 6, 1), text), text)
    # members
    m1 = member(raw(a, 6, 1), a, FNAME | FEXTRA, extra=b"ab\x03\x00xyz", name=b"one.fq")
    m2 = member(raw(b, 6, 8), b, FCOMMENT | FHCRC, comment=b"a comment, with \x1f\x8b\x08 inside")
    m3 = member(raw(c, 9, 2), c, FNAME | FEXTRA | FCOMMENT | FHCRC, extra=bytes(300), name=b"three", comment=b"c")
    add("three_members", m1 + m2 + m3, a + b + c)
    add("empty_member_in_the_middle", m1 + member(raw(b""), b"") + m3, a + c)
    add("members_of_stored_and_fixed", member(raw(a, 0), a) + member(raw(b, 6, 8, zlib.Z_FIXED), b) + m3, a + b + c)
    return out


def _flip(data: bytes, bit: int) -> bytes:
    d = bytearray(data)
    d[bit >> 3] ^= 1 << (bit & 7)
    return bytes(d)


@functools.lru_cache(maxsize=None)
def bad_cases():
    """[(name, gzip bytes)]: zlib refuses every one"""
    fq = fastq_with_edits(60_000, seed=7)
    good = member(raw(fq, 6, 1), fq)
    out = []

    def add(name, data):
        assert zlib_text(data) is None, name
        out.append((name, data))

    add("cut_inside_a_block", good[:len(good) // 2])
    add("cut_inside_the_first_block", good[:40])
    add("cut_inside_the_trailer", good[:-3])
    add("cut_before_the_trailer", good[:-8])
    add("crc_off_by_one_bit", _flip(good, (len(good) - 8) * 8 + 5))
    add("isize_off_by_one", member(raw(fq, 6, 1), fq, isize=len(fq) + 1))
    add("huffman_header_bit_first_block", _flip(good, 10 * 8 + 20))
    # the same in a later block: the block behind a Z_FULL_FLUSH starts at a known byte
    first = raw(fq[:30_000], 6, 1, end=zlib.Z_FULL_FLUSH)
    late = member(first + raw(fq[30_000:], 6, 1), fq)
    assert zlib_text(late) == fq
    add("huffman_header_bit_later_block", _flip(late, (10 + len(first)) * 8 + 20))
    add("second_member_cut", good + good[:len(good) // 3])
    add("second_member_bad_crc", good + _flip(good, (len(good) - 7) * 8))
    add("no_member_behind_the_first", good + b"\x1f\x8b\x09" + bytes(20))
    # a back-reference across a member boundary: the second member opens with a match (fixed code, written by hand)
    w = bu.fixed_start(final=1)
    _match(w, 3, 1)
    w.fixed(256)
    add("match_in_front_of_its_member", good + member(w.done(), fq[-1:] * 3))
    # the same out of reach of the run that holds it: 5 000 bytes of member, then a match 32 768 back
    short = fq[:5000]
    w = bu.fixed_start(final=1)
    _match(w, 3, 32768)
    w.fixed(256)
    before = (fq + short)[-32768:]
    add("far_match_in_front_of_its_member", good + member(raw(short, 6, 1, end=zlib.Z_SYNC_FLUSH) + w.done(), short + before[:3]))
    return out
