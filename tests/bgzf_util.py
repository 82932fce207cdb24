"""A pure-Python BGZF writer, a Python restatement of the member walker, a bit writer for hand-made deflate streams, and the
corpus of members the inflate tests (CPU: the host form of the decoder, GPU: the kernel) share.  zlib is the oracle: every
hand-made stream is shown to it before it is shown to the code under test."""
import gzip
import struct
import zlib

import numpy as np

HEADER = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6)
MAX_IN = 0xFF00  # input bytes per member (0xFE00 at level 0: a stored block is longer than its text)


def wrap(raw: bytes, data: bytes, extra_before: bytes = b"", extra_after: bytes = b"", crc=None, isize=None) -> bytes:
    """A BGZF member around the raw deflate stream ``raw`` of ``data`` (other extra subfields before / after ``BC``)."""
    xlen = len(extra_before) + 6 + len(extra_after)
    bsize = 12 + xlen + len(raw) + 8
    assert bsize <= 65536, bsize
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen)
    return (head + extra_before + struct.pack("<BBHH", 66, 67, 2, bsize - 1) + extra_after + raw
            + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw) -> bytes:
    assert len(data) <= MAX_IN
    return wrap(deflate(data, level, strategy), data, **kw)


EOF_MARK = member(b"")
assert EOF_MARK.hex() == "1f8b08040000000000ff0600424302001b0003000000000000000000"


def bgzf(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, block=None, eof=True) -> bytes:
    block = block or (0xFE00 if level == 0 else MAX_IN)
    out = b"".join(member(data[i:i + block], level, strategy) for i in range(0, len(data), block))
    return out + (EOF_MARK if eof else b"")


def py_walk(buf: bytes):
    """The walker restated: ([(payload offset, payload length, ISIZE, CRC32)], offset reached, 0 end / 1 need more / 2 not BGZF)"""
    members, at = [], 0
    while at < len(buf):
        p = buf[at:]
        if p[:4] != b"\x1f\x8b\x08\x04"[:len(p[:4])]:
            return members, at, 2
        if len(p) < 12:
            return members, at, 1
        xlen = p[10] | (p[11] << 8)
        if len(p) < 12 + xlen:
            return members, at, 1
        x, bsize, sub = p[12:12 + xlen], None, 0
        while sub < xlen:
            if sub + 4 > xlen:
                return members, at, 2
            slen = x[sub + 2] | (x[sub + 3] << 8)
            if sub + 4 + slen > xlen:
                return members, at, 2
            if x[sub] == 66 and x[sub + 1] == 67 and slen == 2 and bsize is None:
                bsize = (x[sub + 4] | (x[sub + 5] << 8)) + 1
            sub += 4 + slen
        if bsize is None or bsize < 12 + xlen + 8:
            return members, at, 2
        if len(p) < bsize:
            return members, at, 1
        crc, isize = struct.unpack("<II", p[bsize - 8:bsize])
        if isize > 65536:
            return members, at, 2
        members.append((at + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        at += bsize
    return members, at, 0


def zlib_verdict(member_bytes: bytes):
    """(accepted, text) of ONE member's bytes as zlib's gzip reader sees them: accepted means a complete member, its CRC32
    and ISIZE right, and nothing behind it."""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(member_bytes)
    except zlib.error:
        return False, None
    if not d.eof or d.unused_data:
        return False, None
    return True, out


def payload_verdict(payload: bytes, isize: int, crc: int):
    """the same for (payload, ISIZE, CRC32) as the decoder is handed them: a plain gzip member around the payload"""
    return zlib_verdict(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, k):  # LSB first: header fields, extra bits
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, k):  # Huffman codes go in MSB first
        for i in range(k - 1, -1, -1):
            self.bits((v >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def fixed(self, sym):  # a literal/length symbol of the fixed code (0..287)
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def done(self):
        self.align()
        return bytes(self.out)


def fixed_start(final=1):
    w = BitWriter()
    w.bits(final, 1)
    w.bits(1, 2)
    return w


def fastq_text(n, length=150, seed=1):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        s = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=length))
        q = "".join("FFFFFFF:,#"[int(x)] for x in rng.integers(0, 10, size=length))
        recs.append("@read%d/1\n%s\n+\n%s\n" % (i, s, q))
    return "".join(recs).encode()


def random_bytes(n, seed=2):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def far_match_member():
    """32768 literals, then matches of length 258 at distance 32768 up to 64 KiB (fixed Huffman)"""
    head = bytes(int(x) for x in np.random.default_rng(7).integers(0, 144, size=32768))
    w = fixed_start()
    for c in head:
        w.fixed(c)
    out = bytearray(head)
    while len(out) + 258 <= 65536:
        w.fixed(285)
        w.code(29, 5)
        w.bits(32768 - 24577, 13)
        out += out[-32768:-32768 + 258]
    w.fixed(256)
    return w.done(), bytes(out)


def run_member():
    """"A" + (length 258, distance 1) = 259 x "A" """
    w = fixed_start()
    w.fixed(65)
    w.fixed(285)
    w.code(0, 5)
    w.fixed(256)
    return w.done(), b"A" * 259


def good_corpus():
    """[(name, payload, text)]: every payload a complete raw deflate stream of text that zlib accepts"""
    out = []
    fq = fastq_text(400)
    rnd = random_bytes(MAX_IN)
    for level in (0, 1, 6, 9):
        cap = 0xFE00 if level == 0 else MAX_IN
        out.append(("fastq_l%d" % level, deflate(fq[:cap], level), fq[:cap]))
        out.append(("random_l%d" % level, deflate(rnd[:cap], level), rnd[:cap]))
    for name, strat in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        out.append(("fastq_" + name, deflate(fq[:MAX_IN], 6, strat), fq[:MAX_IN]))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = co.compress(fq[:20000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(fq[20000:40000]) + co.flush(zlib.Z_FULL_FLUSH)
    raw += co.compress(fq[40000:60000]) + co.flush()
    out.append(("flushes", raw, fq[:60000]))
    for n in (0, 1, 2, 258, 259, MAX_IN):
        out.append(("isize_%d" % n, deflate(fq[:n]), fq[:n]))
    out.append(("zeros_65536", deflate(bytes(65536)), bytes(65536)))
    # incompressible bytes up to the largest payload BSIZE allows (65536 - 18 - 8 bytes of stored blocks)
    big = random_bytes(65536 - 26 - 5, seed=3)
    raw = b"\x01" + struct.pack("<HH", len(big), len(big) ^ 0xFFFF) + big  # one final stored block
    assert len(raw) == 65536 - 26, len(raw)
    out.append(("largest_payload", raw, big))
    out.append(("far_matches",) + far_match_member())
    out.append(("run_of_a",) + run_member())
    for name, raw, text in out:
        assert zlib.decompress(raw, -15) == text, name
        assert len(text) <= 65536 and len(raw) <= 65536 - 26, name
    return out


def _dynamic_header(w, cl_lens, hlit=257, hdist=1):
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(19 - 4, 4)
    for s in order:
        w.bits(cl_lens.get(s, 0), 3)


def bad_corpus():
    """[(name, payload, isize, crc)]: every one rejected by zlib (checked here)"""
    out = []
    w = fixed_start()
    for c in b"ACGT":
        w.fixed(c)
    w.fixed(257)
    w.code(4, 5)
    w.bits(0, 1)  # length 3, distance 5 with 4 bytes written
    w.fixed(256)
    out.append(("too_far_back", w.done(), 7, 0))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    out.append(("btype3", w.done() + b"\0\0\0", 0, 0))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    out.append(("stored_len_nlen", w.done() + struct.pack("<HH", 4, 0xFFFB ^ 1) + b"ACGT", 4, zlib.crc32(b"ACGT")))
    # dynamic: code-length code over-subscribed (three 1-bit codes) and incomplete (one 2-bit code)
    for name, cl in (("cl_oversubscribed", {0: 1, 1: 1, 2: 1}), ("cl_incomplete", {0: 2})):
        w = BitWriter()
        w.bits(1, 1)
        w.bits(2, 2)
        _dynamic_header(w, cl)
        out.append((name, w.done() + b"\0" * 8, 0, 0))
    # dynamic: literal/length lengths over-subscribed (257 codes of 1 bit) and incomplete (only 256 and one more, 2 bits each)
    for name in ("litlen_oversubscribed", "litlen_incomplete"):
        w = BitWriter()
        w.bits(1, 1)
        w.bits(2, 2)
        _dynamic_header(w, {0: 1, 1: 2, 2: 2})  # code-length code: 0 -> '0', 1 -> '10', 2 -> '11'
        emit = {0: (0, 1), 1: (2, 2), 2: (3, 2)}
        lens = [1] * 257 + [1] if name == "litlen_oversubscribed" else [2] + [0] * 255 + [2] + [1]
        for l in lens:
            w.code(*emit[l])
        out.append((name, w.done() + b"\0" * 8, 0, 0))
    for sym in (286, 287):
        w = fixed_start()
        w.fixed(65)
        w.fixed(sym)
        w.fixed(256)
        out.append(("fixed_symbol_%d" % sym, w.done(), 1, zlib.crc32(b"A")))
    for dc in (30, 31):
        w = fixed_start()
        for c in b"ACGT":
            w.fixed(c)
        w.fixed(257)
        w.code(dc, 5)
        w.fixed(256)
        out.append(("fixed_distance_%d" % dc, w.done(), 7, 0))
    fq = fastq_text(100)
    raw = deflate(fq)
    out.append(("cut_by_one", raw[:-1], len(fq), zlib.crc32(fq)))
    out.append(("cut_by_half", raw[:len(raw) // 2], len(fq), zlib.crc32(fq)))
    out.append(("wrong_crc", raw, len(fq), zlib.crc32(fq) ^ 1))
    out.append(("wrong_isize", raw, len(fq) + 1, zlib.crc32(fq)))
    out.append(("isize_too_small", raw, len(fq) - 1, zlib.crc32(fq)))
    for name, raw, isize, crc in out:
        assert not payload_verdict(raw, isize, crc)[0], name
    return out


def flip_members():
    """a ~1.3 KB dynamic and a ~1.7 KB fixed member of 12 FASTQ records"""
    txt = fastq_text(12)
    return [("dynamic", member(txt), txt), ("fixed", member(txt, 6, zlib.Z_FIXED), txt)]


assert gzip.decompress(bgzf(b"ACGT" * 10)) == b"ACGT" * 10
