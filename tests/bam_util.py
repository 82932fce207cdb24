"""BAM in pure Python (``struct`` + the BGZF writer of ``bgzf_util``; the project does not depend on htslib): a writer from a list of
records, a reader that walks a BAM back into records, ``fastq_pair`` -- the two FASTQ texts a BAM stands for, which are the
oracle of every BAM test through code that knows nothing of BAM -- and the constructed files the CPU and GPU tests share."""
import gzip
import struct
from collections import namedtuple

import numpy as np

import bgzf_util as bz

NIBBLES = "=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(NIBBLES)}
COMPLEMENT = {c: NIBBLES[int("{:04b}".format(i)[::-1], 2)] for i, c in enumerate(NIBBLES)}  # A=1 C=2 G=4 T=8: the bits reversed
assert [COMPLEMENT[c] for c in "ACGTNMRSWY="] == list("TGCANKYSWR=")

PAIRED, REVERSE, FIRST, SECOND, SECONDARY, SUPPLEMENTARY = 0x1, 0x10, 0x40, 0x80, 0x100, 0x800
# class of a record, as the library numbers them
C_FIRST, C_SECOND, C_DROP900, C_OTHER, C_MALFORMED = range(5)

Rec = namedtuple("Rec", "name flag seq qual aux cigar")


def rec(name, flag, seq, qual=None, aux=b"", cigar=()):
    name = name if isinstance(name, bytes) else name.encode()
    return Rec(name, flag, seq, bytes([30]) * len(seq) if qual is None else qual, aux, tuple(cigar))


def encode_record(r: Rec) -> bytes:
    packed = bytearray((len(r.seq) + 1) // 2)
    for i, c in enumerate(r.seq):
        packed[i >> 1] |= CODE[c] << (0 if i & 1 else 4)
    assert len(r.qual) == len(r.seq) and len(r.name) < 255
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(r.name) + 1, 0, 4680, len(r.cigar), r.flag, len(r.seq), -1, -1, 0)
    body += r.name + b"\0" + b"".join(struct.pack("<I", c) for c in r.cigar) + bytes(packed) + r.qual + r.aux
    return struct.pack("<I", len(body)) + body


def encode_header(text: bytes = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n", refs=()) -> bytes:
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for name, length in refs:
        out += struct.pack("<I", len(name) + 1) + name + b"\0" + struct.pack("<I", length)
    return out


def inflated(records, text=None, refs=()) -> bytes:
    head = encode_header(refs=refs) if text is None else encode_header(text, refs)
    return head + b"".join(encode_record(r) for r in records)


def write(records, text=None, refs=(), block=None, eof=True, level=6) -> bytes:
    """The BAM file (BGZF) of the records."""
    return bz.bgzf(inflated(records, text, refs), level, block=block, eof=eof)


def header_len(data: bytes) -> int:
    assert data[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<I", data, 4)[0]
    n_ref = struct.unpack_from("<I", data, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<I", data, at)[0] + 4
    return at


def walk(data: bytes, start=None):
    """The records of inflated BAM bytes by the serial walk: [(offset, Rec or None when malformed, (flag, l_seq, seq_off))],
    and how it ended: ("clean" | "cut" | "dead", offset)."""
    at = header_len(data) if start is None else start
    out = []
    while at < len(data):
        if at + 4 > len(data):
            return out, ("cut", at)
        bs = struct.unpack_from("<I", data, at)[0]
        if bs < 32:
            return out, ("dead", at)
        if at + 4 + bs > len(data):
            return out, ("cut", at)
        _, _, l_name, _, _, n_cigar, flag, l_seq, _, _, _ = struct.unpack_from("<iiBBHHHIiii", data, at + 4)
        seq_off = at + 36 + l_name + 4 * n_cigar
        if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
            out.append((at, None, (flag, 0, seq_off)))
        else:
            name = data[at + 36:at + 36 + l_name - 1] if l_name else b""
            cigar = struct.unpack_from("<%dI" % n_cigar, data, at + 36 + l_name)
            packed = data[seq_off:seq_off + (l_seq + 1) // 2]
            seq = "".join(NIBBLES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
            q = seq_off + (l_seq + 1) // 2
            out.append((at, Rec(name, flag, seq, data[q:q + l_seq], data[q + l_seq:at + 4 + bs], cigar), (flag, l_seq, seq_off)))
        at += 4 + bs
    return out, ("clean", at)


def read(bam: bytes):
    """A BAM file back into its records."""
    records, end = walk(gzip.decompress(bam))
    assert end[0] == "clean", end
    return [r for _, r, _ in records]


def classify(flag: int) -> int:
    if flag & (SECONDARY | SUPPLEMENTARY):
        return C_DROP900
    if not flag & PAIRED or bool(flag & FIRST) == bool(flag & SECOND):
        return C_OTHER
    return C_FIRST if flag & FIRST else C_SECOND


def couples(flags):
    """(couples as (index of the first, index of the second), index of the couple that is no couple or None, index of an
    odd record left over or None) of records with these flags, by the rules: drop, then two at a time."""
    part = [i for i, f in enumerate(flags) if classify(f) <= C_SECOND]
    out, bad = [], None
    for c in range(len(part) // 2):
        a, b = part[2 * c], part[2 * c + 1]
        ca, cb = classify(flags[a]), classify(flags[b])
        if ca == cb and bad is None:
            bad = c
        out.append((a, b) if ca == C_FIRST else (b, a))
    return out, bad, (part[-1] if len(part) & 1 else None)


def end_text(r: Rec) -> str:
    """The sequence of an end as ``samtools fastq`` prints it."""
    return "".join(COMPLEMENT[c] for c in reversed(r.seq)) if r.flag & REVERSE else r.seq


def fastq_pair(records):
    """The two FASTQ texts (bytes) the records stand for; ValueError when they are not collated."""
    cp, bad, odd = couples([r.flag for r in records])
    if bad is not None or odd is not None:
        raise ValueError("not collated")
    texts = []
    for which in (0, 1):
        out = []
        for c in cp:
            s = end_text(records[c[which]])
            out.append("@%s/%d\n%s\n+\n%s\n" % (records[c[which]].name.decode("latin-1").replace("\n", "_"), which + 1, s, "I" * len(s)))
        texts.append("".join(out).encode("latin-1"))
    return texts[0], texts[1]


# ---- constructed files ----------------------------------------------------------------------------------------------------
def _seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


def _patch_fake(data: bytearray, at: int, target: int):
    """a block_size at `at` whose record would end exactly at `target`"""
    assert target - (at + 4) >= 32
    data[at:at + 4] = struct.pack("<I", target - (at + 4))


def constructed():
    """[(name, inflated bytes)]: every file walked by ``walk`` for the truth.  Fake ``block_size`` fields are planted in
    quality, name and aux bytes: a chain of plausible records that starts at a wrong place must never be followed."""
    rng = np.random.default_rng(11)
    out = []

    # mixed lengths incl. l_seq 0, 1, odd, 300; reversed ends; second before first; secondary / supplementary between mates
    recs = []
    for i, n in enumerate([0, 1, 2, 3, 31, 75, 150, 151, 300, 33]):
        a = rec("r%d" % i, PAIRED | FIRST | (REVERSE if i % 3 == 0 else 0), _seq(rng, n, "ACGTN" if i % 4 == 0 else "ACGT"))
        b = rec("r%d" % i, PAIRED | SECOND | (REVERSE if i % 2 else 0), _seq(rng, max(0, n - 1), "ACGTRYM" if i == 5 else "ACGT"))
        mates = [b, a] if i % 2 else [a, b]
        recs.append(mates[0])
        if i % 3 == 1:
            recs.append(rec("r%d" % i, PAIRED | FIRST | SECONDARY, _seq(rng, 20)))
            recs.append(rec("r%d" % i, PAIRED | SECOND | SUPPLEMENTARY | REVERSE, _seq(rng, 40), cigar=(40 << 4,)))
        if i % 4 == 2:
            recs.append(rec("single%d" % i, 0, _seq(rng, 50)))           # unpaired: other
            recs.append(rec("both%d" % i, PAIRED | FIRST | SECOND, _seq(rng, 9)))  # both ends: other
        recs.append(mates[1])
    out.append(("mixed", inflated(recs)))

    # a header of 3 000 @SQ lines and their references
    refs = [(b"chr%d" % i, 1000 + i) for i in range(3000)]
    text = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out.append(("big_header", inflated(recs[:8], text, refs)))

    # a 70 KB aux array that skips whole segments, between ordinary records; fake headers inside it
    aux = bytearray(b"XYBC" + struct.pack("<I", 70000) + bytes(int(x) for x in rng.integers(0, 256, size=70000)))
    for k in range(100, 69000, 997):
        aux[k:k + 4] = struct.pack("<I", 32 + k % 300)  # plausible sizes all over it
    big = [rec("a", PAIRED | FIRST, _seq(rng, 100)), rec("a", PAIRED | SECOND, _seq(rng, 100), aux=bytes(aux)),
           rec("b", PAIRED | SECOND | REVERSE, _seq(rng, 90)), rec("b", PAIRED | FIRST, _seq(rng, 91))]
    out.append(("big_aux", inflated(big)))

    # fake headers in quality, name and aux: one whose fake chain lands exactly on a later true record start, one DEAD
    fk = []
    for i in range(12):
        qual = bytes(int(x) for x in rng.integers(0, 256, size=120))
        name = b"n%d" % i + (struct.pack("<I", 5) if i % 3 == 0 else struct.pack("<I", 40 + i))  # (5: a DEAD size)
        fk.append(rec(name, PAIRED | (FIRST if i % 2 == 0 else SECOND), _seq(rng, 120), qual=qual, aux=b"ZZZ" + struct.pack("<II", 33 + i, 7)))
    data = bytearray(inflated(fk))
    truth, end = walk(bytes(data))
    assert end[0] == "clean"
    starts = [t[0] for t in truth]
    # in the quality of record 2: a fake record that ends exactly where record 5 starts; in record 6's: one that ends at
    # record 7's start (the very next); in record 8's: a DEAD one; in record 9's: one that runs beyond the file
    for r_at, target in ((2, starts[5]), (6, starts[7])):
        q = truth[r_at][2][2] + 60 + 10  # inside the quality bytes (60 bytes of bases in front)
        _patch_fake(data, q, target)
    q8 = truth[8][2][2] + 60 + 16
    data[q8:q8 + 4] = struct.pack("<I", 31)
    q9 = truth[9][2][2] + 60 + 16
    data[q9:q9 + 4] = struct.pack("<I", 1 << 20)
    again, end = walk(bytes(data))
    assert [t[0] for t in again] == starts and end[0] == "clean"
    out.append(("fakes", bytes(data)))

    out.append(("header_only", inflated([])))
    return out


def malformed():
    """[(name, inflated bytes, what)]: what = ("dead", record) | ("malformed", record) | ("bad_couple", record of its second
    member) | ("odd", record) | ("cut", record)"""
    rng = np.random.default_rng(12)
    good = []
    for i in range(6):
        good += [rec("g%d" % i, PAIRED | FIRST, _seq(rng, 50 + i)), rec("g%d" % i, PAIRED | SECOND, _seq(rng, 48 + i))]
    out = []
    base = inflated(good)
    starts = [t[0] for t in walk(base)[0]]
    d = bytearray(base)
    d[starts[7]:starts[7] + 4] = struct.pack("<I", 31)
    out.append(("block_size_31", bytes(d), ("dead", 7)))
    d = bytearray(base)
    d[starts[4] + 20:starts[4] + 24] = struct.pack("<I", 500)  # l_seq beyond block_size
    out.append(("l_seq_beyond", bytes(d), ("malformed", 4)))
    d = bytearray(base)
    d[starts[3] + 12] = 0xFF  # l_read_name 255 beyond block_size
    d[starts[3] + 16:starts[3] + 18] = struct.pack("<H", 4000)  # ... and n_cigar
    out.append(("inner_sizes_beyond", bytes(d), ("malformed", 3)))
    two = good[:4] + [good[4], good[6]] + good[8:]
    out.append(("two_firsts", inflated(two), ("bad_couple", 5)))
    out.append(("odd_record", inflated(good[:7]), ("odd", 6)))
    out.append(("cut_record", base[:starts[9] + 40], ("cut", 9)))
    out.append(("cut_size_field", base[:starts[9] + 2], ("cut", 9)))
    return out


EOF_MARKER_HEX = "1f8b08040000000000ff0600424302001b0003000000000000000000"  # SAM spec 4.1.2: the 28 bytes
