"""What the GPU suites of the five streamed ingests check alike since one builder cuts every block (build_block of
vs_reads.hip): the refusal of an end over the length limit, and the edges of the common ends kernel.  Inputs and checks
only; the tests are in the stream's own files."""
import ctypes as C
import struct

import numpy as np
import pytest

LONG = 1 << 24  # one more than a read end's length field holds
ENDS_TPB = 256  # the workgroup of k_block_ends: a block of n pairs has 2n + 1 threads
# 1; 2n + 1 one below, equal to and one above the workgroup, plus one; everything in one block
BLOCK_SIZES = (1, ENDS_TPB // 2 - 1, ENDS_TPB // 2, ENDS_TPB // 2 + 1, 1 << 20)


def edge_pairs(n_pairs=300, other="X", seed=5):
    """(fwd, rve): reads of 0..70 bases, among the first few pairs one with an N, one with a byte outside ACGTN (``other``),
    one of length 0 and two whose length is a multiple of 16 -- and the same kinds again around the workgroup edge"""
    rng = np.random.default_rng(seed)
    fwd, rve = [], []
    for p in range(n_pairs):
        a, b = ("".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(1, 71)))) for _ in range(2))
        k = p % 127
        if k == 1:
            a = a[:3] + "N" + a[3:]
        elif k == 2:
            b = b[:5] + other + b[5:]
        elif k == 3:
            b = ""
        elif k == 4:
            a, b = (a * 16)[:16], (b * 32)[:32]
        elif k == 5:
            a = ""
        fwd.append(a)
        rve.append(b)
    return fwd, rve


def fastq(reads, names) -> bytes:
    return b"".join(b"@" + n + b"\n" + r.encode() + b"\n+\n" + b"I" * len(r) + b"\n" for n, r in zip(names, reads))


def long_record(name: bytes) -> bytes:
    return b"@" + name + b"\n" + b"A" * LONG + b"\n+\n" + b"I" * LONG + b"\n"


def long_bam_record(name: bytes, flag: int) -> bytes:
    """an encoded BAM record with l_seq = LONG (every base an A), without a per-base loop"""
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, 0, flag, LONG, -1, -1, 0)
    body += name + b"\0" + b"\x11" * (LONG // 2) + bytes([30]) * LONG
    return struct.pack("<I", len(body)) + body


def refused(stream, exc, message):
    """Draining ``stream`` raises ``exc`` with ``message``; the native entry asked again gives VS_E_RANGE and exactly the
    message: the stream stays failed."""
    from vstrains_amd import _native as nat

    with pytest.raises(exc) as err:
        for block in stream:
            block.free()
    assert message in str(err.value)
    if exc is nat.NativeError:
        assert err.value.code == nat.VS_E_RANGE
    h, n = C.c_void_p(), C.c_uint64(0)
    rc = getattr(nat.lib(), stream._entries[1])(stream._ctx._h, stream._h, 1, C.byref(h), C.byref(n))
    assert rc == nat.VS_E_RANGE and not h.value
    assert nat.lib().vs_last_error(stream._ctx._h).decode() == message
    stream.close()


def drained(stream):
    """(bases, lengths, flags) of the blocks of ``stream`` concatenated, and ``unpaired`` of every block"""
    parts, unpaired = [], []
    for block in stream:
        parts.append(block.unpack())
        unpaired.append(block.unpaired)
        block.free()
    stream.close()
    return [np.concatenate([p[i] for p in parts]) for i in range(3)], unpaired


def same_at_every_block_size(open_stream, want_block, unpaired):
    """``open_stream(block size)`` drained at BLOCK_SIZES gives what ``want_block`` (the host packer's) holds"""
    want = want_block.unpack()
    for size in BLOCK_SIZES:
        got, un = drained(open_stream(size))
        assert un and all(u == unpaired for u in un), size
        if size == BLOCK_SIZES[-1]:
            assert len(un) == 1
        elif size > 1:
            assert len(un) > 2  # (more than one workgroup's worth, and a last block that is not full)
        for g, w, what in zip(got, want, ("bases", "lengths", "flags")):
            assert np.array_equal(g, w), (size, what)
