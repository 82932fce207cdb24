"""The corpus of texts the BGZF encoder tests share (CPU: the one-lane host twin ``vs_deflate_host``, GPU: the kernel through
``vs_deflate_bgzf``), thin callers of those two entries, and the checks every member must pass.  zlib is the oracle: a
member is what ``zlib_verdict`` accepts and turns back into the text; nothing here compares the encoder with itself."""
import ctypes as C
import functools
import os
import struct
import zlib

import numpy as np

import bgzf_util as bu
import sparse_info_util as su
from conftest import GOLDEN

MAX_TEXT = 0xFF00
STORED, FIXED, DYNAMIC = 0, 1, 2
EXTRA = 31  # header 18 + stored block 5 + trailer 8: no member is larger than its text + 31


def golden_dense(case="hiv_like_k55", name="pe_info") -> bytes:
    with open(os.path.join(GOLDEN, "pe", case, name), "rb") as fh:
        return fh.read()


def golden_sparse(case="hiv_like_k55", name="pe_info") -> bytes:
    return su.filtered(golden_dense(case, name).decode()).encode()


def _far_copy(distance, filler):
    """300 random bytes, filler, and the same 300 bytes again, the copy starting `distance` behind the original"""
    head = bu.random_bytes(300, seed=21)
    fill = bu.random_bytes(distance - 300, seed=22) if filler == "random" else bytes(distance - 300)
    return head + fill + head


@functools.lru_cache(maxsize=None)
def members():
    """[(name, text)]: one member each"""
    fq = bu.fastq_text(400)
    dense = golden_dense()
    assert len(dense) == 27722
    out = [("len_%d" % n, fq[:n]) for n in range(5)]
    out += [
        ("a_259", b"A" * 259),  # distance 1, length 258 and a literal: the copy that overlaps itself
        ("a_full", b"A" * MAX_TEXT),
        ("zeros_full", bytes(MAX_TEXT)),
        ("ab_20000", b"AB" * 20000),
        ("all_bytes_twice", bytes(range(256)) * 2),
        ("random_full", bu.random_bytes(MAX_TEXT)),
        ("far_32768_random", _far_copy(32768, "random")),
        ("far_32769_random", _far_copy(32769, "random")),
        # the same with a filler that leaves the hash table's entries of the first 300 bytes alone: the copy IS a candidate
        ("far_32768_zeros", _far_copy(32768, "zeros")),
        ("far_32769_zeros", _far_copy(32769, "zeros")),
        ("flush_258", dense[:4000] + dense[100:358]),   # the last 258 bytes repeat earlier text: a match ends with the member
        ("flush_3", bu.random_bytes(200, seed=23) + bu.random_bytes(200, seed=23)[50:53]),
        ("fastq", fq[:MAX_TEXT]),
        ("dense_pe_info", dense),
        ("sparse_pe_info", golden_sparse()),
    ]
    assert all(len(t) <= MAX_TEXT for _, t in out)
    return out


def multi_text() -> bytes:
    """3 * 0xFF00 + 17 bytes of the dense golden text repeated: 4 members and the EOF member"""
    dense = golden_dense()
    n = 3 * MAX_TEXT + 17
    return (dense * (n // len(dense) + 1))[:n]


def deflate_host(text: bytes, cap=None):
    """``vs_deflate_host`` -> (return code, member bytes, kind); the output buffer is exactly ``cap`` bytes (default n + 31)"""
    from vstrains_amd import _native as nat

    cap = len(text) + EXTRA if cap is None else cap
    out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    src = np.frombuffer(text or b"\0", dtype=np.uint8)
    size, kind = C.c_uint32(0), C.c_uint32(9)
    rc = nat.lib().vs_deflate_host(src.ctypes.data, len(text), out.ctypes.data, cap, C.byref(size), C.byref(kind))
    return rc, out[:size.value].tobytes(), kind.value


@functools.lru_cache(maxsize=None)
def host_member(name):
    """the twin's member of a corpus text, made once for all tests"""
    text = dict(members())[name]
    rc, member, kind = deflate_host(text)
    assert rc == 0, name
    return member, kind


def deflate_device(ctx, text: bytes, guard=64):
    """``vs_deflate_bgzf`` -> (return code, file bytes, info[5])"""
    from vstrains_amd import _native as nat

    nm = (len(text) + MAX_TEXT - 1) // MAX_TEXT
    cap = nm * (MAX_TEXT + EXTRA) + 28
    out = np.zeros(cap, dtype=np.uint8)
    src = np.frombuffer(text or b"\0", dtype=np.uint8)
    info = (C.c_uint64 * 5)()
    rc = nat.lib().vs_deflate_bgzf(ctx._h, src.ctypes.data, len(text), out.ctypes.data, cap, guard, info)
    info = [int(x) for x in info]
    return rc, out[:info[1]].tobytes(), info


def inflate_host(payload: bytes, isize: int, crc: int):
    """the project's own decoder, one lane -> (status, text)"""
    from vstrains_amd import _native as nat

    src = np.frombuffer(payload or b"\0", dtype=np.uint8)
    out = np.zeros(max(isize, 1), dtype=np.uint8)
    status = C.c_uint32(99)
    assert nat.lib().vs_inflate_host(src.ctypes.data, len(payload), out.ctypes.data, isize, crc, C.byref(status)) == 0
    return status.value, out[:isize].tobytes()


def check_member(member: bytes, text: bytes):
    """one whole BGZF member of ``text``: the walker's, zlib's and the project's decoder's verdict, the size bound, the trailer"""
    found, at, verdict = bu.py_walk(member)
    assert verdict == 0 and at == len(member) and len(found) == 1
    off, length, isize, crc = found[0]
    assert off == 18 and member[:16] == bu.HEADER + b"BC\x02\x00"
    assert struct.unpack("<H", member[16:18])[0] == len(member) - 1
    ok, back = bu.zlib_verdict(member)
    assert ok and back == text
    assert len(member) <= len(text) + EXTRA and len(member) <= 65536
    assert isize == len(text) and crc == zlib.crc32(text)
    status, own = inflate_host(member[off:off + length], isize, crc)
    assert status == 0 and own == text


def block_type(member: bytes) -> int:
    """BTYPE of the member's first (and only) block; BFINAL must be set"""
    assert member[18] & 1
    return (member[18] >> 1) & 3


# ---- the pe_info / st_info writer ------------------------------------------------------------------------------------------
INFO_KEYS = ("lines", "bytes", "blocks", "cells_read", "members", "file_bytes")


def write_bgzf_host(path, ids, counts, wide, tile_map, rank, upper, dense):
    """``vs_write_info_bgzf_host`` on numpy arrays -> (return code, info[6])"""
    from vstrains_amd import _native as nat

    blob, off = su.encode_ids(ids)
    info = (C.c_uint64 * 6)()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    rc = nat.lib().vs_write_info_bgzf_host(None, str(path).encode(), blob.ctypes.data, off.ctypes.data, len(ids), ptr(counts), ptr(wide),
                                           ptr(tile_map), ptr(rank), upper, dense, info)
    return rc, [int(x) for x in info]


def write_bgzf_device(ctx, path, ids, counts, wide, tile_map, rank, upper, dense):
    """``vs_write_info_bgzf`` on torch tensors that live on the device (``rank`` a numpy array) -> (return code, info[6])"""
    from vstrains_amd import _native as nat

    blob, off = su.encode_ids(ids)
    info = (C.c_uint64 * 6)()
    ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = nat.lib().vs_write_info_bgzf(ctx._h, str(path).encode(), blob.ctypes.data, off.ctypes.data, len(ids), ptr(counts), ptr(wide),
                                      ptr(tile_map), None if rank is None else rank.ctypes.data, upper, dense, info)
    return rc, [int(x) for x in info]


def check_file(path, text: bytes, info=None):
    """A whole BGZF file of ``text``: it walks as BGZF to its last byte for the Python walker and for the library's, ends in
    the EOF member, no member holds more than 0xFF00 bytes of text, zlib's gzip reader gives the text back, and the
    member count and file size are the ones the writer reported.  Returns the file's bytes."""
    import gzip

    from vstrains_amd import _native as nat

    with open(path, "rb") as fh:
        data = fh.read()
    found, at, verdict = bu.py_walk(data)
    assert verdict == 0 and at == len(data)
    assert data.endswith(bu.EOF_MARK) and found[-1][2] == 0
    assert all(0 < m[2] <= MAX_TEXT for m in found[:-1])
    assert sum(m[2] for m in found) == len(text)
    walk = (C.c_uint64 * 4)()
    assert nat.lib().vs_bgzf_walk_file(str(path).encode(), None, 0, walk) == 0
    assert [int(x) for x in walk] == [len(found), len(data), 0, len(data)]
    assert gzip.decompress(data) == text
    if info is not None:
        assert info[4] == len(found) - 1 and info[5] == len(data)
        assert info[0] == text.count(b"\n") and info[1] == len(text)
    return data


def golden_matrices(d, ids):
    """the committed pe_info / st_info of a golden case as uint32 matrices in the caller's numbering (st_info: upper triangle)"""
    index = {s: i for i, s in enumerate(ids)}
    mats = []
    for f in ("pe_info", "st_info"):
        m = np.zeros((len(ids), len(ids)), dtype=np.uint32)
        with open(os.path.join(d, f), "r", newline="") as fh:
            for line in fh:
                u, v, c = line[:-1].split(":")
                m[index[u], index[v]] = int(c)
        mats.append(m)
    return mats
