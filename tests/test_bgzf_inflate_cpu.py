"""BGZF without a device: the member walker (vs_bgzf_walk) against a Python restatement, the decoder the inflate kernel runs
in its host form (vs_inflate_host) against zlib -- good members, rejected ones, every single-bit flip of two members -- and
which inputs take the streamed ingest."""
import gzip
import struct
import zlib

import pytest

import bgzf_util as bz


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def _same_walk(host, buf):
    got, want = host.bgzf_walk(buf), bz.py_walk(buf)
    assert got == want, (got[1:], want[1:], len(buf))
    return got


def test_walker_lists_the_members_of_written_files(host):
    text = bz.fastq_text(900)
    for block in (100, 4096, bz.MAX_IN):
        for eof in (True, False):
            buf = bz.bgzf(text, block=block, eof=eof)
            members, at, state = _same_walk(host, buf)
            assert (at, state) == (len(buf), 0)
            assert len(members) == -(-len(text) // block) + (1 if eof else 0)
            assert sum(m[2] for m in members) == len(text)
            assert b"".join(zlib.decompress(buf[o:o + n], -15) for o, n, _, _ in members) == text
            assert all(zlib.crc32(zlib.decompress(buf[o:o + n], -15)) == c for o, n, _, c in members)
    assert _same_walk(host, b"") == ([], 0, 0)


def test_walker_other_subfields_and_end_markers(host):
    a, b = bz.fastq_text(30, seed=3), bz.fastq_text(40, seed=4)
    before = struct.pack("<BBH", 1, 2, 5) + b"hello"
    after = struct.pack("<BBH", 9, 9, 0)
    buf = bz.member(a, extra_before=before) + bz.member(b, extra_after=after) + bz.member(a, extra_before=before, extra_after=after)
    members, at, state = _same_walk(host, buf)
    assert (len(members), at, state) == (3, len(buf), 0)
    assert [m[2] for m in members] == [len(a), len(b), len(a)]
    assert gzip.decompress(buf) == a + b + a
    # the end marker in the middle (two files concatenated), at the end, absent
    for buf, n in ((bz.bgzf(a) + bz.bgzf(b), 4), (bz.bgzf(a), 2), (bz.bgzf(a, eof=False), 1)):
        members, at, state = _same_walk(host, buf)
        assert (len(members), at, state) == (n, len(buf), 0)
    members, _, _ = _same_walk(host, bz.bgzf(a) + bz.bgzf(b))
    assert members[1][1:3] == (2, 0)  # the marker: a two-byte payload, ISIZE 0


def test_walker_needs_more_bytes_at_every_cut(host):
    buf = bz.bgzf(bz.fastq_text(8), block=700)
    first_two = bz.py_walk(buf)[0][:2]
    end1 = first_two[0][0] + first_two[0][1] + 8
    end2 = first_two[1][0] + first_two[1][1] + 8
    for cut in range(1, end2):
        if cut == end1:
            continue
        members, at, state = _same_walk(host, buf[:cut])
        assert state == 1 and at == (0 if cut < end1 else end1) and len(members) == (0 if cut < end1 else 1), cut
    assert _same_walk(host, buf[:end1]) == ([first_two[0]], end1, 0)


def test_walker_says_what_is_not_bgzf(host):
    a = bz.fastq_text(30)
    two = b"".join(bz.member(a[i:i + 3000]) for i in (0, 3000))
    plain = gzip.compress(a)
    assert _same_walk(host, plain + two) == ([], 0, 2)
    members, at, state = _same_walk(host, two + plain + two)
    assert (len(members), at, state) == (2, len(two), 2)
    members, at, state = _same_walk(host, two + b"garbage")
    assert (len(members), at, state) == (2, len(two), 2)
    m = bytearray(bz.member(a))
    big = bytes(m[:-4]) + struct.pack("<I", 65537)
    assert _same_walk(host, two + big)[1:] == (len(two), 2)
    assert _same_walk(host, bytes(m[:-4]) + struct.pack("<I", 65536))[2] == 0  # (65536 itself is a member's largest ISIZE)
    for name, bad in (("flg", m[:3] + b"\x0c" + m[4:]), ("cm", m[:2] + b"\x07" + m[3:]), ("no_bc", m[:12] + b"XY" + m[14:]),
                      ("bsize_small", m[:16] + struct.pack("<H", 24) + m[18:])):
        assert _same_walk(host, bytes(bad))[1:] == (0, 2), name


def _check_good(run, name, raw, text):
    status, out, guard = run(raw, len(text), zlib.crc32(text))
    assert guard, name
    assert status == 0 and out == text, (name, status)


def test_host_decoder_equals_zlib_on_the_corpus(host):
    for name, raw, text in bz.good_corpus():
        _check_good(host.inflate_host, name, raw, text)


def test_host_decoder_rejects_what_zlib_rejects(host):
    seen = {}
    for name, raw, isize, crc in bz.bad_corpus():
        status, _, guard = host.inflate_host(raw, isize, crc)
        assert guard, name
        assert status != 0, name
        seen[name] = status
    # the status word names the first thing wrong
    assert seen["too_far_back"] == 7 and seen["btype3"] == 1 and seen["stored_len_nlen"] == 2
    assert seen["cl_oversubscribed"] == 3 and seen["cl_incomplete"] == 4
    assert seen["litlen_oversubscribed"] == 3 and seen["litlen_incomplete"] == 4
    assert seen["fixed_symbol_286"] == seen["fixed_symbol_287"] == 5
    assert seen["fixed_distance_30"] == seen["fixed_distance_31"] == 6
    assert seen["cut_by_one"] == seen["cut_by_half"] == 8
    assert seen["wrong_crc"] == 11 and seen["wrong_isize"] == 10 and seen["isize_too_small"] == 9


@pytest.mark.parametrize("which", [0, 1], ids=["dynamic", "fixed"])
def test_host_decoder_verdict_equals_zlib_for_every_single_bit_flip(host, which):
    """Payload and trailer flips: the decoder's verdict is zlib's on the same bytes.  Header flips, through the walker and the
    decoder: rejected, or the same text -- never other text.  The guard bytes stay untouched throughout."""
    name, good, text = bz.flip_members()[which]
    (off, n, isize, crc), = bz.py_walk(good)[0]
    assert off == 18 and 1000 < len(good) < 2200
    counts = {"rejected": 0, "same": 0}
    for bit in range(len(good) * 8):
        blk = bytearray(good)
        blk[bit >> 3] ^= 1 << (bit & 7)
        blk = bytes(blk)
        if bit < 18 * 8:
            members, at, state = host.bgzf_walk(blk)
            if state != 0 or at != len(blk) or len(members) != 1:
                counts["rejected"] += 1
                continue
            o, ln, isz, c = members[0]
            status, out, guard = host.inflate_host(blk[o:o + ln], isz, c)
            assert guard, bit
            assert status != 0 or out == text, bit
            counts["rejected" if status else "same"] += 1
            continue
        pay, (c, isz) = blk[off:off + n], struct.unpack("<II", blk[-8:])
        if isz > 65536:  # (the walker never hands such a member on; zlib rejects it too)
            assert not bz.payload_verdict(pay, isz, c)[0]
            counts["rejected"] += 1
            continue
        want_ok, want_text = bz.payload_verdict(pay, isz, c)
        status, out, guard = host.inflate_host(pay, isz, c)
        assert guard, bit
        assert (status == 0) == want_ok, (bit, status, want_ok)
        if want_ok:
            assert out == want_text == text, bit
        counts["same" if want_ok else "rejected"] += 1
    assert counts["rejected"] > 0.95 * len(good) * 8 and counts["same"] > 0, counts


def test_use_stream_takes_regular_bgzf_files(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference

    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    text = bz.fastq_text(20)
    for name, data in (("a.fq.gz", bz.bgzf(text)), ("b.fq.gz", bz.bgzf(text, block=500, eof=False)), ("p.fq", text),
                       ("g1.fq.gz", gzip.compress(text)), ("g2.fq.gz", gzip.compress(text))):
        (tmp_path / name).write_bytes(data)
    p = {n: str(tmp_path / n) for n in ("a.fq.gz", "b.fq.gz", "p.fq", "g1.fq.gz", "g2.fq.gz")}
    assert pe_inference.use_stream(p["a.fq.gz"], p["b.fq.gz"])
    assert pe_inference.use_stream(p["a.fq.gz"], p["p.fq"]) and pe_inference.use_stream(p["p.fq"], p["b.fq.gz"])
    assert not pe_inference.use_stream(p["g1.fq.gz"], p["g2.fq.gz"])
    assert not pe_inference.use_stream(p["p.fq"], p["g1.fq.gz"])
    assert not pe_inference.use_stream(p["p.fq"], str(tmp_path / "missing.fq"))
    monkeypatch.setenv("VS_FASTQ_STREAM", "0")
    assert not pe_inference.use_stream(p["a.fq.gz"], p["b.fq.gz"])


def test_bgzf_entries_declared_and_bound():
    import os
    import re

    from conftest import ROOT
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_bgzf_walk", "vs_inflate_host", "vs_inflate_bgzf", "vs_fastq_stream_inflate_info"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
