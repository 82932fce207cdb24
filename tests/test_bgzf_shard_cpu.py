"""The member-sharded open of a BGZF pair, the parts that need no device: the plan (vs_bgzf_shard_plan) against a brute-force
model that concatenates the members' texts and cuts lines, the bound on how often a member is opened, the host form of the
counting kernel (vs_inflate_count_host: the decoder text of k_inflate_count with one lane) against zlib, and the header hop
over a file (vs_bgzf_walk_file) against the Python walker."""
import zlib

import numpy as np
import pytest

import bgzf_util as bz
from vstrains_amd import pe as host
from vstrains_amd.dist import shard_range


def _fastq(n, length=9, tag="r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag.encode(), i, b"ACGT" * length, b"I" * (4 * length)) for i in range(n))


def _cut(text, block):
    return [text[i:i + block] for i in range(0, len(text), block)]


def _with_empties(members):
    out = []
    for i, m in enumerate(members):
        out.append(m)
        if i % 3 == 1:
            out.append(b"")
    return out + [b""]  # (the end marker)


def _cases():
    """name -> (member texts of the forward file, of the reverse file)"""
    a10, b10 = _fastq(10, tag="f"), _fastq(10, length=7, tag="r")
    rec = len(_fastq(1, tag="f"))  # (one-digit record numbers: every record has this size)
    return {
        "one_member_each": ([a10], [b10]),
        "empty_members_and_end_marker": (_with_empties(_cut(a10, 100)), _with_empties(_cut(b10, 61))),
        "members_without_a_newline": (_cut(a10, 3), _cut(b10, 5)),
        "a_record_in_four_members": ([b"@f0\n", b"ACGT\n", b"+\n", b"IIII\n", b"@f1\nAC", b"GT\n+\nIIII\n"] + _cut(_fastq(4), 50),
                                     [b"@r0\nAC", b"", b"GT\n+", b"\nIIII\n@r1\nACGT\n+\nIIII\n"] + _cut(_fastq(4), 33)),
        "boundaries_on_member_boundaries": (_cut(a10, rec), _cut(a10, 2 * rec)),
        "no_final_newline": (_cut(a10[:-1], 70), _cut(b10[:-1], 300)),
        "no_final_newline_in_a_member_of_its_own": (_cut(a10[:-1], 70) + [b""], [b10[:-5], b10[-5:-1], b""]),
        "unequal_record_counts": (_cut(_fastq(7), 64), _cut(_fastq(10), 90)),
        "unequal_and_the_longer_ends_open": (_cut(_fastq(11)[:-1], 64), _cut(_fastq(5), 90)),
        "three_lines_too_many": (_cut(a10 + b"@x\nAC\n+\n", 41), _cut(b10 + b"@y", 41)),
        "three_records": (_cut(_fastq(3), 25), _cut(_fastq(3), 1000)),
        "no_record": ([b"@f0\nAC", b"GT\n"], [b""]),
        "only_end_markers": ([b""], [b"", b""]),
    }


class Model:
    """One file by brute force: the members' texts concatenated, lines cut at b'\\n'."""

    def __init__(self, members):
        self.members = members
        self.text = b"".join(members)
        self.starts = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        self.newlines = [i for i, c in enumerate(self.text) if c == 10]
        self.open_end = bool(self.text) and self.text[-1] != 10
        self.lines = len(self.newlines) + (1 if self.open_end else 0)
        self.counts = np.asarray([m.count(b"\n") for m in members], dtype=np.uint32)

    def member_of(self, byte):
        return int(np.searchsorted(self.starts, byte, side="right")) - 1

    def plan(self, first, last):
        if last <= first:
            return 0, 0, 0
        a, skip = 0, 0
        if first:
            p = self.newlines[4 * first - 1]  # the newline in front of line 4 * first
            a = self.member_of(p)
            skip = self.text[self.starts[a]:p + 1].count(b"\n")
        e = self.member_of(self.newlines[4 * last - 1]) + 1 if 4 * last <= len(self.newlines) else len(self.members)
        return a, skip, e

    def records(self, first, last):
        if last <= first:
            return b""
        lo = self.newlines[4 * first - 1] + 1 if first else 0
        hi = self.newlines[4 * last - 1] + 1 if 4 * last <= len(self.newlines) else len(self.text)
        return self.text[lo:hi]


@pytest.mark.parametrize("name", sorted(_cases()))
def test_plan_equals_the_brute_force_model_and_opens_few_members(name):
    files = [Model(m) for m in _cases()[name]]
    total = min(f.lines // 4 for f in files)
    for world in range(1, 7):
        ranges = [shard_range(total, r, world) for r in range(world)]
        assert ranges[0][0] == 0 and ranges[-1][1] == total
        assert all(ranges[r][1] == ranges[r + 1][0] for r in range(world - 1))  # the ranges tile the pairs
        for f in files:
            n_members = len(f.members)
            opened = 0
            for first, last in ranges:
                got = host.bgzf_shard_plan(f.counts, f.open_end, first, last)
                assert got == f.plan(first, last), (name, world, first, last)
                a, skip, e = got
                # what the stream does with it: the members' text, `skip` lines dropped, starts with exactly these records
                text = b"".join(f.members[a:e])
                for _ in range(skip):
                    text = text[text.index(b"\n") + 1:]
                want = f.records(first, last)
                assert text.startswith(want) and want.count(b"\n") + (0 if want.endswith(b"\n") or not want else 1) == 4 * (last - first)
                if last > first:
                    assert a < e <= n_members and (skip >= 1) == (first > 0)
                    if 4 * last <= len(f.newlines):
                        assert f.counts[a:e].sum() >= skip + 4 * (last - first) > f.counts[a:e - 1].sum()  # (no member too many)
                opened += e - a
            # pass 2: neighbours share at most the one member that holds their boundary
            assert opened <= n_members + world - 1, (name, world, opened)
            # pass 1: every member on exactly one rank
            shares = [((n_members * r) // world, (n_members * (r + 1)) // world) for r in range(world)]
            assert sorted(m for lo, hi in shares for m in range(lo, hi)) == list(range(n_members))


def test_plan_refuses_ranges_beyond_the_lines():
    from vstrains_amd import _native as nat

    counts = np.asarray([3, 0, 4, 1], dtype=np.uint32)  # 8 newlines: two records
    assert host.bgzf_shard_plan(counts, False, 0, 2) == (0, 0, 4)
    assert host.bgzf_shard_plan(counts[:3], True, 1, 2) == (2, 1, 3)  # 7 newlines and an open last line
    with pytest.raises(nat.NativeError):
        host.bgzf_shard_plan(counts[:3], False, 1, 2)
    with pytest.raises(nat.NativeError):
        host.bgzf_shard_plan(counts, True, 0, 3)
    with pytest.raises(nat.NativeError):
        host.bgzf_shard_plan(counts, False, 2, 1)
    assert host.bgzf_shard_plan(np.zeros(0, dtype=np.uint32), False, 0, 0) == (0, 0, 0)


def test_host_count_equals_zlib_on_the_good_corpus():
    texts = [("crlf", b"@r\r\nACGT\r\n+\r\nIIII\r\n"), ("lone_cr", b"A\rC\n"), ("high_byte", "@r\u00e9\nAC\n".encode()),
             ("no_newline", b"ACGT"), ("newline_only", b"\n"), ("newlines_65536", b"\n" * 65536)]
    extra = [(n, bz.deflate(t), t) for n, t in texts]
    for name, raw, text in bz.good_corpus() + extra:
        want = zlib.decompress(raw, -15)
        assert want == text
        status, nl, flags, last = host.inflate_count_host(raw, len(text), zlib.crc32(text))
        assert status == 0, (name, status)
        assert nl == want.count(b"\n"), name
        assert flags == (1 if b"\r" in want else 0) | (2 if any(c >= 0x80 for c in want) else 0), name
        assert last == (want[-1] if want else 0), name
        assert host.inflate_host(raw, len(text), zlib.crc32(text))[0] == 0


def test_host_count_reports_the_status_of_the_host_inflate_on_the_bad_corpus():
    for name, raw, isize, crc in bz.bad_corpus():
        status, out, guard = host.inflate_host(raw, isize, crc)
        got = host.inflate_count_host(raw, isize, crc)
        assert status != 0 and guard, name
        assert got == (status, 0, 0, 0), (name, got, status)


def test_file_walk_hops_over_headers_like_the_python_walker(tmp_path):
    text = bz.fastq_text(300)
    whole = bz.bgzf(text, block=5000)
    odd = bz.wrap(bz.deflate(text[:900]), text[:900], extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x50\x00" + bytes(80))  # a 110-byte header
    import gzip

    shapes = {
        "whole": (whole, 0),
        "no_end_marker": (bz.bgzf(text, block=5000, eof=False), 0),
        "long_extra_field": (odd + whole, 0),
        "gzip_member_appended": (whole + gzip.compress(b"ACGT\n"), 2),
        "trailing_bytes": (whole + b"no member", 2),
        "cut_in_a_member": (whole[:-40], 1),
        "cut_in_a_header": (whole[:len(whole) - len(bz.EOF_MARK) + 7], 1),
        "plain_gzip": (gzip.compress(text), 2),
        "empty": (b"", 0),
    }
    for name, (data, state) in shapes.items():
        p = tmp_path / (name + ".gz")
        p.write_bytes(data)
        members, at, want_state = bz.py_walk(data)
        assert want_state == state, name
        off, got_state, size = host.bgzf_walk_file(str(p))
        assert (got_state, size) == (state, len(data)), name
        ends = [m[0] + m[1] + 8 for m in members]  # (payload offset + payload length + trailer)
        assert [int(x) for x in off] == [0] + ends, name
        assert int(off[-1]) == at, name
    with pytest.raises(FileNotFoundError):
        host.bgzf_walk_file(str(tmp_path / "missing.gz"))
