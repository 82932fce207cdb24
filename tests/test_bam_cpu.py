"""BAM input without a GPU: the pure-Python writer and reader of tests/bam_util.py against each other and the spec, and the
record chain of csrc/vs_bam_core.h through its host twin ``vs_bam_scan_host`` -- the same passes the kernels run, with one
thread -- against the reader's serial walk: offsets, flags and couples must be EXACTLY the reader's, whatever the segment
size and whatever the quality, name and aux bytes pretend to be.  tests/bam_check.cpp drives the header as plain C++ under
AddressSanitizer and UBSan with every buffer exactly sized."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_util as bu
import bgzf_util as bz
from conftest import ROOT

SEGS = [64, 128, 4096]


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def expected(data, start=None):
    truth, end = bu.walk(data, start)
    flags = [t[2][0] for t in truth]
    cls = [bu.C_MALFORMED if t[1] is None else bu.classify(t[2][0]) for t in truth]
    recs = np.array([(t[0], t[2][0] | (c << 16), t[2][1], t[2][2]) for t, c in zip(truth, cls)], dtype=np.uint32).reshape(-1, 4)
    part_flags = [f if c != bu.C_MALFORMED else bu.SECONDARY for f, c in zip(flags, cls)]  # (a malformed record takes no part)
    cp, bad, odd = bu.couples(part_flags)
    return recs, np.array(cp, dtype=np.uint32).reshape(-1, 2), end, bad, odd


def check_scan(data, got, start=None):
    recs, ends, info = got
    w_recs, w_ends, w_end, w_bad, _ = expected(data, start)
    assert info["records"] == len(w_recs)
    assert np.array_equal(recs, w_recs)
    assert np.array_equal(ends, w_ends)
    assert (info["end"], info["stop"]) == ({"clean": 0, "cut": 1, "dead": 2}[w_end[0]], w_end[1])
    assert info["bad_couple"] == w_bad
    mal = [i for i, r in enumerate(w_recs) if r[1] >> 16 == bu.C_MALFORMED]
    assert info["malformed"] == (mal[0] if mal else None)


def test_the_symbol_is_there_and_an_empty_window_is_clean(host):
    recs, ends, info = host.bam_scan(b"")
    assert len(recs) == 0 and len(ends) == 0 and info["end"] == 0 and info["stop"] == 0


def test_writer_and_reader_agree_and_the_eof_marker_is_the_specs():
    assert bz.EOF_MARK.hex() == bu.EOF_MARKER_HEX and len(bz.EOF_MARK) == 28
    for name, data in bu.constructed():
        truth, end = bu.walk(data)
        assert end[0] == "clean", name
        records = [t[1] for t in truth]
        assert bu.inflated(records)[bu.header_len(bu.inflated(records)):] == data[bu.header_len(data):], name
        bam = bz.bgzf(data)
        assert bam.endswith(bytes.fromhex(bu.EOF_MARKER_HEX)) and gzip.decompress(bam) == data
        assert bu.read(bam) == records


def test_a_hand_written_single_record_bam():
    hand = bytes.fromhex(
        "42414d01" "00000000" "00000000"  # magic, l_text 0, n_ref 0
        "28000000"                       # block_size 40 = 32 + "r\0" + 2 bytes of bases + 4 of quality
        "ffffffff" "ffffffff" "02" "00" "4812" "0000" "4d00" "04000000" "ffffffff" "ffffffff" "00000000"
        "7200" "1248" "ffffffff")        # name, A C G T, quality
    r = bu.rec("r", 77, "ACGT", qual=b"\xff" * 4)
    assert bu.inflated([r], text=b"") == hand
    assert bu.read(bz.bgzf(hand)) == [r]
    assert bu.header_len(hand) == 12


def test_fastq_pair_follows_the_rules():
    recs = [bu.rec("a", 0x1 | 0x80 | 0x10, "AACGN"), bu.rec("x", 0x1 | 0x40 | 0x100, "TTTT"), bu.rec("a", 0x1 | 0x40, "ACGTR"),
            bu.rec("lonely", 0, "CCC")]
    f, r = bu.fastq_pair(recs)
    assert f == b"@a/1\nACGTR\n+\nIIIII\n" and r == b"@a/2\nNCGTT\n+\nIIIII\n"
    with pytest.raises(ValueError):
        bu.fastq_pair(recs[:2])
    with pytest.raises(ValueError):
        bu.fastq_pair([recs[2], recs[2]])


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("case", bu.constructed(), ids=lambda c: c[0])
def test_chain_is_exactly_the_readers(host, case, seg):
    name, data = case
    got = host.bam_scan(data, bu.header_len(data), seg)
    check_scan(data, got)
    if name == "fakes":
        assert got[2]["records"] == 12 and got[2]["taking_part"] == 12
    if name == "big_aux":
        assert got[2]["records"] == 4 and [int(x) for x in got[1].ravel()] == [0, 1, 3, 2]
    if name == "big_header":
        assert bu.header_len(data) > 90000


@pytest.mark.parametrize("seg", SEGS)
def test_a_window_cut_anywhere_stops_in_front_of_the_cut_record(host, seg):
    name, data = bu.constructed()[0]
    start = bu.header_len(data)
    starts = [t[0] for t in bu.walk(data)[0]]
    for n in sorted(set([start, start + 1, start + 3, start + 4, start + 35, starts[3] + 2, starts[3] + 4, starts[5], starts[5] - 1, len(data) - 1])):
        check_scan(data[:n], host.bam_scan(data[:n], start, seg), start)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("case", bu.malformed(), ids=lambda c: c[0])
def test_malformed_inputs_are_named_by_record(host, case, seg):
    name, data, (what, record) = case
    got = host.bam_scan(data, bu.header_len(data), seg)
    check_scan(data, got)
    recs, ends, info = got
    if what == "dead":
        assert info["end"] == 2 and info["records"] == record
    elif what == "malformed":
        assert info["malformed"] == record
    elif what == "bad_couple":
        assert info["bad_couple"] is not None and expected(data)[1][info["bad_couple"]].max() == record
    elif what == "odd":
        assert info["taking_part"] % 2 == 1 and expected(data)[4] == record and info["bad_couple"] is None
    else:
        assert info["end"] == 1 and info["records"] == record


def test_the_header_is_measured_on_the_host(host, tmp_path):
    for name, data in bu.constructed():
        p = tmp_path / (name + ".bam")
        p.write_bytes(bz.bgzf(data, block=1000 if name == "mixed" else None))
        assert host.bam_header_bytes(str(p)) == bu.header_len(data), name
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(bz.bgzf(bz.fastq_text(10)))
    with pytest.raises(ValueError, match="not a BAM"):
        host.bam_header_bytes(str(p))
    p = tmp_path / "cut.bam"
    p.write_bytes(bz.bgzf(bu.constructed()[1][1][:50000], eof=False))
    with pytest.raises(ValueError, match="not a BAM"):
        host.bam_header_bytes(str(p))


def test_input_choice_and_what_is_out_of_scope(tmp_path):
    from vstrains_amd import pe_inference

    recs = [bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]
    a, b, fq = tmp_path / "a.bam", tmp_path / "b.bam", tmp_path / "r.fq.gz"
    a.write_bytes(bu.write(recs))
    b.write_bytes(bu.write(recs))
    fq.write_bytes(bz.bgzf(bz.fastq_text(3)))
    os.symlink(str(a), str(tmp_path / "link.bam"))
    assert pe_inference.bam_input(str(a), str(a)) == str(a)
    assert pe_inference.bam_input(str(a), str(tmp_path / "link.bam")) == str(a)
    assert pe_inference.bam_input(str(fq), str(fq)) is None and pe_inference.bam_input(str(fq), str(tmp_path / "missing")) is None
    with pytest.raises(ValueError, match="one side only"):
        pe_inference.bam_input(str(a), str(fq))
    with pytest.raises(ValueError, match="one side only"):
        pe_inference.bam_input(str(fq), str(a))
    with pytest.raises(ValueError, match="two different BAM"):
        pe_inference.bam_input(str(a), str(b))
    with pytest.raises(ValueError, match="one process only"):
        pe_inference.bam_input(str(a), str(a), world=2)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/bam_check.cpp: vs_bam_core.h as plain C++, exactly sized heap buffers, AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bam_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bam_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[-1] == "OK"
