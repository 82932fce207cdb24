"""Interleaved FASTQ without a GPU: the one-thread twin of the kernels (``vs_fastq_mates_host``, the text of
csrc/vs_mates_core.h) against the plain model of tests/interleaved_model.py on every constructed case, at the end of the file
and in front of it; that every case reaches the edge it was built for; tests/interleaved_check.cpp (the scan form of the
pairing, lanes as loops) under AddressSanitizer and UBSan; what the stream test's workload is made of; what the two commands
refuse before a device is opened; the new entries declared and bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_util as bu
import bgzf_util as bz
import interleaved_model as im
from conftest import ROOT

CASES = im.cases()


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def check_mates(text, eof, got):
    """pairs and info of one window against the model"""
    pairs, info = got
    w_pairs, w_singles, w_held, n = im.pairing(text, eof)
    assert [tuple(int(x) for x in p) for p in pairs] == w_pairs
    assert info == dict(pairs=len(w_pairs), singles=len(w_singles), decided=n - (w_held is not None), held=w_held,
                        first_single=w_singles[0] if w_singles else None, records=n)


@pytest.mark.parametrize("eof", [True, False], ids=["eof", "more_to_come"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_host_twin_equals_the_model(host, case, eof):
    name, text, pairs, singles = case
    check_mates(text, eof, host.fastq_mates(text, eof))
    if eof:  # what the case was written to give, stated without the greedy walk
        got = im.pairing(text, True)
        assert got[0] == pairs and got[1] == singles and got[2] is None


def test_the_last_record_is_held_back_exactly_when_it_is_not_the_second_of_a_pair(host):
    held, not_held = 0, 0
    for name, text, pairs, singles in CASES:
        _, info = host.fastq_mates(text, False)
        w_pairs, _, w_held, n = im.pairing(text, False)
        if n == 0:
            assert info["held"] is None
            continue
        second = bool(w_pairs) and w_pairs[-1][1] == n - 1
        assert (info["held"] is None) == second and info["held"] in (None, n - 1)
        assert info["decided"] == (n if second else n - 1)
        held, not_held = held + (not second), not_held + second
    assert held >= 10 and not_held >= 10  # (both branches are exercised by many cases)


def test_every_case_reaches_its_edge():
    by_name = {c[0]: c for c in CASES}
    count = lambda name: (im.pairing(by_name[name][1])[3], len(by_name[name][2]), by_name[name][3])
    assert count("empty") == (0, 0, []) and count("three_lines_only") == (0, 0, [])
    assert count("one_record") == (1, 0, [0]) and count("one_pair") == (2, 1, []) and count("two_singles") == (2, 0, [0, 1])
    assert count("three_records") == (3, 1, [2])
    assert count("run3_then_pair") == (5, 2, [2]) and by_name["run3_then_pair"][2] == [(0, 1), (3, 4)]  # pair, single, pair
    assert count("run4") == (4, 2, []) and count("run5") == (5, 2, [4])
    assert count("run1000") == (1000, 500, []) and count("run1001") == (1001, 500, [1000])
    assert count("singles_only")[1:] == (0, list(range(70)))
    assert count("alternating_pair_single") == (120, 40, list(range(2, 120, 3)))
    assert count("single_first_and_last") == (6, 2, [0, 5]) and count("two_adjacent_singles") == (6, 2, [2, 3])
    assert count("empty_header_lines") == (4, 1, [0, 1])
    for extra in (1, 2, 3):
        text = by_name["trailing_%d_lines" % extra][1]
        assert text.count(b"\n") == 8 + extra and count("trailing_%d_lines" % extra) == (2, 1, [])
    assert not by_name["no_final_newline"][1].endswith(b"\n") and count("no_final_newline") == (2, 1, [])
    assert im.pairing(by_name["no_final_newline"][1], False)[3] == 1  # (in front of the end of the file the line does not count)
    # the runs of 2..5 equal names start at 61..66 and 253..258: on both sides of, and across, lane 63|64 and thread 255|256
    starts = {}
    for name, headers in im.name_cases():
        if "_at_" not in name:
            continue
        run, off = int(name[3]), int(name.split("_at_")[1])
        assert headers[off:off + run] == [b"@R"] * run and b"@R" not in headers[:off] + headers[off + run:]
        starts.setdefault(run, []).append(off)
        pairs, singles = by_name[name][2], by_name[name][3]
        assert [(off + 2 * p, off + 2 * p + 1) in pairs for p in range(run // 2)] == [True] * (run // 2)
        assert (off + run - 1 in singles) == bool(run % 2)
    assert starts == {run: im.RUN_OFFSETS for run in (2, 3, 4, 5)}
    for edge in (64, 256):
        for run in (2, 3, 4, 5):
            assert any(off < edge < off + run for off in starts[run])  # the run has records on both sides of the edge
            assert any(off + run == edge for off in starts[run]) or run > 3  # ... or ends right at it
            assert edge in starts[run]
    # names of every length 1..40 differing at every byte
    text, pairs, singles = im.differing_names()
    recs = im.records(text)
    assert len(recs) == 4 * sum(range(1, 41)) and len(pairs) * 2 == len(singles)
    seen = set()
    for a, b in zip(singles[0::2], singles[1::2]):
        x, y = recs[a][0], recs[b][0]
        assert len(x) == len(y) and sum(p != q for p, q in zip(x, y)) == 1
        seen.add((len(x), [p != q for p, q in zip(x, y)].index(True)))
    assert seen == {(n, k) for n in range(1, 41) for k in range(n)}
    # the name rule, case by case
    for name, want in (("prefix_short_first", False), ("prefix_long_first", False), ("slash_1_2", True), ("slash_2_1", False), ("slash_1_1", True),
                       ("only_slash_1_2", False), ("only_slash_1_1", True), ("comment_after_space", True), ("comment_after_tab", True)):
        recs = im.records(by_name[name][1])
        assert im.mates(recs[0][0], recs[1][0]) == want == (by_name[name][2] == [(0, 1)]), name
    assert b" " in by_name["comment_after_space"][1] and b"\t" in by_name["comment_after_tab"][1]
    assert im.token(b"@a 1:N:0:x") == b"@a" and im.token(b"@a\tx y") == b"@a" and im.token(b" x") == b"" and im.token(b"") == b""


def test_deinterleave_and_interleave_are_inverse_on_pairs():
    r1, r2 = im.from_headers([b"@a/1", b"@b/1", b"@c/1"]), im.from_headers([b"@a/2", b"@b/2", b"@c/2"])
    text = im.interleave(r1, r2)
    assert im.deinterleave(text, False) == (r1, r2, [])
    mixed = im.record(b"@s0") + text + im.record(b"@s1")
    assert im.deinterleave(mixed, True) == (r1, r2, [0, 7])
    with pytest.raises(ValueError, match="record 0 "):
        im.deinterleave(mixed, False)


def stream_workload():
    """(graph, strict text, text with singles, R1, R2): the pairs of test_bam_gpu._workload as `samtools fastq` names them"""
    import test_bam_gpu as bg

    g, records = bg._workload()
    tf, tr = bu.fastq_pair(records)
    return g, im.interleave(tf, tr), im.with_singles(tf, tr), tf, tr


def test_the_stream_workload_is_what_the_gpu_test_needs():
    from oracle import pe_oracle_c

    g, strict, mixed, tf, tr = stream_workload()
    assert im.deinterleave(strict, False) == (tf, tr, [])
    r1, r2, singles = im.deinterleave(mixed, True)
    n = im.pairing(mixed)[3]
    assert (r1, r2) == (tf, tr) and len(im.records(tf)) == 2000
    assert len(singles) >= 50 and singles[0] == 0 and singles[-1] == n - 1 and n == 4000 + len(singles)
    assert any(b == a + 1 for a, b in zip(singles, singles[1:]))  # two adjacent ones
    with pytest.raises(ValueError, match="record 0 "):
        im.deinterleave(mixed, False)
    # the counters the stream is compared with are not trivially zero
    seqs = [[rec[1].decode() for rec in im.records(t)] for t in (tf, tr)]
    node_mat, short_mat, stats = pe_oracle_c.Oracle(g.seqs, 21).count_pairs(seqs[0], seqs[1])
    assert int(np.count_nonzero(node_mat)) > 100 and int(np.count_nonzero(short_mat)) > 100 and any(int(x) > 0 for x in stats)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/interleaved_check.cpp: the parity scan of vs_mates_core.h with the kernels' lanes as loops against the sequential
    walk and the greedy rule; il_mates on exactly sized heap lines; AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "interleaved_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "interleaved_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[-1] == "OK"


def test_interleaved_entries_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_fastq_il_open", "vs_fastq_il_next", "vs_fastq_il_info", "vs_fastq_il_close", "vs_fastq_mates_host", "vs_fastq_mates_text"):
        assert name + "(" in header
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert _native.lib().vs_abi_version() == 11
    assert "vs_interleaved.hip" in open(os.path.join(ROOT, "vstrains_amd", "csrc", "Makefile")).read()


# ---- what the commands refuse, before a device is opened --------------------------------------------------------------------
def _inputs(tmp_path):
    a, b, bam = tmp_path / "il.fq", tmp_path / "other.fq", tmp_path / "a.bam"
    a.write_bytes(im.from_headers([b"@a/1", b"@a/2"]))
    b.write_bytes(im.from_headers([b"@a/1", b"@a/2"]))
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    return str(a), str(b), str(bam)


def test_interleaved_is_refused_where_it_cannot_apply(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference as pi

    a, b, bam = _inputs(tmp_path)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    assert pi.interleaved_mode(False, False) is None and pi.interleaved_mode(True, False) == "strict" and pi.interleaved_mode(True, True) == "singles"
    with pytest.raises(ValueError, match="--interleaved-singles.*needs --interleaved"):
        pi.interleaved_mode(False, True)
    assert pi.interleaved_input(a, b) is None  # without the flag nothing changes
    for mode in ("strict", "singles"):
        assert pi.interleaved_input(a, a, 1, mode) == a
        os.symlink(a, str(tmp_path / ("link_" + mode)))
        assert pi.interleaved_input(a, str(tmp_path / ("link_" + mode)), 1, mode) == a  # (os.path.samefile)
        assert pi.interleaved_input("/dev/stdin", "/dev/stdin", 1, mode) == "/dev/stdin"
        with pytest.raises(ValueError, match="two different files"):
            pi.interleaved_input(a, b, 1, mode)
        with pytest.raises(ValueError, match="two different files"):
            pi.interleaved_input(a, str(tmp_path / "missing"), 1, mode)
        with pytest.raises(ValueError, match="is a BAM file"):
            pi.interleaved_input(bam, bam, 1, mode)
        with pytest.raises(ValueError, match="one process only.*BGZF pairs.*collated BAMs"):
            pi.interleaved_input(a, a, 2, mode)
        monkeypatch.setenv("VS_FASTQ_STREAM", "0")
        with pytest.raises(ValueError, match="VS_FASTQ_STREAM=0"):
            pi.interleaved_input(a, a, 1, mode)
        monkeypatch.delenv("VS_FASTQ_STREAM")
    with pytest.raises(ValueError, match="'strict' or 'singles'"):
        pi.interleaved_input(a, a, 1, "yes")
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    assert pi.interleaved_input(fifo, fifo, 1, "strict") == fifo  # (named once or twice, a pipe is never opened here)


def _no_device(monkeypatch):
    """any attempt to open a device fails the test"""
    from vstrains_amd import pe as host

    def boom(*a, **k):
        raise AssertionError("a device was opened")

    monkeypatch.setattr(host, "Context", boom)


REFUSALS = [
    ("two_files", lambda a, b, bam: (a, b, ["--interleaved"], {}), "two different files"),
    ("bam", lambda a, b, bam: (bam, bam, ["--interleaved", "--interleaved-singles"], {}), "is a BAM file"),
    ("singles_alone", lambda a, b, bam: (a, a, ["--interleaved-singles"], {}), "needs --interleaved"),
    ("mapped_open", lambda a, b, bam: (a, a, ["--interleaved"], {"VS_FASTQ_STREAM": "0"}), "VS_FASTQ_STREAM=0"),
    ("mapped_open_singles", lambda a, b, bam: (a, a, ["--interleaved", "--interleaved-singles"], {"VS_FASTQ_STREAM": "0"}), "VS_FASTQ_STREAM=0"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_both_commands_refuse_before_a_device_is_opened(tmp_path, monkeypatch, case):
    from vstrains_amd import cli, pe_inference as pi

    _, make, why = case
    fwd, rve, flags, env = make(*_inputs(tmp_path))
    _no_device(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=why):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(out), "-f", fwd, "-r", rve, "-k", "21"] + flags)
    with pytest.raises(ValueError, match=why):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(out), "-fwd", fwd, "-rve", rve] + flags)
    assert not out.exists()  # nothing was written


def test_both_commands_refuse_a_process_group(tmp_path, monkeypatch):
    from vstrains_amd import cli, pe_inference as pi

    a, _, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")  # (torchrun's; the refusal comes before a process group is made)
    with pytest.raises(ValueError, match="one process only"):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "out"), "-f", a, "-r", a, "--interleaved"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(pi, "_rank_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="one process only"):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out"), "-fwd", a, "-rve", a,
                  "--interleaved", "--interleaved-singles"])
    with pytest.raises(ValueError, match="one process only"):
        pi.count_links(None, str(tmp_path / "none.gfa"), a, a, 21, interleaved="singles")
    assert not (tmp_path / "out").exists()


def test_help_texts_say_extension():
    from vstrains_amd import cli

    text = cli.build_parser().format_help()
    proc = subprocess.run([shutil.which("python3") or "python3", "-m", "vstrains_amd.pe_inference", "-h"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    for helptext in (text, proc.stdout):
        flat = " ".join(helptext.split())
        assert "--interleaved extension: " in flat and "--interleaved-singles extension: " in flat
