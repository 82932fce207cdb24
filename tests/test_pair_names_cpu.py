"""Two FASTQ files paired by read name, without a GPU: the one-thread twin of the kernels (``vs_fastq_join_host``, the text of
csrc/vs_pair_names_core.h) against the plain model of tests/pair_names_model.py on every constructed case; that every case
reaches the edge it was built for; the twin driven through the window protocol on 2 000 random valid inputs against the
whole-file model (cut independence); the refusals of invalid inputs; tests/pair_names_check.cpp under AddressSanitizer and
UBSan; what the two commands refuse before a device is opened; the new entries declared and bound."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import bam_util as bu
import interleaved_model as im
import pair_names_cases as pc
import pair_names_model as pm
from conftest import ROOT

CASES = pc.cases()
SEQUENCES = pc.sequences()


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def check_join(got, want):
    pairs, info = got
    assert [tuple(int(x) for x in p) for p in pairs] == want[0]
    assert info == want[1]


@pytest.mark.parametrize("eof", [(True, True), (False, False), (True, False), (False, True)], ids=["eof", "more_to_come", "file_1_ended", "file_2_ended"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_host_twin_equals_the_model(host, case, eof):
    name, t0, t1, opts = case
    check_join(host.fastq_join(t0, t1, eof[0], eof[1], **opts), pm.join(t0, t1, *eof))
    check_join(host.fastq_join(t0, t1, eof[0], eof[1], singles=False), pm.strict(t0, t1, *eof))


def test_every_case_reaches_its_edge():
    by_name = {c[0]: c for c in CASES}
    j = lambda name, *eof: pm.join(by_name[name][1], by_name[name][2], *eof)
    assert j("empty_files") == ([], dict(pairs=0, records=(0, 0), decided=(0, 0), duplicate=None, order=None, first_bad=None))
    assert j("one_record_each_mates")[0] == [(0, 0)] and j("one_record_each_not_mates")[0] == []
    assert j("one_record_each_not_mates")[1]["decided"] == (1, 1) and j("one_record_each_not_mates", False, False)[1]["decided"] == (0, 0)
    assert j("file_2_empty")[1]["decided"] == (2, 0) and j("file_2_empty", False, False)[1]["decided"] == (0, 0)
    assert j("file_2_empty", False, True)[1]["decided"] == (2, 0)  # (file 2 has ended: nothing of file 1 can find a mate)
    assert j("no_shared_name")[1]["records"] == (70, 70) and j("no_shared_name")[0] == []
    assert j("three_lines_only")[1]["records"] == (0, 0)
    assert j("no_final_newline")[0] == [(0, 0), (1, 1)] and j("no_final_newline", False, False)[0] == [(0, 0)]
    for n in pc.EDGE_SIZES:
        assert j("all_mates_%d" % n)[0] == [(p, p) for p in range(n)]
        for pos in sorted({0, 63, 64, n - 1}):
            if pos >= n:
                continue
            shifted = [(p, p) for p in range(pos)] + [(p, p + 1) for p in range(pos, n - 1)]
            assert j("n%d_without_%d_of_file_1" % (n, pos))[0] == shifted
            assert j("n%d_without_%d_of_file_2" % (n, pos))[0] == [(b, a) for a, b in shifted]
            # in front of the end of the files the record behind the gap is decided by the match behind it, the last one waits
            more = j("n%d_without_%d_of_file_2" % (n, pos), False, False)[1]["decided"]
            assert more == ((n, n - 1) if pos < n - 1 else (n - 1, n - 1))
    assert j("keys_differ_in_the_last_byte")[0] == [(1, 0), (2, 2)]
    assert j("comments_differ")[0] == [(0, 0), (1, 1)] and j("tab_against_space")[0] == [(0, 0)]
    assert j("slash_1_2")[0] == [(0, 0)] and j("slash_1_against_bare")[0] == [] and j("bare_against_slash_2")[0] == []
    assert pm.key(b"@x/1", 0) == pm.key(b"@x", 1) == b"@x" and not im.mates(b"@x/1", b"@x")  # (equal keys, no mates: two singles)
    assert j("slash_1_against_slash_1")[0] == [] and im.mates(b"@x/1", b"@x/1")  # (mates side by side, but the keys differ)
    assert pm.strict(by_name["slash_1_against_slash_1"][1], by_name["slash_1_against_slash_1"][2])[1]["first_bad"] is None
    assert j("only_the_suffix")[0] == [(1, 1)] and j("empty_token")[0] == [(1, 1)] and j("empty_header_lines")[0] == [(1, 2)]
    assert j("one_byte_headers")[0] == [(0, 1), (1, 0)] or j("one_byte_headers")[1]["order"] == 1
    assert j("long_names")[0] == [(0, 0), (2, 2)] and len(im.records(by_name["long_names"][1])[0][0]) > 255
    assert j("prefix_of_the_other")[0] == [(1, 0)]
    assert j("swapped_in_file_2")[1]["order"] == 2 and j("file_2_reversed")[1]["order"] == 1
    dup = lambda name: j(name)[1]["duplicate"]
    assert dup("twice_in_file_1_with_mate") == (0, 1) and dup("twice_in_file_1_without_mate") == (0, 1) and dup("three_times_in_file_1") == (0, 2)
    assert dup("twice_in_file_2_with_mate") == (1, 2) and dup("twice_in_file_2_without_mate") == (1, 2) and dup("three_times_in_file_2") == (1, 0)
    assert dup("twice_in_both_files") == (0, 1) and dup("suffix_makes_the_key_twice") == (0, 0)
    assert dup("empty_keys_are_never_twice") is None and j("empty_keys_are_never_twice")[0] == []
    t0, t1 = by_name["headers_at_every_alignment"][1:3]
    assert set(pc.header_offsets(t0)) == set(pc.header_offsets(t1)) == set(range(16))
    assert by_name["name_bits_2"][3] == dict(name_bits=2) and len(j("name_bits_2")[0]) == 134 and dup("name_bits_2_duplicate") == (0, 3)
    # the wrapping chains: every key of the case starts at the table's last slot
    for name, table in (("table_2_wraps", 2), ("table_4_wraps", 4), ("table_8_wraps_full", 8)):
        _, t0, t1, opts = by_name[name]
        assert opts == dict(table=table)
        keys = {pm.key(r[0], f) for f, t in enumerate((t0, t1)) for r in im.records(t)}
        assert sum(pm.pn_hash(k) & (table - 1) == table - 1 for k in keys) >= 2 and len(keys) <= table
    assert len({pm.key(r[0], f) for f, t in enumerate(by_name["table_8_wraps_full"][1:3]) for r in im.records(t)}) == 8  # (the table is full)


def test_a_table_too_small_for_the_keys_ends_in_a_status(host):
    from vstrains_amd import _native

    t0, t1 = pc.text([b"@a", b"@b"]), pc.text([b"@c"])
    with pytest.raises(_native.NativeError, match="is full"):
        host.fastq_join(t0, t1, table=2)
    for bad in (1, 3, 6):
        with pytest.raises(_native.NativeError, match="bad argument"):
            host.fastq_join(t0, t1, table=bad)


# ---- the window protocol ----------------------------------------------------------------------------------------------------
def whole_file(t0, t1):
    pairs, info = pm.join(t0, t1)
    return pairs, (info["records"][0] - len(pairs), info["records"][1] - len(pairs))


@pytest.mark.parametrize("case", SEQUENCES, ids=lambda c: c[0])
def test_window_sequences_through_the_twin(host, case):
    name, t0, t1, e0, e1 = case
    got = pm.drive(host.fastq_join, t0, t1, e0, e1)
    assert (got[0], got[1]) == whole_file(t0, t1)
    assert pm.drive(pm.join, t0, t1, e0, e1)[:2] == got[:2]
    if name == "waiting_singles_decided_a_window_later":
        first = host.fastq_join(t0[:e0[0]], t1[:e1[0]], False, False)[1]
        assert first["records"] == (14, 10) and first["decided"] == (10, 10)  # (four records wait behind the last match)
    if name.endswith("ends_early"):
        assert got[2] >= 5


def random_valid_input(rng, n):
    """n names in one order, three ways to write them; records deleted from both files, records of one file only among them"""
    h0, h1 = [], []
    drop = rng.choice((0.0, 0.03, 0.3))
    for k in range(n):
        name = b"@r%d_%s" % (k, b"x" * rng.randrange(4))
        kind = rng.randrange(3)
        a, b = [(name + b"/1", name + b"/2"), (name + b" 1:N:0:A", name + b"\t2:N:0:A"), (name, name)][kind]
        if rng.random() >= drop:
            h0.append(a)
        if rng.random() >= drop:
            h1.append(b)
        if rng.random() < 0.05:
            h0.append(b"@only1_%d" % k)
        if rng.random() < 0.05:
            h1.append(b"@only2_%d/2" % k)
        if rng.random() < 0.02:
            h1.append(b" empty token %d" % k)
    return pc.text(h0), pc.text(h1, 3)


def test_the_protocol_does_not_depend_on_where_the_windows_are_cut(host):
    """2 000 seeded random valid inputs; the windows cut after every record for the small ones, at random bytes for the rest,
    and which file gets text next chosen at random: the twin through the protocol == the whole-file model"""
    rng = random.Random(20260519)
    total_pairs = total_singles = rounds = 0
    for k in range(2000):
        small = k % 2 == 0
        t0, t1 = random_valid_input(rng, rng.randrange(0, 9) if small else rng.randrange(9, 40))
        if small:
            e0, e1 = pm.chunks_after_every_record(t0), pm.chunks_after_every_record(t1)
        else:
            e0, e1 = (sorted(set(rng.randrange(len(t) + 1) for _ in range(rng.randrange(1, 6))) | {len(t)}) for t in (t0, t1))
        pick = (lambda r, sizes, eof: (rng.random() < 0.6, rng.random() < 0.6)) if k % 3 else None
        got = pm.drive(host.fastq_join, t0, t1, e0, e1, pick)
        assert (got[0], got[1]) == whole_file(t0, t1), k
        total_pairs, total_singles, rounds = total_pairs + len(got[0]), total_singles + sum(got[1]), rounds + got[2]
    assert total_pairs > 10000 and total_singles > 3000 and rounds > 8000


def test_invalid_inputs_are_refused_inside_a_window_and_counted_across_windows(host):
    by_name = {c[0]: c for c in CASES}
    for name in ("twice_in_file_1_with_mate", "three_times_in_file_2", "twice_in_both_files"):
        _, t0, t1, _ = by_name[name]
        with pytest.raises(ValueError, match="duplicate"):
            pm.drive(host.fastq_join, t0, t1, [len(t0)], [len(t1)])
    for name in ("swapped_in_file_2", "file_2_reversed"):
        _, t0, t1, _ = by_name[name]
        with pytest.raises(ValueError, match="order"):
            pm.drive(host.fastq_join, t0, t1, [len(t0)], [len(t1)])
    # the same swap where no window holds both swapped records of file 2 and their mates: file 1's B and C meet file 2's C
    # alone, the cut falls behind that match, and both B come out as singles
    _, t0, t1, _ = by_name["swapped_in_file_2"]
    pairs, singles, _, _ = pm.drive(host.fastq_join, t0, t1, pm.chunks_after_every_record(t0), pm.chunks_after_every_record(t1),
                                    pick=lambda r, sizes, eof: (True, r != 2))
    assert pairs == [(0, 0), (2, 1), (3, 3)] and singles == (1, 1)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/pair_names_check.cpp: pn_join_host on exactly sized heap buffers, tables of 2, 4 and the production size, the
    window protocol cut after every record; AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pair_names_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pair_names_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[-1] == "OK"


def test_pair_names_entries_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_fastq_pn_open", "vs_fastq_pn_next", "vs_fastq_pn_info", "vs_fastq_pn_close", "vs_fastq_join_host", "vs_fastq_join_text"):
        assert name + "(" in header
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert _native.lib().vs_abi_version() == 11
    assert "vs_pair_names.hip" in open(os.path.join(ROOT, "vstrains_amd", "csrc", "Makefile")).read()


# ---- the stream's workload ----------------------------------------------------------------------------------------------------
def stream_workload(n_pairs: int = 3000, deleted: float = 0.03):
    """(graph, R1, R2 in step, R1 damaged, R2 damaged): seeded pairs of 30-120 bases on a small graph, named in turn with
    `/1` `/2`, with a comment, and bare; and the same with about 3 % of the records deleted from each file at seeded
    positions"""
    from vstrains_amd import synth

    st = synth.make_strains(8, 2000, 0.03, seed=41)
    g = synth.compact_dbg(st, 21)
    f, r = synth.sample_pairs(st, n_pairs, 120, seed=42, sub_rate=0.01, n_rate=0.01)
    rng = random.Random(43)
    h0, h1 = pc.mates_files(n_pairs)
    texts, damaged = [], []
    for heads, seqs in ((h0, f), (h1, r)):
        recs = []
        for h, s_ in zip(heads, seqs):
            s_ = s_[:rng.randrange(30, 121)]
            recs.append(h + b"\n" + s_.encode() + b"\n+\n" + b"I" * len(s_) + b"\n")
        texts.append(b"".join(recs))
        damaged.append(b"".join(x for x in recs if rng.random() >= deleted))
    return g, texts[0], texts[1], damaged[0], damaged[1]


def test_the_stream_workload_is_what_the_gpu_test_needs():
    from oracle import pe_oracle_c

    g, tf, tr, df, dr = stream_workload()
    assert pm.join(tf, tr)[0] == [(p, p) for p in range(3000)] and pm.strict(tf, tr)[1]["first_bad"] is None
    r1, r2, s1, s2 = pm.filtered(df, dr)
    n = len(im.records(r1))
    assert 2700 < n < 2900 and s1 > 50 and s2 > 50 and n + s1 == len(im.records(df)) and n + s2 == len(im.records(dr))
    assert pm.strict(df, dr)[1]["first_bad"] is not None and pm.strict(df, dr)[1]["first_bad"] < 100
    # the counters the stream is compared with are not trivially zero, and differ from those of the damaged files taken by position
    seqs = lambda t: [rec[1].decode() for rec in im.records(t)]
    node_mat, short_mat, stats = pe_oracle_c.Oracle(g.seqs, 21).count_pairs(seqs(r1), seqs(r2))
    assert int(np.count_nonzero(node_mat)) > 100 and int(np.count_nonzero(short_mat)) > 100 and any(int(x) > 0 for x in stats)
    m = min(len(seqs(df)), len(seqs(dr)))
    wrong = pe_oracle_c.Oracle(g.seqs, 21).count_pairs(seqs(df)[:m], seqs(dr)[:m])
    assert not np.array_equal(wrong[0], node_mat)  # (what the run without the flags silently computes)


# ---- what the commands refuse, before a device is opened --------------------------------------------------------------------
def _inputs(tmp_path):
    a, b, bam = tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "a.bam"
    a.write_bytes(im.from_headers([b"@a/1"]))
    b.write_bytes(im.from_headers([b"@a/2"]))
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    return str(a), str(b), str(bam)


def test_check_names_is_refused_where_it_cannot_apply(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference as pi

    a, b, bam = _inputs(tmp_path)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    assert pi.check_names_mode(False, False) is None and pi.check_names_mode(True, False) == "strict" and pi.check_names_mode(True, True) == "singles"
    with pytest.raises(ValueError, match="--check-names-singles.*needs --check-names"):
        pi.check_names_mode(False, True)
    assert pi.check_names_input(a, b) is False  # without the flag nothing changes
    for mode in ("strict", "singles"):
        assert pi.check_names_input(a, b, 1, mode) is True
        assert pi.check_names_input("/dev/fd/3", "/dev/fd/4", 1, mode) is True  # (a pipe is never opened here)
        with pytest.raises(ValueError, match="--interleaved"):
            pi.check_names_input(a, a, 1, mode, interleaved="strict")
        with pytest.raises(ValueError, match="--bam-by-name"):
            pi.check_names_input(bam, bam, 1, mode, bam_by_name=True)
        with pytest.raises(ValueError, match="is a BAM file"):
            pi.check_names_input(bam, bam, 1, mode)
        with pytest.raises(ValueError, match="is a BAM file"):
            pi.check_names_input(a, bam, 1, mode)
        with pytest.raises(ValueError, match="one process only"):
            pi.check_names_input(a, b, 2, mode)
        monkeypatch.setenv("VS_FASTQ_STREAM", "0")
        with pytest.raises(ValueError, match="VS_FASTQ_STREAM=0"):
            pi.check_names_input(a, b, 1, mode)
        monkeypatch.delenv("VS_FASTQ_STREAM")
    with pytest.raises(ValueError, match="'strict' or 'singles'"):
        pi.check_names_input(a, b, 1, "yes")


def _no_device(monkeypatch):
    """any attempt to open a device fails the test"""
    from vstrains_amd import pe as host

    def boom(*a, **k):
        raise AssertionError("a device was opened")

    monkeypatch.setattr(host, "Context", boom)


REFUSALS = [
    ("singles_alone", lambda a, b, bam: (a, b, ["--check-names-singles"], {}), "needs --check-names"),
    ("with_interleaved", lambda a, b, bam: (a, a, ["--check-names", "--interleaved"], {}), "--interleaved"),
    ("with_bam_by_name", lambda a, b, bam: (bam, bam, ["--check-names", "--check-names-singles", "--bam-by-name"], {}), "--bam-by-name"),
    ("bam", lambda a, b, bam: (bam, bam, ["--check-names"], {}), "is a BAM file"),
    ("mapped_open", lambda a, b, bam: (a, b, ["--check-names"], {"VS_FASTQ_STREAM": "0"}), "VS_FASTQ_STREAM=0"),
    ("mapped_open_singles", lambda a, b, bam: (a, b, ["--check-names", "--check-names-singles"], {"VS_FASTQ_STREAM": "0"}), "VS_FASTQ_STREAM=0"),
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

    a, b, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")  # (torchrun's; the refusal comes before a process group is made)
    with pytest.raises(ValueError, match="one process only"):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "out"), "-f", a, "-r", b, "--check-names"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(pi, "_rank_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="one process only"):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out"), "-fwd", a, "-rve", b,
                  "--check-names", "--check-names-singles"])
    with pytest.raises(ValueError, match="one process only"):
        pi.count_links(None, str(tmp_path / "none.gfa"), a, b, 21, check_names="singles")
    assert not (tmp_path / "out").exists()


def test_help_texts_say_extension():
    from vstrains_amd import cli

    text = cli.build_parser().format_help()
    proc = subprocess.run([shutil.which("python3") or "python3", "-m", "vstrains_amd.pe_inference", "-h"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    for helptext in (text, proc.stdout):
        flat = " ".join(helptext.split())
        assert "--check-names extension: " in flat and "--check-names-singles extension: " in flat
