"""The kept records without a mate, without a GPU: the singles function of tests/kept_singles_model.py through the window
protocol against the whole-file statement (every chunking of a small case, a few hundred random valid inputs); the one-thread
twin ``vs_fastq_join_singles_host`` against that function on every constructed case; what ``unpaired_input`` and the two
commands refuse and accept before a device is opened; the new entries declared and bound."""
import os
import random

import numpy as np
import pytest

import bam_util as bu
import interleaved_model as im
import kept_singles_model as km
import pair_names_cases as pc
import pair_names_model as pm
from conftest import ROOT

CASES = pc.cases() + km.cases()
EOFS = [(True, True), (False, False), (True, False), (False, True)]
EOF_IDS = ["eof", "more_to_come", "file_1_ended", "file_2_ended"]


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def as_lists(got):
    pairs, s0, s1, info = got
    return [tuple(int(x) for x in p) for p in pairs], [int(r) for r in s0], [int(r) for r in s1], info


# ---- the singles function ---------------------------------------------------------------------------------------------------
def _small():
    h0, h1 = pc.mates_files(7)
    a, b = [b"@only1_%d" % k for k in range(4)], [b"@only2_%d/2" % k for k in range(4)]
    t0 = pc.text([a[0]] + h0[:2] + [a[1], a[2]] + h0[3:6] + [b" x", a[3]])
    t1 = pc.text([b[0], b[1]] + h1[:3] + [b[2]] + h1[4:] + [b[3]], 2)
    return t0, t1


@pytest.mark.parametrize("lead", [None, 0, 1], ids=["smaller_window_first", "file_1_leads", "file_2_leads"])
def test_every_record_chunking_of_a_small_case(lead):
    """a chunk after every record; one file running ahead of the other by all it has, or the windows in step"""
    t0, t1 = _small()
    want = km.whole_file_singles(t0, t1)
    assert len(want[0]) == 6 and len(want[1]) == 6 and pm.join(t0, t1)[1]["order"] is None
    pick = None if lead is None else (lambda r, sizes, eof: (lead == 0 or eof[1], lead == 1 or eof[0]))
    pairs, singles, rounds = km.drive(km.join_with_singles, t0, t1, pm.chunks_after_every_record(t0), pm.chunks_after_every_record(t1), pick)
    assert (singles[0], singles[1]) == want and pairs == pm.join(t0, t1)[0] and rounds >= 10
    # ... and every pair of cut points: the first chunk of either file ends behind any of its records
    e0, e1 = pm.chunks_after_every_record(t0), pm.chunks_after_every_record(t1)
    for c0 in e0:
        for c1 in e1:
            got = km.drive(km.join_with_singles, t0, t1, sorted({c0, len(t0)}), sorted({c1, len(t1)}), pick)
            assert (got[1][0], got[1][1]) == want, (c0, c1)


def test_random_valid_inputs_keep_exactly_the_records_whose_key_is_not_in_both_files():
    rng = random.Random(20261020)
    kept = rounds = 0
    for k in range(400):
        small = k % 2 == 0
        t0, t1 = km.random_valid_input(rng, rng.randrange(0, 9) if small else rng.randrange(9, 40))
        if small:
            e0, e1 = pm.chunks_after_every_record(t0), pm.chunks_after_every_record(t1)
        else:
            e0, e1 = (sorted(set(rng.randrange(len(t) + 1) for _ in range(rng.randrange(1, 6))) | {len(t)}) for t in (t0, t1))
        pick = (lambda r, sizes, eof: (rng.random() < 0.6, rng.random() < 0.6)) if k % 3 else None
        pairs, singles, n = km.drive(km.join_with_singles, t0, t1, e0, e1, pick)
        want = km.whole_file_singles(t0, t1)
        assert (singles[0], singles[1]) == want, k
        n_rec = [len(im.records(t)) for t in (t0, t1)]
        for f in (0, 1):  # (every record once: half of a pair, or a single)
            assert sorted([p[f] for p in pairs] + singles[f]) == list(range(n_rec[f])), k
        kept, rounds = kept + len(singles[0]) + len(singles[1]), rounds + n
    assert kept > 1500 and rounds > 1500


# ---- the host twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eof", EOFS, ids=EOF_IDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_host_twin_equals_the_singles_function(host, case, eof):
    name, t0, t1, opts = case
    pairs, s0, s1, info = as_lists(host.fastq_join_singles(t0, t1, eof[0], eof[1], **opts))
    want_pairs, want_info = pm.join(t0, t1, *eof)
    assert pairs == want_pairs and info == want_info
    assert (s0, s1) == km.window_singles(t0, t1, *eof)
    # the pairs and the decision are those of the join that drops its singles
    plain = host.fastq_join(t0, t1, eof[0], eof[1], **opts)
    assert np.array_equal(plain[0], np.array(pairs, dtype=np.uint32).reshape(-1, 2)) and plain[1] == info


def test_every_new_case_reaches_its_edge():
    by_name = {c[0]: c for c in km.cases()}
    s = lambda name, *eof: km.window_singles(by_name[name][1], by_name[name][2], *eof)
    n = lambda name: tuple(len(im.records(by_name[name][f])) for f in (1, 2))
    assert s("single_at_record_0_of_file_1") == ([0], []) and s("single_at_record_0_of_file_2") == ([], [0])
    assert s("single_at_the_last_record_of_file_1") == ([12], []) and s("single_at_the_last_record_of_file_2") == ([], [12])
    assert s("single_at_the_last_record_of_file_1", False, False) == ([], [])  # (behind the last match: it waits)
    assert s("single_at_the_last_record_of_file_1", False, True) == ([12], [])  # (file 2 has ended: decided)
    assert s("singles_at_both_ends_of_both_files") == ([0, 1, 14, 15, 16], [0, 13, 14])
    assert s("singles_at_both_ends_of_both_files", False, False) == ([0, 1], [0])
    assert s("all_records_single") == (list(range(9)), list(range(7))) and s("all_records_single", False, False) == ([], [])
    assert s("all_records_single", True, False) == ([], list(range(7))) and n("all_records_single") == (9, 7)
    assert s("no_singles") == ([], []) and s("no_singles", False, False) == ([], [])
    assert s("only_file_2_has_singles") == ([], [3, 4, 14]) and s("only_file_1_has_singles") == ([5, 6, 7], [])
    assert s("an_empty_key") == ([0, 2], [1, 2])  # (empty tokens, and "/1" "/2" whose keys are empty)
    assert s("slash_1_against_bare") == ([1], [1])  # (equal keys, no mates: two singles)
    for name, t0, t1, _ in km.cases():
        assert pm.join(t0, t1)[1]["duplicate"] is None and pm.join(t0, t1)[1]["order"] is None
        assert km.window_singles(t0, t1) == km.whole_file_singles(t0, t1), name


def test_records_behind_the_last_match_are_listed_once_a_window_later(host):
    name, t0, t1, e0, e1 = [c for c in pc.sequences() if c[0] == "waiting_singles_decided_a_window_later"][0]
    first = as_lists(host.fastq_join_singles(t0[:e0[0]], t1[:e1[0]], False, False))
    assert first[3]["records"] == (14, 10) and first[3]["decided"] == (10, 10)
    assert first[1] == [] and first[2] == []  # (records 10..13 of file 1 have no mate, but wait behind the last match: not listed)
    twin = lambda *a: as_lists(host.fastq_join_singles(*a))
    pairs, singles, rounds = km.drive(twin, t0, t1, e0, e1)
    assert singles[0] == list(range(10, 16)) and singles[1] == [] and rounds >= 2  # (each of the six exactly once)
    assert (singles[0], singles[1]) == km.whole_file_singles(t0, t1)
    for case in pc.sequences():
        _, a, b, ea, eb = case
        got = km.drive(twin, a, b, ea, eb)
        assert (got[1][0], got[1][1]) == km.whole_file_singles(a, b) and got[0] == pm.join(a, b)[0], case[0]


def test_the_twin_through_the_protocol_on_random_inputs(host):
    rng = random.Random(7)
    twin = lambda *a: as_lists(host.fastq_join_singles(*a))
    for k in range(200):
        t0, t1 = km.random_valid_input(rng, rng.randrange(0, 30))
        e0, e1 = (sorted(set(rng.randrange(len(t) + 1) for _ in range(rng.randrange(1, 6))) | {len(t)}) for t in (t0, t1))
        got = km.drive(twin, t0, t1, e0, e1, lambda r, sizes, eof: (rng.random() < 0.6, rng.random() < 0.6))
        assert (got[1][0], got[1][1]) == km.whole_file_singles(t0, t1), k


def test_a_refused_round_lists_nothing(host):
    by_name = {c[0]: c for c in pc.cases()}
    for name in ("twice_in_file_1_with_mate", "three_times_in_file_2", "swapped_in_file_2", "file_2_reversed"):
        _, t0, t1, opts = by_name[name]
        pairs, s0, s1, info = as_lists(host.fastq_join_singles(t0, t1, **opts))
        assert (info["duplicate"] is not None or info["order"] is not None) and pairs == [] and s0 == [] and s1 == [] and info["decided"] == (0, 0)


def test_the_entries_refuse_bad_arguments(host):
    import ctypes as C

    from vstrains_amd import _native as nat

    t, u = (np.frombuffer(pc.text([h]), dtype=np.uint8) for h in (b"@a", b"@b"))
    info = (C.c_uint64 * 10)()
    out = np.zeros(4, dtype=np.uint32)
    call = lambda mode, s0, c0: nat.lib().vs_fastq_join_singles_host(t.ctypes.data, len(t), u.ctypes.data, len(u), 1, 1, mode, 0, 0, out.ctypes.data, 1, s0, c0,
                                                                       out.ctypes.data, 1, info)
    assert call(0, out.ctypes.data, 1) == nat.VS_E_ARG  # (the strict mode has no singles)
    assert call(3, out.ctypes.data, 1) == nat.VS_E_ARG
    assert call(2, None, 1) == nat.VS_E_ARG  # (room promised, none given)
    assert call(2, None, 0) == nat.VS_OK and call(1, out.ctypes.data, 1) == nat.VS_OK and int(info[8]) == 1 and int(info[9]) == 1


# ---- the flags ----------------------------------------------------------------------------------------------------------------
def _inputs(tmp_path):
    a, b, bam = tmp_path / "f.fq", tmp_path / "r.fq", tmp_path / "a.bam"
    a.write_bytes(im.from_headers([b"@a/1", b"@b/1"]))
    b.write_bytes(im.from_headers([b"@a/2"]))
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    return str(a), str(b), str(bam)


def _no_device(monkeypatch):
    from vstrains_amd import pe as host

    def boom(*a, **k):
        raise AssertionError("a device was opened")

    monkeypatch.setattr(host, "Context", boom)


def test_unpaired_input_takes_the_pairing_mode(tmp_path):
    from vstrains_amd import pe_inference as pi

    a, b, bam = _inputs(tmp_path)
    # the three homes of --count-singles
    assert pi.unpaired_input((), True, 1, "singles") == []
    assert pi.unpaired_input((), True, 1, None, check_names="singles", fwd=a, rve=b) == []
    assert pi.unpaired_input((), True, 1, None, bam_by_name=True, fwd=bam, rve=bam) == []
    assert pi.unpaired_input([a], True, 1, None, check_names="singles") == [a]
    # without one of them, as before -- and the message names the two new homes
    for kw in (dict(), dict(fwd=a, rve=b), dict(check_names=None, bam_by_name=False)):
        with pytest.raises(ValueError, match="--count-singles.*needs --interleaved --interleaved-singles.*--check-names --check-names-singles.*--bam-by-name"
                                             ".*--single FILE"):
            pi.unpaired_input((), True, 1, None, **kw)
    with pytest.raises(ValueError, match="--count-singles.*--check-names alone stops at the first record without a mate: no singles can exist.*"
                                         "--check-names-singles"):
        pi.unpaired_input((), True, 1, None, check_names="strict", fwd=a, rve=b)
    with pytest.raises(ValueError, match="--count-singles.*collated BAM.*has no singletons.*--bam-by-name"):
        pi.unpaired_input((), True, 1, None, fwd=bam, rve=bam)
    # the other refusals hold under the new homes too
    with pytest.raises(ValueError, match="--count-singles: unpaired reads are counted in one process only.*run without torchrun"):
        pi.unpaired_input((), True, 2, None, check_names="singles")
    with pytest.raises(ValueError, match="--count-singles counts unpaired reads.*--pe-text-from"):
        pi.unpaired_input((), True, 1, None, pe_text_from="aln", bam_by_name=True)
    # and without --count-singles nothing is looked at
    assert pi.unpaired_input((), False, 4, None, check_names="strict", bam_by_name=True, fwd=bam, rve=bam) == []


REFUSALS = [
    ("strict_check_names", lambda a, b, bam: (a, b, ["--check-names", "--count-singles"]), "no singles can exist"),
    ("collated_bam", lambda a, b, bam: (bam, bam, ["--count-singles"]), "has no singletons"),
    ("alone", lambda a, b, bam: (a, b, ["--count-singles"]), "needs --interleaved --interleaved-singles"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_both_commands_refuse_before_a_device_is_opened(tmp_path, monkeypatch, case):
    from vstrains_amd import cli, pe_inference as pi

    _, make, why = case
    fwd, rve, flags = make(*_inputs(tmp_path))
    _no_device(monkeypatch)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=why):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(out), "-f", fwd, "-r", rve, "-k", "21"] + flags)
    with pytest.raises(ValueError, match=why):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(out), "-fwd", fwd, "-rve", rve] + flags)
    with pytest.raises(ValueError, match=why):
        pi.count_links(None, str(tmp_path / "none.gfa"), fwd, rve, 21, check_names="strict" if "--check-names" in flags else None, count_singles=True)
    assert not out.exists()  # nothing was written


ACCEPTED = [
    ("check_names_singles", lambda a, b, bam: (a, b, ["--check-names", "--check-names-singles", "--count-singles"])),
    ("bam_by_name", lambda a, b, bam: (bam, bam, ["--bam-by-name", "--count-singles"])),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c[0])
def test_both_commands_accept_the_new_combinations(tmp_path, monkeypatch, case):
    """the flags pass every check that comes before a device is opened: what stops the run is the device (pe_inference) or the
    graph file that is not there (cli), not a ValueError about the flags"""
    from vstrains_amd import cli, pe_inference as pi

    _, make = case
    fwd, rve, flags = make(*_inputs(tmp_path))
    _no_device(monkeypatch)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    with pytest.raises(AssertionError, match="a device was opened"):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "out"), "-f", fwd, "-r", rve, "-k", "21"] + flags)
    with pytest.raises(SystemExit):  # (the graph file is looked for after the flags)
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out2"), "-fwd", fwd, "-rve", rve]
                 + flags)
    assert not (tmp_path / "out2").exists()


def test_the_streams_refuse_a_mode_they_do_not_know():
    from vstrains_amd import pe as host

    with pytest.raises(ValueError, match='singles is False, True or "keep"'):
        host.PairedNameStream("f", "r", None, singles="drop")
    with pytest.raises(ValueError, match='singles is None or "keep"'):
        host.BamStream("x.bam", None, by_name=True, singles=True)
    with pytest.raises(ValueError, match="needs by_name=True"):
        host.BamStream("x.bam", None, singles="keep")


def test_the_new_entries_are_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_fastq_join_singles_host", "vs_fastq_join_singles_text"):
        assert name + "(" in header
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert "VS_PN_KEEP = 2" in header and "VS_BAM_BY_NAME_KEEP = 2" in header
    assert _native.lib().vs_abi_version() == 11
