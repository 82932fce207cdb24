"""Mates of a BAM matched by name, without a GPU: the one-thread twin of the kernels (``vs_bam_mates_host``, the text of
csrc/vs_bam_core.h) against the sequential FIFO rule of tests/bam_mate_model.py on the constructed lists, at every width of
the hash; the window-wise form against the sequential rule at random cuts, in Python and through the twin;
tests/bam_mates_check.cpp under AddressSanitizer and UBSan; and what ``--bam-by-name`` refuses, from the Python layer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_mate_model as mm
import bam_util as bu
import bgzf_util as bz
from conftest import ROOT


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def all_lists():
    """the constructed lists, and the collated files of the chain tests (unique names: by name gives the collated couples)"""
    import test_bam_gpu as bg

    out = list(mm.lists())
    out += [(n, [t[1] for t in bu.walk(d)[0]]) for n, d in bu.constructed() if n != "header_only"]
    out.append(("workload", bg._workload()[1]))
    return out


LISTS = all_lists()


def check_mates(records, got):
    """pairs, waiting and info of one window against the model"""
    pairs, waiting, info = got
    crowd = mm.crowded(records)
    assert info["crowded"] == crowd
    if crowd is not None:
        assert info["pairs"] == 0 and info["waiting"] == 0
        return
    w_pairs, w_single = mm.mates(records)
    assert [tuple(int(x) for x in p) for p in pairs] == w_pairs
    assert [int(x) for x in waiting] == w_single
    assert info["pairs"] == len(w_pairs) and info["waiting"] == len(w_single)


@pytest.mark.parametrize("bits", [64, 2, 0])
@pytest.mark.parametrize("case", LISTS, ids=lambda c: c[0])
def test_the_host_twin_equals_the_model(host, case, bits):
    name, records = case
    data = bu.inflated(records)
    got = host.bam_mates(data, bu.header_len(data), 64 if bits == 2 else 0, hash_bits=bits)
    check_mates(records, got)
    if name == "65_firsts":
        assert got[2]["crowded"] == 64
    if name == "64_firsts_64_seconds":
        assert [tuple(int(x) for x in p) for p in got[0]] == [(j, 64 + j) for j in range(64)]
    if name in ("mixed", "big_aux", "workload"):  # collated, one name per pair: the couples of the collated mode, in its order
        assert [tuple(int(x) for x in p) for p in got[0]] == [tuple(c) for c in bu.couples([r.flag for r in records])[0]]
        assert len(got[1]) == 0
    if name == "fakes":  # (every record of it has a name of its own: the collated mode couples neighbours, by name nothing pairs)
        assert len(got[0]) == 0 and len(got[1]) == 12


def test_the_model_itself():
    F, S = mm.F, mm.S
    r = lambda n, f: bu.rec(n, f, "ACGT")
    recs = [r("a", F), r("a", F), r("b", S), r("a", S), r("b", F), r("a", S), r("a", F)]
    assert mm.mates(recs) == ([(0, 3), (4, 2), (1, 5)], [6])
    f, s, single = mm.fastq_pair_by_name(recs)
    assert f.count(b"\n") == s.count(b"\n") == 12 and single == 1 and f.startswith(b"@a/1\n") and s.startswith(b"@a/2\n")
    assert mm.crowded([r("n", F)] * 64 + [r("n", S)] * 64) is None and mm.crowded([r("n", F)] * 65) == 64
    coll = [r("p%d" % (i // 2), F if i % 2 == 0 else S) for i in range(40)]
    for order in (mm.near(coll, 1, 7), mm.shuffled(coll, 2)):
        assert sorted(order) == sorted(coll) and order != coll
        assert sorted((order[a].name, order[b].name) for a, b in mm.mates(order)[0]) == [(b"p%d" % i, b"p%d" % i) for i in sorted(range(20), key=str)]


def _random_list(rng):
    names = [b"n%d" % i for i in range(4)]
    flags = [mm.F, mm.S, mm.F | bu.REVERSE, mm.S, mm.F | bu.SECONDARY, 0]
    return [bu.rec(names[int(rng.integers(0, 4))], flags[int(rng.integers(0, 6))], "ACGT"[:int(rng.integers(0, 5))]) for _ in range(int(rng.integers(0, 41)))]


def test_window_wise_equals_sequential_at_random_cuts():
    """pairs, their order and the waiting set behind every window, for 6 000 seeded draws of up to 40 records with four
    names and up to 5 cuts"""
    rng = np.random.default_rng(2024)
    for _ in range(6000):
        records = _random_list(rng)
        cuts = [int(c) for c in rng.integers(0, len(records) + 1, size=int(rng.integers(0, 6)))]
        pairs, waiting, trail = mm.mates_windowed(records, cuts)
        assert (pairs, waiting) == mm.mates(records)
        bounds = sorted(cuts) + [len(records)]
        assert trail == [mm.mates(records[:b])[1] for b in bounds]


def test_the_twin_window_by_window_equals_the_sequential_rule(host):
    """the same with the twin matching every window: [carried records, whole][new records] as the stream builds it"""
    rng = np.random.default_rng(2025)

    def twin(bits):
        def match(window):
            data = bu.inflated(window)
            pairs, waiting, info = host.bam_mates(data, bu.header_len(data), 64, hash_bits=bits)
            assert info["crowded"] is None
            return [tuple(int(x) for x in p) for p in pairs], [int(x) for x in waiting]
        return match

    for draw in range(1000):
        records = _random_list(rng)
        cuts = [int(c) for c in rng.integers(0, len(records) + 1, size=int(rng.integers(0, 6)))]
        got = mm.mates_windowed(records, cuts, twin((64, 2, 0)[draw % 3]))
        assert got[:2] == mm.mates(records), draw
        assert got[2] == [mm.mates(records[:b])[1] for b in sorted(cuts) + [len(records)]], draw


def test_by_name_is_refused_where_it_cannot_apply(tmp_path):
    from vstrains_amd import pe_inference

    recs = [bu.rec("a", 0x81, "ACGT"), bu.rec("b", 0x41, "ACGT"), bu.rec("a", 0x41, "ACGT"), bu.rec("b", 0x81, "ACGT")]
    a, fq, fq2 = tmp_path / "a.bam", tmp_path / "r.fq.gz", tmp_path / "plain.fq"
    a.write_bytes(bu.write(recs))
    fq.write_bytes(bz.bgzf(bz.fastq_text(3)))
    fq2.write_bytes(bz.fastq_text(3))
    assert pe_inference.bam_input(str(a), str(a), by_name=True) == str(a)
    for f, r in ((str(fq), str(fq)), (str(fq2), str(fq)), (str(fq2), str(tmp_path / "missing"))):
        with pytest.raises(ValueError, match="--bam-by-name.*not a BAM"):
            pe_inference.bam_input(f, r, by_name=True)
    with pytest.raises(ValueError, match="one side only"):
        pe_inference.bam_input(str(a), str(fq), by_name=True)
    with pytest.raises(ValueError, match="one side only"):
        pe_inference.bam_input(str(fq2), str(a), by_name=True)
    with pytest.raises(ValueError, match="one process only"):
        pe_inference.bam_input(str(a), str(a), world=2, by_name=True)
    # without the flag nothing changes
    assert pe_inference.bam_input(str(fq), str(fq)) is None and pe_inference.bam_input(str(a), str(a)) == str(a)
    # the command line says the same before anything is opened on a device
    proc = subprocess.run([shutil.which("python3") or "python3", "-m", "vstrains_amd.pe_inference", "-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "aln"),
                           "-f", str(fq2), "-r", str(fq2), "--bam-by-name"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode != 0 and "--bam-by-name" in proc.stderr and "not a BAM" in proc.stderr


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/bam_mates_check.cpp: the matching of vs_bam_core.h as plain C++, exactly sized heap buffers, table sizes 2, 4
    and the production size, the window cut after every record, AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bam_mates_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bam_mates_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[-1] == "OK"
