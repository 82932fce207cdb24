"""Mates of a BAM matched by name on the device: the kernels of one window (``vs_bam_mates_text``) against the host twin and
the model of tests/bam_mate_model.py on the constructed lists, and the stream (``pe.BamStream(by_name=True)``, the drop-ins
with ``--bam-by-name``) on the records of a workload in three orders against the FASTQ pair the model says the file stands
for, through code that knows nothing of BAM."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_mate_model as mm
import bam_util as bu
import bgzf_util as bz
import test_bam_gpu as bg
import test_bam_mates_cpu as mc
import test_fastq_stream_gpu as sg
from conftest import ROOT, pe_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


# ---- the kernels of one window --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 2])
@pytest.mark.parametrize("seg", [64, 0], ids=["seg64", "default"])
@pytest.mark.parametrize("case", mc.LISTS, ids=lambda c: c[0])
def test_kernels_equal_the_host_twin(host, ctx, case, seg, bits):
    name, records = case
    data = bu.inflated(records)
    skip = bu.header_len(data)
    dev = host.bam_mates(data, skip, seg, ctx, hash_bits=bits)
    twin = host.bam_mates(data, skip, seg, hash_bits=bits)
    assert np.array_equal(dev[0], twin[0]) and np.array_equal(dev[1], twin[1]) and dev[2] == twin[2]
    mc.check_mates(records, dev)


# ---- the stream -----------------------------------------------------------------------------------------------------------
ORDERS = ["as_is", "near", "shuffled"]


def _fastq_files(tmp, tag, records):
    tf, tr, single = mm.fastq_pair_by_name(records)
    (tmp / (tag + "_f.fq")).write_bytes(tf)
    (tmp / (tag + "_r.fq")).write_bytes(tr)
    seqs = [[l for l in t.decode().split("\n")[1::4]] for t in (tf, tr)]
    return str(tmp / (tag + "_f.fq")), str(tmp / (tag + "_r.fq")), seqs, single


@pytest.fixture(scope="module")
def workload(host, ctx, tmp_path_factory):
    g, records = bg._workload()
    tmp = tmp_path_factory.mktemp("bam_by_name")
    orders = {"as_is": records, "near": mm.near(records, 41, 2000), "shuffled": mm.shuffled(records, 42)}
    # 50 pairs lose one mate (25 their first, 25 their second) in the shuffled order
    lose = {(b"p%d" % (40 * k + 1), bu.C_FIRST if k % 2 else bu.C_SECOND) for k in range(50)}
    orders["shuffled_less_50"] = [r for r in orders["shuffled"] if (r.name, bu.classify(r.flag)) not in lose]
    assert len(orders["shuffled_less_50"]) == len(records) - 50
    out = dict(g=g, n_nodes=len(g.seqs), orders={})
    for tag, recs in orders.items():
        ff, fr, seqs, single = _fastq_files(tmp, tag, recs)
        bam = tmp / (tag + ".bam")
        bam.write_bytes(bu.write(recs, block=4000))
        out["orders"][tag] = dict(records=recs, bam=str(bam), seqs=seqs, singletons=single, fastq=(ff, fr))
    # the counters: sums over pairs, so one mapped count of the collated pair serves every order of all 2 000 pairs
    f0 = out["orders"]["as_is"]["fastq"]
    out["want"] = sg._count(host, ctx, g, host.FastqPair(f0[0], f0[1], ctx), False)
    f1 = out["orders"]["shuffled_less_50"]["fastq"]
    out["want_less_50"] = sg._count(host, ctx, g, host.FastqPair(f1[0], f1[1], ctx), False)
    return out


def _check_stream(host, ctx, w, tag, want, n_pairs, n_single):
    o = w["orders"][tag]
    fs = host.BamStream(o["bam"], ctx, block_pairs=173, by_name=True)
    pair = 0
    try:
        for block in fs:
            text, lens, flags = block.unpack()
            block.free()
            at = 0
            for e in range(len(lens)):
                seq = o["seqs"][e & 1][pair + (e >> 1)]
                assert lens[e] == len(seq), (pair, e)
                assert flags[e] & 3 == (1 if "N" in seq else 0) | (2 if set(seq) - set("ACGTN") else 0), (pair, e)
                got = bytes(text[at:at + lens[e]]).decode()
                assert got == "".join(c if c in "ACGT" else "A" for c in seq), (pair, e)
                at += int(lens[e])
            pair += len(lens) // 2
        info = fs.info
    finally:
        fs.close()
    flags_all = [r.flag for r in o["records"]]
    assert pair == n_pairs and info["pairs"] == n_pairs and info["done"]
    assert info["records"] == len(flags_all)  # (carried records are counted once)
    assert info["dropped_0x900"] == sum(bu.classify(f) == bu.C_DROP900 for f in flags_all) > 0
    assert info["dropped_other"] == sum(bu.classify(f) == bu.C_OTHER for f in flags_all) > 0
    assert info["singletons"] == n_single == o["singletons"]
    assert info["text_bytes"] == len(bu.inflated(o["records"])) and info["windows"] >= 1
    fs = host.BamStream(o["bam"], ctx, block_pairs=173, by_name=True)
    got = sg._count(host, ctx, w["g"], fs, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3] == n_pairs
    return info


@pytest.mark.parametrize("seg", [None, 64], ids=["seg_default", "seg64"])
@pytest.mark.parametrize("chunk", [None, 61, 1000], ids=["chunk_default", "chunk61", "chunk1000"])
@pytest.mark.parametrize("order", ORDERS)
def test_stream_by_name_equals_the_mapped_fastq_pair(host, ctx, workload, monkeypatch, order, chunk, seg):
    assert 250 <= workload["n_nodes"] <= 350
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    if seg is not None:
        monkeypatch.setenv("VS_BAM_SEG", str(seg))
    info = _check_stream(host, ctx, workload, order, workload["want"], 2000, 0)
    if order == "as_is":  # collated: by name gives the collated mode's sequence (the model's pair IS bam_util.fastq_pair's)
        assert [open(p, "rb").read() for p in workload["orders"]["as_is"]["fastq"]] == list(bu.fastq_pair(workload["orders"]["as_is"]["records"]))
    elif chunk == 61:
        assert info["waiting_max"] > 0 and info["carried_bytes_max"] > 0 and info["windows"] > 10


def test_stream_by_name_drops_and_counts_singletons(host, ctx, workload, monkeypatch):
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    info = _check_stream(host, ctx, workload, "shuffled_less_50", workload["want_less_50"], 1950, 50)
    assert info["waiting_max"] >= 50


def test_stream_by_name_with_a_narrow_hash(host, ctx, workload, monkeypatch):
    """VS_BAM_NAME_BITS=2: almost every name shares a hash and a probe chain; only the bytes tell names apart"""
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    monkeypatch.setenv("VS_BAM_NAME_BITS", "2")
    _check_stream(host, ctx, workload, "shuffled", workload["want"], 2000, 0)


def _drain(host, ctx, path, by_name=True):
    fs = host.BamStream(str(path), ctx, block_pairs=2, by_name=by_name)
    try:
        return sum(len(b.unpack()[1]) // 2 for b in fs), fs.info
    finally:
        fs.close()


def _good(host, ctx, tmp_path):
    good = tmp_path / "good.bam"
    good.write_bytes(bu.write([bu.rec("a", 0x81, "ACGT"), bu.rec("b", 0x41, "AC"), bu.rec("a", 0x41, "ACGT")]))
    n, info = _drain(host, ctx, good)
    assert n == 1 and info["singletons"] == 1


def test_65_firsts_of_one_name_are_refused(host, ctx, tmp_path):
    records = dict(mm.lists())["65_firsts"]
    p = tmp_path / "crowded.bam"
    p.write_bytes(bu.write(records))
    with pytest.raises(ValueError, match=r"record 64\b.*samtools collate"):
        _drain(host, ctx, p)
    _good(host, ctx, tmp_path)
    ok = tmp_path / "ok.bam"
    ok.write_bytes(bu.write(dict(mm.lists())["64_firsts_64_seconds"]))
    n, info = _drain(host, ctx, ok)
    assert n == 64 and info["singletons"] == 0


@pytest.mark.parametrize("case", bu.malformed(), ids=lambda c: c[0])
def test_errors_by_name_name_the_record(host, ctx, tmp_path, monkeypatch, case):
    name, data, (what, record) = case
    monkeypatch.setenv("VS_STREAM_CHUNK", "300")
    p = tmp_path / (name + ".bam")
    p.write_bytes(bz.bgzf(data, block=300))
    if what in ("dead", "malformed", "cut"):
        words = {"dead": "malformed", "malformed": "malformed", "cut": "truncated record"}[what]
        with pytest.raises(ValueError, match=r"record %d\b.*%s" % (record, words)):
            _drain(host, ctx, p)
    else:  # what the collated mode refuses as "not collated": by name these are pairs and singletons (two_firsts: 10 records, g2 and g3 lost their seconds)
        n, info = _drain(host, ctx, p)
        assert (n, info["singletons"]) == {"two_firsts": (4, 2), "odd_record": (3, 1)}[name]
        assert info["records"] == len(bu.walk(data)[0])
    _good(host, ctx, tmp_path)


def test_without_the_flag_a_shuffled_file_is_not_collated(host, ctx, workload):
    with pytest.raises(ValueError, match="not collated") as ei:
        _drain(host, ctx, workload["orders"]["shuffled"]["bam"], by_name=False)
    assert "samtools collate" in str(ei.value)


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------
def _drop_in_by_name(d, meta, bam, out, env=None):
    """``sg._drop_in`` with the flag (its argument list is fixed)"""
    return subprocess.run(
        [sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
         "-f", bam, "-r", bam, "-k", str(meta["k"]), "--bam-by-name"],
        cwd=ROOT, capture_output=True, text=True, env=env, timeout=600)


def test_pe_inference_by_name_writes_the_files_of_the_pair(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    records = mm.shuffled(bg._records_of_pair(tf, tr), 7)
    with pytest.raises(ValueError):
        bu.fastq_pair(records)  # (not collated)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(records, block=5000))
    pair = sg._drop_in(d, meta, os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq"), tmp_path / "aln_pair")
    got = _drop_in_by_name(d, meta, str(bam), tmp_path / "aln_bam", env=dict(os.environ, VS_STREAM_CHUNK="7000"))
    assert pair.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    for rel in ("pe_info", "st_info"):
        assert (tmp_path / "aln_bam" / rel).read_bytes() == (tmp_path / "aln_pair" / rel).read_bytes() == open(os.path.join(d, rel), "rb").read()
    strip = lambda out, tag: [l.replace(tag, "X") for l in out.splitlines() if not l.startswith("Global time elapsed")]
    assert strip(got.stdout, "aln_bam") == strip(pair.stdout, "aln_pair")
    plain = sg._drop_in(d, meta, str(bam), str(bam), tmp_path / "aln_plain")  # without the flag: as before
    assert plain.returncode != 0 and "not collated" in plain.stderr


def test_cli_by_name_writes_the_same_strains(tmp_path):
    from graph_case import Case

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    with open(inp["fwd"], "rb") as fh:
        tf = fh.read()
    with open(inp["rve"], "rb") as fh:
        tr = fh.read()
    records = mm.shuffled(bg._records_of_pair(tf, tr), 8)
    records.insert(len(records) // 2, bu.rec("lonely", 0x4D, "ACGTACGTAC"))  # (a first without a second: dropped, and said in the log)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(records))

    def run(fwd, rve, out, *more):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                               "-fwd", fwd, "-rve", rve] + list(more), cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run(inp["fwd"], inp["rve"], tmp_path / "out_pair")
    got = run(str(bam), str(bam), tmp_path / "out_bam", "--bam-by-name")
    assert plain.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    for rel in ("strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"):
        assert (tmp_path / "out_pair" / rel).exists(), rel
        assert (tmp_path / "out_bam" / rel).read_bytes() == (tmp_path / "out_pair" / rel).read_bytes(), rel
    said = lambda out: [l for l in (out / "vstrains.log").read_text().splitlines() if "have no mate" in l]
    assert len(said(tmp_path / "out_bam")) == 1 and said(tmp_path / "out_bam")[0].split(" - ")[-1].startswith("1 records")
    assert said(tmp_path / "out_pair") == []
