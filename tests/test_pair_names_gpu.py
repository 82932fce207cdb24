"""Two FASTQ files paired by read name on the device: the kernels of one pair of windows (``vs_fastq_join_text``) against the
host twin and the plain model of tests/pair_names_model.py on every constructed case; the kernels driven through the window
protocol; the strict stream (``pe.PairedNameStream``) against the mapped ingest block by block, and its refusal; the singles
stream on a pair with records deleted from both files against the mapped ingest of the two files filtered to their shared
names, in every form the reader knows; the duplicate, order and window refusals; and the two drop-ins with the flags on the
damaged pair against the same command on the filtered pair."""
import gzip
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bgzf_util as bz
import interleaved_model as im
import pair_names_cases as pc
import pair_names_model as pm
import test_fastq_stream_gpu as sg
import test_pair_names_cpu as cpu
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


# ---- the kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eof", [(True, True), (False, False), (True, False), (False, True)], ids=["eof", "more_to_come", "file_1_ended", "file_2_ended"])
@pytest.mark.parametrize("case", cpu.CASES, ids=lambda c: c[0])
def test_kernels_equal_the_host_twin_and_the_model(host, ctx, case, eof):
    name, t0, t1, opts = case
    dev = host.fastq_join(t0, t1, eof[0], eof[1], ctx, guard=64, **opts)  # (raises if a sentinel word around the pair list changed)
    twin = host.fastq_join(t0, t1, eof[0], eof[1], **opts)
    assert np.array_equal(dev[0], twin[0]) and dev[1] == twin[1]
    cpu.check_join(dev, pm.join(t0, t1, *eof))
    dev = host.fastq_join(t0, t1, eof[0], eof[1], ctx, singles=False, guard=64)
    cpu.check_join(dev, pm.strict(t0, t1, *eof))


@pytest.mark.parametrize("case", cpu.SEQUENCES, ids=lambda c: c[0])
def test_window_sequences_through_the_kernels(host, ctx, case):
    name, t0, t1, e0, e1 = case
    got = pm.drive(lambda *a: host.fastq_join(*a, ctx=ctx), t0, t1, e0, e1)
    assert (got[0], got[1]) == cpu.whole_file(t0, t1)


def test_a_table_too_small_for_the_keys_ends_in_a_status(host, ctx):
    from vstrains_amd import _native

    with pytest.raises(_native.NativeError, match="is full"):
        host.fastq_join(pc.text([b"@a", b"@b"]), pc.text([b"@c"]), ctx=ctx, table=2)


# ---- the streams ----------------------------------------------------------------------------------------------------------
class Checked:
    """a stream whose every block is compared, end by end and in order, with the sequences of the expected pair"""

    def __init__(self, fs, seqs):
        self.fs, self.seqs, self.pair, self.blocks = fs, seqs, 0, 0

    def next_block(self):
        block = self.fs.next_block()
        if block is None:
            return None
        text, lens, flags = block.unpack()
        at = 0
        for e in range(len(lens)):
            want = self.seqs[e & 1][self.pair + (e >> 1)]
            assert lens[e] == len(want), (self.pair, e)
            assert flags[e] & 3 == (1 if "N" in want else 0) | (2 if set(want) - set("ACGTN") else 0), (self.pair, e)
            assert bytes(text[at:at + lens[e]]).decode() == "".join(c if c in "ACGT" else "A" for c in want), (self.pair, e)
            at += int(lens[e])
        self.pair += len(lens) // 2
        self.blocks += 1
        return block

    @property
    def n_pairs(self):
        return self.fs.n_pairs

    def close(self):
        self.info = self.fs.info
        self.fs.close()


def same_counters(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3]


@pytest.fixture(scope="module")
def workload(host, ctx, tmp_path_factory):
    """the in-step pair, the damaged pair, the damaged pair filtered to its shared names; the mapped ingest's counters of the
    in-step and of the filtered pair, computed once"""
    g, tf, tr, df, dr = cpu.stream_workload()
    r1, r2, s1, s2 = pm.filtered(df, dr)
    tmp = tmp_path_factory.mktemp("pn_workload")
    for name, data in (("f.fq", tf), ("r.fq", tr), ("df.fq", df), ("dr.fq", dr), ("r1.fq", r1), ("r2.fq", r2)):
        (tmp / name).write_bytes(data)
    mapped = lambda a, b: sg._count(host, ctx, g, host.FastqPair(str(tmp / a), str(tmp / b), ctx), False)
    seqs = lambda a, b: [[rec[1].decode() for rec in im.records(t)] for t in (a, b)]
    return dict(g=g, tmp=tmp, tf=tf, tr=tr, df=df, dr=dr, singles=(s1, s2), n_filtered=len(im.records(r1)), want_step=mapped("f.fq", "r.fq"),
                want_filtered=mapped("r1.fq", "r2.fq"), seqs_step=seqs(tf, tr), seqs_filtered=seqs(r1, r2))


@pytest.mark.parametrize("chunk", [61, 1000], ids=["chunk61", "chunk1000"])
def test_strict_stream_equals_the_mapped_pair(host, ctx, workload, monkeypatch, chunk):
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    tmp = workload["tmp"]
    fs = Checked(host.PairedNameStream(str(tmp / "f.fq"), str(tmp / "r.fq"), ctx, block_pairs=173), workload["seqs_step"])
    got = sg._count(host, ctx, workload["g"], fs, True)
    same_counters(got, workload["want_step"])
    info = fs.info
    assert got[3] == fs.pair == 3000 and fs.blocks >= 18
    assert info["pairs"] == 3000 and info["singles_fwd"] == info["singles_rve"] == 0 and info["records_fwd"] == info["records_rve"] == 3000
    assert info["text_bytes"] == info["file_bytes"] == len(workload["tf"]) + len(workload["tr"]) and info["flags"] == 16
    assert info["max_window_bytes"] < 3 * chunk + 1000  # (carry + one slot; a record is at most some 270 bytes)


def _drain(host, ctx, fwd, rve, singles=False):
    fs = host.PairedNameStream(str(fwd), str(rve), ctx, block_pairs=173, singles=singles)
    try:
        return sum(len(b.unpack()[1]) // 2 for b in fs), fs.info
    finally:
        fs.close()


def test_strict_stream_fails_at_the_pair_behind_a_lost_record(host, ctx, workload, monkeypatch):
    tmp = workload["tmp"]
    recs = [im.records(workload["tf"]), im.records(workload["tr"])]
    lost = 1234
    (tmp / "r_lost.fq").write_bytes(b"".join(b"\n".join(r) + b"\n" for r in recs[1][:lost] + recs[1][lost + 1:]))
    (tmp / "f_short.fq").write_bytes(b"".join(b"\n".join(r) + b"\n" for r in recs[0][:2990]))
    messages = []
    for chunk in (61, 1000):
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
        with pytest.raises(ValueError) as err:
            _drain(host, ctx, tmp / "f.fq", tmp / "r_lost.fq")
        messages.append(str(err.value))
    msg = messages[0]
    assert messages[1] == msg  # (the same message whatever the chunk size)
    assert str(tmp / "f.fq") in msg and str(tmp / "r_lost.fq") in msg and "pair %d " % lost in msg and "--check-names-singles" in msg
    assert '"%s"' % recs[0][lost][0].decode() in msg and '"%s"' % recs[1][lost + 1][0].decode() in msg
    # a complete record left over in the longer file
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    for fwd, rve, longer in (("f_short.fq", "r.fq", 1), ("r.fq", "f_short.fq", 0)):
        if longer == 0:  # (file 1 = the R2 records: no pair is a pair of mates, the first stops the run)
            with pytest.raises(ValueError, match="pair 0 is no pair of mates"):
                _drain(host, ctx, tmp / fwd, tmp / rve)
            continue
        with pytest.raises(ValueError) as err:
            _drain(host, ctx, tmp / fwd, tmp / rve)
        msg = str(err.value)
        assert "pair 2990 " in msg and "end of file" in msg and '"%s"' % recs[1][2990][0].decode() in msg and str(tmp / "f_short.fq") in msg
    # the singles mode takes the same inputs: one record of file 1 dropped, ten of file 2
    n, info = _drain(host, ctx, tmp / "f.fq", tmp / "r_lost.fq", singles=True)
    assert n == 2999 and (info["singles_fwd"], info["singles_rve"]) == (1, 0)
    n, info = _drain(host, ctx, tmp / "f_short.fq", tmp / "r.fq", singles=True)
    assert n == 2990 and (info["singles_fwd"], info["singles_rve"]) == (0, 10)


@pytest.mark.parametrize("chunk", [61, 1000], ids=["chunk61", "chunk1000"])
def test_singles_stream_equals_the_mapped_pair_of_the_filtered_files(host, ctx, workload, monkeypatch, chunk):
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    monkeypatch.setenv("VS_PAIR_WINDOW", str(8 * 1024))  # (in-order files never come near it)
    if chunk == 1000:
        monkeypatch.setenv("VS_PAIR_NAME_BITS", "2")  # (every key of a window on one of four probe chains: the bytes decide)
    tmp = workload["tmp"]
    fs = Checked(host.PairedNameStream(str(tmp / "df.fq"), str(tmp / "dr.fq"), ctx, block_pairs=173, singles=True), workload["seqs_filtered"])
    got = sg._count(host, ctx, workload["g"], fs, True)
    same_counters(got, workload["want_filtered"])
    info, n = fs.info, workload["n_filtered"]
    assert got[3] == fs.pair == n == info["pairs"]
    assert (info["singles_fwd"], info["singles_rve"]) == workload["singles"]
    assert info["records_fwd"] == n + workload["singles"][0] and info["records_rve"] == n + workload["singles"][1]
    assert info["text_bytes"] == info["file_bytes"] == len(workload["df"]) + len(workload["dr"]) and info["flags"] == 16
    assert info["max_window_bytes"] < 8 * 1024


FORMS = ["plain", "gzip", "bgzf", "fifo", "gzip_device", "mixed", "crlf", "no_final_newline"]


@pytest.mark.parametrize("form", FORMS)
def test_every_form_of_the_same_reads_counts_the_same(host, ctx, workload, tmp_path, monkeypatch, form):
    df, dr = workload["df"], workload["dr"]
    monkeypatch.setenv("VS_STREAM_CHUNK", "4093")
    make = {"plain": lambda t: t, "gzip": gzip.compress, "bgzf": lambda t: bz.bgzf(t, block=3000), "fifo": lambda t: t, "gzip_device": gzip.compress,
            "crlf": lambda t: t.replace(b"\n", b"\r\n"), "no_final_newline": lambda t: t[:-1]}
    data = (gzip.compress(df), bz.bgzf(dr, block=3000)) if form == "mixed" else (make[form](df), make[form](dr))
    if form == "gzip_device":
        monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    if form == "fifo":
        with sg.Fifos(tmp_path, data[0], data[1]) as (pf, pr):
            fs = Checked(host.PairedNameStream(pf, pr, ctx, block_pairs=173, singles=True), workload["seqs_filtered"])
            got = sg._count(host, ctx, workload["g"], fs, True)
    else:
        (tmp_path / "f.fq").write_bytes(data[0])
        (tmp_path / "r.fq").write_bytes(data[1])
        fs = Checked(host.PairedNameStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, block_pairs=173, singles=True), workload["seqs_filtered"])
        got = sg._count(host, ctx, workload["g"], fs, True)
    same_counters(got, workload["want_filtered"])
    info = fs.info
    assert info["pairs"] == workload["n_filtered"] and (info["singles_fwd"], info["singles_rve"]) == workload["singles"]
    assert info["file_bytes"] == len(data[0]) + len(data[1])
    assert info["flags"] & 3 == (1 if form == "crlf" else 0) and bool(info["flags"] & 12) == (form in ("gzip", "bgzf", "gzip_device", "mixed"))
    if form != "crlf":
        assert info["text_bytes"] == len(df) + len(dr) - 2 * (form == "no_final_newline")


# ---- the refusals through the stream ------------------------------------------------------------------------------------------
def test_the_stream_refuses_a_name_twice_mates_out_of_order_and_a_window_without_a_decision(host, ctx, workload, tmp_path, monkeypatch):
    monkeypatch.setenv("VS_STREAM_CHUNK", "20000")  # (some hundred records: the records that collide share a window)
    recs = [im.records(workload["df"]), im.records(workload["dr"])]
    write = lambda name, rs: (tmp_path / name).write_bytes(b"".join(b"\n".join(r) + b"\n" for r in rs)) and str(tmp_path / name)
    f, r = write("f.fq", recs[0]), write("r.fq", recs[1])
    # a name twice in file 2, two records apart
    twice = write("twice.fq", recs[1][:502] + [recs[1][500]] + recs[1][502:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, twice, singles=True)
    name = pm.key(recs[1][500][0], 1).decode()
    assert "name %s occurs twice in %s" % (name, twice) in str(err.value) and "record 500," in str(err.value)
    # ... and in file 1
    twice = write("twice1.fq", recs[0][:41] + [recs[0][40]] + recs[0][41:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, twice, r, singles=True)
    assert "name %s occurs twice in %s" % (pm.key(recs[0][40][0], 0).decode(), twice) in str(err.value) and "record 40," in str(err.value)
    # two adjacent records of file 2 swapped (both have their mates in file 1)
    pairs = pm.join(workload["df"], workload["dr"])[0]
    p = next(p for p in range(700, len(pairs) - 1) if pairs[p + 1][1] == pairs[p][1] + 1)
    j = pairs[p][1]
    swapped = write("swapped.fq", recs[1][:j] + [recs[1][j + 1], recs[1][j]] + recs[1][j + 2:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, swapped, singles=True)
    msg = str(err.value)
    assert "%s record %d and %s record %d " % (f, pairs[p + 1][0], swapped, j) in msg and "are mates but lie behind" in msg and "same order" in msg
    # the files in different orders: file 2 reversed, no record of a window has its mate in the other
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    monkeypatch.setenv("VS_PAIR_WINDOW", "4096")
    reverse = write("reversed.fq", recs[1][::-1])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, reverse, singles=True)
    msg = str(err.value)
    assert "wait without a mate" in msg and "probably not in the same order" in msg and (f in msg or reverse in msg)


def test_messages_arrive_whole_under_long_paths_and_long_header_lines(host, ctx, tmp_path, monkeypatch):
    """two paths of some 300 bytes and two header lines of more than 200: every message is complete to its last word, the
    header lines cut at 200 bytes"""
    monkeypatch.setenv("VS_STREAM_CHUNK", "20000")
    deep = tmp_path / ("d" * 120) / ("e" * 120)
    os.makedirs(deep)
    long = lambda k, which: b"@" + (b"name%d_" % k) * 40 + b"/%d" % which  # (some 250 bytes)
    h0 = [long(k, 1) for k in range(6)]
    h1 = [long(k, 2) for k in range(6)]
    write = lambda name, heads: (deep / name).write_bytes(pc.text(heads)) and str(deep / name)
    f = write("f.fq", h0)
    assert len(f) > 300 and len(h0[0]) > 240
    # strict: file 2 lacks record 1
    lost = write("lost.fq", h1[:1] + h1[2:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, lost)
    msg = str(err.value)
    assert f in msg and lost in msg and "pair 1 is no pair of mates" in msg and msg.endswith("add --check-names-singles")
    assert '"%s"' % h0[1][:200].decode() in msg and '"%s"' % h1[2][:200].decode() in msg and h0[1][:201].decode() not in msg
    # strict: a record left over
    short = write("short.fq", h1[:5])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, short)
    msg = str(err.value)
    assert f in msg and short in msg and "pair 5 " in msg and "end of file" in msg and '"%s"' % h0[5][:200].decode() in msg
    assert msg.endswith("add --check-names-singles")
    # singles: a name twice, mates out of order
    twice = write("twice.fq", h1[:3] + [h1[1]] + h1[3:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, twice, singles=True)
    msg = str(err.value)
    assert msg.startswith("name %s occurs twice in %s" % (pm.key(h1[1], 1)[:200].decode(), twice))  # (the name as far as the 200 bytes of its line go)
    assert "record 1," in msg and msg.endswith("stands for one record")
    swapped = write("swapped.fq", h1[:2] + [h1[3], h1[2]] + h1[4:])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, f, swapped, singles=True)
    msg = str(err.value)
    assert msg.startswith("%s record 3 and %s record 2 " % (f, swapped)) and "are mates but lie behind" in msg and msg.endswith("both files in the same order")
    # ... and the window without a decision
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    monkeypatch.setenv("VS_PAIR_WINDOW", "2048")
    many0, many1 = [long(k, 1) for k in range(40)], [long(k, 2) for k in range(40)]
    a, b = write("many.fq", many0), write("reversed.fq", many1[::-1])
    with pytest.raises(ValueError) as err:
        _drain(host, ctx, a, b, singles=True)
    msg = str(err.value)
    assert (msg.startswith(a) or msg.startswith(b)) and "wait without a mate" in msg and msg.endswith("probably not in the same order")


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------
def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _named(tf: bytes, tr: bytes):
    """two FASTQ texts under one name per pair (in turn /1 /2, a comment, bare)"""
    h0, h1 = pc.mates_files(len(im.records(tf)))
    out = []
    for heads, t in ((h0, tf), (h1, tr)):
        out.append(b"".join(b"\n".join([h] + rec[1:]) + b"\n" for h, rec in zip(heads, im.records(t))))
    return out


def _damage(t: bytes, seed: int) -> bytes:
    import random

    rng = random.Random(seed)
    return b"".join(b"\n".join(rec) + b"\n" for rec in im.records(t) if rng.random() >= 0.03)


def _pe_inference_case(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    tf, tr = _named(*(open(os.path.join(d, f), "rb").read() for f in ("fwd.fq", "rve.fq")))
    df, dr = _damage(tf, 5), _damage(tr, 6)
    for f, data in (("df.fq", df), ("dr.fq", dr)):
        (tmp_path / f).write_bytes(data)

    def run(fwd, rve, out, flags):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(tmp_path / out) + "/",
                               "-f", str(tmp_path / fwd), "-r", str(tmp_path / rve), "-k", str(meta["k"])] + flags, cwd=ROOT, capture_output=True, text=True,
                              timeout=600)

    return df, dr, run


def test_pe_inference_on_the_damaged_pair_writes_the_files_of_the_filtered_pair(tmp_path):
    df, dr, run = _pe_inference_case(tmp_path)
    r1, r2, s1, s2 = pm.filtered(df, dr)
    assert s1 > 3 and s2 > 3
    for f, data in (("r1.fq", r1), ("r2.fq", r2)):
        (tmp_path / f).write_bytes(data)
    want = run("r1.fq", "r2.fq", "aln_filtered", [])
    got = run("df.fq", "dr.fq", "aln_names", ["--check-names", "--check-names-singles"])
    assert want.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    for rel in ("pe_info", "st_info"):
        assert _sha(tmp_path / "aln_names" / rel) == _sha(tmp_path / "aln_filtered" / rel)
    line = [l for l in got.stdout.splitlines() if l.startswith("Pairs joined by read name")]
    assert line == ["Pairs joined by read name: %d; records without a mate dropped: %d of %s, %d of %s"
                    % (len(im.records(r1)), s1, tmp_path / "df.fq", s2, tmp_path / "dr.fq")]


def test_pe_inference_without_the_singles_flag_stops_at_the_first_pair_that_is_none(tmp_path):
    df, dr, run = _pe_inference_case(tmp_path)
    strict = run("df.fq", "dr.fq", "aln_strict", ["--check-names"])
    bad = pm.strict(df, dr)[1]["first_bad"]
    assert strict.returncode != 0 and "ValueError" in strict.stderr and "pair %d is no pair of mates" % bad in strict.stderr
    assert not (tmp_path / "aln_strict" / "pe_info").exists() and not any(l.startswith("Number of processed reads") for l in strict.stdout.splitlines())


def test_cli_on_the_damaged_pair_writes_every_file_of_the_filtered_pair(tmp_path):
    from graph_case import Case

    inp = Case("two_strain_bubbles_k21").inputs(str(tmp_path), with_reads=True)
    tf, tr = _named(*(open(inp[f], "rb").read() for f in ("fwd", "rve")))
    df, dr = _damage(tf, 7), _damage(tr, 8)
    r1, r2, s1, s2 = pm.filtered(df, dr)
    for f, data in (("df.fq.gz", bz.bgzf(df)), ("dr.fq", dr), ("r1.fq", r1), ("r2.fq", r2)):
        (tmp_path / f).write_bytes(data)

    def run(fwd, rve, out, flags):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                               "-fwd", str(tmp_path / fwd), "-rve", str(tmp_path / rve)] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run("r1.fq", "r2.fq", tmp_path / "out_filtered", [])
    got = run("df.fq.gz", "dr.fq", tmp_path / "out_names", ["--check-names", "--check-names-singles"])
    assert plain.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    files = sorted(os.path.relpath(os.path.join(base, f), tmp_path / "out_filtered") for base, _, fs in os.walk(tmp_path / "out_filtered") for f in fs)
    assert {"strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"} <= set(files)
    for rel in files:
        if rel != "vstrains.log":  # (time stamps and paths)
            assert _sha(tmp_path / "out_names" / rel) == _sha(tmp_path / "out_filtered" / rel), rel
    log = (tmp_path / "out_names" / "vstrains.log").read_text()
    assert "%d records of %s and %d records of %s have no mate by name" % (s1, tmp_path / "df.fq.gz", s2, tmp_path / "dr.fq") in log


# ---- the block builder (block_builder_cases.py): what every streamed ingest checks alike ------------------------------------------
def test_over_long_sequence_line_of_file_2_is_refused(host, ctx, tmp_path):
    """a sequence line of 2^24 bytes in file 2, in a record whose number is not its pair's: file 2 has a record without a mate
    in front of it, so the builder's refusal has to go through the pair list for the record's number"""
    import block_builder_cases as bb

    fwd, rve = bb.edge_pairs(4)
    (tmp_path / "f.fq").write_bytes(bb.fastq(fwd[:3], [b"a", b"b", b"c"]))
    (tmp_path / "r.fq").write_bytes(bb.fastq([rve[3], rve[0]], [b"x", b"a"]) + bb.long_record(b"b") + bb.fastq([rve[2]], [b"c"]))
    fs = host.PairedNameStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, singles=True)
    bb.refused(fs, ValueError, "%s: record 2 has a sequence line of more than %d bytes" % (tmp_path / "r.fq", bb.LONG - 1))


def test_blocks_are_the_host_packers_at_the_edges_of_the_ends_kernel(host, ctx, tmp_path):
    import block_builder_cases as bb

    fwd, rve = bb.edge_pairs()
    names = [b"p%d" % i for i in range(len(fwd))]
    (tmp_path / "f.fq").write_bytes(bb.fastq(fwd, names))
    (tmp_path / "r.fq").write_bytes(bb.fastq(rve, names))
    bb.same_at_every_block_size(lambda n: host.PairedNameStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, block_pairs=n),
                                ctx.pack_pairs(fwd, rve), unpaired=False)
