"""BAM input on the device: the chain kernels (vs_bam_scan_text) against the host twin and the pure-Python reader on the
constructed files of tests/bam_util.py, and the stream (pe.BamStream, the drop-ins) against the FASTQ pair the BAM stands
for (``bam_util.fastq_pair``) through code that knows nothing of BAM: the mapped ingest, and the drop-ins on the pair."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_util as bu
import bgzf_util as bz
import test_bam_cpu as bc
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


# ---- the kernels ----------------------------------------------------------------------------------------------------------
FILES = [(n, d) for n, d in bu.constructed()] + [(n, d) for n, d, _ in bu.malformed()]


@pytest.mark.parametrize("seg", [64, 0], ids=["seg64", "default"])
@pytest.mark.parametrize("case", FILES, ids=lambda c: c[0])
def test_kernels_equal_the_host_twin(host, ctx, case, seg):
    name, data = case
    skip = bu.header_len(data)
    dev = host.bam_scan(data, skip, seg, ctx)
    twin = host.bam_scan(data, skip, seg)
    assert np.array_equal(dev[0], twin[0]) and np.array_equal(dev[1], twin[1]) and dev[2] == twin[2]
    bc.check_scan(data, dev)


def test_kernels_on_a_window_cut_at_many_lengths(host, ctx):
    name, data = bu.constructed()[0]
    start = bu.header_len(data)
    starts = [t[0] for t in bu.walk(data)[0]]
    for n in (start, start + 3, start + 4, starts[3] + 2, starts[5] - 1, starts[5], len(data) - 1):
        bc.check_scan(data[:n], host.bam_scan(data[:n], start, 64, ctx), start)


# ---- the stream -----------------------------------------------------------------------------------------------------------
def _workload():
    """about 300 nodes, about 2 000 pairs of lengths 30-160 with N and IUPAC codes, reversed ends, either order of the mates,
    and records that are dropped in between"""
    from vstrains_amd import synth

    st = synth.make_strains(10, 2500, 0.03, seed=31)
    g = synth.compact_dbg(st, 21)
    f, r = synth.sample_pairs(st, 2000, 160, seed=32, sub_rate=0.01, n_rate=0.01)
    rng = np.random.default_rng(33)
    comp = str.maketrans("ACGTN", "TGCAN")
    records = []
    for i, (a, b) in enumerate(zip(f, r)):
        ends = []
        for which, s in ((bu.FIRST, a), (bu.SECOND, b)):
            s = s[:int(rng.integers(30, 161))]
            if i % 50 == 7:
                s = s[:10] + "RYKM"[i % 4] + s[11:]  # an IUPAC code: the end counts as invalid there
            flag = bu.PAIRED | which
            if rng.integers(0, 2):
                flag |= bu.REVERSE  # stored reversed: the FASTQ shows the read as sequenced
                s = s.translate(comp)[::-1] if set(s) <= set("ACGTN") else "".join(bu.COMPLEMENT[c] for c in reversed(s))
            qual = bytes(int(x) for x in rng.integers(0, 94, size=len(s)))
            ends.append(bu.rec("p%d" % i, flag, s, qual=qual, aux=b"RGZgrp\0" if i % 3 else b""))
        if rng.integers(0, 2):
            ends.reverse()
        records.append(ends[0])
        if i % 40 == 3:
            records.append(bu.rec("p%d" % i, bu.PAIRED | bu.FIRST | bu.SUPPLEMENTARY, "ACGT" * 9))
        if i % 60 == 5:
            records.append(bu.rec("s%d" % i, bu.PAIRED | bu.SECOND | bu.SECONDARY | bu.REVERSE, "TTGCA" * 7))
        if i % 70 == 9:
            records.append(bu.rec("u%d" % i, 0x4, "ACGTT" * 12))  # an unpaired read: other
        records.append(ends[1])
    return g, records


@pytest.fixture(scope="module")
def workload(host, ctx, tmp_path_factory):
    g, records = _workload()
    tmp = tmp_path_factory.mktemp("bam_workload")
    tf, tr = bu.fastq_pair(records)
    (tmp / "f.fq").write_bytes(tf)
    (tmp / "r.fq").write_bytes(tr)
    want = sg._count(host, ctx, g, host.FastqPair(str(tmp / "f.fq"), str(tmp / "r.fq"), ctx), False)
    bam = tmp / "reads.bam"
    bam.write_bytes(bu.write(records, block=4000))  # (small members: records and size fields across members and chunks)
    seqs = [[l for l in t.decode().split("\n")[1::4]] for t in (tf, tr)]
    return dict(g=g, records=records, want=want, bam=str(bam), seqs=seqs, n_nodes=len(g.seqs))


@pytest.mark.parametrize("seg", [None, 64], ids=["seg_default", "seg64"])
@pytest.mark.parametrize("chunk", [None, 61, 1000], ids=["chunk_default", "chunk61", "chunk1000"])
def test_stream_equals_the_mapped_fastq_pair(host, ctx, workload, monkeypatch, chunk, seg):
    from vstrains_amd import pe_inference

    assert 250 <= workload["n_nodes"] <= 350 and workload["want"][3] == 2000
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    if seg is not None:
        monkeypatch.setenv("VS_BAM_SEG", str(seg))
    # the blocks themselves: lengths, flags and the ACGT text of every end
    fs = host.BamStream(workload["bam"], ctx, block_pairs=173)
    pair, blocks = 0, 0
    try:
        for block in fs:
            text, lens, flags = block.unpack()
            block.free()
            at = 0
            for e in range(len(lens)):
                want = workload["seqs"][e & 1][pair + (e >> 1)]
                assert lens[e] == len(want), (pair, e)
                assert flags[e] & 3 == (1 if "N" in want else 0) | (2 if set(want) - set("ACGTN") else 0), (pair, e)
                got = bytes(text[at:at + lens[e]]).decode()
                assert got == "".join(c if c in "ACGT" else "A" for c in want), (pair, e)
                at += int(lens[e])
            pair += len(lens) // 2
            blocks += 1
        info = fs.info
    finally:
        fs.close()
    flags_all = [r.flag for r in workload["records"]]
    assert pair == 2000 and info["pairs"] == 2000 and info["done"]
    assert blocks == 12 if chunk is None else blocks > 12  # (a block never waits for the next chunk)
    assert info["records"] == len(flags_all)
    assert info["dropped_0x900"] == sum(bu.classify(f) == bu.C_DROP900 for f in flags_all) > 0
    assert info["dropped_other"] == sum(bu.classify(f) == bu.C_OTHER for f in flags_all) > 0
    assert info["members_device"] > 100 and info["text_bytes"] == len(bu.inflated(workload["records"]))
    # the counters
    fs = host.BamStream(workload["bam"], ctx, block_pairs=173)
    got = sg._count(host, ctx, workload["g"], fs, True)
    want = workload["want"]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3]


def test_a_header_larger_than_many_windows_and_no_eof_marker(host, ctx, tmp_path, monkeypatch):
    refs = [(b"chr%d" % i, 1000 + i) for i in range(3000)]
    text = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    records = [bu.rec("a", 0x41, "ACGTN"), bu.rec("a", 0x81 | 0x10, "AACC"), bu.rec("b", 0x81, ""), bu.rec("b", 0x41, "T")]
    p = tmp_path / "h.bam"
    p.write_bytes(bu.write(records, text, refs, block=3000, eof=False))
    monkeypatch.setenv("VS_STREAM_CHUNK", "1000")
    fs = host.BamStream(str(p), ctx)
    try:
        blocks = [b.unpack() for b in fs]
        assert fs.info["pairs"] == 2 and fs.info["records"] == 4
    finally:
        fs.close()
    assert [int(x) for b in blocks for x in b[1]] == [5, 4, 1, 0]
    assert bytes(np.concatenate([b[0] for b in blocks])) == b"ACGTA" + b"GGTT" + b"T"


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------
def _records_of_pair(tf: bytes, tr: bytes):
    rng = np.random.default_rng(5)
    fs, rs = tf.decode().split("\n")[1::4], tr.decode().split("\n")[1::4]
    assert len(fs) == len(rs)
    out = []
    for i, (a, b) in enumerate(zip(fs, rs)):
        ends = []
        for which, s in ((bu.FIRST, a), (bu.SECOND, b)):
            flag = bu.PAIRED | which | 0xC  # (unmapped, mate unmapped: samtools view -f 12)
            if rng.integers(0, 2) and set(s) <= set("ACGTN"):
                flag |= bu.REVERSE
                s = s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]
            ends.append(bu.rec("q%d" % i, flag, s))
        if i % 2:
            ends.reverse()
        out += ends[:1] + ([bu.rec("q%d" % i, 0x900 | 0x41, "ACGT")] if i % 9 == 0 else []) + ends[1:]
    return out


def test_pe_inference_on_the_bam_writes_the_files_of_the_pair(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]  # (reads in upper case: BAM has no lower-case bases)
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    records = _records_of_pair(tf, tr)
    assert [t.decode().split("\n")[1::4] for t in bu.fastq_pair(records)] == [t.decode().split("\n")[1::4] for t in (tf, tr)]
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(records, block=5000))
    pair = sg._drop_in(d, meta, os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq"), tmp_path / "aln_pair")
    got = sg._drop_in(d, meta, str(bam), str(bam), tmp_path / "aln_bam", env=dict(os.environ, VS_STREAM_CHUNK="7000"))
    assert pair.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    for rel in ("pe_info", "st_info"):
        assert (tmp_path / "aln_bam" / rel).read_bytes() == (tmp_path / "aln_pair" / rel).read_bytes() == open(os.path.join(d, rel), "rb").read()
    strip = lambda out, tag: [l.replace(tag, "X") for l in out.splitlines() if not l.startswith("Global time elapsed")]
    assert strip(got.stdout, "aln_bam") == strip(pair.stdout, "aln_pair")


def test_cli_on_the_bam_writes_the_same_strains(tmp_path):
    from graph_case import Case

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    with open(inp["fwd"], "rb") as fh:
        tf = fh.read()
    with open(inp["rve"], "rb") as fh:
        tr = fh.read()
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(_records_of_pair(tf, tr)))

    def run(fwd, rve, out):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                               "-fwd", fwd, "-rve", rve], cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run(inp["fwd"], inp["rve"], tmp_path / "out_pair")
    got = run(str(bam), str(bam), tmp_path / "out_bam")
    assert plain.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    for rel in ("strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"):
        assert (tmp_path / "out_pair" / rel).exists(), rel
        assert (tmp_path / "out_bam" / rel).read_bytes() == (tmp_path / "out_pair" / rel).read_bytes(), rel


# ---- errors ---------------------------------------------------------------------------------------------------------------
def _drain(host, ctx, path):
    fs = host.BamStream(str(path), ctx, block_pairs=2)
    try:
        return sum(len(b.unpack()[1]) // 2 for b in fs)
    finally:
        fs.close()


@pytest.mark.parametrize("case", bu.malformed(), ids=lambda c: c[0])
def test_errors_from_the_stream_name_the_record(host, ctx, tmp_path, monkeypatch, case):
    name, data, (what, record) = case
    monkeypatch.setenv("VS_STREAM_CHUNK", "300")
    p = tmp_path / (name + ".bam")
    p.write_bytes(bz.bgzf(data, block=300))
    words = {"dead": "malformed", "malformed": "malformed", "bad_couple": "not collated", "odd": "not collated", "cut": "truncated record"}[what]
    with pytest.raises(ValueError, match=r"record %d\b.*%s" % (record, words)) as ei:
        _drain(host, ctx, p)
    if words == "not collated":
        assert "samtools collate" in str(ei.value)
    # the context and the device are fine afterwards
    good = tmp_path / "good.bam"
    good.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    assert _drain(host, ctx, good) == 1


def test_what_is_out_of_scope_is_refused_in_words(host, ctx, tmp_path):
    recs = [bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]
    bam = bu.write(recs)
    with sg.Fifos(tmp_path, bam, bam) as (pf, pr):
        with pytest.raises(ValueError, match="FIFO"):
            host.BamStream(pf, ctx)
    fq = tmp_path / "r.fq.gz"
    fq.write_bytes(bz.bgzf(bz.fastq_text(3)))
    with pytest.raises(ValueError, match="not a BAM"):
        host.BamStream(str(fq), ctx)
    with pytest.raises(FileNotFoundError):
        host.BamStream(str(tmp_path / "missing.bam"), ctx)
    a, b = tmp_path / "a.bam", tmp_path / "b.bam"
    a.write_bytes(bam)
    b.write_bytes(bam)
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    for fwd, rve, words in ((str(a), str(fq), "one side only"), (str(a), str(b), "two different BAM")):
        proc = sg._drop_in(d, meta, fwd, rve, tmp_path / "aln")
        assert proc.returncode != 0 and sg._exception_line(proc.stderr).startswith("ValueError") and words in proc.stderr
    # a damaged member: the CRC32 check of the device
    raw = bytearray(bu.write([bu.rec("r%d" % i, 0x41 if i % 2 == 0 else 0x81, "ACGT" * 30) for i in range(40)], block=900, level=0))
    raw[len(raw) // 2] ^= 0x55
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="not a complete gzip stream"):
        _drain(host, ctx, bad)


# ---- the block builder (block_builder_cases.py): what every streamed ingest checks alike ------------------------------------------
def test_over_long_sequence_is_refused_by_its_pair(host, ctx, tmp_path):
    """l_seq = 2^24 in the second record of pair 1: the builder's refusal, worded with the pair"""
    import block_builder_cases as bb
    from vstrains_amd import _native as nat

    good = [bu.rec("g0", bu.PAIRED | bu.FIRST, "ACGTACGTAC"), bu.rec("g0", bu.PAIRED | bu.SECOND, "TTGCA"), bu.rec("g1", bu.PAIRED | bu.FIRST, "GATTACA")]
    path = tmp_path / "long.bam"
    path.write_bytes(bz.bgzf(bu.inflated(good) + bb.long_bam_record(b"g1", bu.PAIRED | bu.SECOND), 1))
    bb.refused(host.BamStream(str(path), ctx), nat.NativeError, "%s: pair 1 has a sequence of more than %d bases" % (path, bb.LONG - 1))


def test_blocks_are_the_host_packers_at_the_edges_of_the_ends_kernel(host, ctx, tmp_path):
    import block_builder_cases as bb

    fwd, rve = bb.edge_pairs(other="M")  # (a base that is neither ACGT nor N has a 4-bit code of its own)
    records = [r for i, (a, b) in enumerate(zip(fwd, rve)) for r in (bu.rec("p%d" % i, bu.PAIRED | bu.FIRST, a), bu.rec("p%d" % i, bu.PAIRED | bu.SECOND, b))]
    path = tmp_path / "edges.bam"
    path.write_bytes(bu.write(records))
    bb.same_at_every_block_size(lambda n: host.BamStream(str(path), ctx, block_pairs=n), ctx.pack_pairs(fwd, rve), unpaired=False)
