"""Unpaired reads from files: the one-file stream (``pe.SingleEndStream`` = ``vs_fastq_se_*``) in every form the reader knows
against ``Context.pack_singles`` of the same reads; the interleaved stream that KEEPS its single records
(``InterleavedStream(singles="keep")``) against the one that drops them plus the model of the singles; and the two commands
with ``--single`` / ``--count-singles``."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import bgzf_util as bz
import unpaired_model
from conftest import ROOT, pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu

K = 21


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe

    return pe


def _fastq(reads, tag=b"s") -> bytes:
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s.encode(), b"I" * len(s)) for i, s in enumerate(reads))


@pytest.fixture(scope="module")
def workload(host):
    """graph, a few thousand unpaired reads (some with N, short, empty, with invalid bytes), their counters by pack_singles"""
    from vstrains_amd import synth

    st = synth.make_strains(3, 1500, 0.03, seed=51)
    g = synth.compact_dbg(st, K)
    fwd, rve = synth.sample_pairs(st, 1100, 100, seed=52, sub_rate=0.005, n_rate=0.02)
    reads = [s for pair in zip(fwd, rve) for s in pair]
    reads[3] = reads[3][:K]          # shorter than k+1
    reads[4] = reads[4][:K + 1]
    reads[10] = ""                   # an empty sequence line
    reads[11] = reads[11][:40] + "x" + reads[11][41:]
    reads[12] = "*" + reads[12][1:5] + "nnRY" + reads[12][9:]  # five invalid bytes
    reads[-1] = reads[-1][:60] + "N" + reads[-1][61:]
    ctx = host.Context(0)
    ctx.build_index(g.seqs, K)
    model = unpaired_model.Model(g.seqs, K)
    want = _counters(host, ctx, [ctx.pack_singles(reads)])
    assert want[1].sum() > 0 and min(want[3]) > 0 and not want[0].any() and want[2] == (0, 0, 0)
    assert np.array_equal(want[1], model.count(reads)[1]) and want[3] == model.count(reads)[2]
    yield dict(g=g, reads=reads, ctx=ctx, want=want, model=model, text=_fastq(reads))
    ctx.close()


def _counters(host, ctx, blocks):
    counter = host.PeCounter(ctx)
    for b in blocks:
        counter.add(b)
    node_mat, short_mat, stats = counter.result()
    return node_mat, short_mat, stats, tuple(int(x) for x in counter.single_stats.cpu().numpy())


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3]


class Fifo:
    """one FIFO fed by a writer thread"""

    def __init__(self, tmp, data: bytes):
        self.path, self.data = str(tmp / "reads.fifo"), data
        os.mkfifo(self.path)
        self.thread = threading.Thread(target=self._write, daemon=True)

    def _write(self):
        try:
            with open(self.path, "wb") as fh:
                fh.write(self.data)
        except BrokenPipeError:
            pass

    def __enter__(self):
        self.thread.start()
        return self.path

    def __exit__(self, *exc):
        self.thread.join(timeout=30)
        os.unlink(self.path)


def _stream_blocks(host, ctx, path, block_reads, reads):
    """the stream's blocks, each checked read by read against ``reads`` as it comes; (blocks, info)"""
    fs = host.SingleEndStream(path, ctx, block_reads=block_reads)
    blocks, at = [], 0
    try:
        for b in fs:
            assert b.unpaired
            text, lens, flags = b.unpack()
            assert len(lens) % 2 == 0 and len(lens) // 2 <= block_reads and not lens[1::2].any() and all(int(f) == 8 for f in flags[1::2])
            pos = 0
            for r in range(len(lens) // 2):
                want = reads[at + r]
                assert lens[2 * r] == len(want), (at + r)
                assert flags[2 * r] & 3 == (1 if "N" in want else 0) | (2 if set(want) - set("ACGTN") else 0), (at + r)
                assert bytes(text[pos:pos + len(want)]).decode() == "".join(c if c in "ACGT" else "A" for c in want), (at + r)
                pos += len(want)
            at += len(lens) // 2
            blocks.append(b)
        info = fs.info
    finally:
        fs.close()
    assert at == len(reads)
    return blocks, info


FORMS = ["plain", "gzip", "bgzf", "fifo", "no_final_newline", "crlf", "trailing_partial_record"]


@pytest.mark.parametrize("block_reads", [7, 1000])
@pytest.mark.parametrize("chunk", [61, 1000, 4093])
@pytest.mark.parametrize("form", FORMS)
def test_every_form_counts_as_pack_single(host, workload, tmp_path, monkeypatch, form, chunk, block_reads):
    text, reads, ctx = workload["text"], workload["reads"], workload["ctx"]
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    data = {"plain": text, "gzip": gzip.compress(text), "bgzf": bz.bgzf(text, block=3000), "fifo": text, "no_final_newline": text[:-1],
            "crlf": text.replace(b"\n", b"\r\n"), "trailing_partial_record": text + b"@cut\nACGTACGT\n+\n"}[form]
    if form == "fifo":
        with Fifo(tmp_path, data) as p:
            blocks, info = _stream_blocks(host, ctx, p, block_reads, reads)
    else:
        path = tmp_path / ("reads.fq.gz" if form in ("gzip", "bgzf") else "reads.fq")
        path.write_bytes(data)
        blocks, info = _stream_blocks(host, ctx, str(path), block_reads, reads)
    assert len(blocks) >= len(reads) // block_reads
    _same(_counters(host, ctx, blocks), workload["want"])
    assert info["reads"] == info["records"] == len(reads) and info["file_bytes"] == len(data)
    assert info["flags"] & 3 == (1 if form == "crlf" else 0) and bool(info["flags"] & 4) == (form in ("gzip", "bgzf")) and info["flags"] & 16


def test_plain_gzip_on_the_device(host, workload, tmp_path, monkeypatch):
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    monkeypatch.setenv("VS_STREAM_CHUNK", "4093")
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(gzip.compress(workload["text"]))
    blocks, info = _stream_blocks(host, workload["ctx"], str(path), 1000, workload["reads"])
    _same(_counters(host, workload["ctx"], blocks), workload["want"])


def test_empty_file_gives_no_block(host, workload, tmp_path):
    for name, data in (("empty.fq", b""), ("three_lines.fq", b"@a\nACGT\n+\n")):
        path = tmp_path / name
        path.write_bytes(data)
        fs = host.SingleEndStream(str(path), workload["ctx"])
        assert list(fs) == [] and fs.info["reads"] == 0 and fs.next_block() is None
        fs.close()
    with pytest.raises(FileNotFoundError):
        host.SingleEndStream(str(tmp_path / "missing.fq"), workload["ctx"])


def test_over_long_sequence_line_is_refused(host, workload, tmp_path):
    """a sequence line of 2^24 bytes: one more than a read end's length field holds; named by its record number"""
    from vstrains_amd import _native as nat

    path = tmp_path / "long.fq"
    n = 1 << 24
    with open(path, "wb") as fh:
        fh.write(_fastq(workload["reads"][:2]))
        fh.write(b"@long\n" + b"A" * n + b"\n+\n" + b"I" * n + b"\n")
    fs = host.SingleEndStream(str(path), workload["ctx"])
    with pytest.raises(nat.NativeError) as err:
        list(fs)
    fs.close()
    assert err.value.code == nat.VS_E_RANGE
    assert "%s: record 2 has a sequence line of more than %d bytes" % (path, (1 << 24) - 1) in str(err.value)


# ---- the interleaved stream keeps its singles -----------------------------------------------------------------------------------
def _mixed(workload, held_at_end=False):
    """(text, the single reads in file order): the pairs of the workload's first 1000 reads under one name per pair, single
    records -- real reads of the rest, the dropped kinds among them -- between them: at record 0, two adjacent ones, one
    behind every 23rd pair, one at the end"""
    reads = workload["reads"]
    pairs = [(reads[2 * p], reads[2 * p + 1]) for p in range(500)]
    # (the kinds rules 1 and 2 drop come first: a read with an N, one of k bases, an empty sequence line)
    spare = iter([reads[-1], reads[3], reads[10]] + reads[1000:-1])
    out, singles = [], []

    def single():
        s = next(spare)
        singles.append(s)
        out.append(b"@lone%d extra\n%s\n+\n%s\n" % (len(singles), s.encode(), b"I" * len(s)))

    single()
    for p, (a, b) in enumerate(pairs):
        for which, s in enumerate((a, b)):
            out.append((b"@q%d/%d" % (p, which + 1) if p % 2 else b"@q%d %d:N:0:1" % (p, which + 1)) + b"\n%s\n+\n%s\n" % (s.encode(), b"I" * len(s)))
        if p % 23 == 5:
            single()
        if p == 50:
            single()
            single()
    if held_at_end:
        single()
    return b"".join(out), singles


@pytest.mark.parametrize("held_at_end", [False, True], ids=["ends_in_a_pair", "ends_in_a_held_back_single"])
@pytest.mark.parametrize("chunk", [61, 1000])
def test_interleaved_keep(host, workload, tmp_path, monkeypatch, chunk, held_at_end):
    ctx, model = workload["ctx"], workload["model"]
    text, singles = _mixed(workload, held_at_end)
    assert len(singles) > 20 and text.endswith(b"I\n")
    path = tmp_path / "mixed.fq"
    path.write_bytes(text)
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))

    def run(mode):
        fs = host.InterleavedStream(str(path), ctx, block_pairs=173, singles=mode)
        try:
            blocks = list(fs)
            return blocks, fs.info
        finally:
            fs.close()

    dropped, info_drop = run(True)
    kept, info_keep = run("keep")
    assert info_keep == info_drop and info_keep["singles"] == len(singles) and info_keep["pairs"] == 500
    assert not any(b.unpaired for b in dropped)
    # the kept singles come in file order, as singles blocks
    got = []
    for b in kept:
        if b.unpaired:
            _, lens, _ = b.unpack()
            got += [int(x) for x in lens[0::2]]
    assert got == [len(s) for s in singles]
    want = _counters(host, ctx, dropped)
    m_node, m_short, m_tally = model.count(singles)
    assert m_short.sum() > 0 and m_tally[0] > 0
    have = _counters(host, ctx, kept)
    assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1] + m_short)
    assert have[2] == want[2] and want[3] == (0, 0, 0) and have[3] == m_tally


# ---- the commands ------------------------------------------------------------------------------------------------------------
def _case():
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    f = pe_oracle.fastq_sequences(os.path.join(d, "fwd.fq"))
    r = pe_oracle.fastq_sequences(os.path.join(d, "rve.fq"))
    return d, meta, ids, seqs, f, r


def _pe_inference(d, meta, fwd, rve, out, flags):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/", "-f", fwd, "-r", rve,
                           "-k", str(meta["k"])] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _strip(out, tag):
    return [l.replace(tag, "X") for l in out.splitlines() if not l.startswith("Global time elapsed")]


def test_pe_inference_single(tmp_path):
    d, meta, ids, seqs, f, r = _case()
    # the unpaired reads: ends of the case's own pairs, some dropped kinds among them, in two files (one of them BGZF)
    s1 = f[0:120:3] + [f[1][:meta["k"]], f[2][:30] + "N" + f[2][31:]]
    s2 = r[1:90:4] + [""]
    (tmp_path / "s1.fq").write_bytes(_fastq(s1))
    (tmp_path / "s2.fq.gz").write_bytes(bz.bgzf(_fastq(s2), block=2000))
    fwd, rve = os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq")
    plain = _pe_inference(d, meta, fwd, rve, tmp_path / "aln_pair", [])
    got = _pe_inference(d, meta, fwd, rve, tmp_path / "aln_single", ["--single", str(tmp_path / "s1.fq"), "--single", str(tmp_path / "s2.fq.gz")])
    assert plain.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    assert (tmp_path / "aln_single" / "pe_info").read_bytes() == (tmp_path / "aln_pair" / "pe_info").read_bytes() == open(os.path.join(d, "pe_info"), "rb").read()
    model = unpaired_model.Model(seqs, meta["k"])
    _, pair_short, _ = pe_oracle.pe_matrices(seqs, f, r, meta["k"], table=model.table)
    _, m1, t1 = model.count(s1)
    _, m2, t2 = model.count(s2)
    assert m1.sum() > 0 and m2.sum() > 0
    assert (tmp_path / "aln_single" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short + m1 + m2)
    lines = _strip(got.stdout, "aln_single")
    extra = ["Unpaired reads of %s: %d used, %d with N, %d shorter than k+1" % (p, t[2], t[0], t[1])
             for p, t in ((tmp_path / "s1.fq", t1), (tmp_path / "s2.fq.gz", t2))]
    assert [l for l in lines if l not in extra] == _strip(plain.stdout, "aln_pair") and all(l in lines for l in extra)
    # (works with the other writers unchanged: the flags only reach the counters)
    sparse = _pe_inference(d, meta, fwd, rve, tmp_path / "aln_sparse", ["--single", str(tmp_path / "s1.fq"), "--sparse-info"])
    assert sparse.returncode == 0, sparse.stderr[-3000:]
    dense = pe_oracle.matrix_text(ids, pair_short + m1)
    assert (tmp_path / "aln_sparse" / "st_info").read_text() == "".join(l for l in dense.splitlines(keepends=True) if not l.endswith(":0\n"))


def test_pe_inference_count_singles(tmp_path):
    d, meta, ids, seqs, f, r = _case()
    n = min(len(f), len(r))
    singles, out = [], []
    spare = iter(f[5:200:7] + [r[3][:meta["k"]]])
    for p in range(n):
        for which, s in enumerate((f[p], r[p])):
            out.append(b"@q%d/%d\n%s\n+\n%s\n" % (p, which + 1, s.encode(), b"I" * len(s)))
        if p % 11 == 2:
            s = next(spare, None)
            if s is not None:
                singles.append(s)
                out.append(b"@lone%d\n%s\n+\n%s\n" % (p, s.encode(), b"I" * len(s)))
    assert len(singles) > 10
    il = tmp_path / "il.fq"
    il.write_bytes(b"".join(out))
    drop = _pe_inference(d, meta, str(il), str(il), tmp_path / "aln_drop", ["--interleaved", "--interleaved-singles"])
    got = _pe_inference(d, meta, str(il), str(il), tmp_path / "aln_keep", ["--interleaved", "--interleaved-singles", "--count-singles"])
    assert drop.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    assert (tmp_path / "aln_keep" / "pe_info").read_bytes() == (tmp_path / "aln_drop" / "pe_info").read_bytes() == open(os.path.join(d, "pe_info"), "rb").read()
    model = unpaired_model.Model(seqs, meta["k"])
    _, pair_short, _ = pe_oracle.pe_matrices(seqs, f, r, meta["k"], table=model.table)
    _, m, t = model.count(singles)
    assert m.sum() > 0
    assert (tmp_path / "aln_keep" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short + m)
    line = "Unpaired reads of %s: %d used, %d with N, %d shorter than k+1" % (il, t[2], t[0], t[1])
    lines = _strip(got.stdout, "aln_keep")
    assert line in lines and [l for l in lines if l != line] == _strip(drop.stdout, "aln_drop")


def test_cli_single(tmp_path):
    from graph_case import Case

    inp = Case("two_strain_bubbles_k21").inputs(str(tmp_path), with_reads=True)
    f = pe_oracle.fastq_sequences(inp["fwd"])
    (tmp_path / "single.fq").write_bytes(_fastq(f[0:200:3]))
    (tmp_path / "empty.fq").write_bytes(b"")

    def run(out, flags):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                               "-fwd", inp["fwd"], "-rve", inp["rve"]] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run(tmp_path / "out_pair", [])
    empty = run(tmp_path / "out_empty", ["--single", str(tmp_path / "empty.fq")])
    got = run(tmp_path / "out_single", ["--single", str(tmp_path / "single.fq")])
    assert plain.returncode == 0 and empty.returncode == 0 and got.returncode == 0, (empty.stderr[-2000:], got.stderr[-2000:])
    files = sorted(os.path.relpath(os.path.join(base, f_), tmp_path / "out_pair") for base, _, fs in os.walk(tmp_path / "out_pair") for f_ in fs)
    assert {"strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"} <= set(files)
    for rel in files:
        if rel != "vstrains.log":  # (time stamps and paths)
            assert (tmp_path / "out_empty" / rel).read_bytes() == (tmp_path / "out_pair" / rel).read_bytes(), rel
    # with reads in the file: runs to strain.fasta; pe_info as without, st_info grown
    assert (tmp_path / "out_single" / "strain.fasta").stat().st_size > 0
    assert (tmp_path / "out_single" / "aln" / "pe_info").read_bytes() == (tmp_path / "out_pair" / "aln" / "pe_info").read_bytes()
    assert (tmp_path / "out_single" / "aln" / "st_info").read_bytes() != (tmp_path / "out_pair" / "aln" / "st_info").read_bytes()
    assert "Unpaired reads of %s: " % (tmp_path / "single.fq") in got.stdout
    assert "Unpaired reads of %s: 0 used, 0 with N, 0 shorter than k+1" % (tmp_path / "empty.fq") in empty.stdout


# ---- the block builder (block_builder_cases.py): what every streamed ingest checks alike ------------------------------------------
def test_blocks_are_the_host_packers_at_the_edges_of_the_ends_kernel(host, workload, tmp_path):
    import block_builder_cases as bb

    reads = [s for pair in zip(*bb.edge_pairs()) for s in pair]
    path = tmp_path / "se.fq"
    path.write_bytes(_fastq(reads))
    ctx = workload["ctx"]
    bb.same_at_every_block_size(lambda n: host.SingleEndStream(str(path), ctx, block_reads=n), ctx.pack_singles(reads), unpaired=True)
