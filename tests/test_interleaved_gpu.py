"""Interleaved FASTQ on the device: the kernels of one window (``vs_fastq_mates_text``) against the host twin and the plain
model of tests/interleaved_model.py on every constructed case; the stream (``pe.InterleavedStream``) against the mapped ingest
of the de-interleaved pair, block by block and in its counters, in every form the reader knows; the strict mode's refusal;
and the two drop-ins with the flags against the same command on the de-interleaved pair."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import bgzf_util as bz
import interleaved_model as im
import test_fastq_stream_gpu as sg
import test_interleaved_cpu as ic
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
@pytest.mark.parametrize("eof", [True, False], ids=["eof", "more_to_come"])
@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c[0])
def test_kernels_equal_the_host_twin_and_the_model(host, ctx, case, eof):
    name, text, pairs, singles = case
    dev = host.fastq_mates(text, eof, ctx, guard=64)  # (raises if a sentinel word around the pair list changed)
    twin = host.fastq_mates(text, eof)
    assert np.array_equal(dev[0], twin[0]) and dev[1] == twin[1]
    ic.check_mates(text, eof, dev)


# ---- the stream -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workload(host, ctx, tmp_path_factory):
    g, strict, mixed, tf, tr = ic.stream_workload()
    tmp = tmp_path_factory.mktemp("il_workload")
    (tmp / "f.fq").write_bytes(tf)
    (tmp / "r.fq").write_bytes(tr)
    want = sg._count(host, ctx, g, host.FastqPair(str(tmp / "f.fq"), str(tmp / "r.fq"), ctx), False)
    seqs = [[rec[1].decode() for rec in im.records(t)] for t in (tf, tr)]
    return dict(g=g, strict=strict, mixed=mixed, want=want, seqs=seqs, tmp=tmp)


class Checked:
    """a stream whose every block is compared, end by end and in order, with the sequences of the de-interleaved pair"""

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


@pytest.mark.parametrize("chunk", [61, 1000], ids=["chunk61", "chunk1000"])
@pytest.mark.parametrize("kind", ["strict", "mixed"])
def test_stream_equals_the_mapped_pair(host, ctx, workload, monkeypatch, kind, chunk):
    text = workload[kind]
    _, w_singles, _, n = im.pairing(text)
    path = workload["tmp"] / (kind + ".fq")
    path.write_bytes(text)
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    fs = Checked(host.InterleavedStream(str(path), ctx, block_pairs=173, singles=(kind == "mixed")), workload["seqs"])
    got = sg._count(host, ctx, workload["g"], fs, True)
    same_counters(got, workload["want"])
    assert got[3] == fs.pair == 2000 and fs.blocks >= 12
    assert fs.info["pairs"] == 2000 and fs.info["singles"] == len(w_singles) and fs.info["records"] == n
    assert fs.info["text_bytes"] == fs.info["file_bytes"] == len(text) and fs.info["flags"] == 16


def _drain(host, ctx, path, singles=False):
    fs = host.InterleavedStream(str(path), ctx, block_pairs=173, singles=singles)
    try:
        return sum(len(b.unpack()[1]) // 2 for b in fs)
    finally:
        fs.close()


@pytest.mark.parametrize("chunk", [61, 1000], ids=["chunk61", "chunk1000"])
def test_strict_stream_fails_at_the_first_single(host, ctx, workload, monkeypatch, chunk):
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    first = im.record(b"@single0 extra", 0)
    mixed = workload["mixed"]
    assert mixed.startswith(first)
    later = mixed[len(first):]  # (its first single lies behind six pairs)
    at_end = workload["strict"] + im.record(b"@tail_single x", 3)
    for name, text in (("first", mixed), ("later", later), ("at_end", at_end)):
        path = workload["tmp"] / ("strict_%s_%d.fq" % (name, chunk))
        path.write_bytes(text)
        with pytest.raises(ValueError) as err:
            im.deinterleave(text, False)
        record = int(str(err.value).split()[1])
        recs = im.records(text)
        assert record == {"first": 0, "later": 12, "at_end": 4000}[name]
        with pytest.raises(ValueError) as err:
            _drain(host, ctx, path)
        msg = str(err.value)
        assert str(path) in msg and "record %d " % record in msg and "--interleaved-singles" in msg
        assert '"%s"' % recs[record][0].decode() in msg
        assert ('"%s"' % recs[record + 1][0].decode() if record + 1 < len(recs) else "end of file") in msg
        assert _drain(host, ctx, path, singles=True) == 2000


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


def _utf8(text: bytes) -> bytes:
    """multi-byte characters in a comment, in both names of a pair, and in a single's name"""
    out = text.replace(b"@p7/1\n", "@p7/1 café 中\n".encode(), 1)
    out = out.replace(b"@p9/1\n", "@pé9/1\n".encode(), 1).replace(b"@p9/2\n", "@pé9/2\n".encode(), 1)
    out = out.replace(b"@single5 extra\n", "@singleß5 extra\n".encode(), 1)
    assert sum(out.count(s.encode()) for s in ("@p7/1 café 中\n", "@pé9/1\n", "@pé9/2\n", "@singleß5 extra\n")) == 4
    return out


FORMS = ["plain", "gzip", "gzip_members", "bgzf", "gzip_device", "fifo", "fifo_gzip", "crlf", "no_final_newline", "utf8"]


@pytest.mark.parametrize("form", FORMS)
def test_every_form_of_the_same_reads_counts_the_same(host, ctx, workload, tmp_path, monkeypatch, form):
    text = workload["mixed"]
    n_singles = len(im.pairing(text)[1])
    monkeypatch.setenv("VS_STREAM_CHUNK", "4093")
    data = {"plain": text, "gzip": gzip.compress(text), "gzip_members": gzip.compress(text[:70001]) + gzip.compress(text[70001:]),
            "bgzf": bz.bgzf(text, block=3000), "gzip_device": gzip.compress(text), "fifo": text, "fifo_gzip": gzip.compress(text),
            "crlf": text.replace(b"\n", b"\r\n"), "no_final_newline": text[:-1], "utf8": _utf8(text)}[form]
    if form == "gzip_device":
        monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    path = tmp_path / "reads.fq"
    path.write_bytes(data)
    if form.startswith("fifo"):
        with Fifo(tmp_path, data) as p:
            fs = Checked(host.InterleavedStream(p, ctx, block_pairs=173, singles=True), workload["seqs"])
            got = sg._count(host, ctx, workload["g"], fs, True)
    else:
        fs = Checked(host.InterleavedStream(str(path), ctx, block_pairs=173, singles=True), workload["seqs"])
        got = sg._count(host, ctx, workload["g"], fs, True)
    same_counters(got, workload["want"])
    info = fs.info
    assert info["pairs"] == 2000 and info["singles"] == n_singles and info["records"] == 4000 + n_singles
    assert info["file_bytes"] == len(data)
    assert info["flags"] & 3 == {"crlf": 1, "utf8": 2}.get(form, 0) and bool(info["flags"] & 4) == ("gzip" in form or form == "bgzf")
    if form not in ("crlf", "utf8"):
        assert info["text_bytes"] == len(text) - (form == "no_final_newline")


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------
def _as_samtools_writes(tf: bytes, tr: bytes) -> bytes:
    """the pairs of two FASTQ texts under one name per pair (alternately /1 /2 and a comment), singles among them"""
    out = []
    for which, t in enumerate((tf, tr)):
        recs = im.records(t)
        for k, rec in enumerate(recs):
            rec[0] = (b"@q%d/%d" % (k, which + 1)) if k % 2 else (b"@q%d %d:N:0:1" % (k, which + 1))
        out.append(b"".join(b"\n".join(rec) + b"\n" for rec in recs))
    return im.with_singles(out[0], out[1])


def _il_drop_in(d, meta, path, out, flags, stdin=None):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/", "-f", path, "-r", path,
                           "-k", str(meta["k"])] + flags, cwd=ROOT, stdin=stdin, capture_output=True, text=True, timeout=600)


def test_pe_inference_on_the_interleaved_file_writes_the_files_of_the_pair(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    tf, tr = (open(os.path.join(d, f), "rb").read() for f in ("fwd.fq", "rve.fq"))
    text = _as_samtools_writes(tf, tr)
    r1, r2, singles = im.deinterleave(text, True)
    assert len(singles) > 5 and [rec[1:] for rec in im.records(r1)] == [rec[1:] for rec in im.records(tf)]
    for f, data in (("il.fq", text), ("r1.fq", r1), ("r2.fq", r2)):
        (tmp_path / f).write_bytes(data)
    pair = sg._drop_in(d, meta, str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq"), tmp_path / "aln_pair")
    assert pair.returncode == 0, pair.stderr[-3000:]
    strip = lambda out, tag: [l.replace(tag, "X") for l in out.splitlines() if not l.startswith("Global time elapsed")]
    # as a file, and piped into /dev/stdin
    with open(tmp_path / "il.fq", "rb") as fh:
        runs = [("aln_file", _il_drop_in(d, meta, str(tmp_path / "il.fq"), tmp_path / "aln_file", ["--interleaved", "--interleaved-singles"])),
                ("aln_stdin", _il_drop_in(d, meta, "/dev/stdin", tmp_path / "aln_stdin", ["--interleaved", "--interleaved-singles"], stdin=fh))]
    for tag, got in runs:
        assert got.returncode == 0, got.stderr[-3000:]
        for rel in ("pe_info", "st_info"):
            assert (tmp_path / tag / rel).read_bytes() == (tmp_path / "aln_pair" / rel).read_bytes() == open(os.path.join(d, rel), "rb").read()
        assert strip(got.stdout, tag) == strip(pair.stdout, "aln_pair")
    # without --interleaved-singles the same input stops at its first unmated record, and nothing is written
    strict = _il_drop_in(d, meta, str(tmp_path / "il.fq"), tmp_path / "aln_strict", ["--interleaved"])
    assert strict.returncode != 0 and "ValueError" in strict.stderr and "record 0 " in strict.stderr and "@single0 extra" in strict.stderr
    assert not (tmp_path / "aln_strict" / "pe_info").exists() and not (tmp_path / "aln_strict" / "st_info").exists()
    assert not any(l.startswith("Number of processed reads") for l in strict.stdout.splitlines())


def test_cli_on_the_interleaved_file_writes_every_file_of_the_pair(tmp_path):
    from graph_case import Case

    inp = Case("two_strain_bubbles_k21").inputs(str(tmp_path), with_reads=True)
    tf, tr = (open(inp[f], "rb").read() for f in ("fwd", "rve"))
    text = _as_samtools_writes(tf, tr)
    r1, r2, _ = im.deinterleave(text, True)
    for f, data in (("il.fq.gz", bz.bgzf(text)), ("r1.fq", r1), ("r2.fq", r2)):
        (tmp_path / f).write_bytes(data)

    def run(fwd, rve, out, flags):
        return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                               "-fwd", fwd, "-rve", rve] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run(str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq"), tmp_path / "out_pair", [])
    got = run(str(tmp_path / "il.fq.gz"), str(tmp_path / "il.fq.gz"), tmp_path / "out_il", ["--interleaved", "--interleaved-singles"])
    assert plain.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    files = sorted(os.path.relpath(os.path.join(base, f), tmp_path / "out_pair") for base, _, fs in os.walk(tmp_path / "out_pair") for f in fs)
    assert {"strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"} <= set(files)
    for rel in files:
        if rel != "vstrains.log":  # (time stamps and paths)
            assert (tmp_path / "out_il" / rel).read_bytes() == (tmp_path / "out_pair" / rel).read_bytes(), rel
    assert "records of the interleaved FASTQ have no mate" in (tmp_path / "out_il" / "vstrains.log").read_text()


# ---- the block builder (block_builder_cases.py): what every streamed ingest checks alike ------------------------------------------
def test_over_long_sequence_line_of_a_second_record_is_refused(host, ctx, tmp_path):
    """a sequence line of 2^24 bytes in the second record of a pair: the builder's refusal names the record in file order"""
    import block_builder_cases as bb
    from vstrains_amd import _native as nat

    fwd, rve = bb.edge_pairs(3)
    path = tmp_path / "il.fq"
    path.write_bytes(bb.fastq([fwd[0], rve[0], fwd[1]], [b"p0", b"p0", b"p1"]) + bb.long_record(b"p1") + bb.fastq([fwd[2], rve[2]], [b"p2", b"p2"]))
    bb.refused(host.InterleavedStream(str(path), ctx), nat.NativeError,
               "%s: record 3 has a sequence line of more than %d bytes" % (path, bb.LONG - 1))


def test_blocks_are_the_host_packers_at_the_edges_of_the_ends_kernel(host, ctx, tmp_path):
    import block_builder_cases as bb

    fwd, rve = bb.edge_pairs()
    path = tmp_path / "il.fq"
    path.write_bytes(bb.fastq([s for pair in zip(fwd, rve) for s in pair], [b"p%d" % (i // 2) for i in range(2 * len(fwd))]))
    bb.same_at_every_block_size(lambda n: host.InterleavedStream(str(path), ctx, block_pairs=n), ctx.pack_pairs(fwd, rve), unpaired=False)
