"""The streamed FASTQ ingest (vs_fastq_stream_*, pe.FastqStream): pipes and gzip read once, records found and packed on the
device.  Its counters must be the mapped ingest's, bit for bit, and the drop-ins must take FIFOs."""
import gzip
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, pe_cases

pytestmark = pytest.mark.gpu

TINY_CHUNKS = (61, 1000)  # bytes: records, lines and "\r\n" across chunk boundaries at many offsets


def _read(path):
    with open(path, "r", newline="") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


class Fifos:
    """Two FIFOs, a writer thread per FIFO; on exit a writer still waiting for its reader is released."""

    def __init__(self, tmp, data_f: bytes, data_r: bytes, names=("fwd.fifo", "rve.fifo")):
        self.paths = [os.path.join(str(tmp), n) for n in names]
        self.threads = []
        for path, data in zip(self.paths, (data_f, data_r)):
            os.mkfifo(path)
            t = threading.Thread(target=self._write, args=(path, data), daemon=True)
            t.start()
            self.threads.append(t)

    @staticmethod
    def _write(path, data):
        try:
            with open(path, "wb") as fh:
                for i in range(0, len(data), 1 << 16):
                    fh.write(data[i:i + (1 << 16)])
        except (BrokenPipeError, OSError):
            pass

    def __enter__(self):
        return self.paths

    def __exit__(self, *exc):
        for path, t in zip(self.paths, self.threads):
            t.join(timeout=0.5)
            if t.is_alive():  # (nobody opened it: open the reading end and drain, so that the writer finishes)
                fd = os.open(path, os.O_RDONLY | os.O_NONBLOCK)
                try:
                    while t.is_alive():
                        try:
                            if not os.read(fd, 1 << 16):
                                t.join(timeout=0.1)
                        except BlockingIOError:
                            t.join(timeout=0.05)
                finally:
                    os.close(fd)
            t.join(timeout=5)
        return False


def _synth_reads(n_pairs, seed):
    from vstrains_amd import synth

    st = synth.make_strains(5, 1500, 0.03, seed=seed)
    g = synth.compact_dbg(st, 21)
    f, r = synth.sample_pairs(st, n_pairs, 100, seed=seed + 1, sub_rate=0.01, n_rate=0.03)
    return g, f, r


def _variant(kind, f, r):
    """(fwd bytes, rve bytes) of one input shape"""
    from vstrains_amd import synth

    rng = np.random.default_rng(len(kind))
    if kind == "odd_bytes":  # N, other ASCII bytes, valid multi-byte UTF-8 in sequence lines
        f, r = list(f), list(r)
        for lst in (f, r):
            for i in rng.choice(len(lst), size=len(lst) // 5, replace=False):
                s_ = lst[int(i)]
                p_ = int(rng.integers(0, len(s_)))
                lst[int(i)] = s_[:p_] + str(rng.choice(["N", "n", "*", "R", "é", "€", "\U0001d11e"])) + s_[p_ + 1:]
    nl = {"crlf": "\r\n", "lone_cr": "\r"}.get(kind, "\n")
    tf = synth.fastq_text(f, "f", newline=nl).encode("utf-8")
    tr = synth.fastq_text(r, "r", newline=nl).encode("utf-8")
    if kind == "no_final_newline":
        tf, tr = tf[:-1], tr[:-2]
    elif kind == "unequal":
        tr = tr[: len(tr) * 2 // 3 + 7]
    elif kind == "empty":
        tf, tr = b"", b""
    elif kind == "gzip1":
        tf, tr = gzip.compress(tf), gzip.compress(tr)
    elif kind == "gzip_members":
        tf = b"".join(gzip.compress(tf[i:i + 9000]) for i in range(0, len(tf), 9000))
        tr = gzip.compress(tr[:100]) + gzip.compress(tr[100:])
    return tf, tr


def _count(host, ctx, g, fq_or_stream, streamed):
    from vstrains_amd import pe_inference

    ctx.build_index(g.seqs, 21)
    counter = host.PeCounter(ctx)
    if streamed:
        pe_inference.count_stream(ctx, fq_or_stream, counter)
    else:
        pe_inference.count_fastq(ctx, fq_or_stream, counter, 0, len(fq_or_stream), batch=700)
    pairs = fq_or_stream.n_pairs if streamed else len(fq_or_stream)
    fq_or_stream.close()
    return counter.result() + (pairs,)


KINDS = ["plain", "gzip1", "gzip_members", "crlf", "lone_cr", "no_final_newline", "unequal", "odd_bytes", "empty"]


@pytest.mark.parametrize("chunk", [None] + list(TINY_CHUNKS), ids=["default"] + ["chunk%d" % c for c in TINY_CHUNKS])
@pytest.mark.parametrize("kind", KINDS)
def test_stream_counters_equal_mapped(host, ctx, tmp_path, monkeypatch, kind, chunk):
    g, f, r = _synth_reads(2500 if chunk is None else 300, seed=11)
    tf, tr = _variant(kind, f, r)
    (tmp_path / "f.fq").write_bytes(tf)
    (tmp_path / "r.fq").write_bytes(tr)
    want = _count(host, ctx, g, host.FastqPair(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx), False)
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    fs = host.FastqStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, block_pairs=173)
    got = _count(host, ctx, g, fs, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3]
    if kind != "empty":
        assert want[3] > 0


def test_stream_through_fifos_counts_every_pair(host, ctx, tmp_path):
    g, f, r = _synth_reads(1200, seed=5)
    tf, tr = _variant("plain", f, r)
    (tmp_path / "f.fq").write_bytes(tf)
    (tmp_path / "r.fq").write_bytes(tr)
    want = _count(host, ctx, g, host.FastqPair(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx), False)
    with Fifos(tmp_path, gzip.compress(tf), tr) as (pf, pr):
        fs = host.FastqStream(pf, pr, ctx)
        got = _count(host, ctx, g, fs, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert got[3] == want[3] == 1200


def _drop_in(d, meta, fwd, rve, out, env=None):
    return subprocess.run(
        [sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
         "-f", fwd, "-r", rve, "-k", str(meta["k"])],
        cwd=ROOT, capture_output=True, text=True, env=env, timeout=600)


@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_drop_in_reads_fifos(tmp_path, name, d, meta):
    """Every golden case through two FIFOs: the files and the progress lines of the reference."""
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    out = tmp_path / "aln"
    with Fifos(tmp_path, tf, tr) as (pf, pr):
        proc = _drop_in(d, meta, pf, pr, out)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert _read(out / "pe_info") == _read(os.path.join(d, "pe_info"))
    assert _read(out / "st_info") == _read(os.path.join(d, "st_info"))
    lines = proc.stdout.splitlines()
    assert lines[0] == "----------------------Paired-End Information Alignment----------------------"
    assert lines[1] == "Start aligning reads to gfa nodes"
    assert [l for l in lines if l.startswith("Number of processed reads")] == meta["progress_lines"]
    assert lines[-2].startswith("Global time elapsed:  ")
    assert lines[-1] == "result stored in:  %s/pe_info" % out


def test_drop_in_stream_switch_on_regular_gzip(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    for which in ("fwd", "rve"):
        with open(os.path.join(d, which + ".fq"), "rb") as fh:
            raw = fh.read()
        (tmp_path / (which + ".fq.gz")).write_bytes(gzip.compress(raw[:5000]) + gzip.compress(raw[5000:]))
    out = tmp_path / "aln"
    env = dict(os.environ, VS_FASTQ_STREAM="1", VS_STREAM_CHUNK="4093")
    proc = _drop_in(d, meta, str(tmp_path / "fwd.fq.gz"), str(tmp_path / "rve.fq.gz"), out, env=env)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert _read(out / "pe_info") == _read(os.path.join(d, "pe_info"))
    assert _read(out / "st_info") == _read(os.path.join(d, "st_info"))


def _exception_line(stderr):
    return stderr.strip().splitlines()[-1]


@pytest.mark.parametrize("bad", ["utf8", "truncated_gzip"])
def test_stream_errors_match_mapped(tmp_path, bad):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    if bad == "utf8":
        tr = tr[: len(tr) // 2] + b"\xff\xfe" + tr[len(tr) // 2:]
    else:
        tf = gzip.compress(tf)
        tf = tf[: len(tf) - 40]
    (tmp_path / "f.fq").write_bytes(tf)
    (tmp_path / "r.fq").write_bytes(tr)
    mapped = _drop_in(d, meta, str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), tmp_path / "aln_mapped")
    assert mapped.returncode != 0
    out = tmp_path / "aln"
    with Fifos(tmp_path, tf, tr) as (pf, pr):
        proc = _drop_in(d, meta, pf, pr, out)
    assert proc.returncode != 0
    want, got = _exception_line(mapped.stderr), _exception_line(proc.stderr)
    assert got.split(":")[0] == want.split(":")[0], (got, want)
    assert not (out / "pe_info").exists() and not (out / "st_info").exists()
    assert not any(l.startswith("Number of processed reads") for l in proc.stdout.splitlines())


def test_whole_command_through_fifos(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from graph_case import Case

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)

    def run(fwd, rve, out):
        return subprocess.run(
            [sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
             "-fwd", fwd, "-rve", rve], cwd=ROOT, capture_output=True, text=True, timeout=600)

    plain = run(inp["fwd"], inp["rve"], tmp_path / "out_files")
    assert plain.returncode == 0, plain.stderr[-3000:]
    with open(inp["fwd"], "rb") as fh:
        tf = fh.read()
    with open(inp["rve"], "rb") as fh:
        tr = fh.read()
    with Fifos(tmp_path, tf, tr) as (pf, pr):
        piped = run(pf, pr, tmp_path / "out_fifos")
    assert piped.returncode == 0, piped.stderr[-3000:]
    for rel in ("strain.paths", "strain.fasta"):
        assert _read(tmp_path / "out_fifos" / rel) == _read(tmp_path / "out_files" / rel), rel


def test_device_line_scanner_matches_numpy(ctx):
    """Random text, line lengths from 1 byte to several wavefronts of 16-byte words, cut at random chunk sizes: the
    kernel's line ends and record cuts (the line number carried mod 4 from chunk to chunk) against numpy."""
    rng = np.random.default_rng(3)
    for trial in range(6):
        lens = rng.integers(0, 3000 if trial % 2 else 40, size=rng.integers(50, 400))
        parts = [bytes(rng.integers(33, 127, size=int(l), dtype=np.uint8)) + b"\n" for l in lens]
        text = b"".join(parts)
        if trial == 5:
            text = text.replace(b"A", b"\r", 3) + "é".encode()
        at, line0 = 0, 0
        while at < len(text):
            size = int(rng.integers(1, 9000))
            piece = text[at:at + size]
            ends, flags, cut = ctx.scan_text(piece, line0)
            arr = np.frombuffer(piece, dtype=np.uint8)
            want = np.flatnonzero(arr == 10)
            assert np.array_equal(ends, want.astype(np.uint64)), (trial, at)
            closing = [i for i in range(len(want)) if (line0 + i) % 4 == 3]
            assert cut == (int(want[closing[-1]]) + 1 if closing else 0)
            assert flags == (1 if b"\r" in piece else 0) | (2 if (arr >= 0x80).any() else 0)
            line0 = (line0 + len(want)) % 4
            at += size


_RSS_SCRIPT = r"""
import resource, sys
sys.argv = ["pe_inference"] + sys.argv[1:]
from vstrains_amd import pe_inference
pe_inference.main(sys.argv[1:])
print("PEAK_RSS_KB", resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)
"""


def test_stream_memory_does_not_grow_with_input(tmp_path):
    """Peak RSS of the streamed drop-in on a 0.5 M-pair and a 4 M-pair gzip pair: within one ring (both files) of each
    other -- the mapped path holds the whole inflated text."""
    from vstrains_amd import synth

    name, d, meta = [c for c in pe_cases() if c[0] == "hiv_like_k55"][0]
    st = synth.make_strains(4, 1500, 0.02, seed=21)
    f, r = synth.sample_pairs(st, 50000, 150, seed=22, sub_rate=0.005)
    mf = gzip.compress(synth.fastq_text(f, "f").encode(), compresslevel=1)
    mr = gzip.compress(synth.fastq_text(r, "r").encode(), compresslevel=1)
    rss = {}
    for copies in (10, 80):  # 0.5 M and 4 M pairs (multi-member gzip: the member repeated)
        (tmp_path / "f.fq.gz").write_bytes(mf * copies)
        (tmp_path / "r.fq.gz").write_bytes(mr * copies)
        env = dict(os.environ, VS_FASTQ_STREAM="1")
        proc = subprocess.run([sys.executable, "-c", _RSS_SCRIPT, "-g", os.path.join(d, "graph.gfa"), "-o", str(tmp_path / "aln"),
                               "-f", str(tmp_path / "f.fq.gz"), "-r", str(tmp_path / "r.fq.gz"), "-k", str(meta["k"])],
                              cwd=ROOT, capture_output=True, text=True, env=env, timeout=900)
        assert proc.returncode == 0, proc.stderr[-3000:]
        assert "Number of processed reads:  %d" % (copies * 50000 - 100000) in proc.stdout
        rss[copies] = int([l for l in proc.stdout.splitlines() if l.startswith("PEAK_RSS_KB")][0].split()[1]) * 1024
    ring = 2 * 4 * (64 << 20)
    assert abs(rss[80] - rss[10]) < ring, rss


def test_torchrun_refuses_fifo_input(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    env = dict(os.environ, VS_DIST_BACKEND="gloo", VS_DIST_DEVICE="0")
    with Fifos(tmp_path, tf, tf) as (pf, pr):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
             "--master-port", str(port), "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o",
             str(tmp_path / "aln"), "-f", pf, "-r", pr, "-k", str(meta["k"])],
            cwd=ROOT, capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode != 0
    assert "a pipe can be read by one process only" in proc.stderr


# ---- the block builder (block_builder_cases.py): what every streamed ingest checks alike ------------------------------------------
def test_over_long_sequence_line_of_file_2_is_refused(host, ctx, tmp_path):
    """a sequence line of 2^24 bytes in file 2: the builder's refusal, worded with that file and the record's number"""
    import block_builder_cases as bb
    from vstrains_amd import _native as nat

    fwd, rve = bb.edge_pairs(3)
    names = [b"p%d" % i for i in range(3)]
    (tmp_path / "f.fq").write_bytes(bb.fastq(fwd, names))
    (tmp_path / "r.fq").write_bytes(bb.fastq(rve[:1], names[:1]) + bb.long_record(names[1]) + bb.fastq(rve[2:], names[2:]))
    fs = host.FastqStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx)
    bb.refused(fs, nat.NativeError, "%s: record 1 has a sequence line of more than %d bytes" % (tmp_path / "r.fq", bb.LONG - 1))


def test_blocks_are_the_host_packers_at_the_edges_of_the_ends_kernel(host, ctx, tmp_path):
    import block_builder_cases as bb

    fwd, rve = bb.edge_pairs()
    names = [b"p%d" % i for i in range(len(fwd))]
    (tmp_path / "f.fq").write_bytes(bb.fastq(fwd, names))
    (tmp_path / "r.fq").write_bytes(bb.fastq(rve, names))
    bb.same_at_every_block_size(lambda n: host.FastqStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, block_pairs=n),
                                ctx.pack_pairs(fwd, rve), unpaired=False)
