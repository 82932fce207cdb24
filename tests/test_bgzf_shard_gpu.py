"""The member-sharded open of a BGZF pair on the device: the counting kernel against its host form, one process playing
every rank of the two passes, and the drop-in under torchrun (ranks sharing device 0 over gloo, at most eight of them, every
subprocess under a time limit of its own) -- the golden's files byte for byte, the reports of which ingest ran, the
fallbacks, and a corrupt member that one rank alone sees."""
import gzip
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import bgzf_util as bz
import test_fastq_stream_gpu as sg
from conftest import ROOT, pe_cases
from oracle import pe_oracle_c

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


# ---- the counting kernel ------------------------------------------------------------------------------------------------
def _host_counts(data):
    """(members of the walk, per member (status, newlines, flags, last byte) of the host form)"""
    from vstrains_amd import pe

    members, at, state = bz.py_walk(data)
    assert state == 0 and at == len(data)
    return members, [pe.inflate_count_host(data[o:o + n], isize, crc) for o, n, isize, crc in members]


def test_device_count_equals_the_host_form_member_for_member(host, ctx, tmp_path):
    """good_corpus() (every block type, flushes, 0 .. 65536 bytes, far matches, binary bytes) member by member -- one call per
    member, so that flags and last byte are that member's -- and in one call; then a FASTQ text of a few thousand members
    through the grid-stride loop and over several members per wavefront."""
    corpus = bz.good_corpus()
    data = b"".join(bz.wrap(raw, text) for _, raw, text in corpus)
    p = tmp_path / "corpus.gz"
    p.write_bytes(data)
    members, want = _host_counts(data)
    off, state, size = host.bgzf_walk_file(str(p))
    assert state == 0 and len(off) == len(corpus) + 1 and size == len(data)
    for i, (name, raw, text) in enumerate(corpus):
        counts, flags, last, n, nbytes = host.bgzf_count_lines(str(p), off[i:i + 2], ctx)
        print(name, int(counts[0]), flags, last)
        assert want[i][0] == 0, name
        assert (int(counts[0]), flags) == want[i][1:3] == (text.count(b"\n"), (1 if b"\r" in text else 0) | (2 if any(c >= 0x80 for c in text) else 0)), name
        assert last == (want[i][3] if text else 256) and n == 1 and nbytes == int(off[i + 1] - off[i]), name
    counts, flags, last, n, nbytes = host.bgzf_count_lines(str(p), off, ctx)
    assert [int(c) for c in counts] == [w[1] for w in want] and n == len(corpus) and nbytes == len(data)
    assert flags == 3 and last == corpus[-1][2][-1]
    # a few thousand small members and some whole ones, empty ones between them
    text = bz.fastq_text(6000, length=100)
    data = bz.bgzf(text[:900000], block=311, eof=True) + bz.bgzf(text[900000:], level=1)
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(data)
    members, want = _host_counts(data)
    assert len(members) > 2500
    off, state, size = host.bgzf_walk_file(str(p))
    assert state == 0 and len(off) == len(members) + 1
    counts, flags, last, n, nbytes = host.bgzf_count_lines(str(p), off, ctx)
    assert all(w[0] == 0 for w in want)
    assert np.array_equal(counts, np.asarray([w[1] for w in want], dtype=np.uint32))
    assert int(counts.sum()) == text.count(b"\n") and flags == 0 and last == 10 and n == len(members) and nbytes == len(data)
    lo, hi = 1000, 1777  # a share in the middle: those bytes only
    counts, flags, last, n, nbytes = host.bgzf_count_lines(str(p), off[lo:hi + 1], ctx)
    assert [int(c) for c in counts] == [w[1] for w in want[lo:hi]] and n == hi - lo and nbytes == int(off[hi] - off[lo])


def test_device_count_rejects_what_the_host_form_rejects(host, ctx, tmp_path):
    """A corrupt member among good ones ends with its status word (never a hang): the call fails in the words of the streamed
    ingest, zlib's code for that member."""
    from vstrains_amd import _native as nat

    text = bz.fastq_text(40)
    good = [bz.member(text[i:i + 3000]) for i in range(0, len(text), 3000)]
    for name, raw, isize, crc in bz.bad_corpus():
        data = b"".join(good[:2]) + bz.wrap(raw, b"", crc=crc & 0xFFFFFFFF, isize=isize) + b"".join(good[2:])
        members, at, state = bz.py_walk(data)
        if state != 0:
            continue  # (the walker does not hand it on)
        p = tmp_path / (name + ".gz")
        p.write_bytes(data)
        off, state, _ = host.bgzf_walk_file(str(p))
        assert state == 0
        with pytest.raises(nat.NativeError) as ei:
            host.bgzf_count_lines(str(p), off, ctx)
        assert "%s: not a complete gzip stream (zlib code -" % p in str(ei.value), name


# ---- one process plays every rank ---------------------------------------------------------------------------------------
def _blocks(fs):
    seqs, lens = [], []
    for block in fs:
        out, ln, _ = block.unpack()
        seqs.append(out.copy())
        lens.append(ln.copy())
        block.free()
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), (np.concatenate(lens) if lens else np.zeros(0, np.uint32))


SHAPES = {
    # name -> (text variant, member size of R1, of R2, VS_STREAM_CHUNK, world sizes)
    "few_members": ("plain", None, None, None, (1, 2, 3, 5)),  # (two or three members a file: five ranks are more than that)
    "members_never_line_up": ("plain", 7000, 5200, 20000, (1, 2, 3, 5)),
    "members_smaller_than_a_record": ("plain", 97, 61, 4000, (1, 2, 3, 5)),
    "no_final_newline": ("no_final_newline", 4999, 3001, 20000, (1, 2, 3, 5)),
    "unequal_record_counts": ("unequal", 3000, 800, 20000, (1, 3, 5)),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_process_plays_every_rank(host, ctx, tmp_path, monkeypatch, shape):
    """Pass 1 for each rank, the exchange by hand through the injected all_gather, pass 2 for each rank: the ranks' blocks
    one behind the other are the blocks of the single-process stream on the same files, the summed counters the C oracle's;
    every member is inflated once in pass 1, at most M + W - 1 members in pass 2, and a reader reads its range and no more."""
    kind, block_f, block_r, chunk, worlds = SHAPES[shape]
    g, f, r = sg._synth_reads(300, seed=11)
    tf, tr = sg._variant(kind, f, r)
    fwd, rve = str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz")
    (tmp_path / "f.fq.gz").write_bytes(bz.bgzf(tf, block=block_f))
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr, level=1, block=block_r, eof=False))
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    single = host.FastqStream(fwd, rve, ctx, block_pairs=64)
    want_seq, want_len = _blocks(single)
    total = single.n_pairs
    single.close()
    assert (150 < total < 300 if kind == "unequal" else total == 300) and len(want_len) == 2 * total
    ref = pe_oracle_c.Oracle(g.seqs, 21).count_pairs(f[:total], r[:total])
    n_members = [len(bz.py_walk(open(p, "rb").read())[0]) for p in (fwd, rve)]
    if shape == "few_members":
        assert max(n_members) < 5
    for world in worlds:
        mine = [host.FastqStream.shard_count(fwd, rve, ctx, rank, world) for rank in range(world)]
        assert all(m.failure is None for m in mine)
        everyone = [list(m.message) for m in mine]
        assert len({len(v) for v in everyone}) == 1  # (padded to one length)
        for i in range(2):
            assert sum(m.members_pass1[i] for m in mine) == n_members[i], (world, i)
        ctx.build_index(g.seqs, 21)
        counter = host.PeCounter(ctx)
        seqs, lens, first, pass2 = [], [], 0, [0, 0]
        for rank in range(world):
            fs, why = host.FastqStream.shard_open(mine[rank], everyone, lambda vals: [list(vals)] * world, block_pairs=64)
            assert why is None and fs.first == first and fs.total_pairs == total and fs.members == tuple(n_members)
            block = fs.next_block()
            while block is not None:
                out, ln, _ = block.unpack()
                seqs.append(out.copy())
                lens.append(ln.copy())
                counter.add(block)
                ctx.sync()
                block.free()
                block = fs.next_block()
            info = fs.info
            assert info["pairs"] == fs.shard_pairs and info["members_host"] == (0, 0)
            for i, path in enumerate((fwd, rve)):
                a, skip, e = fs.plan[i]
                assert info["members_device"][i] == e - a, (world, rank, i)
                pass2[i] += e - a
            off = [host.bgzf_walk_file(p)[0] for p in (fwd, rve)]
            assert info["file_bytes"] == sum(int(off[i][fs.plan[i][2]] - off[i][fs.plan[i][0]]) for i in range(2)), (world, rank)
            first += fs.shard_pairs
            fs.close()
        assert first == total
        for i in range(2):
            assert pass2[i] <= n_members[i] + world - 1, (world, i, pass2)
        assert np.array_equal(np.concatenate(lens), want_len) and np.array_equal(np.concatenate(seqs), want_seq), world
        node_mat, short_mat, stats = counter.result()
        assert np.array_equal(node_mat, ref[0]) and np.array_equal(short_mat, ref[1]), world
        assert stats == tuple(int(x) for x in ref[2]), world


def test_the_ranks_fall_back_together_from_gathered_values(host, ctx, tmp_path):
    """A '\\r' in the share of ONE rank, and a file whose last member is another gzip member: every rank's pass 2 says so."""
    g, f, r = sg._synth_reads(200, seed=11)
    tf, tr = sg._variant("plain", f, r)
    at = len(tf) * 4 // 5
    at = tf.index(b"\n", at)
    cr = tf[:at] + b"\r" + tf[at:]
    shapes = {"a carriage return or a byte >= 0x80": (bz.bgzf(cr, block=5000), bz.bgzf(tr, block=5000)),
              "not whole BGZF": (bz.bgzf(tf, block=5000), bz.bgzf(tr, block=5000, eof=False) + gzip.compress(b""))}
    for reason, (zf, zr) in shapes.items():
        (tmp_path / "f.fq.gz").write_bytes(zf)
        (tmp_path / "r.fq.gz").write_bytes(zr)
        mine = [host.FastqStream.shard_count(str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"), ctx, rank, 3) for rank in range(3)]
        everyone = [list(m.message) for m in mine]
        if reason.startswith("a carriage"):
            assert [v[3] for v in everyone] == [0, 0, 1]  # (the flags of the forward file's shares)
        for rank in range(3):
            assert host.FastqStream.shard_open(mine[rank], everyone, lambda vals: [list(vals)] * 3) == (None, reason)


# ---- the drop-in under torchrun -----------------------------------------------------------------------------------------
def _torchrun(ranks, d, meta, fwd, rve, out, report, env=None, timeout=600):
    env = dict(env or {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")},
               VS_DIST_BACKEND="gloo", VS_DIST_DEVICE="0", VS_INGEST_REPORT=str(report))
    for attempt in range(3):  # (a port that was free when asked for may be taken a moment later: ask again)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
             "--master-port", str(port), "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out),
             "-f", str(fwd), "-r", str(rve), "-k", str(meta["k"])],
            cwd=ROOT, capture_output=True, text=True, env=env, timeout=timeout)
        if proc.returncode == 0 or "address already in use" not in proc.stderr:
            break
    return proc


def _reports(report, ranks):
    assert sorted(os.listdir(str(report))) == sorted("ingest_rank%d.json" % r for r in range(ranks))
    out = []
    for r in range(ranks):
        with open(os.path.join(str(report), "ingest_rank%d.json" % r)) as fh:
            out.append(json.load(fh))
    return out


def _case(name):
    return [c for c in pe_cases() if c[0] == name][0]


def _same_files(out, d):
    assert sg._read(out / "pe_info") == sg._read(os.path.join(d, "pe_info"))
    assert sg._read(out / "st_info") == sg._read(os.path.join(d, "st_info"))
    assert sorted(os.listdir(str(out))) == ["pe_info", "st_info"]


@pytest.mark.parametrize("ranks", [2, 3, 8])
def test_sharded_drop_in_shares_bgzf_files_by_member(tmp_path, ranks):
    """Both inputs BGZF with member sizes that never line up: the golden's files, rank 0 alone writes, every rank reports
    the member-sharded ingest, every member inflated once in pass 1 and at most M + W - 1 members in pass 2."""
    name, d, meta = _case("errors_k21")
    n_members = []
    for which, block, eof in (("fwd", 3000, True), ("rve", 2100, False)):
        with open(os.path.join(d, which + ".fq"), "rb") as fh:
            data = bz.bgzf(fh.read(), block=block, eof=eof)
        (tmp_path / (which + ".fq.gz")).write_bytes(data)
        n_members.append(len(bz.py_walk(data)[0]))
    out = tmp_path / "aln"
    out.mkdir()
    (out / "stale_file").write_text("x")
    proc = _torchrun(ranks, d, meta, tmp_path / "fwd.fq.gz", tmp_path / "rve.fq.gz", out, tmp_path / "report")
    assert proc.returncode == 0, proc.stderr[-3000:]
    _same_files(out, d)
    assert proc.stdout.count("result stored in:") == 1  # rank 0 only
    assert [l for l in proc.stdout.splitlines() if l.startswith("Number of processed reads")] == meta["progress_lines"]
    reports = _reports(tmp_path / "report", ranks)
    print(reports)
    assert all(r["path"] == "bgzf_members" and r["reason"] is None and r["world"] == ranks and r["members"] == n_members for r in reports)
    first = 0
    for r in reports:  # the blocks tile the pairs in rank order
        assert r["first_pair"] == first
        first += r["pairs"]
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        assert first == fh.read().count(b"\n") // 4
    for i in range(2):
        assert sum(r["members_pass1"][i] for r in reports) == n_members[i]
        assert 0 < sum(r["members_pass2"][i] for r in reports) <= n_members[i] + ranks - 1


FALLBACKS = {
    # name -> (golden case, reason in the report)
    "crlf": ("crlf_k21", "a carriage return or a byte >= 0x80"),
    "utf8_character_in_a_read": ("utf8_reads_k21", "a carriage return or a byte >= 0x80"),
    "plain_gzip_member_appended": ("errors_k21", "not whole BGZF"),
    "one_plain_one_bgzf": ("errors_k21", "the inputs are not both BGZF"),
    "VS_BGZF_DEVICE=0": ("errors_k21", "VS_BGZF_DEVICE=0"),
}


@pytest.mark.parametrize("kind", sorted(FALLBACKS))
def test_sharded_drop_in_falls_back_to_the_whole_file_open(tmp_path, kind):
    case, reason = FALLBACKS[kind]
    name, d, meta = _case(case)
    texts = {}
    for which in ("fwd", "rve"):
        with open(os.path.join(d, which + ".fq"), "rb") as fh:
            texts[which] = fh.read()
    if kind == "crlf":
        assert b"\r\n" in texts["fwd"]
    if kind == "utf8_character_in_a_read":
        assert any(c >= 0x80 for c in texts["fwd"] + texts["rve"])
    packed = {which: bz.bgzf(text, block=2500) for which, text in texts.items()}
    if kind == "plain_gzip_member_appended":
        cut = texts["rve"].index(b"\n@", len(texts["rve"]) // 2) + 1
        packed["rve"] = bz.bgzf(texts["rve"][:cut], block=2500, eof=False) + gzip.compress(texts["rve"][cut:])
    if kind == "one_plain_one_bgzf":
        packed["fwd"] = texts["fwd"]
    for which, data in packed.items():
        (tmp_path / (which + ".fq.gz")).write_bytes(data)
    env = {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")}
    if kind == "VS_BGZF_DEVICE=0":
        env["VS_BGZF_DEVICE"] = "0"
    out = tmp_path / "aln"
    proc = _torchrun(2, d, meta, tmp_path / "fwd.fq.gz", tmp_path / "rve.fq.gz", out, tmp_path / "report", env=env)
    assert proc.returncode == 0, proc.stderr[-3000:]
    _same_files(out, d)
    reports = _reports(tmp_path / "report", 2)
    print(reports)
    assert all(r["path"] == "whole_files" and r["reason"] == reason and r["members_pass2"] == [0, 0] for r in reports)
    assert reports[0]["first_pair"] == 0 and reports[1]["first_pair"] == reports[0]["pairs"]


def test_a_corrupt_member_in_the_share_of_rank_1_fails_every_rank(tmp_path):
    """A flipped CRC32 in a member that only rank 1 reads in pass 1: the run ends non-zero long before its time limit, with
    the line the single-process stream prints for the same files, and writes no pe_info."""
    name, d, meta = _case("errors_k21")
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    members = [bz.member(tf[i:i + 3000]) for i in range(0, len(tf), 3000)] + [bz.EOF_MARK]
    bad = len(members) - 4
    assert bad >= len(members) // 2 + 1  # rank 1 of 2 takes [M // 2, M)
    hurt = bytearray(members[bad])
    hurt[-8] ^= 0x10
    members[bad] = bytes(hurt)
    (tmp_path / "f.fq.gz").write_bytes(b"".join(members))
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr, block=2100))
    env = {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")}
    one = sg._drop_in(d, meta, str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"), tmp_path / "aln_one", env=env)
    assert one.returncode != 0
    line = sg._exception_line(one.stderr)
    assert "%s: not a complete gzip stream (zlib code -3)" % (tmp_path / "f.fq.gz") in line
    out = tmp_path / "aln"
    t0 = time.time()
    proc = _torchrun(2, d, meta, tmp_path / "f.fq.gz", tmp_path / "r.fq.gz", out, tmp_path / "report", timeout=300)
    took = time.time() - t0
    print(took, proc.stderr[-1500:])
    assert proc.returncode != 0 and took < 150
    assert line in proc.stderr  # rank 1, in the words of the single process
    assert "FASTQ open failed on rank(s) [1]" in proc.stderr  # rank 0
    assert not (out / "pe_info").exists() and not (out / "st_info").exists()
    assert not any(l.startswith("Number of processed reads") for l in proc.stdout.splitlines())
