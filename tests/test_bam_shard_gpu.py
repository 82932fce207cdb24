"""The member-sharded open of a collated BAM on the device: the summary kernels against their host twin entry for entry, one
process playing every rank of the two passes, and the drop-in under torchrun (ranks sharing device 0 over gloo, at most eight
of them, every subprocess under a time limit of its own) -- the golden's files byte for byte, the reports of which ingest
ran, the fallbacks, and what fails."""
import gzip
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import bam_shard_model as model
import bam_util as bu
import bgzf_util as bz
import test_bam_gpu as tg
import test_bam_shard_cpu as tc
import test_bgzf_shard_gpu as sb
import test_fastq_stream_gpu as sg
from conftest import ROOT

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


@pytest.fixture(scope="module")
def workload():
    """about 2 000 pairs with dropped records between the mates (test_bam_gpu's), inflated"""
    g, records = tg._workload()
    return records, bu.inflated(records)


def _member_sizes(path):
    members, at, state = bz.py_walk(open(path, "rb").read())
    assert state == 0
    return [isize for _, _, isize, _ in members]


# ---- the summary kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [64, 128, None], ids=["seg64", "seg128", "seg_default"])
def test_device_summary_equals_the_host_twin(host, ctx, workload, tmp_path, monkeypatch, seg):
    """The constructed files and a BAM of a few thousand records, shares of members, windows of a few members (a share spans
    several windows and its candidates are carried across them): X and N of every candidate of every rank, from the file
    (``vs_bam_share_summary``: reader, k_inflate, tables, lanes) and from inflated bytes (``_text``)."""
    if seg is not None:
        monkeypatch.setenv("VS_BAM_SEG", str(seg))
    files = [(n, d, 613, 1500) for n, d in bu.constructed() if n != "header_only"] + [("workload", workload[1], 4000, 30000)]
    for name, data, block, chunk in files:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
        p = tmp_path / (name + ".bam")
        p.write_bytes(bz.bgzf(data, block=block))
        sizes = _member_sizes(str(p))
        for world in (2, 3):
            S = model.boundaries(sizes, world)
            want = tc.messages(host, data, S, seg or 0)
            text = tc.messages(host, data, S, seg or 0, chunk=chunk, ctx=ctx)
            got = [host.BamStream.shard_summary(str(p), ctx, rank, world) for rank in range(world)]
            for rank in range(world):
                assert got[rank].failure is None, got[rank].failure
                msg = got[rank].message
                assert msg[:3] == [0, 1, len(sizes)] and msg[3:] == want[rank][3:], (name, world, rank)
                assert text[rank] == want[rank], (name, world, rank)
                assert msg[5] == (1 if rank == 0 else min(seg or 12288, S[rank + 1] - S[rank]))
            assert sum(m.members_pass1 for m in got) >= len(sizes)  # (every member once, and the few behind a share's end)
            assert sum(m.members_pass1 for m in got) <= len(sizes) + (world - 1) * (1 + model.TAIL // max(1, min(s for s in sizes if s)))


# ---- one process plays every rank -----------------------------------------------------------------------------------------
SHAPES = {
    # name -> (member size, VS_STREAM_CHUNK, VS_BAM_SEG)
    "members_of_3001": (3001, 20000, None),
    "members_of_701_windows_of_a_few": (701, 4000, 1024),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_process_plays_every_rank(host, ctx, workload, tmp_path, monkeypatch, shape):
    """Summaries for each rank, the exchange by hand, the plan, the ranged open for each rank: the ranks' blocks one behind the
    other are the blocks of the whole-file stream, the tallies sum to its tallies, and pass 2 inflates at most two members a
    rank beyond the M of the file."""
    block, chunk, seg = SHAPES[shape]
    records, data = workload
    monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    if seg is not None:
        monkeypatch.setenv("VS_BAM_SEG", str(seg))
    p = str(tmp_path / "reads.bam")
    with open(p, "wb") as fh:
        fh.write(bz.bgzf(data, block=block))
    n_members = len(_member_sizes(p))
    single = host.BamStream(p, ctx, block_pairs=64)
    want_seq, want_len = sb._blocks(single)
    want = single.info
    single.close()
    assert want["pairs"] == 2000 and want["dropped_0x900"] > 0 and want["dropped_other"] > 0
    for world in (1, 2, 3, 5):
        mine = [host.BamStream.shard_summary(p, ctx, rank, world) for rank in range(world)]
        assert all(m.failure is None for m in mine)
        everyone = [list(m.message) for m in mine]
        seqs, lens, first, tallies, pass2 = [], [], 0, dict(pairs=0, records=0, dropped_0x900=0, dropped_other=0), 0
        for rank in range(world):
            fs, why = host.BamStream.shard_open(mine[rank], everyone, lambda vals: [list(vals)] * world, block_pairs=64)
            assert why is None and fs.first_pair == first and fs.members == n_members, (world, rank, why)  # (no fallback)
            a, b = sb._blocks(fs)
            seqs.append(a)
            lens.append(b)
            info = fs.info
            assert info["pairs"] == fs.pairs == len(b) // 2 and info["done"], (world, rank)
            for k in tallies:
                tallies[k] += info[k]
            pass2 += info["members_device"]
            first += fs.pairs
            fs.close()
        assert first == 2000 and tallies == {k: want[k] for k in tallies}, (world, tallies)
        assert n_members - 1 <= pass2 <= n_members + 2 * (world - 1), (world, pass2, n_members)
        assert np.array_equal(np.concatenate(lens), want_len) and np.array_equal(np.concatenate(seqs), want_seq), world


# ---- the drop-in under torchrun -------------------------------------------------------------------------------------------
def _torchrun(ranks, d, meta, bam, out, report, env, extra=(), timeout=300):
    env = dict(env, VS_DIST_BACKEND="gloo", VS_DIST_DEVICE="0", VS_INGEST_REPORT=str(report))
    for attempt in range(3):  # (a port that was free when asked for may be taken a moment later: ask again)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
             "--master-port", str(port), "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out),
             "-f", str(bam), "-r", str(bam), "-k", str(meta["k"])] + list(extra),
            cwd=ROOT, capture_output=True, text=True, env=env, timeout=timeout)
        if proc.returncode == 0 or "address already in use" not in proc.stderr:
            break
    return proc


def _env(**more):
    env = {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK", "VS_BAM_SEG")}
    env.update(more)
    return env


def _golden_records():
    name, d, meta = sb._case("errors_k21")
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    # BAM has no lower-case bases.  The golden's few lower-case letters make their end invalid, as every byte outside ACGTN
    # does: an IUPAC code in their place stands for the same pair, and the golden's files come out byte for byte
    lower = bytes.maketrans(b"acgtn", b"RRRRR")
    assert tf != tf.translate(lower)
    tf, tr = (b"\n".join(l.translate(lower) if i % 4 == 1 else l for i, l in enumerate(t.split(b"\n"))) for t in (tf, tr))
    records = tg._records_of_pair(tf, tr)
    assert [t.decode().split("\n")[1::4] for t in bu.fastq_pair(records)] == [t.decode().split("\n")[1::4] for t in (tf, tr)]
    return d, meta, records


def _members_that_end_inside_records(data, about=300, before_end=23):
    """The BAM of inflated ``data`` in members of about ``about`` bytes, none of which ends where a record does: every member
    ends ``before_end`` bytes in front of a record's end.  With segments of 64 bytes a share boundary anywhere else in a
    record of 160 bytes would be "a record longer than a segment across a share boundary"; here every boundary leaves less
    than a segment of the record to the next share, whatever the number of ranks."""
    ends = [t[0] for t in bu.walk(data)[0]][1:] + [len(data)]
    cuts, last = [], 0
    for e in ends[:-1]:
        if e - before_end - last >= about:
            cuts.append(e - before_end)
            last = cuts[-1]
    parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    assert all(len(x) <= 65280 for x in parts) and not set(cuts) & set(ends)
    return b"".join(bz.member(x) for x in parts) + bz.EOF_MARK


@pytest.mark.parametrize("ranks", [2, 3, 8])
def test_sharded_drop_in_shares_a_collated_bam_by_member(tmp_path, ranks):
    """The golden's reads as one collated BAM in members of a few hundred bytes, segments of 64: the golden's files, rank 0
    alone writes, every rank reports the member-sharded ingest and the ranks' couples tile the file."""
    d, meta, records = _golden_records()
    bam = tmp_path / "reads.bam"
    bam.write_bytes(_members_that_end_inside_records(bu.inflated(records)))
    n_members = len(_member_sizes(str(bam)))
    assert n_members > 100
    out = tmp_path / "aln"
    out.mkdir()
    (out / "stale_file").write_text("x")
    proc = _torchrun(ranks, d, meta, bam, out, tmp_path / "report", _env(VS_BAM_SEG="64", VS_STREAM_CHUNK="2000"))
    assert proc.returncode == 0, proc.stderr[-3000:]
    sb._same_files(out, d)
    assert proc.stdout.count("result stored in:") == 1  # rank 0 only
    reports = sb._reports(tmp_path / "report", ranks)
    print(reports)
    assert all(r["path"] == "bam_members" and r["reason"] is None and r["world"] == ranks and r["members"] == [n_members] for r in reports)
    first = 0
    for r in reports:  # the couples tile the file in rank order
        assert r["first_pair"] == first
        first += r["pairs"]
    assert first == len(bu.couples([r.flag for r in records])[0]) == 300
    assert sum(r["members_pass1"][0] for r in reports) >= n_members
    assert n_members - 1 <= sum(r["members_pass2"][0] for r in reports) <= n_members + 2 * (ranks - 1)


FALLBACKS = ("a_record_longer_than_the_segment_across_the_boundary", "plain_gzip_member_appended", "VS_BGZF_DEVICE=0")


@pytest.mark.parametrize("kind", FALLBACKS)
def test_sharded_drop_in_leaves_the_file_to_rank_0(host, tmp_path, kind):
    d, meta, records = _golden_records()
    data = bu.inflated(records)
    env = _env(VS_BAM_SEG="64")
    if kind == "plain_gzip_member_appended":
        packed, reason = bz.bgzf(data, block=700, eof=False) + gzip.compress(b""), host.BAM_SHARD_REASONS[3]
    elif kind == "VS_BGZF_DEVICE=0":
        packed, reason = bz.bgzf(data, block=700), "VS_BGZF_DEVICE=0"
        env["VS_BGZF_DEVICE"] = "0"
    else:
        # two members: the first ends 30 bytes behind the start of a record of 160 bytes, so 130 bytes of it lie in rank 1's share
        starts = [t[0] for t in bu.walk(data)[0]]
        cut = starts[len(starts) // 2] + 30
        packed, reason = bz.member(data[:cut]) + bz.member(data[cut:]) + bz.EOF_MARK, host.BAM_SHARD_REASONS[5]
        assert len(bz.py_walk(packed)[0]) == 3  # (rank 0: member 0; rank 1: member 1 and the empty one)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(packed)
    out = tmp_path / "aln"
    proc = _torchrun(2, d, meta, bam, out, tmp_path / "report", env)
    assert proc.returncode == 0, proc.stderr[-3000:]
    sb._same_files(out, d)
    reports = sb._reports(tmp_path / "report", 2)
    print(reports)
    assert all(r["path"] == "bam_whole_file_rank0" and r["reason"] == reason for r in reports)
    assert [r["pairs"] for r in reports] == [300, 0] and reports[1]["members_pass2"] == [0]


def _fails_as_the_single_process(tmp_path, packed, timeout=300):
    d, meta, _ = _golden_records()
    bam = tmp_path / "reads.bam"
    bam.write_bytes(packed)
    one = sg._drop_in(d, meta, str(bam), str(bam), tmp_path / "aln_one", env=_env())
    assert one.returncode != 0
    line = sg._exception_line(one.stderr)
    out = tmp_path / "aln"
    t0 = time.time()
    proc = _torchrun(2, d, meta, bam, out, tmp_path / "report", _env(VS_BAM_SEG="4096"), timeout=timeout)
    took = time.time() - t0
    print(took, line, proc.stderr[-1500:])
    assert proc.returncode != 0 and took < timeout / 2
    assert not (out / "pe_info").exists() and not (out / "st_info").exists()
    return line, proc


def test_a_truncated_file_fails_in_the_words_of_the_single_process(tmp_path):
    """The file ends inside a record: the plan sends it to rank 0, whose whole-file stream names the record as ever."""
    _, _, records = _golden_records()
    data = bu.inflated(records)
    line, proc = _fails_as_the_single_process(tmp_path, bz.bgzf(data[:-50], block=700))
    assert "truncated record" in line and line in proc.stderr


def test_an_uncollated_file_fails_in_the_words_of_the_single_process(tmp_path):
    """Two firsts in a row in rank 1's share: the parities still add up, so the ranks stream their shares, and the owner of the
    couple says what the single process says -- the record named by its offset in the inflated file, which is said too."""
    _, _, records = _golden_records()
    part = [i for i, r in enumerate(records) if bu.classify(r.flag) <= bu.C_SECOND]
    k = 2 * (3 * len(part) // 8)  # (the first record of a couple in the second half of the file)
    same = [i for i in part[k + 2:k + 4] if bu.classify(records[i].flag) == bu.classify(records[part[k]].flag)][0]
    records[part[k + 1]], records[same] = records[same], records[part[k + 1]]  # (couple k: two of one end; the parities stay)
    data = bu.inflated(records)
    assert bu.couples([r.flag for r in records])[1] is not None
    line, proc = _fails_as_the_single_process(tmp_path, bz.bgzf(data, block=700))
    words = line[line.index(" is the same end"):]
    assert "not collated" in words and "samtools collate" in words
    assert words in proc.stderr and "of the inflated file (a member range: records are named by offset)" in proc.stderr


def test_a_corrupt_member_in_the_share_of_rank_1_fails_every_rank(tmp_path):
    """A flipped CRC32 in a member that only rank 1 inflates in pass 1: both ranks end non-zero long before the time limit."""
    _, _, records = _golden_records()
    data = bu.inflated(records)
    members = [bz.member(data[i:i + 700]) for i in range(0, len(data), 700)] + [bz.EOF_MARK]
    bad = len(members) - 5
    hurt = bytearray(members[bad])
    hurt[-8] ^= 0x10
    members[bad] = bytes(hurt)
    line, proc = _fails_as_the_single_process(tmp_path, b"".join(members))
    assert "not a complete gzip stream (BGZF member %d does not inflate to its CRC32 and size)" % bad in line
    assert line in proc.stderr                                  # rank 1, in the words of the single process
    assert "BAM open failed on rank(s) [1]" in proc.stderr      # rank 0
    assert not any(l.startswith("Number of processed reads") for l in proc.stdout.splitlines())


def test_by_name_under_two_ranks_is_refused(tmp_path):
    d, meta, records = _golden_records()
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(records, block=700))
    proc = _torchrun(2, d, meta, bam, tmp_path / "aln", tmp_path / "report", _env(), extra=("--bam-by-name",))
    assert proc.returncode != 0
    assert "--bam-by-name reads the file in one process only" in proc.stderr and "different ranks' shares" in proc.stderr
    assert not (tmp_path / "aln" / "pe_info").exists()
