"""One interleaved BGZF FASTQ shared among ranks by member, on the device: ``vs_fastq_il_range_fn`` alone against the model
of tests/il_shard_model.py, one process playing every rank of the three passes (``pe.InterleavedStream.shard_count`` /
``shard_tail`` / ``shard_open``) with the exchange done by hand, and the drop-in under torchrun (ranks sharing device 0 over
gloo, at most eight of them, every subprocess under a time limit of its own)."""
import gzip
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import bgzf_util as bz
import il_shard_model as sm
import interleaved_model as im
import test_bgzf_shard_gpu as bs
import test_fastq_stream_gpu as sg
from conftest import ROOT
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


# ---- vs_fastq_il_range_fn alone ---------------------------------------------------------------------------------------------
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 4 * 256 + 1]  # the wavefront and workgroup edges of k_il_match


def _patterns(n):
    """(name, m[0 .. n - 2]) for n records"""
    k = n - 1
    out = [("all_true", [True] * k), ("all_false", [False] * k), ("alternating", [j % 2 == 0 for j in range(k)])]
    for name, at in (("false_first", 0), ("false_last", k - 1), ("false_at_wave_edge", 63), ("false_behind_wave_edge", 64)):
        if 0 <= at < k:
            out.append((name, [j != at for j in range(k)]))
    return out


def _headers_of(m, slashes=False):
    """header lines with exactly these match flags: a new name where m is false.  ``slashes`` (m alternating): the pairs are
    named x/1 x/2, with names of every length 1..16 so that the header lines start at every byte alignment."""
    out, name = [], 0
    for j in range(len(m) + 1):
        if j and not m[j - 1]:
            name += 1
        if slashes:
            out.append(b"@" + b"n" * (name % 16) + b"%d/%d" % (name, 1 + j % 2))
        else:
            out.append(b"@r%d" % name)
    return out


def _write_bgzf(tmp_path, name, text, block):
    p = tmp_path / name
    p.write_bytes(bz.bgzf(text, block=block))
    return str(p)


@pytest.mark.parametrize("n", COUNTS)
def test_range_fn_equals_the_model(host, ctx, tmp_path, monkeypatch, n):
    """The whole file as one range, in windows of a few hundred bytes to a few thousand: the function composes across them."""
    monkeypatch.setenv("VS_STREAM_CHUNK", "1500")
    for name, m in _patterns(n):
        headers = _headers_of(m, slashes=(name == "alternating"))
        assert sm.m_of_headers(headers, im.mates) == m
        text = im.from_headers(headers)
        path = _write_bgzf(tmp_path, "%s.fq.gz" % name, text, 700)
        off, state, size = host.bgzf_walk_file(path)
        assert state == 0
        fn, info = host.il_range_fn(path, (0, size), 0, n, ctx)
        print(n, name, fn, info)
        assert fn == sm.share_fn(m, 0, n - 1), (n, name)
        assert info[3] == (n if n > 1 else 0) and info[1] == (size if n > 1 else 0)
        if len(text) > 6000:
            assert info[2] > 2  # several windows
        if n > 3:  # a prefix of the range's records: the m behind it do not count
            fn, info = host.il_range_fn(path, (0, size), 0, n - 2, ctx)
            assert fn == sm.share_fn(m, 0, n - 3) and info[3] == n - 2, (n, name)


def test_range_fn_on_names_at_every_byte_alignment(host, ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("VS_STREAM_CHUNK", "900")
    m = [j % 2 == 0 for j in range(400)]
    headers = _headers_of(m, slashes=True)
    text = im.from_headers(headers)
    starts, at = set(), 0
    for k, h in enumerate(headers):
        starts.add(at % 16)
        at += len(im.record(h, k))
    assert starts == set(range(16))
    path = _write_bgzf(tmp_path, "aligned.fq.gz", text, 1000)
    size = os.path.getsize(path)
    assert host.il_range_fn(path, (0, size), 0, len(headers), ctx)[0] == sm.share_fn(m, 0, len(m)) == sm.CONST0
    assert host.il_range_fn(path, (0, size), 0, len(headers) - 1, ctx)[0] == sm.share_fn(m, 0, len(m) - 1) == sm.CONST1


@pytest.mark.parametrize("block", [97, 5000], ids=["members_smaller_than_a_record", "members_of_many_records"])
def test_range_fn_entered_mid_member_with_lines_to_skip(host, ctx, tmp_path, monkeypatch, block):
    monkeypatch.setenv("VS_STREAM_CHUNK", "2000")
    rng = np.random.default_rng(3)
    m = [bool(x) for x in rng.random(699) < 0.8]
    headers = _headers_of(m)
    recs = [im.record(h + b" a comment that makes every record longer than a member of 97 bytes: " + b"x" * 40, k) for k, h in enumerate(headers)]
    assert min(len(r) for r in recs) > 97
    path = _write_bgzf(tmp_path, "mid.fq.gz", b"".join(recs), block)
    off, state, size = host.bgzf_walk_file(path)
    counts, flags, last, _, _ = host.bgzf_count_lines(path, off, ctx)
    assert state == 0 and flags == 0 and last == 10
    skips = set()
    for first, end in ((0, 700), (1, 700), (137, 138), (137, 139), (200, 457), (331, 700), (698, 700), (5, 70), (411, 476)):
        a, skip, e = host.bgzf_shard_plan(counts, False, first, end)
        skips.add(skip > 0)
        fn, info = host.il_range_fn(path, (off[a], off[e]), skip, end - first, ctx)
        assert fn == sm.share_fn(m, first, end - 1), (first, end)
        if end - first > 1:
            assert info[0] == e - a and info[1] == int(off[e] - off[a]) and info[3] == end - first, (first, end)
    assert skips == {False, True}


# ---- one process plays every rank ---------------------------------------------------------------------------------------
WORLDS = (1, 2, 3, 5, 8)


def _layout(total, anchors):
    """run lengths that sum to ``total``: the run of ``anchors[pos]`` records starts at record pos, pairs fill the gaps (one
    single where a gap is odd)"""
    runs, pos = [], 0
    for at in sorted(anchors) + [total]:
        gap = at - pos
        assert gap >= 0
        runs += [1] * (gap % 2) + [2] * (gap // 2)
        if at < total:
            runs.append(anchors[at])
            pos = at + anchors[at]
    assert sum(runs) == total
    return runs


def _names(runs):
    return sum(([b"@q%d" % k] * n for k, n in enumerate(runs)), [])


def _boundaries(total):
    return {sm.shard_range(total, r, w)[1] for w in WORLDS for r in range(w - 1)}


def _run_of(names, j):
    """[lo, hi): the maximal run of equal names that holds record j"""
    lo, hi = j, j + 1
    while lo > 0 and names[lo - 1] == names[j]:
        lo -= 1
    while hi < len(names) and names[hi] == names[j]:
        hi += 1
    return lo, hi


def _shape(name):
    """(record names, what follows the last record, member size, VS_STREAM_CHUNK); the assertions say that ``shard_range`` puts
    a boundary where the shape wants one"""
    if name in ("features", "no_final_newline", "trailing_1_line", "trailing_3_lines"):
        # T = 300: boundaries at 150 (W = 2), 100 / 200 (W = 3), 60 / 120 / 180 / 240 (W = 5), 37 / 75 / 112 / ... (W = 8)
        names = _names(_layout(300, {0: 1, 59: 3, 99: 1, 118: 4, 149: 2, 178: 5, 200: 1}))
        m = sm.m_of_headers(names, im.mates)
        p = sm.parities(m, 300)
        bounds = _boundaries(300)
        assert 150 in bounds and _run_of(names, 149) == (149, 151) and p[150] == 1  # between the two mates of a pair
        assert 100 in bounds and _run_of(names, 99) == (99, 100)  # right behind a single
        assert 200 in bounds and _run_of(names, 200) == (200, 201)  # right in front of a single
        assert 60 in bounds and _run_of(names, 60) == (59, 62)  # inside runs of 3, 4 and 5 equal names
        assert 120 in bounds and _run_of(names, 120) == (118, 122)
        assert 180 in bounds and _run_of(names, 180) == (178, 183)
        tail = {"features": b"", "no_final_newline": None, "trailing_1_line": b"@x\n", "trailing_3_lines": b"@x\nACGT\n+\n"}[name]
        return names, tail, 2100, 4000
    if name == "run_of_70":
        # W = 2: the boundary 150 lies near the end of a run of 70, 66 of its records in front: the 64 m of the first tail
        # window are all true, one widening finds the run's start
        names = _names(_layout(300, {84: 70}))
        assert 150 in _boundaries(300) and _run_of(names, 150) == (84, 154)
        m = sm.m_of_headers(names, im.mates)
        assert len(sm.tail_fn(m, 0, 150)[1]) == 2
        return names, b"", 97, 3000
    if name == "one_name_shares":
        # W = 8: the shares [75, 112) (37 records) and [187, 225) (38 records) are one name throughout, so the entries of the
        # ranks behind them follow from the rank two before
        names = _names(_layout(300, {70: 50, 183: 47}))
        for a, b in ((75, 112), (187, 225)):
            assert (a, b) in [sm.shard_range(300, r, 8) for r in range(8)] and _run_of(names, a)[0] < a and _run_of(names, a)[1] > b
        m = sm.m_of_headers(names, im.mates)
        assert sm.share_fn(m, 75, 112) == sm.FLIP and sm.share_fn(m, 187, 225) == sm.ID
        return names, b"", 1500, 2500
    if name == "fewer_records_than_ranks":
        return _names([1, 2, 2]), b"", 97, None  # T = 5 < W = 8
    raise KeyError(name)


SHAPES = ["features", "no_final_newline", "trailing_1_line", "trailing_3_lines", "run_of_70", "one_name_shares", "fewer_records_than_ranks"]
LONG_RUNS = {"run_of_70"}  # (the bound on the tail pass holds for the others, whose longest run is checked below)


@pytest.fixture(scope="module")
def reads():
    g, f, r = sg._synth_reads(150, seed=11)
    return g, list(f) + list(r)


def _text(names, tail, seqs):
    recs = [h + b"\n" + seqs[k % len(seqs)].encode() + b"\n+\n" + b"I" * len(seqs[k % len(seqs)]) + b"\n" for k, h in enumerate(names)]
    text = b"".join(recs)
    return text[:-1] if tail is None else text + tail


def _play(host, ctx, path, world, singles, counter=None):
    """the three passes for every rank, the exchange by hand: (streams' results per rank, ShardCounts) or the reason"""
    mine = [host.InterleavedStream.shard_count(path, ctx, rank, world) for rank in range(world)]
    assert all(sc.failure is None for sc in mine)
    everyone = [list(sc.message) for sc in mine]
    assert len({len(v) for v in everyone}) == 1  # (padded to one length)
    whys = [host.InterleavedStream.shard_tail(sc, everyone) for sc in mine]
    assert len(set(whys)) == 1
    if whys[0] is not None:
        return whys[0], mine
    assert all(sc.failure is None for sc in mine)
    tails = [list(sc.tail_message) for sc in mine]
    out = []
    for rank in range(world):
        fs, why = host.InterleavedStream.shard_open(mine[rank], tails, lambda vals: [list(vals)] * world, block_pairs=64, singles=singles)
        assert why is None
        seqs, lens, err = [], [], None
        try:
            block = fs.next_block()
            while block is not None:
                o, ln, _ = block.unpack()
                seqs.append(o.copy())
                lens.append(ln.copy())
                if counter is not None:
                    counter.add(block)
                    ctx.sync()
                block.free()
                block = fs.next_block()
        except ValueError as e:
            err = e
        out.append(dict(fs=fs, info=fs.info, seqs=seqs, lens=lens, err=err))
        fs.close()
    return out, mine


@pytest.mark.parametrize("shape", SHAPES)
def test_one_process_plays_every_rank(host, ctx, tmp_path, monkeypatch, reads, shape):
    g, seqs = reads
    names, tail, block, chunk = _shape(shape)
    text = _text(names, tail, seqs)
    total = len(names)
    m = sm.m_of_headers(names, im.mates)
    p = sm.parities(m, total)
    longest = max(_run_of(names, j)[1] - _run_of(names, j)[0] for j in range(total))
    assert (longest >= 64) == (shape in LONG_RUNS)  # the premise of the bound on the tail pass
    path = _write_bgzf(tmp_path, "il.fq.gz", text, block)
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    off, state, size = host.bgzf_walk_file(path)
    n_members = len(off) - 1
    single = host.InterleavedStream(path, ctx, block_pairs=64, singles=True)
    want_seq, want_len = bs._blocks(single)
    want = single.info
    single.close()
    w_pairs, w_info = host.fastq_mates(text, True)
    assert (want["pairs"], want["singles"], want["records"]) == (w_info["pairs"], w_info["singles"], total) and total == w_info["records"]
    recs = im.records(text)
    ref = pe_oracle_c.Oracle(g.seqs, 21).count_pairs([recs[int(a)][1].decode() for a, _ in w_pairs], [recs[int(b)][1].decode() for _, b in w_pairs])
    ctx.build_index(g.seqs, 21)
    for world in WORLDS:
        counter = host.PeCounter(ctx)
        got, mine = _play(host, ctx, path, world, True, counter)
        assert sum(sc.members_pass1 for sc in mine) == n_members, world  # every member inflated exactly once in the count pass
        first = 0
        for rank, (res, sc) in enumerate(zip(got, mine)):
            fs, info = res["fs"], res["info"]
            a, b = sm.shard_range(total, rank, world)
            assert (fs.first_record, fs.records, fs.total_records, fs.members) == (a, b - a, total, n_members) and first == a
            assert fs.entry == p[a], (world, rank)
            pairs, singles = sm.owned(m, total, a, b)
            assert (info["pairs"], info["singles"], info["records"]) == (len(pairs), len(singles), 2 * len(pairs) + len(singles)), (world, rank)
            assert info["file_bytes"] == int(off[fs.plan[2]] - off[fs.plan[0]]), (world, rank)  # the reader reads its range and no more
            if b - a > fs.entry:
                assert fs.plan == host.bgzf_shard_plan(sc.counts, sc.open_end, a, min(b + 1, total))
            if shape not in LONG_RUNS and rank < world - 1 and a < b < total:
                lo_m, _, hi_m = host.bgzf_shard_plan(sc.counts, sc.open_end, max(a, b - 64), b + 1)
                assert 0 < fs.members_tail <= hi_m - lo_m, (world, rank)  # no more members than hold its last 65 records
            if rank == world - 1 or a == b or b == total:
                assert fs.members_tail == 0
            first = b
        assert first == total
        if shape in LONG_RUNS and world == 2:  # one widening: the last 64 records, then the share from its start
            assert sm.tail_fn(m, 0, 150)[1] == [(86, 150), (0, 150)]
            spans = [host.bgzf_shard_plan(mine[0].counts, mine[0].open_end, lo, 151) for lo in (86, 0)]
            assert mine[0].members_tail == sum(e - a for a, _, e in spans)
        assert np.array_equal(np.concatenate([x for r in got for x in r["lens"]] or [np.zeros(0, np.uint32)]), want_len), world
        assert np.array_equal(np.concatenate([x for r in got for x in r["seqs"]] or [np.zeros(0, np.uint8)]), want_seq), world
        for key in ("pairs", "singles", "records"):
            assert sum(r["info"][key] for r in got) == want[key], (world, key)
        node_mat, short_mat, stats = counter.result()
        assert np.array_equal(node_mat, ref[0]) and np.array_equal(short_mat, ref[1]), world
        assert stats == tuple(int(x) for x in ref[2]), world


# ---- strict mode, played the same way ------------------------------------------------------------------------------------
def _strict_message(host, ctx, path):
    fs = host.InterleavedStream(path, ctx, block_pairs=64)
    try:
        with pytest.raises(ValueError) as err:
            for block in fs:
                block.free()
        return str(err.value)
    finally:
        fs.close()


def test_strict_mode_names_the_smallest_record_in_the_single_process_words(host, ctx, tmp_path, monkeypatch, reads):
    g, seqs = reads
    monkeypatch.setenv("VS_STREAM_CHUNK", "4000")
    valid = _names([2] * 150)
    path = _write_bgzf(tmp_path, "valid.fq.gz", _text(valid, b"", seqs), 2100)
    single = host.InterleavedStream(path, ctx, block_pairs=64)
    want_seq, want_len = bs._blocks(single)
    single.close()
    got, _ = _play(host, ctx, path, 3, False)
    assert all(r["err"] is None for r in got) and sum(r["info"]["pairs"] for r in got) == 150
    assert np.array_equal(np.concatenate([x for r in got for x in r["lens"]]), want_len)
    assert np.array_equal(np.concatenate([x for r in got for x in r["seqs"]]), want_seq)
    # W = 3, shares [0, 100), [100, 200), [200, 300)
    for name, planted, failing in (("one_in_rank_1", {140: 1}, {1: 140}), ("rank_0_and_rank_2", {30: 1, 251: 1}, {0: 30, 2: 251})):
        names = _names(_layout(300, planted))
        path = _write_bgzf(tmp_path, name + ".fq.gz", _text(names, b"", seqs), 2100)
        message = _strict_message(host, ctx, path)
        smallest = min(planted)
        assert message.startswith("%s: record %d (\"%s\") has no mate beside it: what follows it is \"%s\"" % (
            path, smallest, names[smallest].decode(), names[smallest + 1].decode()))
        got, _ = _play(host, ctx, path, 3, False)
        firsts = {}
        for rank, res in enumerate(got):
            if res["err"] is not None:
                firsts[rank] = int(str(res["err"])[len(path + ": record "):].split(" ", 1)[0])
        assert firsts == failing  # every rank's first single is a single of the whole file
        winner = min(firsts, key=firsts.get)
        assert str(got[winner]["err"]) == message  # byte for byte: path, file-wide record number, both header lines


# ---- the fallbacks, from gathered values ----------------------------------------------------------------------------------
def test_the_ranks_fall_back_together_from_gathered_values(host, ctx, tmp_path, monkeypatch, reads):
    g, seqs = reads
    text = _text(_names([2] * 150), b"", seqs)
    at = text.index(b"\n", len(text) * 4 // 5)
    shapes = {"a carriage return or a byte >= 0x80": bz.bgzf(text[:at] + b"\r" + text[at:], block=5000),
              "not whole BGZF": bz.bgzf(text, block=5000, eof=False) + gzip.compress(b"")}
    for reason, data in shapes.items():
        p = tmp_path / "il.fq.gz"
        p.write_bytes(data)
        got, mine = _play(host, ctx, str(p), 3, True)
        assert got == reason
        if reason.startswith("a carriage"):
            assert [sc.message[3] for sc in mine] == [0, 0, 1]  # (the flags of the shares: one rank alone saw it)
    (tmp_path / "il.fq.gz").write_bytes(bz.bgzf(text, block=5000))
    monkeypatch.setenv("VS_BGZF_DEVICE", "0")
    got, mine = _play(host, ctx, str(tmp_path / "il.fq.gz"), 3, True)
    assert got == "VS_BGZF_DEVICE=0" and all(sc.members_pass1 == 0 for sc in mine)


def test_keep_mode_is_not_shared(host, ctx, tmp_path, reads):
    from vstrains_amd import _native as nat
    import ctypes as C

    path = _write_bgzf(tmp_path, "il.fq.gz", _text(_names([2] * 4), b"", reads[1]), None)
    h = C.c_void_p()
    rng = (C.c_uint64 * 3)(0, os.path.getsize(path), 0)
    assert nat.lib().vs_fastq_il_open_range(ctx._h, path.encode(), 2, rng, 8, 0, 0, 0, C.byref(h)) == nat.VS_E_ARG and not h.value


# ---- the drop-in under torchrun -----------------------------------------------------------------------------------------
def _torchrun_il(ranks, d, meta, path, out, report, flags, env=None, timeout=300):
    """``test_bgzf_shard_gpu._torchrun`` for one interleaved file and further flags"""
    env = dict(env or {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")},
               VS_DIST_BACKEND="gloo", VS_DIST_DEVICE="0", VS_INGEST_REPORT=str(report))
    for attempt in range(3):  # (a port that was free when asked for may be taken a moment later: ask again)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
             "--master-port", str(port), "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out),
             "-f", str(path), "-r", str(path), "-k", str(meta["k"]), "--interleaved", "--interleaved-shard"] + list(flags),
            cwd=ROOT, capture_output=True, text=True, env=env, timeout=timeout)
        if proc.returncode == 0 or "address already in use" not in proc.stderr:
            break
    return proc


def _golden_texts():
    """the reads of the golden case errors_k21 under one name per pair (alternately /1 /2 and a comment)"""
    name, d, meta = bs._case("errors_k21")
    out = []
    for which, f in enumerate(("fwd.fq", "rve.fq")):
        with open(os.path.join(d, f), "rb") as fh:
            recs = im.records(fh.read())
        for k, rec in enumerate(recs):
            rec[0] = (b"@q%d/%d" % (k, which + 1)) if k % 2 else (b"@q%d %d:N:0:1" % (k, which + 1))
        out.append(b"".join(b"\n".join(rec) + b"\n" for rec in recs))
    return d, meta, out[0], out[1]


@pytest.mark.parametrize("ranks", [2, 3, 8])
@pytest.mark.parametrize("kind", ["pairs", "singles_among_them"])
def test_sharded_drop_in_shares_the_interleaved_file_by_member(tmp_path, ranks, kind):
    d, meta, tf, tr = _golden_texts()
    text = im.interleave(tf, tr) if kind == "pairs" else im.with_singles(tf, tr)
    pairs, singles, _, total = im.pairing(text)
    assert len(pairs) == 300 and (len(singles) == 0 if kind == "pairs" else 8 <= len(singles) <= 14)
    data = bz.bgzf(text, block=2100)
    (tmp_path / "il.fq.gz").write_bytes(data)
    n_members = len(bz.py_walk(data)[0])
    out = tmp_path / "aln"
    out.mkdir()
    (out / "stale_file").write_text("x")
    proc = _torchrun_il(ranks, d, meta, tmp_path / "il.fq.gz", out, tmp_path / "report", [] if kind == "pairs" else ["--interleaved-singles"])
    assert proc.returncode == 0, proc.stderr[-3000:]
    bs._same_files(out, d)
    assert proc.stdout.count("result stored in:") == 1  # rank 0 only
    assert [l for l in proc.stdout.splitlines() if l.startswith("Number of processed reads")] == meta["progress_lines"]
    reports = bs._reports(tmp_path / "report", ranks)
    print(reports)
    assert all(r["path"] == "il_members" and r["reason"] is None and r["world"] == ranks and r["members"] == [n_members] for r in reports)
    first = 0
    for r in reports:  # the shares tile the records in rank order
        assert r["first_record"] == first and r["total_records"] == total
        first += r["records"]
    assert first == total and sum(r["pairs"] for r in reports) == 300
    assert sum(r["members_pass1"][0] for r in reports) == n_members


def test_sharded_drop_in_leaves_a_file_it_cannot_share_to_rank_0(tmp_path):
    d, meta, tf, tr = _golden_texts()
    text = im.interleave(tf, tr)
    cut = text.index(b"\n@", len(text) // 2) + 1
    (tmp_path / "il.fq.gz").write_bytes(bz.bgzf(text[:cut], block=2100, eof=False) + gzip.compress(text[cut:]))
    out = tmp_path / "aln"
    proc = _torchrun_il(2, d, meta, tmp_path / "il.fq.gz", out, tmp_path / "report", [])
    assert proc.returncode == 0, proc.stderr[-3000:]
    bs._same_files(out, d)
    reports = bs._reports(tmp_path / "report", 2)
    assert all(r["path"] == "il_whole_file_rank0" and r["reason"] == "not whole BGZF" for r in reports)
    assert [r["pairs"] for r in reports] == [300, 0]


def test_a_single_in_the_share_of_rank_1_fails_every_rank_in_the_single_process_words(tmp_path):
    from test_interleaved_gpu import _il_drop_in

    d, meta, tf, tr = _golden_texts()
    recs = im.records(im.interleave(tf, tr))
    recs.insert(450, [b"@lonely", b"ACGTACGTACGTACGTACGTACGTA", b"+", b"I" * 25])  # (behind 225 pairs: rank 1 of 2 owns [300, 601))
    text = b"".join(b"\n".join(rec) + b"\n" for rec in recs)
    assert im.pairing(text)[1] == [450] and len(recs) == 601
    (tmp_path / "il.fq.gz").write_bytes(bz.bgzf(text, block=2100))
    one = _il_drop_in(d, meta, str(tmp_path / "il.fq.gz"), tmp_path / "aln_one", ["--interleaved"])
    assert one.returncode != 0
    line = sg._exception_line(one.stderr)
    assert "%s: record 450 (\"@lonely\") has no mate beside it" % (tmp_path / "il.fq.gz") in line
    out = tmp_path / "aln"
    t0 = time.time()
    proc = _torchrun_il(2, d, meta, tmp_path / "il.fq.gz", out, tmp_path / "report", [])
    took = time.time() - t0
    print(took, proc.stderr[-1500:])
    assert proc.returncode != 0 and took < 150
    assert line in proc.stderr  # rank 1, in the words of the single process
    assert "rank 1 found record 450 without its mate beside it" in proc.stderr  # rank 0
    assert not (out / "pe_info").exists() and not (out / "st_info").exists()
    assert not any(l.startswith("Number of processed reads") for l in proc.stdout.splitlines())
