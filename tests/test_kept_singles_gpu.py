"""The kept records without a mate on the device: the compaction kernels of one pair of windows
(``vs_fastq_join_singles_text``) against the host twin and the model of tests/kept_singles_model.py at the wavefront and
workgroup edges; ``PairedNameStream(singles="keep")`` in every form the reader knows and ``BamStream(by_name=True,
singles="keep")`` against the streams that drop plus the plain model of the unpaired reads; the two commands with
``--count-singles`` in its two new homes; and that the parent's library and commands refuse all of it."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bam_mate_model as mm
import bam_util as bu
import bgzf_util as bz
import interleaved_model as im
import kept_singles_model as km
import pair_names_cases as pc
import pair_names_model as pm
import test_fastq_stream_gpu as sg
import unpaired_model
from conftest import ROOT, pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu

K = 21
EOFS = [(True, True), (False, False), (True, False), (False, True)]
EOF_IDS = ["eof", "more_to_come", "file_1_ended", "file_2_ended"]
CASES = pc.cases() + km.cases()


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


def as_lists(got):
    pairs, s0, s1, info = got
    return [tuple(int(x) for x in p) for p in pairs], [int(r) for r in s0], [int(r) for r in s1], info


# ---- the kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eof", EOFS, ids=EOF_IDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_kernels_equal_the_host_twin(host, ctx, case, eof):
    name, t0, t1, opts = case
    dev = as_lists(host.fastq_join_singles(t0, t1, eof[0], eof[1], ctx, guard=64, **opts))  # (raises if a sentinel word around a list changed)
    twin = as_lists(host.fastq_join_singles(t0, t1, eof[0], eof[1], **opts))
    assert dev == twin
    assert (dev[1], dev[2]) == km.window_singles(t0, t1, *eof)


def _edges(n):
    """record positions at the first and last lane of a wavefront and at the first and last record of a workgroup"""
    return sorted(p for p in {0, 63, 64, 127, 255, 256, 511, 512, n - 1} if 0 <= p < n)


@pytest.mark.parametrize("file", [0, 1], ids=["singles_in_file_1", "singles_in_file_2"])
@pytest.mark.parametrize("n", km.window_sizes())
def test_singles_at_the_wavefront_and_workgroup_edges(host, ctx, n, file):
    """windows of n records of the file that holds the singles (0, 1, 63, 64, 65, PN_TPB - 1, PN_TPB, PN_TPB + 1, 2 PN_TPB + 1);
    the singles at the edges, each alone and all together; every way the files can be at their ends, so that what is decided
    is nothing, every record, or ends inside a wavefront (behind the last match); short tables and two-bit hashes, so that
    long probe chains do not change the lists"""
    placements = [[p] for p in _edges(n)] + [_edges(n)] + ([list(range(n))] if n else [[]]) + ([[n - 2, n - 1]] if n > 2 else [])
    seen_dec = set()
    for at in placements:
        t0, t1 = km.placed(n, at, file)
        n_all = n + n - len(at)
        table = 2
        while table < n_all:
            table <<= 1
        for eof in EOFS:
            want_pairs, want_info = pm.join(t0, t1, *eof)
            want = km.window_singles(t0, t1, *eof)
            for opts in (dict(), dict(name_bits=2), dict(table=table), dict(table=table, name_bits=1)):
                got = as_lists(host.fastq_join_singles(t0, t1, eof[0], eof[1], ctx, guard=64, **opts))
                assert got[0] == want_pairs and got[3] == want_info and (got[1], got[2]) == want, (at, eof, opts)
            seen_dec.add((want_info["decided"][file], len(want[file])))
        assert km.window_singles(t0, t1)[file] == at  # (at the end of both files every lone record is listed, where it was put)
    if n:
        assert any(d == 0 for d, _ in seen_dec) and any(d == n and k for d, k in seen_dec)  # nothing decided; every record decided, singles among them
    if n > 65:
        assert any(0 < d < n and d % 64 for d, _ in seen_dec)  # the decision ends inside a wavefront


def test_a_decision_inside_a_wavefront_lists_only_what_lies_below_it(host, ctx):
    """300 records in file 1: mates up to record 199 with lone records among them, 100 lone records behind; more text to come"""
    h0, h1 = pc.mates_files(200)
    lone = lambda tag, k: b"@%s%d" % (tag, k)
    f0 = []
    for k, h in enumerate(h0):
        if k in (0, 63, 64, 100, 190):
            f0.append(lone(b"in", k))
        f0.append(h)
    f0 += [lone(b"tail", k) for k in range(100)]
    t0, t1 = pc.text(f0), pc.text(h1, 3)
    dev = as_lists(host.fastq_join_singles(t0, t1, False, False, ctx))
    assert dev[3]["decided"] == (205, 200) and dev[1] == [0, 64, 66, 103, 194] and dev[2] == []
    assert dev == as_lists(host.fastq_join_singles(t0, t1, False, False))
    dev = as_lists(host.fastq_join_singles(t0, t1, False, True, ctx))
    assert dev[3]["decided"] == (305, 200) and dev[1] == [0, 64, 66, 103, 194] + list(range(205, 305))


@pytest.mark.parametrize("case", pc.sequences(), ids=lambda c: c[0])
def test_window_sequences_through_the_kernels(host, ctx, case):
    name, t0, t1, e0, e1 = case
    pairs, singles, rounds = km.drive(lambda *a: as_lists(host.fastq_join_singles(*a, ctx=ctx)), t0, t1, e0, e1)
    assert (singles[0], singles[1]) == km.whole_file_singles(t0, t1) and pairs == pm.join(t0, t1)[0]


# ---- what the parent refuses --------------------------------------------------------------------------------------------------
def test_the_library_takes_the_two_new_modes(host, ctx, tmp_path):
    """``vs_fastq_pn_open(mode = 2)`` and ``vs_bam_stream_open_mode(mode = 2)``: VS_E_ARG before this change"""
    import ctypes as C

    from vstrains_amd import _native as nat

    f, r, bam = tmp_path / "f.fq", tmp_path / "r.fq", tmp_path / "a.bam"
    f.write_bytes(pc.text([b"@a/1", b"@b/1"]))
    r.write_bytes(pc.text([b"@b/2"]))
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT")]))
    h = C.c_void_p()
    assert nat.lib().vs_fastq_pn_open(ctx._h, str(f).encode(), str(r).encode(), 2, C.byref(h)) == nat.VS_OK
    nat.lib().vs_fastq_pn_close(h)
    assert nat.lib().vs_fastq_pn_open(ctx._h, str(f).encode(), str(r).encode(), 3, C.byref(h)) == nat.VS_E_ARG
    h = C.c_void_p()
    assert nat.lib().vs_bam_stream_open_mode(ctx._h, str(bam).encode(), 2, C.byref(h)) == nat.VS_OK
    nat.lib().vs_bam_stream_close(h)
    assert nat.lib().vs_bam_stream_open_mode(ctx._h, str(bam).encode(), 3, C.byref(h)) == nat.VS_E_ARG
    # the smallest streams: one pair and one kept single; one kept singleton
    fs = host.PairedNameStream(str(f), str(r), ctx, singles="keep")
    blocks = [(b.unpaired, [int(x) for x in b.unpack()[1]], [int(x) for x in b.unpack()[2]]) for b in fs]
    fs.close()
    assert blocks == [(False, [4, 1], [0, 0]), (True, [1, 0], [0, 8])]
    fs = host.BamStream(str(bam), ctx, by_name=True, singles="keep")
    blocks = [(b.unpaired, [int(x) for x in b.unpack()[1]], [int(x) for x in b.unpack()[2]]) for b in fs]
    assert blocks == [(True, [4, 0], [0, 8])] and fs.info["singletons"] == 1
    fs.close()


# ---- the streams ------------------------------------------------------------------------------------------------------------
def _counters(host, ctx, blocks):
    counter = host.PeCounter(ctx)
    for b in blocks:
        counter.add(b)
    node_mat, short_mat, stats = counter.result()
    return node_mat, short_mat, stats, tuple(int(x) for x in counter.single_stats.cpu().numpy())


def _check_single_block(block, want, at, block_slots):
    """a singles block against the reads want[at:], in order; returns how many it holds"""
    assert block.unpaired
    text, lens, flags = block.unpack()
    n = len(lens) // 2
    assert len(lens) % 2 == 0 and 0 < n <= block_slots and not lens[1::2].any() and all(int(f) == 8 for f in flags[1::2])
    pos = 0
    for r in range(n):
        s = want[at + r]
        assert lens[2 * r] == len(s), (at + r)
        assert flags[2 * r] & 11 == (1 if "N" in s else 0) | (2 if set(s) - set("ACGTN") else 0), (at + r)  # (present: not flagged absent)
        assert bytes(text[pos:pos + len(s)]).decode() == "".join(c if c in "ACGT" else "A" for c in s), (at + r)
        pos += len(s)
    return n


def _pair_ends(blocks):
    """the ends of the pairs' blocks, in order: (lengths, flags, bases)"""
    got = [b.unpack() for b in blocks if not b.unpaired]
    cat = lambda i, dt: np.concatenate([np.asarray(g[i], dtype=dt) for g in got]) if got else np.zeros(0, dtype=dt)
    return cat(1, np.int64), cat(2, np.int64), cat(0, np.uint8)


@pytest.fixture(scope="module")
def pn_workload(host, ctx):
    """a graph; two FASTQ files of about 1 000 records each, in one order, that lack records of each other: at record 0 and at
    the last record of either file, a run of twelve in a row, three per hundred at random -- reads with an N, reads shorter
    than k + 1 and an empty sequence line among the records without a mate"""
    from vstrains_amd import synth

    st = synth.make_strains(6, 1500, 0.03, seed=61)
    g = synth.compact_dbg(st, K)
    n = 1000
    f, r = synth.sample_pairs(st, n, 100, seed=62, sub_rate=0.01, n_rate=0.02)
    rng = random.Random(63)
    seqs = [[s[:rng.randrange(40, 101)] for s in f], [s[:rng.randrange(40, 101)] for s in r]]
    # the records only one file has
    only = [set(), set()]
    only[0] |= {0, n - 1} | set(range(400, 412)) | {20, 21, 22}
    only[1] |= {1, n - 2} | set(range(700, 712)) | {30, 31}
    for k in range(2, n - 2):
        if k not in only[0] and k not in only[1] and rng.random() < 0.03:
            only[rng.randrange(2)].add(k)
    seqs[0][20] = seqs[0][20][:K]                            # shorter than k + 1
    seqs[0][21] = ""                                         # an empty sequence line
    seqs[0][22] = seqs[0][22][:30] + "N" + seqs[0][22][31:]  # an N
    seqs[1][30] = seqs[1][30][:K - 5]
    seqs[1][31] = "N" + seqs[1][31][1:]
    heads = pc.mates_files(n)
    texts = []
    for fl in (0, 1):
        texts.append(b"".join(heads[fl][k] + b"\n" + seqs[fl][k].encode() + b"\n+\n" + b"I" * len(seqs[fl][k]) + b"\n"
                              for k in range(n) if k not in only[1 - fl]))
    want = km.whole_file_singles(*texts)
    reads = [[im.records(texts[fl])[i][1].decode() for i in want[fl]] for fl in (0, 1)]
    assert [len(x) for x in reads] == [len(only[0]), len(only[1])] and min(len(x) for x in reads) >= 20
    ctx.build_index(g.seqs, K)
    model = unpaired_model.Model(g.seqs, K)
    m_node, m_short, m_tally = model.count(reads[0] + reads[1])
    assert m_short.sum() > 0 and min(m_tally) > 0 and not m_node.any()  # used, N-holding and short reads are all among the singles
    return dict(g=g, texts=texts, reads=reads, model=(m_short, m_tally), records=[len(im.records(t)) for t in texts])


FORMS = ["plain_chunk61", "plain", "gzip", "bgzf", "fifo"]


@pytest.mark.parametrize("form", FORMS)
def test_paired_name_stream_keeps_its_singles(host, ctx, pn_workload, tmp_path, monkeypatch, form):
    w = pn_workload
    monkeypatch.setenv("VS_STREAM_CHUNK", "61" if form == "plain_chunk61" else "997")  # (singles in many rounds; the runs of twelve span cuts)
    make = {"plain_chunk61": lambda t: t, "plain": lambda t: t, "gzip": gzip.compress, "bgzf": lambda t: bz.bgzf(t, block=3000), "fifo": lambda t: t}[form]
    data = [make(t) for t in w["texts"]]
    ctx.build_index(w["g"].seqs, K)

    def run(mode):
        if form == "fifo":
            with sg.Fifos(tmp_path, data[0], data[1], names=("f_%s.fifo" % mode, "r_%s.fifo" % mode)) as (pf, pr):
                fs = host.PairedNameStream(pf, pr, ctx, block_pairs=37, singles=mode)
                try:
                    return list(fs), fs.info
                finally:
                    fs.close()
        (tmp_path / "f.fq").write_bytes(data[0])
        (tmp_path / "r.fq").write_bytes(data[1])
        fs = host.PairedNameStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, block_pairs=37, singles=mode)
        try:
            return list(fs), fs.info
        finally:
            fs.close()

    dropped, info_drop = run(True)
    kept, info_keep = run("keep")
    assert not any(b.unpaired for b in dropped)
    if form != "fifo":  # (a regular file comes in the same chunks every time: the same rounds, the same windows)
        assert info_keep == info_drop
    assert (info_keep["pairs"], info_keep["singles_fwd"], info_keep["singles_rve"]) == (info_drop["pairs"], info_drop["singles_fwd"], info_drop["singles_rve"])
    assert (info_keep["singles_fwd"], info_keep["singles_rve"]) == (len(w["reads"][0]), len(w["reads"][1]))
    assert 2 * info_keep["pairs"] + info_keep["singles_fwd"] + info_keep["singles_rve"] == sum(w["records"])
    if form == "plain_chunk61":
        assert info_keep["windows"] > 1000
    # every singles block holds reads of ONE file, the next of that file in its order
    at = [0, 0]
    n_blocks = 0
    for b in kept:
        if not b.unpaired:
            continue
        fl = 0 if _matches(b, w["reads"][0], at[0]) else 1
        at[fl] += _check_single_block(b, w["reads"][fl], at[fl], 37)
        n_blocks += 1
    assert at == [len(w["reads"][0]), len(w["reads"][1])] and n_blocks >= 2
    # the pairs are those of the stream that drops
    for got, want in zip(_pair_ends(kept), _pair_ends(dropped)):
        assert np.array_equal(got, want)
    if form != "fifo":
        assert [len(b.unpack()[1]) for b in kept if not b.unpaired] == [len(b.unpack()[1]) for b in dropped]
    # the counters: those of the drop run, plus the model of the unpaired reads
    want = _counters(host, ctx, dropped)
    have = _counters(host, ctx, kept)
    m_short, m_tally = w["model"]
    assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1] + m_short)
    assert have[2] == want[2] and want[3] == (0, 0, 0) and have[3] == m_tally


def _matches(block, reads, at):
    text, lens, _ = block.unpack()
    n = len(lens) // 2
    if at + n > len(reads) or [int(x) for x in lens[0::2]] != [len(s) for s in reads[at:at + n]]:
        return False
    return bytes(text).decode() == "".join(c if c in "ACGT" else "A" for s in reads[at:at + n] for c in s)


def _revcomp(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


@pytest.fixture(scope="module")
def bam_workload(host, ctx):
    """300 pairs of a small graph as BAM records in a shuffled order, every seventh pair without one of its mates; singletons of
    both classes at the first two and the last two records; among the singletons one with 0x10 whose bases are no reverse
    palindrome, one without bases, one of odd length, one with an N, one shorter than k + 1"""
    from vstrains_amd import synth

    st = synth.make_strains(4, 1500, 0.03, seed=71)
    g = synth.compact_dbg(st, K)
    f, r = synth.sample_pairs(st, 306, 100, seed=72, sub_rate=0.01, n_rate=0.02)
    rng = random.Random(73)

    def rec(name, cls, s, reverse=None):
        reverse = rng.random() < 0.5 if reverse is None else reverse
        return bu.rec(name, bu.PAIRED | cls | 0xC | (bu.REVERSE if reverse else 0), _revcomp(s) if reverse else s)

    body = []
    for i in range(300):
        ends = [rec("q%d" % i, bu.FIRST, f[i]), rec("q%d" % i, bu.SECOND, r[i])]
        if i % 7 == 3:
            ends.pop(rng.randrange(2))
        body += ends
    body = mm.shuffled(body, 74)
    body.insert(100, bu.rec("other", 0, "ACGT"))              # class "other": takes no part, kept or not
    body.insert(200, bu.rec("q5", 0x900 | 0x41, "ACGT"))      # secondary: dropped
    asym = f[300][:99]                                        # odd length, stored reversed: no reverse palindrome
    assert len(asym) % 2 == 1 and _revcomp(asym) != asym
    special = [bu.rec("no_bases", bu.PAIRED | bu.FIRST, ""), rec("with_n", bu.SECOND, f[301][:50] + "N" + f[301][51:], reverse=True),
               rec("short", bu.FIRST, f[302][:K], reverse=False)]
    for k, s in enumerate(special):
        body.insert(150 + 37 * k, s)
    records = [rec("first_rec", bu.FIRST, asym, reverse=True), rec("second_rec", bu.SECOND, r[303], reverse=False)] + body + [
        rec("before_last", bu.FIRST, f[304], reverse=False), rec("last_rec", bu.SECOND, r[305], reverse=True)]
    waiting, reads = km.bam_singletons(records)
    assert waiting[:2] == [0, 1] and waiting[-2:] == [len(records) - 2, len(records) - 1] and len(waiting) > 40
    assert {bu.classify(records[i].flag) for i in waiting[:2] + waiting[-2:]} == {bu.C_FIRST, bu.C_SECOND}
    assert "" in reads and asym in reads and any("N" in s for s in reads) and any(0 < len(s) <= K for s in reads)
    assert records[0].flag & bu.REVERSE and records[0].seq != reads[0] == asym
    ctx.build_index(g.seqs, K)
    model = unpaired_model.Model(g.seqs, K)
    m_node, m_short, m_tally = model.count(reads)
    assert m_short.sum() > 0 and min(m_tally) > 0
    return dict(g=g, records=records, reads=reads, model=(m_short, m_tally))


@pytest.mark.parametrize("block", [1, 1000], ids=["block1", "block1000"])
def test_bam_stream_by_name_keeps_its_singletons(host, ctx, bam_workload, tmp_path, monkeypatch, block):
    w = bam_workload
    monkeypatch.setenv("VS_STREAM_CHUNK", "300")  # (the singletons are carried through many windows)
    monkeypatch.setenv("VS_BAM_SEG", "64")
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(w["records"], block=300))
    ctx.build_index(w["g"].seqs, K)

    def run(singles):
        fs = host.BamStream(str(bam), ctx, block_pairs=block, by_name=True, singles=singles)
        try:
            return list(fs), fs.info
        finally:
            fs.close()

    dropped, info_drop = run(None)
    kept, info_keep = run("keep")
    assert info_keep == info_drop and info_keep["singletons"] == len(w["reads"]) and info_keep["windows"] > 20 and info_keep["waiting_max"] >= 2
    assert not any(b.unpaired for b in dropped)
    kinds = [b.unpaired for b in kept]
    assert kinds == sorted(kinds)  # (the singles blocks come at the end of the input, behind every pair)
    at = 0
    for b in kept:
        if b.unpaired:
            at += _check_single_block(b, w["reads"], at, block)
    assert at == len(w["reads"]) and sum(kinds) == (len(w["reads"]) if block == 1 else 1)
    for got, want in zip(_pair_ends(kept), _pair_ends(dropped)):
        assert np.array_equal(got, want)
    want = _counters(host, ctx, dropped)
    have = _counters(host, ctx, kept)
    m_short, m_tally = w["model"]
    assert np.array_equal(have[0], want[0]) and np.array_equal(have[1], want[1] + m_short)
    assert have[2] == want[2] and want[3] == (0, 0, 0) and have[3] == m_tally


def test_bam_keep_needs_the_match_by_name_and_no_member_range(host, ctx, tmp_path):
    bam = tmp_path / "a.bam"
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    with pytest.raises(ValueError, match="needs by_name=True"):
        host.BamStream(str(bam), ctx, singles="keep")
    fs = host.BamStream(str(bam), ctx, by_name=True, singles="keep")  # (a file without singletons: its pair, no singles block)
    assert [(b.unpaired, len(b.unpack()[1])) for b in fs] == [(False, 2)] and fs.info["singletons"] == 0
    fs.close()


# ---- the commands ------------------------------------------------------------------------------------------------------------
def _strip(out, tag):
    return [l.replace(tag, "X") for l in out.splitlines() if not l.startswith("Global time elapsed")]


def _pe_inference(d, meta, fwd, rve, out, flags):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/", "-f", str(fwd),
                           "-r", str(rve), "-k", str(meta["k"])] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _damaged_pair(tf: bytes, tr: bytes, seeds):
    """the two files under one name per pair, some three records per hundred deleted from each"""
    h0, h1 = pc.mates_files(len(im.records(tf)))
    out = []
    for heads, t, seed in ((h0, tf, seeds[0]), (h1, tr, seeds[1])):
        rng = random.Random(seed)
        out.append(b"".join(b"\n".join([h] + rec[1:]) + b"\n" for h, rec in zip(heads, im.records(t)) if rng.random() >= 0.03))
    return out


def _seqs(text: bytes, which=None):
    recs = im.records(text)
    return [recs[i][1].decode() for i in (range(len(recs)) if which is None else which)]


def _fastq(reads, tag=b"s") -> bytes:
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s.encode(), b"I" * len(s)) for i, s in enumerate(reads))


def test_pe_inference_counts_the_singles_of_two_files_joined_by_name(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    df, dr = _damaged_pair(*(open(os.path.join(d, f), "rb").read() for f in ("fwd.fq", "rve.fq")), seeds=(5, 6))
    (tmp_path / "df.fq").write_bytes(df)
    (tmp_path / "dr.fq").write_bytes(dr)
    r1, r2, s1, s2 = pm.filtered(df, dr)
    want = km.whole_file_singles(df, dr)
    singles = _seqs(df, want[0]) + _seqs(dr, want[1])
    assert (len(want[0]), len(want[1])) == (s1, s2) and s1 > 3 and s2 > 3
    flags = ["--check-names", "--check-names-singles"]
    drop = _pe_inference(d, meta, tmp_path / "df.fq", tmp_path / "dr.fq", tmp_path / "aln_drop", flags)
    got = _pe_inference(d, meta, tmp_path / "df.fq", tmp_path / "dr.fq", tmp_path / "aln_keep", flags + ["--count-singles"])
    assert drop.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    assert (tmp_path / "aln_keep" / "pe_info").read_bytes() == (tmp_path / "aln_drop" / "pe_info").read_bytes()
    model = unpaired_model.Model(seqs, meta["k"])
    node, pair_short, _ = pe_oracle.pe_matrices(seqs, _seqs(r1), _seqs(r2), meta["k"], table=model.table)
    _, m, t = model.count(singles)
    assert m.sum() > 0
    # without --count-singles: what the command wrote before (the files of the two files filtered to their shared names)
    assert (tmp_path / "aln_drop" / "pe_info").read_text() == pe_oracle.matrix_text(ids, node)
    assert (tmp_path / "aln_drop" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short)
    assert (tmp_path / "aln_keep" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short + m)
    joined = "Pairs joined by read name: %d; records without a mate %%s: %d of %s, %d of %s" % (len(im.records(r1)), s1, tmp_path / "df.fq", s2, tmp_path / "dr.fq")
    unpaired = "Unpaired reads of %s + %s: %d used, %d with N, %d shorter than k+1" % (tmp_path / "df.fq", tmp_path / "dr.fq", t[2], t[0], t[1])
    lines, before = _strip(got.stdout, "aln_keep"), _strip(drop.stdout, "aln_drop")
    assert joined % "dropped" in before and not any(l.startswith("Unpaired reads") for l in before)
    assert [l for l in lines if l != unpaired] == [joined % "counted as unpaired reads" if l == joined % "dropped" else l for l in before]
    assert lines.count(unpaired) == 1


def _bam_case(tf: bytes, tr: bytes, seed: int):
    """the pairs as BAM records in a shuffled order, every ninth pair without one of its mates: (records, R1 and R2 texts of the
    pairs by name, the singleton reads)"""
    import test_bam_gpu as bg

    records = mm.shuffled(bg._records_of_pair(tf, tr), seed)
    lose = {(b"q%d" % k, bu.C_FIRST if k % 2 else bu.C_SECOND) for k in range(4, 2000, 9)}
    records = [x for x in records if (x.name, bu.classify(x.flag)) not in lose]
    f1, f2, n_single = mm.fastq_pair_by_name(records)
    waiting, reads = km.bam_singletons(records)
    assert n_single == len(reads) > 10
    return records, f1, f2, reads


def test_pe_inference_counts_the_singletons_of_a_bam(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    records, f1, f2, reads = _bam_case(*(open(os.path.join(d, f), "rb").read() for f in ("fwd.fq", "rve.fq")), seed=9)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bu.write(records, block=5000))
    drop = _pe_inference(d, meta, bam, bam, tmp_path / "aln_drop", ["--bam-by-name"])
    got = _pe_inference(d, meta, bam, bam, tmp_path / "aln_keep", ["--bam-by-name", "--count-singles"])
    assert drop.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    assert (tmp_path / "aln_keep" / "pe_info").read_bytes() == (tmp_path / "aln_drop" / "pe_info").read_bytes()
    model = unpaired_model.Model(seqs, meta["k"])
    node, pair_short, _ = pe_oracle.pe_matrices(seqs, _seqs(f1), _seqs(f2), meta["k"], table=model.table)
    _, m, t = model.count(reads)
    assert m.sum() > 0
    assert (tmp_path / "aln_drop" / "pe_info").read_text() == pe_oracle.matrix_text(ids, node)
    assert (tmp_path / "aln_drop" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short)
    assert (tmp_path / "aln_keep" / "st_info").read_text() == pe_oracle.matrix_text(ids, pair_short + m)
    unpaired = "Unpaired reads of %s: %d used, %d with N, %d shorter than k+1" % (bam, t[2], t[0], t[1])
    lines, before = _strip(got.stdout, "aln_keep"), _strip(drop.stdout, "aln_drop")
    assert [l for l in lines if l != unpaired] == before and lines.count(unpaired) == 1 and unpaired not in before


def _cli(inp, fwd, rve, out, flags):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out), "-fwd", str(fwd),
                           "-rve", str(rve)] + flags, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _files(root):
    return sorted(os.path.relpath(os.path.join(base, f), root) for base, _, fs in os.walk(root) for f in fs)


def _log(out, word):
    return [l.split(" - ")[-1] for l in (out / "vstrains.log").read_text().splitlines() if word in l]


@pytest.mark.parametrize("source", ["check_names", "bam_by_name"])
def test_cli_counts_the_kept_records(tmp_path, source):
    """the whole command with --count-singles in its two new homes writes, file for file, what it writes for the host-side
    repair that the flag makes unnecessary: the pairs as two files and the records without a mate as ``--single FILE``"""
    from graph_case import Case

    inp = Case("two_strain_bubbles_k21").inputs(str(tmp_path), with_reads=True)
    tf, tr = (open(inp[f], "rb").read() for f in ("fwd", "rve"))
    if source == "check_names":
        df, dr = _damaged_pair(tf, tr, seeds=(7, 8))
        r1, r2, s1, s2 = pm.filtered(df, dr)
        want = km.whole_file_singles(df, dr)
        reads = _seqs(df, want[0]) + _seqs(dr, want[1])
        fwd, rve, flags = tmp_path / "df.fq.gz", tmp_path / "dr.fq", ["--check-names", "--check-names-singles"]
        fwd.write_bytes(bz.bgzf(df))
        rve.write_bytes(dr)
        dropped_line, single_path = "have no mate by name", "%s + %s" % (fwd, rve)
    else:
        records, r1, r2, reads = _bam_case(tf, tr, seed=10)
        fwd = rve = tmp_path / "reads.bam"
        fwd.write_bytes(bu.write(records))
        flags = ["--bam-by-name"]
        dropped_line, single_path = "records of the BAM have no mate", str(fwd)
    for f, data in (("r1.fq", r1), ("r2.fq", r2), ("singles.fq", _fastq(reads))):
        (tmp_path / f).write_bytes(data)
    repaired = _cli(inp, tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "out_repaired", ["--single", str(tmp_path / "singles.fq")])
    drop = _cli(inp, fwd, rve, tmp_path / "out_drop", flags)
    got = _cli(inp, fwd, rve, tmp_path / "out_keep", flags + ["--count-singles"])
    assert repaired.returncode == 0 and drop.returncode == 0 and got.returncode == 0, got.stderr[-3000:]
    files = _files(tmp_path / "out_repaired")
    assert {"strain.fasta", "strain.paths", "aln/pe_info", "aln/st_info"} <= set(files) and _files(tmp_path / "out_keep") == files
    for rel in files:
        if rel != "vstrains.log":  # (time stamps and paths)
            assert (tmp_path / "out_keep" / rel).read_bytes() == (tmp_path / "out_repaired" / rel).read_bytes(), rel
    assert (tmp_path / "out_keep" / "aln" / "pe_info").read_bytes() == (tmp_path / "out_drop" / "aln" / "pe_info").read_bytes()
    assert (tmp_path / "out_keep" / "aln" / "st_info").read_bytes() != (tmp_path / "out_drop" / "aln" / "st_info").read_bytes()
    # the log: kept records are not said to be dropped, and are said to be counted
    assert len(_log(tmp_path / "out_drop", dropped_line)) == 1 and _log(tmp_path / "out_keep", dropped_line) == []
    counted = _log(tmp_path / "out_keep", "unpaired reads of")
    assert len(counted) == 1 and counted[0].endswith("unpaired reads of %s were counted into the paired end information" % single_path)
    assert _log(tmp_path / "out_drop", "unpaired reads of") == []
    assert "Unpaired reads of %s: " % single_path in got.stdout and "Unpaired reads of" not in drop.stdout


# ---- the block builder (block_builder_cases.py): the refusal of an over-long end in the singles blocks of the three keep modes ------
def test_over_long_kept_single_is_refused(host, ctx, tmp_path):
    import block_builder_cases as bb
    from vstrains_amd import _native as nat

    fwd, rve = bb.edge_pairs(3)
    limit = bb.LONG - 1
    # interleaved: a single record between two pairs
    il = tmp_path / "il.fq"
    il.write_bytes(bb.fastq([fwd[0], rve[0]], [b"p0", b"p0"]) + bb.long_record(b"s") + bb.fastq([fwd[1], rve[1]], [b"p1", b"p1"]))
    bb.refused(host.InterleavedStream(str(il), ctx, singles="keep"), nat.NativeError, "%s: record 2 has a sequence line of more than %d bytes" % (il, limit))
    # two files by name: a record of file 2 without a mate
    (tmp_path / "f.fq").write_bytes(bb.fastq(fwd[:2], [b"a", b"b"]))
    (tmp_path / "r.fq").write_bytes(bb.fastq(rve[:1], [b"a"]) + bb.long_record(b"s") + bb.fastq(rve[1:2], [b"b"]))
    bb.refused(host.PairedNameStream(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx, singles="keep"), ValueError,
               "%s: record 1 has a sequence line of more than %d bytes" % (tmp_path / "r.fq", limit))
    # BAM by name: a record still waiting at the end of the file
    bam = tmp_path / "w.bam"
    good = [bu.rec("g0", bu.PAIRED | bu.FIRST, "ACGTACGTAC"), bu.rec("g0", bu.PAIRED | bu.SECOND, "TTGCA")]
    bam.write_bytes(bz.bgzf(bu.inflated(good) + bb.long_bam_record(b"w", bu.PAIRED | bu.FIRST), 1))
    bb.refused(host.BamStream(str(bam), ctx, by_name=True, singles="keep"), ValueError, "%s: record 2 has a sequence of more than %d bases" % (bam, limit))
