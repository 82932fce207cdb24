"""The base pileup on the device: ``k_node_pileup`` and the fold through ``PileupCounter`` on the constructed blocks of
tests/pileup_cases.py at k = 21, 55 and 127, against ``Context.contig_mems``, on a golden PE case, and through the two commands
(``vstrains_amd.node_depth --pileup --variants``, ``cli --depth-from-reads --depth-pileup``).  Every comparison is of exact
integers against tests/pileup_model.py."""
import os

import numpy as np
import pytest

import pileup_cases as cases
import pileup_model as model
from conftest import pe_cases
from oracle import pe_oracle
from test_node_depth_gpu import CLI_PAIRS, SYNTH, _cli, _fastq, _files, _node_depth

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


def _pack(host, ctx, case):
    return ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))


def _rows(offsets, depth, alt):
    cut = [(int(offsets[n]), int(offsets[n + 1])) for n in range(len(offsets) - 1)]
    return [depth[a:b].tolist() for a, b in cut], [alt[a:b].tolist() for a, b in cut]


def device_pileup(host, ctx, case, times: int = 1, fold_bound: int = 2 ** 32, M=None):
    """A constructed case through ``PileupCounter``, its block added ``times`` times -> (depth rows, alt rows, tallies, folds)."""
    ctx.build_index(case.seqs, case.k)
    counter = host.PileupCounter(ctx, max_mismatch=case.M if M is None else M, fold_bound=fold_bound)
    block = _pack(host, ctx, case)
    try:
        for _ in range(times):
            counter.add(block)
        offsets, depth, alt = counter.result()
        ctx.sync()
        assert offsets.dtype == depth.dtype == alt.dtype == np.int64 and len(offsets) == len(case.seqs) + 1
        assert depth.shape == (int(offsets[-1]),) and alt.shape == (int(offsets[-1]), 5)
        return _rows(offsets, depth, alt) + (counter.tallies(), counter.folds)
    finally:
        block.free()
        ctx.keep_masks(False)


ALL = [c for k in cases.KS for c in cases.pileup_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model(host, ctx, case):
    want_depth, want_alt, want_tally = model.pileup(case.seqs, case.k, case.ends, case.M)
    depth, alt, tally, folds = device_pileup(host, ctx, case)
    assert depth == want_depth
    assert alt == want_alt
    assert tally == want_tally and folds <= 1
    if case.tally is not None:
        assert tally == case.tally


def _named(k, name):
    return [c for c in cases.pileup_cases(k) if c.name == name][0]


@pytest.mark.parametrize("k", cases.KS)
def test_the_same_block_added_twice_doubles_every_count(host, ctx, k):
    case = _named(k, "flanks_of_31_to_65_bases_beyond_the_anchor")
    d1, a1, t1 = model.pileup(case.seqs, k, case.ends, case.M)
    depth, alt, tally, _ = device_pileup(host, ctx, case, times=2)
    assert max(d1[0]) >= 1 and sum(sum(a) for a in a1[0]) == 2 * len(case.ends)
    assert depth == [[2 * v for v in row] for row in d1]
    assert alt == [[[2 * v for v in a] for a in row] for row in a1]
    assert tally == (2 * t1[0], 2 * t1[1])


@pytest.mark.parametrize("k", cases.KS)
def test_a_fold_after_every_block_and_one_fold_at_the_end_give_the_same(host, ctx, k):
    both = [_named(k, "read_overhanging_the_segments_start_and_end_on_both_strands"), _named(k, "mismatch_at_the_overlaps_first_and_last_base")]
    assert both[0].seqs == both[1].seqs and both[0].ends != both[1].ends
    seqs = both[0].seqs
    want = model.pileup(seqs, k, both[0].ends + both[1].ends, 8)
    got = []
    for bound, folds in ((1, 2), (2 ** 32, 1)):
        ctx.build_index(seqs, k)
        counter = host.PileupCounter(ctx, fold_bound=bound)
        blocks = [_pack(host, ctx, c) for c in both]
        try:
            for b in blocks:
                counter.add(b)
            got.append(_rows(*counter.result()) + (counter.tallies(),))
            assert counter.folds == folds  # (bound 1: before the second block and before the result)
        finally:
            for b in blocks:
                b.free()
            ctx.keep_masks(False)
    assert got[0] == got[1] == want


@pytest.mark.parametrize("k", cases.KS)
def test_a_budget_of_zero_leaves_alt_empty(host, ctx, k):
    case = _named(k, "mismatch_at_the_overlaps_first_and_last_base")
    want = model.pileup(case.seqs, k, case.ends, 0)
    depth, alt, tally, _ = device_pileup(host, ctx, case, M=0)
    assert (depth, alt, tally) == want
    assert tally == (0, 5) and not any(any(a) for row in alt for a in row) and not any(any(row) for row in depth)
    exact = _named(k, "exact_read_forward_and_reverse_complemented")
    depth, alt, tally, _ = device_pileup(host, ctx, exact, M=0)
    assert tally == (2, 0) and sum(depth[0]) == 2 * (k + 1 + 20) and not any(any(a) for row in alt for a in row)


@pytest.mark.parametrize("k", cases.KS)
def test_with_the_budget_beyond_any_read_the_alignments_are_the_diagonals_of_contig_mems(host, ctx, k):
    """``alignments`` == the distinct (end, segment, strand, diagonal) among the maximal matches ``Context.contig_mems`` finds
    on the same block: once per diagonal, however many matches lie on it."""
    names = ("three_matches_on_one_diagonal", "flanks_of_31_to_65_bases_beyond_the_anchor", "one_substitution_in_the_middle_of_2K_plus_1_bases",
             "substitution_K_minus_1_and_K_bases_from_the_reads_start", "exactly_M_and_M_plus_1_mismatches")
    picked = [_named(k, n) for n in names]
    assert all(c.seqs == picked[0].seqs for c in picked)
    ends = [e for c in picked for e in c.ends]
    ctx.build_index(picked[0].seqs, k)
    counter = host.PileupCounter(ctx, max_mismatch=2 ** 31)
    block = ctx.pack(*host.encode_seqs(ends))
    try:
        counter.add(block)
        mems = ctx.contig_mems(block)
        alignments, rejected = counter.tallies()
    finally:
        block.free()
        ctx.keep_masks(False)
    diagonals = set((int(r[0]), int(r[2]), int(r[3]) - int(r[1])) for r in mems)
    assert rejected == 0 and alignments == len(diagonals) < len(mems)
    assert alignments == model.pileup(picked[0].seqs, k, ends, 2 ** 31)[2][0]


def test_a_golden_pe_case_equals_the_model(host, ctx):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]  # (300 pairs; the first case holds ten)
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fwd, rve = pe_oracle.fastq_sequences(os.path.join(d, "fwd.fq")), pe_oracle.fastq_sequences(os.path.join(d, "rve.fq"))
    n = min(len(fwd), len(rve), 300)
    ends = [e for pair in zip(fwd[:n], rve[:n]) for e in pair]
    want = model.pileup(seqs, meta["k"], ends, 8)
    depth, alt, tally, _ = device_pileup(host, ctx, cases.PileupCase(name, meta["k"], seqs, ends, "a golden case"))
    assert want[2][0] > n and (depth, alt, tally) == want


# ---- the commands -----------------------------------------------------------------------------------------------------
def planted_reads(seqs, fwd, rve):
    """The synthetic reads (exact copies of their strains) with something to find: in every second read that holds the 25
    bases around the middle of the longest segment, on either strand, the middle base is changed to ONE other base -- a minor
    variant at one position -- and every tenth forward read carries an N."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    seg = max(seqs, key=len)
    p = len(seg) // 2
    motif, alt = seg[p - 12:p + 13], cases._OTHER[seg[p]]
    rc_motif = model.revcomp(motif)
    seen = 0
    out = []
    for reads in (fwd, rve):
        done = []
        for i, r in enumerate(reads):
            for m, b in ((motif, alt), (rc_motif, comp[alt])):
                at = r.find(m)
                if at >= 0:
                    seen += 1
                    if seen % 2:
                        r = r[:at + 12] + b + r[at + 13:]
            if reads is fwd and i % 10 == 0:
                r = r[:5] + "N" + r[6:]
            done.append(r)
        out.append(done)
    return out[0], out[1], seen


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    from vstrains_amd import node_depth, synth

    c = synth.make_pipeline_case(n_pairs=CLI_PAIRS, **SYNTH)
    d = tmp_path_factory.mktemp("pileup_synth")
    raw = c.gfa_text.encode()
    (d / "graph.gfa").write_bytes(raw)
    (d / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(raw))
    (d / "contigs.paths").write_text(c.paths_text)
    ids, seqs = pe_oracle.read_gfa_segments(str(d / "graph.gfa"))
    fwd, rve, seen = planted_reads(seqs, c.fwd, c.rve)
    assert seen >= 8
    (d / "fwd.fq").write_bytes(_fastq(fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(rve, "2"))
    ends = [e for pair in zip(fwd, rve) for e in pair]
    depth, alt, tally = model.pileup(seqs, 55, ends, 8)
    rows = model.table_rows(ids, seqs, depth, alt)
    return d, rows, model.variant_records(rows), tally


def _table(path):
    import gzip

    with (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)) as fh:
        lines = fh.read().splitlines()
    assert lines[0].split("\t") == ["segment", "pos", "ref", "A", "C", "G", "T", "other"]
    return [tuple(v if i in (0, 2) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]


def _records(path):
    out = []
    for line in open(path).read().splitlines():
        if not line.startswith("#"):
            chrom, pos, _, ref, alt, qual, flt, info = line.split("\t")
            f = dict(kv.split("=") for kv in info.split(";"))
            assert qual == flt == "."
            out.append((chrom, int(pos), ref, alt, int(f["DP"]), int(f["AD"]), f["AF"]))
    return out


def test_node_depth_command_writes_the_models_table_and_records(synth_files):
    d, rows, records, tally = synth_files
    got = _node_depth(d / "graph.gfa", d / "out.gfa", d / "fwd.fq", d / "rve.fq", ["--pileup", str(d / "p.tsv.gz"), "--variants", str(d / "v.vcf")])
    assert got.returncode == 0, got.stderr[-3000:]
    assert len(records) > 0 and sum(r[7] for r in rows) > 0  # (the planted variant and the planted N)
    assert _table(d / "p.tsv.gz") == rows
    assert _records(d / "v.vcf") == records
    assert got.stdout.rstrip().endswith("; pileup in: %s; variants in: %s" % (d / "p.tsv.gz", d / "v.vcf"))


def test_cli_with_depth_pileup_writes_the_two_files(synth_files):
    d, rows, records, tally = synth_files
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_pileup", ["--depth-from-reads", "--depth-pileup"])
    assert got.returncode == 0, got.stderr[-3000:]
    assert set(["gfa/graph_depth.gfa", "gfa/graph_depth.pileup.tsv", "gfa/graph_depth.vcf"]) <= set(_files(d / "out_pileup"))
    assert _table(d / "out_pileup" / "gfa" / "graph_depth.pileup.tsv") == rows
    assert _records(d / "out_pileup" / "gfa" / "graph_depth.vcf") == records
