"""The site-pair pass on the device: ``k_node_site_pairs`` through ``SitePairCounter`` on the constructed blocks of
tests/site_pairs_cases.py at k = 21, 55 and 127, on a block whose pileup share per workgroup would be odd, against the pileup's
depth, on a golden PE case through the commands (``vstrains_amd.node_depth --site-pairs``, with ``--sites`` and by the two-pass
route) and through ``cli --depth-from-reads --depth-pileup --depth-site-pairs``.  Every comparison is of exact integers against
tests/site_pairs_model.py."""
import os

import numpy as np
import pytest

import pileup_model
import site_pairs_cases as cases
import site_pairs_model as model
from conftest import pe_cases
from oracle import pe_oracle
from pileup_cases import _OTHER, sub
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


def device_site_pairs(host, ctx, case, times: int = 1, block=None):
    """A constructed case through ``SitePairCounter``, its block added ``times`` times -> (result rows, tallies)."""
    ctx.build_index(case.seqs, case.k)
    counter = host.SitePairCounter(ctx, case.sites, max_mismatch=case.M, max_span=case.span)
    own = block is None
    if own:
        block = ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))
    try:
        for _ in range(times):
            counter.add(block)
        seg, pos_a, pos_b, counts = counter.result()
        ctx.sync()
        assert seg.dtype == pos_a.dtype == pos_b.dtype == counts.dtype == np.int64 and counts.shape == (len(seg), 5, 5)
        return [(int(n), int(a), int(b), c.tolist()) for n, a, b, c in zip(seg, pos_a, pos_b, counts)], counter.tallies()
    finally:
        if own:
            block.free()
        ctx.keep_masks(False)


def judge(c):
    pairs, tally = model.site_pairs(c.seqs, c.k, c.ends, c.sites, c.M, c.span, c.singles)
    return model.result_rows(pairs), tally


ALL = [c for k in cases.KS for c in cases.site_pair_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model(host, ctx, case):
    want_rows, want_tally = judge(case)
    rows, tally = device_site_pairs(host, ctx, case)
    assert rows == want_rows
    assert tally == want_tally == case.tally


def test_the_index_of_the_reordered_graph_is_reordered(host, ctx):
    case = [c for c in cases.site_pair_cases(21) if c.name == "graph_whose_node_rank_is_not_the_identity"][0]
    ctx.build_index(case.seqs, case.k)
    assert ctx.node_rank is not None and ctx.node_rank.tolist() != list(range(len(case.seqs)))


@pytest.mark.parametrize("k", cases.KS)
def test_the_same_block_added_twice_doubles_every_count(host, ctx, k):
    for name in ("exactly_32_and_33_raw_observations", "mates_overlapping_on_a_site_and_disagreeing"):
        case = [c for c in cases.site_pair_cases(k) if c.name == name][0]
        want_rows, want_tally = judge(case)
        rows, tally = device_site_pairs(host, ctx, case, times=2)
        assert rows == [(n, a, b, [[2 * v for v in r] for r in cell]) for n, a, b, cell in want_rows] and len(rows) > 0
        assert tally == tuple(2 * v for v in want_tally)


def test_refusals_of_the_counter_name_segment_and_position(host, ctx):
    case = cases.site_pair_cases(21)[0]
    seqs = case.seqs + ["ACGT"]
    ctx.build_index(seqs, 21)
    for sites, said in (([(0, len(seqs[0]))], "position %d is outside segment 0" % len(seqs[0])), ([(2, 1)], "segment 2 is shorter than k \\+ 1 = 22"),
                        ([(3, 0)], "no segment 3"), ([(0, -1)], "position -1 is outside segment 0")):
        with pytest.raises(ValueError, match=said):
            host.SitePairCounter(ctx, sites)


def test_a_pair_is_not_cut_where_the_pileups_share_would_be_odd(host, ctx):
    """The smallest block above 2 * n_cu * 1024 ends for which ``pileup_plan``'s ends per workgroup is odd: a workgroup boundary
    there falls between the two mates of a pair; ``site_pairs_plan`` rounds to a multiple of 64.  Three distinct pairs, each
    with one site under either mate and none shared, cycled: a cut pair links nothing and a shifted one the wrong sites."""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    k, K = 21, 22
    R = K + 3
    rng = np.random.default_rng(42)
    node = cases.dna(rng, 6 * R)
    n_ends = next(n for n in range(2 * n_cu * 1024 + 2, 2 * n_cu * 1024 + 2 + 8 * n_cu, 2) if host.pileup_plan(2, k, n, R, n_cu)["ends_per_wg"] % 2)
    plan = host.site_pairs_plan(2, k, n_ends, R, n_cu)
    assert plan["ends_per_wg"] % 64 == 0 and plan["grid"] > 1 and plan["grid"] * plan["ends_per_wg"] >= n_ends
    three = [[sub(node[i * R:(i + 1) * R], 1), pileup_model.revcomp(sub(node[(i + 3) * R:(i + 4) * R], 2))] for i in range(3)]
    sites = [(0, i * R + 1) for i in range(3)] + [(0, (i + 3) * R + 2) for i in range(3)]
    n_pairs = n_ends // 2
    times = [n_pairs // 3 + (i < n_pairs % 3) for i in range(3)]
    want, tally = {}, [0] * 5
    for i, (pair, t) in enumerate(zip(three, times)):
        pairs, one = model.site_pairs([node], k, pair, sites, 8, len(node))
        assert one == (1, 0, 0, 1, 0) and list(pairs) == [((0, i * R + 1), (0, (i + 3) * R + 2))]
        want.update((key, [[t * v for v in r] for r in cell]) for key, cell in pairs.items())
        tally = [a + t * b for a, b in zip(tally, one)]
    data, off = host.encode_seqs([e for pair in three for e in pair])
    assert np.diff(off).tolist() == [R] * 6
    big = np.tile(data, n_ends // 6 + 1)[: n_ends * R]  # the six ends, cycled
    big_off = np.arange(n_ends + 1, dtype=np.uint64) * np.uint64(R)
    case = cases.SitePairCase("odd_share", k, [node, cases.dna(rng, K)], [], sites, "a pair cut at an odd workgroup share", span=len(node))
    ctx.keep_masks(True)
    block = ctx.pack(np.ascontiguousarray(big), big_off)
    try:
        rows, got = device_site_pairs(host, ctx, case, block=block)
    finally:
        block.free()
    assert rows == model.result_rows(want) and got == tuple(tally) and got[3] == n_pairs


def _golden(name):
    name, d, meta = [c for c in pe_cases() if c[0] == name][0]
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fwd, rve = pe_oracle.fastq_sequences(os.path.join(d, "fwd.fq")), pe_oracle.fastq_sequences(os.path.join(d, "rve.fq"))
    n = min(len(fwd), len(rve))
    return d, meta["k"], ids, seqs, [e for pair in zip(fwd[:n], rve[:n]) for e in pair]


@pytest.fixture(scope="module")
def golden():
    """The golden case with sequencing errors (300 pairs): the model's pileup, its records and their sites, once."""
    d, k, ids, seqs, ends = _golden("errors_k21")
    depth, alt, _ = pileup_model.pileup(seqs, k, ends, 8)
    records = pileup_model.variant_records(pileup_model.table_rows(ids, seqs, depth, alt))
    sites = sorted(set((ids.index(r[0]), r[1] - 1) for r in records))
    assert len(sites) > 100
    return d, k, ids, seqs, ends, depth, sites


def test_a_stored_pair_holds_no_more_fragments_than_either_site_has_depth(host, ctx, golden):
    """On the same block and budget, the span larger than every segment and no fragment in overflow: the 25 counts of a stored
    pair sum to at most the smaller of the two sites' pileup depths (a fragment that observes a site has a credited alignment
    over it)."""
    d, k, ids, seqs, ends, depth, sites = golden
    few = sites[::6]
    case = cases.SitePairCase("golden", k, seqs, ends, few, "against the pileup", span=max(len(s) for s in seqs))
    want_rows, want_tally = judge(case)
    assert want_tally[1] == 0 and want_tally[3] > 50 and want_tally[4] > 0
    ctx.build_index(seqs, k)
    piles = host.PileupCounter(ctx, max_mismatch=8)
    block = ctx.pack(*host.encode_seqs(ends))
    try:
        piles.add(block)
        offsets, dev_depth, _ = piles.result()
        rows, tally = device_site_pairs(host, ctx, case, block=block)
    finally:
        block.free()
        ctx.keep_masks(False)
    assert rows == want_rows and tally == want_tally
    assert dev_depth.tolist() == [v for row in depth for v in row]
    for n, a, b, cell in rows:
        assert 0 < sum(sum(r) for r in cell) <= min(int(dev_depth[offsets[n] + a]), int(dev_depth[offsets[n] + b]))


# ---- the commands -----------------------------------------------------------------------------------------------------
def _table(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["segment", "pos_a", "pos_b", "base_a", "base_b", "count"]
    return [tuple(v if i in (0, 3, 4) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]


def test_node_depth_with_sites_and_by_two_passes_writes_the_models_table(golden, tmp_path):
    d, k, ids, seqs, ends, depth, sites = golden
    pairs, tally = model.site_pairs(seqs, k, ends, sites, 8, 1000)
    want = model.table_rows(ids, pairs)
    assert len(want) > 1000 and tally[1] > 0 and tally[4] > 0
    gfa, fwd, rve = os.path.join(d, "graph.gfa"), os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq")
    got = _node_depth(gfa, tmp_path / "o1.gfa", fwd, rve, ["-k", str(k), "--variants", str(tmp_path / "v.vcf")])
    assert got.returncode == 0, got.stderr[-3000:]
    assert "site pairs" not in got.stdout
    got = _node_depth(gfa, tmp_path / "o2.gfa", fwd, rve, ["-k", str(k), "--sites", str(tmp_path / "v.vcf"), "--site-pairs", str(tmp_path / "a.tsv")])
    assert got.returncode == 0, got.stderr[-3000:]
    said = "%d fragments observing, %d overflow fragments, %d discordant sites, %d pairs stored, %d pairs unstored" % tally
    assert got.stdout.rstrip().endswith("; site pairs in: %s (%s)" % (tmp_path / "a.tsv", said))
    assert _table(tmp_path / "a.tsv") == want
    got = _node_depth(gfa, tmp_path / "o3.gfa", fwd, rve, ["-k", str(k), "--variants", str(tmp_path / "w.vcf"), "--site-pairs", str(tmp_path / "b.tsv")])
    assert got.returncode == 0, got.stderr[-3000:]
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes() and (tmp_path / "v.vcf").read_bytes() == (tmp_path / "w.vcf").read_bytes()
    assert (tmp_path / "o1.gfa").read_bytes() == (tmp_path / "o2.gfa").read_bytes() == (tmp_path / "o3.gfa").read_bytes()


def two_planted(seqs, fwd, rve):
    """The synthetic reads (exact copies of their strains) with two things to link: in every second read that holds the 61
    bases around the middle of the longest segment, on either strand, the bases 12 and 48 of that stretch are both changed --
    two minor variants that travel together."""
    seg = max(seqs, key=len)
    p = len(seg) // 2
    motif = seg[p - 30:p + 31]
    changed = motif[:12] + _OTHER[motif[12]] + motif[13:48] + _OTHER[motif[48]] + motif[49:]
    seen = 0
    out = []
    for reads in (fwd, rve):
        done = []
        for r in reads:
            for m, c in ((motif, changed), (pileup_model.revcomp(motif), pileup_model.revcomp(changed))):
                at = r.find(m)
                if at >= 0:
                    seen += 1
                    if seen % 2:
                        r = r[:at] + c + r[at + len(c):]
            done.append(r)
        out.append(done)
    assert seen >= 8
    return out[0], out[1]


def test_cli_with_depth_site_pairs_writes_the_models_table(tmp_path):
    from vstrains_amd import node_depth, synth

    c = synth.make_pipeline_case(n_pairs=CLI_PAIRS, **SYNTH)
    d = tmp_path
    (d / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(c.gfa_text.encode()))
    (d / "contigs.paths").write_text(c.paths_text)
    ids, seqs = pe_oracle.read_gfa_segments(str(d / "stripped.gfa"))
    fwd, rve = two_planted(seqs, c.fwd, c.rve)
    (d / "fwd.fq").write_bytes(_fastq(fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(rve, "2"))
    ends = [e for pair in zip(fwd, rve) for e in pair]
    depth, alt, _ = pileup_model.pileup(seqs, 55, ends, 8)
    records = pileup_model.variant_records(pileup_model.table_rows(ids, seqs, depth, alt))
    sites = sorted(set((ids.index(r[0]), r[1] - 1) for r in records))
    pairs, tally = model.site_pairs(seqs, 55, ends, sites, 8, 1000)
    want = model.table_rows(ids, pairs)
    assert len(sites) >= 2 and len(want) >= 2  # (the two planted bases, together and apart)
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out", ["--depth-from-reads", "--depth-pileup", "--depth-site-pairs"])
    assert got.returncode == 0, got.stderr[-3000:]
    assert "gfa/graph_depth.site_pairs.tsv" in _files(d / "out")
    assert _table(d / "out" / "gfa" / "graph_depth.site_pairs.tsv") == want
    same = _node_depth(d / "stripped.gfa", d / "o.gfa", d / "fwd.fq", d / "rve.fq", ["--variants", str(d / "v.vcf"), "--site-pairs", str(d / "b.tsv")])
    assert same.returncode == 0, same.stderr[-3000:]
    assert (d / "b.tsv").read_bytes() == (d / "out" / "gfa" / "graph_depth.site_pairs.tsv").read_bytes()
    assert (d / "v.vcf").read_bytes() == (d / "out" / "gfa" / "graph_depth.vcf").read_bytes()
