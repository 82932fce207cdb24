"""The depth profile on the device: ``k_node_cover`` and the fold through ``CoverCounter`` on the constructed blocks of
tests/depth_profile_cases.py at k = 21, 55 and 127, on a golden PE case, against the depth pass, and through the two commands
(``vstrains_amd.node_depth --profile``, ``cli --depth-from-reads --depth-profile``).  Every comparison is of exact integers
against tests/depth_profile_model.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_profile_cases as cases
import depth_profile_model as model
import node_depth_cases
from conftest import ROOT, pe_cases
from oracle import pe_oracle
from test_node_depth_gpu import CLI_PAIRS, SYNTH, _cli, _fastq, _files, _kc_of, _node_depth

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


def _rows(offsets, cov):
    return [cov[int(offsets[n]):int(offsets[n + 1])].tolist() for n in range(len(offsets) - 1)]


def device_cover(host, ctx, case, times: int = 1, fold_bound: int = 2 ** 32):
    """The profile of a constructed case through ``CoverCounter``, its block added ``times`` times -> (rows, KC, folds)."""
    ctx.build_index(case.seqs, case.k)
    counter = host.CoverCounter(ctx, fold_bound=fold_bound)
    block = _pack(host, ctx, case)
    try:
        for _ in range(times):
            counter.add(block)
        offsets, cov = counter.result()
        ctx.sync()
        assert offsets.dtype == np.int64 and cov.dtype == np.int64 and len(offsets) == len(case.seqs) + 1
        return _rows(offsets, cov), counter.kc().tolist(), counter.folds
    finally:
        block.free()
        ctx.keep_masks(False)


ALL = [c for k in cases.KS for c in cases.cover_cases(k) + [cases.scan_share_case(k, False), cases.scan_share_case(k, True)]]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model(host, ctx, case):
    want = model.node_cover(case.seqs, case.k, case.ends)
    rows, kc, folds = device_cover(host, ctx, case)
    assert rows == want
    assert kc == model.row_sums(want) and folds <= 1
    if case.want is not None:
        assert {n: rows[n] for n in case.want} == case.want


@pytest.mark.parametrize("k", cases.KS)
def test_the_same_block_added_twice_doubles_the_profile(host, ctx, k):
    case = [c for c in cases.cover_cases(k) if c.name == "two_ends_overlapping_on_one_segment"][0]
    want = model.node_cover(case.seqs, k, case.ends)
    rows, kc, _ = device_cover(host, ctx, case, times=2)
    assert max(want[0]) == 2 and rows == [[2 * v for v in row] for row in want]


@pytest.mark.parametrize("k", cases.KS)
def test_a_fold_after_every_block_and_one_fold_at_the_end_give_the_same(host, ctx, k):
    both = [c for c in cases.cover_cases(k) if c.name in ("every_segment_matched_flush_with_its_end",
                                                          "every_segment_matched_flush_with_its_end_by_reverse_complemented_ends")]
    assert len(both) == 2 and both[0].seqs == both[1].seqs and both[0].ends != both[1].ends
    seqs = both[0].seqs
    want = model.node_cover(seqs, k, both[0].ends + both[1].ends)
    got = []
    for bound, folds in ((1, 2), (2 ** 32, 1)):
        ctx.build_index(seqs, k)
        counter = host.CoverCounter(ctx, fold_bound=bound)
        blocks = [_pack(host, ctx, c) for c in both]
        try:
            for b in blocks:
                counter.add(b)
            got.append(_rows(*counter.result()))
            assert counter.folds == folds  # (bound 1: before the second block and before the result)
        finally:
            for b in blocks:
                b.free()
            ctx.keep_masks(False)
    assert got[0] == got[1] == want


def _both_counters(host, ctx, seqs, k, make_block):
    """KC of one block by the depth pass and by the profile's row sums."""
    ctx.build_index(seqs, k)
    depth, cover = host.DepthCounter(ctx), host.CoverCounter(ctx)
    block = make_block()  # (built after the counters: its masks are kept)
    try:
        depth.add(block)
        cover.add(block)
        ctx.sync()
        return depth.result(), cover.kc()
    finally:
        block.free()
        ctx.keep_masks(False)


def test_row_sums_equal_the_depth_pass_on_a_graph_above_its_node_limit(host, ctx):
    limit = host.depth_plan(10, 21, 100, 100)["node_limit"]
    case = node_depth_cases.many_nodes(21, limit + 1)
    kc_depth, kc_cover = _both_counters(host, ctx, case.seqs, 21, lambda: _pack(host, ctx, case))
    assert kc_depth.sum() > 0 and np.array_equal(kc_depth, kc_cover)


def test_row_sums_equal_the_depth_pass_on_4096_synthetic_pairs(host, ctx, tmp_path):
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[0]
    st, pre, names, seqs, cum, logger, _ = workload_for(0, str(tmp_path))
    sub, nth = int(0.005 * 2 ** 32), int(0.001 * 2 ** 32)
    kc_depth, kc_cover = _both_counters(host, ctx, seqs, cfg["k"], lambda: ctx.synth_pairs(st.genomes, cum, 20250000, 0, 4096, cfg["read_len"], sub, nth))
    assert kc_depth.sum() > 4096 * 100 and np.array_equal(kc_depth, kc_cover)


def test_70_000_copies_of_one_read_put_70_000_on_its_windows(host, ctx):
    small = [c for c in cases.cover_cases(21) if c.name == "match_holding_several_grid_points"][0]
    one = model.node_cover(small.seqs, 21, small.ends)
    assert set(one[0]) == {0, 1} and not any(one[1])
    rows, kc, _ = device_cover(host, ctx, cases.CoverCase("copies", 21, small.seqs, small.ends * 70000))  # (every copy hits the same two slots)
    assert rows == [[70000 * v for v in row] for row in one]


def test_a_golden_pe_case_equals_the_model(host, ctx):
    name, d, meta = pe_cases()[0]
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fwd, rve = pe_oracle.fastq_sequences(os.path.join(d, "fwd.fq")), pe_oracle.fastq_sequences(os.path.join(d, "rve.fq"))
    n = min(len(fwd), len(rve))
    ends = [e for pair in zip(fwd[:n], rve[:n]) for e in pair]
    rows, kc, _ = device_cover(host, ctx, cases.CoverCase(name, meta["k"], seqs, ends))
    want = model.node_cover(seqs, meta["k"], ends)
    assert sum(kc) > 0 and rows == want


# ---- the commands -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    from vstrains_amd import node_depth, synth

    c = synth.make_pipeline_case(n_pairs=CLI_PAIRS, **SYNTH)
    d = tmp_path_factory.mktemp("depth_profile_synth")
    raw = c.gfa_text.encode()
    (d / "graph.gfa").write_bytes(raw)
    (d / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(raw))
    (d / "contigs.paths").write_text(c.paths_text)
    (d / "fwd.fq").write_bytes(_fastq(c.fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(c.rve, "2"))
    ends = [e for pair in zip(c.fwd, c.rve) for e in pair]
    return d, c, model.node_cover(list(c.graph.seqs), 55, ends)


def test_node_depth_command_writes_the_models_profile(synth_files):
    from vstrains_amd import node_depth

    d, c, want = synth_files
    plain = _node_depth(d / "graph.gfa", d / "plain.gfa", d / "fwd.fq", d / "rve.fq")
    got = _node_depth(d / "graph.gfa", d / "out.gfa", d / "fwd.fq", d / "rve.fq",
                      ["--profile", str(d / "p.bedgraph.gz"), "--profile-summary", str(d / "p.tsv")])
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert got.returncode == 0, got.stderr[-3000:]
    ids, seqs = pe_oracle.read_gfa_segments(str(d / "graph.gfa"))
    offsets, cov = node_depth.read_bedgraph(str(d / "p.bedgraph.gz"), ids)
    assert _rows(offsets, cov) == want
    lines = [line.split("\t") for line in (d / "p.tsv").read_text().splitlines()]
    assert lines[0] == list(node_depth.SUMMARY_COLUMNS) and [l[0] for l in lines[1:]] == ids
    assert [int(l[3]) for l in lines[1:]] == _kc_of(d / "out.gfa") == model.row_sums(want)
    assert (d / "out.gfa").read_bytes() == (d / "plain.gfa").read_bytes()
    assert got.stdout.rstrip().endswith("; profile in: %s; summary in: %s" % (d / "p.bedgraph.gz", d / "p.tsv"))
    assert plain.stdout.rstrip().endswith("; result stored in: %s" % (d / "plain.gfa")) and got.stdout.split("; result stored in:")[0] == plain.stdout.split("; result stored in:")[0]


def test_cli_with_depth_profile_writes_the_two_files_and_the_same_strains(synth_files):
    from vstrains_amd import node_depth

    d, c, want = synth_files
    plain = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_plain", ["--depth-from-reads"])
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_profile", ["--depth-from-reads", "--depth-profile"])
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert got.returncode == 0, got.stderr[-3000:]
    assert _files(d / "out_profile") == sorted(_files(d / "out_plain") + ["gfa/graph_depth.bedgraph", "gfa/graph_depth.tsv"])
    for rel in ("strain.fasta", "strain.paths", "gfa/graph_depth.gfa"):
        assert (d / "out_profile" / rel).read_bytes() == (d / "out_plain" / rel).read_bytes(), rel
    ids, seqs = pe_oracle.read_gfa_segments(str(d / "stripped.gfa"))
    offsets, cov = node_depth.read_bedgraph(str(d / "out_profile" / "gfa" / "graph_depth.bedgraph"), ids)
    assert _rows(offsets, cov) == want
    assert len((d / "out_profile" / "gfa" / "graph_depth.tsv").read_text().splitlines()) == len(ids) + 1
