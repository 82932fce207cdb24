"""The depth pass on the device: ``k_node_depth`` through ``Context.node_depth`` / ``DepthCounter`` on the constructed blocks
of tests/node_depth_cases.py at k = 21, 55 and 127, on the golden PE cases, and through the two commands
(``vstrains_amd.node_depth``, ``cli --depth-from-reads``).  Every comparison is of exact integers against
tests/node_depth_model.py."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_util as bu
import bgzf_util as bz
import node_depth_cases as cases
import node_depth_model as model
from conftest import ROOT, pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu

SYNTH = dict(n_strains=4, genome_len=3000, snp_rate=0.02, k=55, read_len=150, seed=5)
CLI_PAIRS = 1000  # the fewest of 400, 1000, 2000, 4000 pairs at which no segment of the synth case is empty (400: three are)


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


def device_depth(host, ctx, case, times: int = 1):
    """KC of a constructed case through ``DepthCounter``, its block added ``times`` times."""
    ctx.build_index(case.seqs, case.k)
    counter = host.DepthCounter(ctx)
    block = ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))
    try:
        for _ in range(times):
            counter.add(block)
        ctx.sync()
        return counter.result().tolist()
    finally:
        block.free()
        ctx.keep_masks(False)


@pytest.mark.parametrize("case", [c for k in cases.KS for c in cases.small_cases(k)], ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model(host, ctx, case):
    want = model.node_depth(case.seqs, case.k, case.ends)
    assert device_depth(host, ctx, case) == want
    if case.want is not None:
        assert {n: v for n, v in enumerate(want) if v} == {n: v for n, v in case.want.items() if v}


@pytest.mark.parametrize("k", cases.KS)
def test_the_same_block_added_twice_doubles_the_totals(host, ctx, k):
    case = cases.small_cases(k)[2]
    want = model.node_depth(case.seqs, k, case.ends)
    assert sum(want) > 0 and device_depth(host, ctx, case, times=2) == [2 * v for v in want]


@pytest.mark.parametrize("k", cases.KS)
def test_end_count_one_more_than_a_multiple_of_the_workgroups_share(host, ctx, k):
    share = 1024  # a batch of 64 ends for each of a workgroup's sixteen wavefronts: the smallest share the plan makes
    case = cases.share_plus_one(k, share)
    plan = host.depth_plan(len(case.seqs), k, 2 * len(case.ends), max(len(e) for e in case.ends))  # (a singles block: two ends per read)
    assert plan["ends_per_wg"] == share and plan["grid"] == 3 and 2 * len(case.ends) == 2 * share + 2
    assert device_depth(host, ctx, case) == model.node_depth(case.seqs, k, case.ends)


@pytest.fixture(scope="module")
def big_graph(host):
    limit = host.depth_plan(10, 21, 100, 100)["node_limit"]
    case = cases.many_nodes(21, limit + 1)
    return case, pe_oracle.build_table(case.seqs, 22)


def test_graph_just_above_the_node_limit_takes_the_global_route(host, ctx, big_graph):
    case, table = big_graph
    plan = host.depth_plan(len(case.seqs), 21, len(case.ends), max(len(e) for e in case.ends))
    assert plan["route"] == "global" and plan["lds_nodes"] == 0
    want = model.node_depth(case.seqs, 21, case.ends, table=table)
    assert want[7] == 70 * 3 + sum(3 for i in range(200) if i * 97 % len(case.seqs) == 7)
    assert device_depth(host, ctx, case) == want


@pytest.mark.parametrize("route", ["lds", "global"])
def test_70_000_copies_of_one_read_credit_one_node(host, ctx, big_graph, route):
    if route == "global":
        big, table = big_graph
        seqs, read = big.seqs, big.seqs[11][1:]
        one = model.node_depth(seqs, 21, [read], table=table)
    else:
        small = cases.small_cases(21)[1]
        seqs, read = small.seqs, small.ends[0]
        one = model.node_depth(seqs, 21, [read])
    case = cases.DepthCase("copies", 21, seqs, [read] * 70000)
    assert host.depth_plan(len(seqs), 21, 70000, len(read))["route"] == route
    assert sum(one) > 0 and sum(1 for v in one if v) == 1
    assert device_depth(host, ctx, case) == [70000 * v for v in one]


def _fastq_seqs(path):
    return pe_oracle.fastq_sequences(path)


@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_golden_pe_cases_equal_the_model(host, ctx, name, d, meta):
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fwd, rve = _fastq_seqs(os.path.join(d, "fwd.fq")), _fastq_seqs(os.path.join(d, "rve.fq"))
    n = min(len(fwd), len(rve))
    ends = [e for pair in zip(fwd[:n], rve[:n]) for e in pair]
    case = cases.DepthCase(name, meta["k"], seqs, ends)
    assert device_depth(host, ctx, case) == model.node_depth(seqs, meta["k"], ends)


# ---- the commands -----------------------------------------------------------------------------------------------------
def _fastq(seqs, tag):
    return "".join("@r%d/%s\n%s\n+\n%s\n" % (i, tag, s, "I" * len(s)) for i, s in enumerate(seqs)).encode()


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    from vstrains_amd import synth

    c = synth.make_pipeline_case(n_pairs=400, **SYNTH)
    d = tmp_path_factory.mktemp("node_depth_synth")
    (d / "graph.gfa").write_text(c.gfa_text)
    (d / "fwd.fq").write_bytes(_fastq(c.fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(c.rve, "2"))
    ends = [e for pair in zip(c.fwd, c.rve) for e in pair]
    return d, c, model.node_depth(list(c.graph.seqs), 55, ends)


def _node_depth(gfa, out, fwd, rve, flags=()):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.node_depth", "-g", str(gfa), "-o", str(out), "-f", str(fwd), "-r", str(rve)] + list(flags),
                          cwd=ROOT, capture_output=True, text=True, timeout=600)


def _kc_of(path):
    out = []
    for line in open(path, "rb").read().splitlines():
        cols = line.split(b"\t")
        if cols[0] == b"S":
            tags = dict((t[:2], t) for t in cols[3:])
            assert tags[b"LN"] == b"LN:i:%d" % len(cols[2]) and b"DP" not in tags
            out.append(int(tags[b"KC"].split(b":")[2]))
    return out


def test_node_depth_command_writes_the_models_counts(synth_files):
    d, c, want = synth_files
    got = _node_depth(d / "graph.gfa", d / "out.gfa", d / "fwd.fq", d / "rve.fq")
    assert got.returncode == 0, got.stderr[-3000:]
    assert _kc_of(d / "out.gfa") == want and sum(want) == 76000
    assert "800 read ends counted" in got.stdout and "76000 window-entry" in got.stdout and "3 of %d segments with KC = 0" % len(want) in got.stdout
    # the rewritten graph parses as the pipeline parses a SPAdes GFA, and k was taken from the L lines
    from vstrains_amd import node_depth

    raw = (d / "out.gfa").read_bytes()
    assert node_depth.infer_k(raw) == 55 and "k = 55" in got.stdout
    assert node_depth.rewrite_gfa((d / "graph.gfa").read_bytes(), want) == raw


WAYS = ("plain", "gz", "bgzf", "interleaved", "bam", "single")


@pytest.mark.parametrize("way", WAYS)
def test_the_same_reads_given_six_ways_write_the_same_file(synth_files, tmp_path, way):
    """every way writes, byte for byte, the graph rewritten with the model's counts -- so the six files are identical"""
    from vstrains_amd import node_depth

    d, c, want = synth_files
    tf, tr = (d / "fwd.fq").read_bytes(), (d / "rve.fq").read_bytes()
    f, r, flags = d / "fwd.fq", d / "rve.fq", []
    if way == "gz":
        f, r = tmp_path / "f.fq.gz", tmp_path / "r.fq.gz"
        f.write_bytes(gzip.compress(tf))
        r.write_bytes(gzip.compress(tr))
    elif way == "bgzf":
        f, r = tmp_path / "f.bgzf.gz", tmp_path / "r.bgzf.gz"
        f.write_bytes(bz.bgzf(tf))
        r.write_bytes(bz.bgzf(tr))
    elif way == "interleaved":
        f = r = tmp_path / "il.fq"
        f.write_bytes(b"".join(b"@r" + a + b"@r" + b for a, b in zip(tf.split(b"@r")[1:], tr.split(b"@r")[1:])))
        flags = ["--interleaved"]
    elif way == "bam":
        records = []
        for i, (a, b) in enumerate(zip(c.fwd, c.rve)):
            records += [bu.rec("r%d" % i, bu.PAIRED | bu.FIRST, a), bu.rec("r%d" % i, bu.PAIRED | bu.SECOND, b)]
        f = r = tmp_path / "reads.bam"
        f.write_bytes(bu.write(records))
    elif way == "single":
        cut = 300  # the first pairs as two files, the ends of the others as unpaired reads
        f, r = tmp_path / "pf.fq", tmp_path / "pr.fq"
        f.write_bytes(_fastq(c.fwd[:cut], "1"))
        r.write_bytes(_fastq(c.rve[:cut], "2"))
        (tmp_path / "s.fq").write_bytes(_fastq(c.fwd[cut:] + c.rve[cut:], "s"))
        flags = ["--single", str(tmp_path / "s.fq")]
    out = tmp_path / "out.gfa"
    got = _node_depth(d / "graph.gfa", out, f, r, flags)
    assert got.returncode == 0, got.stderr[-3000:]
    assert out.read_bytes() == node_depth.rewrite_gfa((d / "graph.gfa").read_bytes(), want)


def _cli(gfa, paths, fwd, rve, out, flags=()):
    return subprocess.run([sys.executable, "-m", "vstrains_amd.cli", "-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fwd),
                           "-rve", str(rve)] + list(flags), cwd=ROOT, capture_output=True, text=True, timeout=600)


def _files(root):
    return sorted(os.path.relpath(os.path.join(base, f), root) for base, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from vstrains_amd import node_depth, synth

    c = synth.make_pipeline_case(n_pairs=CLI_PAIRS, **SYNTH)
    d = tmp_path_factory.mktemp("node_depth_cli")
    ends = [e for pair in zip(c.fwd, c.rve) for e in pair]
    want = model.node_depth(list(c.graph.seqs), 55, ends)
    assert min(want) > 0
    raw = c.gfa_text.encode()
    (d / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(raw))
    (d / "tagged.gfa").write_bytes(node_depth.rewrite_gfa(raw, want))
    (d / "contigs.paths").write_text(c.paths_text)
    (d / "fwd.fq").write_bytes(_fastq(c.fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(c.rve, "2"))
    return d, c, want


def test_cli_with_depth_from_reads_equals_cli_on_the_models_tags(cli_files):
    d, c, want = cli_files
    assert b"DP:" not in (d / "stripped.gfa").read_bytes()
    plain = _cli(d / "tagged.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_tagged")
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_depth", ["--depth-from-reads"])
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert got.returncode == 0, got.stderr[-3000:]
    files = _files(d / "out_tagged")
    assert {"strain.fasta", "strain.paths", "aln/pe_info", "gfa/graph_L0.gfa"} <= set(files)
    assert _files(d / "out_depth") == sorted(files + ["gfa/graph_depth.gfa"])
    assert (d / "out_depth" / "gfa" / "graph_depth.gfa").read_bytes() == (d / "tagged.gfa").read_bytes()
    for rel in files:
        if rel != "vstrains.log":  # (time stamps and paths)
            assert (d / "out_depth" / rel).read_bytes() == (d / "out_tagged" / rel).read_bytes(), rel
    log = (d / "out_depth" / "vstrains.log").read_text()
    assert log.count("segment depth counted from the reads") == 1
    assert "segment depth counted" not in (d / "out_tagged" / "vstrains.log").read_text()


def test_cli_without_the_flag_refuses_a_gfa_without_depth_tags_as_before(cli_files):
    d, c, want = cli_files
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_refused")
    assert got.returncode == 1 and "Illegal graph format" in got.stdout + got.stderr
    assert not (d / "out_refused" / "gfa" / "graph_depth.gfa").exists()


def test_cli_stops_on_a_segment_the_reads_never_touch(cli_files):
    d, c, want = cli_files
    lonely = "S\tnever_read\t%s\n" % cases.dna(np.random.default_rng(99), 120)
    (d / "lonely.gfa").write_bytes((d / "stripped.gfa").read_bytes() + lonely.encode())
    got = _cli(d / "lonely.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_lonely", ["--depth-from-reads"])
    assert got.returncode == 1
    assert "never_read" in got.stdout + got.stderr and "KC = 0" in got.stdout + got.stderr
    assert not (d / "out_lonely" / "strain.fasta").exists()
