"""``vstrains_amd.contig_paths`` and ``cli --contigs-fasta`` on the device.  The contigs of every golden graph case, spelled
from ``in/contigs.paths`` (the first segment of a part whole, then ``seg[k:]``, parts joined by ten ``N``) and written as a
FASTA, must come back as that file byte for byte; and the command given the FASTA must write every file the command given
the .paths file writes, byte for byte."""
import os

import pytest

import contig_thread_model as model
from graph_case import GOLDEN, Case, case_names, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from vstrains_amd.graph.hip_ops import HipBackend

    return HipBackend(0)


def write_fasta(name, path, width=60):
    """The contigs of a golden case as a FASTA of ``width``-column lines -> (k, its contigs.paths text)."""
    from vstrains_amd import node_depth
    from vstrains_amd import pe as host

    d = os.path.join(GOLDEN, name, "in")
    with open(os.path.join(d, "graph.gfa"), "rb") as fh:
        k = node_depth.infer_k(fh.read())
    ids, seqs = host.read_gfa_segments(os.path.join(d, "graph.gfa"))
    with open(os.path.join(d, "contigs.paths")) as fh:
        paths = fh.read()
    seg_of = dict(zip(ids, seqs))
    with open(path, "w") as fh:
        for cname, parts in model.read_paths(paths):
            if not cname.endswith("'"):
                text = model.spell(parts, seg_of, k)
                fh.write(">%s\n%s\n" % (cname, "\n".join(text[i:i + width] for i in range(0, len(text), width))))
    return k, paths


@pytest.mark.parametrize("name", case_names())
def test_threaded_paths_of_the_golden_cases_are_the_assemblers_byte_for_byte(backend, name, tmp_path):
    from vstrains_amd import contig_paths

    fasta = str(tmp_path / "contigs.fasta")
    k, paths = write_fasta(name, fasta)
    text, tally = contig_paths.thread_contigs(backend.ctx, os.path.join(GOLDEN, name, "in", "graph.gfa"), fasta)
    assert text == paths
    n = sum(1 for line in paths.split("\n") if line.startswith("NODE_") and not line.endswith("'"))
    gapped = paths.count(";\n") // 2
    assert tally == dict(threaded=n, gapped=tally["gapped"], left_out=0, ambiguous_windows=0, k=k) and (gapped == 0) == (tally["gapped"] == 0)


def test_the_command_names_unnamed_contigs_and_counts_what_it_leaves_out(tmp_path):
    import subprocess
    import sys

    from conftest import ROOT

    name = "gapped_paths_kc_tags_k21"
    fasta = tmp_path / "contigs.fasta"
    k, paths = write_fasta(name, str(fasta))
    first = model.read_paths(paths)[0]
    lines = fasta.read_text().split("\n")
    assert lines[0] == ">" + first[0]
    # the first contig loses its SPAdes name; one contig without a hit and one of k bases are added
    fasta.write_text("\n".join([">polished first"] + lines[1:]) + ">nothing\n" + "ACGT" * 30 + "\n>short\n" + lines[1][:k] + "\n")
    out = tmp_path / "threaded.paths"
    gfa = os.path.join(GOLDEN, name, "in", "graph.gfa")
    got = subprocess.run([sys.executable, "-m", "vstrains_amd.contig_paths", "-g", gfa, "-c", str(fasta), "-o", str(out)], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert got.returncode == 0, got.stderr[-3000:]
    n = len(model.read_paths(paths)) // 2
    assert "k = 21, %d contigs threaded, 4 of them gapped, 2 left out" % n in got.stdout and "0 ambiguous windows" in got.stdout
    text = out.read_text()
    renamed = text.split("\n")[0]
    # segment 1 alone (LN 22, KC 21754): the window-weighted mean of one segment is its depth
    assert first[1] == [["1+"]] and renamed == "NODE_1_length_22_cov_" + repr(21754 / 22)
    assert text.replace(renamed, first[0]) == paths


def test_cli_threads_after_depth_from_reads_on_that_graph(backend, tmp_path):
    """A GFA without depth tags and contigs without SPAdes names: the depth pass runs first, and the names take their
    coverage from the graph it wrote."""
    from vstrains_amd import cli, contig_paths, node_depth, synth

    c = synth.make_pipeline_case(n_pairs=1000, n_strains=4, genome_len=3000, snp_rate=0.02, k=55, read_len=150, seed=5)
    ids, seqs = list(c.graph.ids), list(c.graph.seqs)
    entries = [(n, p) for n, p in model.read_paths(c.paths_text) if not n.endswith("'")]
    contigs = [model.spell(p, dict(zip(ids, seqs)), 55) for _, p in entries]
    (tmp_path / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(c.gfa_text.encode()))
    (tmp_path / "contigs.fasta").write_text("".join(">polished_%d some tool\n%s\n" % (i, t) for i, t in enumerate(contigs)))
    (tmp_path / "fwd.fq").write_text(synth.fastq_text(c.fwd, "f"))
    (tmp_path / "rve.fq").write_text(synth.fastq_text(c.rve, "r"))
    out = tmp_path / "out"
    cli.main(["-a", "spades", "-g", str(tmp_path / "stripped.gfa"), "-o", str(out), "-fwd", str(tmp_path / "fwd.fq"), "-rve", str(tmp_path / "rve.fq"),
              "--depth-from-reads", "--contigs-fasta", str(tmp_path / "contigs.fasta")], backend=backend)
    depths = contig_paths.segment_depths((out / "gfa" / "graph_depth.gfa").read_bytes())
    assert None not in depths
    table = model.window_table(seqs, 55)
    want = ""
    for i, ((_, walk), text) in enumerate(zip(entries, contigs)):
        parts, _ = model.thread(seqs, 55, text, table=table)
        assert model.tokens(parts, ids) == walk
        acc, total = 0.0, 0
        for part in parts:
            for n, _, w in part:
                acc += depths[n] * w
                total += w
        want += model.entry("NODE_%d_length_%d_cov_%s" % (i + 1, len(text), repr(acc / total)), parts, ids)
    assert (out / "tmp" / "contigs_threaded.paths").read_text() == want
    assert (out / "strain.fasta").exists() and (out / "strain.paths").exists()


@pytest.mark.parametrize("name", ["gapped_paths_kc_tags_k21", "self_loops_k21", "hiv_like_k55"])
def test_cli_given_the_fasta_writes_what_cli_given_the_paths_writes(backend, name, tmp_path):
    from vstrains_amd import cli

    case = Case(name)
    inp = case.inputs(str(tmp_path), with_reads=True)
    fasta = str(tmp_path / "contigs.fasta")
    write_fasta(name, fasta)
    outs = {}
    for way, flags in (("paths", ["-p", inp["paths"]]), ("fasta", ["--contigs-fasta", fasta])):
        outs[way] = str(tmp_path / ("out_" + way))
        argv = ["-a", "spades", "-g", inp["gfa"], "-o", outs[way], "-fwd", inp["fwd"], "-rve", inp["rve"]] + flags + case.meta["cli_extra"]
        if case.meta["returncode"] != 0:
            with pytest.raises(case.expected_exception()):  # (the reference stops on this case, and so do both runs)
                cli.main(argv, backend=backend)
        else:
            cli.main(argv, backend=backend)

    def files(root):
        return sorted(os.path.relpath(os.path.join(base, f), root) for base, _, fs in os.walk(root) for f in fs)

    want = files(outs["paths"])
    assert files(outs["fasta"]) == sorted(want + ["tmp/contigs_threaded.paths"])
    for rel in want:
        if rel != "vstrains.log":  # (time stamps and paths)
            with open(os.path.join(outs["paths"], rel), "rb") as a, open(os.path.join(outs["fasta"], rel), "rb") as b:
                assert a.read() == b.read(), rel
    with open(os.path.join(outs["fasta"], "tmp", "contigs_threaded.paths")) as fh, open(inp["paths"]) as want_fh:
        assert fh.read() == want_fh.read()
    with open(os.path.join(outs["fasta"], "vstrains.log")) as fh:
        assert fh.read().count("contigs threaded through the graph: k = %d" % case.meta["k"]) == 1
    # ... and what the reference wrote for this case (its INFO lines aside: this log holds one more, the tallies)
    problems, _ = compare(case, outs["fasta"], skip=("vstrains.log.info",))
    assert case.binding(problems) in ([], ["unexpected files tmp/contigs_threaded.paths"])
