"""The host side of ``--depth-from-reads`` and ``vstrains_amd.node_depth`` without a device: the GFA rewrite as a pure
function, the inference of k, the refusals (raised before any output exists), and the help texts of ``pe_inference`` and
``cli``, which are the parent's (tests/golden/node_depth/*.txt, recorded at 100 columns) but for the new flag."""
import os

import pytest

from vstrains_amd import cli, node_depth, pe_inference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_depth")

GFA = (b"H\tVN:Z:1.0\n"
       b"S\ta\tACGTAC\tDP:f:12.5\tXX:Z:keep me\n"
       b"S\tb\tGGGG\tLN:i:4\tYY:i:7\tKC:i:99\n"
       b"L\ta\t+\tb\t-\t3M\n"
       b"S\tc\tTT\n"
       b"S\td\tACG\tdp:f:1.0\tkc:i:3\tln:i:3\tdpx:Z:stays\n"
       b"P\tp1\ta+,b-\t*\n"
       b"L\tb\t+\tc\t+\t3M\tXX:i:1\n")


def test_rewrite_replaces_the_depth_tags_and_keeps_the_rest():
    out = node_depth.rewrite_gfa(GFA, [10, 0, 7, 2 ** 40])
    assert out == (b"H\tVN:Z:1.0\n"
                   b"S\ta\tACGTAC\tLN:i:6\tKC:i:10\tXX:Z:keep me\n"
                   b"S\tb\tGGGG\tLN:i:4\tKC:i:0\tYY:i:7\n"
                   b"L\ta\t+\tb\t-\t3M\n"
                   b"S\tc\tTT\tLN:i:2\tKC:i:7\n"
                   b"S\td\tACG\tLN:i:3\tKC:i:1099511627776\tdpx:Z:stays\n"
                   b"P\tp1\ta+,b-\t*\n"
                   b"L\tb\t+\tc\t+\t3M\tXX:i:1\n")
    assert b"DP:f" not in out and b"dp:f" not in out


def test_rewrite_keeps_crlf_and_a_missing_final_newline():
    crlf = GFA.replace(b"\n", b"\r\n")[:-2]  # (the last line without its line end)
    out = node_depth.rewrite_gfa(crlf, [1, 2, 3, 4])
    assert out.count(b"\r\n") == crlf.count(b"\r\n") and not out.endswith(b"\n")
    assert out.replace(b"\r\n", b"\n") + b"\n" == node_depth.rewrite_gfa(GFA, [1, 2, 3, 4])
    # a rewrite of a rewrite changes nothing: the tags are replaced, not added
    assert node_depth.rewrite_gfa(out, [1, 2, 3, 4]) == out


def test_rewrite_wants_one_count_per_segment():
    with pytest.raises(ValueError):
        node_depth.rewrite_gfa(GFA, [1, 2, 3])
    with pytest.raises(ValueError):
        node_depth.rewrite_gfa(GFA, [1, 2, 3, 4, 5])


def test_strip_takes_out_what_rewrite_puts_in():
    stripped = node_depth.strip_depth_tags(GFA)
    assert b"DP:" not in stripped and b"KC:" not in stripped and b"ln:" not in stripped and b"dpx:Z:stays" in stripped
    assert node_depth.strip_depth_tags(node_depth.rewrite_gfa(GFA, [1, 2, 3, 4])) == stripped


def test_k_is_the_overlap_of_the_l_lines():
    assert node_depth.infer_k(GFA) == 3
    assert node_depth.infer_k(GFA.replace(b"\n", b"\r\n")) == 3


def test_k_is_refused_without_l_lines_or_when_they_disagree(tmp_path, capsys):
    none = b"".join(line for line in GFA.splitlines(keepends=True) if not line.startswith(b"L"))
    mixed = GFA.replace(b"3M\tXX", b"5M\tXX")
    for raw, word in ((none, "no L lines"), (mixed, "disagree")):
        with pytest.raises(ValueError, match=word):
            node_depth.infer_k(raw)
        gfa, out = tmp_path / "in.gfa", tmp_path / "out.gfa"
        gfa.write_bytes(raw)
        assert node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq"]) == 1
        assert word in capsys.readouterr().err and not out.exists()


def test_more_than_one_rank_is_refused_before_anything_exists(tmp_path, monkeypatch):
    gfa, out = tmp_path / "in.gfa", tmp_path / "out.gfa"
    gfa.write_bytes(GFA)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process only"):
        node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq"])
    assert not out.exists()
    args = cli.build_parser().parse_args(["-a", "spades", "-g", str(gfa), "-p", "p", "-o", str(tmp_path / "o"), "-fwd", "x", "-rve", "y",
                                          "--depth-from-reads"])
    assert "one process only" in cli.depth_from_reads_refusal(args, 2)
    assert cli.depth_from_reads_refusal(args, 1) is None  # (missing files are named by the ingest)


def test_a_pipe_is_refused_with_the_cli_flag_before_anything_is_written(tmp_path):
    fifo, fq = tmp_path / "reads.fifo", tmp_path / "r.fq"
    os.mkfifo(fifo)
    fq.write_text("@r\nACGT\n+\nIIII\n")
    gfa, paths, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "out"
    gfa.write_bytes(GFA)
    paths.write_text("")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fifo), "-rve", str(fq), "--depth-from-reads"]
    with pytest.raises(ValueError, match="reads the reads twice"):
        cli.main(argv)
    assert not out.exists()
    # with --pe-text-from the reads are read once: no refusal on that account
    args = cli.build_parser().parse_args(argv + ["--pe-text-from", str(tmp_path)])
    assert cli.depth_from_reads_refusal(args, 1) is None


def test_help_of_cli_is_the_parents_but_for_the_new_flag(monkeypatch):
    monkeypatch.setenv("COLUMNS", "100")
    p = cli.build_parser()
    new = [a for a in p._actions if a.dest == "depth_from_reads"]
    assert len(new) == 1 and new[0].option_strings == ["--depth-from-reads"] and new[0].default is False
    assert "--depth-from-reads" in p.format_help()
    p._remove_action(new[0])
    for group in p._action_groups:
        if new[0] in group._group_actions:
            group._group_actions.remove(new[0])
    with open(os.path.join(GOLDEN, "cli_help.txt")) as fh:
        assert p.format_help() == fh.read()


def test_help_of_pe_inference_is_unchanged(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as e:
        pe_inference.main(["--help"])
    assert e.value.code == 0
    with open(os.path.join(GOLDEN, "pe_inference_help.txt")) as fh:
        assert capsys.readouterr().out == fh.read()
