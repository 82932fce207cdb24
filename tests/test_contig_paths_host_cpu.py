"""The host side of ``vstrains_amd.contig_paths`` and ``cli --contigs-fasta`` without a device: the FASTA reader, the naming
of contigs, the entry writer, and the refusals, which are raised before anything is written or a device opened."""
import gzip

import pytest

import contig_thread_model as model
from vstrains_amd import cli, contig_paths

FASTA = (">NODE_1_length_12_cov_3.5 extra words\n"
         "ACGTAC\n"
         "gtacgt\n"
         "\n"
         ">polished_7\n"
         "ACGTNNacgt\n"
         ">empty\n"
         ">last no newline\n"
         "TTTT")


def test_reader_joins_lines_folds_case_and_keeps_the_first_word(tmp_path):
    p = tmp_path / "c.fasta"
    p.write_text(FASTA)
    names, seqs = contig_paths.read_fasta(str(p))
    assert names == ["NODE_1_length_12_cov_3.5", "polished_7", "empty", "last"]
    assert seqs == ["ACGTACGTACGT", "ACGTNNACGT", "", "TTTT"]


def test_reader_accepts_crlf_and_gzip(tmp_path):
    plain, crlf, gz = tmp_path / "c.fasta", tmp_path / "crlf.fasta", tmp_path / "c.fasta.gz"
    plain.write_text(FASTA)
    crlf.write_bytes(FASTA.replace("\n", "\r\n").encode())
    gz.write_bytes(gzip.compress(FASTA.encode()))
    want = contig_paths.read_fasta(str(plain))
    assert contig_paths.read_fasta(str(crlf)) == want and contig_paths.read_fasta(str(gz)) == want


def test_reader_refuses_text_in_front_of_the_first_header(tmp_path):
    p = tmp_path / "c.fasta"
    p.write_text("ACGT\n>a\nACGT\n")
    with pytest.raises(ValueError, match="in front of the first"):
        contig_paths.read_fasta(str(p))


def test_a_record_that_is_too_long_is_refused_by_name(tmp_path, capsys):
    p, out = tmp_path / "c.fasta", tmp_path / "o.paths"
    line = "ACGT" * 16 + "\n"
    n_lines = contig_paths.MAX_CONTIG // 64 + 1  # one line more than fits
    p.write_text(">fine\nACGT\n>chr_too_long some words\n" + line * n_lines)
    with pytest.raises(ValueError, match="chr_too_long holds %d bases" % (64 * n_lines)):
        contig_paths.read_fasta(str(p))
    # the command says so and writes nothing (the FASTA is read before a device is opened)
    assert contig_paths.main(["-g", str(tmp_path / "none.gfa"), "-c", str(p), "-o", str(out)]) == 1
    assert "chr_too_long" in capsys.readouterr().err and not out.exists()
    # exactly 2^24 - 1 bases are taken
    p.write_text(">edge\n" + "A" * contig_paths.MAX_CONTIG + "\n")
    assert len(contig_paths.read_fasta(str(p))[1][0]) == (1 << 24) - 1


GFA = (b"S\ta\tACGTACGTAC\tDP:f:12.5\n"
       b"S\tb\tGGGGACGT\tLN:i:8\tKC:i:100\n"
       b"S\tc\tTTTT\n"
       b"L\ta\t+\tb\t+\t3M\n")


def test_depths_are_read_as_the_graph_loader_reads_them():
    assert contig_paths.segment_depths(GFA) == [12.5, 100 / 8, None]


def test_a_spades_name_is_kept_and_any_other_contig_is_named_from_its_segments():
    ids, depths = ["a", "b", "c"], [10.0, 2.5, None]
    parts = [[(0, 0, 3), (1, 1, 1)], [(0, 1, 4)]]
    assert contig_paths.contig_name("NODE_7_length_99_cov_1.25", 3, 50, parts, depths, ids) == "NODE_7_length_99_cov_1.25"
    # window-weighted mean: (10 * 3 + 2.5 * 1 + 10 * 4) / 8, repr-formatted
    assert contig_paths.contig_name("polished_7", 3, 50, parts, depths, ids) == "NODE_3_length_50_cov_" + repr(72.5 / 8)
    assert contig_paths.contig_name("NODE_x", 1, 9, [[(1, 0, 2)]], depths, ids) == "NODE_1_length_9_cov_2.5"
    with pytest.raises(ValueError, match="segment c carries no depth tag"):
        contig_paths.contig_name("polished_7", 3, 50, [[(2, 0, 1)]], depths, ids)
    # a SPAdes name needs no depth
    assert contig_paths.contig_name("NODE_1_length_4_cov_0.5", 1, 4, [[(2, 0, 1)]], depths, ids) == "NODE_1_length_4_cov_0.5"


def test_entry_is_the_forward_walk_and_its_mirror():
    ids = ["8", "9", "10"]
    parts = [[(0, 0, 3), (1, 0, 1), (2, 1, 2)], [(0, 1, 4), (0, 1, 4)]]
    text = contig_paths.format_entry("NODE_1_length_5_cov_1.0", parts, ids)
    assert text == ("NODE_1_length_5_cov_1.0\n8+,9+,10-;\n8-,8-\n"
                    "NODE_1_length_5_cov_1.0'\n8+,8+;\n10+,9-,8-\n")
    assert text == model.entry("NODE_1_length_5_cov_1.0", parts, ids)


def _argv(tmp_path, *more):
    gfa = tmp_path / "g.gfa"
    gfa.write_bytes(GFA)
    fa = tmp_path / "c.fasta"
    fa.write_text(FASTA)
    fq = tmp_path / "r.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    return ["-a", "spades", "-g", str(gfa), "-o", str(tmp_path / "out"), "-fwd", str(fq), "-rve", str(fq), "--contigs-fasta", str(fa)] + list(more)


def test_cli_refuses_p_together_with_contigs_fasta(tmp_path):
    paths = tmp_path / "c.paths"
    paths.write_text("")
    with pytest.raises(ValueError, match="mutually exclusive"):
        cli.main(_argv(tmp_path, "-p", str(paths)))
    assert not (tmp_path / "out").exists()


def test_cli_and_the_module_refuse_a_process_group_before_anything_exists(tmp_path, monkeypatch):
    argv = _argv(tmp_path)
    args = cli.build_parser().parse_args(argv)
    assert args.contigs_fasta == argv[-1] and args.path_file is None
    assert cli.contigs_fasta_refusal(args, 1) is None
    assert "one process only" in cli.contigs_fasta_refusal(args, 2)
    # (cli.main asks the initialised process group for its size; the module's own command reads WORLD_SIZE, as node_depth does)
    monkeypatch.setenv("WORLD_SIZE", "2")
    out = tmp_path / "o.paths"
    assert contig_paths.main(["-g", argv[3], "-c", argv[-1], "-o", str(out)]) == 1 and not out.exists()


def test_cli_without_either_still_demands_the_paths_file(tmp_path, capsys):
    argv = _argv(tmp_path)[:-2]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1 and "Path to Contig file from SPAdes (.paths format) is required" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.main(argv + ["--contigs-fasta", str(tmp_path / "missing.fasta")])
    assert "--contigs-fasta" in capsys.readouterr().out and not (tmp_path / "out").exists()
