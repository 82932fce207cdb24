"""The site reader, the table writer and the refusals of ``vstrains_amd.node_depth --site-pairs`` and ``cli --depth-site-pairs``:
no device.  What the table must hold is tests/site_pairs_model.py's."""
import gzip
import os

import numpy as np
import pytest

import site_pairs_model as model
from test_pileup_cli_cpu import ALT, DEPTH, IDS, OFFSETS, SEQS, _Fake, _FakeCover, _FakeCtx, _FakeDepth, _FakePileup
from vstrains_amd import cli, node_depth
from vstrains_amd import pe as host

VCF = ("##fileformat=VCFv4.2\n##contig=<ID=s,length=7>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
       "s\t2\t.\tC\tA\t.\t.\tDP=197;AD=2;AF=0.010152\nu\t4\t.\tC\tT\n\ns\t7\ns\t2\t.\tC\tG\t.\t.\tDP=197\n")


@pytest.mark.parametrize("name", ["v.vcf", "v.vcf.gz"])
def test_the_site_reader_takes_chrom_and_pos_of_any_vcf(tmp_path, name):
    path = tmp_path / name
    path.write_bytes(gzip.compress(VCF.encode()) if name.endswith(".gz") else VCF.encode())
    # K = 4: s (7 bases) and u (4 bases) have positions; a position named by two records comes twice and is one site later
    assert node_depth.read_vcf_sites(str(path), IDS, SEQS, 3) == [(0, 1), (2, 3), (0, 6), (0, 1)]


@pytest.mark.parametrize("line, said", [("x\t1", "no segment x"), ("s\t8", "position 8 is outside segment s of 7 bases"), ("s\t0", "position 0 is outside segment s"),
                                        ("t\t1", "segment t has 3 bases, fewer than k \\+ 1 = 4"), ("s\tabc", "integer POS"), ("s", "integer POS")])
def test_the_site_reader_refuses_by_name(tmp_path, line, said):
    path = tmp_path / "v.vcf"
    path.write_text("#CHROM\tPOS\ns\t1\n" + line + "\n")
    with pytest.raises(ValueError, match=said) as e:
        node_depth.read_vcf_sites(str(path), IDS, SEQS, 3)
    assert "line 3" in str(e.value)


def _result(pairs):
    rows = model.result_rows(pairs)
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]).reshape(-1, 5, 5))


CELL = [[0, 2, 0, 0, 0], [0, 0, 0, 0, 0], [7, 0, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 3, 0]]
PAIRS = {((2, 0), (2, 3)): [[int(i == j == 3) * 12 for j in range(5)] for i in range(5)], ((0, 1), (0, 6)): CELL, ((0, 1), (0, 4)): [[5] + [0] * 4] + [[0] * 5] * 4}


@pytest.mark.parametrize("name", ["a.tsv", "a.tsv.gz"])
def test_the_table_has_a_row_for_every_non_zero_count(tmp_path, name):
    path = tmp_path / name
    node_depth.write_site_pairs(str(path), IDS, *_result(PAIRS))
    raw = path.read_bytes()
    assert (raw[:2] == b"\x1f\x8b") == name.endswith(".gz")
    lines = (gzip.decompress(raw) if name.endswith(".gz") else raw).decode().splitlines()
    assert lines[0] == "segment\tpos_a\tpos_b\tbase_a\tbase_b\tcount"
    got = [tuple(v if i in (0, 3, 4) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]
    assert got == model.table_rows(IDS, PAIRS)
    assert got == [("s", 2, 5, "A", "A", 5), ("s", 2, 7, "A", "C", 2), ("s", 2, 7, "G", "A", 7), ("s", 2, 7, "G", "N", 1), ("s", 2, 7, "N", "T", 3),
                   ("u", 1, 4, "T", "T", 12)]


def test_an_empty_result_is_a_header_line(tmp_path):
    node_depth.write_site_pairs(str(tmp_path / "e.tsv"), IDS, *_result({}))
    assert (tmp_path / "e.tsv").read_text() == "segment\tpos_a\tpos_b\tbase_a\tbase_b\tcount\n"


def test_the_sites_of_the_records():
    records = node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT)
    assert node_depth.record_sites(IDS, records) == [(0, 1), (0, 2), (0, 4), (0, 5), (0, 6), (2, 1)]  # (position 6 of s has two records: one site)


# ---- the refusals -------------------------------------------------------------------------------------------------------
@pytest.fixture
def files(tmp_path, monkeypatch):
    gfa, fq, vcf = tmp_path / "in.gfa", tmp_path / "x.fq", tmp_path / "v.vcf"
    gfa.write_bytes(b"S\ts\tACGTACG\tDP:f:3.0\nS\tt\tGGA\nS\tu\tTTAC\nL\ts\t+\tt\t+\t3M\n")
    fq.write_text("@r\nACGTAC\n+\nIIIIII\n")
    vcf.write_text(VCF)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return tmp_path, ["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", str(fq), "-r", str(fq)]


def _refused(d, argv, capsys, said):
    assert node_depth.main(argv) == 1
    assert said in capsys.readouterr().err and not (d / "out.gfa").exists() and not (d / "a.tsv").exists()


def test_flags_that_cannot_hold_are_refused_before_a_device_is_opened(files, monkeypatch, capsys):
    d, argv = files
    monkeypatch.setattr(host, "Context", None)  # (reaching it would fail the test: None is not callable)
    tsv, vcf = str(d / "a.tsv"), str(d / "v.vcf")
    _refused(d, argv + ["--site-pairs-max-span", "10"], capsys, "belong to --site-pairs")
    _refused(d, argv + ["--sites", vcf], capsys, "belong to --site-pairs")
    _refused(d, argv + ["--site-pairs", tsv, "--sites", vcf, "--site-pairs-max-span", "-1"], capsys, "from 0 up")
    _refused(d, argv + ["--site-pairs", tsv], capsys, "give --sites VCF, or --variants")
    _refused(d, argv + ["--site-pairs", tsv, "--pileup", str(d / "p.tsv")], capsys, "give --sites VCF, or --variants")
    _refused(d, argv + ["--site-pairs", tsv, "--sites", vcf, "--pileup-max-mismatch", "-2"], capsys, "from 0 up")
    # the two-pass form reads the reads twice: -f, -r and every --single must be regular files
    os.mkfifo(d / "pipe.fq")
    for flags in (["-f", str(d / "pipe.fq")], ["-r", str(d / "pipe.fq")], ["--single", str(d / "x.fq"), "--single", str(d / "pipe.fq"), "--count-singles"]):
        _refused(d, argv + flags + ["--site-pairs", tsv, "--variants", str(d / "v2.vcf")], capsys, "pipe.fq is not a regular file")
    # the sites are checked by name, before a device is opened
    for line, said in (("x\t1\n", "no segment x"), ("s\t9\n", "position 9 is outside segment s"), ("t\t2\n", "segment t has 3 bases")):
        (d / "bad.vcf").write_text(VCF + line)
        _refused(d, argv + ["-k", "3", "--site-pairs", tsv, "--sites", str(d / "bad.vcf")], capsys, said)


def test_more_than_one_rank_is_refused_with_the_site_pair_flags(files, monkeypatch):
    d, argv = files
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process only"):
        node_depth.main(argv + ["--site-pairs", str(d / "a.tsv"), "--sites", str(d / "v.vcf")])
    assert not (d / "out.gfa").exists() and not (d / "a.tsv").exists()


def test_depth_site_pairs_is_refused_without_depth_pileup_before_anything_is_written(tmp_path):
    gfa, paths, fq, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "r.fq", tmp_path / "out"
    gfa.write_bytes(b"S\ta\tACGT\tDP:f:1.0\n")
    paths.write_text("")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fq), "-rve", str(fq), "--depth-site-pairs"]
    for more in ([], ["--depth-from-reads"]):
        with pytest.raises(ValueError, match="--depth-from-reads --depth-pileup"):
            cli.main(argv + more)
        assert not out.exists()
    with pytest.raises(ValueError, match="--depth-from-reads"):  # (the pileup's own refusal comes first)
        cli.main(argv + ["--depth-pileup"])
    assert not out.exists()
    args = cli.build_parser().parse_args(argv + ["--depth-from-reads", "--depth-pileup"])
    assert cli.depth_site_pairs_refusal(args) is None
    os.mkfifo(tmp_path / "pipe.fq")
    args = cli.build_parser().parse_args(argv[:-2] + [str(tmp_path / "pipe.fq"), "--depth-site-pairs", "--depth-from-reads", "--depth-pileup"])
    assert "not a regular file" in cli.depth_site_pairs_refusal(args)
    assert "--depth-site-pairs" not in cli.build_parser().format_help()
    assert cli.depth_site_pairs_refusal(cli.build_parser().parse_args(argv[:-1])) is None


# ---- the two routes, the device taken out ---------------------------------------------------------------------------------
class _FakeSitePairs(_Fake):
    def __init__(self, ctx, sites, **kw):
        _Fake.__init__(self, ctx, **kw)
        type(self).made[-1] = ("_FakeSitePairs", dict(kw, sites=list(sites)))

    def result(self):
        return _result(PAIRS)

    def tallies(self):
        return 9, 1, 2, 30, 4


@pytest.fixture
def faked(files, monkeypatch):
    from vstrains_amd import pe_inference

    _Fake.made.clear()
    fed = []
    monkeypatch.setattr(host, "Context", _FakeCtx)
    monkeypatch.setattr(host, "DepthCounter", _FakeDepth)
    monkeypatch.setattr(host, "CoverCounter", _FakeCover)
    monkeypatch.setattr(host, "PileupCounter", _FakePileup)
    monkeypatch.setattr(host, "SitePairCounter", _FakeSitePairs)
    monkeypatch.setattr(pe_inference, "_resolve_inputs", lambda *a, **kw: None)
    monkeypatch.setattr(pe_inference, "feed_counter", lambda ctx, counter, *a, **kw: fed.append(counter))
    return files + (fed,)


TALLIES = " (9 fragments observing, 1 overflow fragments, 2 discordant sites, 30 pairs stored, 4 pairs unstored)"


def test_with_sites_the_counter_rides_on_the_one_read_pass(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv) == 0
    plain, said_plain = (d / "out.gfa").read_bytes(), capsys.readouterr().out
    assert "site pairs" not in said_plain and [m[0] for m in _Fake.made] == ["_FakeDepth"]
    _Fake.made.clear()
    del fed[:]
    assert node_depth.main(argv + ["-k", "3", "--site-pairs", str(d / "a.tsv"), "--sites", str(d / "v.vcf"), "--site-pairs-max-span", "5"]) == 0
    assert _Fake.made == [("_FakeDepth", {}), ("_FakeSitePairs", {"max_mismatch": 8, "max_span": 5, "sites": [(0, 1), (2, 3), (0, 6), (0, 1)]})]
    assert len(fed) == 1 and isinstance(fed[0], node_depth._Both) and isinstance(fed[0].main, _FakeDepth) and isinstance(fed[0].extra, _FakeSitePairs)
    said = capsys.readouterr().out
    assert said.rstrip().endswith("result stored in: %s; site pairs in: %s%s" % (d / "out.gfa", d / "a.tsv", TALLIES))
    assert (d / "out.gfa").read_bytes() == plain and len((d / "a.tsv").read_text().splitlines()) == 7
    # with the pileup as well: three counters behind one add, the budget given to both
    _Fake.made.clear()
    del fed[:]
    assert node_depth.main(argv + ["-k", "3", "--site-pairs", str(d / "b.tsv"), "--sites", str(d / "v.vcf"), "--variants", str(d / "w.vcf"), "--pileup-max-mismatch", "2"]) == 0
    assert [m[0] for m in _Fake.made] == ["_FakeDepth", "_FakePileup", "_FakeSitePairs"] and _Fake.made[1][1] == {"max_mismatch": 2}
    assert _Fake.made[2][1]["max_mismatch"] == 2 and _Fake.made[2][1]["max_span"] == 1000
    assert len(fed) == 1 and isinstance(fed[0].main, node_depth._Both) and isinstance(fed[0].extra, _FakeSitePairs)
    assert (d / "b.tsv").read_text() == (d / "a.tsv").read_text() and (d / "w.vcf").exists()


def test_without_sites_the_records_are_the_sites_of_a_second_pass(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv + ["--site-pairs", str(d / "a.tsv"), "--variants", str(d / "v2.vcf"), "--min-alt-count", "3"]) == 0
    want = node_depth.record_sites(IDS, node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT, min_alt_count=3))
    assert _Fake.made == [("_FakeDepth", {}), ("_FakePileup", {"max_mismatch": 8}), ("_FakeSitePairs", {"max_mismatch": 8, "max_span": 1000, "sites": want})]
    assert len(fed) == 2 and isinstance(fed[0], node_depth._Both) and isinstance(fed[1], _FakeSitePairs)  # pass 1 as without the flag, pass 2 alone
    assert capsys.readouterr().out.rstrip().endswith("; variants in: %s; site pairs in: %s%s" % (d / "v2.vcf", d / "a.tsv", TALLIES))
    # the sites of pass 2 are those a --sites run on the records written would read
    assert sorted(set(node_depth.read_vcf_sites(str(d / "v2.vcf"), IDS, SEQS, 3))) == want
