"""The writers and the refusals of ``vstrains_amd.node_depth --strands / --min-alt-strand-count`` and ``cli --depth-strands``
from hand-made ``(offsets, depth [P, 2], alt [P, 2, 5])`` tables: no device.  What the table and the records must hold is
tests/strand_pileup_model.py's; the records are made by ``node_depth.call_host``, the rule the device runs."""
import gzip
import re

import numpy as np
import pytest

import strand_pileup_model as model
from vstrains_amd import cli, node_depth
from vstrains_amd import pe as host

# K = 4: segment s (7 bases) and u (4 bases, exactly K) have rows, t (3 bases) has none
IDS = ["s", "t", "u"]
SEQS = ["ACGTACG", "GGA", "TTAC"]
OFFSETS = np.array([0, 7, 7, 11])
DEPTH = np.array([[0, 0], [120, 80], [100, 100], [150, 50], [3, 0], [600, 400], [4, 3], [5, 0], [2, 3], [0, 0], [2, 4]])
ALT = np.array([[[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                [[2, 0, 1, 0, 3], [0, 0, 0, 0, 0]],    # C: A 2 + 0 of DP 197 -> a record, all on the forward strand
                [[1, 0, 0, 0, 0], [1, 0, 0, 0, 0]],    # G: A 1 + 1 of DP 200: the fraction at equality -> a record on both strands
                [[1, 1, 0, 0, 0], [0, 0, 1, 0, 0]],    # T: three bases with 1 each: none reaches the count of 2
                [[0, 3, 0, 0, 0], [0, 0, 0, 0, 0]],    # A: C 3 of DP 3 -> AF 1.000000
                [[4, 0, 5, 6, 0], [5, 0, 5, 5, 0]],    # C of DP 1000: A 9 < 10.0, G 5 + 5 == 10.0, T 6 + 5
                [[0, 0, 0, 1, 2], [0, 0, 0, 1, 2]],    # G: T 1 + 1 of DP 3 (`other` is not part of DP) -> AF 0.666667
                [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                [[2, 0, 0, 0, 0], [3, 0, 0, 0, 0]],    # T: A 2 + 3 of DP 5: the reference base's own count is 0 on both strands
                [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                [[0, 0, 0, 0, 2], [0, 0, 0, 0, 4]]])   # C: only `other`: DP 0, no record


def _lists():
    cut = [(int(OFFSETS[n]), int(OFFSETS[n + 1])) for n in range(3)]
    return [DEPTH[a:b].tolist() for a, b in cut], [ALT[a:b].tolist() for a, b in cut]


def _lines(path):
    raw = path.read_bytes()
    return (gzip.decompress(raw) if str(path).endswith(".gz") else raw).decode().splitlines()


@pytest.mark.parametrize("name", ["p.tsv", "p.tsv.gz"])
def test_the_table_has_the_columns_of_both_strands(tmp_path, name):
    path = tmp_path / name
    node_depth.write_strand_pileup(str(path), IDS, SEQS, OFFSETS, DEPTH, ALT)
    assert (path.read_bytes()[:2] == b"\x1f\x8b") == name.endswith(".gz")
    lines = _lines(path)
    assert lines[0] == "segment\tpos\tref\tA+\tC+\tG+\tT+\tother+\tA-\tC-\tG-\tT-\tother-" == "\t".join(model.PILEUP_COLUMNS)
    got = [tuple(v if i in (0, 2) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]
    assert got == model.table_rows(IDS, SEQS, *_lists()) and len(got) == 11 and not [r for r in got if r[0] == "t"]
    assert got[1] == ("s", 2, "C", 2, 114, 1, 0, 3, 0, 80, 0, 0, 0) and got[8] == ("u", 2, "T", 2, 0, 0, 0, 0, 3, 0, 0, 0, 0)
    # summed over the strands it is the unstranded table
    node_depth.write_pileup(str(tmp_path / "sum.tsv"), IDS, SEQS, OFFSETS, DEPTH.sum(axis=1), ALT.sum(axis=1))
    plain = [[int(v) for v in line.split("\t")[3:]] for line in _lines(tmp_path / "sum.tsv")[1:]]
    assert plain == [[r[3 + c] + r[8 + c] for c in range(5)] for r in got]


@pytest.mark.parametrize("S", [0, 1, 2])
def test_the_records_are_the_models(S):
    called = node_depth.call_host(SEQS, OFFSETS, DEPTH, ALT, 2, 0.01, S)
    got = node_depth.strand_records(IDS, called, S)
    want = model.variant_records(IDS, SEQS, *_lists(), 2, 0.01, S)
    assert [r[:6] + r[6:] for r in got] == [r[:6] + r[7:] for r in want] and len(got) == 7
    assert [r[7] for r in got] == {0: ["."] * 7, 1: ["strand", "PASS", "strand", "PASS", "PASS", "PASS", "PASS"],
                                   2: ["strand", "strand", "strand", "PASS", "PASS", "strand", "PASS"]}[S]
    assert got[3] == ("s", 6, "C", "G", 1000, 10, (585, 385, 5, 5), got[3][7])
    assert [a.dtype for a in called] == [np.int64] * 6 + [np.bool_] and called[5].shape == (7, 4)


@pytest.mark.parametrize("name, S", [("v.vcf", 0), ("v.vcf.gz", 2)])
def test_the_vcf_gains_dp4_and_with_a_threshold_the_filter(tmp_path, name, S):
    path = tmp_path / name
    node_depth.write_strand_vcf(str(path), IDS, SEQS, OFFSETS, node_depth.call_host(SEQS, OFFSETS, DEPTH, ALT, 2, 0.01, S), S)
    lines = _lines(path)
    head = [line for line in lines if line.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == "##source=vstrains_amd.node_depth"
    assert head[2:4] == ["##contig=<ID=s,length=7>", "##contig=<ID=u,length=4>"]
    assert [line.split(",")[0] for line in head[4:8]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=AF", "##INFO=<ID=DP4"]
    assert head[7].startswith("##INFO=<ID=DP4,Number=4,Type=Integer,Description=")
    assert [line for line in head if line.startswith("##FILTER")] == (['##FILTER=<ID=strand,Description="Fewer than 2 reads carry the alternate base on one '
                                                                       'of the two strands">'] if S else [])
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and len(head) == (10 if S else 9)
    body = lines[len(head):]
    assert body == ["%s\t%d\t.\t%s\t%s\t.\t%s\tDP=%d;AD=%d;AF=%s;DP4=%d,%d,%d,%d" % (r[:4] + (r[8],) + r[4:7] + r[7])
                    for r in model.variant_records(IDS, SEQS, *_lists(), 2, 0.01, S)]
    assert body[0] == "s\t2\t.\tC\tA\t.\t%s\tDP=197;AD=2;AF=0.010152;DP4=114,80,2,0" % ("strand" if S else ".")


def strip(lines):
    """The records with ``;DP4=...`` dropped and FILTER put back to ``.``: what the unstranded command writes."""
    out = []
    for line in lines:
        if not line.startswith("#"):
            cols = re.sub(r";DP4=\d+,\d+,\d+,\d+$", "", line).split("\t")
            cols[6] = "."
            out.append("\t".join(cols))
    return out


@pytest.mark.parametrize("C_, F, S", [(2, 0.01, 0), (2, 0.01, 1), (0, 0.0, 3), (3, 0.0101, 0)])
def test_without_dp4_and_filter_the_records_are_the_unstranded_ones_byte_for_byte(tmp_path, C_, F, S):
    node_depth.write_strand_vcf(str(tmp_path / "s.vcf"), IDS, SEQS, OFFSETS, node_depth.call_host(SEQS, OFFSETS, DEPTH, ALT, C_, F, S), S)
    node_depth.write_vcf(str(tmp_path / "u.vcf"), IDS, SEQS, OFFSETS, DEPTH.sum(axis=1), ALT.sum(axis=1), C_, F)
    plain = [line for line in _lines(tmp_path / "u.vcf") if not line.startswith("#")]
    assert strip(_lines(tmp_path / "s.vcf")) == plain and len(plain) == {(2, 0): 7, (2, 1): 7, (0, 3): 12, (3, 0): 3}[(C_, S)]


# ---- the refusals -------------------------------------------------------------------------------------------------------
def test_the_parser_defaults():
    args = node_depth.build_parser().parse_args(["-g", "g", "-o", "o", "-f", "f", "-r", "r"])
    assert args.strands is False and args.min_alt_strand_count is None and node_depth.pileup_refusal(args) is None
    args = node_depth.build_parser().parse_args(["-g", "g", "-o", "o", "-f", "f", "-r", "r", "--variants", "v", "--strands", "--min-alt-strand-count", "2"])
    assert args.strands is True and args.min_alt_strand_count == 2 and node_depth.pileup_refusal(args) is None
    args = node_depth.build_parser().parse_args(["-g", "g", "-o", "o", "-f", "f", "-r", "r", "--pileup", "p", "--strands"])
    assert node_depth.pileup_refusal(args) is None


@pytest.mark.parametrize("flags, said", [(["--strands"], "--strands keeps the strands of the pileup apart: give --pileup or --variants with it"),
                                         (["--strands", "--profile", "p.bg"], "give --pileup or --variants with it"),
                                         (["--variants", "v.vcf", "--min-alt-strand-count", "2"], "--min-alt-strand-count filters the records of --variants by strand: "
                                                                                                  "give --strands and --variants with it"),
                                         (["--pileup", "p.tsv", "--strands", "--min-alt-strand-count", "2"], "give --strands and --variants with it"),
                                         (["--min-alt-strand-count", "2"], "give --strands and --variants with it"),
                                         (["--variants", "v.vcf", "--strands", "--min-alt-strand-count", "0"], "--min-alt-strand-count 0: a count from 1 up is needed"),
                                         (["--variants", "v.vcf", "--strands", "--min-alt-strand-count", "-3"], "a count from 1 up is needed")])
def test_flags_that_cannot_hold_are_refused_by_name_before_a_device_is_opened(tmp_path, monkeypatch, capsys, flags, said):
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(host, "Context", None)  # (reaching it would fail the test: None is not callable)
    assert node_depth.main(["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", "x.fq", "-r", "y.fq"] + flags) == 1
    assert said in capsys.readouterr().err and not (tmp_path / "out.gfa").exists()


def test_more_than_one_rank_is_refused_with_the_strand_flags(tmp_path, monkeypatch):
    gfa, out, vcf = tmp_path / "in.gfa", tmp_path / "out.gfa", tmp_path / "v.vcf"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process only"):
        node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq", "--variants", str(vcf), "--strands"])
    assert not out.exists() and not vcf.exists()


def test_depth_strands_is_refused_without_depth_pileup_before_anything_is_written(tmp_path, monkeypatch):
    gfa, paths, fq, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "r.fq", tmp_path / "out"
    gfa.write_bytes(b"S\ta\tACGT\tDP:f:1.0\n")
    paths.write_text("")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fq), "-rve", str(fq), "--depth-strands"]
    for more in ([], ["--depth-from-reads"]):
        with pytest.raises(ValueError, match="--depth-strands keeps the strands of the pileup apart: give --depth-from-reads --depth-pileup with it"):
            cli.main(argv + more)
        assert not out.exists()
    with pytest.raises(ValueError, match="--depth-from-reads"):  # (--depth-pileup's own refusal comes first)
        cli.main(argv + ["--depth-pileup"])
    assert not out.exists()
    args = cli.build_parser().parse_args(argv + ["--depth-from-reads", "--depth-pileup"])
    assert args.depth_strands and cli.depth_strands_refusal(args) is None
    assert cli.build_parser().parse_args(argv[:-1]).depth_strands is False
    assert "--depth-strands" not in cli.build_parser().format_help()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    assert "one process only" in cli.depth_from_reads_refusal(args, 2)  # (under a process group: refused like the depth pass it rides on)


# ---- the command with the device taken out --------------------------------------------------------------------------------
class _Fake:
    made = []

    def __init__(self, ctx, *a, **kw):
        type(self).made.append((type(self).__name__, kw))
        self.ends_seen = 4
        self.device, self.single_stats = "dev", None


class _FakeDepth(_Fake):
    def result(self):
        return np.array([10, 13, 2])


class _FakePileup(_Fake):
    def result(self):
        return OFFSETS, DEPTH.sum(axis=1), ALT.sum(axis=1)

    def tallies(self):
        return 12, 1


class _FakeStrands(_Fake):
    called = []

    def result(self):
        return OFFSETS, DEPTH, ALT

    def tallies(self):
        return 12, 1

    def call(self, *thresholds):
        type(self).called.append(thresholds)
        return node_depth.call_host(SEQS, OFFSETS, DEPTH, ALT, *thresholds)


class _FakeCtx:
    def __init__(self, device=0):
        pass

    def build_index(self, seqs, k):
        pass

    def sync(self):
        pass

    def keep_masks(self, on):
        pass


@pytest.fixture
def faked(monkeypatch, tmp_path):
    """``node_depth.main`` with the device taken out: the context, the counters and the input dispatch are stand-ins."""
    from vstrains_amd import pe_inference

    _Fake.made.clear()
    _FakeStrands.called.clear()
    fed = []
    monkeypatch.setattr(host, "Context", _FakeCtx)
    monkeypatch.setattr(host, "DepthCounter", _FakeDepth)
    monkeypatch.setattr(host, "PileupCounter", _FakePileup)
    monkeypatch.setattr(host, "StrandPileupCounter", _FakeStrands)
    monkeypatch.setattr(pe_inference, "_resolve_inputs", lambda *a, **kw: None)
    monkeypatch.setattr(pe_inference, "feed_counter", lambda ctx, counter, *a, **kw: fed.append(counter))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ts\tACGTACG\tDP:f:3.0\nS\tt\tGGA\nS\tu\tTTAC\nL\ts\t+\tt\t+\t3M\n")
    (tmp_path / "x.fq").write_text("@r\nACGTAC\n+\nIIIIII\n")
    return tmp_path, ["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", str(tmp_path / "x.fq"), "-r", str(tmp_path / "x.fq")], fed


def test_with_strands_the_stranded_counter_takes_the_pileups_place_in_the_one_read_pass(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv + ["--pileup", str(d / "p.tsv"), "--variants", str(d / "v.vcf")]) == 0
    assert [m[0] for m in _Fake.made] == ["_FakeDepth", "_FakePileup"] and not _FakeStrands.called  # (without the flag: as before)
    plain_gfa, said_plain = (d / "out.gfa").read_bytes(), capsys.readouterr().out
    _Fake.made.clear()
    del fed[:]
    flags = ["--pileup", str(d / "q.tsv"), "--variants", str(d / "w.vcf"), "--strands", "--min-alt-strand-count", "2", "--min-alt-count", "1", "--pileup-max-mismatch", "3"]
    assert node_depth.main(argv + flags) == 0
    assert _Fake.made == [("_FakeDepth", {}), ("_FakeStrands", {"max_mismatch": 3})] and _FakeStrands.called == [(1, 0.01, 2)]
    assert len(fed) == 1 and isinstance(fed[0], node_depth._Both) and isinstance(fed[0].extra, _FakeStrands)  # one read pass
    assert (d / "out.gfa").read_bytes() == plain_gfa
    assert capsys.readouterr().out.split("; pileup in:")[0] == said_plain.split("; pileup in:")[0]
    assert (d / "q.tsv").read_text().splitlines()[0].split("\t")[3:] == list(model.PILEUP_COLUMNS[3:])
    lines = (d / "w.vcf").read_text().splitlines()
    node_depth.write_vcf(str(d / "want.vcf"), IDS, SEQS, OFFSETS, DEPTH.sum(axis=1), ALT.sum(axis=1), 1, 0.01)
    assert strip(lines) == [line for line in (d / "want.vcf").read_text().splitlines() if not line.startswith("#")]
    assert set(line.split("\t")[6] for line in lines if not line.startswith("#")) == {"PASS", "strand"}


def test_site_pairs_without_sites_take_them_from_the_stranded_records(faked, monkeypatch):
    d, argv, fed = faked
    seen = []

    def second_pass(ctx, sites, *a, **kw):
        seen.append(sites)
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 5, 5), np.int64), (0, 0, 0, 0, 0)

    monkeypatch.setattr(node_depth, "site_pairs_pass", second_pass)
    assert node_depth.main(argv + ["--variants", str(d / "v.vcf"), "--strands", "--site-pairs", str(d / "sp.tsv")]) == 0
    want = node_depth.record_sites(IDS, node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH.sum(axis=1), ALT.sum(axis=1)))
    assert seen == [want] and len(want) == 6
