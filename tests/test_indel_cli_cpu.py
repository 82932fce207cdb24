"""The record rule, the writer and the refusals of ``vstrains_amd.node_depth --indels`` and ``cli --depth-indels`` from hand-made
events and pileup tables, and the command with the device taken out: no device."""
import gzip

import numpy as np
import pytest

from vstrains_amd import cli, node_depth
from vstrains_amd import pe as host

# K = 4: segment s (12 bases) and u (6 bases) have rows, t (3 bases) has none
IDS = ["s", "t", "u"]
SEQS = ["ACGTACGGTCAT", "GGA", "TTACGA"]
OFFSETS = np.array([0, 12, 12, 18])
DEPTH = np.zeros(18, dtype=np.int64)
ALT = np.zeros((18, 5), dtype=np.int64)
DEPTH[2], ALT[2] = 95, [1, 0, 0, 0, 2]      # s pos0 2 (G): 93 reads with A, C, G or T
DEPTH[5], ALT[5] = 93, [0, 0, 0, 0, 0]      # s pos0 5 (C): 93
DEPTH[0], ALT[0] = 10, [0, 3, 0, 0, 1]      # s pos0 0 (A): 9
DEPTH[3], ALT[3] = 40, [0, 0, 0, 0, 0]      # s pos0 3 (T): 40
DEPTH[12], ALT[12] = 7, [0, 0, 0, 0, 0]     # u pos0 0 (T): 7
DEPTH[14], ALT[14] = 6, [0, 0, 0, 0, 0]     # u pos0 2 (A): 6
EVENTS = [(0, 0, 0, 3, "", 2, 2),           # a deletion at u == 0: the anchor is F[3] behind it
          (0, 0, 1, 2, "GG", 0, 5),         # an insertion at u == 0: the anchor is F[0] behind it
          (0, 3, 0, 2, "", 4, 3),           # AD 7 of DP 100: 0.07 * 100 > 7 in doubles, so F = 0.07 takes it out
          (0, 3, 1, 1, "C", 1, 0),          # AD 1: below the count of 2
          (0, 6, 1, 3, "TTA", 3, 4),        # AD 7 of DP 100 again, as an insertion
          (2, 1, 0, 1, "", 2, 0),           # on u, forward strand only
          (2, 3, 1, 1, "G", 1, 1)]


def test_the_records_anchor_and_alleles():
    got = node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 2, 0.01, 0)
    assert got == [("s", 1, "ACGT", "T", 44, 4, 2, 2, "."),         # POS 1, REF F[0:4], ALT F[3]; DP = 4 + 40
                   ("s", 1, "A", "GGA", 14, 5, 0, 5, "."),          # REF F[0], ALT I + F[0]; DP = 5 + 9
                   ("s", 3, "GTA", "G", 100, 7, 4, 3, "."),         # POS u, REF F[u-1 : u+L], ALT F[u-1]; DP = 7 + 93
                   ("s", 6, "C", "CTTA", 100, 7, 3, 4, "."),        # REF F[u-1], ALT F[u-1] + I
                   ("u", 1, "TT", "T", 9, 2, 2, 0, "."),
                   ("u", 3, "A", "AG", 8, 2, 1, 1, ".")]


def test_the_fraction_at_equality_is_one_double_product():
    assert 0.07 * 100.0 > 7.0  # (the product as it stands: AD = 7 of DP = 100 is no record at F = 0.07)
    got = node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 2, 0.07, 0)
    assert [r[:2] for r in got] == [("s", 1), ("s", 1), ("u", 1), ("u", 3)]
    assert 0.0625 * 112.0 == 7.0
    depth = DEPTH.copy()
    depth[2] += 12  # DP = 7 + 105 = 112
    got = node_depth.indel_records(IDS, SEQS, EVENTS[2:3], OFFSETS, depth, ALT, 2, 0.0625, 0)
    assert got == [("s", 3, "GTA", "G", 112, 7, 4, 3, ".")]  # an exact product at equality is a record
    assert node_depth.indel_records(IDS, SEQS, EVENTS[2:3], OFFSETS, depth, ALT, 8, 0.0, 0) == []
    assert len(node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 0, 0.0, 0)) == len(EVENTS)


def test_the_strand_threshold_marks_and_never_removes():
    for S, want in ((1, ["PASS", "strand", "PASS", "PASS", "strand", "PASS"]), (3, ["strand", "strand", "PASS", "PASS", "strand", "strand"])):
        got = node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 2, 0.01, S)
        assert [r[8] for r in got] == want and [r[:8] for r in got] == [r[:8] for r in node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 2, 0.01, 0)]


def test_the_planes_of_a_stranded_pileup_are_summed():
    depth2 = np.stack([DEPTH // 2, DEPTH - DEPTH // 2], axis=1)
    alt2 = np.stack([ALT // 2, ALT - ALT // 2], axis=1)
    assert node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, depth2, alt2) == node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT)


def _lines(path):
    raw = path.read_bytes()
    return (gzip.decompress(raw) if str(path).endswith(".gz") else raw).decode().splitlines()


@pytest.mark.parametrize("name, S", [("i.vcf", 0), ("i.vcf.gz", 2)])
def test_the_vcf(tmp_path, name, S):
    path = tmp_path / name
    records = node_depth.indel_records(IDS, SEQS, EVENTS, OFFSETS, DEPTH, ALT, 2, 0.01, S)
    node_depth.write_indel_vcf(str(path), IDS, SEQS, OFFSETS, records, S)
    assert (path.read_bytes()[:2] == b"\x1f\x8b") == name.endswith(".gz")
    lines = _lines(path)
    head = [line for line in lines if line.startswith("#")]
    assert head[:4] == ["##fileformat=VCFv4.2", "##source=vstrains_amd.node_depth", "##contig=<ID=s,length=12>", "##contig=<ID=u,length=6>"]
    assert [line.split(",")[0] for line in head[4:9]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=AF", "##INFO=<ID=ADF", "##INFO=<ID=ADR"]
    assert [line for line in head if line.startswith("##FILTER")] == (['##FILTER=<ID=strand,Description="Fewer than 2 read ends carry the event on one of the two '
                                                                       'strands">'] if S else [])
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and len(head) == (11 if S else 10)
    body = lines[len(head):]
    assert len(body) == 6
    assert body[0] == "s\t1\t.\tACGT\tT\t.\t%s\tDP=44;AD=4;AF=0.090909;ADF=2;ADR=2" % ("PASS" if S else ".")
    assert body[2] == "s\t3\t.\tGTA\tG\t.\t%s\tDP=100;AD=7;AF=0.070000;ADF=4;ADR=3" % ("PASS" if S else ".")


# ---- the refusals -------------------------------------------------------------------------------------------------------
def test_the_parser_defaults():
    args = node_depth.build_parser().parse_args(["-g", "g", "-o", "o", "-f", "f", "-r", "r"])
    assert args.indels is None and args.indel_max_length is None and args.min_indel_count is None and args.min_indel_frac is None
    assert node_depth.indel_refusal(args) is None
    args = node_depth.build_parser().parse_args(["-g", "g", "-o", "o", "-f", "f", "-r", "r", "--indels", "i.vcf", "--indel-max-length", "32", "--min-indel-count", "0",
                                                 "--min-indel-frac", "1.0", "--min-alt-strand-count", "2"])
    assert node_depth.indel_refusal(args) is None and node_depth.pileup_refusal(args) is None


@pytest.mark.parametrize("flags, said", [(["--indels", "i.vcf", "--indel-max-length", "0"], "--indel-max-length 0: a length from 1 to 32 is needed"),
                                         (["--indels", "i.vcf", "--indel-max-length", "33"], "--indel-max-length 33: a length from 1 to 32 is needed"),
                                         (["--indels", "i.vcf", "--min-indel-count", "-1"], "--min-indel-count -1: a count from 0 up is needed"),
                                         (["--indels", "i.vcf", "--min-indel-frac", "1.5"], "--min-indel-frac 1.5: a fraction between 0 and 1 is needed"),
                                         (["--indel-max-length", "8"], "--indel-max-length, --min-indel-count and --min-indel-frac belong to --indels: give it"),
                                         (["--variants", "v.vcf", "--min-indel-count", "3"], "belong to --indels: give it"),
                                         (["--pileup", "p.tsv", "--min-indel-frac", "0.1"], "belong to --indels: give it"),
                                         (["--indels", "i.vcf", "--strands"], "--strands keeps the strands of the pileup apart: give --pileup or --variants with it"),
                                         (["--min-alt-strand-count", "2"], "give --strands and --variants with it")])
def test_flags_that_cannot_hold_are_refused_by_name_before_a_device_is_opened(tmp_path, monkeypatch, capsys, flags, said):
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(host, "Context", None)  # (reaching it would fail the test: None is not callable)
    assert node_depth.main(["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", "x.fq", "-r", "y.fq"] + flags) == 1
    assert said in capsys.readouterr().err and not (tmp_path / "out.gfa").exists() and not (tmp_path / "i.vcf").exists()


def test_a_process_group_is_refused_by_name(tmp_path, monkeypatch, capsys):
    gfa, out, vcf = tmp_path / "in.gfa", tmp_path / "out.gfa", tmp_path / "i.vcf"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(host, "Context", None)
    assert node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq", "--indels", str(vcf)]) == 1
    assert "--indels finds its events in one process only, and this process group has 2 ranks" in capsys.readouterr().err
    assert not out.exists() and not vcf.exists()


def test_depth_indels_is_refused_without_depth_pileup_before_anything_is_written(tmp_path):
    gfa, paths, fq, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "r.fq", tmp_path / "out"
    gfa.write_bytes(b"S\ta\tACGT\tDP:f:1.0\n")
    paths.write_text("")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fq), "-rve", str(fq), "--depth-indels"]
    for more in ([], ["--depth-from-reads"]):
        with pytest.raises(ValueError, match="--depth-indels measures its events against the pileup: give --depth-from-reads --depth-pileup with it"):
            cli.main(argv + more)
        assert not out.exists()
    args = cli.build_parser().parse_args(argv + ["--depth-from-reads", "--depth-pileup"])
    assert args.depth_indels and cli.depth_indels_refusal(args) is None
    assert cli.build_parser().parse_args(argv[:-1]).depth_indels is False
    assert "--depth-indels" not in cli.build_parser().format_help()


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
        return OFFSETS, DEPTH, ALT

    def tallies(self):
        return 12, 1


class _FakeIndels(_Fake):
    def result(self):
        return EVENTS

    def tallies(self):
        return 31, 3, 4, 1


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
    fed = []
    monkeypatch.setattr(host, "Context", _FakeCtx)
    monkeypatch.setattr(host, "DepthCounter", _FakeDepth)
    monkeypatch.setattr(host, "PileupCounter", _FakePileup)
    monkeypatch.setattr(host, "IndelCounter", _FakeIndels)
    monkeypatch.setattr(pe_inference, "_resolve_inputs", lambda *a, **kw: None)
    monkeypatch.setattr(pe_inference, "feed_counter", lambda ctx, counter, *a, **kw: fed.append(counter))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ts\tACGTACGGTCAT\tDP:f:3.0\nS\tt\tGGA\nS\tu\tTTACGA\nL\ts\t+\tt\t+\t3M\n")
    (tmp_path / "x.fq").write_text("@r\nACGTAC\n+\nIIIIII\n")
    return tmp_path, ["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", str(tmp_path / "x.fq"), "-r", str(tmp_path / "x.fq")], fed


def test_the_variants_file_and_the_gfa_are_byte_identical_with_and_without_indels(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv + ["--variants", str(d / "v.vcf")]) == 0
    assert [m[0] for m in _Fake.made] == ["_FakeDepth", "_FakePileup"]  # (without the flag no indel counter is built)
    plain_gfa, plain_vcf, said_plain = (d / "out.gfa").read_bytes(), (d / "v.vcf").read_bytes(), capsys.readouterr().out
    assert "indels" not in said_plain and "matches tested" not in said_plain
    _Fake.made.clear()
    del fed[:]
    assert node_depth.main(argv + ["--variants", str(d / "w.vcf"), "--indels", str(d / "i.vcf"), "--indel-max-length", "7", "--min-indel-frac", "0.07"]) == 0
    assert _Fake.made == [("_FakeDepth", {}), ("_FakePileup", {"max_mismatch": 8}), ("_FakeIndels", {"max_len": 7})]
    assert len(fed) == 1 and isinstance(fed[0], node_depth._Both) and isinstance(fed[0].extra, _FakeIndels)  # one read pass
    assert (d / "out.gfa").read_bytes() == plain_gfa and (d / "w.vcf").read_bytes() == plain_vcf
    said = capsys.readouterr().out
    assert said.split("; variants in:")[0] == said_plain.split("; variants in:")[0]
    assert said.rstrip("\n").endswith("; indels in: %s (31 matches tested, 3 deletions, 4 insertions, 1 insertions dropped)" % (d / "i.vcf"))
    body = [line.split("\t") for line in (d / "i.vcf").read_text().splitlines() if not line.startswith("#")]
    assert [(r[0], r[1]) for r in body] == [("s", "1"), ("s", "1"), ("u", "1"), ("u", "3")] and set(r[6] for r in body) == {"."}


def test_indels_alone_run_the_pileup_pass_too(faked):
    d, argv, fed = faked
    assert node_depth.main(argv + ["--indels", str(d / "i.vcf.gz"), "--min-alt-strand-count", "1"]) == 0
    assert _Fake.made == [("_FakeDepth", {}), ("_FakePileup", {"max_mismatch": 8}), ("_FakeIndels", {"max_len": 16})] and len(fed) == 1
    lines = gzip.decompress((d / "i.vcf.gz").read_bytes()).decode().splitlines()
    assert [line for line in lines if line.startswith("##FILTER")]
    assert [line.split("\t")[6] for line in lines if not line.startswith("#")] == ["PASS", "strand", "PASS", "PASS", "strand", "PASS"]
    assert not (d / "p.tsv").exists() and sorted(p.name for p in d.iterdir()) == ["i.vcf.gz", "in.gfa", "out.gfa", "x.fq"]
