"""The writers and the refusals of ``vstrains_amd.node_depth --pileup / --variants`` and ``cli --depth-pileup`` from constructed
``(offsets, depth, alt)`` arrays: no device.  What the table and the records must hold is tests/pileup_model.py's."""
import gzip

import numpy as np
import pytest

import pileup_model as model
from vstrains_amd import cli, node_depth
from vstrains_amd import pe as host

# K = 4: segment s (7 bases) and u (4 bases, exactly K) have rows, t (3 bases) has none
IDS = ["s", "t", "u"]
SEQS = ["ACGTACG", "GGA", "TTAC"]
OFFSETS = np.array([0, 7, 7, 11])
DEPTH = np.array([0, 200, 200, 200, 3, 1000, 7, 5, 5, 0, 6])
ALT = np.array([[0, 0, 0, 0, 0],
                [2, 0, 1, 0, 3],    # C: A 2 of DP 197: 2 >= 2 and 2 >= 1.97 -> a record; G 1: below the count
                [2, 0, 0, 0, 0],    # G: A 2 of DP 200: 2 >= 2.0, the fraction at equality -> a record
                [1, 1, 1, 0, 0],    # T: three bases with 1 each: none reaches the count of 2
                [0, 3, 0, 0, 0],    # A: C 3 of DP 3 -> AF 1.000000
                [9, 0, 10, 11, 0],  # C of DP 1000: A 9 < 10.0, G 10 == 10.0 -> a record, T 11 -> a record (ACGT order)
                [0, 0, 0, 2, 4],    # G: T 2 of DP 3 (`other` 4 is not part of DP) -> AF 0.666667
                [0, 0, 0, 0, 0],
                [5, 0, 0, 0, 0],    # T: A 5 of DP 5: the reference base's own count is 0
                [0, 0, 0, 0, 0],
                [0, 0, 0, 0, 6]])   # C: only `other`: DP 0, no record


def _rows():
    depth = [DEPTH[OFFSETS[n]:OFFSETS[n + 1]].tolist() for n in range(3)]
    alt = [ALT[OFFSETS[n]:OFFSETS[n + 1]].tolist() for n in range(3)]
    return model.table_rows(IDS, SEQS, depth, alt)


@pytest.mark.parametrize("name", ["p.tsv", "p.tsv.gz"])
def test_the_table_has_a_row_for_every_position_of_every_segment_of_K_bases(tmp_path, name):
    path = tmp_path / name
    node_depth.write_pileup(str(path), IDS, SEQS, OFFSETS, DEPTH, ALT)
    raw = path.read_bytes()
    assert (raw[:2] == b"\x1f\x8b") == name.endswith(".gz")
    lines = (gzip.decompress(raw) if name.endswith(".gz") else raw).decode().splitlines()
    assert lines[0] == "segment\tpos\tref\tA\tC\tG\tT\tother"
    got = [tuple(v if i in (0, 2) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]
    assert got == _rows() and len(got) == 11 and not [r for r in got if r[0] == "t"]
    assert got[0] == ("s", 1, "A", 0, 0, 0, 0, 0) and got[1] == ("s", 2, "C", 2, 194, 1, 0, 3) and got[8] == ("u", 2, "T", 5, 0, 0, 0, 0)


def test_the_records_hold_the_two_thresholds_at_equality():
    want = [("s", 2, "C", "A", 197, 2), ("s", 3, "G", "A", 200, 2), ("s", 5, "A", "C", 3, 3), ("s", 6, "C", "G", 1000, 10), ("s", 6, "C", "T", 1000, 11),
            ("s", 7, "G", "T", 3, 2), ("u", 2, "T", "A", 5, 5)]
    got = node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT)
    assert got == want == [r[:6] for r in model.variant_records(_rows())]
    # one above either threshold drops exactly the records that sat on it
    assert node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT, min_alt_count=3) == [r for r in want if r[5] >= 3]
    assert node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT, min_alt_frac=0.0101) == [r for r in want if r not in (want[1], want[3])]
    assert len(node_depth.variant_records(IDS, SEQS, OFFSETS, DEPTH, ALT, min_alt_count=0, min_alt_frac=0.0)) == 12  # (every base some read carries; never one that none does)


@pytest.mark.parametrize("name", ["v.vcf", "v.vcf.gz"])
def test_the_vcf_has_its_fixed_header_and_six_decimals(tmp_path, name):
    path = tmp_path / name
    node_depth.write_vcf(str(path), IDS, SEQS, OFFSETS, DEPTH, ALT)
    raw = path.read_bytes()
    lines = (gzip.decompress(raw) if name.endswith(".gz") else raw).decode().splitlines()
    head = [line for line in lines if line.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == "##source=vstrains_amd.node_depth"
    assert head[2:4] == ["##contig=<ID=s,length=7>", "##contig=<ID=u,length=4>"]  # (t is shorter than K: no rows, no contig line)
    assert [line.split(",")[0] for line in head[4:7]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=AF"]
    assert head[7] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and len(head) == 8
    body = lines[len(head):]
    assert body == ["%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d;AF=%s" % r for r in model.variant_records(_rows())]
    assert body[0] == "s\t2\t.\tC\tA\t.\t.\tDP=197;AD=2;AF=0.010152" and body[2].endswith("AF=1.000000") and body[5].endswith("DP=3;AD=2;AF=0.666667")


# ---- the refusals -------------------------------------------------------------------------------------------------------
def test_depth_pileup_without_depth_from_reads_is_refused_before_anything_is_written(tmp_path):
    gfa, paths, fq, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "r.fq", tmp_path / "out"
    gfa.write_bytes(b"S\ta\tACGT\tDP:f:1.0\n")
    paths.write_text("")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fq), "-rve", str(fq), "--depth-pileup"]
    with pytest.raises(ValueError, match="--depth-from-reads"):
        cli.main(argv)
    assert not out.exists()
    args = cli.build_parser().parse_args(argv + ["--depth-from-reads"])
    assert cli.depth_pileup_refusal(args) is None
    assert "--depth-pileup" not in cli.build_parser().format_help()


def test_more_than_one_rank_is_refused_with_the_pileup_flags(tmp_path, monkeypatch):
    gfa, out, pile, vcf = tmp_path / "in.gfa", tmp_path / "out.gfa", tmp_path / "p.tsv", tmp_path / "v.vcf"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process only"):
        node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq", "--pileup", str(pile), "--variants", str(vcf)])
    assert not out.exists() and not pile.exists() and not vcf.exists()


@pytest.mark.parametrize("flags, said", [(["--pileup", "p.tsv", "--pileup-max-mismatch", "-1"], "from 0 up"),
                                         (["--pileup-max-mismatch", "3"], "--pileup / --variants"),
                                         (["--min-alt-count", "3"], "--pileup / --variants"),
                                         (["--pileup", "p.tsv", "--min-alt-frac", "0.1"], "--variants"),
                                         (["--variants", "v.vcf", "--min-alt-frac", "1.5"], "between 0 and 1")])
def test_flags_that_cannot_hold_are_refused_before_a_device_is_opened(tmp_path, monkeypatch, capsys, flags, said):
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(host, "Context", None)  # (reaching it would fail the test: None is not callable)
    assert node_depth.main(["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", "x.fq", "-r", "y.fq"] + flags) == 1
    assert said in capsys.readouterr().err and not (tmp_path / "out.gfa").exists()


class _Fake:
    made = []

    def __init__(self, ctx, *a, **kw):
        type(self).made.append((type(self).__name__, kw))
        self.ends_seen = 4
        self.device, self.single_stats = "dev", None


class _FakeDepth(_Fake):
    def result(self):
        return np.array([10, 13, 2])


class _FakeCover(_Fake):
    def result(self):
        return np.array([0, 4, 4, 5]), np.array([1, 2, 3, 4, 2])

    def kc(self):
        return np.array([10, 13, 2])


class _FakePileup(_Fake):
    def result(self):
        return OFFSETS, DEPTH, ALT

    def tallies(self):
        return 12, 1


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
    monkeypatch.setattr(host, "CoverCounter", _FakeCover)
    monkeypatch.setattr(host, "PileupCounter", _FakePileup)
    monkeypatch.setattr(pe_inference, "_resolve_inputs", lambda *a, **kw: None)
    monkeypatch.setattr(pe_inference, "feed_counter", lambda ctx, counter, *a, **kw: fed.append(counter))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ts\tACGTACG\tDP:f:3.0\nS\tt\tGGA\nS\tu\tTTAC\nL\ts\t+\tt\t+\t3M\n")
    (tmp_path / "x.fq").write_text("@r\nACGTAC\n+\nIIIIII\n")
    return tmp_path, ["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", str(tmp_path / "x.fq"), "-r", str(tmp_path / "x.fq")], fed


def test_node_depth_without_the_new_flags_builds_no_pileup_counter(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv) == 0
    assert [m[0] for m in _Fake.made] == ["_FakeDepth"] and isinstance(fed[0], _FakeDepth)
    plain = (d / "out.gfa").read_bytes()
    said = capsys.readouterr().out
    assert said.rstrip().endswith("result stored in: %s" % (d / "out.gfa")) and "pileup" not in said and "variants" not in said
    _Fake.made.clear()
    assert node_depth.main(argv + ["--profile", str(d / "p.bg")]) == 0
    assert [m[0] for m in _Fake.made] == ["_FakeCover"] and (d / "out.gfa").read_bytes() == plain


def test_node_depth_with_either_flag_rides_the_pileup_on_the_depth_pass(faked, capsys):
    d, argv, fed = faked
    assert node_depth.main(argv) == 0
    plain, said_plain = (d / "out.gfa").read_bytes(), capsys.readouterr().out
    for flags, files in ((["--pileup", str(d / "p.tsv")], ["p.tsv"]), (["--variants", str(d / "v.vcf")], ["v.vcf"]),
                         (["--pileup", str(d / "q.tsv"), "--variants", str(d / "w.vcf"), "--profile", str(d / "p.bg")], ["q.tsv", "w.vcf", "p.bg"])):
        _Fake.made.clear()
        del fed[:]
        assert node_depth.main(argv + flags) == 0
        assert [m[0] for m in _Fake.made] == ["_FakeCover" if "--profile" in flags else "_FakeDepth", "_FakePileup"]
        assert _Fake.made[1][1] == {"max_mismatch": 8}
        both = fed[0]  # one read pass: both counters behind one add
        assert isinstance(both, node_depth._Both) and isinstance(both.extra, _FakePileup) and both.device == "dev"
        assert (d / "out.gfa").read_bytes() == plain and all((d / f).exists() for f in files)
        said = capsys.readouterr().out
        assert said.split("; result stored in:")[0] == said_plain.split("; result stored in:")[0]
    assert said.rstrip().endswith("result stored in: %s; profile in: %s; pileup in: %s; variants in: %s" % (d / "out.gfa", d / "p.bg", d / "q.tsv", d / "w.vcf"))
    assert (d / "p.tsv").read_text() == (d / "q.tsv").read_text() and (d / "v.vcf").read_text() == (d / "w.vcf").read_text()
    assert len((d / "p.tsv").read_text().splitlines()) == 12
    _Fake.made.clear()
    assert node_depth.main(argv + ["--variants", str(d / "v3.vcf"), "--pileup-max-mismatch", "0", "--min-alt-count", "3"]) == 0
    assert _Fake.made[1] == ("_FakePileup", {"max_mismatch": 0})
    assert len([line for line in (d / "v3.vcf").read_text().splitlines() if not line.startswith("#")]) == 4
