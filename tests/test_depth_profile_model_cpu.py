"""The depth profile without a device: the definition against its restatement by matches on every constructed case, the
named mistakes, the fold plan (``vs_cover_plan``, a pure host function of the library), the bedGraph and summary writers, the
median as a depth statistic, and the refusals."""
import gzip

import numpy as np
import pytest

import depth_profile_cases as cases
import depth_profile_model as model
import node_depth_model
from vstrains_amd import cli, node_depth
from vstrains_amd import pe as host


def all_cases(k):
    return cases.cover_cases(k) + [cases.scan_share_case(k, False), cases.scan_share_case(k, True)]


@pytest.fixture(scope="module", params=cases.KS)
def judged(request):
    """Every case of one k with its profile by the definition, computed once."""
    k = request.param
    return k, [(c, model.node_cover(c.seqs, k, c.ends)) for c in all_cases(k)]


def test_the_definition_equals_the_form_by_matches_in_either_slot_order(judged):
    k, rows = judged
    for c, truth in rows:
        assert model.node_cover_by_matches(c.seqs, k, c.ends) == truth, c.name
        assert model.node_cover_by_matches(c.seqs, k, c.ends, order=list(reversed(range(len(c.seqs))))) == truth, c.name
        assert [len(r) for r in truth] == [max(len(s) - k, 0) for s in c.seqs]
        if c.want is not None:
            assert {n: truth[n] for n in c.want} == c.want, c.name


def test_the_row_sums_are_the_depth_pass(judged):
    k, rows = judged
    for c, truth in rows:
        if len(c.seqs) <= 100:  # (the scan cases: 512 segments, nothing the others do not have)
            assert model.row_sums(truth) == node_depth_model.node_depth(c.seqs, k, c.ends), c.name


def test_every_named_mistake_is_told_from_the_truth(judged):
    k, rows = judged
    told = set()
    for c, truth in rows:
        for v in c.tells:
            assert model.node_cover_by_matches(c.seqs, k, c.ends, variant=v) != truth, (c.name, v)
            told.add(v)
    assert told == set(model.MATCH_VARIANTS)


def test_without_the_sentinel_all_first_windows_but_one_are_wrong_in_any_slot_order(judged):
    k, rows = judged
    for c, truth in rows:
        if "leak_past_end" not in c.tells:
            continue
        n = len(c.seqs)
        assert n == 12 and all(row[0] == 0 and row[-1] == 1 for row in truth)
        for order in (list(range(n)), list(reversed(range(n))), [(5 * i + 3) % n for i in range(n)]):
            bad = model.node_cover_by_matches(c.seqs, k, c.ends, variant="leak_past_end", order=order)
            wrong = [i for i in range(n) if bad[i][0] != 0]
            assert sorted(wrong) == sorted(set(range(n)) - {order[0]}), (c.name, order)  # (the first in slot order has nobody before it)


def test_slot_totals_of_the_scan_cases():
    for k in cases.KS:
        assert cases.slot_total(cases.scan_share_case(k, False).seqs, k) == cases.SCAN_SHARE
        assert cases.slot_total(cases.scan_share_case(k, True).seqs, k) == cases.SCAN_SHARE + 2


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_no_fold_below_the_bound_and_a_fold_at_it():
    K, max_len, n_ends = 56, 150, 1000
    weight = n_ends * 2 * (max_len - K + 1)
    p = host.cover_plan(100, 55, n_ends, max_len)
    assert p["launch"] and p["weight"] == weight == 190000 and not p["fold_first"] and p["pending"] == weight and p["threads"] == 1024
    assert (p["grid"] - 1) * p["ends_per_wg"] < n_ends <= p["grid"] * p["ends_per_wg"]
    # pending + weight one below the bound: no fold; at the bound: a fold first, and only this block pends
    for bound in (2 ** 32, 10 ** 6):
        below = host.cover_plan(100, 55, n_ends, max_len, pending=bound - weight - 1, bound=bound)
        assert not below["fold_first"] and below["pending"] == bound - 1
        at = host.cover_plan(100, 55, n_ends, max_len, pending=bound - weight, bound=bound)
        assert at["fold_first"] and at["pending"] == weight
    # nothing pends: nothing to fold, however low the bound
    assert not host.cover_plan(100, 55, n_ends, max_len, pending=0, bound=1)["fold_first"]
    assert host.cover_plan(100, 55, n_ends, max_len, pending=1, bound=1)["fold_first"]


def test_the_smallest_block_that_forces_a_fold():
    K, max_len, pending = 22, 101, 2 ** 32 - 16000
    per_end = 2 * (max_len - K + 1)
    assert per_end == 160
    assert not host.cover_plan(10, 21, 98, max_len, pending=pending)["fold_first"]  # (98 ends: 15 680; ends come in twos)
    assert host.cover_plan(10, 21, 100, max_len, pending=pending)["fold_first"]     # 100 ends: 16 000 reaches 2^32


def test_a_block_without_a_window_neither_launches_nor_weighs():
    for n_ends, max_len in ((0, 150), (1000, 55), (1000, 0)):
        p = host.cover_plan(100, 55, n_ends, max_len, pending=77)
        assert not p["launch"] and p["weight"] == 0 and not p["fold_first"] and p["pending"] == 77


def test_a_block_that_could_put_two_to_the_32_on_one_window_is_refused():
    from vstrains_amd import _native as nat

    span = 150 - 56 + 1
    most = (2 ** 32 - 1) // (2 * span)
    assert host.cover_plan(100, 55, most, 150)["weight"] < 2 ** 32
    for bad in (dict(n_ends=most + 1), dict(n_ends=2 ** 32), dict(n_ends=2 ** 31, max_len=2 ** 32 - 1, ksize=0),
                dict(n_nodes=2 ** 25 - 1), dict(bound=2 ** 32 + 1), dict(pending=2 ** 32)):
        kw = dict(n_nodes=100, ksize=55, n_ends=1000, max_len=150)
        kw.update(bad)
        with pytest.raises(nat.NativeError):
            host.cover_plan(**kw)


# ---- the writers -------------------------------------------------------------------------------------------------------
IDS = ["a", "short", "one", "b"]
LENGTHS = [13, 3, 6, 9]  # K = 6: 8 windows, none, one, 4
OFFSETS = np.array([0, 8, 8, 9, 13])
COV = np.array([0, 0, 3, 3, 3, 1, 0, 0, 7, 2, 2, 5, 4])


@pytest.mark.parametrize("name", ["p.bedgraph", "p.bedgraph.gz"])
def test_bedgraph_merges_runs_keeps_zeros_and_reads_back(tmp_path, name):
    path = str(tmp_path / name)
    node_depth.write_bedgraph(path, IDS, OFFSETS, COV)
    raw = open(path, "rb").read()
    text = (gzip.decompress(raw) if name.endswith(".gz") else raw).decode()
    assert (raw[:2] == b"\x1f\x8b") == name.endswith(".gz")
    assert text == ("a\t0\t2\t0\na\t2\t5\t3\na\t5\t6\t1\na\t6\t8\t0\n"
                    "one\t0\t1\t7\n"
                    "b\t0\t2\t2\nb\t2\t3\t5\nb\t3\t4\t4\n")
    offsets, cov = node_depth.read_bedgraph(path, IDS)
    assert offsets.tolist() == OFFSETS.tolist() and cov.tolist() == COV.tolist()


def test_summary_has_breadth_and_the_lower_median(tmp_path):
    path = str(tmp_path / "s.tsv")
    node_depth.write_summary(path, IDS, LENGTHS, OFFSETS, COV)
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == ["segment", "length", "windows", "KC", "breadth", "min", "median", "max"]
    assert [l.split("\t") for l in lines[1:]] == [["a", "13", "8", "10", "4", "0", "0", "3"],  # sorted 0 0 0 0 1 3 3 3: index 3
                                                  ["short", "3", "0", "0", "0", "0", "0", "0"],
                                                  ["one", "6", "1", "7", "1", "7", "7", "7"],
                                                  ["b", "9", "4", "13", "4", "2", "2", "5"]]     # sorted 2 2 4 5: index 1


def test_depth_stat_median_makes_kc_over_ln_the_median():
    gfa = b"S\ta\t" + b"A" * 13 + b"\tKC:i:1\nS\tshort\tACG\nS\tone\tACGTAC\nS\tb\t" + b"C" * 9 + b"\tDP:f:2.0\n"
    assert node_depth.depth_stat("sum", LENGTHS, OFFSETS, COV) == [10, 0, 7, 13]
    tags = node_depth.depth_stat("median", LENGTHS, OFFSETS, COV)
    assert tags == [0, 0, 42, 18]
    out = node_depth.rewrite_gfa(gfa, tags)
    assert out == b"S\ta\t" + b"A" * 13 + b"\tLN:i:13\tKC:i:0\nS\tshort\tACG\tLN:i:3\tKC:i:0\nS\tone\tACGTAC\tLN:i:6\tKC:i:42\nS\tb\t" + b"C" * 9 + b"\tLN:i:9\tKC:i:18\n"
    for line, median in zip(out.splitlines(), (0, 0, 7, 2)):
        cols = line.split(b"\t")
        assert int(cols[4][5:]) / int(cols[3][5:]) == median
    with pytest.raises(ValueError):
        node_depth.depth_stat("mean", LENGTHS, OFFSETS, COV)


# ---- the commands ------------------------------------------------------------------------------------------------------
def test_depth_profile_without_depth_from_reads_is_refused_before_anything_is_written(tmp_path):
    gfa, paths, fq, out = tmp_path / "g.gfa", tmp_path / "c.paths", tmp_path / "r.fq", tmp_path / "out"
    gfa.write_bytes(b"S\ta\tACGT\tDP:f:1.0\n")
    paths.write_text("")
    fq.write_text("@r\nACGT\n+\nIIII\n")
    argv = ["-a", "spades", "-g", str(gfa), "-p", str(paths), "-o", str(out), "-fwd", str(fq), "-rve", str(fq), "--depth-profile"]
    with pytest.raises(ValueError, match="--depth-from-reads"):
        cli.main(argv)
    assert not out.exists()
    args = cli.build_parser().parse_args(argv + ["--depth-from-reads"])
    assert cli.depth_profile_refusal(args) is None
    assert "--depth-profile" not in cli.build_parser().format_help()


def test_more_than_one_rank_is_refused_with_the_profile_flags(tmp_path, monkeypatch):
    gfa, out, prof = tmp_path / "in.gfa", tmp_path / "out.gfa", tmp_path / "p.bedgraph"
    gfa.write_bytes(b"S\ta\tACGTAC\nS\tb\tGTACGG\nL\ta\t+\tb\t+\t3M\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process only"):
        node_depth.main(["-g", str(gfa), "-o", str(out), "-f", "x.fq", "-r", "y.fq", "--profile", str(prof), "--depth-stat", "median"])
    assert not out.exists() and not prof.exists()


class _Fake:
    made = []

    def __init__(self, ctx, *a, **kw):
        type(self).made.append(type(self).__name__)
        self.ends_seen = 4


class _FakeDepth(_Fake):
    def result(self):
        return np.array([10, 13])


class _FakeCover(_Fake):
    def result(self):
        return np.array([0, 4, 8]), np.array([1, 2, 3, 4, 2, 2, 4, 5])

    def kc(self):
        return np.array([10, 13])


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
    """``node_depth.main`` with the device taken out: the context, the two counters and the input dispatch are stand-ins."""
    from vstrains_amd import pe_inference

    _Fake.made.clear()
    monkeypatch.setattr(host, "Context", _FakeCtx)
    monkeypatch.setattr(host, "DepthCounter", _FakeDepth)
    monkeypatch.setattr(host, "CoverCounter", _FakeCover)
    monkeypatch.setattr(pe_inference, "_resolve_inputs", lambda *a, **kw: None)
    monkeypatch.setattr(pe_inference, "feed_counter", lambda *a, **kw: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gfa = tmp_path / "in.gfa"
    gfa.write_bytes(b"S\ta\tACGTACG\tDP:f:3.0\nS\tb\tGTACGGA\nL\ta\t+\tb\t+\t3M\n")
    (tmp_path / "x.fq").write_text("@r\nACGTAC\n+\nIIIIII\n")
    return tmp_path, ["-g", str(gfa), "-o", str(tmp_path / "out.gfa"), "-f", str(tmp_path / "x.fq"), "-r", str(tmp_path / "x.fq")]


def test_node_depth_without_the_new_flags_builds_no_cover_counter(faked, capsys):
    d, argv = faked
    assert node_depth.main(argv) == 0
    assert _Fake.made == ["_FakeDepth"]
    plain = (d / "out.gfa").read_bytes()
    assert plain == b"S\ta\tACGTACG\tLN:i:7\tKC:i:10\nS\tb\tGTACGGA\tLN:i:7\tKC:i:13\nL\ta\t+\tb\t+\t3M\n"
    said = capsys.readouterr().out
    assert said.rstrip().endswith("result stored in: %s" % (d / "out.gfa")) and "profile" not in said


def test_node_depth_with_any_new_flag_counts_through_the_cover_counter(faked, capsys):
    d, argv = faked
    plain = b"S\ta\tACGTACG\tLN:i:7\tKC:i:10\nS\tb\tGTACGGA\tLN:i:7\tKC:i:13\nL\ta\t+\tb\t+\t3M\n"
    for flags in (["--profile", str(d / "p.bg")], ["--profile-summary", str(d / "s.tsv")], ["--depth-stat", "sum"]):
        _Fake.made.clear()
        assert node_depth.main(argv + flags) == 0
        assert _Fake.made == ["_FakeCover"]
        assert (d / "out.gfa").read_bytes() == plain  # (sum, the default: today's file)
    assert (d / "p.bg").read_text() == "a\t0\t1\t1\na\t1\t2\t2\na\t2\t3\t3\na\t3\t4\t4\nb\t0\t2\t2\nb\t2\t3\t4\nb\t3\t4\t5\n"
    assert (d / "s.tsv").read_text().splitlines()[1:] == ["a\t7\t4\t10\t4\t1\t2\t4", "b\t7\t4\t13\t4\t2\t2\t5"]
    capsys.readouterr()
    assert node_depth.main(argv + ["--depth-stat", "median", "--profile", str(d / "p.bg")]) == 0
    assert (d / "out.gfa").read_bytes() == plain.replace(b"KC:i:10", b"KC:i:14").replace(b"KC:i:13", b"KC:i:14")
    assert capsys.readouterr().out.rstrip().endswith("result stored in: %s; profile in: %s" % (d / "out.gfa", d / "p.bg"))
