"""The device caller (``k_pileup_call_count``, the exclusive scan, ``k_pileup_call_write``) through ``StrandPileupCounter.call``
and ``PileupCounter.call``: on the constructed blocks of tests/strand_pileup_cases.py, on hand-written tables put straight into a
counter's device arrays, and through the two commands (``vstrains_amd.node_depth --strands``, ``cli --depth-strands``).  Every
comparison is of exact integers against tests/strand_pileup_model.py."""
import ctypes as C
import re

import numpy as np
import pytest

import pileup_model
import strand_pileup_cases as cases
import strand_pileup_model as model
from oracle import pe_oracle
from test_node_depth_gpu import CLI_PAIRS, SYNTH, _cli, _fastq, _files, _node_depth
from test_pileup_gpu import planted_reads

pytestmark = pytest.mark.gpu
ACGT = "ACGT"


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


def _records(ids, called, S=0):
    from vstrains_amd import node_depth

    return node_depth.strand_records(ids, called, S)


def _model_records(ids, seqs, depth, alt, C_, F, S):
    """tests/strand_pileup_model.py's records in the shape of ``node_depth.strand_records``."""
    return [r[:6] + r[7:] for r in model.variant_records(ids, seqs, depth, alt, C_, F, S)]


# ---- on the constructed blocks ------------------------------------------------------------------------------------------
PICKED = [c for k in cases.KS for c in cases.strand_cases(k)
          if c.name in ("reverse_complemented_read_first_with_one_mismatch_each", "overlap_flush_with_the_end_of_every_segment_on_each_strand",
                        "a_segment_shorter_than_K_between_two_long_ones", "a_block_of_65_ends", "rejected_on_one_strand_beside_credited_on_the_other")]


@pytest.mark.parametrize("case", PICKED, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_the_records_of_a_constructed_block_are_the_models(host, ctx, case):
    from vstrains_amd import node_depth

    ids = ["s%d" % n for n in range(len(case.seqs))]
    depth, alt, _ = model.strand_pileup(case.seqs, case.k, case.ends, case.M)
    ctx.build_index(case.seqs, case.k)
    counter = host.StrandPileupCounter(ctx, max_mismatch=case.M)
    plain = host.PileupCounter(ctx, max_mismatch=case.M)
    block = ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))
    try:
        counter.add(block)
        plain.add(block)
        for C_, F, S in ((1, 0.01, 0), (1, 0.01, 1), (2, 0.3, 2), (0, 0.0, 0)):
            want = _model_records(ids, case.seqs, depth, alt, C_, F, S)
            called = counter.call(C_, F, S)
            assert _records(ids, called, S) == want and (len(want) > 0 or C_ == 2)
            assert [a.dtype for a in called] == [np.int64] * 6 + [np.bool_] and called[5].shape == (len(want), 4)
            # one plane, the same kernels: today's Python on the unstranded tables
            one = _records(ids, plain.call(C_, F))
            assert [r[:6] for r in one] == node_depth.variant_records(ids, case.seqs, *plain.result(), C_, F) == [r[:6] for r in want]
            assert all(r[6][1] == r[6][3] == 0 and r[7] == "." for r in one)
        assert counter.folds == plain.folds == 1 and counter.pending == 0  # (call folds what pends, once)
    finally:
        block.free()
        ctx.keep_masks(False)


# ---- hand-written tables, put straight into the counters' device arrays ------------------------------------------------------
K_HAND = 21
HAND_LENGTHS = (300, 40, 10, 100)  # 301 + 41 + 0 + 101 = 443 slots: more than one workgroup of the caller (256 lanes)


class Hand:
    """An index over four random segments and, by slot, the tables a test writes into a counter: ``put`` sets one position."""

    def __init__(self, host, ctx):
        import torch

        self.torch = torch
        rng = np.random.default_rng(77)
        self.seqs = ["".join(ACGT[i] for i in rng.integers(0, 4, size=n)) for n in HAND_LENGTHS]
        self.ids = ["h%d" % n for n in range(len(self.seqs))]
        ctx.build_index(self.seqs, K_HAND)
        self.counter = host.StrandPileupCounter(ctx)
        self.plain = host.PileupCounter(ctx)
        ctx.keep_masks(False)
        self.S = self.counter.slots
        first = self.counter.first.cpu().numpy().view(np.uint32).astype(np.int64)
        rank = self.counter.node_rank if self.counter.node_rank is not None else np.arange(len(self.seqs))
        self.where = {}      # slot -> (segment in the GFA's order, position)
        self.sentinels = []
        for n, seq in enumerate(self.seqs):
            r = int(rank[n])
            if first[r + 1] > first[r]:
                assert first[r + 1] - first[r] == len(seq) + 1
                self.where.update((int(first[r]) + p, (n, p)) for p in range(len(seq)))
                self.sentinels.append(int(first[r]) + len(seq))
        self.depth = np.zeros((2, self.S), dtype=np.int64)
        self.alt = np.zeros((self.S, 2, 5), dtype=np.int64)

    def ref(self, slot):
        n, p = self.where[slot]
        return self.seqs[n][p]

    def put(self, slot, others, agree=(0, 0)):
        """``others``: per plane the counts of the three bases that are not the segment's, in ACGT order, then `other`."""
        r = ACGT.index(self.ref(slot))
        for t in (0, 1):
            row = list(others[t][:3])
            row.insert(r, 0)
            self.alt[slot, t] = row + [others[t][3]]
            self.depth[t, slot] = sum(others[t]) + agree[t]

    def upload(self, garbage=False):
        if garbage:
            self.depth[:, self.sentinels] = 2 ** 40 + 7
            self.alt[self.sentinels] = 12345
        dev = self.counter.device
        self.counter.depth.copy_(self.torch.from_numpy(self.depth).to(dev))
        self.counter.alt.copy_(self.torch.from_numpy(self.alt).to(dev))
        self.plain.depth.copy_(self.torch.from_numpy(self.depth[0]).to(dev))
        self.plain.alt.copy_(self.torch.from_numpy(np.ascontiguousarray(self.alt[:, 0])).to(dev))

    def want(self, C_, F, S, planes=2):
        """The model's records of the tables, slot by slot, in the GFA's order."""
        out = []
        for slot, (n, p) in sorted(self.where.items(), key=lambda kv: kv[1]):
            depth, alt = self.depth[:planes, slot].tolist(), self.alt[slot, :planes].tolist()
            for base, dp, ad, dp4, fail in model.position_records(self.seqs[n][p], depth, alt, C_, F, S):
                out.append((self.ids[n], p + 1, self.seqs[n][p], base, dp, ad, dp4, "." if S < 1 else ("strand" if fail else "PASS")))
        return out


@pytest.fixture
def hand(host, ctx):
    return Hand(host, ctx)


def test_empty_tables_have_no_records(hand):
    hand.upload()
    called = hand.counter.call(0, 0.0, 0)
    assert [len(a) for a in called] == [0] * 7 and called[5].shape == (0, 4)
    assert [len(a) for a in hand.plain.call(0, 0.0)] == [0] * 7


def test_records_at_the_wavefront_and_workgroup_edges_and_at_the_last_position(hand):
    S = hand.S
    assert S == 443 and sorted(hand.sentinels)[-1] == S - 1 and S - 2 in hand.where and 0 in hand.where
    edge = [0, 63, 64, 255, 256, S - 2]
    assert all(s in hand.where for s in edge)
    for i, slot in enumerate(edge):
        hand.put(slot, [[2 + i, 0, 0, 0], [1, 0, 0, 1]], agree=(10, 20))
    three = 128
    hand.put(three, [[3, 1, 2, 0], [0, 4, 2, 5]], agree=(7, 0))  # three records in one slot
    hand.upload(garbage=True)  # (a sentinel's counts are never read: they hold no position)
    for C_, F, S_ in ((2, 0.01, 0), (2, 0.01, 1), (2, 0.01, 2), (0, 0.0, 0), (4, 0.2, 3)):
        want = hand.want(C_, F, S_)
        assert _records(hand.ids, hand.counter.call(C_, F, S_), S_) == want
        assert len(want) == {(2, 0): 9, (2, 1): 9, (2, 2): 9, (0, 0): 9, (4, 3): 3}[(C_, S_)]
    got = _records(hand.ids, hand.counter.call(2, 0.01, 2), 2)
    at = hand.where[three]
    assert [(r[3], r[6], r[7]) for r in got if (hand.ids.index(r[0]), r[1] - 1) == at] == \
        [(b, (7, 0, f, r), flt) for b, (f, r), flt in zip([c for c in ACGT if c != hand.ref(three)], ((3, 0), (1, 4), (2, 2)), ("strand", "strand", "PASS"))]
    last = hand.where[S - 2]
    assert last[1] == len(hand.seqs[last[0]]) - 1 and [r for r in got if (hand.ids.index(r[0]), r[1] - 1) == last][0][4:7] == (38, 8, (10, 20, 7, 1))
    # one plane: plane 0 of the same tables through PileupCounter.call, against today's Python on the counter's own result
    from vstrains_amd import node_depth

    one = _records(hand.ids, hand.plain.call(2, 0.01))
    assert one == hand.want(2, 0.01, 0, planes=1) and len(one) == 8
    assert [r[:6] for r in one] == node_depth.variant_records(hand.ids, hand.seqs, *hand.plain.result(), 2, 0.01)


def test_the_fraction_is_the_double_product_python_forms(hand):
    a, b, c = 10, 200, 400
    hand.put(a, [[4, 0, 0, 0], [3, 0, 0, 0]], agree=(60, 33))    # DP 100, AD 7
    hand.put(b, [[20, 0, 0, 0], [9, 0, 0, 0]], agree=(40, 31))   # DP 100, AD 29
    hand.put(c, [[1, 0, 0, 0], [1, 0, 0, 0]], agree=(3, 3))      # DP 8, AD 2
    hand.upload()
    sites = lambda F: sorted((hand.ids.index(r[0]), r[1] - 1) for r in _records(hand.ids, hand.counter.call(1, F, 0)))  # noqa: E731
    assert sites(0.07) == sorted([hand.where[b], hand.where[c]])      # 0.07 * 100 = 7.000000000000001 > 7
    assert sites(0.29) == sorted([hand.where[b]])                     # 0.29 * 100 = 28.999999999999996 <= 29
    assert sites(0.25) == sorted([hand.where[b], hand.where[c]])      # 0.25 * 8 = 2.0, exactly
    assert sites(0.06) == sorted([hand.where[a], hand.where[b], hand.where[c]])
    for F in (0.07, 0.29, 0.25):
        assert _records(hand.ids, hand.counter.call(1, F, 0)) == hand.want(1, F, 0)


def test_a_buffer_one_record_short_gets_the_count_and_nothing_else(hand, ctx):
    import torch

    for slot in (5, 63, 64, 310):
        hand.put(slot, [[2, 3, 0, 0], [2, 0, 0, 0]], agree=(9, 9))
    hand.upload()
    cnt = hand.counter
    args = (cnt.first.data_ptr(), cnt.slots, 2, cnt.depth.data_ptr(), cnt.alt.data_ptr(), 2, 0.01, 0)
    n = ctx.pileup_call(*args)
    assert n == 8
    out = torch.full((n + 1, 6), -1, dtype=torch.int64, device=cnt.device)
    assert ctx.pileup_call(*args, out_ptr=out.data_ptr(), cap=n - 1) == n and bool((out == -1).all())
    assert ctx.pileup_call(*args, out_ptr=out.data_ptr(), cap=n) == n
    got = out.cpu().numpy()
    assert (got[n] == -1).all() and (got[:n, 0] >> 5).tolist() == [5, 5, 63, 63, 64, 64, 310, 310]  # ascending by slot, then alt base
    assert all(got[i, 0] & 3 < got[i + 1, 0] & 3 for i in range(0, n, 2)) and (got[:n, 1] == 25).all()


def test_what_the_device_caller_refuses(hand, ctx, host):
    from vstrains_amd import _native as nat

    cnt = hand.counter
    ok = (cnt.first.data_ptr(), cnt.slots, 2, cnt.depth.data_ptr(), cnt.alt.data_ptr(), 2, 0.01, 0)
    for bad in (ok[:2] + (3,) + ok[3:], ok[:2] + (0,) + ok[3:], ok[:6] + (float("nan"), 0), ok[:6] + (-0.1, 0), ok[:2] + (1,) + ok[3:7] + (1,)):
        with pytest.raises(nat.NativeError) as ei:
            ctx.pileup_call(*bad)
        assert ei.value.code == nat.VS_E_ARG
    n = C.c_uint64(9)
    assert nat.lib().vs_pileup_call(ctx._h, None, cnt.slots, 2, C.c_void_p(cnt.depth.data_ptr()), C.c_void_p(cnt.alt.data_ptr()), 2, 0.01, 0, None, 0,
                                    C.byref(n)) == nat.VS_E_ARG
    with pytest.raises(nat.NativeError):
        hand.plain.ctx.pileup_call(hand.plain.first.data_ptr(), hand.plain.slots, 1, hand.plain.depth.data_ptr(), hand.plain.alt.data_ptr(), 2, 0.01, 1)


# ---- the commands -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    from vstrains_amd import node_depth, synth

    c = synth.make_pipeline_case(n_pairs=CLI_PAIRS, **SYNTH)
    d = tmp_path_factory.mktemp("strand_pileup_synth")
    raw = c.gfa_text.encode()
    (d / "graph.gfa").write_bytes(raw)
    (d / "stripped.gfa").write_bytes(node_depth.strip_depth_tags(raw))
    (d / "contigs.paths").write_text(c.paths_text)
    ids, seqs = pe_oracle.read_gfa_segments(str(d / "graph.gfa"))
    fwd, rve, seen = planted_reads(seqs, c.fwd, c.rve)
    assert seen >= 8
    (d / "fwd.fq").write_bytes(_fastq(fwd, "1"))
    (d / "rve.fq").write_bytes(_fastq(rve, "2"))
    ends = [e for pair in zip(fwd, rve) for e in pair]
    depth, alt, tally = model.strand_pileup(seqs, 55, ends, 8)
    return d, ids, seqs, depth, alt


def _table(path, columns):
    import gzip

    with (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)) as fh:
        lines = fh.read().splitlines()
    assert lines[0].split("\t") == list(columns)
    return [tuple(v if i in (0, 2) else int(v) for i, v in enumerate(line.split("\t"))) for line in lines[1:]]


def _vcf(path):
    head, out = [], []
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            head.append(line)
            continue
        chrom, pos, _, ref, alt, qual, flt, info = line.split("\t")
        f = dict(kv.split("=") for kv in info.split(";"))
        assert qual == "."
        out.append((chrom, int(pos), ref, alt, int(f["DP"]), int(f["AD"]), f["AF"], tuple(int(v) for v in f["DP4"].split(",")), flt))
    return head, out


def _stripped(path):
    out = []
    for line in open(path).read().splitlines():
        if not line.startswith("#"):
            cols = re.sub(r";DP4=\d+,\d+,\d+,\d+$", "", line).split("\t")
            cols[6] = "."
            out.append("\t".join(cols))
    return out


def test_node_depth_with_strands_writes_the_models_files_and_leaves_the_unstranded_ones_as_they_are(synth_files):
    d, ids, seqs, depth, alt = synth_files
    base = [d / "graph.gfa", d / "plain.gfa", d / "fwd.fq", d / "rve.fq"]
    got = _node_depth(*base, ["--pileup", str(d / "p.tsv"), "--variants", str(d / "v.vcf"), "--profile", str(d / "c.bg")])
    assert got.returncode == 0, got.stderr[-3000:]
    base[1] = d / "strands.gfa"
    got = _node_depth(*base, ["--pileup", str(d / "ps.tsv.gz"), "--variants", str(d / "vs.vcf"), "--profile", str(d / "cs.bg"), "--strands",
                              "--min-alt-strand-count", "2"])
    assert got.returncode == 0, got.stderr[-3000:]
    assert got.stdout.rstrip().endswith("; profile in: %s; pileup in: %s; variants in: %s" % (d / "cs.bg", d / "ps.tsv.gz", d / "vs.vcf"))
    # the stranded files are the model's
    rows = model.table_rows(ids, seqs, depth, alt)
    assert _table(d / "ps.tsv.gz", model.PILEUP_COLUMNS) == rows and sum(r[7] + r[12] for r in rows) > 0
    head, records = _vcf(d / "vs.vcf")
    want = model.variant_records(ids, seqs, depth, alt, 2, 0.01, 2)
    assert records == want and len(want) > 0 and set(r[8] for r in want) <= {"PASS", "strand"}
    assert len([h for h in head if h.startswith("##INFO=<ID=DP4,Number=4,Type=Integer")]) == 1 and len([h for h in head if h.startswith("##FILTER=<ID=strand,")]) == 1
    # ... and, DP4 and FILTER dropped, the records of the same command without --strands, byte for byte; nothing else it writes changes
    plain = [line for line in open(d / "v.vcf").read().splitlines() if not line.startswith("#")]
    assert _stripped(d / "vs.vcf") == plain
    assert (d / "strands.gfa").read_bytes() == (d / "plain.gfa").read_bytes() and (d / "cs.bg").read_bytes() == (d / "c.bg").read_bytes()
    # the existing outputs without the flag: the unstranded model's
    p_rows = pileup_model.table_rows(ids, seqs, *model.plane_sum(depth, alt))
    assert _table(d / "p.tsv", ("segment", "pos", "ref", "A", "C", "G", "T", "other")) == p_rows
    assert plain == ["%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d;AF=%s" % r for r in pileup_model.variant_records(p_rows)]
    assert not [h for h in open(d / "v.vcf").read().splitlines() if "DP4" in h or "FILTER=" in h]


def test_cli_with_depth_strands_writes_the_two_files_in_their_stranded_form(synth_files):
    d, ids, seqs, depth, alt = synth_files
    got = _cli(d / "stripped.gfa", d / "contigs.paths", d / "fwd.fq", d / "rve.fq", d / "out_strands", ["--depth-from-reads", "--depth-pileup", "--depth-strands"])
    assert got.returncode == 0, got.stderr[-3000:]
    assert set(["gfa/graph_depth.gfa", "gfa/graph_depth.pileup.tsv", "gfa/graph_depth.vcf"]) <= set(_files(d / "out_strands"))
    assert _table(d / "out_strands" / "gfa" / "graph_depth.pileup.tsv", model.PILEUP_COLUMNS) == model.table_rows(ids, seqs, depth, alt)
    head, records = _vcf(d / "out_strands" / "gfa" / "graph_depth.vcf")
    assert records == model.variant_records(ids, seqs, depth, alt) and len(records) > 0 and not [h for h in head if h.startswith("##FILTER")]
    p_rows = pileup_model.table_rows(ids, seqs, *model.plane_sum(depth, alt))
    assert _stripped(d / "out_strands" / "gfa" / "graph_depth.vcf") == ["%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d;AF=%s" % r for r in pileup_model.variant_records(p_rows)]
