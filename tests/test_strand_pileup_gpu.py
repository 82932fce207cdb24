"""The stranded pileup on the device: ``k_node_pileup_strands`` and the fold of both planes through ``StrandPileupCounter`` on
the constructed blocks of tests/strand_pileup_cases.py at k = 21, 55 and 127, beside ``PileupCounter`` on the same block, and on
a golden PE case.  Every comparison is of exact integers against tests/strand_pileup_model.py."""
import os

import numpy as np
import pytest

import strand_pileup_cases as cases
import strand_pileup_model as model
from conftest import pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


def _pack(host, ctx, case):
    return ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))


def _rows(offsets, depth, alt):
    cut = [(int(offsets[n]), int(offsets[n + 1])) for n in range(len(offsets) - 1)]
    return [depth[a:b].tolist() for a, b in cut], [alt[a:b].tolist() for a, b in cut]


def device_strands(host, ctx, case, times: int = 1, fold_bound: int = 2 ** 32, M=None):
    """A constructed case through ``StrandPileupCounter`` and, on the same index and block, through ``PileupCounter``, the
    block added ``times`` times -> ((depth rows, alt rows, tallies, folds) of the stranded counter, (depth rows, alt rows,
    tallies) of the unstranded one)."""
    ctx.build_index(case.seqs, case.k)
    budget = case.M if M is None else M
    counter = host.StrandPileupCounter(ctx, max_mismatch=budget, fold_bound=fold_bound)
    plain = host.PileupCounter(ctx, max_mismatch=budget)
    block = _pack(host, ctx, case)
    try:
        for _ in range(times):
            counter.add(block)
            plain.add(block)
        offsets, depth, alt = counter.result()
        p_offsets, p_depth, p_alt = plain.result()
        ctx.sync()
        total = int(offsets[-1])
        assert offsets.dtype == depth.dtype == alt.dtype == np.int64 and len(offsets) == len(case.seqs) + 1
        assert depth.shape == (total, 2) and alt.shape == (total, 2, 5) and offsets.tolist() == p_offsets.tolist()
        assert counter.ends_seen == plain.ends_seen and counter.pending == 0
        return _rows(offsets, depth, alt) + (counter.tallies(), counter.folds), _rows(p_offsets, p_depth, p_alt) + (plain.tallies(),)
    finally:
        block.free()
        ctx.keep_masks(False)


ALL = [c for k in cases.KS for c in cases.strand_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model_and_sum_to_the_pileup(host, ctx, case):
    want_depth, want_alt, want_tally = model.strand_pileup(case.seqs, case.k, case.ends, case.M)
    (depth, alt, tally, folds), plain = device_strands(host, ctx, case)
    assert depth == want_depth
    assert alt == want_alt
    assert tally == want_tally and folds <= 1
    if case.tally is not None:
        assert tally == case.tally
    assert model.plane_sum(depth, alt) + (tally,) == plain  # (what PileupCounter counts on the same block)


def _named(k, name):
    return [c for c in cases.strand_cases(k) if c.name == name][0]


@pytest.mark.parametrize("k", cases.KS)
def test_the_same_block_added_twice_doubles_every_count(host, ctx, k):
    case = _named(k, "a_block_of_65_ends")
    d1, a1, t1 = model.strand_pileup(case.seqs, k, case.ends, case.M)
    (depth, alt, tally, _), _ = device_strands(host, ctx, case, times=2)
    assert sum(a[t][c] for a in a1[0] for t in (0, 1) for c in range(5)) >= 65 and min(sum(d[t] for d in d1[0]) for t in (0, 1)) > 0
    assert depth == [[[2 * v for v in d] for d in row] for row in d1]
    assert alt == [[[[2 * v for v in plane] for plane in a] for a in row] for row in a1]
    assert tally == (2 * t1[0], 2 * t1[1])


@pytest.mark.parametrize("k", cases.KS)
def test_a_fold_after_every_block_and_one_fold_at_the_end_give_the_same(host, ctx, k):
    both = [_named(k, "overlap_flush_with_the_end_of_every_segment_on_each_strand"), _named(k, "overlap_flush_with_the_start_of_every_segment_on_each_strand")]
    assert both[0].seqs == both[1].seqs and both[0].ends != both[1].ends
    seqs = both[0].seqs
    want = model.strand_pileup(seqs, k, both[0].ends + both[1].ends, 8)
    got = []
    for bound, folds in ((1, 2), (2 ** 32, 1)):
        ctx.build_index(seqs, k)
        counter = host.StrandPileupCounter(ctx, fold_bound=bound)
        blocks = [_pack(host, ctx, c) for c in both]
        try:
            plans = []
            for b in blocks:
                info = b.info
                plans.append(host.pileup_plan(len(seqs), k, info["ends"], info["max_len"], pending=counter.pending, bound=bound))
                counter.add(b)
            got.append(_rows(*counter.result()) + (counter.tallies(),))
            # what the plan predicts: a fold before every block that finds weight pending under this bound, and one before the result
            assert counter.folds == sum(p["fold_first"] for p in plans) + 1 == folds
        finally:
            for b in blocks:
                b.free()
            ctx.keep_masks(False)
    assert got[0] == got[1] == want


@pytest.mark.parametrize("k", cases.KS)
def test_a_budget_of_zero_gives_the_models_result(host, ctx, k):
    case = _named(k, "an_N_in_a_plane_1_read")
    want = model.strand_pileup(case.seqs, k, case.ends, 0)
    (depth, alt, tally, _), _ = device_strands(host, ctx, case, M=0)
    assert (depth, alt, tally) == want
    assert tally == (1, 1) and not any(any(a[0]) or any(a[1]) for row in alt for a in row)
    assert sum(d[0] for d in depth[0]) == k + 1 + 2 and not any(d[1] for row in depth for d in row)  # (the exact read of plane 0 alone)
    case = _named(k, "reverse_complemented_read_first_with_one_mismatch_each")
    (depth, alt, tally, _), _ = device_strands(host, ctx, case, M=0)
    assert tally == (0, 2) and (depth, alt, tally) == model.strand_pileup(case.seqs, k, case.ends, 0) and not any(any(d) for row in depth for d in row)


def test_a_golden_pe_case_equals_the_model(host, ctx):
    name, d, meta = [c for c in pe_cases() if c[0] == "bubbles_k21"][0]  # (300 pairs; the case tests/test_pileup_gpu.py uses)
    ids, seqs = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fwd, rve = pe_oracle.fastq_sequences(os.path.join(d, "fwd.fq")), pe_oracle.fastq_sequences(os.path.join(d, "rve.fq"))
    n = min(len(fwd), len(rve), 300)
    ends = [e for pair in zip(fwd[:n], rve[:n]) for e in pair]
    want = model.strand_pileup(seqs, meta["k"], ends, 8)
    (depth, alt, tally, _), plain = device_strands(host, ctx, cases.PileupCase(name, meta["k"], seqs, ends, "a golden case"))
    assert want[2][0] > n and (depth, alt, tally) == want
    assert min(sum(d[t] for row in depth for d in row) for t in (0, 1)) > 0 and model.plane_sum(depth, alt) + (tally,) == plain
