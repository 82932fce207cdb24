"""The contig threader on the device: ``k_contig_mems`` through ``Context.contig_mems`` and ``vs_contig_chain`` on the cases
of tests/contig_thread_cases.py, at k = 21 and one set at k = 127, against tests/contig_thread_model.py -- the walks, the
windows per token and the ambiguous windows exactly; on the small cases the match records themselves too."""
import numpy as np
import pytest

import contig_thread_cases as cases
import contig_thread_model as model

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


def device_mems(ctx, case):
    ctx.build_index(case.seqs, case.k)
    ctx.keep_masks(True)
    try:
        block = ctx.pack_singles(case.contigs)
        try:
            return ctx.contig_mems(block)
        finally:
            block.free()
    finally:
        ctx.keep_masks(False)


def model_walks(case):
    table = model.window_table(case.seqs, case.k)
    got = [model.thread(case.seqs, case.k, c, table=table) for c in case.contigs]
    return [[[tuple(t) for t in part] for part in parts] for parts, _ in got], [a for _, a in got]


def check(host, ctx, case, records: bool = False):
    mems = device_mems(ctx, case)
    assert len({tuple(r) for r in mems.tolist()}) == len(mems)  # every match once
    if records:
        want = sorted(m for c, text in enumerate(case.contigs) for m in model.mems(case.seqs, case.k, text, c))
        assert sorted(tuple(r) for r in mems.tolist()) == want
    parts, ambiguous = host.contig_chain(mems, [len(s) for s in case.seqs], case.k, len(case.contigs))
    want_parts, want_ambiguous = model_walks(case)
    assert parts == want_parts and ambiguous == want_ambiguous
    if case.want is not None:
        ids = [str(i) for i in range(len(case.seqs))]
        assert [[",".join(t) for t in model.tokens(p, ids)] or None for p in parts] == case.want
    return mems


@pytest.mark.parametrize("case", [c for k in cases.KS for c in cases.small_cases(k)], ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_small_cases_equal_the_model(host, ctx, case):
    check(host, ctx, case, records=case.k == 21)  # (the record search over strings is quadratic: the short texts of k = 21 only)


@pytest.mark.parametrize("case", [c for k in cases.KS for c in cases.long_cases(k)], ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_contigs_of_more_probes_than_a_round_and_than_a_share(host, ctx, case):
    check(host, ctx, case)
    info = ctx.contig_mems_last()
    assert ctx.index_info["stride"] == cases.stride(case.k)
    floor = 64 if "round" in case.name else 2 * cases.SHARE
    # the first contig alone has that many probes, so it lies in more than one round / in three workgroups' shares
    assert (len(case.contigs[0]) - ctx.index_info["seed_len"] + 1) // cases.stride(case.k) > floor and info["probes"] > floor


@pytest.mark.parametrize("k", cases.KS)
def test_more_matches_than_the_first_capacity_run_the_pass_again(host, k):
    case = cases.past_first_capacity(k)
    fresh = host.Context(0)  # (the buffer only grows: a context that has threaded before may hold a larger one)
    try:
        mems = check(host, fresh, case)
        info = fresh.contig_mems_last()
        assert len(mems) == len(case.contigs) > cases.FIRST_CAPACITY
        assert info == dict(records=len(mems), launches=2, probes=info["probes"], capacity_before=0)
        # the same block again fits what the buffer has grown to: one launch
        again = check(host, fresh, case)
        assert sorted(map(tuple, again.tolist())) == sorted(map(tuple, mems.tolist()))
        info = fresh.contig_mems_last()
        assert info["launches"] == 1 and info["capacity_before"] >= len(mems)
    finally:
        fresh.close()


def test_two_seeds_under_one_key_match_on_compared_text_only(host, ctx):
    case = cases.colliding_seed_case()
    mems = check(host, ctx, case)
    # every contig but the orphans is one match over all of its length
    assert sorted((int(c), int(n)) for c, _, _, _, n in mems) == sorted((c, len(t)) for c, t in enumerate(case.contigs) if case.want[c])


def test_a_block_of_pairs_names_its_ends_and_an_empty_block_gives_nothing(host, ctx):
    case = cases.small_cases(21)[0]
    ctx.build_index(case.seqs, 21)
    seg = case.seqs[0]
    block = ctx.pack(*host.encode_seqs([seg[:30], seg[2:40], "ACGT", model.revcomp(seg[1:30])]))
    try:
        got = sorted(map(tuple, ctx.contig_mems(block).tolist()))
    finally:
        block.free()
    assert got == [(0, 0, 0, 0, 30), (1, 0, 0, 2, 38), (3, 0, 1 << 31, len(seg) - 30, 29)]
    block = ctx.pack_singles(["ACGT", ""])
    try:
        assert ctx.contig_mems(block).shape == (0, 5) and ctx.contig_mems_last()["launches"] == 0
    finally:
        block.free()
