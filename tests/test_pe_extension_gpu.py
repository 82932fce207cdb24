"""The extension and acceptance stage of k_pe_tiles (vs_agree_fast, vs_agree_long, vs_extend, vs_seed_limits, vs_accept /
vs_accept32 in vstrains_amd/csrc/vs_pe.hip) on matches cut at every length: the blocks of tests/pe_extension_cases.py, whose
accepted counts sit on the threshold, so that an extension one base long or short flips an end's list.  Per shape the
counters and every end's list equal the C oracle's, under the kernel the shape was chosen for and under every switch
that sends the same block through another one.  Integers, compared for equality.  What the blocks cover -- every left
extension, every window edge +-1 -- is asserted without a device by tests/test_pe_extension_cases_cpu.py."""
import functools
import random

import numpy as np
import pytest

import pe_extension_cases as pec
from oracle import pe_oracle_c

pytestmark = pytest.mark.gpu

SHAPES = list(pec.SHAPES)
STD = [sh for sh in SHAPES if not pec.SHAPES[sh]["kernel"].endswith("0u, 0u")]  # the compile-time shapes


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def xctx(host):
    """A context in experiment mode: the tuning switches of vs_pe_count are live on it (conftest.experiment_context)."""
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


def _reference(k, seqs, fwd, rve):
    orc = pe_oracle_c.Oracle(seqs, k)
    node_mat, short_mat, stats = orc.count_pairs(fwd, rve)
    lists = []
    for f, r in zip(fwd, rve):
        used = "N" not in f and "N" not in r  # (every end has k + 1 bases and more)
        lists += [orc.map_end(f) if used else [], orc.map_end(r) if used else []]
    return node_mat, short_mat, tuple(int(x) for x in stats), lists


@functools.lru_cache(maxsize=None)
def family(k, rlen):
    """The block of a shape and the oracle's answer to it: computed once, shared by the tests, never changed."""
    fam = pec.knife_edge_family(k, rlen, pec.SHAPES[(k, rlen)]["step"])
    ref = _reference(k, fam["seqs"], fam["fwd"], fam["rve"])
    cases, anchor, node_mat = fam["cases"], fam["anchor"], ref[0]
    n_counted = 0
    for p, c in enumerate(cases):  # the pairing reads the answer off node_mat: one cell per case
        cell = (anchor, c["node"]) if c["end"] else (c["node"], anchor)
        kept = c["node"] in ref[3][2 * p + c["end"]]
        assert int(node_mat[cell]) == int(kept)
        n_counted += kept
    assert 0.35 * len(cases) < n_counted < 0.65 * len(cases) and ref[2][0] > 0  # (accepted and rejected; pairs dropped for an N)
    return fam, ref


def _check(host, ctx, k, fam, ref, kernel, adaptive=None):
    seqs, fwd, rve = fam["seqs"], fam["fwd"], fam["rve"]
    ctx.build_index(seqs, k, renumber=False)  # (the text behind a node is the next node of ``seqs``)
    assert ctx.node_order is None
    counter = host.PeCounter(ctx)
    block = ctx.pack_pairs(fwd, rve)
    counter.add(block)
    ran, slow_pairs, launched = ctx.last_kernel, ctx.last_timing()["slow_pairs"], ctx.last_launched
    node_mat, short_mat, stats = counter.result()
    assert ran.startswith(kernel), (ran, kernel)
    if adaptive is not None:
        assert ran.endswith(", true>") == adaptive, ran
    assert np.array_equal(node_mat, ref[0]), np.argwhere(node_mat != ref[0])[:8].tolist()
    assert np.array_equal(short_mat, ref[1]), np.argwhere(short_mat != ref[1])[:8].tolist()
    assert stats == ref[2]
    lists = ctx.map_ends(block, cap=8)
    wrong = [(e // 2, lists[e], ref[3][e]) for e in range(len(lists)) if lists[e] != ref[3][e]]
    assert not wrong, (len(wrong), [(fam["cases"][p % len(fam["cases"])], got, want) for p, got, want in wrong[:4]])
    return slow_pairs, launched


def _overflow_pairs(fam):
    """Counted pairs with an end of more than four bytes outside ACGT: more than the position list of the straight-line
    kernels holds, so those hand the pair to k_pe_mid / k_pe_slow (the generic loops read the validity mask instead)."""
    return sum(1 for p, c in enumerate(fam["cases"]) if c["extra"] and "N" not in fam["fwd"][p] + fam["rve"][p])


@pytest.mark.parametrize("k,rlen", SHAPES)
def test_threshold_matches_under_the_planned_kernel(host, ctx, k, rlen):
    """A production context: the instantiation the shape was chosen for runs, and the ends with more than four bytes outside
    ACGT pass through the overflow kernels (k_pe_mid)."""
    fam, ref = family(k, rlen)
    kernel = pec.SHAPES[(k, rlen)]["kernel"]
    slow, _ = _check(host, ctx, k, fam, ref, kernel, adaptive=False if (k, rlen) in STD else None)
    assert _overflow_pairs(fam) > 0 and slow >= (0 if kernel.startswith("k_pe_tiles<0") else _overflow_pairs(fam)), slow


@pytest.mark.parametrize("k,rlen", SHAPES)
def test_threshold_matches_under_every_switch(host, xctx, k, rlen, monkeypatch):
    """The same block through the other kernels: the generic loops with the validity mask (VS_NO_FAST=1: MODE 0), the
    run-time-shape straight-line kernel in place of a compile-time one (VS_NO_STD=1), the shortcut for overlapping seeds
    forced off and on, the adaptive step grid of the compile-time shapes forced off and on, and the overflow pairs sent
    straight to k_pe_slow (VS_NO_MID=1)."""
    fam, ref = family(k, rlen)
    planned = pec.SHAPES[(k, rlen)]["kernel"]
    generic = planned[:len("k_pe_tiles<1")] + ", 0u, 0u>"  # (the run-time shape of the same mode)
    std = (k, rlen) in STD
    runs = [({"VS_NO_FAST": "1"}, "k_pe_tiles<0, 0u, 0u>", None), ({"VS_SHORTCUT": "0"}, planned, None), ({"VS_SHORTCUT": "1"}, planned, None),
            ({"VS_NO_MID": "1"}, planned, None)]
    if std:
        runs += [({"VS_NO_STD": "1"}, generic, None), ({"VS_ADAPT_GRID": "0"}, planned, False), ({"VS_ADAPT_GRID": "1"}, planned, True)]
    for env, kernel, adaptive in runs:
        with monkeypatch.context() as m:
            for name, value in env.items():
                m.setenv(name, value)
            slow, _ = _check(host, xctx, k, fam, ref, kernel, adaptive)
            assert slow >= (0 if kernel.startswith("k_pe_tiles<0") else _overflow_pairs(fam)), (env, slow)


def test_repeated_threshold_block_through_the_locus_sort_and_runs_of_tiles(host, ctx, xctx, monkeypatch):
    """The k = 55 / 2 x 150 block twelve times over (9 096 pairs) in shuffled order: the locus sort reorders the pairs, and
    with one workgroup per CU (VS_GRID_PER_CU=1) a workgroup takes two tiles, the second one's words arriving while the
    first is worked on."""
    fam, _ = family(55, 150)
    order = [p for p in range(len(fam["cases"])) for _ in range(12)]
    random.Random(55150).shuffle(order)
    assert len(order) >= 4096
    big = dict(fam, fwd=[fam["fwd"][p] for p in order], rve=[fam["rve"][p] for p in order], cases=[fam["cases"][p] for p in order])
    ref = _reference(55, big["seqs"], big["fwd"], big["rve"])
    assert _check(host, ctx, 55, big, ref, "k_pe_tiles<1, 10u, 4u")[1] & ctx.RAN_LOCUS_LDS_SORT
    monkeypatch.setenv("VS_GRID_PER_CU", "1")
    assert _check(host, xctx, 55, big, ref, "k_pe_tiles<1, 10u, 4u")[1] & xctx.RAN_LOCUS_LDS_SORT
