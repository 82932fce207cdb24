"""The probe k_pe_tiles begins a tile early (vstrains_amd/csrc/vs_pe.hip, the non-adaptive compile-time shapes: key, home slot
and the slot's load during tile t, finished from them in the P1 of tile t + 1) on the blocks of
tests/pe_preprobe_cases.py: seven kinds of tile in input order, so that with the locus sort off and one workgroup per CU a
workgroup's run of three or four tiles hands probes over between tiles of different kinds -- to ends of dropped pairs, of
dirty ones that take the plain probe, to empty slots and to chains that go on past the home slot.  Counters, totals and every
end's list equal the C oracle's; integers, compared for equality.  What the blocks hold is asserted without a device by
tests/test_pe_preprobe_cases_cpu.py."""
import functools

import numpy as np
import pytest

import pe_preprobe_cases as ppc
from oracle import pe_oracle_c

pytestmark = pytest.mark.gpu

SHAPES = list(ppc.SHAPES)
RUNS = {"VS_GRID_PER_CU": "1", "VS_NO_SORT": "1"}


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


@pytest.fixture(scope="module")
def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def oracle():
    return pe_oracle_c.Oracle(ppc.graph()["seqs"], ppc.KSIZE)


@functools.lru_cache(maxsize=None)
def family_lists(kernel):
    """The oracle's list of every end of the family (an end of a pair that is not mapped has none): computed once."""
    fam = ppc.family(kernel)
    out = []
    for f, r in zip(fam["fwd"], fam["rve"]):
        used = ppc.pair_used(f, r)
        out += [oracle().map_end(f) if used else [], oracle().map_end(r) if used else []]
    return out


@functools.lru_cache(maxsize=None)
def reference(kernel, n_pairs):
    """The block of ``n_pairs`` pairs and the oracle's answer to it: computed once, shared by the tests, never changed."""
    fwd, rve, idx = ppc.block(kernel, n_pairs)
    node_mat, short_mat, stats = oracle().count_pairs(fwd, rve)
    fl = family_lists(kernel)
    lists = [fl[2 * i + e] for i in idx for e in (0, 1)]
    assert node_mat.sum() > n_pairs // 2 and all(int(x) > 0 for x in stats)
    return fwd, rve, node_mat, short_mat, tuple(int(x) for x in stats), lists


def _check(host, c, kernel_name, n_pairs, want_kernel, lists=True):
    fwd, rve, node_mat, short_mat, stats, ref_lists = reference(kernel_name, n_pairs)
    c.build_index(ppc.graph()["seqs"], ppc.KSIZE, renumber=False)  # (the table the case builder planted its chain in)
    assert c.index_info["slots"] == ppc.graph()["model"]["slots"]
    counter = host.PeCounter(c)
    block = c.pack_pairs(fwd, rve)
    counter.add(block)
    ran, launched = c.last_kernel, c.last_launched
    got_node, got_short, got_stats = counter.result()
    assert ran == want_kernel, (ran, want_kernel)
    assert got_stats == stats
    assert np.array_equal(got_node, node_mat), np.argwhere(got_node != node_mat)[:8].tolist()
    assert np.array_equal(got_short, short_mat), np.argwhere(got_short != short_mat)[:8].tolist()
    if lists:
        got = c.map_ends(block, cap=len(ppc.graph()["seqs"]))
        wrong = [(e // 2, got[e], ref_lists[e]) for e in range(len(got)) if got[e] != ref_lists[e]]
        assert not wrong, (len(wrong), wrong[:4])
    return launched


@pytest.mark.parametrize("r", ppc.REMAINDERS)
@pytest.mark.parametrize("kernel", SHAPES)
def test_runs_of_tiles_of_different_kinds(host, xctx, n_cu, monkeypatch, kernel, r):
    """n_cu * 32 * 3 + r pairs in input order, one workgroup per CU: runs of three tiles (r = 0) or four, the last
    workgroup's run a single partial tile (r = 1, 31) or a full tile and a partial one (r = 33)."""
    n_pairs = ppc.block_pairs(n_cu, r)
    n_tiles, per_wg, wgs, last = ppc.runs_of_tiles(n_pairs, n_cu)
    assert per_wg >= ppc.RUN_TILES and wgs >= len(ppc.KINDS) and last == {0: 3, 1: 1, 31: 1, 33: 2}[r]
    for name, value in RUNS.items():
        monkeypatch.setenv(name, value)
    launched = _check(host, xctx, kernel, n_pairs, kernel)
    assert not launched & (xctx.RAN_LOCUS_LDS_SORT | xctx.RAN_LOCUS_GLOBAL_SORT)


@pytest.mark.parametrize("kernel", SHAPES)
def test_same_blocks_through_the_run_time_shape_kernel(host, xctx, n_cu, monkeypatch, kernel):
    """VS_NO_STD=1: the straight-line kernel with a run-time shape, which probes every tile the plain way."""
    for name, value in dict(RUNS, VS_NO_STD="1").items():
        monkeypatch.setenv(name, value)
    _check(host, xctx, kernel, ppc.block_pairs(n_cu, 33), "k_pe_tiles<1, 0u, 0u>", lists=False)


@pytest.mark.parametrize("kernel", SHAPES)
def test_production_context_and_runs_of_locus_sorted_tiles(host, ctx, xctx, n_cu, monkeypatch, kernel):
    """A production context (the locus sort on, 128 workgroups per CU: one tile per workgroup at this size, every probe
    the first tile's), and the sorted order in runs of four tiles (VS_GRID_PER_CU=1 alone)."""
    n_pairs = ppc.block_pairs(n_cu, 33)
    assert _check(host, ctx, kernel, n_pairs, kernel, lists=False) & ctx.RAN_LOCUS_LDS_SORT
    monkeypatch.setenv("VS_GRID_PER_CU", "1")
    assert _check(host, xctx, kernel, n_pairs, kernel, lists=False) & xctx.RAN_LOCUS_LDS_SORT
