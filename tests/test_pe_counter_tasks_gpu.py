"""k_pe_accumulate's tasks on the device (vstrains_amd/csrc/vs_pe.hip, K4; vs_acc_tasks.h): blocks of constructed end
lists whose pairs fill, overflow and barely start the task region of a wavefront, counted through Context.pe_count_lists
and compared exactly as tests/test_pe_counters_gpu.py compares -- prefilled counters, the block counted twice, every
cell of the plain statement (pe_counter_model.py), the totals of both matrices, the tile map.

A pair of an nl-list and an nr-list is nl + ceil(nl / 2) + ceil(nr / 2) tasks (no node rows when nr = 0): two 20-node
lists are 40, an 8-node and a 6-node list 15.  A wavefront takes 64 pairs a round and cuts them into batches of at most
960 task entries (VS_ACC_TASKS=40 on an experiment context: the smallest region, one large pair per batch)."""
import functools

import numpy as np
import pytest

import pe_counter_cases as cases
import test_pe_counters_gpu as base

pytestmark = pytest.mark.gpu

SHRUNK = {"VS_ACC_TASKS": "40"}


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
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


def _big(rng, n_nodes):
    return (cases._distinct(rng, n_nodes, 20), cases._distinct(rng, n_nodes, 20))


def _small(rng, n_nodes):  # fifteen tasks
    return (cases._distinct(rng, n_nodes, 8), cases._distinct(rng, n_nodes, 6))


# ---- (a) 64 pairs of 20-node lists: 2 560 tasks, three batches of the one wavefront, the longest tasks ---------------------------
@functools.lru_cache(maxsize=None)
def all_long(n_nodes: int = 300, seed: int = 1201):
    rng = np.random.default_rng(seed)
    return n_nodes, [_big(rng, n_nodes) for _ in range(64)]


@pytest.mark.parametrize("mode,extra", [("production", None), ("table", None), ("table", SHRUNK), ("noagg", None)], ids=["production", "table", "shrunk", "noagg"])
def test_64_pairs_of_20_node_lists(monkeypatch, ctx, xctx, mode, extra):
    base._count_and_compare(monkeypatch, ctx, xctx, all_long(), "tasks_long", mode, extra=extra)


# ---- (b) batches that end at 1, 63, 64 and 65 pairs -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_ends(at: int, n_nodes: int = 400, seed: int = 1202):
    """Two rounds of the first wavefront's kind.  63: 63 pairs of 15 tasks (945 of 960 entries) and a pair of 40 that does
    not fit behind them -- a batch of 63 pairs, then one of a single pair; 64: 64 pairs of 15 tasks, one batch that fills
    the region to its last entry and ends with the round; 65: one pair more, which is the second wavefront's only one;
    1: a single pair of 40 tasks per round in front of small ones (with the region of 40 entries a batch of its own),
    and, for the block as a whole, one pair."""
    rng = np.random.default_rng(seed + at)
    if at == 63:
        return n_nodes, ([_small(rng, n_nodes) for _ in range(63)] + [_big(rng, n_nodes)]) * 2
    if at == 64:
        return n_nodes, [_small(rng, n_nodes) for _ in range(128)]
    if at == 65:
        return n_nodes, [_small(rng, n_nodes) for _ in range(65)]
    return n_nodes, ([_big(rng, n_nodes)] + [_small(rng, n_nodes) for _ in range(63)]) * 2


@pytest.mark.parametrize("at", [1, 63, 64, 65])
def test_batches_that_end_at(monkeypatch, ctx, xctx, at):
    case = batch_ends(at)
    tasks = [len(l) + (len(l) + 1) // 2 + (len(r) + 1) // 2 for l, r in case[1][:64]]
    if at == 63:
        assert sum(tasks[:63]) <= 960 < sum(tasks)
    elif at != 1:
        assert sum(tasks) == 960
    base._count_and_compare(monkeypatch, ctx, xctx, case, "tasks_ends%d" % at, "production")
    if at == 1:
        assert tasks[0] == 40 and tasks[1] == 15
        base._count_and_compare(monkeypatch, ctx, xctx, case, "tasks_ends1", "table", extra=SHRUNK)
        base._count_and_compare(monkeypatch, ctx, xctx, (case[0], case[1][:1]), "tasks_one_pair", "production")


# ---- (c) one 20 x 20 pair among 1-node pairs: one long task in a window of short ones ---------------------------------------------
@functools.lru_cache(maxsize=None)
def one_long(n_nodes: int = 300, seed: int = 1203):
    rng = np.random.default_rng(seed)
    pairs = [([int(rng.integers(0, n_nodes))], [int(rng.integers(0, n_nodes))]) for _ in range(200)]
    pairs[30] = _big(rng, n_nodes)
    return n_nodes, pairs


@pytest.mark.parametrize("mode,extra", [("production", None), ("table", SHRUNK), ("noagg", None)], ids=["production", "shrunk", "noagg"])
def test_one_long_pair_among_single_nodes(monkeypatch, ctx, xctx, mode, extra):
    base._count_and_compare(monkeypatch, ctx, xctx, one_long(), "tasks_onelong", mode, extra=extra)


# ---- (d) pairs with one or both ends empty ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def empty_ends(n_nodes: int = 300, seed: int = 1204):
    rng = np.random.default_rng(seed)
    pairs = []
    for p in range(300):
        l = cases._distinct(rng, n_nodes, int(rng.integers(1, 21)))
        r = cases._distinct(rng, n_nodes, int(rng.integers(1, 21)))
        pairs.append([(l, []), ([], r), ([], []), (l, r), ([], []), (l[:1], []), ([], r[:2])][p % 7])
    return n_nodes, pairs


@pytest.mark.parametrize("mode", ["production", "noagg"])
def test_empty_ends(monkeypatch, ctx, xctx, mode):
    base._count_and_compare(monkeypatch, ctx, xctx, empty_ends(), "tasks_empty", mode)


# ---- (e) chunk and round edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", [1, 1023, 1024, 1025])
def test_block_sizes(monkeypatch, ctx, xctx, n_pairs):
    n_nodes, pairs = cases.every_length_pair()
    base._count_and_compare(monkeypatch, ctx, xctx, (n_nodes, pairs[:n_pairs]), "lengths%d" % n_pairs, "table")


# ---- (f) claims, lost cells and write-outs in the middle of a task ---------------------------------------------------------
@pytest.mark.parametrize("fill", ["1", "100"])
@pytest.mark.parametrize("name", ["table_pressure", "probes_exhausted"])
def test_table_cases_under_fill(monkeypatch, ctx, xctx, name, fill):
    case = getattr(cases, name)()
    getattr(cases, "assert_" + name)(case)
    base._count_and_compare(monkeypatch, ctx, xctx, case, {"table_pressure": "pressure", "probes_exhausted": "probes"}[name], "table", extra={"VS_ACC_FILL": fill})


# ---- (g) other tile regions: the 11-bit offsets of the packed hand-off are relative to the wavefront's first tile ----------
@pytest.mark.parametrize("ept", ["6", "128"])
def test_other_tile_sizes(monkeypatch, ctx, xctx, ept):
    base._count_and_compare(monkeypatch, ctx, xctx, cases.every_length_pair(), "lengths", "table", extra={"VS_EPT": ept})
    base._count_and_compare(monkeypatch, ctx, xctx, all_long(), "tasks_long", "table", extra={"VS_EPT": ept})
