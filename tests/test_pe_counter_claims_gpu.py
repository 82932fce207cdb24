"""k_pe_accumulate's claims on the device (vstrains_amd/csrc/vs_pe.hip, K4): a lane whose cell is not in the slot its key
hashes to appends the key to its wavefront's queue of 64 (the last words of the wavefront's task region); the wavefront
claims the queued keys' cells, one lane per key, when a turn's misses do not fit any more and at the end of its round.
Blocks of constructed end lists that reach every state of that -- a queue that overflows in the middle of a window, the
same key queued by many lanes and wavefronts before its cell exists, a queue that is not empty when the round or the
kernel's last, partial round ends, a write-out right behind a drain, the queue carried across the batch cut next to a
full task region, a drained key that finds no slot within eight probes -- counted through Context.pe_count_lists and
compared exactly as tests/test_pe_counters_gpu.py compares: prefilled counters, the block counted twice, every cell of the
plain statement (pe_counter_model.py), the totals of both matrices, the tile map; on a production context (the cell
table) and with VS_NO_AGG=1 (every increment a global atomic), the switches on an experiment context with the table."""
import functools

import numpy as np
import pytest

import pe_counter_cases as cases
import pe_counter_model as pcm
import test_pe_counters_gpu as base

pytestmark = pytest.mark.gpu

MODES = ["production", "noagg"]
QUEUE = 64                 # ACC_QUEUE of vs_pe_plan.h
TASK_MIN, PLAN_CAP, TASK_CAP = 40, 832, 960  # ACC_TASK_MIN, ACC_TASK_PLAN_CAP, ACC_TASK_CAP


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


def _tasks(nl, nr):
    return (nl if nr else 0) + (nl + 1) // 2 + (nr + 1) // 2


def _cells(pair):
    nl, nr = len(pair[0]), len(pair[1])
    return nl * nr + nl * (nl + 1) // 2 + nr * (nr + 1) // 2


# ---- (a) every lane misses every turn ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def disjoint_lists(n_nodes: int = 4096, seed: int = 1401):
    """64 pairs, one wavefront's round, of an 8-node and a 6-node list; no node is listed twice in the block, so every
    increment is the first touch of its cell: every turn queues a key from every lane that has a task."""
    rng = np.random.default_rng(seed)
    nodes = cases._distinct(rng, n_nodes, 64 * 14)
    return n_nodes, [(nodes[14 * p: 14 * p + 8], nodes[14 * p + 8: 14 * p + 14]) for p in range(64)]


@pytest.mark.parametrize("mode", MODES)
def test_every_lane_misses_every_turn(monkeypatch, ctx, xctx, mode):
    case = disjoint_lists()
    listed = [x for pair in case[1] for end in pair for x in end]
    assert len(set(listed)) == len(listed) == 64 * 14
    n_cells = sum(_cells(pair) for pair in case[1])
    # more first touches than a queue holds by two orders, fewer than the table has slots; two batches of the production cut
    assert 100 * QUEUE < n_cells < pcm.ACC_SLOTS and PLAN_CAP < sum(_tasks(8, 6) for _ in range(64)) <= 2 * PLAN_CAP
    base._count_and_compare(monkeypatch, ctx, xctx, case, "claims_disjoint", mode)


# ---- (b) no miss after the first turns: the same keys queued by many lanes and wavefronts ----------------------------------------
@functools.lru_cache(maxsize=None)
def copies_of_one_pair(n_pairs: int, n_nodes: int = 4096, seed: int = 1402):
    rng = np.random.default_rng(seed)
    pair = (cases._distinct(rng, n_nodes, 7), cases._distinct(rng, n_nodes, 5))
    return n_nodes, [pair] * n_pairs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_pairs", [64, 1024])
def test_copies_of_one_pair(monkeypatch, ctx, xctx, n_pairs, mode):
    case = copies_of_one_pair(n_pairs)
    assert len(set(map(str, case[1]))) == 1 and _cells(case[1][0]) <= 35 + 28 + 15 < 2 * QUEUE
    base._count_and_compare(monkeypatch, ctx, xctx, case, "claims_copies%d" % n_pairs, mode)


# ---- (c) a queue that is not empty at the end of a round, and of the kernel's last, partial round ----------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 1025])
def test_block_sizes(monkeypatch, ctx, xctx, n_pairs, mode):
    n_nodes, pairs = cases.every_length_pair()
    base._count_and_compare(monkeypatch, ctx, xctx, (n_nodes, pairs[:n_pairs]), "lengths%d" % n_pairs, mode)


@pytest.mark.parametrize("mode", MODES)
def test_one_cell_waits_at_the_end(monkeypatch, ctx, xctx, mode):
    """One pair of one-node lists: three keys queued, the whole of the block's work is the drain at the end of the round."""
    base._count_and_compare(monkeypatch, ctx, xctx, (100, [([7], [9])]), "claims_one_cell", mode)


# ---- (d) a write-out after every round, of cells the drain in front of it has claimed ----------------------------------------
@pytest.mark.parametrize("n_pairs", [65, 2049])
def test_write_out_after_every_round(monkeypatch, ctx, xctx, n_pairs):
    n_nodes, pairs = cases.every_length_pair()
    base._count_and_compare(monkeypatch, ctx, xctx, (n_nodes, pairs[:n_pairs]), "lengths%d" % n_pairs, "table", extra={"VS_ACC_FILL": "0"})


def test_write_out_after_every_round_of_first_touches(monkeypatch, ctx, xctx):
    base._count_and_compare(monkeypatch, ctx, xctx, disjoint_lists(), "claims_disjoint", "table", extra={"VS_ACC_FILL": "0"})


# ---- (e) the queue carried across the batch cut, next to a full task region ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_long(n_nodes: int = 4096, seed: int = 1403):
    """64 pairs of two 20-node lists: 2 560 tasks, the most a round can have -- batches of 20 pairs at the production cut
    (800 of its 832 entries), of one pair at the smallest."""
    rng = np.random.default_rng(seed)
    return n_nodes, [(cases._distinct(rng, n_nodes, 20), cases._distinct(rng, n_nodes, 20)) for _ in range(64)]


@pytest.mark.parametrize("tasks", [TASK_MIN, PLAN_CAP - 1, PLAN_CAP, PLAN_CAP + 1, TASK_CAP])
def test_task_region_sizes(monkeypatch, ctx, xctx, tasks):
    """(a region asked for beyond the production cut is cut to it: task entries never reach the queue's words)"""
    case = all_long()
    assert all(_tasks(len(l), len(r)) == TASK_MIN for l, r in case[1]) and 2 * (TASK_CAP - PLAN_CAP) == 4 * QUEUE
    base._count_and_compare(monkeypatch, ctx, xctx, case, "claims_long", "table", extra={"VS_ACC_TASKS": str(tasks)})


@pytest.mark.parametrize("mode", MODES)
def test_64_pairs_of_20_node_lists(monkeypatch, ctx, xctx, mode):
    base._count_and_compare(monkeypatch, ctx, xctx, all_long(), "claims_long", mode)


# ---- (f) a drained key that finds no slot within eight probes, while other keys wait --------------------------------------------
@functools.lru_cache(maxsize=None)
def lost_among_waiting(n_nodes: int = 1024, n_keys: int = 12, rounds: int = 3, seed: int = 1404):
    """Rounds of 64 single-node pairs: twelve node_mat cells whose keys share one home slot (pe_counter_cases.
    probes_exhausted's), each twice, among 40 pairs of other nodes.  A pair of one-node lists is three tasks of one
    turn, so the round's 192 keys pass through the queue in three drains, the colliding ones side by side with the rest."""
    rng = np.random.default_rng(seed)
    _, hot = cases.probes_exhausted(n_nodes, n_keys, 1, 0)
    pairs = []
    for _ in range(rounds):
        others = [([int(rng.integers(0, n_nodes))], [int(rng.integers(0, n_nodes))]) for _ in range(64 - 2 * n_keys)]
        block = hot + hot + others
        pairs += [block[i] for i in rng.permutation(64)]
    return n_nodes, pairs


@pytest.mark.parametrize("mode", MODES)
def test_lost_cells_among_waiting_keys(monkeypatch, ctx, xctx, mode):
    case = lost_among_waiting()
    n_nodes, pairs = case
    keys = sorted({int(pcm.acc_key(0, l[0], r[0], n_nodes)) for l, r in pairs[:64]})
    homes = pcm.cell_slot(np.array(keys), pcm.ACC_BITS)
    crowd = [k for k, h in zip(keys, homes.tolist()) if h == np.bincount(homes).argmax()]
    # twelve keys of one home slot: four of them at least find no place, whatever else the table holds
    assert len(crowd) >= 12 and sum(pcm.placed(crowd, pcm.ACC_BITS)) == pcm.CELL_PROBES
    assert all(len(l) == 1 and len(r) == 1 for l, r in pairs) and len(pairs) == 3 * 64
    base._count_and_compare(monkeypatch, ctx, xctx, case, "claims_lost", mode)
