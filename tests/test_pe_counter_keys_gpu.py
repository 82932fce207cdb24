"""k_pe_accumulate's cell keys on the device (vstrains_amd/csrc/vs_pe.hip, K4): the key of a turn is mat * N * N + x * N + y
with (x, y) ordered for short_mat, formed per lane from the task's x -- fixed for a node row, taken anew at the second
stretch of a folded short row -- and the partner y, whichever of the two is smaller; a turn at a position beyond the
task's partners counts nothing.  Blocks of constructed end lists at the corners of the key space, counted through
Context.pe_count_lists and compared exactly as tests/test_pe_counters_gpu.py compares -- prefilled counters, the block
counted twice, every cell of the plain statement (pe_counter_model.py), the totals of both matrices, the tile map -- on a
production context (the cell table) and with VS_NO_AGG=1 (every increment a global atomic)."""
import functools

import numpy as np
import pytest

import test_pe_counters_gpu as base

pytestmark = pytest.mark.gpu

MODES = ["production", "noagg"]


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


def _pool(n_nodes: int):
    """Twenty distinct nodes: 0, 1, N/2, N-2, N-1 first, then their nearest neighbours (an end lists a node once, so a
    list longer than five fills up from these)."""
    N = n_nodes
    corners = [0, 1, N // 2, N - 2, N - 1]
    near = [2, 3, 4, 5, N // 2 - 3, N // 2 - 2, N // 2 - 1, N // 2 + 1, N // 2 + 2, N // 2 + 3, N - 7, N - 6, N - 5, N - 4, N - 3]
    pool = corners + near
    assert len(set(pool)) == 20 and min(pool) == 0 and max(pool) == N - 1
    return pool


def _tasks(nl, nr):
    return (nl if nr else 0) + (nl + 1) // 2 + (nr + 1) // 2


# ---- (a) the corners of the key space in every order -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corner_lists(n_nodes: int):
    """Every (nl, nr) in 1..20 x 1..20, three times: both lists ascending (a short row's partners are never below x),
    both descending (always below x, but for x itself), both shuffled (below, equal and above x in one row; x changes at
    the second stretch of every folded row)."""
    rng = np.random.default_rng(1300 + n_nodes)
    pool = _pool(n_nodes)
    pairs = []
    for order in ("ascending", "descending", "mixed"):
        for nl in range(1, 21):
            for nr in range(1, 21):
                ends = []
                for n in (nl, nr):
                    # the first n of the pool, or, for short lists, any n of the five corners
                    nodes = [pool[i] for i in rng.permutation(5)[:n]] if n < 5 else pool[:n]
                    if order == "mixed":
                        nodes = [nodes[i] for i in rng.permutation(n)]
                    else:
                        nodes = sorted(nodes, reverse=order == "descending")
                    ends.append([int(x) for x in nodes])
                pairs.append((ends[0], ends[1]))
    return n_nodes, pairs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_nodes", [4097, 32768, 46340])
def test_corner_nodes_in_every_order(monkeypatch, ctx, xctx, n_nodes, mode):
    import torch

    case = corner_lists(n_nodes)
    N = n_nodes
    mixed = case[1][800:]
    # a shuffled long list has, behind some x, a partner below it and one above it
    assert any(any(y < l[a] for y in l[a + 1:]) and any(y > l[a] for y in l[a + 1:]) for l, _ in mixed for a in range(len(l)))
    # the corners of both matrices are hit: the largest key of either, the first key of short_mat
    assert any(N - 1 in l and N - 1 in r for l, r in case[1]) and any(0 in l for l, _ in case[1])
    base._count_and_compare(monkeypatch, ctx, xctx, case, "keys_corners%d" % n_nodes, mode)
    torch.cuda.empty_cache()


# ---- (b) node rows and short rows side by side in one wavefront ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_kinds(n_nodes: int = 4097, seed: int = 1302):
    """64 pairs, one wavefront's round: a 1-node list against a 20-node list and the other way round, alternating.  The
    tasks of a batch are ordered by their turns, so the 20 one-turn node rows of an odd pair lie among the one-turn middle
    rows, and the 20-turn node rows of the even pairs next to the folded rows of the 20-node lists (21 turns and more):
    lanes of both kinds, and of both forms of the short rows' key, in the same windows."""
    rng = np.random.default_rng(seed)
    pool = _pool(n_nodes)
    pairs = []
    for p in range(64):
        long = [pool[i] for i in rng.permutation(20)]
        one = [pool[int(rng.integers(0, 20))]]
        pairs.append((one, long) if p % 2 == 0 else (long, one))
    return n_nodes, pairs


@pytest.mark.parametrize("mode", MODES)
def test_node_rows_and_short_rows_in_one_window(monkeypatch, ctx, xctx, mode):
    case = mixed_kinds()
    assert [(len(l), len(r)) for l, r in case[1][:2]] == [(1, 20), (20, 1)] and len(case[1]) == 64
    assert sum(_tasks(len(l), len(r)) for l, r in case[1]) == 32 * (12 + 31)  # more than one batch of 960
    base._count_and_compare(monkeypatch, ctx, xctx, case, "keys_kinds", mode)


# ---- (c) turns that count nothing --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged(n_pairs: int, n_nodes: int = 4097, seed: int = 1303):
    """Lists whose lengths are no multiples of four (the last block of every stretch reaches beyond the list's end, into
    the next list or the padding) and differ inside a window (a short task's lane idles, at a position beyond its end,
    while the window's longest goes on); the tasks do not fill the last window."""
    rng = np.random.default_rng(seed + n_pairs)
    pool = _pool(n_nodes)
    lengths = [1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 18, 19]
    pairs = []
    for _ in range(n_pairs):
        nl, nr = (lengths[int(rng.integers(0, len(lengths)))] for _ in range(2))
        pairs.append(([pool[i] for i in rng.permutation(20)[:nl]], [pool[i] for i in rng.permutation(20)[:nr]]))
    return n_nodes, pairs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_pairs", [1, 3, 70])
def test_partly_empty_windows_and_blocks(monkeypatch, ctx, xctx, n_pairs, mode):
    case = ragged(n_pairs)
    tasks = [_tasks(len(l), len(r)) for l, r in case[1]]
    assert all(len(e) % 4 for pair in case[1] for e in pair)
    # the last window of the first wavefront's round (64 pairs, cut into batches of at most 960 tasks) is partly empty
    first = tasks[:64]
    assert sum(first) % 64 != 0 and (sum(first) <= 960 or n_pairs > 3)
    if n_pairs == 1:
        assert sum(tasks) < 64  # one window, half of its lanes without a task
    base._count_and_compare(monkeypatch, ctx, xctx, case, "keys_ragged%d" % n_pairs, mode)
