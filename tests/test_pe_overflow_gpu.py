"""k_pe_mid and k_pe_slow (vstrains_amd/csrc/vs_pe.hip) at their limits: the blocks of tests/pe_overflow_cases.py, whose ends
sit on either side of 64 probes, 256 touched and 64 accepted nodes per end, and on one, two and three probe batches of
k_pe_slow.  Per family both counters, the statistics and every end's list equal the C oracle's, and -- through
Context.last_overflow() -- exactly the pairs the model names stay in k_pe_mid and exactly the others go on to k_pe_slow.
Under a production context, with k_pe_mid skipped (VS_NO_MID=1) and with the row owners next to it (VS_ACC_ROWS=1).  The
'second pairs' block gives every wavefront of k_pe_mid and every workgroup of k_pe_slow more than three pairs, neighbours of
different kinds: what either kernel resets between pairs is then used.  Integers, compared for equality.  That the families
are what they claim is asserted without a device by tests/test_pe_overflow_cases_cpu.py."""
import functools

import numpy as np
import pytest

import pe_overflow_cases as poc
from oracle import pe_oracle_c

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


@pytest.fixture(scope="module")
def xctx(host):
    """A context in experiment mode: the tuning switches of vs_pe_count are live on it (conftest.experiment_context)."""
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


def _reference(fam, times=1):
    """The oracle's answer to a block: the non-zero cells of both matrices (cell = row * nodes + column, ascending) with
    their counts, the statistics, the list of every end; ``times``: of the block that many times over."""
    orc = pe_oracle_c.Oracle(fam["seqs"], fam["k"])
    fd, fo = pe_oracle_c.concat(fam["fwd"])
    rd, ro = pe_oracle_c.concat(fam["rve"])
    nc, nv, sc, sv, stats = orc.count_pairs_sparse(fd, fo, rd, ro, len(fam["fwd"]))
    lists = []
    K = fam["k"] + 1
    for f, r in zip(fam["fwd"], fam["rve"]):
        used = "N" not in f and "N" not in r and len(f) >= K and len(r) >= K
        lists += [orc.map_end(f) if used else [], orc.map_end(r) if used else []]
    return dict(cells=(nc, sc), counts=(nv * times, sv * times), stats=tuple(int(x) * times for x in stats), lists=lists)


@functools.lru_cache(maxsize=None)
def family(name):
    """A family, the model's verdict on every pair and the oracle's answer: computed once, shared by the tests, never changed."""
    fam = poc.family(name)
    where, mode, mid_fast = poc.verdicts(fam)
    ref = _reference(fam)
    assert len(ref["cells"][0]) > 0 and len(ref["cells"][1]) > 0 and ref["stats"][2] == sum(w != "dropped" for w in where)
    return fam, dict(where=where, mode=mode, mid_fast=mid_fast), ref


def _cells(counter):
    """The non-zero cells of the counter's two matrices and their counts, found on the device."""
    n = counter.n
    out = []
    for m in (counter.mats[0, :n, :n], counter.mats[1, :n, :n]):
        idx = m.nonzero()
        out.append(((idx[:, 0] * n + idx[:, 1]).cpu().numpy(), m[idx[:, 0], idx[:, 1]].cpu().numpy().view(np.uint32).astype(np.int64)))
    return out


def _compare(counter, ref, what):
    for (cells, counts), want_cells, want_counts, mat in zip(_cells(counter), ref["cells"], ref["counts"], ("node_mat", "short_mat")):
        n = counter.n
        assert np.array_equal(cells, want_cells), (what, mat, [divmod(int(c), n) for c in np.setxor1d(cells, want_cells)[:8]])
        bad = np.flatnonzero(counts != want_counts)
        assert bad.size == 0, (what, mat, [(divmod(int(cells[i]), n), int(counts[i]), int(want_counts[i])) for i in bad[:8]])
    assert tuple(int(x) for x in counter.stats.cpu().numpy()) == ref["stats"], what


def _check_overflow(ctx, verdict, pairs, no_mid, what):
    """Context.last_overflow() against the model: the pairs the main path gave up, the pairs k_pe_mid passed on."""
    over = ctx.last_overflow()
    where = [verdict["where"][p] for p in pairs]
    slow = [i for i, w in enumerate(where) if w == "slow"]
    assert over is not None and over["first_n"] == sum(w in ("mid", "slow") for w in where), (what, over)
    assert bool(ctx.last_launched & ctx.RAN_PE_MID) == (not no_mid), what
    if no_mid:
        assert (over["second_n"], over["no_mid"], over["second"].size) == (0, 1, 0), (what, over)
    else:
        assert over["no_mid"] == 0 and over["second_n"] == over["second"].size, (what, over)
        got = sorted(int(x) for x in over["second"])
        assert got == slow, (what, "stayed but must leave", sorted(set(slow) - set(got))[:8], "left but must stay", sorted(set(got) - set(slow))[:8])
    assert ctx.last_kernel.startswith("k_pe_tiles<%d" % verdict["mode"]), (what, ctx.last_kernel)  # (mid_fast = 1 is MODE 1 with exact seed keys)


def _check(host, ctx, fam, verdict, ref, what, no_mid=False, tracked=False, ends=None, times=1):
    import torch

    ctx.build_index(fam["seqs"], fam["k"], renumber=False)
    assert ctx.node_order is None
    order = range(len(fam["fwd"]))
    counter = host.PeCounter(ctx, track_tiles=tracked)
    block = ctx.pack_pairs(fam["fwd"], fam["rve"])
    for _ in range(times):
        counter.add(block)
        _check_overflow(ctx, verdict, order, no_mid, what)
    _compare(counter, ref, what)
    if tracked:  # every non-zero cell lies in a marked tile, and a reset leaves nothing
        n = counter.n
        T = (n + 63) // 64
        marked = counter.tile_map.view(2, T, T).bool()
        idx = (counter.mats[:, :n, :n] != 0).nonzero()
        tiles_nz = torch.zeros((2, T, T), dtype=torch.bool, device=idx.device)
        tiles_nz[idx[:, 0], idx[:, 1] // 64, idx[:, 2] // 64] = True
        assert bool((tiles_nz & ~marked).sum() == 0), (what, "a non-zero cell lies in an unmarked tile")
        counter.reset()
        torch.cuda.synchronize()
        assert int(counter.mats.abs().sum()) == 0 and int(counter.tile_map.sum()) == 0
    if ends is not None:
        cap = max(max(len(x) for x in ref["lists"]), 1)
        lists = ctx.map_ends(block, cap=cap)
        _check_overflow(ctx, verdict, order, no_mid, what + ", map_ends")
        wrong = [(e // 2, fam["label"][e // 2], len(lists[e]), len(ref["lists"][e])) for e in ends if lists[e] != ref["lists"][e]]
        assert not wrong, (what, len(wrong), wrong[:6])


def _with_env(monkeypatch, env, fn):
    with monkeypatch.context() as m:
        for name, value in env.items():
            m.setenv(name, value)
        fn()


@pytest.mark.parametrize("name", poc.FAMILIES)
def test_limits_on_a_production_context(host, ctx, name):
    fam, verdict, ref = family(name)
    _check(host, ctx, fam, verdict, ref, name, ends=range(2 * len(fam["fwd"])))


@pytest.mark.parametrize("name", poc.FAMILIES)
def test_limits_without_k_pe_mid_and_next_to_the_row_owners(host, xctx, name, monkeypatch):
    """VS_NO_MID=1: k_pe_slow takes the first list whole (second_n = 0, no_mid = 1).  VS_ACC_ROWS=1: the pairs that stay on the
    main path are counted by the row owners, the overflow pairs by k_pe_mid / k_pe_slow into the same counters."""
    fam, verdict, ref = family(name)
    _with_env(monkeypatch, {"VS_NO_MID": "1"}, lambda: _check(host, xctx, fam, verdict, ref, name + " VS_NO_MID=1", no_mid=True, ends=range(2 * len(fam["fwd"]))))
    _with_env(monkeypatch, {"VS_ACC_ROWS": "1"}, lambda: _check(host, xctx, fam, verdict, ref, name + " VS_ACC_ROWS=1"))
    if name == "plain":  # (the 200-base pair stays on the main path)
        assert xctx.last_launched & xctx.RAN_ROW_OWNERS


@pytest.mark.parametrize("name,no_mid", [("list", False), ("batches", False), ("list", True)])
def test_tracked_counting_marks_the_tiles_of_either_overflow_kernel(host, xctx, name, no_mid, monkeypatch):
    """PeCounter(track_tiles=True): k_pe_mid (the 'list' family: 4 096 cells from one wavefront) and k_pe_slow (the 'batches'
    family, and 'list' without k_pe_mid) mark the tiles they add to."""
    fam, verdict, ref = family(name)
    assert len(fam["seqs"]) > 128  # (several tiles a side)
    _with_env(monkeypatch, {"VS_NO_MID": "1"} if no_mid else {}, lambda: _check(host, xctx, fam, verdict, ref, name + " tracked", no_mid=no_mid, tracked=True))


def test_map_ends_with_the_cap_on_the_list_limit(host, ctx):
    """The ends of exactly 64 accepted nodes, written out with cap = 64."""
    fam, verdict, ref = family("list")
    keep = [p for p, w in enumerate(verdict["where"]) if w == "mid"]
    ctx.build_index(fam["seqs"], fam["k"], renumber=False)
    lists = ctx.map_ends(ctx.pack_pairs([fam["fwd"][p] for p in keep], [fam["rve"][p] for p in keep]), cap=64)
    assert lists == [ref["lists"][2 * p + e] for p in keep for e in (0, 1)]
    assert sum(len(x) == 64 for x in lists) >= 6 and max(len(x) for x in lists) == 64
    over = ctx.last_overflow()
    assert (over["first_n"], over["second_n"], over["no_mid"]) == (len(keep), 0, 0)


def test_last_overflow_is_invalid_before_a_launch_and_after_an_empty_block(host):
    c = host.Context(0)
    try:
        assert c.last_overflow() is None
        fam, _, _ = family("probes")
        c.build_index(fam["seqs"], fam["k"], renumber=False)
        host.PeCounter(c).add(c.pack_pairs(fam["fwd"], fam["rve"]))
        assert c.last_overflow()["first_n"] == len(fam["fwd"])
        host.PeCounter(c).add(c.pack_pairs([], []))
        assert c.last_overflow() is None
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def second_pairs():
    """The 'second pairs' block for this device: the oracle is asked about one round of distinct pairs and its answer
    multiplied by the repetitions (every pair of the round is in the block that many times) and by the two launches."""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rnd, order, reps = poc.second_pairs(n_cu)
    where, mode, mid_fast = poc.verdicts(rnd)
    n_mid, n_slow = sum(where[i] in ("mid", "slow") for i in order), sum(where[i] == "slow" for i in order)
    assert n_mid > 3 * n_cu * 32 and n_slow > 3 * poc.slow_grid_for(len(rnd["seqs"])), (n_cu, n_mid, n_slow)
    assert (mode, mid_fast) == (1, 1) and 20000 < len(order) <= 60000
    block = dict(rnd, fwd=[rnd["fwd"][i] for i in order], rve=[rnd["rve"][i] for i in order], label=[rnd["label"][i] for i in order])
    one = _reference(rnd)
    ref = _reference(rnd, times=2 * reps)
    ref["lists"] = [one["lists"][2 * i + e] for i in order for e in (0, 1)]
    return block, dict(where=[where[i] for i in order], mode=mode, mid_fast=mid_fast), ref


def test_second_pairs_of_every_walker_counted_twice_into_one_counter(host, ctx):
    """More than three pairs per wavefront of k_pe_mid and per workgroup of k_pe_slow, the block counted twice into one counter:
    twice the oracle's, so the flags, the table, the list lengths and the dense node state start every pair and every launch clean."""
    block, verdict, ref = second_pairs()
    _check(host, ctx, block, verdict, ref, "second pairs", ends=range(0, 2 * len(block["fwd"]), 97), times=2)
    assert ctx.last_launched & ctx.RAN_LOCUS_LDS_SORT


def test_second_pairs_all_through_k_pe_slow(host, xctx, monkeypatch):
    """VS_NO_MID=1: every overflow pair of the block goes through k_pe_slow, twelve and more per workgroup."""
    block, verdict, ref = second_pairs()
    _with_env(monkeypatch, {"VS_NO_MID": "1"}, lambda: _check(host, xctx, block, verdict, ref, "second pairs VS_NO_MID=1", no_mid=True, times=2))
