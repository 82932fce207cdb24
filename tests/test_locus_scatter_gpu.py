"""The turns of k_locus_scatter on the device (vstrains_amd/csrc/vs_pe.hip: a thread places LOCUS_SCATTER_U pairs a turn, the
next turn's keys requested before this turn's LDS atomics) at the block sizes of tests/locus_scatter_cases.py: chunks one
below, at and one above a whole turn of the workgroup, chunks of 16 to 19 pairs, and the two-pass sort of the `chain` graph
(key_lo > 0) -- each also with the scatter cut into two and four launches of a range of keys, the launch rule of
csrc/vs_pe_plan.h for blocks of millions of pairs, reached here through VS_LOCUS_SCATTER.  The reference is the same
context and index build with VS_LOCUS_STAGE=0 (k_locus_count): the keys bit for bit, the order as
tests/test_pe_counters_gpu.py::test_locus_order states it (a permutation, in key order, equal keys of different chunks in
chunk order), the end lists, both counters and the statistics -- those also against a VS_NO_SORT=1 run, which takes the
pairs in input order.  The launched-bit says whether the staged key pass ran."""
import numpy as np
import pytest

import locus_scatter_cases as cases
import test_pe_counters_gpu as base

pytestmark = pytest.mark.gpu

N0 = 5003  # pairs of the inputs a block repeats


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def xctx(host):
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


_inputs = {}


def _graph(xctx, graph):
    """The inputs of one graph, made once, and the context's index built from them (once per run of graphs in file order)."""
    if graph not in _inputs:
        seqs, k, fwd, rve, allowed = base._locus_inputs(graph, N0, 31 + N0)
        _inputs[graph] = dict(seqs=seqs, k=k, fwd=fwd, rve=rve, table=cases.allowed_table(allowed), blocks={})
    g = _inputs[graph]
    if _inputs.get("built") != graph:
        xctx.build_index(g["seqs"], g["k"], renumber=False)
        _inputs["built"] = graph
    return g


def _end_lists(c, reads, cap):
    """The per-end node lists of a block as arrays (vs_pe_map_ends without the Python lists of Context.map_ends): counts
    [ends], lists [ends, cap] with each end's nodes in ascending order and ~0 behind them."""
    from vstrains_amd import _native as nat

    n = reads.info["ends"]
    lists = np.zeros((n, cap), dtype=np.uint32)
    counts = np.zeros(n, dtype=np.uint32)
    nat.check(c._h, nat.lib().vs_pe_map_ends(c._h, reads._h, cap, lists.ctypes.data, counts.ctypes.data))
    assert int(counts.max()) <= cap
    lists[np.arange(cap, dtype=np.uint32)[None, :] >= counts[:, None]] = 0xFFFFFFFF
    lists.sort(axis=1)
    return counts, lists


def _run(monkeypatch, c, data, off, n_nodes, cap, mats, stage=None, no_sort=False, scatter=None):
    """One block mapped and counted into `mats` (zeroed here) under the switches given."""
    import torch

    monkeypatch.delenv("VS_LOCUS_STAGE", raising=False)
    monkeypatch.delenv("VS_NO_SORT", raising=False)
    monkeypatch.delenv("VS_LOCUS_SCATTER", raising=False)
    if scatter is not None:
        monkeypatch.setenv("VS_LOCUS_SCATTER", str(scatter))
    if stage is not None:
        monkeypatch.setenv("VS_LOCUS_STAGE", str(stage))
    if no_sort:
        monkeypatch.setenv("VS_NO_SORT", "1")
    reads = c.pack(data, off)
    counts, lists = _end_lists(c, reads, cap)
    keys, perm, sort, n = c.last_order()
    got = dict(counts=counts, lists=lists, keys=keys.copy(), perm=perm.copy(), sort=sort, n=n, staged=bool(c.last_launched & c.RAN_LOCUS_STAGED))
    mats.zero_()
    stats = torch.zeros(3, dtype=torch.int64, device=mats.device)
    with torch.cuda.device(mats.device):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.pe_count(reads, mats[0].data_ptr(), mats[1].data_ptr(), stats.data_ptr())
        c.sync()
    keys2, perm2, sort2, _ = c.last_order()
    got.update(stats=stats.cpu().numpy(), count_keys=keys2.copy(), count_perm=perm2.copy(), count_sort=sort2,
               count_staged=bool(c.last_launched & c.RAN_LOCUS_STAGED))
    reads.free()
    return got


def _order_ok(keys, perm, n_pairs, n_keys):
    """What test_locus_order states of the LDS sort: a permutation, in key order, equal keys of different chunks in chunk order."""
    assert perm.size == n_pairs and int(perm.max()) < n_pairs
    assert np.array_equal(np.bincount(perm, minlength=n_pairs), np.ones(n_pairs, dtype=np.int64))
    sorted_keys = keys[perm].astype(np.int64)
    assert int(sorted_keys[-1]) < n_keys and (np.diff(sorted_keys) >= 0).all()
    wg = perm.astype(np.int64) // cases.chunk_of(n_pairs)
    assert (np.diff(wg)[np.diff(sorted_keys) == 0] >= 0).all()


def _check(monkeypatch, xctx, graph, n_pairs, cap, staged):
    import torch

    g = _graph(xctx, graph)
    N = len(g["seqs"])
    data, off = cases.tile(g["fwd"], g["rve"], n_pairs)
    dev = "cuda:%d" % xctx.device
    ref_mats = torch.zeros((2, N, N), dtype=torch.int32, device=dev)
    mats = torch.zeros((2, N, N), dtype=torch.int32, device=dev)
    ref = _run(monkeypatch, xctx, data, off, N, cap, ref_mats, stage=0)
    assert ref["n"] == n_pairs and ref["sort"] == ref["count_sort"] == xctx.RAN_LOCUS_LDS_SORT and not ref["staged"] and not ref["count_staged"]
    ok = cases.keys_allowed(ref["keys"], g["table"])
    assert ok.all(), (np.nonzero(~ok)[0][:8], ref["keys"][~ok][:8])
    assert (N + 2 > 36864) == (graph == "chain")  # (two LDS passes over the keys)
    assert bool(ref_mats.any())
    _order_ok(ref["keys"], ref["perm"], n_pairs, N + 2)
    _order_ok(ref["count_keys"], ref["count_perm"], n_pairs, N + 2)
    # what production does (these blocks: every key of a pass in one launch of the scatter), then the scatter in two and in
    # four launches of a range of keys each, as the plan cuts it for blocks of millions of pairs (VS_LOCUS_SCATTER: about
    # that many pairs' worth of keys a launch, four launches at most -- tests/test_locus_scatter_cases_cpu.py)
    for scatter in (None, n_pairs // 2 + 1, 1):
        got = _run(monkeypatch, xctx, data, off, N, cap, mats, scatter=scatter)
        assert got["n"] == n_pairs and got["sort"] == got["count_sort"] == xctx.RAN_LOCUS_LDS_SORT, scatter
        assert got["staged"] == got["count_staged"] == staged, scatter  # (the bit: the staged pass ran)
        diff = np.nonzero(got["keys"] != ref["keys"])[0]
        assert diff.size == 0, (scatter, diff[:8], got["keys"][diff[:8]], ref["keys"][diff[:8]])
        assert np.array_equal(got["count_keys"], ref["keys"]) and np.array_equal(ref["count_keys"], ref["keys"]), scatter
        _order_ok(got["keys"], got["perm"], n_pairs, N + 2)
        _order_ok(got["count_keys"], got["count_perm"], n_pairs, N + 2)
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["lists"], ref["lists"]), scatter
        assert torch.equal(mats, ref_mats) and np.array_equal(got["stats"], ref["stats"]), scatter
    plain = _run(monkeypatch, xctx, data, off, N, cap, mats, no_sort=True)
    assert plain["sort"] == 0 and plain["count_sort"] == 0 and plain["keys"].size == 0
    assert np.array_equal(plain["counts"], ref["counts"]) and np.array_equal(plain["lists"], ref["lists"])
    assert torch.equal(mats, ref_mats) and np.array_equal(plain["stats"], ref["stats"])
    del mats, ref_mats


# (a read of the `small` graph lies in one node, or in the few that share its text; one of the `chain` graph crosses up to 14)
@pytest.mark.parametrize("n_pairs", cases.SMALL_SIZES)
def test_small_chunks(monkeypatch, xctx, n_pairs):
    _check(monkeypatch, xctx, "small", n_pairs, cap=16, staged=True)


@pytest.mark.parametrize("n_pairs", cases.TURN_SIZES)
def test_chunks_round_a_whole_turn(monkeypatch, xctx, n_pairs):
    _check(monkeypatch, xctx, "small", n_pairs, cap=16, staged=True)


@pytest.mark.parametrize("n_pairs", cases.CHAIN_SIZES)
def test_two_passes(monkeypatch, xctx, n_pairs):
    _check(monkeypatch, xctx, "chain", n_pairs, cap=32, staged=False)
    if n_pairs == cases.CHAIN_SIZES[-1]:
        import torch

        torch.cuda.empty_cache()  # (the two matrices of 40 000 nodes: 12.8 GB each)
