"""The two device primitives under almost everything else, at their own size boundaries.

The exclusive scans (vs_scan_u32: three launches, 2 048 values per workgroup, the block sums walked 256 at a time with a
carry; k_sl_scan: one workgroup of 1 024 threads, a slice of ceil(m / 1024) values each) run alone through vs_scan_check
on made-up values and are compared with numpy.cumsum in uint64: the offsets modulo 2^32, the total exactly, and the 64
words behind the values untouched.

Chain ranking (k_chain_rank: one workgroup, ceil(log2(V)) rounds; k_chain_init_wide / k_chain_jump_wide /
k_chain_finish_wide from 8 193 vertices on: four rounds, then the others only if the fourth still found work) runs on
graphs built so that every rank and every head is known from the construction -- the position in the path and the path's
first vertex -- and is compared with the numpy checker as well, flows included.  Everything here is exact integer work (the
flows bit-exact fp64, as in test_graph_gpu.py): every assertion is equality."""
import functools
import random

import numpy as np
import pytest

from oracle import graph_ops as chk
from vstrains_amd.graph.asm_graph import AsmGraph

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = (np.uint32(0x5EED0000) + np.arange(GUARD, dtype=np.uint32)).astype(np.uint32)
SENTINEL.setflags(write=False)
UNTOUCHED = 0x0123456789ABCDEF  # what *total holds before a scan that is given no place for its total


@pytest.fixture(scope="module")
def backend():
    from vstrains_amd.graph.hip_ops import HipBackend

    return HipBackend(0)


# ---- the exclusive scans ----------------------------------------------------------------------------------------------

WIDE_SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 524287, 524288, 524289, 1048576 + 2049]
WIDE_NO_TOTAL_SIZES = [524287, 524288, 524289, 1048576 + 2049]  # 256 block sums and fewer / one pass more of k_scan_sums
SLICE_SIZES = [0, 1, 2, 1023, 1024, 1025, 2047, 2049, 3077, 100003, 1048577]
FILLS = ["ones", "zeros", "last", "random"]


@functools.lru_cache(maxsize=None)
def scan_case(n, fill, below_2_32):
    """(values, exclusive prefix sums modulo 2^32, exact total) -- made once, shared, read-only.  ``below_2_32``: random
    values below 2^32 / n, so that their total stays below 2^32 (what the one-workgroup scan is specified for); otherwise
    the whole uint32 range, whose total passes 2^32 from a few cells on."""
    rng = np.random.default_rng([n, FILLS.index(fill), int(below_2_32)])
    if fill == "ones":
        v = np.ones(n, dtype=np.uint32)
    elif fill == "zeros":
        v = np.zeros(n, dtype=np.uint32)
    elif fill == "last":
        v = np.zeros(n, dtype=np.uint32)
        if n:
            v[-1] = 0xFFFFFFFF
    else:
        v = rng.integers(0, (2 ** 32 // max(n, 1)) if below_2_32 else 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    incl = np.cumsum(v.astype(np.uint64), dtype=np.uint64)
    excl = np.concatenate([np.zeros(1, dtype=np.uint64), incl[:-1]]) if n else np.zeros(0, dtype=np.uint64)
    total = int(incl[-1]) if n else 0
    want = (excl & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if fill == "random" and not below_2_32 and n >= 4096:
        assert total > 2 ** 32 and int(excl[-1]) > 2 ** 32  # (the case is what it says: the offsets wrap, the total must not)
    if below_2_32:
        assert total < 2 ** 32
    for a in (v, want):
        a.setflags(write=False)
    return v, want, total


def check_scan(ctx, which, n, fill, flags):
    v, want, total = scan_case(n, fill, which == 1)
    got, tail, got_total = ctx.scan_check(which, v, SENTINEL, flags, total_before=UNTOUCHED)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first wrong offset at %d of %d: %d, expected %d" % (bad[0], n, got[bad[0]], want[bad[0]])
    assert np.array_equal(tail, SENTINEL), "the scan wrote behind its %d values: %s" % (n, np.flatnonzero(tail != SENTINEL)[:8])
    assert got_total == (UNTOUCHED if flags & 2 else total)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("in_place", [0, 1], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n", WIDE_SIZES)
def test_three_launch_scan_against_cumsum(backend, n, in_place, fill):
    check_scan(backend.ctx, 0, n, fill, in_place)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("in_place", [0, 1], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n", WIDE_NO_TOTAL_SIZES + [0])
def test_three_launch_scan_without_a_place_for_its_total(backend, n, in_place, fill):
    check_scan(backend.ctx, 0, n, fill, in_place | 2)


def test_three_launch_scan_of_nothing_writes_a_zero_total_and_nothing_else(backend):
    for flags in (0, 1):
        got, tail, total = backend.ctx.scan_check(0, np.zeros(0, dtype=np.uint32), SENTINEL, flags, total_before=UNTOUCHED)
        assert got.size == 0 and np.array_equal(tail, SENTINEL) and total == 0


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("n", SLICE_SIZES)
def test_one_workgroup_scan_against_cumsum(backend, n, fill):
    check_scan(backend.ctx, 1, n, fill, 0)


# ---- chain ranking ----------------------------------------------------------------------------------------------------

class Built:
    """A graph of simple paths, rings of simple edges and a branching remainder, with what the ranking must say about it:
    rank[v] = position of v in its path (-1 on a ring), top[v] = the path's first vertex, next[v] = its successor."""

    def __init__(self, nv, seed):
        self.rng = random.Random(seed)
        self.g = AsmGraph()
        for i in range(nv):
            self.g.add_vertex(str(i), self.rng.uniform(1.0, 500.0), "ACGT", True)
        self.rank = [0] * nv
        self.top = list(range(nv))
        self.next = [-1] * nv

    def path(self, vs):
        for a, b in zip(vs, vs[1:]):
            self.g.add_edge(a, b, 21, 0.0, True)
            self.next[a] = b
        for i, v in enumerate(vs):
            self.rank[v], self.top[v] = i, vs[0]

    def ring(self, vs):
        for a, b in zip(vs, vs[1:] + vs[:1]):
            self.g.add_edge(a, b, 21, 0.0, True)
            self.next[a] = b
        for v in vs:
            self.rank[v] = -1

    def diamond(self, vs):
        """a -> b, a -> c, b -> d, c -> d: no edge of it is simple (a has two successors, d two predecessors)"""
        a, b, c, d = vs
        for s, t in ((a, b), (a, c), (b, d), (c, d)):
            self.g.add_edge(s, t, 21, 0.0, True)

    def check(self, scan):
        assert scan.chain_next == self.next
        bad = [v for v in range(len(self.rank)) if scan.chain_rank[v] != self.rank[v]]
        assert not bad, "rank of vertex %d: %d, by construction %d (%d wrong)" % (bad[0], scan.chain_rank[bad[0]], self.rank[bad[0]], len(bad))
        bad = [v for v in range(len(self.rank)) if self.rank[v] >= 0 and scan.chain_top[v] != self.top[v]]
        assert not bad, "head of vertex %d: %d, by construction %d (%d wrong)" % (bad[0], scan.chain_top[bad[0]], self.top[bad[0]], len(bad))


def ordered(n, order, rng):
    vs = list(range(n))
    if order == "reversed":
        vs.reverse()
    elif order == "shuffled":
        rng.shuffle(vs)
    return vs


def assert_same_as_checker(got, g, flows_of):
    """``got``: the device's scan of ``g``; ``flows_of``: the device's flows by edge -- against oracle.graph_ops"""
    ref = chk.NumpyGraphOps()
    h = AsmGraph.__new__(AsmGraph)
    for slot in AsmGraph.__slots__:
        setattr(h, slot, getattr(g, slot))
    h.eflow = list(g.eflow)
    want = ref.refresh(h)
    assert (got.nontrivial, got.fork_kind, got.chain_next, got.chain_rank) == (want.nontrivial, want.fork_kind, want.chain_next, want.chain_rank)
    for v in range(g.num_vertices()):
        if want.chain_rank[v] >= 0:
            assert got.chain_top[v] == want.chain_top[v], v
    for e in g.edges():
        assert flows_of[e] == h.eflow[e], (e, flows_of[e], h.eflow[e])  # bit-exact fp64


def run_one_workgroup(backend, b):
    got = backend.graph_ops.refresh(b.g)  # (vs_graph_refresh: flows into b.g, the scan returned)
    b.check(got)
    assert_same_as_checker(got, b.g, b.g.eflow)


@pytest.mark.parametrize("order", ["path_order", "reversed", "shuffled"])
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 16, 17, 1023, 1024, 1025, 2048, 2049, 4096, 4097])
def test_one_chain_over_the_whole_graph_in_one_workgroup(backend, nv, order):
    """ceil(log2(nv)) rounds are exactly enough only for this graph: a chain of 2^r vertices needs r of them, one of
    2^r + 1 needs r + 1."""
    b = Built(nv, nv)
    b.path(ordered(nv, order, b.rng))
    assert max(b.rank) == nv - 1
    run_one_workgroup(backend, b)


def test_chains_of_two_and_one_vertex_alone_in_one_workgroup(backend):
    b = Built(4097, 1)
    vs = ordered(4097, "shuffled", b.rng)
    for i in range(0, 4096, 2):
        b.path(vs[i:i + 2])
    assert sorted(b.rank) == [0] * 2049 + [1] * 2048
    run_one_workgroup(backend, b)


def test_a_ring_over_the_whole_graph_in_one_workgroup(backend):
    b = Built(1025, 2)
    b.ring(ordered(1025, "shuffled", b.rng))
    assert b.rank == [-1] * 1025
    run_one_workgroup(backend, b)


def test_a_ring_of_three_beside_a_chain_in_one_workgroup(backend):
    b = Built(1025, 3)
    vs = ordered(1025, "shuffled", b.rng)
    b.ring(vs[:3])
    b.path(vs[3:])
    assert sorted(b.rank) == [-1] * 3 + list(range(1022))
    run_one_workgroup(backend, b)


@pytest.fixture(scope="module")
def stage(backend):
    from vstrains_amd.graph.hip_ops import HipPeLinks
    from vstrains_amd.graph.native_stage import NativeStage

    table = HipPeLinks.from_matrices(backend.ctx, ["x"], np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1), dtype=np.int64))
    st = NativeStage.on_device(backend.ctx, table, table.names)
    yield st
    st.close()


def stage_graph(nv, lengths, ring=0, diamond=True, extra_isolated=0, seed=0):
    """``nv`` vertices under shuffled numbers: a path of every length of ``lengths``, a ring of ``ring`` vertices, a
    four-vertex diamond as the branching remainder, the rest alone; then ``extra_isolated`` more vertices, alone too."""
    b = Built(nv + extra_isolated, seed)
    vs = ordered(nv, "shuffled", b.rng)
    at = 0
    for n in lengths:
        b.path(vs[at:at + n])
        at += n
    if ring:
        b.ring(vs[at:at + ring])
        at += ring
    if diamond:
        b.diamond(vs[at:at + 4])
        at += 4
    assert at <= nv, (at, nv)
    return b


SHORT = [15, 16, 17, 31, 32, 33]
STAGE_CASES = {
    # 8 192 vertices are the last graph of k_chain_rank, 8 193 the first of the multi-launch form: the same graph plus one
    # vertex alone.  (15 .. 33 with 4 096 and 4 097 are 8 337 vertices: each graph holds one of the two beside the other
    # pair's member, so that both sizes rank all four lengths.)
    "8192_chains_4096_2049": dict(nv=8192, lengths=SHORT + [4096, 2049], seed=11),
    "8193_chains_4096_2049": dict(nv=8192, lengths=SHORT + [4096, 2049], seed=11, extra_isolated=1),
    "8192_chains_4097_2048": dict(nv=8192, lengths=SHORT + [4097, 2048], seed=12),
    "8193_chains_4097_2048": dict(nv=8192, lengths=SHORT + [4097, 2048], seed=12, extra_isolated=1),
    # the first four rounds finish every chain: nothing may change behind them
    "8193_nothing_longer_than_16": dict(nv=8193, lengths=[16] * 200 + list(range(1, 17)) * 30, seed=13),
    # the smallest graph that needs the rounds launched after the first wait
    "8193_one_chain_of_17": dict(nv=8193, lengths=[17] + [2] * 3000, seed=14),
    # 2^13 + 1 vertices in one chain: all 14 rounds
    "8193_one_chain_over_all": dict(nv=8193, lengths=[8193], diamond=False, seed=15),
    # the ring keeps every round live although no chain needs more than three
    "9000_ring_of_40_chains_up_to_8": dict(nv=9000, lengths=list(range(1, 9)) * 240, ring=40, seed=16),
}


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_chain_ranking_through_the_stage_handle(backend, stage, name, tmp_path):
    from vstrains_amd.graph.formats import stage_graph_from_state

    spec = STAGE_CASES[name]
    b = stage_graph(**spec)
    g = b.g
    assert g.num_vertices() == int(name.split("_")[0])
    assert max(b.rank) == max(spec["lengths"]) - 1 and (min(b.rank) == -1) == bool(spec.get("ring"))
    nodes = {g.vid[v]: v for v in range(g.num_vertices())}
    edges = {(g.vid[g.esrc[e]], g.vid[g.etgt[e]]): e for e in g.edges()}
    a = stage_graph_from_state(g, nodes, edges)
    assert a[0].vid == g.vid  # (the rebuilt graph numbers the vertices as they were made: the construction speaks its numbers)
    stage.load_graph(g, nodes, edges)
    stage.reinit(str(tmp_path / "chains.gfa"))
    got = stage.scan()
    gb, _, _ = stage.graph()
    assert gb.vid == g.vid and gb.esrc == a[0].esrc and gb.etgt == a[0].etgt
    b.check(got)
    assert_same_as_checker(got, a[0], gb.eflow)
