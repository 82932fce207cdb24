"""Constructed inputs of ``vs_graph_refresh`` (K6 vertex scan, K7 edge flow; vstrains_amd/csrc/vs_graph.hip): a builder
from an edge list to a consistent CSR -- every edge one out-entry at its source and one in-entry at its target -- with
shuffled rows, permuted edge indices and free edge slots, and the cases the CPU and GPU tests share.  Expected values
come from tests/graph_refresh_model.py; the decision zoo also carries its expectations written out by construction."""
from collections import namedtuple

import numpy as np

from vstrains_amd.graph.asm_graph import AsmGraph

Csr = namedtuple("Csr", "row_ptr n_out nbr eidx dp vertex_black edge_black n_edge_slots edge_index")


def arrays(c):
    """The arguments of ``refresh_model`` / ``HipGraphOps.refresh_csr``."""
    return c.row_ptr, c.n_out, c.nbr, c.eidx, c.dp, c.vertex_black, c.edge_black, c.n_edge_slots


def build_csr(nv, edges, dp, vertex_black=None, shuffle_seed=None, permute_seed=None, free_slots=0, pinned=None):
    """``edges``: (src, tgt, black) in creation order.  Without options row v holds its out-entries, then its in-entries,
    both in creation order, and edge i has index i.  ``shuffle_seed``: every row's out-part and in-part are shuffled
    (each within itself); ``permute_seed``: the edges take distinct random indices below ``len(edges) + free_slots``, the
    others stay free (their colour is black: nothing may look at it); ``pinned``: {edge number: index} fixed in that
    draw."""
    ne = len(edges)
    n_slots = ne + free_slots
    if permute_seed is None:
        index = np.arange(ne, dtype=np.int64)
        assert not pinned
    else:
        pinned = dict(pinned or {})
        taken = set(pinned.values())
        rest = [k for k in np.random.default_rng(permute_seed).permutation(n_slots).tolist() if k not in taken]
        index = np.zeros(ne, dtype=np.int64)
        for i in range(ne):
            index[i] = pinned[i] if i in pinned else rest.pop()
    assert len(set(index.tolist())) == ne and (ne == 0 or int(index.max()) < n_slots)
    outs = [[] for _ in range(nv)]
    ins = [[] for _ in range(nv)]
    for i, (s, t, _) in enumerate(edges):
        outs[s].append((t, int(index[i])))
        ins[t].append((s, int(index[i])))
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        for part in (outs, ins):
            for v in range(nv):
                if len(part[v]) > 1:
                    part[v] = [part[v][k] for k in rng.permutation(len(part[v])).tolist()]
    n_out = np.asarray([len(r) for r in outs], dtype=np.uint32)
    row_ptr = np.zeros(nv + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum([len(outs[v]) + len(ins[v]) for v in range(nv)], dtype=np.uint64)
    flat = [x for v in range(nv) for x in outs[v] + ins[v]]
    nbr = np.asarray([x[0] for x in flat], dtype=np.uint32)
    eidx = np.asarray([x[1] for x in flat], dtype=np.uint32)
    edge_black = np.ones(max(n_slots, 1), dtype=np.uint8)
    for i, (_, _, black) in enumerate(edges):
        edge_black[index[i]] = 1 if black else 0
    vb = np.ones(nv, dtype=np.uint8) if vertex_black is None else np.asarray(vertex_black, dtype=np.uint8)
    return Csr(row_ptr, n_out, nbr, eidx, np.asarray(dp, dtype=np.float64), vb, edge_black, n_slots, index)


def build_csr_arrays(nv, src, tgt, dp, shuffle_seed):
    """``build_csr`` for the large all-black cases, on numpy arrays: edge i = src[i] -> tgt[i] with index i, every row's
    out-part and in-part in a seeded random order."""
    rng = np.random.default_rng(shuffle_seed)
    ne = len(src)
    e = np.arange(ne, dtype=np.int64)
    key = rng.random(2 * ne)
    owner = np.concatenate([src, tgt]).astype(np.int64)
    side = np.concatenate([np.zeros(ne, dtype=np.int64), np.ones(ne, dtype=np.int64)])  # out-entries before in-entries
    order = np.lexsort((key, side, owner))
    nbr = np.concatenate([tgt, src])[order].astype(np.uint32)
    eidx = np.concatenate([e, e])[order].astype(np.uint32)
    n_out = np.bincount(src, minlength=nv).astype(np.uint32)
    row_ptr = np.zeros(nv + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum(np.bincount(owner, minlength=nv), dtype=np.uint64)
    return Csr(row_ptr, n_out, nbr, eidx, np.asarray(dp, dtype=np.float64), np.ones(nv, dtype=np.uint8),
               np.ones(max(ne, 1), dtype=np.uint8), ne, e)


def asm_graph(nv, edges, dp):
    """The same graph as an ``AsmGraph`` (what the stage handle can hold): all vertices and edges black, no pair twice.
    -> (graph, node map, edge map)."""
    assert all(black for _, _, black in edges) and len({(s, t) for s, t, _ in edges}) == len(edges)
    g = AsmGraph()
    for v in range(nv):
        g.add_vertex(str(v), float(dp[v]), "ACGT", True)
    emap = {}  # (in creation order: a re-initialised stage graph then keeps every row's creation order)
    for s, t, _ in edges:
        emap[(g.vid[s], g.vid[t])] = g.add_edge(s, t, 21, 0.0, True)
    nodes = {g.vid[v]: v for v in range(nv)}
    return g, nodes, emap


# ---------------------------------------------------------------------------------------------------------------------
# (a) the decision zoo
# ---------------------------------------------------------------------------------------------------------------------
class _Zoo:
    def __init__(self):
        self.edges = []
        self.gray_vertices = []
        self.n = 0
        self.centres = {}  # gadget name -> (centre, nontrivial, fork_kind, chain_next)
        self.chain = {}    # vertex -> (chain_next, chain_top, chain_rank or None on a ring)

    def vertex(self, black=True):
        self.n += 1
        if not black:
            self.gray_vertices.append(self.n - 1)
        return self.n - 1

    def edge(self, s, t, black=True):
        self.edges.append((s, t, black))

    def star(self, name, n_in, n_out, shared, expect, gray_in=0, gray_out=0, self_loop=False, centre_black=True):
        """A centre with private neighbours: ``n_in`` black in-edges and ``n_out`` black out-edges, of which ``shared``
        neighbours have both; ``gray_in`` / ``gray_out`` gray edges more; ``expect`` = (nontrivial, fork_kind, does the
        centre have a simple out-edge to its one out-neighbour)."""
        c = self.vertex(centre_black)
        first_out = None
        for k in range(shared):
            x = self.vertex()
            self.edge(x, c)
            self.edge(c, x)
            first_out = x if first_out is None else first_out
        for k in range(n_in - shared):
            self.edge(self.vertex(), c)
        for k in range(n_out - shared):
            x = self.vertex()
            self.edge(c, x)
            first_out = x if first_out is None else first_out
        for k in range(gray_in):
            self.edge(self.vertex(), c, False)
        for k in range(gray_out):
            self.edge(c, self.vertex(), False)
        if self_loop:
            self.edge(c, c)
        nontrivial, fork, simple = expect
        self.centres[name] = (c, nontrivial, fork, first_out if simple else -1)
        return c


def _zoo():
    z = _Zoo()
    # black in / black out / shared                (nontrivial, fork_kind, simple out-edge)
    z.star("1/1/0", 1, 1, 0, (0, 0, True))
    z.star("2/1/0", 2, 1, 0, (0, 2, True))
    z.star("1/2/0", 1, 2, 0, (0, 1, False))
    z.star("2/2/0", 2, 2, 0, (1, 0, False))
    z.star("2/2/1", 2, 2, 1, (1, 0, False))
    z.star("3/3/2", 3, 3, 2, (1, 0, False))
    z.star("4/4/3", 4, 4, 3, (1, 0, False))
    z.star("2/2/2", 2, 2, 2, (0, 0, False))
    z.star("3/2/2", 3, 2, 2, (0, 0, False))
    z.star("2/3/2", 2, 3, 2, (0, 0, False))
    z.star("3/3/3", 3, 3, 3, (0, 0, False))
    z.star("2 black + 1 gray in, 2 out", 2, 2, 0, (1, 0, False), gray_in=1)
    z.star("1 black + 1 gray in, 2 out", 1, 2, 0, (0, 1, False), gray_in=1)
    z.star("1 in, 1 black + 2 gray out", 1, 1, 0, (0, 0, False), gray_out=2)  # out-degree 3: no simple edge
    z.star("self-loop + 1 in + 1 out", 1, 1, 0, (1, 0, False), self_loop=True)  # (the loop is an in- and an out-edge)
    z.star("self-loop + 2 in + 2 out", 2, 2, 0, (1, 0, False), self_loop=True)
    c = z.star("self-loop alone", 0, 0, 0, (0, 0, False), self_loop=True)
    z.chain[c] = (-1, c, 0)
    z.star("gray centre, 1 in, 2 out", 1, 2, 0, (0, 0, False), centre_black=False)
    # a -> c twice and c -> a twice: the shared neighbour counts once (2 > 1); counted per edge it would be 2 > 2
    a, c = z.vertex(), z.vertex()
    for _ in range(2):
        z.edge(a, c)
        z.edge(c, a)
    z.centres["parallel edges both ways"] = (c, 1, 0, -1)
    # a -> c black, c -> a gray, one more in, two more out: a gray return is not shared
    a, c = z.vertex(), z.vertex()
    z.edge(a, c)
    z.edge(c, a, False)
    z.edge(z.vertex(), c)
    z.edge(c, z.vertex())
    z.edge(c, z.vertex())
    z.centres["gray return"] = (c, 1, 0, -1)
    # the same with both in-neighbours returned to by gray edges: were those shared, 2 > 2 would fail
    a, b, c = z.vertex(), z.vertex(), z.vertex()
    z.edge(a, c)
    z.edge(b, c)
    z.edge(c, a, False)
    z.edge(c, b, False)
    z.edge(c, z.vertex())
    z.edge(c, z.vertex())
    z.centres["two gray returns"] = (c, 1, 0, -1)
    # chain gadgets: vertex -> (chain_next, chain_top, chain_rank)
    a, b = z.vertex(), z.vertex()  # a simple edge
    z.edge(a, b)
    z.chain[a], z.chain[b] = (b, a, 0), (-1, a, 1)
    a, b, x = z.vertex(), z.vertex(), z.vertex()  # the target's second in-edge is gray: not simple
    z.edge(a, b)
    z.edge(x, b, False)
    z.chain[a], z.chain[b], z.chain[x] = (-1, a, 0), (-1, b, 0), (-1, x, 0)
    a, b, y = z.vertex(), z.vertex(), z.vertex()  # the source's second out-edge is gray: not simple
    z.edge(a, b)
    z.edge(a, y, False)
    z.chain[a], z.chain[b], z.chain[y] = (-1, a, 0), (-1, b, 0), (-1, y, 0)
    a, b = z.vertex(), z.vertex()  # a ring of two
    z.edge(a, b)
    z.edge(b, a)
    z.chain[a], z.chain[b] = (b, None, -1), (a, None, -1)
    a, b, c = z.vertex(), z.vertex(), z.vertex()  # a path of three
    z.edge(a, b)
    z.edge(b, c)
    z.chain[a], z.chain[b], z.chain[c] = (b, a, 0), (c, a, 1), (-1, a, 2)
    return z


ZOO = _zoo()
assert ZOO.n < 255
ZOO_SIZES = (ZOO.n, 255, 256, 257, 512, 513)


def assert_zoo_expectations(got, off):
    """``got``: a mapping with the arrays nontrivial / fork_kind / chain_next / chain_top / chain_rank of a graph that holds
    the zoo from vertex ``off`` on: what the gadgets were built to give."""
    for name, (c, nontrivial, fork, nxt) in ZOO.centres.items():
        v = c + off
        assert (int(got["nontrivial"][v]), int(got["fork_kind"][v])) == (nontrivial, fork), name
        assert int(got["chain_next"][v]) == (nxt + off if nxt >= 0 else -1), name
    for c, (nxt, top, rank) in ZOO.chain.items():
        v = c + off
        assert int(got["chain_next"][v]) == (nxt + off if nxt >= 0 else -1), c
        assert int(got["chain_rank"][v]) == rank, c
        if rank >= 0:
            assert int(got["chain_top"][v]) == top + off, c


def zoo_case(nv=None, plain=False):
    """The zoo at the END of a graph of ``nv`` vertices (isolated ones in front), rows shuffled, edge indices permuted,
    3 slots free.  -> (Csr, offset of the zoo's vertex numbers).  ``plain``: no shuffle, no permutation, no free slot."""
    nv = ZOO.n if nv is None else nv
    off = nv - ZOO.n
    edges = [(s + off, t + off, black) for s, t, black in ZOO.edges]
    dp = np.random.default_rng(nv).uniform(0.5, 2000.0, nv)
    vb = np.ones(nv, dtype=np.uint8)
    vb[[v + off for v in ZOO.gray_vertices]] = 0
    if plain:
        return build_csr(nv, edges, dp, vb), off
    return build_csr(nv, edges, dp, vb, shuffle_seed=1000 + nv, permute_seed=2000 + nv, free_slots=3), off


# ---------------------------------------------------------------------------------------------------------------------
# (b) sum degrees.  SUM_SEEDS[d]: the first seed s = 0, 1, 2, ... whose d values default_rng(s).uniform(0.001, 5000, d) have
# a numpy.sum different from EVERY variant of graph_refresh_model.SUM_VARIANTS that is shaped differently at d addends
# (found by search with numpy 2.2.6; tests/test_graph_refresh_cases_cpu.py checks the property where it runs).  Most degrees
# need a handful of seeds; 1025 needed 152 and 4097 needed 66, because four variants are shaped differently there at once
# (left_to_right, linear_combine and BOTH leaf_127 and leaf_129: 1025 = 512 + 513 splits down to leaves of 128 and of 129)
# and one seed has to tell all of them from numpy's sum.
# ---------------------------------------------------------------------------------------------------------------------
SUM_SEEDS = {0: 0, 1: 0, 3: 0, 7: 0, 8: 2, 9: 4, 15: 10, 16: 2, 17: 2, 127: 0, 128: 18, 129: 16, 135: 23, 136: 1, 137: 0,
             255: 10, 256: 2, 257: 20, 264: 18, 272: 1, 273: 1, 300: 0, 511: 7, 512: 2, 513: 1, 1000: 33, 1025: 152, 2049: 1,
             4097: 66}
DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 264, 272, 273, 511, 512, 513, 1000, 1025,
           2049, 4097)
#: (out-degree, in-degree) of the hub
HUBS = [(d, 0) for d in DEGREES] + [(0, d) for d in DEGREES if d] + [(129, 3), (129, 257)]


HUB_DP = 987654321.0


def sum_values(d):
    return np.random.default_rng(SUM_SEEDS[d]).uniform(0.001, 5000.0, d)


def hub_parts(n_out, n_in, first=0, nv=None):
    """One hub (vertex ``first``) with ``n_out`` out-neighbours and ``n_in`` in-neighbours of its own, the vertices after
    it in a scattered order.  The k-th neighbour of a side IN ADJACENCY ORDER has dp ``sum_values(degree)[k]``, so the
    hub's neighbour sum is the sum the seed was chosen for.  The sums themselves are no output: they show in the flows
    only.  A leaf's other sum is the hub's dp alone, so its edge has flow (leaf + (leaf / sum) * hub) / 2, and the hub's dp
    is large so that the term with the sum carries the result -- with a hub of the leaves' size a last-place difference of
    the sum is rounded away in most edges, and in ALL edges of some degrees.  -> (edges, {vertex: dp})."""
    ids = (first + 1 + np.random.default_rng(n_out * 7919 + n_in).permutation(n_out + n_in)).tolist()
    edges, dp = [], {first: HUB_DP}
    for k, val in enumerate(sum_values(n_out).tolist()):
        edges.append((first, ids[k], True))
        dp[ids[k]] = val
    for k, val in enumerate(sum_values(n_in).tolist()):
        edges.append((ids[n_out + k], first, True))
        dp[ids[n_out + k]] = val
    return edges, dp


def hub_case(n_out, n_in):
    """-> (Csr with permuted edge indices and 2 free slots, rows in creation order; nv; edges; dp)."""
    edges, dpd = hub_parts(n_out, n_in)
    nv = 1 + n_out + n_in
    dp = np.asarray([dpd[v] for v in range(nv)], dtype=np.float64)
    return build_csr(nv, edges, dp, permute_seed=n_out + 3 * n_in, free_slots=2), nv, edges, dp


# ---------------------------------------------------------------------------------------------------------------------
# (c) many listed vertices: h hubs of 129 out-edges each to ONE pool of 129 leaves; above 128 hubs the leaves are listed too
# ---------------------------------------------------------------------------------------------------------------------
POOL = 129
#: hubs -> vertices with more than 128 neighbours on a side
LISTED = {1: 1, 64: 64, 65: 65, 3966: 4095, 3967: 4096, 3968: 4097}


def many_hubs_case(h):
    nv = h + POOL
    src = np.repeat(np.arange(h, dtype=np.int64), POOL)
    tgt = np.tile(np.arange(h, h + POOL, dtype=np.int64), h)
    dp = np.random.default_rng(h).uniform(0.001, 5000.0, nv)
    c = build_csr_arrays(nv, src, tgt, dp, shuffle_seed=h + 1)
    deg_in = (c.row_ptr[1:] - c.row_ptr[:-1]).astype(np.int64) - c.n_out.astype(np.int64)
    assert int(((c.n_out > 128) | (deg_in > 128)).sum()) == LISTED[h]
    return c


# ---------------------------------------------------------------------------------------------------------------------
# (d) zero sums
# ---------------------------------------------------------------------------------------------------------------------
ZERO_EDGES = (700, 5, 3)


def zero_sum_case(with_zero_sums=True):
    """About 700 vertices.  ``with_zero_sums``: three edges would divide by zero, with indices 700 (row of vertex 0:
    out_sum == 0, its only target has dp 0), 5 (row of vertex 520, the same) and 3 (row of vertex 600, whose dp is 0 and
    which is the only in-neighbour of its target: in_sum == 0 while its out_sum is positive).  Otherwise: no zero sum, but
    vertex 650 has dp 0 between neighbours that have other neighbours -- its two flows are exactly 0.0.
    dp is 0 or within [1e-3, 1e6]."""
    nv = 700
    rng = np.random.default_rng(41 if with_zero_sums else 42)
    dp = 10.0 ** rng.uniform(-3.0, 6.0, nv)
    seen, edges = set(), []
    while len(edges) < 760:  # a random remainder among vertices 1 .. 499, all dp positive
        s, t = int(rng.integers(1, 500)), int(rng.integers(1, 500))
        if (s, t) not in seen:
            seen.add((s, t))
            edges.append((s, t, True))
    pinned = {}
    if with_zero_sums:
        for s, t, zero, index in ((0, 510, 510, 700), (520, 521, 521, 5), (600, 601, 600, 3)):
            dp[zero] = 0.0
            pinned[len(edges)] = index
            edges.append((s, t, True))
    else:
        dp[650] = 0.0
        edges += [(651, 650, True), (651, 652, True), (650, 653, True), (654, 653, True)]
    return build_csr(nv, edges, dp, shuffle_seed=7, permute_seed=8, free_slots=3, pinned=pinned), edges


# ---------------------------------------------------------------------------------------------------------------------
# (e) a sequence of graphs for ONE stage handle: all black, no pair twice
# ---------------------------------------------------------------------------------------------------------------------
def _with_remainder(nv, hubs, seed):
    """Hubs (out-degree, in-degree) one after the other, then a sparse remainder of chains and small forks up to nv."""
    edges, dp, first = [], {}, 0
    for n_out, n_in in hubs:
        e, d = hub_parts(n_out, n_in, first)
        edges += e
        dp.update(d)
        first += 1 + n_out + n_in
    assert first <= nv
    rng = np.random.default_rng(seed)
    for v in range(first, nv):
        dp[v] = float(rng.uniform(0.001, 5000.0))
    for v in range(first, nv - 2, 3):
        edges.append((v, v + 1, True))
        if v % 2:
            edges.append((v, v + 2, True))
    return nv, edges, np.asarray([dp[v] for v in range(nv)], dtype=np.float64)


def sequence():
    """G1 (hubs of 129 and 257), G2 (no hub, more vertices and edges than G1), G3 (smaller, one hub of 300), G1 again."""
    g1 = _with_remainder(900, [(129, 129), (257, 257)], 1)
    g2 = _with_remainder(2600, [], 2)
    g3 = _with_remainder(400, [(300, 0)], 3)
    assert g2[0] > g1[0] and len(g2[1]) > len(g1[1]) and g3[0] < g1[0] and len(g3[1]) < len(g1[1])
    return [g1, g2, g3, g1]
