"""Reference model of ``vs_graph_refresh`` (include/vstrains_hip.h, "graph stages") on raw CSR arrays: what K6
(``k_vertex_scan``, ``k_vertex_sums_big``) and K7 (``k_edge_flow``) of vstrains_amd/csrc/vs_graph.hip have to compute,
stated from the reference's own lines and not from the kernels.

* neighbour sums are ``numpy.sum`` itself, called when the test runs (the installed numpy is the arbiter);
* flows are ``numpy.mean`` of the two products of utils/VStrains_Utilities.py:14-31, per edge, or the same arithmetic
  on whole float64 arrays (``vectorised=True``, for the large cases);
* ``nontrivial`` is ``is_non_trivial`` (Utilities.py:162-172), ``fork_kind`` the two tests of
  utils/VStrains_Decomposition.py:715,763, ``chain_next`` the simple-edge test of ``simp_path`` (Utilities.py:398-402),
  ``chain_top`` / ``chain_rank`` a walk along ``chain_next``.

The CSR: row v = entries ``row_ptr[v] .. row_ptr[v + 1]`` of ``nbr`` / ``eidx``; the first ``n_out[v]`` are out-entries
(target, edge index), the rest in-entries (source, edge index).

``VARIANTS`` names deliberate mistakes of the decisions and ``pairwise_sum`` restates numpy's summation order with
switchable mistakes: both exist to show that the cases tell a wrong implementation from a right one, never as the
expected value of a test."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

NO_EDGE = 0xFFFFFFFF

Refresh = namedtuple("Refresh", "flow nontrivial fork_kind chain_next chain_top chain_rank zero_sum_edge zero_set "
                                "out_sum in_sum")

#: deliberate mistakes of the decisions (``refresh_model(..., variant=name)``)
VARIANTS = ("gray_edges_counted", "shared_counted_per_edge", "greater_or_equal", "chain_on_black_degrees",
            "self_loop_is_simple", "fork_on_gray_vertex")


def neighbour_sums(row_ptr, n_out, nbr, dp):
    """(out_sum, in_sum): ``numpy.sum`` of the neighbours' dp in adjacency order (Utilities.py:20,23)."""
    nv = len(n_out)
    dp = np.asarray(dp, dtype=np.float64)
    out_sum = np.zeros(nv, dtype=np.float64)
    in_sum = np.zeros(nv, dtype=np.float64)
    for v in range(nv):
        lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
        mid = lo + int(n_out[v])
        out_sum[v] = np.sum(np.ascontiguousarray(dp[nbr[lo:mid]]))
        in_sum[v] = np.sum(np.ascontiguousarray(dp[nbr[mid:hi]]))
    return out_sum, in_sum


def _out_entries(row_ptr, n_out):
    """(source vertex, position in nbr / eidx) of every out-entry."""
    nv = len(n_out)
    src = np.repeat(np.arange(nv, dtype=np.int64), np.asarray(n_out, dtype=np.int64))
    starts = np.asarray(row_ptr[:nv], dtype=np.int64)
    first = np.cumsum(np.asarray(n_out, dtype=np.int64)) - np.asarray(n_out, dtype=np.int64)
    pos = starts[src] + (np.arange(src.size, dtype=np.int64) - first[src])
    return src, pos


def edge_flows(row_ptr, n_out, nbr, eidx, dp, out_sum, in_sum, n_edge_slots, vectorised=False):
    """(flow [n_edge_slots], sorted list of the edges that would divide by a zero sum).  Free slots and zero-sum edges
    read 0.0."""
    dp = np.asarray(dp, dtype=np.float64)
    flow = np.zeros(n_edge_slots, dtype=np.float64)
    src, pos = _out_entries(row_ptr, n_out)
    tgt = np.asarray(nbr, dtype=np.int64)[pos]
    e = np.asarray(eidx, dtype=np.int64)[pos]
    zero = (out_sum[src] == 0.0) | (in_sum[tgt] == 0.0)
    zero_set = sorted(set(e[zero].tolist()))
    ok = ~zero
    if vectorised:
        du, dv, os_, is_ = dp[src[ok]], dp[tgt[ok]], out_sum[src[ok]], in_sum[tgt[ok]]
        flow[e[ok]] = ((dv / os_) * du + (du / is_) * dv) / 2.0
    else:
        with np.errstate(all="raise"):
            for u, v, k in zip(src[ok].tolist(), tgt[ok].tolist(), e[ok].tolist()):
                flow[k] = np.mean([(dp[v] / out_sum[u]) * dp[u], (dp[u] / in_sum[v]) * dp[v]])
    return flow, zero_set


def fused_edge_flows(row_ptr, n_out, nbr, eidx, dp, out_sum, in_sum, n_edge_slots):
    """What a compiler that contracts ``a + b`` with the multiplication of ``a`` into one fused multiply-add would
    give: ``fma(dv / os, du, (du / is) * dv) / 2``, the product exact (rationals) and rounded once with the sum."""
    dp = np.asarray(dp, dtype=np.float64)
    flow = np.zeros(n_edge_slots, dtype=np.float64)
    src, pos = _out_entries(row_ptr, n_out)
    for u, p in zip(src.tolist(), pos.tolist()):
        v, k = int(nbr[p]), int(eidx[p])
        if out_sum[u] == 0.0 or in_sum[v] == 0.0:
            continue
        x = float(dp[v] / out_sum[u])
        b = float((dp[u] / in_sum[v]) * dp[v])
        flow[k] = float(Fraction(x) * Fraction(float(dp[u])) + Fraction(b)) / 2
    return flow


def decisions(row_ptr, n_out, nbr, eidx, vertex_black, edge_black, variant=None):
    """(nontrivial u8, fork_kind u8, chain_next i32) of every vertex."""
    assert variant is None or variant in VARIANTS, variant
    nv = len(n_out)
    eb = np.asarray(edge_black).astype(bool)
    if variant == "gray_edges_counted":
        eb = np.ones_like(eb)
    row = np.asarray(row_ptr, dtype=np.int64)
    deg_out = np.asarray(n_out, dtype=np.int64)
    deg_in = (row[1:] - row[:-1]) - deg_out
    nontrivial = np.zeros(nv, dtype=np.uint8)
    fork = np.zeros(nv, dtype=np.uint8)
    nxt = np.full(nv, -1, dtype=np.int32)
    for v in range(nv):
        lo, hi = int(row[v]), int(row[v + 1])
        mid = lo + int(deg_out[v])
        us = nbr[mid:hi][eb[eidx[mid:hi]]].tolist()  # sources of the black in-edges
        ws = nbr[lo:mid][eb[eidx[lo:mid]]].tolist()  # targets of the black out-edges
        if variant == "shared_counted_per_edge":
            both = sum(1 for u in us if u in set(ws))
        else:
            both = len(set(us) & set(ws))
        if variant == "greater_or_equal":
            nontrivial[v] = len(us) >= max(both, 1) and len(ws) >= max(both, 1)
        else:
            nontrivial[v] = len(us) > max(both, 1) and len(ws) > max(both, 1)
        if vertex_black[v] or variant == "fork_on_gray_vertex":
            if len(us) == 1 and len(ws) > 1:
                fork[v] = 1
            elif len(us) > 1 and len(ws) == 1:
                fork[v] = 2
        if variant == "chain_on_black_degrees":
            if len(ws) == 1:
                t = ws[0]
                t_lo, t_hi = int(row[t]) + int(deg_out[t]), int(row[t + 1])
                if int(eb[eidx[t_lo:t_hi]].sum()) == 1 and t != v:
                    nxt[v] = t
        elif deg_out[v] == 1:  # degrees count every edge, gray included
            t = int(nbr[lo])
            if deg_in[t] == 1 and (t != v or variant == "self_loop_is_simple"):
                nxt[v] = t
    return nontrivial, fork, nxt


def chains(chain_next):
    """(chain_top, chain_rank) by walking ``chain_next`` from every head (a vertex no simple edge enters).  A vertex no
    walk reaches lies on a ring of simple edges: rank -1, and its top is not defined (reported as the vertex itself)."""
    nv = len(chain_next)
    nxt = [int(x) for x in chain_next]
    entered = [False] * nv
    for v in range(nv):
        if nxt[v] >= 0:
            entered[nxt[v]] = True
    top = list(range(nv))
    rank = [-1] * nv
    for v in range(nv):
        if not entered[v]:
            cur, d = v, 0
            while cur >= 0:
                top[cur], rank[cur] = v, d
                cur, d = nxt[cur], d + 1
    return np.asarray(top, dtype=np.int32), np.asarray(rank, dtype=np.int32)


def refresh_model(row_ptr, n_out, nbr, eidx, dp, vertex_black, edge_black, n_edge_slots, vectorised=False, variant=None):
    nbr = np.asarray(nbr, dtype=np.int64)
    eidx = np.asarray(eidx, dtype=np.int64)
    out_sum, in_sum = neighbour_sums(row_ptr, n_out, nbr, dp)
    flow, zero_set = edge_flows(row_ptr, n_out, nbr, eidx, dp, out_sum, in_sum, n_edge_slots, vectorised=vectorised)
    nontrivial, fork, nxt = decisions(row_ptr, n_out, nbr, eidx, vertex_black, edge_black, variant=variant)
    top, rank = chains(nxt)
    return Refresh(flow, nontrivial, fork, nxt, top, rank, zero_set[0] if zero_set else NO_EDGE, zero_set, out_sum, in_sum)


def model_of_graph(g):
    """The model on an ``AsmGraph``'s own CSR (``csr_arrays()``), every vertex and edge black."""
    row_ptr, n_out, nbr, eidx = g.csr_arrays()
    return refresh_model(row_ptr, n_out, nbr, eidx, g.vdp, np.ones(g.num_vertices(), dtype=np.uint8),
                         np.ones(max(len(g.esrc), 1), dtype=np.uint8), len(g.esrc), vectorised=True)


def assert_scan_equals_model(scan, want, what):
    """``scan``: a ``GraphScan`` (lists per vertex); ``want``: the model's ``Refresh``.  The head of a ring is not defined."""
    assert scan.nontrivial == want.nontrivial.astype(bool).tolist(), what
    assert scan.fork_kind == want.fork_kind.tolist(), what
    assert scan.chain_next == want.chain_next.tolist(), what
    assert scan.chain_rank == want.chain_rank.tolist(), what
    for v, rank in enumerate(scan.chain_rank):
        if rank >= 0:
            assert scan.chain_top[v] == int(want.chain_top[v]), (what, v)


# ---------------------------------------------------------------------------------------------------------------------
# numpy's pairwise sum (numpy/_core/src/umath/loops_utils.h.src, @TYPE@_pairwise_sum), restated with its constants as
# arguments.  ``add`` may be replaced to record the shape of the sum instead of its value (``sum_shape``).
# ---------------------------------------------------------------------------------------------------------------------
#: name -> keyword arguments of ``pairwise_sum``: the mistakes the degree cases have to tell from numpy's order
SUM_VARIANTS = {
    "left_to_right": dict(sequential=True),
    "split_not_rounded": dict(round_split=False),
    "leaf_127": dict(leaf=127),
    "leaf_129": dict(leaf=129),
    "linear_combine": dict(linear_combine=True),
    "sequential_up_to_8": dict(small=9),
}


def pairwise_sum(a, leaf=128, round_split=True, small=8, linear_combine=False, sequential=False, add=None):
    """Sum of the sequence ``a`` in numpy's order: fewer than ``small`` addends one after the other; up to ``leaf``
    addends through eight accumulators combined as a tree, then the tail; more split at n / 2 rounded down to a multiple
    of 8 (``round_split``), halves summed the same way."""
    if add is None:
        add = lambda x, y: x + y
    n = len(a)
    if n == 0:
        return 0.0
    if sequential or n < small:
        res = a[0]  # (0.0 + a[0] is a[0])
        for i in range(1, n):
            res = add(res, a[i])
        return res
    if n <= leaf:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = add(r[j], a[i + j])
            i += 8
        if linear_combine:
            res = r[0]
            for j in range(1, 8):
                res = add(res, r[j])
        else:
            res = add(add(add(r[0], r[1]), add(r[2], r[3])), add(add(r[4], r[5]), add(r[6], r[7])))
        while i < n:
            res = add(res, a[i])
            i += 1
        return res
    n2 = n // 2
    if round_split:
        n2 -= n2 % 8
    kw = dict(leaf=leaf, round_split=round_split, small=small, linear_combine=linear_combine, add=add)
    return add(pairwise_sum(a[:n2], **kw), pairwise_sum(a[n2:], **kw))


def sum_shape(n, table, **kw):
    """The shape of the sum of n addends: addends are numbered 0 .. n - 1 and every distinct addition (left, right) gets
    the next number from ``table``, so two settings that share a table return the same number exactly when they perform
    the same additions in the same order -- no values can tell those apart."""
    return pairwise_sum(list(range(n)), add=lambda x, y: table.setdefault((x, y), n + len(table)), **kw)


def different_variants(n):
    """The names of ``SUM_VARIANTS`` whose sum of n addends is shaped differently from numpy's."""
    if n == 0:
        return []
    table = {}
    want = sum_shape(n, table)
    return [name for name, kw in SUM_VARIANTS.items() if sum_shape(n, table, **kw) != want]
