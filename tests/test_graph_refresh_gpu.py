"""K6 (``k_vertex_scan``, ``k_vertex_sums_big``) and K7 (``k_edge_flow``) of vstrains_amd/csrc/vs_graph.hip on constructed
adjacency rows (tests/graph_refresh_cases.py), through ``vs_graph_refresh`` on raw CSR arrays and through the stage
handle, against the model of tests/graph_refresh_model.py: integers exactly, fp64 flows bit for bit.
tests/test_graph_refresh_cases_cpu.py shows without a GPU that the cases tell the named mistakes apart."""
import functools

import numpy as np
import pytest

import graph_refresh_cases as cases
import graph_refresh_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    from vstrains_amd.graph.hip_ops import HipBackend

    return HipBackend(0)


@pytest.fixture(scope="module")
def ops(backend):
    return backend.graph_ops


def assert_equals_model(got, want, nv):
    """``got``: what ``refresh_csr`` returned (any subset of the outputs); ``want``: the model's ``Refresh``."""
    for name in ("nontrivial", "fork_kind", "chain_next", "chain_rank"):
        if name in got:
            assert got[name].dtype == getattr(want, name).dtype
            bad = np.flatnonzero(got[name][:nv] != getattr(want, name))
            assert bad.size == 0, (name, bad[:8].tolist(), got[name][bad[:8]].tolist(), getattr(want, name)[bad[:8]].tolist())
    if "chain_top" in got and "chain_rank" in got:
        on_chain = want.chain_rank >= 0  # (the head of a ring is not defined)
        assert np.array_equal(got["chain_top"][:nv][on_chain], want.chain_top[on_chain])
    if "zero_sum_edge" in got:
        assert got["zero_sum_edge"] == want.zero_sum_edge
    if "flow" in got:
        a, b = got["flow"][:want.flow.size], want.flow
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))  # bit for bit; free slots and zero-sum edges read +0.0
        assert bad.size == 0, ("flow", bad[:8].tolist(), a[bad[:8]].tolist(), b[bad[:8]].tolist())


@functools.lru_cache(maxsize=None)
def zoo(nv):
    c, off = cases.zoo_case(nv)
    return c, off, model.refresh_model(*cases.arrays(c))


def assert_zoo_call_is_right(ops, nv=257):
    c, off, want = zoo(nv)
    assert_equals_model(ops.refresh_csr(*cases.arrays(c)), want, nv)


# ---- (a) the decision zoo ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", cases.ZOO_SIZES)
def test_decision_zoo_at_the_end_of_the_last_workgroup(ops, nv):
    c, off, want = zoo(nv)
    got = ops.refresh_csr(*cases.arrays(c))
    assert_equals_model(got, want, nv)
    cases.assert_zoo_expectations(got, off)  # ... and what the gadgets were built to give
    free = sorted(set(range(c.n_edge_slots)) - set(c.edge_index.tolist()))
    assert len(free) == 3 and got["flow"][free].tobytes() == bytes(24)


# ---- (b) sum degrees -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out,n_in", cases.HUBS)
def test_neighbour_sums_of_a_hub_follow_numpy_order(ops, n_out, n_in):
    c, nv, _, _ = cases.hub_case(n_out, n_in)
    want = model.refresh_model(*cases.arrays(c), vectorised=True)
    got = ops.refresh_csr(*cases.arrays(c))
    assert_equals_model(got, want, nv)
    free = sorted(set(range(c.n_edge_slots)) - set(c.edge_index.tolist()))
    assert len(free) == 2 and got["flow"][free].tobytes() == bytes(16)


# ---- (c) many listed vertices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hubs", sorted(cases.LISTED))
def test_many_rows_of_more_than_128_neighbours(ops, hubs):
    """64 x 64 threads stride over the listed rows: 4095 / 4096 / 4097 of them are the last without a second turn, a full
    grid, and the first second turn."""
    c = cases.many_hubs_case(hubs)
    want = model.refresh_model(*cases.arrays(c), vectorised=True)
    assert_equals_model(ops.refresh_csr(*cases.arrays(c)), want, len(c.n_out))


# ---- (d) zero sums -------------------------------------------------------------------------------------------------
def test_smallest_zero_sum_edge_among_several_workgroups(ops):
    c, _ = cases.zero_sum_case(True)
    want = model.refresh_model(*cases.arrays(c))
    assert want.zero_set == sorted(cases.ZERO_EDGES)
    got = ops.refresh_csr(*cases.arrays(c))
    assert got["zero_sum_edge"] == 3
    assert_equals_model(got, want, len(c.n_out))  # (the three edges themselves read 0.0)
    assert got["flow"][want.zero_set].tobytes() == bytes(24)


def test_vertex_of_depth_zero_without_a_zero_sum(ops):
    c, edges = cases.zero_sum_case(False)
    want = model.refresh_model(*cases.arrays(c))
    got = ops.refresh_csr(*cases.arrays(c))
    assert got["zero_sum_edge"] == model.NO_EDGE
    assert_equals_model(got, want, len(c.n_out))
    through = [int(c.edge_index[i]) for i, (s, t, _) in enumerate(edges) if 650 in (s, t)]
    assert len(through) == 2 and got["flow"][through].tobytes() == bytes(16)


# ---- NULL outputs and refusals -------------------------------------------------------------------------------------
def test_any_output_pointer_may_be_null(ops):
    from vstrains_amd.graph.hip_ops import HipGraphOps

    c, off, want = zoo(257)
    full = ops.refresh_csr(*cases.arrays(c))
    for asked in [(name,) for name in HipGraphOps.OUTPUTS] + [()]:
        got = ops.refresh_csr(*cases.arrays(c), outputs=asked)
        assert sorted(got) == sorted(asked)
        for name in asked:
            if name == "zero_sum_edge":
                assert got[name] == full[name]
            else:
                assert got[name].tobytes() == full[name].tobytes(), name
        assert_zoo_call_is_right(ops)


def test_malformed_and_out_of_range_rows_are_refused(ops):
    from vstrains_amd import _native as nat

    c, off, _ = zoo(257)
    v = off + 3  # a vertex of the zoo with a row
    assert c.row_ptr[v + 1] > c.row_ptr[v]

    def changed(field, at, value):
        a = getattr(c, field).copy()
        a[at] = value
        return c._replace(**{field: a})

    first = int(c.row_ptr[v])
    refused = [
        ("n_out larger than the row", changed("n_out", v, int(c.row_ptr[v + 1] - c.row_ptr[v]) + 1), nat.VS_E_ARG),
        ("decreasing row_ptr", changed("row_ptr", v + 1, first - 1), nat.VS_E_ARG),
        ("no nbr", c._replace(nbr=None), nat.VS_E_ARG),
        ("no eidx", c._replace(eidx=None), nat.VS_E_ARG),
        ("no edge_black", c._replace(edge_black=None), nat.VS_E_ARG),
        ("nbr == nv", changed("nbr", first, 257), nat.VS_E_RANGE),
        ("eidx == n_edge_slots", changed("eidx", first, c.n_edge_slots), nat.VS_E_RANGE),
        ("last eidx far out", changed("eidx", -1, 0xFFFFFFFF), nat.VS_E_RANGE),
    ]
    assert first >= 1 and c.row_ptr[v] >= c.row_ptr[v - 1]  # (the decreased entry is below its predecessor only)
    for what, bad, code in refused:
        with pytest.raises(nat.NativeError) as err:
            ops.refresh_csr(*cases.arrays(bad))
        assert err.value.code == code, what
        assert_zoo_call_is_right(ops)


# ---- (e) one stage handle, graph after graph ------------------------------------------------------------------------
def test_one_stage_handle_takes_a_sequence_of_graphs(backend, tmp_path):
    """Buffers kept and regrown, the counter of listed rows reset only for graphs that have one: hubs, then a larger graph
    without, then a smaller one with a hub, then the first again."""
    from vstrains_amd.graph.formats import stage_graph_from_state
    from vstrains_amd.graph.hip_ops import HipPeLinks
    from vstrains_amd.graph.native_stage import NativeStage

    table = HipPeLinks.from_matrices(backend.ctx, ["x"], np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1), dtype=np.int64))
    st = NativeStage.on_device(backend.ctx, table, table.names)
    for k, (nv, edges, dp) in enumerate(cases.sequence()):
        g, nodes, emap = cases.asm_graph(nv, edges, dp)
        want = model.model_of_graph(stage_graph_from_state(g, nodes, emap)[0])
        st.load_graph(g, nodes, emap)
        st.reinit(str(tmp_path / "g.gfa"))
        assert st.graph()[0].eflow == want.flow.tolist(), k
        model.assert_scan_equals_model(st.scan(), want, k)
    st.close()
