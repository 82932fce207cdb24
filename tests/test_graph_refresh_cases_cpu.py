"""The constructed cases of the vertex scan and edge flow kernels (tests/graph_refresh_cases.py) and their model
(tests/graph_refresh_model.py), checked without a GPU: the model returns the zoo's written-out expectations, every named
mistake of the model or of the summation order changes a value the cases look at, the model agrees with the numpy
checker (oracle/graph_ops.py) where both apply, and the CPU twin of the device operations (oracle/stage_check.cpp) passes
the stage-handle cases.  tests/test_graph_refresh_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

import graph_refresh_cases as cases
import graph_refresh_model as model
from oracle import graph_ops as chk
from vstrains_amd.graph.formats import stage_graph_from_state


@pytest.mark.parametrize("nv", cases.ZOO_SIZES)
def test_model_gives_the_zoo_expectations_written_out_by_construction(nv):
    for plain in (True, False):
        c, off = cases.zoo_case(nv, plain=plain)
        got = model.refresh_model(*cases.arrays(c))
        cases.assert_zoo_expectations(got._asdict(), off)
        assert not got.nontrivial[:off].any() and not got.fork_kind[:off].any() and (got.chain_next[:off] == -1).all()
        assert got.zero_sum_edge == model.NO_EDGE
        free = sorted(set(range(c.n_edge_slots)) - set(c.edge_index.tolist()))
        assert len(free) == (0 if plain else 3) and not got.flow[free].any()


@pytest.mark.parametrize("variant", model.VARIANTS)
def test_every_named_mistake_of_the_decisions_changes_a_zoo_value(variant):
    c, _ = cases.zoo_case()
    want = model.refresh_model(*cases.arrays(c))
    got = model.refresh_model(*cases.arrays(c), variant=variant)
    changed = [f for f in ("nontrivial", "fork_kind", "chain_next", "chain_rank") if not np.array_equal(getattr(want, f), getattr(got, f))]
    assert changed, variant


def test_pairwise_restatement_is_numpy_sum_and_every_differently_shaped_variant_differs():
    pairs = 0
    for d in sorted(cases.SUM_SEEDS):
        vals = cases.sum_values(d)
        want = float(np.sum(vals)) if d else 0.0
        assert model.pairwise_sum(vals.tolist()) == want, d
        for name in model.different_variants(d):
            assert model.pairwise_sum(vals.tolist(), **model.SUM_VARIANTS[name]) != want, (d, name)
            pairs += 1
    print("(degree, variant) pairs compared: %d" % pairs)
    assert pairs > 60
    # the shapes themselves: which mistakes can show at which degree
    assert model.different_variants(7) == []
    assert model.different_variants(8) == ["left_to_right", "linear_combine", "sequential_up_to_8"]
    assert "leaf_127" in model.different_variants(128) and "leaf_129" in model.different_variants(129)
    assert "split_not_rounded" not in model.different_variants(256)
    for d in (135, 136, 137, 255, 264, 272, 273, 511, 1000):
        assert "split_not_rounded" in model.different_variants(d), d
    assert set(cases.DEGREES) <= set(cases.SUM_SEEDS)


def test_hub_rows_hold_the_values_their_seed_was_chosen_for():
    for n_out, n_in in cases.HUBS:
        c, _, _, _ = cases.hub_case(n_out, n_in)
        row = c.nbr[int(c.row_ptr[0]):int(c.row_ptr[1])]
        assert np.array_equal(c.dp[row[:n_out]], cases.sum_values(n_out)) and np.array_equal(c.dp[row[n_out:]], cases.sum_values(n_in))


def test_a_differently_shaped_sum_shows_in_the_flows_of_its_hub():
    """The sums are no output of ``vs_graph_refresh``: a hub case bites only if the other sum changes a flow."""
    pairs = 0
    for n_out, n_in in cases.HUBS:
        c, _, _, _ = cases.hub_case(n_out, n_in)
        want = model.refresh_model(*cases.arrays(c), vectorised=True)
        for side, d in (("out", n_out), ("in", n_in)):
            vals = cases.sum_values(d).tolist()
            for name in model.different_variants(d):
                out_sum, in_sum = want.out_sum.copy(), want.in_sum.copy()
                (out_sum if side == "out" else in_sum)[0] = model.pairwise_sum(vals, **model.SUM_VARIANTS[name])
                flow, _ = model.edge_flows(c.row_ptr, c.n_out, c.nbr, c.eidx, c.dp, out_sum, in_sum, c.n_edge_slots, vectorised=True)
                assert (flow != want.flow).any(), (n_out, n_in, side, name)
                pairs += 1
    print("(hub, side, variant) triples whose flows differ: %d" % pairs)
    assert pairs > 120


def small_cases():
    yield cases.zoo_case()[0]
    yield cases.zoo_case(257)[0]
    for hub in ((0, 0), (7, 0), (0, 9), (129, 3), (137, 0)):
        yield cases.hub_case(*hub)[0]
    yield cases.many_hubs_case(1)
    yield cases.zero_sum_case(True)[0]
    yield cases.zero_sum_case(False)[0]


def test_per_edge_and_vectorised_flows_agree_and_a_fused_multiply_add_would_show():
    for c in small_cases():
        a = model.refresh_model(*cases.arrays(c))
        b = model.refresh_model(*cases.arrays(c), vectorised=True)
        assert a.flow.tobytes() == b.flow.tobytes() and a.zero_set == b.zero_set
    c, _ = cases.zoo_case()
    a = model.refresh_model(*cases.arrays(c))
    fused = model.fused_edge_flows(c.row_ptr, c.n_out, c.nbr, c.eidx, c.dp, a.out_sum, a.in_sum, c.n_edge_slots)
    assert int((fused != a.flow).sum()) >= 1


def test_zero_sum_cases_are_what_they_claim():
    c, edges = cases.zero_sum_case(True)
    got = model.refresh_model(*cases.arrays(c))
    assert got.zero_set == sorted(cases.ZERO_EDGES) and got.zero_sum_edge == 3
    rows = {int(c.edge_index[i]): edges[i][0] for i in range(len(edges))}
    assert [rows[e] for e in cases.ZERO_EDGES] == [0, 520, 600]
    assert got.out_sum[0] == 0.0 and got.out_sum[520] == 0.0 and got.in_sum[601] == 0.0 and got.out_sum[600] > 0.0
    c, edges = cases.zero_sum_case(False)
    got = model.refresh_model(*cases.arrays(c))
    assert got.zero_set == [] and c.dp[650] == 0.0
    through = [int(c.edge_index[i]) for i, (s, t, _) in enumerate(edges) if 650 in (s, t)]
    assert len(through) == 2 and not got.flow[through].any()
    others = sorted(set(c.edge_index.tolist()) - set(through))
    assert (got.flow[others] > 0.0).all()
    for c in (cases.zero_sum_case(True)[0], cases.zero_sum_case(False)[0]):
        assert ((c.dp == 0.0) | ((c.dp >= 1e-3) & (c.dp <= 1e6))).all()


def asm_cases():
    for n_out, n_in in cases.HUBS:
        _, nv, edges, dp = cases.hub_case(n_out, n_in)
        yield "hub %d/%d" % (n_out, n_in), nv, edges, dp
    for k, (nv, edges, dp) in enumerate(cases.sequence()[:3]):
        yield "sequence G%d" % (k + 1), nv, edges, dp


def test_model_agrees_with_the_numpy_checker_where_both_apply():
    for what, nv, edges, dp in asm_cases():
        g, _, _ = cases.asm_graph(nv, edges, dp)
        want = model.model_of_graph(g)
        scan = chk.NumpyGraphOps().refresh(g)
        model.assert_scan_equals_model(scan, want, what)
        assert g.eflow == want.flow.tolist(), what


def test_cpu_twin_of_the_device_operations_on_the_stage_handle_cases(tmp_path):
    """One handle over oracle/stage_check.cpp takes the hub graphs and the sequence one after the other."""
    import native_check

    st = native_check.stage_over_checker(["x"], np.zeros((1, 1), dtype=np.int64))
    for what, nv, edges, dp in list(asm_cases()) + [("sequence G1 again",) + cases.sequence()[3]]:
        g, nodes, emap = cases.asm_graph(nv, edges, dp)
        want = model.model_of_graph(stage_graph_from_state(g, nodes, emap)[0])
        st.load_graph(g, nodes, emap)
        st.reinit(str(tmp_path / "g.gfa"))
        assert st.graph()[0].eflow == want.flow.tolist(), what
        model.assert_scan_equals_model(st.scan(), want, what)
    st.close()
