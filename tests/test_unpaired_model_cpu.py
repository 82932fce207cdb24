"""tests/unpaired_model.py tied to the oracle's whole path, and tests/unpaired_cases.py shown to hold what the GPU test
needs them to hold.  No device."""
import numpy as np
import pytest

import unpaired_cases as uc
from oracle import pe_oracle


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_model_is_half_of_a_read_paired_with_itself(graph):
    """For reads without N and of length >= k+1, a pair (S, S) adds S's triangle to short_mat once per end:
    pe_matrices(S, S).short_mat == 2 * model(S).short_mat; the model's node_mat is zero."""
    g = uc.GRAPHS[graph]()
    K = g.k + 1
    reads = [s for s in uc.block(graph, 77) if not s.count("N") and len(s) >= K]
    assert len(reads) > 60
    _, want_short, want_stats = pe_oracle.pe_matrices(g.seqs, reads, reads, g.k, table=g.model.table)
    node_mat, short_mat, tallies = g.model.count(reads)
    assert want_stats == (0, 0, len(reads)) and tallies == (0, 0, len(reads))
    assert int(short_mat.sum()) > 0
    assert np.array_equal(want_short, 2 * short_mat)
    assert not node_mat.any()


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_tallies_follow_the_rules_in_their_order(graph):
    g = uc.GRAPHS[graph]()
    sp = uc.specials(g)
    K = g.k + 1
    for name, cls in (("with_N", 0), ("len_k", 1), ("len_k+1", 2), ("len_k+2", 2), ("len_0", 1), ("one_invalid", 2), ("five_invalid", 2),
                      ("maps_nowhere", 2)):
        tallies = g.model.count([sp[name]])[2]
        assert tallies == tuple(1 if i == cls else 0 for i in range(3)), name
    assert g.model.count(["N" * 3])[2] == (1, 0, 0)  # (short AND with N: rule 1 comes first)
    assert (len(sp["len_k"]), len(sp["len_k+1"]), len(sp["len_k+2"])) == (K - 1, K, K + 1)


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_blocks_hold_the_cases(graph):
    g = uc.GRAPHS[graph]()
    sp = uc.specials(g)
    full = uc.block(graph, 77)
    assert len(full) == 77 and set(sp.values()) <= set(full)
    for n in uc.SIZES:
        assert len(uc.block(graph, n)) == n
    # what the special reads are for
    assert g.model.nodes(sp["len_k+1"]) and g.model.nodes(sp["len_k+2"])          # the shortest used reads do map
    assert g.model.nodes(sp["one_invalid"]) and g.model.nodes(sp["five_invalid"])  # reads with invalid bytes still map
    assert g.model.nodes(sp["maps_nowhere"]) == []
    bad = [p for p, c in enumerate(sp["five_invalid"]) if c not in "ACGT"]
    assert len(bad) == 5 and "N" not in sp["five_invalid"]                        # more than inv4 holds: VS_FLAG_MANY
    assert sum(c not in "ACGT" for c in sp["one_invalid"]) == 1
    # a block in which every read is dropped
    dropped = uc.all_dropped(graph)
    _, short_mat, tallies = g.model.count(dropped)
    assert tallies[2] == 0 and tallies[0] > 0 and tallies[1] > 0 and not short_mat.any()


def test_chain_reads_span_one_two_and_three_nodes():
    g = uc.chain()
    for n, reads in g.spans.items():
        for s in reads:
            assert len(g.model.nodes(s)) == n, (n, g.model.nodes(s))
    assert g.model.nodes(g.spans[3][0]) == [1, 2, 3]
    _, short_mat, _ = g.model.count(g.spans[3][:1])
    want = np.zeros((4, 4), dtype=np.int64)
    want[1, 1] = want[1, 2] = want[1, 3] = want[2, 2] = want[2, 3] = want[3, 3] = 1  # a triangle of six cells, diagonal included
    assert np.array_equal(short_mat, want)


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_cases_see_the_pair_filter(graph):
    """A counter that drops a read because its NEIGHBOUR has an N or is short (the filter of a pair, applied to two
    singles) gives other counters and other tallies on these blocks."""
    g = uc.GRAPHS[graph]()
    for n in (31, 77):
        reads = uc.block(graph, n)
        _, right, t_right = g.model.count(reads)
        _, wrong, t_wrong = g.model.count(reads, pair_filter=True)
        assert t_right != t_wrong and t_wrong[2] < t_right[2]
        assert not np.array_equal(right, wrong)


def test_shape_block_is_clean():
    reads = uc.shape_block()
    assert all(len(s) == 150 and set(s) <= set("ACGT") for s in reads)
