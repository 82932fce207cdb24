"""The definition of the site-pair pass (tests/site_pairs_model.py) held to the cells of the constructed cases
(tests/site_pairs_cases.py): every named mistake is told, every case reaches its cell, and the order in which a fragment's
raw observations arrive changes nothing.  No device."""
import numpy as np
import pytest

import site_pairs_cases as cases
import site_pairs_model as model
from pileup_model import ACGT, _COMP

ALL = [c for k in cases.KS for c in cases.site_pair_cases(k)]
IDS = ["%s_k%d" % (c.name, c.k) for c in ALL]


def judge(c, **kw):
    return model.site_pairs(c.seqs, c.k, c.ends, c.sites, c.M, c.span, c.singles, **kw)


@pytest.fixture(scope="module")
def judged():
    """case -> the model's (pairs, tallies), computed once."""
    return {(c.name, c.k): judge(c) for c in ALL}


def test_every_named_mistake_is_told_by_some_case():
    for k in cases.KS:
        told = set(v for c in cases.site_pair_cases(k) for v in c.tells)
        assert told == set(model.VARIANTS), k


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_case_reaches_its_cell_and_tells_its_mistakes(case, judged):
    pairs, tally = judged[(case.name, case.k)]
    assert case.cell and case.tally is not None and tally == case.tally
    assert case.tells or not case.sites  # (every case but the empty site list is there to expose some named mistake)
    for v in case.tells:
        assert judge(case, variant=v) != (pairs, tally), v
    K = case.k + 1
    for n, p in case.sites:
        assert len(case.seqs[n]) >= K and 0 <= p < len(case.seqs[n])
    assert sum(sum(sum(r) for r in cell) for cell in pairs.values()) == tally[3]
    for (s, t), cell in pairs.items():
        assert s[0] == t[0] and 0 < t[1] - s[1] <= case.span


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_the_order_of_a_fragments_raw_observations_changes_nothing(case, judged):
    for seed in range(3):
        assert judge(case, shuffle=np.random.default_rng(seed)) == judged[(case.name, case.k)]


@pytest.mark.parametrize("k", cases.KS)
def test_cells_the_construction_fixes_by_hand(k, judged):
    K, R = k + 1, k + 9
    by = {c.name: c for c in cases.site_pair_cases(k)}

    def only(name):
        pairs, _ = judged[(name, k)]
        return by[name], pairs

    def one_hot(a, b, n=1):
        return [[n * int((i, j) == (a, b)) for j in range(5)] for i in range(5)]

    # one site under each mate: the cell holds the two substituted bases as they read on the forward strand
    c, pairs = only("one_site_under_each_mate_and_none_shared")
    node, a2 = c.seqs[0], 2 * K + 60
    ca, cb = ACGT.index(c.ends[0][3]), ACGT.index(_COMP[c.ends[1][R - 1 - 5]])
    assert c.ends[0][3] != node[13] and ACGT[cb] != node[a2 + 5]
    assert pairs == {((0, 13), (0, a2 + 5)): one_hot(ca, cb)}
    # a read and its reverse complement: the same cell, twice
    c, pairs = only("two_sites_under_one_end_forward_and_reverse_complemented")
    assert pairs == {((0, 22), (0, 20 + R - 3)): one_hot(ACGT.index(c.ends[0][2]), ACGT.index(c.ends[0][R - 3]), 2)}
    # mates agreeing on the shared site: once
    c, pairs = only("mates_overlapping_on_a_site_and_agreeing")
    assert pairs == {((0, 31), (0, 30 + R - 2)): one_hot(ACGT.index(node[31]), ACGT.index(c.ends[0][R - 2]))}
    # mates disagreeing: the shared site is out, the outer two link with the segment's own bases
    c, pairs = only("mates_overlapping_on_a_site_and_disagreeing")
    assert pairs == {((0, 31), (0, 30 + 2 * R - 8)): one_hot(ACGT.index(node[31]), ACGT.index(node[30 + 2 * R - 8]))}
    # the edges: the sites one before and one behind the overlap take part in no pair
    c, pairs = only("sites_on_the_overlaps_first_and_last_base_and_the_segments_ends")
    r1, L = R + 5, len(node)
    assert set(pairs) == {((0, r1), (0, r1 + R - 1))} | {((0, a), (0, b)) for a in (0, R - 1, L - R, L - 1) for b in (0, R - 1, L - R, L - 1) if a < b}
    assert pairs[((0, 0), (0, L - 1))] == one_hot(ACGT.index(node[0]), ACGT.index(node[L - 1]))
    # span and span + 1
    c, pairs = only("sites_exactly_span_and_span_plus_1_apart")
    assert set(pairs) == {((0, 51), (0, 58)), ((0, 58), (0, 59))}
    # 32 observations deposit, 33 do not
    c, pairs = only("exactly_32_and_33_raw_observations")
    assert len(pairs) == 496 and max(t[1] for s, t in pairs) == 60 + R + 5 + 15
    # the N
    c, pairs = only("an_N_on_a_site")
    assert pairs == {((0, 121), (0, 120 + K + 3)): one_hot(ACGT.index(node[121]), 4)}
    # across the junction nothing is stored
    c, pairs = only("sites_on_two_segments_sharing_a_k_overlap")
    assert list(pairs) == [((0, len(c.seqs[0]) - k - 8), (0, len(c.seqs[0]) - k - 5))]
    # sites come back in the file's numbering, the doubled one once
    c, pairs = only("graph_whose_node_rank_is_not_the_identity")
    assert sorted(set(s[0] for s, t in pairs)) == [0, 2, 3] and len(model.site_list(c.sites)) == len(c.sites) - 1


def test_the_reduction_on_a_list_written_out():
    s, t, u = (0, 5), (0, 9), (1, 2)
    raw = [(t, 1), (s, 0), (t, 1), (u, 4), (s, 2)]
    assert model.reduce_fragment(raw) == ([(t, 1), (u, 4)], 1)
    assert model.reduce_fragment(raw, "no_discordance") == ([(s, 0), (s, 2), (t, 1), (u, 4)], 0)
    assert model.reduce_fragment(raw, "twice_when_mates_overlap") == ([(t, 1), (t, 1), (u, 4)], 1)
    assert model.reduce_fragment([]) == ([], 0)


def test_the_table_rows_of_a_tiny_result():
    cell = [[0] * 5 for _ in range(5)]
    cell[1][4], cell[0][2], cell[1][0] = 3, 2, 1
    pairs = {((1, 4), (1, 9)): cell, ((0, 0), (0, 1)): [[int(i == j == 3) for j in range(5)] for i in range(5)]}
    assert model.table_rows(["s", "t"], pairs) == [("s", 1, 2, "T", "T", 1), ("t", 5, 10, "A", "G", 2), ("t", 5, 10, "C", "A", 1), ("t", 5, 10, "C", "N", 3)]
    assert model.result_rows(pairs)[1][:3] == (1, 4, 9)
