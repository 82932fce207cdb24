"""tests/strand_pileup_model.py held to tests/pileup_model.py (the planes sum to the pileup on every case of both case
files), the constructed cases of tests/strand_pileup_cases.py to their cells, and every named mistake of the model told from
the truth by at least one case.  No device."""
import pytest

import pileup_cases
import pileup_model
import strand_pileup_cases as cases
import strand_pileup_model as model

STRAND = [c for k in cases.KS for c in cases.strand_cases(k)]
PLAIN = [c for k in cases.KS for c in pileup_cases.pileup_cases(k)]
_ID = lambda c: "%s_k%d" % (c.name, c.k)  # noqa: E731


@pytest.fixture(scope="module")
def truth():
    """The model's tables of every stranded case, computed once."""
    return dict(((c.name, c.k), model.strand_pileup(c.seqs, c.k, c.ends, c.M)) for c in STRAND)


@pytest.mark.parametrize("case", STRAND + PLAIN, ids=_ID)
def test_the_planes_sum_to_the_pileup_and_the_tallies_are_equal(case):
    depth, alt, tally = model.strand_pileup(case.seqs, case.k, case.ends, case.M)
    want_depth, want_alt, want_tally = pileup_model.pileup(case.seqs, case.k, case.ends, case.M)
    assert model.plane_sum(depth, alt) == (want_depth, want_alt) and tally == want_tally
    if case.tally is not None:
        assert tally == case.tally


@pytest.mark.parametrize("case", STRAND, ids=_ID)
def test_every_case_tells_the_mistakes_it_names(case, truth):
    want = truth[(case.name, case.k)]
    assert case.tells
    for variant in case.tells:
        assert model.strand_pileup(case.seqs, case.k, case.ends, case.M, variant=variant)[:2] != want[:2], variant


def test_every_named_mistake_of_the_pileup_is_told_by_some_case():
    for k in cases.KS:
        told = set(v for c in cases.strand_cases(k) for v in c.tells)
        assert told == set(model.PILE_VARIANTS)


def test_the_graphs_are_small():
    for c in STRAND:
        assert 2 <= len(c.seqs) <= 4 and max(len(s) for s in c.seqs) <= 2 * (c.k + 1) + 60


@pytest.mark.parametrize("k", cases.KS)
def test_a_palindromic_overlap_puts_one_into_each_plane(k, truth):
    depth, alt, tally = truth[("palindromic_overlap", k)]
    assert tally == (2, 0) and all(d == [1, 1] for d in depth[0])
    hit = [(p, t, a[t]) for p, a in enumerate(alt[0]) for t in (0, 1) if any(a[t])]
    L = len(depth[0])
    assert [(p, t) for p, t, _ in hit] == [(1, 0), (L - 2, 1)] and sum(hit[0][2]) == sum(hit[1][2]) == 1
    assert hit[0][2].index(1) == 3 - hit[1][2].index(1)  # (the read's base, and its complement at the mirror position)


@pytest.mark.parametrize("k", cases.KS)
def test_a_read_and_its_reverse_complement_put_the_same_column_into_different_planes(k, truth):
    depth, alt, tally = truth[("a_read_and_its_reverse_complement", k)]
    hit = [(p, a) for p, a in enumerate(alt[0]) if any(a[0]) or any(a[1])]
    assert len(hit) == 1 and hit[0][0] == 5 + k + 1 + 10 and hit[0][1][0] == hit[0][1][1] and sum(hit[0][1][0]) == 1
    assert all(d[0] == d[1] for d in depth[0]) and sum(d[0] for d in depth[0]) == k + 1 + 20


@pytest.mark.parametrize("k", cases.KS)
def test_the_flush_cases_reach_the_first_and_the_last_position_of_every_segment_in_both_planes(k, truth):
    depth = truth[("overlap_flush_with_the_end_of_every_segment_on_each_strand", k)][0]
    assert all(row[-1] == [1, 1] and row[0] == [0, 0] for row in depth)
    depth = truth[("overlap_flush_with_the_start_of_every_segment_on_each_strand", k)][0]
    assert all(row[0] == [1, 1] and row[-1] == [0, 0] for row in depth)


@pytest.mark.parametrize("k", cases.KS)
def test_the_rejected_alignment_leaves_its_plane_empty(k, truth):
    depth, alt, tally = truth[("rejected_on_one_strand_beside_credited_on_the_other", k)]
    assert tally == (1, 1) and not any(d[0] for d in depth[0]) and sum(d[1] for d in depth[0]) == k + 1 + 12
    assert sum(sum(a[1]) for a in alt[0]) == 2 and not any(any(a[0]) for a in alt[0])


def test_the_edge_blocks_have_the_sizes_they_are_named_for():
    for k in cases.KS:
        by = dict((c.name, c) for c in cases.strand_cases(k))
        assert len(by["a_block_of_65_ends"].ends) == 66  # (65 and the end that makes the block even)
        assert len(by["a_block_of_one_end_more_than_a_workgroups_least_share"].ends) == cases.MIN_ENDS + 2
        assert by["singles_block_with_absent_ends"].singles


# ---- the records ------------------------------------------------------------------------------------------------------
# (ref, depth per plane, alt per plane, C, F, S) and the named mistakes the position is there to tell from the truth
CALLS = [
    ("other_is_not_part_of_DP", "A", [10, 10], [[0, 1, 0, 0, 9], [0, 1, 0, 0, 9]], 2, 0.5, 0, ("dp_with_other",)),
    ("the_fraction_at_exact_equality", "A", [4, 4], [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0]], 2, 0.25, 0, ("frac_gt",)),
    ("the_double_product_above_AD", "C", [60, 40], [[4, 0, 0, 0, 0], [3, 0, 0, 0, 0]], 2, 0.07, 0, ("frac_by_division",)),
    ("the_double_product_at_AD", "C", [60, 40], [[20, 0, 0, 0, 0], [9, 0, 0, 0, 0]], 2, 0.29, 0, ()),
    ("all_on_one_strand", "G", [20, 20], [[0, 0, 0, 6, 0], [0, 0, 0, 0, 0]], 2, 0.01, 2, ("strand_on_total",)),
    ("the_reference_column_of_plane_1", "T", [9, 30], [[2, 0, 0, 0, 0], [2, 0, 0, 0, 1]], 2, 0.01, 1, ("ref_from_plane0",)),
]


@pytest.mark.parametrize("name, ref, depth, alt, C, F, S, tells", CALLS, ids=[c[0] for c in CALLS])
def test_the_record_rule_and_its_named_mistakes(name, ref, depth, alt, C, F, S, tells):
    want = model.position_records(ref, depth, alt, C, F, S)
    for variant in tells:
        assert model.position_records(ref, depth, alt, C, F, S, variant=variant) != want, variant


def test_every_named_mistake_of_the_caller_is_told_by_some_position():
    assert set(v for c in CALLS for v in c[7]) == set(model.CALL_VARIANTS)


def test_the_rule_by_hand():
    assert 0.07 * 100 > 7 and 0.29 * 100 <= 29  # (what makes the two inexact cases what they are)
    assert model.position_records("C", [60, 40], [[4, 0, 0, 0, 0], [3, 0, 0, 0, 0]], 2, 0.07) == []
    assert model.position_records("C", [60, 40], [[20, 0, 0, 0, 0], [9, 0, 0, 0, 0]], 2, 0.29) == [("A", 100, 29, (40, 31, 20, 9), False)]
    assert model.position_records("A", [4, 4], [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0]], 2, 0.25) == [("C", 8, 2, (3, 3, 1, 1), False)]
    got = model.position_records("G", [20, 20], [[0, 0, 0, 6, 0], [0, 0, 0, 0, 0]], 2, 0.01, 2)
    assert got == [("T", 40, 6, (14, 20, 6, 0), True)]  # (the strand threshold marks the record and never removes it)
    assert model.position_records("G", [20, 20], [[0, 0, 0, 6, 0], [0, 0, 0, 0, 0]], 2, 0.01, 0)[0][4] is False
    assert model.position_records("A", [0, 0], [[0] * 5, [0] * 5], 0, 0.0) == []  # (AD = 0 is never a record, whatever C is)
    three = model.position_records("A", [9, 9], [[0, 1, 2, 3, 0], [0, 3, 2, 1, 0]], 2, 0.01, 2)
    assert [(r[0], r[2], r[4]) for r in three] == [("C", 4, True), ("G", 4, False), ("T", 4, True)]
    assert model.position_records("A", [5], [[0, 0, 3, 0, 0]], 2, 0.01) == [("G", 5, 3, (2, 0, 3, 0), False)]  # (one plane: the second is zeros)


def test_with_the_planes_summed_the_records_are_the_unstranded_ones():
    for case in [c for c in STRAND if c.k == 21]:
        depth, alt, _ = model.strand_pileup(case.seqs, case.k, case.ends, case.M)
        ids = ["s%d" % n for n in range(len(case.seqs))]
        got = model.variant_records(ids, case.seqs, depth, alt, 1, 0.01)
        rows = pileup_model.table_rows(ids, case.seqs, *model.plane_sum(depth, alt))
        assert model.unstranded(got) == pileup_model.variant_records(rows, 1, 0.01)
        assert all(r[8] == "." and r[7][2] + r[7][3] == r[5] and sum(r[7]) <= r[4] for r in got)
