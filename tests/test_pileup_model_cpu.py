"""The definition of the base pileup (tests/pileup_model.py) held to the depth profile's model and to the cells of the
constructed cases (tests/pileup_cases.py): no device."""
import pytest

import depth_profile_model
import pileup_cases as cases
import pileup_model as model

ALL = [c for k in cases.KS for c in cases.pileup_cases(k)]
IDS = ["%s_k%d" % (c.name, c.k) for c in ALL]


@pytest.fixture(scope="module")
def judged():
    """case -> the model's (depth, alt, tally), computed once."""
    return {(c.name, c.k): model.pileup(c.seqs, c.k, c.ends, c.M) for c in ALL}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_the_anchored_alignments_are_the_diagonals_of_the_depth_profiles_matches(case):
    """(end, segment, strand, diagonal) of every anchored alignment == the diagonals of ``depth_profile_model.maximal_matches``;
    and the runs of K on a diagonal are that model's matches on it."""
    table = depth_profile_model.strand_table(case.seqs, case.k + 1)
    want = {}
    for e, end in enumerate(case.ends):
        for a, n, strand, qa, length in depth_profile_model.maximal_matches(case.seqs, case.k, end, table):
            want[(e, n, strand, qa - a)] = want.get((e, n, strand, qa - a), 0) + 1
    got = {(e, n, t, d): runs for e, n, t, d, x_lo, agree, runs in model.anchored(case.seqs, case.k, case.ends)}
    assert got == want and len(got) > 0


@pytest.mark.parametrize("case", [c for c in ALL if c.k == 21 and len(c.seqs) <= 6], ids=lambda c: c.name)
def test_walking_every_diagonal_finds_the_same_alignments(case):
    assert model.pileup(case.seqs, case.k, case.ends, case.M, brute=True) == model.pileup(case.seqs, case.k, case.ends, case.M)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_case_holds_its_cell(case, judged):
    depth, alt, tally = judged[(case.name, case.k)]
    assert case.cell
    if case.tally is not None:
        assert tally == case.tally
    K = case.k + 1
    for n, seq in enumerate(case.seqs):
        assert len(depth[n]) == len(alt[n]) == (len(seq) if len(seq) >= K else 0)
        for dp, a in zip(depth[n], alt[n]):
            assert 0 <= sum(a) <= dp  # (the reference base's count, the depth minus the others, is never negative)
    assert case.tells  # (every case is there to expose some named mistake)
    for v in case.tells:
        assert model.pileup(case.seqs, case.k, case.ends, case.M, variant=v) != (depth, alt, tally), v


def test_every_named_mistake_is_told_by_some_case():
    for k in cases.KS:
        told = set(v for c in cases.pileup_cases(k) for v in c.tells)
        assert told == set(model.VARIANTS), k


@pytest.mark.parametrize("k", cases.KS)
def test_cells_the_construction_fixes_by_hand(k, judged):
    K = k + 1
    by = {c.name: c for c in cases.pileup_cases(k)}
    # an exact read covers its own bases once and writes no alt; the reverse-complemented one lands on the forward positions
    depth, alt, _ = judged[("exact_read_forward_and_reverse_complemented", k)]
    want = [0] * len(by["exact_read_forward_and_reverse_complemented"].seqs[0])
    for a in (7, 40):
        for p in range(a, a + K + 20):
            want[p] += 1
    assert depth[0] == want and not any(any(a) for a in alt[0]) and not any(depth[1])
    # one substitution in the middle: ONE alignment over 2K + 1 positions, the read's base at the substituted position
    c = by["one_substitution_in_the_middle_of_2K_plus_1_bases"]
    depth, alt, _ = judged[(c.name, k)]
    node = c.seqs[0]
    assert depth[0][11:11 + 2 * K + 1] == [1] * (2 * K + 1) and depth[0][10] == 0
    col = model.ACGT.index(c.ends[0][K])
    assert c.ends[0][K] != node[11 + K] and alt[0][11 + K] == [int(i == col) for i in range(5)]
    # ... and from the reverse-complemented read: the complement of what the read carries, at the mirrored position
    rc_read = c.ends[1]
    fwd_base = model.revcomp(rc_read)[K]  # (the read as it reads on the forward strand)
    assert fwd_base != node[4 * K + 20] and alt[0][4 * K + 20] == [int(i == model.ACGT.index(fwd_base)) for i in range(5)]
    assert sum(sum(a) for a in alt[0]) == 2
    # N goes to `other`
    depth, alt, _ = judged[("one_N_and_five_N_inside_the_overlap", k)]
    assert alt[0][33 + K + 3] == [0, 0, 0, 0, 3] and alt[0][33 + K + 30] == [0, 0, 0, 0, 1] and sum(sum(a) for a in alt[0]) == 7
    # a segment of exactly K bases: both strands of the exact read and the overhanging one; the shorter segments have no rows
    depth, alt, _ = judged[("segments_of_K_minus_1_and_K_bases", k)]
    assert depth[0] == [] and depth[2] == [] and depth[1] == [3] * K
    # the overlap flush with a segment's end stays on the segment
    c = by["overlap_flush_with_the_end_of_every_segment"]
    depth, alt, _ = judged[(c.name, k)]
    for n, s in enumerate(c.seqs):
        assert depth[n] == [0] * (len(s) - (K + 9)) + [2] * (K + 9)  # (each read and its reverse complement)


def test_the_table_and_the_variant_records_of_a_tiny_pileup():
    depth = [[4, 200, 3], []]
    alt = [[[0, 0, 0, 0, 0], [2, 0, 1, 0, 3], [0, 1, 0, 0, 0]], []]  # (the column of the segment's own base is never counted into)
    rows = model.table_rows(["s", "t"], ["ACA", "GG"], depth, alt)
    assert rows == [("s", 1, "A", 4, 0, 0, 0, 0), ("s", 2, "C", 2, 194, 1, 0, 3), ("s", 3, "A", 2, 1, 0, 0, 0)]
    # DP = 197: A has AD 2 >= 2 and 2 >= 0.01 * 197; G has AD 1 < 2
    assert model.variant_records(rows) == [("s", 2, "C", "A", 197, 2, "0.010152")]
