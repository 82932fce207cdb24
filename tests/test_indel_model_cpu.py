"""tests/indel_model.py against the constructed cases of tests/indel_cases.py and against planted events: no device.  The
model gives the records every case's construction fixes, every named mistake changes a record of at least one case, and an
indel planted in random unique sequence comes back as the planted event, left-aligned, from either strand."""
import numpy as np
import pytest

import indel_cases as cases
import indel_model as model
from node_depth_cases import dna
from pileup_model import revcomp

ALL = [c for k in cases.KS for c in cases.indel_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_the_model_gives_the_records_the_construction_fixes(case):
    records, tally = model.indels(case.seqs, case.k, case.ends, case.G)
    assert records == case.records
    assert tally[1] == sum(r[5] + r[6] for r in records if r[2] == model.DEL) and tally[2] == sum(r[5] + r[6] for r in records if r[2] == model.INS)
    if case.tally is not None:
        assert tally == case.tally
    K = case.k + 1
    assert all(len(s) <= 6 * K + 150 for s in case.seqs) and len(case.ends) <= 300 and max(len(e) for e in case.ends) <= 3 * K + 2 * case.G + 8
    assert case.singles or len(case.ends) % 2 == 0  # (a block of pairs)


def test_the_cases_cover_what_they_are_there_for():
    for k in cases.KS:
        K = k + 1
        assert K % 32 == {22: 22, 56: 24, 128: 0}[K]
        by_name = dict((c.name, c) for c in cases.indel_cases(k))
        assert len(by_name) == len(cases.indel_cases(k))
        assert len(by_name["a_block_of_70_ends"].ends) > 64
        assert by_name["a_singles_block_with_an_empty_and_a_short_end"].singles
        assert any(r[1] == 0 for r in by_name["an_insertion_that_left_aligns_to_the_segments_first_base"].records)
        assert by_name["an_N_in_the_insert_and_an_N_in_the_flank"].tally[3] == 1
        assert any(len(s) < K for s in by_name["a_segment_shorter_than_K_and_an_end_shorter_than_2K"].seqs)
        # the breakpoints' read offsets: the match right of the event starts at a mod 16 in {0, 1, 15}
        c = by_name["breakpoints_at_a_mod_16_of_0_1_and_15"]
        starts = sorted(set((kind, a % 16) for e, n, t, a, qa, ln in model.matches(c.seqs, k, c.ends) if a > 0
                            for kind in [model.scan(c.ends[e], c.seqs[n], t, a, qa, K, c.G)[1]]))
        assert starts == [(model.DEL, 0), (model.DEL, 1), (model.DEL, 15), (model.INS, 0), (model.INS, 1), (model.INS, 15)]


@pytest.mark.parametrize("variant", model.VARIANTS)
def test_every_named_mistake_changes_a_record_of_a_case_that_tells_it(variant):
    told = 0
    for case in ALL:
        wrong = model.indels(case.seqs, case.k, case.ends, case.G, variant=variant)[0]
        if variant in case.tells:
            assert wrong != case.records, (case.name, case.k, variant)
            told += 1
    assert told >= len(cases.KS)


@pytest.mark.parametrize("k", cases.KS)
def test_planted_indels_come_back_left_aligned_from_either_strand(k):
    K, G = k + 1, 16
    rng = np.random.default_rng(300 + k)
    F = dna(rng, 40 * (K + G))
    ends, want = [], {}
    for i in range(24):
        L = int(rng.integers(1, G + 1))
        u = int(rng.integers(2 * (K + G), len(F) - 3 * (K + G)))
        fl = fr = K + G + int(rng.integers(0, 5))
        if i % 2:
            I = dna(rng, L)
            read = F[u - fl:u] + I + F[u:u + fr]
            key = (0,) + _left_aligned(F, u, model.INS, L, I)
        else:
            read = F[u - fl:u] + F[u + L:u + L + fr]
            key = (0,) + _left_aligned(F, u, model.DEL, L, "")
        plane = i // 2 % 2
        ends.append(revcomp(read) if plane else read)
        want.setdefault(key, [0, 0])[plane] += 1
    records, tally = model.indels([F], k, ends, G)
    assert records == sorted(key + tuple(c) for key, c in want.items())
    assert tally == (24, 12, 12, 0)


def _left_aligned(F, u, kind, L, I):
    """The planted event moved left along F, by the rule as it is written in the issue -- not through the model's code."""
    if kind == model.DEL:
        while u > 0 and F[u - 1] == F[u + L - 1]:
            u -= 1
        return (u, kind, L, "")
    while u > 0 and F[u - 1] == I[-1]:
        u, I = u - 1, F[u - 1] + I[:-1]
    return (u, kind, L, I)
