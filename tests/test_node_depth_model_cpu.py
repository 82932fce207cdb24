"""The definition of the depth pass (tests/node_depth_model.py) on the CPU: its invariant on error-free reads, its agreement
with the ``v`` the oracle's read mapping sums per node, its restatement by maximal matches, and the constructed cases of
tests/node_depth_cases.py -- the counts their construction fixes, and that every named mistake changes a count."""
import pytest

import node_depth_cases as cases
import node_depth_model as model
from oracle.pe_oracle import build_table
from vstrains_amd import synth


@pytest.fixture(scope="module")
def synth_case():
    c = synth.make_pipeline_case(n_strains=4, genome_len=3000, snp_rate=0.02, k=55, n_pairs=400, read_len=150, seed=5)
    seqs = list(c.graph.seqs)
    ends = [e for pair in zip(c.fwd, c.rve) for e in pair]
    return seqs, ends, build_table(seqs, 56)


def test_error_free_reads_of_the_graphs_own_strains_count_every_window_exactly_once(synth_case):
    seqs, ends, table = synth_case
    kc = model.node_depth(seqs, 55, ends, table=table)
    per_window = model.window_entries(seqs, 55, ends, table=table)
    assert len(ends) == 800 and len(per_window) == 800 * (150 - 56 + 1)
    assert max(per_window) == 1 and min(per_window) == 1  # no window has more than one table entry, none has none
    assert sum(kc) == 76000
    assert sum(1 for v in kc if v == 0) == 3


def test_model_is_the_sum_of_the_mappings_pre_acceptance_v(synth_case):
    """``hits[node][0]`` inside the oracle's ``map_read_end`` (oracle/pe_oracle.py:81-95), restated: the count per node of one
    end before the acceptance test, summed over the ends."""
    seqs, ends, table = synth_case
    kc = [0] * len(seqs)
    for read in ends[:200]:
        hits = {}
        for i in range(len(read) - 56 + 1):
            bucket = table.get(read[i:i + 56])
            if bucket is None:
                continue
            for node, off in bucket:
                rec = hits.get(node)
                if rec is None:
                    hits[node] = [1, off, i]
                else:
                    rec[0] += 1
        for node, rec in hits.items():
            kc[node] += rec[0]
    assert kc == model.node_depth(seqs, 55, ends[:200], table=table)


ALL = [c for k in cases.KS for c in cases.small_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_counts_hold_in_the_model(case):
    kc = model.node_depth(case.seqs, case.k, case.ends)
    if case.want is not None:
        assert {n: v for n, v in enumerate(kc) if v} == {n: v for n, v in case.want.items() if v}
    if case.name == "seed_with_100_postings":
        assert kc == [6 * 2] * 100
    if case.name == "node_whose_first_K_bases_are_a_palindrome":
        assert kc[0] == 2 + 4  # the palindromic window twice, four more windows once
    if case.name == "same_window_at_two_offsets_of_one_node_and_in_two_nodes":
        assert kc == [2, 1, 0]
    assert sum(kc) > 0


@pytest.mark.parametrize("case", [c for c in ALL if c.k != 127 and not c.name.startswith("seed_with_100")], ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_restatement_by_maximal_matches_gives_the_same_counts(case):
    assert model.node_depth_by_matches(case.seqs, case.k, case.ends) == model.node_depth(case.seqs, case.k, case.ends)


@pytest.mark.parametrize("variant", model.TABLE_VARIANTS + model.MATCH_VARIANTS)
@pytest.mark.parametrize("k", (21, 55))
def test_every_named_mistake_changes_the_count_of_the_cases_that_name_it(variant, k):
    told = 0
    for case in cases.small_cases(k):
        if variant not in case.tells:
            continue
        want = model.node_depth(case.seqs, k, case.ends)
        if variant in model.TABLE_VARIANTS:
            got = model.node_depth(case.seqs, k, case.ends, variant=variant)
        else:
            got = model.node_depth_by_matches(case.seqs, k, case.ends, variant=variant)
        assert got != want, (variant, case.name)
        told += 1
    assert told, variant


def test_larger_cases_are_what_their_names_say():
    share = cases.share_plus_one(21, 1024)
    assert len(share.ends) == 1024 + 1 and share.singles
    many = cases.many_nodes(21, 33533)
    assert len(many.seqs) == 33533 and all(len(s) == 24 for s in many.seqs)
