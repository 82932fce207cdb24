"""Constructed blocks for the base pileup (``vs_node_pileup``): graphs and reads in which one thing at a time can go wrong
about laying a read along an anchor's diagonal -- who owns the alignment, where the overlap starts and ends, what counts
against the budget, which base is written down where.  Every case names the cell it is there for (``cell``) and the named
mistakes of tests/pileup_model.py it must expose (``tells``).  Expected tables come from that model;
tests/test_pileup_model_cpu.py holds the model to the depth profile's and the cases to their cells, tests/test_pileup_gpu.py
runs them on the device at k = 21, 55 and 127."""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from node_depth_cases import KS, _OTHER, dna  # noqa: F401  (KS: for the tests)
from pileup_model import revcomp


class PileupCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    ends: List[str]
    cell: str                                   # what the case is there for
    singles: bool = False                       # packed as a singles block: every second end absent
    M: int = 8                                  # the mismatch budget it runs with
    tally: Optional[Tuple[int, int]] = None     # (alignments, rejected) the construction fixes
    tells: tuple = ()                           # the named mistakes (pileup_model.VARIANTS) this case must expose


def sub(s: str, *at: int) -> str:
    """``s`` with another base at each offset of ``at`` (negative: from the end)."""
    b = list(s)
    for i in at:
        b[i] = _OTHER[b[i]]
    return "".join(b)


def with_n(s: str, *at: int) -> str:
    b = list(s)
    for i in at:
        b[i] = "N"
    return "".join(b)


def _even(rng, ends: List[str]) -> List[str]:
    """A block of pairs holds an even number of ends: an end of five bases, which counts nothing, fills it up."""
    return ends + [dna(rng, 5)] if len(ends) % 2 else ends


FLANKS = (31, 32, 33, 63, 64, 65)


def pileup_cases(k: int) -> List[PileupCase]:
    K = k + 1
    rng = np.random.default_rng(7000 + k)
    node = dna(rng, 6 * K + 150)
    other = dna(rng, 2 * K + 1)
    L = len(node)
    out: List[PileupCase] = []

    def add(name, seqs, ends, cell, **kw):
        singles = kw.get("singles", False)
        out.append(PileupCase(name, k, seqs, ends if singles else _even(rng, ends), cell, **kw))

    add("exact_read_forward_and_reverse_complemented", [node, other], [node[7:7 + K + 20], revcomp(node[40:40 + K + 20])],
        "depth only, alt stays 0; the reverse-complemented read lands at its forward position", tally=(2, 0), tells=("no_mirror",))
    mid = sub(node[11:11 + 2 * K + 1], K)
    add("one_substitution_in_the_middle_of_2K_plus_1_bases", [node, other], [mid, revcomp(sub(node[3 * K + 20:5 * K + 21], K))],
        "two matches on one diagonal are ONE alignment; the substituted base is written once, complemented and mirrored on the reverse strand",
        tally=(2, 0), tells=("per_match", "no_complement", "no_mirror"))
    add("three_matches_on_one_diagonal", [node, other], [sub(node[5:5 + 3 * K + 2], K, 2 * K + 1), other[:K - 1]],
        "the third match finds the second to its left and the second the first: credited once", tally=(1, 0), tells=("per_match",))
    add("substitution_K_minus_1_and_K_bases_from_the_reads_start", [node, other], [sub(node[9:9 + 2 * K + 5], K - 1), sub(node[9:9 + 2 * K + 5], K)],
        "a run of K - 1 to the left is no anchor (the right match owns), a run of exactly K is one (the left match owns)", tally=(2, 0), tells=("per_match",))
    junk_a, junk_b = dna(rng, 10), dna(rng, 10)
    over = [junk_a + node[:K + 5], node[L - (K + 5):] + junk_b]
    add("read_overhanging_the_segments_start_and_end_on_both_strands", [node, other], over + [revcomp(r) for r in over],
        "the overlap is clipped to the segment: the ten bases beyond it are neither compared nor counted", tally=(4, 0), tells=("unclipped",))
    seqs = [dna(rng, 2 * K + 3 + 2 * i) for i in range(6)]
    flush = [sub(s[len(s) - (K + 9):], 3) for s in seqs]
    add("overlap_flush_with_the_end_of_every_segment", seqs, flush + [revcomp(r) for r in flush],
        "the -1 lands in the segment's sentinel, not on the next segment's first position; on the other strand the overlap starts the text",
        tally=(12, 0), tells=("no_mirror", "no_complement"))
    add("mismatch_at_the_overlaps_first_and_last_base", [node, other], [sub(node[20:20 + K + 12], 0), sub(node[70:70 + K + 12], -1),
                                                                       revcomp(sub(node[20:20 + K + 12], 0)), sub(node[:K + 6], 0), sub(node[L - (K + 6):], -1)],
        "the first and the last bit of the walk's windows; position 0 and the last position of the segment", tally=(5, 0), tells=("no_complement", "no_mirror"))
    ends = []
    for f in FLANKS:
        a = int(rng.integers(0, L - (2 * f + K + 4)))
        read = sub(node[a:a + 2 * f + K + 4], f, f + K + 3)  # flank, mismatch, anchor of K + 2, mismatch, flank
        ends += [read, revcomp(read)]
    add("flanks_of_31_to_65_bases_beyond_the_anchor", [node, other], ends,
        "the walk's 32-base windows end exactly at, one before and one behind the overlap's ends, leftwards and rightwards", tally=(len(ends), 0),
        tells=("no_complement", "no_mirror") + (("per_match",) if K <= 65 else ()))
    tail = node[100:100 + K + 12]
    add("exactly_M_and_M_plus_1_mismatches", [node, other], [sub(tail, K + 2, K + 5, K + 8), sub(tail, K + 2, K + 5, K + 8, K + 11)],
        "M mismatches are credited, M + 1 rejected and tallied", M=3, tally=(1, 1), tells=("budget_lt",))
    n_read = node[33:33 + K + 40]
    add("one_N_and_five_N_inside_the_overlap", [node, other], [with_n(n_read, K + 3), with_n(n_read, K + 3, K + 9, K + 15, K + 21, K + 30), revcomp(with_n(n_read, K + 3))],
        "a byte outside ACGT goes to `other` under the mask, for an end with one and with more than the four the position list holds, on either strand",
        tally=(3, 0), tells=("no_mirror",))
    add("five_N_against_a_budget_of_four", [node, other], [with_n(n_read, K + 3, K + 9, K + 15, K + 21, K + 30), sub(n_read, K + 3, K + 9, K + 15, K + 21)],
        "N counts against the budget like any other non-agreeing byte", M=4, tally=(1, 1), tells=("n_free",))
    half = dna(rng, K // 2 + 3)
    pal = half + revcomp(half)
    add("palindromic_segment", [pal, other], [sub(pal, 1), other[:K - 1]], "one read, two alignments: one per strand, the mismatch written at both mirror positions",
        tally=(2, 0), tells=("no_mirror", "no_complement"))
    rep = dna(rng, K + 3)
    twice = dna(rng, 9) + rep + dna(rng, 17) + rep + dna(rng, 5)
    add("one_read_at_two_offsets_of_a_segment", [twice, other], [sub(rep, -1), revcomp(sub(rep, -1))], "two diagonals of one strand, each credited, for a read of either strand",
        tally=(4, 0), tells=("no_mirror", "no_complement"))
    ov = dna(rng, k)
    left, right = dna(rng, K + 10) + ov, ov + dna(rng, K + 10)
    add("two_segments_sharing_a_k_overlap", [left, right], [sub(left[-(k + 10):] + right[k:k + 10], 2, -2), other[:K - 1]],
        "the read is credited on both, overhanging the end of one and the start of the other", tally=(2, 0), tells=("unclipped",))
    exact = dna(rng, K)
    shorts = [dna(rng, K - 1), exact, dna(rng, 3), node]
    add("segments_of_K_minus_1_and_K_bases", shorts, [exact, revcomp(exact), dna(rng, 5) + exact + dna(rng, 5), shorts[0]],
        "a segment of K bases has K rows, a shorter one none; a read longer than the segment overhangs it on both sides", tally=(3, 0), tells=("unclipped",))
    add("singles_block_with_an_empty_and_a_short_end", [node, other], [node[3:3 + K + 4], "", dna(rng, K - 1), revcomp(sub(node[50:50 + K + 9], K + 4))],
        "absent, empty and short ends count nothing", singles=True, tally=(2, 0), tells=("no_mirror", "no_complement"))
    common = dna(rng, K + 2)
    uniq = [dna(rng, 25) for _ in range(70)]
    add("seed_with_more_than_64_postings", [u + common for u in uniq], [uniq[3][5:] + common, revcomp(uniq[40][5:] + common)],
        "70 postings are dealt in two rounds of lanes; each read is credited on its own segment and rejected on the 69 others",
        tally=None, tells=("no_mirror",))
    return out
