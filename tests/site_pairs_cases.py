"""Constructed blocks for the site-pair pass (``vs_node_site_pairs``): graphs, reads and site lists in which one thing at a time
can go wrong about keeping together what ONE fragment saw -- which end belongs to which fragment, what a site under two
alignments is worth, where the overlap's sites start and end, which pairs have a cell.  Every case names the cell it is there
for (``cell``), the tallies its construction fixes (``tally``) and the named mistakes of tests/site_pairs_model.py it must
expose (``tells``); the reads are a few bases longer than an anchor.  Expected tables come from that model;
tests/test_site_pairs_model_cpu.py holds the cases to their cells, tests/test_site_pairs_gpu.py runs them on the device at
k = 21, 55 and 127."""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from node_depth_cases import KS, dna  # noqa: F401  (KS: for the tests)
from pileup_cases import sub, with_n
from pileup_model import revcomp


class SitePairCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    ends: List[str]
    sites: List[Tuple[int, int]]                # (segment in the order of ``seqs``, 0-based position)
    cell: str                                   # what the case is there for
    singles: bool = False                       # packed as a singles block: every second end absent, every end a fragment
    M: int = 8                                  # the mismatch budget it runs with
    span: int = 1000
    tally: Optional[Tuple[int, int, int, int, int]] = None  # (observing, overflow, discordant, stored, unstored) the construction fixes
    tells: tuple = ()                           # the named mistakes (site_pairs_model.VARIANTS) this case must expose


def site_pair_cases(k: int) -> List[SitePairCase]:
    K = k + 1
    R = K + 8  # a read: an anchor and eight bases
    rng = np.random.default_rng(9000 + k)
    node = dna(rng, 6 * K + 150)
    other = dna(rng, 2 * K + 1)
    L = len(node)
    nothing = other[:K - 1]  # a mate too short for an anchor
    out: List[SitePairCase] = []

    def add(name, seqs, ends, sites, cell, **kw):
        assert kw.get("singles", False) or len(ends) % 2 == 0
        out.append(SitePairCase(name, k, seqs, ends, sites, cell, **kw))

    a2 = 2 * K + 60
    add("one_site_under_each_mate_and_none_shared", [node, other], [sub(node[10:10 + R], 3), revcomp(sub(node[a2:a2 + R], 5))], [(0, 13), (0, a2 + 5)],
        "the two mates are ONE fragment: the pair of sites gets its count from a read pair neither end of which sees both",
        tally=(1, 0, 0, 1, 0), tells=("per_end", "no_complement", "no_mirror"))
    two = sub(node[20:20 + R], 2, R - 3)
    add("two_sites_under_one_end_forward_and_reverse_complemented", [node, other], [two, nothing, revcomp(two), nothing], [(0, 22), (0, 20 + R - 3)],
        "the read and its reverse complement land in the same cell: count 2", tally=(2, 0, 0, 2, 0), tells=("no_complement", "no_mirror"))
    s2 = 30 + R - 2
    add("mates_overlapping_on_a_site_and_agreeing", [node, other], [sub(node[30:30 + R], R - 2), revcomp(sub(node[30 + R - 6:30 + 2 * R - 6], 4))],
        [(0, 31), (0, s2)], "three raw observations, two of them of one site with one base: observed once, one pair",
        tally=(1, 0, 0, 1, 0), tells=("twice_when_mates_overlap",))
    add("mates_overlapping_on_a_site_and_disagreeing", [node, other], [node[30:30 + R], revcomp(sub(node[30 + R - 6:30 + 2 * R - 6], 4))],
        [(0, 31), (0, s2), (0, 30 + 2 * R - 8)], "the shared site is discordant and left out; the first mate's site still links with the second mate's",
        tally=(1, 0, 1, 1, 0), tells=("no_discordance", "per_end", "no_mirror"))
    r1 = R + 5
    add("sites_on_the_overlaps_first_and_last_base_and_the_segments_ends", [node, other],
        [node[r1:r1 + R], nothing, node[:R], revcomp(node[L - R:])],
        [(0, r1 - 1), (0, r1), (0, r1 + R - 1), (0, r1 + R), (0, 0), (0, R - 1), (0, L - R), (0, L - 1)],
        "the edges of the binary search: the sites one before and one behind an overlap are not seen, position 0 and the last are", span=L,
        tally=(2, 0, 0, 7, 0), tells=("no_mirror", "no_complement"))
    add("sites_exactly_span_and_span_plus_1_apart", [node, other], [node[50:50 + R], nothing], [(0, 51), (0, 58), (0, 59)],
        "span = 7: (51, 58) and (58, 59) have cells, (51, 59) is unstored", span=7, tally=(1, 0, 0, 2, 1), tells=("span_lt",))
    b0 = 60
    b1, b2, b3 = b0 + R + 5, b0 + 2 * R + 10, b0 + 3 * R + 15
    add("exactly_32_and_33_raw_observations", [node, other], [node[b0:b0 + R], revcomp(node[b1:b1 + R]), node[b2:b2 + R], revcomp(node[b3:b3 + R])],
        [(0, b + i) for b in (b0, b1, b2) for i in range(16)] + [(0, b3 + i) for i in range(17)],
        "16 sites under each mate: 32 observations and 496 pairs; 16 and 17: overflow, nothing deposited", span=L,
        tally=(2, 1, 0, 496, 0), tells=("cap_ge",))
    m1, m2 = 100, 100 + R + 10
    add("M_plus_1_mismatches_over_a_site", [node, other], [sub(node[m1:m1 + R], K + 2, K + 4, K + 6), sub(node[m2:m2 + R], K + 1, K + 3, K + 5, K + 7)],
        [(0, m1 + 1), (0, m1 + K + 2), (0, m2 + 2), (0, m2 + K + 1)], "M = 3: the mate with four mismatches is rejected and observes nothing", M=3,
        tally=(1, 0, 0, 1, 0), tells=("rejected_observe",))
    add("an_N_on_a_site", [node, other], [revcomp(with_n(node[120:120 + R], K + 3)), nothing], [(0, 121), (0, 120 + K + 3)],
        "a byte outside ACGT is column 4, on either strand", tally=(1, 0, 0, 1, 0), tells=("no_mirror", "no_complement"))
    u = K + 10
    unit = dna(rng, u)
    tandem = dna(rng, 2) + unit + sub(unit, 3) + dna(rng, 2)
    add("tandem_repeat_two_diagonals_with_different_bases_on_one_site", [tandem, other], [unit + sub(unit, 3), nothing],
        [(0, 2 + 1), (0, 2 + u + 3), (0, 2 + u + 20)],
        "one end, three diagonals: the site where the copies differ is discordant inside one end; where they agree a site seen twice is seen once",
        tally=(1, 0, 1, 1, 0), tells=("no_discordance", "twice_when_mates_overlap"))
    half = dna(rng, K // 2 + 3)
    pal = half + revcomp(half)
    add("palindromic_segment", [pal, other], [sub(pal, 1), nothing], [(0, 1), (0, 5), (0, 9)],
        "one read, two alignments: the substituted base meets the segment's own base on the other strand (discordant); the other sites agree with themselves",
        tally=(1, 0, 1, 1, 0), tells=("no_complement", "no_discordance"))
    ov = dna(rng, k)
    left, right = dna(rng, K + 10) + ov, ov + dna(rng, K + 10)
    add("sites_on_two_segments_sharing_a_k_overlap", [left, right], [left[-(k + 10):] + right[k:k + 10], nothing],
        [(0, len(left) - k - 8), (0, len(left) - k - 5), (1, k + 5)],
        "the read is credited on both segments: the pair on the left one is stored, the two pairs across the junction are unstored",
        tally=(1, 0, 0, 1, 2), tells=("cross_segment_stored",))
    add("singles_block_with_an_absent_an_empty_and_a_short_end", [node, other],
        [sub(node[3:3 + R], 2), "", dna(rng, K - 1), revcomp(node[3 + R - 4:3 + 2 * R - 4])], [(0, 5), (0, 3 + R - 2), (0, 3 + R + 6)],
        "every present end is a fragment of its own: the first and the last read are not joined over the site they share", singles=True,
        tally=(2, 0, 0, 2, 0), tells=("no_mirror", "no_complement"))
    add("an_empty_site_list", [node, other], [node[10:10 + R], revcomp(node[a2:a2 + R])], [], "nothing is launched and nothing is counted",
        tally=(0, 0, 0, 0, 0))
    # three segments in a chain c <- b <- a, listed against it: the index numbers them along the path, not as the file does
    chain = dna(rng, 3 * (K + 20))
    c0, c1 = K + 20, 2 * (K + 20)
    sa, sb, sc = chain[:c0 + k], chain[c0:c1 + k], chain[c1:]
    add("graph_whose_node_rank_is_not_the_identity", [sc, other, sa, sb, dna(rng, K + 1)],
        [sub(sa[2:2 + R], 4), revcomp(sa[8:8 + R]), sub(sc[len(sc) - R:], 3), nothing, sb[12:12 + R], nothing],
        [(2, 6), (2, 8 + R - 1), (0, len(sc) - R + 3), (0, len(sc) - 2), (3, 13), (3, 14), (2, 6)],
        "sites are given in the file's numbering and come back in it, whatever the index made of it; a site named twice is one",
        tally=(3, 0, 0, 3, 0), tells=("per_end", "no_mirror"))
    return out
