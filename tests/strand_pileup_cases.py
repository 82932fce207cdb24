"""Constructed blocks for the stranded pileup (``vs_node_pileup_strands``): graphs of two to four segments of at most a few
hundred bases and reads in which one thing at a time can go wrong about WHICH PLANE an alignment is counted in.  Every case
names the cell it is there for (``cell``) and the named mistakes of tests/strand_pileup_model.py it must expose (``tells``).
Expected tables come from that model; tests/test_strand_pileup_model_cpu.py holds the model to the pileup's and the cases to
their cells, tests/test_strand_pileup_gpu.py runs them on the device at k = 21, 55 and 127."""
from typing import List

import numpy as np

from node_depth_cases import KS, dna  # noqa: F401  (KS: for the tests)
from pileup_cases import PileupCase, _even, sub, with_n
from pileup_model import revcomp

MIN_ENDS = 1024  # PILEUP_MIN_ENDS (csrc/vs_pileup_plan.h): the least share of a workgroup -- one end more makes a second workgroup
ALL_PILE = ("planes_swapped", "strand_by_mate", "plane1_unmirrored", "plane1_uncomplemented")


def _many(rng, node: str, K: int, n: int) -> List[str]:
    """``n`` reads of K + 6 bases with one substitution each among the first or the last six (K agreeing bases stay in a row),
    every third one reverse-complemented: the strand is neither the end's parity nor the same for a whole batch."""
    out = []
    for i in range(n):
        a = int(rng.integers(0, len(node) - (K + 6) + 1))
        at = int(rng.integers(0, 12))
        read = sub(node[a:a + K + 6], at if at < 6 else K + at - 6)
        out.append(revcomp(read) if i % 3 == 0 else read)
    return out


def strand_cases(k: int) -> List[PileupCase]:
    K = k + 1
    rng = np.random.default_rng(9000 + k)
    a, b, c = dna(rng, 2 * K + 60), dna(rng, 2 * K + 9), dna(rng, 2 * K + 3)
    short = dna(rng, K - 1)
    out: List[PileupCase] = []

    def add(name, seqs, ends, cell, **kw):
        out.append(PileupCase(name, k, seqs, ends if kw.get("singles", False) else _even(rng, ends), cell, **kw))

    read = sub(a[5:5 + K + 20], K + 10)
    add("a_read_and_its_reverse_complement", [a, b], [read, revcomp(read)],
        "the same forward-strand column at the same position, once in each plane", tally=(2, 0), tells=("plane1_unmirrored", "plane1_uncomplemented"))
    add("reverse_complemented_read_first_with_one_mismatch_each", [a, b], [revcomp(sub(a[5:5 + K + 20], K + 10)), sub(a[30:30 + K + 20], 2)],
        "the plane is the alignment's strand: the FIRST end of the pair lies in plane 1, the second in plane 0", tally=(2, 0), tells=ALL_PILE)
    half = dna(rng, K // 2 + 3)
    pal = half + revcomp(half)
    add("palindromic_overlap", [pal, b], [sub(pal, 1), b[:K - 1]], "one read, one alignment per strand: 1 in each plane, the mismatch at mirror positions",
        tally=(2, 0), tells=("plane1_unmirrored", "plane1_uncomplemented"))
    n_read = a[33:33 + K + 25]
    add("an_N_in_a_plane_1_read", [a, b], [revcomp(with_n(n_read, K + 3)), n_read[:K + 2]], "`other` of plane 1, at the mirrored position; plane 0 has depth only",
        tally=(2, 0), tells=("planes_swapped", "strand_by_mate", "plane1_unmirrored"))
    seqs = [a, b, c]
    flush = [sub(s[len(s) - (K + 9):], 3) for s in seqs]
    flush_rc = [revcomp(sub(s[len(s) - (K + 9):], 6)) for s in seqs]  # (another mismatch: the planes are not mirror images of each other)
    add("overlap_flush_with_the_end_of_every_segment_on_each_strand", seqs, flush_rc + flush,
        "the -1 lands in the segment's sentinel of ITS plane -- for the last segment slot S - 1 of plane 0, not slot 0 of plane 1",
        tally=(6, 0), tells=ALL_PILE)
    start = [sub(s[:K + 9], -4) for s in seqs]
    start_rc = [revcomp(sub(s[:K + 9], -7)) for s in seqs]
    add("overlap_flush_with_the_start_of_every_segment_on_each_strand", seqs, start_rc + start,
        "the +1 lands in the segment's first slot of its plane -- for the first segment slot 0 of plane 1 right behind plane 0's last sentinel",
        tally=(6, 0), tells=ALL_PILE)
    add("a_segment_shorter_than_K_between_two_long_ones", [a, short, b], [flush_rc[0], start[1], flush[0], start_rc[1], short, revcomp(short)],
        "the short segment owns no slot in either plane; its neighbours' slots follow each other", tally=(4, 0), tells=ALL_PILE)
    add("singles_block_with_absent_ends", [a, b], [revcomp(sub(a[3:3 + K + 9], K + 4)), "", dna(rng, K - 1), a[40:40 + K + 4]],
        "every read is an EVEN end: the plane cannot come from the parity; absent, empty and short ends count nothing", singles=True, tally=(2, 0),
        tells=("planes_swapped", "plane1_unmirrored", "plane1_uncomplemented"))
    add("a_block_of_65_ends", [a, b], _many(rng, a, K, 65), "the second batch of a wavefront holds one end", tally=(65, 0), tells=ALL_PILE)
    add("a_block_of_one_end_more_than_a_workgroups_least_share", [a, b], _many(rng, a, K, MIN_ENDS + 1), "the second workgroup holds one end",
        tally=(MIN_ENDS + 1, 0), tells=ALL_PILE)
    x = a[10:10 + K + 12]
    add("rejected_on_one_strand_beside_credited_on_the_other", [a, b], [revcomp(sub(x, K + 2, K + 5)), sub(x, K + 2, K + 5, K + 8)],
        "two mismatches are credited in plane 1; three against a budget of two deposit nothing in plane 0", M=2, tally=(1, 1), tells=ALL_PILE)
    return out
