"""Constructed graphs and contigs for the contig threader (``k_contig_mems`` + ``vs_contig_chain``): one thing at a time
that can go wrong.  What a case must give comes from tests/contig_thread_model.py; where the construction itself fixes the
walk it is written into the case (``want``: per contig the parts as strings of ``<segment index><sign>``, None = left out)
and tests/test_contig_thread_model_cpu.py holds the model to it.  tests/test_contig_thread_gpu.py runs the same cases on the
device at k = 21 (21-base seeds, stride 2) and one set at k = 127 (63-base seeds whose key only nominates, stride 66)."""
from typing import List, NamedTuple, Optional

import numpy as np

from contig_thread_model import revcomp

KS = (21, 127)
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}
FIRST_CAPACITY = 4096  # records of the match buffer's first allocation (MEMS_FIRST_CAP)
SHARE = 256            # probes a workgroup of k_contig_mems takes (MEMS_TPB)


class ThreadCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    contigs: List[str]
    want: Optional[List[Optional[List[str]]]] = None


def dna(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def stride(k: int) -> int:
    """The probe stride of the index at k: K - w + 1 with the seed length w = min(k, 31) made odd, 63 from k = 95 on."""
    K = k + 1
    w = 63 if k >= 95 else min(K, 31)
    w -= 1 - w % 2
    return K - w + 1


def chain_graph(rng, k: int, n_seg: int, seg_windows: int):
    """A genome cut into ``n_seg`` segments that overlap by k bases, as a compacted de Bruijn graph has them."""
    K = k + 1
    g = dna(rng, n_seg * seg_windows + k)
    return g, [g[i * seg_windows:(i + 1) * seg_windows + k] for i in range(n_seg)]


def small_cases(k: int) -> List[ThreadCase]:
    K = k + 1
    rng = np.random.default_rng(4000 + k)
    out: List[ThreadCase] = []
    g, three = chain_graph(rng, k, 3, 2 * K)
    c1, c2 = 2 * K, 4 * K  # the first windows of segments 1 and 2 in g
    other = dna(rng, 3 * K)

    out.append(ThreadCase("contig_of_exactly_K_bases", k, three + [other], [three[0][5:5 + K]], want=[["0+"]]))
    out.append(ThreadCase("contig_of_K_minus_1_bases", k, three + [other], [three[0][5:5 + K - 1], other[:K]], want=[None, ["3+"]]))
    out.append(ThreadCase("whole_segment_on_the_reverse_strand", k, three + [other], [revcomp(three[1]), revcomp(g)],
                          want=[["1-"], ["2-,1-,0-"]]))
    x = dna(rng, k)
    loop = x + dna(rng, K + 3) + x
    out.append(ThreadCase("self_loop", k, [loop, other], [loop + loop[k:], loop + loop[k:] + loop[k:]], want=[["0+,0+"], ["0+,0+,0+"]]))
    x, y = dna(rng, k), dna(rng, k)
    a, b = x + dna(rng, K + 2) + y, y + dna(rng, K + 5) + x
    out.append(ThreadCase("segment_visited_twice_with_another_between", k, [a, b, other], [a + b[k:] + a[k:], revcomp(a + b[k:] + a[k:])],
                          want=[["0+,1+,0+"], ["0-,1-,0-"]]))
    out.append(ThreadCase("start_and_end_inside_a_segment", k, three + [other], [g[10:c2 + K + 4], g[c1 - 3:c1 + K], g[c1 + 1:c1 + 1 + K + 2]],
                          want=[["0+,1+,2+"], ["0+,1+"], ["1+"]]))
    half = dna(rng, K // 2)
    pal = half + revcomp(half)
    pal_seg = dna(rng, K + 4) + pal + dna(rng, K + 6)
    at = K + 4
    # through the palindrome on either strand: continuity keeps the strand; a contig that BEGINS on it takes strand 0 (the
    # smaller hit), and has to leave the segment and come back (a second part) when that was the wrong one
    out.append(ThreadCase("palindromic_window_inside_a_segment", k, [other, pal_seg],
                          [pal_seg[3:-2], revcomp(pal_seg[3:-2]), pal_seg[at:at + K + 5], revcomp(pal_seg)[len(pal_seg) - at - K:][:K + 5], pal]))
    rep = dna(rng, K)
    n_a = dna(rng, K + 2) + rep + dna(rng, K + 5)
    n_b = dna(rng, K + 7) + rep + dna(rng, K + 1)
    out.append(ThreadCase("repeated_window_in_two_segments", k, [n_a, n_b, other], [n_b, n_a, revcomp(n_b), rep],
                          want=[["1+"], ["0+"], ["1-"], ["0+"]]))
    piece = g[7:c2 + 9]
    mid = len(piece) // 2
    with_n = piece[:mid] + "N" + piece[mid + 1:]
    with_sub = piece[:mid] + _OTHER[piece[mid]] + piece[mid + 1:]
    out.append(ThreadCase("one_N_and_one_substituted_base", k, three + [other], [with_n, with_sub, revcomp(with_sub)]))
    out.append(ThreadCase("contig_with_no_hit", k, three + [other], [dna(rng, 5 * K), other[:K + 3], "N" * (2 * K), ""],
                          want=[None, ["3+"], None, None]))
    return out


def long_cases(k: int) -> List[ThreadCase]:
    """Contigs whose probes exceed one round of 64 lanes, and one workgroup's share of 256 probes."""
    K = k + 1
    s = stride(k)
    rng = np.random.default_rng(5000 + k)
    out = []
    for name, probes in (("more_probes_than_one_round_of_64_lanes", 64 + 9), ("more_probes_than_one_workgroups_share", 2 * SHARE + 70)):
        n_seg = 5
        g, segs = chain_graph(rng, k, n_seg, (probes * s + K) // n_seg + 1)
        contigs = [g[3:-5], revcomp(g[9:-2]), segs[2]]
        out.append(ThreadCase(name, k, segs, contigs, want=[["0+,1+,2+,3+,4+"], ["4-,3-,2-,1-,0-"], ["2+"]]))
    return out


def past_first_capacity(k: int) -> ThreadCase:
    """More matches than the buffer's first allocation holds: the pass runs a second time in a buffer of the size it asked for."""
    K = k + 1
    rng = np.random.default_rng(6000 + k)
    segs = [dna(rng, 3 * K) for _ in range(5)]
    contigs = []
    for i in range(FIRST_CAPACITY + 150):
        n = segs[i % 5]
        a = (i * 7) % (len(n) - K - 3)
        c = n[a:a + K + (i % 4)]
        contigs.append(revcomp(c) if i % 3 == 0 else c)
    return ThreadCase("more_matches_than_the_first_capacity", k, segs, contigs)


def colliding_seed_case() -> ThreadCase:
    """k = 127: two 63-base seeds under one 62-bit key (tests/seed_index_model.py:colliding_seeds), each in a segment of its
    own between different flanks.  Contigs that hold one seed nominate both segments; only compared text may make a match.
    Every phase of the probe grid is met: the contigs start at every offset of a stride."""
    import seed_index_model as sim

    k, K = 127, 128
    rng = np.random.default_rng(7000)
    x = dna(rng, 63)
    y = sim.colliding_seeds(x, 1, rng)[0]
    f1, f2, g1, g2 = dna(rng, 70), dna(rng, 70), dna(rng, 70), dna(rng, 70)
    a, b = f1 + x + f2, g1 + y + g2
    orphan = f1 + y + f2  # the flanks of one, the seed of the other: no K bases of it are in the graph
    contigs, want = [], []
    for i in range(stride(k)):
        contigs += [a[i:], b[i:], revcomp(a)[i:], orphan[i:]]
        want += [["0+"], ["1+"], ["0-"], None]
    return ThreadCase("two_seeds_under_one_key", k, [a, b], contigs, want=want)
