"""Constructed blocks for the indel pass (``vs_node_indels``): segments of a few hundred bases and read ends of about 2K + G
bases in which one thing at a time can go wrong about finding an insertion or a deletion left of a match -- the order of the
candidates, the flank of exactly K bases, the room each candidate needs, the mirror and the left-alignment.  Every case names
the cell it is there for (``cell``), carries the records its construction fixes (``records``: ``(segment, u, kind, L, insert,
count on plane 0, count on plane 1)``, sorted) and, where the construction fixes them, the four tallies.
tests/test_indel_model_cpu.py holds tests/indel_model.py to them and the named mistakes to at least one case each;
tests/test_indel_scan_cpu.py runs every match of every case through the host export; tests/test_indels_gpu.py runs the cases
on the device at k = 21, 55 and 127 (K mod 32 = 22, 24, 0)."""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from indel_model import DEL, INS
from node_depth_cases import KS, _OTHER, dna  # noqa: F401  (KS: for the tests)
from pileup_cases import sub, with_n
from pileup_model import revcomp


class IndelCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    ends: List[str]
    cell: str                                  # what the case is there for
    records: List[Tuple]                       # the records the construction fixes
    G: int = 5                                 # the maximum length it runs with
    singles: bool = False                      # packed as a singles block: every second end absent
    tally: Optional[Tuple[int, int, int, int]] = None  # (tested, deletions, insertions, dropped) where the construction fixes them
    tells: tuple = ()                          # the named mistakes (indel_model.VARIANTS) this case must expose


def spot(F: str, lo: int, L: int) -> int:
    """The first u >= lo at which a deletion of L bases is left-aligned as it stands: F[u-1] != F[u+L-1]."""
    u = lo
    while F[u - 1] == F[u + L - 1]:
        u += 1
    return u


def insert_for(rng, F: str, u: int, L: int) -> str:
    """L random bases that stand left-aligned before u: the last is not F[u-1]."""
    I = dna(rng, L)
    return I[:-1] + _OTHER[I[-1]] if I[-1] == F[u - 1] else I


def del_read(F: str, u: int, L: int, fl: int, fr: int) -> str:
    """fl bases, F[u : u + L] missing, fr bases."""
    return F[u - fl:u] + F[u + L:u + L + fr]


def ins_read(F: str, u: int, I: str, fl: int, fr: int) -> str:
    """fl bases, I before position u, fr bases."""
    return F[u - fl:u] + I + F[u:u + fr]


def _even(rng, ends: List[str]) -> List[str]:
    """A block of pairs holds an even number of ends: an end of five bases, which counts nothing, fills it up."""
    return ends + [dna(rng, 5)] if len(ends) % 2 else ends


def indel_cases(k: int) -> List[IndelCase]:
    K = k + 1
    G = 5
    rng = np.random.default_rng(9100 + k)
    F = dna(rng, 6 * K + 150)
    other = dna(rng, 2 * K + 1)
    n = len(F)
    out: List[IndelCase] = []

    def add(name, seqs, ends, cell, records, **kw):
        singles = kw.get("singles", False)
        out.append(IndelCase(name, k, seqs, ends if singles else _even(rng, ends), cell, sorted(records), **kw))

    def pair(L, at_del, at_ins, fl=K + 3, fr=K + 3):
        """A read with a deletion of L near at_del and one with an insertion of L near at_ins -> (ends, records)."""
        u, v = spot(F, at_del, L), at_ins
        I = insert_for(rng, F, v, L)
        return [del_read(F, u, L, fl, fr), ins_read(F, v, I, fl, fr)], [(0, u, DEL, L, "", 1, 0), (0, v, INS, L, I, 1, 0)]

    ends, recs = pair(1, 2 * K, 4 * K)
    add("deletion_and_insertion_of_one_base", [F, other], ends, "the first candidates of the loop", recs, tally=(2, 1, 1, 0))
    ends, recs = pair(G, 2 * K, 4 * K)
    add("deletion_and_insertion_of_G_bases", [F, other], ends, "the last candidates of the loop", recs, tally=(2, 1, 1, 0))
    ends, _ = pair(G + 1, 2 * K, 4 * K)
    add("deletion_and_insertion_of_G_plus_1_bases", [F, other], ends, "one base too long: tested, nothing found", [], tally=(2, 0, 0, 0), tells=("len_le",))
    ends, recs = pair(2, 2 * K, 4 * K, fl=K)
    add("left_flank_of_exactly_K_bases", [F, other], ends, "a == K for the deletion and a == L + K for the insertion: the room limits at equality", recs,
        tally=(2, 1, 1, 0))
    ends, _ = pair(2, 2 * K, 4 * K, fl=K - 1)
    add("left_flank_of_K_minus_1_bases", [F, other], ends, "a == K - 1 and a == L + K - 1: one short of the room, nothing found", [], tally=(2, 0, 0, 0),
        tells=("flank_lt",))
    # the strand's side of the room: the event K bases behind the segment's start, the read overhanging the start with junk
    junk = dna(rng, 4)
    u = spot(F, K, 2)
    Fd = F if u == K else F[:K + 1] + _OTHER[F[K - 1]] + F[K + 2:]  # (F[K-1] != F[K+1]: the deletion at K is left-aligned as it stands)
    jd = junk[:-1] + _OTHER[Fd[1]]  # (the junk's last base does not continue the read's flank leftwards on the shifted diagonal)
    I2 = insert_for(rng, Fd, K, 2)
    ji = junk
    add("event_K_bases_behind_the_segments_start", [Fd, other], [jd + Fd[0:K] + Fd[K + 2:2 * K + 5], ji + Fd[0:K] + I2 + Fd[K:2 * K + 3]],
        "qa == L + K for the deletion and qa == K for the insertion: the room limits at equality", [(0, K, DEL, 2, "", 1, 0), (0, K, INS, 2, I2, 1, 0)])
    Fe = F[:K] + _OTHER[F[K - 2]] + F[K + 1:] if F[K - 2] == F[K] else F  # (the deletion of [K-1, K+1) left-aligned as it stands)
    I3 = insert_for(rng, Fe, K - 1, 2)
    add("event_K_minus_1_bases_behind_the_segments_start", [Fe, other], [junk + Fe[0:K - 1] + Fe[K + 1:2 * K + 5], junk + Fe[0:K - 1] + I3 + Fe[K - 1:2 * K + 3]],
        "qa == L + K - 1 and qa == K - 1 with room in the read: one short, nothing found", [], tells=("flank_lt",))
    u = spot(F, 3 * K, 1)
    base = del_read(F, u, 1, K + 5, K + 3)
    add("substitution_K_minus_1_and_K_bases_before_the_breakpoint", [F, other], [sub(base, 5), sub(base, 4)],
        "the K-th base left of the breakpoint is the flank's last: substituted, no event; one further left, an event", [(0, u, DEL, 1, "", 1, 0)],
        tally=(3, 1, 0, 0), tells=("flank_lt",))  # (the K bases between a substitution at 4 and the breakpoint are a match of their own, tested)
    ends, recs = [], []
    at = K + 40
    for r in (0, 1, 15):
        fl = K + (r - K) % 16  # a == fl for the deletion
        u = spot(F, at, 3)
        ends.append(del_read(F, u, 3, fl, K + 2))
        recs.append((0, u, DEL, 3, "", 1, 0))
        at = u + 20
        fl = K + (r - K - 3) % 16  # a == fl + 3 for the insertion
        I = insert_for(rng, F, at, 3)
        ends.append(ins_read(F, at, I, fl, K + 2))
        recs.append((0, at, INS, 3, I, 1, 0))
        at += 20
    add("breakpoints_at_a_mod_16_of_0_1_and_15", [F, other], ends, "the flank's windows start at, one behind and one before a word of the packed read", recs,
        tally=(6, 3, 3, 0))
    # repeats: the same record from a read and from its reverse complement, in the other plane
    h = 6
    A, B = dna(rng, 2 * K + h), dna(rng, 2 * K + h + 7)
    A = A[:-1] + ("C" if A[-1] == "A" else A[-1])
    B = ("C" if B[0] == "A" else B[0]) + B[1:]
    homo = A + "A" * h + B
    more = A[-(K + h):] + "A" * (h + 1) + B[:K + h]
    less = A[-(K + h):] + "A" * (h - 1) + B[:K + h]
    add("one_base_more_and_one_less_in_a_homopolymer", [homo, other], [more, revcomp(more), less, revcomp(less)],
        "the read's event stands at the run's start as it is; its reverse complement's stands at the run's end and moves there: one record, both planes",
        [(0, len(A), DEL, 1, "", 1, 1), (0, len(A), INS, 1, "A", 1, 1)], tally=(4, 2, 2, 0), tells=("no_left_align", "no_mirror", "no_complement"))
    A2 = dna(rng, 2 * K + 8)[:-4] + "GTGC"
    B2 = dna(rng, 2 * K + 19)
    B2 = ("T" if B2[0] in "AC" else B2[0]) + B2[1:]
    m = 4
    dinuc = A2 + "AC" * m + B2
    more = A2[-(K + 2 * m):] + "AC" * (m + 1) + B2[:K + 2 * m]
    add("one_unit_more_in_a_dinucleotide_repeat", [dinuc, other], [more, revcomp(more)],
        "the segment's C before (AC)4 makes the repeat (CA)4 C: the insert is the rotated CA one base before the AC's, from either strand",
        [(0, len(A2) - 1, INS, 2, "CA", 1, 1)], tally=(2, 0, 2, 0), tells=("no_left_align", "no_mirror", "no_complement"))
    units = (K + 6) // 3 + 2
    A3 = dna(rng, K + 10)
    A3 = A3[:-1] + ("T" if A3[-1] == "G" else A3[-1])
    B3 = dna(rng, 2 * K)
    micro = A3 + "ACG" * units + B3
    at = len(A3) + 3 * units
    add("a_base_inserted_behind_a_microsatellite_of_unit_3", [micro, other], [micro[at - (K + 7):at] + "T" + micro[at:at + K + 2], other[:K - 1]],
        "the flanks of insertion 1, 4 and 7 all lie in the repeat and all agree: the smallest length is the event", [(0, at, INS, 1, "T", 1, 0)], G=8,
        tells=("longest_first",))
    # a repeat of period 4 and a deletion of 2 at its end: the flank of insertion 2 lies in the repeat and agrees as well
    m4 = (K + 8) // 4 + 1
    A5 = dna(rng, K + 10)
    B5 = dna(rng, 2 * K)
    B5 = ("A" if B5[0] in "CT" else B5[0]) + B5[1:]
    quad = A5 + "ACGT" * m4 + B5
    u = len(A5) + 4 * m4 - 2
    add("a_deletion_of_2_at_the_end_of_a_repeat_of_period_4", [quad, other], [del_read(quad, u, 2, K + 3, K + 3), other[:K - 1]],
        "deletion 2 and insertion 2 both hold: the deletion is tried first and is the event", [(0, u, DEL, 2, "", 1, 0)], tells=("ins_before_del",))
    # the read that carries one A more than a run of K at the segment's start: seen on the reverse complement only
    B4 = dna(rng, 2 * K)
    B4 = ("C" if B4[0] == "A" else B4[0]) + B4[1:]
    edge = "A" * K + B4
    add("an_insertion_that_left_aligns_to_the_segments_first_base", [edge, other], [revcomp("A" * (K + 1) + B4[:K + 3]), other[:K - 1]],
        "on the reverse complement the event stands K bases inside and moves to u == 0 on the forward text; the anchor is the base behind it",
        [(0, 0, INS, 1, "A", 0, 1)], tells=("no_left_align", "no_mirror", "no_complement"))
    u, v = spot(F, 2 * K, 2), 4 * K
    I = insert_for(rng, F, v, 3)
    r_ins = ins_read(F, v, I, K + 4, K + 3)
    r_del = del_read(F, u, 2, K + 4, K + 3)
    add("an_N_in_the_insert_and_an_N_in_the_flank", [F, other], [with_n(r_ins, K + 5), with_n(r_ins, 6), with_n(r_del, 6), with_n(r_del, 2)],
        "an N among the inserted bases drops the event and is tallied; an N among the K flank bases is no flank; an N further left changes nothing",
        [(0, u, DEL, 2, "", 1, 0)], tally=(5, 1, 0, 1), tells=("n_agrees",))  # (the bases behind the N at 2 are a match of their own, tested)
    u = spot(F, 2 * K, 2)
    v = u + 2 + K + 6
    I = insert_for(rng, F, v, 2)
    two = F[u - (K + 2):u] + F[u + 2:v] + I + F[v:v + K + 2]
    add("two_indels_in_one_end", [F, other], [two, revcomp(two)], "each is emitted by the match to its right, on either strand",
        [(0, u, DEL, 2, "", 1, 1), (0, v, INS, 2, I, 1, 1)], tally=(4, 2, 2, 0), tells=("no_mirror", "no_complement"))
    u = spot(F, 3 * K, 1)
    cut = sub(del_read(F, u, 1, K + 2, 2 * K + 3), K + 2 + K)
    add("a_substitution_right_of_a_deletion", [F, other], [cut, other[:K - 1]],
        "the second match on the deletion's diagonal is tested too and finds no flank: one event", [(0, u, DEL, 1, "", 1, 0)], tally=(2, 1, 0, 0))
    u = spot(F, 3 * K, 3)
    add("mates_overlapping_one_deletion", [F, other], [del_read(F, u, 3, K + 6, K + 1), revcomp(del_read(F, u, 3, K + 1, K + 6))],
        "per end and per strand: two mates over one event are two events, one in each plane", [(0, u, DEL, 3, "", 1, 1)], tally=(2, 2, 0, 0),
        tells=("no_mirror",))
    short = dna(rng, K - 1)
    u = spot(F, 2 * K, 1)
    add("a_segment_shorter_than_K_and_an_end_shorter_than_2K", [short, F], [short, del_read(F, u, 1, K, K - 1), del_read(F, u, 1, K - 1, K), dna(rng, 3)],
        "no match, or one match with no room left of it, or a flank that is no match: nothing", [], tells=("flank_lt",))
    u, v = spot(F, 2 * K, 2), 4 * K
    I = insert_for(rng, F, v, 2)
    add("a_singles_block_with_an_empty_and_a_short_end", [F, other], [del_read(F, u, 2, K + 3, K + 3), "", dna(rng, K - 1), revcomp(ins_read(F, v, I, K + 3, K + 3))],
        "absent, empty and short ends find nothing; the reads of a singles block are found as those of pairs are", [(0, u, DEL, 2, "", 1, 0), (0, v, INS, 2, I, 0, 1)],
        singles=True, tally=(2, 1, 1, 0), tells=("no_mirror", "no_complement"))
    ends, recs = [], {}
    u, v = spot(F, 2 * K, 2), 4 * K
    I = insert_for(rng, F, v, 2)
    for e in range(70):
        if e in (5, 62, 63, 64, 65, 69):
            if e % 2:
                ends.append(revcomp(ins_read(F, v, I, K + 3, K + 3)) if e == 63 else ins_read(F, v, I, K + 3, K + 3))
                key, plane = (0, v, INS, 2, I), int(e == 63)
            else:
                ends.append(del_read(F, u, 2, K + 3, K + 3))
                key, plane = (0, u, DEL, 2, ""), 0
            recs.setdefault(key, [0, 0])[plane] += 1
        else:
            a = int(rng.integers(0, n - (K + 10)))
            ends.append(F[a:a + K + 10])
    add("a_block_of_70_ends", [F, other], ends, "a batch of 64 ends ends between two events: the records of both batches are claimed and counted",
        [key + tuple(c) for key, c in recs.items()], tally=(6, 2, 4, 0))
    return out
