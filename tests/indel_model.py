"""The definition of the indel pass (``vs_node_indels``, ``IndelCounter``, ``vstrains_amd.node_depth --indels``), stated as
plain Python over strings, on tests/pileup_model.py's ``strands``, ``revcomp`` and agreement rule.  With K = k + 1 and a
maximum length G (1 <= G <= 32):

* R is a read end as the ingest delivers it, T a strand ``t`` of a segment ``n`` with ``len_n >= K``; ``(a, qa, len)`` is a
  maximal run of at least K agreeing positions of R laid on T (a position AGREES when the read byte is one of ACGT and equals
  the strand's base): the match the pileup's lane holds;
* the match is TESTED when ``a > 0`` and ``qa > 0``: its left neighbour lies inside both texts and does not agree;
* the candidates are tried in the order deletion 1, insertion 1, deletion 2, insertion 2, ... deletion G, insertion G, and
  the first that holds is the event -- a match yields at most one:

  - DELETION of L: ``a >= K`` and ``qa >= L + K``, and ``R[a-K : a]`` agrees with ``T[qa-L-K : qa-L]``; the strand's bases
    ``[qa-L, qa)`` are missing from the read;
  - INSERTION of L: ``a >= L + K`` and ``qa >= K``, and ``R[a-L-K : a-L]`` agrees with ``T[qa-K : qa]``; ``I = R[a-L : a]``
    stands before strand position ``qa``; if I holds a byte outside ACGT the event is DROPPED and tallied, and no further
    candidate is tried;

* NORMALISATION, F the segment's forward text: on strand 1 a deletion of ``[s, s+L)`` is forward ``[len_n-s-L, len_n-s)`` and
  an insertion of I before ``s`` is ``revcomp(I)`` before ``len_n - s``; then a deletion ``(u, L)`` moves to ``u - 1`` while
  ``u > 0 and F[u-1] == F[u+L-1]``, an insertion ``(u, I)`` becomes ``(u - 1, F[u-1] + I[:-1])`` while ``u > 0 and F[u-1] ==
  I[-1]``; the PLANE of the event is ``t``.

Per end and per strand: two mates over one event count two, a palindromic context may count on both strands.  ``variant``: a
named mistake, made on purpose, that the constructed cases (tests/indel_cases.py) must be able to tell from the truth."""
from typing import Dict, List, Optional, Sequence, Tuple

from pileup_model import ACGT, anchored, revcomp, strands

VARIANTS = ("longest_first", "ins_before_del", "no_left_align", "no_mirror", "no_complement", "flank_lt", "len_le", "n_agrees")
UNTESTED, NONE, EVENT, DROPPED = 0, 1, 2, 3  # the status codes of vs_indel_scan_host
DEL, INS = 0, 1


def matches(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]]):
    """Every maximal run of K or more agreeing positions: (end index, segment, strand, a, qa, length)."""
    K = ksize + 1
    out = []
    for e, n, t, d, x_lo, agree, _ in anchored(seqs, ksize, ends):
        start = None
        for i, ok in enumerate(list(agree) + [False]):
            if ok and start is None:
                start = i
            if not ok and start is not None:
                if i - start >= K:
                    out.append((e, n, t, x_lo + start, x_lo + start + d, i - start))
                start = None
    return out


def _agree(R: str, T: str, x: int, q: int, n: int, variant) -> bool:
    if variant == "n_agrees":
        return all(R[x + i] not in ACGT or R[x + i] == T[q + i] for i in range(n))
    return all(R[x + i] in ACGT and R[x + i] == T[q + i] for i in range(n))


def find(R: str, T: str, a: int, qa: int, K: int, G: int, variant: Optional[str] = None):
    """The candidate loop of one match -> (UNTESTED,), (NONE,), (DROPPED, INS, L) or (EVENT, kind, L, strand position, I): the
    raw event on the strand -- a deletion of the strand's ``[s, s + L)``, or I standing before ``s``."""
    if a <= 0 or qa <= 0:
        return (UNTESTED,)
    Kf = K - 1 if variant == "flank_lt" else K
    top = G + 1 if variant == "len_le" else G
    for L in (range(top, 0, -1) if variant == "longest_first" else range(1, top + 1)):
        for kind in ((INS, DEL) if variant == "ins_before_del" else (DEL, INS)):
            if kind == DEL:
                if a >= Kf and qa >= L + Kf and _agree(R, T, a - Kf, qa - L - Kf, Kf, variant):
                    return (EVENT, DEL, L, qa - L, "")
            elif a >= L + Kf and qa >= Kf and _agree(R, T, a - L - Kf, qa - Kf, Kf, variant):
                I = R[a - L:a]
                if any(c not in ACGT for c in I):
                    return (DROPPED, INS, L)
                return (EVENT, INS, L, qa, I)
    return (NONE,)


def normalise(F: str, t: int, kind: int, L: int, s: int, I: str, variant: Optional[str] = None) -> Tuple[int, str]:
    """The raw event of strand ``t`` in forward coordinates of the segment, left-aligned -> (u, I on the forward strand)."""
    mirrored = t == 1 and variant != "no_mirror"
    if kind == DEL:
        u = len(F) - s - L if mirrored else s
    else:
        u = len(F) - s if mirrored else s
        if t == 1:
            I = I[::-1] if variant == "no_complement" else revcomp(I)
    if variant != "no_left_align":
        if kind == DEL:
            while u > 0 and F[u - 1] == F[u + L - 1]:
                u -= 1
        else:
            while u > 0 and F[u - 1] == I[-1]:
                u, I = u - 1, F[u - 1] + I[:-1]
    return u, I


def scan(R: str, seq: str, t: int, a: int, qa: int, K: int, G: int, variant: Optional[str] = None):
    """One match through ``find`` and ``normalise`` -> (status, kind, L, u, I); what does not apply is 0 / ""."""
    got = find(R, strands(seq)[t], a, qa, K, G, variant)
    if got[0] in (UNTESTED, NONE):
        return (got[0], 0, 0, 0, "")
    if got[0] == DROPPED:
        return (DROPPED, got[1], got[2], 0, "")
    _, kind, L, s, I = got
    u, I = normalise(seq, t, kind, L, s, I, variant)
    return (EVENT, kind, L, u, I)


def indels(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]], G: int = 16, variant: Optional[str] = None):
    """-> (records, tallies): records sorted ``(segment, u, kind, L, I, count on plane 0, count on plane 1)``; tallies
    ``(matches tested, deletions, insertions, insertions dropped)``.  ``ends``: ``None`` is an absent end."""
    assert variant is None or variant in VARIANTS
    K = ksize + 1
    table: Dict[Tuple, List[int]] = {}
    tested = dels = ins = dropped = 0
    for e, n, t, a, qa, _ in matches(seqs, ksize, ends):
        status, kind, L, u, I = scan(ends[e], seqs[n], t, a, qa, K, G, variant)
        tested += status != UNTESTED
        dropped += status == DROPPED
        if status == EVENT:
            dels += kind == DEL
            ins += kind == INS
            table.setdefault((n, u, kind, L, I), [0, 0])[t] += 1
    return [key + tuple(v) for key, v in sorted(table.items())], (tested, dels, ins, dropped)

