"""The definition of the site-pair pass (``vs_node_site_pairs``, ``SitePairCounter``, ``vstrains_amd.node_depth --site-pairs``),
stated as plain Python over strings, on ``pileup_model.anchored``.  With K = k + 1, a mismatch budget M and a span:

* a SITE is (segment n, forward position p) with ``len_n >= K`` and ``0 <= p < len_n``; the site list is a set;
* a FRAGMENT is the two ends ``2p`` and ``2p + 1`` of a block -- in a singles block the one present end; an absent, empty or
  short end contributes nothing;
* the CREDITED alignments of an end are the pileup's (tests/pileup_model.py): anchored, once per diagonal, at most M
  non-agreeing positions in the whole overlap, both strands; a rejected one observes nothing;
* a credited alignment makes one RAW observation ``(site, c)`` for every site under its overlap, ``c`` the read's byte there as
  it reads on the forward strand: 0..3 = ACGT, complemented on the reverse-complement strand, 4 for a byte outside ACGT -- the
  column rule of ``alt``, taken at agreeing positions too;
* a fragment with more than ``CAP`` = 32 raw observations over both ends, before any reduction, is OVERFLOW: it deposits
  nothing and is tallied;
* REDUCTION: the fragment OBSERVES ``(s, c)`` once if every raw observation it holds of site s has the same c; otherwise s is
  DISCORDANT for it, left out and tallied once, and its other sites stay;
* DEPOSIT: for every pair ``s < t`` of distinct observed sites: both on one segment and ``pos_t - pos_s <= span`` ->
  ``pairs[s, t][c_s][c_t] += 1`` (stored); else the pair is UNSTORED and tallied;
* TALLIES: (fragments with a raw observation, overflow fragments, discordant (fragment, site) incidences, pairs stored, pairs
  unstored).

The reduction is a property of the SET of raw observations: ``shuffle`` permutes every fragment's list before it is looked
at, and nothing may change.  ``variant``: a named mistake, made on purpose, that the constructed cases
(tests/site_pairs_cases.py) must be able to tell from the truth."""
from typing import Dict, List, Optional, Sequence, Tuple

from pileup_model import ACGT, _COMP, anchored

CAP = 32
BASES = "ACGTN"  # the five columns as the table writes them
VARIANTS = ("per_end", "no_discordance", "twice_when_mates_overlap", "no_complement", "no_mirror", "span_lt", "cap_ge", "rejected_observe",
            "cross_segment_stored")


def site_list(sites) -> List[Tuple[int, int]]:
    """The site list as a set, ascending by (segment, position)."""
    return sorted(set((int(n), int(p)) for n, p in sites))


def raw_observations(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]], sites, max_mismatch: int = 8, singles: bool = False,
                     variant: Optional[str] = None) -> Dict[int, List[Tuple[Tuple[int, int], int]]]:
    """fragment -> its raw observations ((segment, position), c), in the order the alignments are found."""
    wanted = set(site_list(sites))
    raw: Dict[int, List] = {}
    for e, n, t, d, x_lo, agree, runs in anchored(seqs, ksize, ends):
        miss = sum(1 for ok in agree if not ok)
        if miss > max_mismatch and variant != "rejected_observe":
            continue
        end, len_n = ends[e], len(seqs[n])
        frag = e if singles or variant == "per_end" else e // 2
        for i in range(len(agree)):
            x = x_lo + i
            p = x + d if t == 0 or variant == "no_mirror" else len_n - 1 - (x + d)
            if (n, p) in wanted:
                b = end[x]
                c = 4 if b not in ACGT else ACGT.index(b if t == 0 or variant == "no_complement" else _COMP[b])
                raw.setdefault(frag, []).append(((n, p), c))
    return raw


def reduce_fragment(raw, variant: Optional[str] = None):
    """One fragment's raw list -> (its observations [(site, c)], ascending by site; the discordant sites)."""
    by: Dict = {}
    for site, c in raw:
        by.setdefault(site, []).append(c)
    kept, discordant = [], 0
    for site in sorted(by):
        cs = by[site]
        if len(set(cs)) == 1:
            kept += [(site, cs[0])] * (len(cs) if variant == "twice_when_mates_overlap" else 1)
        elif variant == "no_discordance":
            kept += [(site, c) for c in sorted(set(cs))]
        else:
            discordant += 1
    return kept, discordant


def site_pairs(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]], sites, max_mismatch: int = 8, span: int = 1000, singles: bool = False,
               variant: Optional[str] = None, shuffle=None):
    """-> (pairs: {((n, pos_s), (n_t, pos_t)): 5 x 5 counts}, only the pairs some fragment stored; the five tallies).
    ``singles``: every end is a fragment of its own (a singles block: the second end of every pair is absent).  ``shuffle``: a
    ``numpy.random.Generator`` that permutes every fragment's raw list first."""
    assert variant is None or variant in VARIANTS
    pairs: Dict = {}
    seen = overflow = discordant = stored = unstored = 0
    for frag, raw in sorted(raw_observations(seqs, ksize, ends, sites, max_mismatch, singles, variant).items()):
        if shuffle is not None:
            raw = [raw[i] for i in shuffle.permutation(len(raw))]
        seen += 1
        if len(raw) >= CAP if variant == "cap_ge" else len(raw) > CAP:
            overflow += 1
            continue
        kept, bad = reduce_fragment(raw, variant)
        discordant += bad
        for i, (s, cs) in enumerate(kept):
            for t, ct in kept[i + 1:]:
                if s == t:  # (only a mistake keeps a site twice)
                    continue
                near = t[1] - s[1] < span if variant == "span_lt" else t[1] - s[1] <= span
                if (s[0] == t[0] and near) or (s[0] != t[0] and variant == "cross_segment_stored"):
                    pairs.setdefault((s, t), [[0] * 5 for _ in range(5)])[cs][ct] += 1
                    stored += 1
                else:
                    unstored += 1
    return pairs, (seen, overflow, discordant, stored, unstored)


def result_rows(pairs) -> List[Tuple]:
    """What ``SitePairCounter.result`` hands out, as a list: (segment, pos_a, pos_b, 5 x 5 counts), ascending."""
    return [(s[0], s[1], t[1], [list(r) for r in cell]) for (s, t), cell in sorted(pairs.items())]


def table_rows(ids: Sequence[str], pairs) -> List[Tuple]:
    """The rows of the ``--site-pairs`` table: (segment, 1-based pos_a, 1-based pos_b, base_a, base_b, count), non-zero counts
    only; segments in file order, then pos_a, pos_b, base_a, base_b in the order of ``BASES``."""
    out = []
    for (s, t), cell in sorted(pairs.items()):
        for a in range(5):
            for b in range(5):
                if cell[a][b]:
                    out.append((ids[s[0]], s[1] + 1, t[1] + 1, BASES[a], BASES[b], cell[a][b]))
    return out
