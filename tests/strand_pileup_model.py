"""The definition of the stranded pileup and of its records (``vs_node_pileup_strands``, ``vs_pileup_call``,
``StrandPileupCounter``, ``vstrains_amd.node_depth --strands``), stated as plain Python over strings, on top of
tests/pileup_model.py: overlap, agreement, anchoring, crediting within the budget M, once per diagonal, mirroring and
complementing on the reverse complement, column 4 for a byte outside ACGT -- all of that holds unchanged.

* The PLANE of a credited alignment is its strand ``t``: plane 0 -- the end's bytes, as the ingest delivers them, read along
  the segment's forward text; plane 1 -- read along the segment's reverse complement.  It is not the mate number and not the
  end's parity.
* For every overlap position ``depth[n][p][t] += 1``, and where it does not agree ``alt[n][p][t][c] += 1``, ``c`` as in the
  pileup.  Summed over ``t`` both tables are ``pileup_model.pileup``'s and the tallies are equal; a palindromic overlap puts 1
  into each plane; a read and its reverse complement put the same forward-strand column into different planes.
* A table row per plane: ``count[t][b] = alt[t][b]`` for ``b != ref``, ``count[t][ref] = depth[t] - sum(alt[t][0..4])``.
* RECORDS of one position: ``DP`` = the sum of ``count[t][b]`` over both planes and A, C, G, T (``other`` is left out); for
  every ``b != ref`` in ACGT order ``AD = count[0][b] + count[1][b]``, and ``b`` is a record when ``AD > 0``, ``AD >= C`` and
  ``AD >= F * DP`` -- the one double product Python forms there, no division (F = 0.07, DP = 100, AD = 7 is NOT a record:
  ``0.07 * 100 == 7.000000000000001``; F = 0.29, DP = 100, AD = 29 is one).  A record carries ``DP4 = (count[0][ref],
  count[1][ref], count[0][b], count[1][b])``; with a strand threshold ``S >= 1`` it FAILS when ``alt_f < S`` or ``alt_r < S``;
  the threshold never removes a record.

``variant``: a named mistake, made on purpose, that the constructed cases (tests/strand_pileup_cases.py,
tests/test_strand_pileup_model_cpu.py) must be able to tell from the truth."""
from typing import List, Optional, Sequence, Tuple

from pileup_model import ACGT, _COMP, anchored

PILE_VARIANTS = ("planes_swapped", "strand_by_mate", "plane1_unmirrored", "plane1_uncomplemented")
CALL_VARIANTS = ("dp_with_other", "frac_gt", "frac_by_division", "strand_on_total", "ref_from_plane0")
VARIANTS = PILE_VARIANTS + CALL_VARIANTS


def strand_pileup(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]], max_mismatch: int = 8, variant: Optional[str] = None):
    """-> (depth: per segment a list of [plane 0, plane 1] per position, alt: per segment a list of [[A, C, G, T, other] of
    plane 0, of plane 1] per position, (alignments credited, alignments rejected)).  A segment shorter than K has no rows."""
    K = ksize + 1
    assert variant is None or variant in PILE_VARIANTS
    rows = [len(s) if len(s) >= K else 0 for s in seqs]
    depth = [[[0, 0] for _ in range(r)] for r in rows]
    alt = [[[[0] * 5, [0] * 5] for _ in range(r)] for r in rows]
    credited = rejected = 0
    for e, n, t, d, x_lo, agree, runs in anchored(seqs, ksize, ends):
        end, len_n = ends[e], len(seqs[n])
        if sum(1 for ok in agree if not ok) > max_mismatch:
            rejected += 1
            continue
        credited += 1
        plane = t
        if variant == "planes_swapped":
            plane = 1 - t
        if variant == "strand_by_mate":
            plane = e & 1
        for i, same in enumerate(agree):
            x = x_lo + i
            p = x + d if t == 0 or variant == "plane1_unmirrored" else len_n - 1 - (x + d)
            depth[n][p][plane] += 1
            if not same:
                b = end[x]
                c = 4 if b not in ACGT else ACGT.index(b if t == 0 or variant == "plane1_uncomplemented" else _COMP[b])
                alt[n][p][plane][c] += 1
    return depth, alt, (credited, rejected)


def plane_sum(depth, alt):
    """Both tables summed over the planes: the shape of ``pileup_model.pileup``'s."""
    return [[d[0] + d[1] for d in row] for row in depth], [[[a[0][c] + a[1][c] for c in range(5)] for a in row] for row in alt]


def flat(depth, alt):
    """(offsets [N + 1], depth [P][2], alt [P][2][5]): the shape ``StrandPileupCounter.result`` hands out."""
    offsets, dd, aa = [0], [], []
    for drow, arow in zip(depth, alt):
        dd += [list(d) for d in drow]
        aa += [[list(a[0]), list(a[1])] for a in arow]
        offsets.append(len(dd))
    return offsets, dd, aa


def plane_counts(ref: str, depth: Sequence[int], alt: Sequence[Sequence[int]], variant: Optional[str] = None) -> List[List[int]]:
    """count[t] = [A, C, G, T, other] of one position, per plane: the alt columns as counted, and in the column of the
    segment's base the reads that agree."""
    r = ACGT.index(ref)
    out = []
    for t in range(len(depth)):
        src = 0 if variant == "ref_from_plane0" else t
        row = list(alt[t])
        row[r] = depth[src] - sum(alt[src])
        out.append(row)
    if len(out) == 1:
        out.append([0] * 5)
    return out


def position_records(ref: str, depth: Sequence[int], alt: Sequence[Sequence[int]], min_alt_count: int = 2, min_alt_frac: float = 0.01,
                     min_alt_strand: int = 0, variant: Optional[str] = None) -> List[Tuple]:
    """The records of one position with the segment's base ``ref``; ``depth``: one count per plane, ``alt``: five columns per
    plane (one plane: the unstranded tables; its second plane is zeros).
    -> [(alt base, DP, AD, (ref_f, ref_r, alt_f, alt_r), strand_fail)], in ACGT order."""
    assert variant is None or variant in CALL_VARIANTS
    count = plane_counts(ref, depth, alt, variant)
    r = ACGT.index(ref)
    dp = sum(count[t][b] for t in (0, 1) for b in range(5 if variant == "dp_with_other" else 4))
    out = []
    for b in range(4):
        if b == r:
            continue
        alt_f, alt_r = count[0][b], count[1][b]
        ad = alt_f + alt_r
        if variant == "frac_gt":
            enough = ad > min_alt_frac * dp
        elif variant == "frac_by_division":
            enough = dp > 0 and ad / dp >= min_alt_frac
        else:
            enough = ad >= min_alt_frac * dp
        if ad > 0 and ad >= min_alt_count and enough:
            if variant == "strand_on_total":
                fail = min_alt_strand >= 1 and ad < min_alt_strand
            else:
                fail = min_alt_strand >= 1 and (alt_f < min_alt_strand or alt_r < min_alt_strand)
            out.append((ACGT[b], dp, ad, (count[0][r], count[1][r], alt_f, alt_r), bool(fail)))
    return out


PILEUP_COLUMNS = ("segment", "pos", "ref", "A+", "C+", "G+", "T+", "other+", "A-", "C-", "G-", "T-", "other-")


def table_rows(ids: Sequence[str], seqs: Sequence[str], depth, alt) -> List[Tuple]:
    """The rows of the stranded ``--pileup`` table: (segment, 1-based pos, ref, A+ C+ G+ T+ other+, A- C- G- T- other-)."""
    rows = []
    for name, seq, drow, arow in zip(ids, seqs, depth, alt):
        for p, (d, a) in enumerate(zip(drow, arow)):
            count = plane_counts(seq[p], d, a)
            rows.append((name, p + 1, seq[p]) + tuple(count[0]) + tuple(count[1]))
    return rows


def variant_records(ids: Sequence[str], seqs: Sequence[str], depth, alt, min_alt_count: int = 2, min_alt_frac: float = 0.01,
                    min_alt_strand: int = 0, variant: Optional[str] = None) -> List[Tuple]:
    """The records of the stranded ``--variants``: (segment, pos, ref, alt base, DP, AD, "%.6f" % AF, DP4, FILTER), in file
    order, then by position, then by base; FILTER is ``.`` without a strand threshold, else ``PASS`` or ``strand``."""
    out = []
    for name, seq, drow, arow in zip(ids, seqs, depth, alt):
        for p, (d, a) in enumerate(zip(drow, arow)):
            for base, dp, ad, dp4, fail in position_records(seq[p], d, a, min_alt_count, min_alt_frac, min_alt_strand, variant):
                flt = "." if min_alt_strand < 1 else ("strand" if fail else "PASS")
                out.append((name, p + 1, seq[p], base, dp, ad, "%.6f" % (ad / dp), dp4, flt))
    return out


def unstranded(records) -> List[Tuple]:
    """The records with DP4 and FILTER dropped: what ``pileup_model.variant_records`` gives on the summed planes."""
    return [r[:7] for r in records]
