"""The definition of the base pileup (``vs_node_pileup``, ``PileupCounter``, ``vstrains_amd.node_depth --pileup / --variants``),
stated as plain Python over strings.  With K = k + 1 and a mismatch budget M (an integer >= 0):

* a read end ``e`` (bytes as the ingest delivers them), a segment ``n`` with ``len_n >= K``, a strand ``t`` (0: the forward
  text, 1: the reverse complement) and a diagonal ``d = strand offset - read offset`` make a candidate alignment; its
  OVERLAP is the read offsets ``x`` with ``0 <= x < len_e`` and ``0 <= x + d < len_n``;
* a position AGREES when the read byte is one of ACGT and equals the strand's base;
* the alignment is ANCHORED when its overlap holds a run of at least K consecutive agreeing positions;
* an anchored alignment is CREDITED when the non-agreeing positions of its whole overlap number at most M (a byte outside
  ACGT does not agree); it counts ONCE, however many runs of K lie on its diagonal; a rejected one deposits nothing and is
  tallied;
* for every overlap position of a credited alignment, ``p`` the forward offset on the segment (``x + d``, or
  ``len_n - 1 - (x + d)`` on the reverse complement): ``depth[n][p] += 1``, and where the position does not agree
  ``alt[n][p][c] += 1``, ``c`` the read's base as it reads on the forward strand (complemented for the reverse complement),
  column 4 for a byte outside ACGT.

``pileup`` is the definition.  ``brute=True`` walks every diagonal there is; otherwise the anchored diagonals are found
through a table of the strands' K-windows (a run of K agreeing positions IS a K-window of the read, all ACGT, equal to a
K-window of the strand) and everything else is computed the same way: tests/test_pileup_model_cpu.py holds the two to each
other and the anchored set to tests/depth_profile_model.py's matches.  ``variant``: a named mistake, made on purpose, that
the constructed cases (tests/pileup_cases.py) must be able to tell from the truth."""
from typing import Dict, List, Optional, Sequence, Tuple

ACGT = "ACGT"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
VARIANTS = ("per_match", "no_complement", "no_mirror", "unclipped", "budget_lt", "n_free")


def revcomp(s: str) -> str:
    """(a byte outside ACGT stays what it is)"""
    return "".join(_COMP.get(c, c) for c in reversed(s))


def overlap(len_e: int, len_n: int, d: int) -> Tuple[int, int]:
    """[x_lo, x_hi): the read offsets x with 0 <= x < len_e and 0 <= x + d < len_n (empty: x_lo >= x_hi)."""
    return max(0, -d), min(len_e, len_n - d)


def agreement(end: str, text: str, d: int) -> Tuple[int, List[bool]]:
    x_lo, x_hi = overlap(len(end), len(text), d)
    return x_lo, [end[x] in ACGT and end[x] == text[x + d] for x in range(x_lo, x_hi)]


def runs_of(agree: Sequence[bool], K: int) -> int:
    """How many maximal runs of at least K agreeing positions."""
    n = run = 0
    for ok in list(agree) + [False]:
        if ok:
            run += 1
        else:
            n += run >= K
            run = 0
    return n


def strands(seq: str) -> Tuple[str, str]:
    return seq, revcomp(seq)


def _window_table(seqs: Sequence[str], K: int) -> Dict[str, List[Tuple[int, int, int]]]:
    table: Dict[str, List[Tuple[int, int, int]]] = {}
    for n, seq in enumerate(seqs):
        for t, text in enumerate(strands(seq)):
            for q in range(len(text) - K + 1):
                table.setdefault(text[q:q + K], []).append((n, t, q))
    return table


def anchored(seqs: Sequence[str], ksize: int, ends: Sequence[str], brute: bool = False, table=None):
    """Every anchored alignment, once: (end index, segment, strand, diagonal, x_lo, agreement over the overlap, runs of K)."""
    K = ksize + 1
    out = []
    if not brute and table is None:
        table = _window_table(seqs, K)
    for e, end in enumerate(ends):
        if end is None or len(end) < K:
            continue
        if brute:
            cand = [(n, t, d) for n, seq in enumerate(seqs) if len(seq) >= K for t in (0, 1) for d in range(-(len(end) - 1), len(seq))]
        else:
            cand = sorted(set((n, t, q - i) for i in range(len(end) - K + 1) for n, t, q in table.get(end[i:i + K], ())))
        for n, t, d in cand:
            x_lo, agree = agreement(end, strands(seqs[n])[t], d)
            r = runs_of(agree, K)
            if r:
                out.append((e, n, t, d, x_lo, agree, r))
    return out


def pileup(seqs: Sequence[str], ksize: int, ends: Sequence[Optional[str]], max_mismatch: int = 8, variant: Optional[str] = None, brute: bool = False):
    """-> (depth: per segment a list per position, alt: per segment a list of [A, C, G, T, other] per position,
    (alignments credited, alignments rejected)).  A segment shorter than K has no rows.  ``ends``: ``None`` is an absent end."""
    K = ksize + 1
    assert variant is None or variant in VARIANTS
    depth = [[0] * (len(s) if len(s) >= K else 0) for s in seqs]
    alt = [[[0] * 5 for _ in range(len(s) if len(s) >= K else 0)] for s in seqs]
    credited = rejected = 0
    for e, n, t, d, x_lo, agree, runs in anchored(seqs, ksize, ends, brute):
        end, len_n = ends[e], len(seqs[n])
        miss = sum(1 for ok in agree if not ok)
        if variant == "n_free":
            miss = sum(1 for i, ok in enumerate(agree) if not ok and end[x_lo + i] in ACGT)
        if variant == "unclipped":  # the read's bases beyond the segment compared too, with nothing
            miss += len(end) - len(agree)
        ok = miss < max_mismatch if variant == "budget_lt" else miss <= max_mismatch
        if not ok:
            rejected += 1
            continue
        times = runs if variant == "per_match" else 1
        credited += times
        for i, same in enumerate(agree):
            x = x_lo + i
            p = x + d if t == 0 or variant == "no_mirror" else len_n - 1 - (x + d)
            depth[n][p] += times
            if not same:
                b = end[x]
                if b not in ACGT:
                    c = 4
                else:
                    c = ACGT.index(b if t == 0 or variant == "no_complement" else _COMP[b])
                alt[n][p][c] += times
    return depth, alt, (credited, rejected)


def flat(depth, alt):
    """(offsets [N + 1], depth [P], alt [P][5]): the shape ``PileupCounter.result`` hands out."""
    offsets, dd, aa = [0], [], []
    for drow, arow in zip(depth, alt):
        dd += list(drow)
        aa += [list(a) for a in arow]
        offsets.append(len(dd))
    return offsets, dd, aa


def table_rows(ids: Sequence[str], seqs: Sequence[str], depth, alt) -> List[Tuple]:
    """The rows of the ``--pileup`` table: (segment, 1-based pos, ref, A, C, G, T, other); the reference base's count is the
    depth minus every alt column."""
    rows = []
    for name, seq, drow, arow in zip(ids, seqs, depth, alt):
        for p, (dp, a) in enumerate(zip(drow, arow)):
            counts = list(a[:4])
            counts[ACGT.index(seq[p])] = dp - sum(a)
            rows.append((name, p + 1, seq[p], counts[0], counts[1], counts[2], counts[3], a[4]))
    return rows


def variant_records(rows, min_alt_count: int = 2, min_alt_frac: float = 0.01) -> List[Tuple]:
    """The records of ``--variants`` from the table's rows: (segment, pos, ref, alt base, DP, AD, "%.6f" % AF), one per
    (position, non-reference base) with AD >= min_alt_count and AD >= min_alt_frac * DP (and at least one read), DP = A + C + G + T."""
    out = []
    for name, pos, ref, a, c, g, t, other in rows:
        dp = a + c + g + t
        for b, ad in zip(ACGT, (a, c, g, t)):
            if b != ref and ad > 0 and ad >= min_alt_count and ad >= min_alt_frac * dp:
                out.append((name, pos, ref, b, dp, ad, "%.6f" % (ad / dp)))
    return out
