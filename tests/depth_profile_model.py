"""The definition of the depth profile (``vs_node_cover``, ``CoverCounter``, ``vstrains_amd.node_depth --profile``), stated
over the oracle's table of the nodes' (k+1)-mers.  With K = k + 1, for node n and forward offset p in [0, len_n - K]:

    cov[n][p] = the number of (read end, read offset i, table entry (n, p)) triples whose read window end[i : i + K] is a
                key holding that entry

-- the triples ``node_depth_model.node_depth`` counts per node, kept apart by their entry's offset.  The value belongs to
the window that STARTS at p: k-mer coverage, not base coverage.

``node_cover`` is the definition.  ``node_cover_by_matches`` restates it the way the kernel computes it: maximal exact
matches of a read end with either strand of a node, each written as +1 / -1 into a difference array in which every node of
K bases or more owns one slot per window and ONE sentinel slot behind them, and a scan.  It takes a ``variant``: a named
mistake, made on purpose, that the constructed cases (tests/depth_profile_cases.py) must be able to tell from the truth."""
from typing import Dict, List, Optional, Sequence, Tuple

from oracle.pe_oracle import build_table, revcomp
from seed_extend_model import geometry, phase

MATCH_VARIANTS = ("no_mirror", "leak_past_end", "first_window_only", "per_grid_point", "palindrome_once")


def node_cover(seqs: Sequence[str], ksize: int, ends: Sequence[str], table=None) -> List[List[int]]:
    K = ksize + 1
    table = build_table(seqs, K) if table is None else table
    cov = [[0] * max(len(s) - K + 1, 0) for s in seqs]
    for end in ends:
        for i in range(len(end) - K + 1):
            for node, off in table.get(end[i:i + K], ()):
                cov[node][off] += 1
    return cov


def row_sums(cov: Sequence[Sequence[int]]) -> List[int]:
    return [sum(row) for row in cov]


def flat(cov: Sequence[Sequence[int]]) -> Tuple[List[int], List[int]]:
    """(offsets [N + 1], values [W]): the shape ``CoverCounter.result`` hands out."""
    offsets, values = [0], []
    for row in cov:
        values += list(row)
        offsets.append(len(values))
    return offsets, values


def strand_table(seqs: Sequence[str], K: int) -> Dict[str, List[Tuple[int, int, int]]]:
    """window text -> (node, strand, offset in THAT strand's text): the forward text's windows and the reverse complement's."""
    table: Dict[str, List[Tuple[int, int, int]]] = {}
    for n, seq in enumerate(seqs):
        for strand, text in enumerate((seq, revcomp(seq))):
            for q in range(len(text) - K + 1):
                table.setdefault(text[q:q + K], []).append((n, strand, q))
    return table


def maximal_matches(seqs: Sequence[str], ksize: int, end: str, table=None) -> List[Tuple[int, int, int, int, int]]:
    """(read offset a, node, strand, offset qa in the strand's text, length) of every maximal exact match of K bases or more:
    the runs of consecutive read windows that hit the same strand of a node on the same diagonal."""
    K = ksize + 1
    table = strand_table(seqs, K) if table is None else table
    runs: Dict[Tuple[int, int, int], List[int]] = {}  # (node, strand, diagonal) -> read offsets, ascending
    for i in range(len(end) - K + 1):
        for n, strand, q in table.get(end[i:i + K], ()):
            runs.setdefault((n, strand, i - q), []).append(i)
    out = []
    for (n, strand, d), offs in runs.items():
        a = prev = offs[0]
        for i in offs[1:] + [None]:
            if i is None or i != prev + 1:
                out.append((a, n, strand, a - d, prev - a + K))
                a = i
            prev = i
    return out


def node_cover_by_matches(seqs: Sequence[str], ksize: int, ends: Sequence[str], variant: Optional[str] = None,
                          order: Optional[Sequence[int]] = None) -> List[List[int]]:
    """``order``: the numbering the index gave the nodes (internal number -> position in ``seqs``), in which the slots are
    laid out; the result is in the order of ``seqs`` whatever it is.  A node's profile is read from its OWN slots, a running
    sum from its first slot on; the kernel's fold scans all slots in one piece, which is the same thing exactly when every
    node's slots sum to 0 -- what the sentinel slot is for, and what the true form asserts."""
    K = ksize + 1
    assert variant is None or variant in MATCH_VARIANTS
    w, s = geometry(K)
    order = list(range(len(seqs))) if order is None else list(order)
    sentinel = 0 if variant == "leak_past_end" else 1
    first = {}
    total = 0
    for n in order:
        first[n] = total
        if len(seqs[n]) >= K:
            total += len(seqs[n]) - K + 1 + sentinel
    diff = [0] * total
    table = strand_table(seqs, K)
    for e, end in enumerate(ends):
        if len(end) < K:
            continue
        grid = [phase(len(end), w, s) + p * s for p in range((len(end) - w + 1) // s)]
        seen = set()
        for a, n, strand, qa, length in maximal_matches(seqs, ksize, end, table):
            p0 = qa if strand == 0 or variant == "no_mirror" else len(seqs[n]) - qa - length
            windows = length - K + 1
            credit = 1
            if variant == "per_grid_point":
                credit = sum(1 for g in grid if a <= g and g + w <= a + length)
                assert credit >= 1
            if variant == "first_window_only":
                windows = 1
            if variant == "palindrome_once":  # window by window, an entry once per read offset
                for t in range(windows):
                    i = a + t
                    p = p0 + t if strand == 0 else p0 + windows - 1 - t
                    if (i, n, p) not in seen:
                        seen.add((i, n, p))
                        diff[first[n] + p] += 1
                        diff[first[n] + p + 1] -= 1
                continue
            lo, hi = first[n] + p0, first[n] + p0 + windows
            if 0 <= lo < total:
                diff[lo] += credit
            if 0 <= hi < total:  # (without the sentinel the last node's -1 has no slot at all)
                diff[hi] -= credit
    cov = []
    for n, seq in enumerate(seqs):
        row, run = [], 0
        slots = len(seq) - K + 1 + sentinel if len(seq) >= K else 0
        for i in range(slots):
            run += diff[first[n] + i]
            row.append(run & 0xFFFFFFFF)
        if variant is None:
            assert sum(diff[first[n]:first[n] + slots]) == 0 and (not slots or row[-1] == 0)
        cov.append(row[:max(len(seq) - K + 1, 0)])
    return cov
