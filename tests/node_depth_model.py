"""The definition of the depth pass (``vs_node_depth``, ``DepthCounter``, ``vstrains_amd.node_depth``), stated over the
oracle's table of the nodes' (k+1)-mers: KC[n] = the number of (read end, read offset, table entry of node n) triples whose
read window is a key holding that entry.  Every end counts, whatever its mate is like; a window over a byte outside ACGT is
no key; an end shorter than k+1 has no window.

``node_depth`` is the definition.  ``node_depth_by_matches`` restates it the way the kernel computes it -- maximal exact
matches of a read end with either strand of a node, ``len - K + 1`` per match -- and both take a ``variant``: a named
mistake, made on purpose, that the constructed cases (tests/node_depth_cases.py) must be able to tell from the truth."""
from typing import List, Optional, Sequence

from oracle.pe_oracle import build_table, revcomp
from seed_extend_model import geometry, phase

TABLE_VARIANTS = ("one_strand", "palindrome_once", "pair_filter")
MATCH_VARIANTS = ("per_grid_point", "len_not_windows")


def _filtered(ends: Sequence[str], K: int) -> List[str]:
    """The mistake of applying the PE filter (PE_Inference.py:160-165): the ends of a pair with an 'N' or a short end dropped."""
    out = []
    for i in range(0, len(ends) - 1, 2):
        a, b = ends[i], ends[i + 1]
        if "N" in a or "N" in b or len(a) < K or len(b) < K:
            continue
        out += [a, b]
    return out


def node_depth(seqs: Sequence[str], ksize: int, ends: Sequence[str], table=None, variant: Optional[str] = None) -> List[int]:
    K = ksize + 1
    assert variant is None or variant in TABLE_VARIANTS
    if variant == "one_strand":
        table = {}
        for idx, seq in enumerate(seqs):
            for off in range(len(seq) - K + 1):
                table.setdefault(seq[off:off + K], []).append((idx, off))
    elif table is None:
        table = build_table(seqs, K)
    if variant == "pair_filter":
        ends = _filtered(ends, K)
    kc = [0] * len(seqs)
    for end in ends:
        for i in range(len(end) - K + 1):
            bucket = table.get(end[i:i + K], ())
            if variant == "palindrome_once":
                bucket = set(bucket)
            for node, _off in bucket:
                kc[node] += 1
    return kc


def window_entries(seqs: Sequence[str], ksize: int, ends: Sequence[str], table=None) -> List[int]:
    """Table entries per window, for every window of every end (0 for a window that is no key)."""
    K = ksize + 1
    table = build_table(seqs, K) if table is None else table
    return [len(table.get(end[i:i + K], ())) for end in ends for i in range(len(end) - K + 1)]


def node_depth_by_matches(seqs: Sequence[str], ksize: int, ends: Sequence[str], variant: Optional[str] = None) -> List[int]:
    """The same sums from maximal exact matches: on every diagonal of (end, strand of a node) the runs of equal ACGT bases;
    a run of ``L >= K`` bases holds ``L - K + 1`` windows, each one table entry of that node."""
    K = ksize + 1
    assert variant is None or variant in MATCH_VARIANTS
    w, s = geometry(K)
    kc = [0] * len(seqs)
    for end in ends:
        if len(end) < K:
            continue
        grid = [phase(len(end), w, s) + p * s for p in range((len(end) - w + 1) // s)]
        for n, seq in enumerate(seqs):
            if len(seq) < K:
                continue
            for text in (seq, revcomp(seq)):
                for d in range(-(len(text) - K), len(end) - K + 1):  # read offset minus text offset
                    i = max(d, 0)
                    run = 0
                    stop = min(len(end), len(text) + d)
                    while i <= stop:
                        same = i < stop and end[i] == text[i - d] and end[i] in "ACGT"
                        if same:
                            run += 1
                        else:
                            if run >= K:
                                a = i - run
                                credit = run - K + 1
                                if variant == "len_not_windows":
                                    credit = run
                                if variant == "per_grid_point":
                                    credit *= sum(1 for g in grid if a <= g and g + w <= i)
                                kc[n] += credit
                            run = 0
                        i += 1
    return kc
