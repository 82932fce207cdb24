"""What threading a contig through the graph means, stated once, as plain Python over strings (no packing, no seeds, no
matches): the definition ``k_contig_mems`` + ``vs_contig_chain`` are held to.

Take K = k + 1, a contig text ``c`` and the segments in GFA order.  Window ``i`` is ``c[i : i + K]``; its hits are all
(segment, strand, pos) where the strand's text (strand 1: the reverse complement) has the window at ``pos``.  A window over
a byte outside ACGT has none.  Left to right:

  continue  the previous window chose (n, s, p) and (n, s, p + 1) is a hit: take it, no new token;
  cross     else, p was the segment's last window (p == len(n) - K) and some hit has pos == 0: take the smallest such
            (segment, strand) and append a token to the current part -- a segment followed by itself is a new token;
  new part  else, the window has hits: the smallest (segment, strand, pos) starts a new part;
  break     a window without hits ends the current part.

Parts are joined by ``;\\n``; a part may begin or end inside a segment; a contig with no hit, or shorter than K, has no
parts; the ``L`` lines are not looked at; the entry ``NAME'`` is the mirror of the forward one.
"""
from typing import Dict, List, Sequence, Tuple

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
Hit = Tuple[int, int, int]


def revcomp(s: str) -> str:
    return "".join(_COMP[c] for c in reversed(s))


def window_table(seqs: Sequence[str], k: int) -> Dict[str, List[Hit]]:
    """Every (k+1)-mer of either strand of every segment -> its sorted (segment, strand, pos).  A segment that holds a byte
    outside ACGT is an error here as it is for the index."""
    K = k + 1
    table: Dict[str, List[Hit]] = {}
    for n, seq in enumerate(seqs):
        if len(seq) < K:
            continue
        for strand, text in ((0, seq), (1, revcomp(seq))):
            for p in range(len(text) - K + 1):
                table.setdefault(text[p:p + K], []).append((n, strand, p))
    for hits in table.values():
        hits.sort()
    return table


def thread(seqs: Sequence[str], k: int, contig: str, table=None):
    """-> (parts: lists of [segment, strand, windows the token was chosen for], windows with more than one hit)."""
    K = k + 1
    if table is None:
        table = window_table(seqs, k)
    parts: List[List[List[int]]] = []
    prev = None
    ambiguous = 0
    for i in range(len(contig) - K + 1):
        hits = table.get(contig[i:i + K], ())
        if not hits:
            prev = None
            continue
        ambiguous += len(hits) > 1
        chosen = None
        if prev is not None:
            n, s, p = prev
            if (n, s, p + 1) in hits:
                chosen = (n, s, p + 1)
                parts[-1][-1][2] += 1
            elif p == len(seqs[n]) - K:
                first = [h for h in hits if h[2] == 0]
                if first:
                    chosen = first[0]
                    parts[-1].append([chosen[0], chosen[1], 1])
        if chosen is None:
            chosen = hits[0]
            parts.append([[chosen[0], chosen[1], 1]])
        prev = chosen
    return parts, ambiguous


def tokens(parts, ids: Sequence[str]) -> List[List[str]]:
    return [[ids[n] + "+-"[s] for n, s, _ in part] for part in parts]


def mirror(parts):
    """The walk of the reverse entry: parts reversed, tokens reversed, signs flipped."""
    return [[[n, 1 - s, w] for n, s, w in reversed(part)] for part in reversed(parts)]


def entry(name: str, parts, ids: Sequence[str]) -> str:
    """The two entries of a .paths file for one contig."""
    out = ""
    for nm, pp in ((name, parts), (name + "'", mirror(parts))):
        out += "%s\n%s\n" % (nm, ";\n".join(",".join(t) for t in tokens(pp, ids)))
    return out


def mems(seqs: Sequence[str], k: int, contig: str, c: int = 0) -> List[Tuple[int, int, int, int, int]]:
    """Every maximal exact match of K bases or more between the contig and a strand of a segment, as the device reports
    them: (contig, first base in the contig, segment | strand << 31, first base in the strand's text, length), sorted.
    Found diagonal by diagonal over the strings: quadratic, for small cases only."""
    K = k + 1
    out = []
    for n, seq in enumerate(seqs):
        for strand, text in ((0, seq), (1, revcomp(seq))):
            for d in range(-(len(text) - 1), len(contig)):  # diagonal: contig offset - text pos
                i, p = max(d, 0), max(-d, 0)
                run = 0
                while i <= len(contig) and p <= len(text):
                    same = i < len(contig) and p < len(text) and contig[i] == text[p] and contig[i] in _COMP
                    if same:
                        run += 1
                    else:
                        if run >= K:
                            out.append((c, i - run, n | (strand << 31), p - run, run))
                        run = 0
                    i += 1
                    p += 1
    return sorted(out)


def spell(parts_tokens: Sequence[Sequence[str]], seg_of: Dict[str, str], k: int) -> str:
    """The text of a .paths walk: the first segment of a part whole, then ``seg[k:]``; parts joined by ten ``N``."""
    texts = []
    for part in parts_tokens:
        s = ""
        for j, t in enumerate(part):
            x = seg_of[t[:-1]] if t[-1] == "+" else revcomp(seg_of[t[:-1]])
            s += x if j == 0 else x[k:]
        texts.append(s)
    return ("N" * 10).join(texts)


def read_paths(text: str):
    """A .paths file -> [(name, parts of tokens)] for every entry, primed ones included."""
    lines = text.split("\n")
    out = []
    i = 0
    while i < len(lines) and lines[i]:
        name = lines[i]
        i += 1
        parts = []
        while True:
            ln = lines[i]
            i += 1
            if ln.endswith(";"):
                parts.append(ln[:-1].split(","))
            else:
                parts.append(ln.split(","))
                break
        out.append((name, parts))
    return out
