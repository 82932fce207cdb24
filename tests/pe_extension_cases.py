"""Constructed read pairs for the stage between the seed index and the counters: the exact extension of a seed hit and the
acceptance test (vs_agree_fast / vs_agree_long / vs_extend / vs_seed_limits / vs_accept in vstrains_amd/csrc/vs_pe.hip),
with the accepted count v sitting ON the threshold -- pure Python, one fixed random.Random seed per shape; checked against
the oracles without a device by tests/test_pe_extension_cases_cpu.py and on the device by tests/test_pe_extension_gpu.py.

The reference keeps a node when v >= saturate or v * rlen >= span * (rlen - K), span = min(rlen, nlen) - K + 1.  A CUT
case is a node of nlen bases (K <= nlen <= rlen) of its own random text, embedded in a read with random flanks, with
one base of the read changed inside the node: the match is cut to l bases on one side of it, fewer than K on the other.
``saturate`` then cannot fire (see ``_needs_flank``), v = l - K + 1, and with T = ceil(span * (rlen - K) / rlen) the node
is kept exactly when v >= T.  For every nlen with T < span, either side of the cut and either strand there is one case with
v = T and one with v = T - 1: an extension that is one base long or short, on either side, flips one of them.

Across the family: the read's left flank varies, so that the match's start in the read and the seed's offset in the node
take every residue mod 16 (the shifts of alignbit); the changed base takes the three XOR patterns of the 2-bit code
(A<->C, A<->G, A<->T and the same on C / G / T); a share of the cuts is a byte outside ACGT instead -- a lower-case or
IUPAC letter where the pair must still count, N where the reference drops it -- over a node base A, which is what such
a byte packs to; some ends carry five more such bytes away from the match (the overflow kernels take those).

TEXT BEHIND THE NODE.  Where the match ends at the last base of the node's text as the device compares it (the forward
text for a cut on the left, the reverse complement for a cut on the right of a read given reverse-complemented), half
the cases continue the read with what FOLLOWS that text in the packed array of an index built with renumber=False: A up
to the 16-base word boundary, then the first bases of the next node.  A comparison that does not stop at the node's end
then counts on and v = T - 1 becomes accepted.  Only the device can show that: the string model and the oracles have no
neighbouring text.

FULL matches (no cut): reads that equal a node of rlen bases, and reads that overhang either end of one by 1, 15, 16, 17
bases.  They are accepted through ``saturate`` (hanging over the node's end, where saturate ignores the overhang, through
the second clause or, at k = 21 with 17 bases, not at all); they reach the `far` sentinel of the straight-line comparison
and ext == rem, but they pin nothing to +-1.

Every case read is paired with the exact text of ONE anchor node of rlen bases (the last node; its reverse complement in
half the pairs), so node_mat[case node][anchor] (or its transpose, where the case read is the reverse end: half the
cases) is 1 exactly when the case node is accepted."""
import functools
import random

import seed_extend_model as model

_XOR = {1: str.maketrans("ACGT", "CATG"), 2: str.maketrans("ACGT", "GTAC"), 3: str.maketrans("ACGT", "TGCA")}  # code ^ 1, ^ 2, ^ 3
_OTHER = "nacgtRYKMSWBDHV*"  # bytes outside ACGT that do not drop the pair
OVERHANGS = (1, 15, 16, 17)

# (k, read length) -> the k_pe_tiles instantiation a counting run takes for the block (asserted by both tests), and
# ``step``: every step-th node length (the long shapes are thinned as far as the coverage conditions of the CPU test allow)
SHAPES = {
    (55, 100): dict(kernel="k_pe_tiles<1, 7u, 2u", step=1),
    (55, 112): dict(kernel="k_pe_tiles<1, 7u, 3u", step=1),
    (55, 128): dict(kernel="k_pe_tiles<1, 8u, 3u", step=1),
    (55, 150): dict(kernel="k_pe_tiles<1, 10u, 4u", step=1),
    (31, 191): dict(kernel="k_pe_tiles<1, 0u, 0u", step=1),
    (21, 90): dict(kernel="k_pe_tiles<1, 0u, 0u", step=1),
    (55, 191): dict(kernel="k_pe_tiles<1, 0u, 0u", step=1),
    (127, 256): dict(kernel="k_pe_tiles<2, 16u, 2u", step=1),
    (127, 317): dict(kernel="k_pe_tiles<2, 0u, 0u", step=2),
    (94, 287): dict(kernel="k_pe_tiles<2, 0u, 0u", step=2),
    (140, 299): dict(kernel="k_pe_tiles<2, 0u, 0u", step=1),  # stride 79; the longest reads the long-window kernel takes at k = 140
    (140, 330): dict(kernel="k_pe_tiles<0, 0u, 0u", step=2),  # beyond its reach (276 bases behind the first probe of 330): the generic loops
    (31, 287): dict(kernel="k_pe_tiles<2, 0u, 0u", step=1),
}


def threshold(nlen: int, rlen: int, K: int):
    """(span, T): the k+1-windows of the shorter of node and read, and the smallest v the second clause accepts."""
    span = min(rlen, nlen) - K + 1
    return span, -(-span * (rlen - K) // rlen)


def _needs_flank(side: str, strand: int) -> str:
    """Which flank of the read AS WRITTEN (before the reverse complement of strand 1) must hold a base, or ''.
    saturate = right - coord - K + 2 with right = min(coord + nlen - 1, coord - kidx + rlen - 1) is span when the node's
    forward start lies in the read as mapped, and min(span, flank + v) when the match ends at the node's forward end:
    with no base behind that end it equals v and the node is accepted whatever the threshold."""
    if side == "L" and strand == 0:
        return "right"
    if side == "R" and strand == 1:
        return "left"
    return ""


def _text(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def knife_edge_family(k: int, rlen: int, step: int = 1, seed: int = None):
    """-> dict(seqs, fwd, rve, cases, anchor, K, w, s).  ``cases[p]`` describes pair p: kind 'cut' / 'full', node, nlen,
    side ('R': the cut lies right of the match, 'L': left), v, T, span, strand (1: the read is given reverse-complemented),
    end (0: the case read is fwd[p], 1: rve[p]), xor (1..3, 0: a byte outside ACGT -- ``byte``), extra (more such bytes in
    the end), behind (the read goes on with the text behind the node), accept (the intended answer)."""
    K = k + 1
    w, s = model.geometry(K)
    rng = random.Random(1000 * k + rlen if seed is None else seed)
    plan = []
    for nlen in range(K, rlen + 1, step):
        span, T = threshold(nlen, rlen, K)
        if T >= span:
            continue
        for side in "RL":
            for strand in (0, 1):
                for v in (T, T - 1):
                    l = v + K - 1
                    if v < 1 or nlen - l - 1 >= K:
                        continue
                    need = _needs_flank(side, strand)
                    if need and nlen == rlen:
                        continue
                    plan.append(dict(kind="cut", nlen=nlen, side=side, strand=strand, v=v, T=T, span=span, l=l, need=need))
    for strand in (0, 1):
        plan.append(dict(kind="full", nlen=rlen, side="", strand=strand, over=0))
        for o in OVERHANGS:
            for side in "RL":  # the read hangs over the node's right / left end by o bases
                plan.append(dict(kind="full", nlen=rlen, side=side, strand=strand, over=o))
    seqs = [_text(rng, c["nlen"]) for c in plan]
    anchor = len(seqs)
    seqs.append(_text(rng, rlen))
    for i, c in enumerate(plan):  # what varies from case to case, drawn independently of (nlen, side, strand, v)
        c.update(node=i, end=rng.randrange(2), mate_rc=rng.randrange(2), xor=rng.randrange(1, 4), byte="", extra=0, behind=False)
        if c["kind"] == "cut":
            c["cut"] = c["l"] if c["side"] == "R" else c["nlen"] - c["l"] - 1  # node offset of the changed base
            if rng.randrange(4) == 0:  # a byte outside ACGT over a node base A (what it packs to): only its position list / mask cuts here
                c["xor"], c["byte"] = 0, ("N" if rng.randrange(4) == 0 else rng.choice(_OTHER))
                seqs[i] = seqs[i][:c["cut"]] + "A" + seqs[i][c["cut"] + 1:]
            c["behind"] = bool(c["need"]) and rng.randrange(2) == 0
            c["extra"] = 5 if not c["behind"] and rng.randrange(12) == 0 else 0
    fwd, rve = [], []
    for i, c in enumerate(plan):
        nlen, strand, node = c["nlen"], c["strand"], seqs[i]
        if c["kind"] == "full":
            o = c["over"]
            read = node if not o else (node[o:] + _text(rng, o) if c["side"] == "R" else _text(rng, o) + node[:-o])
            v = rlen - o - K + 1  # saturate is v where the read as mapped hangs over the node's forward start or not at all, rlen - K + 1 otherwise
            c.update(v=v, accept=c["side"] == "" or (c["side"] == "R") == bool(strand) or v * rlen >= (rlen - K + 1) * (rlen - K))
        else:
            l, side, need, cut = c["l"], c["side"], c["need"], c["cut"]
            room = rlen - nlen
            # the left flank: at random among those that give the crediting probe the left extension whose turn it is (the
            # match starts that many bases before a point of the end's probe grid), so that every value up to s - 1 comes up
            turn, at = (i // 2 + 3 * (i // 8)) % s, (0 if side == "R" else cut + 1)
            fs = range(1 if need == "left" else 0, (room - 1 if need == "right" else room) + 1)
            start = (lambda f: rlen - (f + at + l)) if strand else (lambda f: f + at)  # of the match, in the read as given
            f = rng.choice([f for f in fs if (start(f) + turn - model.phase(rlen, w, s)) % s == 0] or fs)
            g = room - f
            left, right = _text(rng, f), _text(rng, g)
            if c["behind"]:  # the text behind the node, where the match ends at the last base of the text the device compares
                nxt = seqs[i + 1] if strand == 0 else model.rc(seqs[i + 1])
                behind = "A" * (-nlen % 16) + nxt[:K - 1]
                if strand == 0:
                    right = behind[:g] + right[len(behind[:g]):]
                else:
                    left = left[:max(0, f - len(behind))] + model.rc(behind[:f])
            read = list(left + node + right)
            read[f + cut] = c["byte"] or node[cut].translate(_XOR[c["xor"]])
            if c["extra"]:  # five more bytes outside ACGT away from the match and its two neighbours: more than a position list holds
                a = f + (0 if side == "R" else cut + 1)
                free = [p for p in range(rlen) if p < a - 1 or p > a + l]
                if len(free) >= 5:
                    for p in rng.sample(free, 5):
                        read[p] = rng.choice(_OTHER)
                else:
                    c["extra"] = 0
            read = "".join(read)
            c.update(f=f, accept=c["v"] >= c["T"])
        if strand:
            read = "".join(model._C.get(ch, ch) for ch in reversed(read))
        assert len(read) == rlen and len(seqs[i]) == nlen
        mate = model.rc(seqs[anchor]) if c["mate_rc"] else seqs[anchor]
        fwd.append(mate if c["end"] else read)
        rve.append(read if c["end"] else mate)
    return dict(seqs=seqs, fwd=fwd, rve=rve, cases=plan, anchor=anchor, K=K, w=w, s=s)


def case_read(fam, p):
    return (fam["rve"] if fam["cases"][p]["end"] else fam["fwd"])[p]


def dirty_bytes(read: str) -> int:
    return sum(ch not in "ACGT" for ch in read)
