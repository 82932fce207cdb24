"""String-level model of the device algorithm (seeds at stride s from the end's phase, canonical w-mer table, exact
extension, first-seed-owns-the-match rule).  It exists to pin the *algorithm* of
vstrains_amd/csrc/vs_pe.hip against the oracle on the CPU, where no GPU is available; the HIP
kernels themselves are checked against the oracle on the device: on random reads in tests/test_pe_gpu.py, and on matches
cut at every length -- the cases of tests/pe_extension_cases.py, whose coverage is read off this model's trace -- in
tests/test_pe_extension_gpu.py."""
from typing import Dict, List, Sequence, Tuple

_C = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s: str) -> str:
    return "".join(_C[c] for c in reversed(s))


def geometry(K: int) -> Tuple[int, int]:
    """seed_geometry (csrc/vs_index.hip): 31-base seeds, 63-base ones from K = k + 1 = 96 on, made odd."""
    w = 63 if K >= 96 else min(K, 31)
    if w % 2 == 0:
        w -= 1
    return w, K - w + 1


def build(seqs: Sequence[str], K: int, key_fn=None):
    """``key_fn`` (canonical seed text -> key, default the text itself): what the table files a seed under.  A function
    that is not injective -- the device's mixed key of a 63-base seed (vs_seed_key), or a lossy one a test makes up --
    puts different seeds into one bucket, and each then nominates the postings of the others."""
    w, s = geometry(K)
    table: Dict[str, List[Tuple[int, int, int]]] = {}
    for i, seq in enumerate(seqs):
        if len(seq) < K:
            continue
        for p in range(len(seq) - w + 1):
            f = seq[p : p + w]
            r = rc(f)
            key, strand = (f, 0) if f < r else (r, 1)
            if key_fn is not None:
                key = key_fn(key)
            table.setdefault(key, []).append((i, p, strand))
    return table, w, s


def phase(rlen: int, w: int, s: int) -> int:
    """First probe offset of an end (vs_seed_phase in csrc/vs_internal.h): any phase of the grid is exact; this one gives
    the fewest probes, floor((rlen - w + 1) / s)."""
    return ((rlen - w) % s + s) // 2 if rlen >= w else 0


def valid(ch: str) -> bool:
    return ch in _C


def step_grid(rlen: int, w: int, s: int, t: int) -> List[int]:
    """The adaptive grid of the compile-time-shape kernels (round 5): grid positions s-1, 2s-1, ... with the positions from
    the t-th on moved D = s - 2 - (rlen - w) mod s bases towards the read's start (t = 0: all of them, the lowest exact phase;
    t = n: none, the highest).  Every such grid starts within the first s offsets, ends within the last s, and has no gap
    wider than s -- so every match of K bases holds one of its points; which t an end gets (the one with the fewest
    postings) changes the work, not the result."""
    m = rlen - w
    n = max(1, (m + 1) // s)
    D = max(0, s - 2 - m % s)
    return [s - 1 + i * s - (D if i >= t else 0) for i in range(n)]


def seed_verified(w: int) -> int:
    """VS_SEED_VERIFIED(w) (csrc/vs_pe_plan.h): exact keys up to 31 bases, mixed ones above."""
    return w if w <= 31 else 0


def map_end(read: str, seqs: Sequence[str], rcs: Sequence[str], table, w: int, s: int, K: int, first=None, probes=None, grid=None, key_fn=None,
            verified=None, trace=None, hook=None) -> List[int]:
    """``verified``: the seed bases the comparison after a probe takes for granted, the device's VS_SEED_VERIFIED(w)
    (csrc/vs_pe_plan.h) -- all w (the default) where equal keys mean equal seeds, 0 where they do not: the comparison
    then starts at the seed's first base, and a posting whose seed differs from the read's ends below K bases.

    ``trace``: a list that gets one dict per posting looked at, in the device's terms (k_pe_tiles, vs_agree_fast /
    vs_agree_long) -- ``j`` the read offset, ``q`` the seed's offset in the text compared, ``node``, ``strand`` (1: the
    read runs against the node), ``left``, ``c`` the left limit min(gap, j, q), ``ext`` the equal bases from where the
    comparison starts (j + verified), ``rem`` = min(rlen - j, tlen - q) - verified, what is left of read and text from
    there (behind the seed, min(rlen - j - w, tlen - q - w), when verified = w), ``credited`` -- and then one dict per
    touched node with what the acceptance test used: ``node``, ``v``, ``coord``, ``kidx``, ``saturate``, ``T`` (the
    smallest v the second clause takes) and ``kept``.
    ``hook`` (left, ext) -> (left, ext): a test's mutation of what the comparison found.  Neither changes the result."""
    rlen = len(read)
    if verified is None:
        verified = w
    agg: Dict[int, List[int]] = {}
    if grid is not None:  # explicit probe offsets: a match is credited by the first of them inside it (left extension < gap)
        todo = [(j, (j - grid[i - 1]) if i else s) for i, j in enumerate(grid) if j + w <= rlen]
    else:
        j = phase(rlen, w, s) if first is None else first
        todo = []
        while j + w <= rlen:
            todo.append((j, s))
            j += s
    for j, gap in todo:
        if probes is not None:
            probes.append(j)
        f = read[j : j + w]
        if all(valid(c) for c in f):
            r = rc(f)
            key, sr = (f, 0) if f < r else (r, 1)
            if key_fn is not None:
                key = key_fn(key)
            for node, p, sn in table.get(key, ()):
                opp = sn ^ sr
                text = rcs[node] if opp else seqs[node]
                tlen = len(text)
                q = tlen - p - w if opp else p
                c = min(gap, j, q)
                left = 0
                while left < c and read[j - 1 - left] == text[q - 1 - left]:
                    left += 1
                ext = 0  # (bases found equal behind the ``verified`` ones that are known to be)
                while j + verified + ext < rlen and q + verified + ext < tlen and read[j + verified + ext] == text[q + verified + ext]:
                    ext += 1
                if hook is not None:
                    left, ext = hook(left, ext)
                ln = left + verified + ext
                credited = left < gap and ln >= K
                if trace is not None:
                    trace.append(dict(j=j, q=q, node=node, strand=opp, left=left, c=c, ext=ext, rem=min(rlen - j, tlen - q) - verified, credited=credited))
                if not credited:
                    continue
                a = j - left
                qa = q - left
                minp = tlen - qa - ln if opp else qa
                rec = agg.setdefault(node, [0, minp, a])
                rec[0] += ln - K + 1
                rec[1] = min(rec[1], minp)
                rec[2] = min(rec[2], a)
    keep = []
    for node in sorted(agg):
        v, c, ki = agg[node]
        nlen = len(seqs[node])
        right = min(c + nlen - 1, c - ki + rlen - 1)
        saturate = right - c - K + 2
        span = min(rlen, nlen) - K + 1
        kept = v >= saturate or v * rlen >= span * (rlen - K)
        if trace is not None:
            trace.append(dict(node=node, v=v, coord=c, kidx=ki, saturate=saturate, T=-(-span * (rlen - K) // rlen), kept=kept))
        if kept:
            keep.append(node)
    return keep

