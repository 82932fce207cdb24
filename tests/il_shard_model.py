"""The plain model of an interleaved FASTQ shared among ranks (``pe.InterleavedStream.open_shard``), stated on a list m of
match flags: m[j] says that records j and j + 1 are mates (the file's last record has none, so a file of T records has
m[0 .. T - 2]; the model reads a missing m as false).

The single process pairs greedily from the front: p(0) = 0, p(j + 1) = m[j] ? !p(j) : 0, and record j is the SECOND of a pair
iff p(j) = 1.  ``parities`` walks that by brute force.  Rank r owns the records [a_r, b_r) = ``shard_range(T, r, W)``; its
entry is p(a_r).  A function of one bit is the pair (f(0), f(1)), packed as f(0) | f(1) << 1 as the library packs it; the
function of a share is the composition, in order, of flip (m true) or const-0 (m false) over m[a_r .. b_r - 1]."""

CONST0, FLIP, ID, CONST1 = 0, 1, 2, 3


def shard_range(n, rank, world):
    return (n * rank) // world, (n * (rank + 1)) // world


def parities(m, total):
    """p(j) for j in 0 .. total (p(total): the parity a record behind the last one would have)"""
    p = [0]
    for j in range(total):
        mj = bool(m[j]) if j < len(m) else False
        p.append((1 - p[-1]) if mj else 0)
    return p


def apply(f, x):
    return (f >> x) & 1


def compose(f, g):
    """g after f"""
    return apply(g, apply(f, 0)) | (apply(g, apply(f, 1)) << 1)


def share_fn(m, a, b, order="forward", lookahead=True, all_true_is_const0=False):
    """The function of the share [a, b) from m[a .. b - 1], a missing m read as false.  The keyword arguments are the named
    mistakes: ``order="backward"`` composes from the back, ``lookahead=False`` ignores m[b - 1] (which needs the header line of
    record b, the next rank's), ``all_true_is_const0`` takes a share without a false m for a constant."""
    js = list(range(a, b))
    if not lookahead and js:
        js.pop()
    fns = [FLIP if (j < len(m) and m[j]) else CONST0 for j in js]
    if all_true_is_const0 and fns and all(f == FLIP for f in fns):
        return CONST0
    if order == "backward":
        fns.reverse()
    f = ID
    for g in fns:
        f = compose(f, g)
    return f


def tail_fn(m, a, b, reach=64, grow=16):
    """(the function of the share as the tail pass finds it, the windows it looked at): the last ``reach`` records first, a
    constant is final, identity or flip widens the window until it holds the share"""
    windows = []
    while True:
        lo = max(a, b - reach)
        f = share_fn(m, lo, b)
        windows.append((lo, b))
        if f in (CONST0, CONST1) or lo == a:
            return f, windows
        reach *= grow


def plan(fns):
    """entry of every rank from the functions of the shares: e_0 = 0, e_{r + 1} = F_r(e_r)"""
    e, out = 0, []
    for f in fns:
        out.append(e)
        e = apply(f, e)
    return out


def owned(m, total, a, b):
    """(pairs (i, i + 1), singles [i]) that the rank of [a, b) owns: every pair whose FIRST record it owns, every single it
    owns -- from the whole file's parities"""
    p = parities(m, total)
    pairs, singles = [], []
    for j in range(a, b):
        mj = j < len(m) and bool(m[j]) and j + 1 < total
        if p[j]:
            continue
        if mj:
            pairs.append((j, j + 1))
        else:
            singles.append(j)
    return pairs, singles


def m_of_headers(headers, mates):
    return [mates(headers[j], headers[j + 1]) for j in range(len(headers) - 1)]
