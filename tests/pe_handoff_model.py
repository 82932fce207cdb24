"""Plain model of the hand-off the mapping kernel leaves for the counter kernels (k_pe_tiles P4 / P5 in
vstrains_amd/csrc/vs_pe.hip): per tile the (end, node) table, per end the list length, its quads and its offset in the
tile's region, per pair whether it goes to the overflow list, and the count word P5 writes.

What it is given per end is what tests/seed_extend_model.py's trace says about it (held to the oracle there and in
tests/test_pe_handoff_cpu.py): the credited nodes and which of them are accepted.  Everything else restates the kernel.

THE RULE, AS THE KERNEL HAS IT (a rule of the kernel, not of the reference: the reference knows no tiles, no list cap and no
overflow; whichever path a pair takes, the counters are the reference's):
  * An end of a pair the filters drop (an N, an end shorter than k + 1: PE_Inference.py:160-165) has n = 0, q = 0, count word 0.
  * An end of a used pair has n = its accepted nodes.  n > LCAP makes it an overflow end with q = 0; otherwise q = ceil(n / 4).
  * o = the sum of q over the ends in front of it in the tile (two ends per lane of one wavefront, an exclusive prefix sum).
  * o + q > capq, capq = (ept * LC - trim) / 4, makes it an overflow end as well.  The prefix sum INCLUDES the quads of an end
    that did not fit, so every later end of the tile has o + q > capq too -- an empty one included (o alone is above capq) --
    and is an overflow end.
  * A used pair with an overflow end goes to the overflow list; both its count words are 0 -- but an end of it
    that fits keeps its quads in the prefix sum, and its nodes their place in the region.  A pair the filters drop never goes
    there.
  * Count word of every other end: packed layout n | o << 8 (0 for n = 0), row layout n.
  * The tile's packed lists take 4 * min(sum q, capq) words.
The table: key = end slot in the tile << 25 | node, home slot (key * 0x9E3779B1 mod 2^32) >> (32 - log2 pool), or the high
word of that product times 768 for the 768-slot table; linear probing.  Which slots end up occupied does not depend on the
order of the insertions while none fails; an insertion fails after 64 probes, which no order can reach while the occupied
set has no cyclic run of 64 slots: such a tile is TABLE-SAFE and everything above is exact for it.  On any other tile an end
may lose a node and is then an overflow end of the kernel's own making; only the order-free statements hold."""
LC, LCAP, PROBES = 16, 20, 64
GOLDEN = 0x9E3779B1


def capq(ept, trim):
    return (ept * LC - trim) >> 2


def home(key, pool):
    h = (key * GOLDEN) & 0xFFFFFFFF
    if pool & (pool - 1):
        return (h * pool) >> 32  # __umulhi(h, pool)
    return h >> (32 - (pool.bit_length() - 1))


def insert(occ, key, pool):
    """One more key into the occupied set ``occ`` (a list of booleans): the slot it takes, whatever came before."""
    at = home(key, pool)
    for _ in range(pool):
        if not occ[at]:
            occ[at] = True
            return at
        at = at + 1 if at + 1 < pool else 0
    return None  # (more keys than slots)


def longest_run(occ):
    """The longest cyclic run of occupied slots (the whole table if every slot is)."""
    pool = len(occ)
    if all(occ):
        return pool
    start = occ.index(False)
    best = run = 0
    for i in range(1, pool + 1):
        if occ[(start + i) % pool]:
            run += 1
            best = max(best, run)
        else:
            run = 0
    return best


def tile(ends, ept, pool, trim, rows):
    """``ends``: the ends of one tile in tile order (an even number, at most ``ept``), each a dict ``used`` (its pair passes the
    filters) and ``nodes`` = [(node, accepted)] for every credited node.  -> dict: ``entries`` (table keys), ``occupied``
    (slots, None if the keys outnumber them), ``run``, ``safe``; per end lists ``n``, ``q``, ``o``, ``over_lcap``,
    ``over_region``, ``word``, ``accepted`` (node lists); per pair ``listed``; ``sum_q``, ``used_words``, ``first_unfit`` (the
    first end with o + q > capq, or None)."""
    assert len(ends) % 2 == 0 and len(ends) <= ept
    cq = capq(ept, trim)
    keys = [(e << 25) | node for e, end in enumerate(ends) if end["used"] for node, _ in end["nodes"]]
    assert len(set(keys)) == len(keys)
    occ = [False] * pool
    fits = len(keys) <= pool
    if fits:
        for key in keys:
            insert(occ, key, pool)
    run = longest_run(occ) if fits else pool
    out = dict(entries=len(keys), occupied=[i for i, x in enumerate(occ) if x] if fits else None, run=run, safe=run < PROBES,
               n=[], q=[], o=[], over_lcap=[], over_region=[], word=[], accepted=[], listed=[], first_unfit=None)
    o = 0
    for e, end in enumerate(ends):
        acc = [node for node, ok in end["nodes"] if ok] if end["used"] else []
        n = len(acc)
        over_lcap = n > LCAP
        q = 0 if over_lcap else (n + 3) // 4
        over_region = o + q > cq
        if over_region and out["first_unfit"] is None:
            out["first_unfit"] = e
        out["accepted"].append(acc)
        out["n"].append(n)
        out["q"].append(q)
        out["o"].append(o)
        out["over_lcap"].append(over_lcap)
        out["over_region"].append(over_region)
        o += q
    out["sum_q"] = o
    out["used_words"] = 4 * min(o, cq)
    for p in range(len(ends) // 2):
        used = ends[2 * p]["used"]
        assert used == ends[2 * p + 1]["used"]
        over = any(out["over_lcap"][e] or out["over_region"][e] for e in (2 * p, 2 * p + 1))
        out["listed"].append(used and over)
        for e in (2 * p, 2 * p + 1):
            n = out["n"][e]
            if not used or over:
                out["word"].append(0)
            elif rows:
                out["word"].append(n)
            else:
                out["word"].append(n | out["o"][e] << 8 if n else 0)
    return out


def block(ends, ept, pool, trim, rows, perm=None):
    """The tiles of a block: ``ends`` by input end index (2 p, 2 p + 1 = pair p), taken ``ept`` / 2 pairs at a time in input
    order or in the order ``perm`` names.  -> (tile models, for every tile the pairs it holds)."""
    n_pairs = len(ends) // 2
    order = list(range(n_pairs)) if perm is None else [int(p) for p in perm]
    assert sorted(order) == list(range(n_pairs))
    ppt = ept // 2
    tiles, pairs = [], []
    for lo in range(0, n_pairs, ppt):
        mine = order[lo:lo + ppt]
        tiles.append(tile([ends[2 * p + side] for p in mine for side in (0, 1)], ept, pool, trim, rows))
        pairs.append(mine)
    return tiles, pairs


def unpack(lists, counts, n_ends, ept, list_ends, rows):
    """vs_pe_unpack_lists (csrc/vs_pe_pack.h) restated: the first ``n_ends`` end slots of a hand-off as Python lists."""
    out = []
    for e in range(n_ends):
        c = int(counts[e])
        n = c if rows else c & 0xFF
        if rows:
            row = [int(lists[e * LC + i]) if i < LC else int(lists[list_ends * LC + e * 4 + (i - LC)]) for i in range(n)]
        else:
            base = (e // ept) * ept * LC + 4 * (c >> 8)
            row = [int(x) for x in lists[base:base + n]]
        out.append(row)
    return out
