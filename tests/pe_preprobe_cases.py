"""Constructed blocks for the hand-over of a probe from one tile of k_pe_tiles to the next (vstrains_amd/csrc/vs_pe.hip: the
non-adaptive compile-time shapes begin a thread's probe of tile t + 1 during tile t and finish it in the P1 of tile t + 1).
What can go wrong lies between neighbouring tiles of one workgroup's run, so a block is ONE family of seven tiles of 32 pairs
-- seven KINDS -- repeated in input order: with the locus sort off, tile t of the block is of kind t mod 7, every tile
differs in kind from the one before it, and runs of three or four tiles start at every kind (7 is prime to both).

The graph (k = 55: K = 56, 31-base seeds, stride 26; built with renumber=False) has 27 nodes: random text, three nodes
that share a stretch of 150 bases (its seeds have three postings), and six nodes of 201 bases with a planted seed in the
middle -- six seeds whose home slot in the table is the same one (tests/seed_index_model.seeds_with_home_slot, as
tests/test_seed_index_gpu.py builds its chains), so that five of them sit behind another key.

KINDS  usable     exact windows of nodes, either strand: seeds with one posting and with three
       edited     the same with one to three substitutions
       n          every second pair has an N in one end (the pair is dropped)
       short      ends of K - 1 and of 40 bases (below K), of 20 and of 5 (below w): pairs dropped as short
       dirty      ends with 1, 2, 3, 4 bytes outside ACGT (limits from inv4: today's probe beside handed-over ones in one
                  tile), with one inside a seed of the grid, and with six (the overflow path)
       empty      ends of random text: none of their seeds is in the index, most home slots are empty
       displaced  windows of the planted nodes with the planted seed ON the end's probe grid, and the same with the seed
                  replaced by one that is in no node and has the same home slot (it walks the whole chain)

Lengths: every end of a usable pair has one of the two lengths of its shape -- the edges of the range the shape is chosen
for -- alternating, so that the ends of a tile differ in phase (vs_seed_phase) and in their number of probes.
Checked without a device by tests/test_pe_preprobe_cases_cpu.py, on the device by tests/test_pe_preprobe_gpu.py."""
import functools

import numpy as np

import seed_extend_model as model
import seed_index_model as sim

KSIZE = 55
K, W, S = 56, 31, 26
TILE_PAIRS = 32  # STD_EPT / 2 (vs_pe_plan.h)
KINDS = ("usable", "edited", "n", "short", "dirty", "empty", "displaced")
FAMILY_PAIRS = TILE_PAIRS * len(KINDS)
FLANK = 85  # bases on either side of a planted seed
GROUP = 6   # planted seeds on one home slot
# instantiation -> (shortest, longest) read the plan takes it for; the longest read of a block chooses
SHAPES = {"k_pe_tiles<1, 10u, 4u>": (145, 159), "k_pe_tiles<1, 8u, 3u>": (113, 128), "k_pe_tiles<1, 7u, 3u>": (108, 112),
          "k_pe_tiles<1, 7u, 2u>": (97, 107)}
RUN_TILES = 3                # T: n_pairs = n_cu * 32 * T + r
REMAINDERS = (0, 1, 31, 33)  # r
_OTHER = "nRYKMSWBDHV"       # bytes outside ACGT that do not drop the pair


def grid(rlen: int):
    """Read offsets an end of ``rlen`` bases is probed at (vs_seed_phase, vs_seed_probes)."""
    return list(range(model.phase(rlen, W, S), rlen - W + 1, S)) if rlen >= K else []


@functools.lru_cache(maxsize=None)
def graph():
    """-> dict(seqs, model (seed_index_model.build), planted [(seed, node)], home slot, misses [seeds of that home slot in no node])"""
    rng = np.random.default_rng(5531)
    plain = [sim.random_seq(rng, 320) for _ in range(12)] + [sim.random_seq(rng, 200) for _ in range(6)]
    shared = sim.random_seq(rng, 150)
    repeats = [sim.random_seq(rng, 90) + shared + sim.random_seq(rng, 90) for _ in range(3)]

    def wrap(q):
        return sim.random_seq(rng, FLANK) + q + sim.random_seq(rng, FLANK)

    bits = sim.build(plain + repeats + [wrap(sim.random_seq(rng, W)) for _ in range(GROUP)], KSIZE)["bits"]
    for _ in range(8):
        home = (1 << bits) // 2 + 12345
        seeds = sim.seeds_with_home_slot(W, bits, home, GROUP, rng)
        seqs = plain + repeats + [wrap(q) for q in seeds]
        m = sim.build(seqs, KSIZE)
        if m["bits"] == bits:
            misses = sim.seeds_with_home_slot(W, bits, home, 3, rng, avoid=set(m["postings"]))
            first = len(plain) + len(repeats)
            return dict(seqs=seqs, model=m, planted=[(q, first + i) for i, q in enumerate(seeds)], home=home, misses=misses,
                        plain=list(range(len(plain))), repeats=list(range(len(plain), first)), shared=(90, 240))
        bits = m["bits"]
    raise AssertionError("the table size did not settle")


def _strand(rng, read):
    return sim.rc(read) if rng.integers(0, 2) else read


def _window(rng, g, node, rlen, cover=None):
    """A window of ``rlen`` bases of a node; ``cover`` = (lo, hi): one that holds at least K bases of that stretch."""
    text = g["seqs"][node]
    lo, hi = 0, len(text) - rlen
    if cover is not None:
        lo, hi = max(lo, cover[0] + K - rlen), min(hi, cover[1] - K)
    assert lo <= hi, (node, rlen)
    st = int(rng.integers(lo, hi + 1))
    return text[st: st + rlen]


def _usable_end(rng, g, rlen, i):
    if i % 3 == 0:  # the stretch three nodes share
        return _strand(rng, _window(rng, g, g["repeats"][i // 3 % 3], rlen, cover=g["shared"]))
    nodes = [n for n in g["plain"] if len(g["seqs"][n]) >= rlen]
    return _strand(rng, _window(rng, g, nodes[i % len(nodes)], rlen))


def _put(read, pos, chars):
    for p, ch in zip(pos, chars):
        read = read[:p] + ch + read[p + 1:]
    return read


def _planted_window(g, which, rlen, pi, seed=None):
    """The window of planted node ``which`` that has the planted seed at the end's pi-th probe offset (``seed``: put there instead)."""
    q, node = g["planted"][which]
    text = g["seqs"][node]
    o = grid(rlen)[pi]
    st = FLANK - o
    assert 0 <= st <= len(text) - rlen, (rlen, pi)
    win = text[st: st + rlen]
    assert win[o: o + W] == q
    return win if seed is None else win[:o] + seed + win[o + W:]


def on_grid_probes(rlen):
    """The probe indices pi of an end of ``rlen`` bases that a window of a planted node can put its seed on."""
    return [pi for pi, o in enumerate(grid(rlen)) if 0 <= FLANK - o <= 2 * FLANK + W - rlen]


@functools.lru_cache(maxsize=None)
def family(kernel: str):
    """The seven tiles of a shape -> dict(fwd, rve, kind [per pair])."""
    g = graph()
    lo_len, hi_len = SHAPES[kernel]
    rng = np.random.default_rng(5500 + hi_len)
    fwd, rve, kind = [], [], []

    def lens(i):
        return (hi_len, lo_len) if i % 2 == 0 else (lo_len, hi_len)

    for kd in KINDS:
        for i in range(TILE_PAIRS):
            lf, lr = lens(i)
            f, r = _usable_end(rng, g, lf, i), _usable_end(rng, g, lr, i + 1)
            if kd == "edited":
                f = _put(f, sorted(rng.choice(lf, size=1 + i % 3, replace=False)), "ACGT" * 1)  # (some leave the base as it is)
                r = sim.sub_at(r, int(rng.integers(0, lr)))
            elif kd == "n" and i % 2:
                if i % 4 == 1:
                    f = _put(f, [int(rng.integers(0, lf))], "N")
                else:
                    r = _put(r, [int(rng.integers(0, lr))], "N")
            elif kd == "short" and i % 4 != 3:
                if i % 4 == 0:
                    f = f[:40]
                elif i % 4 == 1:
                    r = r[:20]
                else:
                    f, r = f[:K - 1], r[:5]
            elif kd == "dirty" and i % 4 != 3:
                if i % 4 == 0:  # 1 .. 4 bytes anywhere
                    n = 1 + (i // 4) % 4
                    f = _put(f, sorted(rng.choice(lf, size=n, replace=False)), [_OTHER[(i + t) % len(_OTHER)] for t in range(n)])
                elif i % 4 == 1:  # six: more than inv4 holds
                    r = _put(r, sorted(rng.choice(lr, size=6, replace=False)), [_OTHER[(i + t) % len(_OTHER)] for t in range(6)])
                else:  # one inside a seed of the grid
                    o = grid(lr)[(i // 4) % len(grid(lr))]
                    r = _put(r, [o + int(rng.integers(0, W))], _OTHER[i % len(_OTHER)])
            elif kd == "empty":
                f = sim.random_seq(rng, lf)
                if i % 2 == 0:
                    r = sim.random_seq(rng, lr)
            elif kd == "displaced":
                pf, pr = on_grid_probes(lf), on_grid_probes(lr)
                f = _planted_window(g, i % GROUP, lf, pf[i % len(pf)])
                miss = g["misses"][i % len(g["misses"])] if i % 3 == 2 else None
                r = _planted_window(g, (i + 1 + i // GROUP) % GROUP, lr, pr[(i // 2) % len(pr)], seed=miss)
                if i % 2:
                    f = sim.rc(f)
                if i % 4 < 2:
                    r = sim.rc(r)
            fwd.append(f)
            rve.append(r)
            kind.append(kd)
    assert len(fwd) == FAMILY_PAIRS and max(len(x) for x in fwd + rve) == hi_len
    return dict(fwd=fwd, rve=rve, kind=kind)


def block(kernel: str, n_pairs: int):
    """The family repeated in input order up to ``n_pairs`` pairs -> (fwd, rve, index of every pair in the family)."""
    fam = family(kernel)
    idx = [p % FAMILY_PAIRS for p in range(n_pairs)]
    return [fam["fwd"][i] for i in idx], [fam["rve"][i] for i in idx], idx


def block_pairs(n_cu: int, r: int) -> int:
    return n_cu * TILE_PAIRS * RUN_TILES + r


def runs_of_tiles(n_pairs: int, n_cu: int, grid_per_cu: int = 1):
    """vs_pe_plan (vs_pe_plan.h): tiles, tiles per workgroup, workgroups, tiles of the last workgroup's run."""
    n_tiles = -(-n_pairs // TILE_PAIRS)
    max_grid = n_cu * grid_per_cu
    wgs = min(n_tiles, max_grid)
    per_wg = -(-n_tiles // wgs)
    wgs = -(-n_tiles // per_wg)
    return n_tiles, per_wg, wgs, n_tiles - per_wg * (wgs - 1)


def pair_used(f: str, r: str) -> bool:
    """PE_Inference.py:160-165: a pair with an N, or with an end below K bases, is not mapped."""
    return "N" not in f and "N" not in r and len(f) >= K and len(r) >= K


def dirty_bytes(read: str) -> int:
    return sum(ch not in "ACGTN" for ch in read)


def end_features(read: str, used: bool):
    """What the probes of one end meet, from the host statement of the index (seed_index_model): a set of
    'single' / 'multi' (postings of a seed that is in the index), 'empty' (not in the index, home slot empty), 'walk' (not
    in the index, home slot taken: the chain is walked to an empty slot), and the home slots of the seeds that are in the
    index as ('home', slot).  Only clean ends of used pairs are handed over; dirty ones are reported as 'dirty<n>'."""
    g = graph()
    m = g["model"]
    out = set()
    if "N" in read:
        out.add("n")
    if len(read) < W:
        out.add("below_w")
    elif len(read) < K:
        out.add("below_K")
    d = dirty_bytes(read)
    if d:
        out.add("dirty%d" % min(d, 5))
    if not used or d or "N" in read:
        return out
    for o in grid(len(read)):
        key, _ = sim.seed_key(read[o: o + W])
        home = sim.slot_of(key, m["bits"])
        if key in m["postings"]:
            out.add("multi" if len(m["postings"][key]) > 1 else "single")
            out.add(("home", home, key))
        else:
            out.add("walk" if home in m["occupied"] else "empty")
    return out
