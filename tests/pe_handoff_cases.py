"""Constructed blocks that drive the mapping kernel (k_pe_tiles, vstrains_amd/csrc/vs_pe.hip) to each state of its hand-off
(P4 / P5) on purpose, for tests/test_pe_handoff_cpu.py (which shows by the model, tests/pe_handoff_model.py, that every
state is reached) and tests/test_pe_handoff_gpu.py (which reads what the kernel left).

The graph of a shape: one random TEXT of ``rlen`` bases per end slot of a tile, and as nodes its OFFSETS substrings of
exactly K = k + 1 bases at offsets 0 .. OFFSETS - 1, plus unrelated padding nodes of K bases (enough of them that the index
statistics keep the plan off the adaptive grid by themselves).  The read of slot e with m nodes is the text up to base
K - 1 + m and every base behind it replaced by another one: it holds the nodes at offsets 0 .. m - 1 whole (v = 1 = span:
accepted) and no K-mer of any other node.  A tile is then a list of m per slot ("N": a read with an N, "S": a read of k
bases -- either drops its pair), a block a list of tiles, and the table key (slot << 25 | node) of a node of text e is the
same in every tile: ONE greedy search per shape (fixed random seed) numbers the nodes so that every tile that is to be
table-safe is."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import pe_handoff_model as hm
import seed_extend_model as sem
from test_pe_plan_cpu import DEFAULTS, IN, OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = 21
LENGTHS = [0, 1, 3, 4, 5, 16, 17, 19, 20, 21]  # case (a): either end of a pair, partners of every other length
N_CU = 256

# k, read length, the switches an experiment context needs to reach the instantiation (None: a production context picks it),
# the instantiation, its table slots and list trim as the project states them (vs_std_table), padding nodes.
# (Reads of 60 bases at k = 20 take the straight-line kernel with a run-time pool by themselves, "k20fast"; the generic one,
# which only long reads, long strides or nodes of 2^23 bases reach in production, needs VS_NO_FAST at this size.)
SHAPES = {
    "k20": dict(k=20, rlen=60, env={"VS_NO_FAST": "1"}, tune=dict(no_fast=1), kernel="k_pe_tiles<0, 0u, 0u>", ept=32, pool=512, trim=0, pad=1300),
    "k20fast": dict(k=20, rlen=60, env=None, tune={}, kernel="k_pe_tiles<1, 0u, 0u>", ept=32, pool=512, trim=0, pad=1300),
    "k55": dict(k=55, rlen=150, env=None, tune={}, kernel="k_pe_tiles<1, 10u, 4u>", ept=64, pool=768, trim=64, pad=1300),
    "k55ad": dict(k=55, rlen=150, env={"VS_ADAPT_GRID": "1"}, tune=dict(adapt_grid=1), kernel="k_pe_tiles<1, 10u, 4u, true>", ept=64, pool=1024,
                  trim=0, pad=1300),
    "k127": dict(k=127, rlen=250, env=None, tune={}, kernel="k_pe_tiles<2, 16u, 2u>", ept=60, pool=768, trim=192, pad=1300),
}
_ROT = {"A": "C", "C": "G", "G": "T", "T": "A"}


# ---- the plan on the CPU (oracle/plan_check.cpp) ---------------------------------------------------------------------------
_plan_lib = None


def _lib():
    global _plan_lib
    if _plan_lib is None:
        path = os.path.join(ROOT, "oracle", "_build", "libvs_plan_check.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
        lib = C.CDLL(path)
        lib.vs_pe_plan_check.restype = C.c_int
        lib.vs_pe_plan_check.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.vs_std_table_check.restype = None
        lib.vs_std_table_check.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]
        _plan_lib = lib
    return _plan_lib


def plan(graph, n_ends, **tune):
    """The launch plan of a count of ``n_ends`` ends of the shape's read length on ``graph`` (vs_pe_plan), with the name of
    the instantiation as vs_pe_last_kernel gives it and the slots and trim of its table (vs_std_table)."""
    sh = graph.shape
    K = sh["k"] + 1
    w, s = sem.geometry(K)
    d = dict(DEFAULTS, n_nodes=len(graph.seqs), K=K, w=w, s=s, n_seed_pos=graph.n_seed_pos, n_distinct=graph.n_distinct, max_node_len=K, n_cu=N_CU,
             n_ends=n_ends, max_len=sh["rlen"], has_mask=0, has_inv4=0, count=1, tile_map=0)
    d.update(sh["tune"])
    d.update(tune)
    a = np.array([[d[f] for f in IN]], dtype=np.int64)
    out = np.zeros((1, len(OUT)), dtype=np.uint64)
    msgs = C.create_string_buffer(128)
    assert _lib().vs_pe_plan_check(1, a.ctypes.data, out.ctypes.data, msgs) == len(OUT)
    p = dict(zip(OUT, out[0].astype(np.int64).tolist()))
    assert p["status"] == 0, msgs.value
    p["kernel"] = "k_pe_tiles<%d, %du, %du%s>" % (p["mode"], p["sw"], p["sp"], ", true" if p["ad"] else "")
    tab = np.zeros(2, dtype=np.uint32)
    _lib().vs_std_table_check(p["mode"], p["sw"], p["ad"], p["pool"], tab.ctypes.data)
    p["table_pool"], p["table_trim"] = int(tab[0]), int(tab[1])
    return p


# ---- tiles -----------------------------------------------------------------------------------------------------------------
def _m(spec):
    return spec if isinstance(spec, int) else 0


def _spread(total_q, n_ends):
    """``total_q`` quads over ``n_ends`` ends as evenly as it goes, the longer ones first; list lengths with the fewest nodes
    that take the quads (4 q - 3), except the first three ends, which end on a full, a three-quarter and a half quad."""
    base, extra = divmod(total_q, n_ends)
    assert 1 <= base and base + (1 if extra else 0) <= 5, (total_q, n_ends)
    qs = [base + (1 if i < extra else 0) for i in range(n_ends)]
    return [4 * q - (0, 1, 2)[i] if i < 3 else 4 * q - 3 for i, q in enumerate(qs)]


def tiles_a(ept):
    """Case (a): every ordered pair of LENGTHS, half a tile of them at a time (the other half empty pairs: in front of, behind
    or between them), and one more tile in which a 21 stands without a 20."""
    pairs = [(x, y) for x in LENGTHS for y in LENGTHS]
    ppt = ept // 2
    real = ppt // 2
    out = []
    for t, lo in enumerate(range(0, len(pairs), real)):
        mine = pairs[lo:lo + real]
        mine += [(0, 0)] * (real - len(mine))
        empty = [(0, 0)] * (ppt - real)
        if t % 3 == 0:
            tile = mine + empty
        elif t % 3 == 1:
            tile = empty + mine
        else:
            tile = [p for pair in zip(mine, empty) for p in pair] + mine[len(empty):] + empty[len(mine):]
        out.append([m for p in tile[:ppt] for m in p])
    alone = [(21, 3), (4, 5), (1, 0), (16, 17), (19, 1)] + [(0, 0)] * (ppt - 5)
    out.append([m for p in alone for m in p])
    return out


def tile_b(ept, cq):
    """Case (b): every end of the tile listed, the quads sum to ``cq``."""
    return _spread(cq, ept)


def tile_c_last(ept, cq):
    """Case (c): tile (b) with its last end one quad longer: the first end that does not fit is the last end of the tile."""
    t = tile_b(ept, cq)
    t[-1] += 4
    return t


def tile_c_mid(ept, cq):
    """Case (c): ends of five quads up to one quad past the region in the middle of the tile; behind the end that does not
    fit a short one, an empty one, a one-node one, ..., and a dropped pair last."""
    x = cq // 5
    rem = cq + 1 - 5 * x
    assert 1 <= rem <= 5 and x + 5 <= ept
    t = [17] * x + [4 * rem - 3]
    while len(t) < ept - 2:
        t.append((4, 0, 1)[(len(t) - x - 1) % 3])
    return t + ["N", 5]


def tile_c_follow(ept, cq):
    """Case (c): one quad past the region at end ept - 5, followed by an empty pair and by a dropped pair."""
    return _spread(cq + 1, ept - 4) + [0, 0, "N", 3]


def tile_dropped(ept):
    """Case (d): every pair dropped -- an N on either side, an end of k bases on either side, both."""
    kinds = [("N", 5), (3, "S"), ("S", "N"), (20, "N"), ("S", 0), ("N", "N")]
    return [m for p in range(ept // 2) for m in kinds[p % len(kinds)]]


def tile_e(ept, pool):
    """Case (e): more credited (end, node) entries than the table has slots."""
    assert ept * 20 > pool
    return [20] * ept


def tile_light(ept):
    return [m for p in range(ept // 2) for m in ((2, 7), (0, 0), (12, 1))[p % 3]]


# ---- the graph of a shape --------------------------------------------------------------------------------------------------
class Graph:
    pass


_graphs = {}


def _search(configs, ept, pool, n_ids, rng):
    """Node numbers for (slot, offset) such that every tile of ``configs`` (m per slot) is table-safe: greedy, the nodes most
    tiles hold first, each taking -- of a sample of the numbers still free -- the one that leaves the shortest run of occupied
    slots around where it lands, over the tiles that hold it.  Raises if a node finds no number that keeps every run below 64."""
    occ = [[False] * pool for _ in configs]
    free = list(range(n_ids))
    rng.shuffle(free)
    ids = {}

    def landing(o, key):
        at = hm.home(key, pool)
        while o[at]:
            at = at + 1 if at + 1 < pool else 0
        run, i = 1, at
        while run < hm.PROBES:
            i = i + 1 if i + 1 < pool else 0
            if not o[i]:
                break
            run += 1
        i = at
        while run < hm.PROBES:
            i = i - 1 if i else pool - 1
            if not o[i]:
                break
            run += 1
        return at, run

    for j in range(OFFSETS):
        for e in range(ept):
            holders = [c for c, cfg in enumerate(configs) if e < len(cfg) and _m(cfg[e]) > j]
            best = None
            for tries, cand in enumerate(reversed(free)):
                key = (e << 25) | cand
                worst = max([landing(occ[c], key)[1] for c in holders], default=0)
                if best is None or worst < best[0]:
                    best = (worst, cand)
                if worst <= 4 or (tries >= 64 and best[0] < hm.PROBES // 2) or tries >= 2048:
                    break
            if best is None or best[0] >= hm.PROBES:
                raise AssertionError("no node number keeps the tiles table-safe at slot %d, offset %d" % (e, j))
            cand = best[1]
            free.remove(cand)
            ids[(e, j)] = cand
            for c in holders:
                occ[c][landing(occ[c], (e << 25) | cand)[0]] = True
    return ids, free


def graph(name):
    """The graph and the blocks of shape ``name``, made once per process."""
    if name in _graphs:
        return _graphs[name]
    sh = SHAPES[name]
    g = Graph()
    g.name, g.shape = name, sh
    K = sh["k"] + 1
    ept, pool, trim = sh["ept"], sh["pool"], sh["trim"]
    g.K, g.ept, g.pool, g.trim, g.capq = K, ept, pool, trim, hm.capq(ept, trim)
    rng = random.Random(1000 + K)
    assert sh["rlen"] - K + 1 >= OFFSETS and K - 1 >= OFFSETS - 1  # (a replaced base lies behind every node's first base)
    g.texts = ["".join(rng.choice("ACGT") for _ in range(sh["rlen"])) for _ in range(ept)]
    # the region cannot be filled inside 768 slots with 64 ends (test_pe_handoff_cpu.py): the fullest tile the search takes
    g.reachable = 4 * g.capq - 3 * ept <= pool - pool // hm.PROBES - 1
    blocks = {}
    blocks["a"] = tiles_a(ept)
    if g.reachable:
        b = tile_b(ept, g.capq)
        # (behind each a tile that writes no list word: what a tile writes past its region shows in words nothing else touches)
        blocks["c"] = [tile_c_last(ept, g.capq), tile_dropped(ept), tile_c_mid(ept, g.capq), tile_dropped(ept), tile_c_follow(ept, g.capq),
                       tile_dropped(ept), tile_light(ept)]
    safe_extra = []
    n_ids = ept * OFFSETS + sh["pad"]
    if not g.reachable:
        # ends of 13 nodes (four quads) in front of ends of 9 (three): as many of the longer ones as the search places
        for x in range(ept, -1, -2):
            b = [13] * x + [9] * (ept - x)
            if sum(b) > pool - pool // hm.PROBES - 1:
                continue
            try:
                _search([b], ept, pool, n_ids, random.Random(7))
            except AssertionError:
                continue
            break
    blocks["b"] = [b, tile_light(ept)]
    blocks["d"] = [b, tile_dropped(ept), b, [5, 18]]
    blocks["e"] = [tile_e(ept, pool), tile_light(ept)]
    g.blocks = blocks
    g.safe = {"a": blocks["a"], "b": blocks["b"], "d": blocks["d"], "c": blocks.get("c", []), "e": blocks["e"][1:]}
    configs = []
    for case in "abcd":
        for t in g.safe[case]:
            if t not in configs:
                configs.append(t)
    configs.append(tile_light(ept))
    ids, free = _search(configs, ept, pool, n_ids, random.Random(2000 + K))
    seqs = [None] * n_ids
    g.node = {}
    for (e, j), i in ids.items():
        seqs[i] = g.texts[e][j:j + K]
        g.node[(e, j)] = i
    for i in free:
        seqs[i] = "".join(rng.choice("ACGT") for _ in range(K))
    assert len(set(seqs)) == n_ids
    g.seqs = seqs
    w, s = sem.geometry(K)
    g.w, g.s = w, s
    g.n_seed_pos = n_ids * (K - w + 1)
    seeds = set()
    for t in seqs:
        for p in range(K - w + 1):
            f = t[p:p + w]
            seeds.add(min(f, sem.rc(f)))
    g.n_distinct = len(seeds)
    _graphs[name] = g
    return g


def read(g, e, spec):
    """The read of slot ``e`` for a tile entry."""
    t, K = g.texts[e], g.K
    if spec == "S":
        return t[:K - 1]
    m = _m(spec)
    cut = K - 1 + m
    r = t[:cut] + "".join(_ROT[c] for c in t[cut:])
    if spec == "N":
        return r[:K // 2] + "N" + r[K // 2 + 1:]
    return r


def reads(g, tiles):
    """(fwd, rve) of a block given as tiles."""
    fwd, rve = [], []
    for t in tiles:
        for e, spec in enumerate(t):
            (rve if e & 1 else fwd).append(read(g, e, spec))
    return fwd, rve


_traces = {}


def mapped(g, text):
    """What the string model of the device algorithm says about a read: [(node, accepted)] over the credited nodes."""
    key = (g.name, text)
    if key not in _traces:
        if not hasattr(g, "table"):
            g.table = sem.build(g.seqs, g.K)[0]
            g.rcs = [sem.rc(s) for s in g.seqs]
        tr = []
        kept = sem.map_end(text, g.seqs, g.rcs, g.table, g.w, g.s, g.K, verified=sem.seed_verified(g.w), trace=tr)
        nodes = [(d["node"], d["kept"]) for d in tr if "kept" in d]
        assert [n for n, ok in nodes if ok] == kept
        _traces[key] = nodes
    return _traces[key]


def model_ends(g, fwd, rve, singles=False):
    """The model's input for a block of reads: per end ``used`` and ``nodes``.  ``singles``: a singles block -- ``rve`` holds
    empty texts for the absent second ends, and a slot passes the filters on its first end alone."""
    ends = []
    for f, r in zip(fwd, rve):
        used = "N" not in f and "N" not in r and len(f) >= g.K and (len(r) >= g.K or (singles and not r))
        for text in (f, r):
            ends.append(dict(used=used, nodes=mapped(g, text) if used and text else []))
    return ends
