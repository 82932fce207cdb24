"""The blocks of unpaired reads the counting kernels are tested on (tests/test_unpaired_gpu.py), on two graphs:

* ``golden``: the graph and the reads of tests/golden/pe/hiv_like_k55 (k = 55), every read taken as a single;
* ``chain``: a constructed chain of three nodes at k = 21 whose middle node is short, with reads placed so that they span
  exactly 1, 2 and 3 nodes.

A block of n reads opens with the special reads (``specials``), each next to ordinary ones, and is filled up from the
graph's pool; tests/test_unpaired_model_cpu.py checks without a device that the blocks hold what they were built for."""
import functools
import os

import numpy as np

import unpaired_model
from oracle import pe_oracle

GOLDEN_CASE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pe", "hiv_like_k55")

# slots per block: one; either side of a tile (a tile holds ept / 2 = 32 slots); either side of the locus sort's threshold
# (4096 slots); an odd count in between
SIZES = (1, 31, 32, 33, 77, 4095, 4096, 4097)

CHAIN_K = 21
CHAIN_READ = 100


class Graph:
    def __init__(self, name, seqs, ksize, pool, spans=None):
        self.name, self.seqs, self.k, self.pool, self.spans = name, list(seqs), ksize, list(pool), spans
        self.model = unpaired_model.Model(self.seqs, ksize)


@functools.lru_cache(maxsize=None)
def golden() -> Graph:
    _, seqs = pe_oracle.read_gfa_segments(os.path.join(GOLDEN_CASE, "graph.gfa"))
    pool = pe_oracle.fastq_sequences(os.path.join(GOLDEN_CASE, "fwd.fq")) + pe_oracle.fastq_sequences(os.path.join(GOLDEN_CASE, "rve.fq"))
    return Graph("golden", seqs, 55, pool)


@functools.lru_cache(maxsize=None)
def chain() -> Graph:
    """genome[0:300], genome[279:320], genome[299:340], genome[319:600]: consecutive nodes share k bases, as the nodes of a
    compacted de Bruijn graph do, so that every (k+1)-window of the genome lies in exactly one node.  The two middle nodes
    are short (20 windows each): a 100-base read holds them whole, and its tail reaches the node behind them."""
    rng = np.random.default_rng(2101)
    genome = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 600))
    k = CHAIN_K
    seqs = [genome[0:300], genome[300 - k:320], genome[320 - k:340], genome[340 - k:600]]
    L = CHAIN_READ
    pool = []
    for start in range(0, 600 - L, 7):
        s = genome[start:start + L]
        pool.append(s if (start // 7) % 2 == 0 else pe_oracle.revcomp(s))
    g = Graph("chain", seqs, k, pool)
    # reads that span exactly 1, 2 and 3 nodes, as the model maps them: by their start in the genome
    g.spans = {1: [genome[10:10 + L], genome[450:450 + L]], 2: [genome[299:299 + L], genome[302:302 + L]], 3: [genome[250:250 + L], genome[279:279 + L]]}
    for n in (1, 2, 3):
        g.pool += g.spans[n]
    return g


GRAPHS = {"golden": golden, "chain": chain}


def _edit(s, changes):
    b = list(s)
    for pos, ch in changes:
        b[pos] = ch
    return "".join(b)


def specials(g: Graph):
    """name -> read; the ordinary reads they are cut from come from the pool"""
    K = g.k + 1
    # (the first read of the pool whose first k+1 and k+2 bases lie in the graph as they are: no sampled error in them)
    base = next(s for s in g.pool if len(s) > K and g.model.nodes(s[:K]) and g.model.nodes(s[:K + 1]))
    rng = np.random.default_rng(77 + g.k)
    nowhere = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, len(base)))

    def edited(changes):  # the first read of the pool that maps, and still does with these bytes changed
        return next(_edit(s, changes) for s in g.pool if len(s) > K + 12 and g.model.nodes(s) and g.model.nodes(_edit(s, changes)))

    return {
        "with_N": _edit(g.pool[5], [(len(g.pool[5]) // 2, "N")]),
        "len_k": base[:K - 1],
        "len_k+1": base[:K],
        "len_k+2": base[:K + 1],
        "len_0": "",
        "one_invalid": edited([(3, "x")]),
        "five_invalid": edited([(0, "*"), (2, "n"), (4, "R"), (6, "."), (8, "-")]),  # VS_FLAG_MANY: the overflow path
        "maps_nowhere": nowhere,
    }


@functools.lru_cache(maxsize=None)
def block(graph: str, n: int):
    """The n reads of a block: an ordinary read, then every special read followed by an ordinary one, then the pool"""
    g = GRAPHS[graph]()
    reads = [g.pool[0]]
    for i, s in enumerate(specials(g).values()):
        reads += [s, g.pool[(11 + i) % len(g.pool)]]
    i = 0
    while len(reads) < n:
        reads.append(g.pool[i % len(g.pool)])
        i += 1
    return tuple(reads[:n])


@functools.lru_cache(maxsize=None)
def all_dropped(graph: str):
    """A block in which rules 1 and 2 drop every read"""
    g = GRAPHS[graph]()
    sp = specials(g)
    return tuple([sp["with_N"], sp["len_k"], sp["len_0"], "N", sp["len_k"][:5]] * 9)


@functools.lru_cache(maxsize=None)
def shape_block(n: int = 300):
    """150-base reads without a byte outside ACGT at k = 55: what a compile-time shape of k_pe_tiles is picked for"""
    g = golden()
    reads = [s for s in g.pool if len(s) == 150 and set(s) <= set("ACGT")]
    assert len(reads) >= 100
    return tuple(reads[i % len(reads)] for i in range(n))


@functools.lru_cache(maxsize=None)
def expected(graph: str, reads: tuple):
    """(node_mat = zeros, short_mat, tallies) of the model, computed once per block"""
    return GRAPHS[graph]().model.count(reads)
