"""Constructed blocks for the depth pass (``vs_node_depth``): small graphs and read ends in which one thing at a time can go
wrong.  Expected counts come from tests/node_depth_model.py; where the construction itself fixes a count it is written into
the case (``want``) and tests/test_node_depth_model_cpu.py holds the model to it.  tests/test_node_depth_gpu.py runs the same
cases on the device at k = 21 (stride 2), 55 and 127 (63-base seeds whose key only nominates)."""
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from oracle.pe_oracle import revcomp

KS = (21, 55, 127)
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


class DepthCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    ends: List[str]            # the block's ends in order (a singles block: its reads)
    singles: bool = False      # packed as a singles block: every second end absent (a block of pairs holds an even number of ends)
    want: Optional[Dict[int, int]] = None  # counts the construction fixes (every other node: 0)
    tells: tuple = ()          # the named mistakes (node_depth_model variants) this case must expose


def dna(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _flank(rng, n: int, avoid: str, at_end: bool) -> str:
    """n random bases whose base next to the match is not ``avoid``: the match cannot grow into the flank."""
    f = dna(rng, n)
    if not n:
        return f
    if at_end and f[-1] == avoid:
        f = f[:-1] + _OTHER[avoid]
    if not at_end and f[0] == avoid:
        f = _OTHER[avoid] + f[1:]
    return f


def _cut(rng, node: str, a: int, n: int, left: int = 9, right: int = 7) -> str:
    """node[a : a + n] between flanks that match nothing next to it."""
    before = node[a - 1] if a > 0 else "A"
    after = node[a + n] if a + n < len(node) else "A"
    return _flank(rng, left, before, True) + node[a:a + n] + _flank(rng, right, after, False)


def small_cases(k: int) -> List[DepthCase]:
    K = k + 1
    rng = np.random.default_rng(1000 + k)
    out: List[DepthCase] = []
    long_node = dna(rng, 5 * K + 11)
    other = dna(rng, 2 * K)

    out.append(DepthCase("match_of_exactly_K", k, [long_node, other], [_cut(rng, long_node, 17, K), _cut(rng, long_node, 3, K - 1)],
                         want={0: 1}, tells=("len_not_windows",)))
    rlen = 2 * K + 7 + (3 * K if k == 21 else 0)  # (k = 21: long enough to hold several grid points of one match)
    rlen = min(rlen, len(long_node) - 5)
    out.append(DepthCase("read_inside_a_long_node", k, [long_node, other], [long_node[5:5 + rlen], other[:K - 1]],
                         want={0: rlen - K + 1}, tells=("per_grid_point", "len_not_windows")))
    # nodes that share k-base overlaps, as a compacted de Bruijn graph has them
    g = dna(rng, 6 * K)
    c1, c2 = 2 * K, 4 * K
    two = [g[:c1], g[c1 - k:]]
    three = [g[:c1], g[c1 - k:c2], g[c2 - k:]]
    out.append(DepthCase("read_across_a_junction_of_two_nodes", k, two, [g[c1 - K - 4:c1 + K], revcomp(g[c1 - K - 4:c1 + K])],
                         want={0: 2 * 5, 1: 2 * K}, tells=("one_strand",)))
    span = g[c1 - K - 2:c2 + K + 3]
    out.append(DepthCase("read_across_a_junction_of_three_nodes", k, three, [span], singles=True,
                         want={0: 3, 1: c2 - c1, 2: K + 3}))
    out.append(DepthCase("either_strand", k, [long_node, other], [revcomp(long_node[7:7 + K + 6]), long_node[7:7 + K + 6]],
                         want={0: 14}, tells=("one_strand",)))
    half = dna(rng, K // 2)
    pal = half + revcomp(half)
    pal_node = pal + dna(rng, K)
    out.append(DepthCase("node_whose_first_K_bases_are_a_palindrome", k, [pal_node, other], [pal_node[:K + 4]], singles=True,
                         tells=("palindrome_once",)))
    rep = dna(rng, K)
    n_a = dna(rng, 12) + rep + dna(rng, 15) + rep + dna(rng, 9)
    n_b = dna(rng, 20) + rep + dna(rng, 8)
    out.append(DepthCase("same_window_at_two_offsets_of_one_node_and_in_two_nodes", k, [n_a, n_b, other], [rep], singles=True))
    core = dna(rng, K + 5)
    hundred = [dna(rng, 20) + core + dna(rng, 20) for _ in range(100)]
    out.append(DepthCase("seed_with_100_postings", k, hundred, [core, revcomp(core)]))
    piece = long_node[9:9 + 2 * K]
    out.append(DepthCase("N_cuts_a_match_into_K_and_K_minus_1", k, [long_node, other], [piece[:K] + "N" + piece[K + 1:], long_node[:K + 2]],
                         want={0: 1 + 3}, tells=("pair_filter",)))
    dirty = list(long_node[2:2 + 4 * K + 6])
    for pos, ch in zip((K, 2 * K + 1, 2 * K + 3, 3 * K + 3, 3 * K + 4, 4 * K + 5), "NRn*.-"):
        dirty[pos] = ch
    out.append(DepthCase("six_bad_bytes_in_one_end", k, [long_node, other], ["".join(dirty), other[:K + 1]]))
    low = long_node[4:4 + 2 * K + 9]
    out.append(DepthCase("lowercase_bases", k, [long_node, other], [low[:K + 2] + low[K + 2:K + 5].lower() + low[K + 5:], low.lower()],
                         want={0: 3 + max(0, len(low) - (K + 5) - K + 1)}))
    out.append(DepthCase("ends_of_length_K_minus_1_0_and_absent", k, [long_node, other], [long_node[:K - 1], "", long_node[3:3 + K + 3]],
                         singles=True, want={0: 4}))
    out.append(DepthCase("short_mate_and_N_mate_still_count", k, [long_node, other],
                         [long_node[:K + 1], long_node[:K - 1], long_node[6:6 + K + 2], "N" + other[:K]],
                         want={0: 2 + 3, 1: 1}, tells=("pair_filter",)))
    chain_text = dna(rng, 5 * (K + 5))
    chain = [chain_text[i * 5:i * 5 + K + 5] for i in range((len(chain_text) - K - 5) // 5 + 1)]
    out.append(DepthCase("read_longer_than_every_node", k, chain, [_cut(rng, chain_text, 0, len(chain_text))], singles=True))
    out.append(DepthCase("block_of_one_end", k, [long_node, other], [long_node[1:1 + K + 8]], singles=True, want={0: 9}))
    return out


def share_plus_one(k: int, share: int):
    """A singles block of ``share + 1`` short reads over a few nodes: ``2 * share + 2`` ends, so the last workgroup's share
    holds one read and its absent twin -- one end more than a multiple of the share is no block (ends come in twos)."""
    K = k + 1
    rng = np.random.default_rng(2000 + k)
    seqs = [dna(rng, 3 * K) for _ in range(5)]
    ends = []
    for i in range(share + 1):
        n = seqs[i % 5]
        a = (i * 7) % (len(n) - K - 3)
        ends.append(n[a:a + K + (i % 4)])
    return DepthCase("end_count_one_more_than_a_multiple_of_the_share", k, seqs, ends, singles=True)


def many_nodes(k: int, n_nodes: int):
    """``n_nodes`` short random nodes (the global route when that is above the plan's limit) and ends that credit one node
    from many lanes of a wavefront, many nodes from one wavefront, and either strand."""
    K = k + 1
    rng = np.random.default_rng(3000 + k)
    codes = rng.integers(0, 4, size=(n_nodes, K + 2))
    seqs = ["".join("ACGT"[c] for c in row) for row in codes]
    ends = [seqs[7]] * 70 + [seqs[i * 97 % n_nodes] for i in range(200)] + [revcomp(seqs[n_nodes - 1]), seqs[0][:K], seqs[1][1:], "ACGT" * K]
    return DepthCase("graph_just_above_the_node_limit", k, seqs, ends)
