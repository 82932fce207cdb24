"""Constructed blocks for the depth profile (``vs_node_cover``): the blocks of the depth pass (tests/node_depth_cases.py,
unchanged) and graphs in which one thing at a time can go wrong about WHERE on a segment a match is written down.  Expected
profiles come from tests/depth_profile_model.py; where the construction fixes one it is written into the case (``want``:
segment -> its profile) and tests/test_depth_profile_model_cpu.py holds the model to it.  tests/test_depth_profile_gpu.py
runs the same cases on the device at k = 21, 55 and 127."""
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from node_depth_cases import KS, DepthCase, _cut, dna, small_cases  # noqa: F401  (KS, DepthCase: for the tests)
from oracle.pe_oracle import revcomp

SCAN_SHARE = 2048  # values one workgroup of the library's exclusive scan takes


class CoverCase(NamedTuple):
    name: str
    k: int
    seqs: List[str]
    ends: List[str]
    singles: bool = False
    want: Optional[Dict[int, List[int]]] = None  # profiles the construction fixes
    tells: tuple = ()                            # the named mistakes (depth_profile_model variants) this case must expose


def _from_depth(c: DepthCase) -> CoverCase:
    return CoverCase(c.name, c.k, c.seqs, c.ends, c.singles, None, ())


def _profile(n_windows: int, *runs) -> List[int]:
    row = [0] * n_windows
    for a, b, v in runs:
        for p in range(a, b):
            row[p] += v
    return row


def flush_graph(k: int, rng, n_segs: int = 12):
    """A dozen segments of different lengths and, for each, an end matching its last K + 3 bases flush with its end."""
    K = k + 1
    seqs = [dna(rng, 2 * K + 3 + 2 * i) for i in range(n_segs)]
    ends = [_cut(rng, s, len(s) - (K + 3), K + 3) for s in seqs]
    want = {i: _profile(len(s) - K + 1, (len(s) - K + 1 - 4, len(s) - K + 1, 1)) for i, s in enumerate(seqs)}
    return seqs, ends, want


def cover_cases(k: int) -> List[CoverCase]:
    K = k + 1
    rng = np.random.default_rng(4000 + k)
    out = [_from_depth(c) for c in small_cases(k)]
    node = dna(rng, 4 * K + 9)
    other = dna(rng, 2 * K + 1)
    W = len(node) - K + 1

    a = 5  # (the mirror position of a match of K + 5 bases at a is len - a - (K + 5): far from a)
    assert abs((len(node) - a - (K + 5)) - a) > K
    out.append(CoverCase("reverse_complement_read_away_from_the_mirror_position", k, [node, other],
                         [revcomp(node[a:a + K + 5]), other[:K - 1]], want={0: _profile(W, (a, a + 6, 1))}, tells=("no_mirror", "first_window_only")))
    out.append(CoverCase("two_ends_overlapping_on_one_segment", k, [node, other], [node[3:3 + K + 9], node[8:8 + K + 9]],
                         want={0: _profile(W, (3, 13, 1), (8, 18, 1))}, tells=("first_window_only",)))
    win = node[K + 4:2 * K + 4]
    gap = [b for b in "ACGT" if b not in (node[2 * K + 4], node[K + 3])][0]  # (neither copy grows into it)
    out.append(CoverCase("one_end_holding_a_window_of_the_segment_twice", k, [node, other], [win + gap + win], singles=True,
                         want={0: _profile(W, (K + 4, K + 5, 2))}))
    long_read = node[2:2 + 3 * K + 4]
    out.append(CoverCase("match_holding_several_grid_points", k, [node, other], [long_read], singles=True,
                         want={0: _profile(W, (2, 2 + 2 * K + 5, 1))}, tells=("per_grid_point", "first_window_only")))
    exact = dna(rng, K)
    shorts = [dna(rng, K - 1), exact, dna(rng, 3), node, dna(rng, 1), dna(rng, K // 2)]
    out.append(CoverCase("segment_of_exactly_K_bases_and_shorter_ones_between_others", k, shorts,
                         [exact, revcomp(exact), node[1:1 + K + 2], shorts[0]], want={1: [2], 3: _profile(W, (1, 4, 1))}))
    half = dna(rng, K // 2)
    pal_node = half + revcomp(half) + dna(rng, K + 2)
    out.append(CoverCase("palindromic_first_window", k, [pal_node, other], [pal_node[:K]], singles=True,
                         want={0: _profile(len(pal_node) - K + 1, (0, 1, 2))}, tells=("palindrome_once",)))
    seqs, ends, want = flush_graph(k, rng)
    out.append(CoverCase("every_segment_matched_flush_with_its_end", k, seqs, ends, want=want, tells=("leak_past_end", "first_window_only")))
    out.append(CoverCase("every_segment_matched_flush_with_its_end_by_reverse_complemented_ends", k, seqs, [revcomp(e) for e in ends], want=want,
                         tells=("leak_past_end", "no_mirror")))  # (flush with the START of the other strand's text)
    out.append(CoverCase("every_segment_matched_flush_with_its_start_by_reverse_complements", k, [revcomp(s) for s in seqs], ends,
                         want={i: _profile(len(s) - K + 1, (0, 4, 1)) for i, s in enumerate(seqs)}, tells=("no_mirror", "first_window_only")))
    return out


def scan_share_case(k: int, extra: bool) -> CoverCase:
    """512 segments of K + 2 bases -- 3 windows and the sentinel: 2 048 slots, one scan workgroup's share -- and, with
    ``extra``, one of K bases behind them (2 050 slots: no segment owns a single slot, so 2 049 cannot be made); a read on
    every segment."""
    K = k + 1
    rng = np.random.default_rng(5000 + k)
    codes = rng.integers(0, 4, size=(512, K + 2))
    seqs = ["".join("ACGT"[c] for c in row) for row in codes]
    ends = [s[i % 3:i % 3 + K] if i % 2 else revcomp(s) for i, s in enumerate(seqs)]
    if extra:
        seqs.append(dna(rng, K))
        ends.append(seqs[-1])
    if len(ends) % 2:
        ends.append(seqs[0][1:])
    return CoverCase("slot_total_%d" % slot_total(seqs, k), k, seqs, ends)


def slot_total(seqs, k: int) -> int:
    K = k + 1
    return sum(len(s) - K + 2 for s in seqs if len(s) >= K)
