"""The plain model of counting UNPAIRED reads: what the reference does with one end of a pair
(utils/VStrains_PE_Inference.py:160-184, restricted to one end), over the oracle's own table and mapper.

1. a read with an 'N' is counted as an N read, nothing else;
2. otherwise a read shorter than k+1 is counted as a short read, nothing else;
3. otherwise it is used: L = the nodes it saturates, short_mat[L[a]][L[b]] += 1 for every a <= b;
4. node_mat is never touched.
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import pe_oracle


def read_class(read: str, split_len: int) -> int:
    """0: N read, 1: short read, 2: used"""
    if read.count("N") > 0:
        return 0
    if len(read) < split_len:
        return 1
    return 2


class Model:
    """The table of one graph, built once and shared by the cases that count on it."""

    def __init__(self, seqs: Sequence[str], ksize: int):
        self.seqs = list(seqs)
        self.split_len = ksize + 1
        self.table: Dict[str, List[Tuple[int, int]]] = pe_oracle.build_table(self.seqs, self.split_len)
        self.seqlens = [len(s) for s in self.seqs]
        self._seen: Dict[str, List[int]] = {}  # (the blocks repeat their reads)

    def nodes(self, read: str) -> List[int]:
        """accepted nodes of a USED read, ascending"""
        got = self._seen.get(read)
        if got is None:
            got = self._seen[read] = pe_oracle.map_read_end(read, self.table, self.seqlens, self.split_len)
        return list(got)

    def lists(self, reads: Sequence[str]) -> List[List[int]]:
        """per read: its accepted nodes, [] for a read that rules 1 / 2 drop"""
        return [self.nodes(s) if read_class(s, self.split_len) == 2 else [] for s in reads]

    def count(self, reads: Sequence[str], pair_filter: bool = False):
        """-> (node_mat, short_mat, (n_reads, short_reads, used_reads)); node_mat is returned to be compared with zero.

        ``pair_filter``: the MISTAKE the cases must be able to see -- reads taken two at a time as if they were the ends of
        a pair, both dropped when either has an 'N' or is short (PE_Inference.py:160-165)."""
        n = len(self.seqs)
        node_mat = np.zeros((n, n), dtype=np.int64)
        short_mat = np.zeros((n, n), dtype=np.int64)
        tally = [0, 0, 0]
        for r, s in enumerate(reads):
            cls = read_class(s, self.split_len)
            if pair_filter and (r ^ 1) < len(reads):
                cls = min(cls, read_class(reads[r ^ 1], self.split_len))
            tally[cls] += 1
            if cls != 2:
                continue
            L = self.nodes(s)
            for a in range(len(L)):
                for b in range(a, len(L)):
                    short_mat[L[a], L[b]] += 1
        return node_mat, short_mat, tuple(tally)
