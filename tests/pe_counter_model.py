"""Host statement of the counter stage of a PE count (vstrains_amd/csrc/vs_pe.hip, K4): what node_mat and short_mat
must hold after a block of per-end node lists, in plain numpy int64 -- PE_Inference.py:174-188 and nothing else -- and
restatements of the hashing of the counter kernels.  The restatements never predict a result: they construct inputs and
assert that an input has the property a test is about (tests/test_pe_counters_gpu.py on the device,
tests/test_pe_counters_cpu.py the same assertions without one).  Nothing here imports the library."""
import numpy as np

LCAP = 20  # nodes an end may list
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


# ---- the plain statement ---------------------------------------------------------------------------------------------
def count_block(lists, counts, n_nodes: int):
    """lists int [2 P, 20], counts int [2 P] (left end, right end of pair 0, of pair 1, ...) ->
    ((cells, values) of node_mat, (cells, values) of short_mat): ascending flat cell indices x * n_nodes + y (int64) of
    the cells that are not zero, and what they hold (int64).  No n_nodes x n_nodes array is made."""
    lists = np.asarray(lists, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    node_keys, short_keys = [], []
    for p in range(counts.size // 2):
        left = lists[2 * p, : counts[2 * p]]
        right = lists[2 * p + 1, : counts[2 * p + 1]]
        # node_mat[l][r] += 1 for l in the left list, r in the right list (:185-188)
        node_keys.append((left[:, None] * n_nodes + right[None, :]).ravel())
        # short_mat[min][max] += 1 over the positions a <= b of either end's list (:174-184); an empty end adds nothing
        for end in (left, right):
            a, b = np.triu_indices(end.size)
            short_keys.append(np.minimum(end[a], end[b]) * n_nodes + np.maximum(end[a], end[b]))
    out = []
    for keys in (node_keys, short_keys):
        allk = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
        cells, values = np.unique(allk, return_counts=True)
        out.append((cells.astype(np.int64), values.astype(np.int64)))
    return out[0], out[1]


def count_block_dense(lists, counts, n_nodes: int):
    """The same as obvious loops into two dense matrices (small n_nodes only)."""
    node = np.zeros((n_nodes, n_nodes), dtype=np.int64)
    short = np.zeros((n_nodes, n_nodes), dtype=np.int64)
    for p in range(len(counts) // 2):
        left = [int(x) for x in lists[2 * p][: counts[2 * p]]]
        right = [int(x) for x in lists[2 * p + 1][: counts[2 * p + 1]]]
        for l in left:
            for r in right:
                node[l][r] += 1
        for end in (left, right):
            for a in range(len(end)):
                for b in range(a, len(end)):
                    short[min(end[a], end[b])][max(end[a], end[b])] += 1
    return node, short


def tiles_of(cells, n_nodes: int):
    """The 64 x 64 tiles that hold the cells, as a set of tx * T + ty with T = ceil(n_nodes / 64)."""
    T = (n_nodes + 63) // 64
    cells = np.asarray(cells, dtype=np.int64)
    return set(int(t) for t in np.unique((cells // n_nodes // 64) * T + (cells % n_nodes) // 64))


# ---- restated hashing: the cell tables (CellTable<BITS>) -------------------------------------------------------------------
ACC_BITS, RS_BITS = 14, 13          # k_pe_accumulate's table, the strips' (k_rows_sum)
ACC_SLOTS, RS_SLOTS = 1 << ACC_BITS, 1 << RS_BITS
CELL_PROBES = 8                     # vs_cell_claim


def cell_slot(key, bits: int):
    """CellTable<bits>::slot: a group of 16 slots from the key >> 4, the slot inside it from the low four bits."""
    key = np.asarray(key, dtype=np.uint64)
    return ((((((key >> np.uint64(4)) * np.uint64(0x9E3779B1)) & np.uint64(M32)) >> np.uint64(36 - bits)) << np.uint64(4)) | (key & np.uint64(15))).astype(np.int64)


def cell_next(at: int, bits: int) -> int:
    return (at + 16) & ((1 << bits) - 1)


def acc_key(mat: int, x, y, n_nodes: int):
    """k_pe_accumulate's key of cell (x, y) of matrix ``mat`` (0 node_mat, 1 short_mat); 2 * n_nodes^2 must fit 32 bits."""
    assert 2 * n_nodes * n_nodes - 1 <= M32
    return (mat * n_nodes + np.asarray(x, dtype=np.int64)) * n_nodes + np.asarray(y, dtype=np.int64)


def rows_key(x, y, first: int, n_nodes: int, mat_ptr: int):
    """k_rows_sum's key of cell (x, y) in a strip whose first row is ``first``: the cell index relative to that row,
    shifted so that key >> 4 is one 64-byte stretch of the matrix at device address ``mat_ptr``."""
    off = (mat_ptr >> 2) & 15
    align = (first * n_nodes + off) & 15
    return (np.asarray(x, dtype=np.int64) - first) * n_nodes + align + np.asarray(y, dtype=np.int64)


def placed(keys, bits: int):
    """Which of ``keys`` (distinct, in this order, one after another) find a slot within CELL_PROBES probes of an empty table."""
    taken, out = set(), []
    for home in cell_slot(np.asarray(keys), bits).reshape(-1).tolist():
        at, ok = int(home), False
        for _ in range(CELL_PROBES):
            if at not in taken:
                taken.add(at)
                ok = True
                break
            at = cell_next(at, bits)
        out.append(ok)
    return out


# ---- restated hashing: the list table (k_list_owners) ------------------------------------------------------------------
LTAB_PROBES = 16


def node_hash(nodes):
    """What one listed node adds to the fingerprint of its list.  uint64, the shape of ``nodes``."""
    with np.errstate(over="ignore"):
        g = (np.asarray(nodes, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        g ^= g >> np.uint64(29)
        return g * np.uint64(0xBF58476D1CE4E5B9)


def list_fingerprint(lists, counts):
    """f2 of every end: its length plus a sum over its nodes (order-independent), 64-bit wrap-around.  uint64 [ends]."""
    counts = np.asarray(counts, dtype=np.uint64)
    with np.errstate(over="ignore"):
        g = node_hash(lists)
        g[np.arange(LCAP, dtype=np.uint64)[None, :] >= counts[:, None]] = 0
        return counts + g.sum(axis=1, dtype=np.uint64)


def list_tag(f2, counts):
    """The 32-bit tag of a list: 27 bits of the fingerprint, the length - 1 in the low five (lists of length >= 1)."""
    f2 = np.asarray(f2, dtype=np.uint64)
    return ((((f2 >> np.uint64(32)) & np.uint64(M32 & ~31)) | (np.asarray(counts, dtype=np.uint64) - np.uint64(1))) & np.uint64(M32)).astype(np.int64)


def list_home(f2, ltab_bits: int):
    with np.errstate(over="ignore"):
        return ((np.asarray(f2, dtype=np.uint64) * np.uint64(0xD6E8FEB86659FD93)) >> np.uint64(64 - ltab_bits)).astype(np.int64)


def ltab_bits_for(n_pairs: int) -> int:
    """The table of a transposition of n_pairs pairs: a power of two of slots, at least one per end, at least 1 024."""
    b = 10
    while (1 << b) < 2 * n_pairs and b < 31:
        b += 1
    return b


def tag_collisions(lists, counts):
    """Pairs of ends (i, j) that hold DIFFERENT node sets under one tag."""
    f2 = list_fingerprint(lists, counts)
    tags = list_tag(f2, np.maximum(np.asarray(counts), 1))
    by_tag = {}
    for e in np.nonzero(np.asarray(counts) > 0)[0]:
        by_tag.setdefault(int(tags[e]), []).append(int(e))
    out = []
    for ends in by_tag.values():
        sets = {}
        for e in ends:
            sets.setdefault(frozenset(int(x) for x in lists[e][: counts[e]]), e)
        reps = sorted(sets.values())
        out += [(reps[0], other) for other in reps[1:]]
    return out
