"""Constructed inputs for the PE-link table kernels (K5), each about one edge of a tile, a list or a launch.

Every generator has a fixed seed, is made once (``functools.lru_cache``) and hands out read-only arrays.  A case carries its
inputs, the plain model of its table (``links_model.LinksModel``), the queries and group lists to ask, and the facts about
itself that ``test_links_model_cpu.py`` asserts -- so that a case cannot lose its edge unnoticed.  numpy only: the GPU test
puts the arrays on the device, the CPU test compares the model with the literal dict of the reference.

Counters are uint32 (``*_counts``), int64 (``wide``); a tile is 64 x 64 cells of a counter matrix; ``marks[m, I, J]`` is the
dirty-tile byte of tile (I, J) of matrix m (0 node, 1 short) as ``vs_pe_count_tracked`` keeps it."""
import functools
import types

import numpy as np

from links_model import LinksModel

TILE = 64
GARBAGE = 0xDEADBEEF  # what unmarked tiles hold: never read, so never part of a result
BIG = 2 ** 61 - 1     # the largest magnitude of an int64 input (four of them still fit int64)

DENSE_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 97]
GROUP_SIZES = [255, 256, 257]
COL_LIST_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129]  # and 2 n
ROW_LIST_LENGTHS = [0, 1, 2, 64, 65]
QUERY_COUNTS = [1, 3, 4, 5, 1025]
SUBSET_NAMES = {1: "node(I,J)", 2: "node(J,I)", 4: "short(I,J)", 8: "short(J,I)"}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _case(**kw):
    return types.SimpleNamespace(**kw)


def fits_int64(x):
    return -2 ** 63 <= x < 2 ** 63


def random_queries(rng, n, count, max_rows, max_cols, repeats=True):
    out = []
    for _ in range(count):
        a, b = int(rng.integers(0, max_rows + 1)), int(rng.integers(0, max_cols + 1))
        if repeats:
            out.append((rng.integers(0, n, a).tolist(), rng.integers(0, n, b).tolist()))
        else:
            out.append((rng.permutation(n)[:a].tolist(), rng.permutation(n)[:b].tolist()))
    return out


def group_sets(rng, n):
    """Group lists of 1, 2 and 7 groups, an empty group among them, the last index in one of them."""
    draw = lambda k: rng.integers(0, n, k).tolist()
    return [[draw(5) + [n - 1]],
            [[], draw(64) + [n - 1]],
            [draw(1), draw(2), [], draw(63), draw(64) + [n - 1, 0], draw(65), draw(129)]]


# ---- dense build ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_case(n, wide):
    """Two n x n matrices, filled independently at (i, j) and (j, i) so that a transposed read shows.  ``wide=False``: the
    whole uint32 range, 2^31 and 2^32 - 1 on the diagonal and off it.  ``wide=True``: int64 of either sign, magnitudes up
    to 2^61 - 1.  The lists of the wide case hold no index twice, so that no block sum leaves int64."""
    rng = np.random.default_rng([1, n, int(wide)])
    d = n - 1
    if wide:
        node = rng.integers(-2 ** 40, 2 ** 40, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.4)
        short = rng.integers(-2 ** 40, 2 ** 40, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.3)
        node[d, d], short[d, d] = BIG, BIG
        if n > 1:
            node[0, 0], short[0, 0] = BIG, -BIG + 7  # (cancels to 7)
            node[0, d] = -BIG
    else:
        node = rng.integers(0, 2 ** 32, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.4)
        short = rng.integers(0, 2 ** 32, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.3)
        node[d, d], short[d, d] = 2 ** 32 - 1, 2 ** 31
        if n > 1:
            node[0, d], node[d, 0], short[0, d], short[d, 0] = 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31
    _freeze(node, short)
    queries = random_queries(rng, n, 12, n, n, repeats=False) + [(list(range(n)), list(range(n))), ([d], [0]), ([0], [d])]
    same = rng.permutation(n)[:max(1, n // 2)].tolist()
    queries.append((same, same))
    perm = rng.permutation(n).tolist()
    groups = [[perm[:n // 3], [], perm[n // 3:2 * n // 3], perm[2 * n // 3:]]]
    if not wide:
        queries += random_queries(rng, n, 12, 5, 130)
        groups += group_sets(rng, n)
    return _case(id="dense_n%d_%s" % (n, "int64" if wide else "uint32"), n=n, wide=wide, node=node, short=short,
                 model=LinksModel.from_matrices(node, short), queries=queries, groups=groups)


# ---- source-tile mixes ------------------------------------------------------------------------------------------------------

def tile_pairs(T):
    """The off-diagonal tile pairs (I, J), I < J, those that contain the last tile first."""
    off = [(I, J) for I in range(T) for J in range(I + 1, T)]
    return [p for p in off if p[1] == T - 1] + [p for p in off if p[1] != T - 1]


def _tile(mat, I, J):
    return mat[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE]


def _dirty(mats, marks):
    dirty = mats.copy()
    T = marks.shape[1]
    for m in range(2):
        for I in range(T):
            for J in range(T):
                if not marks[m, I, J]:
                    _tile(dirty[m], I, J)[...] = GARBAGE
    return dirty


@functools.lru_cache(maxsize=None)
def tile_mix_case(n, rot):
    """uint32 counters with a dirty-tile map.  The pair at position p of ``tile_pairs`` has the subset (p + 5 rot) mod 15 + 1
    of its four source tiles marked (bit 1 node (I,J), 2 node (J,I), 4 short (I,J), 8 short (J,I)); the diagonal tile I has
    node only, short only or both by (I + rot) mod 3.  With T = 6, five pairs contain the partial last tile: rot = 0, 1, 2
    puts every one of the 15 subsets on such a pair once.  Marked tiles hold random cells, one of them is completely
    non-zero and one completely zero; unmarked tiles hold GARBAGE in ``dirty``."""
    T = -(-n // TILE)
    rng = np.random.default_rng([2, n, rot])
    marks = np.zeros((2, T, T), dtype=np.uint8)
    subsets = {}
    for pos, (I, J) in enumerate(tile_pairs(T)):
        mask = (pos + 5 * rot) % 15 + 1
        subsets[(I, J)] = mask
        marks[0, I, J], marks[0, J, I], marks[1, I, J], marks[1, J, I] = mask & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1
    diagonal = {}
    for I in range(T):
        kind = (I + rot) % 3
        diagonal[I] = ("node", "short", "both")[kind]
        marks[0, I, I], marks[1, I, I] = kind != 1, kind != 0
    mats = rng.integers(1, 2 ** 32, size=(2, n, n), dtype=np.int64) * (rng.random((2, n, n)) < 0.1)
    marked = [(m, I, J) for m in range(2) for I in range(T) for J in range(T) if marks[m, I, J]]
    whole = [t for t in marked if _tile(mats[t[0]], t[1], t[2]).shape == (TILE, TILE)] or marked
    full = whole[rot % len(whole)]
    rest = [t for t in marked if t != full]
    zero = rest[(3 * rot + 1) % len(rest)]
    for m in range(2):
        for I in range(T):
            for J in range(T):
                if not marks[m, I, J]:
                    _tile(mats[m], I, J)[...] = 0
    t = _tile(mats[full[0]], full[1], full[2])
    t[...] = rng.integers(1, 2 ** 32, size=t.shape, dtype=np.int64)
    _tile(mats[zero[0]], zero[1], zero[2])[...] = 0
    dirty = _dirty(mats, marks)
    _freeze(mats, dirty, marks)
    queries = random_queries(rng, n, 40, 5, 130) + [(list(range(n)), list(range(n)))]
    return _case(id="tiles_n%d_rot%d" % (n, rot), n=n, T=T, node=mats[0], short=mats[1], dirty_node=dirty[0], dirty_short=dirty[1],
                 marks=marks, subsets=subsets, diagonal=diagonal, full=full, zero=zero, model=LinksModel.from_matrices(mats[0], mats[1]),
                 queries=queries, groups=group_sets(rng, n))


TILE_MIX_CASES = [(322, 0), (322, 1), (322, 2), (64, 2), (65, 1)]


# ---- lists ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lists_case():
    """n = 322 uint32 counters with a dirty-tile map whose table has empty rows (EMPTY), a row with exactly one stored cell
    (SINGLE, at column SINGLE_COL) and a row stored only from column 100 to column 200 (NARROW) -- and the row lists, column
    lists and query counts at which lane striding, the shuffle reduction and the workgroup of four wavefronts change."""
    n = 322
    T = -(-n // TILE)
    rng = np.random.default_rng([3])
    EMPTY, SINGLE, SINGLE_COL, NARROW = (7, 130, 131, 321), 250, 64, 40
    mats = rng.integers(1, 2 ** 32, size=(2, n, n), dtype=np.int64) * (rng.random((2, n, n)) < 0.03)
    for x in EMPTY + (SINGLE,):
        mats[:, x, :] = 0
        mats[:, :, x] = 0
    mats[1, SINGLE_COL, SINGLE] = 5  # (read transposed)
    mats[:, NARROW, :100] = 0
    mats[:, NARROW, 201:] = 0
    mats[:, :100, NARROW] = 0
    mats[:, 201:, NARROW] = 0
    for c in (100, 200):
        mats[:, NARROW, c] = 0
        mats[:, c, NARROW] = 0
    mats[0, NARROW, 100] = 3
    mats[1, 200, NARROW] = 9
    for m, I, J in ((0, 1, 3), (1, 3, 1), (0, 2, 2), (1, 5, 0)):  # whole tiles without a cell: unmarked
        _tile(mats[m], I, J)[...] = 0
    marks = np.zeros((2, T, T), dtype=np.uint8)
    for m in range(2):
        for I in range(T):
            for J in range(T):
                marks[m, I, J] = 1 if _tile(mats[m], I, J).any() else 0
    dirty = _dirty(mats, marks)
    _freeze(mats, dirty, marks)
    draw = lambda k: rng.integers(0, n, k).tolist()
    named = {}
    for cl in COL_LIST_LENGTHS + [2 * n]:
        cols = draw(cl)
        for rl in ROW_LIST_LENGTHS:
            named["rows%d_cols%d" % (rl, cl)] = (draw(rl), cols)
    named["one_index_repeated"] = ([17] * 65, [64] * 129)
    named["single_cell_repeated"] = ([SINGLE] * 64, [SINGLE_COL] * 65)
    same = draw(65)
    named["same_list_both_sides"] = (same, same)
    named["only_empty_rows"] = (list(EMPTY) * 3, draw(129))
    named["empty_rows_as_columns"] = (draw(64), list(EMPTY))
    named["below_first_stored"] = ([NARROW], list(range(0, 100)))
    named["above_last_stored"] = ([NARROW], list(range(201, n)))
    named["just_below_first"] = ([NARROW], [99])
    named["just_above_last"] = ([NARROW], [201])
    named["equal_first"] = ([NARROW], [100])
    named["equal_last"] = ([NARROW], [200])
    named["first_and_last"] = ([NARROW, NARROW], [200, 100, 0, n - 1])
    named["single_row_its_cell"] = ([SINGLE], [SINGLE_COL])
    named["single_row_one_below"] = ([SINGLE], [SINGLE_COL - 1])
    named["single_row_one_above"] = ([SINGLE], [SINGLE_COL + 1])
    named["single_row_many"] = ([SINGLE], draw(65) + [SINGLE_COL])
    named["last_column_of_empty_row"] = ([0, 1, 2], [n - 1])
    by_count = {k: random_queries(rng, n, k, 3, 5) for k in QUERY_COUNTS}
    return _case(id="lists_n322", n=n, T=T, node=mats[0], short=mats[1], dirty_node=dirty[0], dirty_short=dirty[1], marks=marks,
                 EMPTY=EMPTY, SINGLE=SINGLE, SINGLE_COL=SINGLE_COL, NARROW=NARROW, model=LinksModel.from_matrices(mats[0], mats[1]),
                 named=named, queries=list(named.values()), by_count=by_count, groups=group_sets(rng, n))


@functools.lru_cache(maxsize=None)
def group_case(n):
    """The dense group matrix at the column guard of its first pass (256 columns per workgroup)."""
    rng = np.random.default_rng([5, n])
    node = rng.integers(0, 2 ** 32, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.2)
    short = rng.integers(0, 2 ** 32, size=(n, n), dtype=np.int64) * (rng.random((n, n)) < 0.2)
    node[0, n - 1], short[n - 1, n - 2], node[n - 1, n - 1] = 2 ** 32 - 1, 2 ** 31, 77
    _freeze(node, short)
    groups = group_sets(rng, n) + [[list(range(n)), [n - 1], [n - 2, n - 1, 255 % n, 254]]]
    return _case(id="groups_n%d" % n, n=n, wide=False, node=node, short=short, model=LinksModel.from_matrices(node, short),
                 queries=random_queries(rng, n, 20, 5, 130), groups=groups)


# ---- pieces and chunks ---------------------------------------------------------------------------------------------------------

PIECES_CASES = [(4096, "full"), (4096, "thin"), (4097, "full"), (4097, "thin")]


@functools.lru_cache(maxsize=None)
def pieces_case(n, variant):
    """uint32 counters of n = 4096 / 4097 nodes (T = 64 / 65 tile columns: one 64-lane chunk of k_sl_rows, or one and a
    carry into a second) given as cells, a few thousand of them, never as a matrix.

    The table is symmetric, so a row that is non-zero in every column leaves no row empty: the rows the issue lists are
    spread over two tables per n.
      "full": FULL is non-zero in every column (every piece full, at n = 4097 the last piece has 1 cell) -- and so every
              other row has a cell in column FULL; STRIPE as below; scattered cells.
      "thin": STRIPE has one cell in every tile column, in the piece's first column for even tile columns and its last for
              odd ones; ONLY_LAST's only cell lies in the last tile column (tile column 64 at n = 4097); CARRY has cells in
              the last two tile columns only (63 and 64 at n = 4097: the chunk carry); row n - 1 (at n = 4097 the lone row of
              the last tile row) holds the mirrors of those; scattered cells among 1 200 indices, every other row empty."""
    T = -(-n // TILE)
    rng = np.random.default_rng([4, n, int(variant == "full")])
    FULL, STRIPE, ONLY_LAST, CARRY = 100, 300, 500, 700
    cells = {}  # (m, r, c) -> value

    def put(m, r, c):
        cells[(m, r, c)] = int(rng.integers(1, 2 ** 32))

    stripe_cols = []
    for t in range(T):
        c = t * TILE if t % 2 == 0 else min(t * TILE + TILE - 1, n - 1)
        stripe_cols.append(c)
        if t % 3 == 0:
            put(t % 2, STRIPE, c)
        else:
            put(t % 2, c, STRIPE)
    carry_cols = [(T - 2) * TILE + 5, n - 1]
    if variant == "full":
        for c in range(n):
            if c % 2 == 0:
                put(0, FULL, c)
            else:
                put(1, c, FULL)
    else:
        put(0, n - 1, ONLY_LAST)
        put(1, CARRY, carry_cols[0])
        put(0, CARRY, carry_cols[1])
    taken = set(stripe_cols) | set(carry_cols) | {FULL, STRIPE, ONLY_LAST, CARRY, n - 1}
    pool = np.asarray([i for i in rng.permutation(n).tolist() if i not in taken][:1200])
    for _ in range(3000):
        put(int(rng.integers(0, 2)), int(rng.choice(pool)), int(rng.choice(pool)))
    touched = taken | set(pool.tolist())
    empty_rows = [i for i in range(n) if i not in touched][:8] if variant == "thin" else []
    keys = sorted(cells)
    split = {}
    marks = np.zeros((2, T, T), dtype=np.uint8)
    for m in range(2):
        ks = [k for k in keys if k[0] == m]
        r = np.asarray([k[1] for k in ks], dtype=np.int64)
        c = np.asarray([k[2] for k in ks], dtype=np.int64)
        v = np.asarray([cells[k] for k in ks], dtype=np.int64)
        marks[m, r // TILE, c // TILE] = 1
        _freeze(r, c, v)
        split[m] = (r, c, v)
    _freeze(marks)
    model = LinksModel(n, ((r, c, v) for (m, r, c), v in cells.items()))
    specials = [STRIPE] + ([FULL] if variant == "full" else [ONLY_LAST, CARRY])
    row_lists = [[x] for x in specials] + [[n - 1], specials + [n - 1], empty_rows, rng.choice(pool, 5).tolist()]
    col_lists = [list(range(n)), list(range((T - 2) * TILE, n)), [n - 1], stripe_cols, [(T - 1) * TILE - 1, (T - 1) * TILE],
                 rng.integers(0, n, 129).tolist()]
    queries = [(a, b) for a in row_lists for b in col_lists]
    groups = [[specials, [], [n - 1, 0, 63, 64], rng.choice(pool, 65).tolist()]]
    return _case(id="pieces_n%d_%s" % (n, variant), n=n, T=T, variant=variant, node_cells=split[0], short_cells=split[1], marks=marks,
                 FULL=FULL, STRIPE=STRIPE, ONLY_LAST=ONLY_LAST, CARRY=CARRY, empty_rows=empty_rows, n_cells=len(cells), model=model,
                 queries=queries, groups=groups)


# ---- cells ---------------------------------------------------------------------------------------------------------------------

CELLS_CASES = ["none", "duplicates_add", "duplicates_cancel", "mirror_given", "diagonal", "descending_columns", "cells_524288",
               "cells_524289", "one_cell_100000", "hub_row_4097"]


@functools.lru_cache(maxsize=None)
def cells_case(name):
    """(row, column, value) cells as ``vs_links_from_cells`` takes them; n = 97 but for the hub (4 097)."""
    n = 97
    rng = np.random.default_rng([6, CELLS_CASES.index(name)])
    facts = {}
    if name == "none":
        cells = []
    elif name == "duplicates_add":
        cells = [(3, 5, 7), (3, 5, 8), (5, 3, 9), (3, 5, -1), (96, 0, 2 ** 40), (96, 0, 2 ** 40), (0, 96, -3)]
    elif name == "duplicates_cancel":
        cells = [(3, 5, 7), (5, 3, -7), (4, 4, 9), (4, 4, -9), (10, 20, 5), (10, 20, -2), (20, 10, -3), (3, 6, 1), (10, 21, 4),
                 (60, 61, 2 ** 50), (60, 61, -2 ** 50), (96, 96, -1), (96, 96, 1)]
        facts["cancelled"] = [(3, 5), (4, 4), (10, 20), (60, 61), (96, 96)]
    elif name == "mirror_given":
        cells = [(8, 30, 11), (30, 8, 100), (30, 8, 1000), (0, 1, 2), (1, 0, 3)]
    elif name == "diagonal":
        cells = [(0, 0, 5), (96, 96, -6), (40, 40, 1), (40, 40, 2), (40, 41, 3)]
    elif name == "descending_columns":
        cells = [(50, c, c + 1) for c in range(96, -1, -1)] + [(r, 2, -r - 1) for r in range(96, 50, -1)]
    elif name in ("cells_524288", "cells_524289"):
        k = int(name.split("_")[1])  # (the scatter's 2 048 workgroups of 256 take one cell each up to 524 288)
        cells = list(zip(rng.integers(0, n, k).tolist(), rng.integers(0, n, k).tolist(), rng.integers(-2 ** 30, 2 ** 30, k).tolist()))
        cells[-1] = (96, 95, 2 ** 45)  # (the last cell, the one a second turn of the loop takes, is seen in the table)
    elif name == "one_cell_100000":
        cells = [(11, 80, v) for v in rng.integers(-2 ** 30, 2 ** 30, 100000).tolist()] + [(80, 12, 1)]
    elif name == "hub_row_4097":
        n = 4097
        H = 2048
        facts["hub"] = H
        cells = [(H, c, v) for c, v in zip(rng.integers(0, n, 120000).tolist(), rng.integers(-1000, 1000, 120000).tolist()) if c != H]
        cells += [(H, H, v) for v in rng.integers(-1000, 1000, 100000).tolist()]
        cells += list(zip(rng.integers(0, n, 5000).tolist(), rng.integers(0, n, 5000).tolist(), rng.integers(-1000, 1000, 5000).tolist()))
        cells.append((n - 1, 0, 4))
    rows = np.asarray([c[0] for c in cells], dtype=np.uint32)
    cols = np.asarray([c[1] for c in cells], dtype=np.uint32)
    vals = np.asarray([c[2] for c in cells], dtype=np.int64)
    _freeze(rows, cols, vals)
    queries = random_queries(rng, n, 30, 5, 130) + [(list(range(0, n, 7)), list(range(n)))]
    if name == "hub_row_4097":
        queries += [([facts["hub"]], list(range(n))), (list(range(n)), [facts["hub"]])]
    return _case(id="cells_" + name, n=n, rows=rows, cols=cols, vals=vals, facts=facts, model=LinksModel(n, cells), queries=queries,
                 groups=group_sets(rng, n)[2:])


def cells_as_matrices(case):
    """The dense matrices m[r][c] += v the cells stand for (node; short stays zero)."""
    node = np.zeros((case.n, case.n), dtype=np.int64)
    np.add.at(node, (case.rows.astype(np.int64), case.cols.astype(np.int64)), case.vals)
    return node, np.zeros_like(node)


def matrices_as_cells(node, short):
    """The non-zero cells of both matrices, node's first: (rows uint32, cols uint32, vals int64)."""
    r0, c0 = np.nonzero(node)
    r1, c1 = np.nonzero(short)
    return (np.concatenate([r0, r1]).astype(np.uint32), np.concatenate([c0, c1]).astype(np.uint32),
            np.concatenate([node[r0, c0], short[r1, c1]]).astype(np.int64))


def small_cases():
    """(id, thunk) of every case of at most 322 nodes together with the two matrices it stands for."""
    out = []
    for n in DENSE_SIZES:
        for wide in (False, True):
            out.append(("dense_n%d_%s" % (n, "int64" if wide else "uint32"), functools.partial(dense_case, n, wide)))
    for n in GROUP_SIZES:
        out.append(("groups_n%d" % n, functools.partial(group_case, n)))
    for n, rot in TILE_MIX_CASES:
        out.append(("tiles_n%d_rot%d" % (n, rot), functools.partial(tile_mix_case, n, rot)))
    out.append(("lists_n322", lists_case))
    for name in CELLS_CASES:
        if name != "hub_row_4097":
            out.append(("cells_" + name, functools.partial(cells_case, name)))
    return out


def matrices_of(case):
    return (case.node, case.short) if hasattr(case, "node") else cells_as_matrices(case)
