"""The plain model of the PE-link table (links_model.py) against the literal dict of the reference (oracle.graph_ops.DictPeLinks,
process_pe_info, IO.py:598-627), and the constructed cases (links_cases.py) against what they claim to be: a case that lost
its edge -- a subset that never meets the partial tile, a table without an empty row, a hub row that is no hub -- fails
here, on any machine.  Everything is integer: every assertion is equality."""
import numpy as np
import pytest

import links_cases as lc
from links_model import LinksModel
from oracle import graph_ops as chk

SMALL = lc.small_cases()


@pytest.mark.parametrize("make", [m for _, m in SMALL], ids=[i for i, _ in SMALL])
def test_model_equals_the_literal_dict(make):
    case = make()
    n, model = case.n, case.model
    node, short = lc.matrices_of(case)
    names = ["%03d" % i for i in range(n)]
    ref = chk.DictPeLinks(names, node.tolist(), short.tolist())
    p0 = model.dense()
    want = np.array([[ref.table[(names[min(i, j)], names[max(i, j)])] for j in range(n)] for i in range(n)], dtype=np.int64).reshape(n, n)
    assert np.array_equal(p0, want)
    assert np.array_equal(p0, p0.T)
    got = model.block_sums(case.queries)
    assert all(lc.fits_int64(s) for s in got)
    assert got == ref.block_sums(case.queries)
    # the model's CSR rows: strictly ascending columns, no zeros, and the same answers from the checker's CSR table
    row_ptr, col, val = model.csr()
    assert row_ptr[0] == 0 and row_ptr[n] == col.size == val.size == np.count_nonzero(p0)
    for r in range(n):
        c = col[row_ptr[r]:row_ptr[r + 1]].astype(np.int64)
        assert np.all(np.diff(c) > 0)
        assert np.array_equal(c, np.flatnonzero(p0[r]))
        assert np.array_equal(val[row_ptr[r]:row_ptr[r + 1]], p0[r][c])
    assert chk.SparsePeLinks(names, row_ptr, col, val).block_sums(case.queries) == got
    for groups in case.groups:
        gm = model.group_matrix(groups)
        assert all(lc.fits_int64(s) for row in gm for s in row)
        assert np.array_equal(np.array(gm, dtype=np.int64).reshape(len(groups), len(groups)), ref.group_matrix(groups))


def test_model_from_cells_equals_model_from_the_matrices_they_add_up_to():
    for name in lc.CELLS_CASES[:-1]:
        case = lc.cells_case(name)
        node, short = lc.cells_as_matrices(case)
        assert LinksModel.from_matrices(node, short).rows == case.model.rows, name


@pytest.mark.parametrize("n", lc.DENSE_SIZES)
def test_dense_cases_hold_their_edge_values(n):
    u, w = lc.dense_case(n, False), lc.dense_case(n, True)
    d = n - 1
    assert u.node.min() >= 0 and u.short.min() >= 0 and max(u.node.max(), u.short.max()) == 2 ** 32 - 1
    assert {int(u.node[d, d]), int(u.short[d, d])} == {2 ** 32 - 1, 2 ** 31}
    assert max(abs(int(w.node.min())), int(w.node.max())) == lc.BIG < 2 ** 61
    if n > 1:
        assert w.node.min() == -lc.BIG
        assert {int(u.node[0, d]), int(u.node[d, 0])} == {2 ** 32 - 1, 2 ** 31} == {int(u.short[0, d]), int(u.short[d, 0])}
        assert w.short.min() < 0
    if n > 2:
        for c in (u, w):  # asymmetric: a transposed read of either matrix gives another table
            assert not np.array_equal(c.node, c.node.T) and not np.array_equal(c.short, c.short.T)
            assert LinksModel.from_matrices(c.node.T, c.short).rows == c.model.rows  # (the table itself is symmetric in that)
            assert not np.array_equal(c.node + c.short, c.model.dense())


def test_every_subset_of_source_tiles_meets_the_partial_last_tile():
    on_partial, on_full, diag_partial = set(), set(), set()
    for rot in range(3):
        case = lc.tile_mix_case(322, rot)
        T = case.T
        assert T == 6 and 322 - 5 * 64 == 2
        assert sorted(case.subsets.values()) == list(range(1, 16))  # 15 pairs, 15 different non-empty subsets
        for (I, J), mask in case.subsets.items():
            (on_partial if J == T - 1 else on_full).add(mask)
            assert [int(case.marks[0, I, J]), int(case.marks[0, J, I]), int(case.marks[1, I, J]), int(case.marks[1, J, I])] == \
                [mask & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1]
        assert set(case.diagonal.values()) == {"node", "short", "both"}
        diag_partial.add(case.diagonal[T - 1])
    assert on_partial == set(range(1, 16)) and on_full == set(range(1, 16))
    assert diag_partial == {"node", "short", "both"}


@pytest.mark.parametrize("n,rot", lc.TILE_MIX_CASES)
def test_tile_mix_cases_are_what_they_say(n, rot):
    case = lc.tile_mix_case(n, rot)
    T = case.T
    for m, (clean, dirty) in enumerate(((case.node, case.dirty_node), (case.short, case.dirty_short))):
        for I in range(T):
            for J in range(T):
                t, g = lc._tile(clean, I, J), lc._tile(dirty, I, J)
                if case.marks[m, I, J]:
                    assert np.array_equal(t, g)
                else:
                    assert not t.any() and np.all(g == lc.GARBAGE)
    m, I, J = case.full
    assert case.marks[m, I, J] and np.all(lc._tile((case.node, case.short)[m], I, J) != 0)
    assert lc._tile(case.node, I, J).shape == (64, 64)  # 64 rows of the table with a full piece of 64 cells, and their mirrors
    p0 = case.model.dense()
    assert np.all(lc._tile(p0, I, J) != 0) and np.all(lc._tile(p0, J, I) != 0)
    m, I, J = case.zero
    assert case.marks[m, I, J] and not lc._tile((case.node, case.short)[m], I, J).any() and case.zero != case.full
    _, _, val = case.model.csr()
    assert lc.GARBAGE not in set(val.tolist()) and not np.any(case.model.dense() == lc.GARBAGE)
    assert (case.marks == 0).any() or n == 64
    if n == 64:
        assert T == 1 and np.all(case.model.dense() != 0)  # one diagonal tile, every piece full
    if n == 65:
        assert T == 2 and case.subsets == {(0, 1): 6}  # a last tile of one row, fed by node (J,I) and short (I,J)


def test_lists_case_has_its_rows_and_list_lengths():
    case = lc.lists_case()
    n, model = case.n, case.model
    lengths = model.row_lengths()
    for r in case.EMPTY:
        assert lengths[r] == 0
    assert lengths[case.SINGLE] == 1 and model.cell(case.SINGLE, case.SINGLE_COL) == 5
    row_ptr, col, _ = model.csr()
    narrow = col[row_ptr[case.NARROW]:row_ptr[case.NARROW + 1]]
    assert narrow[0] == 100 and narrow[-1] == 200 and narrow.size > 2
    assert {len(c) for _, c in case.named.values()} >= set(lc.COL_LIST_LENGTHS) | {2 * n}
    assert {len(r) for r, _ in case.named.values()} >= set(lc.ROW_LIST_LENGTHS)
    for rl in lc.ROW_LIST_LENGTHS:
        for cl in lc.COL_LIST_LENGTHS + [2 * n]:
            rows, cols = case.named["rows%d_cols%d" % (rl, cl)]
            assert (len(rows), len(cols)) == (rl, cl)
    assert len(set(case.named["rows65_cols%d" % (2 * n)][1])) < 2 * n  # the 2 n list has repeats
    assert case.named["same_list_both_sides"][0] is case.named["same_list_both_sides"][1]
    assert set(case.named["only_empty_rows"][0]) == set(case.EMPTY)
    assert model.block_sum(*case.named["equal_first"]) == 3 and model.block_sum(*case.named["equal_last"]) == 9
    assert model.block_sum(*case.named["first_and_last"]) == 24
    assert model.block_sum(*case.named["single_cell_repeated"]) == 64 * 65 * 5
    assert sorted(case.by_count) == lc.QUERY_COUNTS and all(len(q) == k for k, q in case.by_count.items())
    assert (case.marks == 0).any()
    for groups in case.groups:
        assert any(len(g) == 0 for g in groups) or len(groups) == 1
    assert sorted(len(g) for g in case.groups) == [1, 2, 7]


@pytest.mark.parametrize("n", lc.GROUP_SIZES)
def test_group_cases_reach_the_last_column(n):
    case = lc.group_case(n)
    assert case.model.cell(0, n - 1) and case.model.cell(n - 1, n - 2) and case.model.cell(n - 1, n - 1)
    assert sorted(len(g) for g in case.groups)[:3] == [1, 2, 3]
    assert all(any(n - 1 in g for g in groups) for groups in case.groups)


@pytest.mark.parametrize("n,variant", lc.PIECES_CASES)
def test_pieces_cases_have_their_rows(n, variant):
    case = lc.pieces_case(n, variant)
    T, model = case.T, case.model
    assert T == (64 if n == 4096 else 65) and 2000 < case.n_cells < 10000
    lengths = model.row_lengths()
    row_ptr, col, val = model.csr()
    assert row_ptr[n] == sum(lengths) and lc.GARBAGE not in set(val.tolist())
    pieces = lambda r: sorted({c // 64 for c in model.rows.get(r, {})})
    stripe = sorted(model.rows[case.STRIPE])
    assert len(stripe) >= T and pieces(case.STRIPE) == list(range(T))
    own = [c for c in stripe if c != case.FULL or variant == "thin"]
    if variant == "thin":
        assert own == [t * 64 if t % 2 == 0 else min(t * 64 + 63, n - 1) for t in range(T)]
        assert 0 in lengths and 1 in lengths
        assert case.empty_rows and all(lengths[r] == 0 for r in case.empty_rows)
        assert lengths[case.ONLY_LAST] == 1 and pieces(case.ONLY_LAST) == [T - 1]
        assert pieces(case.CARRY) == [T - 2, T - 1]
        assert lengths[n - 1] >= 3
    else:
        assert lengths[case.FULL] == n and min(lengths) >= 1  # every piece of the row is full, the last one holds n - 64 (T - 1)
        assert n - 64 * (T - 1) == (1 if n == 4097 else 64)
        assert 1 in lengths or n == 4096
    if n == 4097:
        # the chunk carry of k_sl_rows: rows with a piece below tile column 64 and one in it
        both = [r for r in model.rows if pieces(r)[0] < 64 and pieces(r)[-1] == 64]
        assert both and (case.CARRY in both or variant == "full")
        assert pieces(n - 1) and 64 * 64 == n - 1  # row 4096 is the lone row of the last tile row, and it holds cells
        if variant == "full":
            ones = [r for r in range(n) if lengths[r] == 1]
            assert ones and all(pieces(r) == [1] for r in ones)
    assert all(lc.fits_int64(s) for s in model.block_sums(case.queries))


def test_cells_cases_have_their_cells():
    none = lc.cells_case("none")
    assert none.rows.size == 0 and none.model.rows == {}
    add = lc.cells_case("duplicates_add").model
    assert add.cell(3, 5) == add.cell(5, 3) == 23 and add.cell(0, 96) == 2 ** 41 - 3
    cancel = lc.cells_case("duplicates_cancel")
    for r, c in cancel.facts["cancelled"]:
        assert cancel.model.keys[(r, c)] == 0 and c not in cancel.model.rows.get(r, {}) and r not in cancel.model.rows.get(c, {})
    assert cancel.model.rows[3] == {6: 1} and cancel.model.rows[10] == {21: 4} and 4 not in cancel.model.rows
    assert lc.cells_case("mirror_given").model.cell(8, 30) == 1111
    diag = lc.cells_case("diagonal").model
    assert (diag.cell(0, 0), diag.cell(96, 96), diag.cell(40, 40), diag.cell(41, 40)) == (5, -6, 3, 3)
    desc = lc.cells_case("descending_columns")
    assert np.all(np.diff(desc.cols[:97].astype(np.int64)) == -1) and len(desc.model.rows[50]) == 97
    for k in (524288, 524289):
        case = lc.cells_case("cells_%d" % k)
        assert case.rows.size == k == 2048 * 256 + (k - 524288) and (case.rows[-1], case.cols[-1]) == (96, 95)
        assert abs(case.model.cell(96, 95)) > 2 ** 44
    one = lc.cells_case("one_cell_100000")
    assert np.count_nonzero((one.rows == 11) & (one.cols == 80)) == 100000 and one.model.cell(80, 11) == int(one.vals[:100000].sum())
    hub = lc.cells_case("hub_row_4097")
    H = hub.facts["hub"]
    diag = hub.rows == hub.cols
    entries = int(np.count_nonzero(diag) + 2 * np.count_nonzero(~diag))
    in_hub = int(np.count_nonzero((hub.rows == H) | (hub.cols == H)))
    assert hub.n == 4097 and entries >= 300000 and entries >= 131072 and 2 * in_hub > entries
    assert len(hub.model.rows[H]) > 4000
