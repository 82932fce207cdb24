"""The PE-link table kernels (K5, vs_graph.hip) called through the C ABI on the constructed cases of links_cases.py and
compared, cell for cell and sum for sum, with the plain model of links_model.py (process_pe_info, IO.py:598-627).

What is compared: a dense table's cells (vs_links_to_host); a CSR table's rows as the device holds them
(vs_links_export_csr: row_ptr, columns strictly ascending, no stored zero, row_ptr[n] == nnz), and its cells as well up
to 322 nodes; block sums and group matrices of either form.  The table holds integers: every assertion is equality.
test_links_model_cpu.py checks, without a GPU, that the model is the reference's dict and that every case holds the edge it
is named after."""
import ctypes as C
import time

import numpy as np
import pytest

import links_cases as lc

pytestmark = pytest.mark.gpu

DENSE_ONLY = 10 ** 6  # a sparse_min_nodes no case reaches
CSR_FROM = 64


@pytest.fixture(scope="module")
def ctx():
    from vstrains_amd import pe as host

    return host.Context(0)


# ---- builders: every way the library makes a table ------------------------------------------------------------------------

def _wrap(ctx, h, n):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ctx.sync()
    return HipPeLinks(ctx, h, [str(i) for i in range(n)])


def _device(arrays, dtype):
    import torch

    a = np.stack(arrays)
    a = a.astype(np.uint32).view(np.int32) if dtype == "uint32" else a.astype(np.int64)
    t = torch.from_numpy(a).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


def from_counts(ctx, node, short):
    from vstrains_amd import _native as nat

    n, mats, h = node.shape[0], _device([node, short], "uint32"), C.c_void_p()
    nat.check(ctx._h, nat.lib().vs_links_from_counts(ctx._h, C.c_void_p(mats[0].data_ptr()), C.c_void_p(mats[1].data_ptr()), n, C.byref(h)))
    return _wrap(ctx, h, n)


def from_tracked_device(ctx, mats, marks, n, sparse_min_nodes):
    import torch

    from vstrains_amd import _native as nat

    tile_map = torch.from_numpy(np.ascontiguousarray(marks).reshape(-1).copy()).to(mats.device)
    torch.cuda.synchronize()
    h = C.c_void_p()
    nat.check(ctx._h, nat.lib().vs_links_from_counts_tracked(ctx._h, C.c_void_p(mats[0].data_ptr()), C.c_void_p(mats[1].data_ptr()), n,
                                                             C.c_void_p(tile_map.data_ptr()), sparse_min_nodes, C.byref(h)))
    return _wrap(ctx, h, n)


def from_tracked(ctx, node, short, marks, sparse_min_nodes):
    return from_tracked_device(ctx, _device([node, short], "uint32"), marks, node.shape[0], sparse_min_nodes)


def from_wide(ctx, node, short):
    from vstrains_amd import _native as nat

    n, mats, h = node.shape[0], _device([node, short], "int64"), C.c_void_p()
    nat.check(ctx._h, nat.lib().vs_links_from_wide(ctx._h, C.c_void_p(mats[0].data_ptr()), C.c_void_p(mats[1].data_ptr()), n, C.byref(h)))
    return _wrap(ctx, h, n)


def from_host(ctx, node, short):
    from vstrains_amd import _native as nat

    n, h = node.shape[0], C.c_void_p()
    a, b = np.ascontiguousarray(node, dtype=np.int64), np.ascontiguousarray(short, dtype=np.int64)
    nat.check(ctx._h, nat.lib().vs_links_from_host(ctx._h, a.ctypes.data, b.ctypes.data, n, C.byref(h)))
    return _wrap(ctx, h, n)


def cells_call(ctx, rows, cols, vals, n, sparse_min_nodes):
    from vstrains_amd import _native as nat

    p = lambda a: a.ctypes.data if a.size else None
    h = C.c_void_p()
    rc = nat.lib().vs_links_from_cells(ctx._h, p(rows), p(cols), p(vals), rows.size, n, sparse_min_nodes, C.byref(h))
    return rc, h


def from_cells(ctx, rows, cols, vals, n, sparse_min_nodes):
    from vstrains_amd import _native as nat

    rc, h = cells_call(ctx, rows, cols, vals, n, sparse_min_nodes)
    nat.check(ctx._h, rc)
    return _wrap(ctx, h, n)


# ---- asking a table -------------------------------------------------------------------------------------------------------

def pool(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    flat = np.asarray([x for l in lists for x in l], dtype=np.uint32)
    return off, flat


def block_sums_call(table, lists, qa, qb, off=None):
    """vs_links_block_sums as it is: (return code, out)."""
    from vstrains_amd import _native as nat

    off0, flat = pool(lists)
    off = off0 if off is None else off
    qa, qb = np.asarray(qa, dtype=np.uint32), np.asarray(qb, dtype=np.uint32)
    out = np.full(max(len(qa), 1), -12345, dtype=np.int64)
    rc = nat.lib().vs_links_block_sums(table.ctx._h, table._h, off.ctypes.data, flat.ctypes.data if flat.size else None, len(lists),
                                       qa.ctypes.data, qb.ctypes.data, len(qa), out.ctypes.data)
    return rc, out[:len(qa)].tolist()


def block_sums(table, queries):
    """One call for all queries; a query whose two lists are one object names one list twice."""
    from vstrains_amd import _native as nat

    lists, qa, qb = [], [], []
    for rows, cols in queries:
        qa.append(len(lists))
        lists.append(rows)
        if cols is rows:
            qb.append(qa[-1])
        else:
            qb.append(len(lists))
            lists.append(cols)
    rc, out = block_sums_call(table, lists, qa, qb)
    nat.check(table.ctx._h, rc)
    return out


def group_matrix_call(table, groups, off=None):
    from vstrains_amd import _native as nat

    off0, flat = pool(groups)
    off = off0 if off is None else off
    g = len(groups)
    out = np.full((g, g), -12345, dtype=np.int64)
    rc = nat.lib().vs_links_group_matrix(table.ctx._h, table._h, off.ctypes.data, flat.ctypes.data if flat.size else None, g, out.ctypes.data)
    return rc, out


def last_error(ctx):
    from vstrains_amd import _native as nat

    return (nat.lib().vs_last_error(ctx._h) or b"").decode()


def check_answers(table, case):
    got, want = block_sums(table, case.queries), case.model.block_sums(case.queries)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s: block sum %d of %d: %d, expected %d (rows %s..., %d columns)" % (
        case.id, bad[0], len(want), got[bad[0]], want[bad[0]], case.queries[bad[0]][0][:4], len(case.queries[bad[0]][1]))
    for groups in case.groups:
        rc, gm = group_matrix_call(table, groups)
        assert rc == 0, last_error(table.ctx)
        assert gm.tolist() == case.model.group_matrix(groups), "%s: group matrix of %d groups" % (case.id, len(groups))


def check_table(table, case, csr):
    """The table against the model of its case: the stored form, the cells, and every answer."""
    from vstrains_amd import _native as nat

    n, model = case.n, case.model
    if csr:
        row_ptr, col, val, nnz = table.csr()
        want_ptr, want_col, want_val = model.csr()
        assert nnz == int(row_ptr[n]) == want_col.size, "%s: nnz %d, row_ptr[n] %d, expected %d" % (case.id, nnz, row_ptr[n], want_col.size)
        assert np.array_equal(row_ptr, want_ptr), "%s: row_ptr differs first at row %d" % (case.id, np.flatnonzero(row_ptr != want_ptr)[0] - 1)
        assert np.array_equal(col, want_col), "%s: columns differ first at stored cell %d" % (case.id, np.flatnonzero(col != want_col)[0])
        assert np.array_equal(val, want_val), "%s: values differ first at stored cell %d" % (case.id, np.flatnonzero(val != want_val)[0])
        assert lc.GARBAGE not in set(val.tolist())
    else:
        with pytest.raises(nat.NativeError) as ei:
            table.csr()
        assert ei.value.code == nat.VS_E_ARG and "dense" in str(ei.value)
    if n <= 322:
        got, want = table.to_numpy(), model.dense()
        assert got.shape == want.shape
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d cells differ, first P0[%d][%d] = %d, expected %d" % (
            case.id, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
    check_answers(table, case)


# ---- dense build ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["counts", "wide", "host"])
@pytest.mark.parametrize("n", lc.DENSE_SIZES)
def test_dense_table_at_the_symmetrize_tile_edges(ctx, n, form):
    """k_links_symmetrize (tiles of 32 x 32, tile pairs (I, J) and (J, I) through LDS), both instantiations."""
    if form == "counts":
        case = lc.dense_case(n, False)
        check_table(from_counts(ctx, case.node, case.short), case, csr=False)
        return
    build = from_wide if form == "wide" else from_host
    for wide in (True, False):  # int64 of either sign, and the uint32 range held as int64
        case = lc.dense_case(n, wide)
        check_table(build(ctx, case.node, case.short), case, csr=False)


@pytest.mark.parametrize("n", lc.GROUP_SIZES)
def test_dense_group_matrix_at_its_column_guard(ctx, n):
    """k_links_group_rows takes 256 columns per workgroup: n = 255, 256, 257."""
    case = lc.group_case(n)
    check_table(from_counts(ctx, case.node, case.short), case, csr=False)


# ---- source-tile mixes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,rot", lc.TILE_MIX_CASES, ids=["n%d_rot%d" % c for c in lc.TILE_MIX_CASES])
def test_csr_table_from_every_mix_of_marked_source_tiles(ctx, n, rot):
    """sl_load_pair: each of the 15 non-empty subsets of {node (I,J), node (J,I), short (I,J), short (J,I)} on full tiles and
    on pairs with the partial last tile, the diagonal tiles with node, short or both; unmarked tiles hold garbage."""
    case = lc.tile_mix_case(n, rot)
    check_table(from_tracked(ctx, case.dirty_node, case.dirty_short, case.marks, CSR_FROM), case, csr=True)
    # below the threshold the same entry point gives the dense table of the counters as they are: the clean ones here
    check_table(from_tracked(ctx, case.node, case.short, case.marks, DENSE_ONLY), case, csr=False)


# ---- pieces and chunks ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,variant", lc.PIECES_CASES, ids=["n%d_%s" % c for c in lc.PIECES_CASES])
def test_csr_table_of_64_and_65_tile_columns(ctx, n, variant):
    """k_sl_count / k_sl_rows / k_sl_fill at T = 64 and T = 65: full pieces, a row of n cells, single cells at piece edges,
    the carry of k_sl_rows from its first chunk of 64 tile columns into the second.  The counters are zeros plus the
    case's cells, put together on the device."""
    import torch

    case = lc.pieces_case(n, variant)
    t0 = time.perf_counter()
    dev = torch.device("cuda:0")
    mats = torch.zeros((2, n, n), dtype=torch.int32, device=dev)
    for m, (r, c, v) in enumerate((case.node_cells, case.short_cells)):
        mats[m].view(-1)[torch.from_numpy(r * n + c).to(dev)] = torch.from_numpy(v.astype(np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    table = from_tracked_device(ctx, mats, case.marks, n, CSR_FROM)
    t1 = time.perf_counter()
    check_table(table, case, csr=True)
    print("%s: counters and table %.2f s, export and answers %.2f s" % (case.id, t1 - t0, time.perf_counter() - t1))


# ---- lists ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lists_tables(ctx):
    case = lc.lists_case()
    return {"dense": from_counts(ctx, case.node, case.short),
            "csr": from_tracked(ctx, case.dirty_node, case.dirty_short, case.marks, CSR_FROM)}


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_row_and_column_lists_at_the_wavefront_edges(lists_tables, form):
    """k_links_block_sums / k_links_block_sums_csr: column lists of 0 .. 129 and 2 n entries against row lists of 0 .. 65,
    one index repeated, one list on both sides, and -- what only the CSR rows can get wrong -- empty rows, a row of one
    stored cell, columns below the first stored one, above the last, equal to either."""
    case, table = lc.lists_case(), lists_tables[form]
    check_table(table, case, csr=form == "csr")
    names = list(case.named)
    want = [case.model.block_sum(*case.named[k]) for k in names]
    got = block_sums(table, [case.named[k] for k in names])
    assert not [(k, g, w) for k, g, w in zip(names, got, want) if g != w]
    alone = [block_sums(table, [case.named[k]])[0] for k in names]  # every query again as the only one of its launch
    assert not [(k, g, w) for k, g, w in zip(names, alone, want) if g != w]


@pytest.mark.parametrize("count", lc.QUERY_COUNTS)
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_query_counts_that_do_not_fill_the_last_workgroup(lists_tables, form, count):
    """Four wavefronts, one query each, per workgroup: 1, 3, 4, 5 and 1 025 queries."""
    case = lc.lists_case()
    queries = case.by_count[count]
    assert block_sums(lists_tables[form], queries) == case.model.block_sums(queries)


def test_one_table_built_seven_ways(ctx, lists_tables):
    case = lc.lists_case()
    n, node, short = case.n, case.node, case.short
    rows, cols, vals = lc.matrices_as_cells(node, short)
    tables = {"counts": (lists_tables["dense"], False),
              "tracked_dense": (from_tracked(ctx, node, short, case.marks, DENSE_ONLY), False),
              "tracked_csr": (lists_tables["csr"], True),
              "wide": (from_wide(ctx, node, short), False),
              "host": (from_host(ctx, node, short), False),
              "cells_dense": (from_cells(ctx, rows, cols, vals, n, DENSE_ONLY), False),
              "cells_csr": (from_cells(ctx, rows, cols, vals, n, CSR_FROM), True)}
    queries = case.queries + case.by_count[5]
    first = None
    for name, (table, csr) in tables.items():
        check_table(table, case, csr=csr)
        answer = (table.to_numpy().tolist(), block_sums(table, queries), [group_matrix_call(table, g)[1].tolist() for g in case.groups])
        if first is None:
            first = answer
        assert answer == first, name
    a, b = tables["tracked_csr"][0].csr(), tables["cells_csr"][0].csr()
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


# ---- cells ------------------------------------------------------------------------------------------------------------------

# (the table of 4 097 nodes is a CSR case: no dense table of that size is built and read back)
CELLS_RUNS = [(name, form) for name in lc.CELLS_CASES for form in ("dense", "csr") if (name, form) != ("hub_row_4097", "dense")]


@pytest.mark.parametrize("name,form", CELLS_RUNS, ids=["%s_%s" % r for r in CELLS_RUNS])
def test_table_from_cells(ctx, name, form):
    """k_links_scatter (a grid of at most 2 048 x 256 threads: 524 288 cells in one turn, 524 289 in two; 100 000 adds on one
    cell) and the host's CSR merge (mirrors, duplicates, sums of zero dropped, rows dealt to threads by entry count from
    131 072 entries on, one row holding most of them)."""
    case = lc.cells_case(name)
    t0 = time.perf_counter()
    table = from_cells(ctx, case.rows, case.cols, case.vals, case.n, DENSE_ONLY if form == "dense" else CSR_FROM)
    check_table(table, case, csr=form == "csr")
    if case.n > 322:
        print("%s: %.2f s" % (case.id, time.perf_counter() - t0))


# ---- refusals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "csr"])
def test_bad_lists_are_refused_and_the_next_call_is_right(ctx, lists_tables, form):
    """Host-side argument checks (nothing is launched): the code, the message, and the context is as good as before."""
    from vstrains_amd import _native as nat

    case, table = lc.lists_case(), lists_tables[form]
    n = case.n
    good = case.by_count[5]

    def still_right():
        assert block_sums(table, good) == case.model.block_sums(good)
        rc, gm = group_matrix_call(table, case.groups[1])
        assert rc == 0 and gm.tolist() == case.model.group_matrix(case.groups[1])

    rc, _ = block_sums_call(table, [[0, 1], [2, n]], [0], [1])
    assert rc == nat.VS_E_RANGE and last_error(ctx) == "list index %d out of range (n=%d)" % (n, n)
    still_right()
    rc, _ = group_matrix_call(table, [[0], [n, 1]])
    assert rc == nat.VS_E_RANGE and last_error(ctx) == "list index %d out of range (n=%d)" % (n, n)
    still_right()
    rc, _ = block_sums_call(table, [[0, 1], [2, 3]], [0], [1], off=np.asarray([0, 3, 2], dtype=np.uint64))
    assert rc == nat.VS_E_ARG and last_error(ctx) == "list offsets must not decrease"
    still_right()
    rc, _ = group_matrix_call(table, [[0, 1], [2, 3]], off=np.asarray([0, 3, 2], dtype=np.uint64))
    assert rc == nat.VS_E_ARG and last_error(ctx) == "list offsets must not decrease"
    still_right()
    for qa, qb, q in (([0, 2], [1, 1], 1), ([0], [2], 0), ([0, 1, 0xFFFFFFFF], [0, 1, 1], 2)):
        rc, _ = block_sums_call(table, [[0, 1], [2, 3]], qa, qb)
        assert rc == nat.VS_E_RANGE and last_error(ctx) == "query %d names a list out of range" % q
        still_right()


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_a_cell_outside_the_table_is_refused(ctx, form):
    from vstrains_amd import _native as nat

    n = 97
    rows = np.asarray([1, 2, n, 4], dtype=np.uint32)
    cols = np.asarray([5, 6, 7, 8], dtype=np.uint32)
    vals = np.asarray([1, 2, 3, 4], dtype=np.int64)
    min_nodes = DENSE_ONLY if form == "dense" else CSR_FROM
    rc, h = cells_call(ctx, rows, cols, vals, n, min_nodes)
    assert rc == nat.VS_E_RANGE and not h.value
    assert last_error(ctx) == "vs_links_from_cells: cell 2 (%d, 7) outside %d nodes" % (n, n)
    rc, h = cells_call(ctx, cols, rows[::-1].copy(), vals, n, min_nodes)
    assert rc == nat.VS_E_RANGE and not h.value
    assert last_error(ctx) == "vs_links_from_cells: cell 1 (6, %d) outside %d nodes" % (n, n)
    case = lc.cells_case("duplicates_add")
    check_table(from_cells(ctx, case.rows, case.cols, case.vals, case.n, min_nodes), case, csr=form == "csr")


def test_csr_export_says_what_it_cannot_give(ctx, lists_tables):
    """vs_links_export_csr: a dense table has no rows to show; a buffer shorter than nnz gets nothing but the count."""
    from vstrains_amd import _native as nat

    L, h = nat.lib(), ctx._h
    nnz = C.c_uint64(7)
    assert L.vs_links_export_csr(h, lists_tables["dense"]._h, None, None, None, 0, C.byref(nnz)) == nat.VS_E_ARG
    assert last_error(ctx) == "vs_links_export_csr: the table of 322 nodes is dense" and nnz.value == 7
    table = lists_tables["csr"]
    want_ptr, want_col, want_val = lc.lists_case().model.csr()
    col = np.full(want_col.size, 0xABCDABCD, dtype=np.uint32)
    val = np.full(want_col.size, -7, dtype=np.int64)
    assert L.vs_links_export_csr(h, table._h, None, col.ctypes.data, val.ctypes.data, want_col.size - 1, C.byref(nnz)) == nat.VS_E_RANGE
    assert nnz.value == want_col.size and np.all(col == 0xABCDABCD) and np.all(val == -7)
    assert last_error(ctx) == "vs_links_export_csr: %d stored cells, room for %d" % (want_col.size, want_col.size - 1)
    assert L.vs_links_export_csr(h, table._h, None, col.ctypes.data, None, want_col.size, None) == nat.VS_E_ARG
    row_ptr = np.zeros(323, dtype=np.uint32)
    assert L.vs_links_export_csr(h, table._h, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, want_col.size, None) == 0
    assert np.array_equal(row_ptr, want_ptr) and np.array_equal(col, want_col) and np.array_equal(val, want_val)
