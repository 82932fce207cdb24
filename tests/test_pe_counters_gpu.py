"""The counter kernels of a PE count (vstrains_amd/csrc/vs_pe.hip, K4: k_mark_tiles, k_pe_accumulate, k_list_owners ..
k_rows_sum) run alone on constructed per-end node lists (vs_pe_count_lists) and compared with the plain statement of
PE_Inference.py:174-188 (pe_counter_model.py), and the locus order in front of the mapping kernel, observed
(vs_pe_last_order).  The lists are the ones reads never produce: every length pair, unordered, colliding in the cell
tables and the list table, wider than a strip's table, spread over more tiles than k_mark_tiles keeps in registers, at
the edges of the 32-bit cell keys.  Every comparison is exact: the model's cells are fetched and compared, the sum of each
whole matrix equals the model's total (counters never go down, so no stray cell), and the tile map equals the model's
tile set.  Every run starts from counters that already hold values (some >= 2^31) and counts the block twice."""
import numpy as np
import pytest

import pe_counter_cases as cases
import pe_counter_model as pcm
import seed_extend_model as sem

pytestmark = pytest.mark.gpu

PREFILL = [1, 0x7FFFFFFF, 0x80000000, 0xF0000000, 12345]


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def xctx(host):
    """A context in experiment mode: the tuning switches of a count are live on it (conftest.experiment_context)."""
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


# the witnesses of a case: what a production context picks, the row owners, plain atomics; and, where production picks the
# row owners by itself or a case is about k_pe_accumulate's table, that table forced
MODES = {"production": None, "rows": {"VS_ACC_ROWS": "1"}, "noagg": {"VS_NO_AGG": "1"}, "table": {"VS_ACC_ROWS": "0"}}
_models = {}


def _model(key, n_nodes, lists, counts):
    """The model of a block, computed once per (case, tile size) and shared by every run of it (never changed)."""
    if key not in _models:
        node, short = pcm.count_block(lists, counts, n_nodes)
        _models[key] = (node, short, pcm.tiles_of(node[0], n_nodes), pcm.tiles_of(short[0], n_nodes))
    return _models[key]


def _usum(t):
    """Sum of a counter buffer read as uint32, in slices (a Python int)."""
    import torch

    total, step = 0, 1 << 27
    for lo in range(0, t.numel(), step):
        total += int((t[lo: lo + step].to(torch.int64) & 0xFFFFFFFF).sum().item())
    return total


def _fetch(t, cells):
    import torch

    if cells.size == 0:
        return np.zeros(0, dtype=np.int64)
    return t[torch.from_numpy(cells).to(t.device)].cpu().numpy().view(np.uint32).astype(np.int64)


def _count_and_compare(monkeypatch, ctx, xctx, case, key, mode, extra=None, tile_map=True, reps=2, then_zero=False, expect_rows=None):
    """Count ``case`` ``reps`` times into prefilled counters on the context of ``mode`` and compare with the model."""
    import ctypes as C

    import torch

    from vstrains_amd import _native as nat

    env = dict(MODES[mode] or {})
    env.update(extra or {})
    c = ctx if mode == "production" else xctx
    assert mode != "production" or not extra
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ept = c.lists_ept
    assert ept == int(env.get("VS_EPT", 64))
    n_nodes, lists, counts = cases.block(case, ept)
    (ncell, nval), (scell, sval), ntiles, stiles = _model((key, ept), n_nodes, lists, counts)
    dev = torch.device("cuda:%d" % c.device)
    N, T = n_nodes, (n_nodes + 63) // 64
    mats = [torch.zeros(N * N, dtype=torch.int32, device=dev) for _ in range(2)]
    tmap = torch.zeros(2 * T * T, dtype=torch.uint8, device=dev) if tile_map else None
    assert mats[0].data_ptr() % 64 == 0 and mats[1].data_ptr() % 64 == 0  # (what the cases' strip keys take for granted)
    # counters that already hold something: a few of the block's cells and a few it does not touch
    rng = np.random.default_rng(len(key) + n_nodes)
    want = []
    for m, (cells, vals) in enumerate(((ncell, nval), (scell, sval))):
        mine = rng.choice(cells, size=min(5, cells.size), replace=False) if cells.size else np.zeros(0, dtype=np.int64)
        other = np.setdiff1d(np.unique(rng.integers(0, N * N, size=12)), cells)[:5]
        pre_cells = np.concatenate([mine, other]).astype(np.int64)
        pre_vals = np.array([PREFILL[i % 5] for i in range(pre_cells.size)], dtype=np.int64)
        if pre_cells.size:
            mats[m][torch.from_numpy(pre_cells).to(dev)] = torch.from_numpy(pre_vals.astype(np.uint32).view(np.int32)).to(dev)
        all_cells = np.union1d(cells, pre_cells)
        exp = np.zeros(all_cells.size, dtype=np.int64)
        exp[np.searchsorted(all_cells, cells)] += reps * vals
        exp[np.searchsorted(all_cells, pre_cells)] += pre_vals
        want.append((all_cells, exp % (1 << 32), pre_cells, pre_vals))
    with torch.cuda.device(dev):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(reps):
            c.pe_count_lists(N, lists, counts, mats[0].data_ptr(), mats[1].data_ptr(), tmap.data_ptr() if tile_map else None)
        ran_rows = bool(c.last_launched & c.RAN_ROW_OWNERS)
        if expect_rows is None:
            expect_rows = mode == "rows"
        assert ran_rows == expect_rows
        for m in range(2):
            all_cells, exp, _, _ = want[m]
            got = _fetch(mats[m], all_cells)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "matrix %d: %d of %d cells differ, first (%d, %d): %d, expected %d" % (
                m, bad.size, all_cells.size, all_cells[bad[0]] // N, all_cells[bad[0]] % N, got[bad[0]], exp[bad[0]])
            assert _usum(mats[m]) == int(exp.sum()), "matrix %d holds a cell the model does not" % m
        if tile_map:
            marked = set(int(t) for t in torch.nonzero(tmap).flatten().cpu().numpy())
            expected = ntiles | {T * T + t for t in stiles}
            assert marked == expected, "tiles marked but untouched: %s; touched but unmarked: %s" % (sorted(marked - expected)[:8], sorted(expected - marked)[:8])
        if then_zero:
            nat.check(c._h, nat.lib().vs_counts_zero_tracked(c._h, C.c_void_p(mats[0].data_ptr()), C.c_void_p(mats[1].data_ptr()), N, C.c_void_p(tmap.data_ptr())))
            c.sync()
            assert not bool(tmap.any())
            for m, tiles in enumerate((ntiles, stiles)):
                _, _, pre_cells, pre_vals = want[m]
                kept = [v for cell, v in zip(pre_cells.tolist(), pre_vals.tolist()) if (cell // N // 64) * T + (cell % N) // 64 not in tiles]
                assert _usum(mats[m]) == sum(kept)  # (what the block touched is zero again; nothing else was)
    del mats, tmap


# ---- 1: every length pair --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_every_length_pair(monkeypatch, ctx, xctx, mode):
    _count_and_compare(monkeypatch, ctx, xctx, cases.every_length_pair(), "lengths", mode)


@pytest.mark.parametrize("ept", ["6", "32", "128"])
@pytest.mark.parametrize("mode", ["table", "rows", "noagg"])
def test_every_length_pair_other_tile_sizes(monkeypatch, ctx, xctx, mode, ept):
    _count_and_compare(monkeypatch, ctx, xctx, cases.every_length_pair(), "lengths", mode, extra={"VS_EPT": ept})


@pytest.mark.parametrize("n_pairs", [1, 31, 32, 33, 1023, 1024, 1025])
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_every_length_pair_block_sizes(monkeypatch, ctx, xctx, mode, n_pairs):
    n_nodes, pairs = cases.every_length_pair()
    _count_and_compare(monkeypatch, ctx, xctx, (n_nodes, pairs[:n_pairs]), "lengths%d" % n_pairs, mode)


# ---- 2: the smallest graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_smallest_graphs(monkeypatch, ctx, xctx, mode, n_nodes):
    _count_and_compare(monkeypatch, ctx, xctx, cases.tiny_graph(n_nodes), "tiny%d" % n_nodes, mode, then_zero=True)


# ---- 3: one hot cell, one hot list ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_one_hot_cell(monkeypatch, ctx, xctx, mode):
    _count_and_compare(monkeypatch, ctx, xctx, cases.hot_cell(), "hotcell", mode)


@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_one_hot_list_in_every_order(monkeypatch, ctx, xctx, mode):
    _count_and_compare(monkeypatch, ctx, xctx, cases.hot_list(), "hotlist", mode)


# ---- 4 / 5: the pair-major cell table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,fill", [("production", None), ("table", "1"), ("table", "100"), ("rows", None), ("rows", "1"), ("noagg", None)])
def test_cell_table_pressure(monkeypatch, ctx, xctx, mode, fill):
    case = cases.table_pressure()
    cases.assert_table_pressure(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "pressure", mode, extra={"VS_ACC_FILL": fill} if fill else None)


@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_eight_probes_exhausted(monkeypatch, ctx, xctx, mode):
    case = cases.probes_exhausted()
    cases.assert_probes_exhausted(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "probes", mode)


# ---- 6: a row wider than the strip table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["row", "column", "short"])
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_row_wider_than_the_strip_table(monkeypatch, ctx, xctx, mode, form):
    case = cases.wide_row(form)
    node, short, _, _ = _model(("wide" + form, 64), *cases.block(case))
    cases.assert_wide_row(case, form, node[0], short[0])
    _count_and_compare(monkeypatch, ctx, xctx, case, "wide" + form, mode)


# ---- 7: the list table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ltab", [None, "3", "0"])
def test_list_table_tag_collisions(monkeypatch, ctx, xctx, ltab):
    """A list table of 65 536 owners, the crowded one of eight slots (nearly every end stands for itself) and none.
    The block holds different lists under one tag, but in a table this large their home slots lie thousands apart, and
    no walk brings one upon the other: the tag comparison that must tell them apart is reached by
    test_different_lists_under_one_tag_that_meet_in_the_table, not here."""
    case = cases.list_table_distinct()
    cases.assert_tag_collisions(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "ltab", "rows", extra={"VS_LTAB_BITS": ltab} if ltab else None, reps=1)


MEETING = {"short12": (12, 0), "short16": (16, 0), "long20": (20, 16)}  # length, common leading positions


@pytest.mark.parametrize("mode,ltab", [("rows", None), ("rows", "3"), ("production", None), ("noagg", None)])
@pytest.mark.parametrize("kind", sorted(MEETING))
def test_different_lists_under_one_tag_that_meet_in_the_table(monkeypatch, ctx, xctx, kind, mode, ltab):
    """The only runs in which vs_same_list is certain to see a matching tag over another list: the block's lists share
    tag AND home slot, so the one that loses the slot walks into the winner's word whoever wins."""
    length, shared = MEETING[kind]
    case = cases.meeting_lists(length, shared)
    cases.assert_lists_meet(case, length, shared)
    _count_and_compare(monkeypatch, ctx, xctx, case, "meet" + kind, mode, extra={"VS_LTAB_BITS": ltab} if ltab else None)


@pytest.mark.parametrize("mode", ["production", "noagg"])
def test_list_table_block_pair_major(monkeypatch, ctx, xctx, mode):
    _count_and_compare(monkeypatch, ctx, xctx, cases.list_table_distinct(), "ltab", mode, reps=1)


@pytest.mark.parametrize("mode,ltab", [("production", None), ("noagg", None), ("rows", None), ("rows", "3"), ("rows", "0")])
def test_long_lists_that_differ_behind_position_16(monkeypatch, ctx, xctx, mode, ltab):
    case = cases.list_table_long()
    cases.assert_long_tag_collisions(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "ltablong", mode, extra={"VS_LTAB_BITS": ltab} if ltab else None)


# ---- 8: transposition limits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, {"VS_ROWS_KEYS": "7"}, {"VS_ROWS_SUB": "1024"}, {"VS_ROWS_PER_STRIP": "1"}, {"VS_ROWS_PER_STRIP": "64"}],
                         ids=["default", "keys7", "sub1024", "strip1", "strip64"])
def test_transposition_limits(monkeypatch, ctx, xctx, env):
    case = cases.many_rows()
    cases.assert_many_rows(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "manyrows", "rows", extra=env)


@pytest.mark.parametrize("mode", ["production", "noagg"])
def test_transposition_block_pair_major(monkeypatch, ctx, xctx, mode):
    _count_and_compare(monkeypatch, ctx, xctx, cases.many_rows(), "manyrows", mode)


# ---- 9: tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["production", "rows", "noagg"])
def test_lists_over_more_tiles_than_the_registers_hold(monkeypatch, ctx, xctx, mode):
    case = cases.spread_tiles()
    cases.assert_spread_tiles(case)
    _count_and_compare(monkeypatch, ctx, xctx, case, "spread", mode, then_zero=True)


# ---- 10: the 32-bit key edge -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [46340, 46341])
def test_key_edge_on_a_production_context(monkeypatch, ctx, xctx, n_nodes):
    import torch

    case = cases.key_edge(n_nodes)
    node, short, _, _ = _model(("edge%d" % n_nodes, 64), *cases.block(case))
    cases.assert_key_edge(case, node[0], short[0])
    # (the first graph that takes the row owners by itself)
    _count_and_compare(monkeypatch, ctx, xctx, case, "edge%d" % n_nodes, "production", expect_rows=n_nodes > 46340)
    if n_nodes > 46340:  # no table, 64-bit indices
        _count_and_compare(monkeypatch, ctx, xctx, case, "edge%d" % n_nodes, "table", expect_rows=False)
    torch.cuda.empty_cache()


# ---- 11: cell indices beyond 2^32 -------------------------------------------------------------------------------------------
def test_cell_indices_beyond_32_bits(monkeypatch, ctx, xctx):
    import torch

    n_nodes = 65600
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(ctx.device)
    need = 2 * 4 * n_nodes * n_nodes + (6 << 30)
    if free < need:
        pytest.skip("%.1f GB of device memory free, the two matrices of %d nodes and their sums take %.1f GB" % (free / 1e9, n_nodes, need / 1e9))
    case = cases.key_edge(n_nodes, spread=40)
    node, short, _, _ = _model(("edge%d" % n_nodes, 64), *cases.block(case))
    cases.assert_key_edge(case, node[0], short[0])
    assert node[0].max() >= 1 << 32 and short[0].max() >= 1 << 32
    _count_and_compare(monkeypatch, ctx, xctx, case, "edge%d" % n_nodes, "production", expect_rows=True, then_zero=True)
    torch.cuda.empty_cache()


def test_refusals_reach_the_caller(host, ctx):
    import torch

    mats = torch.zeros(2, 100, dtype=torch.int32, device="cuda:%d" % ctx.device)
    lists, counts = host.list_block([([1, 2], [3])], 64)
    for bad_lists, bad_counts in ((np.where(lists == 2, 10, lists), counts), (np.where(lists == 2, 1, lists), counts), (lists, np.array([21, 1]))):
        with pytest.raises(Exception) as e:
            ctx.pe_count_lists(10, bad_lists, bad_counts, mats[0].data_ptr(), mats[1].data_ptr())
        assert getattr(e.value, "code", None) == -6
    ctx.sync()
    assert not bool(mats.any())


# ---- the locus order, observed ---------------------------------------------------------------------------------------------
def _random_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _locus_inputs(graph, n_pairs, seed):
    """A graph (k = 21), pairs of reads over it -- clean ones, reads that hit nothing, dirty ones, pairs the filters drop --
    and per pair what its locus key may be: N + 1, N, or the nodes that hold a posting of the forward read's first grid
    seed that hits."""
    rng = np.random.default_rng(seed)
    k, K = 21, 22
    if graph == "small":
        seqs = [_random_seq(rng, int(rng.integers(10, 260))) for _ in range(600)]
        seqs[17] = seqs[16]  # the same text twice: a seed with two postings
        seqs[40] = sem.rc(seqs[41])
    else:  # a chain of short nodes: N + 2 keys are more than one LDS histogram holds
        text = _random_seq(rng, 40000 * 10 + k)
        seqs = [text[10 * i: 10 * i + 10 + k] for i in range(40000)]
    table, w, s = sem.build(seqs, K)
    N = len(seqs)
    long_nodes = [i for i, x in enumerate(seqs) if len(x) >= 30]
    fwd, rve, allowed = [], [], []
    for p in range(n_pairs):
        kind = p % 11
        node = long_nodes[int(rng.integers(0, len(long_nodes)))]
        text = seqs[node] if p % 2 else sem.rc(seqs[node])
        if graph != "small":  # a read across several nodes of the chain
            at = int(rng.integers(0, len(seqs) - 20))
            text = seqs[at] + "".join(x[k:] for x in seqs[at + 1: at + 14])
            text = text if p % 2 else sem.rc(text)
        lo = int(rng.integers(0, max(len(text) - 29, 1)))
        f = text[lo: lo + int(rng.integers(30, 151))]
        r = sem.rc(f)
        if kind == 0:
            f = _random_seq(rng, int(rng.integers(K, 151)))  # hits nothing
        elif kind == 1:
            f = f[: int(rng.integers(0, K))]  # too short: dropped
        elif kind == 2:
            r = r[:5] + "N" + r[6:]  # an N in the mate: dropped
        elif kind == 3:  # dirty: bytes outside ACGT that are no N
            cut = int(rng.integers(0, len(f)))
            f = f[:cut] + "X" + f[cut + 1:]
        elif kind == 4:
            f = f[: len(f) // 2] + _random_seq(rng, 40)  # a tail that hits nothing
        elif kind == 5:
            f = _random_seq(rng, 45)[: 150 - min(len(f), 100)] + f[:100]  # a head that hits nothing
        fwd.append(f)
        rve.append(r)
        if "N" in f or "N" in r or len(f) < K or len(r) < K:
            allowed.append({N + 1})
            continue
        hit = {N}
        for j in range(sem.phase(len(f), w, s), len(f) - w + 1, s):
            seed_text = f[j: j + w]
            if not all(sem.valid(ch) for ch in seed_text):
                continue
            rc = sem.rc(seed_text)
            post = table.get(min(seed_text, rc))
            if post:
                hit = {node for node, _, _ in post}
                break
        allowed.append(hit)
    return seqs, k, fwd, rve, allowed


_locus_cache = {}


@pytest.mark.parametrize("graph,n_pairs,global_sort", [("small", 5003, False), ("chain", 5003, False), ("small", 5003, True), ("chain", 5003, True),
                                                       ("small", 4095, False), ("small", 4096, False)])
def test_locus_order(monkeypatch, host, ctx, xctx, graph, n_pairs, global_sort):
    if (graph, n_pairs) not in _locus_cache:
        _locus_cache[(graph, n_pairs)] = _locus_inputs(graph, n_pairs, 31 + n_pairs)
    seqs, k, fwd, rve, allowed = _locus_cache[(graph, n_pairs)]
    N = len(seqs)
    c = xctx if global_sort else ctx
    if global_sort:
        monkeypatch.setenv("VS_LOCUS_GLOBAL", "1")
    c.build_index(seqs, k, renumber=False)
    reads = c.pack_pairs(fwd, rve)
    c.map_ends(reads, cap=64)
    keys, perm, sort, n = c.last_order()
    reads.free()
    assert n == n_pairs
    if n_pairs < 4096:  # too few pairs to be worth a sort: the mapping kernel takes them in input order
        assert sort == 0 and keys.size == 0 and perm.size == 0
        return
    assert sort == (c.RAN_LOCUS_GLOBAL_SORT if global_sort else c.RAN_LOCUS_LDS_SORT) == c.last_launched & 3
    assert (N + 2 > 36864) == (graph == "chain")  # (two LDS passes over the keys)
    # the keys against the host model
    kinds = {"dropped": 0, "none": 0, "hit": 0, "several": 0}
    for p in range(n_pairs):
        assert int(keys[p]) in allowed[p], (p, int(keys[p]), sorted(allowed[p])[:5], fwd[p])
        kinds["dropped" if allowed[p] == {N + 1} else "none" if allowed[p] == {N} else "hit"] += 1
        kinds["several"] += len(allowed[p]) > 1
    assert min(kinds["dropped"], kinds["none"], kinds["hit"]) > n_pairs // 20 and (kinds["several"] > 0 or graph == "chain")
    # a permutation, in key order
    assert np.array_equal(np.sort(perm), np.arange(n_pairs, dtype=perm.dtype))
    sorted_keys = keys[perm].astype(np.int64)
    assert (np.diff(sorted_keys) >= 0).all()
    if not global_sort:
        # pairs of one key from different workgroup chunks keep the chunks' order (the scan runs in (key, workgroup)
        # order); nothing is promised inside a chunk
        chunk = -(-n_pairs // 256)
        wg = perm.astype(np.int64) // chunk
        same = np.diff(sorted_keys) == 0
        assert (np.diff(wg)[same] >= 0).all()
        assert int(same.sum()) > n_pairs // 10 and len(set(wg.tolist())) > 200
