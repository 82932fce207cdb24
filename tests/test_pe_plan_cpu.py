"""The launch plan of a PE count (vstrains_amd/csrc/vs_pe_plan.h: vs_pe_plan, one pure function of scalars) on the CPU,
through oracle/plan_check.cpp.  Expected values are the decisions the code took before the plan existed
(tests/golden/pe_plan_parent.json, recorded from those lines) and what the project's documents state -- never what the plan
itself gives.  No device, no HIP call."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from seed_index_model import geometry  # (w, s) of an index with K = k + 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = ["n_nodes", "K", "w", "s", "n_seed_pos", "n_distinct", "max_node_len", "n_cu", "n_ends", "max_len", "has_mask", "has_inv4",
      "count", "tile_map", "ept", "grid_per_cu", "acc_fill_pct", "shortcut", "adapt_grid", "acc_rows", "ltab_bits", "rows_keys",
      "rows_sub", "rows_per_strip", "no_sort", "locus_global", "no_fast", "no_std", "no_agg", "no_mid"]
OUT = ["status", "ept", "pmax", "wpe", "pool", "pool_bits", "words_cap", "magic_pmax", "magic_wpe", "lds_bytes", "mode", "sw", "sp", "ad",
       "n_tiles", "grid", "list_ends", "list_words", "tiles_per_wg", "shortcut", "mid_fast", "use_sort", "lds_sort", "locus_chunk",
       "locus_per_pass", "locus_keys", "locus_hist_words", "use_rows", "use_table", "mark_tiles", "acc_grid", "acc_per_wg", "acc_fill",
       "rows_sub_pairs", "rows_ltab_bits", "rows_keys", "rows_fill", "rows_per_strip", "slow_grid", "dense_bytes"]
DEFAULTS = dict(n_nodes=5039, n_seed_pos=3500000, n_distinct=1000000, max_node_len=30000, n_cu=256, n_ends=2 * 10 ** 7, max_len=150,
                has_mask=0, has_inv4=0, count=1, tile_map=0, ept=0, grid_per_cu=128, acc_fill_pct=-1, shortcut=-1, adapt_grid=-1,
                acc_rows=-1, ltab_bits=-1, rows_keys=0, rows_sub=0, rows_per_strip=0, no_sort=0, locus_global=0, no_fast=0, no_std=0,
                no_agg=0, no_mid=0)
VS_E_RANGE = -6
# the instantiations of k_pe_tiles the library holds, as (MODE, SW, SP, AD): five compile-time shapes with and without the
# adaptive grid, and the run-time shape of every mode
SHAPES = [(1, 10, 4), (1, 8, 3), (1, 7, 2), (1, 7, 3), (2, 16, 2)]
TABLE = {s + (ad,) for s in SHAPES for ad in (0, 1)} | {(m, 0, 0, 0) for m in (0, 1, 2)}
STD = {1: dict(ept=64, pool_bits=10, K=56, w=31, s=26), 2: dict(ept=60, pool_bits=10, K=128, w=63, s=66)}  # STD_* / STD2_*


@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "oracle", "_build", "libvs_plan_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    lib = C.CDLL(path)
    lib.vs_pe_plan_check.restype = C.c_int
    lib.vs_pe_plan_check.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(rows):
        """rows: lists in the order of IN, or dicts over DEFAULTS with k (or K, w, s).  Returns (plans as dicts, messages)."""
        full = []
        for r in rows:
            if isinstance(r, dict):
                d = dict(DEFAULTS, **r)
                if "k" in d:
                    d["K"] = d.pop("k") + 1
                    d["w"], d["s"] = geometry(d["K"])
                r = [d[f] for f in IN]
            full.append(r)
        a = np.array(full, dtype=np.int64).reshape(len(full), len(IN))
        out = np.zeros((len(full), len(OUT)), dtype=np.uint64)
        msgs = C.create_string_buffer(128 * len(full))
        assert lib.vs_pe_plan_check(len(full), a.ctypes.data, out.ctypes.data, msgs) == len(OUT)
        plans = []
        for o in out.astype(np.int64).tolist():  # (status is negative on failure)
            plans.append(dict(zip(OUT, o)))
        raw = msgs.raw
        return plans, [raw[128 * i:128 * i + 128].split(b"\0")[0].decode() for i in range(len(full))]

    return run


def name(p):
    return "<%d, %du, %du%s>" % (p["mode"], p["sw"], p["sp"], ", true" if p["ad"] else "")


# ---- 1. the recorded decisions of the code before the plan ---------------------------------------------------------------
def test_every_recorded_decision_of_the_parent(plan):
    with open(os.path.join(ROOT, "tests", "golden", "pe_plan_parent.json")) as f:
        g = json.load(f)
    assert g["in"] == IN and g["out"] == OUT
    assert len(g["rows"]) >= 300
    plans, msgs = plan([r[0] for r in g["rows"]])
    seen = set()
    for (inp, want, msg), got, got_msg in zip(g["rows"], plans, msgs):
        assert [got[f] for f in OUT] == want and got_msg == msg, (dict(zip(IN, inp)), [(f, w, got[f]) for f, w in zip(OUT, want) if got[f] != w], msg, got_msg)
        if got["n_tiles"]:
            seen.add((got["mode"], got["sw"], got["sp"], got["ad"]))
    assert seen == TABLE  # (the record reaches every instantiation)
    assert {m for _, _, m in g["rows"] if m} >= {"more than 2^25-2 nodes", "reads of 20000 bases with k+1=22 need 263052 B of LDS per pair (limit 160 KiB)"}


# ---- 2. what the project states ----------------------------------------------------------------------------------------------
K55 = [(range(97, 108), "<1, 7u, 2u>"), (range(108, 113), "<1, 7u, 3u>"), (range(113, 129), "<1, 8u, 3u>"), (range(129, 145), "<1, 0u, 0u>"),
       (range(145, 160), "<1, 10u, 4u>"), (range(160, 161), "<1, 0u, 0u>")]


def test_compile_time_shapes_by_read_length_at_k55(plan):
    lens = list(range(56, 161))
    few, _ = plan([dict(k=55, max_len=n) for n in lens])
    many, _ = plan([dict(k=55, max_len=n, n_seed_pos=6 * DEFAULTS["n_distinct"]) for n in lens])
    edge, _ = plan([dict(k=55, max_len=n, n_seed_pos=6 * DEFAULTS["n_distinct"] - 1) for n in lens])
    for p in few + many + edge:
        assert (p["status"], p["ept"], p["pool_bits"]) == (0, 64, 10)
    for rng, want in K55:
        for n in rng:
            assert name(few[n - 56]) == want, n
            assert name(edge[n - 56]) == want, n  # fewer than 6 positions per distinct seed
            assert name(many[n - 56]) == (want if want.endswith("0u>") else want[:-1] + ", true>"), n
    for n in range(56, 97):
        assert name(few[n - 56]) == name(many[n - 56]) == "<1, 0u, 0u>"


def test_compile_time_shape_at_k127(plan):
    lens = list(range(200, 300))
    few, _ = plan([dict(k=127, max_len=n) for n in lens])
    many, _ = plan([dict(k=127, max_len=n, n_seed_pos=6 * DEFAULTS["n_distinct"]) for n in lens])
    for n, p, q in zip(lens, few, many):
        if 241 <= n <= 256:
            assert (p["ept"], name(p), name(q)) == (60, "<2, 16u, 2u>", "<2, 16u, 2u, true>"), n
        else:
            assert name(p) == name(q) == "<2, 0u, 0u>", n


@pytest.mark.parametrize("k,max_len", [(55, 100), (55, 110), (55, 120), (55, 150), (127, 250)])
def test_switches_and_call_kinds(plan, k, max_len):
    base = dict(k=k, max_len=max_len)
    (std, no_std, no_fast, lists, ad1, ad0, long_node, longer_node, short_node, masked, listed), _ = plan(
        [base, dict(base, no_std=1), dict(base, no_fast=1), dict(base, count=0), dict(base, adapt_grid=1),
         dict(base, adapt_grid=0, n_seed_pos=10 ** 7), dict(base, max_node_len=2 ** 23), dict(base, max_node_len=2 ** 31),
         dict(base, max_node_len=2 ** 23 - 1), dict(base, has_mask=1), dict(base, has_mask=1, has_inv4=1)])
    mode = 1 if k == 55 else 2
    assert (std["mode"], std["sw"] != 0, std["ad"]) == (mode, True, 0)
    assert name(no_std) == "<%d, 0u, 0u>" % mode           # VS_NO_STD
    assert name(no_fast) == "<0, 0u, 0u>"                  # VS_NO_FAST
    assert name(lists) == "<%d, 0u, 0u>" % mode            # a call that only wants the lists never gets a compile-time shape
    assert name(ad1) == name(std)[:-1] + ", true>" and name(ad0) == name(std)
    assert name(long_node) == name(longer_node) == "<0, 0u, 0u>" and long_node["mid_fast"] == 0  # nodes of 2^23 bases and more
    assert name(short_node) == name(std) and short_node["mid_fast"] == (1 if k == 55 else 0)
    assert name(masked) == "<0, 0u, 0u>" and name(listed) == name(std)  # a mask alone: the generic loops; with position lists: as without


def test_long_window_reach(plan):
    """The rule test_long_stride_kernel_with_ragged_dirty_reads states for nine cases, for every k from 86 to 160 and
    every maximum read length up to 511."""
    cases = [(k, n) for k in range(86, 161) for n in range(k + 1, 512)]
    plans, _ = plan([dict(k=k, max_len=n) for k, n in cases])
    off, _ = plan([dict(k=k, max_len=n, no_fast=1) for k, n in cases[::17]])
    reach = {}
    for (k, max_len), p in zip(cases, plans):
        K, w = k + 1, (63 if k >= 95 else 31)
        s_ = K - w + 1
        ok = max_len - ((max_len - w) % s_ + s_) // 2 - (w if w <= 31 else 0) <= 256
        reach[k, max_len] = in_reach = ok and reach.get((k, max_len - 1), True)  # (all lengths from K to max_len)
        assert p["status"] == 0 and p["mode"] == (2 if in_reach else 0), (k, max_len)
    assert all(p["mode"] == 0 for p in off)
    assert reach[127, 317] and not reach[127, 318]


def test_graph_and_block_size_boundaries(plan):
    (a, b), _ = plan([dict(k=55, n_nodes=46340), dict(k=55, n_nodes=46341)])
    assert (a["use_rows"], a["use_table"], b["use_rows"], b["use_table"]) == (0, 1, 1, 1)
    (c,), _ = plan([dict(k=55, n_nodes=46341, acc_rows=0)])
    assert (c["use_rows"], c["use_table"]) == (0, 0)  # beyond 46 340 nodes without the row owners: no cell table
    (a, b), _ = plan([dict(k=55, n_nodes=147454), dict(k=55, n_nodes=147455)])
    assert (a["use_sort"], a["lds_sort"], a["locus_keys"], b["use_sort"], b["lds_sort"]) == (1, 1, 147456, 1, 0)
    (a, b), _ = plan([dict(k=55, n_ends=2 * 4095), dict(k=55, n_ends=2 * 4096)])
    assert (a["use_sort"], b["use_sort"]) == (0, 1)
    (a, b), msgs = plan([dict(k=55, n_nodes=2 ** 25 - 2), dict(k=55, n_nodes=2 ** 25 - 1)])
    assert a["status"] == 0 and b["status"] == VS_E_RANGE and msgs == ["", "more than 2^25-2 nodes"]


# ---- 3. invariants over every index geometry and read length --------------------------------------------------------------
def pool_for(ept):
    b = 6
    while (1 << b) < 16 * ept:
        b += 1
    return b


def tile_words(ept, pmax, words_cap, pool, trim):
    """The LDS carve of a tile (TileLayout), in words."""
    ni, lc, chunk = ept * pmax, 16, 512
    return (2 * ((ept + 2) & ~1) + 2 * ept + 2 * ept + ept + 2 * (words_cap + 8) + (ni + 1) + 2 * ni + 4 * pool + 2 * ept
            + max(ept * lc - trim, chunk) + 16)


@pytest.mark.parametrize("n_seed_pos,count", [(3500000, 1), (8900000, 1), (3500000, 0)])
def test_invariants_over_the_full_sweep(plan, n_seed_pos, count):
    n_pairs = 10 ** 7 + 1
    cases = [(K, n) for K in range(22, 161) for n in range(1, 512)]
    plans, msgs = plan([dict(K=K, w=geometry(K)[0], s=geometry(K)[1], max_len=n, n_ends=2 * n_pairs, n_seed_pos=n_seed_pos, count=count)
                        for K, n in cases])
    shapes = set()
    for (K, n), p, msg in zip(cases, plans, msgs):
        w, s = geometry(K)
        if p["status"]:
            assert p["status"] == VS_E_RANGE and msg.startswith("reads of %d bases with k+1=%d need " % (n, K)) and msg.endswith(" B of LDS per pair (limit 160 KiB)")
            assert int(msg.split(" need ")[1].split(" B")[0]) > 160 * 1024
            continue
        assert msg == ""
        ept, pmax, wpe = p["ept"], p["pmax"], p["wpe"]
        assert ept % 2 == 0 and ept >= 2 and ept * pmax <= 4096, (K, n, p)
        assert wpe == max(1, (n + 15) // 16) and pmax == max(1, (n - w + 1) // s if n >= w else 0) and p["words_cap"] == ept * wpe
        assert p["pool_bits"] == pool_for(ept) and p["pool"] == 1 << p["pool_bits"]
        shape = (p["mode"], p["sw"], p["sp"], p["ad"])
        assert shape in TABLE, (K, n, shape)
        shapes.add(shape)
        std12 = p["sw"] != 0 and not p["ad"]  # the 768-slot table and the trimmed lists of the non-adaptive compile-time shapes
        pool, trim = (768, 192 if p["mode"] == 2 else 64) if std12 else (p["pool"], 0)
        assert p["lds_bytes"] == 4 * tile_words(ept, pmax, p["words_cap"], pool, trim) <= 160 * 1024, (K, n, p)
        assert p["n_tiles"] * (ept // 2) >= n_pairs > (p["n_tiles"] - 1) * (ept // 2)
        assert p["grid"] * p["tiles_per_wg"] >= p["n_tiles"] and p["grid"] <= 256 * 128 and p["list_ends"] == p["n_tiles"] * ept
        if p["sw"]:  # every run-time value the instantiation replaces by a constant
            assert count and dict(ept=ept, pool_bits=p["pool_bits"], K=K, w=w, s=s) == STD[p["mode"]], (K, n, p)
            assert (wpe, pmax) == (p["sw"], p["sp"])
            assert not p["ad"] or ept * p["sp"] <= 256  # static_assert(C_EPT * SP <= TTPB)
    if count:
        assert shapes == {t for t in TABLE if t[3] == (n_seed_pos >= 6000000) or t[1] == 0}
    else:
        assert shapes == {(m, 0, 0, 0) for m in (0, 1, 2)}
