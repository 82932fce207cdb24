"""The constructed families of tests/pe_overflow_cases.py without a device: every case sits on the side of k_pe_mid's and
k_pe_slow's limits it claims (probes, touched nodes, accepted nodes per end, read off the model), the model's lists equal the
C oracle's, the decoys are touched and rejected, the crowd of one home slot and the run across slot 255 -> 0 exist, and what
the model restates of the host code (seed_geometry, vs_seed_probes, slow_grid_for, the plan's mode and mid_fast) equals
vs_pe_plan through oracle/plan_check.cpp and a table of values.  What the device makes of them: tests/test_pe_overflow_gpu.py."""
import collections
import functools

import pytest

import pe_overflow_cases as poc
import seed_extend_model as model
from oracle import pe_oracle_c

# label -> where the pair must end, and (probes, touched, accepted) of its heavy end
PROBES = {"83 bases": ("mid", (63, 63, 63)), "84 bases": ("mid", (64, 64, 64)), "85 bases": ("slow", (65, 65, 65)),
          "84 + 84": ("mid", (64, 64, 64)), "85 + 84": ("slow", (65, 65, 65))}
LIST = {"21": ("mid", (11, 21, 21)), "63": ("mid", (32, 63, 63)), "64": ("mid", (32, 64, 64)), "65": ("slow", (33, 65, 65)),
        "66": ("slow", (33, 66, 66)), "64 + 64": ("mid", (32, 64, 64)), "64 + 0": ("mid", (32, 64, 64)), "65 + 64": ("slow", (33, 65, 65)),
        "64 + 63": ("mid", (32, 64, 64))}


@functools.lru_cache(maxsize=None)
def modelled(name):
    """A family with its model, the model's verdicts and the C oracle (computed once, shared, not changed)."""
    fam = poc.family(name)
    mdl = poc.Model(fam["seqs"], fam["k"])
    where, mode, mid_fast = poc.verdicts(fam, mdl)
    return dict(fam=fam, mdl=mdl, where=where, mode=mode, mid_fast=mid_fast, orc=pe_oracle_c.Oracle(fam["seqs"], fam["k"]))


def _heavy(mdl, f, r):
    """(probes, touched, accepted) of the end of a pair with the most accepted nodes."""
    e = max((mdl.end(f), mdl.end(r)), key=lambda e: (len(e["accepted"]), len(e["touched"])))
    return e["probes"], len(e["touched"]), len(e["accepted"])


@pytest.mark.parametrize("name", poc.FAMILIES)
def test_the_model_lists_equal_the_c_oracle_and_every_pair_is_given_up(name):
    m = modelled(name)
    fam, mdl, orc = m["fam"], m["mdl"], m["orc"]
    assert len(fam["fwd"]) == len(fam["rve"]) == len(fam["label"]) == len(m["where"])
    for f, r, lab, where in zip(fam["fwd"], fam["rve"], fam["label"], m["where"]):
        if where == "dropped":
            assert "N" in f + r
            continue
        for e in (f, r):
            assert mdl.end(e)["accepted"] == orc.map_end(e), (name, lab)
            assert set(mdl.end(e)["accepted"]) <= set(mdl.end(e)["touched"])
        assert where in ("mid", "slow") or lab == "long", (name, lab, where)
    # small enough for its time budget: a few hundred pairs, dense matrices of at most a few MB but for the numbered graph
    assert len(fam["fwd"]) <= 600 and (len(fam["seqs"]) <= 1100 or name == "slots")
    assert max(len(x) for x in fam["fwd"] + fam["rve"]) <= {"batches": 600, "plain": 200}.get(name, 90)


@pytest.mark.parametrize("name,table", [("probes", PROBES), ("list", LIST)])
def test_probe_and_list_limits_sit_on_their_edges(name, table):
    m = modelled(name)
    fam, mdl = m["fam"], m["mdl"]
    assert (m["mode"], m["mid_fast"], mdl.K, mdl.w, mdl.s) == (1, 1, 21, 21, 1)
    assert set(fam["label"]) == set(table)
    for f, r, lab, where in zip(fam["fwd"], fam["rve"], fam["label"], m["where"]):
        assert (where, _heavy(mdl, f, r)) == table[lab], (lab, where, _heavy(mdl, f, r))
        assert max(len(f), len(r)) <= (85 if name == "probes" else 60)
    if name == "list":  # the heavy ends keep away from the probe limit, and both sides of a pair come up heavy
        assert all(mdl.end(e)["probes"] <= 40 for e in fam["fwd"] + fam["rve"])
        both = {lab: (len(mdl.end(f)["accepted"]), len(mdl.end(r)["accepted"])) for f, r, lab in zip(fam["fwd"], fam["rve"], fam["label"])}
        assert both["64 + 64"] == (64, 64) and both["64 + 0"] == (64, 0) and both["65 + 64"] == (65, 64)
        twins = [x for x in fam["seqs"] if fam["seqs"].count(x) == 1 and model.rc(x) in fam["seqs"]]
        assert len(twins) >= 100 and max(collections.Counter(fam["seqs"]).values()) == 2  # (twins and duplicates)
    heavy_side = {(lab, len(mdl.end(f)["accepted"]) > len(mdl.end(r)["accepted"])) for f, r, lab in zip(fam["fwd"], fam["rve"], fam["label"])}
    assert all((lab, True) in heavy_side and (lab, False) in heavy_side for lab in ("84 bases", "85 bases") if name == "probes")
    assert all((lab, True) in heavy_side and (lab, False) in heavy_side for lab in ("64", "65") if name == "list")


def test_slots_touch_255_256_257_nodes_through_rejected_decoys():
    m = modelled("slots")
    fam, mdl, orc = m["fam"], m["mdl"], m["orc"]
    assert (m["mode"], m["mid_fast"]) == (1, 1) and len(fam["seqs"]) == poc.SLOTS_NODES
    assert {(c["variant"], c["touched"]) for c in fam["cases"]} == {(v, t) for v in poc.SLOT_VARIANTS for t in (255, 256, 257)}
    for c in fam["cases"]:
        e = mdl.end(c["read"])
        assert e["touched"] == sorted(c["chain"] + c["decoys"]) and len(e["touched"]) == c["touched"]
        assert e["accepted"] == sorted(c["chain"]) == orc.map_end(c["read"]) and len(c["chain"]) == poc.SLOT_ACCEPTED <= poc.LCAP
        assert e["probes"] == 40 and e["dirty"] == 0
        rc_read = model.rc(c["read"])
        assert orc.map_end(rc_read) == e["accepted"] and mdl.end(rc_read)["touched"] == e["touched"]
        # every decoy shares exactly one (k+1)-mer with the read, is as long as it, and both strands of the nodes are there
        windows = collections.Counter()
        for n in c["decoys"]:
            node = fam["seqs"][n]
            assert len(node) == len(c["read"])
            shared = [(p, o, st) for st, text in ((0, node), (1, model.rc(node))) for o in range(len(text) - 20) for p in range(40)
                      if text[o:o + 21] == c["read"][p:p + 21]]
            assert len(shared) == 1
            windows[shared[0][0]] += 1
            windows["strand", shared[0][2]] += 1
        assert windows["strand", 0] > 100 and windows["strand", 1] > 100
        seeds = {p: n for p, n in windows.items() if isinstance(p, int)}
        if c["variant"] == "oneseed":
            assert max(seeds.values()) >= 200
        else:
            assert len(seeds) == 25 and max(seeds.values()) <= 10
        homes = collections.Counter(poc.home_slot(n) for n in e["touched"])
        if c["variant"] == "crowd":
            assert max(homes.values()) >= 40
        if c["variant"] == "wrap":  # 30 nodes and more start in the last six slots: their run goes on through slot 0
            assert sum(homes[h] for h in range(250, 256)) >= 30
    for lab, where in zip(fam["label"], m["where"]):
        assert where == ("slow" if lab.endswith("257") else "mid"), (lab, where)
    assert [poc.home_slot(n) for n in (0, 1, 2, 3, 255, 10495)] == [0, 158, 60, 218, 153, 68]  # (2654435761 * n mod 2^32, top byte: 255 -> 2571253583, 10495 -> 1145429839)


def test_batches_end_in_k_pe_slow_with_one_two_and_three_probe_batches():
    m = modelled("batches")
    fam, mdl = m["fam"], m["mdl"]
    assert (m["mode"], m["mid_fast"]) == (0, 0) and set(m["where"]) == {"slow"}
    batches = {len(e): -(-mdl.end(e)["probes"] // poc.SLOW_BATCH) for e in fam["fwd"] + fam["rve"]}
    assert [batches[n] for n in (276, 277, 533, 600)] == [1, 2, 3, 3]
    dirty = [e for e in fam["fwd"] + fam["rve"] if mdl.end(e)["dirty"]]
    six = [e for e in dirty if mdl.end(e)["dirty"] == 6]
    assert len(six) == 2 and all(len(e) == 533 for e in six)
    for e in six:  # bytes outside ACGT on both sides of the first batch boundary (probe 256 = read offset 256), within a window of it
        bad = [p for p, c in enumerate(e) if not model.valid(c)]
        assert any(256 - 21 < p < 256 for p in bad) and any(256 <= p < 256 + 21 for p in bad)
        assert 256 < len(mdl.end(e)["accepted"]) < mdl.end(e)["probes"]


@pytest.mark.parametrize("name", ["fast", "plain"])
def test_the_knife_edge_pairs_keep_their_answers_with_the_dirty_bytes_in_the_mate(name):
    import pe_extension_cases as pec

    m = modelled(name)
    fam, mdl, orc = m["fam"], m["mdl"], m["orc"]
    orig = pec.knife_edge_family(21, 90, pec.SHAPES[(21, 90)]["step"])
    assert (m["mode"], m["mid_fast"]) == ((1, 1) if name == "fast" else (2, 0))
    clean = kept = 0
    for p, c in enumerate(fam["cases"]):
        case, mate = (fam["rve"][p], fam["fwd"][p]) if c["end"] else (fam["fwd"][p], fam["rve"][p])
        assert case == pec.case_read(orig, p) and pec.dirty_bytes(mate) == 5
        if m["where"][p] == "dropped":
            continue
        assert m["where"][p] == "mid"
        assert orc.map_end(mate) == [fam["anchor"]]
        clean += pec.dirty_bytes(case) == 0
        kept += c["node"] in mdl.end(case)["accepted"]
    n = sum(w == "mid" for w in m["where"])
    assert clean > 0.6 * n and 0.35 * n < kept < 0.65 * n, (clean, kept, n)
    if name == "plain":
        assert m["where"][-1] == "tiles" and len(fam["fwd"][-1]) == 200 and fam["fwd"][:-1] == poc.family("fast")["fwd"]


def test_second_pairs_outnumber_the_walkers_of_both_kernels_three_times():
    rnd, order, reps = poc.second_pairs(256)
    where, mode, mid_fast = poc.verdicts(rnd)
    assert (mode, mid_fast) == (1, 1)
    n_mid = sum(where[i] in ("mid", "slow") for i in order)
    n_slow = sum(where[i] == "slow" for i in order)
    assert poc.mid_waves(256) == 8192 and poc.slow_grid_for(len(rnd["seqs"])) == 2048
    assert n_mid > 3 * 8192 and n_slow > 3 * 2048, (n_mid, n_slow)
    assert len(order) == reps * len(where) <= 40000 and collections.Counter(order) == {i: reps for i in range(len(where))}
    assert max(len(x) for x in rnd["fwd"] + rnd["rve"]) <= 90
    # neighbours differ in kind: a knife-edge pair (at most two accepted nodes an end), then a pair with an end of 62 and more,
    # which leaves k_pe_mid every other time
    mdl = poc.Model(rnd["seqs"], rnd["k"])
    for i in range(0, len(where), 2):
        assert rnd["label"][i] == "knife" and where[i] in ("mid", "dropped") and where[i + 1] == ("slow" if (i // 2) % 2 else "mid")
        if where[i] == "mid":
            assert max(len(mdl.end(e)["accepted"]) for e in (rnd["fwd"][i], rnd["rve"][i])) <= 2
        assert max(len(mdl.end(e)["accepted"]) for e in (rnd["fwd"][i + 1], rnd["rve"][i + 1])) >= 62
    assert order[:len(where)] == list(range(len(where))) and order[len(where):2 * len(where)] != list(range(len(where)))
    assert poc.second_pairs(304)[2] > reps  # (more wavefronts, more repetitions)


def test_what_the_model_restates_equals_the_plan_and_a_table_of_values():
    """seed_geometry, vs_seed_probes, slow_grid_for, the mode and mid_fast: against vs_pe_plan (csrc/vs_pe_plan.h through
    oracle/plan_check.cpp, as tests/test_pe_plan_cpu.py runs it) on every family's scalars, and against values worked out by hand."""
    import ctypes as C
    import os
    import subprocess

    import numpy as np

    import test_pe_plan_cpu as tp

    assert [model.geometry(K) for K in (21, 22, 56, 128)] == [(21, 1), (21, 2), (31, 26), (63, 66)]
    assert [poc.seed_probes(n, 21, 1) for n in (20, 21, 83, 84, 85, 276, 277, 533, 600)] == [0, 1, 63, 64, 65, 256, 257, 513, 580]
    assert [poc.seed_probes(n, 21, 2) for n in (21, 22, 90, 200)] == [0, 1, 35, 90]
    assert [poc.seed_probes(n, 31, 26) for n in (55, 56, 150)] == [0, 1, 4]
    # 4 GB / (24 bytes a node): 2 048 workgroups up to 87 381 nodes, 64 from 2 796 203 on
    assert [poc.slow_grid_for(n) for n in (0, 1, 881, 10496, 87381, 87382, 1000000, 2796202, 2796203, 30000000)] == [2048, 2048, 2048, 2048, 2048, 2047, 178, 64, 64, 64]
    path = os.path.join(tp.ROOT, "oracle", "_build", "libvs_plan_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(tp.ROOT, "oracle")])
    lib = C.CDLL(path)
    lib.vs_pe_plan_check.restype = C.c_int
    lib.vs_pe_plan_check.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    rows, want = [], []
    fams = [(name, poc.family(name)) for name in poc.FAMILIES] + [("second", poc.second_pairs_round())]
    for name, fam in fams:
        K = fam["k"] + 1
        w, s = model.geometry(K)
        seqs, maxlen = fam["seqs"], max(len(x) for x in fam["fwd"] + fam["rve"])
        table, _, _ = model.build(seqs, K)
        rows.append([dict(tp.DEFAULTS, n_nodes=len(seqs), K=K, w=w, s=s, n_seed_pos=sum(len(x) - w + 1 for x in seqs), n_distinct=len(table),
                          max_node_len=max(len(x) for x in seqs), n_ends=2 * len(fam["fwd"]), max_len=maxlen, has_mask=1, has_inv4=1)[f] for f in tp.IN])
        want.append((name,) + poc.block_shape(K, w, s, maxlen) + (poc.slow_grid_for(len(seqs)), max(poc.seed_probes(maxlen, w, s), 1)))
    a = np.array(rows, dtype=np.int64)
    out = np.zeros((len(rows), len(tp.OUT)), dtype=np.uint64)
    msgs = C.create_string_buffer(128 * len(rows))
    assert lib.vs_pe_plan_check(len(rows), a.ctypes.data, out.ctypes.data, msgs) == len(tp.OUT)
    for o, (name, mode, mid_fast, grid, pmax) in zip(out.astype(np.int64).tolist(), want):
        p = dict(zip(tp.OUT, o))
        assert p["status"] == 0 and (p["mode"], p["mid_fast"], p["slow_grid"], p["pmax"]) == (mode, mid_fast, grid, pmax), (name, p)
    assert {(name, w[1], w[2]) for (name, _), w in zip(fams, want)} == {("probes", 1, 1), ("list", 1, 1), ("slots", 1, 1), ("batches", 0, 0), ("fast", 1, 1),
                                                                      ("plain", 2, 0), ("second", 1, 1)}
