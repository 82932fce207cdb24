"""The constructed family of tests/pe_extension_cases.py without a device: per shape the string model, the Python oracle and
the C oracle agree on every end; the family is balanced, means what it says, reaches the window edges of the device's
comparison (read off the model's trace), and changes its answer under five off-by-one mutants of the comparison that a
block of random reads with substitutions does not all notice.  What the device makes of it: tests/test_pe_extension_gpu.py."""
import functools

import pytest

import pe_extension_cases as pec
import seed_extend_model as model
from oracle import pe_oracle, pe_oracle_c

MODE1 = [(55, 100), (55, 112), (55, 128), (55, 150), (31, 191), (21, 90), (55, 191)]
MODE2 = [(127, 256), (127, 317), (94, 287), (140, 299), (31, 287)]
MODE0 = [(140, 330)]  # (what the plan makes of 330-base reads at k = 140: beyond the long-window kernel's 256 bases)
assert sorted(MODE1 + MODE2 + MODE0) == sorted(pec.SHAPES)

EDGES1 = (32, 48, 64, 96, 112, 128)
EDGES2 = EDGES1 + (160, 176, 192, 224)
# ``ext`` values next to a window edge or sentinel of the device's comparison that no threshold case reaches, and why: no
# shape the plan sends to that mode puts the threshold there -- MODE 1 ends at reads of 191 bases (the longest threshold
# match, 31-base seed included, is 165 bases at k = 31: ext <= 134; `far` = 160 is reached by the full matches only), MODE 2
# at 256 bases behind the first probe (the longest threshold matches: ext <= 226 at k = 31 / 287; 240 is where the last
# text word is loaded, 256 the sentinel: the full matches reach them).  Not to grow without a reason written here.
UNREACHED_EXT = {1: (159, 160, 161), 2: (239, 240, 241, 255, 256, 257)}
REM1 = (48, 49, 64, 65, 112, 113)
REM2 = REM1 + (176, 177, 240, 241)

MUTANTS = {
    "left - 1 when left > 0": lambda left, ext: (left - 1 if left > 0 else left, ext),
    "left + 1 when left == 5": lambda left, ext: (left + 1 if left == 5 else left, ext),
    "ext - 1 when ext >= 64": lambda left, ext: (left, ext - 1 if ext >= 64 else ext),
    "ext + 1 when ext == 32": lambda left, ext: (left, ext + 1 if ext == 32 else ext),
    "ext capped at 96": lambda left, ext: (left, min(ext, 96)),
}


@functools.lru_cache(maxsize=None)
def traced(k, rlen):
    """The family of a shape with the model's answer and trace of every case read (computed once, shared, not changed)."""
    fam = pec.knife_edge_family(k, rlen, pec.SHAPES[(k, rlen)]["step"])
    K, w, s, seqs = fam["K"], fam["w"], fam["s"], fam["seqs"]
    table, _, _ = model.build(seqs, K)
    rcs = [model.rc(x) for x in seqs]
    ctx = dict(fam=fam, table=table, rcs=rcs, got=[], trace=[])
    for p in range(len(fam["cases"])):
        tr = []
        ctx["got"].append(model.map_end(pec.case_read(fam, p), seqs, rcs, table, w, s, K, verified=model.seed_verified(w), trace=tr))
        ctx["trace"].append(tr)
    return ctx


def threshold_matches(k, rlen, kept):
    """The credited matches of the cut cases whose node ended with v in {T - 1, T} and was accepted (``kept``) or rejected."""
    t = traced(k, rlen)
    out = []
    for c, tr in zip(t["fam"]["cases"], t["trace"]):
        if c["kind"] != "cut":
            continue
        verdict = [r for r in tr if "v" in r and r["node"] == c["node"]]
        if len(verdict) == 1 and verdict[0]["v"] in (verdict[0]["T"] - 1, verdict[0]["T"]) and verdict[0]["kept"] == kept:
            out += [(c, r) for r in tr if "j" in r and r["credited"] and r["node"] == c["node"]]
    return out


@pytest.mark.parametrize("k,rlen", MODE1 + MODE2 + MODE0)
def test_model_and_both_oracles_agree_and_the_family_is_what_it_says(k, rlen):
    t = traced(k, rlen)
    fam = t["fam"]
    K, seqs, cases = fam["K"], fam["seqs"], fam["cases"]
    assert len(cases) <= 4000 and len(seqs) <= 4001 and max(len(x) for x in seqs) <= 330
    tab = pe_oracle.build_table(seqs, K)
    lens = [len(x) for x in seqs]
    orc = pe_oracle_c.Oracle(seqs, k)
    accepted = rejected = off = 0
    for p, c in enumerate(cases):
        read = pec.case_read(fam, p)
        want = pe_oracle.map_read_end(read, tab, lens, K)
        assert t["got"][p] == want == orc.map_end(read), (p, c)
        mate = (fam["fwd"] if c["end"] else fam["rve"])[p]
        assert orc.map_end(mate) == [fam["anchor"]]
        assert set(want) <= {c["node"], c["node"] + 1}  # (the next node only through the text behind this one)
        if c["kind"] == "full":
            assert (c["node"] in want) == c["accept"]
            continue
        accepted += c["node"] in want
        rejected += c["node"] not in want
        off += (c["node"] in want) != c["accept"]
    n = accepted + rejected
    print("k=%d rlen=%d: %d pairs, %d nodes, cut cases %d accepted / %d rejected, %d against the intent" % (k, rlen, len(cases), len(seqs), accepted, rejected, off))
    assert n > 100 and accepted >= 0.4 * n and rejected >= 0.4 * n, (accepted, rejected)
    assert off <= 0.02 * n, (off, n)
    # every variation is there, on both sides of the threshold
    cuts = [c for c in cases if c["kind"] == "cut"]
    for acc in (True, False):
        some = [c for c in cuts if c["accept"] == acc]
        assert {c["xor"] for c in some} == {0, 1, 2, 3} and {c["strand"] for c in some} == {0, 1} and {c["end"] for c in some} == {0, 1}
        assert {c["side"] for c in some} == {"R", "L"} and any(c["byte"] == "N" for c in some) and any(c["byte"] not in ("", "N") for c in some)
        assert any(c["behind"] and c["strand"] == st for c in some for st in (0, 1)) and any(c["extra"] for c in some)
    assert all(pec.dirty_bytes(pec.case_read(fam, p)) > 4 for p, c in enumerate(cases) if c["extra"])


def _coverage(shapes, kept):
    left, cs, ext, rem, lit, ra, rq = {}, set(), set(), set(), set(), set(), set()
    for k, rlen in shapes:
        s = traced(k, rlen)["fam"]["s"]
        for c, r in threshold_matches(k, rlen, kept):
            left.setdefault((k, rlen), set()).add(r["left"])
            if s > 32:
                cs.add(r["c"])
            ext.add(r["ext"])
            rem.add(r["rem"])
            lit.add(r["rem"] + model.seed_verified(traced(k, rlen)["fam"]["w"]) - traced(k, rlen)["fam"]["w"])  # min(rlen - j - w, tlen - q - w)
            ra.add((r["j"] - r["left"]) % 16)  # the match's start in the read
            rq.add(r["q"] % 16)  # the seed's offset in the node text
    return left, cs, ext, rem, lit, ra, rq


@pytest.mark.parametrize("mode,shapes,edges,rems", [(1, MODE1, EDGES1, REM1), (2, MODE2, EDGES2, REM2)])
@pytest.mark.parametrize("kept", [True, False], ids=["accepted", "rejected"])
def test_threshold_cases_reach_every_window_edge(mode, shapes, edges, rems, kept):
    left, cs, ext, rem, lit, ra, rq = _coverage(tuple(shapes), kept)
    for k, rlen in shapes:
        s = traced(k, rlen)["fam"]["s"]
        assert left[(k, rlen)] >= set(range(s)), (k, rlen, sorted(set(range(s)) - left[(k, rlen)]))
    if mode == 2:
        assert cs >= {32, 33, 64, 65}, sorted(cs)
    want = {e + d for e in edges for d in (-1, 0, 1)}
    print("mode %d %s: ext %d..%d, rem %d..%d" % (mode, "accepted" if kept else "rejected", min(ext), max(ext), min(rem), max(rem)))
    assert ext >= want, sorted(want - ext)
    assert not ext & set(UNREACHED_EXT[mode]), sorted(ext & set(UNREACHED_EXT[mode]))
    # what is left from where the comparison starts (the device's `rem`), and what is left behind the seed: one number
    # for the verified 31-base seeds, 63 apart for the 63-base ones
    assert rem >= set(rems), sorted(set(rems) - rem)
    assert lit >= set(rems), sorted(set(rems) - lit)
    assert ra == set(range(16)) and rq == set(range(16))


def _changed_ends(reads, seqs, K, w, s, table, rcs, base, hook):
    v = model.seed_verified(w)
    return sum(model.map_end(r, seqs, rcs, table, w, s, K, verified=v, hook=hook) != b for r, b in zip(reads, base))


def test_off_by_one_mutants_change_the_family_and_not_all_of_them_a_random_block():
    """Five mutants of what the comparison finds (``hook`` of the model).  Each changes the list of some end of the family, taken
    over the shapes whose stride reaches left == 5 (26 and more; one shape need not see them all: a 100-base read at k = 55
    has no threshold match with ext >= 32).  The block the random-read tests of tests/test_pe_gpu.py are
    made like -- _dense_case(55, 2000, 100, snp=0.03): reads with 1 % substitutions off six strains -- lets at least one of
    them pass on every end; which, is printed and recorded in the assertion."""
    from vstrains_amd import synth

    total = dict.fromkeys(MUTANTS, 0)
    for k, rlen in MODE1 + MODE2:
        t = traced(k, rlen)
        fam = t["fam"]
        if fam["s"] < 26:
            continue
        reads = [pec.case_read(fam, p) for p in range(len(fam["cases"]))]
        for name, hook in MUTANTS.items():
            n = _changed_ends(reads, fam["seqs"], fam["K"], fam["w"], fam["s"], t["table"], t["rcs"], t["got"], hook)
            print("k=%d rlen=%d  %-24s changes %d of %d ends" % (k, rlen, name, n, len(reads)))
            total[name] += n
    assert min(total.values()) > 0, total
    st = synth.make_strains(6, 1500, 0.03, seed=455)
    g = synth.compact_dbg(st, 55)
    f, r = synth.sample_pairs(st, 2000, 100, seed=456, sub_rate=0.01, n_rate=0.02)
    K, (w, s) = 56, model.geometry(56)
    table, _, _ = model.build(g.seqs, K)
    rcs = [model.rc(x) if len(x) >= K else "" for x in g.seqs]
    reads = [x for x in f + r if len(x) >= K]
    base = [model.map_end(x, g.seqs, rcs, table, w, s, K) for x in reads]
    seen = {name: _changed_ends(reads, g.seqs, rcs=rcs, K=K, w=w, s=s, table=table, base=base, hook=hook) for name, hook in MUTANTS.items()}
    print("random block of %d ends: %s" % (len(reads), seen))
    assert min(seen.values()) == 0, seen


def test_the_plan_sends_every_shape_to_the_kernel_it_was_chosen_for():
    """vs_pe_plan (csrc/vs_pe_plan.h through oracle/plan_check.cpp, as tests/test_pe_plan_cpu.py runs it) on each block's
    scalars: the instantiation pec.SHAPES names, MODE 0 under VS_NO_FAST=1, and the run-time shape of the same mode under
    VS_NO_STD=1 -- what tests/test_pe_extension_gpu.py then asserts of the kernel that ran."""
    import ctypes as C
    import os
    import subprocess

    import numpy as np

    import test_pe_plan_cpu as tp

    path = os.path.join(tp.ROOT, "oracle", "_build", "libvs_plan_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(tp.ROOT, "oracle")])
    lib = C.CDLL(path)
    lib.vs_pe_plan_check.restype = C.c_int
    lib.vs_pe_plan_check.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    rows, want = [], []
    for (k, rlen), sh in pec.SHAPES.items():
        t = traced(k, rlen)
        fam = t["fam"]
        seqs, w = fam["seqs"], fam["w"]
        base = dict(tp.DEFAULTS, n_nodes=len(seqs), K=fam["K"], w=w, s=fam["s"], n_seed_pos=sum(len(x) - w + 1 for x in seqs),
                    n_distinct=len(t["table"]), max_node_len=max(len(x) for x in seqs), n_ends=2 * len(fam["fwd"]), max_len=rlen,
                    has_mask=1, has_inv4=1)
        for tune, name in ((dict(), sh["kernel"][len("k_pe_tiles"):] + ">"), (dict(no_fast=1), "<0, 0u, 0u>"),
                           (dict(no_std=1), sh["kernel"][len("k_pe_tiles"):len("k_pe_tiles<1")] + ", 0u, 0u>")):
            rows.append([dict(base, **tune)[f] for f in tp.IN])
            want.append(((k, rlen), tune, name))
    a = np.array(rows, dtype=np.int64)
    out = np.zeros((len(rows), len(tp.OUT)), dtype=np.uint64)
    msgs = C.create_string_buffer(128 * len(rows))
    assert lib.vs_pe_plan_check(len(rows), a.ctypes.data, out.ctypes.data, msgs) == len(tp.OUT)
    for o, (shape, tune, name) in zip(out.astype(np.int64).tolist(), want):
        p = dict(zip(tp.OUT, o))
        assert p["status"] == 0 and tp.name(p) == name, (shape, tune, tp.name(p), name)
