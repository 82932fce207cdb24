"""The seed index itself (vstrains_amd/csrc/vs_index.hip), exported with vs_index_export and compared with its host
statement (seed_index_model.py), and the three parts of it random inputs do not reach: probe chains that wrap round the
end of the table, seeds that are in no node and walk a whole chain, and different 63-base seeds that share a key (k >= 95),
where only the comparison from the seed's first base (VS_SEED_VERIFIED) keeps the links right.  Every comparison is exact;
every index is built with renumber=False, so that node numbers in the export are the test's own."""
import numpy as np
import pytest

from oracle import pe_oracle_c
import seed_extend_model as model
import seed_index_model as sim

pytestmark = pytest.mark.gpu


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
    """A context in experiment mode: the tuning switches of vs_pe_count are live on it (conftest.experiment_context)."""
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


# ---- 4.1 the built index equals the model ----------------------------------------------------------------------------
def _node_set(k, rng):
    K = k + 1
    lens = [0, 1, 15, 16, 17, 31, 32, 33, K - 1, K, K + 1, 2 * K + 5, 300, 457]
    seqs = []
    for i, n in enumerate(lens):
        seqs.append(sim.random_seq(rng, n))
        if i % 3 == 2:
            seqs.append(sim.random_seq(rng, max(K - 2, 0)))  # a node below K between indexed ones: equal neighbours in seed_off
    twin = sim.random_seq(rng, K + 40)
    seqs += [twin, twin, sim.random_seq(rng, max(K - 1, 0)), sim.rc(twin)]  # the same text twice, and next to its reverse complement
    seqs += ["A" * 1100, "T" * 300, "AC" * 1100, "GT" * 90 + "G"]  # one seed with > 1 000 postings each, on both strands
    if K % 2 == 0:  # palindromic (k+1)-windows: equal to their own reverse complement (the seeds inside, w odd, are not)
        h = sim.random_seq(rng, K // 2)
        seqs += [h + sim.rc(h), sim.random_seq(rng, 7) + h + sim.rc(h) + sim.random_seq(rng, 9)]
    seqs += ["", sim.random_seq(rng, K + 3)]
    return seqs


@pytest.mark.parametrize("k", [1, 2, 14, 15, 16, 29, 30, 31, 32, 55, 94, 95, 96, 127, 150])
def test_built_index_equals_the_host_statement(host, ctx, k):
    seqs = _node_set(k, np.random.default_rng(4100 + k))
    m = sim.build(seqs, k)
    ctx.build_index(seqs, k, renumber=False)
    info, exp = ctx.index_info, ctx.index_export()
    # the packed texts of both strands, their pad words, the node headers
    assert exp["fwd"].size == exp["rc"].size == m["n_words"] + sim.PAD_WORDS
    assert np.array_equal(exp["fwd"], m["fwd"]) and np.array_equal(exp["rc"], m["rc"])
    assert not exp["fwd"][m["n_words"]:].any() and not exp["rc"][m["n_words"]:].any()
    assert np.array_equal(exp["meta"], m["meta"])
    # geometry and sizes
    assert (info["seed_len"], info["stride"]) == (m["w"], m["s"]) == model.geometry(k + 1)
    assert info["seed_positions"] == m["seed_positions"] == exp["postings"].shape[0]
    assert info["distinct_seeds"] == m["distinct"]
    assert info["slots"] == m["slots"] == exp["slot_key"].size == 1 << exp["table_bits"]
    # keys and postings
    table = sim.read_table(exp)
    assert set(table) == set(m["postings"])
    ranges, singles = [], 0
    for key, want in m["postings"].items():
        multi, got = table[key]
        assert sorted(got) == sorted(want), key
        assert multi == (len(want) > 1), key
    occupied = np.nonzero(exp["slot_key"] != np.uint64(sim.EMPTY_KEY))[0]
    for sl in occupied:
        raw, a, b = int(exp["slot_key"][sl]), int(exp["slot_a"][sl]), int(exp["slot_b"][sl])
        assert raw >> 63 == 0
        if raw & sim.MULTI_BIT:  # (first posting, count)
            assert b >= 2
            ranges.append((a, a + b))
        else:  # a = node, b = pos | strand << 31
            (node, pos, strand, _, _), = m["postings"][raw]
            assert (a, b) == (node, pos | strand << 31)
            singles += 1
    ranges.sort()
    assert all(lo >= 0 and hi <= m["seed_positions"] for lo, hi in ranges)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert sum(hi - lo for lo, hi in ranges) + singles == m["seed_positions"]
    assert max([hi - lo for lo, hi in ranges] + [0]) > 1000
    # every key is reachable from its home slot without crossing an empty slot; the occupied slots are linear probing's
    assert set(int(x) for x in occupied) == m["occupied"]
    mask = m["slots"] - 1
    for sl in occupied:
        key = int(exp["slot_key"][sl]) & ~sim.MULTI_BIT
        at = sim.slot_of(key, m["bits"])
        while at != sl:
            assert int(exp["slot_key"][at]) != sim.EMPTY_KEY, (key, at)
            at = (at + 1) & mask


# ---- blocks of read ends against the oracle --------------------------------------------------------------------------
def _count_and_compare(host, c, orc, n_nodes, ends, K, lists=True, memo=None):
    """Every end once as a forward and once as a reverse read (the list rotated by three): counters, stats and the per-end
    lists against the C oracle (``memo``: a dict that keeps the oracle's answers for these ends between variants).
    -> (kernel name of the counting run, its timing, its VS_RAN_* bits)"""
    memo = {} if memo is None else memo
    fwd = list(ends)
    rve = fwd[3:] + fwd[:3]
    if "want" not in memo:
        memo["want"] = orc.count_pairs(fwd, rve)
    want = memo["want"]
    counter = host.PeCounter(c)
    block = c.pack_pairs(fwd, rve)
    counter.add(block)
    node_mat, short_mat, stats = counter.result()
    ran = (c.last_kernel, c.last_timing(), c.last_launched)
    assert np.array_equal(node_mat, want[0]) and np.array_equal(short_mat, want[1])
    assert stats == tuple(int(x) for x in want[2])
    if lists:
        got = c.map_ends(block, cap=max(n_nodes, 1))
        if "lists" not in memo:
            memo["lists"] = [orc.map_end(read) for read in fwd]
        want_lists = memo["lists"]
        for e, read in enumerate(fwd):
            # (a pair with an end below K bases is not mapped at all, PE_Inference.py:160-163: both lists stay empty)
            used = len(read) >= K and len(rve[e]) >= K
            assert got[2 * e] == (want_lists[e] if used else []), (e, read)
            assert got[2 * e + 1] == (want_lists[(e + 3) % len(fwd)] if used else []), (e, rve[e])
    return ran


VARIANTS = [  # (context, environment, what last_kernel must be for a block of one compile-time shape `shape`)
    ("ctx", {}, lambda name, shape: name.startswith("k_pe_tiles<" + shape)),
    ("xctx", {"VS_NO_STD": "1"}, lambda name, shape: name == "k_pe_tiles<%s, 0u, 0u>" % shape[0]),
    ("xctx", {"VS_NO_FAST": "1"}, lambda name, shape: name == "k_pe_tiles<0, 0u, 0u>"),
    ("xctx", {"VS_ADAPT_GRID": "1"}, lambda name, shape: name.startswith("k_pe_tiles<" + shape) and name.endswith(", true>")),
    ("xctx", {"VS_ADAPT_GRID": "0"}, lambda name, shape: name.startswith("k_pe_tiles<" + shape) and not name.endswith(", true>")),
]


# ---- 4.2 chains and wrap-round, exact keys ---------------------------------------------------------------------------
def _chain_graph(k, rng):
    """Nodes whose seeds include nine keys with home slots in the last three slots of the table (a run of occupied slots
    from there across slot 0) and thirteen keys on one home slot in mid-table.  k = 30: the nodes ARE the seeds (K = w =
    31); k = 55: every planted seed sits in the middle of a node of 201 bases.  The table size is the model's for the
    finished graph; a draw that changes it is made again."""
    K = k + 1
    w, s = sim.geometry(K)
    flank = 0 if K == w else 85

    def wrap(q):
        return sim.random_seq(rng, flank) + q + sim.random_seq(rng, flank)

    filler = [sim.random_seq(rng, 2 * flank + w) for _ in range(40 if flank == 0 else 10)]
    bits = sim.build([wrap(sim.random_seq(rng, w)) for _ in range(22)] + filler, k)["bits"]
    for _ in range(8):
        n_slots = 1 << bits
        planted, keys = [], set()
        for slot, n in ((n_slots - 3, 3), (n_slots - 2, 3), (n_slots - 1, 3), (n_slots // 2, 13)):
            got = sim.seeds_with_home_slot(w, bits, slot, n, rng, avoid=keys)
            keys.update(sim.seed_key(q)[0] for q in got)
            planted += [(q, slot) for q in got]
        seqs = [wrap(q) for q, _ in planted] + filler
        m = sim.build(seqs, k)
        if m["bits"] == bits:
            return seqs, planted, flank, m
        bits = m["bits"]
    raise AssertionError("the table size did not settle")


def _chain_case(host, c, k, rng):
    seqs, planted, flank, m = _chain_graph(k, rng)
    c.build_index(seqs, k, renumber=False)
    exp = c.index_export()
    n_slots = m["slots"]
    # non-vacuity, on the exported table: the size is the predicted one, the planted keys are in it, and the two runs exist
    assert c.index_info["slots"] == n_slots == exp["slot_key"].size
    occupied = set(int(x) for x in np.nonzero(exp["slot_key"] != np.uint64(sim.EMPTY_KEY))[0])
    assert occupied == m["occupied"]
    table = sim.read_table(exp)
    assert all(sim.seed_key(q)[0] in table for q, _ in planted)
    runs = sim.runs(occupied, n_slots)
    wrapping = [r for r in runs if r[0] + r[1] > n_slots]
    assert len(wrapping) == 1 and wrapping[0][1] >= 8 and wrapping[0][0] <= n_slots - 3, runs
    middle = [r for r in runs if r[0] <= n_slots // 2 < r[0] + r[1]]
    assert len(middle) == 1 and middle[0][1] >= 12, runs
    # seeds that are in no node and start at the first slot of either run: they walk the whole chain to an empty slot
    misses = []
    for start, _ in (wrapping[0], middle[0]):
        misses += sim.seeds_with_home_slot(m["w"], m["bits"], start, 3, rng, avoid=set(m["postings"]))
    assert all(sim.seed_key(q)[0] not in table for q in misses)
    return seqs, planted, flank, m, misses


def test_probe_chains_across_the_end_of_the_table_k30(host, ctx, xctx, monkeypatch):
    """K = w = 31: a node of 31 bases holds exactly one seed and a read of 31 bases makes exactly one probe."""
    rng = np.random.default_rng(4230)
    k = 30
    seqs, planted, _, m, misses = _chain_case(host, ctx, k, rng)
    ends = []
    for q, _ in planted:
        ends += [q, sim.rc(q), sim.sub_at(q, int(rng.integers(0, 31))), sim.rc(sim.sub_at(q, int(rng.integers(0, 31))))]
    for q in misses:
        ends += [q, sim.rc(q)]
    ends += [seqs[-1], sim.rc(seqs[-2])]
    orc = pe_oracle_c.Oracle(seqs, k)
    assert sum(len(orc.map_end(e)) for e in ends) == 2 * len(planted) + 2
    memo = {}
    name, _, _ = _count_and_compare(host, ctx, orc, len(seqs), ends, k + 1, memo=memo)
    assert name == "k_pe_tiles<1, 0u, 0u>"
    xctx.build_index(seqs, k, renumber=False)
    with monkeypatch.context() as mp:
        mp.setenv("VS_NO_FAST", "1")
        name, _, _ = _count_and_compare(host, xctx, orc, len(seqs), ends, k + 1, memo=memo)
    assert name == "k_pe_tiles<0, 0u, 0u>"


@pytest.mark.parametrize("rlen,shape", [(150, "1, 10u, 4u"), (100, "1, 7u, 2u")])
def test_probe_chains_across_the_end_of_the_table_k55(host, ctx, xctx, monkeypatch, rlen, shape):
    """The planted seeds inside nodes of 201 bases; the reads are windows of those nodes at every start that holds the seed,
    exact, one substitution away, and with the seed replaced by one that is in no node and starts at the head of a run."""
    rng = np.random.default_rng(4255)
    k = 55
    seqs, planted, flank, m, misses = _chain_case(host, ctx, k, rng)
    w, s = m["w"], m["s"]
    ends, on_grid = [], 0
    for i, (q, _) in enumerate(planted):
        text = seqs[i]
        for st in range(max(0, flank + w - rlen), min(flank, len(text) - rlen) + 1):
            win = text[st: st + rlen]
            o = flank - st
            on_grid += o >= model.phase(rlen, w, s) and (o - model.phase(rlen, w, s)) % s == 0
            miss = win[:o] + misses[(i + st) % len(misses)] + win[o + w:]
            sub = sim.sub_at(win, int(rng.integers(0, rlen)))
            for e in (win, sub, miss):
                ends.append(e if (st + i) % 2 else sim.rc(e))
                ends.append(sim.rc(e) if (st + i) % 3 == 0 else e)
    assert on_grid >= len(planted)  # (every planted seed is probed exactly, by some read, on the production grid)
    orc = pe_oracle_c.Oracle(seqs, k)
    xctx.build_index(seqs, k, renumber=False)
    memo = {}
    for which, env, kernel_ok in VARIANTS:
        c = ctx if which == "ctx" else xctx
        with monkeypatch.context() as mp:
            for key, v in env.items():
                mp.setenv(key, v)
            name, _, _ = _count_and_compare(host, c, orc, len(seqs), ends, k + 1, lists=not env or "VS_NO_FAST" in env, memo=memo)
        assert kernel_ok(name, shape), (env, name)


# ---- 4.3 shared keys, 63-base seeds ----------------------------------------------------------------------------------
def _canon(q):
    r = sim.rc(q)
    return q if sim.seq_int(q) < sim.seq_int(r) else r


SHARED_VARIANTS = [("ctx", {}), ("xctx", {"VS_NO_STD": "1"}), ("xctx", {"VS_NO_FAST": "1"}), ("xctx", {"VS_NO_MID": "1"}),
                   ("xctx", {"VS_ADAPT_GRID": "1"})]


@pytest.mark.parametrize("k", [95, 127, 140])
def test_different_seeds_under_one_key(host, ctx, xctx, monkeypatch, k):
    """Twins (only the seed's own bases tell two nodes apart), an orphan (the read's seed is in no node, its key is),
    three seeds on one key with one stored reverse-complemented, the shared seed flush with a node's end, and a seed in a
    hundred nodes next to a colliding one in a single node -- seed_index_model.shared_key_scenarios.  Reads: windows of the
    source texts at EVERY start across more than 2 s positions, both strands, so that any exact grid of stride s puts a
    probe on the shared seed; K, K + 1, 250 bases, 2 x 241..256, a ragged set; then with a byte outside ACGT outside the
    seed and inside its bases 32..62."""
    rng = np.random.default_rng(4300 + k)
    sc = sim.shared_key_scenarios(k, rng)
    K, w, s, seqs = sc["K"], sc["w"], sc["s"], sc["seqs"]
    assert w == 63 and all(len(q) >= K for q in seqs)
    m = sim.build(seqs, k)
    ctx.build_index(seqs, k, renumber=False)
    xctx.build_index(seqs, k, renumber=False)
    orc = pe_oracle_c.Oracle(seqs, k)

    # non-vacuity on the exported table: the planted keys are shared by different 63-mers
    table = sim.read_table(ctx.index_export())
    in_graph = {}
    for i, q in enumerate(seqs):
        for p in range(len(q) - w + 1):
            in_graph.setdefault(_canon(q[p: p + w]), []).append((i, p))
    collisions = 0
    for name, groups in sc["groups"].items():
        for g in groups:
            keys = {sim.seed_key(q)[0] for q in g}
            assert len(keys) == 1 and len({_canon(q) for q in g}) == len(g)
            multi, postings = table[keys.pop()]
            stored = {_canon(seqs[n][p: p + w]) for n, p, _, _, _ in postings}
            present = {_canon(q) for q in g if _canon(q) in in_graph}
            assert stored == present
            if name == "orphan":  # the read's seed is not in the graph; the slot its key leads to holds the other seed alone
                assert not multi and len(present) == 1 and _canon(g[1]) not in in_graph
            else:
                assert multi and len(present) == len(g) >= 2
            collisions += len(present) - 1
    assert ctx.index_info["distinct_seeds"] == len(in_graph) - collisions == m["distinct"]

    blocks = [("K", sim.scenario_reads(sc, [K])), ("K+1", sim.scenario_reads(sc, [K + 1])), ("250", sim.scenario_reads(sc, [250])),
              ("241..256", sim.scenario_reads(sc, list(range(241, 257)), cycle=True)),
              ("ragged", sim.scenario_reads(sc, [int(x) for x in rng.integers(K - 3, 301, size=23)], cycle=True))]

    # non-vacuity on the reads: on the production grid (vs_seed_phase) and on every step grid t, some read of every
    # scenario has a probe exactly on the shared seed; and some such read of a twin B is B's alone for the oracle
    twin_b_alone = 0
    for label, reads in blocks[:3]:
        rlen = len(reads[0][0])
        grids = [set(range(model.phase(rlen, w, s), rlen - w + 1, s))] + [set(model.step_grid(rlen, w, s, t)) for t in range(max(1, (rlen - w + 1) // s) + 1)]
        for name in sc["groups"]:
            for grid in grids:
                assert any(o in grid for _, nm, o, _ in reads if nm == name and o is not None), (label, name)
        for read, nm, o, si in reads:
            if nm == "twins" and si % 2 == 1 and o in grids[0]:
                b, = sc["sources"][si][3]
                a, = sc["sources"][si - 1][3]
                got = orc.map_end(read)
                twin_b_alone += b in got and a not in got
    assert twin_b_alone > 0

    shape4 = k == 127  # (the compile-time shape of the long-window kernel: k = 127, 2 x 241..256)
    for label, reads in blocks:
        passes = [("clean", reads), ("dirty outside", sim.dirty_reads(reads, w, rng, inside=False)),
                  ("dirty inside", sim.dirty_reads(reads, w, rng, inside=True))]
        for pass_name, rd in passes:
            ends = [r[0] for r in rd]
            memo = {}
            for which, env in SHARED_VARIANTS:
                c = ctx if which == "ctx" else xctx
                with monkeypatch.context() as mp:
                    for key, v in env.items():
                        mp.setenv(key, v)
                    name, timing, launched = _count_and_compare(host, c, orc, len(seqs), ends, k + 1, lists=not env and pass_name != "dirty outside", memo=memo)
                # the intended instantiation ran (reads of up to 256 bases are within the long-window kernel's reach at these k)
                if pass_name != "clean":
                    continue
                if "VS_NO_FAST" in env:
                    assert name == "k_pe_tiles<0, 0u, 0u>", (label, env, name)
                elif shape4 and label in ("250", "241..256") and "VS_NO_STD" not in env:
                    assert name.startswith("k_pe_tiles<2, 16u, 2u") and name.endswith(", true>") == ("VS_ADAPT_GRID" in env), (label, env, name)
                elif label != "ragged":
                    assert name == "k_pe_tiles<2, 0u, 0u>", (label, env, name)
                # the crowd: ends accepted by a hundred nodes leave the main kernel for k_pe_mid, and k_pe_slow behind it
                if label in ("K", "K+1"):
                    assert timing["slow_pairs"] > 0, (label, env)
                    assert bool(launched & c.RAN_PE_MID) == ("VS_NO_MID" not in env), (label, env)
