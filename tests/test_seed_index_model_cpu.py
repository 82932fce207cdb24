"""The host statement of the seed index (seed_index_model.py) against itself, and the algorithm model
(seed_extend_model.py) with the device's 63-base seeds, mixed keys and "compare from the seed's first base" rule against
the oracle -- on graphs around the switch to 63-base seeds and on constructed seeds that share a key.  CPU only."""
import random

import numpy as np
import pytest

from oracle import pe_oracle
import seed_extend_model as model
import seed_index_model as sim


def test_unmix64_inverts_mix64():
    rng = random.Random(3)
    for z in [0, 1, 2 ** 64 - 1, 2 ** 63, 0x9E3779B97F4A7C15] + [rng.getrandbits(64) for _ in range(2000)]:
        assert sim.unmix64(sim.mix64(z)) == z
        assert sim.mix64(sim.unmix64(z)) == z


def test_geometry_is_the_devices_for_every_k():
    for K in range(2, 400):
        w, s = sim.geometry(K)
        assert (w, s) == model.geometry(K)
        assert w % 2 == 1 and w <= K and s == K - w + 1
        assert w == (63 if K >= 96 else 31 if K >= 31 else K if K % 2 else K - 1)


def test_constructed_seeds_share_a_key_and_are_different_seeds():
    rng = np.random.default_rng(11)
    for _ in range(20):
        x = sim.random_seq(rng, 63)
        ys = sim.colliding_seeds(x, 10, rng)
        group = [x] + ys
        assert len({sim.seed_key(q)[0] for q in group}) == 1
        for i, a in enumerate(group):
            assert sim.seed_key(sim.rc(a)) == (sim.seed_key(a)[0], 1 - sim.seed_key(a)[1])  # (either strand, one key)
            for b in group[i + 1:]:
                assert a != b and a != sim.rc(b)


def test_packing_and_keys_restate_the_bit_layout():
    assert sim.pack_words("C").tolist() == [1] and sim.pack_words("ACGT" * 4 + "T").tolist() == [0xE4E4E4E4, 3]
    assert sim.pack_words("").size == 0
    assert sim.seq_int("CA") == 1 and sim.seq_int("AC") == 4 and sim.int_seq(0b1110, 2) == "GT"
    # w <= 31: the smaller of the two values, strand 1 when that is the reverse complement
    assert sim.seed_key("AAC") == (sim.seq_int("AAC"), 0) and sim.seed_key("TTT") == (0, 1)
    # w = 63: compared as 126-bit values, base 62 the most significant
    x = "C" + "A" * 62  # (value 1; its reverse complement T..TG holds the largest codes at the top)
    assert sim.seed_key(x)[1] == 0 and sim.seed_key(sim.rc(x)) == (sim.seed_key(x)[0], 1)
    y = "A" * 32 + "C" + "A" * 30  # differs from A..A in the upper half only: bit 64
    assert sim.seq_int(y) == 1 << 64 and sim.seed_key(y)[0] == sim.mix64(sim.mix64(1 + sim.KEY_SALT)) >> 2
    assert sim.table_bits(0) == 4 and sim.table_bits(1) == 4 and sim.table_bits(2) == 5 and sim.table_bits(4095) == 15


def test_slot_targeted_seeds_have_the_home_slot_asked_for():
    rng = np.random.default_rng(12)
    for w, bits, slot in ((31, 9, 511), (31, 9, 0), (31, 12, 2048), (15, 6, 63), (29, 10, 1022)):
        seeds = sim.seeds_with_home_slot(w, bits, slot, 12, rng)
        keys = [sim.seed_key(q)[0] for q in seeds]
        assert len(set(keys)) == 12 and all(len(q) == w for q in seeds)
        assert all(sim.slot_of(key, bits) == slot for key in keys)
        # twelve keys on one home slot: a run of twelve slots from it, round the end of the table where it is the last
        placed = sim.occupied_slots(keys, bits)
        assert sorted(placed.values()) == sorted((slot + i) % (1 << bits) for i in range(12))
        assert sim.runs(placed.values(), 1 << bits) == [(slot, 12)]
        assert set(sim.occupied_slots(reversed(keys), bits).values()) == set(placed.values())  # (any insertion order)


def _device_rules(K):
    """(key function, verified) as the device has them for this K: exact keys and a seed taken for granted up to w = 31,
    the mixed key and a comparison from the seed's first base for w = 63 (VS_SEED_VERIFIED, csrc/vs_internal.h)."""
    w, _ = model.geometry(K)
    if w <= 31:
        return None, w
    return (lambda c: sim.seed_key(c)[0]), 0


def _check_every_grid(read, seqs, rcs, mtab, w, s, K, want, key_fn, verified, ctx):
    """every probe phase and every step grid of the model == the oracle's list"""
    rlen = len(read)
    if rlen < K:
        return
    assert model.map_end(read, seqs, rcs, mtab, w, s, K, key_fn=key_fn, verified=verified) == want, (ctx, read)
    for first in range(s):
        assert model.map_end(read, seqs, rcs, mtab, w, s, K, first=first, key_fn=key_fn, verified=verified) == want, (ctx, first, read)
    n = max(1, (rlen - w + 1) // s)
    for t in range(n + 1):
        grid = model.step_grid(rlen, w, s, t)
        assert model.map_end(read, seqs, rcs, mtab, w, s, K, grid=grid, key_fn=key_fn, verified=verified) == want, (ctx, t, read)


@pytest.mark.parametrize("k", [94, 95, 96, 127, 140])
def test_model_with_the_devices_seeds_equals_oracle_on_graphs(k):
    """k = 94 is the last 31-base geometry, 95 the first with 63-base seeds (K = 96).  A genome cut into overlapping nodes,
    a variant of it, a reverse-complemented node; reads of many lengths, exact, from the variant, with one odd byte."""
    K = k + 1
    rng = random.Random(k)
    G = 1400
    genome = "".join(rng.choice("ACGT") for _ in range(G))
    var = list(genome)
    for p in range(40, G, 97):
        var[p] = {"A": "C", "C": "G", "G": "T", "T": "A"}[var[p]]
    var = "".join(var)
    seqs = [genome[i:i + K + 40] for i in range(0, G - K - 40, 35)] + [var[i:i + K + 30] for i in range(5, G - K - 30, 61)]
    seqs.append(model.rc(genome[300:300 + K + 5]))
    seqs.append(genome[10:10 + K - 1])  # (shorter than K: not indexed)
    tab = pe_oracle.build_table(seqs, K)
    lens = [len(x) for x in seqs]
    key_fn, verified = _device_rules(K)
    mtab, w, s = model.build(seqs, K, key_fn=key_fn)
    assert (w, s) == sim.geometry(K) and w == (31 if k == 94 else 63)
    rcs = [model.rc(x) for x in seqs]
    hits = 0
    for rlen in list(range(K, K + 2 * s + 4, 7)) + [250, 256]:
        for rep in range(3):
            a = rng.randrange(0, G - rlen)
            read = list((genome if rep != 1 else var)[a:a + rlen])
            if rep == 2:
                read[rng.randrange(rlen)] = rng.choice("ACGTnR.")
            read = "".join(read)
            if rng.random() < 0.5:
                read = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, c) for c in reversed(read))
            want = pe_oracle.map_read_end(read, tab, lens, K)
            hits += len(want)
            _check_every_grid(read, seqs, rcs, mtab, w, s, K, want, key_fn, verified, (k, rlen))
    assert hits > 50


def _scenario_reads_cpu(sc):
    K, s, w = sc["K"], sc["s"], sc["w"]
    # the corners of c = min(s, j, q) and rem in vs_extend: the shared seed at read offsets 0, 1, s - 1, s and flush with the end
    # ((K - w) // 2: where the crowd's core, a read of exactly K bases, holds it)
    reads = sim.scenario_reads(sc, [K, K + 1, min(250, K + 2 * s + 40)], offsets_only=(0, 1, s - 1, s, -1, (K - w) // 2))
    rng = np.random.default_rng(sc["k"])
    some = reads[::3]
    return reads + sim.dirty_reads(some, w, rng, inside=False) + sim.dirty_reads(some, w, rng, inside=True)


def _run_scenarios(sc, key_fn, verified, every_grid=True):
    """-> (ends compared, ends whose list differs from the oracle's) under the given rules; with ``every_grid`` a
    difference is an assertion failure instead."""
    K, w, s, seqs = sc["K"], sc["w"], sc["s"], sc["seqs"]
    tab = pe_oracle.build_table(seqs, K)
    lens = [len(x) for x in seqs]
    mtab, w2, s2 = model.build(seqs, K, key_fn=key_fn)
    assert (w2, s2) == (w, s)
    rcs = [model.rc(x) for x in seqs]
    n = differ = 0
    for read, name, o, _ in _scenario_reads_cpu(sc):
        want = pe_oracle.map_read_end(read, tab, lens, K)
        n += 1
        if every_grid:
            _check_every_grid(read, seqs, rcs, mtab, w, s, K, want, key_fn, verified, (sc["k"], name, o))
        elif o is not None:  # (a probe exactly on the shared seed)
            differ += model.map_end(read, seqs, rcs, mtab, w, s, K, first=o % s, key_fn=key_fn, verified=verified) != want
    return n, differ


@pytest.mark.parametrize("k", [95, 127, 140])
def test_model_equals_oracle_on_seeds_that_share_a_key(k):
    """The scenarios of tests/test_seed_index_gpu.py (twins, orphan, strands, edges, crowd) under the device's rules."""
    sc = sim.shared_key_scenarios(k, np.random.default_rng(1000 + k), crowd=24)
    for name, groups in sc["groups"].items():
        for g in groups:
            assert len({sim.seed_key(q)[0] for q in g}) == 1 and len(set(g)) == len(g), name
    n, _ = _run_scenarios(sc, lambda c: sim.seed_key(c)[0], 0)
    assert n > 500


def _lossy_scenarios(k, rng):
    """w <= 31, where the device's keys are exact: two seeds that differ in their middle base only, and a key function
    that drops that base.  Same shape as shared_key_scenarios (twins on both sides of s, an orphan)."""
    K = k + 1
    w, s = sim.geometry(K)
    assert w == 31
    seqs, sources, groups = [], [], {"twins": [], "orphan": []}
    pad = 2 * s + 320
    for i, (n1, n2) in enumerate([(1, s - 1), (3, s + 2), (s + 2, 3), (s - 1, s - 1), (s, s), (K - 1, K - 1)]):
        # 'A' first and no 'T' last: the forward text is the canonical one for both twins
        x = "A" + sim.random_seq(rng, w - 2) + "ACG"[i % 3]
        y = sim.sub_at(x, w // 2)
        f1, f2 = sim.random_seq(rng, n1), sim.random_seq(rng, n2)
        orphan = i % 2 == 1
        groups["orphan" if orphan else "twins"].append([x, y])
        seqs.append(f1 + x + f2)
        sources.append(("orphan" if orphan else "twins", sim.random_seq(rng, pad) + f1 + y + f2 + sim.random_seq(rng, pad), pad + n1, []))
        if not orphan:
            seqs.append(f1 + y + f2)
            sources.append(("twins", sim.random_seq(rng, pad) + f1 + x + f2 + sim.random_seq(rng, pad), pad + n1, []))
    return dict(k=k, K=K, w=w, s=s, seqs=seqs, groups=groups, sources=sources)


def _lossy_key(c):
    return c[:15] + c[16:]


@pytest.mark.parametrize("k", [30, 55, 94])
def test_model_equals_oracle_when_a_lossy_key_merges_exact_seeds(k):
    sc = _lossy_scenarios(k, np.random.default_rng(2000 + k))
    for groups in sc["groups"].values():
        for x, y in groups:
            assert x != y and x < model.rc(x) and y < model.rc(y) and _lossy_key(x) == _lossy_key(y)
    n, _ = _run_scenarios(sc, _lossy_key, 0)
    assert n > 100


@pytest.mark.parametrize("k", [55, 95, 127, 140])
def test_negative_control_a_model_that_trusts_a_shared_key_differs_from_the_oracle(k):
    """The same scenarios with ``verified = w`` -- the seed's bases taken for granted although the key is shared: the lists
    must differ from the oracle's on some end of every scenario kind, or the scenarios could not tell a kernel that skips
    the comparison from one that makes it."""
    if k == 55:
        sc = _lossy_scenarios(k, np.random.default_rng(2000 + k))
        key_fn = _lossy_key
    else:
        sc = sim.shared_key_scenarios(k, np.random.default_rng(1000 + k), crowd=24)
        key_fn = lambda c: sim.seed_key(c)[0]  # noqa: E731
    for name in sc["groups"]:
        one = dict(sc, sources=[x for x in sc["sources"] if x[0] == name])
        n, differ = _run_scenarios(one, key_fn, sc["w"], every_grid=False)
        assert differ > 0, (name, n)
        _, differ = _run_scenarios(one, key_fn, 0, every_grid=False)
        assert differ == 0, name
