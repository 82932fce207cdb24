"""What the blocks of tests/pe_preprobe_cases.py hold, asserted without a device: every kind of tile is what it says (used
and unused pairs from the C oracle's totals, the slots the probes meet from the host statement of the index,
seed_index_model), neighbouring tiles differ in kind, both lengths of a shape and so different probe phases occur in every
tile, the oracle accepts a node for more than half of the usable ends, and the run lengths the device test relies on follow
from the plan's formula.  The device side: tests/test_pe_preprobe_gpu.py."""
import functools

import pytest

import pe_preprobe_cases as ppc
import seed_extend_model as model
import seed_index_model as sim
from oracle import pe_oracle_c

SHAPES = list(ppc.SHAPES)


@functools.lru_cache(maxsize=None)
def oracle():
    return pe_oracle_c.Oracle(ppc.graph()["seqs"], ppc.KSIZE)


def _tiles(kernel):
    fam = ppc.family(kernel)
    for t, kd in enumerate(ppc.KINDS):
        sl = slice(t * ppc.TILE_PAIRS, (t + 1) * ppc.TILE_PAIRS)
        assert set(fam["kind"][sl]) == {kd}
        yield kd, fam["fwd"][sl], fam["rve"][sl]


def _features(fwd, rve):
    out = []
    for f, r in zip(fwd, rve):
        used = ppc.pair_used(f, r)
        out.append((used, ppc.end_features(f, used), ppc.end_features(r, used)))
    return out


def test_graph_has_the_planted_chain_and_seeds_of_one_and_of_several_postings():
    g = ppc.graph()
    m = g["model"]
    assert 24 <= len(g["seqs"]) <= 48
    keys = [sim.seed_key(q)[0] for q, _ in g["planted"]]
    assert len(set(keys)) == ppc.GROUP and all(k in m["postings"] for k in keys)
    assert all(sim.slot_of(k, m["bits"]) == g["home"] for k in keys)
    # six keys on one home slot take the six slots from there on (nothing else is near): five of them sit behind another key
    run, = [r for r in sim.runs(m["occupied"], m["slots"]) if r[0] <= g["home"] < r[0] + r[1]]
    assert run[0] == g["home"] and run[1] >= ppc.GROUP
    assert all(sim.seed_key(q)[0] not in m["postings"] and sim.slot_of(sim.seed_key(q)[0], m["bits"]) == g["home"] for q in g["misses"])
    counts = [len(v) for v in m["postings"].values()]
    assert counts.count(1) > 1000 and sum(c == 3 for c in counts) >= 100
    # the adaptive grid and the run-time shapes stay out: few postings per seed (vs_pe_plan: 6 and more would choose AD)
    assert m["seed_positions"] < 2 * m["distinct"]


@pytest.mark.parametrize("kernel", SHAPES)
def test_every_tile_is_of_its_kind(kernel):
    lo_len, hi_len = ppc.SHAPES[kernel]
    assert len(ppc.grid(lo_len)) <= len(ppc.grid(hi_len)) == int(kernel.split(",")[2].strip(" u>"))
    assert model.phase(lo_len, ppc.W, ppc.S) != model.phase(hi_len, ppc.W, ppc.S)
    g = ppc.graph()
    planted = {sim.seed_key(q)[0] for q, _ in g["planted"]}
    orc = oracle()
    for kd, fwd, rve in _tiles(kernel):
        feats = _features(fwd, rve)
        n_used = sum(u for u, _, _ in feats)
        ends = [x for _, a, b in feats for x in (a, b)]
        every = set().union(*ends)
        # the oracle's totals: pairs dropped for an N, dropped as short, used
        stats = tuple(int(x) for x in orc.count_pairs(fwd, rve)[2])
        assert stats[2] == n_used and sum(stats) == ppc.TILE_PAIRS, (kd, stats)
        # both lengths among the ends of used pairs: different phases inside the tile
        used_lens = {len(x) for f, r in zip(fwd, rve) if ppc.pair_used(f, r) for x in (f, r)}
        assert used_lens == {lo_len, hi_len}, (kd, used_lens)
        if kd in ("usable", "edited"):
            assert n_used == ppc.TILE_PAIRS and not any(x in every for x in ("n", "below_K", "below_w")) and not any(str(x).startswith("dirty") for x in every)
            assert "single" in every and "multi" in every
        elif kd == "n":
            assert stats[0] == ppc.TILE_PAIRS // 2 and stats[1] == 0 and "n" in every
        elif kd == "short":
            assert stats[0] == 0 and stats[1] == 3 * ppc.TILE_PAIRS // 4 and {"below_K", "below_w"} <= every
        elif kd == "dirty":
            assert n_used == ppc.TILE_PAIRS
            assert {"dirty1", "dirty2", "dirty3", "dirty4", "dirty5"} <= every
            assert sum(1 for x in ends if not any(str(y).startswith("dirty") for y in x)) >= ppc.TILE_PAIRS  # clean ends beside them
        elif kd == "empty":
            assert n_used == ppc.TILE_PAIRS and "empty" in every
            assert all(not ({"single", "multi"} & a) for _, a, _ in feats)  # (every forward end is random text)
        elif kd == "displaced":
            assert n_used == ppc.TILE_PAIRS and "walk" in every
            probed = {x[2] for x in every if isinstance(x, tuple) and x[1] == g["home"]}
            assert probed == planted  # all six keys of the one home slot are probed on the grid: at least five from behind another key
    kinds = [kd for kd, _, _ in _tiles(kernel)]
    assert all(a != b for a, b in zip(kinds, kinds[1:] + kinds[:1])) and len(set(kinds)) == len(ppc.KINDS) == 7


@pytest.mark.parametrize("kernel", SHAPES)
def test_oracle_accepts_a_node_for_most_usable_ends(kernel):
    fam = ppc.family(kernel)
    orc = oracle()
    usable = [x for f, r in zip(fam["fwd"], fam["rve"]) if ppc.pair_used(f, r) for x in (f, r)]
    accepted = sum(1 for x in usable if orc.map_end(x))
    assert 2 * accepted > len(usable) > ppc.FAMILY_PAIRS, (accepted, len(usable))
    # and the planted windows are accepted by their own node
    g = ppc.graph()
    t = ppc.KINDS.index("displaced") * ppc.TILE_PAIRS
    for i in range(ppc.TILE_PAIRS):
        assert g["planted"][i % ppc.GROUP][1] in orc.map_end(fam["fwd"][t + i])


@pytest.mark.parametrize("n_cu", [256, 304, 64])
def test_blocks_make_runs_of_three_tiles_and_more(n_cu):
    """n_pairs = n_cu * 32 * 3 + r under one workgroup per CU: r = 0 gives runs of exactly three tiles; r = 1 and 31 a partial
    tile that is the last workgroup's whole run; r = 33 a partial tile behind a full one in that run.  Runs of three and four
    tiles over a cycle of seven kinds start at every kind."""
    want = {0: (3, 3, 32), 1: (4, 1, 1), 31: (4, 1, 31), 33: (4, 2, 1)}
    for r in ppc.REMAINDERS:
        n_pairs = ppc.block_pairs(n_cu, r)
        n_tiles, per_wg, wgs, last = ppc.runs_of_tiles(n_pairs, n_cu)
        assert per_wg >= ppc.RUN_TILES and wgs > 1 and wgs <= n_cu
        assert (per_wg, last, n_pairs - (n_tiles - 1) * ppc.TILE_PAIRS) == want[r], (r, per_wg, last)
        assert {(w * per_wg) % len(ppc.KINDS) for w in range(wgs)} == set(range(len(ppc.KINDS)))
    # the production grid (128 workgroups per CU) takes one tile per workgroup at this size: nothing is handed over there
    assert ppc.runs_of_tiles(ppc.block_pairs(n_cu, 33), n_cu, 128)[1] == 1


def test_block_repeats_the_family_in_input_order():
    kernel = SHAPES[0]
    fwd, rve, idx = ppc.block(kernel, 2 * ppc.FAMILY_PAIRS + 33)
    fam = ppc.family(kernel)
    assert idx[:ppc.FAMILY_PAIRS] == list(range(ppc.FAMILY_PAIRS)) and idx[-1] == 32
    assert fwd[ppc.FAMILY_PAIRS + 5] == fam["fwd"][5] and rve[-1] == fam["rve"][32]
