"""The cases of tests/pe_handoff_cases.py without a device: the plan names the instantiation, tile size, table and trim every
shape is built for; by the model (tests/pe_handoff_model.py) every case reaches the state it is named for; on the tiles
that are table-safe the model's count words are the host packer's (vstrains_amd/csrc/vs_pe_pack.h through
oracle/pack_check.cpp), both layouts; the per-end lists the model is given are the oracle's and the counters they imply are
the oracle's.  tests/test_pe_handoff_gpu.py holds the mapping kernel to the same statements."""
import numpy as np
import pytest

import pe_handoff_cases as hc
import pe_handoff_model as hm
from oracle import pe_oracle_c
from test_pe_pack_cpu import pack  # noqa: F401  (the fixture: vs_pe_pack_lists / vs_pe_unpack_lists on host arrays)

SHAPES = sorted(hc.SHAPES)


def _models(g, case, rows=0):
    fwd, rve = hc.reads(g, g.blocks[case])
    ends = hc.model_ends(g, fwd, rve)
    tiles, pairs = hm.block(ends, g.ept, g.pool, g.trim, rows)
    return fwd, rve, ends, tiles, pairs


@pytest.mark.parametrize("name", SHAPES)
def test_the_plan_names_the_shape(name):
    g = hc.graph(name)
    sh = g.shape
    for case, tiles in g.blocks.items():
        n_ends = sum(len(t) for t in tiles)
        assert n_ends < 2 * 4096  # (no locus sort: tiles in input order)
        p = hc.plan(g, n_ends)
        assert (p["kernel"], p["ept"], p["table_pool"], p["table_trim"]) == (sh["kernel"], sh["ept"], sh["pool"], sh["trim"]), (case, p)
        assert p["use_sort"] == 0 and p["use_rows"] == 0 and p["n_tiles"] == len(tiles) and p["list_ends"] == len(tiles) * sh["ept"]
        assert hc.plan(g, n_ends, acc_rows=1)["use_rows"] == 1
    if sh["env"] is None:  # a production context reaches it by itself: the padding keeps the index statistics off the adaptive grid
        assert g.n_seed_pos < 6 * g.n_distinct
    assert len(g.seqs) <= 3000 and all(len(s) == g.K for s in g.seqs)
    assert {"k20": 128, "k20fast": 128, "k55": 240, "k55ad": 256, "k127": 192}[name] == g.capq  # (as the project states them)


def test_sixty_four_ends_cannot_fill_the_trimmed_region_before_the_table():
    """pool 768, trim 64, ept 64: an end of n nodes takes n slots and ceil(n / 4) = (n + 3) / 4 quads at most, so 64 ends inside 768
    slots take at most (768 + 3 * 64) / 4 = 240 = capq quads -- `o + q > capq` cannot hold before a credit has failed -- and 240
    only with every slot taken, which is no table-safe tile.  The maximum itself by dynamic programming over the ends."""
    ept, pool, trim = 64, 768, 64
    assert hm.capq(ept, trim) == 240 == (pool + 3 * ept) // 4
    best = [0] + [-1] * pool  # best[s]: most quads of the ends so far with s slots taken
    for _ in range(ept):
        nxt = list(best)
        for s in range(pool + 1):
            if best[s] < 0:
                continue
            for n in range(1, hm.LCAP + 1):
                if s + n <= pool:
                    nxt[s + n] = max(nxt[s + n], best[s] + (n + 3) // 4)
        best = nxt
    assert max(best) == 240 and [s for s in range(pool + 1) if best[s] == 240] == [pool]
    assert max(best[:pool - pool // hm.PROBES + 1]) < 240  # (a table-safe tile leaves a slot free in every 64)
    # the k = 127 shape (ept 60, trim 192) can: the same arithmetic gives 237 > 192
    assert (pool + 3 * 60) // 4 == 237 > hm.capq(60, 192) == 192
    assert not hc.graph("k55").reachable and all(hc.graph(n).reachable for n in ("k20", "k20fast", "k55ad", "k127"))


@pytest.mark.parametrize("name", SHAPES)
def test_every_case_reaches_its_state(name):
    g = hc.graph(name)
    ept, cq = g.ept, g.capq
    # (a) every ordered pair of lengths; a 21 beside a 20 in one tile, a 21 without a 20 in another
    _, _, ends, tiles, _ = _models(g, "a")
    assert all(t["safe"] and t["first_unfit"] is None for t in tiles)
    seen = {(t["n"][2 * p], t["n"][2 * p + 1]) for t in tiles for p in range(len(t["n"]) // 2)}
    assert seen >= {(x, y) for x in hc.LENGTHS for y in hc.LENGTHS}
    assert any(21 in t["n"] and 20 in t["n"] for t in tiles) and any(21 in t["n"] and 20 not in t["n"] for t in tiles)
    assert all(t["listed"][p] == (21 in t["n"][2 * p:2 * p + 2]) for t in tiles for p in range(len(t["listed"])))
    assert sum(sum(t["listed"]) for t in tiles) > 0
    # (b) the region exactly full (or, where 64 ends cannot fill it, the fullest tile the search placed), nothing listed
    _, _, _, tiles, _ = _models(g, "b")
    b = tiles[0]
    assert b["safe"] and not any(b["listed"]) and all(n > 0 for n in b["n"]) and not any(any(t["listed"]) for t in tiles)
    if g.reachable:
        assert b["sum_q"] == cq and b["used_words"] == 4 * cq == ept * hm.LC - g.trim
        assert max(b["o"][e] + b["q"][e] for e in range(ept)) == cq
    else:
        assert b["entries"] >= g.pool * 9 // 10 and b["run"] >= hm.PROBES // 2 and cq - 8 < b["sum_q"] < cq
    # (c) one quad over: the first end that does not fit last in the tile / in its middle / in front of an empty and a dropped pair
    if g.reachable:
        _, _, ends, tiles, _ = _models(g, "c")
        last, _, mid, _, follow, _, light = tiles  # (a tile of dropped pairs behind each)
        assert all(tiles[t]["entries"] == 0 and tiles[t]["used_words"] == 0 for t in (1, 3, 5))
        assert all(t["safe"] and not any(t["over_lcap"]) for t in tiles)
        assert last["sum_q"] == cq + 1 and last["first_unfit"] == ept - 1 and last["listed"] == [False] * (ept // 2 - 1) + [True]
        x = mid["first_unfit"]
        assert ept // 2 <= x < ept - 4 and mid["o"][x] + mid["q"][x] == cq + 1 and mid["o"][x] <= cq
        behind = range(x + 1, ept - 2)
        assert {mid["n"][e] for e in behind} >= {0, 1, 4} and all(mid["over_region"][e] for e in behind)
        assert not ends[2 * ept + ept - 1]["used"]  # (the last pair of that tile is a dropped one)
        assert mid["listed"] == [False] * (x // 2) + [True] * (ept // 2 - 1 - x // 2) + [False]
        x = follow["first_unfit"]
        assert x == ept - 5 and follow["sum_q"] == cq + 1 and follow["n"][x + 1:x + 3] == [0, 0] and follow["over_region"][x + 1:x + 3] == [True, True]
        assert follow["listed"] == [False] * (x // 2) + [True, True, False] and not ends[4 * ept + ept - 1]["used"]
        assert follow["used_words"] == last["used_words"] == mid["used_words"] == 4 * cq
        assert not any(light["listed"])
    # (d) a tile of dropped pairs between full ones, one pair in the last tile
    _, _, ends, tiles, _ = _models(g, "d")
    assert not any(e["used"] for e in ends[ept:2 * ept]) and tiles[1]["entries"] == 0 and tiles[1]["word"] == [0] * ept
    assert tiles[0]["word"] == tiles[2]["word"] == b["word"] and len(tiles[3]["n"]) == 2 and tiles[3]["n"] == [5, 18]
    assert all(t["safe"] and not any(t["listed"]) for t in tiles)
    # (e) more entries than slots: some credit must fail
    _, _, _, tiles, _ = _models(g, "e")
    assert tiles[0]["entries"] > g.pool and not tiles[0]["safe"] and tiles[1]["safe"]


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("name", SHAPES)
def test_count_words_are_the_host_packers(pack, name, rows):  # noqa: F811
    """What the model says the kernel leaves on tiles whose ends all fit is what vs_pe_pack_lists writes for the same lists:
    count words (lengths and quad offsets), and the lists come back through either unpacker."""
    g = hc.graph(name)
    compared = 0
    for case in sorted(g.blocks):
        _, _, ends, tiles, _ = _models(g, case, rows)
        n_ends = len(ends)
        lists = np.full((n_ends, hm.LCAP), 0xFFFFFFFF, dtype=np.uint32)
        counts = np.zeros(n_ends, dtype=np.uint32)
        fits = []
        for t, tm in enumerate(tiles):
            # (no overflow end at all: the partner of an end of more than LCAP nodes keeps its quads in the kernel's prefix sum,
            # though its pair is listed and its count word 0 -- the packer would not know)
            ok = tm["safe"] and not any(tm["listed"])
            fits.append(ok)
            for i in range(len(tm["n"])):
                if ok and not tm["listed"][i // 2] and tm["n"][i]:
                    counts[t * g.ept + i] = tm["n"][i]
                    lists[t * g.ept + i, :tm["n"][i]] = tm["accepted"][i]
        rc, msg, out, oc, list_ends = pack(len(g.seqs), lists, counts, g.ept, rows)
        assert rc == 0, msg
        assert list_ends == len(tiles) * g.ept
        for t, tm in enumerate(tiles):
            if fits[t]:
                assert oc[t * g.ept:t * g.ept + len(tm["word"])].tolist() == tm["word"], (case, t)
                compared += 1
        back, bc = pack.unpack(n_ends, out, oc, g.ept, list_ends, rows)
        mine = hm.unpack(out, oc, n_ends, g.ept, list_ends, rows)
        assert bc.tolist() == counts.tolist() and [back[e, :bc[e]].tolist() for e in range(n_ends)] == mine
        assert mine == [lists[e, :counts[e]].tolist() for e in range(n_ends)]
    assert compared >= 6


def _implied(ends, n_nodes):
    """node_mat / short_mat of PE_Inference.py:174-188 from the accepted lists of the used pairs."""
    node = np.zeros((n_nodes, n_nodes), dtype=np.int64)
    short = np.zeros((n_nodes, n_nodes), dtype=np.int64)
    for p in range(len(ends) // 2):
        if not ends[2 * p]["used"]:
            continue
        left, right = ([n for n, ok in ends[2 * p + side]["nodes"] if ok] for side in (0, 1))
        for l in left:
            for r in right:
                node[l, r] += 1
        for end in (left, right):
            for a in range(len(end)):
                for b in range(a, len(end)):
                    short[min(end[a], end[b]), max(end[a], end[b])] += 1
    return node, short


@pytest.mark.parametrize("name", SHAPES)
def test_lists_and_counters_are_the_oracles(name):
    g = hc.graph(name)
    orc = pe_oracle_c.Oracle(g.seqs, g.shape["k"])
    checked = set()
    for case in sorted(g.blocks):
        fwd, rve, ends, _, _ = _models(g, case)
        for p, (f, r) in enumerate(zip(fwd, rve)):
            for side, text in enumerate((f, r)):
                if text in checked or "N" in text:
                    continue
                checked.add(text)
                want = orc.map_end(text) if len(text) >= g.K else []
                assert sorted(n for n, ok in hc.mapped(g, text) if ok) == sorted(want), (case, p, side)
                assert all(ok for _, ok in hc.mapped(g, text))  # (whole nodes: v = 1 = span, nothing credited is turned down)
        node, short, stats = orc.count_pairs(fwd, rve)
        mine = _implied(ends, len(g.seqs))
        assert np.array_equal(node, mine[0]) and np.array_equal(short, mine[1]), case
        assert int(stats[2]) == sum(e["used"] for e in ends) // 2
    orc.close()
