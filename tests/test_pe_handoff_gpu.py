"""The hand-off between the mapping kernel and the counter kernels as k_pe_tiles (vstrains_amd/csrc/vs_pe.hip, P4 / P5)
writes it, read back with vs_pe_last_handoff: the count words, the lists, the first overflow list and every word the kernel
has no business writing, on the blocks of tests/pe_handoff_cases.py -- list lengths around LCAP, a tile region exactly full
and one quad over, ends behind the first that did not fit, a full tile table, the row layout, a singles block, a block
through the locus sort -- against the model of tests/pe_handoff_model.py and the oracle.  tests/test_pe_handoff_cpu.py
shows without a device that every block reaches the state it is named for.

Every run first counts a block of full tiles of the same size (so that the scratch holds known words), then the case, and
compares: what is exact on every tile (nothing about the order of atomics enters), what is exact on table-safe tiles (count
words from a prefix sum in end order, the overflow list as a set), the counters with the oracle's, and the counters with
what the counter kernels give from the hand-off read back plus the oracle's counters of the listed pairs."""
import random

import numpy as np
import pytest

import pe_handoff_cases as hc
import pe_handoff_model as hm
from oracle import pe_oracle_c

pytestmark = pytest.mark.gpu

SHAPES = sorted(hc.SHAPES)
CASES = [(name, case) for name in SHAPES for case in "abcde" if case != "c" or name != "k55"]  # (c) needs a region 64 ends can fill


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe

    return pe


@pytest.fixture(scope="module")
def shapes(host):
    """name -> (graph, context with its index, oracle), made once; an experiment context only where the shape needs a switch."""
    from conftest import experiment_context

    made = {}

    def get(name, experiment=False):
        g = hc.graph(name)
        experiment = experiment or g.shape["env"] is not None
        if (name, experiment) not in made:
            c = experiment_context(host) if experiment else host.Context(0)
            c.build_index(g.seqs, g.shape["k"], renumber=False)
            assert c.node_order is None  # (the matrices and the hand-off speak the numbering of g.seqs)
            info = c.index_info
            assert (info["seed_positions"], info["distinct_seeds"]) == (g.n_seed_pos, g.n_distinct)  # (what the plan on the CPU was given)
            made[(name, experiment)] = c
        if name not in made:
            made[name] = pe_oracle_c.Oracle(g.seqs, g.shape["k"])
        return g, made[(name, experiment)], made[name]

    yield get
    for v in made.values():
        v.close()


_lists = {}


def _oracle_list(name, orc, g, text):
    if (name, text) not in _lists:
        _lists[(name, text)] = sorted(orc.map_end(text)) if len(text) >= g.K else []
    return _lists[(name, text)]


def _run(host, monkeypatch, g, c, orc, fwd, rve, env=None, singles=False):
    """Count the block on ``c`` and hold everything the call left to the model and the oracle.  -> (hand-off, tile models,
    pairs on the overflow list)"""
    import torch

    for k, v in dict(g.shape["env"] or {}, **(env or {})).items():
        monkeypatch.setenv(k, v)
    rows = 1 if (env or {}).get("VS_ACC_ROWS") == "1" else 0
    n_pairs, N, ept = len(fwd), len(g.seqs), g.ept
    ppt = ept // 2
    want_plan = hc.plan(g, 2 * n_pairs, acc_rows=1 if rows else -1)
    counter = host.PeCounter(c)
    assert counter.tile_map is None
    # known words in the scratch: full tiles in every tile of a block of the same size
    full = g.blocks["b"][0]
    paint = hc.reads(g, [full] * (-(-n_pairs // ppt)))
    counter.add(c.pack_pairs(paint[0][:n_pairs], paint[1][:n_pairs]))
    before = c.last_handoff()
    assert before is not None and (before["pairs"], before["rows"], before["list_ends"]) == (n_pairs, rows, want_plan["list_ends"])
    counter.reset()
    block = c.pack_singles(fwd) if singles else c.pack_pairs(fwd, rve)
    assert block.unpaired == singles and block.info["ends"] == 2 * n_pairs
    counter.add(block)
    h = c.last_handoff()
    keys, perm, sort, n_order = c.last_order()
    timing = c.last_timing()
    kernel = c.last_kernel
    mats = counter.mats.cpu().numpy().view(np.uint32).astype(np.int64)
    stats = tuple(int(x) for x in (counter.single_stats if singles else counter.stats).cpu().numpy())

    # the instantiation, tile size, layout, table and trim the plan names
    assert kernel == g.shape["kernel"] == want_plan["kernel"]
    assert h is not None and n_order == n_pairs
    assert (h["pairs"], h["ept"], h["list_ends"], h["rows"], h["pool"], h["trim"]) == (
        n_pairs, want_plan["ept"], want_plan["list_ends"], rows, want_plan["table_pool"], want_plan["table_trim"])
    assert (h["ept"], h["pool"], h["trim"]) == (ept, g.pool, g.trim)
    assert bool(sort) == bool(want_plan["use_sort"]) and bool(c.last_launched & c.RAN_ROW_OWNERS) == bool(rows)
    assert h["lists"].size == h["list_ends"] * (hm.LC + 4 if rows else hm.LC) + 16 and h["counts"].size == h["list_ends"]
    cq = hm.capq(ept, g.trim)

    # the counters are the oracle's
    if singles:  # what the reference gives one end of a pair: its own short_mat triangle, nothing in node_mat
        ends1 = hc.model_ends(g, fwd, rve, singles=True)
        short = np.zeros((N, N), dtype=np.int64)
        for e in ends1:
            acc = [n for n, ok in e["nodes"] if ok] if e["used"] else []
            for a in range(len(acc)):
                for b in range(a, len(acc)):
                    short[min(acc[a], acc[b]), max(acc[a], acc[b])] += 1
        assert not mats[0].any() and np.array_equal(mats[1], short)
        assert stats[2] == sum(e["used"] for e in ends1) // 2 and sum(stats) == n_pairs
    else:
        ref = orc.count_pairs(fwd, rve)
        assert np.array_equal(mats[0], ref[0]), "node_mat differs from the oracle"
        assert np.array_equal(mats[1], ref[1]), "short_mat differs from the oracle"
        assert stats == tuple(int(x) for x in ref[2])

    # the model of the block, tiles as the kernel took them
    ends = hc.model_ends(g, fwd, rve, singles=singles)
    tiles, tile_pairs = hm.block(ends, ept, g.pool, g.trim, rows, perm=perm if sort else None)
    assert len(tiles) == h["list_ends"] // ept

    # the overflow list: no pair twice, used pairs only, as long as the timing says
    over = [int(p) for p in h["overflow"]]
    listed = set(over)
    assert len(listed) == len(over) == timing["slow_pairs"]
    assert all(p < n_pairs and ends[2 * p]["used"] for p in listed)

    got = hm.unpack(h["lists"], h["counts"], 2 * n_pairs, ept, h["list_ends"], rows)
    for t, (tm, mine) in enumerate(zip(tiles, tile_pairs)):
        spans = []
        for i in range(2 * len(mine)):
            p, side = mine[i // 2], i & 1
            word = int(h["counts"][t * ept + i])
            text = (fwd, rve)[side][p]
            # order-free, every tile
            if not ends[2 * p]["used"]:
                assert word == 0 and p not in listed, ("an end of a dropped pair", t, i)
                continue
            if p in listed:
                assert word == 0, ("an end of a listed pair", t, i, word)
                continue
            want = _oracle_list(g.name, orc, g, text)
            n = word if rows else word & 0xFF
            nodes = got[t * ept + i]
            assert n == len(want) <= hm.LCAP, (t, i, n, len(want))
            assert all(x < N for x in nodes) and len(set(nodes)) == n and sorted(nodes) == want, (t, i, nodes, want)
            if singles and side:
                assert word == 0
            if not rows and n:
                o, q = word >> 8, (n + 3) // 4
                assert o + q <= cq and (not tm["safe"] or 4 * (o + q) <= tm["used_words"]), (t, i, o, q)
                spans.append((o, o + q))
            elif not rows:
                assert word == 0
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), ("lists of a tile overlap", t, spans)
        # exact on table-safe tiles: the count words (offsets from a prefix sum in end order) and who is listed
        if tm["safe"]:
            assert [int(x) for x in h["counts"][t * ept:t * ept + 2 * len(mine)]] == tm["word"], (t, tm["first_unfit"])
            assert [p in listed for p in mine] == tm["listed"], (t, tm["first_unfit"])
    if all(tm["safe"] for tm in tiles):
        assert listed == {p for tm, mine in zip(tiles, tile_pairs) for p, x in zip(mine, tm["listed"]) if x}

    # the kernel writes the words it hands over and no other: everything else is as the block before left it
    a, b = before["lists"], h["lists"]
    assert a.size == b.size
    if not rows:
        for t, tm in enumerate(tiles):
            lo = t * ept * hm.LC + (tm["used_words"] if tm["safe"] else 4 * cq)
            assert np.array_equal(a[lo:(t + 1) * ept * hm.LC], b[lo:(t + 1) * ept * hm.LC]), ("words behind the lists of tile", t)
        assert np.array_equal(a[h["list_ends"] * hm.LC:], b[h["list_ends"] * hm.LC:])
    else:
        hi = h["list_ends"] * hm.LC
        for e in range(h["list_ends"]):
            n = int(h["counts"][e]) if e < 2 * n_pairs else 0
            lo = 4 * ((min(n, hm.LC) + 3) // 4)
            assert np.array_equal(a[e * hm.LC + lo:(e + 1) * hm.LC], b[e * hm.LC + lo:(e + 1) * hm.LC]), ("row", e)
            if n <= hm.LC:
                assert np.array_equal(a[hi + 4 * e:hi + 4 * e + 4], b[hi + 4 * e:hi + 4 * e + 4]), ("second array", e)
        assert np.array_equal(a[hi + 4 * h["list_ends"]:], b[hi + 4 * h["list_ends"]:])

    # closing the chain: the counter kernels on the lists read back (tile order), plus the oracle on the listed pairs alone
    handed = []
    for t, mine in enumerate(tile_pairs):
        for j, p in enumerate(mine):
            handed.append(((), ()) if p in listed else (got[t * ept + 2 * j], got[t * ept + 2 * j + 1]))
    lists, counts = c.list_block(handed)
    dev = counter.mats.device
    again = torch.zeros((2, N, N), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.pe_count_lists(N, lists, counts, again[0].data_ptr(), again[1].data_ptr())
    assert c.last_handoff() is None  # (host-made lists are no hand-off of a mapping kernel)
    again = again.cpu().numpy().view(np.uint32).astype(np.int64)
    rest = sorted(listed)
    if rest and not singles:
        extra = orc.count_pairs([fwd[p] for p in rest], [rve[p] for p in rest])
        again[0] += extra[0]
        again[1] += extra[1]
    for p in rest if singles else ():  # (a listed unpaired read: its own triangle)
        acc = _oracle_list(g.name, orc, g, fwd[p])
        for x in range(len(acc)):
            for y in range(x, len(acc)):
                again[1][acc[x], acc[y]] += 1
    assert np.array_equal(again[0], mats[0]) and np.array_equal(again[1], mats[1])
    return h, tiles, listed


@pytest.mark.parametrize("name,case", CASES, ids=["%s-%s" % nc for nc in CASES])
def test_case(host, shapes, monkeypatch, name, case):
    g, c, orc = shapes(name)
    fwd, rve = hc.reads(g, g.blocks[case])
    h, tiles, listed = _run(host, monkeypatch, g, c, orc, fwd, rve)
    if case == "a":  # every pair with an end of 21 nodes and no other
        assert listed and len(listed) == sum(sum(tm["listed"]) for tm in tiles)
    if case in "bd":
        assert not listed
    if case == "b" and g.reachable:
        assert max((int(w) >> 8) + ((int(w) & 0xFF) + 3) // 4 for w in h["counts"][:g.ept]) == g.capq  # the region's last quad is taken
    if case == "c":
        assert len(listed) == sum(sum(tm["listed"]) for tm in tiles) >= 3
    if case == "e":  # some credit failed: pairs are listed though no end of the tile has more than LCAP nodes
        assert listed and not any(tiles[0]["over_lcap"]) and all(p < g.ept // 2 for p in listed)


@pytest.mark.parametrize("name,case,env", [("k55ad", "a", {}), ("k55ad", "c", {}), ("k20", "a", {}), ("k20", "c", {}), ("k55ad", "c", {"VS_NO_MID": "1"}),
                                           ("k127", "c", {})],
                         ids=["k55ad-a", "k55ad-c", "k20-a", "k20-c", "k55ad-c-nomid", "k127-c"])
def test_row_layout(host, shapes, monkeypatch, name, case, env):
    """The row layout through the mapping kernel (what graphs beyond 46 340 nodes take): nodes 1 .. 16 in the end's row, 17 .. 20
    in its quad of the second array, count words without offsets -- and the same ends are overflow ends."""
    g, c, orc = shapes(name, experiment=True)
    fwd, rve = hc.reads(g, g.blocks[case])
    h, tiles, listed = _run(host, monkeypatch, g, c, orc, fwd, rve, env=dict(env, VS_ACC_ROWS="1"))
    assert h["rows"] == 1 and listed
    assert any(17 <= int(w) <= 20 for w in h["counts"])  # an end with nodes in the second array


def test_overflow_straight_to_the_general_kernel(host, shapes, monkeypatch):
    """VS_NO_MID=1, packed layout: the first overflow list is k_pe_slow's input."""
    g, c, orc = shapes("k55ad")
    fwd, rve = hc.reads(g, g.blocks["c"])
    _, _, listed = _run(host, monkeypatch, g, c, orc, fwd, rve, env={"VS_NO_MID": "1"})
    assert listed and not c.last_launched & c.RAN_PE_MID


def test_singles_block(host, shapes, monkeypatch):
    """The even ends of case (a) as unpaired reads: odd slots have count 0 and are never overflow ends, node_mat is untouched."""
    g, c, orc = shapes("k55")
    fwd, _ = hc.reads(g, g.blocks["a"])
    h, tiles, listed = _run(host, monkeypatch, g, c, orc, fwd, [""] * len(fwd), singles=True)
    assert listed == {p for p, f in enumerate(fwd) if len(hc.mapped(g, f)) > hm.LCAP} and listed  # (only a read's own 21 nodes list its slot)
    assert not h["counts"][1:2 * len(fwd):2].any() and h["counts"][0:2 * len(fwd):2].any()


def test_block_through_the_locus_sort(host, shapes, monkeypatch):
    """Some 4 900 pairs, case (a)'s repeated and shuffled, with dropped pairs among them: tiles are taken from the order the sort made."""
    g, c, orc = shapes("k55")
    fwd, rve = hc.reads(g, g.blocks["a"] + [hc.tile_dropped(g.ept)])
    rng = random.Random(5)
    order = [p for p in range(len(fwd)) for _ in range(16)] + list(range(len(fwd) - 32))
    rng.shuffle(order)
    assert len(order) >= 4096
    h, tiles, listed = _run(host, monkeypatch, g, c, orc, [fwd[p] for p in order], [rve[p] for p in order])
    safe = [tm for tm in tiles if tm["safe"]]
    assert len(safe) >= len(tiles) // 2 and listed
    assert any(any(tm["listed"]) for tm in safe) and any(tm["first_unfit"] is not None or any(tm["over_lcap"]) for tm in safe)


def test_no_handoff_after_map_ends_and_empty_blocks(host, shapes):
    g, c, orc = shapes("k55")
    fwd, rve = hc.reads(g, g.blocks["d"][3:])
    counter = host.PeCounter(c)
    counter.add(c.pack_pairs(fwd, rve))
    assert c.last_handoff() is not None
    lists = c.map_ends(c.pack_pairs(fwd, rve), cap=32)
    assert [len(x) for x in lists] == [5, 18] and c.last_handoff() is None
    counter.add(c.pack_pairs(fwd, rve))
    assert c.last_handoff()["pairs"] == 1
    counter.add(c.pack_pairs([], []))
    assert c.last_handoff() is None
