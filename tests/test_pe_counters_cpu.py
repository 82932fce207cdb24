"""The host statement of the counter stage (pe_counter_model.py) against the oracle's own loops, and the constructed
blocks of tests/test_pe_counters_gpu.py against the properties they were built for -- the same assertions, on the same
seeds, that the GPU tests make before they count: a case that lost its property fails here, without a device."""
import numpy as np
import pytest

from oracle import pe_oracle
import pe_counter_cases as cases
import pe_counter_model as pcm


def test_model_equals_the_oracles_loops():
    rng = np.random.default_rng(2024)
    for trial in range(300):
        n_nodes = int(rng.integers(1, 40))
        n_pairs = int(rng.integers(0, 12))
        top = min(n_nodes, pcm.LCAP)
        pairs = [tuple([int(x) for x in rng.choice(n_nodes, size=int(rng.integers(0, top + 1)), replace=False)] for _ in range(2)) for _ in range(n_pairs)]
        # the oracle gets a mapper that hands out the prepared lists, ascending as the reference has them; the model
        # gets them in the order drawn
        lookup = {}
        fwd, rve = [], []
        for p, (l, r) in enumerate(pairs):
            fwd.append("AC%dF" % p)
            rve.append("AC%dR" % p)
            lookup[fwd[-1]], lookup[rve[-1]] = sorted(l), sorted(r)
        want_node, want_short, stats = pe_oracle.pe_matrices([""] * n_nodes, fwd, rve, 1, table={}, mapper=lambda read, *_: lookup[read])
        assert stats == (0, 0, n_pairs)
        lists = np.zeros((2 * n_pairs, pcm.LCAP), dtype=np.int64)
        counts = np.zeros(2 * n_pairs, dtype=np.int64)
        for p, pair in enumerate(pairs):
            for side, end in enumerate(pair):
                counts[2 * p + side] = len(end)
                lists[2 * p + side, : len(end)] = end
        (nc, nv), (sc, sv) = pcm.count_block(lists, counts, n_nodes)
        for (cells, values), want in (((nc, nv), want_node), ((sc, sv), want_short)):
            got = np.zeros(n_nodes * n_nodes, dtype=np.int64)
            got[cells] = values
            assert np.array_equal(got.reshape(n_nodes, n_nodes), want), trial
            assert (values > 0).all() and (np.diff(cells) > 0).all()
            assert pcm.tiles_of(cells, n_nodes) == {(int(x) // 64) * ((n_nodes + 63) // 64) + int(y) // 64 for x, y in zip(*np.nonzero(want))}
        dn, ds = pcm.count_block_dense(lists, counts, n_nodes)
        assert np.array_equal(dn, want_node) and np.array_equal(ds, want_short)


def test_every_length_pair_block():
    n_nodes, pairs = cases.every_length_pair()
    assert len(pairs) == 2205 and n_nodes == 200
    for ept in (6, 32, 64, 128):
        _, lists, counts = cases.block((n_nodes, pairs), ept)
        real = [(int(a), int(b)) for a, b in counts.reshape(-1, 2)]
        assert len({x for x in real}) == 441 and counts.size % 2 == 0


def test_table_pressure_block():
    assert cases.assert_table_pressure(cases.table_pressure()) > 100000


def test_probes_exhausted_block():
    cases.assert_probes_exhausted(cases.probes_exhausted())


@pytest.mark.parametrize("form", ["row", "column", "short"])
def test_wide_row_block(form):
    case = cases.wide_row(form)
    (nc, _), (sc, _) = pcm.count_block(*cases.block(case)[1:], case[0])
    unplaced = cases.assert_wide_row(case, form, nc, sc)
    assert form == "column" or unplaced > 0


def test_list_table_blocks():
    hits = cases.assert_tag_collisions(cases.list_table_distinct())
    assert len(hits) == 18  # (what LIST_TABLE_SEED gives; about 16 are expected from 2^27 tags)
    assert len(cases.assert_long_tag_collisions(cases.list_table_long())) >= 3


@pytest.mark.parametrize("length,shared", [(12, 0), (16, 0), (20, 16)])
def test_lists_that_meet_in_the_list_table(length, shared):
    assert len(cases.assert_lists_meet(cases.meeting_lists(length, shared), length, shared)) == 4


def test_many_rows_spread_tiles_and_key_edge_blocks():
    cases.assert_many_rows(cases.many_rows())
    cases.assert_spread_tiles(cases.spread_tiles())
    for n_nodes in (46340, 46341, 65600):
        case = cases.key_edge(n_nodes, spread=40 if n_nodes == 65600 else 0)
        (nc, _), (sc, _) = pcm.count_block(*cases.block(case)[1:], n_nodes)
        cases.assert_key_edge(case, nc, sc)
        if n_nodes == 65600:
            assert nc.max() >= 1 << 32 and sc.max() >= 1 << 32


def test_restated_hashing_is_self_consistent():
    # a slot keeps the low four bits of its key; sixteen cells of one 64-byte stretch sit in sixteen neighbouring slots
    for bits in (pcm.ACC_BITS, pcm.RS_BITS):
        keys = np.arange(0x12340, 0x12350)
        slots = pcm.cell_slot(keys, bits)
        assert (slots & 15 == keys & 15).all() and len(set((slots >> 4).tolist())) == 1 and slots.max() < 1 << bits
        assert pcm.cell_next((1 << bits) - 3, bits) == 13
    # permuted copies of one set share fingerprint, tag and home slot; the length rides in the tag
    rng = np.random.default_rng(5)
    row = rng.choice(5000, size=20, replace=False)
    lists = np.stack([row, row[::-1], rng.permutation(row)])
    f2 = pcm.list_fingerprint(lists, [20, 20, 20])
    assert len(set(f2.tolist())) == 1 and (pcm.list_tag(f2, [20, 20, 20]) & 31 == 19).all()
    assert pcm.list_fingerprint(lists[:1], [19])[0] != f2[0]
    assert pcm.ltab_bits_for(32768) == 16 and pcm.ltab_bits_for(3) == 10
    # the row-owner key: relative to the strip's first row, shifted by the matrix's place inside its 64-byte stretch
    assert pcm.rows_key(7, 3, 6, 100, 0x1000) == 100 + (600 & 15) + 3
    assert pcm.rows_key(7, 3, 6, 100, 0x1004) == 100 + ((600 + 1) & 15) + 3
