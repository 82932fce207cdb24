"""Unpaired reads through the counting kernels: singles blocks (``Context.pack_singles`` = ``vs_reads_pack_single``: end 2r
is read r, end 2r+1 is absent) against the plain model of tests/unpaired_model.py -- what the reference does with ONE end
of a pair.  The blocks are those of tests/unpaired_cases.py, which tests/test_unpaired_model_cpu.py checks without a device."""
import numpy as np
import pytest

import unpaired_cases as uc

pytestmark = pytest.mark.gpu

VARIANTS = [{}, {"VS_ACC_ROWS": "1"}, {"VS_NO_AGG": "1"}, {"VS_NO_SORT": "1"}, {"VS_NO_STD": "1"}, {"VS_NO_FAST": "1"}, {"VS_NO_MID": "1"}]


def _vid(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "production"


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe

    return pe


@pytest.fixture(scope="module")
def contexts(host):
    """(graph, experiment?) -> a context with that graph's index, made once"""
    from conftest import experiment_context

    made = {}

    def get(graph, experiment=False):
        key = (graph, experiment)
        if key not in made:
            g = uc.GRAPHS[graph]()
            ctx = experiment_context(host) if experiment else host.Context(0)
            ctx.build_index(g.seqs, g.k)
            made[key] = ctx
        return made[key]

    yield get
    for ctx in made.values():
        ctx.close()


def _count(host, ctx, reads):
    counter = host.PeCounter(ctx)
    block = ctx.pack_singles(reads)
    assert block.unpaired and block.info["ends"] == 2 * len(reads)
    counter.add(block)
    node_mat, short_mat, stats = counter.result()
    return node_mat, short_mat, stats, tuple(int(x) for x in counter.single_stats.cpu().numpy())


def _check(got, want):
    node_mat, short_mat, stats, single_stats = got
    assert not node_mat.any(), "an unpaired read reached node_mat"
    assert np.array_equal(short_mat, want[1])
    assert single_stats == want[2]
    assert stats == (0, 0, 0), "the pairs' tallies moved"


@pytest.mark.parametrize("n", uc.SIZES)
@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_block_sizes(host, contexts, graph, n):
    reads = uc.block(graph, n)
    want = uc.expected(graph, reads)
    if n >= 31:
        assert want[1].sum() > 0 and want[2][0] > 0 and want[2][1] > 0
    _check(_count(host, contexts(graph), reads), want)


@pytest.mark.parametrize("env", VARIANTS[1:], ids=_vid)
@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_plans(host, contexts, graph, env, monkeypatch):
    """The other plans of a count (row owners, no aggregation, input order, no compile-time shape, the generic mapping kernel,
    the overflow pairs straight to the general kernel) on a block beyond the sort's threshold and on a small one."""
    ctx = contexts(graph, experiment=True)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n in (77, 4097):
        reads = uc.block(graph, n)
        _check(_count(host, ctx, reads), uc.expected(graph, reads))
        if "VS_ACC_ROWS" in env:
            assert ctx.last_launched & ctx.RAN_ROW_OWNERS


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_overflow_path_with_an_absent_mate(host, contexts, graph):
    """Reads with five bytes outside ACGT (VS_FLAG_MANY) alone in a block: every used slot goes to k_pe_mid / k_pe_slow."""
    g = uc.GRAPHS[graph]()
    reads = tuple([uc.specials(g)["five_invalid"]] * 5)
    ctx = contexts(graph)
    want = uc.expected(graph, reads)
    assert want[1].sum() > 0
    _check(_count(host, ctx, reads), want)
    assert ctx.last_timing()["slow_pairs"] == 5


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_every_read_dropped(host, contexts, graph):
    reads = uc.all_dropped(graph)
    want = uc.expected(graph, reads)
    assert want[2][2] == 0
    _check(_count(host, contexts(graph), reads), want)


def test_empty_block(host, contexts):
    _check(_count(host, contexts("chain"), ()), uc.expected("chain", ()))


def test_compile_time_shape(host, contexts):
    """150-base singles at k = 55 take a compile-time shape of k_pe_tiles, as pairs of that length do."""
    reads = uc.shape_block()
    ctx = contexts("golden")
    _check(_count(host, ctx, reads), uc.expected("golden", reads))
    assert ctx.last_kernel.startswith("k_pe_tiles<1, 10u, 4u"), ctx.last_kernel


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_map_ends(host, contexts, graph):
    """vs_pe_map_ends on a singles block: the model's lists for the even ends, nothing for the absent ones"""
    g = uc.GRAPHS[graph]()
    reads = uc.block(graph, 77)
    ctx = contexts(graph)
    lists = ctx.map_ends(ctx.pack_singles(reads), cap=max(len(g.seqs), 1))
    want = g.model.lists(reads)
    assert len(lists) == 2 * len(reads)
    for r in range(len(reads)):
        assert lists[2 * r] == want[r], (r, reads[r])
        assert lists[2 * r + 1] == []
    assert sum(len(l) > 1 for l in want) > 0


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_unpack_and_info(host, contexts, graph):
    """read r at end 2r; end 2r+1 of length 0, flagged absent (bit 3) and nothing else"""
    reads = uc.block(graph, 33)
    block = contexts(graph).pack_singles(reads)
    text, lens, flags = block.unpack()
    assert [int(x) for x in lens[0::2]] == [len(s) for s in reads]
    assert not lens[1::2].any() and all(int(f) == 8 for f in flags[1::2]) and not (flags[0::2] & 8).any()
    want = "".join("".join(c if c in "ACGT" else "A" for c in s) for s in reads)
    assert text.tobytes().decode() == want
    info = block.info
    assert info["ends"] == 66 and info["words"] == sum((len(s) + 15) // 16 for s in reads) and info["max_len"] == max(len(s) for s in reads)
    pairs = contexts(graph).pack_pairs(list(reads[:4]), list(reads[4:8]))
    assert not pairs.unpaired


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_hand_built_block_with_empty_second_ends(host, contexts, graph):
    """What singles were before: a PAIRS block of (read, "") counts nothing, because the empty end makes the pair short."""
    reads = uc.block(graph, 33)
    ctx = contexts(graph)
    counter = host.PeCounter(ctx)
    counter.add(ctx.pack_pairs(list(reads), [""] * len(reads)))
    node_mat, short_mat, stats = counter.result()
    n_with_n = sum(1 for s in reads if "N" in s)
    assert not node_mat.any() and not short_mat.any() and stats == (n_with_n, len(reads) - n_with_n, 0)
    counter.add(ctx.pack_singles(reads))
    assert np.array_equal(counter.result()[1], uc.expected(graph, reads)[1])


@pytest.mark.parametrize("graph", sorted(uc.GRAPHS))
def test_pairs_and_singles_into_one_counter(host, contexts, graph):
    """A pairs block and a singles block into one counter: the sum of both, each kind in its own tallies"""
    from oracle import pe_oracle

    g = uc.GRAPHS[graph]()
    ctx = contexts(graph)
    reads = uc.block(graph, 77)
    fwd, rve = list(reads[0:60:2]), list(reads[1:60:2])
    want_pairs = pe_oracle.pe_matrices(g.seqs, fwd, rve, g.k, table=g.model.table)
    want_single = uc.expected(graph, reads)
    counter = host.PeCounter(ctx)
    counter.add(ctx.pack_pairs(fwd, rve))
    counter.add(ctx.pack_singles(reads))
    counter.add(ctx.pack_pairs(fwd, rve))
    node_mat, short_mat, stats = counter.result()
    assert np.array_equal(node_mat, 2 * want_pairs[0])
    assert np.array_equal(short_mat, 2 * want_pairs[1] + want_single[1])
    assert stats == tuple(2 * int(x) for x in want_pairs[2])
    assert tuple(int(x) for x in counter.single_stats.cpu().numpy()) == want_single[2]
    counter.reset()
    assert not counter.single_stats.any()
