"""The same pairs through every route that builds a read block -- ``Context.pack_pairs`` (host bytes + offsets),
``FastqPair.block`` (mapped ingest), ``FastqStream`` (streamed ingest, in one block and in tiny chunks and blocks) -- give
the same block: text, lengths and flags as a model written here says, the same ``info``, and (this is how ``mask`` and
``inv4`` are seen, which have no export) the same ``map_ends`` and the same PE counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 21
N_PAIRS = 40
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 150, 254, 255, 256, 257, 300)  # every one occurs; the other ends are 150 long
ROUTES = ("pack_pairs", "mapped", "stream_one_block", "stream_chunk61_blocks7")


def _pairs():
    """(graph, fwd, rve) of the dirty variant: ends sampled from the graph's genomes, some of them edited"""
    from vstrains_amd import synth

    st = synth.make_strains(3, 1500, 0.03, seed=5)
    g = synth.compact_dbg(st, K)
    rng = np.random.default_rng(6)
    # (ends 0 .. 7 stay 150 long for the edits below; the special lengths are spread over both files among the others)
    rest = list(LENGTHS) + [150] * (2 * N_PAIRS - 8 - len(LENGTHS))
    lens = [150] * 8 + [rest[int(i)] for i in rng.permutation(len(rest))]
    ends = []
    for e, n in enumerate(lens):
        genome = st.genomes[int(rng.integers(0, len(st.genomes)))]
        start = int(rng.integers(0, len(genome) - n + 1))
        s = genome[start:start + n]
        ends.append(synth.revcomp(s) if (e & 1) else s)

    def edit(e, changes):
        b = bytearray(ends[e].encode())
        for pos, ch in changes:
            b[pos] = ord(ch)
        ends[e] = b.decode()

    def end_of_len(n):
        return lens.index(n)

    edit(0, [(40, "N")])                                                # an N
    edit(3, [(10, "a")])                                                # a lower-case base
    edit(4, [(0, "*"), (17, "N"), (100, "x"), (149, "-")])              # exactly four bytes outside ACGT
    edit(7, [(5, "*"), (16, "n"), (31, "N"), (32, "R"), (140, ".")])    # five
    edit(end_of_len(300), [(254, "*")])                                 # the last position inv4 holds
    edit(end_of_len(256), [(255, "*")])                                 # the first it does not
    edit(end_of_len(257), [(255, "N")])                                 # an N there, nothing else: not MANY
    return g, ends[0::2], ends[1::2]


def _model(fwd, rve):
    """(text, lens, flags) as ReadBlock.unpack gives them"""
    text, lens, flags = [], [], []
    for pair in zip(fwd, rve):
        for s in pair:
            bad = [p for p, c in enumerate(s) if c not in "ACGT"]
            fl = (1 if "N" in s else 0) | (2 if any(s[p] != "N" for p in bad) else 0)
            if (fl & 2) and (len(bad) > 4 or any(p >= 255 for p in bad[:4])):
                fl |= 4
            text.append("".join(c if c in "ACGT" else "A" for c in s))
            lens.append(len(s))
            flags.append(fl)
    return (np.frombuffer("".join(text).encode(), dtype=np.uint8), np.array(lens, dtype=np.uint32), np.array(flags, dtype=np.uint8))


def _measure(host, ctx, blocks):
    """what the tests compare, over the blocks of one route in order"""
    counter = host.PeCounter(ctx)
    unpacked, infos, mapped = [], [], []
    for b in blocks:
        unpacked.append(b.unpack())
        infos.append(b.info)
        mapped += ctx.map_ends(b)
        counter.add(b)
    node_mat, short_mat, stats = counter.result()
    info = {k: sum(int(i[k]) for i in infos) for k in ("ends", "words", "invalid_ends")}
    info["max_len"] = max(int(i["max_len"]) for i in infos)
    return dict(unpack=tuple(np.concatenate([u[j] for u in unpacked]) for j in range(3)), info=info, map_ends=mapped,
                counters=(node_mat, short_mat, stats), n_blocks=len(infos))


@pytest.fixture(scope="module", params=["dirty", "clean"])
def routes(request, tmp_path_factory):
    """variant -> (fwd, rve, {route: measurements}); everything computed once"""
    from vstrains_amd import pe as host
    from vstrains_amd import synth

    g, fwd, rve = _pairs()
    if request.param == "clean":  # only ACGT and N: the mapped route keeps its host packer
        fwd, rve = (["".join(c if c in "ACGT" else "N" for c in s) for s in lst] for lst in (fwd, rve))
    tmp = tmp_path_factory.mktemp(request.param)
    pf, pr = str(tmp / "f.fq"), str(tmp / "r.fq")
    for path, reads, tag in ((pf, fwd, "f"), (pr, rve, "r")):
        with open(path, "wb") as fh:
            fh.write(synth.fastq_text(reads, tag).encode("ascii"))
    ctx = host.Context(0)
    ctx.build_index(g.seqs, K)
    out = {}
    out["pack_pairs"] = _measure(host, ctx, [ctx.pack_pairs(fwd, rve)])
    fq = host.FastqPair(pf, pr, ctx)
    assert len(fq) == N_PAIRS
    out["mapped"] = _measure(host, ctx, [fq.block(0, N_PAIRS)])
    fq.close()
    fs = host.FastqStream(pf, pr, ctx, block_pairs=N_PAIRS)
    out["stream_one_block"] = _measure(host, ctx, list(fs))
    fs.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VS_STREAM_CHUNK", "61")
        fs = host.FastqStream(pf, pr, ctx, block_pairs=7)
        out["stream_chunk61_blocks7"] = _measure(host, ctx, list(fs))
        fs.close()
    yield request.param, fwd, rve, out
    ctx.close()


def test_input_holds_the_cases(routes):
    variant, fwd, rve, out = routes
    _, lens, flags = _model(fwd, rve)
    assert set(LENGTHS) <= set(int(x) for x in lens) and len(lens) == 2 * N_PAIRS
    if variant == "dirty":  # N alone; invalid; N + invalid; invalid + MANY; all three
        assert {1, 2, 3, 6, 7} <= set(int(x) for x in flags)
        assert int(flags[lens == 257][0]) == 1 and int(flags[lens == 300][0]) == 2 and int(flags[lens == 256][0]) == 6
    else:
        assert set(int(x) for x in flags) == {0, 1}
    assert out["stream_one_block"]["n_blocks"] == 1 and out["stream_chunk61_blocks7"]["n_blocks"] >= N_PAIRS // 7
    assert any(len(m) > 0 for m in out["pack_pairs"]["map_ends"])  # (the mapping is not trivial)
    assert out["pack_pairs"]["counters"][0].sum() > 0              # (nor is the counting)


@pytest.mark.parametrize("route", ROUTES)
def test_block_equals_model(routes, route):
    _, fwd, rve, out = routes
    want = _model(fwd, rve)
    got = out[route]["unpack"]
    for name, w, g_ in zip(("text", "lengths", "flags"), want, got):
        assert np.array_equal(w, g_), (route, name)
    info = out[route]["info"]
    lens, flags = want[1], want[2]
    assert info["ends"] == 2 * N_PAIRS
    assert info["words"] == int(((lens.astype(np.int64) + 15) // 16).sum())
    assert info["max_len"] == int(lens.max())
    assert info["invalid_ends"] == int(((flags & 2) != 0).sum())


@pytest.mark.parametrize("route", ROUTES[1:])
def test_routes_agree(routes, route):
    _, _, _, out = routes
    ref, got = out[ROUTES[0]], out[route]
    for a, b in zip(ref["unpack"], got["unpack"]):
        assert np.array_equal(a, b)
    assert got["info"] == ref["info"]
    assert got["map_ends"] == ref["map_ends"]
    assert np.array_equal(got["counters"][0], ref["counters"][0]) and np.array_equal(got["counters"][1], ref["counters"][1])
    assert got["counters"][2] == ref["counters"][2]
