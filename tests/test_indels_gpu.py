"""The indel pass on the device: ``k_node_indels`` through ``IndelCounter`` on the constructed blocks of tests/indel_cases.py at
k = 21, 55 and 127, beside ``PileupCounter`` on the same block, and one command end to end.  Every comparison is of exact
integers and strings against tests/indel_model.py."""
import gzip

import pytest

import indel_cases as cases
import indel_model as model

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


def _pack(host, ctx, case):
    return ctx.pack_singles(case.ends) if case.singles else ctx.pack(*host.encode_seqs(case.ends))


def device_indels(host, ctx, case, times: int = 1, first_cap: int = 4096, beside_pileup: bool = False):
    """A constructed case through ``IndelCounter`` -> (records, tallies, launches[, the pileup's result and tallies])."""
    ctx.build_index(case.seqs, case.k)
    counter = host.IndelCounter(ctx, max_len=case.G, first_cap=first_cap)
    plain = host.PileupCounter(ctx) if beside_pileup else None
    block = _pack(host, ctx, case)
    try:
        for _ in range(times):
            counter.add(block)
            if plain is not None:
                plain.add(block)
        got = (counter.result(), counter.tallies(), counter.launches)
        if plain is not None:
            got += (tuple(a.tolist() for a in plain.result()) + (plain.tallies(),),)
        ctx.sync()
        assert counter.ends_seen == times * len(case.ends)
        return got
    finally:
        block.free()
        ctx.keep_masks(False)


ALL = [c for k in cases.KS for c in cases.indel_cases(k)]


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_constructed_blocks_equal_the_model(host, ctx, case):
    want, want_tally = model.indels(case.seqs, case.k, case.ends, case.G)
    records, tally, launches = device_indels(host, ctx, case)
    assert records == want == case.records
    assert tally == want_tally and launches == 1
    if case.tally is not None:
        assert tally == case.tally


def _named(k, name):
    return [c for c in cases.indel_cases(k) if c.name == name][0]


@pytest.mark.parametrize("k", cases.KS)
def test_a_buffer_of_one_record_is_outgrown_once_and_the_tallies_are_counted_once(host, ctx, k):
    case = _named(k, "a_block_of_70_ends")
    want, want_tally = model.indels(case.seqs, k, case.ends, case.G)
    assert sum(r[5] + r[6] for r in want) == 6
    records, tally, launches = device_indels(host, ctx, case, first_cap=1)
    assert launches == 2  # the first call found six events for one place, the second had room
    assert records == want and tally == want_tally
    # the grown buffer is kept: the same block once more is one launch more and doubles every count
    records, tally, launches = device_indels(host, ctx, case, times=2, first_cap=1)
    assert launches == 3
    assert records == [r[:5] + (2 * r[5], 2 * r[6]) for r in want] and tally == tuple(2 * v for v in want_tally)


@pytest.mark.parametrize("k", cases.KS)
def test_the_pileup_counts_the_same_with_and_without_the_indel_counter_beside_it(host, ctx, k):
    for name in ("two_indels_in_one_end", "one_base_more_and_one_less_in_a_homopolymer"):
        case = _named(k, name)
        ctx.build_index(case.seqs, k)
        alone = host.PileupCounter(ctx)
        block = _pack(host, ctx, case)
        try:
            alone.add(block)
            want = tuple(a.tolist() for a in alone.result()) + (alone.tallies(),)
        finally:
            block.free()
            ctx.keep_masks(False)
        records, tally, _, beside = device_indels(host, ctx, case, beside_pileup=True)
        assert beside == want and records == case.records
        assert want[3][1] > 0  # (the ends that carry the events are what the pileup rejects)


def test_max_len_outside_1_to_32_is_refused(host, ctx):
    case = _named(21, "deletion_and_insertion_of_one_base")
    ctx.build_index(case.seqs, case.k)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            host.IndelCounter(ctx, max_len=bad)
    counter = host.IndelCounter(ctx, max_len=4)
    block = _pack(host, ctx, case)
    try:
        for bad in (0, 33):
            with pytest.raises(Exception) as err:
                ctx.node_indels(block, counter.first.data_ptr(), bad, counter.events.data_ptr(), counter.events.shape[0], counter.tally.data_ptr())
            assert "1 to 32" in str(err.value)
        assert counter.tallies() == (0, 0, 0, 0)
    finally:
        block.free()
        ctx.keep_masks(False)


def _fastq(path, reads):
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


def test_one_command_end_to_end_writes_the_expected_vcf(host, tmp_path):
    from vstrains_amd import node_depth

    k = 21
    K = k + 1
    case = _named(k, "two_indels_in_one_end")
    F = case.seqs[0]
    (_, u, _, _, _, _, _), (_, v, _, _, I, _, _) = case.records
    two = case.ends[0]
    n = 6
    exact = [F[a:a + 2 * K + 10] for a in range(0, len(F) - (2 * K + 10), 7)]
    fwd = [two] * n + exact
    rve = [model.revcomp(two)] * n + [model.revcomp(r) for r in reversed(exact)]
    gfa = tmp_path / "g.gfa"
    gfa.write_text("H\tVN:Z:1.0\nS\tseg_a\t%s\nS\tseg_b\t%s\n" % (F, case.seqs[1]))
    _fastq(tmp_path / "f.fq", fwd)
    _fastq(tmp_path / "r.fq", rve)
    out = tmp_path / "indels.vcf.gz"
    assert node_depth.main(["-g", str(gfa), "-o", str(tmp_path / "o.gfa"), "-f", str(tmp_path / "f.fq"), "-r", str(tmp_path / "r.fq"), "-k", str(k),
                            "--indels", str(out), "--indel-max-length", "4", "--min-alt-strand-count", "1"]) == 0
    with gzip.open(out, "rt") as fh:
        lines = fh.read().splitlines()
    records = [ln.split("\t") for ln in lines if not ln.startswith("#")]
    assert [ln for ln in lines if ln.startswith("##FILTER")] and lines[0] == "##fileformat=VCFv4.2"
    assert [r[:5] + r[6:7] for r in records] == [["seg_a", str(u), ".", F[u - 1:u + 2], F[u - 1], "PASS"], ["seg_a", str(v), ".", F[v - 1], F[v - 1] + I, "PASS"]]
    for r in records:
        info = dict(kv.split("=") for kv in r[7].split(";"))
        assert (info["AD"], info["ADF"], info["ADR"]) == (str(2 * n), str(n), str(n))
        assert int(info["DP"]) > 2 * n and info["AF"] == "%.6f" % (2 * n / int(info["DP"]))
