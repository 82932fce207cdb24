"""pe_info / st_info read on the device (vs_links_from_info: k_inflate, k_info_scan, k_info_parse) against the host route
(``from_files(device_parse=False)``: vs_info_parse + vs_links_from_cells, the code of the commit before) on a counted workload
of a few hundred nodes, and against the hand-written outcomes of info_read_cases.py on constructed texts, plain and as BGZF
whose members cut the lines.  Every comparison is exact; ``HipPeLinks.last_read`` says which route a file took."""
import gzip
import os

import numpy as np
import pytest

import bgzf_util as bu
import info_read_cases as irc

pytestmark = pytest.mark.gpu


def _read_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


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
def links():
    from vstrains_amd.graph.hip_ops import HipPeLinks

    return HipPeLinks


@pytest.fixture(scope="module")
def workload(host, ctx):
    """A random graph of a few hundred nodes counted under the default renumbering, with a dirty-tile map."""
    from vstrains_amd import synth

    st = synth.make_strains(5, 4000, 0.03, seed=11)
    g = synth.compact_dbg(st, 21)
    fwd, rve = synth.sample_pairs(st, 3000, 100, seed=12, sub_rate=0.005, n_rate=0.01)
    ids = ["%d%s" % (i, "&%d*0" % i if i % 5 == 0 else "") for i in range(len(g.seqs))]
    assert 100 <= len(ids) <= 400
    ctx.build_index(g.seqs, 21)
    counter = host.PeCounter(ctx, track_tiles=True)
    counter.add(ctx.pack_pairs(fwd, rve))
    return ids, counter


KINDS = {"plain_dense": {}, "plain_sparse": dict(sparse=True), "dense_gz": dict(bgzf=True), "sparse_gz": dict(bgzf=True, sparse=True)}


@pytest.fixture(scope="module")
def pairs(workload, tmp_path_factory):
    from vstrains_amd import pe_inference

    ids, counter = workload
    root = tmp_path_factory.mktemp("pairs")
    out = {}
    for key, kw in KINDS.items():
        os.makedirs(root / key)
        pe_inference.write_info_files(str(root / key), ids, counter, **kw)
        suffix = ".gz" if kw.get("bgzf") else ""
        out[key] = (str(root / key / ("pe_info" + suffix)), str(root / key / ("st_info" + suffix)))
    return out


@pytest.fixture(scope="module")
def wanted(ctx, links, workload, pairs):
    """the tables of the host route, dense and CSR, from the plain dense pair: computed once, never written to"""
    ids, _ = workload
    out = {s: links.from_files(ctx, ids, *pairs["plain_dense"], sparse_min_nodes=s, device_parse=False).to_numpy() for s in (0, 64)}
    assert out[0].any() and np.array_equal(out[0], out[64])
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("sparse_min_nodes", [0, 64], ids=["dense-table", "csr-table"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_tables_of_the_four_file_kinds(ctx, links, workload, pairs, wanted, kind, sparse_min_nodes):
    ids, _ = workload
    host_table = links.from_files(ctx, ids, *pairs[kind], sparse_min_nodes=sparse_min_nodes, device_parse=False).to_numpy()
    assert np.array_equal(host_table, wanted[sparse_min_nodes])
    assert links.last_read["pe"]["route"] == "host"
    table = links.from_files(ctx, ids, *pairs[kind], sparse_min_nodes=sparse_min_nodes, device_parse=True)
    read = links.last_read
    assert np.array_equal(table.to_numpy(), host_table)
    route = "bgzf_device" if kind.endswith("_gz") else "plain_device"
    for f, path in zip(("pe", "st"), pairs[kind]):
        rec = read[f]
        text = gzip.decompress(_read_bytes(path)) if kind.endswith("_gz") else _read_bytes(path)
        assert rec["route"] == route and rec["flags"] == 0 and rec["windows"] == 1, rec
        assert (rec["lines"], rec["skipped"], rec["cells"], rec["text_bytes"]) == (text.count(b"\n"), 0, text.count(b"\n"), len(text))
        assert (rec["members_device"] > 0) == kind.endswith("_gz")


def _outcome(links, ctx, names, pe, st, **kw):
    try:
        table = links.from_files(ctx, names, pe, st, **kw)
    except Exception as e:  # (the type and the text are what is compared)
        return ("raised", type(e), str(e))
    return ("table", table.to_numpy().tolist(), links.last_read["pe"]["route"])


@pytest.mark.parametrize("form", ["plain", "bgzf64"])
@pytest.mark.parametrize("case", irc.CASES, ids=irc.CASE_IDS)
def test_constructed_texts_on_the_device(ctx, links, tmp_path, case, form):
    """as plain text and as BGZF with members of 64 bytes of text, so that lines straddle members"""
    pe, st = tmp_path / "pe_info", tmp_path / "st_info"
    pe.write_bytes(case.text if form == "plain" else bu.bgzf(case.text, 6, block=64))
    st.write_bytes(b"")
    on_host = _outcome(links, ctx, case.names, str(pe), str(st), device_parse=False)
    on_device = _outcome(links, ctx, case.names, str(pe), str(st), device_parse=True)
    assert on_device[:2] == on_host[:2]
    if case.kind == "ok":
        assert on_device[1] == case.matrix().tolist()
        if case.text:
            assert on_device[2] == ("plain_device" if form == "plain" else "bgzf_device")
    elif case.kind == "python":
        assert on_device[2] == "python" or on_device[0] == "raised"  # (a byte >= 0x80: Python's decoder raises, on both routes)
    else:
        assert on_device[0] == "raised" and on_device[1] is ValueError and on_device[2] == case.message(str(pe))
    # the same text as the second file, behind a first file that is read: the error is the second file's
    if case.kind == "error":
        st.write_bytes(_read_bytes(pe))
        pe.write_bytes(b"1:2:1\n")
        got = _outcome(links, ctx, case.names, str(pe), str(st), device_parse=True)
        assert got == ("raised", ValueError, case.message(str(st)))


def test_both_files_add_into_one_table(ctx, links, tmp_path):
    pe, st = tmp_path / "pe_info", tmp_path / "st_info.gz"
    pe.write_bytes(b"1:2:3\n2:2:1\n")
    st.write_bytes(bu.bgzf(b"2:1:4\n3:1:-2\n", 6))
    for s in (0, 2):
        got = links.from_files(ctx, irc.NAMES, str(pe), str(st), sparse_min_nodes=s).to_numpy()
        assert got.tolist() == [[0, 7, -2], [7, 1, 0], [-2, 0, 0]]
        assert [links.last_read[f]["route"] for f in ("pe", "st")] == ["plain_device", "bgzf_device"]


@pytest.mark.parametrize("sparse_min_nodes", [0, 64], ids=["dense-table", "csr-table"])
def test_windows(ctx, links, workload, pairs, wanted, sparse_min_nodes):
    ids, _ = workload
    # a window that holds one member and the line carried, not two whole members: the sparse .gz pair, and the dense one,
    # which has many members
    for kind in ("sparse_gz", "dense_gz"):
        texts = [gzip.decompress(_read_bytes(p)) for p in pairs[kind]]
        got = links.from_files(ctx, ids, *pairs[kind], sparse_min_nodes=sparse_min_nodes, window_bytes=bu.MAX_IN + 4096)
        assert np.array_equal(got.to_numpy(), wanted[sparse_min_nodes])
        for f, t in zip(("pe", "st"), texts):
            rec = links.last_read[f]
            assert rec["route"] == "bgzf_device" and rec["windows"] >= max(1, len(t) // bu.MAX_IN) and rec["lines"] == t.count(b"\n"), rec
            if kind == "dense_gz":
                assert rec["windows"] > 2 and rec["members_device"] > rec["windows"] - 2
    got = links.from_files(ctx, ids, *pairs["plain_dense"], sparse_min_nodes=sparse_min_nodes, window_bytes=4096)
    assert np.array_equal(got.to_numpy(), wanted[sparse_min_nodes])
    for f, p in zip(("pe", "st"), pairs["plain_dense"]):
        rec = links.last_read[f]
        assert rec["route"] == "plain_device" and rec["windows"] >= os.path.getsize(p) // 4096 > 1 and rec["lines"] == len(ids) ** 2, rec


def test_a_line_longer_than_the_window_takes_the_host_route(ctx, links, workload, pairs, wanted, tmp_path):
    ids, _ = workload
    pe = tmp_path / "pe_info"
    lines = _read_bytes(pairs["plain_sparse"][0]).split(b"\n")
    lines[len(lines) // 2] += b":" + b"7" * 5000  # (fields behind the third are ignored)
    pe.write_bytes(b"\n".join(lines))
    for s in (0, 64):
        got = links.from_files(ctx, ids, str(pe), pairs["plain_sparse"][1], sparse_min_nodes=s, window_bytes=4096)
        assert np.array_equal(got.to_numpy(), wanted[s])
        assert [links.last_read[f]["route"] for f in ("pe", "st")] == ["host", "plain_device"]


def test_other_gzip_files_take_the_host_route(ctx, links, workload, pairs, wanted, tmp_path):
    ids, _ = workload
    text = gzip.decompress(_read_bytes(pairs["sparse_gz"][0]))
    half = text.index(b"\n", len(text) // 2) + 1
    pe = tmp_path / "pe_info.gz"
    for data in (gzip.compress(text), bu.bgzf(text[:half], 6, eof=False) + gzip.compress(text[half:])):
        pe.write_bytes(data)
        for s in (0, 64):
            got = links.from_files(ctx, ids, str(pe), pairs["sparse_gz"][1], sparse_min_nodes=s)
            assert np.array_equal(got.to_numpy(), wanted[s])
            assert [links.last_read[f]["route"] for f in ("pe", "st")] == ["host", "bgzf_device"]


def test_corrupt_and_cut_gz_are_errors_as_on_the_host_route(ctx, links, workload, pairs, tmp_path):
    ids, _ = workload
    data = _read_bytes(pairs["dense_gz"][0])
    members, at, state = bu.py_walk(data)
    assert state == 0 and len(members) >= 5
    off, length, _, _ = members[len(members) // 2]
    flipped = bytearray(data)
    flipped[off + length // 2] ^= 0x10
    pe = tmp_path / "pe_info.gz"
    for bad in (bytes(flipped), data[:len(data) // 2]):
        pe.write_bytes(bad)
        on_host = _outcome(links, ctx, ids, str(pe), pairs["dense_gz"][1], device_parse=False)
        on_device = _outcome(links, ctx, ids, str(pe), pairs["dense_gz"][1], device_parse=True)
        assert on_host[0] == "raised" and on_host[1] is ValueError
        assert on_device == on_host
    # the context still works
    assert links.from_files(ctx, ids, *pairs["dense_gz"]).to_numpy().any()


def test_reserved_table_is_taken_and_given_back(ctx, links, workload, pairs, wanted, tmp_path):
    from vstrains_amd import _native as nat

    ids, _ = workload
    nat.check(ctx._h, nat.lib().vs_links_reserve(ctx._h, len(ids)))
    bad = tmp_path / "st_info"
    bad.write_bytes(b"1:2:3\r\n")
    got = links.from_files(ctx, ids, pairs["plain_sparse"][0], str(bad))  # Python's to read: the buffer goes back, then is taken
    assert links.last_read["pe"]["route"] == "python" and got.to_numpy().any()
    nat.check(ctx._h, nat.lib().vs_links_reserve(ctx._h, len(ids)))
    assert np.array_equal(links.from_files(ctx, ids, *pairs["sparse_gz"]).to_numpy(), wanted[0])
    nat.check(ctx._h, nat.lib().vs_links_reserve(ctx._h, 0))


def test_reference_api_takes_the_device_route(links, workload, pairs, wanted):
    from vstrains_amd.graph import reference_api as ra

    ids, _ = workload
    got = ra.process_pe_info(ids, *pairs["dense_gz"])[1].to_numpy()
    assert np.array_equal(got, wanted[0])
    assert [links.last_read[f]["route"] for f in ("pe", "st")] == ["bgzf_device", "bgzf_device"]


def _tree(root):
    out = {}
    for base, _, files in os.walk(root):
        for fn in files:
            rel = os.path.relpath(os.path.join(base, fn), root)
            if rel != "vstrains.log" and not rel.startswith("aln" + os.sep):
                out[rel] = _read_bytes(os.path.join(base, fn))
    return out


def test_whole_command_from_the_files_of_an_earlier_run(links, tmp_path):
    from graph_case import Case
    from vstrains_amd import cli

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    argv = ["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-fwd", inp["fwd"], "-rve", inp["rve"]]
    first, again = str(tmp_path / "first"), str(tmp_path / "again")
    cli.main(argv + ["-o", first, "--bgzf-pe-text"])
    assert sorted(os.listdir(os.path.join(first, "aln"))) == ["pe_info.gz", "st_info.gz"]
    links.last_read = None
    cli.main(argv + ["-o", again, "--pe-text-from", os.path.join(first, "aln")])
    assert [links.last_read[f]["route"] for f in ("pe", "st")] == ["bgzf_device", "bgzf_device"]
    a, b = _tree(first), _tree(again)
    assert "strain.paths" in a and "strain.fasta" in a and len(a) > 5
    assert a == b
    assert os.listdir(os.path.join(again, "aln")) == []
    log = open(os.path.join(again, "vstrains.log")).read()
    assert "paired end information is read from" in log and "WARNING" not in log
