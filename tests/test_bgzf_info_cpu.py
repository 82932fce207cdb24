"""pe_info / st_info as BGZF without a device: the host twin of the device writer (``vs_write_info_bgzf_host``: the kernels'
text for the lines, the kernel's text for the members, one thread) against the committed files of the real reference
script -- dense: byte for byte once inflated; sparse: without their ``:0`` lines --, the shape of the file, and the readers
that take such a file back.  gzip and zlib are the oracle; every comparison is exact."""
import gzip
import os
import types

import numpy as np
import pytest

import bgzf_util as bu
import deflate_cases as dc
import sparse_info_util as su
from conftest import pe_cases
from oracle import pe_oracle


def _read_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_golden_cases_through_the_twin(tmp_path, name, d, meta):
    ids, _ = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    mats = dc.golden_matrices(d, ids)
    for upper, f in enumerate(("pe_info", "st_info")):
        dense_text = _read_bytes(os.path.join(d, f))
        for dense, want in ((1, dense_text), (0, su.filtered(dense_text.decode()).encode())):
            p = tmp_path / (f + ".gz")
            rc, info = dc.write_bgzf_host(p, ids, mats[upper], None, None, None, upper, dense)
            assert rc == 0
            dc.check_file(p, want, info)
            assert info[2] == (1 if want else 0)


@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
def test_tile_map_wide_totals_and_renumbering(tmp_path, upper):
    """257 nodes, cells on both sides of the internal diagonal, a dirty-tile map with unmarked tiles, totals folded into
    ``wide`` up to 19 digits, a permuted numbering: about a megabyte of dense text, 17 members."""
    c = su.crafted(257, upper, True, True)
    dense_text = pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], upper)).encode()
    assert dense_text.count(b"\n") == 257 * 257
    p = tmp_path / "info.gz"
    rc, info = dc.write_bgzf_host(p, c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper, 1)
    assert rc == 0
    dc.check_file(p, dense_text, info)
    assert info[4] == (len(dense_text) + dc.MAX_TEXT - 1) // dc.MAX_TEXT > 10
    rc, info = dc.write_bgzf_host(p, c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper, 0)
    assert rc == 0
    dc.check_file(p, c["want"].encode(), info)
    # the text is the plain writer's, and so are the lines and the cells it read
    rc, plain = su.write_host(tmp_path / "plain", c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper)
    assert rc == 0 and info[:4] == plain and _read_bytes(tmp_path / "plain") == c["want"].encode()


@pytest.mark.parametrize("dense", [0, 1], ids=["sparse", "dense"])
def test_small_blocks_cut_members_short_and_keep_the_text(tmp_path, monkeypatch, dense):
    """Members never span blocks: with VS_TEXT_BLOCK small every block ends in a short member, the inflated text stays."""
    c = su.crafted(130, 1, True, True)
    want = pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], 1)).encode() if dense else c["want"].encode()
    p = tmp_path / "st_info.gz"
    blocks, members = [], []
    for block in su.BLOCKS:
        monkeypatch.setenv("VS_TEXT_BLOCK", block)
        rc, info = dc.write_bgzf_host(p, c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], 1, dense)
        assert rc == 0
        dc.check_file(p, want, info)
        blocks.append(info[2])
        members.append(info[4])
    assert blocks == sorted(blocks, reverse=True) and blocks[0] > 2 and blocks[0] > blocks[3] == (1 if len(want) <= 100000 else 3)
    assert all(m >= b and m >= (len(want) + dc.MAX_TEXT - 1) // dc.MAX_TEXT for m, b in zip(members, blocks))


def test_zeros_negative_totals_and_a_stale_file(tmp_path):
    from vstrains_amd import _native as nat

    p = tmp_path / "info.gz"
    ids = su.make_ids(65)
    zeros = np.zeros((65, 65), dtype=np.uint32)
    for upper in (0, 1):
        p.write_bytes(b"stale" * 100)
        rc, info = dc.write_bgzf_host(p, ids, zeros, None, None, None, upper, 0)  # sparse: the EOF member alone
        assert rc == 0 and info == [0, 0, 0, info[3], 0, 28] and _read_bytes(p) == bu.EOF_MARK
        p.write_bytes(b"stale" * 10000)
        rc, info = dc.write_bgzf_host(p, ids, zeros, None, None, None, upper, 1)  # dense: 65 * 65 lines of zeros
        assert rc == 0
        dc.check_file(p, pe_oracle.matrix_text(ids, zeros.astype(np.int64)).encode(), info)
    rc, info = dc.write_bgzf_host(p, [], np.zeros((0, 0), dtype=np.uint32), None, None, None, 0, 1)  # no nodes at all
    assert rc == 0 and _read_bytes(p) == bu.EOF_MARK and info[5] == 28
    for upper, cell in ((0, (2, 1)), (1, (2, 1)), (1, (1, 1))):
        wide = np.zeros((3, 3), dtype=np.int64)
        wide[cell] = -5
        counts = np.full((3, 3), 7, dtype=np.uint32)
        counts[cell] = 4
        for dense in (0, 1):
            rc, _ = dc.write_bgzf_host(p, su.make_ids(3), counts, wide, None, None, upper, dense)
            assert rc == nat.VS_E_ARG and b"negative" in nat.lib().vs_last_error(None)
    rc, _ = dc.write_bgzf_host(tmp_path / "no" / "dir.gz", ids, zeros, None, None, None, 0, 1)
    assert rc == nat.VS_E_ARG and b"cannot open" in nat.lib().vs_last_error(None)


# ---- reading them back ------------------------------------------------------------------------------------------------------
def _python_cells(names, path):
    from vstrains_amd.graph.formats import read_pe_text

    index = {n: i for i, n in enumerate(names)}
    return [(index[u], index[v], c) for u, v, c in read_pe_text(str(path)) if u in index and v in index]


def _native_cells(names, path):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    got = HipPeLinks._parse_cells(names, str(path))
    if got is None:
        return None
    return [(int(r), int(c), int(v)) for r, c, v in zip(*got)]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """a dense and a sparse .gz of 130 nodes with their plain texts"""
    c = su.crafted(130, 0, False, True)
    root = tmp_path_factory.mktemp("bgzf_info")
    dense_text = pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], 0))
    out = {}
    for dense, text in ((1, dense_text), (0, c["want"])):
        p = root / ("pe_info_%d.gz" % dense)
        assert dc.write_bgzf_host(p, c["ids"], c["counts"], c["wide"], None, c["rank"], 0, dense)[0] == 0
        plain = root / ("pe_info_%d" % dense)
        with open(plain, "w", newline="") as fh:
            fh.write(text)
        out[dense] = (p, plain)
    return c["ids"], out


@pytest.mark.parametrize("dense", [0, 1], ids=["sparse", "dense"])
def test_both_readers_take_the_gz_file(written, dense):
    ids, files = written
    gz, plain = files[dense]
    want = _python_cells(ids, plain)
    assert len(want) > 500
    assert _native_cells(ids, gz) == want == _native_cells(ids, plain)
    assert _python_cells(ids, gz) == want
    some = ids[::3]  # a subset of the names: the id filter is the plain file's
    assert _native_cells(some, gz) == _python_cells(some, plain)


def test_line_count_flags_and_plain_gzip(written, tmp_path):
    """cap == 0 counts the lines of the inflated text; a '\\r' or a high byte inside the gzip sets the plain file's flags, and
    the Python loop, which such a file falls back to, reads it through gzip with universal newlines; any gzip will do."""
    import ctypes as C

    from vstrains_amd import _native as nat

    ids, files = written
    blob, off = su.encode_ids(["a", "b"])
    info = (C.c_uint64 * 4)()

    def count(path):
        assert nat.lib().vs_info_parse(str(path).encode(), blob.ctypes.data, off.ctypes.data, 2, None, None, None, 0, info) == 0
        return [int(x) for x in info]

    assert count(files[1][0]) == count(files[1][1]) and count(files[1][0])[0] == 130 * 130
    p = tmp_path / "st_info.gz"
    for raw, flag in ((b"a:b:1\r\nb:b:2\r\n", 1), (b"a:b:1\rb:b:2\n", 1), (b"a:\xc3\xa9:1\n", 2)):
        p.write_bytes(bu.bgzf(raw))
        assert count(p)[:2] == [0, flag]
        assert _native_cells(["a", "b"], p) is None
    p.write_bytes(bu.bgzf(b"a:b:1\r\nb:b:2\r\n"))
    assert _python_cells(["a", "b"], p) == [(0, 1, 1), (1, 1, 2)]
    # plain gzip, two members, and a text that stops at its first empty line
    p.write_bytes(gzip.compress(b"a:b:1\nb:a:2\n") + gzip.compress(b"b:b:3\n\nb:b:oops\n"))
    assert _native_cells(["a", "b"], p) == [(0, 1, 1), (1, 0, 2), (1, 1, 3)] == _python_cells(["a", "b"], p)
    p.write_bytes(bu.EOF_MARK)  # no text at all
    assert _native_cells(["a", "b"], p) == [] == _python_cells(["a", "b"], p)


def test_a_cut_or_corrupt_gz_is_an_error_not_a_short_table(written, tmp_path):
    ids, files = written
    data = _read_bytes(files[1][0])
    p = tmp_path / "pe_info.gz"
    p.write_bytes(data[:len(data) // 2])  # cut in the middle of a member
    with pytest.raises(ValueError):
        _native_cells(ids, p)
    with pytest.raises((EOFError, OSError)):
        _python_cells(ids, p)
    members, _, _ = bu.py_walk(data)
    first = members[0][0] + members[0][1] + 8  # cut exactly behind the first member's trailer: a whole gzip stream, but
    p.write_bytes(data[:first] + data[first:first + 40])  # ... followed by a member that ends after 40 bytes
    with pytest.raises(ValueError):
        _native_cells(ids, p)
    bad = bytearray(data)
    bad[members[0][0] + 200] ^= 0x55  # a flipped payload byte: zlib's data error or the CRC32
    p.write_bytes(bytes(bad))
    with pytest.raises(ValueError):
        _native_cells(ids, p)


# ---- PeCounter on CPU tensors, and the file names -------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_counter_on_cpu_tensors_writes_through_the_twin(tmp_path, dense):
    import torch
    from vstrains_amd import pe as host
    from vstrains_amd import pe_inference

    n = 130
    node, short = su.crafted(n, 0, True, True), su.crafted(n, 1, True, True)
    rank = node["rank"].astype(np.int64)
    order = np.empty(n, dtype=np.int64)
    order[rank] = np.arange(n)
    ctx = types.SimpleNamespace(n_nodes=n, device=0, _h=None, node_order=order, node_rank=rank)
    counter = host.PeCounter(ctx, device="cpu", track_tiles=True)
    counter.mats.copy_(torch.from_numpy(np.stack([node["counts"], np.triu(short["counts"])]).view(np.int32)))
    counter.tile_map.copy_(torch.from_numpy(np.concatenate([node["tile_map"], short["tile_map"]])))
    counter.wide = torch.from_numpy(np.stack([node["wide"], np.triu(short["wide"])]))
    name, stats = pe_inference.write_info_files(str(tmp_path), node["ids"], counter, sparse=not dense, bgzf=True)
    assert name == str(tmp_path) + "/pe_info.gz" and sorted(os.listdir(tmp_path)) == ["pe_info.gz", "st_info.gz"]
    info = counter.write_bgzf_text(str(tmp_path / "pe_info.gz"), str(tmp_path / "st_info.gz"), node["ids"], dense=dense)
    node_mat, short_mat, _ = counter.result()
    for f, mat, inf in (("pe_info.gz", node_mat, info[0]), ("st_info.gz", short_mat, info[1])):
        want = pe_oracle.matrix_text(node["ids"], mat)
        want = (want if dense else su.filtered(want)).encode()
        assert tuple(inf) == dc.INFO_KEYS
        dc.check_file(tmp_path / f, want, [inf[k] for k in dc.INFO_KEYS])


def test_the_flag_clash_exits_before_anything_is_created(tmp_path):
    from vstrains_amd import cli

    with pytest.raises(SystemExit):
        cli.main(["-a", "spades", "-g", "g.gfa", "-p", "c.paths", "-o", str(tmp_path / "never"), "-fwd", "f.fq", "-rve", "r.fq",
                  "--bgzf-pe-text", "--no-pe-text"])
    assert not os.path.exists(tmp_path / "never")
    args = cli.build_parser().parse_args(["-a", "spades", "-g", "g.gfa", "-p", "c.paths", "-o", "o", "-fwd", "f.fq", "-rve", "r.fq"])
    assert args.bgzf_pe_text is False  # off by default
