"""Sparse pe_info / st_info without a device: the host twin of the device writer (the same text, vs_info_core.h) against the
oracle's dense text without its ``:0`` lines, the claim that the reference reads such files to the same dict, and the
native parser against ``formats.read_pe_text`` plus the id filter.  Every comparison is exact."""
import os
import types

import numpy as np
import pytest

import sparse_info_util as su
from conftest import pe_cases
from oracle import graph_ops, pe_oracle


def _read(path):
    with open(path, "r", newline="") as fh:
        return fh.read()


@pytest.mark.parametrize("with_wide", [False, True], ids=["u32", "wide"])
@pytest.mark.parametrize("with_map", [False, True], ids=["nomap", "map"])
@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
@pytest.mark.parametrize("n", su.SIZES)
def test_host_twin_writes_the_filtered_oracle_text(tmp_path, n, upper, with_map, with_wide):
    c = su.crafted(n, upper, with_map, with_wide)
    p = tmp_path / "info"
    rc, info = su.write_host(p, c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper)
    assert rc == 0
    got = _read(p)
    assert got == c["want"]
    assert "\n\n" not in got and not got.startswith("\n")  # (the reference stops reading at an empty line)
    assert info[0] == got.count("\n") and info[1] == len(got.encode("latin-1"))
    cells = n * (n + 1) // 2 if upper else n * n
    if with_map and not with_wide and n > 64:
        assert info[3] < (2 * cells if upper else cells)  # unmarked tiles were skipped without a read
    if not with_map:
        assert info[3] == (n * n if upper else cells)  # (above the diagonal the short_mat rule reads two cells)


def test_identity_numbering_and_wide_totals_alone(tmp_path):
    c = su.crafted(65, 1, False, True, with_rank=False)
    assert c["rank"] is None
    p = tmp_path / "info"
    assert su.write_host(p, c["ids"], c["counts"], c["wide"], None, None, 1)[0] == 0
    assert _read(p) == c["want"]
    total = c["counts"].astype(np.int64) + c["wide"]  # the same totals held in int64 alone: no uint32 cells at all
    assert su.write_host(p, c["ids"], None, total, None, None, 1)[0] == 0
    assert _read(p) == c["want"]


def test_a_matrix_of_zeros_gives_an_empty_file(tmp_path):
    p = tmp_path / "info"
    p.write_text("stale")
    for upper in (0, 1):
        rc, info = su.write_host(p, su.make_ids(65), np.zeros((65, 65), dtype=np.uint32), None, None, None, upper)
        assert rc == 0 and info[:3] == [0, 0, 0]
        assert os.path.getsize(p) == 0
    rc, info = su.write_host(p, [], np.zeros((0, 0), dtype=np.uint32), None, None, None, 0)  # no nodes at all
    assert rc == 0 and os.path.getsize(p) == 0


def test_a_negative_total_is_refused(tmp_path):
    from vstrains_amd import _native as nat

    ids = su.make_ids(3)
    for upper, cell in ((0, (2, 1)), (1, (2, 1)), (1, (1, 1))):
        wide = np.zeros((3, 3), dtype=np.int64)
        wide[cell] = -5
        counts = np.full((3, 3), 7, dtype=np.uint32)
        counts[cell] = 4  # (4 + -5 < 0; in the short_mat rule the mirror cell's 7 must not hide it)
        rc, _ = su.write_host(tmp_path / "info", ids, counts, wide, None, None, upper)
        assert rc == nat.VS_E_ARG
        assert b"negative" in nat.lib().vs_last_error(None)


def test_a_rank_outside_the_matrix_is_refused(tmp_path):
    from vstrains_amd import _native as nat

    rc, _ = su.write_host(tmp_path / "info", su.make_ids(3), np.ones((3, 3), dtype=np.uint32), None, None, np.asarray([0, 3, 1], dtype=np.uint32), 0)
    assert rc == nat.VS_E_RANGE


@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
def test_same_bytes_for_every_block_size(tmp_path, monkeypatch, upper):
    """Blocks of whole rows, as the dense writer cuts them: the same bytes whatever VS_TEXT_BLOCK, also when one row is
    larger than a block."""
    c = su.crafted(130, upper, True, True)
    assert max(len(line) for line in c["want"].splitlines()) > 1  # (so a block of 1 byte is smaller than any row)
    p = tmp_path / "info"
    blocks = []
    for block in su.BLOCKS:
        monkeypatch.setenv("VS_TEXT_BLOCK", block)
        rc, info = su.write_host(p, c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper)
        assert rc == 0
        assert _read(p) == c["want"], block
        blocks.append(info[2])
    assert blocks[0] >= blocks[1] > blocks[2] > blocks[3] == 1


@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_the_reference_reads_sparse_files_to_the_same_dict(tmp_path, name, d, meta):
    """process_pe_info (IO.py:598-623) zeroes every key before it adds the lines: the oracle's literal restatement of it
    builds the same dict from the committed files with and without their ``:0`` lines."""
    ids, _ = pe_oracle.read_gfa_segments(os.path.join(d, "graph.gfa"))
    sparse = []
    for f in ("pe_info", "st_info"):
        p = tmp_path / f
        with open(p, "w", newline="") as fh:
            fh.write(su.filtered(_read(os.path.join(d, f))))
        sparse.append(str(p))
    dense = graph_ops.DictPeLinks.from_files(ids, os.path.join(d, "pe_info"), os.path.join(d, "st_info"))
    assert graph_ops.DictPeLinks.from_files(ids, *sparse).table == dense.table


# ---- the reader ---------------------------------------------------------------------------------
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


def test_parse_shuffled_lines_with_duplicates_and_unknown_ids(tmp_path):
    c = su.crafted(130, 0, False, True)
    rng = np.random.default_rng(5)
    dense = pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], 0)).splitlines(True)
    lines = dense + [dense[i] for i in rng.integers(0, len(dense), 500)]  # duplicates
    lines += ["nobody:%s:7\n" % c["ids"][3], "%s:ghost:9\n" % c["ids"][4], "%s:%s:-12\n" % (c["ids"][1], c["ids"][2]),
              "%s:%s:+3\n" % (c["ids"][2], c["ids"][2]), "%s:%s:5:trailing:fields\n" % (c["ids"][0], c["ids"][5])]
    lines = [lines[i] for i in rng.permutation(len(lines))]
    p = tmp_path / "pe_info"
    p.write_text("".join(lines))
    assert os.path.getsize(p) > 3 << 16  # (large enough for several parser threads)
    want = _python_cells(c["ids"], p)
    assert len(want) == len(lines) - 2
    assert _native_cells(c["ids"], p) == want
    # a subset of the names: every line naming another node is skipped
    some = c["ids"][::3]
    assert _native_cells(some, p) == _python_cells(some, p)


@pytest.mark.parametrize("text", [
    "a:b:1\nb:a:2\n\nb:b:oops\na:a:4\n",   # stop at the first empty line; what follows is not even looked at
    "\na:b:1\n",                            # an empty first line: nothing is read
    "a:b:1\nb:b:57",                        # a last line without a newline loses its last character: 5
    "a:b:1\nb:b:5\n",
    "a:b:-3\na:b:+4\nb:a:0\n",
    "a:b:1\nb:b:7x",                        # ... also when that character is what made it malformed
    "",
], ids=["empty-line", "empty-first", "no-final-newline", "plain", "signs", "cut-saves", "empty-file"])
def test_parse_follows_read_pe_text(tmp_path, text):
    p = tmp_path / "st_info"
    with open(p, "w", newline="") as fh:
        fh.write(text)
    assert _native_cells(["a", "b"], p) == _python_cells(["a", "b"], p)


@pytest.mark.parametrize("text", ["a:b\n", "a:b:\n", "a:b:x\n", "a:b:1.5\n", "a:b:--1\n", "a:b:1\nab\n", "a:b:1\nb", "zz:b:nope\n", "a:b: 1\n"],
                         ids=["two-fields", "empty-count", "letters", "float", "two-signs", "no-colon", "one-char-last-line", "unknown-id-bad-count",
                              "blank-in-count"])
def test_parse_refuses_malformed_lines(tmp_path, text):
    p = tmp_path / "pe_info"
    with open(p, "w", newline="") as fh:
        fh.write(text)
    with pytest.raises(ValueError):
        _native_cells(["a", "b"], p)
    if text != "a:b: 1\n":  # (int() of the Python loop strips blanks; the library reads an optionally signed decimal integer only)
        with pytest.raises(ValueError):
            _python_cells(["a", "b"], p)


def test_parse_leaves_carriage_returns_and_other_encodings_to_python(tmp_path):
    from vstrains_amd import _native as nat
    import ctypes as C

    p = tmp_path / "pe_info"
    for raw, flag in ((b"a:b:1\r\nb:b:2\r\n", 1), (b"a:b:1\rb:b:2\n", 1), (b"a:\xc3\xa9:1\n", 2)):
        p.write_bytes(raw)
        assert _native_cells(["a", "b"], p) is None
        info = (C.c_uint64 * 4)()
        blob, off = su.encode_ids(["a", "b"])
        assert nat.lib().vs_info_parse(str(p).encode(), blob.ctypes.data, off.ctypes.data, 2, None, None, None, 0, info) == 0
        assert int(info[1]) == flag and int(info[0]) == 0
    with pytest.raises(FileNotFoundError):
        _native_cells(["a"], tmp_path / "missing")


# ---- PeCounter on CPU tensors ---------------------------------------------------------------------
@pytest.mark.parametrize("with_wide", [False, True], ids=["u32", "wide"])
def test_counter_on_cpu_tensors_writes_through_the_host_twin(tmp_path, with_wide):
    import torch
    from vstrains_amd import pe as host

    n = 130
    node, short = su.crafted(n, 0, True, with_wide), su.crafted(n, 1, True, with_wide)
    rank = node["rank"].astype(np.int64)
    order = np.empty(n, dtype=np.int64)
    order[rank] = np.arange(n)
    ctx = types.SimpleNamespace(n_nodes=n, device=0, _h=None, node_order=order, node_rank=rank)
    counter = host.PeCounter(ctx, device="cpu", track_tiles=True)
    # (a counted short_mat holds a pair of nodes at (smaller, larger) internal number only; result() adds the two sides in
    # uint32, so the crafted cells below the diagonal, which could carry the sum past 2^32, are left out here)
    counter.mats.copy_(torch.from_numpy(np.stack([node["counts"], np.triu(short["counts"])]).view(np.int32)))
    counter.tile_map.copy_(torch.from_numpy(np.concatenate([node["tile_map"], short["tile_map"]])))
    if with_wide:
        counter.wide = torch.from_numpy(np.stack([node["wide"], np.triu(short["wide"])]))
    info = counter.write_sparse_text(str(tmp_path / "pe_info"), str(tmp_path / "st_info"), node["ids"])
    node_mat, short_mat, _ = counter.result()
    for f, mat, inf in (("pe_info", node_mat, info[0]), ("st_info", short_mat, info[1])):
        got = _read(tmp_path / f)
        assert got == su.filtered(pe_oracle.matrix_text(node["ids"], mat))
        assert inf["lines"] == got.count("\n") and inf["bytes"] == len(got)
    # (the short matrix was crafted under another numbering: only the node matrix has a crafted expectation here)
    assert _read(tmp_path / "pe_info") == node["want"]
