"""Sparse pe_info / st_info on the device: the writer's kernels (k_info_row_sizes / k_info_format) against the committed
files of the real reference script without their ``:0`` lines and, byte for byte, against the host twin; the drop-in's and
the whole command's flags; the native reader and the table built from its cells.  Every comparison is exact."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import sparse_info_util as su
from conftest import ROOT, pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu


def _read(path):
    with open(path, "r", newline="") as fh:
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


def _count_case(host, ctx, d, meta):
    ids, seqs = host.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fq = host.FastqPair(os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq"), ctx)
    ctx.build_index(seqs, meta["k"])
    counter = host.PeCounter(ctx)
    if len(fq):
        counter.add(fq.block(0, len(fq)))
    return ids, counter


@pytest.mark.parametrize("tracked", [False, True], ids=["plain", "tile-map"])
@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_golden_cases_through_the_device_writer(host, ctx, tmp_path, monkeypatch, name, d, meta, tracked):
    """The files of the real reference script without their ``:0`` lines, from counters counted on the device; once with the
    default counter and once with the dirty-tile map (VS_TRACK_TILES=1)."""
    if tracked:
        monkeypatch.setenv("VS_TRACK_TILES", "1")
    ids, counter = _count_case(host, ctx, d, meta)
    assert (counter.tile_map is not None) == tracked
    info = counter.write_sparse_text(str(tmp_path / "pe_info"), str(tmp_path / "st_info"), ids)
    for f, inf in zip(("pe_info", "st_info"), info):
        want = su.filtered(_read(os.path.join(d, f)))
        got = _read(tmp_path / f)
        assert got == want, f
        assert inf["lines"] == want.count("\n") and inf["bytes"] == len(want)


@pytest.mark.parametrize("tracked", [False, True], ids=["plain", "tile-map"])
def test_golden_case_with_the_totals_folded_into_int64(host, ctx, tmp_path, monkeypatch, tracked):
    """fold() forced in the middle: half of the pairs live in ``wide``, the other half in the uint32 cells."""
    if tracked:
        monkeypatch.setenv("VS_TRACK_TILES", "1")
    name, d, meta = [c for c in pe_cases() if c[0] == "hiv_like_k55"][0]
    ids, seqs = host.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fq = host.FastqPair(os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq"), ctx)
    ctx.build_index(seqs, meta["k"])
    counter = host.PeCounter(ctx)
    half = len(fq) // 2
    counter.add(fq.block(0, half))
    counter.fold()
    counter.add(fq.block(half, len(fq) - half))
    assert counter.wide is not None
    counter.write_sparse_text(str(tmp_path / "pe_info"), str(tmp_path / "st_info"), ids)
    for f in ("pe_info", "st_info"):
        assert _read(tmp_path / f) == su.filtered(_read(os.path.join(d, f))), f
    counter.fold()  # ... and with everything in ``wide``
    counter.write_sparse_text(str(tmp_path / "pe_info"), str(tmp_path / "st_info"), ids)
    for f in ("pe_info", "st_info"):
        assert _read(tmp_path / f) == su.filtered(_read(os.path.join(d, f))), f


def _on_device(c):
    import torch

    dev = lambda a, dt: None if a is None else torch.from_numpy(a.view(dt) if dt is not None else a).cuda()  # noqa: E731
    return dev(c["counts"], np.int32), dev(c["wide"], None), dev(c["tile_map"], None)


@pytest.mark.parametrize("with_wide", [False, True], ids=["u32", "wide"])
@pytest.mark.parametrize("with_map", [False, True], ids=["nomap", "map"])
@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
@pytest.mark.parametrize("n", su.SIZES)
def test_crafted_matrices_equal_the_host_twin(ctx, tmp_path, n, upper, with_map, with_wide):
    c = su.crafted(n, upper, with_map, with_wide)
    counts, wide, tmap = _on_device(c)
    rc_h, info_h = su.write_host(tmp_path / "host", c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper)
    rc_d, info_d = su.write_device(ctx, tmp_path / "dev", c["ids"], counts, wide, tmap, c["rank"], upper)
    assert rc_h == 0 and rc_d == 0
    got = _read(tmp_path / "dev")
    assert got == _read(tmp_path / "host")
    assert got == c["want"]
    assert info_d == info_h


@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
def test_block_sizes_through_the_double_buffer(ctx, tmp_path, monkeypatch, upper):
    c = su.crafted(130, upper, True, True)
    counts, wide, tmap = _on_device(c)
    blocks = []
    for block in su.BLOCKS:
        monkeypatch.setenv("VS_TEXT_BLOCK", block)
        rc_h, info_h = su.write_host(tmp_path / "host", c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper)
        rc_d, info_d = su.write_device(ctx, tmp_path / "dev", c["ids"], counts, wide, tmap, c["rank"], upper)
        assert rc_h == 0 and rc_d == 0
        assert _read(tmp_path / "dev") == c["want"], block
        assert info_d == info_h
        blocks.append(info_d[2])
    assert blocks[0] > 2 and blocks[-1] == 1  # (many blocks alternate between the two buffer pairs; one block takes one)


def test_zeros_and_negative_totals_on_the_device(ctx, tmp_path):
    import torch
    from vstrains_amd import _native as nat

    ids = su.make_ids(65)
    zeros = torch.zeros((65, 65), dtype=torch.int32, device="cuda")
    p = tmp_path / "info"
    p.write_text("stale")
    rc, info = su.write_device(ctx, p, ids, zeros, None, None, None, 0)
    assert rc == 0 and info[:3] == [0, 0, 0] and os.path.getsize(p) == 0
    wide = torch.zeros((65, 65), dtype=torch.int64, device="cuda")
    wide[64, 3] = -1
    for upper in (0, 1):
        rc, _ = su.write_device(ctx, p, ids, zeros, wide, None, None, upper)
        assert rc == nat.VS_E_ARG
        assert b"negative" in nat.lib().vs_last_error(ctx._h)


@pytest.fixture(scope="module")
def workload(host, ctx):
    """A random graph of a few hundred nodes counted under the default renumbering, with a dirty-tile map."""
    from vstrains_amd import synth

    st = synth.make_strains(5, 4000, 0.03, seed=11)
    g = synth.compact_dbg(st, 21)
    fwd, rve = synth.sample_pairs(st, 3000, 100, seed=12, sub_rate=0.005, n_rate=0.01)
    ids = ["%d%s" % (i, "&%d*0" % i if i % 5 == 0 else "") for i in range(len(g.seqs))]
    ctx.build_index(g.seqs, 21)
    counter = host.PeCounter(ctx, track_tiles=True)
    counter.add(ctx.pack_pairs(fwd, rve))
    return ids, counter


def test_default_renumbering_equals_the_filtered_dense_files(host, workload, tmp_path):
    from vstrains_amd import pe_inference

    ids, counter = workload
    assert 200 <= len(ids) <= 500
    assert counter.node_rank is not None and not np.array_equal(counter.node_rank, np.arange(len(ids)))
    os.makedirs(tmp_path / "dense")
    pe_inference.write_info_files(str(tmp_path / "dense"), ids, counter)
    counter.write_sparse_text(str(tmp_path / "pe_info"), str(tmp_path / "st_info"), ids)
    for f in ("pe_info", "st_info"):
        want = su.filtered(_read(tmp_path / "dense" / f))
        assert want.count("\n") > 100
        assert _read(tmp_path / f) == want, f


def test_drop_in_with_sparse_info(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    outs = {}
    for flag in ((), ("--sparse-info",)):
        out = tmp_path / ("aln" + "_".join(flag))
        proc = subprocess.run(
            [sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
             "-f", os.path.join(d, "fwd.fq"), "-r", os.path.join(d, "rve.fq"), "-k", str(meta["k"]), *flag],
            cwd=ROOT, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        lines = proc.stdout.splitlines()
        assert lines[-2].startswith("Global time elapsed:  ")
        assert lines[-1] == "result stored in:  %s/pe_info" % out
        outs[flag] = (lines[:-2], out)
    assert outs[()][0] == outs[("--sparse-info",)][0]  # the same stdout lines
    assert [l for l in outs[()][0] if l.startswith("Number of processed reads")] == meta["progress_lines"]
    for f in ("pe_info", "st_info"):
        assert _read(outs[()][1] / f) == _read(os.path.join(d, f))
        assert _read(outs[("--sparse-info",)][1] / f) == su.filtered(_read(os.path.join(d, f)))


def _tree(root, subs):
    out = {}
    for sub in subs:
        base = os.path.join(root, sub) if sub else root
        for fn in sorted(os.listdir(base)):
            p = os.path.join(base, fn)
            if os.path.isfile(p):
                out[os.path.join(sub, fn)] = _read(p)
    return out


def test_whole_command_with_sparse_pe_text(tmp_path):
    from graph_case import Case
    from vstrains_amd import cli

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    runs = {}
    for flag in ((), ("--sparse-pe-text",)):
        out = str(tmp_path / ("out" + "_".join(flag)))
        cli.main(["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", out, "-fwd", inp["fwd"], "-rve", inp["rve"], *flag])
        runs[flag] = out
    plain, sparse = runs[()], runs[("--sparse-pe-text",)]
    a, b = _tree(plain, ("gfa", "tmp")), _tree(sparse, ("gfa", "tmp"))
    assert a and a == b
    for f in ("strain.fasta", "strain.paths"):
        assert _read(os.path.join(plain, f)) == _read(os.path.join(sparse, f))
    for f in ("pe_info", "st_info"):
        dense = _read(os.path.join(plain, "aln", f))
        assert dense.count("\n") > su.filtered(dense).count("\n") > 0
        assert _read(os.path.join(sparse, "aln", f)) == su.filtered(dense)
    with pytest.raises(SystemExit):
        cli.main(["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(tmp_path / "never"), "-fwd", inp["fwd"], "-rve", inp["rve"],
                  "--sparse-pe-text", "--no-pe-text"])
    assert not os.path.exists(tmp_path / "never")


# ---- the reader -----------------------------------------------------------------------------------
def _parsed_matrices(names, pe_file, st_file):
    from vstrains_amd.graph.formats import read_pe_text

    index = {n: i for i, n in enumerate(names)}
    mats = []
    for path in (pe_file, st_file):
        m = np.zeros((len(names), len(names)), dtype=np.int64)
        for u, v, c in read_pe_text(str(path)):
            if u in index and v in index:
                m[index[u], index[v]] += c
        mats.append(m)
    return mats


@pytest.mark.parametrize("sparse_min_nodes", [0, 64], ids=["dense-table", "csr-table"])
@pytest.mark.parametrize("kind", ["sparse", "dense", "shuffled"])
def test_tables_read_from_files(ctx, workload, tmp_path, kind, sparse_min_nodes):
    """HipPeLinks.from_files through vs_info_parse + vs_links_from_cells: the table of from_matrices over the parsed
    matrices, in either form, with the same block sums."""
    from vstrains_amd import pe_inference
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, counter = workload
    files = [str(tmp_path / "pe_info"), str(tmp_path / "st_info")]
    if kind == "sparse":
        counter.write_sparse_text(files[0], files[1], ids)
    else:
        pe_inference.write_info_files(str(tmp_path), ids, counter)
    if kind == "shuffled":
        rng = random.Random(9)
        for p in files:
            lines = [l for l in _read(p).splitlines(True) if not l.endswith(":0\n") or rng.random() < 0.02]
            lines += [rng.choice(lines) for _ in range(300)] + ["%s:%s:-2\n" % (ids[1], ids[0]), "ghost:%s:4\n" % ids[0]]
            rng.shuffle(lines)
            with open(p, "w", newline="") as fh:
                fh.write("".join(lines))
    table = HipPeLinks.from_files(ctx, ids, files[0], files[1], sparse_min_nodes=sparse_min_nodes)
    node, short = _parsed_matrices(ids, files[0], files[1])
    want = HipPeLinks.from_matrices(ctx, ids, node, short)
    assert np.array_equal(table.to_numpy(), want.to_numpy())
    assert table.to_numpy().any()
    py = random.Random(3)
    n = len(ids)
    queries = [([py.randrange(n) for _ in range(py.randrange(0, 6))], [py.randrange(n) for _ in range(py.choice([0, 1, 2, 5, 70, 130]))])
               for _ in range(300)]
    assert table.block_sums(queries) == want.block_sums(queries)
    groups = [[py.randrange(n) for _ in range(py.randrange(0, 5))] for _ in range(20)]
    assert np.array_equal(table.group_matrix(groups), want.group_matrix(groups))


def test_files_with_carriage_returns_keep_the_python_loop(ctx, workload, tmp_path):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, counter = workload
    files = [str(tmp_path / "pe_info"), str(tmp_path / "st_info")]
    counter.write_sparse_text(files[0], files[1], ids)
    want = HipPeLinks.from_files(ctx, ids, files[0], files[1]).to_numpy()
    text = _read(files[1])  # (read before the file is opened for writing, which empties it)
    assert text.count("\n") > 100
    with open(files[1], "w", newline="") as fh:
        fh.write(text.replace("\n", "\r\n"))
    assert HipPeLinks._parse_cells(ids, files[1]) is None and b"\r\n" in open(files[1], "rb").read()
    assert np.array_equal(HipPeLinks.from_files(ctx, ids, files[0], files[1]).to_numpy(), want)


def test_round_trip_of_a_csr_table_through_its_own_sparse_files(ctx, workload, tmp_path):
    """The table from tracked counters (CSR rows from 64 nodes on) equals the table read back from the sparse files those
    counters wrote, in the same form."""
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, counter = workload
    from_counters = HipPeLinks.from_counter(ctx, counter, ids, sparse_min_nodes=64)
    files = [str(tmp_path / "pe_info"), str(tmp_path / "st_info")]
    counter.write_sparse_text(files[0], files[1], ids)
    read_back = HipPeLinks.from_files(ctx, ids, files[0], files[1], sparse_min_nodes=64)
    assert np.array_equal(from_counters.to_numpy(), read_back.to_numpy())
    py = random.Random(4)
    n = len(ids)
    queries = [([py.randrange(n) for _ in range(py.randrange(1, 6))], [py.randrange(n) for _ in range(py.choice([1, 2, 5, 70]))]) for _ in range(200)]
    # (the table from the counters is in the index's numbering, rows found by name)
    by_name = [([from_counters.index_of(ids[r]) for r in rows], [from_counters.index_of(ids[c]) for c in cols]) for rows, cols in queries]
    assert from_counters.block_sums(by_name) == read_back.block_sums(queries)
