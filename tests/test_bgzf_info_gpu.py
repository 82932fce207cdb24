"""pe_info / st_info as BGZF from the device: k_info_format + k_deflate + the pack, from counters counted on the device,
against the committed files of the real reference script (dense: byte for byte once inflated; sparse: without their ``:0``
lines) and, file for file, against the host twin; the drop-in's and the whole command's flags; the tables read back from
the ``.gz`` pair.  gzip is the oracle; every comparison is exact."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bgzf_util as bu
import deflate_cases as dc
import sparse_info_util as su
from conftest import ROOT, pe_cases
from oracle import pe_oracle

pytestmark = pytest.mark.gpu


def _read(path):
    with open(path, "r", newline="") as fh:
        return fh.read()


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


@pytest.mark.parametrize("name,d,meta", pe_cases(), ids=[c[0] for c in pe_cases()])
def test_golden_cases_through_the_device_writer(host, ctx, tmp_path, name, d, meta):
    ids, seqs = host.read_gfa_segments(os.path.join(d, "graph.gfa"))
    fq = host.FastqPair(os.path.join(d, "fwd.fq"), os.path.join(d, "rve.fq"), ctx)
    ctx.build_index(seqs, meta["k"])
    counter = host.PeCounter(ctx)
    if len(fq):
        counter.add(fq.block(0, len(fq)))
    mats = dc.golden_matrices(d, ids)
    files = (str(tmp_path / "pe_info.gz"), str(tmp_path / "st_info.gz"))
    for dense in (True, False):
        info = counter.write_bgzf_text(files[0], files[1], ids, dense=dense)
        for upper, (f, inf) in enumerate(zip(("pe_info", "st_info"), info)):
            want = _read_bytes(os.path.join(d, f))
            if not dense:
                want = su.filtered(want.decode()).encode()
            data = dc.check_file(files[upper], want, [inf[k] for k in dc.INFO_KEYS])
            # the twin, from the committed matrix in the caller's numbering: the same file
            assert dc.write_bgzf_host(tmp_path / "twin.gz", ids, mats[upper], None, None, None, upper, int(dense))[0] == 0
            assert data == _read_bytes(tmp_path / "twin.gz")


def test_golden_case_with_the_tile_map_and_totals_folded(host, ctx, tmp_path, monkeypatch):
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
    assert counter.wide is not None and counter.tile_map is not None
    files = (str(tmp_path / "pe_info.gz"), str(tmp_path / "st_info.gz"))
    for dense in (True, False):
        info = counter.write_bgzf_text(files[0], files[1], ids, dense=dense)
        for p, f, inf in zip(files, ("pe_info", "st_info"), info):
            want = _read(os.path.join(d, f))
            dc.check_file(p, (want if dense else su.filtered(want)).encode(), [inf[k] for k in dc.INFO_KEYS])


def _on_device(c):
    import torch

    dev = lambda a, dt: None if a is None else torch.from_numpy(a.view(dt) if dt is not None else a).cuda()  # noqa: E731
    return dev(c["counts"], np.int32), dev(c["wide"], None), dev(c["tile_map"], None)


@pytest.mark.parametrize("dense", [0, 1], ids=["sparse", "dense"])
@pytest.mark.parametrize("upper", [0, 1], ids=["node", "short"])
@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_crafted_matrices_equal_the_twin_file(ctx, tmp_path, n, upper, dense):
    """n = 257, dense: about a megabyte of text in 17 members, the last one short"""
    c = su.crafted(n, upper, True, True)
    counts, wide, tmap = _on_device(c)
    rc_h, info_h = dc.write_bgzf_host(tmp_path / "host.gz", c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], upper, dense)
    rc_d, info_d = dc.write_bgzf_device(ctx, tmp_path / "dev.gz", c["ids"], counts, wide, tmap, c["rank"], upper, dense)
    assert rc_h == 0 and rc_d == 0 and info_d == info_h
    want = pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], upper)) if dense else c["want"]
    data = dc.check_file(tmp_path / "dev.gz", want.encode(), info_d)
    assert data == _read_bytes(tmp_path / "host.gz")


@pytest.mark.parametrize("dense", [0, 1], ids=["sparse", "dense"])
def test_block_sizes_through_the_double_buffer(ctx, tmp_path, monkeypatch, dense):
    c = su.crafted(130, 1, True, True)
    counts, wide, tmap = _on_device(c)
    want = (pe_oracle.matrix_text(c["ids"], su.user_matrix(c["counts"], c["wide"], c["rank"], 1)) if dense else c["want"]).encode()
    blocks = []
    for block in su.BLOCKS:
        monkeypatch.setenv("VS_TEXT_BLOCK", block)
        rc_h, info_h = dc.write_bgzf_host(tmp_path / "host.gz", c["ids"], c["counts"], c["wide"], c["tile_map"], c["rank"], 1, dense)
        rc_d, info_d = dc.write_bgzf_device(ctx, tmp_path / "dev.gz", c["ids"], counts, wide, tmap, c["rank"], 1, dense)
        assert rc_h == 0 and rc_d == 0 and info_d == info_h
        assert dc.check_file(tmp_path / "dev.gz", want, info_d) == _read_bytes(tmp_path / "host.gz"), block
        blocks.append(info_d[2])
    assert blocks[0] > 2 and blocks[0] > blocks[-1]  # (many blocks alternate between the two buffer pairs)


def test_zeros_negative_totals_and_a_stale_file_on_the_device(ctx, tmp_path):
    import torch
    from vstrains_amd import _native as nat

    ids = su.make_ids(65)
    zeros = torch.zeros((65, 65), dtype=torch.int32, device="cuda")
    p = tmp_path / "info.gz"
    p.write_bytes(b"stale" * 10000)
    rc, info = dc.write_bgzf_device(ctx, p, ids, zeros, None, None, None, 0, 0)
    assert rc == 0 and info[:3] == [0, 0, 0] and info[4:] == [0, 28] and _read_bytes(p) == bu.EOF_MARK
    p.write_bytes(b"stale" * 10000)
    rc, info = dc.write_bgzf_device(ctx, p, ids, zeros, None, None, None, 1, 1)
    assert rc == 0
    dc.check_file(p, pe_oracle.matrix_text(ids, np.zeros((65, 65), dtype=np.int64)).encode(), info)
    wide = torch.zeros((65, 65), dtype=torch.int64, device="cuda")
    wide[64, 3] = -1
    for upper in (0, 1):
        for dense in (0, 1):
            rc, _ = dc.write_bgzf_device(ctx, p, ids, zeros, wide, None, None, upper, dense)
            assert rc == nat.VS_E_ARG
            assert b"negative" in nat.lib().vs_last_error(ctx._h)


# ---- flags ---------------------------------------------------------------------------------------------------------------------
def test_drop_in_with_bgzf_info(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    outs = {}
    for flag in ((), ("--bgzf-info",), ("--bgzf-info", "--sparse-info")):
        out = tmp_path / ("aln" + "_".join(flag))
        proc = subprocess.run(
            [sys.executable, "-m", "vstrains_amd.pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
             "-f", os.path.join(d, "fwd.fq"), "-r", os.path.join(d, "rve.fq"), "-k", str(meta["k"]), *flag],
            cwd=ROOT, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        lines = proc.stdout.splitlines()
        assert lines[-2].startswith("Global time elapsed:  ")
        assert lines[-1] == "result stored in:  %s/pe_info%s" % (out, ".gz" if flag else "")
        outs[flag] = (lines[:-2], out)
    assert outs[()][0] == outs[("--bgzf-info",)][0] == outs[("--bgzf-info", "--sparse-info")][0]  # the same stdout lines
    for f in ("pe_info", "st_info"):
        golden = _read_bytes(os.path.join(d, f))
        assert _read_bytes(outs[()][1] / f) == golden
        assert sorted(os.listdir(outs[("--bgzf-info",)][1])) == ["pe_info.gz", "st_info.gz"]
        dc.check_file(outs[("--bgzf-info",)][1] / (f + ".gz"), golden)
        dc.check_file(outs[("--bgzf-info", "--sparse-info")][1] / (f + ".gz"), su.filtered(golden.decode()).encode())
    if os.path.exists("/bin/gzip") or os.path.exists("/usr/bin/gzip"):  # what a reference user would type
        got = subprocess.run(["gzip", "-dc", str(outs[("--bgzf-info",)][1] / "pe_info.gz")], capture_output=True).stdout
        assert got == _read_bytes(os.path.join(d, "pe_info"))


def _tree(root, subs):
    out = {}
    for sub in subs:
        base = os.path.join(root, sub) if sub else root
        for fn in sorted(os.listdir(base)):
            p = os.path.join(base, fn)
            if os.path.isfile(p):
                out[os.path.join(sub, fn)] = _read(p)
    return out


def test_whole_command_with_bgzf_pe_text(tmp_path):
    from graph_case import Case
    from vstrains_amd import cli

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    runs = {}
    for flag in ((), ("--bgzf-pe-text",), ("--bgzf-pe-text", "--sparse-pe-text")):
        out = str(tmp_path / ("out" + "_".join(flag)))
        cli.main(["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", out, "-fwd", inp["fwd"], "-rve", inp["rve"], *flag])
        runs[flag] = out
    plain = runs[()]
    a = _tree(plain, ("gfa", "tmp"))
    assert a
    for flag in list(runs)[1:]:
        assert _tree(runs[flag], ("gfa", "tmp")) == a
        for f in ("strain.fasta", "strain.paths"):
            assert _read(os.path.join(plain, f)) == _read(os.path.join(runs[flag], f))
        assert sorted(os.listdir(os.path.join(runs[flag], "aln"))) == ["pe_info.gz", "st_info.gz"]
        for f in ("pe_info", "st_info"):
            dense = _read(os.path.join(plain, "aln", f))
            want = su.filtered(dense) if "--sparse-pe-text" in flag else dense
            assert dense.count("\n") > su.filtered(dense).count("\n") > 0
            dc.check_file(os.path.join(runs[flag], "aln", f + ".gz"), want.encode())
    with pytest.raises(SystemExit):
        cli.main(["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(tmp_path / "never"), "-fwd", inp["fwd"], "-rve", inp["rve"],
                  "--bgzf-pe-text", "--no-pe-text"])
    assert not os.path.exists(tmp_path / "never")


# ---- reading them back ------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def pairs(workload, tmp_path_factory):
    """the plain dense pair (through result(), as the drop-in writes it) and the dense and the sparse .gz pair of the workload"""
    from vstrains_amd import pe_inference

    ids, counter = workload
    root = tmp_path_factory.mktemp("pairs")
    out = {}
    for key, kw in (("plain", {}), ("dense_gz", dict(bgzf=True)), ("sparse_gz", dict(bgzf=True, sparse=True))):
        os.makedirs(root / key)
        name, _ = pe_inference.write_info_files(str(root / key), ids, counter, **kw)
        suffix = ".gz" if kw else ""
        assert name == str(root / key) + "/pe_info" + suffix
        out[key] = (str(root / key / ("pe_info" + suffix)), str(root / key / ("st_info" + suffix)))
    for i, f in enumerate(("pe_info", "st_info")):
        dense = _read_bytes(out["plain"][i])
        assert gzip.decompress(_read_bytes(out["dense_gz"][i])) == dense
        assert gzip.decompress(_read_bytes(out["sparse_gz"][i])) == su.filtered(dense.decode()).encode()
    return out


@pytest.mark.parametrize("sparse_min_nodes", [0, 64], ids=["dense-table", "csr-table"])
@pytest.mark.parametrize("kind", ["dense_gz", "sparse_gz"])
def test_tables_read_from_gz_files(ctx, workload, pairs, kind, sparse_min_nodes):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, _ = workload
    want = HipPeLinks.from_files(ctx, ids, *pairs["plain"], sparse_min_nodes=sparse_min_nodes).to_numpy()
    assert want.any()
    assert HipPeLinks._parse_cells(ids, pairs[kind][0]) is not None  # (the library's parser took it, not the Python loop)
    assert np.array_equal(HipPeLinks.from_files(ctx, ids, *pairs[kind], sparse_min_nodes=sparse_min_nodes).to_numpy(), want)


def test_a_gz_with_carriage_returns_keeps_the_python_loop(ctx, workload, pairs, tmp_path):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, _ = workload
    want = HipPeLinks.from_files(ctx, ids, *pairs["plain"]).to_numpy()
    text = gzip.decompress(_read_bytes(pairs["sparse_gz"][1]))
    assert text.count(b"\n") > 100
    p = tmp_path / "st_info.gz"
    p.write_bytes(bu.bgzf(text.replace(b"\n", b"\r\n"), 1))
    assert HipPeLinks._parse_cells(ids, str(p)) is None
    assert np.array_equal(HipPeLinks.from_files(ctx, ids, pairs["sparse_gz"][0], str(p)).to_numpy(), want)


def test_a_cut_gz_is_an_error(ctx, workload, pairs, tmp_path):
    from vstrains_amd.graph.hip_ops import HipPeLinks

    ids, _ = workload
    data = _read_bytes(pairs["dense_gz"][0])
    p = tmp_path / "pe_info.gz"
    p.write_bytes(data[:len(data) // 2])
    with pytest.raises(ValueError):
        HipPeLinks.from_files(ctx, ids, str(p), pairs["dense_gz"][1])


def test_reference_api_takes_the_gz_pair(workload, pairs):
    from vstrains_amd.graph import reference_api as ra

    ids, _ = workload
    plain = ra.process_pe_info(ids, *pairs["plain"])[1].to_numpy()
    assert np.array_equal(ra.process_pe_info(ids, *pairs["dense_gz"])[1].to_numpy(), plain)
