"""Plain gzip decoded in parallel on the device: the kernels of vs_gzip.hip (``vs_gzip_inflate``) on the constructed
streams of gzip_cases.py.  zlib is the oracle for the text; the one-lane host twin, which the CPU suite holds against zlib,
is the reference for the counts and the status words -- both sides run the same routines of vs_gzip_core.h."""
import functools

import pytest

import gzip_cases as gc

pytestmark = pytest.mark.gpu

COUNTS = ("candidates", "selected", "chain_runs", "dropped", "members", "status", "recounted")


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def ctx(host):
    c = host.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _twin(name, gran):
    from vstrains_amd import pe as host

    data = {n: d for n, d, _ in gc.good_cases()}
    data.update(dict(gc.bad_cases()))
    return host.gzip_inflate_host(data[name], gran)[0]


@pytest.mark.parametrize("gran", [gc.EVERY, gc.COARSE], ids=["every", "coarse"])
def test_kernels_equal_zlib_and_the_host_twin_on_every_case(host, ctx, gran):
    for name, data, text in gc.good_cases():
        info, got, guard = host.gzip_inflate(data, ctx, gran)
        twin = _twin(name, gran)
        print(name, gran, info)
        assert guard, name
        assert info["status"] == 0 and got == text, (name, info)
        assert all(info[k] == twin[k] for k in COUNTS), (name, info, twin)
    info, _, _ = host.gzip_inflate(dict((n, d) for n, d, _ in gc.good_cases())["small_blocks"], ctx, gc.EVERY)
    assert info["chain_runs"] >= 100  # (more than one wavefront's work: 206 runs)


@pytest.mark.parametrize("gran", [gc.EVERY, gc.COARSE], ids=["every", "coarse"])
def test_kernels_refuse_the_corrupt_streams_as_the_host_twin_does(host, ctx, gran):
    for name, data in gc.bad_cases():
        info, got, guard = host.gzip_inflate(data, ctx, gran)
        twin = _twin(name, gran)
        print(name, gran, info)
        assert guard, name
        assert info["status"] != 0 and got == b"" and info["text"] == 0, (name, info)
        assert info["status"] == twin["status"], (name, info, twin)
        assert all(info[k] == twin[k] for k in COUNTS), (name, info, twin)


# ---- the streamed ingest with the switch on -------------------------------------------------------------------------------
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

import test_bgzf_inflate_gpu as bg  # noqa: E402
import test_bgzf_shard_gpu as sh  # noqa: E402
import test_fastq_stream_gpu as sg  # noqa: E402
from conftest import ROOT, pe_cases  # noqa: E402

SWITCHES = ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK", "VS_GZIP_DEVICE", "VS_GZIP_TEXT")


def _gz(text, mem):
    return gc.member(gc.raw(text, 6, mem), text)


@functools.lru_cache(maxsize=None)
def _reads():
    """(graph, fwd text, rve text): 2 500 pairs whose quality lines are random, so that a file is several default-sized
    deflate blocks (the synthetic reads' constant qualities would leave one)"""
    import numpy as np

    g, f, r = sg._synth_reads(2500, seed=17)
    rng = np.random.default_rng(18)
    texts = []
    for t in sg._variant("plain", f, r):
        lines = t.split(b"\n")
        for i in range(3, len(lines), 4):
            lines[i] = bytes(rng.choice(np.frombuffer(b"FFFFFFF:,#I", dtype=np.uint8), size=len(lines[i])))
        texts.append(b"\n".join(lines))
    return g, texts[0], texts[1]


@pytest.fixture(scope="module")
def mapped(host, ctx, tmp_path_factory):
    g, tf, tr = _reads()
    return bg._mapped(host, ctx, g, tmp_path_factory.mktemp("plain"), tf, tr)


@pytest.mark.parametrize("mem", [1, 8], ids=["memlevel1", "default"])
def test_stream_of_plain_gzip_over_several_windows(host, ctx, tmp_path, monkeypatch, mapped, mem):
    """Both files plain gzip, the chunk a sixth of the smaller file (less than a default-sized block): every file is decoded in at least three windows, the
    counters and the pair count are the mapped plain files', zlib inflated nothing."""
    g, tf, tr = _reads()
    paths = (str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    for p, t in zip(paths, (tf, tr)):
        with open(p, "wb") as fh:
            fh.write(_gz(t, mem))
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    monkeypatch.setenv("VS_STREAM_CHUNK", str(min(os.path.getsize(p) for p in paths) // 6))
    got, info = bg._count_stream(host, ctx, g, *paths)
    print(mem, info)
    bg._same(got, mapped)
    assert all(f["windows"] >= 3 and f["runs"] > 0 and f["members"] == 1 for f in info["gzip_device"]), info
    assert info["members_host"] == (0, 0) and info["members_device"] == (0, 0)
    assert info["text_bytes"] == len(tf) + len(tr) and info["file_bytes"] == sum(os.path.getsize(p) for p in paths)
    monkeypatch.delenv("VS_GZIP_DEVICE")  # (the same files without the switch: host zlib, as before)
    got, info = bg._count_stream(host, ctx, g, *paths)
    bg._same(got, mapped)
    assert info["members_host"] == (1, 1) and all(f["windows"] == 0 for f in info["gzip_device"])


@pytest.mark.parametrize("chunk", [None, 50_000], ids=["one_slot", "chunk50000"])
def test_stream_with_a_small_text_cap_takes_several_rounds_per_slot(host, ctx, tmp_path, monkeypatch, mapped, chunk):
    """VS_GZIP_TEXT (tests only) caps the text of a round at 120 000 bytes, which two or three runs of the memLevel-1 files fill (a run is at most
    16 KiB of compressed bytes and a block, about 65 000 bytes of text): the
    runs the cap holds back stay compressed and are decoded by further rounds WITHOUT a new slot -- with the default chunk
    the whole file is one slot, so every window but the first is such a round; with a chunk of 50 000 bytes a slot brings
    more text than one round takes, so rounds on pending bytes and rounds on new slots alternate.  The pending bytes never pile up, the counters are the
    mapped files', no run is counted as dropped that a later round decodes."""
    g, tf, tr = _reads()
    paths = (str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    for p, t in zip(paths, (tf, tr)):
        with open(p, "wb") as fh:
            fh.write(_gz(t[: len(t) // 2], 1) + _gz(t[len(t) // 2:], 1))  # two members: a trailer in the middle of the rounds
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    monkeypatch.setenv("VS_GZIP_TEXT", "120000")
    if chunk:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    got, info = bg._count_stream(host, ctx, g, *paths)
    print(chunk, info)
    bg._same(got, mapped)
    for f, t in zip(info["gzip_device"], (tf, tr)):
        assert f["windows"] >= len(t) // 120000 and f["members"] == 2 and f["dropped"] == 0, info  # (no round above the cap)
    assert info["text_bytes"] == len(tf) + len(tr) and info["members_host"] == (0, 0)


def test_stream_refuses_a_single_run_above_the_text_cap(host, ctx, tmp_path, monkeypatch):
    """A default-sized block is more than 100 000 bytes of text here: with the cap at 50 000 the first run alone does not fit,
    which is VS_E_RANGE with the advice to leave the switch out -- not a failed stream, and not a message about zlib."""
    from vstrains_amd import _native as nat

    g, tf, tr = _reads()
    paths = (str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    for p, t in zip(paths, (tf, tr)):
        with open(p, "wb") as fh:
            fh.write(_gz(t, 8))
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    monkeypatch.setenv("VS_GZIP_TEXT", "50000")
    with pytest.raises(nat.NativeError) as err:
        bg._count_stream(host, ctx, g, *paths)
    print(err.value)
    assert err.value.code == nat.VS_E_RANGE and "leave the device gzip switch out" in str(err.value) and "50000 bytes of text" in str(err.value)


def test_stream_of_one_gzip_file_through_a_fifo_and_one_plain_file(host, ctx, tmp_path, monkeypatch, mapped):
    g, tf, tr = _reads()
    (tmp_path / "r.fq").write_bytes(tr)
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    data = _gz(tf[: len(tf) // 2], 1) + _gz(tf[len(tf) // 2:], 8)  # two members
    monkeypatch.setenv("VS_STREAM_CHUNK", str(len(data) // 5))
    with sg.Fifos(tmp_path, data, b"", names=("f.fifo", "unused.fifo")) as (fifo, _):
        got, info = bg._count_stream(host, ctx, g, fifo, str(tmp_path / "r.fq"))
    print(info)
    bg._same(got, mapped)
    assert info["gzip_device"][0]["windows"] >= 3 and info["gzip_device"][0]["members"] == 2 and info["gzip_device"][1]["windows"] == 0
    assert info["members_host"] == (0, 0)


def _golden_gz(tmp_path, d, mem=8):
    for which in ("fwd", "rve"):
        with open(os.path.join(d, which + ".fq"), "rb") as fh:
            (tmp_path / (which + ".fq.gz")).write_bytes(_gz(fh.read(), mem))
    return str(tmp_path / "fwd.fq.gz"), str(tmp_path / "rve.fq.gz")


def _clean_env(**more):
    return dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **more)


def test_drop_in_with_gzip_device(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    fwd, rve = _golden_gz(tmp_path, d, mem=1)
    out = tmp_path / "aln"
    proc = subprocess.run([sys.executable, "-c", bg._INFO_SCRIPT, "pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
                           "-f", fwd, "-r", rve, "-k", str(meta["k"]), "--gzip-device"],
                          cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert sg._read(out / "pe_info") == sg._read(os.path.join(d, "pe_info"))
    assert sg._read(out / "st_info") == sg._read(os.path.join(d, "st_info"))
    assert [l for l in proc.stdout.splitlines() if l.startswith("Number of processed reads")] == meta["progress_lines"]
    info = bg._stream_info(proc.stdout)
    assert all(f["runs"] > 0 for f in info["gzip_device"]) and info["members_host"] == (0, 0)


def test_whole_command_with_gzip_device(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from graph_case import Case, compare

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)
    for which in ("fwd", "rve"):
        with open(inp[which], "rb") as fh:
            (tmp_path / (which + ".fq.gz")).write_bytes(_gz(fh.read(), 8))
    out = tmp_path / "out"
    proc = subprocess.run([sys.executable, "-c", bg._INFO_SCRIPT, "cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
                           "-fwd", str(tmp_path / "fwd.fq.gz"), "-rve", str(tmp_path / "rve.fq.gz"), "--gzip-device"],
                          cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    problems, got = compare(case, str(out))
    assert not case.binding(problems), problems
    info = bg._stream_info(proc.stdout)
    assert all(f["runs"] > 0 for f in info["gzip_device"]) and info["members_host"] == (0, 0)


def _bad_pair(tmp_path, bad):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    fwd, rve = _golden_gz(tmp_path, d, mem=1)
    data = open(fwd, "rb").read()
    if bad == "truncated":
        data = data[: len(data) * 2 // 3]
    elif bad == "bad_crc":
        data = gc._flip(data, (len(data) - 8) * 8 + 3)
    elif bad == "trailing_garbage":
        data = data + b"this is no gzip member"
    elif bad == "second_member_cut":
        data = data + data[: len(data) // 2]
    else:
        assert bad == "reserved_header_flag"
        data = gc._flip(data, 3 * 8 + 6)
    assert gc.zlib_text(data) is None
    open(fwd, "wb").write(data)
    return d, meta, fwd, rve, data


@pytest.mark.parametrize("bad", ["truncated", "bad_crc", "trailing_garbage", "second_member_cut", "reserved_header_flag"])
def test_gzip_device_errors_are_worded_as_the_host_zlib_leg_words_them(tmp_path, bad):
    """Regular files: the exception line of the device leg is, character for character, the streamed host-zlib leg's."""
    d, meta, fwd, rve, _ = _bad_pair(tmp_path, bad)
    lines = {}
    for leg, env in (("device", _clean_env(VS_GZIP_DEVICE="1")), ("host", _clean_env(VS_FASTQ_STREAM="1"))):
        out = tmp_path / ("aln_" + leg)
        proc = sg._drop_in(d, meta, fwd, rve, out, env=env)
        assert proc.returncode != 0, leg
        lines[leg] = sg._exception_line(proc.stderr)
        print(leg, lines[leg])
        assert not (out / "pe_info").exists() and not (out / "st_info").exists(), leg
    assert lines["device"] == lines["host"]
    assert "not a complete gzip stream (zlib code" in lines["device"]


@pytest.mark.parametrize("bad", ["truncated", "bad_crc"])
def test_gzip_device_errors_through_a_pipe_name_the_device_status(tmp_path, bad):
    """A pipe cannot be read again by zlib: the same exception type, the file's name, the device's status by name."""
    d, meta, fwd, rve, data = _bad_pair(tmp_path, bad)
    with sg.Fifos(tmp_path, data, open(rve, "rb").read()) as (pf, pr):
        proc = sg._drop_in(d, meta, pf, pr, tmp_path / "aln_pipe", env=_clean_env(VS_GZIP_DEVICE="1"))
    assert proc.returncode != 0
    line = sg._exception_line(proc.stderr)
    print("pipe", line)
    assert line.startswith("vstrains_amd._native.NativeError:") and pf in line and "not a complete gzip stream" in line
    assert ("device status INF_E_INPUT" if bad == "truncated" else "device status INF_E_CRC") in line
    assert not (tmp_path / "aln_pipe" / "pe_info").exists()


def test_gzip_device_is_refused_under_two_ranks(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    fwd, rve = _golden_gz(tmp_path, d)
    proc = sh._torchrun(2, d, meta, fwd, rve, tmp_path / "aln", tmp_path / "report", env=_clean_env(VS_GZIP_DEVICE="1"), timeout=300)
    assert proc.returncode != 0
    assert "ValueError" in proc.stderr and "VS_GZIP_DEVICE=1" in proc.stderr and "is not built" in proc.stderr
    assert not (tmp_path / "aln" / "pe_info").exists()
