"""BGZF on the device: the inflate kernel (vs_inflate_bgzf) on the corpus the CPU suite runs through its host form, and the
streamed ingest on BGZF files -- the counters of the mapped ingest bit for bit, the members inflated where they should be,
the failures worded as the host zlib leg words them."""
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_util as bz
import test_fastq_stream_gpu as sg
from conftest import ROOT, pe_cases

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


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def test_kernel_equals_zlib_on_the_corpus_good_and_bad_in_one_batch(host, ctx):
    good, bad = bz.good_corpus(), bz.bad_corpus()
    batch, want = [], []
    for i in range(max(len(good), len(bad))):  # interleaved: every member its own verdict
        if i < len(good):
            name, raw, text = good[i]
            batch.append(bz.wrap(raw, text))
            want.append((name, text))
        if i < len(bad):
            name, raw, isize, crc = bad[i]
            batch.append(bz.wrap(raw, b"", crc=crc & 0xFFFFFFFF, isize=isize))
            want.append((name, None))
    got = host.inflate_bgzf(b"".join(batch), ctx)
    assert len(got) == len(want)
    for (name, text), (status, out, guard) in zip(want, got):
        print(name, status)
        assert guard, name
        if text is None:
            assert status != 0, name
        else:
            assert status == 0 and out == text, (name, status)
    by_name = {name: g[0] for (name, _), g in zip(want, got)}
    assert by_name["too_far_back"] == 7 and by_name["btype3"] == 1 and by_name["stored_len_nlen"] == 2
    assert by_name["cl_oversubscribed"] == 3 and by_name["litlen_incomplete"] == 4
    assert by_name["fixed_symbol_286"] == 5 and by_name["fixed_distance_31"] == 6
    assert by_name["cut_by_half"] == 8 and by_name["wrong_crc"] == 11 and by_name["wrong_isize"] == 10 and by_name["isize_too_small"] == 9


@pytest.mark.parametrize("which", [0, 1], ids=["dynamic", "fixed"])
def test_kernel_verdict_equals_zlib_for_single_bit_flips(host, ctx, which):
    """Every bit of the header and the trailer and every 8th bit of the payload, all flipped members in ONE batch."""
    name, good, text = bz.flip_members()[which]
    (off, n, isize, crc), = bz.py_walk(good)[0]
    bits = list(range(18 * 8)) + list(range(18 * 8, (off + n) * 8, 8)) + list(range((off + n) * 8, len(good) * 8))
    batch, want, rejected_before = [], [], 0
    for bit in bits:
        blk = bytearray(good)
        blk[bit >> 3] ^= 1 << (bit & 7)
        blk = bytes(blk)
        members, at, state = bz.py_walk(blk)
        if state != 0 or at != len(blk) or len(members) != 1:
            rejected_before += 1  # (the walker does not hand it on)
            continue
        o, ln, isz, c = members[0]
        header = bit < 18 * 8
        ok, out = bz.payload_verdict(blk[o:o + ln], isz, c)
        batch.append(blk)
        want.append((bit, header, ok, out))
    got = host.inflate_bgzf(b"".join(batch), ctx)
    assert len(got) == len(want) and len(want) > 0.8 * len(bits)
    same = 0
    for (bit, header, ok, out), (status, text_got, guard) in zip(want, got):
        assert guard, bit
        if header:
            assert status != 0 or text_got == text, bit
        else:
            assert (status == 0) == ok, (bit, status, ok)
        if status == 0:
            assert text_got == text, bit
            same += 1
    assert 0 < same < 0.1 * len(want), (same, len(want), rejected_before)


# ---- the streamed ingest ------------------------------------------------------------------------------------------------
def _count_stream(host, ctx, g, fwd, rve):
    from vstrains_amd import pe_inference

    fs = host.FastqStream(fwd, rve, ctx, block_pairs=173)
    try:
        ctx.build_index(g.seqs, 21)
        counter = host.PeCounter(ctx)
        pe_inference.count_stream(ctx, fs, counter)
        info = fs.info
    finally:
        fs.close()
    return counter.result() + (info["pairs"],), info


def _mapped(host, ctx, g, tmp_path, tf, tr):
    (tmp_path / "f.fq").write_bytes(tf)
    (tmp_path / "r.fq").write_bytes(tr)
    return sg._count(host, ctx, g, host.FastqPair(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx), False)


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3]


BGZF_KINDS = ["plain", "crlf", "lone_cr", "no_final_newline", "unequal", "odd_bytes", "empty"]


@pytest.mark.parametrize("chunk", [None] + list(sg.TINY_CHUNKS), ids=["default"] + ["chunk%d" % c for c in sg.TINY_CHUNKS])
@pytest.mark.parametrize("kind", BGZF_KINDS)
def test_bgzf_stream_counters_equal_mapped(host, ctx, tmp_path, monkeypatch, kind, chunk):
    g, f, r = sg._synth_reads(2500 if chunk is None else 300, seed=11)
    tf, tr = sg._variant(kind, f, r)
    want = _mapped(host, ctx, g, tmp_path, tf, tr)
    block = bz.MAX_IN if chunk is None else 5000
    (tmp_path / "f.fq.gz").write_bytes(bz.bgzf(tf, block=block))
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr, level=1, block=block - 77, eof=False))
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    paths = (str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    got, info = _count_stream(host, ctx, g, *paths)
    _same(got, want)
    n_f, n_r = -(-len(tf) // block) + 1, -(-len(tr) // (block - 77))
    assert info["members_host"] == (0, 0)
    if kind == "unequal":  # (the rest of the longer file is inflated on the device as well)
        assert info["members_device"] == (n_f, n_r)
    assert info["members_device"][0] > 0 and (info["members_device"][1] > 0 or kind == "empty")
    assert info["text_bytes"] == len(tf) + len(tr)
    assert info["file_bytes"] == sum(os.path.getsize(p) for p in paths)
    if kind != "empty":
        assert want[3] > 0
    monkeypatch.setenv("VS_BGZF_DEVICE", "0")
    got, info = _count_stream(host, ctx, g, *paths)
    _same(got, want)
    assert info["members_device"] == (0, 0) and info["members_host"] == (n_f, n_r)


@pytest.mark.parametrize("chunk", [None, 1000], ids=["default", "chunk1000"])
def test_bgzf_rest_of_the_longer_file_is_still_validated(host, ctx, tmp_path, monkeypatch, chunk):
    g, f, r = sg._synth_reads(600, seed=11)
    tf, tr = sg._variant("unequal", f, r)
    lines = tf.split(b"\n")
    at = 4 * 550 + 1  # a sequence line of a record beyond the shorter file's end
    lines[at] = lines[at][:10] + b"\xff" + lines[at][11:]
    tf = b"\n".join(lines)
    (tmp_path / "f.fq").write_bytes(tf)
    (tmp_path / "r.fq").write_bytes(tr)
    with pytest.raises(ValueError) as mapped:
        host.FastqPair(str(tmp_path / "f.fq"), str(tmp_path / "r.fq"), ctx)
    (tmp_path / "f.fq.gz").write_bytes(bz.bgzf(tf, block=4000))
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr, block=4000))
    if chunk is not None:
        monkeypatch.setenv("VS_STREAM_CHUNK", str(chunk))
    with pytest.raises(ValueError) as streamed:
        _count_stream(host, ctx, g, str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    assert "not valid UTF-8" in str(streamed.value) and "not valid UTF-8" in str(mapped.value)


@pytest.mark.parametrize("shape", ["bgzf_then_gzip", "gzip_then_bgzf", "two_bgzf_files"])
def test_bgzf_mixed_with_other_gzip_members(host, ctx, tmp_path, shape):
    g, f, r = sg._synth_reads(1500, seed=11)
    tf, tr = sg._variant("plain", f, r)
    want = _mapped(host, ctx, g, tmp_path, tf, tr)
    half = len(tf) // 2 + 13
    if shape == "bgzf_then_gzip":
        zf = bz.bgzf(tf[:half], block=9000, eof=False) + gzip.compress(tf[half:])
    elif shape == "gzip_then_bgzf":
        zf = gzip.compress(tf[:half]) + bz.bgzf(tf[half:], block=9000)
    else:
        zf = bz.bgzf(tf[:half], block=9000) + bz.bgzf(tf[half:], block=9000)
    (tmp_path / "f.fq.gz").write_bytes(zf)
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr))
    got, info = _count_stream(host, ctx, g, str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz"))
    _same(got, want)
    dev, hst = info["members_device"][0], info["members_host"][0]
    n_first, n_second = -(-half // 9000), -(-(len(tf) - half) // 9000)
    if shape == "bgzf_then_gzip":
        assert (dev, hst) == (n_first, 1)
    elif shape == "gzip_then_bgzf":
        assert (dev, hst) == (0, 1 + n_second + 1)  # (a file that starts with another member never leaves the zlib loop)
    else:
        assert (dev, hst) == (n_first + 1 + n_second + 1, 0)
    assert info["members_device"][1] > 0 and info["members_host"][1] == 0


def _bad_bgzf(kind, text):
    members = [bz.member(text[i:i + len(text) // 5 + 1]) for i in range(0, len(text), len(text) // 5 + 1)]
    assert len(members) == 5
    whole = b"".join(members) + bz.EOF_MARK
    if kind == "cut_in_member":
        return whole[: len(members[0]) + len(members[1]) + len(members[2]) // 2]
    if kind == "cut_in_header":
        return whole[: len(members[0]) + len(members[1]) + 9]
    if kind == "trailing_garbage":
        return whole + b"this is no gzip member"
    assert kind == "bit_flip"
    at = len(members[0]) + len(members[1]) + 18 + (len(members[2]) - 26) // 2
    for bit in range(8):
        bad = bytearray(members[2])
        bad[at - len(members[0]) - len(members[1])] ^= 1 << bit
        if not bz.zlib_verdict(bytes(bad))[0]:
            return whole[:at] + bytes([whole[at] ^ (1 << bit)]) + whole[at + 1:]
    raise AssertionError("zlib accepts every flip of that byte")


@pytest.mark.parametrize("bad", ["cut_in_member", "cut_in_header", "bit_flip", "trailing_garbage"])
def test_bgzf_errors_are_worded_as_the_host_zlib_leg_words_them(tmp_path, bad):
    """The device leg's exception line is, character for character, the streamed host-zlib leg's (VS_BGZF_DEVICE=0); it has
    the mapped path's class and message up to the zlib code (the mapped open reports zlib's raw code)."""
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    with open(os.path.join(d, "fwd.fq"), "rb") as fh:
        tf = fh.read()
    with open(os.path.join(d, "rve.fq"), "rb") as fh:
        tr = fh.read()
    fwd, rve = str(tmp_path / "f.fq.gz"), str(tmp_path / "r.fq.gz")
    (tmp_path / "f.fq.gz").write_bytes(_bad_bgzf(bad, tf))
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(tr))
    base = {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")}
    legs = {"mapped": dict(base, VS_FASTQ_STREAM="0"), "device": base, "host": dict(base, VS_BGZF_DEVICE="0", VS_FASTQ_STREAM="1")}
    lines = {}
    for leg, env in legs.items():
        out = tmp_path / ("aln_" + leg)
        proc = sg._drop_in(d, meta, fwd, rve, out, env=env)
        assert proc.returncode != 0, leg
        lines[leg] = sg._exception_line(proc.stderr)
        print(leg, lines[leg])
        assert not (out / "pe_info").exists() and not (out / "st_info").exists(), leg
        assert not any(l.startswith("Number of processed reads") for l in proc.stdout.splitlines()), leg
    assert lines["device"] == lines["host"]
    assert "not a complete gzip stream (zlib code" in lines["device"]
    assert lines["device"].split(":")[0] == lines["mapped"].split(":")[0]
    assert lines["device"].split("(zlib code")[0] == lines["mapped"].split("(zlib code")[0]


_INFO_SCRIPT = r"""
import resource, sys
from vstrains_amd import pe
_close = pe.FastqStream.close
def close(self):
    if self._h:
        print("STREAM_INFO", self.info)
    _close(self)
pe.FastqStream.close = close
mod = sys.argv[1]
if mod == "pe_inference":
    from vstrains_amd import pe_inference
    pe_inference.main(sys.argv[2:])
else:
    from vstrains_amd import cli
    cli.main(sys.argv[2:])
print("PEAK_RSS_KB", resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)
"""


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")}


def _stream_info(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("STREAM_INFO")]
    assert lines, stdout[-2000:]
    return eval(lines[0][len("STREAM_INFO "):])


def test_drop_in_on_regular_bgzf_files_with_no_switch_set(tmp_path):
    name, d, meta = [c for c in pe_cases() if c[0] == "errors_k21"][0]
    for which in ("fwd", "rve"):
        with open(os.path.join(d, which + ".fq"), "rb") as fh:
            (tmp_path / (which + ".fq.gz")).write_bytes(bz.bgzf(fh.read(), block=7000))
    out = tmp_path / "aln"
    proc = subprocess.run([sys.executable, "-c", _INFO_SCRIPT, "pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(out) + "/",
                           "-f", str(tmp_path / "fwd.fq.gz"), "-r", str(tmp_path / "rve.fq.gz"), "-k", str(meta["k"])],
                          cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert sg._read(out / "pe_info") == sg._read(os.path.join(d, "pe_info"))
    assert sg._read(out / "st_info") == sg._read(os.path.join(d, "st_info"))
    assert [l for l in proc.stdout.splitlines() if l.startswith("Number of processed reads")] == meta["progress_lines"]
    info = _stream_info(proc.stdout)
    assert min(info["members_device"]) > 0 and info["members_host"] == (0, 0)


def test_whole_command_on_regular_bgzf_files(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from graph_case import Case

    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path), with_reads=True)

    def run(fwd, rve, out):
        return subprocess.run(
            [sys.executable, "-c", _INFO_SCRIPT, "cli", "-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", str(out),
             "-fwd", fwd, "-rve", rve], cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=600)

    plain = run(inp["fwd"], inp["rve"], tmp_path / "out_files")
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert "STREAM_INFO" not in plain.stdout  # (plain regular files are mapped)
    for which in ("fwd", "rve"):
        with open(inp[which], "rb") as fh:
            (tmp_path / (which + ".fq.gz")).write_bytes(bz.bgzf(fh.read(), block=20000))
    packed = run(str(tmp_path / "fwd.fq.gz"), str(tmp_path / "rve.fq.gz"), tmp_path / "out_bgzf")
    assert packed.returncode == 0, packed.stderr[-3000:]
    for rel in ("strain.paths", "strain.fasta"):
        assert sg._read(tmp_path / "out_bgzf" / rel) == sg._read(tmp_path / "out_files" / rel), rel
    info = _stream_info(packed.stdout)
    assert min(info["members_device"]) > 0 and info["members_host"] == (0, 0)


def test_bgzf_stream_memory_does_not_grow_with_input(tmp_path):
    """Peak RSS of the drop-in on a 0.5 M-pair and a 4 M-pair BGZF pair: within one ring (both files) of each other."""
    from vstrains_amd import synth

    name, d, meta = [c for c in pe_cases() if c[0] == "hiv_like_k55"][0]
    st = synth.make_strains(4, 1500, 0.02, seed=21)
    f, r = synth.sample_pairs(st, 50000, 150, seed=22, sub_rate=0.005)
    mf = bz.bgzf(synth.fastq_text(f, "f").encode(), level=1, eof=False)
    mr = bz.bgzf(synth.fastq_text(r, "r").encode(), level=1, eof=False)
    rss = {}
    for copies in (10, 80):
        (tmp_path / "f.fq.gz").write_bytes(mf * copies)
        (tmp_path / "r.fq.gz").write_bytes(mr * copies)
        proc = subprocess.run([sys.executable, "-c", _INFO_SCRIPT, "pe_inference", "-g", os.path.join(d, "graph.gfa"), "-o", str(tmp_path / "aln"),
                               "-f", str(tmp_path / "f.fq.gz"), "-r", str(tmp_path / "r.fq.gz"), "-k", str(meta["k"])],
                              cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=900)
        assert proc.returncode == 0, proc.stderr[-3000:]
        assert "Number of processed reads:  %d" % (copies * 50000 - 100000) in proc.stdout
        info = _stream_info(proc.stdout)
        assert info["pairs"] == copies * 50000 and min(info["members_device"]) > 0 and info["members_host"] == (0, 0)
        rss[copies] = int([l for l in proc.stdout.splitlines() if l.startswith("PEAK_RSS_KB")][0].split()[1]) * 1024
    ring = 2 * 4 * (64 << 20)
    assert abs(rss[80] - rss[10]) < ring, rss
