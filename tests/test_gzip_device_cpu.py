"""Plain gzip decoded in parallel, on the host: every routine of vstrains_amd/csrc/vs_gzip_core.h with one lane
(``vs_gzip_inflate_host``: find, count, chain, decode to symbols, windows, resolve, trailers -- the steps the kernels take,
in the same text).  zlib is the oracle.  tests/gzip_check.cpp drives the header as plain C++ under the sanitizers."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import gzip_cases as gc
from conftest import ROOT


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.mark.parametrize("gran", [gc.EVERY, gc.COARSE], ids=["every", "coarse"])
def test_host_twin_equals_zlib_on_every_case(host, gran):
    for name, data, text in gc.good_cases():
        info, got = host.gzip_inflate_host(data, gran)
        print(name, gran, len(data), len(text), info)
        assert info["status"] == 0 and got == text, (name, info)
        assert info["text"] == len(text) and info["chain_runs"] + info["dropped"] == info["selected"] + 1, (name, info)


def test_chain_is_made_of_many_runs(host):
    """The counts the one-lane twin reports for the cases that are about them (recorded, then held): the stream of small
    blocks cannot pass by being decoded in one run, the default blocks are runs of more than 32 KiB of text."""
    by_name = {name: (data, text) for name, data, text in gc.good_cases()}
    data, text = by_name["small_blocks"]
    info, _ = host.gzip_inflate_host(data, gc.EVERY)
    print("small_blocks", len(data), info)
    assert info["chain_runs"] >= 100 and info["members"] == 1  # (206 runs from 54 609 compressed bytes)
    coarse, _ = host.gzip_inflate_host(data, gc.COARSE)
    assert 2 <= coarse["chain_runs"] <= -(-len(data) // gc.COARSE) + 1 and coarse["chain_runs"] < info["chain_runs"]
    data, text = by_name["default_blocks"]
    info, _ = host.gzip_inflate_host(data, gc.EVERY)
    print("default_blocks", len(data), info)
    assert 4 <= info["chain_runs"] and len(text) / info["chain_runs"] > 32768
    for name in ("stored_only", "fixed_only", "empty_text"):  # no dynamic block: one run, and correct
        info, got = host.gzip_inflate_host(by_name[name][0], gc.EVERY)
        assert info["chain_runs"] == 1 and info["status"] == 0 and got == by_name[name][1], (name, info)
    info, got = host.gzip_inflate_host(by_name["false_candidate"][0], gc.EVERY)
    print("false_candidate", info)
    assert info["dropped"] >= 1 and info["candidates"] > info["chain_runs"] - 1 and got == by_name["false_candidate"][1]
    for gran in (gc.EVERY, gc.COARSE):  # a chain run past its span of input is counted again, no other case needs that
        info, got = host.gzip_inflate_host(by_name["long_stored_between_dynamic"][0], gran)
        print("long_stored_between_dynamic", gran, info)
        assert info["recounted"] == 1 and info["status"] == 0 and got == by_name["long_stored_between_dynamic"][1]
    assert all(host.gzip_inflate_host(by_name[n][0], gc.EVERY)[0]["recounted"] == 0 for n in ("small_blocks", "default_blocks", "false_candidate"))
    for name, members in (("three_members", 3), ("empty_member_in_the_middle", 3), ("members_of_stored_and_fixed", 3)):
        info, _ = host.gzip_inflate_host(by_name[name][0], gc.EVERY)
        assert info["members"] == members, (name, info)


@pytest.mark.parametrize("gran", [gc.EVERY, gc.COARSE], ids=["every", "coarse"])
def test_host_twin_refuses_what_zlib_refuses(host, gran):
    want = {"cut_inside_a_block": 8, "cut_inside_the_first_block": 8, "cut_inside_the_trailer": 8, "cut_before_the_trailer": 8,
            "crc_off_by_one_bit": 11, "isize_off_by_one": 16, "second_member_cut": 8, "second_member_bad_crc": 11,
            "no_member_behind_the_first": 15, "match_in_front_of_its_member": 7, "far_match_in_front_of_its_member": 7}
    for name, data in gc.bad_cases():
        info, got = host.gzip_inflate_host(data, gran)
        print(name, gran, info)
        assert info["status"] != 0 and got == b"" and info["text"] == 0, (name, info)
        if name in want:
            assert info["status"] == want[name], (name, info)


def _random_stream(rng, pool):
    members, texts = [], []
    for _ in range(int(rng.integers(1, 4))):
        n = int(rng.integers(5_000, 300_000)) // int(rng.integers(1, 4))
        at = int(rng.integers(0, len(pool) - n))
        text = pool[at: at + n]
        level = int(rng.choice([0, 1, 6, 9]))
        mem = int(rng.choice([1, 1, 2, 3, 8, 9]))
        strategy = int(rng.choice([zlib.Z_DEFAULT_STRATEGY] * 4 + [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]))
        flushes = tuple((int(p), int(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_BLOCK] if hasattr(zlib, "Z_BLOCK") else [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])))
                        for p in sorted(rng.integers(0, n, size=int(rng.integers(0, 4)))))
        members.append(gc.member(gc.raw(text, level, mem, strategy, flushes), text))
        texts.append(text)
    return b"".join(members), b"".join(texts)


def test_seeded_fuzz_of_small_streams(host):
    rng = np.random.default_rng(20240611)
    pool = gc.fastq_with_edits(600_000, seed=11)
    runs = 0
    for i in range(200):
        data, text = _random_stream(rng, pool)
        assert gc.zlib_text(data) == text
        gran = gc.EVERY if i % 2 == 0 else int(rng.integers(16, 20_000))
        info, got = host.gzip_inflate_host(data, gran)
        assert info["status"] == 0 and got == text, (i, gran, info)
        runs += info["chain_runs"]
    print("chain runs in all:", runs)
    assert runs > 2000


def test_gzip_entries_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_gzip_inflate", "vs_gzip_inflate_host", "vs_fastq_stream_gzip_info"):
        assert name + "(" in header
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/gzip_check.cpp: the header as plain C++, one lane, exactly sized heap buffers, AddressSanitizer and UBSan; the
    cases as files, a small stream cut at every byte length and with every bit of its first 64 bytes flipped."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gzip_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "gzip_check.cpp"), "-o", exe, "-lz"])
    names = []
    for name, data, text in gc.good_cases():
        (tmp_path / (name + ".gz")).write_bytes(data)
        (tmp_path / (name + ".txt")).write_bytes(text)
        names.append(name)
    for name, data in gc.bad_cases():
        (tmp_path / (name + ".gz")).write_bytes(data)
        names.append(name)
    small = gc.fastq_with_edits(3000, seed=3)
    (tmp_path / "small.gz").write_bytes(gc.member(gc.raw(small[:1500], 6, 1), small[:1500]) + gc.member(gc.raw(small[1500:], 6, 1), small[1500:]))
    (tmp_path / "small.txt").write_bytes(small)
    run = subprocess.run([exe, str(tmp_path), "small"] + names, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    verdict = {l.split()[0]: l.split()[1] for l in lines if l.split()[1:2] and l.split()[1] in ("good", "refused")}
    assert all(verdict[name] == "good" for name, _, _ in gc.good_cases()), verdict
    assert all(verdict[name] == "refused" for name, _ in gc.bad_cases()), verdict
    cuts = [l for l in lines if l.startswith("small cuts")]
    flips = [l for l in lines if l.startswith("small flips")]
    assert len(cuts) == 1 and len(flips) == 1
    print(cuts[0], "|", flips[0])
    assert int(flips[0].split()[2]) == 2 * 512


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_use_stream_and_the_refusals_with_the_switch_on(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference as pi

    for k in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_GZIP_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    text = gc.fastq_with_edits(4000)
    plain, gz, other = str(tmp_path / "a.fq"), str(tmp_path / "b.fq.gz"), str(tmp_path / "c.fq")
    open(plain, "wb").write(text)
    open(other, "wb").write(text)
    open(gz, "wb").write(gc.member(gc.raw(text), text))
    assert not pi.use_stream(plain, gz) and not pi.use_stream(gz, gz)  # (off: regular gzip files keep the mapped open)
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    assert pi.use_stream(plain, gz) and pi.use_stream(gz, plain) and pi.use_stream(gz, gz)
    assert not pi.use_stream(plain, other)  # (each file is judged on its own: plain text keeps the plain path)
    assert pi.gzip_device_refusal(1) is None
    assert "is not built" in pi.gzip_device_refusal(2)
    monkeypatch.setenv("VS_FASTQ_STREAM", "0")
    assert "VS_FASTQ_STREAM=0" in pi.gzip_device_refusal(1)
    with pytest.raises(ValueError, match="VS_FASTQ_STREAM=0"):
        pi.use_stream(gz, gz)
    monkeypatch.setenv("VS_GZIP_DEVICE", "0")
    assert pi.gzip_device_refusal(2) is None and not pi.use_stream(gz, gz)
    for mod in ("pe_inference", "cli"):  # the flags exist and only set the switch
        src = open(os.path.join(ROOT, "vstrains_amd", mod + ".py")).read()
        assert '"--gzip-device"' in src and 'os.environ["VS_GZIP_DEVICE"] = "1"' in src
