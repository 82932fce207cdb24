"""The BGZF encoder without a device: ``vs_deflate_host`` runs the text the kernel runs (csrc/vs_deflate_core.h) with one lane,
and every output byte is the same for 1 lane and for 64, so what is shown here holds for the device (test_bgzf_deflate_gpu.py
compares the two byte for byte).  zlib is the oracle.  tests/deflate_check.cpp drives the same header as plain C++ under
AddressSanitizer and UBSan, with every buffer exactly sized, and the code-length builder alone."""
import gzip
import os
import shutil
import subprocess
import zlib

import pytest

import bgzf_util as bu
import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [name for name, _ in dc.members()]


@pytest.mark.parametrize("name", NAMES)
def test_member_of_the_twin(name):
    text = dict(dc.members())[name]
    member, kind = dc.host_member(name)
    dc.check_member(member, text)
    assert dc.block_type(member) == kind


def test_every_kind_occurs_and_where_it_must():
    kinds = {name: dc.host_member(name)[1] for name in NAMES}
    assert set(kinds.values()) == {dc.STORED, dc.FIXED, dc.DYNAMIC}
    # incompressible text takes the stored form: exactly n + 31 bytes
    assert kinds["random_full"] == dc.STORED and len(dc.host_member("random_full")[0]) == dc.MAX_TEXT + 31
    assert kinds["dense_pe_info"] == dc.DYNAMIC and kinds["sparse_pe_info"] == dc.DYNAMIC and kinds["fastq"] == dc.DYNAMIC
    assert dc.host_member("len_0")[0] == bu.EOF_MARK  # the empty member is the EOF member, byte for byte


def test_runs_collapse():
    """distance 1 / 2 with length 258 over and over: a member of 64 KiB of one byte is a few dozen tokens' worth of bits"""
    for name in ("a_full", "zeros_full", "ab_20000"):
        assert len(dc.host_member(name)[0]) < 400, name
    assert len(dc.host_member("a_259")[0]) <= 18 + 5 + 8  # a literal, one match, end of block


def test_the_distance_limit_is_where_rfc_1951_puts_it():
    """A copy that starts 32768 back is taken, one that starts 32769 back is not (zlib would refuse the member: check_member
    has shown it does not).  With the zero filler the first 300 bytes are still in the hash table when their copy arrives,
    so the two members differ by about the 300 literals; with the random filler they were overwritten long before, and
    both members are stored."""
    near, far = dc.host_member("far_32768_zeros")[0], dc.host_member("far_32769_zeros")[0]
    assert len(far) - len(near) > 200
    assert dc.host_member("far_32768_random")[1] == dc.STORED and dc.host_member("far_32769_random")[1] == dc.STORED


def test_a_buffer_one_byte_short_is_refused_and_left_alone():
    from vstrains_amd import _native as nat

    for name in ("dense_pe_info", "random_full", "len_0"):
        text = dict(dc.members())[name]
        member, _ = dc.host_member(name)
        rc, got, _ = dc.deflate_host(text, cap=len(member))  # exactly its size: fits
        assert rc == 0 and got == member
        rc, got, _ = dc.deflate_host(text, cap=len(member) - 1)
        assert rc == nat.VS_E_RANGE and got == b""
    rc, _, _ = dc.deflate_host(bytes(dc.MAX_TEXT + 1), cap=70000)
    assert rc == nat.VS_E_ARG


def test_members_are_a_function_of_the_text_alone():
    text = dict(dc.members())["dense_pe_info"]
    assert dc.deflate_host(text)[1] == dc.host_member("dense_pe_info")[0]
    assert dc.deflate_host(text, cap=65536)[1] == dc.host_member("dense_pe_info")[0]


def _twin_file(text: bytes) -> bytes:
    out = []
    for at in range(0, len(text), dc.MAX_TEXT):
        rc, member, _ = dc.deflate_host(text[at:at + dc.MAX_TEXT])
        assert rc == 0
        out.append(member)
    return b"".join(out) + bu.EOF_MARK


@pytest.fixture(scope="module")
def synth_sparse_text():
    """the sparse pe_info text of a random graph of a few hundred nodes (ids as test_sparse_info_gpu.py's workload names them)"""
    import numpy as np

    rng = np.random.default_rng(31)
    n = 300
    ids = ["%d%s" % (i, "&%d*0" % i if i % 5 == 0 else "") for i in range(n)]
    lines = []
    for i in range(n):
        for j in np.flatnonzero(rng.random(n) < 0.04):
            lines.append("%s:%s:%d\n" % (ids[i], ids[int(j)], int(rng.integers(1, 40))))
    return "".join(lines).encode()


# Measured with the twin (profiles/bgzf_info.md): file size / len(bgzf_util.bgzf(text, 1)), zlib level 1 with the same member
# cut.  The margin over 1.0 is what a single-candidate greedy matcher costs against zlib's chains; asserted: the figure + 0.05.
RATIO_DENSE, RATIO_SPARSE = 0.848, 0.998


def test_compression_against_zlib(synth_sparse_text):
    """Smaller than a fixed-code compressor (zlib level 1 with Z_FIXED reaches 12.4 kB on the dense golden text, level 1 8.1 kB):
    that holds only if the dynamic block is live and the matches 10 - 60 bytes back, inside a chunk of 64 positions, are
    found.  The ratio to zlib level 1 is printed and held at the recorded figure + 0.05."""
    for name, text, recorded in (("dense", dc.golden_dense(), RATIO_DENSE), ("sparse", synth_sparse_text, RATIO_SPARSE)):
        ours = _twin_file(text)
        assert gzip.decompress(ours) == text
        fixed, level1 = len(bu.bgzf(text, 1, zlib.Z_FIXED)), len(bu.bgzf(text, 1))
        ratio = len(ours) / level1
        print("%s: text %d, file %d, zlib level 1 %d, zlib level 1 fixed codes %d, ratio to level 1 %.3f" % (name, len(text), len(ours), level1, fixed, ratio))
        assert len(ours) < fixed, name
        assert ratio <= recorded + 0.05, (name, ratio)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/deflate_check.cpp: the header as plain C++, one lane, exactly sized heap buffers, AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "deflate_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "deflate_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    kinds = {l.split()[0]: int(l.split()[-1].split("=")[1]) for l in lines if " kind=" in l}
    assert set(kinds.values()) == {0, 1, 2} and kinds["random_full"] == 0
    assert sum(1 for l in lines if l.startswith("fib_")) >= 20 and sum(1 for l in lines if l.startswith("single_")) == 8
