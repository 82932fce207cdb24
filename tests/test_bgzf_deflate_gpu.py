"""The BGZF encoder on the device: k_deflate, one wavefront per member, through the test aid ``vs_deflate_bgzf``.  Every member
must pass what the twin's members pass on the CPU (zlib is the oracle) AND equal the twin's member byte for byte: the
compressed bytes are a function of the text, not of scheduling.  The aid itself checks the 0xA5 guard bytes behind every
device slot, and the rest of the slot behind the member, before the members are packed."""
import gzip

import pytest

import bgzf_util as bu
import deflate_cases as dc

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in dc.members()]


@pytest.fixture(scope="module")
def ctx():
    from vstrains_amd import pe as host

    c = host.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_members(ctx):
    """every corpus text through the kernel once: name -> (file bytes, info)"""
    out = {}
    for name, text in dc.members():
        rc, data, info = dc.deflate_device(ctx, text)
        assert rc == 0, name
        out[name] = (data, info)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_member_of_the_kernel(device_members, name):
    text = dict(dc.members())[name]
    data, info = device_members[name]
    assert data.endswith(bu.EOF_MARK) and info[1] == len(data)
    member = data[:-len(bu.EOF_MARK)]
    twin, kind = dc.host_member(name)
    if not text:  # no text, no member: the file is the EOF member alone
        assert member == b"" and info[0] == 0
        return
    assert info[0] == 1 and info[2:] == [int(kind == k) for k in (dc.STORED, dc.FIXED, dc.DYNAMIC)]
    dc.check_member(member, text)
    assert member == twin  # byte for byte what one lane writes


def test_every_kind_came_out_of_the_kernel(device_members):
    seen = [sum(device_members[name][1][2 + k] for name in NAMES) for k in range(3)]
    assert all(seen), seen
    assert len(device_members["random_full"][0]) == dc.MAX_TEXT + 31 + 28


@pytest.mark.parametrize("guard", [0, 1, 64, 4096])
def test_four_members_packed_on_the_device(ctx, guard):
    text = dc.multi_text()
    rc, data, info = dc.deflate_device(ctx, text, guard=guard)
    assert rc == 0 and info[0] == 4 and info[1] == len(data) and sum(info[2:]) == 4
    found, at, verdict = bu.py_walk(data)
    assert verdict == 0 and at == len(data) and len(found) == 5
    assert [m[2] for m in found] == [dc.MAX_TEXT] * 3 + [17, 0]
    assert data.endswith(bu.EOF_MARK)
    assert gzip.decompress(data) == text
    twin = b"".join(dc.deflate_host(text[at:at + dc.MAX_TEXT])[1] for at in range(0, len(text), dc.MAX_TEXT)) + bu.EOF_MARK
    assert data == twin


def test_bad_arguments(ctx):
    from vstrains_amd import _native as nat
    import ctypes as C
    import numpy as np

    text = np.frombuffer(dc.golden_dense(), dtype=np.uint8)
    out = np.zeros(100, dtype=np.uint8)
    info = (C.c_uint64 * 5)()
    assert nat.lib().vs_deflate_bgzf(ctx._h, text.ctypes.data, text.size, out.ctypes.data, out.size, 16, info) == nat.VS_E_RANGE
    assert not out.any()
    assert nat.lib().vs_deflate_bgzf(ctx._h, text.ctypes.data, text.size, None, 0, 16, info) == nat.VS_E_ARG
