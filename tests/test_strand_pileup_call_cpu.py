"""The rule of one position (csrc/vs_pileup_call_core.h), the code both passes of the device caller run, through its host
entry ``vs_pileup_call_host`` against the record rule of tests/strand_pileup_model.py: small exhaustive grids of (ref,
depth, alt) per plane, the equality cases of the fraction, and with one plane ``node_depth.variant_records`` on the same
tables.  No device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import strand_pileup_model as model
from vstrains_amd import _native as nat
from vstrains_amd import node_depth
from vstrains_amd import pe as host

ACGT = "ACGT"


def _want(ref, depth, alt, C_, F, S):
    """The model's records in the shape of ``pe.pileup_call_host``."""
    r = ACGT.index(ref)
    return [(int(fail), r, ACGT.index(b), dp) + dp4 for b, dp, ad, dp4, fail in model.position_records(ref, depth, alt, C_, F, S)]


def _alts(ref, values):
    """Every alt row [A, C, G, T, other] over ``values`` with 0 in the column of ``ref`` (no read differs by carrying the segment's base)."""
    r = ACGT.index(ref)
    for combo in itertools.product(values, repeat=4):
        row = list(combo)
        row.insert(r, 0)
        yield row


@pytest.mark.parametrize("ref", ACGT)
def test_two_planes_on_an_exhaustive_grid(ref):
    rows = list(_alts(ref, (0, 1, 3)))
    n = 0
    for a0, a1 in itertools.product(rows, rows[::2]):
        for agree in ((0, 0), (5, 0), (2, 40)):
            depth = [sum(a0) + agree[0], sum(a1) + agree[1]]
            for C_, F, S in ((0, 0.0, 0), (2, 0.01, 0), (2, 0.1, 1), (3, 0.25, 2)):
                assert host.pileup_call_host(ACGT.index(ref), depth, [a0, a1], C_, F, S) == _want(ref, depth, [a0, a1], C_, F, S), (depth, a0, a1, C_, F, S)
                n += 1
    assert n == 81 * 41 * 3 * 4


@pytest.mark.parametrize("ref", ACGT)
def test_one_plane_on_an_exhaustive_grid(ref):
    for a0 in _alts(ref, (0, 1, 2, 7)):
        for agree in (0, 1, 93):
            depth = [sum(a0) + agree]
            for C_, F in ((0, 0.0), (2, 0.01), (2, 0.07), (1, 0.5)):
                got = host.pileup_call_host(ACGT.index(ref), depth, [a0], C_, F)
                assert got == _want(ref, depth, [a0], C_, F, 0), (depth, a0, C_, F)
                assert all(r[5] == r[7] == 0 for r in got)  # (ref_r and alt_r of one plane)


# F * DP == AD in the reals; whether the double product exceeds AD (the last column: is it a record) was worked out once by hand
EQUALITY = [(0.25, 8, 2, True), (0.07, 100, 7, False), (0.29, 100, 29, True), (0.01, 200, 2, True), (0.01, 1000, 10, True), (0.1, 30, 3, True),
            (0.7, 10, 7, True), (0.57, 100, 57, True), (0.14, 50, 7, False), (0.28, 25, 7, False), (0.035, 200, 7, False), (0.07, 300, 21, False),
            (1.0, 5, 5, True), (0.0, 9, 1, True)]


@pytest.mark.parametrize("F, dp, ad, record", EQUALITY)
def test_the_fraction_is_one_double_product(F, dp, ad, record):
    """A record exactly when the double product does not exceed AD -- what Python computes, and no division: 7 / 100 >= 0.07."""
    assert (ad >= F * dp) == record
    half = ad // 2
    for depth, alt in (([dp], [[0, ad, 0, 0, 0]]), ([dp - half, half], [[0, ad - half, 0, 0, 0], [0, half, 0, 0, 0]])):
        got = host.pileup_call_host(0, depth, alt, 1, F)
        assert got == _want("A", depth, alt, 1, F, 0) and (len(got) == 1) == record
        if record:
            assert got[0][3] == dp and got[0][6] + got[0][7] == ad


def test_positions_picked_by_hand():
    call = host.pileup_call_host
    assert call(0, [0, 0], [[0] * 5, [0] * 5], 0, 0.0) == []                                 # AD = 0 with C = 0
    assert call(2, [6, 0], [[0, 0, 0, 0, 6], [0] * 5], 0, 0.0) == []                         # `other` only: DP = 0
    three = call(0, [9, 9], [[0, 1, 2, 3, 0], [0, 3, 2, 1, 0]], 2, 0.01, 2)                   # all three alt bases at one position
    assert three == [(1, 0, 1, 18, 3, 3, 1, 3), (0, 0, 2, 18, 3, 3, 2, 2), (1, 0, 3, 18, 3, 3, 3, 1)]
    assert call(3, [5, 5], [[2, 0, 0, 0, 1], [0, 0, 0, 0, 0]], 2, 0.01, 1) == [(1, 3, 0, 9, 2, 5, 2, 0)]  # S = 1: one strand only
    assert call(3, [5, 5], [[2, 0, 0, 0, 1], [1, 0, 0, 0, 0]], 2, 0.01, 1) == [(0, 3, 0, 9, 2, 4, 2, 1)]
    assert call(3, [5, 5], [[2, 0, 0, 0, 1], [1, 0, 0, 0, 0]], 2, 0.01, 2) == [(1, 3, 0, 9, 2, 4, 2, 1)]
    big = 2 ** 40
    assert call(1, [3 * big, big], [[big, 0, 0, 0, 0], [0] * 5], 2, 0.25) == [(0, 1, 0, 4 * big, 2 * big, big, big, 0)]  # counts beyond 32 bits


def test_what_the_host_entry_refuses():
    L = nat.lib()
    d, a, out, n = np.zeros(2, np.uint64), np.zeros(10, np.uint64), np.zeros(18, np.uint64), C.c_uint32(7)
    ok = lambda *args: L.vs_pileup_call_host(*args, out.ctypes.data, C.byref(n))  # noqa: E731
    assert ok(0, 2, d.ctypes.data, a.ctypes.data, 2, 0.01, 0) == nat.VS_OK and n.value == 0
    assert ok(4, 2, d.ctypes.data, a.ctypes.data, 2, 0.01, 0) == nat.VS_E_ARG
    assert ok(0, 0, d.ctypes.data, a.ctypes.data, 2, 0.01, 0) == nat.VS_E_ARG
    assert ok(0, 3, d.ctypes.data, a.ctypes.data, 2, 0.01, 0) == nat.VS_E_ARG
    assert ok(0, 2, d.ctypes.data, a.ctypes.data, 2, float("nan"), 0) == nat.VS_E_ARG
    assert ok(0, 2, d.ctypes.data, a.ctypes.data, 2, -0.5, 0) == nat.VS_E_ARG
    assert ok(0, 1, d.ctypes.data, a.ctypes.data, 2, 0.01, 1) == nat.VS_E_ARG  # (a strand threshold needs two planes)
    assert ok(0, 2, None, a.ctypes.data, 2, 0.01, 0) == nat.VS_E_ARG
    assert L.vs_pileup_call_host(0, 2, d.ctypes.data, a.ctypes.data, 2, 0.01, 0, None, C.byref(n)) == nat.VS_E_ARG
    with pytest.raises(nat.NativeError):
        host.pileup_call_host(0, [1], [[0, 1, 0, 0, 0]], 2, 0.01, 1)


def test_one_plane_equals_variant_records_on_the_same_tables():
    rng = np.random.default_rng(41)
    ids = ["s", "t", "u"]
    seqs = ["".join(ACGT[i] for i in rng.integers(0, 4, size=n)) for n in (300, 3, 120)]
    offsets = np.array([0, 300, 300, 420])
    alt = rng.integers(0, 4, size=(420, 5)) * (rng.random((420, 5)) < 0.3)
    for n, seq in enumerate(seqs):
        for p in range(int(offsets[n + 1] - offsets[n])):
            alt[offsets[n] + p, ACGT.index(seq[p])] = 0
    depth = alt.sum(axis=1) + rng.integers(0, 300, size=420)
    for C_, F in ((2, 0.01), (0, 0.0), (1, 0.02), (3, 0.5)):
        want = node_depth.variant_records(ids, seqs, offsets, depth, alt, C_, F)
        called = node_depth.call_host(seqs, offsets, depth, alt, C_, F)
        got = node_depth.strand_records(ids, called)
        assert len(want) > (10 if F < 0.5 else 0) and [r[:6] for r in got] == want
        assert all(r[6][1] == r[6][3] == 0 and r[6][2] == r[5] and r[7] == "." for r in got)
