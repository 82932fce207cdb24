"""The diagonal walk of the base pileup (csrc/vs_pileup_core.h), the code k_node_pileup runs, through its host entry
``vs_pileup_scan_host`` against tests/pileup_model.py: no device.  For a read laid on a strand every maximal run of K agreeing
positions is a match (a, qa) the kernel would hold; for each of them the owner flag (is it the leftmost run of its diagonal),
the overlap and the count of non-agreeing positions are compared."""
import ctypes as C

import numpy as np
import pytest

import pileup_model as model
from node_depth_cases import dna
from pileup_cases import sub, with_n
from vstrains_amd import _native as nat

KS_PLUS_1 = (22, 56, 128)
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def pack(text: str):
    """(words, mask): 2 bits a base, 16 a word, the first base lowest; the mask 0b11 at a byte outside ACGT (its word: code
    0); three zero words behind the last."""
    n_words = (len(text) + 15) // 16 + 3
    words, mask = np.zeros(n_words, dtype=np.uint32), np.zeros(n_words, dtype=np.uint32)
    for i, ch in enumerate(text):
        if ch in _CODE:
            words[i >> 4] |= np.uint32(_CODE[ch] << (2 * (i & 15)))
        else:
            mask[i >> 4] |= np.uint32(3 << (2 * (i & 15)))
    return words, mask


def scan(read: str, strand: str, a: int, qa: int, K: int, use_mask=None):
    rw, rm = pack(read)
    tw, _ = pack(strand)
    masked = rm.any() if use_mask is None else use_mask
    out = (C.c_uint32 * 4)()
    rc = nat.lib().vs_pileup_scan_host(rw.ctypes.data, rm.ctypes.data if masked else None, tw.ctypes.data, len(read), len(strand), a, qa, K, out)
    assert rc == nat.VS_OK
    return tuple(int(v) for v in out)


def runs(agree, K):
    """[(first index, length)] of the maximal runs of K or more."""
    out, start = [], None
    for i, ok in enumerate(list(agree) + [False]):
        if ok and start is None:
            start = i
        if not ok and start is not None:
            if i - start >= K:
                out.append((start, i - start))
            start = None
    return out


def check(read: str, strand: str, d: int, K: int, use_mask=None) -> int:
    """Every match on diagonal ``d`` through the host entry against the model; -> how many there were."""
    x_lo, agree = model.agreement(read, strand, d)
    x_hi = x_lo + len(agree)
    assert (x_lo, x_hi) == model.overlap(len(read), len(strand), d)
    miss = sum(1 for ok in agree if not ok)
    found = runs(agree, K)
    for i, (start, length) in enumerate(found):
        a = x_lo + start
        assert scan(read, strand, a, a + d, K, use_mask) == (1 if i == 0 else 0, x_lo, x_hi, miss), (len(read), d, a, K)
    return len(found)


@pytest.fixture(scope="module")
def strand():
    return dna(np.random.default_rng(99), 900)


@pytest.mark.parametrize("K", KS_PLUS_1)
def test_every_overlap_length_left_and_right_of_the_anchor(strand, K):
    """An anchor of exactly K bases with 1 .. 130 more bases of overlap on one side, the base next to the anchor
    substituted: a flank of K or more is an anchor itself, and then the left one owns.  At K = 128 the walk spans four windows
    and the boundaries 32, 64, 96, 128 are crossed one base at a time."""
    p = 300
    for n in range(1, 131):
        left = sub(strand[p - n:p + K], n - 1)
        assert check(left, strand, p - n, K) == (2 if n - 1 >= K else 1)
        right = sub(strand[p:p + K + n], K)
        assert check(right, strand, p, K) == (2 if n - 1 >= K else 1)


@pytest.mark.parametrize("K", KS_PLUS_1)
def test_overlaps_clipped_by_the_strands_start_and_end(strand, K):
    """The read overhangs the strand by 1 .. 40 bases: a negative diagonal on the left, and the text ending under the read."""
    junk = dna(np.random.default_rng(5), 40)
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 40):
        assert check(junk[:n] + sub(strand[:K + 37], K + 1), strand, -n, K) == (2 if 35 >= K else 1)  # (K + 1 bases, a mismatch, 35 bases)
        tail = strand[len(strand) - (K + 37):]
        assert check(sub(tail, 3) + junk[:n], strand, len(strand) - (K + 37), K) == 1


@pytest.mark.parametrize("K", KS_PLUS_1)
def test_a_single_mismatch_at_every_position_and_pairs_of_them(strand, K):
    p, n = 211, K + 70
    read = strand[p:p + n]
    assert check(read, strand, p, K) == 1
    seen = set()
    for i in range(n):
        seen.add(check(sub(read, i), strand, p, K))
    assert seen == ({1, 2} if 2 * K + 1 <= n else {0, 1})  # (two anchors beside one mismatch only when 2K + 1 bases fit the read)
    rng = np.random.default_rng(K)
    for _ in range(300):
        i, j = sorted(int(v) for v in rng.choice(n, size=2, replace=False))
        check(sub(read, i, j), strand, p, K)
    long_read = strand[p:p + 3 * K + 2]
    for i, j in ((K, 2 * K + 1), (K - 1, 2 * K + 1), (K, 2 * K), (0, K + 1), (K, 3 * K + 1)):
        check(sub(long_read, i, j), strand, p, K)
    assert check(sub(long_read, K, 2 * K + 1), strand, p, K) == 3


@pytest.mark.parametrize("K", KS_PLUS_1)
def test_runs_of_exactly_K_minus_1_and_K_to_the_left(strand, K):
    p = 123
    for extra in (0, 1, 31, 32, 33):  # (bases of the overlap left of the run, the last of them one more mismatch)
        further = 1 if extra - 1 >= K else 0  # (at K = 22 the bases left of that mismatch are an anchor themselves)
        for run, n_matches in ((K - 1, 1 + further), (K, 2 + further)):
            at = [extra + run] + ([extra - 1] if extra else [])
            read = sub(strand[p:p + extra + run + 1 + K + 5], *at)
            x_lo, agree = model.agreement(read, strand, p)
            found = runs(agree, K)
            assert len(found) == n_matches
            a = found[-1][0]  # the match right of the run
            assert a == extra + run + 1
            assert scan(read, strand, a, a + p, K)[0] == (1 if run == K - 1 and not further else 0)
            check(read, strand, p, K)


@pytest.mark.parametrize("K", KS_PLUS_1)
def test_masked_bytes_do_not_agree_and_break_a_run(strand, K):
    """A byte outside ACGT is packed as code 0 under a mask: over an A of the strand only the mask tells it from a match."""
    p = 150
    where = [i for i in range(p + K + 2, p + K + 60) if strand[i] == "A"][:3]
    assert len(where) == 3
    read = strand[p:p + 2 * K + 70]
    masked = with_n(read, *[i - p for i in where])
    assert check(masked, strand, p, K) >= 1
    assert scan(masked, strand, 0, p, K)[3] == 3
    assert scan(masked, strand, 0, p, K, use_mask=False)[3] == 0  # (without the mask the three would pass for A)
    left_n = with_n(read, K)  # a run of exactly K left of an N: the match behind it is not the owner
    assert scan(left_n, strand, K + 1, p + K + 1, K)[0] == 0
    assert scan(with_n(read, K - 1), strand, K, p + K, K)[0] == 1
    check(left_n, strand, p, K)


def test_arguments_outside_their_range_are_refused():
    w, _ = pack("ACGT" * 8)
    out = (C.c_uint32 * 4)()
    lib = nat.lib()
    assert lib.vs_pileup_scan_host(None, None, w.ctypes.data, 32, 32, 0, 0, 4, out) == nat.VS_E_ARG
    assert lib.vs_pileup_scan_host(w.ctypes.data, None, w.ctypes.data, 32, 32, 32, 0, 4, out) == nat.VS_E_ARG
    assert lib.vs_pileup_scan_host(w.ctypes.data, None, w.ctypes.data, 32, 32, 0, 0, 0, out) == nat.VS_E_ARG
