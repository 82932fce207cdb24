"""The host side of the site-pair pass, held to plain Python without a device: the reduction the kernel runs on one fragment's
list (``vs_site_pairs_frag_host``, csrc/vs_site_pairs_core.h) against tests/site_pairs_model.py, the rows of the cell table
(``vs_site_pairs_rows_host``) against a double loop, and the launch plan (``vs_site_pairs_plan``)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import site_pairs_model as model
from vstrains_amd import _native as nat
from vstrains_amd import pe as host


def frag_host(entries):
    raw = np.array(entries, dtype=np.uint32)
    kept = np.full(32, 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint32)
    rc = nat.lib().vs_site_pairs_frag_host(raw.ctypes.data, len(entries), kept.ctypes.data, out.ctypes.data)
    assert rc == nat.VS_OK
    return kept[:int(out[0])].tolist(), int(out[1])


def frag_model(entries):
    kept, bad = model.reduce_fragment([((0, int(e) >> 3), int(e) & 7) for e in entries])
    return [(s[1] << 3) | c for s, c in kept], bad


def test_the_reduction_equals_the_models_on_seeded_random_lists():
    rng = np.random.default_rng(20261021)
    discordant = overlapping = 0
    for i in range(4000):
        n = int(rng.integers(0, 33))
        n_sites = int(rng.integers(1, 2 + n))  # few sites: many repeats; many sites: few
        far = int(rng.integers(0, 2 ** 29 - n_sites))  # (a site number has 29 bits)
        cols = 5 if i % 2 else 2
        entries = [((far + int(rng.integers(0, n_sites))) << 3) | int(rng.integers(0, cols)) for _ in range(n)]
        want = frag_model(entries)
        assert frag_host(entries) == want
        assert frag_host([entries[j] for j in rng.permutation(n)]) == want
        discordant += want[1]
        overlapping += len(want[0]) < len(set(e >> 3 for e in entries)) or len(entries) > len(set(entries))
    assert discordant > 1000 and overlapping > 1000


def test_every_permutation_of_a_list_gives_the_same_answer():
    entries = [(7 << 3) | 1, (7 << 3) | 1, (3 << 3) | 0, (3 << 3) | 2, (9 << 3) | 4, ((2 ** 29 - 1) << 3) | 3]
    want = ([(7 << 3) | 1, (9 << 3) | 4, ((2 ** 29 - 1) << 3) | 3], 1)
    assert frag_model(entries) == want
    for perm in itertools.permutations(entries):
        assert frag_host(list(perm)) == want


def test_the_reduction_at_its_edges():
    assert frag_host([]) == ([], 0)
    assert frag_host([5 << 3]) == ([5 << 3], 0)
    full = [(i << 3) | (i % 5) for i in range(32)]
    assert frag_host(full[::-1]) == (full, 0)
    assert frag_host([(1 << 3) | (i % 2) for i in range(32)]) == ([], 1)          # 32 observations of one site, two columns
    assert frag_host([(i // 2 << 3) | (i % 2) for i in range(32)]) == ([], 16)    # sixteen discordant sites
    assert frag_host([(4 << 3) | 3] * 32) == ([(4 << 3) | 3], 0)
    kept, out = np.zeros(32, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    raw = np.zeros(33, dtype=np.uint32)
    assert nat.lib().vs_site_pairs_frag_host(raw.ctypes.data, 33, kept.ctypes.data, out.ctypes.data) == nat.VS_E_ARG


def rows_by_hand(seg, pos, span):
    first, total = [], 0
    for i in range(len(seg)):
        first.append(total)
        total += sum(1 for j in range(i + 1, len(seg)) if seg[j] == seg[i] and pos[j] - pos[i] <= span)
    return first + [total], total


@pytest.mark.parametrize("span", [0, 1, 7, 50, 10 ** 6])
def test_the_rows_equal_a_plain_double_loop(span):
    rng = np.random.default_rng(span + 3)
    for _ in range(30):
        sites = sorted(set((int(rng.integers(0, 6)), int(rng.integers(0, 120))) for _ in range(int(rng.integers(0, 80)))))
        seg, pos = [s[0] for s in sites], [s[1] for s in sites]
        row_first, total = host.site_pairs_rows(seg, pos, span)
        want = rows_by_hand(seg, pos, span)
        assert row_first.dtype == np.uint32 and (row_first.tolist(), total) == want
        # the partners of a site are contiguous behind it: the cell of (s, t) is row_first[s] + (t - s - 1)
        for i in range(len(sites)):
            n = int(row_first[i + 1]) - int(row_first[i])
            assert all(seg[j] == seg[i] and pos[j] - pos[i] <= span for j in range(i + 1, i + 1 + n))
            assert i + 1 + n == len(sites) or seg[i + 1 + n] != seg[i] or pos[i + 1 + n] - pos[i] > span


def test_rows_that_cannot_be():
    assert host.site_pairs_rows([], [], 1000)[1] == 0
    for seg, pos in (([0, 0], [5, 5]), ([0, 0], [5, 4]), ([1, 0], [0, 0])):  # a site twice, descending positions, descending segments
        with pytest.raises(nat.NativeError):
            host.site_pairs_rows(seg, pos, 10)
    # 2^32 cells: 92 683 sites of one segment all within the span make 92 683 * 92 682 / 2 = 4 295 022 903 pairs
    n = 92683
    with pytest.raises(nat.NativeError, match="lower the span") as e:
        host.site_pairs_rows(np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), n)
    assert e.value.code == nat.VS_E_RANGE
    row_first, total = host.site_pairs_rows(np.zeros(n - 1, dtype=np.uint32), np.arange(n - 1, dtype=np.uint32), n)  # one site fewer fits
    assert total == (n - 1) * (n - 2) // 2 < 2 ** 32 and int(row_first[-1]) == total
    row_first, total = host.site_pairs_rows(np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), 1000)  # ... and so does a lower span
    assert total == 1000 * (n - 1000) + 1000 * 999 // 2
    # 2^29 sites: refused before the lists are looked at (the arrays need not be that long for the refusal)
    total = C.c_uint64(0)
    one = np.zeros(2, dtype=np.uint32)
    assert nat.lib().vs_site_pairs_rows_host(one.ctypes.data, one.ctypes.data, 2 ** 29, 0, one.ctypes.data, C.byref(total)) == nat.VS_E_RANGE


@pytest.mark.parametrize("n_cu", [1, 256, 304])
@pytest.mark.parametrize("times", [1, 3])
def test_the_plan_never_cuts_a_pair(n_cu, times):
    centre = 2 * n_cu * 1024 * times
    for n_ends in range(centre - 8, centre + 10, 2):
        for max_len in (150, 22):
            plan = host.site_pairs_plan(100, 21, n_ends, max_len, n_cu)
            assert plan["launch"] and plan["ends_per_wg"] % 64 == 0 and plan["ends_per_wg"] >= 64 * plan["threads"] // 64
            assert plan["grid"] * plan["ends_per_wg"] >= n_ends > (plan["grid"] - 1) * plan["ends_per_wg"]
            assert plan["threads"] == 512 and plan["lds_bytes"] == 4 * (4 + 8 * (324 + 32 * 33))
    # the pileup's own quotient is odd somewhere in that range, which is what the multiple of 64 is there for
    odd = [n for n in range(centre + 2, centre + 8 * n_cu, 2) if host.pileup_plan(100, 21, n, 150, n_cu)["ends_per_wg"] % 2]
    assert odd and all(host.site_pairs_plan(100, 21, n, 150, n_cu)["ends_per_wg"] % 64 == 0 for n in odd[:50])


def test_plans_that_cannot_be():
    for n_ends in (1, 3, 2 * 256 * 1024 + 1):
        with pytest.raises(nat.NativeError, match="odd") as e:
            host.site_pairs_plan(100, 21, n_ends, 150)
        assert e.value.code == nat.VS_E_ARG
    for n_nodes, n_ends in ((2 ** 25 - 1, 64), (100, 2 ** 32)):
        with pytest.raises(nat.NativeError) as e:
            host.site_pairs_plan(n_nodes, 21, n_ends, 150)
        assert e.value.code == nat.VS_E_RANGE
    assert not host.site_pairs_plan(100, 21, 0, 150)["launch"]
    assert not host.site_pairs_plan(100, 21, 64, 21)["launch"]  # no end holds k + 1 bases
    small = host.site_pairs_plan(100, 21, 2, 150)
    assert small["launch"] and small["grid"] == 1 and small["ends_per_wg"] == 512
