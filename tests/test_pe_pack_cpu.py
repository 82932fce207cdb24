"""The host packing of per-end node lists into the two hand-off layouts of a PE count (vstrains_amd/csrc/vs_pe_pack.h,
one pure function) on the CPU, through oracle/pack_check.cpp: unpacking gives the input back, offsets are quad-aligned, no
tile leaves its region, the tail padding is there, and everything the mapping kernel would never hand over is refused.
No device, no HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vstrains_amd import pe as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LC, LCAP, TAIL, FILL, E_RANGE = 16, 20, 16, 0xFFFFFFFF, -6


@pytest.fixture(scope="module")
def pack():
    path = os.path.join(ROOT, "oracle", "_build", "libvs_pack_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    lib = C.CDLL(path)
    lib.vs_pack_check_words.restype = C.c_uint64
    lib.vs_pack_check_words.argtypes = [C.c_uint64, C.c_int]
    lib.vs_pack_check.restype = C.c_int
    lib.vs_pack_check.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.vs_unpack_check.restype = None
    lib.vs_unpack_check.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]

    def run(n_nodes, lists, counts, ept, rows, list_ends=None):
        """-> (status, message, packed lists, packed counts, list_ends)"""
        lists = np.ascontiguousarray(lists, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        n_pairs = counts.size // 2
        if list_ends is None:
            list_ends = -(-n_pairs // (ept // 2)) * ept
        words = int(lib.vs_pack_check_words(list_ends, rows))
        out = np.full(words + 8, 0x5A5A5A5A, dtype=np.uint32)  # (eight guard words behind what the function may write)
        oc = np.full(list_ends + 8, 0x5A5A5A5A, dtype=np.uint32)
        msg = C.create_string_buffer(128)
        rc = lib.vs_pack_check(n_nodes, n_pairs, lists.ctypes.data, counts.ctypes.data, ept, list_ends, rows, out.ctypes.data, oc.ctypes.data, msg)
        assert (out[words:] == 0x5A5A5A5A).all() and (oc[list_ends:] == 0x5A5A5A5A).all()
        return rc, msg.value.decode(), out[:words], oc[:list_ends], list_ends

    run.unpack = lambda n_ends, out, oc, ept, list_ends, rows: _unpack(lib, n_ends, out, oc, ept, list_ends, rows)
    return run


def _unpack(lib, n_ends, out, oc, ept, list_ends, rows):
    lists = np.zeros((max(n_ends, 1), LCAP), dtype=np.uint32)
    counts = np.zeros(max(n_ends, 1), dtype=np.uint32)
    out, oc = np.ascontiguousarray(out), np.ascontiguousarray(oc)
    lib.vs_unpack_check(n_ends, out.ctypes.data, oc.ctypes.data, ept, list_ends, rows, lists.ctypes.data, counts.ctypes.data)
    return lists[:n_ends], counts[:n_ends]


def _random_pairs(rng, n_nodes, n_pairs):
    top = min(n_nodes, LCAP)
    return [tuple([int(x) for x in rng.choice(n_nodes, size=int(rng.integers(0, top + 1)), replace=False)] for _ in range(2)) for _ in range(n_pairs)]


@pytest.mark.parametrize("ept", [6, 32, 64, 128])
@pytest.mark.parametrize("rows", [0, 1])
def test_packing_round_trip_and_layout(pack, ept, rows):
    rng = np.random.default_rng(50 + ept + rows)
    for n_nodes, n_pairs in ((1, 5), (19, 40), (200, 1), (200, ept // 2), (200, ept // 2 + 1), (3000, 700)):
        lists, counts = host.list_block(_random_pairs(rng, n_nodes, n_pairs), ept)
        rc, msg, out, oc, list_ends = pack(n_nodes, lists, counts, ept, rows)
        assert rc == 0, msg
        back, bc = pack.unpack(counts.size, out, oc, ept, list_ends, rows)
        assert np.array_equal(bc, counts) and np.array_equal(back, lists)
        assert (out[-TAIL:] == FILL).all() and out.size == list_ends * (LC + 4 if rows else LC) + TAIL
        assert not oc[counts.size:].any()  # the unused ends of the last tile
        owned = np.zeros(out.size, dtype=np.int32)
        for e in range(counts.size):
            n = int(counts[e])
            if rows:
                assert oc[e] == n
                owned[e * LC: e * LC + min(n, LC)] += 1
                owned[list_ends * LC + 4 * e: list_ends * LC + 4 * e + max(n - LC, 0)] += 1
            elif n == 0:
                assert oc[e] == 0
            else:
                assert oc[e] & 0xFF == n and oc[e] >> 8 < ept * LC // 4
                first = (e // ept) * ept * LC + 4 * (int(oc[e]) >> 8)  # quad-aligned by construction of the count word
                last = first + 4 * ((n + 3) // 4)
                assert last <= (e // ept + 1) * ept * LC  # the list and its padding stay inside the tile's region
                owned[first:last] += 1
                assert (out[first + n: last] == FILL).all()  # (the padding of the list's last quad)
        assert owned.max(initial=0) <= 1  # no two lists share a word
        assert (out[owned == 0] == FILL).all()  # what no list owns holds the fill word


def test_packing_refuses_what_the_mapping_kernel_never_hands_over(pack):
    rng = np.random.default_rng(77)
    n_nodes, ept = 500, 64
    lists, counts = host.list_block(_random_pairs(rng, n_nodes, 300), ept)
    for rows in (0, 1):
        assert pack(n_nodes, lists, counts, ept, rows)[0] == 0

        def refused(l2, c2, word, **kw):
            rc, msg = pack(n_nodes, l2, c2, ept, rows, **kw)[:2]
            assert rc == E_RANGE and word in msg, (rc, msg)

        e = int(np.nonzero(counts >= 3)[0][5])
        c2 = counts.copy(); c2[e] = 21
        refused(lists, c2, "at most 20")
        c2[e] = 0xFFFFFFFF
        refused(lists, c2, "at most 20")
        for bad in (n_nodes, n_nodes + 1, 0xFFFFFFFF):
            l2 = lists.copy(); l2[e, 1] = bad
            refused(l2, counts, "lists node")
        l2 = lists.copy(); l2[e, 2] = l2[e, 0]
        refused(l2, counts, "twice")
        # a tile whose 64 ends hold 17 nodes each: five quads per end where the region has four
        l2, c2 = lists.copy(), counts.copy()
        l2[ept: 2 * ept, :17] = np.arange(17)
        c2[ept: 2 * ept] = 17
        refused(l2, c2, "tile 1")
        # end slots that do not hold the block, or are no whole tiles
        refused(lists, counts, "end slots", list_ends=counts.size // ept * ept - ept)
        refused(lists, counts, "end slots", list_ends=counts.size + 1 + ept)
    # the fullest tile there is: 51 ends of 17..20 nodes and the rest empty is accepted, one more quad is not
    full = [list(range(20))] * 51 + [[0]] + [[]] * 12
    lists = np.full((64, LCAP), FILL, dtype=np.uint32)
    counts = np.array([len(x) for x in full], dtype=np.uint32)
    for e, row in enumerate(full):
        lists[e, : len(row)] = row
    assert sum((len(x) + 3) // 4 for x in full) == 64 * LC // 4
    assert pack(n_nodes, lists, counts, 64, 0)[0] == 0 and pack(n_nodes, lists, counts, 64, 1)[0] == 0
    counts[53] = 1; lists[53, 0] = 3
    assert pack(n_nodes, lists, counts, 64, 0)[0] == E_RANGE and pack(n_nodes, lists, counts, 64, 1)[0] == E_RANGE


def test_list_block_closes_a_tile_early_with_empty_pairs():
    pairs = [(list(range(20)), list(range(20)))] * 60
    lists, counts = host.list_block(pairs, 64)
    # ten quads per pair, 256 per tile: 25 pairs, then seven empty ones
    assert counts.size == 2 * (32 + 32 + 10)
    per_tile = counts[:128].reshape(2, 64)
    assert (per_tile[:, :50] == 20).all() and not per_tile[:, 50:].any() and (counts[128:] == 20).all()
    lists, counts = host.list_block([([1], [2])] * 40, 64)
    assert counts.size == 80 and (counts == 1).all()
