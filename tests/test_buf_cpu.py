"""The owning buffer every device and pinned allocation of the library goes through (vstrains_amd/csrc/vs_buf.h), on the
CPU: oracle/buf_check.cpp instantiates the template with an allocator that counts its live blocks and can refuse the
next allocation.  No device, no HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, CAP, ERR, FRESH, LIVE, PEAK, LAST_ALLOC, BAD_FREES = range(8)
OK, OOM = 0, 1


@pytest.fixture(scope="module")
def run():
    path = os.path.join(ROOT, "oracle", "_build", "libvs_buf_check.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    lib = C.CDLL(path)
    lib.vs_buf_check.restype = C.c_int
    lib.vs_buf_check.argtypes = [C.c_int, C.c_void_p]

    def scenario(which):
        out = np.zeros((16, 8), dtype=np.uint64)
        n = lib.vs_buf_check(which, out.ctypes.data)
        assert n > 0
        obs = [[int(x) for x in row] for row in out[:n]]
        assert all(o[BAD_FREES] == 0 for o in obs), "a pointer was freed twice, or one the allocator never gave out"
        return obs

    return scenario


def assert_empty_invariant(obs):
    for o in obs:
        assert (o[PTR] == 0) == (o[CAP] == 0), o


def test_failed_reserve_on_empty_buffer(run):
    failed, again = run(0)
    assert_empty_invariant([failed, again])
    assert (failed[PTR], failed[CAP], failed[ERR], failed[FRESH], failed[LIVE]) == (0, 0, OOM, 0, 0)
    assert (again[PTR], again[CAP], again[ERR], again[FRESH], again[LIVE]) == (1, 1000, OK, 1, 1)


def test_failed_reserve_on_held_buffer_leaves_it_empty(run):
    """The sequence a counting context goes through when a block is too large for the device and the caller answers
    with a smaller one: nothing may be left that passes a capacity test with a null pointer."""
    first, failed, smaller = run(1)
    assert_empty_invariant([first, failed, smaller])
    assert (first[PTR], first[CAP], first[ERR], first[FRESH], first[LIVE]) == (1, 1000, OK, 1, 1)
    assert (failed[PTR], failed[CAP], failed[ERR], failed[FRESH], failed[LIVE]) == (0, 0, OOM, 0, 0)
    assert (smaller[PTR], smaller[CAP], smaller[ERR], smaller[FRESH], smaller[LIVE]) == (1, 500, OK, 1, 1)
    assert smaller[LAST_ALLOC] == 500


def test_out_pointer_of_a_failed_allocation_does_not_survive(run):
    poisoned, held, untouched = run(2)
    assert_empty_invariant([poisoned, held, untouched])
    assert (poisoned[PTR], poisoned[CAP], poisoned[ERR], poisoned[LIVE]) == (0, 0, OOM, 0)
    assert (held[PTR], held[CAP], held[ERR]) == (1, 64, OK)
    assert (untouched[PTR], untouched[CAP], untouched[ERR], untouched[LIVE]) == (0, 0, OOM, 0)


def test_reserve_is_grow_only_and_never_holds_two_blocks(run):
    first, below, at, above, exact = run(3)
    assert_empty_invariant([first, below, at, above, exact])
    assert (first[CAP], first[FRESH], first[LAST_ALLOC]) == (1500, 1, 1500)  # the slack asked for, not the need
    assert below[PTR] == 1, "a reserve below the capacity replaced the block"
    assert (below[CAP], below[ERR], below[FRESH], below[LAST_ALLOC]) == (1500, OK, 0, 1500)
    assert (at[CAP], at[FRESH]) == (1500, 0)
    assert (above[PTR], above[CAP], above[ERR], above[FRESH], above[LAST_ALLOC]) == (1, 3000, OK, 1, 3000)
    assert (exact[PTR], exact[CAP], exact[ERR], exact[LAST_ALLOC]) == (1, 4000, OK, 4000)
    for o in (first, below, at, above, exact):
        assert o[LIVE] == 1 and o[PEAK] == 1, "old and new block were held at once"


def test_move_release_and_lifetime(run):
    moved_from, moved_to, assigned_from, assigned_to, released, adopted, other, end = run(4)
    assert_empty_invariant([moved_from, moved_to, assigned_from, assigned_to, released, adopted, other])
    assert (moved_from[PTR], moved_from[CAP]) == (0, 0) and (moved_to[PTR], moved_to[CAP], moved_to[LIVE]) == (1, 100, 1)
    assert (assigned_from[PTR], assigned_from[CAP]) == (0, 0)
    assert (assigned_to[PTR], assigned_to[CAP], assigned_to[LIVE]) == (1, 100, 1)  # the target's own block is gone
    assert (released[PTR], released[CAP], released[LIVE]) == (0, 0, 1)  # nothing to free, the block lives on
    assert (adopted[PTR], adopted[CAP], adopted[LIVE]) == (1, 100, 1)
    assert (other[CAP], other[LIVE]) == (300, 2)
    allocs, frees = end[0], end[1]
    assert end[LIVE] == 0 and allocs == frees == 3
