"""The launch plan of the depth pass (vstrains_amd/csrc/vs_depth_plan.h through ``vs_depth_plan``, a pure host function of
the library, which loads without a device).  Expected values are worked out here from what the header and DESIGN.md state:
160 KB of LDS per workgroup, sixteen wavefronts with 464 words of their own, four words of workgroup state, one uint32
counter per node."""
import pytest

from vstrains_amd import pe as host

LDS_WORDS = 160 * 1024 // 4
NODE_LIMIT = LDS_WORDS - 4 - 16 * 464


def test_the_node_limit_is_what_160_kb_of_lds_leave():
    p = host.depth_plan(1000, 55, 2 * 10 ** 6, 150)
    assert NODE_LIMIT == 33532
    assert p["node_limit"] == NODE_LIMIT and p["threads"] == 1024


@pytest.mark.parametrize("n_nodes,route", [(NODE_LIMIT - 1, "lds"), (NODE_LIMIT, "lds"), (NODE_LIMIT + 1, "global")])
def test_route_flips_above_the_node_limit(n_nodes, route):
    p = host.depth_plan(n_nodes, 55, 2 * 10 ** 6, 150)
    assert p["route"] == route
    if route == "lds":
        assert p["lds_nodes"] == n_nodes
        assert p["lds_bytes"] == 4 * ((n_nodes + 3) // 4 * 4 + 4 + 16 * 464) <= 160 * 1024
    else:
        assert p["lds_nodes"] == 0 and p["lds_bytes"] == 4 * (4 + 16 * 464)
    # every end belongs to exactly one workgroup
    assert (p["grid"] - 1) * p["ends_per_wg"] < 2 * 10 ** 6 <= p["grid"] * p["ends_per_wg"]


@pytest.mark.parametrize("max_len", [150, 250, 2 ** 20 - 1])
@pytest.mark.parametrize("n_ends", [1, 2 * 10 ** 6, 0xFFFFFFF0])
def test_an_lds_counter_cannot_wrap(max_len, n_ends):
    K = 56
    span = max_len - K + 1  # the windows of the longest end: the most one end adds to one counter, a repeat inside a node aside
    p = host.depth_plan(5000, 55, n_ends, max_len)
    assert p["wrap_ends"] * span < 2 ** 32 <= (p["wrap_ends"] + 1) * span
    assert 1 <= p["ends_per_wg"] <= p["wrap_ends"]
    assert p["ends_per_wg"] * span < 2 ** 32
    assert (p["grid"] - 1) * p["ends_per_wg"] < n_ends <= p["grid"] * p["ends_per_wg"]
    assert p["grid"] < 2 ** 31


def test_the_wrap_bound_binds_for_very_long_ends():
    p = host.depth_plan(5000, 55, 0xFFFFFFF0, 2 ** 20 - 1)
    assert p["ends_per_wg"] == p["wrap_ends"] == (2 ** 32 - 1) // (2 ** 20 - 1 - 55)


def test_small_blocks_take_one_workgroup_of_at_least_a_batch_per_wavefront():
    assert host.depth_plan(5000, 55, 1024, 150)["grid"] == 1
    p = host.depth_plan(5000, 55, 2 * 1024 + 1, 150)
    assert p["ends_per_wg"] == 1024 and p["grid"] == 3


@pytest.mark.parametrize("n_nodes,n_ends,max_len", [(5000, 0, 0), (5000, 0, 150), (0, 100, 150), (5000, 100, 55)])
def test_nothing_is_launched_without_a_window(n_nodes, n_ends, max_len):
    p = host.depth_plan(n_nodes, 55, n_ends, max_len)
    assert p["route"] == "none" and p["grid"] == 0


def test_sizes_beyond_the_build_are_refused():
    from vstrains_amd import _native as nat

    with pytest.raises(nat.NativeError):
        host.depth_plan(0x01FFFFFF, 55, 100, 150)
    with pytest.raises(nat.NativeError):
        host.depth_plan(5000, 55, 2 ** 32, 150)
