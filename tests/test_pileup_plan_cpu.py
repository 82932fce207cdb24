"""``vs_pileup_plan`` (csrc/vs_pileup_plan.h), a pure host function: the weight of a block, when a fold is due and what is
refused, each expected value worked out from the header's statement -- one end adds at most 2 * len_e to one slot (one
diagonal per read offset through a position, two strands), a slot must stay below 2^32 between two folds.  No device."""
import pytest

from vstrains_amd import _native as nat
from vstrains_amd import pe as host

B = 2 ** 32


def test_the_weight_is_ends_times_two_times_the_longest_end():
    p = host.pileup_plan(10, 21, 1000, 150)
    assert p["launch"] and p["weight"] == 1000 * 2 * 150 and p["pending"] == p["weight"] and not p["fold_first"]
    # (the profile's weight counts windows, the pileup's bases: the same block weighs more here)
    assert host.cover_plan(10, 21, 1000, 150)["weight"] == 1000 * 2 * (150 - 22 + 1)
    assert p["threads"] == 1024 and p["lds_bytes"] == 4 * (4 + 16 * 324)


def test_the_launch_shares_the_ends_among_two_workgroups_a_compute_unit():
    p = host.pileup_plan(10, 21, 2 ** 20, 150, n_cu=256)
    assert p["ends_per_wg"] == 2 ** 20 // 512 and p["grid"] == 512
    p = host.pileup_plan(10, 21, 100, 150, n_cu=256)
    assert p["ends_per_wg"] == 1024 and p["grid"] == 1  # (a share is at least one batch of 64 ends per wavefront)
    p = host.pileup_plan(10, 21, 1025, 150, n_cu=1)
    assert p["ends_per_wg"] == 1024 and p["grid"] == 2


def test_no_fold_below_the_bound_and_a_fold_at_it():
    w = 1000 * 2 * 150
    # pending + weight one short of the bound: no fold; at the bound: a fold first, and only this block pends
    p = host.pileup_plan(10, 21, 1000, 150, pending=B - w - 1)
    assert not p["fold_first"] and p["pending"] == B - 1
    p = host.pileup_plan(10, 21, 1000, 150, pending=B - w)
    assert p["fold_first"] and p["pending"] == w
    # a bound of its own; nothing pending: nothing to fold, whatever the bound
    assert host.pileup_plan(10, 21, 1000, 150, pending=w, bound=2 * w)["fold_first"]
    assert not host.pileup_plan(10, 21, 1000, 150, pending=w, bound=2 * w + 1)["fold_first"]
    p = host.pileup_plan(10, 21, 1000, 150, pending=0, bound=1)
    assert not p["fold_first"] and p["pending"] == w
    assert host.pileup_plan(10, 21, 1000, 150, pending=w, bound=1)["fold_first"]


def test_a_block_without_an_anchor_neither_launches_nor_weighs():
    for n_ends, max_len, n_nodes in ((1000, 21, 10), (0, 150, 10), (1000, 150, 0)):
        p = host.pileup_plan(n_nodes, 21, n_ends, max_len, pending=77)
        assert not p["launch"] and p["weight"] == 0 and p["pending"] == 77 and not p["fold_first"] and p["grid"] == 0
    assert host.pileup_plan(10, 21, 1000, 22)["launch"]  # (an end of exactly K bases holds one)


def test_a_block_that_could_put_two_to_the_32_on_one_position_is_refused():
    # n_ends * 2 * max_len < 2^32 is the most one launch may weigh
    most = (B - 1) // (2 * 150)
    assert host.pileup_plan(10, 21, most, 150)["weight"] == most * 300 < B
    with pytest.raises(nat.NativeError) as e:
        host.pileup_plan(10, 21, most + 1, 150)
    assert e.value.code == nat.VS_E_RANGE
    # 2^24 - 1 bases (the longest end a block holds): 128 ends fit, 129 do not
    assert host.pileup_plan(10, 21, 128, 2 ** 24 - 1)["weight"] == 128 * 2 * (2 ** 24 - 1)
    with pytest.raises(nat.NativeError):
        host.pileup_plan(10, 21, 129, 2 ** 24 - 1)


@pytest.mark.parametrize("kw", [dict(n_nodes=2 ** 25 - 1), dict(n_ends=2 ** 32 - 15), dict(bound=B + 1), dict(pending=B)])
def test_every_other_range_case(kw):
    args = dict(n_nodes=10, ksize=21, n_ends=1000, max_len=150, pending=0, bound=B)
    args.update(kw)
    with pytest.raises(nat.NativeError) as e:
        host.pileup_plan(**args)
    assert e.value.code == nat.VS_E_RANGE


def test_the_values_next_to_every_range_case_pass():
    assert host.pileup_plan(2 ** 25 - 2, 21, 1000, 150)["launch"]
    assert host.pileup_plan(10, 21, 1000, 150, pending=B - 1)["fold_first"]
    assert host.pileup_plan(10, 21, 1000, 150, bound=B)["launch"]
