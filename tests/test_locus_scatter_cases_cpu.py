"""tests/locus_scatter_cases.py without a device: its constants are the kernel's, its sizes put a chunk's end where the
docstring there says, a tiled block holds the pairs of the inputs it repeats, and the plan cuts the scatter into the
launches the device tests count on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import locus_scatter_cases as cases
import test_pe_counters_gpu as base
from vstrains_amd.pe import encode_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    c = cases.constants()
    assert c["wgs"] == cases.WGS and c["tpb"] == cases.TPB
    assert c["u"] in (2, 4, 8) and cases.ROW == 1024 * c["u"]


def test_turn_sizes_put_the_chunk_round_a_whole_turn():
    below_last, whole, above, below = (cases.shape(n) for n in cases.TURN_SIZES)
    # the issue's first size: whole turns in 255 workgroups, the last one 255 pairs short
    assert below_last["chunk"] == cases.ROW and below_last["last_wg_pairs"] == cases.ROW - 255 and below_last["empty_wgs"] == 0
    assert whole == dict(chunk=cases.ROW, last_wg_pairs=0, empty_wgs=0, turns=1, rows_last_turn=cases.U, lanes_last_row=1024)
    # one pair more: a second turn with one live lane in its first row; the last workgroup stops 254 pairs short of the first turn's end
    assert above["chunk"] == cases.ROW + 1 and above["turns"] == 2 and above["rows_last_turn"] == 1 and above["lanes_last_row"] == 1
    assert above["last_wg_pairs"] == cases.ROW - 254
    # one below: one turn, its last row one lane short
    assert below["chunk"] == cases.ROW - 1 and below["turns"] == 1 and below["rows_last_turn"] == cases.U and below["lanes_last_row"] == 1023
    assert below["last_wg_pairs"] == 0 and below["empty_wgs"] == 0
    assert max(cases.TURN_SIZES) < 1 << 24  # (a few seconds a test)


def test_small_sizes_leave_most_lanes_idle():
    got = [cases.shape(n) for n in cases.SMALL_SIZES]
    assert [g["chunk"] for g in got] == [16, 17, 18, 19]
    assert got[1]["empty_wgs"] == 15 and got[1]["last_wg_pairs"] == 0  # 4 097: workgroups 241 .. 255 empty
    # 4 096: no workgroup empty or short; 4 353 and 4 609: a short workgroup (15 and 11 pairs) in front of the empty ones
    assert [(g["empty_wgs"], g["last_wg_pairs"]) for g in (got[0], got[2], got[3])] == [(0, 0), (14, 15), (13, 11)]
    assert all(g["turns"] == 1 and g["rows_last_turn"] == 1 for g in got)
    assert all(n >= 4096 for n in cases.SMALL_SIZES + cases.CHAIN_SIZES)  # (below that no sort runs)


def test_tile_repeats_the_inputs():
    _, _, fwd, rve, _ = base._locus_inputs("small", 301, 5)
    for n_pairs in (1, 300, 301, 302, 1000):
        data, off = cases.tile(fwd, rve, n_pairs)
        want, want_off = encode_seqs([x for p in range(n_pairs) for x in (fwd[p % 301], rve[p % 301])])
        assert np.array_equal(off, want_off) and np.array_equal(data, want[: max(int(want_off[-1]), 1)])


def test_keys_allowed():
    table = cases.allowed_table([{3}, {5, 9}, {0}])
    assert table.shape == (3, 2)
    keys = np.array([3, 9, 0, 3, 5, 1, 4, 5], dtype=np.uint32)
    assert cases.keys_allowed(keys, table).tolist() == [True, True, True, True, True, False, False, True]


# ---- the launch rule (csrc/vs_pe_plan.h), through tests/locus_scatter_plan_check.cpp ---------------------------------------------
@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("locus_scatter") / "locus_scatter_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "locus_scatter_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        head, tail = line.split("|")
        _, n_nodes, n_pairs, hook = head.split()
        keys, per_pass, scatter_keys, launches = (int(x) for x in tail.split())
        out[(int(n_nodes), int(n_pairs), int(hook))] = dict(keys=keys, per_pass=per_pass, scatter_keys=scatter_keys, launches=launches)
    return out


def test_small_blocks_are_placed_as_before(planned):
    """Up to LOCUS_SCATTER_PAIRS pairs: one launch per pass of the sort, as many keys as the pass has."""
    limit = 2621440
    for (n_nodes, n_pairs, hook), p in planned.items():
        if hook == 0 and n_pairs <= limit:
            assert p["scatter_keys"] == p["per_pass"] == min(p["keys"], 36864) and p["launches"] == -(-p["keys"] // 36864), (n_nodes, n_pairs, p)


def test_large_blocks_are_placed_in_key_ranges(planned):
    limit = 2621440
    assert planned[(5039, limit + 1, 0)]["launches"] == 2 and planned[(5039, 2 * limit + 1, 0)]["launches"] == 3
    for n_pairs in (10000000, 100000000):  # four launches at most
        assert planned[(5039, n_pairs, 0)] == dict(keys=5041, per_pass=5041, scatter_keys=1261, launches=4)
        assert planned[(54000, n_pairs, 0)]["launches"] == 4 and planned[(147000, n_pairs, 0)]["launches"] == 4
        assert planned[(1, n_pairs, 0)] == dict(keys=3, per_pass=3, scatter_keys=1, launches=3)
    for (n_nodes, n_pairs, hook), p in planned.items():
        assert p["launches"] >= -(-p["keys"] // 36864) and p["launches"] <= max(4, -(-p["keys"] // 36864))


def test_the_hook_cuts_small_blocks(planned):
    """VS_LOCUS_SCATTER as tests/test_locus_scatter_gpu.py sets it: the launches it asks the plan for."""
    for n_nodes in (600, 40000):
        assert [planned[(n_nodes, 4097, hook)]["launches"] for hook in (1, 1024, 2500)] == [4, 4, 2]
        assert planned[(n_nodes, 2097153, 1048577)]["launches"] == 2
    assert planned[(40000, 4097, 2500)]["scatter_keys"] == 20001  # the second launch starts inside the sort's first pass of 36 864 keys
