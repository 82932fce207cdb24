"""The work units of k_pe_accumulate (vstrains_amd/csrc/vs_acc_tasks.h: one task per matrix row, short rows folded with
their mirror rows, the batch cut) on the CPU: tests/acc_tasks_check.cpp, built here with the host compiler under
AddressSanitizer and UBSan, writes and walks the tasks of every (nl, nr) in 0..20 x 0..20 exactly as the kernel's lanes
do and prints the cells it counts; they must be the cells of the plain statement (pe_counter_model.py), with
multiplicities.  No device, no HIP call."""
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import pe_counter_model as pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK_MIN, TASK_CAP = 40, 960  # ACC_TASK_MIN, ACC_TASK_CAP of vs_pe_plan.h


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("acc_tasks") / "acc_tasks_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "acc_tasks_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.splitlines()


def test_tasks_of_every_length_pair_expand_to_the_model_cells(printed):
    pairs, cur = [], None
    for line in printed:
        if line.startswith("P "):
            head, left, right = line[2:].split("|")
            nl, nr = (int(v) for v in head.split())
            cur = ([int(v) for v in left.split()], [int(v) for v in right.split()], Counter())
            assert (len(cur[0]), len(cur[1])) == (nl, nr)
            pairs.append(cur)
        elif line.startswith("C "):
            mat, x, y = (int(v) for v in line[2:].split())
            cur[2][(mat, x, y)] += 1
    assert [(len(l), len(r)) for l, r, _ in pairs] == [(nl, nr) for nl in range(21) for nr in range(21)]
    n_nodes = 200
    for left, right, got in pairs:
        lists = np.zeros((2, pcm.LCAP), dtype=np.int64)
        lists[0, : len(left)] = left
        lists[1, : len(right)] = right
        (nc, nv), (sc, sv) = pcm.count_block(lists, np.array([len(left), len(right)]), n_nodes)
        want = Counter()
        for mat, cells, vals in ((0, nc, nv), (1, sc, sv)):
            for cell, v in zip(cells.tolist(), vals.tolist()):
                want[(mat, cell // n_nodes, cell % n_nodes)] = v
        assert got == want, (len(left), len(right), sorted((got - want).items())[:4], sorted((want - got).items())[:4])
        # (min, max) of short_mat, and the diagonal once per node of either list
        assert all(x <= y for (mat, x, y) in got if mat == 1)
        assert sum(v for (mat, x, y), v in got.items() if mat == 1 and x == y) == len(left) + len(right)


def test_batch_cut_never_splits_a_pair_and_never_returns_none(printed):
    rounds = []
    for line in printed:
        if line.startswith("B "):
            head, tasks = line[2:].split("|")
            cap, n, first, last = (int(v) for v in head.split())
            tasks = tuple(int(v) for v in tasks.split())
            assert len(tasks) == n and TASK_MIN <= cap <= TASK_CAP and max(tasks) <= TASK_MIN
            if first == 0:  # a new round
                rounds.append((cap, tasks, []))
            assert rounds[-1][:2] == (cap, tasks)
            rounds[-1][2].append((first, last))
    assert len(rounds) == 400
    seen_cut = set()
    for cap, tasks, cuts in rounds:
        n = len(tasks)
        # whole pairs, one after the other, all of them: a batch starts where the last one ended
        assert cuts[0][0] == 0 and cuts[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        for first, last in cuts:
            assert first < last <= n  # at least one pair
            assert sum(tasks[first:last]) <= cap  # fits the region
            assert last == n or sum(tasks[first: last + 1]) > cap  # and is the longest run that does
            seen_cut.add(last - first)
    assert 1 in seen_cut and 64 in seen_cut and len(seen_cut) > 10
