#!/usr/bin/env python3
"""CPU model of the work units of k_pe_accumulate on a config's own read stream (no GPU): per pair, what a wavefront's
lanes spend in three forms of the kernel --

  runs      the form before the tasks: list rows cut into runs of at most four partners, one lane per run, every run
            four positions
  tasks     one task per matrix row (vstrains_amd/csrc/vs_acc_tasks.h: node rows, short rows folded with their mirror
            rows), handed to lanes in pair order; a window of 64 tasks takes as many turns as its longest task
  ordered   the same tasks ordered by their turns inside a batch (the pairs of a wavefront's round of 64 whose tasks fit
            its task region), longest first

for the pairs in locus order (first node of the forward read's list), 64 consecutive pairs per wavefront round.
The end lists come from the CPU oracle (oracle/pe_oracle_c) on reads of the bench generator's seed.  A MODEL of lane
occupancy, not a timing: profiles/EXPERIMENTS.md sets it next to the measured kernel times.

    python tools/acc_tasks_model.py [--config 2] [--pairs 200000] [--region 960]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import pe_oracle_c  # noqa: E402
from vstrains_amd.workloads import CONFIGS, workload_for  # noqa: E402

LCAP = 20


def fold(n, a):
    """vs_acc_fold -> (p1, p2, e)"""
    a2 = n - 1 - a
    if a2 == a:
        return a, n, n
    a_first = (-(n - a)) % 4 <= (-(a + 1)) % 4
    return (a, a2, n) if a_first else (a2, a, n)


def turns(p1, p2, e):
    return -(-(e - p1) // 4) * 4 + (e - p2) if p2 < e else e - p1


def pair_tasks(nl, nr):
    """(partners, turns) of every task of a pair, in the order a lane writes them"""
    out = [(nr, nr)] * (nl if nr else 0)
    for n in (nl, nr):
        for a in range((n + 1) // 2):
            p1, p2, e = fold(n, a)
            out.append(((e - p1) + (e - p2), turns(p1, p2, e)))
    return out


def windows(tasks):
    """lane turns of a run of tasks handed out 64 at a time: every window as long as its longest task"""
    return sum(64 * max(t for _, t in tasks[i: i + 64]) for i in range(0, len(tasks), 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--region", type=int, default=960, help="task entries per wavefront (ACC_TASK_CAP)")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    st, _, _, seqs, cum, _, _ = workload_for(args.config, tempfile.mkdtemp())
    orc = pe_oracle_c.Oracle(seqs, cfg["k"])
    fwd, rve = pe_oracle_c.synth_pairs(st.genomes, cum, 20250000 + args.config, 0, args.pairs, cfg["read_len"], int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    ends = []
    for p in range(args.pairs):
        f, r = fwd[p].tobytes().decode(), rve[p].tobytes().decode()
        if "N" in f or "N" in r:  # (dropped pairs add nothing)
            ends.append(([], []))
            continue
        l, r2 = orc.map_end(f), orc.map_end(r)
        ends.append(([], []) if len(l) > LCAP or len(r2) > LCAP else (l, r2))  # (longer lists: the overflow kernels)
    n_nodes = len(seqs)
    order = sorted(range(args.pairs), key=lambda p: ends[p][0][0] if ends[p][0] else n_nodes)
    shape = [(len(ends[p][0]), len(ends[p][1])) for p in order]
    g = [sum(-(-m // 4) for m in range(1, n + 1)) for n in range(LCAP + 1)]
    n_pairs = float(args.pairs)
    runs = sum(nl * -(-nr // 4) + g[nl] + g[nr] for nl, nr in shape)
    incs = sum(nl * nr + nl * (nl + 1) // 2 + nr * (nr + 1) // 2 for nl, nr in shape)
    n_tasks = plain = ordered = batches = 0
    for lo in range(0, args.pairs, 64):
        group = [pair_tasks(nl, nr) for nl, nr in shape[lo: lo + 64]]
        flat = [t for pt in group for t in pt]
        n_tasks += len(flat)
        plain += windows(flat)
        first = 0
        while first < len(group):  # the batch cut
            last, words = first, 0
            while last < len(group) and words + len(group[last]) <= args.region:
                words += len(group[last])
                last += 1
            batch = sorted((t for pt in group[first:last] for t in pt), key=lambda t: -t[1])
            ordered += windows(batch)
            batches += 1 if batch else 0
            first = last
    print("config %d, %d pairs in locus order, rounds of 64 pairs, task region %d entries" % (args.config, args.pairs, args.region))
    print("increments per pair            %.1f" % (incs / n_pairs))
    print("runs     : %.1f runs per pair, %.1f positions per pair, utilisation %.2f" % (runs / n_pairs, 4 * runs / n_pairs, incs / (4.0 * runs)))
    print("tasks    : %.1f tasks per pair, %.1f turns per pair, utilisation %.2f" % (n_tasks / n_pairs, plain / n_pairs, incs / float(plain)))
    print("ordered  : %.1f tasks per pair, %.1f turns per pair, utilisation %.2f, %.2f batches per round" % (
        n_tasks / n_pairs, ordered / n_pairs, incs / float(ordered), batches / (n_pairs / 64)))


if __name__ == "__main__":
    main()
