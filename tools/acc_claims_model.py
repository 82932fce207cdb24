#!/usr/bin/env python3
"""CPU count of how often k_pe_accumulate meets a cell that is not in its table yet, on a config's own read stream (no
GPU).  The end lists come from the CPU oracle (oracle/pe_oracle_c) on reads of the bench generator's seed, in locus order
(first node of the forward read's list).  Every run of 1 024 consecutive pairs of ONE locus is laid out as a workgroup
round: 16 wavefronts x 64 pairs, every wavefront's tasks cut into batches and ordered by length as the kernel orders them
(tools/acc_tasks_model.py: pair_tasks, windows), a lane walking its task a partner a turn, the sixteen wavefronts turn by
turn side by side.  The round has one cell set, empty at its start (the table is written out at 1/16 fill: far fewer
cells than a round brings).  Counted:

  first touches   a cell counts as present from the turn that first touches it, and a turn's first touch of it is one miss
                  whatever the number of lanes that bring it: the fewest misses any table can have
  lane misses     every lane of the sixteen wavefronts whose cell was not present when the turn began misses (what the
                  kernel's lanes see when a claim lands within its turn; slots held by ANOTHER cell are not modelled)

and from the per-turn misses of a wavefront, how often it has to stop for a claim pass: once per turn that has a miss
(claim where the miss happens), once per Q queued keys (the pass drains the queue when a turn's misses do not fit), and
with one waiting key per lane (the pass comes when a lane that holds a key misses again).  A MODEL: profiles/EXPERIMENTS.md
sets it next to the device's own counts.

    python tools/acc_claims_model.py [--config 2] [--pairs 800000] [--region 832] [--queue 64]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from acc_tasks_model import LCAP, fold, pair_tasks, turns  # noqa: E402
from oracle import pe_oracle_c  # noqa: E402
from vstrains_amd.workloads import CONFIGS, workload_for  # noqa: E402

WAVES, PPW = 16, 64


def task_cells(l, r, n_nodes):
    """Per task of a pair, in pair_tasks' order: the cell key of every turn (None: a padding turn of a folded row)."""
    NN = n_nodes * n_nodes
    out = [[x * n_nodes + y for y in r] for x in l] if r else []
    for e in (l, r):
        n = len(e)
        for a in range((n + 1) // 2):
            p1, p2, end = fold(n, a)
            row = [NN + min(e[p1], y) * n_nodes + max(e[p1], y) for y in e[p1:end]]
            if p2 < end:
                row += [None] * ((-len(row)) % 4)
                row += [NN + min(e[p2], y) * n_nodes + max(e[p2], y) for y in e[p2:end]]
            assert len(row) == turns(p1, p2, end)
            out.append(row)
    return out


def wave_turns(pairs, n_nodes, region):
    """The turns of one wavefront's round: a list of turns, each the (lane, cell key) of every lane that counts in it."""
    shapes = [pair_tasks(len(l), len(r)) for l, r in pairs]
    cells = [task_cells(l, r, n_nodes) for l, r in pairs]
    out, first = [], 0
    while first < len(pairs):  # the batch cut
        last, words = first, 0
        while last < len(pairs) and words + len(shapes[last]) <= region:
            words += len(shapes[last])
            last += 1
        batch = sorted((row for p in range(first, last) for row in cells[p]), key=lambda row: -len(row))
        for lo in range(0, len(batch), 64):  # a window: as many turns as its longest task
            window = batch[lo: lo + 64]
            for t in range(len(window[0])):
                out.append([(lane, row[t]) for lane, row in enumerate(window) if t < len(row) and row[t] is not None])
        first = last
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=800000)
    ap.add_argument("--region", type=int, default=832, help="task entries per wavefront")
    ap.add_argument("--queue", type=int, default=64, help="keys a wavefront collects before a claim pass")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    st, _, _, seqs, cum, _, _ = workload_for(args.config, tempfile.mkdtemp())
    orc = pe_oracle_c.Oracle(seqs, cfg["k"])
    fwd, rve = pe_oracle_c.synth_pairs(st.genomes, cum, 20250000 + args.config, 0, args.pairs, cfg["read_len"], int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    n_nodes = len(seqs)
    by_locus = {}
    for p in range(args.pairs):
        f, r = fwd[p].tobytes().decode(), rve[p].tobytes().decode()
        if "N" in f or "N" in r:
            continue
        l, r2 = orc.map_end(f), orc.map_end(r)
        if l and len(l) <= LCAP and len(r2) <= LCAP:
            by_locus.setdefault(l[0], []).append((l, r2))
    rounds = [g[lo: lo + WAVES * PPW] for g in by_locus.values() for lo in range(0, len(g) - WAVES * PPW + 1, WAVES * PPW)]
    if not rounds:
        sys.exit("no locus has %d pairs among %d: raise --pairs" % (WAVES * PPW, args.pairs))
    Q = args.queue
    n_turns = incs = distinct = 0
    first_t = first_n = lane_t = lane_n = 0          # turns with a miss / misses, by either rule
    pass_q = [0, 0]                                  # claim passes of a queue of Q keys, by either rule
    pass_reg = [0, 0]                                # ... of one waiting key per lane
    for rnd in rounds:
        waves = [wave_turns(rnd[w * PPW: (w + 1) * PPW], n_nodes, args.region) for w in range(WAVES)]
        present = set()
        qn = [[0, 0] for _ in range(WAVES)]
        held = [[set(), set()] for _ in range(WAVES)]  # lanes that hold a waiting key
        for t in range(max(len(w) for w in waves)):
            before = set(present)
            for w in range(WAVES):
                if t >= len(waves[w]):
                    continue
                keys = waves[w][t]
                n_turns += 1
                incs += len(keys)
                new_lanes = [i for i, k in keys if k not in before]
                firsts, seen = [], set()
                for i, k in keys:
                    if k not in present and k not in seen:
                        firsts.append(i)
                        seen.add(k)
                present |= seen
                for rule, lanes in enumerate((firsts, new_lanes)):
                    if not lanes:
                        continue
                    if rule == 0:
                        first_t += 1
                        first_n += len(lanes)
                    else:
                        lane_t += 1
                        lane_n += len(lanes)
                    if qn[w][rule] + len(lanes) > Q:
                        pass_q[rule] += 1
                        qn[w][rule] = 0
                    qn[w][rule] += len(lanes)
                    if held[w][rule] & set(lanes):
                        pass_reg[rule] += 1
                        held[w][rule] = set()
                    held[w][rule] |= set(lanes)
        for w in range(WAVES):  # what waits at the end of the round
            for rule in range(2):
                pass_q[rule] += 1 if qn[w][rule] else 0
                pass_reg[rule] += 1 if held[w][rule] else 0
        distinct += len(present)
    R = float(len(rounds))
    print("config %d, %d pairs, %d rounds of %d pairs of one locus, task region %d entries" % (args.config, args.pairs, len(rounds), WAVES * PPW, args.region))
    print("per round: %.0f increments on %.0f distinct cells (%.1f %% of the increments are a first touch), %.0f wavefront turns" % (
        incs / R, distinct / R, 100.0 * distinct / incs, n_turns / R))
    for name, tt, nn, pq, pr in (("first touches", first_t, first_n, pass_q[0], pass_reg[0]), ("lane misses", lane_t, lane_n, pass_q[1], pass_reg[1])):
        print("%-13s: %.1f %% of the turns have one, %.2f per turn, %.2f per turn that has one" % (name, 100.0 * tt / n_turns, nn / float(n_turns), nn / float(max(tt, 1))))
        print("               a claim pass once in %.1f turns with a queue of %d keys, once in %.1f turns with one waiting key per lane, once in %.1f where the miss happens" % (
            n_turns / float(max(pq, 1)), Q, n_turns / float(max(pr, 1)), n_turns / float(max(tt, 1))))


if __name__ == "__main__":
    main()
