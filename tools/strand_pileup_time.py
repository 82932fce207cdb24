#!/usr/bin/env python3
"""Time the stranded pileup (``k_node_pileup_strands``) beside the pileup's kernel (``k_node_pileup``, the yardstick) and the
device caller (``vs_pileup_call``, one plane) beside the path it would replace (``PileupCounter.result()`` +
``node_depth.variant_records``) on the graph of a BASELINE config, by the procedure of profiles/pileup.md: one block of
synthetic pairs, the index built once, then on the same block and context ``--rounds`` rounds of ``Context.node_pileup`` and
``Context.node_pileup_strands``, alternating, each call timed with events on the stream.  The two ways to the records are then
timed by the wall clock on the same folded tables of ONE pass over the block (both end synchronised, with the records on the
host), ``--rounds`` times each, and their records compared.

    python tools/strand_pileup_time.py [--config 2] [--pairs 1048576] [--rounds 7] [--out FILE.json]

Prints one JSON line; times in milliseconds (every call, and the median of all but the first two)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1048576)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from vstrains_amd import node_depth
    from vstrains_amd import pe as host
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[a.config]
    k, L = cfg["k"], cfg["read_len"]
    with tempfile.TemporaryDirectory() as tmp:
        st, pre, names, seqs, cum, logger, _ = workload_for(a.config, tmp)
    ctx = host.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.build_index(seqs, k)
    piles = host.PileupCounter(ctx, max_mismatch=8)  # (the blocks built from here on keep their masks)
    strands = host.StrandPileupCounter(ctx, max_mismatch=8)
    block = ctx.synth_pairs(st.genomes, cum, 20250000 + a.config, 0, a.pairs, L, int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    res = dict(config=a.config, k=k, nodes=len(seqs), bases=sum(len(q) for q in seqs), pairs=a.pairs, read_len=L, rounds=a.rounds, slots=piles.slots)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    # one pass of each kernel first: the tables the two ways to the records are timed on, and the planes held to the pileup
    piles.add(block)
    strands.add(block)
    offsets, depth, alt = piles.result()
    s_offsets, s_depth, s_alt = strands.result()
    res.update(tallies=piles.tallies(), planes_sum_to_the_pileup=bool((s_depth.sum(axis=1) == depth).all() and (s_alt.sum(axis=1) == alt).all()
                                                                       and strands.tallies() == piles.tallies()),
               depth_per_plane=[int(v) for v in s_depth.sum(axis=0)], alt_per_plane=[int(v) for v in s_alt.sum(axis=(0, 2))])

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return 1000.0 * (time.perf_counter() - t0), out

    legs = dict(k_node_pileup=[], k_node_pileup_strands=[], call_on_device_one_plane=[], call_on_device_two_planes=[], result_and_variant_records=[])
    for r in range(a.rounds):
        ms, called = wall(lambda: piles.call(2, 0.01))
        legs["call_on_device_one_plane"].append(ms)
        ms, called2 = wall(lambda: strands.call(2, 0.01, 0))
        legs["call_on_device_two_planes"].append(ms)
        ms, records = wall(lambda: node_depth.variant_records(names, seqs, *piles.result()))
        legs["result_and_variant_records"].append(ms)
        print("round %d: %d records, %.1f ms on the host" % (r, len(records), ms), file=sys.stderr, flush=True)
    on_device = [r[:6] for r in node_depth.strand_records(names, called)]
    res.update(records=len(records), device_records_equal_the_hosts=on_device == records == [r[:6] for r in node_depth.strand_records(names, called2)],
               record_bytes=48 * len(records), table_bytes_one_plane=48 * piles.slots, table_bytes_two_planes=96 * piles.slots)

    for r in range(a.rounds):
        legs["k_node_pileup"].append(timed(lambda: ctx.node_pileup(block, piles.first.data_ptr(), piles.diff.data_ptr(), piles.alt.data_ptr(), 8,
                                                                  piles.tally.data_ptr())))
        piles.fold()  # (outside the timing: the differences of one block stay below 2^32)
        legs["k_node_pileup_strands"].append(timed(lambda: ctx.node_pileup_strands(block, strands.first.data_ptr(), strands.slots, strands.diff.data_ptr(),
                                                                                  strands.alt.data_ptr(), 8, strands.tally.data_ptr())))
        strands.fold()
    ctx.sync()
    res.update(totals_are_passes_times_one_pass=strands.tallies() == piles.tallies() == tuple((a.rounds + 1) * v for v in res["tallies"]))
    for name, ms in legs.items():
        res[name] = dict(ms=[round(v, 3) for v in ms], median=round(statistics.median(ms[2:] if len(ms) > 2 else ms), 3))
    block.free()
    ctx.keep_masks(False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["planes_sum_to_the_pileup"] and res["device_records_equal_the_hosts"] and res["totals_are_passes_times_one_pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
