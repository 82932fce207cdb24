#!/usr/bin/env python3
"""Time the site-pair pass (``k_node_site_pairs``) beside the pileup's kernel (``k_node_pileup``, the yardstick) on the graph
of a BASELINE config, by the procedure of profiles/pileup.md: one block of synthetic pairs, the index built once, then on the
same block and context ``--rounds`` rounds of ``Context.node_pileup`` and ``Context.node_site_pairs``, alternating, each call
timed with events on the stream.  The sites are those the default ``--variants`` thresholds call on that block.  A third leg
runs the site-pair kernel with ONE site on the shortest segment that has positions, so that nearly every alignment leaves at
the empty range: what the early exit buys.

    python tools/site_pairs_time.py [--config 2] [--pairs 1048576] [--rounds 7] [--span 1000] [--out FILE.json]

Prints one JSON line; times in milliseconds (every call, and the median of all but the first two)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1048576)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--span", type=int, default=1000)
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
    block = ctx.synth_pairs(st.genomes, cum, 20250000 + a.config, 0, a.pairs, L, int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    res = dict(config=a.config, k=k, nodes=len(seqs), pairs=a.pairs, read_len=L, rounds=a.rounds, span=a.span, slots=piles.slots)

    # the sites: what --variants would call on this block
    piles.add(block)
    offsets, depth, alt = piles.result()
    records = node_depth.variant_records(names, seqs, offsets, depth, alt)
    sites = node_depth.record_sites(names, records)
    res.update(records=len(records), sites=len(sites), pileup_tallies=piles.tallies())
    linked = host.SitePairCounter(ctx, sites, max_mismatch=8, max_span=a.span)
    res.update(cells=linked.n_cells, plan=host.site_pairs_plan(len(seqs), k, 2 * a.pairs, L, torch.cuda.get_device_properties(0).multi_processor_count))
    short = min((n for n in range(len(seqs)) if len(seqs[n]) >= k + 1), key=lambda n: len(seqs[n]))
    alone = host.SitePairCounter(ctx, [(short, 0)], max_mismatch=8, max_span=a.span)
    res.update(lone_site_segment_bases=len(seqs[short]))

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = dict(k_node_pileup=[], k_node_site_pairs=[], k_node_site_pairs_lone_site=[])
    first = None
    for r in range(a.rounds):
        legs["k_node_pileup"].append(timed(lambda: ctx.node_pileup(block, piles.first.data_ptr(), piles.diff.data_ptr(), piles.alt.data_ptr(), 8,
                                                                  piles.tally.data_ptr())))
        piles.fold()  # (outside the timing: the differences of one block stay below 2^32)
        legs["k_node_site_pairs"].append(timed(lambda: linked.add(block)))
        legs["k_node_site_pairs_lone_site"].append(timed(lambda: alone.add(block)))
        if first is None:
            first = linked.tallies()
    ctx.sync()
    total = linked.tallies()
    seg, pos_a, pos_b, counts = linked.result()
    res.update(tallies_per_pass=first, totals_are_rounds_times_one_pass=total == tuple(a.rounds * v for v in first),
               pairs_of_sites_with_a_count=len(seg), count_sum_per_pass=int(counts.sum()) // a.rounds, lone_site_tallies_per_pass=tuple(v // a.rounds for v in alone.tallies()))
    for name, ms in legs.items():
        res[name] = dict(ms=[round(v, 3) for v in ms], median=round(statistics.median(ms[2:] if len(ms) > 2 else ms), 3))
    block.free()
    ctx.keep_masks(False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["totals_are_rounds_times_one_pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
