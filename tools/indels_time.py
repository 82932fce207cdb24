#!/usr/bin/env python3
"""Time the indel pass (``k_node_indels``) beside the pileup's kernel (``k_node_pileup``, the yardstick) on the graph of a
BASELINE config, by the procedure of profiles/pileup.md: one block of synthetic pairs, the index built once, then on the same
block and context ``--rounds`` rounds of ``Context.node_pileup`` and ``Context.node_indels``, alternating, each call timed with
events on the stream.  ``node_indels`` is timed whole: the clearing of its five words of scratch, the kernel, the copy of the
record count to the host, the synchronisation on it and the small launch that adds the four tallies.  The event buffer is
sized by one call before the rounds, so every timed call fits.

    python tools/indels_time.py [--config 2] [--pairs 1048576] [--rounds 7] [--max-len 16] [--out FILE.json]

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
    ap.add_argument("--max-len", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

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
    gapped = host.IndelCounter(ctx, max_len=a.max_len)
    block = ctx.synth_pairs(st.genomes, cum, 20250000 + a.config, 0, a.pairs, L, int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    res = dict(config=a.config, k=k, nodes=len(seqs), bases=sum(len(q) for q in seqs), pairs=a.pairs, read_len=L, rounds=a.rounds, slots=piles.slots,
               max_len=a.max_len)

    def timed(fn):
        ctx.sync()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    # one pass of each first: the tallies of one pass, the distinct records, and a buffer every timed call fits
    piles.add(block)
    gapped.add(block)
    ctx.sync()
    one_pass = gapped.tallies()
    records = gapped.result()
    events = one_pass[1] + one_pass[2]
    res.update(pileup_tallies=piles.tallies(), tallies=one_pass, events=events, distinct_records=len(records), launches_of_the_first_pass=gapped.launches,
               longest=max([r[3] for r in records] or [0]), by_length=[sum(r[5] + r[6] for r in records if r[3] == n) for n in range(1, a.max_len + 1)])
    buf = torch.zeros((max(events, 1), 2), dtype=torch.int64, device=gapped.device)
    found = []

    legs = dict(k_node_pileup=[], node_indels=[])
    for r in range(a.rounds):
        legs["k_node_pileup"].append(timed(lambda: ctx.node_pileup(block, piles.first.data_ptr(), piles.diff.data_ptr(), piles.alt.data_ptr(), 8,
                                                                  piles.tally.data_ptr())))
        piles.fold()  # (outside the timing: the differences of one block stay below 2^32)
        legs["node_indels"].append(timed(lambda: found.append(ctx.node_indels(block, gapped.first.data_ptr(), a.max_len, buf.data_ptr(), buf.shape[0],
                                                                             gapped.tally.data_ptr()))))
    ctx.sync()
    res.update(every_call_found_the_same=found == [events] * a.rounds,
               totals_are_passes_times_one_pass=gapped.tallies() == tuple((a.rounds + 1) * v for v in one_pass)
               and piles.tallies() == tuple((a.rounds + 1) * v for v in res["pileup_tallies"]))
    for name, ms in legs.items():
        res[name] = dict(ms=[round(v, 3) for v in ms], median=round(statistics.median(ms[2:] if len(ms) > 2 else ms), 3))
    block.free()
    ctx.keep_masks(False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["every_call_found_the_same"] and res["totals_are_passes_times_one_pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
