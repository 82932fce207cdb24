#!/usr/bin/env python3
"""Time the contig threading pass on the graph of a BASELINE config (default configs[2]) beside the plain window model on
the host (tests/contig_thread_model.py), and check that both give the config's own contigs.paths back byte for byte.

    python tools/contig_paths_time.py [--config 2] [--repeat 5] [--out FILE.json]

The contigs are spelled from the config's contigs.paths and graph (the first segment of a part whole, then seg[k:], parts
joined by ten N).  Prints one JSON line; times in milliseconds, the device legs as the best and the median of the repeats."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import contig_thread_model as model
    from vstrains_amd import contig_paths, synth
    from vstrains_amd import pe as host
    from vstrains_amd.workloads import CONFIGS

    c = CONFIGS[a.config]
    pc = synth.make_pipeline_case(n_strains=c["n_strains"], genome_len=c["genome_len"], snp_rate=c["snp_rate"], k=c["k"], n_pairs=0,
                                  read_len=c["read_len"], seed=c["seed"], abundance_ratio=c["abundance_ratio"])
    k = c["k"]
    res = dict(config=a.config, k=k)
    with tempfile.TemporaryDirectory() as tmp:
        gfa, fasta = os.path.join(tmp, "input.gfa"), os.path.join(tmp, "contigs.fasta")
        with open(gfa, "w") as fh:
            fh.write(pc.gfa_text)
        ids, seqs = host.read_gfa_segments(gfa)
        seg_of = dict(zip(ids, seqs))
        entries = [(n, p) for n, p in model.read_paths(pc.paths_text) if not n.endswith("'")]
        contigs = [model.spell(p, seg_of, k) for _, p in entries]
        with open(fasta, "w") as fh:
            for (n, _), text in zip(entries, contigs):
                fh.write(">%s\n%s\n" % (n, text))
        res.update(segments=len(seqs), segment_bases=sum(map(len, seqs)), contigs=len(contigs), contig_bases=sum(map(len, contigs)),
                   longest_contig=max(map(len, contigs)))

        # the plain model on the host: the table of every (k+1)-mer of the graph, then the walk
        t0 = time.perf_counter()
        table = model.window_table(seqs, k)
        t1 = time.perf_counter()
        text = "".join(model.entry(n, model.thread(seqs, k, cg, table=table)[0], ids) for (n, _), cg in zip(entries, contigs))
        t2 = time.perf_counter()
        res.update(model_table_ms=1e3 * (t1 - t0), model_walk_ms=1e3 * (t2 - t1), model_equals_paths=text == pc.paths_text)

        ctx = host.Context(0)
        whole = []
        for _ in range(a.repeat + 1):  # (the first pass allocates: not counted)
            t0 = time.perf_counter()
            got, tally = contig_paths.thread_contigs(ctx, gfa, fasta)
            whole.append(1e3 * (time.perf_counter() - t0))
        res.update(device_equals_paths=got == pc.paths_text, tally=tally, command_ms_best=min(whole[1:]), command_ms_median=statistics.median(whole[1:]))

        # the legs of the pass on their own: index, block, matches (the kernels and the copy), chain
        legs = dict(index=[], pack=[], mems=[], chain=[])
        lens = [len(s) for s in seqs]
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            ctx.build_index(seqs, k)
            ctx.sync()
            t1 = time.perf_counter()
            ctx.keep_masks(True)
            block = ctx.pack_singles(contigs)
            ctx.sync()
            t2 = time.perf_counter()
            mems = ctx.contig_mems(block)
            t3 = time.perf_counter()
            host.contig_chain(mems, lens, k, len(contigs))
            t4 = time.perf_counter()
            block.free()
            ctx.keep_masks(False)
            for name, dt in zip(("index", "pack", "mems", "chain"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                legs[name].append(1e3 * dt)
        info = ctx.contig_mems_last()
        res.update(records=info["records"], probes=info["probes"], launches_last=info["launches"])
        for name, v in legs.items():
            res[name + "_ms_best"] = min(v[1:])
            res[name + "_ms_median"] = statistics.median(v[1:])
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["device_equals_paths"] and res["model_equals_paths"] else 1


if __name__ == "__main__":
    sys.exit(main())
