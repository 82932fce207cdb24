#!/usr/bin/env python3
"""The read leg of the pe_info / st_info hand-off on one GPU: host route against device route (profiles/info_read.md).

Builds the graph of BASELINE configs[--config], counts --pairs pairs of its bench stream on the device, writes the four file
pairs once (d dense, s sparse, D dense BGZF, S sparse BGZF), and then times ``HipPeLinks.from_files`` from the call to the
table ready and the stream synchronised, per pair in two legs:

    h  host route     device_parse=False: vs_info_parse on the host threads (gzip inflated by zlib on one thread), the cells
                      concatenated and uploaded, vs_links_from_cells -- the parent commit's code
    v  device route   device_parse=True: vs_links_from_info (k_inflate, k_info_scan, k_info_parse)

The legs alternate inside ONE process in the order of --only x --routes, --rounds rounds, with a warm page cache (every file is
read once before the first round); the order is part of the summary.  Every leg's table is downloaded and compared with the
first one.  Prints one JSON line; --out writes it to a file as well.

    python tools/info_read_legs.py --config 2 --out info_read.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/info_read_legs.py --only D --routes v --rounds 1     (no counters in that run)
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"d": ("dense", {}), "s": ("sparse", dict(sparse=True)), "D": ("dense_bgzf", dict(bgzf=True)), "S": ("sparse_bgzf", dict(bgzf=True, sparse=True))}
ROUTES = {"h": ("host", False), "v": ("device", True)}
STREAM_SEED = 77
BLOCK = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=None, help="pairs counted before the files are written (default: the config's whole job, at most 10 M)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="dsDS", help="the file pairs and their order inside a round")
    ap.add_argument("--routes", default="hv", help="the legs of a pair and their order")
    ap.add_argument("--sparse-min-nodes", type=int, default=0, help="from how many nodes the table is CSR rows (0: the library's 32 768)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from vstrains_amd import pe as host
    from vstrains_amd import pe_inference
    from vstrains_amd.graph.hip_ops import HipPeLinks
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[args.config]
    pairs = args.pairs if args.pairs is not None else min(cfg["total_pairs"], 10_000_000)
    kinds = [k for k in args.only if k in KINDS]
    routes = [r for r in args.routes if r in ROUTES]
    with tempfile.TemporaryDirectory() as work:
        t0 = time.perf_counter()
        st, pre, names, seqs, cum, logger, _ = workload_for(args.config, work)
        ctx = host.Context(0)
        ctx.build_index(seqs, cfg["k"])
        counter = host.PeCounter(ctx)
        for first in range(0, pairs, BLOCK):
            block = ctx.synth_pairs(st.genomes, cum, STREAM_SEED, first, min(BLOCK, pairs - first), cfg["read_len"], int(0.005 * 2 ** 32),
                                    int(0.001 * 2 ** 32))
            counter.add(block)
            ctx.sync()
            block.free()
        files, sizes = {}, {}
        for k in kinds:
            tag, kw = KINDS[k]
            out = os.path.join(work, "aln_" + tag)
            os.makedirs(out)
            pe_inference.write_info_files(out, names, counter, **kw)
            suffix = ".gz" if kw.get("bgzf") else ""
            files[k] = (os.path.join(out, "pe_info" + suffix), os.path.join(out, "st_info" + suffix))
            sizes[tag] = [os.path.getsize(f) for f in files[k]]
            for f in files[k]:  # (warm page cache)
                with open(f, "rb") as fh:
                    while fh.read(1 << 24):
                        pass
        setup = time.perf_counter() - t0
        legs = [(k, r) for k in kinds for r in routes]
        runs = {leg: [] for leg in legs}
        reads, first_table, equal = {}, None, []
        for rnd in range(args.rounds):
            for k, r in legs:
                ctx.sync()
                t1 = time.perf_counter()
                table = HipPeLinks.from_files(ctx, names, files[k][0], files[k][1], sparse_min_nodes=args.sparse_min_nodes, device_parse=ROUTES[r][1])
                ctx.sync()
                dt = time.perf_counter() - t1
                runs[(k, r)].append(dt)
                reads["%s/%s" % (KINDS[k][0], ROUTES[r][0])] = HipPeLinks.last_read
                got = table.to_numpy()
                table.close()
                if first_table is None:
                    first_table = got
                equal.append(bool(np.array_equal(got, first_table)))
                print("round %d %s %s: %.4f s  equal to the first table: %s" % (rnd, KINDS[k][0], ROUTES[r][0], dt, equal[-1]), flush=True)
    summary = dict(config=args.config, nodes=len(names), pairs=pairs, setup_seconds=setup, sparse_min_nodes=args.sparse_min_nodes,
                   order=["%s/%s" % (KINDS[k][0], ROUTES[r][0]) for k, r in legs], file_bytes=sizes,
                   legs={"%s/%s" % (KINDS[k][0], ROUTES[r][0]): dict(seconds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
                         for (k, r), v in runs.items() if v},
                   last_read=reads, tables_equal=all(equal), table_nonzero=int(np.count_nonzero(first_table)) if first_table is not None else 0)
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if not all(equal):
        sys.exit("a leg's table differs from the first")


if __name__ == "__main__":
    main()
