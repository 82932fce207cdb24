#!/usr/bin/env python3
"""The write leg of the PE drop-in, dense against sparse, on one GPU (profiles/sparse_info.md).

Builds the graph of BASELINE configs[--config], counts --pairs pairs of its bench stream on the device, and then times
``pe_inference.write_info_files`` from counters on the device to files closed:

    d  dense   pe_info / st_info, N^2 lines each (result() on the host, vs_write_matrix_text): the code as it was
    s  sparse  the lines of non-zero count only, formatted on the device (vs_write_info_sparse)

The legs alternate inside ONE process, --rounds rounds (the first round carries the one-off costs of either leg: pinned
buffers, page cache); every sparse file is checked against the dense one of the same round without its ``:0`` lines when
both legs run.  Prints one JSON line; --out writes it to a file as well.

    python tools/sparse_info_legs.py --config 2 --out sparse_info.json
    python tools/sparse_info_legs.py --config 4 --only s --rounds 1        (dense is 36 GB per file there: not attempted)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sparse_info_legs.py --only s --rounds 1
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"d": "dense", "s": "sparse"}
STREAM_SEED = 77
BLOCK = 1 << 20


def same_without_zero_lines(dense_path, sparse_path):
    with open(dense_path, "rb") as fd, open(sparse_path, "rb") as fs:
        for line in fd:
            if line.endswith(b":0\n"):
                continue
            if fs.readline() != line:
                return False
        return fs.readline() == b""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=None, help="pairs counted before the legs (default: the config's whole job, at most 10 M)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="ds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from vstrains_amd import pe as host
    from vstrains_amd import pe_inference
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[args.config]
    pairs = args.pairs if args.pairs is not None else min(cfg["total_pairs"], 10_000_000)
    legs = [l for l in args.only if l in LEGS]
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
        setup = time.perf_counter() - t0
        runs = {l: [] for l in legs}
        sizes, checked = {}, []
        for rnd in range(args.rounds):
            dirs = {}
            for l in legs:
                out = os.path.join(work, "aln_%s_%d" % (l, rnd))
                os.makedirs(out)
                ctx.sync()
                t1 = time.perf_counter()
                pe_inference.write_info_files(out, names, counter, sparse=(l == "s"))
                dt = time.perf_counter() - t1
                runs[l].append(dt)
                dirs[l] = out
                sizes[LEGS[l]] = {f: os.path.getsize(os.path.join(out, f)) for f in ("pe_info", "st_info")}
                print("round %d %s: %.4f s  %s" % (rnd, LEGS[l], dt, sizes[LEGS[l]]), flush=True)
            if len(dirs) == 2:
                checked.append(all(same_without_zero_lines(os.path.join(dirs["d"], f), os.path.join(dirs["s"], f)) for f in ("pe_info", "st_info")))
            for out in dirs.values():  # (the dense files of a round are not kept: 0.6 GB at configs[2])
                for f in ("pe_info", "st_info"):
                    os.remove(os.path.join(out, f))
        lines = None
        if "s" in legs:
            out = os.path.join(work, "aln_count")
            os.makedirs(out)
            info = counter.write_sparse_text(os.path.join(out, "pe_info"), os.path.join(out, "st_info"), names)
            lines = dict(pe_info=info[0], st_info=info[1])
    summary = dict(config=args.config, nodes=len(names), pairs=pairs, setup_seconds=setup, tile_map=counter.tile_map is not None,
                   legs={LEGS[l]: dict(seconds=runs[l], median=sorted(runs[l])[len(runs[l]) // 2], spread=max(runs[l]) - min(runs[l]))
                         for l in legs if runs[l]},
                   file_bytes=sizes, sparse_info=lines, sparse_equals_filtered_dense=checked)
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if checked and not all(checked):
        sys.exit("a sparse file differs from the dense file without its zero lines")


if __name__ == "__main__":
    main()
