#!/usr/bin/env python3
"""The write leg of the PE drop-in on one GPU: dense, sparse, and the two BGZF forms (profiles/bgzf_info.md).

Builds the graph of BASELINE configs[--config], counts --pairs pairs of its bench stream on the device, and then times
``pe_inference.write_info_files`` from counters on the device to files closed:

    d  dense        pe_info / st_info, N^2 lines each (result() on the host, vs_write_matrix_text)
    s  sparse       the lines of non-zero count only, formatted on the device (vs_write_info_sparse)
    D  dense BGZF   pe_info.gz / st_info.gz: the dense text formatted and deflated on the device (vs_write_info_bgzf)
    S  sparse BGZF  the sparse text, formatted and deflated on the device

The legs alternate inside ONE process in the order of --only, --rounds rounds (the first round carries the one-off costs of
every leg: pinned buffers, page cache); the order is part of the summary.  Every BGZF file is inflated with zlib and
compared with the plain file of the same round when that leg runs too.  The d and s legs are the parent commit's code: their
times on the same box are what the BGZF legs are compared with.  Prints one JSON line; --out writes it to a file as well.

    python tools/bgzf_info_legs.py --config 2 --out bgzf_info.json
    python tools/bgzf_info_legs.py --config 4 --only sS --rounds 1        (dense is 36 GB of text per file there)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bgzf_info_legs.py --only D --rounds 1      (no counters in that run)
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"d": "dense", "s": "sparse", "D": "dense_bgzf", "S": "sparse_bgzf"}
PLAIN_OF = {"D": "d", "S": "s"}
STREAM_SEED = 77
BLOCK = 1 << 20


def inflates_to(gz_path, plain_path):
    """every gzip member of gz_path, inflated in pieces, equals plain_path"""
    with open(gz_path, "rb") as fz, open(plain_path, "rb") as fp:
        d = zlib.decompressobj(31)
        for chunk in iter(lambda: fz.read(1 << 22), b""):
            while chunk:
                out = d.decompress(chunk)
                if out and fp.read(len(out)) != out:
                    return False
                chunk = b""
                if d.eof:  # the next member starts in what this one left over
                    chunk, d = d.unused_data, zlib.decompressobj(31)
        return fp.read(1) == b""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=None, help="pairs counted before the legs (default: the config's whole job, at most 10 M)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="dsDS", help="the legs and their order inside a round")
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
                out = os.path.join(work, "aln_%s_%d" % (LEGS[l], rnd))
                os.makedirs(out)
                ctx.sync()
                t1 = time.perf_counter()
                pe_inference.write_info_files(out, names, counter, sparse=(l in "sS"), bgzf=(l in "DS"))
                dt = time.perf_counter() - t1
                runs[l].append(dt)
                dirs[l] = out
                sizes[LEGS[l]] = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))}
                print("round %d %s: %.4f s  %s" % (rnd, LEGS[l], dt, sizes[LEGS[l]]), flush=True)
            for z, p in PLAIN_OF.items():
                if z in dirs and p in dirs:
                    checked.append(all(inflates_to(os.path.join(dirs[z], f + ".gz"), os.path.join(dirs[p], f)) for f in ("pe_info", "st_info")))
            for out in dirs.values():  # (the files of a round are not kept: the dense pair is 0.6 GB at configs[2])
                for f in os.listdir(out):
                    os.remove(os.path.join(out, f))
        info = {}
        for l in legs:
            if l in "DS":
                out = os.path.join(work, "aln_info_" + LEGS[l])
                os.makedirs(out)
                got = counter.write_bgzf_text(os.path.join(out, "pe_info.gz"), os.path.join(out, "st_info.gz"), names, dense=(l == "D"))
                info[LEGS[l]] = dict(pe_info=got[0], st_info=got[1])
    summary = dict(config=args.config, nodes=len(names), pairs=pairs, setup_seconds=setup, tile_map=counter.tile_map is not None,
                   order=[LEGS[l] for l in legs],
                   legs={LEGS[l]: dict(seconds=runs[l], median=sorted(runs[l])[len(runs[l]) // 2], spread=max(runs[l]) - min(runs[l]))
                         for l in legs if runs[l]},
                   file_bytes=sizes, bgzf_info=info, bgzf_inflates_to_plain=checked)
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if checked and not all(checked):
        sys.exit("a BGZF file does not inflate to the plain file of its round")


if __name__ == "__main__":
    main()
