#!/usr/bin/env python3
"""The two ingests that find records without a mate, from open to counters, with and without keeping them
(profiles/kept_singles.md).

Takes --block pairs of the bench stream of BASELINE configs[--config] (tools/bam_ingest_legs.py has the generator and the
record writers) under one name per pair and writes them twice: as two plain FASTQ files in one order, 5 % of the records
deleted from each at seeded positions (d1.fq, d2.fq: what `--check-names --check-names-singles` reads), and as ONE BAM with
the later mate of every pair moved back by a random 0..2 000 records, 2.5 % of all records deleted (near.bam: what
`--bam-by-name` reads; about 5 % of what is left has no mate).  Every leg is a fresh child process under its own time limit
that indexes the config's graph, opens the stream, counts every block into a PeCounter and reads the counters back; the clock
runs from the open to the counters:

    pd  pe.PairedNameStream(singles=True)              pk  ... singles="keep"
    bd  pe.BamStream(by_name=True)                     bk  ... singles="keep"

--parent-lib runs pd and bd on another build of the library as well (legs pd0, bd0; e.g. tools/_ab/parent.so of
tools/ab_build.sh in a worktree of the parent commit).  The legs alternate, --rounds rounds; a leg that fails ends the run.

    python tools/kept_singles_legs.py --keep DIR [--parent-lib tools/_ab/parent.so] [--out legs.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/kept_singles_legs.py --leg pd --dir DIR   (one leg, no counters)
    python tools/kept_singles_legs.py --kernel-stats OUT    (kernel names and call counts of such a run as JSON)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEGS = {"pd": "two FASTQ files joined by name, singles dropped", "pk": "two FASTQ files joined by name, singles kept",
        "bd": "BAM by name, singletons dropped", "bk": "BAM by name, singletons kept",
        "pd0": "two FASTQ files joined by name, singles dropped, the other build", "bd0": "BAM by name, singletons dropped, the other build"}
NEW_ENTRIES = ("vs_fastq_join_singles_host", "vs_fastq_join_singles_text")
FILES = ("d1.fq", "d2.fq", "near.bam")
SEED = 79


def make_inputs(d, config, block, level):
    import bam_ingest_legs as bl
    import bam_util as bu
    import bgzf_util as bz

    fwd, rve = bl.bench_ends(d, config, block)
    rng = np.random.default_rng(SEED)
    sizes = {}
    for name, ends in (("d1.fq", fwd), ("d2.fq", rve)):
        rows = np.frombuffer(bl.fastq_bytes(ends, b"p"), dtype=np.uint8).reshape(block, -1)  # (one name per pair: "@p%09d" in both files)
        keep = rng.random(block) >= 0.05
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(rows[keep].tobytes())
        sizes[name] = dict(records=int(keep.sum()), text=int(keep.sum()) * rows.shape[1])
    rows, later = bl.bam_records(fwd, rve, rows_out=True)
    order = np.argsort(np.arange(len(rows), dtype=np.float64) + np.where(later, rng.integers(0, 2001, size=len(rows)) + 0.5, 0.0), kind="stable")
    keep = rng.random(len(rows)) >= 0.025
    recs = rows[order][keep[order]].tobytes()
    head = bu.encode_header(b"@HD\tVN:1.6\tSO:unsorted\n")
    packed = bl.bgzf_members(recs, level)
    with open(os.path.join(d, "near.bam"), "wb") as fh:
        fh.write(bz.member(head, level))
        fh.write(packed)
        fh.write(bz.EOF_MARK)
    sizes["near.bam"] = dict(records=int(keep.sum()), text=len(head) + len(recs), file=len(packed) + 28)
    return sizes


def run_leg(d, leg, config, lib):
    """(child) one leg: prints one JSON line"""
    from vstrains_amd import _native as nat

    if lib:  # another build of the library: without the entries it does not have
        nat.LIB_PATH = lib
        for name in NEW_ENTRIES:
            nat.SYMBOLS.pop(name, None)
    from vstrains_amd import pe as host
    from vstrains_amd import pe_inference
    from vstrains_amd.workloads import CONFIGS, workload_for

    with tempfile.TemporaryDirectory() as tmp:
        st, pre, names, seqs, cum, logger, _ = workload_for(config, tmp)
    ctx = host.Context(0)
    ctx.build_index(seqs, CONFIGS[config]["k"])
    counter = host.PeCounter(ctx)
    path = lambda f: os.path.join(d, f)
    for f in FILES:  # (warm page cache)
        with open(path(f), "rb") as fh:
            while fh.read(1 << 24):
                pass
    keep = leg.endswith("k")
    t0 = time.perf_counter()
    if leg[0] == "p":
        fs = host.PairedNameStream(path("d1.fq"), path("d2.fq"), ctx, singles="keep" if keep else True)
    elif keep:
        fs = host.BamStream(path("near.bam"), ctx, by_name=True, singles="keep")
    else:
        fs = host.BamStream(path("near.bam"), ctx, by_name=True)
    pe_inference.count_stream(ctx, fs, counter)
    node_mat, short_mat, stats = counter.result()
    single = tuple(int(x) for x in counter.single_stats.cpu().numpy())
    dt = time.perf_counter() - t0
    info = dict(fs.info)
    fs.close()
    print(json.dumps(dict(leg=leg, seconds=dt, pairs=info["pairs"], singles=[info.get("singles_fwd", 0), info.get("singles_rve", 0), info.get("singletons", 0)],
                          windows=info.get("windows", 0), node_sum=int(node_mat.sum()), short_sum=int(short_mat.sum()), stats=[int(x) for x in stats],
                          single_stats=list(single))))


def kernel_stats(out_dir):
    """{kernel name: calls} of a rocprofv3 --kernel-trace --stats run (names cut at the first parenthesis)"""
    calls = {}
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Name"].split("(")[0].strip()
                calls[name] = calls.get(name, 0) + int(row["Calls"])
    return dict(sorted(calls.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1)
    ap.add_argument("--block", type=int, default=1_000_000)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="pd,bd,pk,bk")
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", dest="kernel_stats", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats), indent=1))
        return
    if args.leg:
        return run_leg(args.dir, args.leg.rstrip("0"), args.config, os.environ.get("KS_LEG_LIB"))
    legs = [l for l in args.only.split(",") if l in LEGS]
    if args.parent_lib:
        legs = [x for l in legs for x in ((l, l + "0") if l + "0" in LEGS else (l,))]
    d = args.keep or tempfile.mkdtemp(prefix="ks_legs_")
    os.makedirs(d, exist_ok=True)
    if not all(os.path.exists(os.path.join(d, f)) for f in FILES + ("sizes.json",)):
        sizes = make_inputs(d, args.config, args.block, args.level)
        with open(os.path.join(d, "sizes.json"), "w") as fh:
            json.dump(sizes, fh)
    with open(os.path.join(d, "sizes.json")) as fh:
        sizes = json.load(fh)
    results = []
    for rnd in range(args.rounds):
        for leg in legs:
            env = dict(os.environ)
            if leg.endswith("0"):
                env["KS_LEG_LIB"] = os.path.abspath(args.parent_lib)
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--dir", d, "--config", str(args.config)], env=env,
                                  capture_output=True, text=True, timeout=args.limit)
            if proc.returncode != 0:
                print(proc.stderr[-3000:], file=sys.stderr)
                sys.exit("leg %s failed (exit status %d): nothing more is run" % (leg, proc.returncode))
            rec = json.loads(proc.stdout.strip().splitlines()[-1])
            rec.update(leg=leg, round=rnd, what=LEGS[leg])
            results.append(rec)
            print(json.dumps(rec), flush=True)
    summary = {}
    for leg in legs:
        secs = [r["seconds"] for r in results if r["leg"] == leg]
        last = [r for r in results if r["leg"] == leg][-1]
        summary[leg] = dict(what=LEGS[leg], runs=len(secs), seconds=secs, median_s=statistics.median(secs), min_s=min(secs), max_s=max(secs),
                            pairs=last["pairs"], singles=last["singles"], node_sum=last["node_sum"], short_sum=last["short_sum"], stats=last["stats"],
                            single_stats=last["single_stats"])
    out = dict(config=args.config, pairs_generated=args.block, sizes=sizes, summary=summary, runs=results)
    print(json.dumps(out["summary"], indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not args.keep:
        for f in FILES + ("sizes.json",):
            os.unlink(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
