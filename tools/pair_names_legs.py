#!/usr/bin/env python3
"""Pairs per second of the two-file FASTQ ingest that pairs by read name (`--check-names`, `pe.PairedNameStream`) against the
plain two-file stream on the same reads, on one GPU (profiles/pair_names.md).

Makes the inputs from a seed -- one block of --block pairs, 2 x 150 bp, named `@r<repeat>_<k>/1` and `/2` (no name twice), its
text written --repeat times: 4 M pairs by default -- as the in-step pair and as the same pair with 5 % of the records deleted
from each file at seeded positions, and runs every leg as a fresh child process under a time limit of its own: the stream
opened, every block taken and freed (no counting), from the open to the end of the input.  The legs alternate, --rounds
rounds; the first leg that fails ends the run.

    s  pe.PairedNameStream, strict, on the in-step pair
    j  pe.PairedNameStream, singles (the hash join), on the in-step pair
    d  pe.PairedNameStream, singles, on the pair with 5 % deleted from each file
    f  pe.FastqStream on the in-step pair
    p  leg f on another build of the library (--parent-lib, e.g. tools/_ab/parent.so of tools/ab_build.sh)

    python tools/pair_names_legs.py [--parent-lib tools/_ab/parent.so] [--out legs.json]
    python tools/pair_names_legs.py --only d --rounds 1 --keep DIR      (one leg, e.g. under rocprofv3 ... -- python ...)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"s": "strict, in-step pair", "j": "singles (join), in-step pair", "d": "singles (join), 5 % deleted from each file", "f": "FastqStream, in-step pair",
        "p": "FastqStream, in-step pair, the other build of the library"}
NEW_ENTRIES = ("vs_fastq_pn_open", "vs_fastq_pn_next", "vs_fastq_pn_info", "vs_fastq_pn_close", "vs_fastq_join_host", "vs_fastq_join_text")
FILES = ("r1.fq", "r2.fq", "d1.fq", "d2.fq")


def make_inputs(d, block, repeat, seed, deleted=0.05):
    import numpy as np

    rng = np.random.default_rng(seed)
    out = [open(os.path.join(d, f), "wb") for f in FILES]
    seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(block, 150))] for _ in (1, 2)]
    for rep in range(repeat):
        for which in (0, 1):
            recs = [b"@r%d_%d/%d\n%s\n+\n%s\n" % (rep, k, which + 1, seqs[which][k].tobytes(), b"I" * 150) for k in range(block)]
            out[which].write(b"".join(recs))
            keep = rng.random(block) >= deleted
            out[2 + which].write(b"".join(r for r, k in zip(recs, keep) if k))
    for fh in out:
        fh.close()


def run_leg(d, leg, lib):
    """(child) one leg"""
    from vstrains_amd import _native as nat

    if lib:  # another build of the library: without the entries it does not have
        nat.LIB_PATH = lib
        for name in NEW_ENTRIES:
            nat.SYMBOLS.pop(name, None)
    from vstrains_amd import pe as host

    ctx = host.Context(0)
    path = lambda f: os.path.join(d, f)
    t0 = time.perf_counter()
    if leg in ("s", "j"):
        fs = host.PairedNameStream(path("r1.fq"), path("r2.fq"), ctx, singles=(leg == "j"))
    elif leg == "d":
        fs = host.PairedNameStream(path("d1.fq"), path("d2.fq"), ctx, singles=True)
    else:
        fs = host.FastqStream(path("r1.fq"), path("r2.fq"), ctx)
    blocks = 0
    for block in fs:
        block.free()
        blocks += 1
    ctx.sync()
    dt = time.perf_counter() - t0
    info = fs.info
    fs.close()
    print(json.dumps(dict(leg=leg, seconds=dt, pairs=info["pairs"], blocks=blocks, text_bytes=info["text_bytes"], singles_fwd=info.get("singles_fwd", 0),
                          singles_rve=info.get("singles_rve", 0), windows=info.get("windows", 0), max_window_bytes=info.get("max_window_bytes", 0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="sjdf")
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.dir, args.leg, os.environ.get("PN_LEG_LIB"))
    legs = [l for l in args.only + ("p" if args.parent_lib and "p" not in args.only else "") if l in LEGS and (l != "p" or args.parent_lib)]
    d = args.keep or tempfile.mkdtemp(prefix="pn_legs_")
    os.makedirs(d, exist_ok=True)
    if not all(os.path.exists(os.path.join(d, f)) for f in FILES):
        make_inputs(d, args.block, args.repeat, args.seed)
    results = []
    for rnd in range(args.rounds):
        for leg in legs:
            env = dict(os.environ)
            if leg == "p":
                env["PN_LEG_LIB"] = os.path.abspath(args.parent_lib)
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--dir", d], env=env, capture_output=True, text=True,
                                  timeout=args.limit)
            if proc.returncode != 0:
                print(proc.stderr[-3000:], file=sys.stderr)
                sys.exit("leg %s failed (exit status %d): nothing more is run" % (leg, proc.returncode))
            rec = json.loads(proc.stdout.strip().splitlines()[-1])
            rec.update(round=rnd, what=LEGS[leg], pairs_per_s=rec["pairs"] / rec["seconds"])
            results.append(rec)
            print(json.dumps(rec), flush=True)
    summary = {}
    for leg in legs:
        runs = [r for r in results if r["leg"] == leg]
        rates, secs = [r["pairs_per_s"] for r in runs], [r["seconds"] for r in runs]
        summary[leg] = dict(what=LEGS[leg], pairs=runs[0]["pairs"], median_s=statistics.median(secs), min_s=min(secs), max_s=max(secs),
                            median_pairs_per_s=statistics.median(rates), min_pairs_per_s=min(rates), max_pairs_per_s=max(rates), runs=len(runs))
    out = dict(pairs=args.block * args.repeat, summary=summary, runs=results)
    print(json.dumps(out["summary"], indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not args.keep:
        for f in FILES:
            os.unlink(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
