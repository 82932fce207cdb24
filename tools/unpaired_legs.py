#!/usr/bin/env python3
"""Reads per second of the one-file stream of unpaired reads (--single) on a BGZF file beside pairs per second of the
two-file BGZF stream on the same reads, on one GPU (profiles/unpaired.md).

Makes the inputs from a seed -- one block of --block pairs, 2 x 150 bp, compressed as BGZF, repeated --repeat times: 1 M
pairs by default -- as the pair r1.fq.gz / r2.fq.gz and as ONE file single.fq.gz that holds the records of both, and runs
every leg as a fresh child process under a time limit of its own: the stream opened, every block taken and freed (no
counting), from the open to the end of the input.  The legs alternate, --rounds rounds; the first leg that fails ends the run.

    s  pe.SingleEndStream on single.fq.gz (2 x pairs reads, singles blocks)
    f  pe.FastqStream on r1.fq.gz / r2.fq.gz

    python tools/unpaired_legs.py [--out legs.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = {"s": "one file of unpaired reads", "f": "two files of pairs"}
FILES = ("r1.fq.gz", "r2.fq.gz", "single.fq.gz")


def make_inputs(d, block, repeat, seed):
    import numpy as np

    import bgzf_util as bz

    rng = np.random.default_rng(seed)
    packed = []
    for which in (1, 2):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(block, 150))]
        text = b"".join(b"@read%d/%d\n%s\n+\n%s\n" % (k, which, seq[k].tobytes(), b"I" * 150) for k in range(block))
        packed.append(bz.bgzf(text, level=1, eof=False))
    for name, parts in (("r1.fq.gz", packed[:1]), ("r2.fq.gz", packed[1:]), ("single.fq.gz", packed)):
        with open(os.path.join(d, name), "wb") as fh:
            for part in parts:
                for _ in range(repeat):
                    fh.write(part)
            fh.write(bz.bgzf(b""))  # (the empty member that ends a BGZF file)


def run_leg(d, leg):
    """(child) one leg"""
    from vstrains_amd import pe as host

    ctx = host.Context(0)
    t0 = time.perf_counter()
    if leg == "s":
        fs = host.SingleEndStream(os.path.join(d, "single.fq.gz"), ctx)
    else:
        fs = host.FastqStream(os.path.join(d, "r1.fq.gz"), os.path.join(d, "r2.fq.gz"), ctx)
    blocks = 0
    for block in fs:
        block.free()
        blocks += 1
    ctx.sync()
    dt = time.perf_counter() - t0
    info = fs.info
    fs.close()
    print(json.dumps(dict(leg=leg, seconds=dt, units=info["reads"] if leg == "s" else info["pairs"], unit="reads" if leg == "s" else "pairs",
                          blocks=blocks, text_bytes=info["text_bytes"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="sf")
    ap.add_argument("--limit", type=int, default=120, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.dir, args.leg)
    legs = [l for l in args.only if l in LEGS]
    d = tempfile.mkdtemp(prefix="unpaired_legs_")
    try:
        make_inputs(d, args.block, args.repeat, args.seed)
        results = []
        for rnd in range(args.rounds):
            for leg in legs:
                proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--dir", d], capture_output=True, text=True,
                                      timeout=args.limit)
                if proc.returncode != 0:
                    print(proc.stderr[-3000:], file=sys.stderr)
                    sys.exit("leg %s failed (exit status %d): nothing more is run" % (leg, proc.returncode))
                rec = json.loads(proc.stdout.strip().splitlines()[-1])
                rec.update(round=rnd, what=LEGS[leg], units_per_s=rec["units"] / rec["seconds"])
                results.append(rec)
                print(json.dumps(rec), flush=True)
        summary = {}
        for leg in legs:
            rates = [r["units_per_s"] for r in results if r["leg"] == leg]
            summary[leg] = dict(what=LEGS[leg], unit=[r["unit"] for r in results if r["leg"] == leg][0] + "/s", median=statistics.median(rates),
                                min=min(rates), max=max(rates), runs=len(rates))
        out = dict(pairs=args.block * args.repeat, reads=2 * args.block * args.repeat, summary=summary, runs=results)
        print(json.dumps(out["summary"], indent=1))
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)
    finally:
        for f in FILES:
            if os.path.exists(os.path.join(d, f)):
                os.unlink(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
