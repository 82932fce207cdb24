#!/usr/bin/env python3
"""Pairs per second of the interleaved FASTQ ingest against the two-file stream on the same reads, on one GPU
(profiles/interleaved.md).

Makes the inputs from a seed -- one block of --block pairs, 2 x 150 bp, named as `samtools fastq` names mates (one name, /1
and /2), its text repeated --repeat times: 4 M pairs by default -- as ONE interleaved file and as the de-interleaved pair, and
runs every leg as a fresh child process under a time limit of its own: the stream opened, every block taken and freed (no
counting), from the open to the end of the input.  The legs alternate, --rounds rounds; the first leg that fails ends the run.

    i  pe.InterleavedStream on the interleaved file (strict: the mates checked by name on the device)
    f  pe.FastqStream on the de-interleaved pair
    p  leg f on another build of the library (--parent-lib, e.g. tools/_ab/parent.so of tools/ab_build.sh)

    python tools/interleaved_legs.py [--parent-lib tools/_ab/parent.so] [--out legs.json]
    python tools/interleaved_legs.py --only i --rounds 1 --block 100000 --repeat 4      (one leg, e.g. under rocprofv3 ... -- python ...)
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

LEGS = {"i": "interleaved file, mates by name", "f": "two files", "p": "two files on the other build of the library"}
NEW_ENTRIES = ("vs_fastq_il_open", "vs_fastq_il_next", "vs_fastq_il_info", "vs_fastq_il_close", "vs_fastq_mates_host", "vs_fastq_mates_text")


def make_inputs(d, block, repeat, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    texts = []
    for which in (1, 2):
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(block, 150))]
        texts.append([b"@read%d/%d\n%s\n+\n%s\n" % (k, which, seq[k].tobytes(), b"I" * 150) for k in range(block)])
    both = b"".join(a + b for a, b in zip(texts[0], texts[1]))
    with open(os.path.join(d, "il.fq"), "wb") as fh:
        for _ in range(repeat):
            fh.write(both)
    for name, recs in (("r1.fq", texts[0]), ("r2.fq", texts[1])):
        one = b"".join(recs)
        with open(os.path.join(d, name), "wb") as fh:
            for _ in range(repeat):
                fh.write(one)


def run_leg(d, leg, lib):
    """(child) one leg"""
    from vstrains_amd import _native as nat

    if lib:  # another build of the library: without the entries it does not have
        nat.LIB_PATH = lib
        for name in NEW_ENTRIES:
            nat.SYMBOLS.pop(name, None)
    from vstrains_amd import pe as host

    ctx = host.Context(0)
    t0 = time.perf_counter()
    if leg == "i":
        fs = host.InterleavedStream(os.path.join(d, "il.fq"), ctx)
    else:
        fs = host.FastqStream(os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"), ctx)
    blocks = 0
    for block in fs:
        block.free()
        blocks += 1
    ctx.sync()
    dt = time.perf_counter() - t0
    info = fs.info
    fs.close()
    print(json.dumps(dict(leg=leg, seconds=dt, pairs=info["pairs"], blocks=blocks, text_bytes=info["text_bytes"], singles=info.get("singles", 0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="if")
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.dir, args.leg, os.environ.get("IL_LEG_LIB"))
    legs = [l for l in args.only + ("p" if args.parent_lib and "p" not in args.only else "") if l in LEGS and (l != "p" or args.parent_lib)]
    d = args.keep or tempfile.mkdtemp(prefix="il_legs_")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(os.path.join(d, "il.fq")):
        make_inputs(d, args.block, args.repeat, args.seed)
    results = []
    for rnd in range(args.rounds):
        for leg in legs:
            env = dict(os.environ)
            if leg == "p":
                env["IL_LEG_LIB"] = os.path.abspath(args.parent_lib)
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
        rates = [r["pairs_per_s"] for r in results if r["leg"] == leg]
        summary[leg] = dict(what=LEGS[leg], median_pairs_per_s=statistics.median(rates), min=min(rates), max=max(rates), runs=len(rates))
    pairs = {r["pairs"] for r in results}
    out = dict(pairs=args.block * args.repeat, same_pairs_in_every_leg=len(pairs) == 1, summary=summary, runs=results)
    print(json.dumps(out["summary"], indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not args.keep:
        for f in ("il.fq", "r1.fq", "r2.fq"):
            os.unlink(os.path.join(d, f))
        os.rmdir(d)


if __name__ == "__main__":
    main()
