#!/usr/bin/env python3
"""The streamed ingest on plain gzip input, decoded on the device, against its neighbours, on one GPU
(profiles/gzip_device.md).

Makes the inputs from a seed as tools/bgzf_legs.py does -- one block of --block pairs, 2 x 150 bp, its text repeated
--repeat times; the plain gzip form is that whole text written by zlib at level 6 as ONE member (what `gzip -6` writes;
--members: the block as one member, repeated as often, i.e. a file of concatenated members); the BGZF form is bgzf_legs'
-- and runs every leg as a fresh child process
(the child of bgzf_legs.py: from the FASTQ paths to counters on the device), under a time limit of its own.  The legs
alternate, --rounds rounds; the first leg that fails ends the run.  All legs must give the same counters (an untimed
property of every run: the digest of the counters, which do not depend on the order of the pairs).

    z  streamed plain gzip, inflated by zlib on the host (VS_FASTQ_STREAM=1): what the streamed ingest does without the switch
    g  streamed plain gzip, decoded on the device       (VS_GZIP_DEVICE=1)
    c  the same text as BGZF, inflated on the device
    a  streamed, plain text                             (VS_FASTQ_STREAM=1)

    python tools/gzip_legs.py [--out legs.json]
    python tools/gzip_legs.py --only g --rounds 1 --keep DIR     (one leg, e.g. under rocprofv3 ... -- python ...)

The summary says whether the median of g exceeds the median of z by more than the larger of the two legs' spreads.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bgzf_legs  # noqa: E402  (the child that runs one leg, and the inputs it shares)

LEGS = {
    "z": ("streamed plain gzip, host zlib (VS_FASTQ_STREAM=1)", "fq.gzip", {"VS_FASTQ_STREAM": "1"}),
    "g": ("streamed plain gzip, decoded on the device (VS_GZIP_DEVICE=1)", "fq.gzip", {"VS_GZIP_DEVICE": "1"}),
    "c": ("streamed BGZF, inflated on the device", "fq.gz", {}),
    "a": ("streamed, plain text", "fq", {"VS_FASTQ_STREAM": "1"}),
}
SWITCHES = ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK", "VS_GZIP_DEVICE", "VS_GZIP_TEXT")


def make_inputs(d, block, repeat, seed, members):
    sizes = bgzf_legs.make_inputs(d, block, repeat, seed)
    for tag in ("f", "r"):
        with open(os.path.join(d, tag + ".fq"), "rb") as fh:
            text = fh.read(sizes[tag + ".fq"] // repeat)  # one block
        path = os.path.join(d, tag + ".fq.gzip")
        with open(path, "wb") as fh:
            if members:  # the block as one member, repeated
                c = zlib.compressobj(6, zlib.DEFLATED, 31)
                member = c.compress(text) + c.flush()
                for _ in range(repeat):
                    fh.write(member)
            else:  # the whole text as ONE member, as `gzip -6` writes the file
                c = zlib.compressobj(6, zlib.DEFLATED, 31)
                for _ in range(repeat):
                    fh.write(c.compress(text))
                fh.write(c.flush())
        sizes[tag + ".fq.gzip"] = os.path.getsize(path)
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--only", default="zgca")
    ap.add_argument("--members", action="store_true", help="write the gzip input as --repeat concatenated members, not as one")
    ap.add_argument("--limit", type=int, default=240, help="seconds per leg")
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return bgzf_legs.run_leg(args.leg, None)
    tmp = None
    if args.keep:
        d = args.keep
        os.makedirs(d, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        d = tmp.name
    pairs = args.block * args.repeat
    if not os.path.exists(os.path.join(d, "gzip_sizes.json")):
        sizes = make_inputs(d, args.block, args.repeat, args.seed, args.members)
        with open(os.path.join(d, "gzip_sizes.json"), "w") as fh:
            json.dump(sizes, fh)
    sizes = json.load(open(os.path.join(d, "gzip_sizes.json")))
    legs = [l for l in args.only if l in LEGS]
    runs = {l: [] for l in legs}
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    failed = None
    for rnd in range(args.rounds):
        for l in legs:
            env = dict(base, BGZF_LEG_EXT=LEGS[l][1], **LEGS[l][2])
            try:
                proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", d], env=env, capture_output=True, text=True,
                                      timeout=args.limit, cwd=ROOT)
            except subprocess.TimeoutExpired:
                failed = "leg %s round %d: over %d s" % (l, rnd, args.limit)
                break
            line = [x for x in proc.stdout.splitlines() if x.startswith("LEG ")]
            if proc.returncode != 0 or not line:
                failed = "leg %s round %d: exit %d\n%s" % (l, rnd, proc.returncode, proc.stderr[-2000:])
                break
            res = json.loads(line[0][4:])
            res["pairs_per_s"] = pairs / res["seconds"]
            runs[l].append(res)
            print("round %d leg %s: %.3f s, %.3g pairs/s, %.0f MB  %s" % (rnd, l, res["seconds"], res["pairs_per_s"], res["rss_mb"], res["info"]),
                  flush=True)
        if failed:
            break
    digests = {r["digest"] for rs in runs.values() for r in rs}
    summary = dict(pairs=pairs, sizes=sizes, legs={}, same_counters=len(digests) == 1, failed=failed)
    for l, rs in runs.items():
        if rs:
            rates = sorted(r["pairs_per_s"] for r in rs)
            summary["legs"][l] = dict(what=LEGS[l][0], pairs_per_s=rates, median=rates[len(rates) // 2], spread=rates[-1] - rates[0],
                                      rss_mb=max(r["rss_mb"] for r in rs), info=rs[-1]["info"])
    if "g" in summary["legs"] and "z" in summary["legs"]:
        g, z = summary["legs"]["g"], summary["legs"]["z"]
        summary["g_beats_z"] = g["median"] - z["median"] > max(g["spread"], z["spread"])
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if tmp:
        tmp.cleanup()
    if failed:
        sys.exit(failed)
    if not summary["same_counters"]:
        sys.exit("the legs disagree on the counters")


if __name__ == "__main__":
    main()
