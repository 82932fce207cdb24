#!/usr/bin/env python3
"""Wall time of the three passes of the member-sharded interleaved ingest (`pe.InterleavedStream.open_shard`) per rank, with
W = 1, 2, 4, 8 ranks SHARING one GPU, against the single-process interleaved stream on the same file (profiles/interleaved_shard.md).
Ranks on one GPU say nothing about scaling; what the legs show is what each pass costs and how many members it inflates.

Makes the input from a seed -- one block of --block pairs, 2 x 150 bp, named as `samtools fastq` names mates (one name, /1 and
/2), interleaved, written as BGZF members of 65 280 text bytes (zlib level 1) and repeated --repeat times: 4 M pairs by default.
Every leg is a set of fresh child processes under a time limit of its own; the first leg that fails ends the run.

    s   one process, pe.InterleavedStream on the file (strict), every block taken and freed, nothing counted
    p   leg s on another build of the library (--parent-lib, e.g. tools/_ab/parent.so of tools/ab_build.sh)
    W   W processes over gloo, each: shard_count, exchange, shard_tail, exchange, shard_open, every block taken and freed

    python tools/interleaved_shard_legs.py [--parent-lib tools/_ab/parent.so] [--out legs.json]
"""
import argparse
import json
import os
import socket
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_ENTRIES = ("vs_fastq_il_range_fn", "vs_il_shard_plan", "vs_fastq_il_open_range")
EOF_MARK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def make_input(path, block, repeat, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(2 * block, 150))]
    text = b"".join(b"@read%d/%d\n%s\n+\n%s\n" % (k >> 1, 1 + (k & 1), seq[k].tobytes(), b"I" * 150) for k in range(2 * block))
    members = b"".join(bgzf_member(text[i:i + 65280]) for i in range(0, len(text), 65280))
    with open(path, "wb") as fh:
        for _ in range(repeat):
            fh.write(members)
        fh.write(EOF_MARK)
    return len(text) * repeat


def other_library(lib):
    from vstrains_amd import _native as nat

    nat.LIB_PATH = lib
    for name in NEW_ENTRIES:
        nat.SYMBOLS.pop(name, None)


def drain(fs, ctx):
    blocks = 0
    for block in fs:
        block.free()
        blocks += 1
    ctx.sync()
    return blocks


def run_single(path, lib):
    """(child) leg s / p"""
    if lib:
        other_library(lib)
    from vstrains_amd import pe as host

    ctx = host.Context(0)
    t0 = time.perf_counter()
    fs = host.InterleavedStream(path, ctx)
    blocks = drain(fs, ctx)
    dt = time.perf_counter() - t0
    info = fs.info
    fs.close()
    print(json.dumps(dict(seconds=dt, pairs=info["pairs"], records=info["records"], blocks=blocks, text_bytes=info["text_bytes"])))


def run_rank(path):
    """(child) one rank of leg W: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT from the environment"""
    import torch.distributed as dist

    from vstrains_amd import pe as host

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    ctx = host.Context(0)

    def all_gather(vals):
        got = [None] * world
        dist.all_gather_object(got, [int(v) for v in vals])
        return got

    IS = host.InterleavedStream
    dist.barrier()
    t = [time.perf_counter()]
    mine = IS.shard_count(path, ctx, rank, world)
    t.append(time.perf_counter())
    everyone = all_gather(mine.message)
    t.append(time.perf_counter())
    why = IS.shard_tail(mine, everyone)
    if why is not None:
        sys.exit("the file is not shared: " + why)
    t.append(time.perf_counter())
    tails = all_gather(mine.tail_message)
    t.append(time.perf_counter())
    fs, _ = IS.shard_open(mine, tails, all_gather)
    blocks = drain(fs, ctx)
    t.append(time.perf_counter())
    info = fs.info
    rec = dict(rank=rank, world=world, count_s=t[1] - t[0], wait1_s=t[2] - t[1], tail_s=t[3] - t[2], wait2_s=t[4] - t[3], open_and_stream_s=t[5] - t[4],
               total_s=t[5] - t[0], pairs=info["pairs"], records=info["records"], blocks=blocks, members=fs.members, members_pass1=fs.members_pass1,
               members_tail=fs.members_tail, members_pass3=fs.plan[2] - fs.plan[0], entry=fs.entry)
    fs.close()
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps(rec))


def leg_single(path, lib, limit):
    env = dict(os.environ)
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "p" if lib else "s", "--file", path] + (["--parent-lib", lib] if lib else []),
                          env=env, capture_output=True, text=True, timeout=limit)
    if proc.returncode != 0:
        print(proc.stderr[-3000:], file=sys.stderr)
        sys.exit("the single-process leg failed (exit status %d): nothing more is run" % proc.returncode)
    return json.loads(proc.stdout.strip().splitlines()[-1])


def leg_world(path, world, limit):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "rank", "--file", path], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    out, failed = [], None
    deadline = time.time() + limit
    for rank, proc in enumerate(procs):
        try:
            so, se = proc.communicate(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            failed = "rank %d ran into the time limit" % rank
            break
        if proc.returncode != 0:
            failed = "rank %d failed (exit status %d)\n%s" % (rank, proc.returncode, se[-3000:])
            break
        out.append(json.loads(so.strip().splitlines()[-1]))
    if failed:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
                proc.communicate()
        sys.exit(failed + ": nothing more is run")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--keep", default=None, help="make (or reuse) the input in this directory")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--file", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "rank":
        return run_rank(args.file)
    if args.child:
        return run_single(args.file, os.path.abspath(args.parent_lib) if args.child == "p" else None)
    worlds = [int(w) for w in args.worlds.split(",") if w]
    if max(worlds) > 8:
        sys.exit("at most 8 ranks share the GPU")
    d = args.keep or tempfile.mkdtemp(prefix="il_shard_legs_")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "il.fq.gz")
    if not os.path.exists(path):
        text_bytes = make_input(path, args.block, args.repeat, args.seed)
        print(json.dumps(dict(input=path, pairs=args.block * args.repeat, text_bytes=text_bytes, file_bytes=os.path.getsize(path))), flush=True)
    runs = []
    for rnd in range(args.rounds):
        for leg in ["s"] + (["p"] if args.parent_lib else []) + worlds:
            if leg in ("s", "p"):
                rec = dict(leg=leg, round=rnd, **leg_single(path, os.path.abspath(args.parent_lib) if leg == "p" else None, args.limit))
            else:
                ranks = leg_world(path, leg, args.limit)
                rec = dict(leg="W%d" % leg, round=rnd, ranks=ranks, seconds=max(r["total_s"] for r in ranks), pairs=sum(r["pairs"] for r in ranks),
                           records=sum(r["records"] for r in ranks))
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    summary = {}
    for leg in sorted({r["leg"] for r in runs}):
        mine = [r for r in runs if r["leg"] == leg]
        summary[leg] = dict(median_seconds=statistics.median(r["seconds"] for r in mine), min=min(r["seconds"] for r in mine), max=max(r["seconds"] for r in mine),
                            runs=len(mine))
        if leg.startswith("W"):
            ranks = [x for r in mine for x in r["ranks"]]
            for key in ("count_s", "tail_s", "open_and_stream_s"):
                summary[leg][key + "_median_over_ranks_and_runs"] = statistics.median(x[key] for x in ranks)
            summary[leg]["tail_over_count_max"] = max(x["tail_s"] / x["count_s"] for x in ranks if x["count_s"] > 0)
            for key in ("members_pass1", "members_tail", "members_pass3"):
                summary[leg][key + "_sum"] = sum(x[key] for x in mine[0]["ranks"])
            summary[leg]["members"] = mine[0]["ranks"][0]["members"]
    out = dict(pairs=args.block * args.repeat, same_pairs_in_every_leg=len({r["pairs"] for r in runs}) == 1, summary=summary, runs=runs)
    print(json.dumps(out["summary"], indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not args.keep:
        os.unlink(path)
        os.rmdir(d)


if __name__ == "__main__":
    main()
