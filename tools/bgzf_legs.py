#!/usr/bin/env python3
"""The streamed ingest on BGZF input against its neighbours, on one GPU (profiles/stream_ingest.md, "BGZF").

Makes the inputs from a seed -- one block of --block pairs, 2 x 150 bp, its text repeated --repeat times, its BGZF form
(level 6, the pure-Python writer of tests/bgzf_util.py) repeated as often: concatenated BGZF files are BGZF -- and runs
every leg as a fresh child process, from the FASTQ paths to counters on the device (pe_inference.count_links: GFA read,
index build, ingest with counting), under a time limit of its own.  The legs alternate, --rounds rounds; the first leg
that fails ends the run.  All legs must give the same counters.

    a  streamed, plain text                      (VS_FASTQ_STREAM=1)
    b  streamed BGZF, inflated by zlib on the host (VS_BGZF_DEVICE=0): what the streamed ingest did before
    c  streamed BGZF, inflated on the device
    d  mapped BGZF                               (VS_FASTQ_STREAM=0: inflated whole at open)
    p  leg b on another build of the library (--parent-lib, e.g. tools/_ab/parent.so of tools/ab_build.sh)
    q  leg c on that other build (needs --parent-lib; a build that has the device inflate)
    s  sharded BGZF: --ranks processes under torchrun on ONE device over gloo, the files shared by member and inflated
       on the device (FastqStream.open_shard); seconds = the slowest rank's wall time from the FASTQ paths to the summed
       counters, rss_mb = the ranks' peak RSS added up.  Ranks sharing one GPU say nothing about scaling.  (Not measured yet:
       profiles/stream_ingest.md, "Sharded BGZF", says what is to be reported.)
    t  the same run on the other build (needs --parent-lib): what a sharded run did before, every rank inflating both
       whole files with zlib at the open (VS_BGZF_DEVICE=0 keeps the new open out of the way)

    python tools/bgzf_legs.py [--out legs.json]
    python tools/bgzf_legs.py --only c --rounds 1 --keep DIR     (one leg, e.g. under rocprofv3 ... -- python ...)
"""
import argparse
import hashlib
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = {
    "a": ("streamed, plain text", "fq", {"VS_FASTQ_STREAM": "1"}),
    "b": ("streamed BGZF, host zlib (VS_BGZF_DEVICE=0)", "fq.gz", {"VS_FASTQ_STREAM": "1", "VS_BGZF_DEVICE": "0"}),
    "c": ("streamed BGZF, inflated on the device", "fq.gz", {}),
    "d": ("mapped BGZF (VS_FASTQ_STREAM=0)", "fq.gz", {"VS_FASTQ_STREAM": "0"}),
    "p": ("streamed BGZF on the other build of the library", "fq.gz", {"VS_FASTQ_STREAM": "1"}),
    "q": ("streamed BGZF, inflated on the device, on the other build of the library", "fq.gz", {}),
    "s": ("sharded BGZF by member, device inflate, ranks on one GPU over gloo", "fq.gz", {}),
    "t": ("sharded BGZF on the other build: whole-file zlib open on every rank", "fq.gz", {"VS_BGZF_DEVICE": "0"}),
}
OTHER_BUILD = "pqt"  # legs that run on --parent-lib
SHARDED = "st"       # legs that run under torchrun
NEW_ENTRIES = ("vs_bgzf_walk_file", "vs_bgzf_count_lines", "vs_inflate_count_host", "vs_bgzf_shard_plan", "vs_fastq_stream_open_range")
K = 55


def make_inputs(d, block, repeat, seed):
    import bgzf_util as bz
    from vstrains_amd import synth

    st = synth.make_strains(6, 3000, 0.02, seed=seed)
    g = synth.compact_dbg(st, K)
    with open(os.path.join(d, "graph.gfa"), "w") as fh:
        fh.write(g.gfa_text())
    f, r = synth.sample_pairs(st, block, 150, seed=seed + 1, sub_rate=0.005)
    sizes = {}
    for tag, reads in (("f", f), ("r", r)):
        text = synth.fastq_text(reads, tag).encode()
        packed = bz.bgzf(text, level=6, eof=False)
        for ext, data in (("fq", text), ("fq.gz", packed)):
            with open(os.path.join(d, "%s.%s" % (tag, ext)), "wb") as fh:
                for _ in range(repeat):
                    fh.write(data)
            sizes["%s.%s" % (tag, ext)] = len(data) * repeat
    return sizes


def run_leg(d, lib):
    """(child) one leg: the environment says which"""
    from vstrains_amd import _native as nat

    if lib:  # another build of the library: without the entries it does not have
        nat.LIB_PATH = lib
        import ctypes

        import torch  # noqa: F401  (first, as _native.lib() does: the build must bind to the HIP runtime torch brings)

        have = ctypes.CDLL(lib)
        for name in ("vs_bgzf_walk", "vs_inflate_host", "vs_inflate_bgzf", "vs_fastq_stream_inflate_info") + NEW_ENTRIES:
            if not hasattr(have, name):
                nat.SYMBOLS.pop(name, None)
    import numpy as np

    from vstrains_amd import pe as host
    from vstrains_amd import pe_inference

    ext = os.environ["BGZF_LEG_EXT"]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:  # (a sharded leg: the ranks share device 0, the counters are summed over gloo)
        import torch.distributed as dist

        os.environ.setdefault("VS_DIST_BACKEND", "gloo")
        dist.init_process_group("gloo")
    ctx = host.Context(0)
    info = {}
    if lib and "vs_fastq_stream_inflate_info" not in nat.SYMBOLS:  # (that build has no member counts to report)
        import ctypes as C

        def plain_info(self):
            a = (C.c_uint64 * 4)()
            nat.lib().vs_fastq_stream_info(self._h, a)
            return dict(pairs=int(a[0]), text_bytes=int(a[1]), file_bytes=int(a[2]), flags=int(a[3]))

        host.FastqStream.info = property(plain_info)
    else:
        close = host.FastqStream.close

        def closing(self):
            if self._h:
                info.update(self.info)
            close(self)

        host.FastqStream.close = closing
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull  # (the held progress lines)
    t0 = time.perf_counter()
    ids, counter = pe_inference.count_links(ctx, os.path.join(d, "graph.gfa"), os.path.join(d, "f." + ext), os.path.join(d, "r." + ext), K)
    ctx.sync()
    dt = time.perf_counter() - t0
    sys.stdout = stdout
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, (dt, rss))
        dt, rss = max(e[0] for e in every), sum(e[1] for e in every)
        info = dict(ranks=world, rss_mb_per_rank=[round(e[1]) for e in every])
        if dist.get_rank() != 0:
            dist.barrier()
            return
    node, short, stats = counter.result()
    h = hashlib.sha256(np.ascontiguousarray(node).tobytes() + np.ascontiguousarray(short).tobytes() + repr(stats).encode()).hexdigest()
    print("LEG " + json.dumps(dict(seconds=dt, rss_mb=rss, digest=h, node_sum=int(node.sum()), info={k: v for k, v in info.items()})))
    if world > 1:
        dist.barrier()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ranks", type=int, default=2, help="processes of the sharded legs s and t (at most 8: they share one GPU)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per leg")
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.leg, os.environ.get("BGZF_LEG_LIB"))
    tmp = None
    if args.keep:
        d = args.keep
        os.makedirs(d, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        d = tmp.name
    pairs = args.block * args.repeat
    if not os.path.exists(os.path.join(d, "sizes.json")):
        sizes = make_inputs(d, args.block, args.repeat, args.seed)
        with open(os.path.join(d, "sizes.json"), "w") as fh:
            json.dump(sizes, fh)
    sizes = json.load(open(os.path.join(d, "sizes.json")))
    legs = [l for l in args.only if l in LEGS and (l not in OTHER_BUILD or args.parent_lib)]
    if args.parent_lib and args.only == "abcd":
        legs.append("p")
    if not 1 < args.ranks <= 8 and any(l in SHARDED for l in legs):
        sys.exit("--ranks must be 2 .. 8")
    runs = {l: [] for l in legs}
    base = {k: v for k, v in os.environ.items() if k not in ("VS_FASTQ_STREAM", "VS_BGZF_DEVICE", "VS_STREAM_CHUNK")}
    failed = None
    for rnd in range(args.rounds):
        for l in legs:
            env = dict(base, BGZF_LEG_EXT=LEGS[l][1], **LEGS[l][2])
            if l in OTHER_BUILD:
                env["BGZF_LEG_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable]
            if l in SHARDED:
                import socket

                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    port = sk.getsockname()[1]
                cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.ranks), "--master-addr", "127.0.0.1",
                        "--master-port", str(port)]
                env.update(VS_DIST_BACKEND="gloo", VS_DIST_DEVICE="0")
            try:
                proc = subprocess.run(cmd + [os.path.abspath(__file__), "--leg", d], env=env, capture_output=True, text=True,
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
