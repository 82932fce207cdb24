#!/usr/bin/env python3
"""The BAM ingest against the BGZF FASTQ ingest on one GPU, from open to the last block (profiles/bam_ingest.md).

Takes --block pairs of the bench stream of BASELINE configs[--config] (the device generator, unpacked to text), writes them
once as a BGZF FASTQ pair -- the route such reads took before BAM could be read -- and once as ONE collated BAM (every
second end stored reversed, the mates in alternating order, a supplementary record after every 64th pair), both with the
pure-Python BGZF writer of tests/bgzf_util.py at --level, the members of the block repeated --repeat times (concatenated
BGZF is BGZF; the BAM header and the end marker are written once).  Then two legs, alternating inside ONE process in the
order of --only, --rounds rounds, a warm page cache, a host clock from the open of the stream to the block after the last
(every block freed, the stream synchronised by the library before a block is handed out), after one untimed pass per leg
in which every block is downloaded -- both legs must deliver the same ends:

    f  pe.FastqStream on the pair      (k_inflate, k_sl_*, k_pack_reads<PackLines>)
    b  pe.BamStream on the BAM         (k_inflate, k_bam_exits / k_bam_walk / k_bam_count / k_bam_scatter, k_bam_couples,
                                        k_pack_reads<PackBam>)

No counting: the legs end where vs_pe_count would begin.  Prints one JSON line; --out writes it to a file as well.

    python tools/bam_ingest_legs.py --out bam_ingest.json

--by-name measures the mates matched by name instead (profiles/bam_by_name.md).  The records of the same block (written
once: a name occurs in one pair only) go into three BAM files -- "collated" as above, "near": the later mate of every pair
moved back by a random 0..2 000 records, as the proper pairs of a sorted alignment lie, and "far": a uniform shuffle of all
records -- and four legs alternate inside ONE process:

    c  pe.BamStream on the collated file                  (the collated mode, the yardstick)
    n  pe.BamStream(by_name=True) on the collated file    (k_mate_hash / _claim / _rank / _partner / _emit, k_mate_carry)
    m  ... on "near"
    x  ... on "far"

The untimed pass compares a sum over pairs of a hash of both ends, which no order of the pairs changes.

    python tools/bam_ingest_legs.py --by-name --out bam_by_name.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bam_ingest_legs.py --only b --rounds 1   (no counters in that run)
"""
import argparse
import hashlib
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_SEED = 77
LEGS = {"f": "BGZF FASTQ pair (FastqStream)", "b": "collated BAM (BamStream)"}
NAME_LEGS = {"c": ("collated BAM, collated mode", "collated.bam", False), "n": ("collated BAM, by name", "collated.bam", True),
             "m": ("near BAM, by name", "near.bam", True), "x": ("far BAM, by name", "far.bam", True)}


def bgzf_members(data: bytes, level: int) -> bytes:
    import bgzf_util as bz

    out = []
    for i in range(0, len(data), bz.MAX_IN if level else 0xFE00):
        out.append(bz.member(data[i:i + (bz.MAX_IN if level else 0xFE00)], level))
    return b"".join(out)


def fastq_bytes(text: np.ndarray, tag: bytes) -> bytes:
    """text: (n, L) uint8 of ACGT; records "@<tag><i>\\n<seq>\\n+\\n<qual>\\n" with names of one width"""
    n, L = text.shape
    names = np.frombuffer(b"".join(b"@%s%09d\n" % (tag, i) for i in range(n)), dtype=np.uint8).reshape(n, -1)
    middle = np.tile(np.frombuffer(b"\n+\n", dtype=np.uint8), (n, 1))
    return np.concatenate([names, text, middle, np.full((n, L), 73, np.uint8), np.full((n, 1), 10, np.uint8)], axis=1).tobytes()


def bam_records(fwd: np.ndarray, rve: np.ndarray, rows_out: bool = False):
    """the collated records of the pairs (n, L) + (n, L): fixed-width names, no cigar, no aux (``rows_out``: as an array of
    one record per row, all of one width, and which rows are the later mate of their pair)"""
    n, L = fwd.shape
    code = np.zeros(256, np.uint8)
    for c, v in zip(b"ACGT", (1, 2, 4, 8)):
        code[c] = v
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b

    def one(text, flag, rev):
        m = text.shape[0]
        t = comp[text[:, ::-1]] if rev else text
        nib = code[t]
        if L & 1:
            nib = np.concatenate([nib, np.zeros((m, 1), np.uint8)], axis=1)
        packed = (nib[:, 0::2] << 4) | nib[:, 1::2]
        names = np.frombuffer(b"".join(b"p%09d\0" % i for i in range(m)), dtype=np.uint8).reshape(m, 11)
        bs = 32 + 11 + packed.shape[1] + L
        fixed = struct.pack("<IiiBBHHHIiii", bs, -1, -1, 11, 0, 4680, 0, flag | (0x10 if rev else 0), L, -1, -1, 0)
        head = np.tile(np.frombuffer(fixed, dtype=np.uint8), (m, 1))
        return np.concatenate([head, names, packed, np.full((m, L), 40, np.uint8)], axis=1)

    a, b = one(fwd, 0x4D, False), one(rve, 0x8D, True)  # (paired, unmapped, mate unmapped; the second end stored reversed)
    width = a.shape[1]
    out = np.empty((n, 2, width), np.uint8)
    odd = (np.arange(n) & 1).astype(bool)
    out[~odd, 0], out[~odd, 1] = a[~odd], b[~odd]
    out[odd, 0], out[odd, 1] = b[odd], a[odd]  # (second before first in every other couple)
    if rows_out:
        sup_row = one(fwd[:1], 0x841, False)
        parts, later = [], []
        for i in range(0, n, 64):
            m = min(64, n - i)
            parts += [out[i:i + m].reshape(2 * m, width), sup_row]
            later += [np.tile(np.array([False, True]), m), np.array([False])]
        return np.concatenate(parts, axis=0), np.concatenate(later)
    sup = one(fwd[:1], 0x841, False).tobytes()  # a supplementary record, dropped by the ingest
    rows = out.reshape(n, 2 * width)
    parts = []
    for i in range(0, n, 64):
        parts.append(rows[i:i + 64].tobytes())
        parts.append(sup)
    return b"".join(parts)


def bench_ends(d, config, block):
    """the two ends (block, L) of the first `block` pairs of the bench stream"""
    from vstrains_amd import pe as host
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[config]
    st, pre, names, seqs, cum, logger, _ = workload_for(config, d)
    ctx = host.Context(0)
    blk = ctx.synth_pairs(st.genomes, cum, STREAM_SEED, 0, block, cfg["read_len"], int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    text, lens, flags = blk.unpack()
    blk.free()
    ctx.close()
    assert (lens == cfg["read_len"]).all()
    ends = np.asarray(text).reshape(2 * block, cfg["read_len"])
    return ends[0::2], ends[1::2]


def make_by_name_inputs(d, config, block, level):
    """collated.bam, near.bam, far.bam: the same records in three orders"""
    import bam_util as bu
    import bgzf_util as bz

    fwd, rve = bench_ends(d, config, block)
    rows, later = bam_records(fwd, rve, rows_out=True)
    rng = np.random.default_rng(STREAM_SEED)
    at = np.arange(len(rows), dtype=np.float64)
    orders = {"collated.bam": None,
              "near.bam": np.argsort(at + np.where(later, rng.integers(0, 2001, size=len(rows)) + 0.5, 0.0), kind="stable"),
              "far.bam": rng.permutation(len(rows))}
    head = bu.encode_header(b"@HD\tVN:1.6\tSO:unsorted\n")
    sizes = {}
    for name, order in orders.items():
        recs = (rows if order is None else rows[order]).tobytes()
        packed = bgzf_members(recs, level)
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(bz.member(head, level))
            fh.write(packed)
            fh.write(bz.EOF_MARK)
        sizes[name] = dict(file=len(packed) + 28, text=len(head) + len(recs), records=int(len(rows)))
    return sizes


def pair_sum(text, lens):
    """a sum over the pairs of a hash of both ends (uint64, wrapping): the same for every order of the same pairs"""
    L = int(lens[0]) if len(lens) else 0
    if not len(lens) or not (np.asarray(lens) == L).all():
        sys.exit("the by-name digest expects ends of one length")
    t = np.asarray(text).reshape(-1, 2 * L)
    mult = (np.random.default_rng(5).integers(1, 1 << 62, size=2 * L, dtype=np.uint64) << np.uint64(1)) | np.uint64(1)
    total = 0
    for lo in range(0, len(t), 1 << 15):  # (in slices: the products are eight times the text)
        h = (t[lo:lo + (1 << 15)].astype(np.uint64) * mult).sum(axis=1, dtype=np.uint64)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0x9E3779B97F4A7C15)
        total = (total + int(h.sum(dtype=np.uint64))) & ((1 << 64) - 1)
    return total


def run_name_leg(host, ctx, d, leg, block_pairs, digest):
    """one leg of --by-name from open to the end of the input: (seconds, pairs, info, order-free sum over the pairs or None)"""
    what, name, by_name = NAME_LEGS[leg]
    total = 0
    t0 = time.perf_counter()
    fs = host.BamStream(os.path.join(d, name), ctx, block_pairs=block_pairs, by_name=by_name)
    pairs = 0
    try:
        for block in fs:
            if digest:
                text, lens, flags = block.unpack()
                total = (total + pair_sum(text, lens)) & ((1 << 64) - 1)
            pairs += int(block.info["ends"]) // 2
            block.free()
        info = dict(fs.info)
    finally:
        fs.close()
    return time.perf_counter() - t0, pairs, info, total if digest else None


def by_name_main(args):
    from vstrains_amd import pe as host

    tmp = None
    if args.keep:
        d = args.keep
        os.makedirs(d, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        d = tmp.name
    if not os.path.exists(os.path.join(d, "sizes_by_name.json")):
        sizes = make_by_name_inputs(d, args.config, args.block, args.level)
        with open(os.path.join(d, "sizes_by_name.json"), "w") as fh:
            json.dump(sizes, fh)
    with open(os.path.join(d, "sizes_by_name.json")) as fh:
        sizes = json.load(fh)
    for name in sizes:  # (warm page cache)
        with open(os.path.join(d, name), "rb") as fh:
            while fh.read(1 << 24):
                pass
    ctx = host.Context(0)
    legs = [l for l in (args.only if args.only != "fb" else "cnmx") if l in NAME_LEGS]
    runs, order = {l: [] for l in legs}, []
    digests = {}
    for l in legs:  # untimed: every block downloaded, every leg must deliver the same pairs
        dt, pairs, info, digests[l] = run_name_leg(host, ctx, d, l, args.block_pairs, True)
        if pairs != args.block:
            sys.exit("leg %s delivered %d pairs of %d" % (l, pairs, args.block))
    for rnd in range(args.rounds):
        for l in legs:
            dt, pairs, info, _ = run_name_leg(host, ctx, d, l, args.block_pairs, False)
            if pairs != args.block:
                sys.exit("leg %s delivered %d pairs of %d" % (l, pairs, args.block))
            order.append(l)
            runs[l].append(dict(seconds=dt, pairs_per_s=pairs / dt, info=info))
            print("round %d leg %s: %.3f s, %.4g pairs/s  %s" % (rnd, l, dt, pairs / dt, info), flush=True)
    summary = dict(config=args.config, pairs=args.block, level=args.level, sizes=sizes, order="".join(order), legs={},
                   same_pairs=len(set(digests.values())) <= 1, single_run=True)
    for l, rs in runs.items():
        rates = sorted(r["pairs_per_s"] for r in rs)
        info = rs[-1]["info"]
        summary["legs"][l] = dict(what=NAME_LEGS[l][0], file=NAME_LEGS[l][1], pairs_per_s=rates, median=rates[len(rates) // 2], spread=rates[-1] - rates[0],
                                  waiting_max=info["waiting_max"], carried_bytes_max=info["carried_bytes_max"], windows=info["windows"],
                                  singletons=info["singletons"], info=info)
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if tmp:
        tmp.cleanup()
    if not summary["same_pairs"]:
        sys.exit("the legs disagree on the pairs")


def make_inputs(d, config, block, repeat, level):
    import bam_util as bu
    import bgzf_util as bz
    from vstrains_amd import pe as host
    from vstrains_amd.workloads import CONFIGS, workload_for

    cfg = CONFIGS[config]
    st, pre, names, seqs, cum, logger, _ = workload_for(config, d)
    ctx = host.Context(0)
    blk = ctx.synth_pairs(st.genomes, cum, STREAM_SEED, 0, block, cfg["read_len"], int(0.005 * 2 ** 32), int(0.001 * 2 ** 32))
    text, lens, flags = blk.unpack()
    blk.free()
    ctx.close()
    L = cfg["read_len"]
    assert (lens == L).all()
    ends = np.asarray(text).reshape(2 * block, L)
    fwd, rve = ends[0::2], ends[1::2]
    sizes = {}
    for name, data in (("f.fq.gz", fastq_bytes(fwd, b"f")), ("r.fq.gz", fastq_bytes(rve, b"r"))):
        packed = bgzf_members(data, level)
        with open(os.path.join(d, name), "wb") as fh:
            for _ in range(repeat):
                fh.write(packed)
            fh.write(bz.EOF_MARK)
        sizes[name] = dict(file=len(packed) * repeat + 28, text=len(data) * repeat)
    recs = bam_records(fwd, rve)
    packed = bgzf_members(recs, level)
    head = bu.encode_header(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n")
    with open(os.path.join(d, "reads.bam"), "wb") as fh:
        fh.write(bz.member(head, level))
        for _ in range(repeat):
            fh.write(packed)
        fh.write(bz.EOF_MARK)
    sizes["reads.bam"] = dict(file=len(packed) * repeat + 28, text=len(head) + len(recs) * repeat)
    return sizes


def run_leg(host, ctx, d, leg, block_pairs, digest):
    """one leg from open to the end of the input: (seconds, pairs, info, digest of all lengths and all text or None)"""
    h_len, h_text = (hashlib.sha256(), hashlib.sha256()) if digest else (None, None)
    t0 = time.perf_counter()
    if leg == "f":
        fs = host.FastqStream(os.path.join(d, "f.fq.gz"), os.path.join(d, "r.fq.gz"), ctx, block_pairs=block_pairs)
    else:
        fs = host.BamStream(os.path.join(d, "reads.bam"), ctx, block_pairs=block_pairs)
    pairs = 0
    try:
        for block in fs:
            if digest:  # (the two streams cut their blocks at different pairs: lengths and text hashed apart)
                text, lens, flags = block.unpack()
                h_len.update(np.ascontiguousarray(lens).tobytes())
                h_text.update(np.ascontiguousarray(text).tobytes())
            pairs += int(block.info["ends"]) // 2
            block.free()
        info = dict(fs.info)
    finally:
        fs.close()
    return time.perf_counter() - t0, pairs, info, h_len.hexdigest() + h_text.hexdigest() if digest else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--block", type=int, default=1 << 20, help="pairs taken from the bench stream")
    ap.add_argument("--repeat", type=int, default=10, help="times the block's members are written (10 x 2^20: the 10 M pairs of configs[2])")
    ap.add_argument("--level", type=int, default=1, help="zlib level of the members")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="fb", help="the legs and their order inside a round")
    ap.add_argument("--block-pairs", type=int, default=1 << 20)
    ap.add_argument("--keep", default=None, help="make (or reuse) the inputs in this directory")
    ap.add_argument("--out", default=None)
    ap.add_argument("--by-name", action="store_true", help="the by-name legs c, n, m, x on three orders of the block (--repeat is not used)")
    args = ap.parse_args()
    if args.by_name:
        return by_name_main(args)
    from vstrains_amd import pe as host

    tmp = None
    if args.keep:
        d = args.keep
        os.makedirs(d, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        d = tmp.name
    if not os.path.exists(os.path.join(d, "sizes.json")):
        sizes = make_inputs(d, args.config, args.block, args.repeat, args.level)
        with open(os.path.join(d, "sizes.json"), "w") as fh:
            json.dump(sizes, fh)
    with open(os.path.join(d, "sizes.json")) as fh:
        sizes = json.load(fh)
    for name in sizes:  # (warm page cache)
        with open(os.path.join(d, name), "rb") as fh:
            while fh.read(1 << 24):
                pass
    ctx = host.Context(0)
    legs = [l for l in args.only if l in LEGS]
    want = args.block * args.repeat
    runs, order = {l: [] for l in legs}, []
    # an untimed pass first: every block downloaded, both legs must deliver the same ends (it also warms both routes)
    digests = {l: run_leg(host, ctx, d, l, args.block_pairs, True)[3] for l in legs}
    for rnd in range(args.rounds):
        for l in legs:
            dt, pairs, info, _ = run_leg(host, ctx, d, l, args.block_pairs, False)
            if pairs != want:
                sys.exit("leg %s delivered %d pairs of %d" % (l, pairs, want))
            order.append(l)
            runs[l].append(dict(seconds=dt, pairs_per_s=pairs / dt, info=info))
            print("round %d leg %s: %.3f s, %.4g pairs/s  %s" % (rnd, l, dt, pairs / dt, info), flush=True)
    summary = dict(config=args.config, pairs=want, level=args.level, sizes=sizes, order="".join(order), legs={},
                   same_pairs=len(set(digests.values())) <= 1)
    for l, rs in runs.items():
        rates = sorted(r["pairs_per_s"] for r in rs)
        summary["legs"][l] = dict(what=LEGS[l], pairs_per_s=rates, median=rates[len(rates) // 2], spread=rates[-1] - rates[0],
                                  info=rs[-1]["info"])
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    if tmp:
        tmp.cleanup()
    if not summary["same_pairs"]:
        sys.exit("the legs disagree on the pairs")


if __name__ == "__main__":
    main()
