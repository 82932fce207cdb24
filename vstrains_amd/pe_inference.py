#!/usr/bin/env python3
"""Drop-in for the reference's ``utils/VStrains_PE_Inference.py`` (same argv, same files, same
stdout lines; reference lines cited inline), running on MI355X through libvstrains_hip.so.

    python -m vstrains_amd.pe_inference -g s_graph_L1.gfa -o OUT/aln -f fwd.fq -r rve.fq -k 55
"""
import argparse
import os
import shutil
import stat
import sys
import time

from . import pe as host

BATCH_PAIRS = 1 << 20


def _rank_world():
    try:
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return 0, 1


def count_links(ctx, gfa: str, fwd: str, rve: str, kmer_size: int, stages_follow: bool = False, bam_by_name: bool = False, interleaved=None,
                check_names=None, single=(), count_singles: bool = False, interleaved_shard: bool = False):
    """Index the nodes of ``gfa`` and count every pair of the two FASTQ files; the counters stay
    on the device.  Returns ``(node ids in file order, PeCounter)``.  ``stages_follow``: the graph stages will build their
    PE-link table from these counters in this process (the pipeline; not the stand-alone script, which writes the two text
    files) -- the table's device buffer is then set aside together with the counters.  ``bam_by_name``: the inputs are ONE
    BAM in any record order, its mates matched by name (``BamStream(by_name=True)``); ``count_links.bam_info`` is then the
    stream's ``info`` (``singletons`` among it), else None.  ``interleaved`` (None, ``"strict"`` or ``"singles"``): the inputs
    are ONE interleaved FASTQ, each pair's two records one behind the other, the mates checked by name on the device
    (``InterleavedStream``; ``"singles"`` drops and counts the records without a mate, ``"strict"`` refuses the first);
    ``count_links.interleaved_info`` is then the stream's ``info``, else None.  ``interleaved_shard``: under a process group
    the ranks share that file by member (``InterleavedStream.open_shard``), each counting the pairs whose first record lies
    in its share of the records; ``interleaved_info`` then holds the ranks' SUMS of ``pairs``, ``singles`` and ``records`` on
    every rank.  ``check_names`` (None, ``"strict"`` or
    ``"singles"``): the two FASTQ files are paired by read name on the device (``PairedNameStream``, whatever ``use_stream``
    says; ``"strict"`` refuses the first pair that is no pair of mates, ``"singles"`` joins the files by name and drops and
    counts the records without a mate); ``count_links.pair_names_info`` is then the stream's ``info``, else None.
    ``single``: files of UNPAIRED reads (the unpaired survivors of a trimmer, merged reads), each streamed into the same
    counter after the pairs (``SingleEndStream``); ``count_singles``: the single records of the interleaved FASTQ
    (``interleaved="singles"``), the records without a mate of the two files joined by name (``check_names="singles"``) or the
    singletons of the BAM (``bam_by_name``) are kept and counted instead of dropped.  An unpaired read is worth what the reference gives
    one end of a pair: its own triangle of ``short_mat``, nothing in ``node_mat``; its tallies go to
    ``PeCounter.single_stats``, apart from the pairs'.  ``count_links.single_info`` is the list of per-file dicts (``path``,
    ``reads``, ``with_n``, ``short``, ``used``), the kept records' first under ``count_singles``: one entry for the interleaved
    file or the BAM, one entry with ``path = "FWD + RVE"`` for the two files joined by name (their blocks alternate per round;
    the per-file kept counts are ``pair_names_info``'s ``singles_fwd`` / ``singles_rve``)."""
    rank, world = _rank_world()
    inp = _resolve_inputs(fwd, rve, world, bam_by_name, interleaved, check_names, single, count_singles, interleaved_shard)
    ids, seqs = host.read_gfa_segments(gfa)  # :100-112
    ctx.build_index(seqs, kmer_size)  # :114-135  (KeyError on a bad node base, as :13)
    counter = host.PeCounter(ctx)

    feed_counter(ctx, counter, inp, rank, world, stages_follow=stages_follow)
    if world > 1:
        counter.all_reduce()  # (every rank ends with the full sums; only rank 0 writes the files and runs the stages)
    return ids, counter


def _resolve_inputs(fwd, rve, world, bam_by_name, interleaved, check_names, single, count_singles, interleaved_shard):
    """Which ingest reads the inputs of ``count_links``, decided (and what the flags cannot apply to refused with a
    ``ValueError``) before a device is opened or the graph is read."""
    count_links.bam_info = None
    count_links.interleaved_info = None
    count_links.pair_names_info = None
    count_links.single_info = []
    single = unpaired_input(single, count_singles, world, interleaved, check_names=check_names, bam_by_name=bam_by_name, fwd=fwd,
                            rve=rve)  # (what the flags cannot apply to is a ValueError)
    by_names = check_names_input(fwd, rve, world, check_names, bam_by_name=bam_by_name, interleaved=interleaved)  # (False without the flag)
    il_path = interleaved_input(fwd, rve, world, interleaved, shard=interleaved_shard)  # (None without the flag; what it cannot apply to is a ValueError)
    why = gzip_device_refusal(world)  # (reads the environment only; None with the switch unset)
    if why is not None:
        raise ValueError(why)
    bam = None if il_path or by_names else bam_input(fwd, rve, world, by_name=bam_by_name, sharded=not bam_by_name)  # (a collated BAM is shared by member)
    streamed = bam is None and not il_path and not by_names and use_stream(fwd, rve)
    if world > 1 and not (_regular(fwd) and _regular(rve)):  # (the sharded path maps regular files; VS_FASTQ_STREAM aside)
        raise ValueError("the FASTQ inputs %s / %s are not both regular files: a pipe can be read by one process only, so "
                         "the sharded (torchrun) run cannot take it; run one process, or write the reads to files" % (fwd, rve))
    return dict(fwd=fwd, rve=rve, single=single, by_names=by_names, il_path=il_path, bam=bam, streamed=streamed, bam_by_name=bam_by_name,
                interleaved=interleaved, check_names=check_names, count_singles=count_singles)


def feed_counter(ctx, counter, inp, rank: int = 0, world: int = 1, stages_follow: bool = False, tally_singles: bool = True):
    """Every block the chosen input delivers through ``counter.add`` -- a ``PeCounter`` (``count_links``) or a
    ``DepthCounter`` (``node_depth.depth_pass``, one process, ``tally_singles=False``: it keeps no tallies of unpaired reads).
    ``inp``: what ``_resolve_inputs`` decided."""
    fwd, rve, single, by_names, il_path, bam, streamed = (inp[k] for k in ("fwd", "rve", "single", "by_names", "il_path", "bam", "streamed"))
    bam_by_name, interleaved, check_names, count_singles = (inp[k] for k in ("bam_by_name", "interleaved", "check_names", "count_singles"))
    print("Start aligning reads to gfa nodes")  # :146
    # one process per GPU (torchrun): this rank counts its contiguous block of the pairs and the
    # counters are summed over ranks afterwards (RCCL all-reduce); a single process takes everything
    if rank == 0 and stages_follow:
        counter.reserve_link_table()  # (the graph stages run on this rank: their table's buffer is taken now)
    if il_path and world > 1:
        count_interleaved_shard(ctx, il_path, counter, rank, world, interleaved == "singles")
        fq = None
    elif il_path:
        fq = host.InterleavedStream(il_path, ctx, block_pairs=BATCH_PAIRS,
                                    singles="keep" if count_singles else (interleaved == "singles"))  # one file, opened once
        try:
            count_stream(ctx, fq, counter, progress=True)
            count_links.interleaved_info = fq.info
        finally:
            fq.close()
        if count_singles and tally_singles:
            count_links.single_info.append(_single_tally(il_path, counter, (0, 0, 0)))
    elif by_names:
        fq = host.PairedNameStream(fwd, rve, ctx, block_pairs=BATCH_PAIRS,
                                   singles="keep" if count_singles else (check_names == "singles"))  # both files, each read once
        try:
            count_stream(ctx, fq, counter, progress=True)
            count_links.pair_names_info = info = fq.info
        finally:
            fq.close()
        if check_names == "singles":
            print("Pairs joined by read name: %d; records without a mate %s: %d of %s, %d of %s"
                  % (info["pairs"], "counted as unpaired reads" if count_singles else "dropped", info["singles_fwd"], fwd, info["singles_rve"], rve))
        if count_singles and tally_singles:
            count_links.single_info.append(_single_tally("%s + %s" % (fwd, rve), counter, (0, 0, 0)))
    elif bam is not None and world > 1:
        # one collated whole-BGZF BAM: the ranks share it by member, summarise their shares for every entry the previous share
        # could hand them, and each streams its own couples (BamStream.open_shard); why == the reason when rank 0 reads the
        # whole file instead, as the single process does and in its words, and the others only join the sum
        why = "VS_BGZF_DEVICE=0" if os.environ.get("VS_BGZF_DEVICE") == "0" else None
        fq = None
        if why is None:
            fq, why = host.BamStream.open_shard(bam, ctx, rank, world, block_pairs=BATCH_PAIRS)
        if fq is not None:
            try:
                count_stream(ctx, fq, counter, progress=(rank == 0))
                info = fq.info
            finally:
                fq.close()
            if info["pairs"] != fq.pairs:
                raise RuntimeError("%s: %d pairs in the member range of rank %d where its plan says %d (did the file change?)"
                                   % (bam, info["pairs"], rank, fq.pairs))
            ingest_report(rank, world, "bam_members", None, fq.first_pair, info["pairs"], [fq.members], (fq.members_pass1,), (info["members_device"],))
        elif rank == 0:
            fq = host.BamStream(bam, ctx, block_pairs=BATCH_PAIRS)
            try:
                count_stream(ctx, fq, counter, progress=True)
                info = fq.info
            finally:
                fq.close()
            ingest_report(rank, world, "bam_whole_file_rank0", why, 0, info["pairs"], None, (0,), (info["members_device"],))
        else:
            ingest_report(rank, world, "bam_whole_file_rank0", why, 0, 0, None, (0,), (0,))
    elif bam is not None:
        fq = host.BamStream(bam, ctx, block_pairs=BATCH_PAIRS, by_name=bam_by_name,
                            singles="keep" if count_singles else None)  # one BAM stands for the pair (-f and -r both name it)
        try:
            count_stream(ctx, fq, counter, progress=True)
            if bam_by_name:
                count_links.bam_info = fq.info
        finally:
            fq.close()
        if count_singles and tally_singles:
            count_links.single_info.append(_single_tally(bam, counter, (0, 0, 0)))
    elif world > 1:
        # two whole-BGZF files: the ranks share them by member, count lines and inflate on their devices only, and each
        # streams its own records (FastqStream.open_shard); why == the reason when that is not what happens
        fq, why = None, member_shard_refusal(fwd, rve)
        if why is None:
            fq, why = host.FastqStream.open_shard(fwd, rve, ctx, rank, world, block_pairs=BATCH_PAIRS)
        if fq is not None:
            try:
                count_stream(ctx, fq, counter, progress=(rank == 0))  # (:156-157 for rank 0's own block, as below)
                info = fq.info
            finally:
                fq.close()
            if info["pairs"] != fq.shard_pairs:
                raise RuntimeError("%s / %s: %d pairs in the member range of rank %d where %d were counted (did a file change?)"
                                   % (fwd, rve, info["pairs"], rank, fq.shard_pairs))
            ingest_report(rank, world, "bgzf_members", None, fq.first, info["pairs"], fq.members, fq.members_pass1, info["members_device"])
        else:
            # nobody reads a whole plain file: every rank counts the lines of its byte range, the ranks exchange the counts
            # and each indexes only the bytes of its own records (:154's total follows from the counts); gzip files and
            # files with carriage returns are opened whole by every rank
            fq = host.FastqPair.open_shard(fwd, rve, ctx, rank, world)
            count_fastq(ctx, fq, counter, fq.block_offset, fq.block_offset + len(fq), progress=(rank == 0))
            ingest_report(rank, world, "whole_files" if fq.whole else "byte_ranges", why, fq.first, len(fq), None, (0, 0), (0, 0))
    elif streamed:
        fq = host.FastqStream(fwd, rve, ctx, block_pairs=BATCH_PAIRS)  # :146-154 from any readable file, read once
        try:
            count_stream(ctx, fq, counter, progress=True)
        finally:
            fq.close()
    else:
        fq = host.FastqPair(fwd, rve, ctx)  # :146-154, native multi-threaded ingest
        count_fastq(ctx, fq, counter, 0, len(fq), progress=True)
    if fq is not None:
        fq.close()
    for path in single:  # (one process only: unpaired_input)
        before = tuple(int(x) for x in counter.single_stats.cpu().numpy()) if tally_singles else None
        fs = host.SingleEndStream(path, ctx, block_reads=BATCH_PAIRS)
        try:
            count_stream(ctx, fs, counter)
        finally:
            fs.close()
        if tally_singles:
            count_links.single_info.append(_single_tally(path, counter, before))
    for rec in count_links.single_info:
        print("Unpaired reads of %s: %d used, %d with N, %d shorter than k+1" % (rec["path"], rec["used"], rec["with_n"], rec["short"]))


def count_interleaved_shard(ctx, il_path: str, counter, rank: int, world: int, singles: bool, all_gather=None):
    """One interleaved FASTQ shared among the ranks by member (``--interleaved --interleaved-shard`` under a process group):
    this rank's share through ``counter``.  When the ranks cannot share the file (``open_shard`` says why: the same on every
    rank) rank 0 reads it whole as the single process does, in its words, and the others only join the sum.  After a rank's
    stream has ended or failed every rank joins one exchange of [status, the first single's file-wide record or -1, pairs,
    singles, records]: if any rank failed every rank raises, before any collective of the counters.  The entries are exact,
    so in the strict mode every rank's first single is a single of the whole file, and the rank with the smallest record
    raises the single process's own message; the others name that rank.  On success ``count_links.interleaved_info`` holds
    the sums on every rank, and rank 0 prints the progress lines of its own pairs."""
    if all_gather is None:
        import torch.distributed as dist

        def all_gather(vals):
            got = [None] * world
            dist.all_gather_object(got, [int(v) for v in vals])
            return got

    fq, why = host.InterleavedStream.open_shard(il_path, ctx, rank, world, all_gather=all_gather, block_pairs=BATCH_PAIRS, singles=singles)
    if fq is None and rank == 0:
        fq = host.InterleavedStream(il_path, ctx, block_pairs=BATCH_PAIRS, singles=singles)
    err, first_single = None, -1
    info = dict(pairs=0, singles=0, records=0)
    if fq is not None:
        try:
            count_stream(ctx, fq, counter)
        except Exception as e:  # noqa: BLE001 (the peers hear of it through the exchange, then this rank raises)
            err = e
            head = il_path + ": record "
            if isinstance(e, ValueError) and str(e).startswith(head) and "has no mate beside it" in str(e):
                first_single = int(str(e)[len(head):].split(" ", 1)[0])
        info = fq.info
        fq.close()
    status = all_gather([0 if err is None else 2 if first_single >= 0 else 1, first_single, info["pairs"], info["singles"], info["records"]])
    lone = sorted((vals[1], r) for r, vals in enumerate(status) if vals[0] == 2)
    if err is not None and (first_single < 0 or lone[0][1] == rank):
        raise err
    if lone:
        raise RuntimeError("%s: rank %d found record %d without its mate beside it" % (il_path, lone[0][1], lone[0][0]))
    failed = [r for r, vals in enumerate(status) if vals[0]]
    if failed:
        raise RuntimeError("interleaved FASTQ ingest failed on rank(s) %s" % failed)
    if why is None:
        ingest_report(rank, world, "il_members", None, fq.first_record, info["pairs"], [fq.members], (fq.members_pass1,), (fq.plan[2] - fq.plan[0],),
                      first_record=fq.first_record, records=fq.records, total_records=fq.total_records, entry=fq.entry, members_tail=fq.members_tail)
    else:
        ingest_report(rank, world, "il_whole_file_rank0", why, 0, info["pairs"], None, (0,), (0,))
    if rank == 0:
        for mark in range(0, info["pairs"], 100000):
            print("Number of processed reads: ", mark)
    count_links.interleaved_info = dict(info, pairs=sum(v[2] for v in status), singles=sum(v[3] for v in status), records=sum(v[4] for v in status))


def _single_tally(path: str, counter, before):
    """What one file added to ``PeCounter.single_stats`` (with N, shorter than k+1, used) since ``before``."""
    now = tuple(int(x) for x in counter.single_stats.cpu().numpy())
    with_n, short, used = (a - b for a, b in zip(now, before))
    return dict(path=path, reads=with_n + short + used, with_n=with_n, short=short, used=used)


def unpaired_input(single=(), count_singles: bool = False, world: int = 1, interleaved=None, pe_text_from=None, check_names=None,
                   bam_by_name: bool = False, fwd=None, rve=None):
    """The ``--single`` files as a list, after ``--single`` / ``--count-singles`` are checked against what they cannot apply
    to -- a ``ValueError`` that says why and what to do instead, before a device is opened: ``--count-singles`` without one of
    its three homes (``--interleaved --interleaved-singles``, ``--check-names --check-names-singles``, ``--bam-by-name``;
    ``check_names`` / ``bam_by_name`` say which pairing mode is on, ``fwd`` / ``rve`` are the paired inputs, looked at only to
    say that a collated BAM has no singletons), a BAM named by ``--single``, either flag with ``--pe-text-from`` (nothing is
    counted then) or under a process group of more than one rank."""
    single = [os.fspath(p) for p in (single or ())]
    if not single and not count_singles:
        return single
    what = " and ".join(f for f, on in (("--single", bool(single)), ("--count-singles", count_singles)) if on)
    if pe_text_from is not None:
        raise ValueError("%s counts unpaired reads, and --pe-text-from reads the counts of an earlier run instead of counting: add the "
                         "unpaired reads to the run that wrote %s, or leave one of the flags out" % (what, pe_text_from))
    if count_singles and interleaved != "singles" and check_names != "singles" and not bam_by_name:
        if check_names == "strict":
            raise ValueError("--count-singles counts the records without a mate instead of dropping them, and --check-names alone stops "
                             "at the first record without a mate: no singles can exist there; add --check-names-singles, which joins "
                             "the two files by name and lets either lack records, or leave --count-singles out")
        if interleaved is None and fwd is not None and rve is not None and _starts_bam(fwd) and _starts_bam(rve):
            raise ValueError("--count-singles counts the records without a mate instead of dropping them, and %s is read as a collated "
                             "BAM, whose records come two by two: such a file has no singletons; for a BAM in any record order, or one "
                             "that lost some mates, add --bam-by-name, or leave --count-singles out" % fwd)
        raise ValueError("--count-singles counts the single records of an interleaved FASTQ instead of dropping them and needs "
                         "--interleaved --interleaved-singles, which say that -f and -r name one and that it may hold such records "
                         "(or --check-names --check-names-singles for two FASTQ files joined by read name, or --bam-by-name for one "
                         "BAM: their records without a mate are counted alike); "
                         "unpaired reads in a file of their own are given with --single FILE")
    for path in single:
        if _starts_bam(path):
            raise ValueError("%s is a BAM file, and --single reads a FASTQ of unpaired reads; convert it first, e.g. `samtools fastq "
                             "-0 unpaired.fq -s unpaired.fq %s`" % (path, path))
    if world > 1:
        raise ValueError("%s: unpaired reads are counted in one process only; sharing them among the %d ranks of this process group is "
                         "not built: run without torchrun" % (what, world))
    return single


def _regular(path: str) -> bool:
    try:
        return stat.S_ISREG(os.stat(path).st_mode)
    except OSError:
        return True  # (a missing file: the mapped open names it)


def _starts_bgzf(path: str) -> bool:
    """The first bytes of a regular file are the header of a BGZF member (gzip with FEXTRA only and a ``BC`` subfield)."""
    try:
        if not stat.S_ISREG(os.stat(path).st_mode):
            return False
        with open(path, "rb") as fh:
            head = fh.read(12)
            if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
                return False
            extra = fh.read(head[10] | (head[11] << 8))
    except OSError:
        return False  # (missing or unreadable: the mapped open names it)
    at = 0
    while at + 4 <= len(extra):
        slen = extra[at + 2] | (extra[at + 3] << 8)
        if extra[at:at + 2] == b"BC" and slen == 2:
            return True
        at += 4 + slen
    return False


def _starts_bam(path: str) -> bool:
    """The first BGZF member of a regular file inflates to bytes that start with the BAM magic."""
    if not _starts_bgzf(path):
        return False
    import zlib

    try:
        with open(path, "rb") as fh:
            head = fh.read(65536)
        xlen = head[10] | (head[11] << 8)
        return zlib.decompressobj(-15).decompress(head[12 + xlen:], 4) == b"BAM\1"
    except (OSError, zlib.error, IndexError):
        return False


def bam_input(fwd: str, rve: str, world: int = 1, by_name: bool = False, sharded: bool = False):
    """The path when ``-f`` and ``-r`` name the same regular file and it is a BAM: the pair is read from it
    (``BamStream``).  None when neither input is a BAM.  ``ValueError`` for what is out of scope: BAM on one side only, two
    different BAM files, a BAM under a process group of more than one rank -- and, with ``by_name`` (``--bam-by-name``),
    inputs that are not a BAM at all.  ``sharded``: the caller shares a collated BAM among the ranks by member
    (``BamStream.open_shard``; ``count_links`` does), so a process group is no refusal -- except with ``by_name``, whose
    mates may lie in different ranks' shares."""
    is_bam = (_starts_bam(fwd), _starts_bam(rve))
    if not any(is_bam):
        if by_name:
            raise ValueError("--bam-by-name matches the mates of ONE BAM file by their names, and %s / %s are not a BAM; name the "
                             "same BAM for both reads, or leave the flag out" % (fwd, rve))
        return None
    if not all(is_bam):
        raise ValueError("%s is a BAM file and %s is not: BAM on one side only is not supported; name the same collated BAM "
                         "for both reads, or convert it with `samtools fastq`" % ((fwd, rve) if is_bam[0] else (rve, fwd)))
    if not os.path.samefile(fwd, rve):
        raise ValueError("%s and %s are two different BAM files: a pair is read from ONE collated BAM (both mates in it); "
                         "name the same file for both reads" % (fwd, rve))
    if world > 1 and by_name:
        raise ValueError("%s: --bam-by-name reads the file in one process only: the mates of a pair may lie in different ranks' shares of "
                         "a member-sharded run; run without torchrun, or `samtools collate` the file and leave the flag out" % fwd)
    if world > 1 and not sharded:
        raise ValueError("%s: a BAM file is read by one process only by this caller (count_links shares a collated BAM among the "
                         "ranks by member); run without torchrun" % fwd)
    return fwd


def interleaved_mode(interleaved: bool, singles: bool, shard: bool = False):
    """The flags of the commands as ``count_links`` takes them: None, ``"strict"`` or ``"singles"`` (``shard``,
    ``--interleaved-shard``, is only checked here: it goes on as it is)."""
    if shard and not interleaved:
        raise ValueError("--interleaved-shard says that the ranks of a process group share an interleaved FASTQ by member and needs "
                         "--interleaved, which says that -f and -r name one")
    if singles and not interleaved:
        raise ValueError("--interleaved-singles says what to do with the single records of an interleaved FASTQ and needs "
                         "--interleaved, which says that -f and -r name one")
    return ("singles" if singles else "strict") if interleaved else None


def interleaved_input(fwd: str, rve: str, world: int = 1, interleaved=None, shard: bool = False):
    """The path when ``interleaved`` (``--interleaved``) asks for ONE interleaved FASTQ and ``-f`` and ``-r`` name it (the same
    string -- ``/dev/stdin`` twice, a FIFO -- or the same file), None without the flag.  ``ValueError`` for what the flag
    cannot apply to, before a device is opened: two different files, a BAM, ``VS_FASTQ_STREAM=0``, a process group of more
    than one rank -- unless ``shard`` (``--interleaved-shard``) says that the ranks share the file by member
    (``InterleavedStream.open_shard``), which a regular file allows and a pipe does not."""
    if interleaved is None:
        return None
    if interleaved not in ("strict", "singles"):
        raise ValueError("interleaved is None, 'strict' or 'singles', not %r" % (interleaved,))
    same = fwd == rve
    if not same:
        try:
            same = os.path.samefile(fwd, rve)
        except OSError:
            same = False
    if not same:
        raise ValueError("--interleaved reads the pairs from ONE file in which each pair's two records follow each other, and %s / %s "
                         "are two different files; name the same file for both reads, or leave the flag out" % (fwd, rve))
    if _starts_bam(fwd):
        raise ValueError("%s is a BAM file, and --interleaved reads an interleaved FASTQ; leave the flag out (a collated BAM is read "
                         "as it is, one in any record order with --bam-by-name)" % fwd)
    if os.environ.get("VS_FASTQ_STREAM") == "0":
        raise ValueError("--interleaved reads its file in the streamed ingest, and VS_FASTQ_STREAM=0 asks for the mapped open of two "
                         "files: set one of the two")
    if world > 1 and shard:
        if not _regular(fwd):  # (a pipe keeps the refusal count_links has for it, said here before a device is opened)
            raise ValueError("the FASTQ inputs %s / %s are not both regular files: a pipe can be read by one process only, so "
                             "the sharded (torchrun) run cannot take it; run one process, or write the reads to files" % (fwd, rve))
        return fwd
    if world > 1:
        raise ValueError("%s: --interleaved reads the file in one process only; sharing an interleaved file among the %d ranks of this "
                         "process group is not built: run without torchrun -- what the ranks share by member are BGZF pairs (two "
                         "bgzip files) and collated BAMs" % (fwd, world))
    return fwd


def check_names_mode(check_names: bool, singles: bool):
    """The two flags of the commands as ``count_links`` takes them: None, ``"strict"`` or ``"singles"``."""
    if singles and not check_names:
        raise ValueError("--check-names-singles says what to do with the records of two FASTQ files that have no mate in the other "
                         "file and needs --check-names, which says that the two files are paired by read name")
    return ("singles" if singles else "strict") if check_names else None


def check_names_input(fwd: str, rve: str, world: int = 1, check_names=None, bam_by_name: bool = False, interleaved=None) -> bool:
    """True when ``check_names`` (``--check-names``) asks for the two FASTQ files to be paired by read name
    (``PairedNameStream``), False without the flag.  ``ValueError`` for what the flag cannot apply to, before a device is
    opened: together with ``--interleaved`` or ``--bam-by-name`` (those inputs are checked or joined by name already), a BAM
    input, ``VS_FASTQ_STREAM=0``, a process group of more than one rank."""
    if check_names is None:
        return False
    if check_names not in ("strict", "singles"):
        raise ValueError("check_names is None, 'strict' or 'singles', not %r" % (check_names,))
    if interleaved is not None:
        raise ValueError("--check-names pairs TWO FASTQ files by read name, and --interleaved reads one file whose mates are checked by "
                         "name already: set one of the two")
    if bam_by_name:
        raise ValueError("--check-names pairs two FASTQ files by read name, and --bam-by-name joins the records of one BAM by name "
                         "already: set one of the two")
    for path in (fwd, rve):
        if _starts_bam(path):
            raise ValueError("%s is a BAM file, and --check-names pairs two FASTQ files by read name; leave the flag out (a collated BAM "
                             "is checked by its first / second flags, one in any record order is joined with --bam-by-name)" % path)
    if os.environ.get("VS_FASTQ_STREAM") == "0":
        raise ValueError("--check-names reads its files in the streamed ingest, and VS_FASTQ_STREAM=0 asks for the mapped open: set one "
                         "of the two")
    if world > 1:
        raise ValueError("%s / %s: --check-names reads the two files in one process only; pairing by name among the %d ranks of this "
                         "process group is not built: run without torchrun" % (fwd, rve, world))
    return True


def member_shard_refusal(fwd: str, rve: str):
    """None when a sharded run tries the member-sharded open (both inputs regular files that start with a BGZF member, and
    neither ``VS_FASTQ_STREAM=0`` nor ``VS_BGZF_DEVICE=0`` -- the switches that give the mapped open and host zlib in
    one process), else the reason it does not; the same on every rank, which all see the same files and environment."""
    if os.environ.get("VS_FASTQ_STREAM") == "0":
        return "VS_FASTQ_STREAM=0"
    if os.environ.get("VS_BGZF_DEVICE") == "0":
        return "VS_BGZF_DEVICE=0"
    if not (_starts_bgzf(fwd) and _starts_bgzf(rve)):
        return "the inputs are not both BGZF"
    return None


def ingest_report(rank, world, path, reason, first_pair, pairs, members, members_pass1, members_pass2, **more):
    """Which ingest a rank of a sharded run took, for whoever asks with ``VS_INGEST_REPORT=DIR`` (stdout stays the
    reference's): ``DIR/ingest_rank<r>.json``.  ``more``: further integers of that ingest, under their names."""
    d = os.environ.get("VS_INGEST_REPORT")
    if not d:
        return
    import json

    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "ingest_rank%d.json" % rank), "w") as fh:
        json.dump(dict(rank=rank, world=world, path=path, reason=reason, first_pair=int(first_pair), pairs=int(pairs),
                       members=None if members is None else [int(x) for x in members],
                       members_pass1=[int(x) for x in members_pass1], members_pass2=[int(x) for x in members_pass2],
                       **{k: int(v) for k, v in more.items()}), fh)


def _starts_gzip(path: str) -> bool:
    """The first two bytes of a regular file are the gzip magic (a pipe is not read here: it streams whatever it holds)."""
    try:
        if not stat.S_ISREG(os.stat(path).st_mode):
            return False
        with open(path, "rb") as fh:
            return fh.read(2) == b"\x1f\x8b"
    except OSError:
        return False


def gzip_device_refusal(world: int):
    """None, or why ``VS_GZIP_DEVICE=1`` (``--gzip-device``: plain gzip decoded in parallel on the device, in the streamed
    ingest) cannot hold: under a process group of more than one rank -- one deflate stream shared among ranks is not built --
    and together with ``VS_FASTQ_STREAM=0``, which asks for the mapped open."""
    if os.environ.get("VS_GZIP_DEVICE") != "1":
        return None
    if world > 1:
        return ("VS_GZIP_DEVICE=1 (--gzip-device) decodes a plain gzip file as one stream in one process; sharing one stream among the "
                "%d ranks of this process group is not built: leave the switch out, or write the reads as BGZF (bgzip), which the "
                "ranks share by member" % world)
    if os.environ.get("VS_FASTQ_STREAM") == "0":
        return ("VS_GZIP_DEVICE=1 (--gzip-device) decodes gzip in the streamed ingest, and VS_FASTQ_STREAM=0 asks for the mapped "
                "open: set one of the two")
    return None


def use_stream(fwd: str, rve: str) -> bool:
    """The streamed ingest reads the pair when either input is not a regular file (a FIFO, /dev/stdin, a process
    substitution: there is nothing to map), when ``VS_FASTQ_STREAM=1`` asks for it, or when both are regular files and at
    least one starts with a BGZF member (its members are inflated on the device there, where the mapped open inflates the
    whole file on one host core) unless ``VS_FASTQ_STREAM=0``; other regular files are mapped.  With ``VS_GZIP_DEVICE=1``
    a regular file that starts with the gzip magic streams too (ValueError where the switch cannot hold:
    ``gzip_device_refusal``)."""
    env = os.environ.get("VS_FASTQ_STREAM")
    gzip_device = os.environ.get("VS_GZIP_DEVICE") == "1"
    if gzip_device:  # (the world size is asked for only with the switch on)
        why = gzip_device_refusal(_rank_world()[1])
        if why is not None:
            raise ValueError(why)
    if env == "1" or not (_regular(fwd) and _regular(rve)):
        return True
    if gzip_device and (_starts_gzip(fwd) or _starts_gzip(rve)):
        return True
    return env != "0" and (_starts_bgzf(fwd) or _starts_bgzf(rve))


def count_stream(ctx, fs, counter, progress: bool = False):
    """Every pair of a ``FastqStream`` through the counters, block by block: the device packs block i+1 while it still
    counts block i.  The total is known only at the end of the input, so the progress lines (:156-157) are held and
    printed then -- and not at all when the input fails its end-of-input checks, as the mapped path prints none."""
    import torch

    with torch.cuda.device(counter.device):
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    block = fs.next_block()
    while block is not None:
        counter.add(block)
        nxt = fs.next_block()
        ctx.sync()
        block.free()
        block = nxt
    if progress:
        for mark in range(0, fs.n_pairs, 100000):
            print("Number of processed reads: ", mark)


def count_fastq(ctx, fq, counter, first: int, last: int, batch: int = BATCH_PAIRS, progress: bool = False):
    """Pairs [first, last) of an indexed FASTQ pair through the counters, one block of ``batch``
    pairs at a time.  The host cores pack block i+1 (``vs_fastq_block``: 2 bits per base into
    pinned staging, upload enqueued) while the device still counts block i."""
    spans = [(lo, min(last, lo + batch)) for lo in range(first, last, batch)]
    # the uploads of a block are enqueued on the context's stream: make that the stream the counting runs on
    # BEFORE the first block is made (PeCounter.add sets the same stream again for every block)
    import torch

    with torch.cuda.device(counter.device):
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    nxt = fq.block(spans[0][0], spans[0][1] - spans[0][0]) if spans else None
    for i, (lo, hi) in enumerate(spans):
        if progress:
            for mark in range(((lo + 99999) // 100000) * 100000, hi, 100000):
                print("Number of processed reads: ", mark)  # :156-157 (rank 0's own block under torchrun)
        block = nxt
        counter.add(block)  # enqueued behind the block's uploads
        nxt = fq.block(spans[i + 1][0], spans[i + 1][1] - spans[i + 1][0]) if i + 1 < len(spans) else None
        ctx.sync()
        block.free()


def write_info_files(out_dir: str, ids, counter, sparse: bool = False, bgzf: bool = False):
    """pe_info / st_info text, PE_Inference.py:190-207.  Returns the first file's name and the stats.  ``sparse``: only the
    lines with a non-zero count, written from the counters on the device (``PeCounter.write_sparse_text``) -- the
    reference reads them to the same dict (``process_pe_info`` zeroes every key first, IO.py:598-623).  ``bgzf``: the
    files are ``pe_info.gz`` / ``st_info.gz``, BGZF made on the device (``PeCounter.write_bgzf_text``); they inflate to
    the dense text, or with ``sparse`` to the sparse one."""
    out_file = "{0}/pe_info".format(out_dir)
    out_file2 = "{0}/st_info".format(out_dir)
    if bgzf:
        out_file, out_file2 = out_file + ".gz", out_file2 + ".gz"
        counter.write_bgzf_text(out_file, out_file2, ids, dense=not sparse)
        s = counter.stats.cpu().numpy()
        return out_file, (int(s[0]), int(s[1]), int(s[2]))
    if sparse:
        counter.write_sparse_text(out_file, out_file2, ids)
        s = counter.stats.cpu().numpy()
        return out_file, (int(s[0]), int(s[1]), int(s[2]))
    node_mat, short_mat, stats = counter.result()
    host.write_matrix_text(out_file, ids, node_mat)
    host.write_matrix_text(out_file2, ids, short_mat)
    return out_file, stats


def run(gfa: str, out_dir: str, fwd: str, rve: str, kmer_size: int, device: int = 0, ctx=None, stages_follow: bool = False,
        sparse_info: bool = False, bgzf_info: bool = False, bam_by_name: bool = False, interleaved=None, check_names=None, single=(),
        count_singles: bool = False, interleaved_shard: bool = False):
    # PE_Inference.py:93-96: the output directory is wiped and recreated
    if out_dir[-1] == "/":
        out_dir = out_dir[:-1]
    rank, world = _rank_world()
    if rank == 0:  # under torchrun only the writer touches the directory
        shutil.rmtree(out_dir, ignore_errors=True)
        os.makedirs(out_dir, exist_ok=True)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()  # nobody counts (or could fail half-way) before the directory is in its final state

    glb_start = time.time()
    if bam_by_name:
        bam_input(fwd, rve, world, by_name=True)  # (what the flag cannot apply to is said before a device is opened)
    interleaved_input(fwd, rve, world, interleaved, shard=interleaved_shard)  # (the same)
    check_names_input(fwd, rve, world, check_names, bam_by_name=bam_by_name, interleaved=interleaved)  # (the same)
    unpaired_input(single, count_singles, world, interleaved, check_names=check_names, bam_by_name=bam_by_name, fwd=fwd, rve=rve)  # (the same)
    if ctx is None:
        ctx = host.Context(device)
    ids, counter = count_links(ctx, gfa, fwd, rve, kmer_size, stages_follow=stages_follow, bam_by_name=bam_by_name, interleaved=interleaved,
                               check_names=check_names, single=single, count_singles=count_singles, interleaved_shard=interleaved_shard)
    run.last = (ids, counter)
    if rank != 0:
        return None  # the counters were reduced to rank 0, which writes the files
    out_file, stats = write_info_files(out_dir, ids, counter, sparse=sparse_info, bgzf=bgzf_info)
    glb_elapsed = time.time() - glb_start
    print("Global time elapsed: ", glb_elapsed)  # :209-211
    print("result stored in: ", out_file)
    return stats


def main(argv=None):
    print("----------------------Paired-End Information Alignment----------------------")  # :52-54
    parser = argparse.ArgumentParser(
        prog="pe_info", description="""Align Paired-End reads to nodes in graph to obtain strong links""")
    parser.add_argument("-g", "--gfa,", dest="gfa", type=str, required=True, help="graph, .gfa format")
    parser.add_argument("-o", "--output_dir", dest="dir", type=str, required=True, help="output directory")
    parser.add_argument("-f", "--forward", dest="fwd", required=True, help="forward read, .fastq")
    parser.add_argument("-r", "--reverse", dest="rve", required=True, help="reverse read, .fastq")
    parser.add_argument("-k", "--kmer_size", dest="kmer_size", type=int, default=128, help="unique kmer size")
    parser.add_argument("--device", dest="device", type=int, default=0, help="HIP device ordinal (extension)")
    parser.add_argument("--sparse-info", dest="sparse_info", action="store_true", default=False,
                        help="extension: write only the lines of pe_info / st_info whose count is not 0, formatted on the "
                             "device (the reference reads such files to the same result)")
    parser.add_argument("--bgzf-info", dest="bgzf_info", action="store_true", default=False,
                        help="extension: write pe_info.gz / st_info.gz, BGZF deflated on the device; `gzip -dc` gives the "
                             "reference's file byte for byte (with --sparse-info: the sparse file)")
    parser.add_argument("--bam-by-name", dest="bam_by_name", action="store_true", default=False,
                        help="extension: -f and -r name ONE BAM in any record order (coordinate-sorted, `samtools view -f 12` of "
                             "a sorted alignment, ...); the mates are matched by read name on the device, records without a mate "
                             "are dropped (counted as unpaired reads with --count-singles) -- no `samtools collate` first")
    parser.add_argument("--gzip-device", dest="gzip_device", action="store_true", default=False,
                        help="extension: decode plain .fastq.gz (one deflate stream, as gzip and pigz write it) on the device, in "
                             "parallel from speculative block starts, instead of with zlib on one host core (sets VS_GZIP_DEVICE=1; "
                             "one process only)")
    parser.add_argument("--interleaved", dest="interleaved", action="store_true", default=False,
                        help="extension: -f and -r name ONE interleaved FASTQ (a file, a pipe, /dev/stdin; any compression the "
                             "two-file input takes), each pair's two records one behind the other as `samtools fastq`, `seqtk "
                             "mergepe` and `fastp --stdout` write them; the mates are checked by name on the device and a record "
                             "without its mate beside it stops the run")
    parser.add_argument("--interleaved-singles", dest="interleaved_singles", action="store_true", default=False,
                        help="extension: with --interleaved, records without their mate beside them (the single reads `samtools "
                             "fastq x.bam` writes among the pairs) are dropped and counted instead")
    parser.add_argument("--interleaved-shard", dest="interleaved_shard", action="store_true", default=False,
                        help="extension, off by default: with --interleaved under torchrun, the ranks share ONE whole-BGZF interleaved "
                             "file (`... | bgzip`) by member, each counting the pairs whose first record lies in its share; any other "
                             "regular file is read whole by rank 0 (without the flag --interleaved is one process's)")
    parser.add_argument("--check-names", dest="check_names", action="store_true", default=False,
                        help="extension: pair the two FASTQ files by read name on the device instead of by position: record i of -f and "
                             "record i of -r must be mates by name (as `bwa mem` demands), and the first pair that is not stops the run "
                             "-- what two files trimmed or filtered separately would otherwise turn into wrong links unnoticed")
    parser.add_argument("--check-names-singles", dest="check_names_singles", action="store_true", default=False,
                        help="extension: with --check-names, the two files are in the same order but either may lack records the other "
                             "has; mates are found by a hash join on the names, records without a mate are dropped and counted per file")
    parser.add_argument("--single", dest="single", action="append", default=[], metavar="FILE",
                        help="extension (repeatable): a FASTQ of UNPAIRED reads -- the unpaired survivors of a trimmer, the merged reads "
                             "of an overlapping library -- in any form the paired input takes; each read is counted into st_info as the "
                             "reference counts one end of a pair, pe_info does not change (one process only)")
    parser.add_argument("--count-singles", dest="count_singles", action="store_true", default=False,
                        help="extension: with --interleaved --interleaved-singles, with --check-names --check-names-singles or with "
                             "--bam-by-name, the records without a mate are counted into st_info as unpaired reads instead of dropped")
    args = parser.parse_args(argv)
    interleaved = interleaved_mode(args.interleaved, args.interleaved_singles, args.interleaved_shard)
    check_names = check_names_mode(args.check_names, args.check_names_singles)
    if args.gzip_device:
        os.environ["VS_GZIP_DEVICE"] = "1"  # (the library reads the switch where it reads VS_BGZF_DEVICE)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    interleaved_input(args.fwd, args.rve, world, interleaved, shard=args.interleaved_shard)  # (refused before a device is opened or a process group made)
    check_names_input(args.fwd, args.rve, world, check_names, bam_by_name=args.bam_by_name, interleaved=interleaved)  # (the same)
    unpaired_input(args.single, args.count_singles, world, interleaved, check_names=check_names, bam_by_name=args.bam_by_name, fwd=args.fwd,
                   rve=args.rve)  # (the same)
    if world > 1:  # launched by torchrun: one rank per GPU, counters all-reduced over RCCL
        import torch
        import torch.distributed as dist

        local = int(os.environ.get("LOCAL_RANK", "0"))
        # (VS_DIST_BACKEND=gloo VS_DIST_DEVICE=0: several ranks on ONE GPU, counters summed through gloo --
        # how the sharded drop-in is exercised end to end on a one-GPU box; RCCL wants one device per rank)
        backend = os.environ.get("VS_DIST_BACKEND", "nccl")
        local = int(os.environ.get("VS_DIST_DEVICE", str(local)))
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        args.device = local
        # every rank indexes both FASTQ files on the host: share the cores between the local ranks
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        os.environ.setdefault("VS_HOST_THREADS", str(max(1, (os.cpu_count() or 1) // max(local_world, 1))))
    run(args.gfa, args.dir, args.fwd, args.rve, args.kmer_size, args.device, sparse_info=args.sparse_info, bgzf_info=args.bgzf_info,
        bam_by_name=args.bam_by_name, interleaved=interleaved, check_names=check_names, single=args.single, count_singles=args.count_singles,
        interleaved_shard=args.interleaved_shard)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
    sys.exit(0)
