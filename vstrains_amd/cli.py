#!/usr/bin/env python3
"""``vstrains``-compatible command line (reference ``vstrains:32-277``): same flags, same output
directory layout, same log lines; the work runs on MI355X through libvstrains_hip.so.

    python -m vstrains_amd.cli -a spades -g graph.gfa -p contigs.paths -o OUT -fwd f.fq -rve r.fq
    python -m vstrains_amd.cli -a spades -g graph.gfa --contigs-fasta contigs.fasta -o OUT -fwd f.fq -rve r.fq

``--contigs-fasta FILE`` (extension, in place of ``-p``): the contigs are threaded through the graph on the device
(vstrains_amd.contig_paths) and the pipeline goes on with OUT/tmp/contigs_threaded.paths -- for an assembly whose
contigs.paths is gone, polished or filtered contigs, known genomes as guides, a graph of another de Bruijn assembler.

Not restated: ``-r/--reference_fa`` (hidden debug mode that shells out to minimap2) is accepted
and refused with a message; the coverage histogram PNG is not drawn.
"""
import argparse
import logging
import os
import platform
import sys
import time
from datetime import date

import numpy

__version__ = "1.1.0"


def build_parser():
    p = argparse.ArgumentParser(
        prog="VStrains",
        description="""Construct full-length viral strains under de novo approach
        from contigs and assembly graph, currently supports SPAdes""")
    p.add_argument("-a", "--assembler", dest="assembler", type=str, required=True, choices=["spades"],
                   help="name of the assembler used. [spades]")
    p.add_argument("-g", "--graph", dest="gfa_file", type=str, required=True,
                   help="path to the assembly graph, (.gfa format)")
    p.add_argument("-p", "--path", dest="path_file", type=str, required=False,
                   help="contig file from SPAdes (.paths format), only required for SPAdes. e.g., contigs.paths")
    p.add_argument("-mc", "--minimum_coverage", dest="min_cov", default=None, type=int, help=argparse.SUPPRESS)
    p.add_argument("-ml", "--minimum_contig_length", dest="min_len", default=None, type=int, help=argparse.SUPPRESS)
    p.add_argument("-r", "--reference_fa", dest="ref_file", default=None, type=str, help=argparse.SUPPRESS)
    p.add_argument("-o", "--output_dir", dest="output_dir", default="acc/", type=str,
                   help="path to the output directory [default: acc/]")
    p.add_argument("-d", "--dev_mode", dest="dev", action="store_true", default=False, help=argparse.SUPPRESS)
    p.add_argument("-fwd", "--fwd_file", dest="fwd", required=True, default=None, type=str,
                   help="paired-end sequencing reads, forward strand (.fastq format)")
    p.add_argument("-rve", "--rve_file", dest="rve", required=True, default=None, type=str,
                   help="paired-end sequencing reads, reverse strand (.fastq format)")
    p.add_argument("--device", dest="device", default=0, type=int, help="HIP device ordinal (extension)")
    p.add_argument("--no-pe-text", dest="no_pe_text", action="store_true", default=False,
                   help="extension: do not write the N^2-line aln/pe_info and aln/st_info (the graph stages read "
                        "the counters from device memory either way)")
    p.add_argument("--sparse-pe-text", dest="sparse_pe_text", action="store_true", default=False,
                   help="extension: write aln/pe_info and aln/st_info with the lines of non-zero count only, formatted on "
                        "the device (not together with --no-pe-text)")
    p.add_argument("--bgzf-pe-text", dest="bgzf_pe_text", action="store_true", default=False,
                   help="extension: write aln/pe_info.gz and aln/st_info.gz, BGZF deflated on the device; `gzip -dc` gives the "
                        "reference's files byte for byte, or with --sparse-pe-text the sparse ones (not together with "
                        "--no-pe-text)")
    p.add_argument("--pe-text-from", dest="pe_text_from", default=None, type=str, metavar="ALN_DIR",
                   help="extension: do not count the reads again; read ALN_DIR/pe_info.gz + st_info.gz (or pe_info + st_info) "
                        "that an earlier run or vstrains_amd.pe_inference wrote, on the device (not together with --no-pe-text, "
                        "--sparse-pe-text or --bgzf-pe-text; -fwd / -rve are still required and are not opened)")
    p.add_argument("--bam-by-name", dest="bam_by_name", action="store_true", default=False,
                   help="extension: -fwd and -rve name ONE BAM in any record order (coordinate-sorted, `samtools view -f 12` of a "
                        "sorted alignment, ...); the mates are matched by read name on the device and records without a mate are "
                        "dropped, no `samtools collate` first (not together with --pe-text-from)")
    p.add_argument("--interleaved", dest="interleaved", action="store_true", default=False,
                   help="extension: -fwd and -rve name ONE interleaved FASTQ (a file, a pipe, /dev/stdin; any compression the two-file "
                        "input takes), each pair's two records one behind the other as `samtools fastq`, `seqtk mergepe` and `fastp "
                        "--stdout` write them; the mates are checked by name on the device and a record without its mate beside it "
                        "stops the run (not together with --pe-text-from)")
    p.add_argument("--interleaved-singles", dest="interleaved_singles", action="store_true", default=False,
                   help="extension: with --interleaved, records without their mate beside them (the single reads `samtools fastq "
                        "x.bam` writes among the pairs) are dropped and counted instead")
    p.add_argument("--interleaved-shard", dest="interleaved_shard", action="store_true", default=False,
                   help="extension, off by default: with --interleaved under torchrun, the ranks share ONE whole-BGZF interleaved file "
                        "(`... | bgzip`) by member, each counting the pairs whose first record lies in its share; any other regular "
                        "file is read whole by rank 0 (without the flag --interleaved is one process's)")
    p.add_argument("--check-names", dest="check_names", action="store_true", default=False,
                   help="extension: pair the two FASTQ files by read name on the device instead of by position: record i of -fwd and "
                        "record i of -rve must be mates by name (as `bwa mem` demands), and the first pair that is not stops the run -- "
                        "what two files trimmed or filtered separately would otherwise turn into wrong links unnoticed (not together "
                        "with --pe-text-from)")
    p.add_argument("--check-names-singles", dest="check_names_singles", action="store_true", default=False,
                   help="extension: with --check-names, the two files are in the same order but either may lack records the other has; "
                        "mates are found by a hash join on the names, records without a mate are dropped and counted per file")
    p.add_argument("--gzip-device", dest="gzip_device", action="store_true", default=False,
                   help="extension: decode plain .fastq.gz (one deflate stream, as gzip and pigz write it) on the device, in parallel "
                        "from speculative block starts, instead of with zlib on one host core (sets VS_GZIP_DEVICE=1; one process only)")
    p.add_argument("--single", dest="single", action="append", default=[], metavar="FILE",
                   help="extension (repeatable): a FASTQ of UNPAIRED reads -- the unpaired survivors of a trimmer, the merged reads of an "
                        "overlapping library -- in any form the paired input takes; each read is counted into aln/st_info as the "
                        "reference counts one end of a pair, aln/pe_info does not change (one process only; not together with "
                        "--pe-text-from)")
    p.add_argument("--count-singles", dest="count_singles", action="store_true", default=False,
                   help="extension: with --interleaved --interleaved-singles, with --check-names --check-names-singles or with "
                        "--bam-by-name, the records without a mate are counted into aln/st_info as unpaired reads instead of dropped")
    p.add_argument("--depth-from-reads", dest="depth_from_reads", action="store_true", default=False,
                   help="extension: take every segment's depth from THESE reads instead of from the assembler's tags: the (k+1)-mer "
                        "occurrences of each segment in the reads are counted on the device first (vstrains_amd.node_depth) and "
                        "the graph goes on as gfa/graph_depth.gfa with LN:i / KC:i tags -- for one assembly graph run against many "
                        "samples, subsampled or depleted reads, or a GFA that lost its tags; a segment no read touches stops the run; "
                        "the reads are read twice, so they must be regular files (one process only)")
    # (not listed by --help, whose text is pinned to the reference's flags and the extensions before this one: see the module's
    # docstring and README.md)
    p.add_argument("--contigs-fasta", dest="contigs_fasta", default=None, type=str, metavar="FILE", help=argparse.SUPPRESS)
    # with --depth-from-reads: the same single pass also writes the depth of every window of k + 1 bases (k-mer coverage by window
    # START, not base coverage) as gfa/graph_depth.bedgraph and a line per segment as gfa/graph_depth.tsv (vstrains_amd.node_depth)
    p.add_argument("--depth-profile", dest="depth_profile", action="store_true", default=False, help=argparse.SUPPRESS)
    # with --depth-from-reads: the same read pass also lays every end along its anchors' diagonals across mismatches and writes the
    # base pileup as gfa/graph_depth.pileup.tsv and its minor bases as gfa/graph_depth.vcf (vstrains_amd.node_depth --pileup --variants)
    p.add_argument("--depth-pileup", dest="depth_pileup", action="store_true", default=False, help=argparse.SUPPRESS)
    # with --depth-from-reads --depth-pileup: the reads are then read once more and what one read pair carries at the positions of the
    # records of gfa/graph_depth.vcf is written as gfa/graph_depth.site_pairs.tsv (vstrains_amd.node_depth --variants --site-pairs)
    p.add_argument("--depth-site-pairs", dest="depth_site_pairs", action="store_true", default=False, help=argparse.SUPPRESS)
    # with --depth-from-reads --depth-pileup: the pileup keeps the two strands apart and the two files are written in their stranded
    # form, the records found on the device and carrying DP4 (vstrains_amd.node_depth --pileup --variants --strands)
    p.add_argument("--depth-strands", dest="depth_strands", action="store_true", default=False, help=argparse.SUPPRESS)
    # with --depth-from-reads --depth-pileup: the same read pass also finds the insertions and deletions of at most 16 bases that the read
    # ends carry and writes them as gfa/graph_depth.indels.vcf (vstrains_amd.node_depth --indels)
    p.add_argument("--depth-indels", dest="depth_indels", action="store_true", default=False, help=argparse.SUPPRESS)
    return p


def contigs_fasta_refusal(args, world: int):
    """None, or why ``--contigs-fasta`` cannot hold, said before anything is written or a device opened."""
    if args.path_file:
        return "--contigs-fasta and -p are mutually exclusive: the contigs' paths are either given or threaded from the FASTA"
    if world > 1:
        return ("--contigs-fasta threads in one process only; sharing the pass among the %d ranks of this process group is not built: "
                "run without torchrun" % world)
    return None


def contigs_fasta(args, logger, ctx):
    """The threading pass on ``-g`` (after ``--depth-from-reads``: on that graph): OUT/tmp/contigs_threaded.paths, which the
    pipeline then takes as its ``-p``."""
    from . import contig_paths

    try:
        text, tally = contig_paths.thread_contigs(ctx, args.gfa_file, args.contigs_fasta)
    except ValueError as e:
        logger.error("--contigs-fasta: %s" % e)
        sys.exit(1)
    out = args.output_dir + "/tmp/contigs_threaded.paths"
    with open(out, "w") as fh:
        fh.write(text)
    logger.info("contigs threaded through the graph: {0}; the paths go on as {1}".format(contig_paths.tally_line(tally), out))
    args.path_file = out


def depth_profile_refusal(args):
    """None, or why ``--depth-profile`` cannot hold, said before anything is written: it is a by-product of the depth pass."""
    if args.depth_profile and not args.depth_from_reads:
        return "--depth-profile writes the profile of the depth pass: give --depth-from-reads with it"
    return None


def depth_pileup_refusal(args):
    """None, or why ``--depth-pileup`` cannot hold, said before anything is written: it rides on the depth pass."""
    if args.depth_pileup and not args.depth_from_reads:
        return "--depth-pileup writes the base pileup of the depth pass: give --depth-from-reads with it"
    return None


def depth_strands_refusal(args):
    """None, or why ``--depth-strands`` cannot hold, said before anything is written: the strands are those of the pileup."""
    if args.depth_strands and not (args.depth_from_reads and args.depth_pileup):
        return "--depth-strands keeps the strands of the pileup apart: give --depth-from-reads --depth-pileup with it"
    return None


def depth_indels_refusal(args):
    """None, or why ``--depth-indels`` cannot hold, said before anything is written: its depth is the pileup's."""
    if getattr(args, "depth_indels", False) and not (args.depth_from_reads and args.depth_pileup):
        return "--depth-indels measures its events against the pileup: give --depth-from-reads --depth-pileup with it"
    return None


def depth_site_pairs_refusal(args):
    """None, or why ``--depth-site-pairs`` cannot hold, said before anything is written: its sites are the pileup's records, and
    the reads are read once more for it."""
    if not args.depth_site_pairs:
        return None
    if not (args.depth_from_reads and args.depth_pileup):
        return "--depth-site-pairs links the minor bases of the pileup: give --depth-from-reads --depth-pileup with it"
    for path in [args.fwd, args.rve] + list(args.single or ()):
        if not os.path.isfile(path):
            return "--depth-site-pairs reads the reads once more, and %s is not a regular file: write the reads to a file" % path
    return None


def depth_from_reads_refusal(args, world: int):
    """None, or why ``--depth-from-reads`` cannot hold, said before anything is written: under a process group, or -- the
    reads are read twice, once for the depth and once for the PE links -- with an input that is not a regular file (with
    ``--pe-text-from`` the PE links are not counted and the reads are read once: a pipe is fine)."""
    if world > 1:
        return ("--depth-from-reads counts in one process only; sharing the depth pass among the %d ranks of this process group is not "
                "built: run without torchrun" % world)
    if args.pe_text_from is None:
        from .pe_inference import _regular

        for path in [args.fwd, args.rve] + list(args.single or ()):
            if not _regular(path):
                return ("--depth-from-reads reads the reads twice (the depth pass, then the PE links), and %s is not a regular file: a "
                        "pipe can be read once; write the reads to a file, or run vstrains_amd.node_depth on its own and give its GFA "
                        "with -g" % path)
    return None


def depth_from_reads(args, logger, ctx):
    """The depth pass on ``-g``: OUT/gfa/graph_depth.gfa, which the pipeline then takes as its graph.  Exit 1 when a segment
    has KC = 0 (the reference stops on such a tag itself, IO.py:49-77)."""
    from . import node_depth

    with open(args.gfa_file, "rb") as fh:
        raw = fh.read()
    try:
        k = node_depth.infer_k(raw)
    except ValueError as e:
        logger.error("--depth-from-reads: %s" % e)
        sys.exit(1)
    got = node_depth.depth_pass(ctx, args.gfa_file, args.fwd, args.rve, k, bam_by_name=args.bam_by_name, interleaved=args.interleaved,
                                check_names=args.check_names, single=args.single, count_singles=args.count_singles, quiet=True,
                                profile=args.depth_profile, pileup=8 if args.depth_pileup else None,
                                **(dict(strands=(2, 0.01, 0)) if args.depth_strands else {}),
                                **(dict(indels=16) if args.depth_indels else {}))
    gapped = None
    if args.depth_indels:
        got, gapped = got[:-1], got[-1]
    ids, kc, ends = got[:3]
    out = args.output_dir + "/gfa/graph_depth.gfa"
    with open(out, "wb") as fh:
        fh.write(node_depth.rewrite_gfa(raw, kc.tolist()))
    if args.depth_profile:
        lengths, offsets, cov = got[3]
        node_depth.write_bedgraph(args.output_dir + "/gfa/graph_depth.bedgraph", ids, offsets, cov)
        node_depth.write_summary(args.output_dir + "/gfa/graph_depth.tsv", ids, lengths, offsets, cov)
        logger.info("depth profile of every window of k + 1 bases: {0}/gfa/graph_depth.bedgraph, per segment: {0}/gfa/graph_depth.tsv".format(args.output_dir))
    if args.depth_pileup:
        seqs, p_offsets, p_depth, p_alt, (credited, rejected) = got[-1][:5]
        if args.depth_strands:
            node_depth.write_strand_pileup(args.output_dir + "/gfa/graph_depth.pileup.tsv", ids, seqs, p_offsets, p_depth, p_alt)
            node_depth.write_strand_vcf(args.output_dir + "/gfa/graph_depth.vcf", ids, seqs, p_offsets, got[-1][5])
        else:
            node_depth.write_pileup(args.output_dir + "/gfa/graph_depth.pileup.tsv", ids, seqs, p_offsets, p_depth, p_alt)
            node_depth.write_vcf(args.output_dir + "/gfa/graph_depth.vcf", ids, seqs, p_offsets, p_depth, p_alt)
        logger.info("base pileup of every position: {0}/gfa/graph_depth.pileup.tsv, minor bases: {0}/gfa/graph_depth.vcf ({1} alignments, {2} rejected)"
                    .format(args.output_dir, credited, rejected))
    if gapped is not None:
        node_depth.write_indel_vcf(args.output_dir + "/gfa/graph_depth.indels.vcf", ids, seqs, p_offsets,
                                   node_depth.indel_records(ids, seqs, gapped[0], p_offsets, p_depth, p_alt))
        logger.info("insertions and deletions of the read ends: {0}/gfa/graph_depth.indels.vcf ({1})"
                    .format(args.output_dir, ", ".join("%d %s" % (v, what) for v, what in zip(gapped[1], node_depth.INDEL_TALLIES))))
    if args.depth_site_pairs:
        records = node_depth.strand_records(ids, got[-1][5]) if args.depth_strands else node_depth.variant_records(ids, seqs, p_offsets, p_depth, p_alt)
        linked = node_depth.site_pairs_pass(ctx, node_depth.record_sites(ids, records), args.fwd, args.rve, bam_by_name=args.bam_by_name,
                                            interleaved=args.interleaved, check_names=args.check_names, single=args.single,
                                            count_singles=args.count_singles, quiet=True)
        node_depth.write_site_pairs(args.output_dir + "/gfa/graph_depth.site_pairs.tsv", ids, *linked[:4])
        logger.info("bases that travel together on one read pair: {0}/gfa/graph_depth.site_pairs.tsv ({1})".format(
            args.output_dir, ", ".join("%d %s" % (v, what) for v, what in zip(linked[4], node_depth.SITE_PAIR_TALLIES))))
    logger.info("segment depth counted from the reads: k = {0}, {1} read ends, KC sum {2}; the graph goes on as {3}".format(k, ends, int(kc.sum()), out))
    empty = [ids[i] for i in range(len(ids)) if kc[i] == 0]
    if empty:
        logger.error("--depth-from-reads: {0} of {1} segments are touched by no read (KC = 0), e.g. {2}; take them out of the graph, or use "
                     "the assembler's depth".format(len(empty), len(ids), ", ".join(empty[:5])))
        sys.exit(1)
    args.gfa_file = out


def pe_text_pair(aln_dir):
    """The pe_info / st_info pair of ``aln_dir`` that --pe-text-from reads: the .gz pair if both are there, else the plain
    pair, else None."""
    for suffix in (".gz", ""):
        pair = (os.path.join(aln_dir, "pe_info" + suffix), os.path.join(aln_dir, "st_info" + suffix))
        if all(os.path.isfile(f) for f in pair):
            return pair
    return None


def _bail(*lines):
    for line in lines:
        print(line)
    print("\nExiting...\n")
    sys.exit(1)


def main(argv=None, backend=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.gzip_device:
        os.environ["VS_GZIP_DEVICE"] = "1"  # (the library reads the switch where it reads VS_BGZF_DEVICE)
    if args.no_pe_text and args.sparse_pe_text:
        parser.error("--no-pe-text and --sparse-pe-text are mutually exclusive")
    if args.no_pe_text and args.bgzf_pe_text:
        parser.error("--no-pe-text and --bgzf-pe-text are mutually exclusive")
    if args.pe_text_from is not None:
        for flag, name in ((args.no_pe_text, "--no-pe-text"), (args.sparse_pe_text, "--sparse-pe-text"), (args.bgzf_pe_text, "--bgzf-pe-text"),
                           (args.bam_by_name, "--bam-by-name"), (args.interleaved or args.interleaved_singles or args.interleaved_shard, "--interleaved"),
                           (args.check_names or args.check_names_singles, "--check-names")):
            if flag:
                parser.error("--pe-text-from and %s are mutually exclusive" % name)
    from . import pe_inference

    # (what the flags cannot apply to is a ValueError that says why, before anything is written or a device opened)
    args.interleaved = pe_inference.interleaved_mode(args.interleaved, args.interleaved_singles, args.interleaved_shard)
    pe_inference.interleaved_input(args.fwd, args.rve, pe_inference._rank_world()[1], args.interleaved, shard=args.interleaved_shard)
    args.check_names = pe_inference.check_names_mode(args.check_names, args.check_names_singles)
    pe_inference.check_names_input(args.fwd, args.rve, pe_inference._rank_world()[1], args.check_names, bam_by_name=args.bam_by_name,
                                   interleaved=args.interleaved)
    args.single = pe_inference.unpaired_input(args.single, args.count_singles, pe_inference._rank_world()[1], args.interleaved,
                                              pe_text_from=args.pe_text_from, check_names=args.check_names, bam_by_name=args.bam_by_name,
                                              fwd=args.fwd, rve=args.rve)
    why = depth_profile_refusal(args) or depth_pileup_refusal(args) or depth_strands_refusal(args) or depth_indels_refusal(args) or depth_site_pairs_refusal(args)
    if why is not None:
        raise ValueError(why)
    if args.depth_from_reads:
        why = depth_from_reads_refusal(args, pe_inference._rank_world()[1])
        if why is not None:
            raise ValueError(why)
    if args.contigs_fasta is not None:
        why = contigs_fasta_refusal(args, pe_inference._rank_world()[1])
        if why is not None:
            raise ValueError(why)
    if (not args.gfa_file) or (not os.path.exists(args.gfa_file)):
        _bail("\nPath to the assembly graph is required, (.gfa format)", "Please ensure the path is correct")
    args.pe_text_files = None
    if args.pe_text_from is not None:
        args.pe_text_files = pe_text_pair(args.pe_text_from)
        if args.pe_text_files is None:
            _bail("\nPath to the paired-end information (--pe-text-from) must hold pe_info.gz and st_info.gz, or pe_info and st_info",
                  "Please ensure the path is correct")
    args.assembler = args.assembler.lower()
    if args.contigs_fasta is not None:
        if not os.path.exists(args.contigs_fasta):
            _bail("\nPath to the contigs (--contigs-fasta, .fasta format) does not exist", "Please ensure the path is correct")
    elif (not args.path_file) or (not os.path.exists(args.path_file)):
        _bail("\nPath to Contig file from SPAdes (.paths format) is required for SPAdes assmbler option. e.g., contigs.paths")
    if args.min_len is not None:
        if args.min_len < 0:
            _bail("\nPlease make sure to provide the correct option (invalid value for min_len or min_cov).")
    else:
        args.min_len = 250
    if args.min_cov is not None and args.min_cov < 0:
        _bail("\nPlease make sure to provide the correct option (invalid value for min_len or min_cov).")
    if args.ref_file:
        _bail("\n-r/--reference_fa is the reference's minimap2 debug mode and is not part of this build")
    if args.output_dir[-1] == "/":
        args.output_dir = args.output_dir[:-1]

    os.makedirs(args.output_dir, exist_ok=True)
    try:
        for sub in ("/gfa/", "/tmp/", "/paf/", "/aln/"):
            os.makedirs(args.output_dir + sub)
    except OSError:
        print("\nCurrent output directory is not empty")
        print("Please empty/re-create the output directory: " + str(args.output_dir))
        _bail()
    if os.path.exists(args.output_dir + "/vstrains.log"):
        os.remove(args.output_dir + "/vstrains.log")

    logger = logging.getLogger("VStrains %s" % __version__)
    logger.setLevel(logging.DEBUG if args.dev else logging.INFO)
    console = logging.StreamHandler()
    console.setLevel(logging.INFO)
    console.setFormatter(logging.Formatter("%(message)s"))
    logger.addHandler(console)
    to_file = logging.FileHandler(args.output_dir + "/vstrains.log")
    to_file.setLevel(logging.DEBUG if args.dev else logging.INFO)
    to_file.setFormatter(logging.Formatter("%(message)s"))
    logger.addHandler(to_file)

    logger.info("Welcome to VStrains!")
    logger.info("VStrains is a strain-aware assembly tools, which constructs full-length ")
    logger.info("virus strain with aid from de Bruijn assembly graph and contigs.")
    logger.info("")
    logger.info("System information:")
    try:
        logger.info("  VStrains version: " + str(__version__).strip())
        logger.info("  Python version: " + ".".join(map(str, sys.version_info[0:3])))
        logger.info("  OS: " + platform.platform())
    except Exception:
        logger.info("  Problem occurred when getting system information")
    logger.info("")
    start = time.time()
    logger.info("Input arguments:")
    logger.info("Assembly type: " + args.assembler)
    logger.info("Assembly graph file: " + args.gfa_file)
    logger.info("Forward read file: " + args.fwd)
    logger.info("Reverse read file: " + args.rve)
    logger.info("Contig paths file: " + (args.path_file if args.contigs_fasta is None else "threaded from " + args.contigs_fasta))
    logger.info("Output directory: " + os.path.abspath(args.output_dir))
    if args.dev:
        logger.info("*DEBUG MODE is turned ON")
    logger.info("\n\n")
    logger.info("======= VStrains pipeline started. Log can be found here: " + os.path.abspath(args.output_dir)
                + "/vstrains.log\n")
    stamped = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
    console.setFormatter(stamped)
    to_file.setFormatter(stamped)

    from .graph import pipeline

    if backend is None and (args.no_pe_text or args.sparse_pe_text or args.bgzf_pe_text or args.bam_by_name or args.interleaved or
                            args.check_names or args.single or args.depth_from_reads or args.contigs_fasta is not None):
        from .graph.hip_ops import HipBackend

        backend = HipBackend(args.device, write_info_text=not args.no_pe_text, sparse_info_text=args.sparse_pe_text,
                             bgzf_info_text=args.bgzf_pe_text, bam_by_name=args.bam_by_name, interleaved=args.interleaved,
                             check_names=args.check_names, single=args.single, count_singles=args.count_singles,
                             interleaved_shard=args.interleaved_shard)
    elif backend is not None:
        if args.single:
            backend.single = list(args.single)
        if args.count_singles:
            backend.count_singles = True
        if args.check_names:
            backend.check_names = args.check_names
        if args.interleaved:
            backend.interleaved = args.interleaved
            backend.interleaved_shard = args.interleaved_shard
        if args.bam_by_name:
            backend.bam_by_name = True
        if args.sparse_pe_text:
            backend.sparse_info_text = True
        if args.bgzf_pe_text:
            backend.bgzf_info_text = True

    old_err = numpy.seterr(all="raise")  # vstrains:25
    try:
        if args.depth_from_reads:
            depth_from_reads(args, logger, backend.ctx)
        if args.contigs_fasta is not None:
            contigs_fasta(args, logger, backend.ctx)
        timings = pipeline.run(args, logger, backend)
    except BaseException:
        logger.removeHandler(to_file)
        logger.removeHandler(console)
        to_file.close()
        raise
    finally:
        numpy.seterr(**old_err)

    elapsed = time.time() - start
    console.setFormatter(logging.Formatter("%(message)s"))
    to_file.setFormatter(logging.Formatter("%(message)s"))
    logger.info("")
    logger.info("Thanks for using VStrains")
    logger.info("Result is stored in {0}/strain.fasta".format(os.path.abspath(args.output_dir)))
    logger.info("You can visualise the path stored in {0}/strain.paths via {0}/gfa/graph_L0.gfa".format(
        os.path.abspath(args.output_dir)))
    logger.info("Finished: {0}".format(date.today().strftime("%B %d, %Y")))
    logger.info("Elapsed time: {0}".format(elapsed))
    logger.info("Exiting...")
    logger.removeHandler(to_file)
    logger.removeHandler(console)
    to_file.close()
    return timings


if __name__ == "__main__":
    main()
    sys.exit(0)
