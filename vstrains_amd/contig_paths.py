#!/usr/bin/env python3
"""Contigs threaded through the graph on the device: write SPAdes' ``contigs.paths`` for a ``contigs.fasta`` and a GFA.

    python -m vstrains_amd.contig_paths -g graph.gfa -c contigs.fasta -o contigs.paths [-k K] [--device D]

The reference takes every contig's walk from the assembler's ``contigs.paths`` (utils/VStrains_IO.py) and has no counterpart
of this.  A contig that spells a walk of the graph is a chain of maximal exact matches against consecutive segments, each
overlapping the next by k bases.  With K = k + 1, window i of a contig is ``c[i : i + K]`` and its hits are the (segment,
strand, pos) whose text holds it; left to right a window CONTINUES its segment, CROSSES from a segment's last window to a
first window (a new token), opens a NEW PART (``;``) or, without a hit, ends the part (``tests/contig_thread_model.py``).
The matches are found on the device (``Context.contig_mems``), chained on the host (``pe.contig_chain``).  A contig without
a hit, or shorter than K, is left out.  Matching is exact: a changed base cuts a contig into ``;`` parts, which the parser
of ``.paths`` files handles.  ``L`` lines are not looked at; the parser checks the walks against them itself.
"""
import argparse
import gzip
import re
import sys
from typing import List, Optional, Sequence, Tuple

MAX_CONTIG = (1 << 24) - 1  # bases a read block holds per end
SPADES_NAME = re.compile(r"NODE_(.*)_length_(.*)_cov_(.*)")


def read_fasta(path: str) -> Tuple[List[str], List[str]]:
    """-> (the first word of every header, the sequences in upper case).  Records may span lines, ``\\r\\n`` is accepted, a
    ``.gz`` file is read through gzip.  ``ValueError``, by name, for a record of more than 2^24 - 1 bases."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as fh:
        raw = fh.read()
    names: List[str] = []
    seqs: List[str] = []
    chunks: Optional[List[bytes]] = None

    def close():
        if chunks is not None:
            seq = b"".join(chunks).upper().decode("latin-1")
            if len(seq) > MAX_CONTIG:
                raise ValueError("contig %s holds %d bases: more than the %d a block takes per sequence" % (names[-1], len(seq), MAX_CONTIG))
            seqs.append(seq)

    for line in raw.split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            close()
            words = line[1:].split()
            names.append(words[0].decode("latin-1") if words else "")
            chunks = []
        elif chunks is not None:
            chunks.append(line.strip())
        elif line.strip():
            raise ValueError("%s: text in front of the first '>' header" % path)
    close()
    return names, seqs


def segment_depths(raw: bytes) -> List[Optional[float]]:
    """The depth of every ``S`` line in file order as ``prep.load_assembly_graph`` reads it (``DP``, else ``KC / LN``);
    None where the line carries neither."""
    out: List[Optional[float]] = []
    for line in raw.splitlines():
        rec = line.decode("latin-1").split("\t")
        if rec[0] != "S":
            continue
        dp = 0.0
        ln = kc = 0
        for tag in rec[3:]:
            if tag.startswith("dp") or tag.startswith("DP"):
                dp = float(tag.split(":")[2])
                break
            if tag.startswith("ln") or tag.startswith("LN"):
                ln = int(tag.split(":")[2])
            if tag.startswith("kc") or tag.startswith("KC"):
                kc = int(tag.split(":")[2])
            if ln != 0 and kc != 0:
                break
        if dp == 0 and ln != 0 and kc != 0:
            dp = kc / ln
        out.append(dp if dp != 0 else None)
    return out


def contig_name(header: str, ordinal: int, bases: int, parts, depths: Sequence[Optional[float]], ids: Sequence[str]) -> str:
    """A header whose first word is a SPAdes name keeps it; any other contig is ``NODE_<ordinal>_length_<bases>_cov_<c>``, c
    the mean depth of its chosen segments weighted by the windows each was chosen for."""
    if SPADES_NAME.fullmatch(header):
        return header
    total = 0
    acc = 0.0
    for part in parts:
        for seg, _strand, windows in part:
            if depths[seg] is None:
                raise ValueError("contig %r needs a name with a coverage, and segment %s carries no depth tag: run "
                                 "vstrains_amd.node_depth (or cli --depth-from-reads) on the graph first" % (header, ids[seg]))
            acc += depths[seg] * windows
            total += windows
    return "NODE_%d_length_%d_cov_%s" % (ordinal, bases, repr(acc / total))


def format_entry(name: str, parts, ids: Sequence[str]) -> str:
    """The forward entry and its mirror ``NAME'``: parts reversed, tokens reversed, signs flipped."""
    fwd = [[ids[seg] + "+-"[strand] for seg, strand, _ in part] for part in parts]
    rev = [[ids[seg] + "-+"[strand] for seg, strand, _ in reversed(part)] for part in reversed(parts)]
    return "".join("%s\n%s\n" % (nm, ";\n".join(",".join(p) for p in pp)) for nm, pp in ((name, fwd), (name + "'", rev)))


def thread_contigs(ctx, gfa: str, fasta: str, kmer_size: Optional[int] = None, parsed=None):
    """Index the segments of ``gfa`` (this replaces the context's index) and thread every contig of ``fasta`` (``parsed``: what
    ``read_fasta`` gave for it, if the caller has read it already).
    -> (the text of the .paths file, tallies: contigs threaded / gapped / left out, ambiguous windows, k)."""
    from . import node_depth
    from . import pe as host

    with open(gfa, "rb") as fh:
        raw = fh.read()
    k = kmer_size if kmer_size is not None else node_depth.infer_k(raw)
    headers, contigs = parsed if parsed is not None else read_fasta(fasta)
    ids, seqs = host.read_gfa_segments(gfa)
    depths = segment_depths(raw)
    ctx.build_index(seqs, k)
    ctx.keep_masks(True)  # (an 'N' of a contig has to bound a match)
    try:
        block = ctx.pack_singles(contigs)
        try:
            mems = ctx.contig_mems(block)
        finally:
            block.free()
    finally:
        ctx.keep_masks(False)
    parts, ambiguous = host.contig_chain(mems, [len(s) for s in seqs], k, len(contigs))
    out = []
    tally = dict(threaded=0, gapped=0, left_out=0, ambiguous_windows=sum(ambiguous), k=k)
    for c, pp in enumerate(parts):
        if not pp:
            tally["left_out"] += 1
            continue
        tally["threaded"] += 1
        tally["gapped"] += len(pp) > 1
        out.append(format_entry(contig_name(headers[c], c + 1, len(contigs[c]), pp, depths, ids), pp, ids))
    return "".join(out), tally


def tally_line(tally: dict) -> str:
    return ("k = %d, %d contigs threaded, %d of them gapped, %d left out (no match of k + 1 bases), %d ambiguous windows"
            % (tally["k"], tally["threaded"], tally["gapped"], tally["left_out"], tally["ambiguous_windows"]))


def refuse_ranks(world: int) -> None:
    if world > 1:
        raise ValueError("contigs are threaded in one process only; sharing the pass among the %d ranks of this process group is not "
                         "built: run without torchrun" % world)


def build_parser():
    p = argparse.ArgumentParser(prog="contig_paths", description="Thread contigs through a GFA on the device and write them as a SPAdes .paths file")
    p.add_argument("-g", "--gfa", dest="gfa", type=str, required=True, help="graph, .gfa format")
    p.add_argument("-c", "--contigs", dest="contigs", type=str, required=True, help="contigs, .fasta format (.gz accepted)")
    p.add_argument("-o", "--output", dest="out", type=str, required=True, help="the .paths file to write")
    p.add_argument("-k", "--kmer_size", dest="kmer_size", type=int, default=None, help="kmer size [default: the overlap of the L lines]")
    p.add_argument("--device", dest="device", type=int, default=0, help="HIP device ordinal")
    return p


def main(argv=None) -> int:
    import os

    args = build_parser().parse_args(argv)
    try:
        refuse_ranks(int(os.environ.get("WORLD_SIZE", "1")))  # (before a device is opened)
        parsed = read_fasta(args.contigs)
        from . import pe as host

        ctx = host.Context(args.device)
        text, tally = thread_contigs(ctx, args.gfa, args.contigs, args.kmer_size, parsed=parsed)
    except ValueError as e:
        print("contig_paths: %s" % e, file=sys.stderr)
        return 1
    with open(args.out, "w") as fh:
        fh.write(text)
    print("contig_paths: %s; result stored in: %s" % (tally_line(tally), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
