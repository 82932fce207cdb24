#!/usr/bin/env python3
"""Segment depth from the reads, counted on the device: write a GFA again with ``LN:i`` / ``KC:i`` tags made from a read set.

    python -m vstrains_amd.node_depth -g IN.gfa -o OUT.gfa -f R1 -r R2 [-k K] [--device D] [the input flags of pe_inference]

The reference takes a segment's depth from the assembler's ``DP:f`` or ``KC:i / LN:i`` tag (utils/VStrains_IO.py:49-77) and
has no counterpart of this.  ``KC`` is SPAdes' number: the (k+1)-mer occurrences of the segment in the reads.  With K = k + 1,
``KC[n]`` is the number of triples (read end, read offset i, entry of segment n in the table of the segments' (k+1)-mers,
PE_Inference.py:117-135) whose read window ``end[i : i + K]`` is a key holding that entry (``tests/node_depth_model.py``);
every end of the input counts, whatever its mate is like.  No ``DP:f`` is written: the reference's own rule ``kc / ln`` then
applies, exactly as for a SPAdes GFA.

    ... --profile FILE [--profile-summary FILE] [--depth-stat {sum,median}]

With any of these the same single pass keeps the triples apart by their entry's forward offset ``p`` (``pe.CoverCounter``,
``tests/depth_profile_model.py``): ``cov[n][p]`` belongs to the WINDOW of ``k + 1`` bases that starts at ``p`` -- k-mer
coverage, not base coverage -- and ``KC[n]`` is the sum of its row.  ``--profile`` writes it as a bedGraph, ``--profile-summary``
as one line per segment, ``--depth-stat median`` puts ``median * LN`` into ``KC:i``.

    ... --pileup FILE[.gz] [--variants FILE[.gz]] [--pileup-max-mismatch M] [--min-alt-count C] [--min-alt-frac F]

With ``--pileup`` or ``--variants`` the same read pass also lays every end along the diagonal of each exact anchor of ``k + 1``
bases ACROSS its mismatches (``pe.PileupCounter``, ``tests/pileup_model.py``): an alignment with at most ``M`` non-agreeing
positions in its overlap adds one to the depth of every position it covers and is written down where it differs -- BASE
coverage, substitutions only, no base qualities.  ``--pileup`` writes the A/C/G/T/other table of every position, ``--variants``
the minor bases above the two thresholds as VCF 4.2.

    ... --site-pairs FILE[.gz] [--sites VCF[.gz]] [--site-pairs-max-span D]

    ... --strands [--min-alt-strand-count S]

With ``--strands`` the pileup keeps the alignments on a segment's forward text and those on its reverse complement apart
(``pe.StrandPileupCounter``, ``tests/strand_pileup_model.py``; still one read pass): ``--pileup`` gets the columns of both
strands, and the records of ``--variants`` are found on the device (``vs_pileup_call``) and carry ``DP4`` -- reads of either
strand with the reference and with the alternate base.  With ``S`` a record whose alternate base has fewer than ``S`` reads on
a strand gets the FILTER ``strand``, every other one ``PASS``; no record is removed.

    ... --indels FILE[.gz] [--indel-max-length G] [--min-indel-count C] [--min-indel-frac F]

With ``--indels`` the same read pass also finds every insertion or deletion of at most ``G`` bases that one read end carries
against one strand of a segment, with ``k + 1`` exact bases on each side (``pe.IndelCounter``, ``tests/indel_model.py``) -- the
ends the pileup rejects on both diagonals -- and writes the events, left-aligned and counted by strand, as a VCF 4.2 of its own;
the depth they are measured against is the pileup's at the anchor base, so the pileup pass runs too.

With ``--site-pairs`` the pass also keeps together what ONE fragment -- the two mates of a pair -- carries at a list of sites
(``pe.SitePairCounter``, ``tests/site_pairs_model.py``) and writes, for every two sites of one segment at most ``D`` positions
apart, how many fragments carry which two bases: which minor bases travel together.  The sites are the CHROM / POS of
``--sites`` (one read pass), or without it the records of ``--variants``, for which the reads are read a second time.
"""
import argparse
import contextlib
import io
import os
import sys

DEPTH_TAGS = ("dp", "DP", "kc", "KC", "ln", "LN")


def _is_depth_tag(field: bytes) -> bool:
    return field[:2].decode("latin-1") in DEPTH_TAGS and field[2:3] == b":"


def profile_runs(offsets, cov, n: int):
    """The maximal runs of equal counts of segment ``n``: (start, end, count), 0-based half-open window starts."""
    import numpy as np

    row = np.asarray(cov[int(offsets[n]):int(offsets[n + 1])])
    if not row.size:
        return []
    cut = np.flatnonzero(row[1:] != row[:-1]) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [row.size]))
    return list(zip(starts.tolist(), ends.tolist(), row[starts].tolist()))


def _open_text(path: str):
    if path.endswith(".gz"):
        import gzip

        return gzip.open(path, "wt", encoding="latin-1", newline="\n")
    return open(path, "w", encoding="latin-1", newline="\n")


def write_bedgraph(path: str, ids, offsets, cov) -> None:
    """``segment<TAB>start<TAB>end<TAB>count``, one line per maximal run of equal counts, runs of 0 included: every segment of
    ``k + 1`` bases or more is covered from 0 to ``len - k``, a shorter one has no line.  Segments in file order, no track
    line; a name ending in ``.gz`` is written through gzip.  The positions are window STARTS (k-mer coverage)."""
    with _open_text(path) as fh:
        for n, name in enumerate(ids):
            fh.write("".join("%s\t%d\t%d\t%d\n" % (name, a, b, v) for a, b, v in profile_runs(offsets, cov, n)))


def read_bedgraph(path: str, ids):
    """What ``write_bedgraph`` wrote, back as ``(offsets, cov)`` over ``ids`` (a segment without a line: an empty range)."""
    import gzip

    import numpy as np

    rows = dict((name, []) for name in ids)
    with (gzip.open(path, "rt", encoding="latin-1") if path.endswith(".gz") else open(path, encoding="latin-1")) as fh:
        for line in fh:
            name, a, b, v = line.rstrip("\n").split("\t")
            row = rows[name]
            if int(a) != len(row) or int(b) <= int(a):
                raise ValueError("%s: the runs of %s do not follow each other at %s" % (path, name, a))
            row.extend([int(v)] * (int(b) - int(a)))
    offsets = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum([len(rows[name]) for name in ids], out=offsets[1:])
    return offsets, np.array([v for name in ids for v in rows[name]], dtype=np.int64)


SUMMARY_COLUMNS = ("segment", "length", "windows", "KC", "breadth", "min", "median", "max")


def profile_summary(lengths, offsets, cov):
    """Per segment (length, windows, KC, breadth, min, median, max), all integers: ``breadth`` the windows with a count
    above 0, ``median`` the lower median (the sorted value at index ``(windows - 1) // 2``); a segment without windows gets
    zeros."""
    import numpy as np

    out = []
    for n, ln in enumerate(lengths):
        row = np.sort(np.asarray(cov[int(offsets[n]):int(offsets[n + 1])], dtype=np.int64))
        if not row.size:
            out.append((int(ln), 0, 0, 0, 0, 0, 0))
            continue
        out.append((int(ln), int(row.size), int(row.sum()), int((row > 0).sum()), int(row[0]), int(row[(row.size - 1) // 2]), int(row[-1])))
    return out


def write_summary(path: str, ids, lengths, offsets, cov) -> None:
    """A TSV with a header line and the columns of ``SUMMARY_COLUMNS``, one line per segment in file order."""
    with _open_text(path) as fh:
        fh.write("\t".join(SUMMARY_COLUMNS) + "\n")
        for name, row in zip(ids, profile_summary(lengths, offsets, cov)):
            fh.write("%s\t%s\n" % (name, "\t".join(str(v) for v in row)))


def depth_stat(stat: str, lengths, offsets, cov):
    """The number that goes into ``KC:i``, per segment: ``sum`` -- the row sum, the depth pass's own ``KC``; ``median`` --
    ``median * LN``, so that the reference's ``kc / ln`` is the lower median of the windows exactly."""
    rows = profile_summary(lengths, offsets, cov)
    if stat == "sum":
        return [r[2] for r in rows]
    if stat == "median":
        return [r[5] * r[0] for r in rows]
    raise ValueError("no depth statistic %r" % (stat,))


PILEUP_COLUMNS = ("segment", "pos", "ref", "A", "C", "G", "T", "other")
VCF_SOURCE = "vstrains_amd.node_depth"


def pileup_counts(seqs, offsets, depth, alt):
    """-> int64 [P, 5]: A, C, G, T, other per position, in the order of ``offsets``: the alt columns as counted, and in the
    column of the segment's own base the depth minus every alt column (the reads that agree there).  A segment whose base
    is not one of ACGT at a position keeps its four columns as counted."""
    import numpy as np

    depth, counts = np.asarray(depth, dtype=np.int64), np.array(alt, dtype=np.int64).reshape(-1, 5)
    for n, seq in enumerate(seqs):
        a, b = int(offsets[n]), int(offsets[n + 1])
        if b == a:
            continue
        ref = np.frombuffer(seq[:b - a].encode("latin-1"), dtype=np.uint8)
        for col, base in enumerate(b"ACGT"):
            at = a + np.flatnonzero(ref == base)
            counts[at, col] = depth[at] - counts[at].sum(axis=1) + counts[at, col]
    return counts


def write_pileup(path: str, ids, seqs, offsets, depth, alt) -> None:
    """A TSV with a header line and the columns of ``PILEUP_COLUMNS``: one row for every position (1-based) of every segment of
    ``k + 1`` bases or more, zeros included, segments in file order; a shorter segment has no row.  ``.gz``: through gzip."""
    counts = pileup_counts(seqs, offsets, depth, alt)
    with _open_text(path) as fh:
        fh.write("\t".join(PILEUP_COLUMNS) + "\n")
        for n, name in enumerate(ids):
            a, b = int(offsets[n]), int(offsets[n + 1])
            seq = seqs[n]
            fh.write("".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((name, p + 1, seq[p]) + tuple(counts[a + p].tolist())) for p in range(b - a)))


def variant_records(ids, seqs, offsets, depth, alt, min_alt_count: int = 2, min_alt_frac: float = 0.01):
    """(segment, 1-based pos, ref, alt base, DP, AD) of every (position, non-reference base) with ``AD >= min_alt_count`` and
    ``AD >= min_alt_frac * DP`` (and, whatever the thresholds, at least one read), ``DP = A + C + G + T``; in file order, then by position, then by base in ACGT order."""
    counts = pileup_counts(seqs, offsets, depth, alt)
    out = []
    for n, name in enumerate(ids):
        a, b = int(offsets[n]), int(offsets[n + 1])
        seq = seqs[n]
        for p in range(b - a):
            row = counts[a + p, :4].tolist()
            dp = sum(row)
            for base, ad in zip("ACGT", row):
                if base != seq[p] and ad > 0 and ad >= min_alt_count and ad >= min_alt_frac * dp:
                    out.append((name, p + 1, seq[p], base, dp, ad))
    return out


def write_vcf(path: str, ids, seqs, offsets, depth, alt, min_alt_count: int = 2, min_alt_frac: float = 0.01) -> None:
    """VCF 4.2: ``fileformat``, ``source``, a ``contig`` line per segment that has rows, ``INFO`` DP, AD, AF, and one biallelic
    record per entry of ``variant_records``; ``AF = "%.6f" % (AD / DP)``, ``ID``, ``QUAL`` and ``FILTER`` are ``.``."""
    with _open_text(path) as fh:
        fh.write("##fileformat=VCFv4.2\n##source=%s\n" % VCF_SOURCE)
        for n, name in enumerate(ids):
            if offsets[n + 1] > offsets[n]:
                fh.write("##contig=<ID=%s,length=%d>\n" % (name, len(seqs[n])))
        fh.write('##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads carrying A, C, G or T at the position">\n'
                 '##INFO=<ID=AD,Number=1,Type=Integer,Description="Reads carrying the alternate base">\n'
                 '##INFO=<ID=AF,Number=1,Type=Float,Description="AD / DP">\n'
                 "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, pos, ref, base, dp, ad in variant_records(ids, seqs, offsets, depth, alt, min_alt_count, min_alt_frac):
            fh.write("%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d;AF=%.6f\n" % (name, pos, ref, base, dp, ad, ad / dp))


STRAND_PILEUP_COLUMNS = ("segment", "pos", "ref", "A+", "C+", "G+", "T+", "other+", "A-", "C-", "G-", "T-", "other-")
BASES = "ACGT"


def strand_pileup_counts(seqs, offsets, depth, alt):
    """-> int64 [P, 2, 5]: ``pileup_counts`` per plane (``pe.StrandPileupCounter.result``: depth [P, 2], alt [P, 2, 5])."""
    import numpy as np

    depth, alt = np.asarray(depth, dtype=np.int64).reshape(-1, 2), np.asarray(alt, dtype=np.int64).reshape(-1, 2, 5)
    return np.stack([pileup_counts(seqs, offsets, depth[:, t], alt[:, t]) for t in range(2)], axis=1)


def write_strand_pileup(path: str, ids, seqs, offsets, depth, alt) -> None:
    """``write_pileup`` with the columns of ``STRAND_PILEUP_COLUMNS``: ``+`` the reads laid along the segment's forward text,
    ``-`` those along its reverse complement, every base as it reads on the forward strand."""
    counts = strand_pileup_counts(seqs, offsets, depth, alt).reshape(-1, 10)
    with _open_text(path) as fh:
        fh.write("\t".join(STRAND_PILEUP_COLUMNS) + "\n")
        for n, name in enumerate(ids):
            a, b = int(offsets[n]), int(offsets[n + 1])
            seq = seqs[n]
            fh.write("".join("%s\t%d\t%s\t%s\n" % (name, p + 1, seq[p], "\t".join(str(v) for v in counts[a + p].tolist())) for p in range(b - a)))


def call_host(seqs, offsets, depth, alt, min_alt_count: int = 2, min_alt_frac: float = 0.01, min_alt_strand: int = 0):
    """What ``pe.StrandPileupCounter.call`` (depth [P, 2], alt [P, 2, 5]) or ``pe.PileupCounter.call`` (depth [P], alt [P, 5])
    gives, made on the host from the tables of ``result()``, position by position through the rule the device runs
    (``pe.pileup_call_host``): for small tables and tests; no device is needed.  A position whose base is not one of ACGT has
    no records."""
    import numpy as np

    from . import pe as host

    depth = np.asarray(depth, dtype=np.int64)
    planes = 2 if depth.ndim == 2 else 1
    depth, alt = depth.reshape(-1, planes), np.asarray(alt, dtype=np.int64).reshape(-1, planes, 5)
    rows = []
    for n, seq in enumerate(seqs):
        a, b = int(offsets[n]), int(offsets[n + 1])
        for p in range(b - a):
            if seq[p] in BASES:
                rows += [(n, p) + r for r in host.pileup_call_host(BASES.index(seq[p]), depth[a + p], alt[a + p], min_alt_count, min_alt_frac, min_alt_strand)]
    got = np.array(rows, dtype=np.int64).reshape(-1, 10)
    return got[:, 0], got[:, 1], got[:, 3], got[:, 4], got[:, 5], got[:, 6:10], got[:, 2].astype(bool)


def strand_records(ids, called, min_alt_strand: int = 0):
    """(segment, 1-based pos, ref, alt base, DP, AD, (ref_f, ref_r, alt_f, alt_r), FILTER) of every record a counter's
    ``call()`` found, in its order; FILTER: ``.`` without a strand threshold, else ``PASS`` or ``strand``."""
    seg, pos0, ref, alt, dp, dp4, fail = called
    return [(ids[int(n)], int(p) + 1, BASES[int(r)], BASES[int(b)], int(d), int(q[2] + q[3]), tuple(int(v) for v in q),
             "." if min_alt_strand < 1 else ("strand" if f else "PASS"))
            for n, p, r, b, d, q, f in zip(seg, pos0, ref, alt, dp, dp4, fail)]


def write_strand_vcf(path: str, ids, seqs, offsets, called, min_alt_strand: int = 0) -> None:
    """``write_vcf`` from the records of ``pe.StrandPileupCounter.call``: INFO gains ``DP4``; with a strand threshold the
    header gains the FILTER ``strand`` and every record says ``PASS`` or ``strand``, else FILTER stays ``.``.  With
    ``;DP4=...`` and the FILTER value dropped the records are ``write_vcf``'s, byte for byte."""
    with _open_text(path) as fh:
        fh.write("##fileformat=VCFv4.2\n##source=%s\n" % VCF_SOURCE)
        for n, name in enumerate(ids):
            if offsets[n + 1] > offsets[n]:
                fh.write("##contig=<ID=%s,length=%d>\n" % (name, len(seqs[n])))
        fh.write('##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads carrying A, C, G or T at the position">\n'
                 '##INFO=<ID=AD,Number=1,Type=Integer,Description="Reads carrying the alternate base">\n'
                 '##INFO=<ID=AF,Number=1,Type=Float,Description="AD / DP">\n'
                 '##INFO=<ID=DP4,Number=4,Type=Integer,Description="Reads along the forward text with the reference base, along the reverse '
                 'complement with it, along the forward text with the alternate base, along the reverse complement with it">\n')
        if min_alt_strand >= 1:
            fh.write('##FILTER=<ID=strand,Description="Fewer than %d reads carry the alternate base on one of the two strands">\n' % min_alt_strand)
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, pos, ref, base, dp, ad, dp4, flt in strand_records(ids, called, min_alt_strand):
            fh.write("%s\t%d\t.\t%s\t%s\t.\t%s\tDP=%d;AD=%d;AF=%.6f;DP4=%d,%d,%d,%d\n" % ((name, pos, ref, base, flt, dp, ad, ad / dp) + dp4))


INDEL_TALLIES = ("matches tested", "deletions", "insertions", "insertions dropped")


def indel_records(ids, seqs, events, offsets, depth, alt, min_count: int = 2, min_frac: float = 0.01, min_strand: int = 0):
    """The records of ``--indels`` from the events of ``pe.IndelCounter.result`` -- ``(seg, pos0, kind, length, insert, count_f,
    count_r)`` -- and the tables of a pileup counter's ``result()`` (with or without the plane axis): ``(segment, 1-based POS,
    REF, ALT, DP, AD, ADF, ADR, FILTER)``, one per event, in the events' order.  With ``pos0 = u > 0`` the anchor is ``F[u-1]``
    and POS is ``u``: ``F[u-1 : u+L]`` / ``F[u-1]`` for a deletion, ``F[u-1]`` / ``F[u-1] + I`` for an insertion; with
    ``u == 0`` the anchor is the base BEHIND the event and POS is 1: ``F[0 : L+1]`` / ``F[L]``, and ``F[0]`` / ``I + F[0]``.
    ``AD = ADF + ADR``; ``DP = AD +`` the reads the pileup has with A, C, G or T at the anchor.  A record needs ``AD >=
    min_count`` and ``AD >= min_frac * DP``, one double product compared as it stands.  FILTER: ``.`` without a strand
    threshold, else ``PASS`` when both ``ADF`` and ``ADR`` reach it, else ``strand``; no record is removed for it."""
    import numpy as np

    depth = np.asarray(depth, dtype=np.int64)
    alt = np.asarray(alt, dtype=np.int64)
    if depth.ndim == 2:  # (the planes of pe.StrandPileupCounter: the depth an event is measured against is that of both)
        depth, alt = depth.sum(axis=1), alt.reshape(-1, 2, 5).sum(axis=1)
    alt = alt.reshape(-1, 5)
    out = []
    for n, u, kind, length, insert, adf, adr in events:
        seq = seqs[n]
        if u > 0:
            at, pos = u - 1, u
            ref, new = (seq[u - 1:u + length], seq[u - 1]) if kind == 0 else (seq[u - 1], seq[u - 1] + insert)
        else:
            at, pos = (length, 1) if kind == 0 else (0, 1)
            ref, new = (seq[0:length + 1], seq[length]) if kind == 0 else (seq[0], insert + seq[0])
        row = int(offsets[n]) + at
        here = int(depth[row] - alt[row, 4]) if seq[at] in BASES else int(alt[row, :4].sum())
        ad = adf + adr
        dp = ad + here
        if ad >= min_count and float(ad) >= min_frac * float(dp):
            out.append((ids[n], pos, ref, new, dp, ad, adf, adr, "." if min_strand < 1 else ("PASS" if adf >= min_strand and adr >= min_strand else "strand")))
    return out


def write_indel_vcf(path: str, ids, seqs, offsets, records, min_strand: int = 0) -> None:
    """VCF 4.2 of the records ``indel_records`` made: the header of ``write_vcf`` with ``ADF`` / ``ADR`` behind ``AF`` and, with a
    strand threshold, the FILTER ``strand``; ``AF = "%.6f" % (AD / DP)``, ``ID`` and ``QUAL`` are ``.``.  ``.gz``: through gzip."""
    with _open_text(path) as fh:
        fh.write("##fileformat=VCFv4.2\n##source=%s\n" % VCF_SOURCE)
        for n, name in enumerate(ids):
            if offsets[n + 1] > offsets[n]:
                fh.write("##contig=<ID=%s,length=%d>\n" % (name, len(seqs[n])))
        fh.write('##INFO=<ID=DP,Number=1,Type=Integer,Description="AD and the reads carrying A, C, G or T at the anchor base">\n'
                 '##INFO=<ID=AD,Number=1,Type=Integer,Description="Read ends carrying the insertion or deletion">\n'
                 '##INFO=<ID=AF,Number=1,Type=Float,Description="AD / DP">\n'
                 '##INFO=<ID=ADF,Number=1,Type=Integer,Description="Read ends carrying it along the forward text">\n'
                 '##INFO=<ID=ADR,Number=1,Type=Integer,Description="Read ends carrying it along the reverse complement">\n')
        if min_strand >= 1:
            fh.write('##FILTER=<ID=strand,Description="Fewer than %d read ends carry the event on one of the two strands">\n' % min_strand)
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, pos, ref, new, dp, ad, adf, adr, flt in records:
            fh.write("%s\t%d\t.\t%s\t%s\t.\t%s\tDP=%d;AD=%d;AF=%.6f;ADF=%d;ADR=%d\n" % (name, pos, ref, new, flt, dp, ad, ad / dp, adf, adr))


def indel_refusal(args, world: int = 1):
    """None, or why the flags of ``--indels`` cannot hold, said before a device is opened."""
    indels = getattr(args, "indels", None)
    length, count, frac = getattr(args, "indel_max_length", None), getattr(args, "min_indel_count", None), getattr(args, "min_indel_frac", None)
    if length is not None and not 1 <= length <= 32:
        return "--indel-max-length %d: a length from 1 to 32 is needed" % length
    if count is not None and count < 0:
        return "--min-indel-count %d: a count from 0 up is needed" % count
    if frac is not None and not 0.0 <= frac <= 1.0:
        return "--min-indel-frac %r: a fraction between 0 and 1 is needed" % frac
    if indels is None and (length is not None or count is not None or frac is not None):
        return "--indel-max-length, --min-indel-count and --min-indel-frac belong to --indels: give it"
    if indels is not None and world > 1:
        return "--indels finds its events in one process only, and this process group has %d ranks: run without torchrun" % world
    return None


def pileup_refusal(args):
    """None, or why the pileup's flags cannot hold, said before a device is opened."""
    asked = args.pileup is not None or args.variants is not None
    if args.pileup_max_mismatch is not None and args.pileup_max_mismatch < 0:
        return "--pileup-max-mismatch %d: the budget is an integer from 0 up" % args.pileup_max_mismatch
    if args.min_alt_count is not None and args.min_alt_count < 0:
        return "--min-alt-count %d: a count from 0 up is needed" % args.min_alt_count
    if args.min_alt_frac is not None and not 0.0 <= args.min_alt_frac <= 1.0:
        return "--min-alt-frac %r: a fraction between 0 and 1 is needed" % args.min_alt_frac
    if not asked and (args.pileup_max_mismatch is not None or args.min_alt_count is not None or args.min_alt_frac is not None):
        return "--pileup-max-mismatch, --min-alt-count and --min-alt-frac belong to --pileup / --variants: give one of them"
    if args.variants is None and (args.min_alt_count is not None or args.min_alt_frac is not None):
        return "--min-alt-count and --min-alt-frac select the records of --variants: give it"
    strands, strand_count = getattr(args, "strands", False), getattr(args, "min_alt_strand_count", None)
    if strands and not asked:
        return "--strands keeps the strands of the pileup apart: give --pileup or --variants with it"
    if strand_count is not None and not (strands and args.variants is not None) and getattr(args, "indels", None) is None:
        return "--min-alt-strand-count filters the records of --variants by strand: give --strands and --variants with it"
    if strand_count is not None and strand_count < 1:
        return "--min-alt-strand-count %d: a count from 1 up is needed" % strand_count
    return None


SITE_PAIR_COLUMNS = ("segment", "pos_a", "pos_b", "base_a", "base_b", "count")
SITE_PAIR_BASES = "ACGTN"  # the five columns of a cell: N is `other`
SITE_PAIR_TALLIES = ("fragments observing", "overflow fragments", "discordant sites", "pairs stored", "pairs unstored")


def read_vcf_sites(path: str, ids, seqs, kmer_size: int):
    """The sites of ``--sites``: any VCF against the segments (``.gz``: through gzip).  Lines that start with ``#`` are skipped
    and only CHROM and POS (1-based) are read.  -> [(segment index in file order, 0-based position)], in the file's order.  A
    ``ValueError`` names an unknown segment, a position outside its segment and a segment shorter than ``k + 1`` bases."""
    import gzip

    index = dict((name, n) for n, name in reversed(list(enumerate(ids))))
    out = []
    with (gzip.open(path, "rt", encoding="latin-1") if path.endswith(".gz") else open(path, encoding="latin-1")) as fh:
        for no, line in enumerate(fh, 1):
            if line.startswith("#") or not line.strip():
                continue
            cols = line.rstrip("\n").split("\t")
            if len(cols) < 2 or not cols[1].lstrip("-").isdigit():
                raise ValueError("%s, line %d: CHROM and an integer POS are needed" % (path, no))
            name, pos = cols[0], int(cols[1])
            if name not in index:
                raise ValueError("%s, line %d: the graph has no segment %s" % (path, no, name))
            n = index[name]
            if len(seqs[n]) < kmer_size + 1:
                raise ValueError("%s, line %d: segment %s has %d bases, fewer than k + 1 = %d: it has no positions" % (path, no, name, len(seqs[n]), kmer_size + 1))
            if not 1 <= pos <= len(seqs[n]):
                raise ValueError("%s, line %d: position %d is outside segment %s of %d bases" % (path, no, pos, name, len(seqs[n])))
            out.append((n, pos - 1))
    return out


def write_site_pairs(path: str, ids, seg, pos_a, pos_b, counts) -> None:
    """A TSV with a header line and the columns of ``SITE_PAIR_COLUMNS``: one row per non-zero count of every stored pair of
    sites (``pe.SitePairCounter.result``); positions 1-based, bases ``A C G T N`` (``N``: a byte outside ACGT); in the order
    of the result, then ``base_a``, ``base_b`` in that column order.  ``.gz``: through gzip."""
    with _open_text(path) as fh:
        fh.write("\t".join(SITE_PAIR_COLUMNS) + "\n")
        for n, a, b, cell in zip(seg, pos_a, pos_b, counts):
            fh.write("".join("%s\t%d\t%d\t%s\t%s\t%d\n" % (ids[int(n)], int(a) + 1, int(b) + 1, SITE_PAIR_BASES[i], SITE_PAIR_BASES[j], int(cell[i][j]))
                             for i in range(5) for j in range(5) if cell[i][j]))


def site_pairs_refusal(args):
    """None, or why the site-pair flags cannot hold, said before a device is opened."""
    if args.site_pairs_max_span is not None and args.site_pairs_max_span < 0:
        return "--site-pairs-max-span %d: a span from 0 up is needed" % args.site_pairs_max_span
    if args.site_pairs is None:
        if args.site_pairs_max_span is not None or args.sites is not None:
            return "--sites and --site-pairs-max-span belong to --site-pairs: give it"
        return None
    if args.sites is None:
        if args.variants is None:
            return "--site-pairs needs its sites: give --sites VCF, or --variants, whose records are then the sites"
        # the sites are known only once the reads have been read: they are read a second time
        for path in [args.fwd, args.rve] + list(args.single):
            if not os.path.isfile(path):
                return ("--site-pairs without --sites reads the reads twice, and %s is not a regular file: write the records with --variants first "
                        "and give them as --sites" % path)
    return None


class _Both:
    """Two counters behind one ``add``: what the input dispatch needs of a counter (``pe_inference.feed_counter``), handed on
    to both, so that the pileup rides on the read pass of the depth."""

    def __init__(self, main, extra):
        self.main, self.extra = main, extra
        self.device, self.single_stats = main.device, main.single_stats

    def add(self, reads):
        self.main.add(reads)
        self.extra.add(reads)


def rewrite_gfa(raw: bytes, kc) -> bytes:
    """``raw`` again, every ``S`` line carrying ``LN:i:<sequence length>`` and ``KC:i:<count>`` right behind its sequence in
    place of any ``dp / DP / kc / KC / ln / LN`` tag it had; its other tags stay, in their order; every other line, and every
    line end (``\\n``, ``\\r\\n``, none at the end of the file), stays byte for byte.  ``kc``: one count per ``S`` line, in file
    order."""
    out = []
    n = 0
    for line in raw.splitlines(keepends=True):
        body = line.rstrip(b"\r\n")
        if not body.startswith(b"S\t"):
            out.append(line)
            continue
        cols = body.split(b"\t")
        if len(cols) < 3:
            raise ValueError("S line %d has no sequence: %r" % (n + 1, body[:60]))
        if n >= len(kc):
            raise ValueError("the GFA holds more S lines than the %d counts given" % len(kc))
        tags = [b"LN:i:%d" % len(cols[2]), b"KC:i:%d" % int(kc[n])] + [t for t in cols[3:] if not _is_depth_tag(t)]
        out.append(b"\t".join(cols[:3] + tags) + line[len(body):])
        n += 1
    if n != len(kc):
        raise ValueError("the GFA holds %d S lines and %d counts were given" % (n, len(kc)))
    return b"".join(out)


def strip_depth_tags(raw: bytes) -> bytes:
    """``raw`` with the depth tags of every ``S`` line taken out (what Bandage, gfatools or awk subsets leave behind)."""
    out = []
    for line in raw.splitlines(keepends=True):
        body = line.rstrip(b"\r\n")
        if body.startswith(b"S\t"):
            cols = body.split(b"\t")
            body = b"\t".join(cols[:3] + [t for t in cols[3:] if not _is_depth_tag(t)])
        out.append(body + line[len(line.rstrip(b"\r\n")):])
    return b"".join(out)


def infer_k(raw: bytes) -> int:
    """The overlap of the ``L`` lines (``<k>M``).  ``ValueError`` when there are none or they disagree."""
    seen = set()
    for line in raw.splitlines():
        if line.startswith(b"L\t"):
            cols = line.split(b"\t")
            ovl = [t for t in cols[5:] if t[-1:] in (b"M", b"m")]
            if not ovl or not ovl[0][:-1].isdigit():
                raise ValueError("an L line has no <k>M overlap: %r" % line[:80])
            seen.add(int(ovl[0][:-1]))
    if not seen:
        raise ValueError("the GFA has no L lines to take k from: give -k")
    if len(seen) > 1:
        raise ValueError("the L lines of the GFA disagree on the overlap (%s): give -k" % ", ".join(str(v) for v in sorted(seen)))
    return seen.pop()


def refuse_ranks(world: int) -> None:
    if world > 1:
        raise ValueError("the depth pass counts in one process only; sharing it among the %d ranks of this process group is not built "
                         "(the sums are additive, so it can follow): run without torchrun" % world)


def depth_pass(ctx, gfa: str, fwd: str, rve: str, kmer_size: int, bam_by_name: bool = False, interleaved=None, check_names=None, single=(),
               count_singles: bool = False, quiet: bool = False, profile: bool = False, pileup=None, site_pairs=None, strands=None, indels=None):
    """Index the segments of ``gfa`` and count every end the chosen input delivers (the input dispatch of
    ``pe_inference.count_links``, one process only).  -> (segment ids in file order, KC int64 in file order, ends counted).
    Replaces the context's index; the context stops keeping masks when the pass is over, so a PE count may follow on it.
    ``quiet``: the dispatch's progress lines are not printed.  ``profile``: the pass counts per window (``pe.CoverCounter``,
    still one kernel per block; KC is its row sums) and a fourth value follows: (segment lengths, offsets, cov).  ``pileup``:
    a mismatch budget; a ``pe.PileupCounter`` then takes every block as well and one more value follows at the end:
    (segment sequences, offsets, depth, alt, (alignments, rejected)).  Without it no such counter is built.  ``site_pairs``:
    (sites, mismatch budget, span); a ``pe.SitePairCounter`` then takes every block as well and its ``result()`` with the five
    tallies behind it follows as the very last value.  ``strands``: ``None``, or (min_alt_count, min_alt_frac, min_alt_strand)
    beside ``pileup``: a ``pe.StrandPileupCounter`` takes the ``PileupCounter``'s place, depth and alt of the pileup's value have
    its plane axis, and what its ``call()`` found on the device with these thresholds follows as that value's sixth member.
    ``indels``: a maximum length; a ``pe.IndelCounter`` then takes every block as well and (its ``result()``, its four tallies)
    follows behind everything else."""
    from . import pe as host
    from . import pe_inference

    rank, world = pe_inference._rank_world()
    refuse_ranks(world)
    inp = pe_inference._resolve_inputs(fwd, rve, world, bam_by_name, interleaved, check_names, single, count_singles, False)
    ids, seqs = host.read_gfa_segments(gfa)
    ctx.build_index(seqs, kmer_size)
    counter = host.CoverCounter(ctx) if profile else host.DepthCounter(ctx)  # (the blocks built from here on keep their masks)
    if strands is not None and pileup is None:
        raise ValueError("the strands are those of the pileup: give its mismatch budget")
    piles = None if pileup is None else (host.PileupCounter if strands is None else host.StrandPileupCounter)(ctx, max_mismatch=pileup)
    linked = host.SitePairCounter(ctx, site_pairs[0], max_mismatch=site_pairs[1], max_span=site_pairs[2]) if site_pairs is not None else None
    fed = counter if piles is None else _Both(counter, piles)
    gapped = host.IndelCounter(ctx, max_len=indels) if indels is not None else None
    if gapped is not None:
        fed = _Both(fed, gapped)
    try:
        with contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext():
            pe_inference.feed_counter(ctx, fed if linked is None else _Both(fed, linked), inp, 0, 1, stages_follow=False, tally_singles=False)
        ctx.sync()
    finally:
        ctx.keep_masks(False)
    piled = () if piles is None else ((seqs,) + piles.result() + (piles.tallies(),) + (() if strands is None else (piles.call(*strands),)),)
    if linked is not None:
        piled += (linked.result() + (linked.tallies(),),)
    if gapped is not None:
        piled += ((gapped.result(), gapped.tallies()),)
    if profile:
        offsets, cov = counter.result()
        return (ids, counter.kc(), counter.ends_seen, ([len(q) for q in seqs], offsets, cov)) + piled
    return (ids, counter.result(), counter.ends_seen) + piled


def site_pairs_pass(ctx, sites, fwd: str, rve: str, max_mismatch: int = 8, max_span: int = 1000, bam_by_name: bool = False, interleaved=None,
                    check_names=None, single=(), count_singles: bool = False, quiet: bool = False):
    """The reads once more, through a ``pe.SitePairCounter`` alone, on the index the context holds (``depth_pass`` built it):
    the second pass of ``--site-pairs`` without ``--sites``, whose sites are known only when the first is over.
    -> (seg, pos_a, pos_b, counts, the five tallies)."""
    from . import pe as host
    from . import pe_inference

    rank, world = pe_inference._rank_world()
    refuse_ranks(world)
    inp = pe_inference._resolve_inputs(fwd, rve, world, bam_by_name, interleaved, check_names, single, count_singles, False)
    linked = host.SitePairCounter(ctx, sites, max_mismatch=max_mismatch, max_span=max_span)
    try:
        with contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext():
            pe_inference.feed_counter(ctx, linked, inp, 0, 1, stages_follow=False, tally_singles=False)
        ctx.sync()
    finally:
        ctx.keep_masks(False)
    return linked.result() + (linked.tallies(),)


def record_sites(ids, records):
    """The sites of the records ``variant_records`` made: (segment index in file order, 0-based position), each once."""
    index = dict((name, n) for n, name in reversed(list(enumerate(ids))))
    return sorted(set((index[r[0]], r[1] - 1) for r in records))


def build_parser():
    p = argparse.ArgumentParser(prog="node_depth", description="Write a GFA again with LN:i / KC:i tags counted from a read set on the device")
    p.add_argument("-g", "--gfa", dest="gfa", type=str, required=True, help="graph, .gfa format (its depth tags, if any, are replaced)")
    p.add_argument("-o", "--output", dest="out", type=str, required=True, help="the GFA to write")
    p.add_argument("-f", "--forward", dest="fwd", required=True, help="forward read, .fastq")
    p.add_argument("-r", "--reverse", dest="rve", required=True, help="reverse read, .fastq")
    p.add_argument("-k", "--kmer_size", dest="kmer_size", type=int, default=None, help="kmer size [default: the overlap of the L lines]")
    p.add_argument("--device", dest="device", type=int, default=0, help="HIP device ordinal")
    p.add_argument("--bam-by-name", dest="bam_by_name", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--gzip-device", dest="gzip_device", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--interleaved", dest="interleaved", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--interleaved-singles", dest="interleaved_singles", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--check-names", dest="check_names", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--check-names-singles", dest="check_names_singles", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--single", dest="single", action="append", default=[], metavar="FILE", help="as pe_inference (repeatable)")
    p.add_argument("--count-singles", dest="count_singles", action="store_true", default=False, help="as pe_inference")
    p.add_argument("--profile", dest="profile", type=str, default=None, metavar="FILE",
                   help="also write the depth of every window of k + 1 bases as a bedGraph (segment, start, end, count; 0-based half-open "
                        "window STARTS: k-mer coverage, not base coverage; runs of equal counts merged, zeros included; .gz: through gzip)")
    p.add_argument("--profile-summary", dest="profile_summary", type=str, default=None, metavar="FILE",
                   help="also write a TSV per segment: length, windows, KC, breadth (windows with a count above 0), min, lower median, max")
    p.add_argument("--depth-stat", dest="depth_stat", choices=("sum", "median"), default=None,
                   help="what KC:i holds: sum (default) the (k+1)-mer occurrences, as SPAdes; median: the lower median of the windows' "
                        "counts times LN, so that kc / ln is that median")
    p.add_argument("--pileup", dest="pileup", type=str, default=None, metavar="FILE",
                   help="also write the base pileup as a TSV (segment, pos, ref, A, C, G, T, other; pos 1-based; one row per position of every "
                        "segment of k + 1 bases or more, zeros included; base coverage, substitutions only; .gz: through gzip)")
    p.add_argument("--variants", dest="variants", type=str, default=None, metavar="FILE",
                   help="also write the minor bases of the pileup as VCF 4.2 (INFO DP, AD, AF; .gz: through gzip)")
    p.add_argument("--pileup-max-mismatch", dest="pileup_max_mismatch", type=int, default=None, metavar="M",
                   help="non-agreeing positions an alignment may hold in its overlap [default: 8]")
    p.add_argument("--min-alt-count", dest="min_alt_count", type=int, default=None, metavar="C", help="--variants: records need AD >= C [default: 2]")
    p.add_argument("--min-alt-frac", dest="min_alt_frac", type=float, default=None, metavar="F", help="--variants: records need AD >= F * DP [default: 0.01]")
    p.add_argument("--strands", dest="strands", action="store_true", default=False,
                   help="--pileup / --variants: keep the reads laid along a segment's forward text and along its reverse complement apart: the "
                        "pileup gets the columns A+ C+ G+ T+ other+ A- C- G- T- other-, the records are found on the device and carry DP4")
    p.add_argument("--min-alt-strand-count", dest="min_alt_strand_count", type=int, default=None, metavar="S",
                   help="--strands --variants: FILTER is PASS when at least S reads carry the alternate base on EACH strand, else strand; "
                        "no record is removed [default: FILTER stays .]")
    p.add_argument("--indels", dest="indels", type=str, default=None, metavar="FILE",
                   help="also write the insertions and deletions of at most G bases that the read ends carry, k + 1 exact bases on each side, "
                        "left-aligned and counted by strand, as a VCF 4.2 of its own (INFO DP, AD, AF, ADF, ADR; the pileup pass runs too; "
                        ".gz: through gzip)")
    p.add_argument("--indel-max-length", dest="indel_max_length", type=int, default=None, metavar="G", help="--indels: the longest event, 1 to 32 [default: 16]")
    p.add_argument("--min-indel-count", dest="min_indel_count", type=int, default=None, metavar="C", help="--indels: records need AD >= C [default: 2]")
    p.add_argument("--min-indel-frac", dest="min_indel_frac", type=float, default=None, metavar="F", help="--indels: records need AD >= F * DP [default: 0.01]")
    p.add_argument("--site-pairs", dest="site_pairs", type=str, default=None, metavar="FILE",
                   help="also write which bases travel together on one read pair at pairs of sites of one segment, as a TSV (segment, pos_a, pos_b, "
                        "base_a, base_b, count; positions 1-based; non-zero counts only; .gz: through gzip).  The sites: --sites, or the records "
                        "of --variants, for which the reads are read a second time")
    p.add_argument("--sites", dest="sites", type=str, default=None, metavar="VCF",
                   help="--site-pairs: the sites, any VCF against the segments (only CHROM and POS are read; .gz: through gzip); one read pass")
    p.add_argument("--site-pairs-max-span", dest="site_pairs_max_span", type=int, default=None, metavar="D",
                   help="--site-pairs: two sites are linked when at most D positions apart [default: 1000]")
    return p


def main(argv=None) -> int:
    from . import pe_inference

    args = build_parser().parse_args(argv)
    with open(args.gfa, "rb") as fh:
        raw = fh.read()
    k = args.kmer_size
    if k is None:
        try:
            k = infer_k(raw)
        except ValueError as e:
            print("node_depth: %s" % e, file=sys.stderr)
            return 1
    interleaved = pe_inference.interleaved_mode(args.interleaved, args.interleaved_singles)
    check_names = pe_inference.check_names_mode(args.check_names, args.check_names_singles)
    if args.gzip_device:
        os.environ["VS_GZIP_DEVICE"] = "1"
    why = indel_refusal(args, int(os.environ.get("WORLD_SIZE", "1")))
    if why is not None:
        print("node_depth: %s" % why, file=sys.stderr)
        return 1
    refuse_ranks(int(os.environ.get("WORLD_SIZE", "1")))  # (before a device is opened)
    why = pileup_refusal(args) or site_pairs_refusal(args)
    if why is not None:
        print("node_depth: %s" % why, file=sys.stderr)
        return 1
    world = 1
    pe_inference.interleaved_input(args.fwd, args.rve, world, interleaved)
    pe_inference.check_names_input(args.fwd, args.rve, world, check_names, bam_by_name=args.bam_by_name, interleaved=interleaved)
    pe_inference.unpaired_input(args.single, args.count_singles, world, interleaved, check_names=check_names, bam_by_name=args.bam_by_name,
                                fwd=args.fwd, rve=args.rve)
    from . import pe as host

    sites = None
    budget = 8 if args.pileup_max_mismatch is None else args.pileup_max_mismatch
    span = 1000 if args.site_pairs_max_span is None else args.site_pairs_max_span
    if args.sites is not None:
        try:
            sites = read_vcf_sites(args.sites, *host.read_gfa_segments(args.gfa), kmer_size=k)
        except ValueError as e:
            print("node_depth: --sites: %s" % e, file=sys.stderr)
            return 1
    ctx = host.Context(args.device)
    min_count, min_frac = 2 if args.min_alt_count is None else args.min_alt_count, 0.01 if args.min_alt_frac is None else args.min_alt_frac
    strand_count = 0 if args.min_alt_strand_count is None else args.min_alt_strand_count
    profiled = args.profile is not None or args.profile_summary is not None or args.depth_stat is not None
    piled = args.pileup is not None or args.variants is not None or args.indels is not None  # (--indels alone: its depth is the pileup's)
    got = depth_pass(ctx, args.gfa, args.fwd, args.rve, k, bam_by_name=args.bam_by_name, interleaved=interleaved,
                     check_names=check_names, single=args.single, count_singles=args.count_singles, quiet=True, profile=profiled,
                     pileup=budget if piled else None, **(dict(site_pairs=(sites, budget, span)) if sites is not None else {}),
                     **(dict(strands=(min_count, min_frac, strand_count)) if args.strands else {}),
                     **(dict(indels=16 if args.indel_max_length is None else args.indel_max_length) if args.indels is not None else {}))
    ids, kc, ends = got[:3]
    gapped = None
    if args.indels is not None:
        got, gapped = got[:-1], got[-1]
    linked = None
    if sites is not None:
        got, linked = got[:-1], got[-1]
    tags = kc.tolist()
    if profiled:
        lengths, offsets, cov = got[3]
        if args.depth_stat == "median":
            tags = depth_stat("median", lengths, offsets, cov)
        if args.profile is not None:
            write_bedgraph(args.profile, ids, offsets, cov)
        if args.profile_summary is not None:
            write_summary(args.profile_summary, ids, lengths, offsets, cov)
    if piled:
        seqs, p_offsets, p_depth, p_alt = got[-1][:4]
        called = got[-1][5] if args.strands else None
        if args.pileup is not None:
            (write_strand_pileup if args.strands else write_pileup)(args.pileup, ids, seqs, p_offsets, p_depth, p_alt)
        if args.variants is not None and args.strands:
            write_strand_vcf(args.variants, ids, seqs, p_offsets, called, strand_count)
        elif args.variants is not None:
            write_vcf(args.variants, ids, seqs, p_offsets, p_depth, p_alt, min_count, min_frac)
        if gapped is not None:
            write_indel_vcf(args.indels, ids, seqs, p_offsets,
                            indel_records(ids, seqs, gapped[0], p_offsets, p_depth, p_alt, 2 if args.min_indel_count is None else args.min_indel_count,
                                          0.01 if args.min_indel_frac is None else args.min_indel_frac, strand_count), strand_count)
        if args.site_pairs is not None and sites is None:  # the records just written are the sites: the reads once more
            records = strand_records(ids, called) if args.strands else variant_records(ids, seqs, p_offsets, p_depth, p_alt, min_count, min_frac)
            linked = site_pairs_pass(ctx, record_sites(ids, records), args.fwd, args.rve, budget, span, bam_by_name=args.bam_by_name,
                                     interleaved=interleaved, check_names=check_names, single=args.single, count_singles=args.count_singles, quiet=True)
    if linked is not None:
        write_site_pairs(args.site_pairs, ids, *linked[:4])
    text = rewrite_gfa(raw, tags)
    with open(args.out, "wb") as fh:
        fh.write(text)
    stored = args.out + "".join("; %s in: %s" % (what, path) for what, path in (("profile", args.profile), ("summary", args.profile_summary),
                                                                                  ("pileup", args.pileup), ("variants", args.variants),
                                                                                  ("site pairs", args.site_pairs),
                                                                                  ("indels", getattr(args, "indels", None)))
                                if path is not None)
    if linked is not None:
        stored += " (%s)" % ", ".join("%d %s" % (v, what) for v, what in zip(linked[4], SITE_PAIR_TALLIES))
    if gapped is not None:
        stored += " (%s)" % ", ".join("%d %s" % (v, what) for v, what in zip(gapped[1], INDEL_TALLIES))
    print("node_depth: k = %d, %d read ends counted, %d window-entry coincidences (sum of KC), %d of %d segments with KC = 0; result stored in: %s"
          % (k, ends, int(kc.sum()), int((kc == 0).sum()), len(ids), stored))
    return 0


if __name__ == "__main__":
    sys.exit(main())
