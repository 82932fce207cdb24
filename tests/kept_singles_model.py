"""The plain model of the KEPT records without a mate (``--count-singles`` with ``--check-names --check-names-singles`` or
``--bam-by-name``; ``VS_PN_KEEP`` of csrc/vs_pair_names.hip, ``VS_BAM_BY_NAME_KEEP`` of csrc/vs_bam.hip).

Two FASTQ files joined by name (tests/pair_names_model.py has the join).  A kept single of a ROUND is a record the round
decided that is in none of its pairs: ``window_singles``.  A record the round did not decide is no single of it -- it is in
the next windows and is judged there.  Over a whole valid input the kept singles of file f are the complete records of file f
whose key is not in both files (or whose namesake in the other file is no mate: ``x/1`` against ``x``), in file order:
``whole_file_singles`` says that from the keys alone, without the join.  ``drive`` runs the window protocol of
``pair_names_model.drive`` on a join that also returns the singles and collects them under file-wide record numbers.

One BAM whose mates are matched by name (tests/bam_mate_model.py has the rule): the kept singletons are the records that
still wait at the end of the input, in file order, each read as ``samtools fastq -s`` writes it (``bam_util.end_text``)."""
import random

import bam_mate_model as mm
import bam_util as bu
import pair_names_cases as pc
import pair_names_model as pm
from interleaved_model import mates, records


def window_singles(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True):
    """(singles of window 1, singles of window 2): the decided records in no pair; ([], []) where the round is refused"""
    pairs, info = pm.join(text0, text1, eof0, eof1)
    paired = [{p[f] for p in pairs} for f in (0, 1)]
    return tuple([r for r in range(info["decided"][f]) if r not in paired[f]] for f in (0, 1))


def join_with_singles(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True):
    """``pm.join`` and ``window_singles`` in the form ``drive`` takes"""
    pairs, info = pm.join(text0, text1, eof0, eof1)
    s0, s1 = window_singles(text0, text1, eof0, eof1)
    return pairs, s0, s1, info


def whole_file_singles(text0: bytes, text1: bytes):
    """(singles of file 1, singles of file 2) of a VALID input, from the keys alone: the complete records whose key is empty,
    is not in the other file, or names a record there that is no mate"""
    heads = [[r[0] for r in records(t)] for t in (text0, text1)]
    index = [{pm.key(h, f): h for h in heads[f] if pm.key(h, f)} for f in (0, 1)]
    out = ([], [])
    for f in (0, 1):
        for r, h in enumerate(heads[f]):
            other = index[1 - f].get(pm.key(h, f))
            if other is None or not (mates(h, other) if f == 0 else mates(other, h)):
                out[f].append(r)
    return out


def drive(join_fn, text0: bytes, text1: bytes, ends0, ends1, pick=None):
    """``pm.drive`` for a ``join_fn(w0, w1, eof0, eof1)`` -> (pairs, singles 1, singles 2, info): returns (pairs, (singles of
    file 1, singles of file 2)) under file-wide record numbers, the singles in the order the rounds hand them out, and the
    number of rounds.  A record is handed out once: the windows are cut behind what a round decided."""
    text, ends = (text0, text1), (list(ends0), list(ends1))
    win, at, nxt, base = [b"", b""], [0, 0], [0, 0], [0, 0]
    eof = [False, False]
    pairs, singles, rounds = [], ([], []), 0
    while True:
        want = pick(rounds, (len(win[0]), len(win[1])), tuple(eof)) if pick else (len(win[0]) <= len(win[1]), len(win[1]) <= len(win[0]))
        want = [bool(want[f]) and not eof[f] for f in (0, 1)]
        if not any(want):
            want = [not eof[0], not eof[1]]
        for f in (0, 1):
            if want[f]:
                win[f] += text[f][at[f]:ends[f][nxt[f]]]
                at[f] = ends[f][nxt[f]]
                nxt[f] += 1
                eof[f] = nxt[f] == len(ends[f])
        got, s0, s1, info = join_fn(win[0], win[1], eof[0], eof[1])
        rounds += 1
        assert info["duplicate"] is None and info["order"] is None
        pairs += [(base[0] + int(i), base[1] + int(j)) for i, j in got]
        for f, s in ((0, s0), (1, s1)):
            dec = info["decided"][f]
            assert all(int(r) < dec for r in s) and len(s) == dec - len(got)
            singles[f].extend(base[f] + int(r) for r in s)
            win[f] = win[f][pm.end_of_record(win[f], dec):]
            base[f] += dec
        if eof[0] and eof[1]:
            return pairs, singles, rounds


def random_valid_input(rng: random.Random, n: int):
    """n names in one order written three ways; records deleted from both files, records of one file only, empty tokens and
    ``x/1`` against ``x`` (equal keys, no mates) among them"""
    h0, h1 = [], []
    drop = rng.choice((0.0, 0.05, 0.3, 0.6))
    for k in range(n):
        name = b"@r%d_%s" % (k, b"x" * rng.randrange(4))
        a, b = [(name + b"/1", name + b"/2"), (name + b" 1:N:0:A", name + b"\t2:N:0:A"), (name, name), (name + b"/1", name)][rng.choice((0, 0, 1, 1, 2, 2, 3))]
        if rng.random() >= drop:
            h0.append(a)
        if rng.random() >= drop:
            h1.append(b)
        if rng.random() < 0.1:
            h0.append(b"@only1_%d" % k)
        if rng.random() < 0.1:
            h1.append(b"@only2_%d/2" % k)
        if rng.random() < 0.03:
            (h0 if rng.random() < 0.5 else h1).append(b" empty token %d" % k)
    return pc.text(h0), pc.text(h1, 3)


# ---- constructed windows -------------------------------------------------------------------------------------------------
def cases():
    """(name, window 1, window 2, options): the edges of the singles lists, beside ``pair_names_cases.cases()``"""
    h0, h1 = pc.mates_files(12)
    lone = lambda tag, n: [b"@%s%d" % (tag, k) for k in range(n)]
    out = [
        ("single_at_record_0_of_file_1", pc.text(lone(b"a", 1) + h0), pc.text(h1, 2), {}),
        ("single_at_record_0_of_file_2", pc.text(h0), pc.text(lone(b"b", 1) + h1, 2), {}),
        ("single_at_the_last_record_of_file_1", pc.text(h0 + lone(b"a", 1)), pc.text(h1, 2), {}),
        ("single_at_the_last_record_of_file_2", pc.text(h0), pc.text(h1 + lone(b"b", 1), 2), {}),
        ("singles_at_both_ends_of_both_files", pc.text(lone(b"a", 2) + h0 + lone(b"c", 3)), pc.text(lone(b"b", 1) + h1 + lone(b"d", 2), 2), {}),
        ("all_records_single", pc.text(lone(b"a", 9)), pc.text(lone(b"b", 7), 2), {}),
        ("no_singles", pc.text(h0), pc.text(h1, 2), {}),
        ("only_file_2_has_singles", pc.text(h0[:3] + h0[3:]), pc.text(h1[:3] + lone(b"b", 2) + h1[3:] + lone(b"d", 1), 2), {}),
        ("only_file_1_has_singles", pc.text(h0[:5] + lone(b"a", 3) + h0[5:]), pc.text(h1, 2), {}),
        ("an_empty_key", pc.text([b" x", b"@A", b"/1"]), pc.text([b"@A", b" x", b"/2"]), {}),
        ("slash_1_against_bare", pc.text([b"@A", b"@x/1", b"@B"]), pc.text([b"@A", b"@x", b"@B"]), {}),
    ]
    return out


def window_sizes():
    """records per window at which the compaction takes another path: a wavefront, a workgroup (PN_TPB = 256), two workgroups"""
    return sorted(set((0, 1, 63, 64, 65, 255, 256, 257, 513)) | set(pc.EDGE_SIZES))


def placed(n: int, singles_at, file: int):
    """two windows of n mates in step, of which the OTHER file lacks the records at the positions ``singles_at``: file `file`
    has n records, the lone ones at exactly those positions of its window"""
    at = set(singles_at)
    h0, h1 = pc.mates_files(n)
    mine, other = (h0, h1) if file == 0 else (h1, h0)
    other = [h for r, h in enumerate(other) if r not in at]
    return (pc.text(mine), pc.text(other, 2)) if file == 0 else (pc.text(other), pc.text(mine, 2))


# ---- the BAM ---------------------------------------------------------------------------------------------------------------
def bam_singletons(recs):
    """the records that still wait at the end of the input, in file order, and the reads they stand for"""
    waiting = mm.mates(recs)[1]
    return waiting, [bu.end_text(recs[i]) for i in waiting]
