"""Mates matched by name, the rule in plain Python over ``bam_util.Rec`` lists -- the oracle of the by-name BAM tests: the
sequential FIFO rule (``mates``), the same rule applied window by window (``mates_windowed``), the FASTQ pair a file stands
for under it (``fastq_pair_by_name``) and the constructed record lists the CPU and GPU tests share."""
import numpy as np

import bam_util as bu

CAP = 64  # records of one name and one end in a window


def mates(records):
    """(pairs as (index of the first, index of the second) in the order of the record that completed them, singletons in
    file order).  A record of class c pairs with the OLDEST waiting record of its name and the other class, else waits."""
    waiting, pairs = {}, []  # (name, class) -> indices, oldest first
    for i, r in enumerate(records):
        c = bu.classify(r.flag)
        if c > bu.C_SECOND:
            continue
        other = waiting.get((r.name, 1 - c))
        if other:
            j = other.pop(0)
            pairs.append((i, j) if c == bu.C_FIRST else (j, i))
        else:
            waiting.setdefault((r.name, c), []).append(i)
    return pairs, sorted(i for q in waiting.values() for i in q)


def mates_windowed(records, cuts, match=None):
    """The same through windows [the waiting records of earlier windows][records[a:b]] for consecutive cuts; ``match``
    takes a window's records and returns (pairs, waiting) as indices into it (default: ``mates`` itself).  Also returns
    the waiting set after every window."""
    match = match or mates
    pairs, carried, trail = [], [], []
    bounds = [0] + sorted(cuts) + [len(records)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        index = carried + list(range(a, b))
        p, w = match([records[i] for i in index])
        pairs += [(index[f], index[s]) for f, s in p]
        carried = [index[i] for i in w]
        trail.append(list(carried))
    return pairs, carried, trail


def crowded(records):
    """The newest record of a name with more than CAP participating records of one class in ONE window holding all the
    records (the newest over all such names), or None."""
    seen, out = {}, None
    for i, r in enumerate(records):
        c = bu.classify(r.flag)
        if c <= bu.C_SECOND:
            seen.setdefault(r.name, [0, 0, i])
            seen[r.name][c] += 1
            seen[r.name][2] = i
    for f, s, last in seen.values():
        if max(f, s) > CAP:
            out = last if out is None else max(out, last)
    return out


def fastq_pair_by_name(records):
    """The two FASTQ texts (bytes) in delivery order, and the number of singletons."""
    pairs, single = mates(records)
    texts = []
    for which in (0, 1):
        out = []
        for p in pairs:
            r = records[p[which]]
            s = bu.end_text(r)
            out.append("@%s/%d\n%s\n+\n%s\n" % (r.name.decode("latin-1").replace("\n", "_"), which + 1, s, "I" * len(s)))
        texts.append("".join(out).encode("latin-1"))
    return texts[0], texts[1], len(single)


# ---- record orders of a collated list -------------------------------------------------------------------------------------
def shuffled(records, seed):
    rng = np.random.default_rng(seed)
    return [records[int(i)] for i in rng.permutation(len(records))]


def near(records, seed, reach=2000):
    """every second participating record of a name moved back by a random 0..reach records, as proper pairs of a sorted
    alignment lie"""
    rng = np.random.default_rng(seed)
    seen, keys = set(), []
    for i, r in enumerate(records):
        mate = bu.classify(r.flag) <= bu.C_SECOND and r.name in seen
        seen.add(r.name)
        keys.append((i + (int(rng.integers(0, reach + 1)) + 0.5 if mate else 0), i))
    return [records[i] for _, i in sorted(keys)]


# ---- constructed lists ----------------------------------------------------------------------------------------------------
F, S = bu.PAIRED | bu.FIRST, bu.PAIRED | bu.SECOND


def _seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def lists():
    """[(name, records)]: a few dozen records each"""
    rng = np.random.default_rng(21)
    rec = lambda name, flag, n=None: bu.rec(name, flag, _seq(rng, int(rng.integers(1, 40)) if n is None else n))
    out = []
    twenty = [rec("m%d" % i, f | (bu.REVERSE if (i + f) % 3 == 0 else 0)) for i in range(20) for f in (F, S)]
    out.append(("twenty_shuffled", shuffled(twenty, 22)))
    out.append(("second_before_first", [rec("a", S), rec("b", S), rec("a", F), rec("c", F), rec("b", F), rec("c", S)]))
    out.append(("dropped_between", [rec("a", F), rec("a", F | bu.SECONDARY), rec("a", 0), rec("a", S | bu.SUPPLEMENTARY), rec("b", S),
                                    rec("a", F | S), rec("b", bu.FIRST), rec("a", S), rec("b", F)]))
    out.append(("prefix_names", [rec("read1", F), rec("read", S), rec("read10", F), rec("read1", S), rec("read", F), rec("read10", S)]))
    out.append(("last_byte_differs", [rec("name_a", F), rec("name_b", F), rec("name_c", S), rec("name_b", S), rec("name_a", S), rec("name_c", F)]))
    out.append(("l_read_name_1_and_255", [rec(b"", F), rec(b"x" * 254, S), rec(b"x" * 253 + b"y", F), rec(b"", S), rec(b"x" * 254, F),
                                          rec(b"x" * 253 + b"y", S), rec(b"x" * 253, F)]))
    out.append(("high_bytes", [rec(b"\xff\x80q", F), rec(b"\xff\x81q", F), rec(b"\x80", S), rec(b"\xff\x81q", S), rec(b"\xff\x80q", S), rec(b"\x80", F)]))
    out.append(("repeated_names", [rec("ffss", F), rec("fsfs", F), rec("ffs", F), rec("ffss", F), rec("fsfs", S), rec("ffs", F), rec("ffss", S),
                                   rec("fsfs", F), rec("ffs", S), rec("ffss", S), rec("fsfs", S)]))
    out.append(("singletons_of_either_class", [rec("a", F), rec("lone1", F), rec("b", S), rec("lone2", S), rec("a", S), rec("b", F), rec("lone3", F)]))
    out.append(("singletons_only", [rec("s%d" % i, F if i % 3 else S) for i in range(12)]))
    out.append(("header_only", []))
    out.append(("64_firsts_64_seconds", [rec("many", F, 5) for _ in range(64)] + [rec("many", S, 6) for _ in range(64)]))
    out.append(("65_firsts", [rec("many", F, 5) for _ in range(65)]))
    return out
