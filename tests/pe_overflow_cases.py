"""Constructed read pairs for the two overflow kernels of vstrains_amd/csrc/vs_pe.hip -- k_pe_mid (one wavefront per pair, its
state in LDS; limits: 64 probes per end, MID_SLOTS = 256 touched nodes, MID_LIST = 64 accepted nodes per end) and k_pe_slow
(one workgroup per pair, dense node state, probes 256 at a time) -- with every limit placed ON its edge, and the MODEL that says
which kernel must finish each pair.  Pure Python, fixed random.Random seeds; checked without a device by
tests/test_pe_overflow_cases_cpu.py and on the device by tests/test_pe_overflow_gpu.py.

THE MODEL (``Model``), per end: probes = (len - w + 1) // s (vs_seed_probes; w, s from seed_geometry); touched = the nodes
that share a (k+1)-mer with the end on either strand (what a probe grid of stride s credits: a match of k + 1 bases and
more); accepted = the list of the string model (seed_extend_model.map_end; the CPU test holds it against the C oracle).
Per pair: the main path (k_pe_tiles) gives a counted pair up when an end is accepted by more than LCAP = 20 nodes, or --
in its straight-line instantiations only, MODE 1 and 2: the generic one reads the validity mask -- when an end holds more
than four bytes outside ACGT (VS_FLAG_MANY).  k_pe_mid passes a pair on to k_pe_slow when an end has more than 64 probes,
touches more than 256 nodes or is accepted by more than 64.  Hence ``where``: 'dropped' (an N, a short end), 'tiles', 'mid'
or 'slow'.  Every counted pair of every family here is given up by the main path, except the 200-base pair that only
lengthens a block: so nothing depends on what else a full tile table would send along.

At k = 20 (K = w = 21, s = 1) a read of L bases has L - 20 probes, and a CHAIN of 21-base nodes that advance one base each
gives one accepted node per probe.  A pair with few accepted nodes reaches the overflow list through five lower-case
bytes in its MATE: ``Mates`` makes ends that are accepted by one anchor node and carry them behind the match.

Families (``family(name)`` -> dict(k, seqs, fwd, rve, label); build the index with renumber=False):
  probes   ends of 83 / 84 / 85 bases on the chain: 63 / 64 / 65 probes and accepted nodes; 84 stays in k_pe_mid, 85 leaves
  list     ends of at most 60 bases whose chain nodes have duplicates and twins (the reverse complement as a node of its
           own): exactly 21, 63, 64, 65, 66 accepted nodes with at most 40 probes; 64 + 64 (4 096 cells from one wavefront),
           64 + 0, 65 + 64
  slots    ends with 12 accepted nodes and DECOYS: nodes as long as the read that share exactly one (k+1)-mer with it
           between mismatching flanks (v = 1: rejected), so that an end touches exactly 255 / 256 / 257 nodes: 256 fills
           k_pe_mid's table and stays, 257 leaves.  Node numbers are chosen (a graph of 10 496 nodes, the rest filler):
           'spread' any numbers, 'crowd' 40 decoys and more whose home slot (node * 0x9E3779B1) >> 24 is one slot, 'wrap'
           a run of home slots 250 .. 255 that crosses 255 -> 0; the decoys' shared windows are spread over 25 seeds, except
           in 'oneseed', where one seed carries 200 postings
  batches  ends of 276 / 277 / 533 / 600 bases on a chain: 1 / 2 / 3 / 3 probe batches of k_pe_slow, and a 533-base end with
           six bytes outside ACGT on either side of a batch boundary.  The block's longest read makes mid_fast = 0
  fast     the k = 21 / 90-base knife-edge family of pe_extension_cases with five dirty bytes in every MATE: the case end
           stays clean and, in a block of this shape (mid_fast = 1), is compared by vs_agree_fast and decided by vs_accept32
  plain    the same pairs with one 200-base pair appended: mid_fast = 0, vs_extend / vs_accept decide
  second_pairs(n_cu)  the 'fast' pairs interleaved with the probes / list pairs rebuilt at k = 21, so that neighbours differ in
           kind (leaves / stays, many accepted / none, v = T / v = T - 1 on one node), repeated in shuffled order until the pairs
           for k_pe_mid exceed three times its wavefronts and those for k_pe_slow three times its workgroups."""
import functools
import random

import pe_extension_cases as pec
import seed_extend_model as model

LCAP = 20          # accepted nodes an end may list on the main path
INV4 = 4           # bytes outside ACGT the straight-line kernels hold positions for
MID_PROBES, MID_SLOTS, MID_LIST = 64, 256, 64
SLOW_BATCH = 256   # probes k_pe_slow takes per pass of its p0 loop
SLOW_WORDS_PER_NODE = 6
SLOTS_NODES = 41 * 256  # nodes of the 'slots' graph: 41 numbers per home slot


def seed_probes(rlen: int, w: int, s: int) -> int:
    """vs_seed_probes (csrc/vs_pe_plan.h)."""
    return 0 if rlen < w else (rlen - w + 1) // s


def slow_grid_for(n_nodes: int) -> int:
    """slow_grid_for (csrc/vs_pe_plan.h): workgroups of k_pe_slow, as many as 4 GB of dense state allow, 64 .. 2048."""
    g = (4 << 30) // (4 * SLOW_WORDS_PER_NODE * max(n_nodes, 1))
    return min(max(g, 64), 2048)


def mid_waves(n_cu: int) -> int:
    """Wavefronts of k_pe_mid: n_cu * 8 workgroups of four."""
    return n_cu * 32


def home_slot(node: int) -> int:
    """Where k_pe_mid's table starts looking for a node."""
    return ((node * 0x9E3779B1) & 0xFFFFFFFF) >> 24


def block_shape(K: int, w: int, s: int, maxlen: int):
    """(mode, mid_fast) of the plan (vs_pe_plan) for a block with a position list for its bytes outside ACGT: MODE 1 up
    to w + 160 bases at stride <= 32, MODE 2 while the part behind an end's first probe fits 256 bases, else the generic MODE 0."""
    v = model.seed_verified(w)
    if s <= 32 and maxlen <= 128 + w + 32:
        return 1, 1 if v else 0
    reach = max([ln - model.phase(ln, w, s) - v for ln in range(K, maxlen + 1)] or [0])
    return (2 if s <= 128 and reach <= 256 and maxlen < 512 else 0), 0


class Model:
    def __init__(self, seqs, k: int):
        self.k, self.K, self.seqs = k, k + 1, list(seqs)
        self.table, self.w, self.s = model.build(self.seqs, self.K)
        self.rcs = [model.rc(x) if len(x) >= self.K else "" for x in self.seqs]
        self.kmers = {}
        for i, x in enumerate(self.seqs):
            for p in range(len(x) - self.K + 1):
                f = x[p:p + self.K]
                self.kmers.setdefault(min(f, model.rc(f)), set()).add(i)
        self._ends = {}

    def end(self, read: str):
        """-> dict(probes, touched (sorted), accepted (sorted), dirty, many)."""
        e = self._ends.get(read)
        if e is None:
            K, touched = self.K, set()
            for p in range(len(read) - K + 1):
                f = read[p:p + K]
                if all(model.valid(c) for c in f):
                    touched |= self.kmers.get(min(f, model.rc(f)), set())
            bad = [p for p, c in enumerate(read) if not model.valid(c)]
            accepted = model.map_end(read, self.seqs, self.rcs, self.table, self.w, self.s, K, verified=model.seed_verified(self.w))
            e = dict(probes=seed_probes(len(read), self.w, self.s), touched=sorted(touched), accepted=accepted, dirty=len(bad),
                     many=len(bad) > INV4 or any(p > 254 for p in bad))
            self._ends[read] = e
        return e

    def where(self, f: str, r: str, mode: int) -> str:
        if "N" in f or "N" in r or len(f) < self.K or len(r) < self.K:
            return "dropped"
        ends = [self.end(f), self.end(r)]
        if not any(len(e["accepted"]) > LCAP or (mode != 0 and e["many"]) for e in ends):
            return "tiles"
        if any(e["probes"] > MID_PROBES or len(e["touched"]) > MID_SLOTS or len(e["accepted"]) > MID_LIST for e in ends):
            return "slow"
        return "mid"


def verdicts(fam, mdl=None):
    """-> (where of every pair, mode, mid_fast): the distinct pairs are modelled once."""
    mdl = mdl or Model(fam["seqs"], fam["k"])
    mode, mid_fast = block_shape(mdl.K, mdl.w, mdl.s, max(len(x) for x in fam["fwd"] + fam["rve"]))
    memo = {}
    out = []
    for f, r in zip(fam["fwd"], fam["rve"]):
        if (f, r) not in memo:
            memo[(f, r)] = mdl.where(f, r, mode)
        out.append(memo[(f, r)])
    return out, mode, mid_fast


def _text(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _rc_any(read):
    """The reverse complement of a read that may hold bytes outside ACGT (kept as they are)."""
    return "".join(model._C.get(c, c) for c in reversed(read))


class Mates:
    """Ends that one anchor node of K + 9 bases accepts: its text and ten more bases, five of them lower-case where asked."""

    def __init__(self, rng, K):
        self.rng, self.node = rng, _text(rng, K + 9)

    def __call__(self, dirty: bool, rc: bool) -> str:
        tail = _text(self.rng, 10)
        if dirty:
            tail = "".join(c.lower() if i % 2 else c for i, c in enumerate(tail))
        read = self.node + tail
        return _rc_any(read) if rc else read


def _pairs_both_ways(pairs, label, read, mates, dirty, tag):
    """The read as the forward end of one pair and, reverse-complemented, as the reverse end of another."""
    pairs.append((read, mates(dirty, True), label, tag))
    pairs.append((mates(dirty, False), model.rc(read), label, tag))


@functools.lru_cache(maxsize=None)
def chain_cases(k: int):
    """The 'probes' and 'list' pairs over one node set: -> dict(k, seqs, pairs [(fwd, rve, family, tag)], anchor)."""
    K = k + 1
    rng = random.Random(7100 + k)
    genome = _text(rng, 160)
    seqs = [genome[i:i + K] for i in range(len(genome) - K + 1)]
    mates = Mates(rng, K)
    anchor = len(seqs)
    seqs.append(mates.node)
    pairs = []
    for L in (83, 84, 85):
        a = rng.randrange(0, len(genome) - L)
        _pairs_both_ways(pairs, "probes", genome[a:a + L], mates, L == 83, "%d bases" % L)
    a, b = 3, 70
    pairs.append((genome[a:a + 84], model.rc(genome[b:b + 84]), "probes", "84 + 84"))
    pairs.append((genome[a:a + 85], model.rc(genome[b:b + 84]), "probes", "85 + 84"))
    reads = {}
    for name, n in (("21", 21), ("63", 63), ("64", 64), ("64b", 64), ("65", 65), ("66", 66)):
        n_chain = (n + 1) // 2
        assert n_chain + k <= 60 or k != 20
        text = _text(rng, n_chain + k)
        own = [text[i:i + K] for i in range(n_chain)]
        seqs += own
        seqs += [own[i] if i % 2 else model.rc(own[i]) for i in range(n - n_chain)]  # duplicates and twins
        reads[name] = text
    for name in ("21", "63", "64", "65", "66"):
        _pairs_both_ways(pairs, "list", reads[name], mates, name in ("21", "64"), name)
    pairs.append((reads["64"], model.rc(reads["64b"]), "list", "64 + 64"))
    pairs.append((model.rc(reads["64b"]), _text(rng, 40), "list", "64 + 0"))
    pairs.append((reads["65"], model.rc(reads["64b"]), "list", "65 + 64"))
    pairs.append((reads["64b"], model.rc(reads["63"]), "list", "64 + 63"))
    return dict(k=k, seqs=seqs, pairs=pairs, anchor=anchor)


def _decoy(rng, read, o_r, K, rc):
    """A node as long as the read that shares read[o_r : o_r + K] and nothing around it."""
    L = len(read)
    o_d = rng.randrange(1, L - K)
    body = list(_text(rng, L))
    body[o_d:o_d + K] = read[o_r:o_r + K]
    body[o_d - 1] = rng.choice([c for c in "ACGT" if c != read[o_r - 1]])
    body[o_d + K] = rng.choice([c for c in "ACGT" if c != read[o_r + K]])
    body = "".join(body)
    return model.rc(body) if rc else body


SLOT_VARIANTS = ("spread", "crowd", "wrap", "oneseed")
SLOT_ACCEPTED = 12


@functools.lru_cache(maxsize=None)
def slots_cases():
    """-> dict(k, seqs, pairs, cases [dict(touched, variant, read, chain, decoys)])."""
    k, K, L = 20, 21, 60
    rng = random.Random(7256)
    N = SLOTS_NODES
    seqs = [None] * N
    by_slot = {}
    for i in range(N):
        by_slot.setdefault(home_slot(i), []).append(i)
    # the chosen numbers first: per 'crowd' case 40 numbers of one home slot, per 'wrap' case five of each of the slots 250 .. 255
    chosen = {("crowd", t): by_slot[h][:40] for t, h in ((255, 7), (256, 100), (257, 200))}
    for j, t in enumerate((255, 256, 257)):
        chosen[("wrap", t)] = [by_slot[h][5 * j + i] for i in range(5) for h in range(250, 256)]
    taken = {i for ids in chosen.values() for i in ids}
    free = [i for i in range(N) if i not in taken]
    rng.shuffle(free)
    take = free.pop

    mates = Mates(rng, K)
    seqs[take()] = mates.node
    cases, pairs = [], []
    for variant in SLOT_VARIANTS:
        for touched in (255, 256, 257):
            read = _text(rng, L)
            chain = []
            for i in range(SLOT_ACCEPTED):
                n = take()
                seqs[n] = read[i:i + K]
                chain.append(n)
            n_decoys = touched - SLOT_ACCEPTED
            numbers = chosen.get((variant, touched), [])
            decoys = []
            for d in range(n_decoys):
                n = numbers[d] if d < len(numbers) else take()
                o_r = 20 if variant == "oneseed" and d < 200 else 13 + d % 25
                seqs[n] = _decoy(rng, read, o_r, K, rc=bool(d % 2))
                decoys.append(n)
            cases.append(dict(touched=touched, variant=variant, read=read, chain=chain, decoys=decoys))
            _pairs_both_ways(pairs, "slots", read, mates, True, "%s %d" % (variant, touched))
    for i in sorted(free):
        seqs[i] = _text(rng, K)
    return dict(k=k, seqs=seqs, pairs=pairs, cases=cases)


@functools.lru_cache(maxsize=None)
def batches_cases():
    k, K = 20, 21
    rng = random.Random(7512)
    genome = _text(rng, 900)
    seqs = [genome[i:i + K] for i in range(len(genome) - K + 1)]
    mates = Mates(rng, K)
    seqs.append(mates.node)
    cut = {L: genome[a:a + L] for L, a in ((276, 5), (277, 400), (533, 120), (600, 290))}
    dirty = list(genome[300:300 + 533])
    # probe 256 starts at read offset 256: seeds on either side of the batch boundary are masked, also in the reverse complement
    for p in (10, 250, 262, 270, 282, 520):
        dirty[p] = dirty[p].lower()
    dirty = "".join(dirty)
    pairs = [(cut[276], model.rc(cut[277]), "batches", "276 + 277"), (cut[533], model.rc(cut[600]), "batches", "533 + 600"),
             (dirty, mates(False, True), "batches", "533 with six bytes outside ACGT"), (mates(False, False), model.rc(cut[600]), "batches", "600"),
             (cut[277], mates(True, True), "batches", "277"), (_rc_any(dirty), model.rc(cut[276]), "batches", "dirty 533 + 276")]
    return dict(k=k, seqs=seqs, pairs=pairs)


@functools.lru_cache(maxsize=None)
def knife_cases(plain: bool):
    """The k = 21 / 90-base knife-edge block with the five dirty bytes moved into the mate (its last five bytes as given: the
    anchor still accepts it); ``plain``: one clean 200-base pair that matches nothing is appended, which takes mid_fast away."""
    fam = pec.knife_edge_family(21, 90, pec.SHAPES[(21, 90)]["step"])
    rng = random.Random(7021)
    fwd, rve = list(fam["fwd"]), list(fam["rve"])
    for p, c in enumerate(fam["cases"]):
        mate = (fwd if c["end"] else rve)[p]
        mate = mate[:-5] + mate[-5:].lower()
        if c["end"]:
            fwd[p] = mate
        else:
            rve[p] = mate
    if plain:
        fwd.append(_text(rng, 200))
        rve.append(_text(rng, 200))
    return dict(k=21, seqs=list(fam["seqs"]), fwd=fwd, rve=rve, label=["knife"] * len(fam["cases"]) + ["long"] * int(plain), cases=fam["cases"],
                anchor=fam["anchor"])


def _from_pairs(c, name):
    pairs = [p for p in c["pairs"] if p[2] == name]
    return dict(c, fwd=[p[0] for p in pairs], rve=[p[1] for p in pairs], label=[p[3] for p in pairs])


FAMILIES = ("probes", "list", "slots", "batches", "fast", "plain")


@functools.lru_cache(maxsize=None)
def family(name: str):
    if name in ("probes", "list"):
        return _from_pairs(chain_cases(20), name)
    if name == "slots":
        return _from_pairs(slots_cases(), name)
    if name == "batches":
        return _from_pairs(batches_cases(), name)
    return knife_cases(plain={"fast": False, "plain": True}[name])


@functools.lru_cache(maxsize=None)
def second_pairs_round():
    """The distinct pairs of the 'second pairs' block, in an order whose neighbours differ in kind: a knife-edge pair (few
    accepted nodes; v = T and v = T - 1 on one node follow each other in that family), then a probes / list pair rebuilt at
    k = 21 (62 .. 66 accepted nodes, every other one leaves k_pe_mid), in turn.  -> dict(k, seqs, fwd, rve, label)."""
    knife, chain = knife_cases(False), chain_cases(21)
    seqs = knife["seqs"] + chain["seqs"]  # (the knife-edge nodes keep their numbers and their neighbours)
    stay = [p for p in chain["pairs"] if p[3] in ("84 bases", "64", "64 + 64", "64 + 0", "63", "64 + 63")]
    leave = [p for p in chain["pairs"] if p[3] in ("65", "66", "65 + 64")]
    fwd, rve, label = [], [], []
    for p in range(len(knife["fwd"])):
        fwd.append(knife["fwd"][p])
        rve.append(knife["rve"][p])
        label.append("knife")
        f, r, _, tag = (leave if p % 2 else stay)[(p // 2) % len(leave if p % 2 else stay)]
        fwd.append(f)
        rve.append(r)
        label.append(tag)
    return dict(k=21, seqs=seqs, fwd=fwd, rve=rve, label=label)


def second_pairs(n_cu: int):
    """-> (round, order, reps): the block is [round pair order[i]] -- ``reps`` times the round, the first time as it stands,
    then shuffled -- with more than 3 * mid_waves(n_cu) pairs for k_pe_mid and more than 3 * slow_grid_for(nodes) for k_pe_slow."""
    rnd = second_pairs_round()
    where, _, _ = verdicts(rnd)
    n_mid, n_slow = sum(v in ("mid", "slow") for v in where), sum(v == "slow" for v in where)
    reps = max(-(-(3 * mid_waves(n_cu) + 1) // n_mid), -(-(3 * slow_grid_for(len(rnd["seqs"])) + 1) // n_slow))
    rng = random.Random(7003)
    order = list(range(len(where)))
    for _ in range(reps - 1):
        again = list(range(len(where)))
        rng.shuffle(again)
        order += again
    return rnd, order, reps
