"""Host statement of the seed index (vstrains_amd/csrc/vs_index.hip, vs_internal.h): what the build must produce for a
list of node texts, in plain Python / numpy, and the constructions that reach the parts of it random inputs do not --
different 63-base seeds with one key, and seeds with a chosen home slot.  Nothing here imports the library: the GPU tests
compare the exported index with this file (tests/test_seed_index_gpu.py), the CPU tests check this file against itself
and the algorithm model against the oracle (tests/test_seed_index_model_cpu.py)."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

M64 = (1 << 64) - 1
PAD_WORDS = 16                    # VS_PAD_WORDS (vs_internal.h): zero words behind either strand's text
EMPTY_KEY = M64                   # VS_EMPTY_KEY
MULTI_BIT = 1 << 62               # VS_MULTI_BIT
KEY_SALT = 0x632BE59BD9B4E019     # vs_seed_key: added to the upper half before it is mixed
SLOT_MULT = 0x9E3779B97F4A7C15    # vs_slot_of
_GAMMA, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB  # vs_mix64
_M1_INV, _M2_INV = pow(_M1, -1, 1 << 64), pow(_M2, -1, 1 << 64)

_COMP = str.maketrans("ACGT", "TGCA")
_DIGITS = str.maketrans("ACGT", "0123")


def rc(s: str) -> str:
    return s.translate(_COMP)[::-1]


# ---- packed text (vs_internal.h "packed text"; k_pack_nodes) ---------------------------------------------------------
def pack_words(s: str) -> np.ndarray:
    """2 bits per base (A=0 C=1 G=2 T=3), base i in word i // 16 at bits 2 * (i % 16); the last word zero-filled."""
    n = (len(s) + 15) // 16
    codes = np.zeros(n * 16, dtype=np.uint32)
    if s:
        codes[: len(s)] = np.frombuffer(s.translate(_DIGITS).encode(), dtype=np.uint8) - ord("0")
    return (codes.reshape(n, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)


def seq_int(s: str) -> int:
    """The bases of ``s`` as the device holds a window of them: base i at bits 2i."""
    return int(s[::-1].translate(_DIGITS), 4) if s else 0


def int_seq(v: int, w: int) -> str:
    return "".join("ACGT"[(v >> (2 * i)) & 3] for i in range(w))


# ---- geometry, key, slot ---------------------------------------------------------------------------------------------
def geometry(K: int) -> Tuple[int, int]:
    """seed_geometry (vs_index.hip): w = min(K, 31), 63 from K = 96 on, made odd; s = K - w + 1."""
    w = 63 if K >= 96 else min(K, 31)
    if w % 2 == 0:
        w -= 1
    return w, K - w + 1


def mix64(z: int) -> int:
    """vs_mix64: the splitmix64 finaliser, a bijection of 64-bit values."""
    z = (z + _GAMMA) & M64
    z = ((z ^ (z >> 30)) * _M1) & M64
    z = ((z ^ (z >> 27)) * _M2) & M64
    return z ^ (z >> 31)


def unmix64(y: int) -> int:
    y ^= y >> 31
    y ^= y >> 62
    y = (y * _M2_INV) & M64
    y ^= y >> 27
    y ^= y >> 54
    y = (y * _M1_INV) & M64
    y ^= y >> 30
    y ^= y >> 60
    return (y - _GAMMA) & M64


def seed_key(seed: str) -> Tuple[int, int]:
    """vs_seed_key: (key, strand) of a w-mer; strand 1 = the reverse complement is the smaller value and is what the key
    is made of.  w <= 31: the smaller value itself.  w = 63: the 126 bits compared as (upper 62 : lower 64), the key a mix
    of the two halves cut to 62 bits."""
    w = len(seed)
    f, r = seq_int(seed), seq_int(rc(seed))
    strand = 1 if r < f else 0
    c = r if strand else f
    if w <= 31:
        return c, strand
    assert w == 63, w
    a, b = c & M64, c >> 64
    return mix64(a ^ mix64((b + KEY_SALT) & M64)) >> 2, strand


def slot_of(key: int, bits: int) -> int:
    """vs_slot_of: multiplicative hash, the top ``bits`` bits of the 64-bit product."""
    return ((key * SLOT_MULT) & M64) >> (64 - bits)


def table_bits(distinct: int) -> int:
    """vs_index_build: the smallest power of two >= 8 * distinct + 2 slots, at least 2^4 (and at most 2^30)."""
    bits = 4
    while (1 << bits) < 8 * distinct + 2:
        bits += 1
    return min(bits, 30)


def occupied_slots(keys, bits: int) -> Dict[int, int]:
    """key -> slot under linear probing from the home slot (k_seed_insert).  WHICH slots end up occupied does not depend
    on the insertion order; which key sits in which slot of a run does, so only ``set(values())`` may be compared."""
    mask = (1 << bits) - 1
    taken: Dict[int, int] = {}
    out: Dict[int, int] = {}
    for key in keys:
        sl = slot_of(key, bits)
        while sl in taken:
            sl = (sl + 1) & mask
        taken[sl] = key
        out[key] = sl
    return out


# ---- the index -------------------------------------------------------------------------------------------------------
def build(seqs: Sequence[str], ksize: int) -> dict:
    """What vs_index_build makes of ``seqs``: packed words of both strands (pad words included), node headers, and per
    key the postings (node, pos, strand, node length, first word) of every seed position of every node of >= K bases."""
    K = ksize + 1
    w, s = geometry(K)
    woff, words_f, words_r = [], [], []
    n_words = 0
    for seq in seqs:
        woff.append(n_words)
        words_f.append(pack_words(seq))
        words_r.append(pack_words(rc(seq)))
        n_words += (len(seq) + 15) // 16
    pad = np.zeros(PAD_WORDS, dtype=np.uint32)
    postings: Dict[int, List[Tuple[int, int, int, int, int]]] = {}
    npos = 0
    for i, seq in enumerate(seqs):
        if len(seq) < K:
            continue
        for p in range(len(seq) - w + 1):
            key, strand = seed_key(seq[p: p + w])
            postings.setdefault(key, []).append((i, p, strand, len(seq), woff[i]))
            npos += 1
    bits = table_bits(len(postings))
    return dict(K=K, w=w, s=s, fwd=np.concatenate(words_f + [pad]), rc=np.concatenate(words_r + [pad]), n_words=n_words,
                meta=np.array([(woff[i], len(q)) for i, q in enumerate(seqs)], dtype=np.uint32).reshape(len(seqs), 2),
                postings=postings, seed_positions=npos, distinct=len(postings), bits=bits, slots=1 << bits,
                occupied=set(occupied_slots(postings, bits).values()))


def read_table(exp: dict) -> Dict[int, Tuple[bool, list]]:
    """The exported table (Context.index_export) decoded: key -> (multi form?, postings as the model's tuples)."""
    out = {}
    post = exp["postings"]
    for sl in np.nonzero(exp["slot_key"] != np.uint64(EMPTY_KEY))[0]:
        raw, a, b = int(exp["slot_key"][sl]), int(exp["slot_a"][sl]), int(exp["slot_b"][sl])
        if raw & MULTI_BIT:
            rows = [tuple(int(x) for x in post[i]) for i in range(a, a + b)]
            recs = [(n, y & 0x00FFFFFF, y >> 31, ln, wo) for n, y, ln, wo in rows]
        else:  # single form: the node header is not in the slot (it is read from meta by the kernels)
            recs = [(a, b & 0x00FFFFFF, b >> 31, int(exp["meta"][a][1]), int(exp["meta"][a][0]))]
        assert (raw & ~MULTI_BIT) not in out, "a key sits in two slots"
        out[raw & ~MULTI_BIT] = (bool(raw & MULTI_BIT), recs)
    return out


def runs(occupied, n_slots: int) -> List[Tuple[int, int]]:
    """Maximal runs of occupied slots as (first slot, length), a run that crosses from the last slot to slot 0 as one."""
    occ = sorted(occupied)
    if not occ:
        return []
    if len(occ) == n_slots:
        return [(0, n_slots)]
    out = []
    start = prev = occ[0]
    for x in occ[1:]:
        if x != prev + 1:
            out.append((start, prev - start + 1))
            start = x
        prev = x
    out.append((start, prev - start + 1))
    if len(out) > 1 and out[0][0] == 0 and out[-1][0] + out[-1][1] == n_slots:
        first = out.pop(0)
        out[-1] = (out[-1][0], out[-1][1] + first[1])
    return out


# ---- constructions ---------------------------------------------------------------------------------------------------
def random_seq(rng, n: int) -> str:
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def colliding_seeds(x: str, n: int, rng) -> List[str]:
    """``n`` further 63-mers with the key of ``x``, none equal to ``x``, to its reverse complement or to one another.
    The key of a canonical 63-mer (a: lower 64 bits, b: upper 62) is mix64(a ^ mix64(b + salt)) >> 2 and mix64 is a
    bijection: for any b and any two low bits r, a = unmix64(key << 2 | r) ^ mix64(b + salt) gives that key -- if (b : a)
    is the smaller of the 63-mer and its reverse complement, which about every second draw is.  The seeds come in the
    orientation of ``x`` (the same strand bit): a posting is compared on the strand its bit and the read's give, so only a
    colliding seed that lies like ``x`` has the text around ``x`` compared with the text around it."""
    assert len(x) == 63
    kx, flip = seed_key(x)
    out: List[str] = []
    taken = {x, rc(x)}
    while len(out) < n:
        b = int(rng.integers(0, 1 << 62))
        r = int(rng.integers(0, 4))
        a = unmix64((kx << 2) | r) ^ mix64((b + KEY_SALT) & M64)
        y = int_seq((b << 64) | a, 63)
        if seq_int(rc(y)) < seq_int(y) or y in taken:
            continue  # (not the canonical orientation: the device would key the reverse complement instead)
        taken.update((y, rc(y)))
        out.append(rc(y) if flip else y)
    return out


def seeds_with_home_slot(w: int, bits: int, slot: int, n: int, rng, avoid=()) -> List[str]:
    """``n`` w-mers (w <= 31, exact keys) with distinct keys whose home slot in a table of 2^bits slots is ``slot``: plain
    search, about 2^bits draws each."""
    assert w <= 31 and w % 2 == 1
    sh = 2 * np.arange(w, dtype=np.uint64)
    out: List[str] = []
    keys = set(avoid)
    while len(out) < n:
        codes = rng.integers(0, 4, size=(1 << 16, w)).astype(np.uint64)
        f = (codes << sh).sum(axis=1, dtype=np.uint64)
        r = ((np.uint64(3) - codes[:, ::-1]) << sh).sum(axis=1, dtype=np.uint64)
        key = np.minimum(f, r)
        home = (key * np.uint64(SLOT_MULT)) >> np.uint64(64 - bits)
        for i in np.nonzero(home == np.uint64(slot))[0]:
            kk = int(key[i])
            if kk in keys or len(out) == n:
                continue
            keys.add(kk)
            out.append("".join("ACGT"[int(c)] for c in codes[i]))
    for q in out:
        assert slot_of(seed_key(q)[0], bits) == slot
    return out


# ---- shared-key scenarios (63-base seeds) ----------------------------------------------------------------------------
def sub_at(s: str, p: int, ch: str = None) -> str:
    return s[:p] + (ch if ch is not None else {"A": "C", "C": "G", "G": "T", "T": "A"}.get(s[p], "A")) + s[p + 1:]


def shared_key_scenarios(k: int, rng, crowd: int = 100) -> dict:
    """One graph at k >= 95 that holds every constructed case of 63-base seeds under one key.  Returns ``seqs``, the
    planted ``groups`` ({scenario: [[63-mers of one key], ...]}) and ``sources``: (scenario, text, offset of the shared
    seed in it, nodes the text holds whole) -- reads are windows of the source texts.  Flanks are random, shorter than
    K = k + 1, and drawn on both sides of the stride s: a shared flank below s bases is what leaves the shared key as the
    deciding probe (with s and more the earlier grid point owns the match)."""
    K = k + 1
    w, s = geometry(K)
    assert w == 63
    seqs: List[str] = []
    groups: Dict[str, list] = {}
    sources: List[tuple] = []
    pad = 2 * s + 320  # (room to slide a window of any tested length 2 s positions past the seed on either side)

    def node(text):
        assert len(text) >= K
        seqs.append(text)
        return len(seqs) - 1

    def source(name, text, off, nodes):
        lead, tail = random_seq(rng, pad), random_seq(rng, pad)
        sources.append((name, lead + text + tail, pad + off, nodes))

    def flanks():
        lo = max(s - 1, 2)
        return [(1, s - 2 + 1), (3, s + 2), (s + 2, 3), (s - 1, s - 1), (s, s), (s + 5, max(s - 3, 1)), (lo // 2, lo - lo // 2), (K - 1, K - 1)]

    # (a) twins: only the seed's own bases tell A from B
    for n1, n2 in flanks():
        x = random_seq(rng, 63)
        y = colliding_seeds(x, 1, rng)[0]
        f1, f2 = random_seq(rng, n1), random_seq(rng, n2)
        groups.setdefault("twins", []).append([x, y])
        a, b = node(f1 + x + f2), node(f1 + y + f2)
        source("twins", f1 + x + f2, n1, [a])
        source("twins", f1 + y + f2, n1, [b])
    # (b) orphan: X in one node, the reads hold Y, which is in none -> the probe lands on a single-form slot
    for n1, n2 in flanks()[:4]:
        x = random_seq(rng, 63)
        y = colliding_seeds(x, 1, rng)[0]
        f1, f2 = random_seq(rng, n1), random_seq(rng, n2)
        groups.setdefault("orphan", []).append([x, y])
        node(f1 + x + f2)
        source("orphan", f1 + y + f2, n1, [])
    # (c) strands: three seeds on one key, one of them stored as its reverse complement
    for n1, n2 in flanks()[:4]:
        x = random_seq(rng, 63)
        y, z = colliding_seeds(x, 2, rng)
        f1, f2 = random_seq(rng, n1), random_seq(rng, n2)
        groups.setdefault("strands", []).append([x, y, z])
        for q, flip in ((x, False), (y, False), (z, True)):
            t = f1 + q + f2
            nd = node(rc(t) if flip else t)
            source("strands", t, n1, [nd])
    # (d) edges: the shared seed is the node's first w bases / its last
    for at_start in (True, False):
        x = random_seq(rng, 63)
        y = colliding_seeds(x, 1, rng)[0]
        f = random_seq(rng, s + 7)
        groups.setdefault("edges", []).append([x, y])
        for q in (x, y):
            t = q + f if at_start else f + q
            source("edges", t, 0 if at_start else len(f), [node(t)])
    # (e) crowd: X in `crowd` nodes around one core, Y in a single node: more postings and accepted nodes than the
    # per-end lists of the main kernel (16) and of k_pe_mid (64) hold
    x = random_seq(rng, 63)
    y = colliding_seeds(x, 1, rng)[0]
    n1 = (K - 63) // 2
    f1, f2 = random_seq(rng, n1), random_seq(rng, K - 63 - n1)
    groups["crowd"] = [[x, y]]
    held = [node(random_seq(rng, 5 + i % 7) + f1 + x + f2 + random_seq(rng, 4 + i % 5)) for i in range(crowd)]
    source("crowd", f1 + x + f2, n1, held)
    lone = node(random_seq(rng, 9) + f1 + y + f2 + random_seq(rng, 6))
    source("crowd", f1 + y + f2, n1, [lone])
    return dict(k=k, K=K, w=w, s=s, seqs=seqs, groups=groups, sources=sources)


def scenario_reads(sc: dict, lengths: Sequence[int], every: int = 1, offsets_only=None, cycle: bool = False) -> List[tuple]:
    """Windows of every source text on both strands: (read, scenario, offset of the shared seed in the read or None when
    the read does not hold all of it, number of the source).  For every length the window start runs over every ``every``-th position from s
    before the first start that holds the whole seed to s behind the last -- (length - 63) + 2 s + 1 starts; with
    ``cycle`` the starts are walked once, for the longest length, and the lengths are taken in turn.
    ``offsets_only``: only the starts that put the seed at one of these read offsets (negative: counted back from
    length - w, the last offset a seed can have)."""
    w, s = sc["w"], sc["s"]
    out = []
    i = 0
    for si, (name, text, off, _) in enumerate(sc["sources"]):
        for L in ([max(lengths)] if cycle else lengths):
            if offsets_only is not None:
                starts = sorted({off - (o if o >= 0 else L - w + 1 + o) for o in offsets_only if 0 <= (o if o >= 0 else L - w + 1 + o) <= L - w})
            else:
                starts = range(off - (L - w) - s, off + s + 1, every)
            for st in starts:
                ln = lengths[i % len(lengths)] if cycle else L
                i += 1
                if st < 0 or st + ln > len(text):
                    continue
                win = text[st: st + ln]
                o = off - st
                inside = 0 <= o and o + w <= ln
                out.append((win, name, o if inside else None, si))
                out.append((rc(win), name, ln - o - w if inside else None, si))
    return out


def dirty_reads(reads: List[tuple], w: int, rng, inside: bool) -> List[tuple]:
    """The same reads with one byte outside ACGT ('n', 'R', '.'; never 'N', which drops the pair): outside the shared
    seed, or -- ``inside`` -- at one of its bases 32..62, the second window the device tests (vs_seed_dirty)."""
    out = []
    for read, name, o, si in reads:
        ch = "nR."[int(rng.integers(0, 3))]
        if o is not None and inside:
            p = o + int(rng.integers(32 if w > 32 else 0, w))
        else:
            p = int(rng.integers(0, len(read)))
            while o is not None and o <= p < o + w and len(read) > w:
                p = int(rng.integers(0, len(read)))
            if o is not None and len(read) == w:
                out.append((read, name, o, si))
                continue
        out.append((sub_at(read, p, ch), name, o, si))
    return out
