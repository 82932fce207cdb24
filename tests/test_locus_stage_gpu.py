"""The staged key pass of the locus sort on the device (vstrains_amd/csrc/vs_pe.hip, k_locus_count_staged: a wavefront
streams the read words of a batch of pairs through LDS and asks the table for a slot and its locus node together) against
the per-pair loads it replaces (VS_LOCUS_STAGE=0 on an experiment context: k_locus_count, the path production keeps where
the buffers do not fit).  Every comparison is made on ONE context and ONE index build -- the order of a seed's postings
differs between builds, and with it the node a seed with several postings stands for -- and is exact: the keys bit for bit,
the per-end node lists, both counters and the statistics.  The keys also lie in the host model's sets (the nodes that hold
a posting of the forward read's first grid seed that hits), the order meets what tests/test_pe_counters_gpu.py states for
it, and the launched-bit says which pass ran.  VS_LOCUS_STAGE=N shrinks a wavefront's buffer to N words, so that blocks of
a few thousand pairs reach batch cuts inside a chunk, batches of one pair and pairs too large for the buffer."""
import numpy as np
import pytest

import seed_extend_model as sem
import test_pe_counters_gpu as base

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


@pytest.fixture(scope="module")
def xctx(host):
    from conftest import experiment_context

    c = experiment_context(host)
    yield c
    c.close()


def _allowed(seqs, K, fwd, rve):
    """Per pair what its locus key may be (as base._locus_inputs states it); rve[p] None: a single read, no second end."""
    table, w, s = sem.build(seqs, K)
    N = len(seqs)
    out = []
    for f, r in zip(fwd, rve):
        if "N" in f or len(f) < K or (r is not None and ("N" in r or len(r) < K)):
            out.append({N + 1})
            continue
        hit = {N}
        for j in range(sem.phase(len(f), w, s), len(f) - w + 1, s):
            seed_text = f[j: j + w]
            if not all(sem.valid(ch) for ch in seed_text):
                continue
            post = table.get(min(seed_text, sem.rc(seed_text)))
            if post:
                hit = {node for node, _, _ in post}
                break
        out.append(hit)
    return out


def _order_ok(keys, perm, n_pairs):
    """What test_locus_order states of the LDS sort: a permutation, in key order, equal keys of different chunks in chunk order."""
    assert np.array_equal(np.sort(perm), np.arange(n_pairs, dtype=perm.dtype))
    sorted_keys = keys[perm].astype(np.int64)
    assert (np.diff(sorted_keys) >= 0).all()
    chunk = -(-n_pairs // 256)
    wg = perm.astype(np.int64) // chunk
    assert (np.diff(wg)[np.diff(sorted_keys) == 0] >= 0).all()


def _observe(monkeypatch, c, pack, stage, n_nodes, count=True):
    """One block mapped (and counted) with VS_LOCUS_STAGE = stage (None: unset, what production does)."""
    import torch

    if stage is None:
        monkeypatch.delenv("VS_LOCUS_STAGE", raising=False)
    else:
        monkeypatch.setenv("VS_LOCUS_STAGE", str(stage))
    reads = pack()
    lists = c.map_ends(reads, cap=64)
    keys, perm, sort, n = c.last_order()
    got = dict(lists=lists, keys=keys.copy(), perm=perm.copy(), sort=sort, n=n, staged=bool(c.last_launched & c.RAN_LOCUS_STAGED))
    if count:
        mats = torch.zeros((2, n_nodes, n_nodes), dtype=torch.int32, device="cuda:%d" % c.device)
        stats = torch.zeros(3, dtype=torch.int64, device=mats.device)
        with torch.cuda.device(mats.device):
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            c.pe_count(reads, mats[0].data_ptr(), mats[1].data_ptr(), stats.data_ptr())
            c.sync()
        keys2, perm2, _, _ = c.last_order()
        got.update(mats=mats.cpu().numpy(), stats=stats.cpu().numpy(), count_keys=keys2.copy(), count_perm=perm2.copy(),
                   count_staged=bool(c.last_launched & c.RAN_LOCUS_STAGED))
    reads.free()
    return got


BY_THE_PLAN = 1000000  # VS_LOCUS_STAGE beyond what fits: the capacity production stages with, whatever the reads' length


def _compare(monkeypatch, c, seqs, k, pack, allowed, stages, count=True, renumber=False, unstaged=()):
    """The common checks of every case: each staging in `stages` against VS_LOCUS_STAGE=0, on one index build.  `unstaged`:
    those of `stages` with which the plan keeps the per-pair loads."""
    N, n_pairs = len(seqs), len(allowed)
    c.build_index(seqs, k, renumber=renumber)
    ref = _observe(monkeypatch, c, pack, 0, N, count)
    assert ref["n"] == n_pairs and ref["sort"] == c.RAN_LOCUS_LDS_SORT and not ref["staged"]
    for p in range(n_pairs):
        assert int(ref["keys"][p]) in allowed[p], (p, int(ref["keys"][p]), sorted(allowed[p])[:5])
    _order_ok(ref["keys"], ref["perm"], n_pairs)
    for stage in stages:
        got = _observe(monkeypatch, c, pack, stage, N, count)
        assert got["staged"] == (stage not in unstaged) and got["sort"] == c.RAN_LOCUS_LDS_SORT and got["n"] == n_pairs, stage  # (the bit: the staged pass ran)
        diff = np.nonzero(got["keys"] != ref["keys"])[0]
        assert diff.size == 0, (stage, diff[:8], got["keys"][diff[:8]], ref["keys"][diff[:8]])
        _order_ok(got["keys"], got["perm"], n_pairs)
        assert got["lists"] == ref["lists"], stage
        if count:
            assert got["count_staged"] == got["staged"] and not ref["count_staged"]
            assert np.array_equal(got["count_keys"], ref["keys"]) and np.array_equal(ref["count_keys"], ref["keys"])
            _order_ok(got["count_keys"], got["count_perm"], n_pairs)
            assert np.array_equal(got["mats"], ref["mats"]) and np.array_equal(got["stats"], ref["stats"]), stage
            assert int(ref["mats"].astype(np.int64).sum()) > 0
    return ref


_inputs = {}


def _small(n_pairs):
    if n_pairs not in _inputs:
        _inputs[n_pairs] = base._locus_inputs("small", n_pairs, 31 + n_pairs)
    return _inputs[n_pairs]


# ---- the `small` graph: production staging, then buffers of a few pairs ----------------------------------------------------
def test_small_graph_production_and_shrunk_buffers(monkeypatch, xctx):
    seqs, k, fwd, rve, allowed = _small(5003)
    N = len(seqs)
    kinds = {"dropped": 0, "none": 0, "hit": 0, "several": 0}
    for a in allowed:
        kinds["dropped" if a == {N + 1} else "none" if a == {N} else "hit"] += 1
        kinds["several"] += len(a) > 1
    assert min(kinds["dropped"], kinds["none"], kinds["hit"]) > 5003 // 20 and kinds["several"] > 0  # (seeds with several postings: the slots' locus nodes)
    # 48 and 64 words: batches of one to a few pairs (a pair of two 150-base reads is 20 words), 257: a dozen, cuts mid-chunk
    _compare(monkeypatch, xctx, seqs, k, lambda: xctx.pack_pairs(fwd, rve), allowed, [None, 48, 64, 257])


# ---- 4 096 pairs: chunks of 16 pairs, one partial batch per workgroup; 4 097: chunks of 17, workgroups 241 .. 255 empty --------
@pytest.mark.parametrize("n_pairs", [4096, 4097])
def test_smallest_blocks(monkeypatch, xctx, n_pairs):
    seqs, k, fwd, rve, allowed = _small(n_pairs)
    _compare(monkeypatch, xctx, seqs, k, lambda: xctx.pack_pairs(fwd, rve), allowed, [None, 64])


# ---- mixed lengths in one block --------------------------------------------------------------------------------------------
def _mixed(seqs, K, n_pairs, seed):
    rng = np.random.default_rng(seed)
    w, s = sem.geometry(K)
    long_nodes = [i for i, x in enumerate(seqs) if len(x) >= 120]
    fwd, rve = [], []

    def text(n):  # n bases off the graph: a node's text, continued by other nodes' where it is shorter
        t = ""
        while len(t) < n:
            x = seqs[long_nodes[int(rng.integers(0, len(long_nodes)))]]
            t += x if rng.integers(0, 2) else sem.rc(x)
        return t[:n]

    for p in range(n_pairs):
        kind = p % 12
        f, r = text(int(rng.integers(60, 151))), text(int(rng.integers(60, 151)))
        if kind == 0:
            f = f[: K - 1]                      # one base short: dropped
        elif kind == 1:
            f = f[:K]                           # the shortest read that is probed
        elif kind == 2:
            f = text(100 + (w - 100) % s)       # (len - w) mod s == 0
        elif kind == 3:
            f = text(100 + (w - 100) % s + s - 1)  # ... == s - 1
        elif kind == 4:
            f, r = text(250), text(250)         # 2 x 250 among 2 x 150: 32 words
        elif kind == 5:
            f = f[:30] + "N" + f[31:]           # an N: dropped
        elif kind in (6, 7):
            # lower-case / IUPAC bytes in the first grid seed, which is dirty and skipped: one (its position is listed), six
            # (more than a list holds: the end keeps to the mask)
            j0 = sem.phase(len(f), w, s)
            for x, ch in zip(range(6 if kind == 7 else 1), "rynkmw"):
                at = j0 + 1 + 2 * x
                f = f[:at] + ch + f[at + 1:]
        elif kind == 8:
            r = r[: K - 1]                      # the mate too short: dropped
        fwd.append(f)
        rve.append(r)
    return fwd, rve


def test_mixed_lengths_dirty_seeds_and_oversize_pairs(monkeypatch, xctx):
    seqs, k, _, _, _ = _small(5003)
    K = k + 1
    w, s = sem.geometry(K)
    fwd, rve = _mixed(seqs, K, 4200, 77)
    allowed = _allowed(seqs, K, fwd, rve)
    lens = {len(f) for f in fwd}
    assert {K - 1, K, 250} <= lens and {(n - w) % s for n in lens if n >= w} >= {0, s - 1}
    dirty_first = sum(1 for f in fwd if len(f) >= K and not all(sem.valid(ch) for ch in f[sem.phase(len(f), w, s):][:w]) and "N" not in f)
    assert dirty_first > 600
    # 24 words: below the 32 of a 2 x 250 pair (keyed alone, by per-pair loads), one 2 x 150 pair a batch; 48: the long pair fits
    # (production does not stage a block whose longest reads leave a buffer 34 pairs: the plan's capacity through the hook)
    ref = _compare(monkeypatch, xctx, seqs, k, lambda: xctx.pack_pairs(fwd, rve), allowed, [None, BY_THE_PLAN, 24, 48], unstaged=[None])
    assert len(set(ref["keys"].tolist())) > 100


def test_singles_block(monkeypatch, xctx):
    seqs, k, fwd, _, _ = _small(5003)
    K = k + 1
    reads = fwd[:4300]
    allowed = _allowed(seqs, K, reads, [None] * len(reads))
    _compare(monkeypatch, xctx, seqs, k, lambda: xctx.pack_singles(reads), allowed, [None, 16, 64])


# ---- k = 127: 63-base seeds with mixed keys, 2 x 250 reads ------------------------------------------------------------------------
def test_k127_index(monkeypatch, xctx):
    rng = np.random.default_rng(127)
    seqs = [base._random_seq(rng, int(rng.integers(100, 900))) for _ in range(300)]
    seqs[11] = seqs[10]  # the same text twice: seeds with two postings
    k, K = 127, 128
    long_nodes = [i for i, x in enumerate(seqs) if len(x) >= 300]
    fwd, rve = [], []
    for p in range(4200):
        x = seqs[10 if p % 9 == 0 else long_nodes[int(rng.integers(0, len(long_nodes)))]]
        x = x if p % 2 else sem.rc(x)
        lo = int(rng.integers(0, len(x) - 250 + 1)) if len(x) > 250 else 0
        f = x[lo: lo + 250]
        if p % 7 == 3:
            f = base._random_seq(rng, 250)
        if p % 7 == 4:
            f = f[:150]
        fwd.append(f)
        rve.append(sem.rc(f))
    allowed = _allowed(seqs, K, fwd, rve)
    assert sum(len(a) > 1 for a in allowed) > 100
    # (2 x 250 bases: production keeps the per-pair loads, the hook stages at the plan's capacity)
    _compare(monkeypatch, xctx, seqs, k, lambda: xctx.pack_pairs(fwd, rve), allowed, [None, BY_THE_PLAN, 64], unstaged=[None])


# ---- the `chain` graph: more keys than one histogram pass holds -- no staging, whatever the switch says ----------------------------
def test_chain_graph_keeps_per_pair_loads(monkeypatch, xctx):
    if "chain" not in _inputs:
        _inputs["chain"] = base._locus_inputs("chain", 5003, 31 + 5003)
    seqs, k, fwd, rve, allowed = _inputs["chain"]
    N = len(seqs)
    assert N + 2 > 36864
    xctx.build_index(seqs, k, renumber=False)
    first = _observe(monkeypatch, xctx, lambda: xctx.pack_pairs(fwd, rve), None, N, count=False)
    again = _observe(monkeypatch, xctx, lambda: xctx.pack_pairs(fwd, rve), 64, N, count=False)
    for got in (first, again):
        assert got["sort"] == xctx.RAN_LOCUS_LDS_SORT and not got["staged"] and got["n"] == 5003
        _order_ok(got["keys"], got["perm"], 5003)
    assert np.array_equal(first["keys"], again["keys"]) and first["lists"] == again["lists"]
    for p in range(5003):
        assert int(first["keys"][p]) in allowed[p], (p, int(first["keys"][p]))
