"""The definition of contig threading without a device: the window model (tests/contig_thread_model.py) against a search
that uses no table, ``vs_contig_chain`` (vstrains_amd/csrc/vs_contig_chain.h through the library, a pure host function)
against the window model on match lists in any order, and the model on the 33 golden graphs, whose contigs -- spelled from
``in/contigs.paths`` -- must give that file back byte for byte."""
import os

import numpy as np
import pytest

import contig_thread_cases as cases
import contig_thread_model as model
from graph_case import GOLDEN, case_names
from vstrains_amd import node_depth
from vstrains_amd import pe as host


def hits_by_search(seqs, K, window):
    """All (segment, strand, pos) of a window, found with str.find on either strand's text."""
    if any(ch not in "ACGT" for ch in window):
        return []
    out = []
    for n, seq in enumerate(seqs):
        for strand, text in ((0, seq), (1, model.revcomp(seq))):
            p = text.find(window)
            while p >= 0:
                out.append((n, strand, p))
                p = text.find(window, p + 1)
    return sorted(out)


def thread_by_search(seqs, k, contig):
    """The four rules again, written separately from the model's, over ``hits_by_search``: token strings only."""
    K = k + 1
    parts, prev = [], None
    for i in range(len(contig) - K + 1):
        hits = hits_by_search(seqs, K, contig[i:i + K])
        if not hits:
            prev = None
            continue
        if prev is not None and (prev[0], prev[1], prev[2] + 1) in hits:
            prev = (prev[0], prev[1], prev[2] + 1)
            continue
        first = [h for h in hits if h[2] == 0]
        if prev is not None and prev[2] == len(seqs[prev[0]]) - K and first:
            prev = first[0]
            parts[-1].append(prev[:2])
            continue
        prev = hits[0]
        parts.append([prev[:2]])
    return parts


def random_graph(rng, k):
    """A few segments cut from one text with k-base overlaps, a repeat and a copy on the other strand thrown in, and
    contigs that walk, jump, hold an N or a changed base."""
    K = k + 1
    g = cases.dna(rng, int(rng.integers(4 * K, 7 * K)))
    cuts = sorted(set(int(c) for c in rng.integers(K, len(g) - K, size=3)))
    bounds = [0] + cuts + [len(g) - k]
    seqs = [g[a:b + k] for a, b in zip(bounds, bounds[1:]) if b + k - a >= K]
    seqs.append(seqs[0][:K + 2] + cases.dna(rng, 5))           # a repeat of the first segment's start
    seqs.append(model.revcomp(seqs[-2][-(K + 3):]) + cases.dna(rng, 3))  # ... and one on the other strand
    contigs = []
    for _ in range(6):
        a = int(rng.integers(0, len(g) - K))
        c = g[a:a + int(rng.integers(K - 1, len(g) - a + 1))]
        what = int(rng.integers(0, 5))
        if what == 0 and len(c) > 2:
            m = int(rng.integers(0, len(c)))
            c = c[:m] + "N" + c[m + 1:]
        elif what == 1 and len(c) > 2:
            m = int(rng.integers(0, len(c)))
            c = c[:m] + cases._OTHER[c[m]] + c[m + 1:]
        elif what == 2:
            c = model.revcomp(c)
        elif what == 3:
            c = c + seqs[int(rng.integers(0, len(seqs)))]
        contigs.append(c)
    return seqs, contigs


@pytest.mark.parametrize("seed", range(12))
def test_window_model_equals_a_search_without_a_table(seed):
    rng = np.random.default_rng(seed)
    k = (5, 8, 11)[seed % 3]
    seqs, contigs = random_graph(rng, k)
    table = model.window_table(seqs, k)
    for c in contigs:
        parts, _ = model.thread(seqs, k, c, table=table)
        assert [[(n, s) for n, s, _ in part] for part in parts] == thread_by_search(seqs, k, c)
        # every window with a hit was chosen for exactly one token
        K = k + 1
        assert sum(w for part in parts for _, _, w in part) == sum(1 for i in range(len(c) - K + 1) if table.get(c[i:i + K]))


def chain(seqs, k, contigs, rng=None):
    recs = [m for c, text in enumerate(contigs) for m in model.mems(seqs, k, text, c)]
    if rng is not None:
        rng.shuffle(recs)
    return host.contig_chain(np.array(recs, dtype=np.uint32).reshape(-1, 5), [len(s) for s in seqs], k, len(contigs))


def model_parts(seqs, k, contigs):
    table = model.window_table(seqs, k)
    got = [model.thread(seqs, k, c, table=table) for c in contigs]
    return [[[tuple(t) for t in part] for part in parts] for parts, _ in got], [a for _, a in got]


@pytest.mark.parametrize("seed", range(12))
def test_chain_equals_the_window_model_on_random_graphs_in_any_order(seed):
    rng = np.random.default_rng(100 + seed)
    k = (5, 8, 11)[seed % 3]
    seqs, contigs = random_graph(rng, k)
    assert chain(seqs, k, contigs, rng) == model_parts(seqs, k, contigs)


@pytest.mark.parametrize("case", cases.small_cases(21) + [cases.long_cases(21)[0]], ids=lambda c: c.name)
def test_chain_and_model_on_the_constructed_cases(case):
    want_parts, want_amb = model_parts(case.seqs, case.k, case.contigs)
    assert chain(case.seqs, case.k, case.contigs, np.random.default_rng(1)) == (want_parts, want_amb)
    if case.want is not None:
        ids = [str(i) for i in range(len(case.seqs))]
        got = [[",".join(t) for t in model.tokens(parts, ids)] or None for parts in want_parts]
        assert got == case.want


def test_palindrome_and_repeat_are_ambiguous_and_resolved_by_continuity():
    by_name = {c.name: c for c in cases.small_cases(21)}
    pal = by_name["palindromic_window_inside_a_segment"]
    parts, amb = model_parts(pal.seqs, 21, pal.contigs)
    ids = [str(i) for i in range(len(pal.seqs))]
    walks = [[",".join(t) for t in model.tokens(p, ids)] for p in parts]
    assert walks[0] == ["1+"] and walks[1] == ["1-"] and walks[2] == ["1+"] and amb[:3] == [1, 1, 1]
    assert walks[3] == ["1+", "1-"]  # began on the palindrome: strand 0 first, then the strand the contig really follows
    assert walks[4] == ["1+"]
    rep = by_name["repeated_window_in_two_segments"]
    assert model_parts(rep.seqs, 21, rep.contigs)[1] == [1, 1, 1, 1]


def test_chain_refuses_records_that_cannot_be():
    lens = [40, 50]
    ok = [[0, 0, 1, 3, 22]]
    assert host.contig_chain(ok, lens, 21, 1)[0] == [[[(1, 0, 1)]]]
    for bad in ([[1, 0, 1, 3, 22]], [[0, 0, 2, 3, 22]], [[0, 0, 1, 3, 21]], [[0, 0, 1 | 1 << 31, 30, 22]]):
        with pytest.raises(Exception, match="vs_contig_chain"):
            host.contig_chain(bad, lens, 21, 1)
    assert host.contig_chain([], lens, 21, 2) == ([[], []], [0, 0])


def _golden(name):
    d = os.path.join(GOLDEN, name, "in")
    with open(os.path.join(d, "graph.gfa"), "rb") as fh:
        raw = fh.read()
    ids, seqs = host.read_gfa_segments(os.path.join(d, "graph.gfa"))
    with open(os.path.join(d, "contigs.paths")) as fh:
        paths = fh.read()
    return node_depth.infer_k(raw), ids, seqs, paths


def spelled_contigs(k, ids, seqs, paths):
    """(name, text) of every forward entry of a .paths file."""
    seg_of = dict(zip(ids, seqs))
    return [(name, model.spell(parts, seg_of, k)) for name, parts in model.read_paths(paths) if not name.endswith("'")]


@pytest.mark.parametrize("name", case_names())
def test_model_gives_the_golden_paths_back_byte_for_byte(name):
    k, ids, seqs, paths = _golden(name)
    table = model.window_table(seqs, k)
    out, ambiguous = "", 0
    for cname, text in spelled_contigs(k, ids, seqs, paths):
        parts, amb = model.thread(seqs, k, text, table=table)
        ambiguous += amb
        out += model.entry(cname, parts, ids)
    assert out == paths and ambiguous == 0
