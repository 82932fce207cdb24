"""The look left of a breakpoint (csrc/vs_indel_core.h), the code a lane of k_node_indels runs, through its host entry
``vs_indel_scan_host`` against tests/indel_model.py: no device.  Every match of every constructed case -- tested or not --
gives the model's status, kind, length, position and insert; so do matches at every flank length around the window
boundaries, and lengths up to 32."""
import ctypes as C

import numpy as np
import pytest

import indel_cases as cases
import indel_model as model
from node_depth_cases import dna
from pileup_cases import sub
from pileup_model import revcomp, strands
from vstrains_amd import _native as nat
from vstrains_amd import pe as host

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def pack(text: str):
    """(words, mask): 2 bits a base, 16 a word, the first base lowest; the mask 0b11 at a byte outside ACGT (its word: code
    0); three zero words behind the last."""
    n_words = (len(text) + 15) // 16 + 3
    words, mask = np.zeros(n_words, dtype=np.uint32), np.zeros(n_words, dtype=np.uint32)
    for i, ch in enumerate(text):
        if ch in _CODE:
            words[i >> 4] |= np.uint32(_CODE[ch] << (2 * (i & 15)))
        else:
            mask[i >> 4] |= np.uint32(3 << (2 * (i & 15)))
    return words, mask


ALL = [c for k in cases.KS for c in cases.indel_cases(k)]


def scan(read: str, seq: str, t: int, a: int, qa: int, K: int, G: int):
    rw, rm = pack(read)
    tw, _ = pack(strands(seq)[t])
    fw, _ = pack(seq)
    status, kind, L, u, w1 = host.indel_scan_host(rw, rm if rm.any() else None, tw, fw, len(read), len(seq), t, a, qa, K, G)
    insert = "".join("ACGT"[w1 >> (2 * i) & 3] for i in range(L)) if status == model.EVENT and kind == model.INS else ""
    assert status == model.EVENT or (u == 0 and w1 == 0)
    assert kind == model.INS or w1 == 0
    return status, kind, L, u, insert


@pytest.mark.parametrize("case", ALL, ids=lambda c: "%s_k%d" % (c.name, c.k))
def test_every_match_of_every_case_equals_the_model(case):
    K = case.k + 1
    found = model.matches(case.seqs, case.k, case.ends)
    assert found or not case.records
    seen = set()
    for e, n, t, a, qa, _ in found:
        want = model.scan(case.ends[e], case.seqs[n], t, a, qa, K, case.G)
        assert scan(case.ends[e], case.seqs[n], t, a, qa, K, case.G) == want, (e, n, t, a, qa)
        seen.add(want[0])
    if case.records:
        assert model.EVENT in seen


@pytest.mark.parametrize("K", (22, 56, 128))
def test_every_length_and_flanks_around_the_window_boundaries(K):
    """Deletions and insertions of 1 .. 32 bases with G = 32, the left flank K .. K + 33 bases long, on both strands: the
    flank's windows of 32 bases start at every offset of a word, and the insert fills w1 to its last bit."""
    rng = np.random.default_rng(K)
    F = dna(rng, 6 * K + 200)
    n = 0
    for L in range(1, 33):
        for extra in (0, 1, 15, 16, 17, 31, 32, 33) if L in (1, 16, 32) else (L % 7,):
            fl = K + extra
            u = cases.spot(F, 2 * K + 40 + L, L)
            reads = [(cases.del_read(F, u, L, fl, K + 12), fl, u + L, (model.EVENT, model.DEL, L, u, ""))]
            I = cases.insert_for(rng, F, u, L)
            reads.append((cases.ins_read(F, u, I, fl, K + 12), fl + L, u, (model.EVENT, model.INS, L, u, I)))
            for read, a, pos, want in reads:
                qa = pos  # (strand 0: the match right of the event starts at forward position pos)
                assert model.scan(read, F, 0, a, qa, K, 32) == want
                assert scan(read, F, 0, a, qa, K, 32) == want
                assert scan(read, F, 0, a, qa, K, L - 1 if L > 1 else 1)[0] == (model.NONE if L > 1 else model.EVENT)
                # its reverse complement on strand 1: the match right of the event there is the read's left flank, mirrored (the right flank
                # has twelve bases to spare: the event may stand a few bases further right on that strand before it is moved left)
                rc = revcomp(read)
                found = [m for m in model.matches([F], K - 1, [rc]) if m[2] == 1 and m[3] > 0]
                assert len(found) == 1
                _, _, t, a1, qa1, _ = found[0]
                assert scan(rc, F, t, a1, qa1, K, 32) == model.scan(rc, F, t, a1, qa1, K, 32) == want
                # one base of the flank substituted: no event, whichever window holds it
                for at in (a - (L if want[1] == model.INS else 0) - 1, a - (L if want[1] == model.INS else 0) - K):
                    bad = sub(read, at)
                    assert scan(bad, F, 0, a, qa, K, 32) == model.scan(bad, F, 0, a, qa, K, 32)
                    assert scan(bad, F, 0, a, qa, K, 32)[0] == model.NONE
                n += 1
    assert n >= 64


def test_an_untested_match_and_arguments_outside_their_range():
    F = "ACGT" * 12
    w, _ = pack(F)
    lib = nat.lib()
    out = (C.c_uint64 * 4)()
    args = (w.ctypes.data, None, w.ctypes.data, w.ctypes.data, 48, 48, 0)
    assert lib.vs_indel_scan_host(*args, 0, 5, 4, 16, out) == nat.VS_OK and tuple(out) == (model.UNTESTED, 0, 0, 0)
    assert lib.vs_indel_scan_host(*args, 5, 0, 4, 16, out) == nat.VS_OK and tuple(out) == (model.UNTESTED, 0, 0, 0)
    assert lib.vs_indel_scan_host(*args, 5, 5, 4, 0, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(*args, 5, 5, 4, 33, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(*args, 5, 5, 0, 16, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(*args, 48, 5, 4, 16, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(*args, 5, 48, 4, 16, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(w.ctypes.data, None, w.ctypes.data, w.ctypes.data, 48, 48, 2, 5, 5, 4, 16, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(None, None, w.ctypes.data, w.ctypes.data, 48, 48, 0, 5, 5, 4, 16, out) == nat.VS_E_ARG
    assert lib.vs_indel_scan_host(w.ctypes.data, None, w.ctypes.data, None, 48, 48, 0, 5, 5, 4, 16, out) == nat.VS_E_ARG
