"""The member-sharded open of a collated BAM, the parts that need no device: the summary of a share (the host twin of the
kernels, ``vs_bam_share_summary_host``) against the pure-Python model candidate for candidate, the plan (``vs_bam_shard_plan``)
against the model's entries, parities and fallbacks, and the composition property on random files.  tests/bam_shard_check.cpp
drives the same header as plain C++ under AddressSanitizer and UBSan with every buffer exactly sized."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_shard_model as model
import bam_util as bu
from conftest import ROOT

SEGS = (64, 128, 4096)


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def messages(host, data, S, seg, chunk=0, ctx=None, tail=model.TAIL):
    """Every rank's pass-1 message from the inflated file: the share and `tail` bytes behind it (or the rest of the file)."""
    H, T = bu.header_len(data), len(data)
    out = []
    for r in range(len(S) - 1):
        lo, hi = S[r], S[r + 1]
        x, n, _ = host.bam_share_summary(data[lo:min(T, hi + tail)], hi - lo, H if r == 0 else None, seg, chunk, ctx)
        out.append([0, 1, 7, H, hi - lo, len(x)] + x + n)
    return out


def block_off_the_records(data, worlds, blocks=(2003, 1499, 997, 613, 389, 211, 97)):
    """a member size (the largest that still gives every rank members) at which no share boundary of these worlds is a record start"""
    starts = {t[0] for t in bu.walk(data)[0]}
    for block in blocks:
        if len(data) // block < 2 * max(worlds) and block != blocks[-1]:
            continue
        sizes = model.member_sizes(len(data), block)
        if all(not (set(model.boundaries(sizes, w)[1:-1]) & starts) for w in worlds):
            return sizes
    raise AssertionError("every block lines up with a record")


def check_plan(host, data, S, seg, msgs):
    """the plan of these messages is what the definitions say; returns the model's verdict"""
    want = model.plan(data, S, seg)
    plan, reason = host.bam_shard_plan(msgs)
    if want[0] != "ok":
        assert (plan, reason) == (None, want), (S, seg)
        return want
    assert reason is None, (reason, S, seg)
    _, entries, before, total = want
    assert [S[r] + p[0] for r, p in enumerate(plan)] == entries and [p[2] for p in plan] == before and [p[3] for p in plan] == S[:-1]
    assert [p[1] for p in plan] == [entries[r + 1] - S[r] for r in range(len(S) - 2)] + [None]
    assert [p[4] for p in plan] == before[1:] + [total]
    t_entries, t_before, _, end, t_total = model.truth(data, S)
    assert end[0] == "clean" and (entries, before, total) == (t_entries, t_before, t_total)  # (the chained summaries ARE the true chain)
    return want


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("case", bu.constructed(), ids=lambda c: c[0])
def test_summary_is_the_models_candidate_for_candidate(host, case, seg):
    """Fake headers in quality, name and aux bytes (one chain of them lands on a true record start), dropped classes between
    the mates, a 70 KB record that skips segments: X and N of every candidate of every share."""
    name, data = case
    worlds = range(1, 9) if len(data) < 20000 else (2, 7)
    sizes = block_off_the_records(data, worlds)
    seen = {}
    ok = 0
    for world in worlds:
        S = model.boundaries(sizes, world)
        msgs = messages(host, data, S, seg, chunk=(0, 50, 1000)[world % 3])
        for r in range(1 if world > 1 else 0, world):
            lo, hi = S[r], S[r + 1]
            if (r == 0, lo, hi) not in seen:
                cands = [bu.header_len(data)] if r == 0 else range(min(seg, hi - lo))
                seen[(r == 0, lo, hi)] = [model.summary(data, lo, hi, c) for c in cands]
            want = seen[(r == 0, lo, hi)]
            c = msgs[r][5]
            assert c == len(want) and list(zip(msgs[r][6:6 + c], msgs[r][6 + c:])) == want, (name, world, r)
        ok += check_plan(host, data, S, seg, msgs)[0] == "ok"
    if name in ("mixed", "fakes"):
        # no test passes by falling back: no record of these files is longer than 4 096 bytes, so no share boundary sends the
        # ranks to the whole file there (segments of 64 and 128 are shorter than most records, and many boundaries do)
        assert ok == len(worlds) if seg == 4096 else ok >= 1, (ok, seg)
        parities = {n & 1 for (_, n) in sum(seen.values(), [])}
        assert parities == {0, 1}  # (candidates of one share disagree about the parity)


def test_two_shares_cut_at_every_member_boundary_and_at_the_edges_of_records(host):
    """One small file in members of 37 bytes, two shares cut at every member boundary; then cuts flush with a record's start,
    inside its size field and inside its fixed part, where the share's own bytes do not say how the record goes on."""
    name, data = [c for c in bu.constructed() if c[0] == "fakes"][0]
    T, starts = len(data), [t[0] for t in bu.walk(data)[0]]
    cuts = [(c, "member") for c in range(37, T, 37) if bu.header_len(data) < c <= starts[-1]]  # (behind the last start the last share holds no record start: a fallback)
    for k in (3, 6, 9):
        cuts += [(starts[k], "flush"), (starts[k] + 2, "size field"), (starts[k] + 20, "fixed part"), (starts[k] + 36, "behind the fixed part")]
    verdicts = {}
    for cut, what in cuts:
        S = [0, cut, T]
        for seg, chunk in ((64, 0), (4096, 41)):
            msgs = messages(host, data, S, seg, chunk)
            want = [model.summary(data, cut, T, c) for c in range(min(seg, T - cut))]
            c = msgs[1][5]
            assert list(zip(msgs[1][6:6 + c], msgs[1][6 + c:])) == want, (cut, what, seg)
            verdicts.setdefault(what, []).append(check_plan(host, data, S, seg, msgs))
        if what == "flush":
            plan, _ = host.bam_shard_plan(msgs)
            assert plan[1][0] == 0 and plan[0][1] == cut  # (the next share is entered at its first byte)
    # (per cut: segments of 64, then of 4 096, which no record of the file exceeds -- there no cut is a fallback)
    assert all(v[0] == "ok" for vs in verdicts.values() for v in vs[1::2])
    assert all(v[0] == "ok" for v in verdicts["flush"])


FLAGS = (bu.PAIRED | bu.FIRST, bu.PAIRED | bu.SECOND, bu.PAIRED | bu.FIRST | bu.REVERSE, bu.PAIRED | bu.SECOND | bu.REVERSE)
DROPPED = (bu.PAIRED | bu.FIRST | bu.SECONDARY, bu.PAIRED | bu.SECOND | bu.SUPPLEMENTARY, 0, bu.PAIRED | bu.FIRST | bu.SECOND, bu.PAIRED)


def random_file(rng):
    recs = []
    for i in range(int(rng.integers(1, 16))):
        mates = [bu.rec("p%d" % i, FLAGS[int(rng.integers(0, 4)) & 2], bu._seq(rng, int(rng.integers(0, 90)))),
                 bu.rec("p%d" % i, FLAGS[1 + (int(rng.integers(0, 4)) & 2)], bu._seq(rng, int(rng.integers(0, 90))))]
        if rng.integers(0, 2):
            mates.reverse()
        for m in mates:
            while rng.integers(0, 4) == 0:
                recs.append(bu.rec("d%d" % len(recs), DROPPED[int(rng.integers(0, len(DROPPED)))], bu._seq(rng, int(rng.integers(0, 60))),
                                   aux=bytes(int(v) for v in rng.integers(0, 256, size=int(rng.integers(0, 40))))))
            recs.append(m)
    if rng.integers(0, 12) == 0:
        recs.pop()  # (an odd participating record now and then)
    return bu.inflated(recs)


def test_chained_summaries_give_every_rank_its_entry_parity_and_couples(host):
    """Random records, flags, member sizes, world sizes and segments: the plan from the chained summaries has the model's
    entries and counts (or the model's reason), and the ranks' couples, in rank order, are the single reader's list."""
    rng = np.random.default_rng(2024)
    verdicts = {}
    for draw in range(3000):
        data = random_file(rng)
        seg = (64, 128, 4096, 4096)[int(rng.integers(0, 4))]
        sizes = model.member_sizes(len(data), int(rng.integers(30, 700)))
        world = int(rng.integers(1, min(8, len(sizes)) + 1))
        S = model.boundaries(sizes, world)
        msgs = messages(host, data, S, seg, chunk=int(rng.integers(0, 3)) * int(rng.integers(40, 400)), tail=model.TAIL + int(rng.integers(0, 30)))
        want = check_plan(host, data, S, seg, msgs)
        verdicts[want if isinstance(want, str) else "ok"] = verdicts.get(want if isinstance(want, str) else "ok", 0) + 1
        if want[0] != "ok":
            continue
        plan, _ = host.bam_shard_plan(msgs)
        _, _, couples, _, total = model.truth(data, S)
        single = [c for rank in couples for c in rank]
        part = [t[0] for t in bu.walk(data)[0] if model.takes_part(t)]
        assert single == [(part[2 * c], part[2 * c + 1]) for c in range(total // 2)], draw  # each couple once, in file order
        first = 0
        for r, p in enumerate(plan):  # what BamStream.shard_open derives from the plan
            assert ((p[2] + 1) // 2, (p[4] + 1) // 2 - (p[2] + 1) // 2) == (first, len(couples[r])), (draw, r)
            first += len(couples[r])
    print(verdicts)
    # (half the draws have segments longer than any record: of those only an odd file, 1 in 12, or a header longer than
    # rank 0's share falls back)
    assert verdicts["ok"] > 1000 and len(verdicts) >= 3


def _case(name):
    return [c for c in bu.constructed() + [m[:2] for m in bu.malformed()] if c[0] == name][0][1]


def test_every_fallback_is_reached_and_has_its_reason(host):
    R = host.BAM_SHARD_REASONS
    reached = {}

    def run(name, S, seg=4096):
        data = _case(name)
        S = S(data) if callable(S) else S
        msgs = messages(host, data, S, seg)
        want = model.plan(data, S, seg)
        plan, reason = host.bam_shard_plan(msgs)
        assert want != "ok" and isinstance(want, str) and (plan, reason) == (None, want), (name, want, reason)
        for rank_copy in range(len(msgs)):  # every rank decides from its own copy of the gathered values
            assert host.bam_shard_plan(copy.deepcopy(msgs)) == (None, want)
        reached[want] = name
        return msgs

    msgs = run("odd_record", lambda d: [0, 500, len(d)])
    run("block_size_31", lambda d: [0, 300, len(d)])
    run("cut_size_field", lambda d: [0, 400, len(d)])          # the file ends inside a size field
    run("cut_record", lambda d: [0, 400, len(d) - 5, len(d)])  # ... beyond the file from an inner share
    run("cut_record", lambda d: [0, 400, len(d)])              # the last share's chain ends beyond the file
    run("big_header", lambda d: [0, 1000, len(d)])             # the header alone is longer than rank 0's share
    aux = _case("big_aux")
    start = [t[0] for t in bu.walk(aux)[0]][1]
    run("big_aux", [0, start + 500, len(aux)], seg=64)                 # a 70 KB record across the boundary, segments of 64
    run("mixed", lambda d: [0, 700, 700, len(d)])              # a share without bytes
    not_bgzf = copy.deepcopy(msgs)
    for m in not_bgzf:
        m[1] = 0
        del m[6:]
        m[5] = 0
    assert host.bam_shard_plan(not_bgzf) == (None, R[3])
    reached[R[3]] = "a gzip member appended"
    assert set(reached) == set(R.values()), sorted(set(R.values()) - set(reached))
    # the same 70 KB record is no fallback when the segment holds the exit, and a failed rank is an error, not a fallback
    assert model.plan(aux, [0, start + 70000, len(aux)], 4096)[0] == "ok"
    assert host.bam_shard_plan(messages(host, aux, [0, start + 70000, len(aux)], 4096))[1] is None
    failed = copy.deepcopy(msgs)
    failed[1] = [1, 0, 0, 0, 0, 0]
    with pytest.raises(RuntimeError, match=r"BAM open failed on rank\(s\) \[1\]"):
        host.bam_shard_plan(failed)
    differ = copy.deepcopy(msgs)
    differ[1][2] += 1
    with pytest.raises(RuntimeError, match="do not see the same BAM"):
        host.bam_shard_plan(differ)


def test_input_choice_under_a_process_group(tmp_path):
    """``bam_input`` called as before keeps refusing a process group; the sharded route is a keyword of its own, and matching
    by name stays refused there with a message that says why."""
    from vstrains_amd import pe_inference

    a = tmp_path / "a.bam"
    a.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    with pytest.raises(ValueError, match="one process only"):
        pe_inference.bam_input(str(a), str(a), world=2)
    assert pe_inference.bam_input(str(a), str(a), world=2, sharded=True) == str(a)
    assert pe_inference.bam_input(str(a), str(a), world=1, sharded=True) == str(a)
    for sharded in (False, True):
        with pytest.raises(ValueError, match="--bam-by-name.*one process only.*different"):
            pe_inference.bam_input(str(a), str(a), world=2, by_name=True, sharded=sharded)


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/bam_shard_check.cpp: the summary and the plan of vs_bam_core.h as plain C++, exactly sized heap buffers,
    AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "bam_shard_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bam_shard_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines()[-1] == "OK"
