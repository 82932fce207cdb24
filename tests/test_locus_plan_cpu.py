"""The staged key pass of the locus sort on the CPU (vstrains_amd/csrc/vs_pe_plan.h: vs_locus_batch, vs_locus_span, the
staging decision of vs_pe_plan): tests/locus_batch_check.cpp, built here with the host compiler under AddressSanitizer and
UBSan, walks the batches of constructed blocks at every buffer capacity as a wavefront of k_locus_count_staged does, checks
every staged index against the buffer itself, and prints the cuts; here they are compared with the plain statement -- a
batch is the longest run of the remaining pairs whose words fit, at most 64 of them, and a pair that does not fit alone
goes alone, unstaged.  The plan's decisions are compared with what the project states (the locus sort).  No
device, no HIP call."""
import json
import os
import shutil
import subprocess

import pytest

import test_pe_plan_cpu as plan_cpu
from test_pe_plan_cpu import plan  # noqa: F401  (the fixture: plans through oracle/plan_check.cpp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_WORDS, WAVES, SLACK, MAX_PAIRS, QUADS = 40960, 16, 16, 64, 5  # 160 KB; LOCUS_STAGE_* of vs_pe_plan.h


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("locus_batch") / "locus_batch_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "locus_batch_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.splitlines()


def model(woff, lo, hi, cap):
    """The batches of pairs [lo, hi) as (pairs, staged), by the plain statement."""
    out, p = [], lo
    while p < hi:
        n = 0
        while n < MAX_PAIRS and p + n < hi and woff[2 * (p + n + 1)] - woff[2 * p] <= cap:
            n += 1
        out.append((n, 1) if n else (1, 0))
        p += out[-1][0]
    return out


def test_batches_tile_every_chunk_at_every_capacity(printed):
    blocks, seen, walks = {}, {}, 0
    for line in printed:
        if line.startswith("W "):
            name, vals = line[2:].split("|")
            blocks[name.strip()] = [int(v) for v in vals.split()]
        elif line.startswith("B "):
            head, cuts = line[2:].split("|")
            name, cap, lo, hi = head.split()
            cap, lo, hi = int(cap), int(lo), int(hi)
            woff = blocks[name]
            got = [tuple(int(v) for v in c.split(":")) for c in cuts.split()]
            # in order, no pair twice, none missing (the cuts are run lengths from lo), each the longest run that fits
            assert sum(n for n, _ in got) == hi - lo, (name, cap, lo, hi)
            assert got == model(woff, lo, hi, cap), (name, cap, lo, hi, got[:6], model(woff, lo, hi, cap)[:6])
            s = seen.setdefault(name, dict(caps=set(), staged=0, alone=0, full=0, partial_last=0, sizes=set()))
            s["caps"].add(cap)
            s["staged"] += sum(st for _, st in got)
            s["alone"] += sum(1 - st for _, st in got)
            s["full"] += sum(n == MAX_PAIRS for n, _ in got)
            s["sizes"] |= {n for n, st in got if st}
            s["partial_last"] += len(got) > 1 and got[-1][0] < got[0][0]
            walks += 1
    assert set(blocks) == {"uniform", "singles", "nothing", "mixed", "oversize", "one", "empty"} and walks > 500
    # every capacity from one word up
    assert seen["uniform"]["caps"] >= set(range(1, 71)) and seen["mixed"]["caps"] >= set(range(1, 81))
    # a pair exactly at capacity is staged, one word over it goes alone: 2 x 10 words at capacities 20 and 19
    u = blocks["uniform"]
    assert model(u, 0, 150, 20)[0] == (1, 1) and model(u, 0, 150, 19)[0] == (1, 0) and model(u, 0, 150, 39)[0] == (1, 1) and model(u, 0, 150, 40)[0] == (2, 1)
    assert seen["uniform"]["staged"] and seen["uniform"]["alone"] and seen["uniform"]["partial_last"]  # (64 pairs of 20 words are more than any buffer holds: full batches are the next blocks')
    # batches capped by the lanes, not by the words: ends of no words
    assert seen["nothing"]["sizes"] == {MAX_PAIRS, 140 % MAX_PAIRS, (140 - 5) % MAX_PAIRS, 1} and seen["nothing"]["alone"] == 0
    assert seen["singles"]["full"] and seen["singles"]["alone"]
    # oversize pairs among pairs that fit, and nothing but oversize pairs
    assert seen["mixed"]["alone"] and seen["mixed"]["staged"] and len(seen["mixed"]["sizes"]) > 5
    assert model(blocks["oversize"], 0, 9, 65) == [(1, 0)] * 9 and model(blocks["oversize"], 0, 9, 66) == [(1, 1)] * 9
    assert seen["one"]["staged"] and seen["one"]["alone"] and seen["empty"]["staged"] == seen["empty"]["alone"] == 0


def test_plan_stages_where_the_histogram_leaves_room(printed):
    plans = {}
    for line in printed:
        if line.startswith("P "):
            name, lds_sort, per_pass, stage, lds = line[2:].split()
            plans[name] = dict(lds_sort=int(lds_sort), per_pass=int(per_pass), stage=int(stage), lds=int(lds))

    def carve(p):  # histogram, then two buffers per wavefront, each its capacity rounded to quads and the slack
        return 4 * (((p["per_pass"] + 3) & ~3) + 2 * WAVES * (((p["stage"] + 3) & ~3) + SLACK))

    c2 = plans["config2"]
    # configs[2]: 5 041 keys, one pass; two buffers per wavefront inside 160 KB, as large as the rest of it allows
    assert (c2["lds_sort"], c2["per_pass"]) == (1, 5041) and c2["stage"] > 0
    assert c2["lds"] == carve(c2) <= 4 * LDS_WORDS < carve(dict(c2, stage=c2["stage"] + 4))
    assert c2["stage"] + SLACK <= QUADS * 4 * 64  # what a wavefront's loads cover
    assert c2["stage"] >= 50 * 20                 # fifty pairs of 2 x 150 bases a batch
    # the hook: off, a capacity of its own, never more than fits
    assert plans["config2_off"] == dict(c2, stage=0, lds=4 * 5041)
    for name, cap in (("config2_48", 48), ("config2_257", 257), ("config2_huge", c2["stage"])):
        assert plans[name]["stage"] == cap and plans[name]["lds"] == carve(plans[name]) <= 4 * LDS_WORDS
    assert plans["small_block"]["stage"] == c2["stage"] and plans["no_sort"] == dict(lds_sort=0, per_pass=0, stage=0, lds=0)
    # no staging: the global-atomic sort, a pass of 36 864 keys, the multi-pass sort, graphs beyond the LDS sort
    assert plans["config2_global"] == dict(lds_sort=0, per_pass=0, stage=0, lds=0)
    for name in ("keys_36864", "keys_36864_64", "multipass", "multipass_64"):
        assert plans[name] == dict(lds_sort=1, per_pass=36864, stage=0, lds=4 * 36864), name
    assert plans["beyond_lds"]["lds_sort"] == 0 and plans["beyond_lds"]["stage"] == 0
    # one pass that leaves little: production keeps the per-pair loads, the hook still stages (and fits)
    assert plans["keys_36863"] == dict(lds_sort=1, per_pass=36863, stage=0, lds=4 * 36863)
    assert plans["keys_36863_64"]["stage"] == 64 and plans["keys_36863_64"]["lds"] == carve(plans["keys_36863_64"]) <= 4 * LDS_WORDS
    # production stages where a buffer holds 48 pairs of the block's longest reads (LOCUS_STAGE_MIN_PAIRS): 2 x 150 bases are
    # 20 words a pair -- 9 000 keys leave 49 pairs a buffer, 10 000 leave 47; at 5 041 keys 2 x 176 bases (22 words) fit 50
    # times, 2 x 177 (24 words) 46 times, 2 x 250 (32 words) 34 times.  The hook stages whatever the reads' length.
    assert plans["keys_9000"]["stage"] == 980 and plans["keys_9000"]["lds"] == carve(plans["keys_9000"]) <= 4 * LDS_WORDS
    assert plans["keys_10000"] == dict(lds_sort=1, per_pass=10000, stage=0, lds=4 * 10000)
    assert plans["len_176"] == c2 and plans["len_250_huge"] == c2
    assert plans["len_177"] == plans["len_250"] == plans["config2_off"]


def test_recorded_fields_of_the_parent_keep_their_values(plan):
    """The fields tests/golden/pe_plan_parent.json records, over its inputs, through oracle/plan_check.cpp as
    tests/test_pe_plan_cpu.py reads them: the staging decision changed none of them."""
    with open(os.path.join(ROOT, "tests", "golden", "pe_plan_parent.json")) as f:
        g = json.load(f)
    plans, msgs = plan([r[0] for r in g["rows"]])
    for (inp, want, msg), got, got_msg in zip(g["rows"], plans, msgs):
        assert [got[f] for f in plan_cpu.OUT] == want and got_msg == msg, dict(zip(plan_cpu.IN, inp))
