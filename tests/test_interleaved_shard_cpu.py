"""An interleaved FASTQ shared among ranks, the parts that need no device: the model of the entry parities against
``vs_il_shard_plan``, the model tied to the shipped pairing rule (``vs_fastq_mates_host`` re-entered at the share
boundaries), the named mistakes shown to be mistakes, and what the two commands accept and refuse with
``--interleaved-shard``."""
import os
import random
import shutil
import subprocess

import pytest

import il_shard_model as sm
import interleaved_model as im
from conftest import ROOT
from test_interleaved_cpu import _inputs, _no_device

WORLDS = range(1, 10)


@pytest.fixture(scope="module")
def host():
    from vstrains_amd import pe as host

    return host


def sequences():
    """(T, m[0 .. T - 2]): a few thousand random ones of every density, all-true ones of odd and even length, T < W"""
    rng = random.Random(20)
    out = [(t, [True] * (t - 1)) for t in (1, 2, 3, 4, 5, 8, 9, 16, 17, 18, 63, 64, 65, 127, 128, 129)]
    out += [(0, []), (1, []), (2, [False]), (3, [True, False]), (3, [False, True])]
    for k in range(3000):
        t = rng.choice([2, 3, 5, 7, 8, 12, 19, 40, 97])
        density = rng.choice([0.05, 0.5, 0.9, 0.99])
        out.append((t, [rng.random() < density for _ in range(t - 1)]))
    return out


def test_the_plan_fed_with_the_models_functions_gives_the_brute_force_parity(host):
    checked = empty = small = 0
    for total, m in sequences():
        p = sm.parities(m, total)
        for world in WORLDS:
            spans = [sm.shard_range(total, r, world) for r in range(world)]
            fns = [sm.share_fn(m, a, b) for a, b in spans]
            want = [p[a] for a, _ in spans]
            assert sm.plan(fns) == want, (total, m, world)
            assert host.il_shard_plan(fns) == want, (total, m, world)
            # the tail pass finds the same function from the share's end (a constant whatever lies in front)
            assert [sm.tail_fn(m, a, b)[0] for a, b in spans] == fns, (total, m, world)
            checked += 1
            empty += any(a == b for a, b in spans)
            small += total < world
    assert checked > 20000 and empty > 1000 and small > 100


def test_the_plan_refuses_what_is_no_function(host):
    from vstrains_amd import _native as nat

    with pytest.raises(nat.NativeError):
        host.il_shard_plan([0, 4])


def test_each_named_mistake_changes_an_entry():
    """T = 6, W = 3: shares [0, 2), [2, 4), [4, 6)."""
    spans = [sm.shard_range(6, r, 3) for r in range(3)]
    assert spans == [(0, 2), (2, 4), (4, 6)]

    def entries(m, **mistake):
        return sm.plan([sm.share_fn(m, a, b, **mistake) for a, b in spans])

    # ignoring the look-ahead m[b - 1]: the pairs (1, 2) and (3, 4) straddle the boundaries
    m = [False, True, False, True, False]
    assert entries(m) == [sm.parities(m, 6)[a] for a, _ in spans] == [0, 1, 1]
    assert entries(m, lookahead=False) != entries(m)
    # an all-true share is identity or flip, not const-0: one name throughout, records 1..5 -- rank 1's share flips nothing
    # (two flips), so rank 2's entry is rank 1's, which is rank 0's last m
    m = [False, True, True, True, True]
    assert entries(m) == [sm.parities(m, 6)[a] for a, _ in spans] == [0, 1, 1]
    assert sm.share_fn(m, 2, 4) == sm.ID
    assert entries(m, all_true_is_const0=True) == [0, 1, 0]
    # composing in the wrong order: (true, false) leaves 0, (false, true) leaves 1
    m = [False, True, False, False, True]
    assert sm.share_fn(m, 0, 2) == sm.CONST1 and sm.share_fn(m, 0, 2, order="backward") == sm.CONST0
    assert entries(m) == [sm.parities(m, 6)[a] for a, _ in spans] == [0, 1, 0]
    assert entries(m, order="backward") != entries(m)


def _headers(rng, total):
    """record names with runs of every short length, singles between them"""
    out = []
    while len(out) < total:
        out += [b"@n%d" % len(out)] * rng.choice([1, 1, 2, 2, 2, 3, 4, 5, 7])
    return out[:total]


def test_the_shipped_rule_re_entered_at_the_share_boundaries_gives_the_single_pass(host):
    """The text cut at the ``shard_range`` boundaries; each piece is matched by ``vs_fastq_mates_host`` from the record behind
    its entry record (the record behind the second of a pair starts with parity 0) and with one look-ahead record, which
    counts only as the second of a pair: the pieces' pairs and singles, renumbered, are the whole text's."""
    rng = random.Random(5)
    for total in (1, 2, 3, 7, 30, 64, 65, 131):
        for rep in range(6):
            headers = [b"@one"] * total if rep == 0 else _headers(rng, total)
            recs = [im.record(h, k) for k, h in enumerate(headers)]
            text = b"".join(recs)
            want_pairs, want_info = host.fastq_mates(text, True)
            want_pairs = [tuple(int(x) for x in p) for p in want_pairs]
            m = sm.m_of_headers(headers, im.mates)
            p = sm.parities(m, total)
            assert want_pairs == [pr for pr in im.pairing(text)[0]]
            for world in (1, 2, 3, 4, 5, 9):
                pairs, singles = [], 0
                for r in range(world):
                    a, b = sm.shard_range(total, r, world)
                    start, end = a + p[a], min(b + 1, total)
                    if start >= b:
                        continue
                    got, info = host.fastq_mates(b"".join(recs[start:end]), end == b)
                    got = [(int(x) + start, int(y) + start) for x, y in got]
                    assert all(x < b for x, _ in got)  # (the look-ahead record never starts a pair)
                    pairs += got
                    singles += info["singles"]
                    assert (got, info["singles"]) == (sm.owned(m, total, a, b)[0], len(sm.owned(m, total, a, b)[1])), (total, world, r)
                assert pairs == want_pairs and singles == want_info["singles"], (total, rep, world)


# ---- the flag -------------------------------------------------------------------------------------------------------------
def test_the_flag_alone_is_refused_by_both_commands_before_a_device_is_opened(tmp_path, monkeypatch):
    from vstrains_amd import cli, pe_inference as pi

    a, _, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    out = tmp_path / "out"
    why = "--interleaved-shard.*needs --interleaved"
    with pytest.raises(ValueError, match=why):
        pi.interleaved_mode(False, False, True)
    assert pi.interleaved_mode(True, True, True) == "singles" and pi.interleaved_mode(True, False, True) == "strict"
    with pytest.raises(ValueError, match=why):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(out), "-f", a, "-r", a, "-k", "21", "--interleaved-shard"])
    with pytest.raises(ValueError, match=why):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(out), "-fwd", a, "-rve", a,
                  "--interleaved-shard"])
    assert not out.exists()


def test_with_the_flag_a_regular_file_is_accepted_under_a_process_group_and_a_pipe_is_not(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference as pi

    a, b, bam = _inputs(tmp_path)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    for mode in ("strict", "singles"):
        assert pi.interleaved_input(a, a, 2, mode, shard=True) == a
        assert pi.interleaved_input(a, a, 1, mode, shard=True) == a
        with pytest.raises(ValueError, match="one process only.*BGZF pairs.*collated BAMs"):  # without the flag: word for word
            pi.interleaved_input(a, a, 2, mode)
        with pytest.raises(ValueError, match="not both regular files: a pipe can be read by one process only"):
            pi.interleaved_input(fifo, fifo, 2, mode, shard=True)
        assert pi.interleaved_input(fifo, fifo, 1, mode, shard=True) == fifo  # (one process reads a pipe as before)
        with pytest.raises(ValueError, match="two different files"):
            pi.interleaved_input(a, b, 2, mode, shard=True)
        with pytest.raises(ValueError, match="is a BAM file"):
            pi.interleaved_input(bam, bam, 2, mode, shard=True)


def test_the_other_refusals_under_a_process_group_stay(tmp_path, monkeypatch):
    from vstrains_amd import cli, pe_inference as pi

    a, _, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    monkeypatch.delenv("VS_GZIP_DEVICE", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2")  # (torchrun's; the refusals come before a process group is made)
    base = ["-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "out"), "-f", a, "-r", a, "--interleaved"]
    with pytest.raises(ValueError, match="one process only"):  # without the flag the old refusal
        pi.main(base)
    with pytest.raises(ValueError, match="--count-singles: unpaired reads are counted in one process only"):
        pi.main(base + ["--interleaved-singles", "--interleaved-shard", "--count-singles"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(pi, "_rank_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="--count-singles: unpaired reads are counted in one process only"):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out"), "-fwd", a, "-rve", a,
                  "--interleaved", "--interleaved-singles", "--interleaved-shard", "--count-singles"])
    with pytest.raises(ValueError, match="--count-singles: unpaired reads are counted in one process only"):
        pi.count_links(None, str(tmp_path / "none.gfa"), a, a, 21, interleaved="singles", count_singles=True, interleaved_shard=True)
    monkeypatch.setenv("VS_GZIP_DEVICE", "1")
    with pytest.raises(ValueError, match="VS_GZIP_DEVICE=1.*one process"):
        pi.count_links(None, str(tmp_path / "none.gfa"), a, a, 21, interleaved="singles", interleaved_shard=True)
    assert not (tmp_path / "out").exists()


def test_the_new_help_texts_say_extension():
    from vstrains_amd import cli

    text = cli.build_parser().format_help()
    proc = subprocess.run([shutil.which("python3") or "python3", "-m", "vstrains_amd.pe_inference", "-h"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    for helptext in (text, proc.stdout):
        assert "--interleaved-shard extension, off by default: " in " ".join(helptext.split())


def test_the_new_entries_are_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_fastq_il_range_fn", "vs_il_shard_plan", "vs_fastq_il_open_range"):
        assert name + "(" in header
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name)
    assert _native.lib().vs_abi_version() == 11
