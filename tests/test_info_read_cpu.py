"""The reader of pe_info / st_info without a device: ``vs_info_read_host`` runs the text the kernels run
(csrc/vs_info_read_core.h: the line rule, the name table, the walk over the windows) with one thread.  Every constructed text
of info_read_cases.py goes through it at the default window, and the short ones at every window from 24 to 64 bytes, so that
a window boundary falls on every position of a line.  What is expected comes from the cases' hand-written outcomes, from the
oracle's ``DictPeLinks.from_files`` and from ``vs_info_parse``, never from the code under test.  tests/info_read_check.cpp
drives the header as plain C++ under AddressSanitizer and UBSan with every buffer exactly sized.  The command line's
``--pe-text-from`` runs over the checker backend."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import info_read_cases as irc
from conftest import ROOT
from graph_case import Case, compare
from oracle import graph_ops as chk
from test_graph_golden import CheckerBackend
from vstrains_amd import _native as nat
from vstrains_amd import cli


def _info_parse(path, names):
    """vs_info_parse (the host reader this one restates): ("ok", cells, lines, skipped), ("python",) or ("error", message)"""
    blob, off = irc.name_arrays(names)
    info = (C.c_uint64 * 4)()
    lib = nat.lib()
    if lib.vs_info_parse(str(path).encode(), blob.ctypes.data, off.ctypes.data, len(names), None, None, None, 0, info) != 0:
        return ("error", lib.vs_last_error(None).decode())
    if info[1]:
        return ("python",)
    cap = int(info[0]) + 1
    rows, cols, vals = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.int64)
    if lib.vs_info_parse(str(path).encode(), blob.ctypes.data, off.ctypes.data, len(names), rows.ctypes.data, cols.ctypes.data, vals.ctypes.data,
                         cap, info) != 0:
        return ("error", lib.vs_last_error(None).decode())
    k = int(info[0]) if info[2] else 0
    return ("ok", list(zip(rows[:k].tolist(), cols[:k].tolist(), vals[:k].tolist())), int(info[2]), int(info[3]))


@pytest.mark.parametrize("case", irc.CASES, ids=irc.CASE_IDS)
def test_the_cases_say_what_the_host_reader_and_the_oracle_say(case, tmp_path):
    """the hand-written outcomes against vs_info_parse and, where the text is read, the oracle's dict"""
    path = tmp_path / "pe_info"
    path.write_bytes(case.text)
    got = _info_parse(path, case.names)
    assert got[0] == case.kind
    if case.kind == "error":
        assert got[1] == case.message(path)
    if case.kind == "ok":
        assert got[1:] == (case.cells, len(case.cells) + case.skipped, case.skipped)
        empty = tmp_path / "st_info"
        empty.write_bytes(b"")
        table = chk.DictPeLinks.from_files(case.names, str(path), str(empty)).table
        index = {n: i for i, n in enumerate(case.names)}
        m = case.matrix()
        for (u, v), total in table.items():
            assert int(m[index[u], index[v]]) == total and int(m[index[v], index[u]]) == total, (u, v)


def _check(case, outcome, cells, rec, window):
    if not case.fits(window):
        assert outcome == "does_not_fit", (case.name, window)
        return
    assert outcome == case.kind, (case.name, window, rec)
    assert rec["flags"] != 0 if case.kind == "python" else rec["flags"] == 0
    if case.kind == "error":
        assert rec["bad_at"] == case.bad_at, (case.name, window)
    if case.kind == "ok":
        assert cells == case.cells, (case.name, window)
        assert (rec["lines"], rec["skipped"], rec["text_bytes"]) == (len(case.cells) + case.skipped, case.skipped, len(case.text))


@pytest.mark.parametrize("case", irc.CASES, ids=irc.CASE_IDS)
def test_twin_at_the_default_window(case):
    outcome, cells, rec = irc.read_host(case.text, case.names)
    _check(case, outcome, cells, rec, 256 << 20)
    assert rec["windows"] == (1 if case.text else 0)


@pytest.mark.parametrize("case", [c for c in irc.CASES if len(c.text) < 200], ids=[c.name for c in irc.CASES if len(c.text) < 200])
def test_twin_at_every_window_from_24_to_64(case):
    seen = set()
    for window in range(24, 65):
        outcome, cells, rec = irc.read_host(case.text, case.names, window)
        _check(case, outcome, cells, rec, window)
        seen.add(outcome)
        if outcome != "does_not_fit" and len(case.text) > window:
            assert rec["windows"] > 1
    assert case.kind in seen or not case.fits(64)


def test_a_boundary_falls_on_every_position_of_a_line():
    """one text of equal lines: at window w the first cut falls on byte w mod 13 of a line, so 24 .. 64 covers each of the 13
    positions -- in front of, on and behind the newline and inside every field -- at least three times"""
    line = b"12:345:67890\n"
    assert len(line) == 13
    names = ["12", "345"]
    text = line * 40
    want = [(0, 1, 67890)] * 40
    cuts = set()
    for window in range(24, 65):
        outcome, cells, rec = irc.read_host(text, names, window)
        assert outcome == "ok" and cells == want, window
        assert rec["windows"] > len(text) // window - 1
        cuts.add(window % 13)
    assert cuts == set(range(13))


def test_cells_beyond_the_room_given_are_refused():
    blob, off = irc.name_arrays(irc.NAMES)
    text = np.frombuffer(b"1:2:3\n2:3:4\n", dtype=np.uint8)
    rows, cols, vals = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int64)
    info = (C.c_uint64 * 8)()
    rc = nat.lib().vs_info_read_host(text.ctypes.data, text.size, blob.ctypes.data, off.ctypes.data, 3, 0, rows.ctypes.data, cols.ctypes.data,
                                     vals.ctypes.data, 1, info)
    assert rc == nat.VS_E_RANGE


def test_stand_alone_check_under_the_sanitizers(tmp_path):
    """tests/info_read_check.cpp: the header as plain C++, exactly sized heap buffers, AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "info_read_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "info_read_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK"
    assert sum(1 for l in lines if l.startswith("case ")) >= 10 and any(l.startswith("walk ") for l in lines)


# ---- the command line ------------------------------------------------------------------------------------------------------------
class FilesBackend(CheckerBackend):
    """the checker backend with the hand-off from files: what --pe-text-from calls"""

    def __init__(self, case):
        CheckerBackend.__init__(self, case, False)
        self.read = None
        self.unknown = 0

    def pe_links(self, *a, **kw):
        raise AssertionError("--pe-text-from must not count")

    def links_from_files(self, names, pe_file, st_file):
        self.read = (pe_file, st_file)
        table = chk.DictPeLinks.from_files(list(names), pe_file, st_file)
        if self.unknown:
            table.read_info = {"pe": {"skipped": self.unknown}, "st": {"skipped": 0}}  # (what HipPeLinks reports of the files)
        return table


def _argv(inp, out, extra=()):
    return ["-a", "spades", "-g", inp["gfa"], "-p", inp["paths"], "-o", out, "-fwd", inp["fwd"], "-rve", inp["rve"]] + list(extra)


def _tree(root):
    out = {}
    for base, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(base, fn)
            rel = os.path.relpath(p, root)
            if rel != "vstrains.log" and not rel.startswith("aln" + os.sep):
                out[rel] = open(p, "rb").read()
    return out


def test_cli_pe_text_from_gives_the_files_of_the_counting_run(tmp_path):
    case = Case("three_strain_scrambled_k21")
    inp = case.inputs(str(tmp_path))
    first = str(tmp_path / "first")
    cli.main(_argv(inp, first), backend=CheckerBackend(case, False))
    assert sorted(os.listdir(os.path.join(first, "aln"))) == ["pe_info", "st_info"]
    again = str(tmp_path / "again")
    backend = FilesBackend(case)
    timings = cli.main(_argv(inp, again, ["--pe-text-from", os.path.join(first, "aln")]), backend=backend)
    assert backend.read == (os.path.join(first, "aln", "pe_info"), os.path.join(first, "aln", "st_info"))
    assert set(timings) == {"pe_inference_s", "strain_extract_s", "total_s"}
    problems, _ = compare(case, again)  # (the reference's own files; aln/ stays empty and the log has one more line)
    assert sorted(problems) == ["differs vstrains.log.info", "missing aln/pe_info", "missing aln/st_info"], problems
    a, b = _tree(first), _tree(again)
    assert a and a == b
    assert os.listdir(os.path.join(again, "aln")) == []
    log = open(os.path.join(again, "vstrains.log")).read()
    assert "paired end information is read from %s and %s" % backend.read in log and "are not opened" in log
    assert "paired end information stored" in log and "WARNING" not in log
    # lines that named a node the graph does not have: one warning line
    backend.unknown = 3
    cli.main(_argv(inp, str(tmp_path / "third"), ["--pe-text-from", os.path.join(first, "aln")]), backend=backend)
    warnings = [l for l in open(os.path.join(str(tmp_path / "third"), "vstrains.log")).read().splitlines() if " - WARNING - " in l]
    assert len(warnings) == 1 and warnings[0].split(" - WARNING - ")[1].startswith("3 lines of the paired end information name a node")


def test_cli_pe_text_from_prefers_the_gz_pair_and_needs_a_whole_pair(tmp_path, capsys):
    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path))
    aln = tmp_path / "aln"
    aln.mkdir()
    (aln / "pe_info").write_text("")
    (aln / "st_info.gz").write_text("")
    assert cli.pe_text_pair(str(aln)) is None
    with pytest.raises(SystemExit) as ei:
        cli.main(_argv(inp, str(tmp_path / "never"), ["--pe-text-from", str(aln)]), backend=FilesBackend(case))
    assert ei.value.code == 1 and "--pe-text-from" in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "never")
    (aln / "st_info").write_text("")
    assert cli.pe_text_pair(str(aln)) == (str(aln / "pe_info"), str(aln / "st_info"))
    (aln / "pe_info.gz").write_text("")
    assert cli.pe_text_pair(str(aln)) == (str(aln / "pe_info.gz"), str(aln / "st_info.gz"))


@pytest.mark.parametrize("flag", ["--no-pe-text", "--sparse-pe-text", "--bgzf-pe-text"])
def test_cli_pe_text_from_conflicts(tmp_path, flag):
    case = Case("two_strain_bubbles_k21")
    inp = case.inputs(str(tmp_path))
    with pytest.raises(SystemExit) as ei:
        cli.main(_argv(inp, str(tmp_path / "never"), ["--pe-text-from", str(tmp_path), flag]), backend=FilesBackend(case))
    assert ei.value.code == 2
    assert not os.path.exists(tmp_path / "never")
