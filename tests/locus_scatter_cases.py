"""Blocks for the turns of k_locus_scatter (vstrains_amd/csrc/vs_pe.hip): a thread of the 1 024 of a workgroup places
LOCUS_SCATTER_U pairs of its chunk a turn -- pairs lo + tid + 1024 * (U * i + j), j < U -- so what can go wrong sits where a
chunk ends inside a turn: one live lane in a turn's first row, a chunk of exactly whole turns, one pair more than that,
and chunks far smaller than a row (16 to 19 pairs: every lane in the first turn, most of them idle).

A block of n pairs is block 0 of tests/test_pe_counters_gpu._locus_inputs repeated: its encoded text tiled with numpy (a
million Python strings are too slow to make), pair p of the block being pair p mod n0 of the inputs.  No device here:
tests/test_locus_scatter_cases_cpu.py holds this file to the kernel's constants and to the inputs it tiles."""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vstrains_amd", "csrc")
WGS, TPB = 256, 1024  # LOCUS_WGS (vs_pe_plan.h), LOCUS_TPB (vs_pe.hip)


def _define(path, name):
    with open(os.path.join(_CSRC, path)) as fh:
        m = re.search(r"^#define %s (\d+)u?\b" % name, fh.read(), re.M)
    return int(m.group(1))


def constants():
    return dict(wgs=_define("vs_pe_plan.h", "LOCUS_WGS"), tpb=_define("vs_pe.hip", "LOCUS_TPB"), u=_define("vs_pe.hip", "LOCUS_SCATTER_U"))


U = constants()["u"]
ROW = TPB * U  # pairs a workgroup places a turn

# chunks round 1024 * U.  The first three are the sizes the issue names; its "- 255" gives the chunk 1024 * U with a short
# LAST workgroup (1024 * U - 255 pairs), so the chunk one BELOW 1024 * U is added as the fourth: 256 * (1024 * U - 1).
TURN_SIZES = [WGS * ROW - 255, WGS * ROW, WGS * ROW + 1, WGS * (ROW - 1)]
SMALL_SIZES = [4096, 4097, 4353, 4609]  # chunks of 16, 17, 18, 19
CHAIN_SIZES = [4097, WGS * ROW + 1]     # two LDS passes: key_lo > 0 in the second


def chunk_of(n_pairs):
    return -(-n_pairs // WGS)


def shape(n_pairs):
    """How the scatter walks a block: the chunk, the pairs of the last workgroup that has any, the workgroups with none,
    per workgroup of a full chunk the turns and the live lanes of the last turn's last started row."""
    chunk = chunk_of(n_pairs)
    full_wgs = n_pairs // chunk
    last = n_pairs - full_wgs * chunk
    empty = WGS - full_wgs - (1 if last else 0)
    turns = -(-chunk // ROW)
    in_last_turn = chunk - (turns - 1) * ROW
    rows_last_turn = -(-in_last_turn // TPB)
    lanes_last_row = in_last_turn - (rows_last_turn - 1) * TPB
    return dict(chunk=chunk, last_wg_pairs=last, empty_wgs=empty, turns=turns, rows_last_turn=rows_last_turn, lanes_last_row=lanes_last_row)


def tile(fwd, rve, n_pairs):
    """(bytes uint8, off uint64 [2 n_pairs + 1]) for Context.pack: ends 2 p, 2 p + 1 = fwd[p mod n0], rve[p mod n0]."""
    n0 = len(fwd)
    lens = np.empty(2 * n0, dtype=np.int64)
    lens[0::2] = [len(x) for x in fwd]
    lens[1::2] = [len(x) for x in rve]
    text = np.frombuffer("".join(x for pair in zip(fwd, rve) for x in pair).encode("latin-1"), dtype=np.uint8)
    reps, rest = divmod(n_pairs, n0)
    rest_bytes = int(lens[: 2 * rest].sum())
    data = np.concatenate([np.tile(text, reps), text[:rest_bytes]])
    all_lens = np.concatenate([np.tile(lens, reps), lens[: 2 * rest]])
    off = np.zeros(2 * n_pairs + 1, dtype=np.uint64)
    off[1:] = np.cumsum(all_lens).astype(np.uint64)
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(data), off


def allowed_table(allowed):
    """allowed (a set of keys per pair of the inputs) as an int64 array [n0, most keys of a pair], padded with -1, so that a
    million keys are checked at once (keys_allowed)."""
    t = np.full((len(allowed), max(len(a) for a in allowed)), -1, dtype=np.int64)
    for p, a in enumerate(allowed):
        t[p, : len(a)] = sorted(a)
    return t


def keys_allowed(keys, table):
    """Per pair of a tiled block: its key is one of those its inputs' pair may have."""
    rows = table[np.arange(keys.size) % table.shape[0]]
    return (rows == keys.astype(np.int64)[:, None]).any(axis=1)
