"""Host side of PE-link inference: the Python mirror of the reference's
``utils/VStrains_PE_Inference.py`` (file:line citations are into /root/reference) on top of the
HIP library.  Torch is used for device buffers, the stream and torch.distributed only."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .dist import U32_LIMIT, ExchangeState


# ---- text inputs ---------------------------------------------------------------------------------
def _universal_newlines(raw: bytes) -> bytes:
    # open(path, "r") translates \r\n and lone \r to \n (PE_Inference.py:105,147-150 use text mode)
    if b"\r" in raw:
        raw = raw.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
    return raw


def read_gfa_segments(path: str) -> Tuple[List[str], List[str]]:
    """``S`` records in file order -> (ids, sequences).  Every line loses its last character
    before the tab split, whatever that character is (PE_Inference.py:105-112)."""
    with open(path, "rb") as fh:
        raw = _universal_newlines(fh.read())
    ids: List[str] = []
    seqs: List[str] = []
    pieces = raw.split(b"\n")
    last_has_nl = raw.endswith(b"\n")
    if last_has_nl:
        pieces = pieces[:-1]
    for i, piece in enumerate(pieces):
        if i == len(pieces) - 1 and not last_has_nl:
            piece = piece[:-1]  # no newline to drop: a real character goes instead
        cols = piece.split(b"\t")
        if cols[0] == b"S":
            ids.append(cols[1].decode("latin-1"))
            seqs.append(cols[2].decode("latin-1"))
    return ids, seqs


class FastqPair:
    """Both FASTQ files mapped and indexed by the library's multi-threaded host ingest
    (``vs_fastq_*``).  ``ctx`` may be None for host-only use (indexing, ``sequence``, ``gather``)."""

    def __init__(self, fwd: str, rve: str, ctx: "Context" = None):
        self._ctx = ctx
        h = C.c_void_p()
        rc = nat.lib().vs_fastq_open(ctx._h if ctx is not None else None, fwd.encode(), rve.encode(), C.byref(h))
        if rc != nat.VS_OK:
            msg = nat.lib().vs_last_error(ctx._h if ctx is not None else None).decode("utf-8", "replace")
            if "cannot open" in msg:
                raise FileNotFoundError(msg)
            if rc == nat.VS_E_UTF8:  # the reference's readlines() raises UnicodeDecodeError, a ValueError (PE_Inference.py:147-152)
                raise ValueError(msg)
            raise nat.NativeError(rc, msg)
        self._h = h
        info = (C.c_uint64 * 3)()
        nat.lib().vs_fastq_info(h, info)
        self.n_pairs = int(info[0])
        self.lines = (int(info[1]), int(info[2]))

    @classmethod
    def open_shard(cls, fwd: str, rve: str, ctx: "Context", rank: int, world: int, all_gather=None) -> "FastqPair":
        """This rank's contiguous block of the pairs without any rank reading a whole file: rank r counts the newlines
        of byte range r of both files (``vs_fastq_count_part``), the counts are exchanged (``all_gather``: a callable
        that takes this rank's list of integers and returns every rank's, default ``torch.distributed``), the total
        ``min(lines_f // 4, lines_r // 4)`` (PE_Inference.py:154) and this rank's record range follow, and only the
        bytes of those records are indexed (``vs_fastq_open_records``).  ``first`` / ``total_pairs`` say where the block
        lies.  gzip files and files with carriage returns are opened whole by every rank (``whole = True``).

        ``all_gather`` is called TWICE per open, on every rank alike and in this order: once with seven integers (the six
        counts and a failure flag) and once with one (the status of the open itself, whole-file or by records).  A caller
        that brings its own must accept lists of either length (it is handed this rank's list and returns the list of
        every rank's lists, rank order)."""
        from .dist import shard_range

        L = nat.lib()
        # A rank that fails (a missing file, a stale count) must not leave its peers waiting in the exchange: the failure
        # travels WITH the counts (a seventh integer) and with a second, one-integer exchange after the open, and every
        # rank raises.
        mine, failure = [], None
        for path in (fwd, rve):
            out = (C.c_uint64 * 3)()
            rc = L.vs_fastq_count_part(path.encode(), rank, world, out)
            if rc != nat.VS_OK and failure is None:
                msg = L.vs_last_error(None).decode("utf-8", "replace")
                failure = FileNotFoundError(msg) if "cannot open" in msg else ValueError(msg) if rc == nat.VS_E_UTF8 else nat.NativeError(rc, msg)
            mine += [int(out[0]), int(out[1]), int(out[2])] if rc == nat.VS_OK else [0, 0, 0]
        mine.append(0 if failure is None else 1)
        if all_gather is None:
            import torch
            import torch.distributed as dist

            def all_gather(vals):
                t = torch.tensor(vals, dtype=torch.int64)
                if dist.get_backend() == "nccl":
                    t = t.cuda()
                got = [torch.zeros_like(t) for _ in range(world)]
                dist.all_gather(got, t)
                return [[int(x) for x in g.cpu().tolist()] for g in got]

        everyone = all_gather(mine)
        if failure is not None:
            raise failure
        failed = [r for r, vals in enumerate(everyone) if len(vals) > 6 and vals[6]]
        if failed:
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        flags = 0
        for vals in everyone:
            flags |= vals[2] | vals[5]
        if flags & 3:  # carriage returns or gzip somewhere: every rank opens the files whole and takes its block of them
            # (a rank that fails alone here -- out of memory while inflating, a transient read error -- tells its peers
            # through the same one-integer exchange as below, so that every rank raises instead of one)
            fq, err = None, None
            try:
                fq = cls(fwd, rve, ctx)
            except Exception as e:  # noqa: BLE001 (whatever it is, the peers must hear of it)
                err = e
            status = all_gather([0 if err is None else 1])
            if err is not None:
                raise err
            failed = [r for r, vals in enumerate(status) if vals[0]]
            if failed:
                fq.close()
                raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
            fq.total_pairs = fq.n_pairs
            fq.first, last = shard_range(fq.n_pairs, rank, world)
            fq.block_offset = fq.first
            fq.n_pairs = last - fq.first
            fq.whole = True
            return fq
        counts = [np.asarray([vals[3 * i] for vals in everyone], dtype=np.uint64) for i in range(2)]
        lines = [int(counts[i].sum()) + (1 if any(vals[3 * i + 2] & 4 for vals in everyone) else 0) for i in range(2)]
        total = min(lines[0] // 4, lines[1] // 4)
        first, last = shard_range(total, rank, world)
        self = cls.__new__(cls)
        self._ctx = ctx
        h = C.c_void_p()
        rc = L.vs_fastq_open_records(ctx._h if ctx is not None else None, fwd.encode(), rve.encode(), world, counts[0].ctypes.data,
                                     counts[1].ctypes.data, first, last, C.byref(h))
        err = None
        if rc != nat.VS_OK:
            msg = L.vs_last_error(ctx._h if ctx is not None else None).decode("utf-8", "replace")
            err = ValueError(msg) if rc == nat.VS_E_UTF8 else nat.NativeError(rc, msg)
        status = all_gather([0 if err is None else 1])
        if err is not None:
            raise err
        failed = [r for r, vals in enumerate(status) if vals[0]]
        if failed:
            if h:
                L.vs_fastq_close(h)
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        self._h = h
        self.n_pairs = last - first
        self.lines = tuple(lines)
        self.total_pairs, self.first, self.block_offset, self.whole = total, first, 0, False
        return self

    @property
    def bytes_indexed(self) -> int:
        return int(nat.lib().vs_fastq_bytes_indexed(self._h))

    def __len__(self):
        return self.n_pairs

    def close(self):
        if self._h:
            nat.lib().vs_fastq_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _raise(ctx_h, rc):
        msg = nat.lib().vs_last_error(ctx_h).decode("utf-8", "replace")
        if rc == nat.VS_E_UTF8:  # the reference's readlines() raises UnicodeDecodeError, a ValueError (PE_Inference.py:147-152)
            raise ValueError(msg)
        raise nat.NativeError(rc, msg)

    def sequence(self, which: int, record: int) -> str:
        """The CHARACTERS of a sequence line, one byte each ('?' stands for a multi-byte UTF-8 character)."""
        n = C.c_uint32(0)
        rc = nat.lib().vs_fastq_sequence(self._h, which, record, None, 0, C.byref(n))
        if rc == nat.VS_E_UTF8:
            self._raise(None, rc)
        if rc != nat.VS_OK:
            raise IndexError(record)
        buf = np.zeros(max(n.value, 1), dtype=np.uint8)
        nat.lib().vs_fastq_sequence(self._h, which, record, buf.ctypes.data, buf.size, C.byref(n))
        return bytes(buf[: n.value]).decode("latin-1")

    def gather(self, first: int, count: int) -> Tuple[np.ndarray, np.ndarray]:
        off = np.zeros(2 * count + 1, dtype=np.uint64)
        rc = nat.lib().vs_fastq_gather(self._h, first, count, off.ctypes.data, None)
        if rc != nat.VS_OK:
            self._raise(None, rc)
        data = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        rc = nat.lib().vs_fastq_gather(self._h, first, count, off.ctypes.data, data.ctypes.data)
        if rc != nat.VS_OK:
            self._raise(None, rc)
        return data, off

    def block(self, first: int, count: int) -> "ReadBlock":
        h = C.c_void_p()
        rc = nat.lib().vs_fastq_block(self._ctx._h, self._h, first, count, C.byref(h))
        if rc != nat.VS_OK:
            self._raise(self._ctx._h, rc)  # ValueError for sequence bytes that are not valid UTF-8
        return ReadBlock(self._ctx, h)


class _NativeStream:
    """What the streamed ingests share: a native handle opened, read block by block and closed through the three entries
    ``_entries`` names (open, next, close).  ``_count`` names the attribute with the block size; a return code of next in
    ``_value_codes`` is an input the stream refuses (``ValueError``), as bytes that are not valid UTF-8 always are."""

    _entries = (None, None, None)
    _count = "block_pairs"
    _value_codes = ()

    @staticmethod
    def _open_error(ctx, rc, value_codes=()):
        msg = nat.lib().vs_last_error(ctx._h).decode("utf-8", "replace")
        return FileNotFoundError(msg) if "cannot open" in msg else ValueError(msg) if rc in value_codes else nat.NativeError(rc, msg)

    def _open(self, ctx, *args, value_codes=()):
        self._ctx, self._h = ctx, None
        h = C.c_void_p()
        rc = getattr(nat.lib(), self._entries[0])(ctx._h, *args, C.byref(h))
        if rc != nat.VS_OK:
            raise self._open_error(ctx, rc, value_codes)
        self._h = h

    def next_block(self) -> Optional["ReadBlock"]:
        """The next block, or None at the end of the input."""
        h = C.c_void_p()
        n = C.c_uint64(0)
        rc = getattr(nat.lib(), self._entries[1])(self._ctx._h, self._h, getattr(self, self._count), C.byref(h), C.byref(n))
        if rc in self._value_codes:
            raise ValueError(nat.lib().vs_last_error(self._ctx._h).decode("utf-8", "replace"))
        if rc != nat.VS_OK:
            FastqPair._raise(self._ctx._h, rc)  # ValueError for bytes that are not valid UTF-8
        return ReadBlock(self._ctx, h) if n.value else None

    def __iter__(self):
        while True:
            block = self.next_block()
            if block is None:
                return
            yield block

    def close(self):
        if self._h:
            getattr(nat.lib(), self._entries[2])(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastqStream(_NativeStream):
    """Both FASTQ files read front to back through the library's streamed ingest (``vs_fastq_stream_*``): any file a
    process can read once -- a FIFO, ``/dev/stdin``, ``<(zcat R1.fq.gz)``, a regular or gzip file -- with host memory
    bounded by a ring of pinned chunks; the records are found and packed on the device, and the members of a BGZF file
    (bgzip, htslib) are inflated there too (``info["members_device"]`` / ``["members_host"]`` per file say where; other
    gzip members go through zlib in the reader thread, ``VS_BGZF_DEVICE=0`` sends all of them there; with
    ``VS_GZIP_DEVICE=1`` a plain gzip file -- one deflate stream, no member directory -- is decoded on the device too, in
    parallel from speculative block starts: ``info["gzip_device"]`` per file says in how many windows, chain runs, dropped
    runs and members, and such members count in neither of the other two).  Iterating yields ``ReadBlock``s
    of at most ``block_pairs`` pairs until the input is exhausted; the checks of the whole input (bytes that are not valid
    UTF-8 anywhere, a cut-off gzip stream) raise before the iteration ends, with the exceptions ``FastqPair`` raises.
    ``close()`` as ``FastqPair``."""

    _entries = ("vs_fastq_stream_open", "vs_fastq_stream_next", "vs_fastq_stream_close")

    def __init__(self, fwd: str, rve: str, ctx: "Context", block_pairs: int = 1 << 20):
        self.block_pairs = block_pairs
        self._open(ctx, fwd.encode(), rve.encode())

    # ---- the member-sharded open of a BGZF pair (one process per GPU) ------------------------------------------------------
    @classmethod
    def open_shard(cls, fwd: str, rve: str, ctx: "Context", rank: int, world: int, all_gather=None, block_pairs: int = 1 << 20):
        """This rank's contiguous block of the pairs of two whole-BGZF files, shared with the other ranks by MEMBER and
        inflated on the devices only: pass 1 (``shard_count``) walks the member headers of both files and counts, on the
        device, the lines of this rank's share of the members; one exchange (``all_gather``: a callable that takes this
        rank's list of integers and returns every rank's, rank order -- the lists may differ in length; default
        ``torch.distributed.all_gather_object``); pass 2 (``shard_open``) opens the stream on the member range of this
        rank's records and exchanges one more integer, the status of that open.  A rank inflates its share twice -- the
        text of pass 1 is not kept, which is what keeps its device memory independent of the file.

        Returns ``(stream, None)``, or ``(None, reason)`` when the ranks -- all of them, the decision is a function of the
        gathered values alone -- must take ``FastqPair.open_shard`` instead: a file that is not whole BGZF, or a ``\\r`` or a
        byte >= 0x80 anywhere (universal newlines and the UTF-8 check of the whole file are the host ingest's).  The
        stream has ``first`` / ``total_pairs`` / ``shard_pairs`` (where its block lies), ``members`` (per file),
        ``members_pass1`` and ``plan`` (per file: first member, lines skipped, one past the last member)."""
        if all_gather is None:
            import torch.distributed as dist

            def all_gather(vals):
                got = [None] * world
                dist.all_gather_object(got, [int(v) for v in vals])
                return got

        mine = cls.shard_count(fwd, rve, ctx, rank, world)
        everyone = all_gather(mine.message)
        return cls.shard_open(mine, everyone, all_gather, block_pairs)

    class ShardCount:
        """What pass 1 leaves on a rank: ``message`` for the exchange, its own failure (raised after the exchange), the
        members' file offsets of both walks, how many members it inflated per file."""

        def __init__(self, fwd, rve, ctx, rank, world):
            self.paths, self.ctx, self.rank, self.world = (fwd, rve), ctx, rank, world
            self.failure, self.offsets, self.states, self.members_pass1 = None, [None, None], [2, 2], [0, 0]
            self.message = [1]

    @classmethod
    def shard_count(cls, fwd: str, rve: str, ctx: "Context", rank: int, world: int) -> "FastqStream.ShardCount":
        """Pass 1 on this rank.  ``message`` = [failed] + per file [whole BGZF, members M, flags of my share (1: a
        ``\\r``, 2: a byte >= 0x80), last byte of the last non-empty member of my share (256: none), members in my share,
        their newline counts padded with zeros to ceil(M / world)].  No share is counted when either file is not whole
        BGZF (every rank sees that in its own walk, and says so in the message)."""
        L = nat.lib()
        sc = cls.ShardCount(fwd, rve, ctx, rank, world)
        try:
            for i, path in enumerate(sc.paths):
                sc.offsets[i], sc.states[i], _ = bgzf_walk_file(path)
            whole = all(st == 0 for st in sc.states)
            msg = [0]
            for i, path in enumerate(sc.paths):
                m = len(sc.offsets[i]) - 1
                lo, hi = (m * rank) // world, (m * (rank + 1)) // world
                counts = np.zeros(max(hi - lo, 1), dtype=np.uint32)
                info = (C.c_uint64 * 4)(0, 256, 0, 0)
                if whole and hi > lo:
                    off = np.ascontiguousarray(sc.offsets[i][lo:hi + 1])
                    rc = L.vs_bgzf_count_lines(ctx._h, path.encode(), off.ctypes.data, hi - lo, counts.ctypes.data, info)
                    if rc != nat.VS_OK:
                        FastqPair._raise(ctx._h, rc)
                    sc.members_pass1[i] = int(info[2])
                share = [int(x) for x in counts[: hi - lo]] if whole else []
                msg += [1 if sc.states[i] == 0 else 0, m, int(info[0]), int(info[1]), len(share)]
                msg += share + [0] * (-(-m // world) - len(share))
            sc.message = msg
        except Exception as e:  # noqa: BLE001 (the peers hear of it through the message, then this rank raises it)
            sc.failure = e
            sc.message = [1]
        return sc

    @classmethod
    def shard_open(cls, mine: "FastqStream.ShardCount", everyone, all_gather, block_pairs: int = 1 << 20):
        """Pass 2 on this rank from every rank's pass-1 message; see ``open_shard`` for what comes back."""
        from .dist import shard_range

        rank, world, ctx = mine.rank, mine.world, mine.ctx
        if mine.failure is not None:
            raise mine.failure
        failed = [r for r, vals in enumerate(everyone) if vals[0]]
        if failed:
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        # every rank's shares, file by file (all that follows is a function of `everyone`: no rank can take another branch)
        whole, members, flags, last_byte, counts = [], [], 0, [256, 256], [[], []]
        at = [1] * len(everyone)
        for i in range(2):
            heads = {(vals[at[r]], vals[at[r] + 1]) for r, vals in enumerate(everyone)}
            if len(heads) != 1:
                raise RuntimeError("the ranks do not see the same file %s: (whole BGZF, members) = %s" % (mine.paths[i], sorted(heads)))
            (w, m), = heads
            whole.append(bool(w))
            members.append(m)
            for r, vals in enumerate(everyone):
                fl, lb, n = vals[at[r] + 2: at[r] + 5]
                flags |= fl
                if lb != 256:
                    last_byte[i] = lb
                counts[i] += vals[at[r] + 5: at[r] + 5 + n]
                at[r] += 5 + -(-m // world)
        if not all(whole):
            return None, "not whole BGZF"
        if flags & 3:
            return None, "a carriage return or a byte >= 0x80"
        if [len(c) for c in counts] != members:
            raise RuntimeError("the ranks' shares do not add up to the members of %s / %s" % mine.paths)
        counts = [np.asarray(c, dtype=np.uint32) for c in counts]
        open_end = [lb not in (256, 10) for lb in last_byte]
        lines = [int(counts[i].sum(dtype=np.uint64)) + (1 if open_end[i] else 0) for i in range(2)]
        total = min(lines[0] // 4, lines[1] // 4)  # PE_Inference.py:154
        first, last = shard_range(total, rank, world)
        plan = [bgzf_shard_plan(counts[i], open_end[i], first, last) for i in range(2)]
        rng = (C.c_uint64 * 6)()
        for i, (a, skip, e) in enumerate(plan):
            rng[3 * i], rng[3 * i + 1], rng[3 * i + 2] = int(mine.offsets[i][a]), int(mine.offsets[i][e]), skip
        self = cls.__new__(cls)
        self._ctx, self._h, self.block_pairs = ctx, None, block_pairs
        h = C.c_void_p()
        rc = nat.lib().vs_fastq_stream_open_range(ctx._h, mine.paths[0].encode(), mine.paths[1].encode(), rng, last - first, C.byref(h))
        err = None if rc == nat.VS_OK else cls._open_error(ctx, rc)
        status = all_gather([0 if err is None else 1])
        if err is not None:
            raise err
        failed = [r for r, vals in enumerate(status) if vals[0]]
        if failed:
            nat.lib().vs_fastq_stream_close(h)
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        self._h = h
        self.first, self.total_pairs, self.shard_pairs, self.lines = first, total, last - first, tuple(lines)
        self.members, self.members_pass1, self.plan = tuple(members), tuple(mine.members_pass1), plan
        return self, None

    @property
    def info(self):
        a = (C.c_uint64 * 4)()
        nat.lib().vs_fastq_stream_info(self._h, a)
        m = (C.c_uint64 * 4)()
        nat.lib().vs_fastq_stream_inflate_info(self._h, m)
        g = (C.c_uint64 * 8)()
        nat.lib().vs_fastq_stream_gzip_info(self._h, g)
        gz = tuple(dict(windows=int(g[4 * f]), runs=int(g[4 * f + 1]), dropped=int(g[4 * f + 2]), members=int(g[4 * f + 3])) for f in (0, 1))
        return dict(pairs=int(a[0]), text_bytes=int(a[1]), file_bytes=int(a[2]), flags=int(a[3]),
                    members_device=(int(m[0]), int(m[2])), members_host=(int(m[1]), int(m[3])), gzip_device=gz)

    @property
    def n_pairs(self) -> int:
        """pairs delivered so far (all of them once the iteration has ended)"""
        return self.info["pairs"]


class InterleavedStream(_NativeStream):
    """The read pairs of ONE interleaved FASTQ -- a file or pipe in which each pair's two records follow each other
    (``samtools fastq x.bam`` to stdout, ``seqtk mergepe``, ``fastp --stdout``; what ``bwa mem -p`` reads) -- through
    ``vs_fastq_il_*``: read front to back like ``FastqStream`` reads two files, in every form that stream reads, the mates
    found by NAME on the device.  Two adjacent records are a pair when their name tokens (the header line up to the first
    space or tab; a ``/1`` on the first and ``/2`` on the second dropped) are non-empty and equal byte for byte, greedily
    from the front as ``bwa mem -p`` pairs; any other record is a single.  The stream stands for the two files (first
    records of the pairs, second records of the pairs).  ``singles=False`` (strict): the first single raises ``ValueError``
    naming the path, the record (numbered from 0 in file order) and both header lines; ``singles=True``: singles are dropped
    and counted; ``singles="keep"``: classified alike, but the singles are KEPT -- when the pairs of a window are out its
    single records follow as singles blocks (``ReadBlock.unpaired``), which a ``PeCounter`` counts as unpaired reads.
    Interface of ``FastqStream``; ``info`` has ``pairs``, ``singles``, ``records``, ``text_bytes``, ``file_bytes``,
    ``flags``."""

    _entries = ("vs_fastq_il_open", "vs_fastq_il_next", "vs_fastq_il_close")
    _value_codes = (nat.VS_E_ARG,)  # (a single record in the strict mode; a stream that is no complete gzip)

    def __init__(self, path: str, ctx: "Context", block_pairs: int = 1 << 20, singles=False):
        self._h = None
        self.block_pairs = block_pairs
        if isinstance(singles, str) and singles != "keep":
            raise ValueError('singles is False, True or "keep" (got %r)' % (singles,))
        self.keep = singles == "keep"
        self.singles = bool(singles)
        self._open(ctx, os.fspath(path).encode(), 2 if self.keep else 1 if singles else 0)

    # ---- the member-sharded open of one whole-BGZF interleaved file (one process per GPU) -----------------------------------
    TAIL_RECORDS = 64  # the records at the end of a share whose mates the tail pass looks at first
    FN_CONST0, FN_FLIP, FN_ID, FN_CONST1 = 0, 1, 2, 3  # a function of one bit: f(0) | f(1) << 1 (vs_mates_core.h)

    @classmethod
    def open_shard(cls, path: str, ctx: "Context", rank: int, world: int, all_gather=None, block_pairs: int = 1 << 20, singles=False):
        """This rank's share of ONE whole-BGZF interleaved file, shared with the other ranks by MEMBER.  The T complete records
        are cut as ``dist.shard_range`` cuts pairs; rank r owns the records [a_r, b_r), every pair whose FIRST record it owns
        and every single it owns.  Whether a_r is the second record of a pair -- its entry parity -- is exact: pass 1
        (``shard_count``) counts lines per member as ``FastqStream.shard_count`` does for one file; pass 2 (``shard_tail``)
        composes, on the device, the parity function of the share from its tail (``vs_fastq_il_range_fn``); pass 3
        (``shard_open``) chains the functions into every rank's entry (``vs_il_shard_plan``), opens the stream on the member
        range of the share plus one look-ahead record (``vs_fastq_il_open_range``) and exchanges the status of that open.
        Three exchanges through ``all_gather`` (as ``FastqStream.open_shard`` takes it), the same on every rank whatever
        the data.  ``singles``: False (strict) or True; keep mode is not shared.

        Returns ``(stream, None)``, or ``(None, reason)`` when the ranks -- all of them, from gathered values alone -- must
        leave the file to one process: "not whole BGZF", "VS_BGZF_DEVICE=0", "a carriage return or a byte >= 0x80".  The
        stream has ``first_record`` / ``records`` / ``total_records`` (where its share lies), ``entry``, ``members``,
        ``members_pass1``, ``members_tail`` and ``plan`` (first member, lines skipped, one past the last member)."""
        if all_gather is None:
            import torch.distributed as dist

            def all_gather(vals):
                got = [None] * world
                dist.all_gather_object(got, [int(v) for v in vals])
                return got

        mine = cls.shard_count(path, ctx, rank, world)
        why = cls.shard_tail(mine, all_gather(mine.message))
        if why is not None:
            return None, why
        return cls.shard_open(mine, all_gather(mine.tail_message), all_gather, block_pairs, singles)

    class ShardCount:
        """What the passes leave on a rank: ``message`` / ``tail_message`` for the exchanges, its own failure (raised after
        the exchange that tells the peers), the members' file offsets, the members inflated per pass, and from ``shard_tail``
        on the line counts of every member, T and the rank's records."""

        def __init__(self, path, ctx, rank, world):
            self.path, self.ctx, self.rank, self.world = path, ctx, rank, world
            self.failure, self.offsets, self.state, self.members_pass1, self.members_tail = None, None, 2, 0, 0
            self.message, self.tail_message = [1], [1, InterleavedStream.FN_ID]

    @classmethod
    def shard_count(cls, path: str, ctx: "Context", rank: int, world: int) -> "InterleavedStream.ShardCount":
        """Pass 1 on this rank.  ``message`` = [failed, whole BGZF, members M, flags of my share (1: a ``\\r``, 2: a byte >=
        0x80; 4: ``VS_BGZF_DEVICE=0``, nothing was counted), last byte of the last non-empty member of my share (256: none),
        members in my share, their newline counts padded with zeros to ceil(M / world)]."""
        path = os.fspath(path)
        sc = cls.ShardCount(path, ctx, rank, world)
        try:
            sc.offsets, sc.state, _ = bgzf_walk_file(path)
            host_zlib = os.environ.get("VS_BGZF_DEVICE") == "0"
            m = len(sc.offsets) - 1
            lo, hi = (m * rank) // world, (m * (rank + 1)) // world
            counts, flags, last = [], 4 if host_zlib else 0, 256
            if sc.state == 0 and not host_zlib and hi > lo:
                counts, flags, last, sc.members_pass1, _ = bgzf_count_lines(path, sc.offsets[lo:hi + 1], ctx)
            share = [int(x) for x in counts]
            sc.message = [0, 1 if sc.state == 0 else 0, m, flags, last, len(share)] + share + [0] * (-(-m // world) - len(share))
        except Exception as e:  # noqa: BLE001 (the peers hear of it through the message, then this rank raises it)
            sc.failure = e
            sc.message = [1]
        return sc

    @classmethod
    def shard_tail(cls, mine: "InterleavedStream.ShardCount", everyone):
        """Pass 2 on this rank from every rank's pass-1 message: the reason when the ranks leave the file to one process,
        else None with ``mine.tail_message`` = [failed, the parity function of my share].  A rank in front of the last one with
        a share of its own composes the m of its last ``TAIL_RECORDS`` records (the look-ahead record behind them lends its
        header line); a constant function is the share's whatever lies in front, identity or flip says that every record
        of the window is its successor's mate, and the window is widened 16-fold until it is constant or holds the share."""
        from .dist import shard_range

        rank, world, ctx = mine.rank, mine.world, mine.ctx
        if mine.failure is not None:
            raise mine.failure
        failed = [r for r, vals in enumerate(everyone) if vals[0]]
        if failed:
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        # (all that follows up to the tail pass is a function of `everyone`: no rank can take another branch)
        heads = {(vals[1], vals[2]) for vals in everyone}
        if len(heads) != 1:
            raise RuntimeError("the ranks do not see the same file %s: (whole BGZF, members) = %s" % (mine.path, sorted(heads)))
        (whole, members), = heads
        flags, last_byte, counts = 0, 256, []
        for vals in everyone:
            flags |= vals[3]
            if vals[4] != 256:
                last_byte = vals[4]
            counts += vals[6: 6 + vals[5]]
        if not whole:
            return "not whole BGZF"
        if flags & 4:
            return "VS_BGZF_DEVICE=0"
        if flags & 3:
            return "a carriage return or a byte >= 0x80"
        if len(counts) != members:
            raise RuntimeError("the ranks' shares do not add up to the members of %s" % mine.path)
        mine.counts = np.asarray(counts, dtype=np.uint32)
        mine.open_end = last_byte not in (256, 10)
        mine.members = members
        mine.total = (int(mine.counts.sum(dtype=np.uint64)) + (1 if mine.open_end else 0)) // 4
        a, b = mine.span = shard_range(mine.total, rank, world)
        fn = cls.FN_ID  # (the last rank, an empty share, a share that ends with the file: nobody's entry follows from it)
        try:
            reach = cls.TAIL_RECORDS
            while rank < world - 1 and a < b < mine.total:
                lo = max(a, b - reach)
                fn, info = cls._range_fn(mine, lo, b + 1)
                mine.members_tail += info[0]
                if fn in (cls.FN_CONST0, cls.FN_CONST1) or lo == a:
                    break
                reach *= 16
            mine.tail_message = [0, fn]
        except Exception as e:  # noqa: BLE001 (as in pass 1)
            mine.failure = e
            mine.tail_message = [1, cls.FN_ID]
        return None

    @staticmethod
    def _range_fn(mine, first: int, last: int):
        """``vs_fastq_il_range_fn`` on the members that hold the records [first, last): (the composition of m[first .. last -
        2], (members inflated, file bytes read, windows, records seen))."""
        a, skip, e = bgzf_shard_plan(mine.counts, mine.open_end, first, last)
        return il_range_fn(mine.path, (mine.offsets[a], mine.offsets[e]), skip, last - first, mine.ctx)

    @classmethod
    def shard_open(cls, mine: "InterleavedStream.ShardCount", everyone, all_gather, block_pairs: int = 1 << 20, singles=False):
        """Pass 3 on this rank from every rank's tail message; see ``open_shard`` for what comes back."""
        rank, world, ctx = mine.rank, mine.world, mine.ctx
        if singles not in (False, True):
            raise ValueError("a shared interleaved file drops its single records (True) or refuses them (False); singles=%r is one "
                             "process's" % (singles,))
        if mine.failure is not None:
            raise mine.failure
        failed = [r for r, vals in enumerate(everyone) if vals[0]]
        if failed:
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        entries = il_shard_plan([vals[1] for vals in everyone])
        (a, b), entry = mine.span, entries[rank]
        lookahead = 1 if b < mine.total else 0
        plan = (0, 0, 0)
        if b - a > entry:  # (else nothing of the share is this rank's to decide: nothing is read)
            plan = bgzf_shard_plan(mine.counts, mine.open_end, a, min(b + 1, mine.total))
        rng = (C.c_uint64 * 3)(int(mine.offsets[plan[0]]), int(mine.offsets[plan[2]]), plan[1])
        self = cls.__new__(cls)
        self._ctx, self._h, self.block_pairs, self.keep, self.singles = ctx, None, block_pairs, False, bool(singles)
        h = C.c_void_p()
        rc = nat.lib().vs_fastq_il_open_range(ctx._h, mine.path.encode(), 1 if singles else 0, rng, b - a, lookahead, entry, a, C.byref(h))
        err = None if rc == nat.VS_OK else cls._open_error(ctx, rc)
        status = all_gather([0 if err is None else 1])
        if err is not None:
            raise err
        failed = [r for r, vals in enumerate(status) if vals[0]]
        if failed:
            nat.lib().vs_fastq_il_close(h)
            raise RuntimeError("FASTQ open failed on rank(s) %s" % failed)
        self._h = h
        self.first_record, self.records, self.total_records, self.entry = a, b - a, mine.total, entry
        self.members, self.members_pass1, self.members_tail, self.plan = mine.members, mine.members_pass1, mine.members_tail, plan
        return self, None

    @property
    def info(self):
        a = (C.c_uint64 * 6)()
        nat.lib().vs_fastq_il_info(self._h, a)
        return dict(pairs=int(a[0]), singles=int(a[1]), records=int(a[2]), text_bytes=int(a[3]), file_bytes=int(a[4]), flags=int(a[5]))

    @property
    def n_pairs(self) -> int:
        """pairs delivered so far (all of them once the iteration has ended)"""
        return self.info["pairs"]


class SingleEndStream(_NativeStream):
    """The UNPAIRED reads of one FASTQ file or pipe -- the unpaired survivors of a trimmer, the merged reads of an overlapping
    library -- through ``vs_fastq_se_*``: read front to back like ``InterleavedStream`` reads its file, in every form that
    stream reads, every complete record one read.  The blocks are singles blocks (``ReadBlock.unpaired``) of up to
    ``block_reads`` reads, built on the device.  ``info`` has ``reads``, ``records``, ``text_bytes``, ``file_bytes``,
    ``flags``."""

    _entries = ("vs_fastq_se_open", "vs_fastq_se_next", "vs_fastq_se_close")
    _count = "block_reads"
    _value_codes = (nat.VS_E_ARG,)  # (a stream that is no complete gzip)

    def __init__(self, path: str, ctx: "Context", block_reads: int = 1 << 20):
        self.block_reads = block_reads
        self._open(ctx, os.fspath(path).encode())

    @property
    def info(self):
        a = (C.c_uint64 * 6)()
        nat.lib().vs_fastq_se_info(self._h, a)
        return dict(reads=int(a[0]), records=int(a[1]), text_bytes=int(a[2]), file_bytes=int(a[3]), flags=int(a[4]))

    @property
    def n_reads(self) -> int:
        """reads delivered so far (all of them once the iteration has ended)"""
        return self.info["reads"]


def fastq_mates(text: bytes, eof: bool = True, ctx: "Context" = None, guard: int = 64):
    """The mates of ONE window of interleaved FASTQ text, bytes as they are (test aid): ``vs_fastq_mates_host`` (one host
    thread), or with ``ctx`` the kernels (``vs_fastq_mates_text``, ``guard`` sentinel words around the device pair list).
    ``eof``: the file ends with the window; otherwise its last complete record is held back unless it is the second of a
    pair.  Returns (pairs uint32 [n, 2]: record index of the first and the second; info dict: ``pairs``, ``singles``,
    ``decided``, ``held`` and ``first_single`` = a record index or None, ``records``)."""
    buf = np.frombuffer(text or b"\0", dtype=np.uint8)
    cap = len(text) // 8 + 1
    pairs = np.zeros((cap, 2), dtype=np.uint32)
    info = (C.c_uint64 * 6)()
    if ctx is None:
        rc = nat.lib().vs_fastq_mates_host(buf.ctypes.data, len(text), 1 if eof else 0, pairs.ctypes.data, cap, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_fastq_mates_text(ctx._h, buf.ctypes.data, len(text), 1 if eof else 0, pairs.ctypes.data, cap, guard, info))
    none = (1 << 64) - 1
    return pairs[:int(info[0])], dict(pairs=int(info[0]), singles=int(info[1]), decided=int(info[2]), held=None if info[3] == none else int(info[3]),
                                      first_single=None if info[4] == none else int(info[4]), records=int(info[5]))


class PairedNameStream(_NativeStream):
    """The read pairs of TWO FASTQ files paired by read NAME on the device, through ``vs_fastq_pn_*``: the two files of
    ``FastqStream``, read front to back in every form that stream reads, but a pair is a pair of mates by name (the rule of
    ``InterleavedStream``: name tokens equal byte for byte, a ``/1`` on the file-1 record and ``/2`` on the file-2 record
    dropped).  ``singles=False`` (strict): pair p is record p of either file; the first that is no pair of mates, or a
    complete record left over in the longer file, raises ``ValueError`` naming both paths, the pair (numbered from 0 in file
    order) and both header lines.  ``singles=True``: the files are in the same order but either may lack records the other
    has (trimmed or filtered separately); mates are found by a hash join on the names, records without a mate are dropped and
    counted per file, and the result is that of the two files filtered to their shared names, whatever the chunk size.  A name
    twice in one file's window, mates out of order inside a pair of windows, and a window beyond ``VS_PAIR_WINDOW`` bytes
    without a decision raise ``ValueError``.  ``singles="keep"``: joined alike, but the records without a mate are KEPT: when
    the pairs of a round are out, its decided records that are in no pair come as singles blocks (``ReadBlock.unpaired``) of
    up to ``block_pairs`` reads, file 1's first, then file 2's, each in file order.  Interface of ``FastqStream``; ``info``
    has ``pairs``, ``singles_fwd``, ``singles_rve`` (dropped, or kept), ``records_fwd``, ``records_rve``, ``windows``,
    ``max_window_bytes``, ``text_bytes``, ``file_bytes``, ``flags``."""

    _entries = ("vs_fastq_pn_open", "vs_fastq_pn_next", "vs_fastq_pn_close")
    _value_codes = (nat.VS_E_ARG, nat.VS_E_RANGE)  # (names that do not pair, a name twice, mates out of order, a window without a decision)

    def __init__(self, fwd: str, rve: str, ctx: "Context", block_pairs: int = 1 << 20, singles=False):
        self._h = None
        self.block_pairs = block_pairs
        if isinstance(singles, str) and singles != "keep":
            raise ValueError('singles is False, True or "keep" (got %r)' % (singles,))
        self.keep = singles == "keep"
        self.singles = bool(singles)
        self._open(ctx, os.fspath(fwd).encode(), os.fspath(rve).encode(), 2 if self.keep else 1 if singles else 0)

    @property
    def info(self):
        a = (C.c_uint64 * 10)()
        nat.lib().vs_fastq_pn_info(self._h, a)
        return dict(pairs=int(a[0]), singles_fwd=int(a[1]), singles_rve=int(a[2]), records_fwd=int(a[3]), records_rve=int(a[4]), windows=int(a[5]),
                    max_window_bytes=int(a[6]), text_bytes=int(a[7]), file_bytes=int(a[8]), flags=int(a[9]))

    @property
    def n_pairs(self) -> int:
        """pairs delivered so far (all of them once the iteration has ended)"""
        return self.info["pairs"]


def fastq_join(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True, ctx: "Context" = None, singles: bool = True, table: int = 0,
               name_bits: int = 0, guard: int = 64):
    """The join by name of ONE pair of FASTQ windows, bytes as they are (test aid): ``vs_fastq_join_host`` (one host thread),
    or with ``ctx`` the kernels (``vs_fastq_join_text``, ``guard`` sentinel words around the device pair list).  ``eof0`` /
    ``eof1``: the file ends with its window.  ``table``: slots of the open-address table (0: the stream's choice);
    ``name_bits``: low bits of the name hash kept (0: all).  Returns (pairs uint32 [n, 2]: record of window 1, record of
    window 2; info dict: ``pairs``, ``records`` and ``decided`` (a pair of counts each), ``duplicate`` = (file, record) or
    None, ``order`` = the first pair out of order or None, ``first_bad`` = strict: the first pair that is no pair of mates,
    or None)."""
    b0, b1 = (np.frombuffer(t or b"\0", dtype=np.uint8) for t in (text0, text1))
    cap = min(len(text0), len(text1)) // 8 + 1
    pairs = np.zeros((cap, 2), dtype=np.uint32)
    info = (C.c_uint64 * 8)()
    args = (b0.ctypes.data, len(text0), b1.ctypes.data, len(text1), 1 if eof0 else 0, 1 if eof1 else 0, 1 if singles else 0, table, name_bits, pairs.ctypes.data, cap)
    if ctx is None:
        rc = nat.lib().vs_fastq_join_host(*args, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_fastq_join_text(ctx._h, *args, guard, info))
    none = (1 << 64) - 1
    opt = lambda v: None if v == none else int(v)
    return pairs[:int(info[0])], dict(pairs=int(info[0]), records=(int(info[1]), int(info[2])), decided=(int(info[3]), int(info[4])),
                                      duplicate=None if info[5] == none else (int(info[5] >> 32), int(info[5] & 0xFFFFFFFF)), order=opt(info[6]),
                                      first_bad=opt(info[7]))


def fastq_join_singles(text0: bytes, text1: bytes, eof0: bool = True, eof1: bool = True, ctx: "Context" = None, table: int = 0, name_bits: int = 0,
                       guard: int = 64):
    """``fastq_join`` (``singles=True``) and the KEPT singles of the round as well (test aid): ``vs_fastq_join_singles_host``, or
    with ``ctx`` the kernels (``vs_fastq_join_singles_text``, ``guard`` sentinel words around both device lists).  Returns
    (pairs, singles of window 1, singles of window 2 -- uint32 record indices in order: the decided records in no pair --,
    info as ``fastq_join`` gives it)."""
    b0, b1 = (np.frombuffer(t or b"\0", dtype=np.uint8) for t in (text0, text1))
    cap = min(len(text0), len(text1)) // 8 + 1
    caps = (len(text0) // 4 + 1, len(text1) // 4 + 1)
    pairs = np.zeros((cap, 2), dtype=np.uint32)
    lists = [np.zeros(c, dtype=np.uint32) for c in caps]
    info = (C.c_uint64 * 10)()
    args = (b0.ctypes.data, len(text0), b1.ctypes.data, len(text1), 1 if eof0 else 0, 1 if eof1 else 0, 2, table, name_bits, pairs.ctypes.data, cap,
            lists[0].ctypes.data, caps[0], lists[1].ctypes.data, caps[1])
    if ctx is None:
        rc = nat.lib().vs_fastq_join_singles_host(*args, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_fastq_join_singles_text(ctx._h, *args, guard, info))
    none = (1 << 64) - 1
    opt = lambda v: None if v == none else int(v)
    return (pairs[:int(info[0])], lists[0][:int(info[8])], lists[1][:int(info[9])],
            dict(pairs=int(info[0]), records=(int(info[1]), int(info[2])), decided=(int(info[3]), int(info[4])),
                 duplicate=None if info[5] == none else (int(info[5] >> 32), int(info[5] & 0xFFFFFFFF)), order=opt(info[6]), first_bad=opt(info[7])))


class BamStream(_NativeStream):
    """The read pairs of ONE collated BAM file (unaligned BAM from the sequencer, or the unmapped pairs of a host
    alignment after ``samtools collate``) through ``vs_bam_stream_*``: the BGZF members inflated on the device, the records
    found there by following their ``block_size`` chain from the end of the header, the 4-bit bases packed by the packer of
    every block.  The file stands for the FASTQ pair ``samtools fastq -1 -2`` writes: secondary and supplementary records
    are dropped, so is every record that is not paired with exactly one of first / second; the rest are taken two at a
    time, one first (the forward end) and one second in either order, an end with flag 0x10 reversed and complemented.
    Anything else -- two firsts in a row, an odd record at the end, a truncated or malformed record -- raises
    ``ValueError`` naming the record (numbered from 0 in file order).  Interface of ``FastqStream``; ``info`` has
    ``pairs``, ``records``, ``dropped_0x900``, ``dropped_other``, ``members_device``, ``text_bytes``, ``file_bytes``.

    ``by_name=True``: the records may lie in any order (a coordinate-sorted alignment, ``samtools view -f 12`` of one, a
    file that lost one mate of some pairs).  The mates are matched on the device by their names, byte for byte: the j-th
    first of a name pairs with its j-th second, pairs come in the order of the record that completed them, and a record
    whose mate never comes is a singleton, dropped and counted -- the pair ``samtools collate | samtools fastq -1 -2 -s
    /dev/null -0 /dev/null`` writes, up to the order of the pairs.  ``info`` also has ``singletons``, ``waiting_max`` (most
    records carried from one window to the next), ``carried_bytes_max`` and ``windows``.  More than 64 records of one name
    and one end in a window, or waiting records beyond the largest window, raise ``ValueError`` advising ``samtools
    collate``.  ``by_name=True, singles="keep"``: matched alike, but the singletons are KEPT: at the end of the input they come
    in file order as singles blocks (``ReadBlock.unpaired``) of up to ``block_pairs`` reads, each read as ``samtools fastq
    -s`` writes it (reversed and complemented under 0x10; no bases: a read of length 0)."""

    _entries = ("vs_bam_stream_open_mode", "vs_bam_stream_next", "vs_bam_stream_close")

    @property
    def _value_codes(self):  # (by name: a file the match refuses)
        return (nat.VS_E_ARG, nat.VS_E_RANGE) if self.by_name else (nat.VS_E_ARG,)

    def __init__(self, path: str, ctx: "Context", block_pairs: int = 1 << 20, by_name: bool = False, singles=None):
        self._h = None
        self.block_pairs = block_pairs
        self.by_name = bool(by_name)
        if singles not in (None, "keep"):
            raise ValueError('singles is None or "keep" (got %r)' % (singles,))
        self.keep = singles == "keep"
        if self.keep and not by_name:
            raise ValueError('singles="keep" keeps the singletons of a BAM whose mates are matched by name and needs by_name=True: a collated BAM has none')
        self._open(ctx, path.encode(), 2 if self.keep else 1 if by_name else 0, value_codes=(nat.VS_E_ARG,))

    # ---- the member-sharded open of a collated BAM (one process per GPU) ---------------------------------------------------
    @classmethod
    def open_shard(cls, path: str, ctx: "Context", rank: int, world: int, all_gather=None, block_pairs: int = 1 << 20):
        """This rank's couples of ONE collated whole-BGZF BAM, shared with the other ranks by MEMBER and inflated on the
        devices only.  A member range cannot be entered at a guessed record start, so pass 1 (``shard_summary``) follows
        the record chain from EVERY candidate start of this rank's share on the device and keeps, per candidate, where the
        chain leaves the share and how many participating records it passed; one exchange (``all_gather`` as
        ``FastqStream.open_shard`` takes it, default ``torch.distributed.all_gather_object``; at most 2 * 12 288 entries a
        rank); ``bam_shard_plan`` chains the summaries into every rank's true entry, and pass 2 (``shard_open``) opens the
        stream on that range and exchanges one more integer, the status of that open.  A rank inflates its share twice.

        Returns ``(stream, None)``, or ``(None, reason)`` -- one of ``BAM_SHARD_REASONS``, the same on every rank, a
        function of the gathered values alone -- when rank 0 must read the whole file as the single process does.  The
        stream has ``first_pair`` / ``pairs`` (where its couples lie among the file's), ``members``, ``members_pass1`` and
        ``plan`` (bytes in front of its first record, where its ownership ends, participating records in front of its
        entry, the inflated offset of its share, participating records in front of the next rank's entry)."""
        if all_gather is None:
            import torch.distributed as dist

            def all_gather(vals):
                got = [None] * world
                dist.all_gather_object(got, [int(v) for v in vals])
                return got

        mine = cls.shard_summary(path, ctx, rank, world)
        everyone = all_gather(mine.message)
        return cls.shard_open(mine, everyone, all_gather, block_pairs)

    class ShardSummary:
        """What pass 1 leaves on a rank: ``message`` for the exchange, its own failure (raised after the exchange), the
        members' file offsets, how many members it inflated."""

        def __init__(self, path, ctx, rank, world):
            self.path, self.ctx, self.rank, self.world = path, ctx, rank, world
            self.failure, self.offsets, self.members_pass1 = None, None, 0
            self.message = [1, 0, 0, 0, 0, 0]

    @classmethod
    def shard_summary(cls, path: str, ctx: "Context", rank: int, world: int) -> "BamStream.ShardSummary":
        """Pass 1 on this rank.  ``message`` = [failed, whole BGZF, members M, header bytes H, my share's inflated size,
        candidates C, X[0 .. C), N[0 .. C)] (``vs_bam_share_summary``); no share is summarised when the file is not whole
        BGZF (every rank sees that in its own walk)."""
        sm = cls.ShardSummary(path, ctx, rank, world)
        try:
            sm.offsets, state, _ = bgzf_walk_file(path)
            m = len(sm.offsets) - 1
            header = bam_header_bytes(path)
            if state != 0:
                sm.message = [0, 0, m, header, 0, 0]
                return sm
            lo, hi = (m * rank) // world, (m * (rank + 1)) // world
            cap = 1 if rank == 0 else BAM_SEG_MAX
            x = np.zeros(cap, dtype=np.uint64)
            n = np.zeros(cap, dtype=np.uint64)
            info = (C.c_uint64 * 5)()
            off = np.ascontiguousarray(sm.offsets, dtype=np.uint64)
            rc = nat.lib().vs_bam_share_summary(ctx._h, path.encode(), off.ctypes.data, m, lo, hi, header if rank == 0 else (1 << 64) - 1, 0,
                                                x.ctypes.data, n.ctypes.data, cap, info)
            if rc != nat.VS_OK:
                msg = nat.lib().vs_last_error(ctx._h).decode("utf-8", "replace")
                raise ValueError(msg) if rc == nat.VS_E_ARG else nat.NativeError(rc, msg)
            c = int(info[0])
            sm.members_pass1 = int(info[2])
            sm.message = [0, 1, m, header, int(info[1]), c] + [int(v) for v in x[:c]] + [int(v) for v in n[:c]]
        except Exception as e:  # noqa: BLE001 (the peers hear of it through the message, then this rank raises it)
            sm.failure = e
            sm.message = [1, 0, 0, 0, 0, 0]
        return sm

    @classmethod
    def shard_open(cls, mine: "BamStream.ShardSummary", everyone, all_gather, block_pairs: int = 1 << 20):
        """Pass 2 on this rank from every rank's pass-1 message; see ``open_shard`` for what comes back."""
        rank, ctx = mine.rank, mine.ctx
        if mine.failure is not None:
            raise mine.failure
        failed = [r for r, vals in enumerate(everyone) if vals[0]]
        if failed:
            raise RuntimeError("BAM open failed on rank(s) %s" % failed)
        plan, reason = bam_shard_plan(everyone)  # (a function of `everyone`: no rank can take another branch)
        if reason is not None:
            return None, reason
        drop, own_end, before, start, after = plan[rank]
        rng = (C.c_uint64 * 5)(int(mine.offsets[(everyone[rank][2] * rank) // mine.world]), drop, (1 << 64) - 1 if own_end is None else own_end,
                               before & 1, start)
        self = cls.__new__(cls)
        self._ctx, self._h, self.block_pairs, self.by_name, self.keep = ctx, None, block_pairs, False, False
        h = C.c_void_p()
        rc = nat.lib().vs_bam_stream_open_range(ctx._h, mine.path.encode(), rng, C.byref(h))
        err = None if rc == nat.VS_OK else cls._open_error(ctx, rc)
        status = all_gather([0 if err is None else 1])
        if err is not None:
            raise err
        failed = [r for r, vals in enumerate(status) if vals[0]]
        if failed:
            nat.lib().vs_bam_stream_close(h)
            raise RuntimeError("BAM open failed on rank(s) %s" % failed)
        self._h = h
        self.first_pair, self.pairs = (before + 1) // 2, (after + 1) // 2 - (before + 1) // 2
        self.members, self.members_pass1, self.plan = everyone[rank][2], mine.members_pass1, plan[rank]
        return self, None

    @property
    def info(self):
        a = (C.c_uint64 * 8)()
        nat.lib().vs_bam_stream_info(self._h, a)
        m = (C.c_uint64 * 4)()
        nat.lib().vs_bam_stream_mate_info(self._h, m)
        return dict(pairs=int(a[0]), records=int(a[1]), dropped_0x900=int(a[2]), dropped_other=int(a[3]), members_device=int(a[4]),
                    text_bytes=int(a[5]), file_bytes=int(a[6]), done=bool(a[7]), singletons=int(m[0]), waiting_max=int(m[1]),
                    carried_bytes_max=int(m[2]), windows=int(m[3]))

    @property
    def n_pairs(self) -> int:
        """pairs delivered so far (all of them once the iteration has ended)"""
        return self.info["pairs"]


def bam_header_bytes(path: str) -> int:
    """Inflated bytes in front of the first record of the BAM at ``path`` (``vs_bam_header``, host only); ``ValueError``
    when the file is no BAM."""
    n = C.c_uint64(0)
    rc = nat.lib().vs_bam_header(path.encode(), C.byref(n))
    if rc != nat.VS_OK:
        raise ValueError(nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    return int(n.value)


BAM_SEG_MAX = 12288  # the largest segment of the chain passes, and so the most candidates of a share's summary
BAM_SUM_DEAD, BAM_SUM_CUT = (1 << 64) - 1, (1 << 64) - 2
# why the ranks of a sharded run leave a BAM to rank 0 (vs_bam_shard_plan's codes 3 ..; pe_inference adds "VS_BGZF_DEVICE=0")
BAM_SHARD_REASONS = {
    3: "not whole BGZF",
    4: "the header reaches beyond the share of rank 0",
    5: "a record longer than a segment across a share boundary, or a share without bytes",
    6: "a block_size below 32 on the chain",
    7: "the file ends inside a record",
    8: "the chain does not end at the end of the file",
    9: "an odd number of records that take part",
}


def bam_share_summary(share: bytes, share_size: int, start: Optional[int] = None, seg: int = 0, chunk: int = 0, ctx: "Context" = None):
    """The summary of a share from its inflated bytes (test aid): ``share[:share_size]`` is the share, what follows are the
    bytes behind it (64 at least, unless the file ends).  ``start``: the one candidate (rank 0: the header's size), None:
    every candidate below min(seg, share_size).  ``chunk``: new bytes per window (0: one window).  ``vs_bam_share_summary_host``
    (one host thread), or with ``ctx`` the kernels (``_text``).  Returns (X list, N list, windows)."""
    buf = np.frombuffer(share or b"\0", dtype=np.uint8)
    cap = 1 if start is not None else BAM_SEG_MAX
    x = np.zeros(cap, dtype=np.uint64)
    n = np.zeros(cap, dtype=np.uint64)
    info = (C.c_uint64 * 2)()
    st = (1 << 64) - 1 if start is None else start
    if ctx is None:
        rc = nat.lib().vs_bam_share_summary_host(buf.ctypes.data, len(share), share_size, st, seg, chunk, x.ctypes.data, n.ctypes.data, cap, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_bam_share_summary_text(ctx._h, buf.ctypes.data, len(share), share_size, st, seg, chunk, x.ctypes.data,
                                                             n.ctypes.data, cap, info))
    c = int(info[0])
    return [int(v) for v in x[:c]], [int(v) for v in n[:c]], int(info[1])


def bam_shard_plan(everyone):
    """``vs_bam_shard_plan`` (a pure function of the host) of every rank's pass-1 message [failed, whole BGZF, M, H, share
    size, C, X[C], N[C]]: (per rank (bytes in front of its first record, where its ownership ends relative to its share or
    None, participating records in front of its entry, inflated offset of its share, participating records in front of
    the next rank's entry), None) or (None, reason of ``BAM_SHARD_REASONS``).  ``RuntimeError`` when a rank failed or the
    ranks do not see the same file."""
    world = len(everyone)
    head = np.zeros(6 * world, dtype=np.uint64)
    xn, off = [], np.zeros(world, dtype=np.uint64)
    for r, vals in enumerate(everyone):
        head[6 * r: 6 * r + 6] = [int(v) for v in vals[:6]]
        c = int(vals[5])
        if len(vals) != 6 + 2 * c:
            raise RuntimeError("the message of rank %d has %d entries where its head says %d" % (r, len(vals), 6 + 2 * c))
        off[r] = len(xn)
        xn += [int(v) for v in vals[6:]]
    xn = np.asarray(xn + [0], dtype=np.uint64)
    plan = np.zeros(5 * world, dtype=np.uint64)
    reason = C.c_int(0)
    rc = nat.lib().vs_bam_shard_plan(world, head.ctypes.data, xn.ctypes.data, off.ctypes.data, plan.ctypes.data, C.byref(reason))
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    if reason.value == 1:
        raise RuntimeError("BAM open failed on rank(s) %s" % [r for r, vals in enumerate(everyone) if vals[0]])
    if reason.value == 2:
        raise RuntimeError("the ranks do not see the same BAM file: (whole BGZF, members, header bytes) = %s" % sorted({tuple(v[1:4]) for v in everyone}))
    if reason.value:
        return None, BAM_SHARD_REASONS[reason.value]
    none = (1 << 64) - 1
    return [(int(p[0]), None if int(p[1]) == none else int(p[1]), int(p[2]), int(p[3]), int(p[4])) for p in plan.reshape(world, 5)], None


def bam_scan(data: bytes, skip: int = 0, seg: int = 0, ctx: "Context" = None):
    """The record chain of inflated BAM bytes from ``skip`` (test aid): ``vs_bam_scan_host`` (one host thread), or with
    ``ctx`` the kernels (``vs_bam_scan_text``).  Returns (recs uint32 [n, 4]: offset, flag | class << 16, l_seq, sequence
    offset; ends uint32 [couples, 2]: record index of the forward and the reverse end; info dict)."""
    buf = np.frombuffer(data or b"\0", dtype=np.uint8)
    cap = len(data) // 36 + 1
    recs = np.zeros((cap, 4), dtype=np.uint32)
    ends = np.zeros(cap + 1, dtype=np.uint32)
    info = (C.c_uint64 * 6)()
    if ctx is None:
        rc = nat.lib().vs_bam_scan_host(buf.ctypes.data, len(data), skip, seg, recs.ctypes.data, cap, ends.ctypes.data, cap, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_bam_scan_text(ctx._h, buf.ctypes.data, len(data), skip, seg, recs.ctypes.data, cap, ends.ctypes.data,
                                                    cap, info))
    none = (1 << 64) - 1
    n_rec, n_part = int(info[0]), int(info[1])
    return recs[:n_rec], ends[:2 * (n_part // 2)].reshape(-1, 2), dict(
        records=n_rec, taking_part=n_part, end=int(info[2]), stop=int(info[3]),
        malformed=None if info[4] == none else int(info[4]), bad_couple=None if info[5] == none else int(info[5]))


def bam_mates(data: bytes, skip: int = 0, seg: int = 0, ctx: "Context" = None, hash_bits: int = 64):
    """The mates of ONE window of inflated BAM bytes matched by name (test aid): ``vs_bam_mates_host`` (one host thread),
    or with ``ctx`` the kernels (``vs_bam_mates_text``).  Returns (pairs uint32 [n, 2]: record index of the first and the
    second in delivery order; waiting uint32 [m]: the records left waiting, in file order; info dict: ``pairs``,
    ``waiting``, ``crowded`` = the newest record of a name with more than 64 records of one end, or None)."""
    buf = np.frombuffer(data or b"\0", dtype=np.uint8)
    cap = len(data) // 36 + 1
    pairs = np.zeros((cap, 2), dtype=np.uint32)
    waiting = np.zeros(cap, dtype=np.uint32)
    info = (C.c_uint64 * 3)()
    if ctx is None:
        rc = nat.lib().vs_bam_mates_host(buf.ctypes.data, len(data), skip, seg, hash_bits, pairs.ctypes.data, cap, waiting.ctypes.data, cap, info)
        if rc != nat.VS_OK:
            raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    else:
        nat.check(ctx._h, nat.lib().vs_bam_mates_text(ctx._h, buf.ctypes.data, len(data), skip, seg, hash_bits, pairs.ctypes.data, cap,
                                                     waiting.ctypes.data, cap, info))
    none = (1 << 64) - 1
    return pairs[:int(info[0])], waiting[:int(info[1])], dict(pairs=int(info[0]), waiting=int(info[1]),
                                                              crowded=None if info[2] == none else int(info[2]))


INFLATE_GUARD = 64  # bytes kept behind every member's output by the inflate test aids; they must stay INFLATE_GUARD_BYTE
INFLATE_GUARD_BYTE = 0xA5


def bgzf_walk(data: bytes):
    """The whole BGZF members at the front of ``data`` (``vs_bgzf_walk``, host only): (list of (payload offset, payload
    length, ISIZE, CRC32), offset of the first byte that is not part of one, what is there: 0 nothing, 1 "need more
    bytes", 2 "not BGZF")."""
    buf = np.frombuffer(data or b"\0", dtype=np.uint8)
    info = (C.c_uint64 * 3)()
    rc = nat.lib().vs_bgzf_walk(buf.ctypes.data, len(data), None, 0, info)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_bgzf_walk")
    mem = np.zeros((max(int(info[0]), 1), 4), dtype=np.uint64)
    nat.lib().vs_bgzf_walk(buf.ctypes.data, len(data), mem.ctypes.data, int(info[0]), info)
    return [tuple(int(x) for x in row) for row in mem[: int(info[0])]], int(info[1]), int(info[2])


def bgzf_walk_file(path: str):
    """The header hop over a regular file (``vs_bgzf_walk_file``, host only, no payload read): (the members' file offsets
    and one past the last as uint64[M + 1], what follows the last member: 0 nothing, 1 a cut-off member, 2 not BGZF, the
    file's size)."""
    info = (C.c_uint64 * 4)()
    cap = os.path.getsize(path) // 4096 + 1024 if os.path.isfile(path) else 1
    while True:
        off = np.zeros(cap + 1, dtype=np.uint64)
        rc = nat.lib().vs_bgzf_walk_file(path.encode(), off.ctypes.data, cap + 1, info)
        if rc != nat.VS_OK:
            msg = nat.lib().vs_last_error(None).decode("utf-8", "replace")
            raise FileNotFoundError(msg) if "cannot open" in msg else nat.NativeError(rc, msg)
        if int(info[0]) <= cap:
            return off[: int(info[0]) + 1].copy(), int(info[2]), int(info[3])
        cap = int(info[0])


def inflate_count_host(payload: bytes, isize: int, crc: int):
    """One raw deflate payload through the host form of the counting kernel (``vs_inflate_count_host``): (status word,
    newlines, flags -- 1: a ``\\r``, 2: a byte >= 0x80 --, last byte)."""
    src = np.frombuffer(payload or b"\0", dtype=np.uint8)
    res = (C.c_uint32 * 4)()
    rc = nat.lib().vs_inflate_count_host(src.ctypes.data, len(payload), isize, crc & 0xFFFFFFFF, res)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_inflate_count_host")
    return tuple(int(x) for x in res)


def bgzf_count_lines(path: str, offsets, ctx: "Context"):
    """The members at ``offsets`` (M + 1 file offsets) counted on the device (``vs_bgzf_count_lines``): (newlines per
    member, flags, last byte of the last non-empty member or 256, members inflated, file bytes read)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    counts = np.zeros(max(n, 1), dtype=np.uint32)
    info = (C.c_uint64 * 4)()
    rc = nat.lib().vs_bgzf_count_lines(ctx._h, path.encode(), off.ctypes.data, n, counts.ctypes.data, info)
    if rc != nat.VS_OK:
        FastqPair._raise(ctx._h, rc)
    return counts[:n], int(info[0]), int(info[1]), int(info[2]), int(info[3])


def bgzf_shard_plan(counts, no_final_newline: bool, first: int, last: int):
    """``vs_bgzf_shard_plan`` (a pure function of the host): for the records [first, last) of a file with these newline
    counts per member, (the first member to open, the lines to skip in front of it, one past the last member needed)."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    plan = (C.c_uint64 * 3)()
    rc = nat.lib().vs_bgzf_shard_plan(c.ctypes.data if c.size else None, c.size, 1 if no_final_newline else 0, first, last, plan)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    return int(plan[0]), int(plan[1]), int(plan[2])


def il_shard_plan(fns):
    """``vs_il_shard_plan`` (a pure function of the host): from the parity function of every rank's share of an interleaved
    file (two bits each: const-0 = 0, flip = 1, identity = 2, const-1 = 3), the parity with which every rank's first record
    starts: 0 for rank 0, ``fns[r]`` applied to rank r's for rank r + 1."""
    f = np.ascontiguousarray(fns, dtype=np.uint32)
    entry = np.zeros(max(f.size, 1), dtype=np.uint32)
    rc = nat.lib().vs_il_shard_plan(f.ctypes.data if f.size else None, f.size, entry.ctypes.data)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, nat.lib().vs_last_error(None).decode("utf-8", "replace"))
    return [int(x) for x in entry[: f.size]]


def il_range_fn(path: str, offsets, skip: int, n_rec: int, ctx: "Context"):
    """``vs_fastq_il_range_fn`` on the bytes [offsets[0], offsets[1]) of a BGZF file behind ``skip`` lines: (the composition of
    m[0 .. n_rec - 2], (members inflated, file bytes read, windows, records seen))."""
    rng = (C.c_uint64 * 3)(int(offsets[0]), int(offsets[1]), skip)
    fn, info = C.c_uint32(0), (C.c_uint64 * 4)()
    rc = nat.lib().vs_fastq_il_range_fn(ctx._h, os.fspath(path).encode(), rng, n_rec, C.byref(fn), info)
    if rc != nat.VS_OK:
        FastqPair._raise(ctx._h, rc)
    return int(fn.value), tuple(int(x) for x in info)


def inflate_host(payload: bytes, isize: int, crc: int):
    """One raw deflate payload through the host form of the device decoder (``vs_inflate_host``): (status word, the
    ``isize`` output bytes, whether the guard bytes behind them are untouched)."""
    src = np.frombuffer(payload or b"\0", dtype=np.uint8)
    out = np.full(isize + INFLATE_GUARD, INFLATE_GUARD_BYTE, dtype=np.uint8)
    status = C.c_uint32(0xFFFFFFFF)
    rc = nat.lib().vs_inflate_host(src.ctypes.data, len(payload), out.ctypes.data, isize, crc & 0xFFFFFFFF, C.byref(status))
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_inflate_host")
    return int(status.value), out[:isize].tobytes(), bool((out[isize:] == INFLATE_GUARD_BYTE).all())


def inflate_bgzf(data: bytes, ctx: "Context"):
    """Whole BGZF members through the device kernel (``vs_inflate_bgzf``): per member (status word, output bytes, whether
    the guard bytes behind its output are untouched)."""
    src = np.frombuffer(data or b"\0", dtype=np.uint8)
    info = (C.c_uint64 * 2)()
    nat.check(ctx._h, nat.lib().vs_inflate_bgzf(ctx._h, src.ctypes.data, len(data), None, 0, INFLATE_GUARD, None, 0, info))
    n, total = int(info[0]), int(info[1])
    out = np.zeros(max(total, 1), dtype=np.uint8)
    status = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    nat.check(ctx._h, nat.lib().vs_inflate_bgzf(ctx._h, src.ctypes.data, len(data), out.ctypes.data, total, INFLATE_GUARD,
                                                status.ctypes.data, n, info))
    members, _, _ = bgzf_walk(data)
    res, at = [], 0
    for i, (_, _, isize, _) in enumerate(members):
        guard = out[at + isize: at + isize + INFLATE_GUARD]
        res.append((int(status[i]), out[at: at + isize].tobytes(), bool((guard == INFLATE_GUARD_BYTE).all())))
        at += isize + INFLATE_GUARD
    return res


GZIP_INFO = ("candidates", "selected", "chain_runs", "dropped", "members", "status", "bad_run", "text", "recounted")


def gzip_inflate_host(data: bytes, gran: int = 0):
    """A whole plain gzip file through the one-lane host form of the parallel decoder (``vs_gzip_inflate_host``):
    (info as a dict of ``GZIP_INFO``, the text -- empty unless the status is 0).  ``gran``: compressed bytes per selected
    run start, 0 = every candidate."""
    src = np.frombuffer(data or b"\0", dtype=np.uint8)
    info = (C.c_uint64 * 9)()
    nat.check(None, nat.lib().vs_gzip_inflate_host(src.ctypes.data, len(data), gran, None, 0, info))
    out = np.zeros(max(int(info[7]), 1), dtype=np.uint8)
    nat.check(None, nat.lib().vs_gzip_inflate_host(src.ctypes.data, len(data), gran, out.ctypes.data, out.size, info))
    return dict(zip(GZIP_INFO, (int(x) for x in info))), out[:int(info[7])].tobytes()


def gzip_inflate(data: bytes, ctx: "Context", gran: int = 0):
    """The same through the kernels (``vs_gzip_inflate``): (info, text, whether the guard bytes behind the text are
    untouched)."""
    src = np.frombuffer(data or b"\0", dtype=np.uint8)
    info = (C.c_uint64 * 9)()
    nat.check(ctx._h, nat.lib().vs_gzip_inflate(ctx._h, src.ctypes.data, len(data), gran, None, 0, INFLATE_GUARD, info))
    n = int(info[7])
    out = np.full(n + INFLATE_GUARD, INFLATE_GUARD_BYTE, dtype=np.uint8)
    nat.check(ctx._h, nat.lib().vs_gzip_inflate(ctx._h, src.ctypes.data, len(data), gran, out.ctypes.data, out.size, INFLATE_GUARD, info))
    got = int(info[7])
    assert got <= n
    return dict(zip(GZIP_INFO, (int(x) for x in info))), out[:got].tobytes(), bool((out[n:] == INFLATE_GUARD_BYTE).all())


def encode_seqs(seqs: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    # one byte per CHARACTER (the reference works on decoded text): a character beyond latin-1 becomes '?', which like
    # any byte outside ACGT makes the windows over it miss
    data = np.frombuffer("".join(seqs).encode("latin-1", "replace"), dtype=np.uint8)
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(data), off


def node_order(seqs: Sequence[str], ksize: int, _encoded=None) -> np.ndarray:
    """Numbering of the nodes along the graph's paths (``vs_node_order_host``, csrc/vs_order_host.cpp):
    ``order[r]`` = position in ``seqs`` of the node that gets number r."""
    data, off = _encoded if _encoded is not None else encode_seqs(seqs)
    order = np.zeros(max(len(seqs), 1), dtype=np.uint32)
    rc = nat.lib().vs_node_order_host(data.ctypes.data, off.ctypes.data, len(seqs), ksize, order.ctypes.data)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_node_order_host")
    return order[: len(seqs)].astype(np.int64)


LIST_CAP = 20  # nodes a read end may list on the main path of a count (LCAP of the kernels)


def list_block(pairs, ept: int = 64) -> Tuple[np.ndarray, np.ndarray]:
    """``pairs`` (sequences of (left list, right list), node numbers in any order) as the arrays ``pe_count_lists``
    takes: uint32 [2 P, 20] and [2 P].  A tile of ``ept`` ends holds ``ept * 4`` quads of four nodes; where the next
    pair would not fit, the tile is closed with empty pairs (both counts 0) -- they are part of the block that comes
    back, so that every layout and every model see the same one."""
    ppt, cap_q = ept // 2, ept * 4
    rows, used_p, used_q = [], 0, 0
    for left, right in pairs:
        q = (len(left) + 3) // 4 + (len(right) + 3) // 4
        if used_p == ppt or used_q + q > cap_q:
            rows += [()] * (2 * (ppt - used_p) if used_p < ppt else 0)
            used_p = used_q = 0
        rows += [left, right]
        used_p += 1
        used_q += q
    lists = np.full((max(len(rows), 1), LIST_CAP), 0xFFFFFFFF, dtype=np.uint32)
    counts = np.zeros(max(len(rows), 1), dtype=np.uint32)
    for e, row in enumerate(rows):
        if len(row) > LIST_CAP:
            raise ValueError("end %d lists %d nodes, at most %d" % (e, len(row), LIST_CAP))
        counts[e] = len(row)
        lists[e, : len(row)] = row
    return lists[: len(rows)], counts[: len(rows)]


# ---- device objects ------------------------------------------------------------------------------
class ReadBlock:
    def __init__(self, ctx: "Context", handle):
        self._ctx = ctx
        self._h = handle

    @property
    def info(self):
        a = (C.c_uint64 * 5)()
        nat.check(self._ctx._h, nat.lib().vs_reads_info(self._h, a))
        return dict(ends=a[0], words=a[1], max_len=a[2], invalid_ends=a[3], device_bytes=a[4])

    @property
    def unpaired(self) -> bool:
        """A singles block (``Context.pack_singles``): end 2r is read r, every odd end is absent."""
        return bool(nat.lib().vs_reads_unpaired(self._h))

    def unpack(self):
        inf = self.info
        n = inf["ends"]
        lens = np.zeros(max(n, 1), dtype=np.uint32)
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        # two passes: lengths first (cheap), then text
        out = np.zeros(max(int(inf["words"]) * 16, 1), dtype=np.uint8)
        nat.check(self._ctx._h, nat.lib().vs_reads_unpack(self._ctx._h, self._h, out.ctypes.data,
                                                          lens.ctypes.data, flags.ctypes.data))
        total = int(lens[:n].sum())
        return out[:total], lens[:n], flags[:n]

    def free(self):
        if self._h:
            nat.lib().vs_reads_free(self._ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One HIP context (= one device).  ``device`` is the HIP ordinal."""

    def __init__(self, device: int = 0):
        L = nat.lib()
        h = C.c_void_p()
        rc = L.vs_ctx_create(device, C.byref(h))
        if rc != nat.VS_OK:
            nat.check(None, rc)
        self._h = h
        self.device = device
        self.n_nodes = 0
        self.ksize = 0
        self.node_order = None  # internal number -> position in the caller's node list (None: identical)
        self.node_rank = None   # the inverse

    def close(self):
        if self._h:
            nat.lib().vs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        nat.check(self._h, nat.lib().vs_ctx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def sync(self):
        nat.check(self._h, nat.lib().vs_ctx_sync(self._h))

    def build_index(self, seqs: Sequence[str], ksize: int, renumber: Optional[bool] = None):
        """KeyError(char) if a node of length >= ksize+1 holds a byte outside ACGT, as the
        reference's reverse_seq raises (PE_Inference.py:12-13).

        ``renumber`` (default on; ``VS_EXPERIMENT=1 VS_RENUMBER=0`` turns the default off): the index is built over the nodes in an
        order that runs along the graph's paths (``node_order``, csrc/vs_order_host.cpp) instead of the GFA's -- the
        device's matrices are then in that INTERNAL numbering (``node_order[internal] = position in seqs``), and
        everything that hands results out maps back: ``PeCounter.result``, ``map_ends``, ``HipPeLinks``.  Sums do not
        depend on the numbering; the time does (20-25 % of the step on a graph whose numbering scatters neighbours)."""
        if renumber is None:  # (the switch exists in experiment mode only, like the library's: INTEGRATION.md)
            renumber = not (os.environ.get("VS_EXPERIMENT") and os.environ.get("VS_RENUMBER", "1") == "0")
        data, off = encode_seqs(seqs)
        order = None
        if renumber and len(seqs) > 1:
            order = node_order(seqs, ksize, _encoded=(data, off))
            if np.array_equal(order, np.arange(len(seqs), dtype=order.dtype)):
                order = None
        if order is not None:
            data, off = encode_seqs([seqs[i] for i in order.tolist()])
        bad_node = C.c_uint32(0)
        bad_char = C.c_uint8(0)
        rc = nat.lib().vs_index_build(self._h, data.ctypes.data, off.ctypes.data, len(seqs), ksize,
                                      C.byref(bad_node), C.byref(bad_char))
        if rc == nat.VS_E_NODE_BASE:
            if order is not None:  # (the byte the reference names is the first one in GFA order: ask again in that order)
                return self.build_index(seqs, ksize, renumber=False)
            raise KeyError(chr(bad_char.value))
        nat.check(self._h, rc)
        self.n_nodes = len(seqs)
        self.ksize = ksize
        self.node_order = order  # None: the numbering of ``seqs``
        self.node_rank = None
        if order is not None:
            self.node_rank = np.empty(len(seqs), dtype=np.int64)
            self.node_rank[order] = np.arange(len(seqs), dtype=np.int64)

    def internal_cells(self, mat: int, u, v) -> np.ndarray:
        """Flat cell index inside ``PeCounter.mats[mat]`` (internal numbering) of the cells (u, v) given in the
        numbering of ``build_index``'s ``seqs``; ``mat`` 1 = short_mat, whose cell is (smaller, larger) index
        (PE_Inference.py:174-184) in the numbering it was counted in."""
        u = np.asarray(u, dtype=np.int64)
        v = np.asarray(v, dtype=np.int64)
        if self.node_rank is not None:
            u, v = self.node_rank[u], self.node_rank[v]
            if mat == 1:
                u, v = np.minimum(u, v), np.maximum(u, v)
        return u * self.n_nodes + v

    @property
    def index_info(self):
        a = (C.c_uint64 * 6)()
        nat.check(self._h, nat.lib().vs_index_info(self._h, a))
        return dict(seed_len=a[0], stride=a[1], seed_positions=a[2], slots=a[3], distinct_seeds=a[4], device_bytes=a[5])

    def index_export(self):
        """The built index as the kernels read it, in host arrays (a test aid, ``vs_index_export``): ``slot_key`` uint64,
        ``slot_a`` / ``slot_b`` uint32 [slots]; ``postings`` uint32 [seed positions, 4] (node, pos | strand << 31, node
        length, first word); ``fwd`` / ``rc`` uint32 packed words of either strand with the pad words; ``meta`` uint32
        [nodes, 2] (first word, length); ``table_bits``."""
        sizes = (C.c_uint64 * 5)()
        nat.check(self._h, nat.lib().vs_index_export(self._h, None, None, None, None, None, sizes))
        n_slots, n_post, n_words, n_nodes, bits = (int(x) for x in sizes)
        slots = np.zeros(n_slots, dtype=np.dtype([("key", "<u8"), ("a", "<u4"), ("b", "<u4")]))
        post = np.zeros((max(n_post, 1), 4), dtype=np.uint32)
        fwd = np.zeros(n_words, dtype=np.uint32)
        rc = np.zeros(n_words, dtype=np.uint32)
        meta = np.zeros((max(n_nodes, 1), 2), dtype=np.uint32)
        nat.check(self._h, nat.lib().vs_index_export(self._h, slots.ctypes.data, post.ctypes.data, fwd.ctypes.data, rc.ctypes.data,
                                                     meta.ctypes.data, sizes))
        return dict(slot_key=slots["key"].copy(), slot_a=slots["a"].copy(), slot_b=slots["b"].copy(), postings=post[:n_post],
                    fwd=fwd, rc=rc, meta=meta[:n_nodes], table_bits=bits)

    def scan_text(self, text: bytes, line0: int = 0):
        """The streamed ingest's device line scanner on ``text`` (a test aid, ``vs_fastq_scan_text``): (byte offsets of the
        newlines, flags: 1 a carriage return, 2 a byte >= 0x80, the record cut when the first line has number ``line0``)."""
        buf = np.frombuffer(text or b"\0", dtype=np.uint8)
        ends = np.zeros(max(text.count(b"\n"), 1), dtype=np.uint64)
        info = (C.c_uint64 * 3)()
        nat.check(self._h, nat.lib().vs_fastq_scan_text(self._h, buf.ctypes.data, len(text), line0, ends.ctypes.data, ends.size, info))
        return ends[: int(info[0])].copy(), int(info[1]), int(info[2])

    def scan_check(self, which: int, values, sentinel, flags: int = 0, total_before: int = 0):
        """One of the library's exclusive scans on ``values`` (a test aid, ``vs_scan_check``): ``which`` 0 the three-launch
        scan (``flags`` 1 in place, 2 without a place for its total), 1 the one-workgroup scan of the streamed ingests.
        ``sentinel``: the words behind the values on the device.  -> (the scanned words, the words behind them afterwards,
        the total; ``total_before`` where the scan was given no place for one)."""
        values = np.asarray(values, dtype=np.uint32)
        buf = np.concatenate([values, np.asarray(sentinel, dtype=np.uint32)])
        out = np.zeros(max(buf.size, 1), dtype=np.uint32)
        total = C.c_uint64(total_before)
        nat.check(self._h, nat.lib().vs_scan_check(self._h, which, buf.ctypes.data if buf.size else None, values.size, flags,
                                                   out.ctypes.data if buf.size else None, buf.size - values.size, C.byref(total)))
        return out[: values.size], out[values.size: buf.size], int(total.value)

    def pack(self, ascii_bytes: np.ndarray, off: np.ndarray) -> ReadBlock:
        ascii_bytes = np.ascontiguousarray(ascii_bytes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        h = C.c_void_p()
        nat.check(self._h, nat.lib().vs_reads_pack(self._h, ascii_bytes.ctypes.data, off.ctypes.data,
                                                   off.size - 1, C.byref(h)))
        return ReadBlock(self, h)

    def pack_pairs(self, fwd: Sequence[str], rve: Sequence[str]) -> ReadBlock:
        n = min(len(fwd), len(rve))
        seqs: List[str] = []
        for r in range(n):
            seqs.append(fwd[r])
            seqs.append(rve[r])
        data, off = encode_seqs(seqs)
        return self.pack(data, off)

    def pack_singles(self, reads: Sequence[str]) -> ReadBlock:
        """A singles block of unpaired reads (``vs_reads_pack_single``): one read per slot, no second end.  Counted, a read
        is worth what the reference gives ONE end of a pair: its own short_mat triangle, nothing in node_mat."""
        data, off = encode_seqs(list(reads))
        h = C.c_void_p()
        nat.check(self._h, nat.lib().vs_reads_pack_single(self._h, data.ctypes.data, off.ctypes.data, off.size - 1, C.byref(h)))
        return ReadBlock(self, h)

    def synth_pairs(self, genomes: Sequence[str], cum: np.ndarray, seed: int, first_pair: int, n_pairs: int,
                    read_len: int, sub_thresh: int = 0, n_thresh: int = 0) -> ReadBlock:
        gd, go = encode_seqs(genomes)
        cum = np.ascontiguousarray(cum, dtype=np.uint32)
        h = C.c_void_p()
        nat.check(self._h, nat.lib().vs_synth_pairs(self._h, gd.ctypes.data, go.ctypes.data, cum.ctypes.data,
                                                    len(genomes), seed, first_pair, n_pairs, read_len,
                                                    sub_thresh, n_thresh, C.byref(h)))
        return ReadBlock(self, h)

    def pe_count(self, reads: ReadBlock, node_mat_ptr: int, short_mat_ptr: int, stats_ptr: int, tile_map_ptr: Optional[int] = None):
        if tile_map_ptr is not None:  # also mark the 64 x 64 counter tiles the block adds to
            nat.check(self._h, nat.lib().vs_pe_count_tracked(self._h, reads._h, C.c_void_p(node_mat_ptr), C.c_void_p(short_mat_ptr),
                                                             C.c_void_p(stats_ptr), C.c_void_p(tile_map_ptr)))
            return
        nat.check(self._h, nat.lib().vs_pe_count(self._h, reads._h, C.c_void_p(node_mat_ptr),
                                                 C.c_void_p(short_mat_ptr), C.c_void_p(stats_ptr)))

    def node_depth(self, reads: ReadBlock, kc_ptr: int):
        """One block through the depth pass (``vs_node_depth``): ``kc_ptr`` is a device pointer to ``n_nodes`` 64-bit totals
        in the index's own numbering, added to.  Blocks must have been built after ``keep_masks(True)``."""
        nat.check(self._h, nat.lib().vs_node_depth(self._h, reads._h, C.c_void_p(kc_ptr)))

    def cover_layout(self, first_ptr: int) -> int:
        """The slots of the depth profile (``vs_cover_layout``): ``first_ptr`` is a device pointer to ``n_nodes + 1`` uint32,
        written with the first slot of every segment in the index's INTERNAL numbering and the slot total behind them -- a
        segment of ``k + 1`` bases or more owns one slot per window and one sentinel.  -> the slot total."""
        n = C.c_uint64(0)
        nat.check(self._h, nat.lib().vs_cover_layout(self._h, C.c_void_p(first_ptr), C.byref(n)))
        return int(n.value)

    def node_cover(self, reads: ReadBlock, first_ptr: int, diff_ptr: int):
        """One block through the profile pass (``vs_node_cover``): +1 / -1 per maximal match on the uint32 difference array
        at ``diff_ptr`` (one word per slot of ``cover_layout``).  Blocks must have been built after ``keep_masks(True)``."""
        nat.check(self._h, nat.lib().vs_node_cover(self._h, reads._h, C.c_void_p(first_ptr), C.c_void_p(diff_ptr)))

    def cover_fold(self, diff_ptr: int, cov_ptr: int, n_slots: int):
        """The differences scanned into counts, added to the uint64 totals at ``cov_ptr`` and zeroed (``vs_cover_fold``)."""
        nat.check(self._h, nat.lib().vs_cover_fold(self._h, C.c_void_p(diff_ptr), C.c_void_p(cov_ptr), n_slots))

    def pileup_layout(self, first_ptr: int) -> int:
        """The slots of the base pileup (``vs_pileup_layout``): ``first_ptr`` is a device pointer to ``n_nodes + 1`` uint32,
        written with the first slot of every segment in the index's INTERNAL numbering and the slot total behind them -- a
        segment of ``k + 1`` bases or more owns one slot per position and one sentinel.  -> the slot total."""
        n = C.c_uint64(0)
        nat.check(self._h, nat.lib().vs_pileup_layout(self._h, C.c_void_p(first_ptr), C.byref(n)))
        return int(n.value)

    def node_pileup(self, reads: ReadBlock, first_ptr: int, diff_ptr: int, alt_ptr: int, max_mismatch: int, tally_ptr: int):
        """One block through the pileup pass (``vs_node_pileup``): +1 / -1 per credited alignment on the uint32 difference
        array at ``diff_ptr`` (one word per slot of ``pileup_layout``), one count per non-agreeing base on the uint64
        ``[slots, 5]`` array at ``alt_ptr``, and (alignments, rejected) added to the two uint64 at ``tally_ptr``.  Blocks
        must have been built after ``keep_masks(True)``."""
        nat.check(self._h, nat.lib().vs_node_pileup(self._h, reads._h, C.c_void_p(first_ptr), C.c_void_p(diff_ptr), C.c_void_p(alt_ptr),
                                                    max_mismatch, C.c_void_p(tally_ptr)))

    def node_site_pairs(self, reads: ReadBlock, first_ptr: int, site_slot_ptr: int, n_sites: int, row_first_ptr: int, cells_ptr: int,
                        max_mismatch: int, tally_ptr: int):
        """One block through the site-pair pass (``vs_node_site_pairs``): ``site_slot_ptr``: ``n_sites`` ascending uint32 slots
        of ``pileup_layout``; ``row_first_ptr``: what ``site_pairs_rows`` made of them; one count per stored pair of sites a
        fragment saw on the uint64 ``[cells, 25]`` array at ``cells_ptr``, and the five tallies added to the uint64 at
        ``tally_ptr``.  Blocks must have been built after ``keep_masks(True)``."""
        nat.check(self._h, nat.lib().vs_node_site_pairs(self._h, reads._h, C.c_void_p(first_ptr), C.c_void_p(site_slot_ptr), n_sites,
                                                        C.c_void_p(row_first_ptr), C.c_void_p(cells_ptr), max_mismatch, C.c_void_p(tally_ptr)))

    def node_pileup_strands(self, reads: ReadBlock, first_ptr: int, n_slots: int, diff_ptr: int, alt_ptr: int, max_mismatch: int, tally_ptr: int):
        """One block through the stranded pileup pass (``vs_node_pileup_strands``): as ``node_pileup``, the alignments on the
        segment's forward text (plane 0) and on its reverse complement (plane 1) kept apart: ``diff_ptr``: uint32
        ``[2, n_slots]``, plane-major, every plane a difference array of its own; ``alt_ptr``: uint64 ``[n_slots, 2, 5]``;
        ``n_slots``: what ``pileup_layout`` gave.  Blocks must have been built after ``keep_masks(True)``."""
        nat.check(self._h, nat.lib().vs_node_pileup_strands(self._h, reads._h, C.c_void_p(first_ptr), n_slots, C.c_void_p(diff_ptr), C.c_void_p(alt_ptr),
                                                            max_mismatch, C.c_void_p(tally_ptr)))

    def pileup_call(self, first_ptr: int, n_slots: int, planes: int, depth_ptr: int, alt_ptr: int, min_alt_count: int, min_alt_frac: float,
                    min_alt_strand: int = 0, out_ptr: int = 0, cap: int = 0) -> int:
        """The records of a folded pileup, found on the device (``vs_pileup_call``): ``planes`` 1 -- ``depth_ptr`` uint64
        ``[n_slots]``, ``alt_ptr`` ``[n_slots, 5]``; 2 -- ``[2, n_slots]`` and ``[n_slots, 2, 5]``.  -> the exact number of
        records; they are written to ``out_ptr`` (device, ``[cap, 6]`` uint64: slot << 5 | strand_fail << 4 | ref << 2 | alt,
        DP, ref_f, ref_r, alt_f, alt_r; ascending by slot, then alt base) only if ``cap`` holds them all.  Synchronises."""
        n = C.c_uint64(0)
        nat.check(self._h, nat.lib().vs_pileup_call(self._h, C.c_void_p(first_ptr), n_slots, planes, C.c_void_p(depth_ptr), C.c_void_p(alt_ptr),
                                                    min_alt_count, min_alt_frac, min_alt_strand, C.c_void_p(out_ptr) if out_ptr else None, cap, C.byref(n)))
        return int(n.value)

    def node_indels(self, reads: ReadBlock, first_ptr: int, max_len: int, events_ptr: int, cap: int, tally_ptr: int) -> int:
        """One block through the indel pass (``vs_node_indels``): every insertion or deletion of at most ``max_len`` bases an end
        carries against a strand of a segment, as two uint64 (slot << 8 | plane << 7 | kind << 6 | (L - 1), the insert on the
        forward strand) at ``events_ptr`` (device, ``[cap, 2]``), in no order.  -> the exact number of events of the block;
        above ``cap`` the buffer holds nothing of use and the four uint64 at ``tally_ptr`` (matches tested, deletions,
        insertions, insertions dropped) were not added to: call again with room.  Synchronises.  Blocks must have been built
        after ``keep_masks(True)``."""
        n = C.c_uint64(0)
        nat.check(self._h, nat.lib().vs_node_indels(self._h, reads._h, C.c_void_p(first_ptr), max_len, C.c_void_p(events_ptr) if events_ptr else None, cap,
                                                    C.byref(n), C.c_void_p(tally_ptr)))
        return int(n.value)

    def contig_mems(self, reads: ReadBlock) -> np.ndarray:
        """Every maximal exact match of k + 1 bases or more between a contig of the block and a strand of a segment
        (``vs_contig_mems``): uint32 [n, 5] -- contig, first base in the contig, segment | strand << 31, first base in that
        strand's text, length -- in no order, the segment in the numbering of the list ``build_index`` was given.  ``contig`` is
        the read of a singles block.  Build the block after ``keep_masks(True)``, so that an 'N' bounds a match."""
        n = C.c_uint64(0)
        nat.check(self._h, nat.lib().vs_contig_mems(self._h, reads._h, None, 0, C.byref(n)))
        out = np.zeros((int(n.value), 5), dtype=np.uint32)
        if n.value:
            nat.check(self._h, nat.lib().vs_contig_mems(self._h, None, out.ctypes.data, n.value, C.byref(n)))
            if self.node_order is not None:
                seg = out[:, 2]
                out[:, 2] = self.node_order[seg & 0x7FFFFFFF].astype(np.uint32) | (seg & 0x80000000)
        return out

    def contig_mems_last(self) -> dict:
        """How the last ``contig_mems`` pass went (``vs_contig_mems_last``)."""
        a = (C.c_uint64 * 4)()
        nat.check(self._h, nat.lib().vs_contig_mems_last(self._h, a))
        return dict(records=int(a[0]), launches=int(a[1]), probes=int(a[2]), capacity_before=int(a[3]))

    def keep_masks(self, on: bool = True):
        """Read blocks built from now on keep their validity mask (``vs_ctx_keep_masks``): the depth pass counts the ends
        with an 'N' too and has to see where it is."""
        nat.check(self._h, nat.lib().vs_ctx_keep_masks(self._h, 1 if on else 0))

    def last_timing(self):
        a = (C.c_double * 5)()
        nat.check(self._h, nat.lib().vs_pe_last_timing(self._h, a))
        return dict(main_ms=a[0], slow_ms=a[1], slow_pairs=int(a[2]), sort_ms=a[3], accumulate_ms=a[4])

    @property
    def last_kernel(self) -> str:
        """Name of the mapping-kernel instantiation the last ``pe_count`` launched."""
        return (nat.lib().vs_pe_last_kernel(self._h) or b"").decode()

    RAN_LOCUS_LDS_SORT, RAN_LOCUS_GLOBAL_SORT, RAN_PE_MID, RAN_ROW_OWNERS = 1, 2, 8, 16
    RAN_LOCUS_STAGED = 4

    @property
    def last_launched(self) -> int:
        """VS_RAN_* bits: which optional kernels the most recent ``pe_count`` launched."""
        return int(nat.lib().vs_pe_last_launched(self._h))

    @property
    def lists_ept(self) -> int:
        """Read ends per tile of the plan ``pe_count_lists`` makes on this context now (``vs_pe_lists_ept``)."""
        return int(nat.lib().vs_pe_lists_ept(self._h))

    def list_block(self, pairs) -> Tuple[np.ndarray, np.ndarray]:
        """``list_block`` with this context's tile size."""
        return list_block(pairs, self.lists_ept)

    def pe_count_lists(self, n_nodes: int, lists: np.ndarray, counts: np.ndarray, node_mat_ptr: int, short_mat_ptr: int,
                       tile_map_ptr: Optional[int] = None):
        """The counter stage alone (a test aid, ``vs_pe_count_lists``): the per-end node lists ``lists`` uint32 [2 P, 20] /
        ``counts`` uint32 [2 P], in the order given, added to the device matrices of ``n_nodes`` nodes by the kernels a real
        count runs behind its mapping kernel.  Refused (``NativeError``, VS_E_RANGE): what ``list_block`` would not make."""
        lists = np.ascontiguousarray(lists, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if lists.ndim != 2 or lists.shape[1] != LIST_CAP or lists.shape[0] != counts.size or counts.size % 2:
            raise ValueError("lists [2 P, %d] and counts [2 P]" % LIST_CAP)
        nat.check(self._h, nat.lib().vs_pe_count_lists(self._h, n_nodes, counts.size // 2, lists.ctypes.data, counts.ctypes.data,
                                                       C.c_void_p(node_mat_ptr), C.c_void_p(short_mat_ptr),
                                                       C.c_void_p(tile_map_ptr) if tile_map_ptr is not None else None))

    def last_order(self):
        """The locus order of the most recent count (a test aid, ``vs_pe_last_order``): (keys uint32 [P] by pair, perm uint32
        [P] = the pairs in the order the mapping kernel took them, which sort ran: 0 none -- then both arrays are empty --
        ``RAN_LOCUS_LDS_SORT`` or ``RAN_LOCUS_GLOBAL_SORT``, pairs of that count)."""
        info = (C.c_uint64 * 2)()
        nat.check(self._h, nat.lib().vs_pe_last_order(self._h, None, None, 0, info))
        n, sort = int(info[0]), int(info[1])
        m = n if sort else 0
        keys = np.zeros(max(m, 1), dtype=np.uint32)
        perm = np.zeros(max(m, 1), dtype=np.uint32)
        if m:
            nat.check(self._h, nat.lib().vs_pe_last_order(self._h, keys.ctypes.data, perm.ctypes.data, m, info))
        return keys[:m], perm[:m], sort, n

    def last_handoff(self):
        """What the mapping kernel of the most recent ``pe_count`` left for the counter kernels (a test aid,
        ``vs_pe_last_handoff``), or None after a call that made no hand-off (``map_ends``, ``pe_count_lists``, an empty block).
        A dict: ``pairs``, ``ept``, ``list_ends``, ``rows`` (0 packed, 1 rows), ``pool`` and ``trim`` of the instantiation that
        ran, ``lists`` uint32 [words of that layout], ``counts`` uint32 [list_ends], ``overflow`` uint32 = the pairs k_pe_tiles
        put on the first overflow list, in the order its atomics took.  Node numbers are the index's internal ones."""
        info = (C.c_uint64 * 9)()
        nat.check(self._h, nat.lib().vs_pe_last_handoff(self._h, None, 0, None, 0, None, 0, info))
        if not info[0]:
            return None
        lists = np.zeros(max(int(info[8]), 1), dtype=np.uint32)
        counts = np.zeros(max(int(info[3]), 1), dtype=np.uint32)
        over = np.zeros(max(int(info[7]), 1), dtype=np.uint32)
        nat.check(self._h, nat.lib().vs_pe_last_handoff(self._h, lists.ctypes.data, lists.size, counts.ctypes.data, counts.size,
                                                        over.ctypes.data, over.size, info))
        return dict(pairs=int(info[1]), ept=int(info[2]), list_ends=int(info[3]), rows=int(info[4]), pool=int(info[5]), trim=int(info[6]),
                    lists=lists[: int(info[8])], counts=counts[: int(info[3])], overflow=over[: int(info[7])])

    def last_overflow(self):
        """Where the overflow pairs of the most recent ``pe_count`` / ``map_ends`` went (a test aid, ``vs_pe_last_overflow``),
        or None after a call that did not launch the overflow kernels (``pe_count_lists``, an empty block).  A dict:
        ``first_n`` = pairs k_pe_tiles gave up, ``second_n`` = pairs k_pe_mid passed on to k_pe_slow, ``second`` uint32 = those
        pairs (indices into the block), in the order its atomics took, ``no_mid`` = 1 where k_pe_mid was skipped."""
        info = (C.c_uint64 * 4)()
        nat.check(self._h, nat.lib().vs_pe_last_overflow(self._h, None, 0, info))
        if not info[0]:
            return None
        second = np.zeros(max(int(info[2]), 1), dtype=np.uint32)
        nat.check(self._h, nat.lib().vs_pe_last_overflow(self._h, second.ctypes.data, second.size, info))
        return dict(first_n=int(info[1]), second_n=int(info[2]), second=second[: int(info[2])], no_mid=int(info[3]))

    def map_ends(self, reads: ReadBlock, cap: int = 64) -> List[List[int]]:
        n = reads.info["ends"]
        lists = np.zeros((max(n, 1), cap), dtype=np.uint32)
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        nat.check(self._h, nat.lib().vs_pe_map_ends(self._h, reads._h, cap, lists.ctypes.data, counts.ctypes.data))
        out = []
        for e in range(n):
            c = int(counts[e])
            if c > cap:
                raise ValueError("end %d has %d nodes, cap %d" % (e, c, cap))
            ids = lists[e, :c] if self.node_order is None else self.node_order[lists[e, :c]]
            out.append(sorted(int(x) for x in ids))
        return out


class PeCounter:
    """node_mat / short_mat accumulation on one device (PE_Inference.py:137-188), counters held
    in torch tensors so that torch.distributed (RCCL) can all-reduce them in place.

    The kernels count in uint32 cells (``mats``: int32 storage, the bits are what matters -- a
    two's-complement sum IS the uint32 sum).  A cell grows by at most 2 per pair (``short_mat[i][i]``
    takes one increment per end, :174-184), so a buffer is exact while ``2 * pairs < 2**32``; before
    that bound is reached the buffer is folded into int64 totals on the device (``vs_counts_fold``),
    the reference's own cell type (``numpy.zeros(..., dtype=int)``, :139-140)."""

    # counters at least this large keep a map of the 64 x 64 tiles their blocks touch, and ``reset`` zeroes those tiles
    # only (vs_pe_count_tracked / vs_counts_zero_tracked); below it clearing the whole buffer is the cheaper way
    TRACK_TILES_MIN_BYTES = 2 << 30

    def __init__(self, ctx: Context, device: Optional[str] = None, track_tiles: Optional[bool] = None):
        import torch

        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        n = ctx.n_nodes
        self.n = n
        self.mats = torch.zeros((2, max(n, 1), max(n, 1)), dtype=torch.int32, device=self.device)
        if track_tiles is None:  # (VS_TRACK_TILES=1: tests run the tracked path on small graphs)
            track_tiles = self.device.type == "cuda" and (self.mats.numel() * 4 >= self.TRACK_TILES_MIN_BYTES or os.environ.get("VS_TRACK_TILES") == "1")
        tiles = (max(n, 1) + 63) // 64
        self.tile_map = torch.zeros(2 * tiles * tiles, dtype=torch.uint8, device=self.device) if track_tiles else None
        self.stats = torch.zeros(3, dtype=torch.int64, device=self.device)
        # unpaired reads (singles blocks) with N / shorter than k+1 / used: kept apart from the pairs' ``stats``
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)
        self.wide = None          # int64 totals, allocated by the first fold
        self.pairs_in_buffer = 0  # pairs counted into ``mats`` since it was last empty (all ranks, after a sum)
        self.pairs_seen = 0
        self.last_all_reduce = None  # "dense" / "compact" after all_reduce()
        self._xstate = ExchangeState()  # (what the exchanges of all_reduce keep between calls)
        # (the numbering of the index this counter counts under: kept here, so that a later build_index on the same context
        # cannot change how these matrices are read)
        self.node_order = getattr(ctx, "node_order", None)
        self.node_rank = getattr(ctx, "node_rank", None)

    def reserve_link_table(self) -> None:
        """Set aside the device buffer of the PE-link table the graph stages will build from these counters (N x N int64,
        ``vs_links_reserve``): called where the counters are made when the stages follow, so that the table's build does
        not wait for a large ``hipMalloc`` (0.3 ms or half a second for 23.7 GB, depending on what was freed before).
        An optimisation only: when the memory is not there now, the build allocates later (or fails there, where every rank
        can be told) -- a lone rank raising here would leave its peers waiting in the next collective."""
        if self.tile_map is not None and self.n >= 32768:
            return  # (the table of such counters is built from their dirty tiles as CSR rows, ABI 10: nothing to set aside)
        rc = nat.lib().vs_links_reserve(self.ctx._h, self.n)
        if rc == nat.VS_E_OOM:
            import warnings

            warnings.warn("the PE-link table's buffer could not be set aside now (%d nodes); it is allocated when the table is built" % self.n)
            return
        nat.check(self.ctx._h, rc)

    def reset(self):
        if self.tile_map is not None:
            # only the tiles the blocks since the last reset touched (every add marks them, every sum over the ranks ORs the
            # ranks' maps): the invariant is that a cell outside the marked tiles is zero
            torch = self.torch
            with torch.cuda.device(self.device):
                self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                nat.check(self.ctx._h, nat.lib().vs_counts_zero_tracked(self.ctx._h, C.c_void_p(self.mats[0].data_ptr()),
                                                                        C.c_void_p(self.mats[1].data_ptr()), self.n,
                                                                        C.c_void_p(self.tile_map.data_ptr())))
        else:
            self.mats.zero_()
        self.stats.zero_()
        self.single_stats.zero_()
        if self.wide is not None:
            self.wide.zero_()
        self.pairs_in_buffer = 0
        self.pairs_seen = 0

    def fold(self):
        """uint32 buffer -> int64 totals (device), buffer left empty."""
        torch = self.torch
        if self.wide is None:
            self.wide = torch.zeros(self.mats.shape, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            nat.check(self.ctx._h, nat.lib().vs_counts_fold(self.ctx._h, C.c_void_p(self.mats.data_ptr()),
                                                            C.c_void_p(self.wide.data_ptr()), self.mats.numel()))
        if self.tile_map is not None:
            self.tile_map.zero_()  # (the fold left every uint32 cell at zero)
        self.pairs_in_buffer = 0

    def add(self, reads: ReadBlock):
        """Count one block.  A singles block (``reads.unpaired``) adds to ``short_mat`` and ``single_stats`` only; a slot
        of it counts as one pair toward the uint32 bound (a cell grows by at most 1 per unpaired read)."""
        torch = self.torch
        n_pairs = reads.info["ends"] // 2
        stats = self.single_stats if reads.unpaired else self.stats
        if 2 * (self.pairs_in_buffer + n_pairs) >= U32_LIMIT:
            self.fold()
        if 2 * n_pairs >= U32_LIMIT:
            raise OverflowError("one read block of %d pairs can overflow a uint32 cell; use blocks of < 2^31 pairs" % n_pairs)
        self.pairs_in_buffer += n_pairs
        self.pairs_seen += n_pairs
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.pe_count(reads, self.mats[0].data_ptr(), self.mats[1].data_ptr(), stats.data_ptr(),
                              tile_map_ptr=self.tile_map.data_ptr() if self.tile_map is not None else None)

    def _occupied(self, head):
        """uint8 [m]: which 64-cell stretches of ``head`` ([m, 64] view of a counter buffer on this device) hold a non-zero
        cell -- one pass of the library's kernel over the buffer, on torch's current stream."""
        torch = self.torch
        occ = torch.empty(head.shape[0], dtype=torch.uint8, device=head.device)
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            nat.check(self.ctx._h, nat.lib().vs_counts_occupied(self.ctx._h, C.c_void_p(head.data_ptr()), head.element_size(),
                                                                head.shape[0], C.c_void_p(occ.data_ptr())))
        return occ

    def all_reduce(self, predict=False):
        """Sum over the ranks of the process group, in place, in TWO collectives (``dist.agree`` + ``Exchange.sum``): a MAX
        over [occupancy of the counters' 64-cell stretches | flag bytes], then a SUM over [the occupied stretches of the
        union | a row with the three stats and the pairs in the buffers].  The flag bytes settle, for every rank alike,
        whether the uint32 buffers can hold the sum: if not, or if some rank already holds int64 totals, every rank folds
        and the int64 totals are agreed on and summed (two more collectives); a rank whose environment turns the compact
        exchange off vetoes it for everybody.  Every rank ends with the full sums.

        ``predict``: the steady state of fixed-size steps (bench.py) -- no host wait at all; the preconditions (no int64
        totals, the bound, the veto) are checked statically here and again from the agreed flag bytes when ``settle()`` is
        called before the buffer is reused."""
        from . import dist as vdist

        world = vdist.group_size()
        if world <= 1:
            return
        torch = self.torch
        may_compact = os.environ.get("VS_COMPACT_ALLREDUCE", "1") not in ("0", "")
        p = int(self.pairs_in_buffer)
        flags = vdist.flag_bytes(no_compact=not may_compact, wide=self.wide is not None, pairs=p)
        tail = torch.cat([self.stats.to(torch.int64), torch.tensor([p], dtype=torch.int64, device=self.stats.device)])
        timing = {} if os.environ.get("VS_DIST_TIMING") else None
        occ_fn = self._occupied if self.mats.is_cuda else None
        xs = self._xstate
        if predict and xs.cap is not None:
            if self.wide is not None or 2 * p * world >= U32_LIMIT or not may_compact:
                raise OverflowError("a predicted exchange sums uint32 buffers through their occupied stretches: 2 * %d pairs * %d "
                                    "ranks must fit, without int64 totals or a veto; use all_reduce()" % (p, world))
            how, out_tail = vdist.sum_counts(self.mats, tail, flags, self.tile_map, timing, occ_fn, state=xs, predict=True)
            self.stats.copy_(out_tail[:3])
            self.pairs_in_buffer = p * world  # (a bound; the steps' blocks are of one size)
        else:
            xs.collectives = xs.host_waits = 0
            x = vdist.agree(self.mats, tail, flags, self.tile_map, timing, occ_fn, xs)
            fl, u = x.read()
            if vdist.must_fold(fl, world):
                self.fold()
                x = vdist.agree(self.wide, tail, vdist.flag_bytes(no_compact=not may_compact), None, timing, occ_fn, xs)
                fl, u = x.read()
            how, out_tail = x.sum(fl, u)
            out = out_tail.cpu()
            self.stats.copy_(out[:3].to(self.stats.device))
            self.pairs_in_buffer = 0 if self.wide is not None else int(out[3])
        self.last_all_reduce = how
        self.last_collectives = xs.collectives
        if timing is not None:
            self.exchange_timing = getattr(self, "exchange_timing", [])
            self.exchange_timing.append(timing)

    def _xstate_cap(self, value=None):
        """The union size the next predicted exchange is staged for (None: not known yet); with a value: set it."""
        if value is not None:
            self._xstate.cap = value
        return self._xstate.cap

    def settle(self):
        """The deferred half of ``all_reduce(predict=True)``; call before the buffer is counted into again."""
        from . import dist as vdist

        vdist.settle(self._xstate)

    def write_sparse_text(self, pe_path: str, st_path: str, ids: Sequence[str]):
        """``pe_info`` / ``st_info`` without the lines whose count is 0 -- the other lines byte for byte those
        ``write_matrix_text`` writes from ``result()``, in the same order -- formatted from the counters where they lie
        (``vs_write_info_sparse``: on the device for device counters; counters held in CPU tensors go through the library's
        host twin).  No permuted copy of a matrix is made and none is downloaded.  Returns per file
        ``dict(lines, bytes, blocks, cells_read)``."""
        return self._write_info_text("vs_write_info_sparse", pe_path, st_path, ids, (), ("lines", "bytes", "blocks", "cells_read"))

    def write_bgzf_text(self, pe_path: str, st_path: str, ids: Sequence[str], dense: bool = False):
        """``pe_info`` / ``st_info`` as BGZF, formatted AND deflated where the counters lie (``vs_write_info_bgzf``: on the
        device for device counters, the library's host twin for CPU tensors -- the same bytes).  ``dense``: every line of
        the reference's file, zeros included, so that ``gzip -dc`` gives back that file byte for byte; otherwise the
        sparse text of ``write_sparse_text``.  Only compressed bytes leave the device.  Returns per file
        ``dict(lines, bytes, blocks, cells_read, members, file_bytes)`` (``bytes``: of text; ``members``: without the
        28-byte EOF member that ends the file)."""
        return self._write_info_text("vs_write_info_bgzf", pe_path, st_path, ids, (1 if dense else 0,),
                                     ("lines", "bytes", "blocks", "cells_read", "members", "file_bytes"))

    def _write_info_text(self, entry: str, pe_path: str, st_path: str, ids: Sequence[str], extra, keys):
        torch = self.torch
        n = self.n
        if len(ids) != n:
            raise ValueError("%d ids for counters of %d nodes" % (len(ids), n))
        blob, off = _encode_ids(ids)
        rank = None if self.node_rank is None else np.ascontiguousarray(self.node_rank, dtype=np.uint32)
        tiles = (max(n, 1) + 63) // 64
        on_device = self.mats.is_cuda
        if on_device:
            torch.cuda.synchronize(self.device)
        out = []
        for m, path in enumerate((pe_path, st_path)):
            info = (C.c_uint64 * len(keys))()
            args = (path.encode(), blob.ctypes.data, off.ctypes.data, n,
                    C.c_void_p(self.mats[m].data_ptr()) if n else None,
                    C.c_void_p(self.wide[m].data_ptr()) if (self.wide is not None and n) else None,
                    C.c_void_p(self.tile_map[m * tiles * tiles:].data_ptr()) if (self.tile_map is not None and n) else None,
                    rank.ctypes.data if rank is not None else None, m) + tuple(extra) + (info,)
            if on_device:
                with torch.cuda.device(self.device):
                    self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                    rc = getattr(nat.lib(), entry)(self.ctx._h, *args)
                err = self.ctx._h
            else:
                rc = getattr(nat.lib(), entry + "_host")(None, *args)
                err = None
            if rc != nat.VS_OK:
                msg = (nat.lib().vs_last_error(err) or b"?").decode("utf-8", "replace")
                raise (OSError if "cannot open" in msg or "write to" in msg else ValueError)(msg)
            out.append({key: int(info[i]) for i, key in enumerate(keys)})
        return out

    def user_order(self, t):
        """[2,N,N] device tensor in the index's internal numbering -> the caller's (``Context.build_index``):
        node_mat rows and columns permuted; short_mat, which holds a pair of nodes at (smaller, larger) number
        (PE_Inference.py:174-184: ``i <= i2`` over ascending indices), mirrored first and cut back to the upper
        triangle of the caller's numbering after."""
        torch = self.torch
        rank = self.node_rank
        if rank is None:
            return t
        r = torch.from_numpy(rank).to(t.device)
        # (one matrix at a time, every intermediate freed before the next is made: a 54 k-node graph is 11.8 GB per
        # int32 matrix, and this runs when a run that counted fine wants its result)
        out = torch.empty_like(t)
        rows = t[0].index_select(0, r)
        torch.index_select(rows, 1, r, out=out[0])
        del rows
        s = t[1] + t[1].t()
        s.diagonal().sub_(t[1].diagonal())  # (the diagonal was doubled by the mirror)
        rows = s.index_select(0, r)
        del s
        torch.index_select(rows, 1, r, out=out[1])
        del rows
        out[1].triu_()
        return out

    def result(self):
        """-> (node_mat int64 [N,N], short_mat int64 [N,N], (n_reads, short_reads, used_reads)), in the numbering of
        the node list ``Context.build_index`` was given."""
        n = self.n
        m = self.user_order(self.mats[:, :n, :n]).cpu().numpy().view(np.uint32).astype(np.int64)
        if self.wide is not None:
            m += self.user_order(self.wide[:, :n, :n]).cpu().numpy()
        s = self.stats.cpu().numpy()
        return m[0], m[1], (int(s[0]), int(s[1]), int(s[2]))


def depth_plan(n_nodes: int, ksize: int, n_ends: int, max_len: int, n_cu: int = 256) -> dict:
    """The launch ``vs_node_depth`` makes (``vs_depth_plan``, a pure host function: no device is needed)."""
    a = (C.c_uint64 * 8)()
    rc = nat.lib().vs_depth_plan(n_nodes, ksize, n_ends, max_len, n_cu, a)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_depth_plan refuses %d nodes / %d ends" % (n_nodes, n_ends))
    return dict(route=("none", "lds", "global")[int(a[0])], grid=int(a[1]), ends_per_wg=int(a[2]), wrap_ends=int(a[3]), lds_nodes=int(a[4]),
                lds_bytes=int(a[5]), node_limit=int(a[6]), threads=int(a[7]))


def contig_chain(mems, seg_lens: Sequence[int], ksize: int, n_contigs: int):
    """Match records (``Context.contig_mems``, any order) chained into .paths entries (``vs_contig_chain``, a pure host
    function: no device is needed).  -> (per contig its parts, each a list of (segment, strand, windows); per contig the
    number of its windows with more than one hit)."""
    mems = np.ascontiguousarray(mems, dtype=np.uint32).reshape(-1, 5)
    lens = np.ascontiguousarray(seg_lens, dtype=np.uint32)
    tokens = np.zeros((max(len(mems), 1), 4), dtype=np.uint32)
    ambiguous = np.zeros(max(n_contigs, 1), dtype=np.uint64)
    n = C.c_uint64(0)
    rc = nat.lib().vs_contig_chain(mems.ctypes.data if len(mems) else None, len(mems), lens.ctypes.data if len(lens) else None, len(lens), ksize,
                                   n_contigs, tokens.ctypes.data, C.byref(n), ambiguous.ctypes.data)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_contig_chain refuses the records: a contig or segment out of range, a match shorter than k + 1 or one that leaves its segment")
    parts: List[List[List[Tuple[int, int, int]]]] = [[] for _ in range(n_contigs)]
    for c, seg, windows, first in tokens[: int(n.value)].tolist():
        if first:
            parts[c].append([])
        parts[c][-1].append((seg & 0x7FFFFFFF, seg >> 31, windows))
    return parts, [int(v) for v in ambiguous[:n_contigs]]


class DepthCounter:
    """KC per segment, counted from the reads on one device (``vs_node_depth``): the number of (k+1)-mer occurrences of the
    segment in the read ends, what SPAdes writes as ``KC:i``.  Takes the place of a ``PeCounter`` in the input dispatch of
    ``pe_inference`` (``add``, ``device``, ``single_stats``); every end of every block counts, mates and filters aside.
    The context keeps the masks of the blocks built after this (``Context.keep_masks``)."""

    def __init__(self, ctx: Context, device: Optional[str] = None):
        import torch

        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.kc = torch.zeros(max(self.n, 1), dtype=torch.int64, device=self.device)
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        self.node_rank = getattr(ctx, "node_rank", None)  # (kept here, as PeCounter does: a later build_index cannot change how kc is read)
        ctx.keep_masks(True)

    def add(self, reads: ReadBlock):
        torch = self.torch
        n_ends = reads.info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.node_depth(reads, self.kc.data_ptr())

    def result(self) -> np.ndarray:
        """int64 [N] in the numbering of the node list ``Context.build_index`` was given (the GFA's order)."""
        kc = self.kc[: self.n]
        if self.node_rank is not None:
            kc = kc.index_select(0, self.torch.from_numpy(self.node_rank).to(kc.device))
        return kc.cpu().numpy().astype(np.int64)


def cover_plan(n_nodes: int, ksize: int, n_ends: int, max_len: int, n_cu: int = 256, pending: int = 0, bound: int = 2 ** 32) -> dict:
    """The launch ``vs_node_cover`` makes for a block and whether a fold is due before it (``vs_cover_plan``, a pure host
    function: no device is needed).  ``pending``: the ``pending`` of the block before (0 at the start and after a fold);
    ``bound``: what the pending weight may not reach between two folds."""
    a = (C.c_uint64 * 8)()
    rc = nat.lib().vs_cover_plan(n_nodes, ksize, n_ends, max_len, n_cu, pending, bound, a)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_cover_plan refuses %d nodes / %d ends of up to %d bases (pending %d, bound %d)" % (n_nodes, n_ends, max_len, pending, bound))
    return dict(launch=bool(a[0]), grid=int(a[1]), ends_per_wg=int(a[2]), weight=int(a[3]), fold_first=bool(a[4]), pending=int(a[5]),
                lds_bytes=int(a[6]), threads=int(a[7]))


class CoverCounter:
    """The k-mer depth of every window of every segment, counted from the reads on one device (``vs_node_cover``):
    ``cov[n][p]`` = the (k+1)-mer occurrences ``KC[n]`` counts whose table entry is ``(n, p)`` -- the window that STARTS at
    forward offset ``p`` (k-mer coverage, not base coverage).  Takes ``DepthCounter``'s place in the input dispatch of
    ``pe_inference`` (``add``, ``device``, ``single_stats``, ``ends_seen``; the context keeps the masks): one kernel per block,
    and ``kc()`` is what ``DepthCounter.result()`` gives.  Holds 4 + 8 bytes per slot (a slot per window and one per segment);
    the context holds 4 more per slot once a fold ran.  ``fold_bound``: ``cover_plan``'s ``bound`` (a test sets it low)."""

    def __init__(self, ctx: Context, fold_bound: int = 2 ** 32, device: Optional[str] = None):
        import torch

        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.ksize = ctx.ksize
        self.fold_bound = fold_bound
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        self.folds = 0
        self.pending = 0    # cover_plan's weight of the blocks since the last fold
        self.node_rank = getattr(ctx, "node_rank", None)  # (kept here: a later build_index cannot change how the slots are read)
        with torch.cuda.device(self.device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.first = torch.zeros(self.n + 1, dtype=torch.int32, device=self.device)  # (uint32 words)
            self.slots = ctx.cover_layout(self.first.data_ptr())
            self.diff = torch.zeros(max(self.slots, 1), dtype=torch.int32, device=self.device)  # (uint32 words, wrap-around adds)
            self.cov = torch.zeros(max(self.slots, 1), dtype=torch.int64, device=self.device)
        ctx.keep_masks(True)

    def fold(self):
        torch = self.torch
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.cover_fold(self.diff.data_ptr(), self.cov.data_ptr(), self.slots)
        self.pending = 0
        self.folds += 1

    def add(self, reads: ReadBlock):
        torch = self.torch
        info = reads.info
        n_ends = info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        plan = cover_plan(self.n, self.ksize, n_ends, info["max_len"], pending=self.pending, bound=self.fold_bound)
        if plan["fold_first"]:
            self.fold()
        self.pending = plan["pending"]
        if not self.slots:
            return
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.node_cover(reads, self.first.data_ptr(), self.diff.data_ptr())

    def result(self):
        """-> (offsets int64 [N + 1], cov int64 [W]): the windows of segment ``n`` of the node list ``Context.build_index`` was
        given (the GFA's order) are ``cov[offsets[n] : offsets[n + 1]]``, without sentinel slots; a segment shorter than
        ``k + 1`` bases is an empty range."""
        if self.pending:
            self.fold()
        first = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
        slots = self.cov[: self.slots].cpu().numpy()
        windows = np.maximum(first[1:] - first[:-1] - 1, 0)
        start = first[:-1]
        if self.node_rank is not None:
            windows, start = windows[self.node_rank], start[self.node_rank]
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(windows, out=offsets[1:])
        total = int(offsets[-1])
        at = np.repeat(start - offsets[:-1], windows) + np.arange(total, dtype=np.int64)
        return offsets, slots[at].astype(np.int64)

    def kc(self) -> np.ndarray:
        """The row sums, int64 [N] in the GFA's order: ``KC`` as ``DepthCounter.result()`` gives it."""
        offsets, cov = self.result()
        run = np.zeros(cov.size + 1, dtype=np.int64)
        np.cumsum(cov, out=run[1:])
        return run[offsets[1:]] - run[offsets[:-1]]


def pileup_plan(n_nodes: int, ksize: int, n_ends: int, max_len: int, n_cu: int = 256, pending: int = 0, bound: int = 2 ** 32) -> dict:
    """The launch ``vs_node_pileup`` makes for a block and whether a fold is due before it (``vs_pileup_plan``, a pure host
    function: no device is needed), with ``cover_plan``'s arguments and fields; the weight is ``n_ends * 2 * max_len``."""
    a = (C.c_uint64 * 8)()
    rc = nat.lib().vs_pileup_plan(n_nodes, ksize, n_ends, max_len, n_cu, pending, bound, a)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_pileup_plan refuses %d nodes / %d ends of up to %d bases (pending %d, bound %d)" % (n_nodes, n_ends, max_len, pending, bound))
    return dict(launch=bool(a[0]), grid=int(a[1]), ends_per_wg=int(a[2]), weight=int(a[3]), fold_first=bool(a[4]), pending=int(a[5]),
                lds_bytes=int(a[6]), threads=int(a[7]))


def pileup_call_host(ref: int, depth, alt, min_alt_count: int = 2, min_alt_frac: float = 0.01, min_alt_strand: int = 0) -> List[Tuple[int, ...]]:
    """The records of ONE position by the rule the device caller runs (``vs_pileup_call_host``, a pure host function: no device
    is needed).  ``ref``: the segment's base code 0..3; ``depth``: one count per plane (1 or 2 of them); ``alt``: ``[planes][5]``.
    -> up to three ``(strand_fail, ref, alt, DP, ref_f, ref_r, alt_f, alt_r)``, in ACGT order of the alt base."""
    d = np.ascontiguousarray(depth, dtype=np.uint64).reshape(-1)
    a = np.ascontiguousarray(alt, dtype=np.uint64).reshape(-1)
    if a.size != 5 * d.size:
        raise ValueError("pileup_call_host: five alt columns per plane are needed")
    out = np.zeros((3, 6), dtype=np.uint64)
    n = C.c_uint32(0)
    rc = nat.lib().vs_pileup_call_host(ref, d.size, d.ctypes.data, a.ctypes.data, min_alt_count, min_alt_frac, min_alt_strand, out.ctypes.data, C.byref(n))
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_pileup_call_host refuses base %r, %d planes, a fraction of %r, a strand threshold of %r" % (ref, d.size, min_alt_frac, min_alt_strand))
    return [(int(r[0]) >> 4 & 1, int(r[0]) >> 2 & 3, int(r[0]) & 3) + tuple(int(v) for v in r[1:]) for r in out[:n.value]]


def _call_on_device(counter, planes: int, min_alt_count: int, min_alt_frac: float, min_alt_strand: int):
    """``call()`` of both pileup counters: the device caller on the counter's folded tables, and the records -- nothing else
    leaves the device -- mapped from slots to the GFA's order and sorted."""
    torch = counter.torch
    if not 0 <= int(min_alt_count) < 2 ** 64 or not 0 <= int(min_alt_strand) < 2 ** 64:
        raise ValueError("call: counts from 0 up are needed")
    if counter.pending:
        counter.fold()
    args = (counter.first.data_ptr(), counter.slots, planes, counter.depth.data_ptr(), counter.alt.data_ptr(), int(min_alt_count), float(min_alt_frac),
            int(min_alt_strand))
    with torch.cuda.device(counter.device):
        counter.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        n = counter.ctx.pileup_call(*args)
        out = torch.zeros((max(n, 1), 6), dtype=torch.int64, device=counter.device)
        if n and counter.ctx.pileup_call(*args, out_ptr=out.data_ptr(), cap=n) != n:
            raise RuntimeError("vs_pileup_call: the number of records changed between two calls on the same tables")
        rec = out[:n].cpu().numpy()
    first = counter.first.cpu().numpy().view(np.uint32).astype(np.int64)
    head = rec[:, 0]
    slot = head >> 5
    rank = np.searchsorted(first, slot, side="right") - 1  # (the segment that holds the slot: one without slots holds none)
    pos0 = slot - first[rank]
    seg = rank
    if counter.node_rank is not None:
        order = np.empty(counter.n, dtype=np.int64)
        order[np.asarray(counter.node_rank, dtype=np.int64)] = np.arange(counter.n, dtype=np.int64)
        seg = order[rank]
    alt = head & 3
    by = np.lexsort((alt, pos0, seg))
    return (seg[by].astype(np.int64), pos0[by].astype(np.int64), (head >> 2 & 3)[by].astype(np.int64), alt[by].astype(np.int64),
            rec[by, 1].astype(np.int64), rec[by, 2:6].astype(np.int64).reshape(n, 4), (head >> 4 & 1)[by].astype(bool))


class PileupCounter:
    """The base pileup of every segment, counted from the reads on one device (``vs_node_pileup``): every read end is laid
    along the diagonal of each exact anchor of ``k + 1`` bases across its mismatches; an alignment with at most
    ``max_mismatch`` non-agreeing positions in its overlap adds 1 to the depth of every position it covers and 1 to
    ``alt[position][base]`` where it differs (``tests/pileup_model.py``) -- BASE coverage, substitutions only.  Takes
    ``CoverCounter``'s place in the input dispatch of ``pe_inference`` (``add``, ``device``, ``single_stats``, ``ends_seen``;
    the context keeps the masks): one kernel per block.  Holds 4 + 8 + 40 bytes per slot (a slot per position and one per
    segment); the context holds 4 more per slot once a fold ran.  ``fold_bound``: ``pileup_plan``'s ``bound``."""

    def __init__(self, ctx: Context, max_mismatch: int = 8, fold_bound: int = 2 ** 32, device: Optional[str] = None):
        import torch

        if not 0 <= int(max_mismatch) < 2 ** 32:
            raise ValueError("a mismatch budget of %r: an integer from 0 up is needed" % (max_mismatch,))
        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.ksize = ctx.ksize
        self.max_mismatch = int(max_mismatch)
        self.fold_bound = fold_bound
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        self.folds = 0
        self.pending = 0    # pileup_plan's weight of the blocks since the last fold
        self.node_rank = getattr(ctx, "node_rank", None)  # (kept here: a later build_index cannot change how the slots are read)
        with torch.cuda.device(self.device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.first = torch.zeros(self.n + 1, dtype=torch.int32, device=self.device)  # (uint32 words)
            self.slots = ctx.pileup_layout(self.first.data_ptr())
            self.diff = torch.zeros(max(self.slots, 1), dtype=torch.int32, device=self.device)  # (uint32 words, wrap-around adds)
            self.depth = torch.zeros(max(self.slots, 1), dtype=torch.int64, device=self.device)
            self.alt = torch.zeros((max(self.slots, 1), 5), dtype=torch.int64, device=self.device)
            self.tally = torch.zeros(2, dtype=torch.int64, device=self.device)
        ctx.keep_masks(True)

    def fold(self):
        torch = self.torch
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.cover_fold(self.diff.data_ptr(), self.depth.data_ptr(), self.slots)
        self.pending = 0
        self.folds += 1

    def add(self, reads: ReadBlock):
        torch = self.torch
        info = reads.info
        n_ends = info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        plan = pileup_plan(self.n, self.ksize, n_ends, info["max_len"], pending=self.pending, bound=self.fold_bound)
        if plan["fold_first"]:
            self.fold()
        self.pending = plan["pending"]
        if not self.slots:
            return
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.node_pileup(reads, self.first.data_ptr(), self.diff.data_ptr(), self.alt.data_ptr(), self.max_mismatch, self.tally.data_ptr())

    def result(self):
        """-> (offsets int64 [N + 1], depth int64 [P], alt int64 [P, 5]): the positions of segment ``n`` of the node list
        ``Context.build_index`` was given (the GFA's order) are rows ``offsets[n] : offsets[n + 1]``, without sentinel slots;
        a segment shorter than ``k + 1`` bases is an empty range.  ``alt[:, 0..3]``: reads carrying A, C, G, T where the
        segment has another base; ``alt[:, 4]``: a byte outside ACGT."""
        if self.pending:
            self.fold()
        first = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
        depth = self.depth[: self.slots].cpu().numpy()
        alt = self.alt[: self.slots].cpu().numpy()
        positions = np.maximum(first[1:] - first[:-1] - 1, 0)
        start = first[:-1]
        if self.node_rank is not None:
            positions, start = positions[self.node_rank], start[self.node_rank]
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(positions, out=offsets[1:])
        total = int(offsets[-1])
        at = np.repeat(start - offsets[:-1], positions) + np.arange(total, dtype=np.int64)
        return offsets, depth[at].astype(np.int64), alt[at].astype(np.int64).reshape(total, 5)

    def call(self, min_alt_count: int = 2, min_alt_frac: float = 0.01):
        """The records of ``--variants`` found on the device (``vs_pileup_call`` with one plane): what
        ``node_depth.variant_records`` makes of ``result()``, without the tables leaving the device.  -> ``(seg, pos0, ref,
        alt, dp, dp4 [R, 4], strand_fail)`` as ``StrandPileupCounter.call``; ``dp4[:, 1]`` and ``dp4[:, 3]`` are 0."""
        return _call_on_device(self, 1, min_alt_count, min_alt_frac, 0)

    def tallies(self):
        """-> (alignments credited, alignments rejected for more than ``max_mismatch`` non-agreeing positions)."""
        t = self.tally.cpu().numpy()
        return int(t[0]), int(t[1])


class StrandPileupCounter:
    """The base pileup kept apart by strand, counted from the reads on one device (``vs_node_pileup_strands``): everything
    ``PileupCounter`` counts, in two PLANES -- 0: the alignments that lay the end, as the ingest delivers it, along the
    segment's forward text; 1: those along its reverse complement (``tests/strand_pileup_model.py``).  Summed over the planes
    it is ``PileupCounter``'s result exactly.  Takes ``PileupCounter``'s place in the input dispatch of ``pe_inference``
    (``add``, ``device``, ``single_stats``, ``ends_seen``; the context keeps the masks): one kernel per block.  Holds 8 + 16 +
    80 = 104 bytes per slot (a slot per position and one per segment); the context holds 4 more per slot once a fold or a
    ``call`` ran.  ``fold_bound``: ``pileup_plan``'s ``bound`` -- the plan is the unstranded one: a plane gets at most half
    the weight it assumes."""

    def __init__(self, ctx: Context, max_mismatch: int = 8, fold_bound: int = 2 ** 32, device: Optional[str] = None):
        import torch

        if not 0 <= int(max_mismatch) < 2 ** 32:
            raise ValueError("a mismatch budget of %r: an integer from 0 up is needed" % (max_mismatch,))
        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.ksize = ctx.ksize
        self.max_mismatch = int(max_mismatch)
        self.fold_bound = fold_bound
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        self.folds = 0      # folds of BOTH planes
        self.pending = 0    # pileup_plan's weight of the blocks since the last fold
        self.node_rank = getattr(ctx, "node_rank", None)  # (kept here: a later build_index cannot change how the slots are read)
        with torch.cuda.device(self.device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.first = torch.zeros(self.n + 1, dtype=torch.int32, device=self.device)  # (uint32 words)
            self.slots = ctx.pileup_layout(self.first.data_ptr())
            self.diff = torch.zeros((2, max(self.slots, 1)), dtype=torch.int32, device=self.device)  # (uint32 words, wrap-around adds; plane-major)
            self.depth = torch.zeros((2, max(self.slots, 1)), dtype=torch.int64, device=self.device)
            self.alt = torch.zeros((max(self.slots, 1), 2, 5), dtype=torch.int64, device=self.device)
            self.tally = torch.zeros(2, dtype=torch.int64, device=self.device)
        ctx.keep_masks(True)

    def fold(self):
        torch = self.torch
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            for t in range(2):  # (every plane is a difference array of its own: S slots each)
                self.ctx.cover_fold(self.diff.data_ptr() + 4 * t * self.slots, self.depth.data_ptr() + 8 * t * self.slots, self.slots)
        self.pending = 0
        self.folds += 1

    def add(self, reads: ReadBlock):
        torch = self.torch
        info = reads.info
        n_ends = info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        plan = pileup_plan(self.n, self.ksize, n_ends, info["max_len"], pending=self.pending, bound=self.fold_bound)
        if plan["fold_first"]:
            self.fold()
        self.pending = plan["pending"]
        if not self.slots:
            return
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.node_pileup_strands(reads, self.first.data_ptr(), self.slots, self.diff.data_ptr(), self.alt.data_ptr(), self.max_mismatch,
                                         self.tally.data_ptr())

    def result(self):
        """-> (offsets int64 [N + 1], depth int64 [P, 2], alt int64 [P, 2, 5]): ``PileupCounter.result`` with a plane axis
        behind the position's: rows ``offsets[n] : offsets[n + 1]`` are the positions of segment ``n`` in the GFA's order,
        without sentinel slots."""
        if self.pending:
            self.fold()
        first = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
        depth = self.depth.cpu().numpy().reshape(2, -1)
        alt = self.alt.cpu().numpy()
        positions = np.maximum(first[1:] - first[:-1] - 1, 0)
        start = first[:-1]
        if self.node_rank is not None:
            positions, start = positions[self.node_rank], start[self.node_rank]
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(positions, out=offsets[1:])
        total = int(offsets[-1])
        at = np.repeat(start - offsets[:-1], positions) + np.arange(total, dtype=np.int64)
        return offsets, np.ascontiguousarray(depth[:, at].T).astype(np.int64).reshape(total, 2), alt[at].astype(np.int64).reshape(total, 2, 5)

    def call(self, min_alt_count: int = 2, min_alt_frac: float = 0.01, min_alt_strand: int = 0):
        """The records of ``--variants``, found on the device (``vs_pileup_call``): every (position, base other than the
        segment's) with ``AD > 0``, ``AD >= min_alt_count`` and ``AD >= min_alt_frac * DP``, both summed over the planes.
        -> ``(seg, pos0, ref, alt, dp, dp4 [R, 4], strand_fail)``: ``seg`` in the GFA's order, ``pos0`` 0-based, ``ref`` and
        ``alt`` base codes (0..3 = ACGT), ``dp4`` = ref_f, ref_r, alt_f, alt_r; ``strand_fail``: ``min_alt_strand >= 1`` and
        the alt base has fewer reads than that in a plane -- the record stays.  Sorted by segment, position, base.  int64 and
        bool; only the records leave the device."""
        return _call_on_device(self, 2, min_alt_count, min_alt_frac, min_alt_strand)

    def tallies(self):
        """-> (alignments credited, alignments rejected for more than ``max_mismatch`` non-agreeing positions)."""
        t = self.tally.cpu().numpy()
        return int(t[0]), int(t[1])


def indel_scan_host(read_words, read_mask, strand_words, fwd_words, rlen: int, tlen: int, strand: int, a: int, qa: int, K: int, G: int):
    """What a lane of ``k_node_indels`` makes of ONE match (``vs_indel_scan_host``, a pure host function: no device is
    needed).  Packed uint32 arrays with three zero words behind the last; ``read_mask``: ``None`` for an end without a byte
    outside ACGT.  -> ``(status, kind, L, u, w1)``: status 0 not tested, 1 tested without an event, 2 an event, 3 dropped."""
    out = np.zeros(4, dtype=np.uint64)
    rc = nat.lib().vs_indel_scan_host(read_words.ctypes.data, None if read_mask is None else read_mask.ctypes.data, strand_words.ctypes.data,
                                      fwd_words.ctypes.data, rlen, tlen, strand, a, qa, K, G, out.ctypes.data)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_indel_scan_host refuses a = %d of %d, qa = %d of %d, strand %d, K = %d, G = %d" % (a, rlen, qa, tlen, strand, K, G))
    return int(out[0]), int(out[1]) >> 8, int(out[1]) & 0xFF, int(out[2]), int(out[3])


class IndelCounter:
    """The insertions and deletions of at most ``max_len`` bases that the read ends carry against the segments, found on one
    device (``vs_node_indels``, ``tests/indel_model.py``): K = k + 1 exact bases on each side, every event written down once,
    left-aligned on the segment's forward text, with the strand it was seen on.  Takes ``PileupCounter``'s place in the input
    dispatch of ``pe_inference`` (``add``, ``device``, ``single_stats``, ``ends_seen``; the context keeps the masks): one
    kernel per block, a second launch when the block's events outgrow the buffer (``first_cap`` records to begin with).  The
    records of every block are merged on the device into a table of distinct records with their counts."""

    def __init__(self, ctx: Context, max_len: int = 16, first_cap: int = 4096, device: Optional[str] = None):
        import torch

        if not 1 <= int(max_len) <= 32:
            raise ValueError("a maximum indel length of %r: 1 to 32 are possible" % (max_len,))
        if int(first_cap) < 1:
            raise ValueError("a buffer of %r records: one or more are needed" % (first_cap,))
        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.ksize = ctx.ksize
        self.max_len = int(max_len)
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        self.launches = 0   # calls of vs_node_indels: one per block, two where the events did not fit
        self.node_rank = getattr(ctx, "node_rank", None)  # (kept here: a later build_index cannot change how the slots are read)
        with torch.cuda.device(self.device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.first = torch.zeros(self.n + 1, dtype=torch.int32, device=self.device)  # (uint32 words)
            self.slots = ctx.pileup_layout(self.first.data_ptr())
            self.events = torch.zeros((int(first_cap), 2), dtype=torch.int64, device=self.device)  # (uint64 words)
            self.keys = torch.zeros((0, 2), dtype=torch.int64, device=self.device)   # the distinct records so far
            self.counts = torch.zeros(0, dtype=torch.int64, device=self.device)
            self.tally = torch.zeros(4, dtype=torch.int64, device=self.device)
        ctx.keep_masks(True)

    def add(self, reads: ReadBlock):
        torch = self.torch
        n_ends = reads.info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        if not self.slots:
            return
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            args = (reads, self.first.data_ptr(), self.max_len)
            n = self.ctx.node_indels(*args, self.events.data_ptr(), self.events.shape[0], self.tally.data_ptr())
            self.launches += 1
            if n > self.events.shape[0]:  # the pass did not fit and tallied nothing: once more, with room
                self.events = torch.zeros((n, 2), dtype=torch.int64, device=self.device)
                self.launches += 1
                if self.ctx.node_indels(*args, self.events.data_ptr(), n, self.tally.data_ptr()) != n:
                    raise RuntimeError("vs_node_indels: the number of events changed between two calls on the same block")
            if n:
                keys, inverse = torch.unique(torch.cat((self.keys, self.events[:n])), dim=0, return_inverse=True)
                counts = torch.zeros(keys.shape[0], dtype=torch.int64, device=self.device)
                counts.index_add_(0, inverse, torch.cat((self.counts, torch.ones(n, dtype=torch.int64, device=self.device))))
                self.keys, self.counts = keys, counts

    def result(self):
        """-> a list of ``(seg, pos0, kind, length, insert, count_f, count_r)``: ``seg`` in the numbering of the node list
        ``Context.build_index`` was given (the GFA's), ``pos0`` the 0-based forward position of the first deleted base or of
        the base the insert stands before, ``kind`` 0 a deletion, 1 an insertion, ``insert`` the inserted bases on the forward
        strand (``""`` for a deletion), the counts those of the ends laid along the forward text and along its reverse
        complement.  Sorted by segment, position, kind, length, insert."""
        keys = self.keys.cpu().numpy().view(np.uint64).reshape(-1, 2)
        counts = self.counts.cpu().numpy()
        first = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
        order = None
        if self.node_rank is not None:
            order = np.empty(self.n, dtype=np.int64)
            order[np.asarray(self.node_rank, dtype=np.int64)] = np.arange(self.n, dtype=np.int64)
        table = {}
        for (w0, w1), c in zip(keys.tolist(), counts.tolist()):
            slot, plane, kind, length = w0 >> 8, w0 >> 7 & 1, w0 >> 6 & 1, (w0 & 63) + 1
            rank = int(np.searchsorted(first, slot, side="right")) - 1  # (the segment that holds the slot: one without slots holds none)
            seg = rank if order is None else int(order[rank])
            insert = "".join("ACGT"[w1 >> (2 * i) & 3] for i in range(length)) if kind else ""
            table.setdefault((seg, slot - int(first[rank]), kind, length, insert), [0, 0])[plane] += c
        return [key + tuple(v) for key, v in sorted(table.items())]

    def tallies(self):
        """-> (matches tested, deletions, insertions, insertions dropped for a byte outside ACGT)."""
        return tuple(int(v) for v in self.tally.cpu().numpy())


def site_pairs_plan(n_nodes: int, ksize: int, n_ends: int, max_len: int, n_cu: int = 256) -> dict:
    """The launch ``vs_node_site_pairs`` makes for a block (``vs_site_pairs_plan``, a pure host function: no device is
    needed): ``ends_per_wg`` is a multiple of 64, so that no workgroup and no batch of 64 ends cuts a pair.  An odd ``n_ends``
    is refused."""
    a = (C.c_uint64 * 8)()
    rc = nat.lib().vs_site_pairs_plan(n_nodes, ksize, n_ends, max_len, n_cu, a)
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_site_pairs_plan refuses %d nodes / %d ends of up to %d bases%s"
                              % (n_nodes, n_ends, max_len, ": fragments are the ends 2p and 2p + 1, an odd number of ends cuts one" if n_ends % 2 else ""))
    return dict(launch=bool(a[0]), grid=int(a[1]), ends_per_wg=int(a[2]), lds_bytes=int(a[6]), threads=int(a[7]))


def site_pairs_rows(seg, pos, span: int) -> Tuple[np.ndarray, int]:
    """The rows of the cell table (``vs_site_pairs_rows_host``, a pure host function): ``(seg[i], pos[i])`` are the sites,
    strictly ascending by segment, then position; site i's partners are the later sites of its segment at most ``span``
    positions behind it, contiguous behind it.  -> (row_first uint32 [n + 1], the number of cells): the cell of (s, t) is
    ``row_first[s] + (t - s - 1)``.  2^32 cells or more are refused: lower the span."""
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    pos = np.ascontiguousarray(pos, dtype=np.uint32)
    if seg.shape != pos.shape or seg.ndim != 1 or not 0 <= int(span) < 2 ** 32:
        raise ValueError("site_pairs_rows: two equally long lists and a span from 0 up are needed")
    row_first = np.zeros(len(seg) + 1, dtype=np.uint32)
    total = C.c_uint64(0)
    rc = nat.lib().vs_site_pairs_rows_host(seg.ctypes.data, pos.ctypes.data, len(seg), int(span), row_first.ctypes.data, C.byref(total))
    if rc == nat.VS_E_RANGE:
        raise nat.NativeError(rc, "%d sites within %d positions of each other make %s cells, and a cell number has 32 bits (a site number 29): lower the span"
                              % (len(seg), span, "2^32 or more" if total.value else "too many"))
    if rc != nat.VS_OK:
        raise nat.NativeError(rc, "vs_site_pairs_rows_host: the sites must ascend strictly by segment, then position")
    return row_first, int(total.value)


class SitePairCounter:
    """Which variant sites travel together on one read pair, counted on one device (``vs_node_site_pairs``): for every
    fragment -- the two mates of a pair, or one single read -- what the alignments the pileup would credit carry at the given
    ``sites`` is kept together, and every pair of sites of one segment at most ``max_span`` apart that the fragment saw adds
    1 to a 5 x 5 cell ``[base at the first][base at the second]`` (A, C, G, T, other; ``tests/site_pairs_model.py``).
    ``sites``: (segment index in the order ``Context.build_index`` was given, 0-based position); a site named twice is one.
    Takes ``PileupCounter``'s place in the input dispatch of ``pe_inference`` (``add``, ``device``, ``single_stats``,
    ``ends_seen``; the context keeps the masks): one kernel per block.  Holds 200 bytes per pair of sites within the span."""

    def __init__(self, ctx: Context, sites, max_mismatch: int = 8, max_span: int = 1000, device: Optional[str] = None):
        import torch

        if not 0 <= int(max_mismatch) < 2 ** 32:
            raise ValueError("a mismatch budget of %r: an integer from 0 up is needed" % (max_mismatch,))
        if not 0 <= int(max_span) < 2 ** 32:
            raise ValueError("a span of %r: an integer from 0 up is needed" % (max_span,))
        self.torch = torch
        self.ctx = ctx
        self.device = torch.device(device or ("cuda:%d" % ctx.device))
        self.n = ctx.n_nodes
        self.ksize = ctx.ksize
        self.max_mismatch = int(max_mismatch)
        self.max_span = int(max_span)
        self.single_stats = torch.zeros(3, dtype=torch.int64, device=self.device)  # (what the dispatch tallies of a PeCounter: stays zero)
        self.ends_seen = 0  # ends the blocks delivered (the absent second ends of singles blocks aside)
        node_rank = getattr(ctx, "node_rank", None)
        with torch.cuda.device(self.device):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.first = torch.zeros(self.n + 1, dtype=torch.int32, device=self.device)  # (uint32 words)
            ctx.pileup_layout(self.first.data_ptr())
            first = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
            given = np.array([(int(n), int(p)) for n, p in sites], dtype=np.int64).reshape(-1, 2)
            for n, p in given.tolist():
                if not 0 <= n < self.n:
                    raise ValueError("site (%d, %d): there is no segment %d among the %d of the index" % (n, p, n, self.n))
                r = n if node_rank is None else int(node_rank[n])
                if first[r + 1] == first[r]:
                    raise ValueError("site (%d, %d): segment %d is shorter than k + 1 = %d bases and has no positions" % (n, p, n, self.ksize + 1))
                if not 0 <= p < first[r + 1] - first[r] - 1:
                    raise ValueError("site (%d, %d): position %d is outside segment %d of %d bases" % (n, p, p, n, first[r + 1] - first[r] - 1))
            rank = given[:, 0] if node_rank is None else np.asarray(node_rank, dtype=np.int64)[given[:, 0]]
            slot = np.unique(first[rank] + given[:, 1])  # (ascending; one slot per site, so a site named twice is one)
            self.site_rank = np.searchsorted(first, slot, side="right") - 1  # the sites' segments, internal numbering
            self.site_pos = slot - first[self.site_rank]
            self.site_seg = self.site_rank if ctx.node_order is None else np.asarray(ctx.node_order, dtype=np.int64)[self.site_rank]
            self.n_sites = len(slot)
            self.row_first, self.n_cells = site_pairs_rows(self.site_rank, self.site_pos, self.max_span)
            self.site_slot = torch.from_numpy(slot.astype(np.uint32).view(np.int32)).to(self.device)
            self.d_row_first = torch.from_numpy(self.row_first.view(np.int32)).to(self.device)
            self.cells = torch.zeros((max(self.n_cells, 1), 25), dtype=torch.int64, device=self.device)
            self.tally = torch.zeros(5, dtype=torch.int64, device=self.device)
        ctx.keep_masks(True)

    def add(self, reads: ReadBlock):
        torch = self.torch
        n_ends = reads.info["ends"]
        self.ends_seen += n_ends // 2 if reads.unpaired else n_ends
        if not self.n_sites:
            return
        with torch.cuda.device(self.device):
            self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            self.ctx.node_site_pairs(reads, self.first.data_ptr(), self.site_slot.data_ptr(), self.n_sites, self.d_row_first.data_ptr(),
                                     self.cells.data_ptr(), self.max_mismatch, self.tally.data_ptr())

    def result(self):
        """-> (seg int64 [P], pos_a int64 [P], pos_b int64 [P], counts int64 [P, 5, 5]): every stored pair of sites with a
        non-zero cell; ``seg`` in the numbering of the node list ``Context.build_index`` was given (the GFA's), positions
        0-based, ``pos_a < pos_b``; ``counts[i, a, b]``: fragments that carry column ``a`` at ``pos_a`` and ``b`` at ``pos_b``
        (A, C, G, T, other).  Ordered by ``seg``, then ``pos_a``, then ``pos_b``."""
        cells = self.cells[: self.n_cells].cpu().numpy()
        at = np.flatnonzero(cells.any(axis=1))
        row_first = self.row_first.astype(np.int64)
        s = np.searchsorted(row_first, at, side="right") - 1  # (the row that holds the cell: an empty row holds none)
        t = s + 1 + at - row_first[s]
        seg, pos_a, pos_b = self.site_seg[s], self.site_pos[s], self.site_pos[t]
        order = np.lexsort((pos_b, pos_a, seg))
        return (seg[order].astype(np.int64), pos_a[order].astype(np.int64), pos_b[order].astype(np.int64),
                cells[at][order].astype(np.int64).reshape(len(at), 5, 5))

    def tallies(self):
        """-> (fragments with a raw observation, overflow fragments: more than 32 raw observations, nothing deposited,
        discordant (fragment, site) incidences, pairs stored, pairs unstored: on two segments or further apart than the span)."""
        return tuple(int(v) for v in self.tally.cpu().numpy())


# ---- outputs -------------------------------------------------------------------------------------
def _encode_ids(ids: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """The node names as the text writers take them: concatenated latin-1 bytes and their n + 1 offsets."""
    names = [s.encode("latin-1") for s in ids]
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    if names:
        off[1:] = np.cumsum([len(b) for b in names], dtype=np.uint64)
    return np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8), off


def write_matrix_text(path: str, ids: Sequence[str], mat: np.ndarray):
    """``{id_i}:{id_j}:{count}`` for all i, j in row-major order, zeros included
    (PE_Inference.py:194-205) -- N^2 lines, formatted by the library on all host cores."""
    blob, off = _encode_ids(ids)
    m = np.ascontiguousarray(mat, dtype=np.int64)
    rc = nat.lib().vs_write_matrix_text(None, path.encode(), blob.ctypes.data, off.ctypes.data, len(ids),
                                        m.ctypes.data if m.size else None)
    if rc != nat.VS_OK:
        raise OSError(nat.lib().vs_last_error(None).decode("utf-8", "replace"))
