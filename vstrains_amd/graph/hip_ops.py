"""Device side of the graph stages: ``ops.GraphOps`` / ``ops.PeLinks`` on top of the C ABI
(``include/vstrains_hip.h``, "graph stages").  No CPU path: constructing ``HipBackend`` without a
usable HIP device raises ``NativeError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _native as nat
from .asm_graph import AsmGraph
from .ops import GraphOps, GraphScan, PeLinks


def _ptr(a: np.ndarray):
    return a.ctypes.data if a.size else None


class HipGraphOps(GraphOps):
    """K6 + K7 called directly: one ``vs_graph_refresh`` call computes the flows and the scan of a graph snapshot.
    (The stages reach the same kernels from inside the library, through the native stage handle; this wrapper is for
    callers that hold an ``AsmGraph`` -- the kernel tests.)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.calls = 0

    #: the outputs of ``vs_graph_refresh``, in the order of its arguments
    OUTPUTS = ("flow", "nontrivial", "fork_kind", "chain_next", "chain_top", "chain_rank", "zero_sum_edge")

    def refresh_csr(self, row_ptr, n_out, nbr, eidx, dp, vertex_black, edge_black, n_edge_slots, outputs=OUTPUTS):
        """(testing aid) ``vs_graph_refresh`` on raw arrays, as the header describes them: the adjacency rows, dp, the
        colours and the number of edge slots are handed over as they are (an array given as ``None`` or empty goes as
        NULL), nothing is checked here.  Only the ``outputs`` asked for get a buffer, the others are passed as NULL.
        -> {name: array, or the int ``zero_sum_edge``}; raises ``NativeError`` with the library's code."""
        nv = len(n_out) if n_out is not None else len(row_ptr) - 1
        unknown = set(outputs) - set(self.OUTPUTS)
        if unknown:
            raise ValueError("unknown outputs %s" % sorted(unknown))

        def given(a, dtype):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype)

        ins = [given(row_ptr, np.uint64), given(n_out, np.uint32), given(nbr, np.uint32), given(eidx, np.uint32),
               given(dp, np.float64), given(vertex_black, np.uint8), given(edge_black, np.uint8)]
        got = {}
        if "flow" in outputs:
            got["flow"] = np.zeros(max(n_edge_slots, 1), dtype=np.float64)
        for name, dtype, fill in (("nontrivial", np.uint8, 0), ("fork_kind", np.uint8, 0), ("chain_next", np.int32, -1),
                                  ("chain_top", np.int32, 0), ("chain_rank", np.int32, 0)):
            if name in outputs:
                got[name] = np.full(max(nv, 1), fill, dtype=dtype)
        bad = C.c_uint32(0xFFFFFFFF)
        outs = [got[name].ctypes.data if name in got else None for name in self.OUTPUTS[:-1]]
        nat.check(self.ctx._h, nat.lib().vs_graph_refresh(
            self.ctx._h, nv, n_edge_slots, *[None if a is None else _ptr(a) for a in ins], *outs,
            C.byref(bad) if "zero_sum_edge" in outputs else None))
        self.calls += 1
        if "zero_sum_edge" in outputs:
            got["zero_sum_edge"] = bad.value
        return got

    def _refresh(self, g: AsmGraph):
        row_ptr, n_out, nbr, eidx = g.csr_arrays()
        n_slots = len(g.esrc)
        got = self.refresh_csr(row_ptr, n_out, nbr, eidx, g.vdp, g.vblack, g.eblack if n_slots else [0], n_slots)
        return tuple(got[name] for name in self.OUTPUTS)

    @staticmethod
    def _apply_flows(g: AsmGraph, flow, bad) -> None:
        if bad != 0xFFFFFFFF:
            # numpy.seterr(all="raise") in the reference's main process (vstrains:25)
            raise FloatingPointError("divide by zero encountered in edge flow of edge %s -> %s"
                                     % (g.vid[g.esrc[bad]], g.vid[g.etgt[bad]]))
        vals = flow.tolist()
        for e in g.edges():
            g.eflow[e] = vals[e]

    @staticmethod
    def _as_scan(g: AsmGraph, nt, fk, nxt, top, rank) -> GraphScan:
        nv = g.num_vertices()
        return GraphScan(nt[:nv].astype(bool).tolist(), fk[:nv].tolist(), nxt[:nv].tolist(), top[:nv].tolist(),
                         rank[:nv].tolist())

    def edge_flows(self, g: AsmGraph) -> None:
        flow, _, _, _, _, _, bad = self._refresh(g)
        self._apply_flows(g, flow, bad)

    def scan(self, g: AsmGraph) -> GraphScan:
        _, nt, fk, nxt, top, rank, _ = self._refresh(g)
        return self._as_scan(g, nt, fk, nxt, top, rank)

    def refresh(self, g: AsmGraph) -> GraphScan:
        flow, nt, fk, nxt, top, rank, bad = self._refresh(g)
        self._apply_flows(g, flow, bad)
        return self._as_scan(g, nt, fk, nxt, top, rank)


class HipPeLinks(PeLinks):
    """K5: the symmetrised PE-link matrix, resident in HBM."""

    def __init__(self, ctx, handle, names: Sequence[str], caller_names: Optional[Sequence[str]] = None):
        """``names``: row i of the device table belongs to names[i]; ``caller_names``: the same names in the order the
        caller knows them (``to_numpy`` answers in that order), when the two differ."""
        self.ctx = ctx
        self._h = handle
        self.names = list(names)
        self._index = {n: i for i, n in enumerate(self.names)}
        self._caller_rows = None if caller_names is None else np.asarray([self._index[n] for n in caller_names], dtype=np.int64)
        self.calls = 0

    @classmethod
    def from_counter(cls, ctx, counter, names: Sequence[str], sparse_min_nodes: int = 0):
        """``counter``: ``pe.PeCounter`` whose [2,N,N] int32 tensor ``vs_pe_count`` filled.  ``sparse_min_nodes``: from how
        many nodes a counter with a dirty-tile map gives a CSR table (0: the library's default, 32 768; tests pass 64)."""
        n = len(names)
        assert counter.n == n
        counter.torch.cuda.synchronize(counter.device)
        h = C.c_void_p()
        if getattr(counter, "wide", None) is not None:  # int64 totals exist: everything goes there first
            counter.fold()
            counter.torch.cuda.synchronize(counter.device)
            nat.check(ctx._h, nat.lib().vs_links_from_wide(ctx._h, C.c_void_p(counter.wide[0].data_ptr()),
                                                           C.c_void_p(counter.wide[1].data_ptr()), n, C.byref(h)))
        elif getattr(counter, "tile_map", None) is not None:
            # (ABI 10) counters that keep a dirty-tile map: from 32 768 nodes on the table is built from the marked tiles
            # only and held as CSR rows of its non-zero cells (0.4 GB instead of 23.7 GB at 54 465 nodes)
            nat.check(ctx._h, nat.lib().vs_links_from_counts_tracked(ctx._h, C.c_void_p(counter.mats[0].data_ptr()),
                                                                     C.c_void_p(counter.mats[1].data_ptr()), n,
                                                                     C.c_void_p(counter.tile_map.data_ptr()), sparse_min_nodes, C.byref(h)))
        else:
            nat.check(ctx._h, nat.lib().vs_links_from_counts(ctx._h, C.c_void_p(counter.mats[0].data_ptr()),
                                                             C.c_void_p(counter.mats[1].data_ptr()), n, C.byref(h)))
        ctx.sync()
        # (the counters are in the numbering the index was built in -- pe.Context.build_index -- and so is the table
        # made from them: rows are found by name, so only the name list has to follow)
        order = getattr(counter, "node_order", None)  # (the numbering of the index it counted under)
        if order is not None:
            return cls(ctx, h, [names[i] for i in order.tolist()], caller_names=names)
        return cls(ctx, h, names)

    @classmethod
    def from_matrices(cls, ctx, names: Sequence[str], node_mat, short_mat):
        n = len(names)
        a = np.ascontiguousarray(node_mat, dtype=np.int64).reshape(n, n)
        b = np.ascontiguousarray(short_mat, dtype=np.int64).reshape(n, n)
        h = C.c_void_p()
        nat.check(ctx._h, nat.lib().vs_links_from_host(ctx._h, _ptr(a), _ptr(b), n, C.byref(h)))
        return cls(ctx, h, names)

    #: what the last ``from_files`` read: {"pe": {...}, "st": {...}} with the route ("bgzf_device", "plain_device", "host";
    #: "python" when the files went to the Python loop), lines, skipped, cells, members_device, text_bytes, windows, flags
    last_read: Optional[Dict[str, Dict[str, object]]] = None
    _ROUTES = {0: "none", 1: "bgzf_device", 2: "plain_device", 3: "host"}

    @classmethod
    def from_files(cls, ctx, names: Sequence[str], pe_file: str, st_file: str, sparse_min_nodes: int = 0,
                   device_parse: bool = True, window_bytes: int = 0):
        """The reference's own hand-off (IO.py:603-623): the two text files, dense (N^2 lines) or sparse (the lines of
        non-zero count only), plain or gzip / BGZF (``pe_info.gz``).

        ``device_parse=True`` (``vs_links_from_info``): the files are read where the table lives.  A file that is BGZF from
        end to end is uploaded compressed and inflated on the device, a plain file is uploaded as it is; windows of
        ``window_bytes`` of text (0: 256 MB) are scanned and parsed by kernels and the counts are added straight into the
        table (dense below ``sparse_min_nodes`` nodes -- 0: the library's 32 768 --, CSR rows from there on).  Any other gzip
        file, a line longer than a window and every error take the host reader.  It is the default for every file kind;
        the legs of ``tools/info_read_legs.py`` that are to confirm it have NOT been measured yet (profiles/info_read.md):
        a file kind whose device leg does not beat its host leg there is to go back to the host route by default.

        ``device_parse=False``: the library parses on the host threads (``vs_info_parse``, gzip inflated by zlib on one
        thread) and builds the table from the cells (``vs_links_from_cells``).

        Either way a file that holds a carriage return or a byte outside ASCII is left to Python's text mode, the loop over
        ``formats.read_pe_text``.  ``HipPeLinks.last_read`` says which route each file took."""
        names = list(names)
        if device_parse:
            got = cls._from_files_device(ctx, names, pe_file, st_file, sparse_min_nodes, window_bytes)
            if got is None:
                HipPeLinks.last_read = {"pe": {"route": "python"}, "st": {"route": "python"}}
                return cls._from_files_python(ctx, names, pe_file, st_file)
            return got
        cells = []
        for path in (pe_file, st_file):
            got = cls._parse_cells(names, path)
            if got is None:
                HipPeLinks.last_read = {"pe": {"route": "python"}, "st": {"route": "python"}}
                return cls._from_files_python(ctx, names, pe_file, st_file)
            cells.append(got)
        rows = np.concatenate([c[0] for c in cells])
        cols = np.concatenate([c[1] for c in cells])
        vals = np.concatenate([c[2] for c in cells])
        h = C.c_void_p()
        nat.check(ctx._h, nat.lib().vs_links_from_cells(ctx._h, _ptr(rows), _ptr(cols), _ptr(vals), rows.size, len(names),
                                                        sparse_min_nodes, C.byref(h)))
        HipPeLinks.last_read = {"pe": {"route": "host", "cells": int(cells[0][0].size)},
                                "st": {"route": "host", "cells": int(cells[1][0].size)}}
        return cls(ctx, h, names)

    @classmethod
    def _from_files_device(cls, ctx, names: Sequence[str], pe_file: str, st_file: str, sparse_min_nodes: int, window_bytes: int):
        """``vs_links_from_info``: the table, or None when the files are Python's to read (a carriage return, a byte outside
        ASCII, a name the library cannot be handed as bytes)."""
        try:
            enc = [s.encode("ascii") for s in names]
        except UnicodeEncodeError:
            return None
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        info = (C.c_uint64 * 16)()
        h = C.c_void_p()
        rc = nat.lib().vs_links_from_info(ctx._h, pe_file.encode(), st_file.encode(), blob.ctypes.data, off.ctypes.data, len(enc),
                                          sparse_min_nodes, window_bytes, C.byref(h), info)
        if rc != nat.VS_OK:
            msg = (nat.lib().vs_last_error(ctx._h) or b"?").decode("utf-8", "replace")
            if rc == nat.VS_E_ARG and "cannot open" in msg:
                raise FileNotFoundError(msg)
            if rc == nat.VS_E_ARG:
                raise ValueError(msg)  # (a malformed line, a corrupt gzip stream: what the host route raises)
            raise nat.NativeError(rc, msg)
        keys = ("route", "lines", "skipped", "cells", "members_device", "text_bytes", "windows", "flags")
        read = {}
        for f, tag in enumerate(("pe", "st")):
            rec = {k: int(info[8 * f + i]) for i, k in enumerate(keys)}
            rec["route"] = cls._ROUTES.get(rec["route"], "none")
            read[tag] = rec
        if not h.value:
            return None
        HipPeLinks.last_read = read
        table = cls(ctx, h, names)
        table.read_info = read
        return table

    @staticmethod
    def _parse_cells(names: Sequence[str], path: str):
        """``vs_info_parse`` of one file: (rows uint32, cols uint32, vals int64), or None when the file is Python's to read
        (a carriage return, a byte outside ASCII, a name the library cannot be handed as bytes)."""
        try:
            enc = [s.encode("ascii") for s in names]
        except UnicodeEncodeError:
            return None
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        info = (C.c_uint64 * 4)()

        def call(rows, cols, vals, cap):
            rc = nat.lib().vs_info_parse(path.encode(), blob.ctypes.data, off.ctypes.data, len(enc), rows, cols, vals, cap, info)
            if rc != nat.VS_OK:
                msg = (nat.lib().vs_last_error(None) or b"?").decode("utf-8", "replace")
                if "cannot open" in msg:
                    raise FileNotFoundError(msg)
                raise ValueError(msg)  # (a malformed line: what the unpacking / int() of the Python loop raises)

        call(None, None, None, 0)
        if int(info[1]):
            return None
        cap = int(info[0])
        rows = np.zeros(max(cap, 1), dtype=np.uint32)
        cols = np.zeros(max(cap, 1), dtype=np.uint32)
        vals = np.zeros(max(cap, 1), dtype=np.int64)
        if cap:
            call(rows.ctypes.data, cols.ctypes.data, vals.ctypes.data, cap)
            cap = int(info[0])
        return rows[:cap], cols[:cap], vals[:cap]

    @classmethod
    def _from_files_python(cls, ctx, names: Sequence[str], pe_file: str, st_file: str):
        from .formats import read_pe_text

        index = {n: i for i, n in enumerate(names)}
        mats = []
        for path in (pe_file, st_file):
            m = np.zeros((len(names), len(names)), dtype=np.int64)
            for u, v, c in read_pe_text(path):
                if u in index and v in index:
                    m[index[u], index[v]] += c
            mats.append(m)
        return cls.from_matrices(ctx, names, mats[0], mats[1])

    def close(self):
        if self._h:
            nat.lib().vs_links_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def index_of(self, name: str) -> int:
        return self._index[name]

    def to_numpy(self) -> np.ndarray:
        n = len(self.names)
        out = np.zeros((max(n, 1), max(n, 1)), dtype=np.int64)
        if n:
            nat.check(self.ctx._h, nat.lib().vs_links_to_host(self.ctx._h, self._h, out.ctypes.data))
        out = out[:n, :n]
        if self._caller_rows is not None:
            out = out[np.ix_(self._caller_rows, self._caller_rows)]
        return out

    def csr(self):
        """(testing aid, ``vs_links_export_csr``) The rows of a CSR table as the device holds them, in the table's own
        numbering: (row_ptr uint32 [n + 1], col uint32 [nnz], val int64 [nnz], nnz as the table records it).  A dense table
        raises ``NativeError`` (VS_E_ARG)."""
        L, h = nat.lib(), self.ctx._h
        nnz = C.c_uint64(0)
        row_ptr = np.zeros(len(self.names) + 1, dtype=np.uint32)
        nat.check(h, L.vs_links_export_csr(h, self._h, row_ptr.ctypes.data, None, None, 0, C.byref(nnz)))
        col = np.zeros(max(nnz.value, 1), dtype=np.uint32)
        val = np.zeros(max(nnz.value, 1), dtype=np.int64)
        nat.check(h, L.vs_links_export_csr(h, self._h, None, col.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz)))
        return row_ptr, col[:nnz.value], val[:nnz.value], int(nnz.value)

    @staticmethod
    def _pool(lists: Sequence[Sequence[int]]):
        ids: Dict[Tuple[int, ...], int] = {}
        order: List[Tuple[int, ...]] = []
        which = []
        for l in lists:
            t = tuple(l)
            k = ids.get(t)
            if k is None:
                k = ids[t] = len(order)
                order.append(t)
            which.append(k)
        off = np.zeros(len(order) + 1, dtype=np.uint64)
        if order:
            off[1:] = np.cumsum([len(t) for t in order], dtype=np.uint64)
        flat = np.asarray([x for t in order for x in t], dtype=np.uint32)
        return off, flat, which, len(order)

    def block_sums(self, queries):
        if not queries:
            return []
        lists = []
        for rows, cols in queries:
            lists.append(rows)
            lists.append(cols)
        off, flat, which, n_lists = self._pool(lists)
        qa = np.asarray(which[0::2], dtype=np.uint32)
        qb = np.asarray(which[1::2], dtype=np.uint32)
        out = np.zeros(len(queries), dtype=np.int64)
        nat.check(self.ctx._h, nat.lib().vs_links_block_sums(self.ctx._h, self._h, off.ctypes.data, _ptr(flat), n_lists,
                                                             qa.ctypes.data, qb.ctypes.data, len(queries),
                                                             out.ctypes.data))
        self.calls += 1
        return out.tolist()

    def group_matrix(self, groups):
        n = len(groups)
        out = np.zeros((max(n, 1), max(n, 1)), dtype=np.int64)
        if n == 0:
            return out[:0, :0]
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(gp) for gp in groups], dtype=np.uint64)
        flat = np.asarray([x for gp in groups for x in gp], dtype=np.uint32)
        out = np.zeros((n, n), dtype=np.int64)
        nat.check(self.ctx._h, nat.lib().vs_links_group_matrix(self.ctx._h, self._h, off.ctypes.data, _ptr(flat), n,
                                                               out.ctypes.data))
        self.calls += 1
        return out


class HipBackend:
    """What ``pipeline.run`` needs from the device: PE-link inference + the graph kernels."""

    def __init__(self, device: int = 0, write_info_text: bool = True, ctx=None, sparse_info_text: bool = False,
                 bgzf_info_text: bool = False, bam_by_name: bool = False, interleaved=None, check_names=None, single=(),
                 count_singles: bool = False, interleaved_shard: bool = False):
        from .. import pe as host

        self.ctx = ctx if ctx is not None else host.Context(device)  # raises NativeError without a HIP device
        self.graph_ops = HipGraphOps(self.ctx)
        self.write_info_text = write_info_text
        self.sparse_info_text = sparse_info_text  # pe_info / st_info with the lines of non-zero count only
        self.bgzf_info_text = bgzf_info_text  # pe_info.gz / st_info.gz: BGZF deflated on the device
        self.bam_by_name = bam_by_name  # -fwd / -rve name ONE BAM in any record order: mates matched by name
        self.bam_info = None  # the by-name stream's info (singletons dropped, ...) after pe_links
        self.interleaved = interleaved  # "strict" / "singles": -fwd / -rve name ONE interleaved FASTQ, mates checked by name
        self.interleaved_shard = interleaved_shard  # --interleaved-shard: under a process group the ranks share that file by member
        self.interleaved_info = None  # that stream's info (singles dropped, ...) after pe_links
        self.check_names = check_names  # "strict" / "singles": the two FASTQ files are paired by read name on the device
        self.pair_names_info = None  # that stream's info (singles dropped per file, ...) after pe_links
        self.single = list(single)  # files of unpaired reads, counted into the same counters after the pairs
        self.count_singles = count_singles  # --count-singles: the records without a mate are counted instead of dropped
        self.single_info = []  # per file of unpaired reads: what it added (pe_inference.count_links.single_info) after pe_links
        self.pe_stats = None

    def pe_links(self, gfa: str, aln_dir: str, fwd: str, rve: str, ksize: int, names: List[str]) -> HipPeLinks:
        """Boundary 1 (VStrains_SPAdes.py:119-138) without the process hop: count on the device,
        write ``pe_info`` / ``st_info`` for drop-in compatibility, and keep the counters in HBM as
        the link table instead of re-parsing N^2 text lines into a dict."""
        from .. import pe_inference

        print("----------------------Paired-End Information Alignment----------------------")
        if self.write_info_text:
            self.pe_stats = pe_inference.run(gfa, aln_dir, fwd, rve, ksize, ctx=self.ctx, stages_follow=True,
                                              sparse_info=self.sparse_info_text, bgzf_info=self.bgzf_info_text, bam_by_name=self.bam_by_name,
                                              interleaved=self.interleaved, check_names=self.check_names, single=self.single,
                                              count_singles=self.count_singles, interleaved_shard=self.interleaved_shard)
            ids, counter = pe_inference.run.last
        else:
            os.makedirs(aln_dir, exist_ok=True)
            ids, counter = pe_inference.count_links(self.ctx, gfa, fwd, rve, ksize, stages_follow=True, bam_by_name=self.bam_by_name,
                                                    interleaved=self.interleaved, check_names=self.check_names, single=self.single,
                                                    count_singles=self.count_singles, interleaved_shard=self.interleaved_shard)
        self.single_info = pe_inference.count_links.single_info
        self.bam_info = pe_inference.count_links.bam_info
        self.interleaved_info = pe_inference.count_links.interleaved_info
        self.pair_names_info = pe_inference.count_links.pair_names_info
        if list(ids) != list(names):
            raise RuntimeError("node order of %s differs from the stage graph" % gfa)
        return HipPeLinks.from_counter(self.ctx, counter, names)

    def links_from_files(self, names: Sequence[str], pe_file: str, st_file: str) -> HipPeLinks:
        """``process_pe_info`` (IO.py:598-627) from the two text files, table resident on the device."""
        return HipPeLinks.from_files(self.ctx, list(names), pe_file, st_file)

    def native_stage(self, table: HipPeLinks):
        """The stage graph in the library (``vs_stage``): what ``pipeline.extract_strains`` runs on."""
        from .native_stage import NativeStage

        return NativeStage.on_device(self.ctx, table, table.names)
