"""Multi-GPU plan for PE-link inference: read pairs are independent and the only shared state
is the two N x N counters (reference utils/VStrains_PE_Inference.py:139-140,174-188), so the
pairs are cut into contiguous blocks, one per rank, every rank holds its own copy of the node
index, and one sum all-reduce (RCCL over xGMI when the backend is "nccl") folds the counters.
Integer addition commutes: any partition gives bit-identical results."""
from __future__ import annotations

import time
from typing import Tuple


def shard_range(n_pairs: int, rank: int, world: int) -> Tuple[int, int]:
    """Pair r goes to rank floor(r * world / n_pairs): contiguous, sizes differ by at most one."""
    lo = (n_pairs * rank) // world
    hi = (n_pairs * (rank + 1)) // world
    return lo, hi


def group_size() -> int:
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


# ---- exchange of the occupied stretches only -----------------------------------------------------------------------
# The counters are mostly zero (a pair of 2x150 bp touches a dozen nodes that lie next to each other in the index's path
# numbering, so the non-zero cells of [2,N,N] sit in short runs along a band) and every rank's non-zero cells lie in
# about the SAME places (reads are sharded at random over the same genomes).  So the ranks first OR their occupancy maps
# of 64-cell stretches (256 bytes of uint32 counters: one small all-reduce), gather the occupied stretches of the UNION
# into a dense [U, 64] tensor, all-reduce THAT with the ordinary ring, and scatter the sums back.  What moves is
# U * 256 bytes through the ring instead of the whole buffer; the decision compact / dense follows from U, which every
# rank knows after the first all-reduce, so no rank can take another branch than its peers.
STRETCH = 64          # counter cells per stretch
COMPACT_MAX_FILL = 0.5  # above this share of occupied stretches the dense ring is no worse


def strong_share(total_pairs: int, rank: int, world: int) -> Tuple[int, int]:
    """Strong scaling: the job's pairs are fixed and rank r takes pairs [lo, hi) of them (``shard_range``)."""
    return shard_range(total_pairs, rank, world)


def _occupancy(head):
    """uint8 [M]: 1 where a 64-cell stretch of ``head`` ([M, 64]) holds a non-zero cell (slabs bound the temporaries)."""
    import torch

    m = head.shape[0]
    occ = torch.empty(m, dtype=torch.uint8, device=head.device)
    slab = 1 << 22  # stretches per slab: 1 GiB of int32 cells
    for lo in range(0, m, slab):
        occ[lo:lo + slab] = (head[lo:lo + slab] != 0).any(dim=1)
    return occ


def _occupancy_from_tiles(tile_map, n: int, m: int):
    """The same map from a counter's dirty-tile bytes (``PeCounter.tile_map``: one byte per 64 x 64 tile of node_mat, then
    of short_mat, set wherever a block added to a cell): stretch j of the flat [2, n, n] buffer is taken as occupied when
    any tile it overlaps is marked -- a superset of the non-zero stretches, found without reading the 23.7 GB of counters a
    54 k-node graph has.  A stretch is 64 consecutive cells of the flat buffer: it lies in one or two matrix rows and
    in one or two tile columns of each."""
    import torch

    T = (n + 63) // 64
    dev = tile_map.device
    first = torch.arange(m, dtype=torch.int64, device=dev) * STRETCH
    last = first + (STRETCH - 1)
    # A stretch (64 <= n cells) lies in one matrix row or in the end of one and the start of the next; each part is shorter
    # than a tile is wide, so it overlaps at most two tile columns: those of its first and of its last cell.  Four cells
    # name every tile: the stretch's first and last, the last cell of the first row, the first cell of the last row.
    row_end = torch.minimum(last, (first // n + 1) * n - 1)
    row_start = torch.maximum(first, (last // n) * n)
    occ = torch.zeros(m, dtype=torch.uint8, device=dev)
    for cell in (first, row_end, row_start, last):
        grow = cell // n  # row of the flat [2 n, n] buffer
        col = cell - grow * n
        mat = grow // n
        row = grow - mat * n
        occ |= tile_map[(mat * T + (row >> 6)) * T + (col >> 6)]
    return occ


# ---- the packed exchange: two collectives per sum ---------------------------------------------------------------------
#   C1  MAX over ONE uint8 tensor: [occupancy map of the 64-cell stretches (or the counter's dirty-tile map, from which
#       every rank derives the same occupancy) | FLAG_BYTES flag bytes].  MAX over bytes is OR for 0 / 1 flags.
#   C2  SUM over ONE staging tensor: [the occupied stretches of the union | one row that carries the caller's small int64
#       sums -- the three stats, the pairs in the buffers -- as 16-bit limbs in the cells' dtype | the leftover cells].
# A rank that issued a differently shaped collective than its peers would hang the group or sum garbage, so the exchange
# is agree -> plan -> execute: everything a rank allocates is taken before C1 (a failure becomes a flag), and every
# decision after C1 is a function of values every rank holds -- the number of stretches m (same N), the agreed flag bytes
# and the union's size u.  A union of more than ``slab_rows(m)`` stretches takes one SUM per slab; a dense union, a veto or
# a rank without staging memory send the whole tensor through the ring, and the tail row after it.
FLAG_BYTES = 8
FLAG_NO_COMPACT, FLAG_WIDE, FLAG_NO_STAGING, FLAG_PAIRS_LOG2 = 0, 1, 2, 3
LIMBS = 4  # 16-bit limbs per int64 of the tail: exact while every addend is below 2^63 and there are fewer than 2^15 ranks
U32_LIMIT = 2 ** 32


def flag_bytes(no_compact: bool = False, wide: bool = False, pairs: int = 0):
    """One rank's flag bytes (uint8 [FLAG_BYTES]): it vetoes the compact form, it holds int64 totals, and its pairs in the
    buffers as (bit length, top eight bits) -- MAX over the bytes bounds the largest rank's pairs from above."""
    import torch

    fl = torch.zeros(FLAG_BYTES, dtype=torch.uint8)
    fl[FLAG_NO_COMPACT] = 1 if no_compact else 0
    fl[FLAG_WIDE] = 1 if wide else 0
    bits = int(pairs).bit_length()
    fl[FLAG_PAIRS_LOG2] = bits
    fl[FLAG_PAIRS_LOG2 + 1] = (pairs >> (bits - 8)) if bits > 8 else pairs
    return fl


def must_fold(fl, world: int) -> bool:
    """From the agreed flag bytes (a list): some rank holds int64 totals, or uint32 cells cannot hold the sum -- a cell grows
    by at most 2 per pair, and the bound on the largest rank's pairs times the ranks says how many pairs there may be."""
    bits, top = int(fl[FLAG_PAIRS_LOG2]), int(fl[FLAG_PAIRS_LOG2 + 1])
    bound = ((top + 1) << (bits - 8)) if bits > 8 else 255
    return bool(fl[FLAG_WIDE]) or 2 * bound * world >= U32_LIMIT


# One staging buffer per (device, dtype), grown only: the exchange walks the occupied stretches in slabs of at most
# SLAB_STRETCHES, so its transient is bounded (1 GB of int32 cells) whatever the union's size.  
SLAB_STRETCHES = 1 << 22
_staging = {}


def slab_rows(m: int) -> int:
    """Stretches per SUM for a counter of ``m`` stretches: a compact union (u <= m / 2) fits in one slab while m / 2 <=
    SLAB_STRETCHES.  A function of m alone, so every rank cuts the union alike."""
    return min(m // 2 + 1, SLAB_STRETCHES)


def _staging_buffer(head, rows: int):
    """At least ``rows`` rows of 64 cells of ``head``'s dtype on its device; None when the allocation fails (the caller
    says so in its flag bytes, before the first collective: no rank is left waiting)."""
    import torch

    key = (str(head.device), head.dtype)
    buf = _staging.get(key)
    if buf is not None and buf.shape[0] >= rows:
        return buf
    try:
        buf = torch.empty((rows, STRETCH), dtype=head.dtype, device=head.device)
    except (RuntimeError, MemoryError):  # (torch.cuda.OutOfMemoryError is a RuntimeError)
        return None
    _staging[key] = buf
    return buf


def _tail_encode(tail, row):
    """``tail`` (int64 [k], k <= 16, non-negative) into ``row`` ([64] of the cells' dtype): int64 cells take the values as
    they are, int32 cells four 16-bit limbs each (a sum over ranks of limbs stays far below 2^31)."""
    import torch

    row.zero_()
    k = tail.numel()
    if row.dtype == torch.int64:
        row[:k] = tail
    else:
        shifts = torch.arange(0, 16 * LIMBS, 16, dtype=torch.int64, device=tail.device).unsqueeze(1)
        row.view(LIMBS, 16)[:, :k] = ((tail.to(torch.int64).unsqueeze(0) >> shifts) & 0xFFFF).to(row.dtype)


def _tail_decode(row, k):
    import torch

    if row.dtype == torch.int64:
        return row[:k].clone()
    shifts = torch.arange(0, 16 * LIMBS, 16, dtype=torch.int64, device=row.device).unsqueeze(1)
    return (row.view(LIMBS, 16)[:, :k].to(torch.int64) << shifts).sum(dim=0)


class ExchangeState:
    """What a counter keeps between its exchanges: ``cap``, the union size the next predicted exchange is staged for (1.25
    times the last one's, learnt only from an exchange on which every rank held its staging buffer -- the cache keeps it),
    the predicted exchange that is not settled yet, and the collectives and host waits of the most recent call."""

    def __init__(self):
        self.cap = None
        self.pending = None
        self.collectives = 0
        self.host_waits = 0


class Exchange:
    """One sum over the ranks of a counter tensor (int32 storage of uint32 cells, or int64 totals), of ``tail`` (small int64
    tensor) and OR of ``flags`` (uint8 [FLAG_BYTES]), from C1 on.  Made by ``agree``; then ``read`` + ``sum``, or
    ``sum_predicted`` + ``settle``."""

    def __init__(self, mats, tail, flags, tile_map, timing, occupancy_fn, state):
        import torch

        self.mats, self.timing, self.state = mats, timing, state
        dev = mats.device
        flat = mats.view(-1)
        self.m = m = flat.numel() // STRETCH
        self.head = flat[: m * STRETCH].view(m, STRETCH)
        self.left = flat[m * STRETCH:]  # the cells behind the last whole stretch (fewer than 64): they ride in a row of their own
        self.rows = slab_rows(m)
        self.k_tail = 0 if tail is None else int(tail.numel())
        assert self.k_tail <= 16
        mine = torch.zeros(FLAG_BYTES, dtype=torch.uint8, device=dev) if flags is None else flags.to(device=dev, dtype=torch.uint8).clone()
        t = time.perf_counter()
        # everything this rank needs BEFORE the first collective: the staging buffer (or a flag that it has none), and the two
        # rows behind the stretches -- the tail's limbs and the leftover cells
        self.buf = _staging_buffer(self.head, self.rows + 2) if m else None
        if m and self.buf is None:
            mine[FLAG_NO_STAGING] = 1
        self.extra = torch.zeros((2, STRETCH), dtype=mats.dtype, device=dev)
        if self.k_tail:
            _tail_encode(tail, self.extra[0])
        self.extra[1][: self.left.numel()] = self.left
        # C1 = [occupancy map (unless the tile map stands for it) | the counter's dirty-tile map, if it keeps one | flag bytes]
        n = mats.shape[-1]
        use_tiles = tile_map is not None and mats.dim() == 3 and mats.shape[0] == 2 and mats.shape[1] == n and n >= STRETCH
        occ_local = None if use_tiles else ((occupancy_fn(self.head) if occupancy_fn is not None else _occupancy(self.head)) if m
                                            else torch.zeros(0, dtype=torch.uint8, device=dev))
        n_occ = 0 if occ_local is None else occ_local.numel()
        n_tiles = 0 if tile_map is None else tile_map.numel()
        nb = n_occ + n_tiles
        c1 = torch.empty(nb + FLAG_BYTES, dtype=torch.uint8, device=dev)
        if n_occ:
            c1[:n_occ] = occ_local
        if n_tiles:
            c1[n_occ:nb] = tile_map
        c1[nb:] = mine
        t = self._mark("occupancy", t)
        self._reduce(c1, "MAX")
        self._t = self._mark("occupancy_allreduce", t)
        self.flags = c1[nb:]
        if n_tiles:
            tile_map.copy_(c1[n_occ:nb])  # (the sum brings the other ranks' cells: their tiles are dirty here too)
        self.occ = _occupancy_from_tiles(tile_map, n, m) if use_tiles else c1[:n_occ]

    def _mark(self, name, t0):
        import torch

        if self.timing is not None:
            if self.mats.is_cuda:
                torch.cuda.synchronize(self.mats.device)
            self.timing[name] = self.timing.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def _reduce(self, t, op="SUM"):
        import torch.distributed as dist

        self.state.collectives += 1
        dist.all_reduce(t, op=getattr(dist.ReduceOp, op))

    def read(self):
        """One host wait: the agreed flag bytes (a list) and the union's size."""
        import torch

        word = torch.cat([self.flags.to(torch.int64), self.occ.sum(dtype=torch.int64).view(1)]).cpu()
        self.state.host_waits += 1
        fl, u = word[:FLAG_BYTES].tolist(), int(word[FLAG_BYTES])
        self._t = self._mark("nonzero", self._t)
        if self.timing is not None:
            self.timing["stretches"] = self.m
            self.timing["occupied_stretches_of_the_union"] = u
        return fl, u

    def sum(self, fl, u):
        """C2 from the agreed ``fl`` and ``u``: -> (how, summed tail or None); how is "compact" or "dense"."""
        import torch

        if not fl[FLAG_NO_STAGING]:
            self.state.cap = max(64, int(1.25 * u) + 16)
        if self.m == 0 or fl[FLAG_NO_COMPACT] or fl[FLAG_NO_STAGING] or u > COMPACT_MAX_FILL * self.m:
            t = time.perf_counter()
            self._reduce(self.mats)
            if self.k_tail:
                self._reduce(self.extra[0])
            self._mark("ring", t)
            return "dense", (_tail_decode(self.extra[0], self.k_tail) if self.k_tail else None)
        idx = torch.nonzero_static(self.occ, size=u, fill_value=0).view(-1)
        return "compact", self._sum_slabs(idx, u, extra=True)

    def sum_predicted(self):
        """C2 sized from ``state.cap`` instead of the union (no host wait): the first min(cap, slab) stretches of the union;
        ``settle`` sums the rest.  -> the summed tail."""
        import torch

        if self.m == 0:
            return self.sum(*self.read())[1]
        cap = min(self.state.cap, self.rows)
        idx = torch.nonzero_static(self.occ, size=cap, fill_value=0).view(-1)
        out = self._sum_slabs(idx, cap, extra=True)
        self.cap = cap
        self.state.pending = self
        return out

    def _sum_slabs(self, idx, n, extra):
        """Sum the stretches ``head[idx]`` (n of them) over the ranks through the staging buffer, ``rows`` at a time; with
        ``extra``, the tail row and the leftover cells ride behind the last slab (one SUM even when n is 0).
        -> the summed tail, if it rode."""
        import torch

        head, rows, out = self.head, self.rows, None
        for lo in range(0, max(n, 1 if extra else 0), rows):
            k = min(rows, n - lo)
            last = extra and lo + rows >= n
            stage = self.buf[: k + (2 if last else 0)]
            part = idx[lo:lo + k]
            t = time.perf_counter() if lo else self._t  # (the first slab's gather includes finding the stretches)
            torch.index_select(head, 0, part, out=stage[:k])
            if last:
                stage[k:].copy_(self.extra)
            t = self._mark("gather", t)
            self._reduce(stage)
            t = self._mark("ring", t)
            head.index_copy_(0, part, stage[:k])
            if last:
                self.left.copy_(stage[k + 1][: self.left.numel()])
                out = _tail_decode(stage[k], self.k_tail) if self.k_tail else None
            self._mark("scatter", t)
        return out


def agree(mats, tail=None, flags=None, tile_map=None, timing=None, occupancy_fn=None, state=None) -> Exchange:
    """C1 of a sum: the staging buffer taken, the occupancy of the union and the flags of all ranks on the device."""
    return Exchange(mats, tail, flags, tile_map, timing, occupancy_fn, state if state is not None else ExchangeState())


def sum_counts(mats, tail=None, flags=None, tile_map=None, timing=None, occupancy_fn=None, state=None, predict=False):
    """In-place sum over the ranks of a counter tensor and of ``tail`` in two collectives (see above); ``predict`` (needs
    ``state`` with a cap from an earlier call): no host wait, ``settle(state)`` completes it.  -> (how, summed tail); how is
    "compact" or "dense", the same on every rank.  Same integers as ``all_reduce(SUM)`` on the whole tensor: the stretches
    that are left out are zero on every rank.  Without a process group there is nothing to sum: (None, tail)."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return None, tail
    if state is None:
        state = ExchangeState()
    state.collectives = state.host_waits = 0
    x = agree(mats, tail, flags, tile_map, timing, occupancy_fn, state)
    if predict and state.cap is not None:
        return "compact", x.sum_predicted()
    return x.sum(*x.read())


def settle(state) -> None:
    """The deferred half of a predicted exchange: ONE host read (the union's real size and the flag bytes, both long since
    computed), then -- every rank alike, they all hold the same numbers -- the stretches beyond the predicted size summed
    now, and the prediction raised.  Raises on every rank if the agreed flags say the predicted exchange was not allowed (a
    rank vetoed the compact form, held int64 totals or had no staging memory, or the bound on the pairs does not fit
    uint32 cells): the bench's steady state checks those statically, each rank for itself."""
    import torch

    x = state.pending
    if x is None:
        return
    state.pending = None
    x.timing = None  # (its exchange's timing was reported already)
    fl, u = x.read()
    if fl[FLAG_NO_COMPACT] or fl[FLAG_NO_STAGING] or must_fold(fl, group_size()):
        raise RuntimeError("a predicted exchange ran although the ranks' flags forbid it: %r" % (fl,))
    if u > x.cap:
        rest = torch.nonzero_static(x.occ, size=u, fill_value=0).view(-1)[x.cap:]
        x._sum_slabs(rest, u - x.cap, extra=False)
    state.cap = max(state.cap or 0, int(1.25 * u) + 16, 64)
