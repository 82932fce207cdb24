"""Shared by test_sparse_info_cpu.py and test_sparse_info_gpu.py: crafted counters for the sparse pe_info / st_info writer,
the value model they are checked against (a numpy restatement of ``PeCounter.user_order`` + ``result()``), and thin callers
of the two library entry points.  The expected text is always ``oracle.pe_oracle.matrix_text`` without the ``:0`` lines."""
import ctypes as C
import functools

import numpy as np

from oracle import pe_oracle

SIZES = (1, 2, 63, 64, 65, 130, 257)  # 257: one past a 256-column chunk of the format kernel, five 64-cell tiles wide
BLOCKS = ("1", "100", "2000", "100000")

# uint32 cells: every digit count from 1 to 10
U32_VALUES = [1, 9, 10, 2 ** 31, 2 ** 32 - 1] + [10 ** k for k in range(2, 10)] + [10 ** k - 1 for k in range(2, 10)]
# int64 totals: every digit count from 11 to 19 (small enough that two of them still add up inside int64)
WIDE_VALUES = [10 ** k for k in range(10, 19)] + [10 ** k - 1 for k in range(11, 20) if 10 ** k - 1 < 2 ** 62] + [4 * 10 ** 18]


def filtered(text: str) -> str:
    """The dense text without the lines whose count is 0."""
    return "".join(line for line in text.splitlines(True) if not line.endswith(":0\n"))


def make_ids(n: int):
    """n distinct ids of 1 to 12 bytes, their lengths varying, some in the ``7&8*0`` style of split nodes."""
    out = []
    for i in range(n):
        s = ["%d", "%d&{0}*0".format(i + 1), "%d*A", "n%d_longname"][i % 4] % i
        out.append(s[:12])
    assert len(set(out)) == n and all(1 <= len(s) <= 12 for s in out)
    return out


def user_matrix(counts, wide, rank, upper):
    """What ``PeCounter.user_order`` + ``result()`` give: int64 [n, n] in the caller's numbering."""
    n = counts.shape[0]
    total = counts.astype(np.int64)
    if wide is not None:
        total = total + wide
    r = np.arange(n) if rank is None else np.asarray(rank, dtype=np.int64)
    if not upper:
        return total[np.ix_(r, r)]
    s = total + total.T
    s[np.diag_indices(n)] -= np.diagonal(total)
    return np.triu(s[np.ix_(r, r)])


@functools.lru_cache(maxsize=None)
def crafted(n: int, upper: int, with_map: bool, with_wide: bool, with_rank: bool = True):
    """Counters of n nodes in the internal numbering: dict(ids, counts uint32 [n, n], wide int64 [n, n] or None, tile_map
    uint8 [T * T] or None, rank uint32 [n] or None, want = the expected sparse text).  Cells on both sides of the internal
    diagonal; with a map, some tiles are unmarked (and really zero) and some marked tiles hold nothing."""
    rng = np.random.default_rng(1000 * n + 100 * upper + 10 * with_map + with_wide)
    T = (n + 63) // 64
    counts = np.zeros((n, n), dtype=np.uint32)
    hit = rng.random((n, n)) < (0.6 if n <= 2 else 0.08)
    counts[hit] = rng.choice(np.asarray(U32_VALUES, dtype=np.uint32), size=int(hit.sum()))
    small = rng.random((n, n)) < 0.05  # (ordinary small counts as well)
    counts[small] = rng.integers(1, 500, size=int(small.sum()), dtype=np.uint32)
    tile_map = None
    if with_map:
        tile_map = (rng.random((T, T)) < 0.6).astype(np.uint8)
        if T > 1:
            tile_map[0, 0] = 1
            tile_map[T - 1, 0] = 0
        keep = np.kron(tile_map, np.ones((64, 64), dtype=np.uint8))[:n, :n].astype(bool)
        counts[~keep] = 0
        if T > 1:  # a marked tile that holds nothing
            tile_map[0, T - 1] = 1
            counts[:64, 64 * (T - 1):] = 0
    wide = None
    if with_wide:
        wide = np.zeros((n, n), dtype=np.int64)
        hit = rng.random((n, n)) < (0.5 if n <= 2 else 0.03)
        wide[hit] = rng.choice(np.asarray(WIDE_VALUES, dtype=np.int64), size=int(hit.sum()))
        # a total that crosses a digit boundary: 4294967295 + 5705032705 = 10^10
        counts[0, 0] = 2 ** 32 - 1
        wide[0, 0] = 5705032705
        if tile_map is not None:
            tile_map[0, 0] = 1
        if n >= 2:  # ... and the short_mat rule's S[a][b] + S[b][a] doing the same
            counts[0, 1], wide[0, 1] = 2 ** 32 - 1, 0
            counts[1, 0], wide[1, 0] = 0, 5705032705
    rank = None
    if with_rank and n > 1:
        rank = rng.permutation(n).astype(np.uint32)
        if np.array_equal(rank, np.arange(n)):
            rank = rank[::-1].copy()
    ids = make_ids(n)
    want = filtered(pe_oracle.matrix_text(ids, user_matrix(counts, wide, rank, upper)))
    return dict(ids=ids, counts=counts, wide=wide, tile_map=None if tile_map is None else tile_map.reshape(-1).copy(), rank=rank,
                upper=upper, want=want)


def encode_ids(ids):
    from vstrains_amd import pe as host

    return host._encode_ids(ids)


def write_host(path, ids, counts, wide, tile_map, rank, upper):
    """``vs_write_info_sparse_host`` on numpy arrays -> (return code, info[4])."""
    from vstrains_amd import _native as nat

    blob, off = encode_ids(ids)
    info = (C.c_uint64 * 4)()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    rc = nat.lib().vs_write_info_sparse_host(None, str(path).encode(), blob.ctypes.data, off.ctypes.data, len(ids), ptr(counts), ptr(wide),
                                             ptr(tile_map), ptr(rank), upper, info)
    return rc, [int(x) for x in info]


def write_device(ctx, path, ids, counts, wide, tile_map, rank, upper):
    """``vs_write_info_sparse`` on torch tensors that live on the device (``rank`` a numpy array) -> (return code, info[4])."""
    from vstrains_amd import _native as nat

    blob, off = encode_ids(ids)
    info = (C.c_uint64 * 4)()
    ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = nat.lib().vs_write_info_sparse(ctx._h, str(path).encode(), blob.ctypes.data, off.ctypes.data, len(ids), ptr(counts), ptr(wide),
                                        ptr(tile_map), None if rank is None else rank.ctypes.data, upper, info)
    return rc, [int(x) for x in info]
