// The text of a sparse pe_info / st_info file, one source for the device kernels and their host twin (vs_info.hip): which
// value a cell of the caller's matrix has, how many bytes its line takes, and the line itself.  The dense file is
// "{id_i}:{id_j}:{count}\n" for all i, j in row-major order (utils/VStrains_PE_Inference.py:194-205); the sparse file is
// that file without the lines whose count is 0.  VsInfoSrc::dense keeps the zero lines, and with them the lines below the
// diagonal of st_info: the dense file itself, for the writer that compresses it on the device (vs_write_info_bgzf).
//
// Compiled twice from this text: by the kernels of vs_info.hip, and by vs_write_info_sparse_host, which walks the same
// cells with one thread -- so that a CPU test drives every branch of it before anything is launched.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define VS_INFO_HD __host__ __device__ __forceinline__
#else
#define VS_INFO_HD inline
#endif

#define VS_INFO_TILE_SHIFT 6u  // the dirty-tile map of the counters: one byte per 64 x 64 cells (vs_pe_count_tracked)

// Where the cells come from.  Every pointer is device memory in a kernel and host memory in the twin.
struct VsInfoSrc {
    const uint32_t *counts;  // n*n uint32 cells in the index's internal numbering, or NULL
    const int64_t *wide;     // n*n int64 totals (vs_counts_fold), or NULL
    const uint8_t *map;      // T*T bytes: the tiles of `counts` that may hold a non-zero cell, or NULL (every tile may);
                             // says nothing about `wide`, which is always read
    const uint32_t *rank;    // rank[i] = internal number of the caller's node i, or NULL (the same numbering)
    uint32_t n, T;           // T = ceil(n / 64)
    int upper;               // 0: node_mat rule, 1: short_mat rule
    int dense = 0;           // 0: only the lines with a count above 0, 1: every line of the reference's file
};

// the first column of the caller's row i that can have a line, and whether the value v has one
VS_INFO_HD uint32_t vs_info_first_col(const VsInfoSrc &s, uint32_t i) { return s.upper && !s.dense ? i : 0u; }
VS_INFO_HD bool vs_info_has_line(const VsInfoSrc &s, int64_t v) { return v > 0 || (s.dense && v == 0); }

// total of the internal cell (r, c): uint32 cell + int64 total; *reads counts the cells whose counters were loaded
VS_INFO_HD int64_t vs_info_total(const VsInfoSrc &s, uint32_t r, uint32_t c, uint32_t *reads) {
    const uint64_t at = (uint64_t)r * s.n + c;
    int64_t v = 0;
    bool read = false;
    if (s.counts && (!s.map || s.map[(uint64_t)(r >> VS_INFO_TILE_SHIFT) * s.T + (c >> VS_INFO_TILE_SHIFT)])) {
        v = (int64_t)s.counts[at];
        read = true;
    }
    if (s.wide) {
        v += s.wide[at];
        read = true;
    }
    *reads += read ? 1u : 0u;
    return v;
}

// The value of the caller's cell (i, j): what PeCounter.user_order followed by result() gives.
//   upper == 0 (node_mat): M[a][b]
//   upper == 1 (short_mat, which holds a pair of nodes at (smaller, larger) INTERNAL number, PE_Inference.py:174-184):
//              0 below the caller's diagonal, S[a][a] on it, S[a][b] + S[b][a] above
VS_INFO_HD int64_t vs_info_value(const VsInfoSrc &s, uint32_t i, uint32_t j, uint32_t *reads) {
    const uint32_t a = s.rank ? s.rank[i] : i, b = s.rank ? s.rank[j] : j;
    if (!s.upper) return vs_info_total(s, a, b, reads);
    if (i > j) return 0;
    if (i == j) return vs_info_total(s, a, a, reads);
    const int64_t x = vs_info_total(s, a, b, reads), y = vs_info_total(s, b, a, reads);
    return (x < 0 || y < 0) ? -1 : x + y;  // (a negative total stays visible as one: the writers refuse it)
}

// decimal digits of v (1 .. 20)
VS_INFO_HD uint32_t vs_info_digits(uint64_t v) {
    if (v < 0x100000000ull) {
        const uint32_t w = (uint32_t)v;
        return w < 10u ? 1u : w < 100u ? 2u : w < 1000u ? 3u : w < 10000u ? 4u : w < 100000u ? 5u : w < 1000000u ? 6u
             : w < 10000000u ? 7u : w < 100000000u ? 8u : w < 1000000000u ? 9u : 10u;
    }
    uint32_t d = 10u;
    uint64_t p = 10000000000ull;  // 10^10
    while (d < 20u && v >= p) {
        d++;
        if (d < 20u) p *= 10u;
    }
    return d;
}

// bytes of the line of a value v between ids of li and lj bytes: id_i ':' id_j ':' digits '\n'
VS_INFO_HD uint32_t vs_info_line_len(uint32_t li, uint32_t lj, uint64_t v) { return li + lj + vs_info_digits(v) + 3u; }

// the line, vs_info_line_len bytes at q
VS_INFO_HD void vs_info_put_line(uint8_t *q, const uint8_t *idi, uint32_t li, const uint8_t *idj, uint32_t lj, uint64_t v) {
    for (uint32_t k = 0; k < li; k++) q[k] = idi[k];
    q += li;
    *q++ = (uint8_t)':';
    for (uint32_t k = 0; k < lj; k++) q[k] = idj[k];
    q += lj;
    *q++ = (uint8_t)':';
    const uint32_t d = vs_info_digits(v);
    uint32_t k = d;
    while (v >= 0x100000000ull) {  // (64-bit division only while the value needs it)
        q[--k] = (uint8_t)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    }
    uint32_t w = (uint32_t)v;
    do {
        q[--k] = (uint8_t)('0' + w % 10u);
        w /= 10u;
    } while (k);
    q[d] = (uint8_t)'\n';
}
