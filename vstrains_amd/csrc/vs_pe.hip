// K2-K4 fused: seed probe -> load-balanced hit expansion + exact extension -> per-end
// aggregation in LDS -> acceptance test -> PE-link counters.
//
// What it computes is single_end_read_mapping + the pair loop of the reference
// (utils/VStrains_PE_Inference.py:16-48 and :155-188), bit for bit:
//   for a read end and a node, the reference's three numbers are
//     v        = number of (read window, table entry) coincidences for that node   (:29)
//     coords   = smallest forward node offset among them                           (:30)
//     kindices = smallest read offset among them                                   (:31)
//   Windows that coincide lie on diagonals; on one diagonal they form maximal runs, and a run
//   is exactly a maximal exact match (MEM) of length l >= K between the read and one strand of
//   the node: it contributes l-K+1 to v, its first node offset to coords (mapped back to the
//   forward strand for reverse matches: the reference stores the forward offset under the
//   reverse-complemented window, :132) and its first read offset to kindices.  Palindromic
//   windows are held twice by the reference (:125,:132) and are found here once per strand.
//   Every MEM holds a seed at a read offset divisible by s; the MEM is credited by the first
//   such seed only (left extension < s), so nothing is counted twice.
//
// The pipeline of one block (vs_pe_count):
//   k_pe_locus / k_locus_*  the pairs in locus order (first node a seed of the forward read hits)
//   k_pe_tiles              the mapping kernel, one 256-thread workgroup per run of tiles of `ept` read ends (ept/2 pairs):
//     P0  the next tile's headers and packed reads brought into the other LDS copy (one wpe-word slot per end), the
//         tile-wide (end, node) table emptied, pairs classified
//     P1  one thread per (end, probe): seed, canonical form, open-address table probe (one 16-B load per slot visited);
//         posting count per probe -> LDS.  (The compile-time shapes of graphs with many postings per seed probe two
//         candidate grids and expand the cheaper one: the adaptive step grid)
//     P2  workgroup inclusive scan of the posting counts
//     P3  one thread per posting (binary search of the scan = CSR-style frontier expansion, so a repeat seed's many
//         postings spread over lanes): left/right extension on 64-bit windows (XOR + clz/ctz), LDS atomics into the
//         tile's (end, node) hash table
//     P4  acceptance test per occupied slot (integer form, see oracle/pe_oracle.py); the accepted nodes of every end
//         PACKED into lists by a wavefront prefix sum; pairs with an overflowed end to the overflow list
//     P5  the hand-off to the counter kernels: the tile's packed lists as one coalesced stretch (or, for the row
//         owners, rows of a fixed stride per end)
//   k_pe_accumulate         the counters pair-major, summed in an LDS cell table (graphs of at most 46 340 nodes), or
//   k_list_owners .. k_rows_sum   the counters by ROW OWNERS (output-major: the lists transposed, a strip of matrix rows
//                           per workgroup)
//   k_pe_mid, k_pe_slow     the overflow: pairs with an end of more than LCAP accepted nodes, a full tile table or many
//                           bytes outside ACGT, one wavefront per pair with LDS state, then what that cannot hold with
//                           dense per-workgroup node state in HBM
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vs_internal.h"
#include "vs_acc_tasks.h"
#include "vs_pe_pack.h"

#define TPB 256
// The hand-off between the mapping kernel and the counter kernels (r6): the accepted nodes of a tile's ends are PACKED --
// end after end, every list padded to whole quads (16 bytes), no fixed row per end.  Found by a wavefront prefix sum over
// the ends' list lengths (k_pe_tiles P4), in LDS first, then written out as one coalesced stretch.
//   LC    list words a tile's region of the hand-off buffer holds per end ON AVERAGE (region = ept * LC words)
//   LCAP  accepted nodes an end may have on the main path (more -> the overflow kernels); rows of 16 sent 2.3 % of the
//         pairs of configs[4] (ends of 17 .. 19 nodes) through k_pe_mid a second time
//   pair-major counters (k_pe_accumulate): counts[end] = n | quad offset inside the tile's region << 8
//   row owners (graphs beyond 46 340 nodes): their entries name lists by END INDEX, so the lists keep a fixed stride
//         there -- a row of LC words per end, of which only the quads that hold nodes are written, and ONE more quad per
//         end, in an array of its own behind the rows, for nodes 17 .. LCAP; counts[end] = n
#define LCAP 20u  // (LC: vs_pe_plan.h)
// (rows of LCAP words, 80 bytes apart, straddle a 64-byte stretch every other time -- the row owners took 13.0 ms instead of
// 10.9 at configs[4] -- and rows 128 bytes apart are fetched as whole 128-byte lines: k_list_owners 2.9 -> 4.1 ms)
__device__ __forceinline__ const uint32_t *vs_row_quad(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ hi, uint64_t row, uint32_t q) {
    return q < LC / 4u ? lists + row * LC + 4u * q : hi + row * 4u;
}
#define EMPTY_NODE 0xFFFFFFFFu

struct PeParams {
    VsIndexDev idx;
    VsReadsDev rd;
    uint32_t *node_mat, *short_mat;
    unsigned long long *stats;
    uint32_t ept, pmax, words_cap, pool, pool_bits;
    uint64_t n_tiles;
    uint32_t *slow_list, *slow_count;
    uint32_t *dbg_lists, *dbg_counts;
    uint32_t dbg_cap;
    uint32_t accumulate;
    const uint32_t *perm;  // pair order of the tiles (locus-sorted) or NULL = input order
    uint32_t wpe;          // LDS words reserved per read end
    uint32_t tiles_per_wg; // contiguous run of tiles per workgroup
    uint32_t magic_pmax, magic_wpe;  // vs_fastdiv constants
    uint32_t *out_lists;             // accepted node ids, tile order: packed regions of ept * LC words / rows of LCAP words (out_rows)
    uint32_t *out_counts;            // [n_tiles * ept] list lengths (0 for ends that add nothing), packed form: | quad offset << 8
    uint32_t out_rows;               // 1: fixed rows of LC words per end + out_lists_hi (the row owners follow), 0: packed
    uint32_t *out_lists_hi;          // [n_tiles * ept * 4] nodes 17 .. LCAP of every end (row layout)
    uint64_t n_pairs;
    uint32_t shortcut;               // overlapping-seed ownership shortcut for single postings (P3 stage A)
    uint8_t *tile_map;               // vs_pe_count_tracked: one byte per 64 x 64 tile of node_mat, then of short_mat; NULL = none
    uint32_t tile_T;                 // tiles per matrix side = ceil(N / 64)
    uint32_t mid_fast;               // k_pe_mid: clean ends are compared straight-line (vs_agree_fast; the block has the shape of MODE 1)
};

// A counter cell is about to be added to: its tile is marked (a plain store of 1; racing stores write the same value).
__device__ __forceinline__ void vs_mark_tile(uint8_t *map, uint32_t T, uint32_t mat, uint32_t x, uint32_t y) {
    if (!map) return;
    const uint64_t t = ((uint64_t)mat * T + (x >> 6)) * T + (y >> 6);
    if (!map[t]) map[t] = 1;
}

// The same without looking first: a plain store that nothing waits for (k_pe_mid marks from inside loops of fire-and-forget
// atomics; the load of the test above was a round trip per loop turn -- r5).
__device__ __forceinline__ void vs_mark_tile_store(uint8_t *map, uint32_t T, uint32_t mat, uint32_t x, uint32_t y) {
    if (map) map[((uint64_t)mat * T + (x >> 6)) * T + (y >> 6)] = 1;
}

// (the wavefront scans by DPP moves, vs_wave_scan_add / vs_wave_scan_max, are in vs_internal.h)
// (r6) SIX workgroups per CU for the compile-time shapes of graphs whose ends touch few nodes (the non-adaptive instantiations):
// a tile table of 768 slots instead of 1 024 (12 per end, placed by a multiply-high range reduction instead of a power-of-two
// mask) and a list region of 960 words make 26.8 KB of LDS per workgroup, and with the thread index laundered at the top of the
// tile loop as well (nothing P0 .. P2 derive from it is hoisted across P3) the kernel fits 80 vector registers without
// scratch: six wavefronts per SIMD instead of five.  configs[2]: 4.70 -> 4.45 ms; either half alone gains nothing
// (the laundering alone: noise; the smaller table at five workgroups: +2 %).
struct Mem {  // one credited maximal exact match
    uint32_t cnt, minp, minj;
};

// Straight-line agreement of a read with node text on either side of a seed, for the common block
// shape (probe stride <= 32, reads <= 191 bases with w = 31): one left window, four / five right
// windows, everything loaded up front, the answer out of selects -- no data-dependent branch.
//   left : bases over which the read (going down from j) equals the text going down from tl, at
//          most cl (<= 32)
//   ext  : bases over which the read (going up from j + w) equals the text going up from tr, at most rem
// tl / tr are base indices into the one array of node texts (forward, and rc_delta words on the
// reverse complements).
struct __attribute__((packed, aligned(4))) VsQuad { uint32_t x, y, z, w; };  // 16-byte load at dword alignment

template <bool W4>  // W4: four right windows are enough (reads <= 159 bases with w = 31)
__device__ __forceinline__ void vs_agree_fast(const uint32_t *rw, uint32_t rbase, const uint32_t *tw, uint32_t tl, uint32_t cl,
                                              uint32_t tr, uint32_t rem, uint32_t j, uint32_t w, uint32_t *left_out,
                                              uint32_t *ext_out) {
    const uint32_t n0 = cl;
    const uint32_t rj = j + w;
    // Node text to the right of the seed: eleven words cover the five windows; they come as 16-byte
    // loads, and the second / third only when the match can reach that far (rem) -- on a graph of
    // short nodes one load settles most postings.  Words not loaded read as zero: whatever they make
    // of the comparison lies beyond `rem` and is clipped.
    const uint32_t ti = tr >> 4, sh = (tr & 15u) * 2u;
    const VsQuad q0 = *(const VsQuad *)(tw + ti);
    VsQuad q1 = {0u, 0u, 0u, 0u}, q2 = {0u, 0u, 0u, 0u};
    if (rem > 48u) q1 = *(const VsQuad *)(tw + ti + 4u);
    if (!W4 && rem > 112u) q2 = *(const VsQuad *)(tw + ti + 8u);  // (the fourth window needs word 8 only)
    if (W4 && rem > 112u) q2.x = tw[ti + 8u];
    auto tw64 = [&](uint32_t w0, uint32_t w1, uint32_t w2) {
        return (uint64_t)__builtin_amdgcn_alignbit(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, sh) << 32);
    };
    // the read's side of the same five windows: eleven consecutive LDS words, one shift
    const uint32_t rr = rbase + rj, rsh = (rr & 15u) * 2u;
    const uint32_t *rp = rw + (rr >> 4);
    const uint32_t r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4];
    auto rw64 = [&](uint32_t w0, uint32_t w1, uint32_t w2) {
        return (uint64_t)__builtin_amdgcn_alignbit(w1, w0, rsh) | ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, rsh) << 32);
    };
    const uint64_t xl = (vs_win(rw, rbase + j - n0) ^ vs_win(tw, tl - n0)) & vs_lowmask(2u * n0);
    const uint64_t x0 = rw64(r0, r1, r2) ^ tw64(q0.x, q0.y, q0.z);
    const uint64_t x1 = rw64(r2, r3, r4) ^ tw64(q0.z, q0.w, q1.x);
    *left_out = xl ? n0 - 1u - (uint32_t)((63 - __clzll((long long)xl)) >> 1) : n0;
    // Windows 2..4 only where the match can reach them: on a graph of nodes hardly longer than k+1 most
    // wavefronts have no such posting and skip the block (a branch on "any lane", not on data of one lane).
    uint32_t far = 160u;  // (nothing differs within reach: clipped by rem below)
    if (rem > 64u) {
        const uint32_t r5 = rp[5], r6 = rp[6], r7 = rp[7], r8 = rp[8], r9 = W4 ? 0u : rp[9], r10 = W4 ? 0u : rp[10];
        const uint64_t x2 = rw64(r4, r5, r6) ^ tw64(q1.x, q1.y, q1.z);
        const uint64_t x3 = rw64(r6, r7, r8) ^ tw64(q1.z, q1.w, q2.x);
        const uint64_t x4 = W4 ? 0ull : rw64(r8, r9, r10) ^ tw64(q2.x, q2.y, q2.z);
        uint64_t xs = x4;  // (W4: zero -- no difference found inside 128 bases means ext = 160, clipped by rem <= 128)
        uint32_t xb = 128u;
        if (x3) { xs = x3; xb = 96u; }
        if (x2) { xs = x2; xb = 64u; }
        if (xs) far = xb + ((uint32_t)(__ffsll((long long)xs) - 1) >> 1);
    }
    // first window that differs (selects), then one find-first-set
    uint64_t xn = x1;
    uint32_t xb = 32u;
    if (x0) { xn = x0; xb = 0u; }
    const uint32_t ext = xn ? xb + ((uint32_t)(__ffsll((long long)xn) - 1) >> 1) : far;
    *ext_out = ext < rem ? ext : rem;
}

// The same for longer strides and reads (k up to 158: stride <= 128; reads <= w + 256 bases): four
// left windows, eight right windows, still without a data-dependent branch.  Text words come as
// 16-byte loads that are skipped where the match cannot reach (cl / rem).
__device__ __forceinline__ void vs_agree_long(const uint32_t *rw, uint32_t rbase, const uint32_t *tw, uint32_t tl, uint32_t cl,
                                              uint32_t tr, uint32_t rem, uint32_t j, uint32_t w, uint32_t *left_out,
                                              uint32_t *ext_out) {
    // ---- left: window i holds the n_i = clamp(cl - 32 i, 0, 32) bases just below the previous one,
    // lowest base first, so a difference nearest the seed is the highest set bit
    uint32_t left = cl;
    {
        uint64_t xs = 0ull;
        uint32_t at = 0u, nn = 0u;
#pragma unroll
        for (int i = 3; i >= 0; i--) {  // (from the far window to the near one: the nearest difference wins)
            const uint32_t lo = 32u * (uint32_t)i;
            const uint32_t n = cl > lo ? (cl - lo < 32u ? cl - lo : 32u) : 0u;
            uint64_t x = 0ull;
            if (n) x = (vs_win(rw, rbase + j - lo - n) ^ vs_win(tw, tl - lo - n)) & vs_lowmask(2u * n);
            if (x) { xs = x; at = lo; nn = n; }
        }
        if (xs) left = at + nn - 1u - (uint32_t)((63 - __clzll((long long)xs)) >> 1);
    }
    // ---- right: seventeen words either side cover eight windows
    const uint32_t rj = j + w;
    const uint32_t ti = tr >> 4, sh = (tr & 15u) * 2u;
    const VsQuad q0 = *(const VsQuad *)(tw + ti);
    VsQuad q1 = {0u, 0u, 0u, 0u}, q2 = q1, q3 = q1;
    uint32_t t16 = 0u;
    if (rem > 48u) q1 = *(const VsQuad *)(tw + ti + 4u);
    if (rem > 112u) q2 = *(const VsQuad *)(tw + ti + 8u);
    if (rem > 176u) q3 = *(const VsQuad *)(tw + ti + 12u);
    if (rem > 240u) t16 = tw[ti + 16u];
    auto tw64 = [&](uint32_t w0, uint32_t w1, uint32_t w2) {
        return (uint64_t)__builtin_amdgcn_alignbit(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, sh) << 32);
    };
    const uint32_t rr = rbase + rj, rsh = (rr & 15u) * 2u;
    const uint32_t *rp = rw + (rr >> 4);
    uint32_t r[17];
#pragma unroll
    for (int i = 0; i < 17; i++) r[i] = rp[i];
    auto rw64 = [&](uint32_t w0, uint32_t w1, uint32_t w2) {
        return (uint64_t)__builtin_amdgcn_alignbit(w1, w0, rsh) | ((uint64_t)__builtin_amdgcn_alignbit(w2, w1, rsh) << 32);
    };
    const uint64_t x0 = rw64(r[0], r[1], r[2]) ^ tw64(q0.x, q0.y, q0.z);
    const uint64_t x1 = rw64(r[2], r[3], r[4]) ^ tw64(q0.z, q0.w, q1.x);
    const uint64_t x2 = rw64(r[4], r[5], r[6]) ^ tw64(q1.x, q1.y, q1.z);
    const uint64_t x3 = rw64(r[6], r[7], r[8]) ^ tw64(q1.z, q1.w, q2.x);
    const uint64_t x4 = rw64(r[8], r[9], r[10]) ^ tw64(q2.x, q2.y, q2.z);
    const uint64_t x5 = rw64(r[10], r[11], r[12]) ^ tw64(q2.z, q2.w, q3.x);
    const uint64_t x6 = rw64(r[12], r[13], r[14]) ^ tw64(q3.x, q3.y, q3.z);
    const uint64_t x7 = rw64(r[14], r[15], r[16]) ^ tw64(q3.z, q3.w, t16);
    uint64_t xs = x7;
    uint32_t xb = 224u;
    if (x6) { xs = x6; xb = 192u; }
    if (x5) { xs = x5; xb = 160u; }
    if (x4) { xs = x4; xb = 128u; }
    if (x3) { xs = x3; xb = 96u; }
    if (x2) { xs = x2; xb = 64u; }
    if (x1) { xs = x1; xb = 32u; }
    if (x0) { xs = x0; xb = 0u; }
    const uint32_t ext = xs ? xb + ((uint32_t)(__ffsll((long long)xs) - 1) >> 1) : 256u;
    *left_out = left;
    *ext_out = ext < rem ? ext : rem;
}

// Bytes outside ACGT cut a read into segments no match can cross (a dict lookup of a window over
// such a byte misses, PE_Inference.py:25-26).  `inv4` lists up to four such positions of an end
// (one byte each, 0xFF = none; ends with more go to the overflow path): is the seed at j clean, and
// which stretch [lo, hi) of the read around it is.
__device__ __forceinline__ bool vs_seed_limits(uint32_t inv4, uint32_t j, uint32_t w, uint32_t rlen, uint32_t *lo, uint32_t *hi) {
    uint32_t l = 0u, h = rlen;
    bool ok = true;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t p = (inv4 >> (8u * i)) & 0xFFu;
        if (p != 0xFFu) {
            if (p < j) l = l > p + 1u ? l : p + 1u;
            else if (p >= j + w) h = h < p ? h : p;
            else ok = false;
        }
    }
    *lo = l;
    *hi = h;
    return ok;
}

// Extension of a seed hit.  rw/rbase: packed read (LDS or global) and its first base; tw/tbase:
// packed node strand.  mk/mbase: validity mask of the read or NULL.  Returns false when the
// match is owned by an earlier probe or is shorter than K.
// The first left window and the first two right windows are loaded before anything is decided
// (independent loads, one memory round trip); most hits are settled by them.  Windows may reach
// past the end of a read / node: every packed buffer carries VS_PAD_WORDS of padding and the
// bits beyond the valid range are never used.
template <typename RB>
__device__ __forceinline__ bool vs_extend(const uint32_t *rw, RB rbase, uint32_t rlen, const uint32_t *tw,
                                          uint32_t tbase, uint32_t tlen, uint32_t j, uint32_t q, uint32_t w,
                                          uint32_t s, uint32_t K, const uint32_t *mk, uint64_t mbase,
                                          uint32_t *a_out, uint32_t *qa_out, uint32_t *len_out) {
    uint32_t c = s < j ? s : j;
    c = c < q ? c : q;
    const uint32_t n0 = c < 32u ? c : 32u;
    const uint32_t rj = j + w, rq = q + w;
    uint32_t rem = rlen - rj;
    {
        const uint32_t rem2 = tlen - rq;
        rem = rem < rem2 ? rem : rem2;
    }
    uint64_t xl = vs_win(rw, rbase + j - n0) ^ vs_win(tw, tbase + q - n0);
    uint64_t xr0 = vs_win(rw, rbase + rj) ^ vs_win(tw, tbase + rq);
    uint64_t xr1 = vs_win(rw, rbase + rj + 32u) ^ vs_win(tw, tbase + rq + 32u);
    if (mk) {
        xl |= vs_win64(mk, mbase + j - n0);
        xr0 |= vs_win64(mk, mbase + rj);
        xr1 |= vs_win64(mk, mbase + rj + 32u);
    }
    xl &= vs_lowmask(2u * n0);
    uint32_t left = 0;
    if (xl) {
        left = n0 - 1u - (uint32_t)((63 - __clzll((long long)xl)) >> 1);
    } else {
        left = n0;
        while (left < c) {  // s > 32 only (k > 85): further windows backwards
            uint32_t n = c - left < 32u ? c - left : 32u;
            uint64_t x = vs_win(rw, rbase + j - left - n) ^ vs_win(tw, tbase + q - left - n);
            if (mk) x |= vs_win64(mk, mbase + j - left - n);
            x &= vs_lowmask(2u * n);
            if (x) {
                left += n - 1u - (uint32_t)((63 - __clzll((long long)x)) >> 1);
                break;
            }
            left += n;
        }
    }
    if (left >= s) return false;  // an earlier probe lies inside this match and owns it
    uint32_t ext = 0;
    if (rem) {
        if (xr0) {
            uint32_t m = (uint32_t)(__ffsll((long long)xr0) - 1) >> 1;
            ext = m < rem ? m : rem;
            rem = 0;
        } else {
            uint32_t adv = rem < 32u ? rem : 32u;
            ext = adv;
            rem -= adv;
            if (rem) {
                if (xr1) {
                    uint32_t m = (uint32_t)(__ffsll((long long)xr1) - 1) >> 1;
                    ext += m < rem ? m : rem;
                    rem = 0;
                } else {
                    adv = rem < 32u ? rem : 32u;
                    ext += adv;
                    rem -= adv;
                }
            }
        }
    }
    while (rem) {
        uint64_t x = vs_win(rw, rbase + rj + ext) ^ vs_win(tw, tbase + rq + ext);
        if (mk) x |= vs_win64(mk, mbase + rj + ext);
        if (x) {
            uint32_t m = (uint32_t)(__ffsll((long long)x) - 1) >> 1;
            ext += m < rem ? m : rem;
            break;
        }
        uint32_t adv = rem < 32u ? rem : 32u;
        ext += adv;
        rem -= adv;
    }
    uint32_t len = left + w + ext;
    if (len < K) return false;
    *a_out = j - left;
    *qa_out = q - left;
    *len_out = len;
    return true;
}

__device__ __forceinline__ bool vs_accept(uint32_t v, uint32_t coord, uint32_t kidx, uint32_t nlen, uint32_t rlen, uint32_t K) {
    long long c = coord, ki = kidx, nl = nlen, rl = rlen, k = K;
    long long right = c + nl - 1;
    long long alt = c - ki + rl - 1;
    if (alt < right) right = alt;
    long long saturate = right - c - k + 2;
    long long span = (rl < nl ? rl : nl) - k + 1;
    return ((long long)v >= saturate) || ((long long)v * rl >= span * (rl - k));
}

// The same test in 32-bit arithmetic for the straight-line kernels (reads <= 191 bases: v, the read
// length and k+1 stay below 2^8, node offsets and lengths below 2^25, so nothing overflows int32).
__device__ __forceinline__ bool vs_accept32(uint32_t v, uint32_t coord, uint32_t kidx, uint32_t nlen, uint32_t rlen, uint32_t K) {
    const int c = (int)coord, ki = (int)kidx, nl = (int)nlen, rl = (int)rlen, k = (int)K;
    int right = c + nl - 1;
    const int alt = c - ki + rl - 1;
    if (alt < right) right = alt;
    const int saturate = right - c - k + 2;
    const int span = (rl < nl ? rl : nl) - k + 1;
    return ((int)v >= saturate) || ((int)v * rl >= span * (rl - k));
}

// Probe the table for the seed at read offset j.  Returns posting count (0 = miss) and payload.
// (Requesting two neighbouring slots together -- at an eighth fill one lane in ten needs the second slot, so nearly every
// wavefront does, as a second dependent round trip -- was measured equal within noise at configs[2..4] (5.97 / 30.2 /
// 11.7 ms against 5.99 / 30.6 / 11.5), like tables of 1/16 .. 1/64 fill: the probes are not where k_pe_tiles waits.
// Fuller tables lose: 1/4 fill +3 %, 1/2 fill +13 %.)
__device__ __forceinline__ uint32_t vs_probe(const VsIndexDev &idx, uint64_t key, uint32_t sr, uint32_t *pa, uint32_t *pb) {
    uint32_t mask = (1u << idx.table_bits) - 1u;
    uint32_t sl = vs_slot_of(key, idx.table_bits);
    const uint4 *tab = (const uint4 *)idx.table;
    for (;;) {
        const uint4 r0 = tab[sl];
        {   // (the slot in a scope of its own: without it the compile-time-shape k_pe_tiles schedule about ten more vector
            // instructions and one more global load)
            const uint4 raw = r0;
            uint64_t k = (uint64_t)raw.x | ((uint64_t)raw.y << 32);
            if (k == VS_EMPTY_KEY) return 0u;
            if ((k & ~VS_MULTI_BIT) == key) {
                if (k & VS_MULTI_BIT) {
                    *pa = raw.z;
                    *pb = raw.w | (sr << 31);
                    return raw.w;
                }
                *pa = raw.z;
                *pb = raw.w ^ (sr << 31);
                return 1u;
            }
        }
        sl = (sl + 1u) & mask;
    }
}

// The same with the first slot of the chain already loaded (`raw`, from slot `sl`): two probes of one thread have their
// first -- nearly always only -- slot loads in flight together before either is looked at.
__device__ __forceinline__ uint32_t vs_probe_from(const VsIndexDev &idx, uint64_t key, uint32_t sr, uint32_t sl, uint4 raw, uint32_t *pa, uint32_t *pb) {
    const uint32_t mask = (1u << idx.table_bits) - 1u;
    const uint4 *tab = (const uint4 *)idx.table;
    for (;;) {
        const uint64_t k = (uint64_t)raw.x | ((uint64_t)raw.y << 32);
        if (k == VS_EMPTY_KEY) return 0u;
        if ((k & ~VS_MULTI_BIT) == key) {
            *pa = raw.z;
            if (k & VS_MULTI_BIT) {
                *pb = raw.w | (sr << 31);
                return raw.w;
            }
            *pb = raw.w ^ (sr << 31);
            return 1u;
        }
        sl = (sl + 1u) & mask;
        raw = tab[sl];
    }
}

extern __shared__ __attribute__((aligned(16))) uint32_t vs_lds[];
__device__ __forceinline__ void vs_wave_sync() {  // LDS written by this wavefront is visible to all of its lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// (TileLayout, the compile-time shapes STD_* / STD2_* and vs_std_table: vs_pe_plan.h)
// MODE 0: generic loops (masked reads through the validity mask, any stride / read length);
//      1: straight-line comparison, stride <= 32, reads <= w + 160; 2: the same for stride <= 128, reads <= w + 256.
// Tile and pair indices inside k_pe_tiles are 32-bit: a block holds fewer than 2^32 ends (64-bit indices spilled six more
// scalar registers and took two more vector registers in the k = 55 shape).
// Compiled for 5 waves per SIMD (<= 96 VGPRs; the LDS tile fits 5 times too), the long-window instantiations (k = 127) as
// well (21.9 ms at configs[3] against 23.3 at 4 waves, 118 VGPRs); 6 for the non-adaptive compile-time shapes (the
// 768-slot table above).
template <int MODE, uint32_t SW, uint32_t SP, bool AD = false>
__global__ void __launch_bounds__(TTPB)
__attribute__((amdgpu_waves_per_eu((SW != 0u && !AD) ? 6 : 5, (SW != 0u && !AD) ? 6 : 5)))
k_pe_tiles(PeParams P) {
    constexpr bool FAST = MODE != 0;
    constexpr uint32_t AB = MODE == 2 ? 9u : 8u;  // bits of the read offset packed under the node length (credit / P4)
    constexpr bool STD = SW != 0u;
    // postings per thread and expansion chunk: two for the k = 55 shapes; ONE for the long-window comparison (MODE 2), whose
    // second posting's state went to scratch (72 B per lane at 96 VGPRs): 8.72 -> 7.29 ms at configs[3] (r5)
    constexpr uint32_t KPPT = MODE == 2 ? PPT_LONG : PPT, KCHUNK = TTPB * KPPT;
    // (r5) ADAPT: the probe grid of an end is chosen among the exact "step grids" (tests/seed_extend_model.step_grid): grid
    // positions s-1, 2s-1, ... of which those from the t-th on are moved D = s - 2 - (len - w) mod s bases towards the
    // read's start.  P1 probes both candidates of every position (8 slot loads per 150-base end instead of 4), picks the t
    // with the fewest postings, and only that grid is expanded: 57 -> 43 postings per end at configs[4], 21.9 -> 17.1
    // at configs[2] (tools/phase_gate.py).  Any grid of the family gives the same lists; the choice only changes the work.
    constexpr bool ADAPT = STD && AD;
    static_assert(!ADAPT || (MODE == 2 ? STD2_EPT : STD_EPT) * SP <= TTPB, "the adaptive probe phase takes one probe position per thread");
    constexpr uint32_t STD_WPE = SW, STD_PMAX = SP;
    const uint32_t tid = threadIdx.x;
    // (the compile-time-shape instantiations only count: vs_pe_map_ends takes the generic ones)
    const bool want_dbg = !STD && P.dbg_counts != nullptr;
    const bool accumulate = STD || P.accumulate;
    // (r3) MODE 2 has one compile-time shape too: k = 127 with 2 x 241..256 bases -- 63-base seeds, stride 66, 16 words and
    // two probes per end, 60 ends per tile (what the plan's LDS budget gives that shape)
    constexpr uint32_t C_EPT = MODE == 2 ? STD2_EPT : STD_EPT, C_K = MODE == 2 ? STD2_K : STD_K;
    constexpr uint32_t C_W = MODE == 2 ? STD2_W : STD_W, C_S = MODE == 2 ? STD2_S : STD_S;
    constexpr uint32_t C_POOL_BITS = MODE == 2 ? STD2_POOL_BITS : STD_POOL_BITS;
    const uint32_t ept = STD ? C_EPT : P.ept, pmax = STD ? STD_PMAX : P.pmax;
    const uint32_t NI = ept * pmax;
    const uint32_t w = STD ? C_W : P.idx.w, s = STD ? C_S : P.idx.s, K = STD ? C_K : P.idx.K;
    const uint32_t wv = VS_SEED_VERIFIED(w);  // seed bases the comparison skips (0: seeds with mixed keys, vs_seed_key)
    constexpr bool P12 = STD && !AD;  // the 768-slot table (vs_std_table)
    constexpr uint32_t C_POOL = vs_std_table(MODE, STD, AD).pool, C_TRIM = vs_std_table(MODE, STD, AD).trim;
    // PRE: a thread's probe of the NEXT tile is begun in front of P4 -- key, home slot, the slot's load -- and finished in that
    // tile's P1 from the carried key and slot (one probe per thread; nothing of it is live across P3).  Measured and not kept
    // (profiles/EXPERIMENTS.md): walking the chain on at places between the two, and issuing the loads of the tile after it
    // behind P1 instead of in front of it.
    constexpr bool PRE = MODE == 1 && STD && !AD;
    static_assert(!PRE || STD_EPT * SP <= TTPB, "the pre-probe takes one probe of the next tile per thread");
    static_assert(!PRE || (STD_W <= 31u && VS_MULTI_BIT == (1ull << 62)), "the carried key keeps the strand in bit 63: exact keys of at most 62 bits");
    const uint32_t pool = STD ? C_POOL : P.pool, pool_shift = 32u - (STD ? C_POOL_BITS : P.pool_bits);
    const uint32_t words_cap = STD ? C_EPT * STD_WPE : P.words_cap;
    const TileLayout T = tile_layout(ept, pmax, words_cap, pool, C_TRIM);
    // (these five point at the current tile's copy; see the top of the tile loop)
    uint32_t *s_gwoff = vs_lds + T.woff;   // global word offsets (mask reads, slow path)
    uint32_t *s_gend = vs_lds + T.gend;
    uint32_t *s_meta = vs_lds + T.meta;
    uint32_t *s_inv = vs_lds + T.inv;      // up to four positions of bytes outside ACGT per end (vs_seed_limits)
    uint32_t *s_words = vs_lds + T.words;  // end e occupies words [e*wpe, (e+1)*wpe)
    const uint32_t hw = (ept + 2u) & ~1u, wcap = words_cap + 8u;
    uint32_t *s_pcnt = vs_lds + T.pcnt + 1u;  // posting counts per probe, then their inclusive scan; s_pcnt[-1] == 0
    uint32_t *s_pa = vs_lds + T.pa;
    uint32_t *s_pb = vs_lds + T.pb;
    uint32_t *s_hkey = vs_lds + T.hkey;    // tile-wide (end, node) table: key = end << 25 | node
    uint32_t *s_hcnt = vs_lds + T.hcnt;
    uint32_t *s_hminp = vs_lds + T.hminp;
    uint32_t *s_hminj = vs_lds + T.hminj;
    uint32_t *s_ns = vs_lds + T.ns;        // accepted nodes per end
    uint32_t *s_state = vs_lds + T.state;  // bit0: end belongs to a used pair, bit1: overflow; bits 8..: first probe offset (vs_seed_phase)
    uint32_t *s_list = vs_lds + T.list;    // accepted node ids, LC per end
    uint32_t *s_misc = vs_lds + T.misc;
    uint32_t *s_owner = vs_lds + T.owner;
    const uint32_t wpe = STD ? STD_WPE : P.wpe;
    const uint32_t ppt = ept / 2u;
    const bool has_inv = FAST && P.rd.inv4 != nullptr;  // (the generic kernel reads the mask instead)

    if (tid < 3) s_misc[12 + tid] = 0;  // workgroup-local stats
    if (tid == 3) vs_lds[T.pcnt] = 0;
    // a workgroup takes a contiguous run of the locus-sorted tiles (node text stays in L1/L2)
    // Workgroups go to the 8 XCDs round-robin (blockIdx % 8).  The runs are handed out so that XCD x
    // works through the x-th eighth of the locus order: what a locus touches (table slots, postings,
    // node text) is then cached in one L2 instead of eight.
    uint32_t wg = blockIdx.x;
    if ((gridDim.x & 7u) == 0u) wg = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    // (pairs and tiles of a block fit 32 bits: vs_reads holds fewer than 2^32 ends)
    const uint32_t n_pairs32 = (uint32_t)P.n_pairs, n_tiles32 = (uint32_t)P.n_tiles;
    const uint32_t tile_lo = wg * P.tiles_per_wg;
    const uint32_t tile_hi = tile_lo + P.tiles_per_wg < n_tiles32 ? tile_lo + P.tiles_per_wg : n_tiles32;
    // The headers of a tile (pair order -> end index -> word offset, length) are two dependent
    // global loads; they run ahead in registers, one link per tile (pair order two tiles ahead, word
    // offset and length one tile ahead; one end per thread, ept <= TTPB), so that neither waits for
    // the other and both are covered by the previous tiles' work.
    uint32_t pf_gend = 0, pf_gwoff = 0, pf_meta = 0, pf_inv = 0xFFFFFFFFu, pf_pair = 0xFFFFFFFFu;
    uint32_t cur_inv = 0xFFFFFFFFu;  // this thread's end of the CURRENT tile (goes to LDS at the top of the tile)
    auto prefetch_pair = [&](uint32_t t) {  // pair (in input order) of this thread's end in tile t
        pf_pair = 0xFFFFFFFFu;
        if (t < tile_hi && tid < ept) {
            const uint32_t p = t * ppt + (tid >> 1);
            if (p < n_pairs32) pf_pair = P.perm ? P.perm[p] : p;
        }
    };
    auto prefetch_headers = [&]() {  // of the tile whose pair order sits in pf_pair
        if (pf_pair != 0xFFFFFFFFu) {
            pf_gend = 2u * pf_pair + (tid & 1u);
            pf_gwoff = P.rd.woff[pf_gend];
            pf_meta = P.rd.meta[pf_gend];
            if (has_inv) pf_inv = P.rd.inv4[pf_gend];
        }
    };
    // One credited maximal exact match into the tile's (end, node) table.
    auto credit = [&](uint32_t e, uint32_t node, uint32_t nlen, uint32_t add, uint32_t minp, uint32_t a) {
        const uint32_t key = (e << 25) | node;
        uint32_t at = P12 ? __umulhi(key * 0x9E3779B1u, C_POOL) : (key * 0x9E3779B1u) >> pool_shift;
        bool placed = false;
        for (uint32_t pr = 0; pr < 64u; pr++) {
            const uint32_t old = atomicCAS(&s_hkey[at], EMPTY_NODE, key);
            if (old == EMPTY_NODE || old == key) {
                atomicAdd(&s_hcnt[at], add);
                atomicMin(&s_hminp[at], minp);
                // (straight-line instantiations: reads <= 191 bases, so the node length rides in the
                // upper 24 bits -- equal for every update of the slot -- and P4 needs no header)
                atomicMin(&s_hminj[at], FAST ? (nlen << AB) | a : a);
                placed = true;
                break;
            }
            at = P12 ? (at + 1u == C_POOL ? 0u : at + 1u) : (at + 1u) & (pool - 1u);
        }
        if (!placed) atomicOr(&s_state[e], 2u);
    };
    // The first tile's headers and words are fetched the plain way; from then on the headers of tile
    // t+1 sit in registers during tile t, are put into the other LDS copy at its start, and the words
    // of tile t+1 follow them there as LDS-direct loads (global_load_lds: no registers, nothing waits
    // for them until just before P4) -- P0 of the next tile finds everything in place.
    const uint32_t lane0 = tid & 63u, wv0 = tid >> 6;
    prefetch_pair(tile_lo);
    prefetch_headers();
    {
        const uint32_t np0 = n_pairs32 - tile_lo * ppt;
        const uint32_t ne0 = 2u * (np0 < ppt ? np0 : ppt);
        if (tid < ne0) {
            s_gend[tid] = pf_gend;
            s_gwoff[tid] = pf_gwoff;
            s_meta[tid] = pf_meta;
        }
        cur_inv = pf_inv;
        if (tid < 8u) { s_words[words_cap + tid] = 0u; s_words[wcap + words_cap + tid] = 0u; }  // pads of both copies
        __syncthreads();
        for (uint32_t i = tid; i < ne0 * wpe; i += TTPB) {
            const uint32_t e = STD ? i / STD_WPE : vs_fastdiv(i, P.magic_wpe), k = i - e * wpe;
            const uint32_t nw = ((s_meta[e] & VS_LEN_MASK) + 15u) >> 4;
            s_words[i] = k < nw ? P.rd.words[s_gwoff[e] + k] : 0u;
        }
    }
    prefetch_pair(tile_lo + 1u);
    prefetch_headers();
    prefetch_pair(tile_lo + 2u);
    // (PRE) this thread's probe of the tile, begun a tile early: key (strand in bit 63), home slot and that slot's words
    uint64_t pre_key = 0;
    uint32_t pre_sl = 0;
    uint4 pre_raw = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t tile = tile_lo; tile < tile_hi; tile++) {
        uint32_t ltop = tid;  // (nothing P0 .. P2 derive from the thread index is hoisted out of the tile loop: see the 768-slot table)
        asm volatile("" : "+v"(ltop));
        const uint32_t p0 = tile * ppt;
        const uint32_t npair = (n_pairs32 - p0) < ppt ? (n_pairs32 - p0) : ppt;
        const uint32_t ne = 2u * npair;
        const uint32_t cur = (tile - tile_lo) & 1u, nxt = cur ^ 1u;
        s_gwoff = vs_lds + T.woff + cur * hw;
        s_gend = vs_lds + T.gend + cur * ept;
        s_meta = vs_lds + T.meta + cur * ept;
        s_words = vs_lds + T.words + cur * wcap;
        uint32_t *n_gwoff = vs_lds + T.woff + nxt * hw, *n_gend = vs_lds + T.gend + nxt * ept;
        uint32_t *n_meta = vs_lds + T.meta + nxt * ept, *n_words = vs_lds + T.words + nxt * wcap;
        uint32_t ne1 = 0;  // ends of the next tile of this run
        if (tile + 1u < tile_hi) {
            const uint32_t np1 = n_pairs32 - (tile + 1u) * ppt;
            ne1 = 2u * (np1 < ppt ? np1 : ppt);
        }
        __syncthreads();  // previous tile fully consumed; this tile's words have landed (see before P4)
        // ---- P0: the next tile's headers go to the other copy, the (end, node) table is emptied
        if (ltop < ne1) {
            n_gend[ltop] = pf_gend;
            n_gwoff[ltop] = pf_gwoff;
            n_meta[ltop] = pf_meta;
        }
        if (has_inv && ltop < ept) {  // (one copy is enough: nothing reads it before the barrier below)
            s_inv[ltop] = cur_inv;
            cur_inv = pf_inv;
        }
        for (uint32_t i = ltop; i < pool; i += TTPB) {
            s_hkey[i] = EMPTY_NODE;
            s_hcnt[i] = 0;
            s_hminp[i] = 0xFFFFFFFFu;
            s_hminj[i] = 0xFFFFFFFFu;
        }
        __syncthreads();
        prefetch_headers();            // tile + 2 (its pair order arrived during the previous tile)
        prefetch_pair(tile + 3u);
        // packed reads of the next tile: one end per wpe-word slot; a wavefront's load instruction
        // fills 64 consecutive LDS words, every lane from its own global address
        for (uint32_t b64 = wv0 * 64u; b64 < ne1 * wpe; b64 += TTPB) {
            const uint32_t i = b64 + lane0;
            if (i < ne1 * wpe) {
                const uint32_t e = STD ? i / STD_WPE : vs_fastdiv(i, P.magic_wpe), k = i - e * wpe;
                const uint32_t nw = ((n_meta[e] & VS_LEN_MASK) + 15u) >> 4;
                // (words behind the read's last one are never looked at: they get a copy of the last)
                if (nw) __builtin_amdgcn_global_load_lds(P.rd.words + n_gwoff[e] + (k < nw ? k : nw - 1u), n_words + b64, 4, 0, 0);
            }
        }
        // pair classification (PE_Inference.py:160-165): one thread per pair
        if (ltop < npair) {
            uint32_t mf = s_meta[2 * ltop], mr = s_meta[2 * ltop + 1];
            // (a slot without a second end, VS_FLAG_ABSENT, is classified from its first end alone: VS_FILTER_LEN_MASK)
            uint32_t cls;
            if (((mf | mr) >> 24) & VS_FLAG_N) cls = 0;
            else if ((mf & VS_LEN_MASK) < K || (mr & VS_FILTER_LEN_MASK) < K) cls = 1;
            else cls = 2;
            atomicAdd(&s_misc[12 + cls], 1u);
            uint32_t st = (cls == 2) ? 1u : 0u;
            // (an end with more bytes outside ACGT than vs_seed_limits can hold: the pair takes the overflow path)
            if (FAST && st && (((mf | mr) >> 24) & VS_FLAG_MANY)) st = 3u;
            // the probe grid of either end.  Plain: phi, phi + s, ... (vs_seed_phase: the shortest exact grid for the end's
            // length), phi in bits 8..31.  ADAPT: base s - 1 in bits 8..15, the step point t in bits 16..19 (set by P1), the
            // shift D in bits 20..27 (0: the length leaves one phase only)
            auto grid_bits = [&](uint32_t len) {
                if (!ADAPT || !(st & 1u)) return vs_seed_phase(len, w, s) << 8;
                const uint32_t r = (len - w) % s;
                return ((s - 1u) << 8) | ((r + 2u <= s ? s - 2u - r : 0u) << 20);
            };
            s_state[2 * ltop] = st | grid_bits(mf & VS_LEN_MASK);
            s_state[2 * ltop + 1] = st | grid_bits(mr & VS_LEN_MASK);
            s_ns[2 * ltop] = s_ns[2 * ltop + 1] = 0;
        }
        __syncthreads();
        // ---- P1: probes
        if (ADAPT) {
            // one grid position per thread; both candidate offsets probed with their slot loads in flight together
            const uint32_t it = ltop;
            const uint32_t e = it / (STD ? STD_PMAX : 1u), pi = it - e * pmax;
            uint32_t c0 = 0, pa0 = 0, pb0 = 0, c1 = 0, pa1 = 0, pb1 = 0, D = 0;
            const uint32_t est = (it < NI && e < ne) ? s_state[e] : 0u;
            const bool used = (est & 3u) == 1u;
            if (used) {
                const uint32_t meta = s_meta[e], rlen = meta & VS_LEN_MASK;
                D = est >> 20;
                const uint32_t j0 = ((est >> 8) & 0xFFu) + pi * s, j1 = j0 - D;
                if (j0 + w <= rlen) {
                    bool ok0 = true, ok1 = D != 0u;
                    if ((meta >> 24) & VS_FLAG_INVALID) {
                        uint32_t lo, hi;
                        ok0 = vs_seed_limits(s_inv[e], j0, w, rlen, &lo, &hi);
                        if (D) ok1 = vs_seed_limits(s_inv[e], j1, w, rlen, &lo, &hi);
                    }
                    uint32_t sr0, sr1;
                    const uint64_t key0 = vs_seed_key(s_words, e * wpe * 16u + j0, w, &sr0);
                    const uint64_t key1 = vs_seed_key(s_words, e * wpe * 16u + j1, w, &sr1);
                    const uint4 *tab = (const uint4 *)P.idx.table;
                    const uint32_t sl0 = vs_slot_of(key0, P.idx.table_bits), sl1 = vs_slot_of(key1, P.idx.table_bits);
                    uint4 r0 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u), r1 = r0;  // (VS_EMPTY_KEY: a seed that is not probed misses)
                    if (ok0) r0 = tab[sl0];
                    if (ok1) r1 = tab[sl1];
                    c0 = vs_probe_from(P.idx, key0, sr0, sl0, r0, &pa0, &pb0);
                    c1 = vs_probe_from(P.idx, key1, sr1, sl1, r1, &pa1, &pb1);
                    if (!D) { c1 = c0; pa1 = pa0; pb1 = pb0; }
                }
            }
            if (it < NI) { s_pa[it] = c0; s_pb[it] = c1; }  // (staged: every thread of an end needs the end's counts)
            __syncthreads();
            uint32_t cnt = c0, pa = pa0, pb = pb0;
            if (used && D) {
                // postings of the grid with step point t: positions below t unmoved, the others moved; the first minimum
                const uint32_t b = e * pmax;
                uint32_t cur = 0;
                for (uint32_t i = 0; i < pmax; i++) cur += s_pb[b + i];
                uint32_t best = cur, bt = 0;
                for (uint32_t t = 1; t <= pmax; t++) {
                    cur += s_pa[b + t - 1u] - s_pb[b + t - 1u];
                    if (cur < best) { best = cur; bt = t; }
                }
                if (pi >= bt) { cnt = c1; pa = pa1; pb = pb1; }
                if (pi == 0u) s_state[e] = est | (bt << 16);
            }
            __syncthreads();
            if (it < NI) {
                s_pcnt[it] = cnt;
                s_pa[it] = pa;
                s_pb[it] = pb;
            }
        } else
        for (uint32_t it = ltop; it < NI; it += TTPB) {
            uint32_t e = STD ? it / STD_PMAX : vs_fastdiv(it, P.magic_pmax), pi = it - e * pmax;
            uint32_t cnt = 0, pa = 0, pb = 0;
            const uint32_t est = e < ne ? s_state[e] : 0u;
            if ((est & 3u) == 1u) {
                uint32_t meta = s_meta[e];
                uint32_t rlen = meta & VS_LEN_MASK;
                uint32_t j = (est >> 8) + pi * s;
                // (PRE) a clean end of a tile behind the run's first: the test the previous tile made when it began this probe
                // (same header, same grid), so the probe is finished from its home slot, which has arrived; a dirty end, whose
                // limits need inv4, and the first tile of a run take the plain probe
                if (PRE && tile != tile_lo && j + w <= rlen && !((meta >> 24) & VS_FLAG_INVALID)) {
                    cnt = vs_probe_from(P.idx, pre_key & ~(1ull << 63), (uint32_t)(pre_key >> 63), pre_sl, pre_raw, &pa, &pb);
                } else if (j + w <= rlen) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(s_words, e * wpe * 16u + j, w, &sr);
                    bool ok = true;
                    if ((meta >> 24) & VS_FLAG_INVALID) {
                        if (FAST) {
                            uint32_t lo, hi;
                            ok = vs_seed_limits(s_inv[e], j, w, rlen, &lo, &hi);
                        } else {
                            ok = !vs_seed_dirty(P.rd.mask, (uint64_t)s_gwoff[e] * 16u + j, w);
                        }
                    }
                    if (ok) cnt = vs_probe(P.idx, key, sr, &pa, &pb);
                }
            }
            s_pcnt[it] = cnt;
            s_pa[it] = pa;
            s_pb[it] = pb;
        }
        __syncthreads();
        // ---- P2: inclusive scan of the postings per probe, s_pcnt[0..NI)
        {
            const uint32_t chunk = (NI + TTPB - 1u) / TTPB;
            const uint32_t b = ltop * chunk;
            uint32_t local = 0;
            for (uint32_t i = 0; i < chunk; i++)
                if (b + i < NI) local += s_pcnt[b + i];
            const uint32_t incl = vs_wave_scan_add(local);
            const uint32_t lane = ltop & 63u;
            if (lane == 63u) s_misc[ltop >> 6] = incl;
            __syncthreads();
            uint32_t off = incl - local;
            for (uint32_t wv = 0; wv < (ltop >> 6); wv++) off += s_misc[wv];
            for (uint32_t i = 0; i < chunk; i++)
                if (b + i < NI) {
                    off += s_pcnt[b + i];
                    s_pcnt[b + i] = off;
                }
        }
        __syncthreads();
        // ---- P3: one thread per posting.  Expansion of the per-probe posting counts (CSR-style
        // frontier expansion) in chunks of KCHUNK postings: every probe marks the first position it
        // owns in the chunk, a workgroup-wide running maximum fills the gaps, and each thread ends
        // up with the owners of its KPPT consecutive postings in registers.
        {
        const uint32_t total = s_pcnt[NI - 1u];
        for (uint32_t c0 = 0; c0 < total; c0 += KCHUNK) {
            for (uint32_t i = tid; i < KCHUNK; i += TTPB) s_owner[i] = 0;
            __syncthreads();
            for (uint32_t it = tid; it < NI; it += TTPB) {
                const uint32_t incl = s_pcnt[it], excl = s_pcnt[(int)it - 1];
                if (incl > excl) {
                    const uint32_t lo = excl > c0 ? excl : c0;
                    const uint32_t hi = incl < c0 + KCHUNK ? incl : c0 + KCHUNK;
                    if (lo < hi) s_owner[lo - c0] = it + 1u;
                }
            }
            __syncthreads();
            uint32_t own[KPPT];
            uint32_t run = 0;
#pragma unroll
            for (uint32_t k2 = 0; k2 < KPPT; k2++) {
                const uint32_t v = s_owner[tid * KPPT + k2];
                run = v > run ? v : run;
                own[k2] = run;
            }
            const uint32_t incl = vs_wave_scan_max(run);
            const uint32_t lane = tid & 63u;
            if (lane == 63u) s_misc[4u + (tid >> 6)] = incl;
            uint32_t carry = __shfl_up(incl, 1, 64);
            if (lane == 0u) carry = 0;
            __syncthreads();
            {   // the wavefronts before this one (TTPB = 256: at most three)
                const uint32_t wv = tid >> 6;
#pragma unroll
                for (uint32_t pw = 0; pw + 1u < TTPB / 64u; pw++) {
                    const uint32_t mw = s_misc[4u + pw];
                    if (wv > pw) carry = mw > carry ? mw : carry;
                }
            }
            // The thread's KPPT postings go through stages with every stage done for all of them before
            // the next one starts: A) which posting (LDS) and its record (one global load for
            // multi-posting seeds; the node header for single ones), B) text windows + decision.
            bool live[KPPT];
            uint32_t p_e[KPPT], p_j[KPPT], p_node[KPPT], p_pos[KPPT], p_opp[KPPT];
            VsNodeMeta p_nm[KPPT];
#pragma unroll
            for (uint32_t k2 = 0; k2 < KPPT; k2++) {
                const uint32_t t = c0 + tid * KPPT + k2;
                live[k2] = t < total;
                const uint32_t it = live[k2] ? (own[k2] > carry ? own[k2] : carry) - 1u : 0u;
                const uint32_t excl = s_pcnt[(int)it - 1];
                const uint32_t cnt = s_pcnt[it] - excl;
                const uint32_t pa = s_pa[it], pb = s_pb[it];
                const uint32_t e = STD ? it / STD_PMAX : vs_fastdiv(it, P.magic_pmax), pi = it - e * pmax;
                p_e[k2] = e;
                // the probe's read offset, and above it (bits 16..) its distance from the probe before it: a match that reaches
                // that far down holds the earlier probe, which credits it
                uint32_t gap = s;
                {
                    const uint32_t est = s_state[e];
                    if (ADAPT) {
                        const uint32_t D = est >> 20, t = (est >> 16) & 15u;
                        p_j[k2] = ((est >> 8) & 0xFFu) + pi * s - (pi >= t ? D : 0u);
                        if (pi && pi == t) gap = s - D;
                    } else {
                        p_j[k2] = (est >> 8) + pi * s;
                    }
                }
                uint32_t node = pa, pos = pb & 0x7FFFFFFFu, opp = pb >> 31;
                p_nm[k2].woff = 0; p_nm[k2].len = 0;
                if (live[k2] && cnt != 1u) {  // (the record carries the node header: no second round trip)
                    const VsPosting po = vs_posting_unpack(P.idx.postings[pa + (t - excl)]);
                    node = po.node; pos = po.pos; opp = po.strand ^ (pb >> 31);
                    p_nm[k2].woff = po.woff; p_nm[k2].len = po.len;
                } else if (live[k2]) {
                    if (P.shortcut && s <= w && pi) {
                        // Overlapping seeds (s <= w): if the previous probe of this end holds the single
                        // posting one stride back on the same diagonal, the bases in between match too,
                        // so that probe (or an earlier one) owns this match -- no memory traffic needed.
                        const uint32_t excl2 = s_pcnt[(int)it - 2];  // (pi != 0, so it >= 1)
                        if (excl - excl2 == 1u && s_pa[it - 1u] == node) {
                            const uint32_t pbp = s_pb[it - 1u];
                            const uint32_t want = opp ? pos + gap : pos - gap;
                            if ((pbp >> 31) == opp && (pbp & 0x7FFFFFFFu) == want && (opp || pos >= gap)) live[k2] = false;
                        }
                    }
                    if (live[k2]) p_nm[k2] = P.idx.meta[node];
                }
                p_node[k2] = node; p_pos[k2] = pos; p_opp[k2] = opp;
                if (ADAPT) p_j[k2] |= gap << 16;
            }
#pragma unroll
            for (uint32_t k2 = 0; k2 < KPPT; k2++) {
                if (!live[k2]) continue;
                const uint32_t e = p_e[k2], j = ADAPT ? p_j[k2] & 0xFFFFu : p_j[k2], node = p_node[k2], opp = p_opp[k2];
                const uint32_t gap = ADAPT ? p_j[k2] >> 16 : s;
                VsNodeMeta nm = p_nm[k2];
                const uint32_t meta = s_meta[e];
                const uint32_t rlen = meta & VS_LEN_MASK;
                // either strand off the one (wave-uniform) text base: the reverse complements lie rc_delta words on
                const uint32_t *tw = P.idx.fwd_words;
                const uint32_t q = opp ? nm.len - p_pos[k2] - w : p_pos[k2];
                uint32_t a, qa, len;
                if (FAST) {
                    // the clean stretch [lo, hi) of the read around the seed bounds the match
                    uint32_t lo = 0u, hi = rlen;
                    if ((meta >> 24) & VS_FLAG_INVALID) vs_seed_limits(s_inv[e], j, w, rlen, &lo, &hi);
                    uint32_t cl = gap < j - lo ? gap : j - lo;
                    cl = cl < q ? cl : q;
                    uint32_t rem = hi - j - wv;
                    const uint32_t dr = nm.len - q - wv;
                    rem = rem < dr ? rem : dr;
                    uint32_t left = 0u, ext = 0u;
                    const uint32_t tb = (nm.woff + (opp ? P.idx.rc_delta : 0u)) * 16u;
                    if (MODE == 2) vs_agree_long(s_words, e * wpe * 16u, tw, tb + q, cl, tb + q + wv, rem, j, wv, &left, &ext);
                    else vs_agree_fast<STD>(s_words, e * wpe * 16u, tw, tb + q, cl, tb + q + wv, rem, j, wv, &left, &ext);
                    len = left + wv + ext;
                    if (left >= gap || len < K) continue;  // an earlier probe lies inside this match and owns it / too short
                    a = j - left;
                    qa = q - left;
                } else {
                    const uint32_t tb = (nm.woff + (opp ? P.idx.rc_delta : 0u)) * 16u;
                    const uint32_t *mk = ((meta >> 24) & VS_FLAG_INVALID) ? P.rd.mask : nullptr;
                    if (!vs_extend(s_words, e * wpe * 16u, rlen, tw, tb, nm.len, j, q, wv, s, K, mk, (uint64_t)s_gwoff[e] * 16u, &a, &qa, &len))
                        continue;
                }
                credit(e, node, nm.len, len - K + 1u, opp ? nm.len - qa - len : qa, a);
            }
            __syncthreads();  // the owner array is reused by the next chunk
        }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wavefront's LDS-direct loads of the next tile's words are in
        __syncthreads();
        // ---- P4: acceptance test per table slot; an accepted node takes the next position of its end's list
        // (r6) The lists are PACKED: first every slot is judged and the ends' list lengths counted (the slot keeps its
        // position, its count is not needed any more), then ONE wavefront turns the lengths -- rounded up to whole quads -- into
        // offsets by a prefix sum over the ends, then the nodes go to their places.  An end with more than LCAP nodes, or one
        // that does not fit what is left of the tile's region (ept * LC words), is an overflow end.
        // (the thread index is laundered through an empty asm: what this phase derives from it -- slot and end indices,
        // LDS and global addresses -- then cannot be hoisted out of the tile loop, where it would sit in vector registers
        // across P3, the phase the kernel's 96-register budget is made for)
        uint32_t lt = tid;
        asm volatile("" : "+v"(lt));
        // (PRE) the next tile's words are all in (the barrier above): begin this thread's probe of that tile.  Its offset
        // follows from the end's length alone; whether the pair is used is decided in the next P0 -- a probe begun for
        // nothing is dropped (the table is read-only).
        if (PRE) {  // (set on every path: the old probe is dead behind its P1, not kept across P3)
            pre_sl = 0;
            pre_key = 0;
            pre_raw = make_uint4(0u, 0u, 0u, 0u);
        }
        if (PRE && lt < NI) {
            const uint32_t e = lt / STD_PMAX, pi = lt - e * pmax;
            if (e < ne1) {  // (0 in the last tile of the run)
                const uint32_t meta = n_meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + pi * s;
                if (j + w <= rlen && !((meta >> 24) & VS_FLAG_INVALID)) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(n_words, e * wpe * 16u + j, w, &sr);
                    pre_key = key | ((uint64_t)sr << 63);
                    pre_sl = vs_slot_of(key, P.idx.table_bits);
                    pre_raw = ((const uint4 *)P.idx.table)[pre_sl];
                }
            }
        }
        // (compile-time shapes: a thread's four slots -- key and position -- stay in registers across the prefix sum)
        constexpr uint32_t SPT = STD ? C_POOL / TTPB : 1u;
        uint32_t r_key[SPT], r_at[SPT];
        auto judge = [&](uint32_t i, uint32_t key) -> uint32_t {  // the position of slot i's node in its end's list, or none
            const uint32_t e = key >> 25, node = key & 0x01FFFFFFu;
            const uint32_t rlen = s_meta[e] & VS_LEN_MASK;
            const uint32_t hj = s_hminj[i];
            const uint32_t nlen = FAST ? hj >> AB : P.idx.meta[node].len;
            const uint32_t minj = FAST ? hj & ((1u << AB) - 1u) : hj;
            if (FAST ? vs_accept32(s_hcnt[i], s_hminp[i], minj, nlen, rlen, K) : vs_accept(s_hcnt[i], s_hminp[i], minj, nlen, rlen, K))
                return atomicAdd(&s_ns[e], 1u);
            return 0xFFFFFFFFu;
        };
        if (STD) {
#pragma unroll
            for (uint32_t j = 0; j < SPT; j++) {
                const uint32_t i = lt + j * TTPB;
                r_key[j] = s_hkey[i];
                r_at[j] = r_key[j] != EMPTY_NODE ? judge(i, r_key[j]) : 0xFFFFFFFFu;
            }
        } else {
            for (uint32_t i = lt; i < pool; i += TTPB) {
                const uint32_t key = s_hkey[i];
                if (key != EMPTY_NODE) s_hcnt[i] = judge(i, key);
            }
        }
        __syncthreads();
        if (lt < 64u) {  // two ends per lane (ept <= TTPB / 2 = 128)
            const uint32_t e0 = 2u * lt, e1 = e0 + 1u;
            const uint32_t st0 = e0 < ne ? s_state[e0] : 0u, st1 = e1 < ne ? s_state[e1] : 0u;
            const uint32_t n0 = (st0 & 3u) == 1u ? s_ns[e0] : 0u, n1 = (st1 & 3u) == 1u ? s_ns[e1] : 0u;
            bool over0 = n0 > LCAP, over1 = n1 > LCAP;
            const uint32_t q0 = over0 ? 0u : (n0 + 3u) >> 2, q1 = over1 ? 0u : (n1 + 3u) >> 2;
            const uint32_t incl = vs_wave_scan_add(q0 + q1);
            const uint32_t capq = (ept * LC - C_TRIM) >> 2;
            const uint32_t o0 = incl - q0 - q1, o1 = o0 + q0;
            over0 |= o0 + q0 > capq;
            over1 |= o1 + q1 > capq;
            // (an end whose nodes are not placed -- overflow, or not an end of a used pair -- says so in its offset)
            if (e0 < ne) { s_pcnt[e0] = over0 || (st0 & 3u) != 1u ? 0xFFFFFFFFu : 4u * o0; if (over0) s_state[e0] = st0 | 2u; }
            if (e1 < ne) { s_pcnt[e1] = over1 || (st1 & 3u) != 1u ? 0xFFFFFFFFu : 4u * o1; if (over1) s_state[e1] = st1 | 2u; }
            if (lt == 63u) s_misc[8] = 4u * (incl < capq ? incl : capq);  // words of the tile's packed lists
        }
        __syncthreads();
        uint32_t *s_off = s_pcnt;  // (the scan of P2 is done with)
        if (STD) {
#pragma unroll
            for (uint32_t j = 0; j < SPT; j++)
                if (r_at[j] != 0xFFFFFFFFu) {
                    const uint32_t o = s_off[r_key[j] >> 25];
                    if (o != 0xFFFFFFFFu) s_list[o + r_at[j]] = r_key[j] & 0x01FFFFFFu;
                }
        } else {
            for (uint32_t i = lt; i < pool; i += TTPB) {
                const uint32_t key = s_hkey[i];
                if (key != EMPTY_NODE) {
                    const uint32_t at = s_hcnt[i], o = s_off[key >> 25];
                    if (at != 0xFFFFFFFFu && o != 0xFFFFFFFFu) s_list[o + at] = key & 0x01FFFFFFu;
                }
            }
        }
        __syncthreads();
        // pairs with an overflowed end go to the slow list
        if (lt < npair) {
            uint32_t st = s_state[2 * lt] | s_state[2 * lt + 1];
            if ((st & 1u) && (st & 2u)) {
                uint32_t at = atomicAdd(P.slow_count, 1u);
                P.slow_list[at] = s_gend[2 * lt] >> 1;
                s_state[2 * lt] |= 2u;
                s_state[2 * lt + 1] |= 2u;
            }
        }
        __syncthreads();
        // ---- P5: hand the accepted lists to the counter kernels, tile order; length 0 for ends of dropped pairs and of
        // pairs the slow path takes
        if (accumulate) {
            if (!P.out_rows) {  // the tile's packed lists as they lie in LDS: one coalesced stretch
                uint32_t *ol = P.out_lists + (uint64_t)tile * ept * LC;
                const uint32_t total = s_misc[8];
                for (uint32_t i = lt; i < total; i += TTPB) ol[i] = s_list[i];
                for (uint32_t i = lt; i < ne; i += TTPB) {
                    const uint32_t n = (s_state[i] & 3u) == 1u ? s_ns[i] : 0u;
                    P.out_counts[(uint64_t)tile * ept + i] = n ? n | (s_off[i] >> 2) << 8 : 0u;
                }
            } else {  // a row per end (+ its quad of the second array); a lane per (end, quad), only the quads that hold nodes
                uint32_t *ol = P.out_lists + (uint64_t)tile * ept * LC, *oh = P.out_lists_hi + (uint64_t)tile * ept * 4u;
                for (uint32_t i = lt; i < ne * (LCAP / 4u); i += TTPB) {
                    const uint32_t e = i / (LCAP / 4u), q4 = 4u * (i - e * (LCAP / 4u));
                    const uint32_t n = (s_state[e] & 3u) == 1u ? s_ns[e] : 0u;
                    if (q4 < n) {
                        const uint32_t *src = s_list + s_off[e] + q4;
                        *(VsQuad *)(q4 < LC ? ol + e * LC + q4 : oh + e * 4u) = VsQuad{src[0], src[1], src[2], src[3]};
                    }
                }
                for (uint32_t i = lt; i < ne; i += TTPB)
                    P.out_counts[(uint64_t)tile * ept + i] = (s_state[i] & 3u) == 1u ? s_ns[i] : 0u;
            }
        }
        if (want_dbg) {
            for (uint32_t i = tid; i < ne; i += TTPB) {
                if (s_state[i] & 2u) continue;  // the slow kernel reports these
                uint32_t n = s_ns[i];
                const uint64_t ge = s_gend[i];
                P.dbg_counts[ge] = n;
                for (uint32_t k2 = 0; k2 < n && k2 < P.dbg_cap; k2++) P.dbg_lists[ge * P.dbg_cap + k2] = s_list[s_off[i] + k2];
            }
        }
    }
    __syncthreads();
    if (tid < 3 && P.stats && s_misc[12 + tid]) atomicAdd(&P.stats[tid], (unsigned long long)s_misc[12 + tid]);
}

// ---- K4: counters ------------------------------------------------------------------------------------
// PE_Inference.py:174-188 from the per-end lists k_pe_tiles wrote (tile order = locus order).  A pair
// with lists l (nl nodes) and r (nr nodes) makes nl*nr node_mat increments and, per end, n(n+1)/2
// short_mat increments: positions a <= b give the cell (min, max) of the two node ids -- the
// reference's "i <= i2 over ascending indices" (:174-184).
// Scattered global atomics run at ~2e10/s chip-wide and would bound the whole step (5.4e8 increments
// at configs[2]), so increments are summed per cell in LDS before they reach memory.  Two loop orders:
//   * k_pe_accumulate (graphs of at most 46 340 nodes): pair-major.  A workgroup (1024 threads, one per CU, a
//     contiguous run of pairs = a few loci) sums in a 16k-slot cell table and issues ONE global atomic per cell when the
//     table is written out.  One wavefront takes 64 pairs at a time and counts them as TASKS, one per matrix row
//     (vs_acc_tasks.h), one lane per task, the tasks of a batch of pairs ordered by length.
//   * the row owners below (larger graphs): output-major.  There a round of locus-ordered pairs brings more distinct
//     cells than the table holds, and the same cell returns from loci hundreds of rounds apart.
// LDS of k_pe_accumulate: the cell table, per wavefront a region of task entries (its last words the queue of missed keys)
// and the counters of their sort, four words
#define ACC_LDS_BYTES ((2u * ACC_SLOTS + (ACC_TPB / 64) * (ACC_TASK_WORDS + ACC_BINS) + 4u) * 4u)
static_assert(ACC_LDS_BYTES <= 160u * 1024u, "k_pe_accumulate: one workgroup per CU");
// The cell table: 16 k slots, 32-bit keys (k_pe_accumulate: mat * N*N + x * N + y, while 2*N*N fits 32 bits, N <= 46340;
// the row owners: cell index relative to the strip's first row).  The 16 cells of one 64-byte stretch of a matrix row
// sit in 16 NEIGHBOURING slots (the hash picks a group of 16 slots from the key >> 4, the low four bits pick the slot
// inside it; a taken slot sends the probe to the same position of the next group).  A write-out walks the slots in
// order, a lane per slot, so the lanes of a wavefront that hold cells of one stretch issue their atomics side by side
// -- and integer atomics, like the float ones of MI355X_MICROARCH.md, leave the L2 as one memory-side request per
// 64-byte stretch a wave instruction touches.
template <uint32_t BITS>
struct CellTable {  // 1 << BITS slots
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    __device__ static uint32_t key(uint32_t mat, uint32_t x, uint32_t y, uint32_t N) { return (mat * N + x) * N + y; }
    __device__ static uint32_t slot(uint32_t k) { return ((((k >> 4) * 0x9E3779B1u) >> (36u - BITS)) << 4) | (k & 15u); }
    __device__ static uint32_t next(uint32_t at) { return (at + 16u) & ((1u << BITS) - 1u); }
};
typedef CellTable<ACC_BITS> Acc32;  // k_pe_accumulate's

// The slot a key hashes to is empty or holds another cell: claim / probe on.  Kept out of line of the common case (the
// cell is already in the table), which stays a short straight-line sequence.  false: no place within eight probes.
template <typename TB>
__device__ __forceinline__ bool vs_cell_claim(uint32_t *s_key, uint32_t *s_cnt, uint32_t *s_used, uint32_t key, uint32_t at, uint32_t wgt) {
    for (uint32_t pr = 0; pr < 8u; pr++) {
        uint32_t kx = s_key[at];
        if (kx == TB::EMPTY) {
            kx = atomicCAS(&s_key[at], TB::EMPTY, key);
            if (kx == TB::EMPTY) { atomicAdd(s_used, 1u); kx = key; }
        }
        if (kx == key) {
            // (workgroup scope: with the scope of a caller's add to memory for the cell that found no place, the compiler
            // makes ONE flat atomic on a selected address of the two)
            __hip_atomic_fetch_add(&s_cnt[at], wgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return true;
        }
        at = TB::next(at);
    }
    return false;
}

// (the same wavefront writes and reads its own task region: no workgroup barrier, only the LDS wait)
__device__ __forceinline__ void vs_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// k_pe_accumulate, per round of 64 pairs of a wavefront (lane = pair):
//   batch  the longest run of the round's next pairs whose tasks fit the wavefront's task region (task_cap entries; a pair
//          has at most 40 tasks, so a batch holds at least one pair): a wavefront scan of the pairs' task counts
//   sort   every lane writes its pair's tasks, 16 bits each (vs_acc_task_entry), placed by a counting sort on their turns,
//          longest first: per pair at most eleven LDS atomics into the wavefront's counters (the node rows of a pair have
//          one length, the folded short rows of a list four -- vs_acc_fold_class -- its middle row one), a scan over the
//          counters, then plain stores
//   count  windows of 64 consecutive tasks, one per lane.  A lane decodes its entry ONCE (pair -> the lengths and places of
//          its lists by one cross-lane read, kind and position -> x, partner list, partner stretches) and walks its
//          partners in blocks of four list words -- one 16-byte load at the word the block starts at, issued one block
//          ahead; the decode, x and first block of the NEXT window are issued before this window is counted, so no global
//          load is waited on.  A turn is one key, one slot read, and an add where the slot holds the cell.  The block's
//          slot reads are written side by side, but as compiled the first is waited on before the second key is formed;
//          issuing all four ahead of one wait was measured and gains nothing (profiles/EXPERIMENTS.md, 2026-10-20b).  A
//          window ends with its longest task, which the order makes nearly every lane's end.
//   claim  a turn claims nothing.  With 64 lanes seven turns in eight have a lane whose cell is not in its slot (measured:
//          7.6 such lanes a turn, four in ten of them at a slot that holds another cell), and a claim is LDS round trips
//          one behind the other -- compare-and-swap, fill counter, add -- which the whole wavefront would walk for those
//          few lanes.  So the lanes that miss append their keys to the wavefront's QUEUE, the last ACC_QUEUE words of its
//          task region (which is why the plan hands out ACC_TASK_PLAN_CAP entries at most): the place from the ballot of
//          the misses and the lane's count of set bits below it, the length wave-uniform, from the ballot's popcount -- one
//          store, no wait, no divergent path.  When a turn's misses do not fit, and at the end of the round in front of the
//          barrier (so the fill and lost counters are complete when they are read and nothing waits across a write-out), the
//          wavefront drains the queue: lane i claims key i (vs_cell_claim, which reads the slot: what the turn saw is stale).
//          A key may wait there more than once, from several lanes and turns: every entry is worth one increment.
// gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage): 123 VGPRs, 0 B of scratch, ACC_LDS_BYTES = 163 344 B of the CU's 163 840 B
// of LDS: one workgroup of sixteen wavefronts per CU, four per SIMD (which 128 VGPRs allow).
__global__ void __launch_bounds__(ACC_TPB)
k_pe_accumulate(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ counts, uint64_t n_slots_pairs,
                uint32_t pairs_per_wg, uint32_t N, uint32_t use_table, uint32_t fill_limit, uint32_t task_cap,
                uint32_t *__restrict__ node_mat, uint32_t *__restrict__ short_mat, uint32_t *__restrict__ queue, uint32_t ept) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t *s_key = vs_lds;                      // [ACC_SLOTS]
    uint32_t *s_cnt = vs_lds + ACC_SLOTS;          // [ACC_SLOTS]
    uint32_t *s_bin = vs_lds + 2u * ACC_SLOTS + wv * (ACC_TASK_WORDS + ACC_BINS);  // [ACC_BINS] of this wavefront
    uint16_t *s_task = (uint16_t *)(s_bin + ACC_BINS);                             // [task_cap <= ACC_TASK_PLAN_CAP]
    uint32_t *s_q = s_bin + ACC_BINS + (ACC_TASK_WORDS - ACC_QUEUE);               // [ACC_QUEUE], the last words of the task region
    uint32_t *s_misc = vs_lds + 2u * ACC_SLOTS + (ACC_TPB / 64) * (ACC_TASK_WORDS + ACC_BINS);
    uint32_t &s_used = s_misc[0], &s_lost = s_misc[1], &s_chunk = s_misc[2];
    const uint32_t NN = N * N;  // (use_table: 2 * N * N fits 32 bits)
    for (uint32_t i = tid; i < ACC_SLOTS; i += ACC_TPB) { s_key[i] = Acc32::EMPTY; s_cnt[i] = 0; }
    if (tid == 0) { s_used = 0; s_lost = 0; }
    __syncthreads();
    // chunks of pairs_per_wg pairs: whichever chunk is next when this workgroup is free -- the table lives across chunks
    // and is written out on fill only
    const uint32_t ppt = ept >> 1, region_q = (ept * LC) >> 2;  // pairs per tile of the mapping kernel; quads of a tile's region
    // every cell of the table to its counter (one global atomic per cell), the table emptied
    auto write_out = [&]() {
        for (uint32_t i = tid; i < ACC_SLOTS; i += ACC_TPB) {
            const uint32_t key = s_key[i];
            if (key != Acc32::EMPTY) {
                atomicAdd(key >= NN ? short_mat + (key - NN) : node_mat + key, s_cnt[i]);
                s_key[i] = Acc32::EMPTY;
                s_cnt[i] = 0;
            }
        }
        if (tid == 0) { s_used = 0; s_lost = 0; }
        __syncthreads();
    };
    // the keys this wavefront has found no cell for yet: claimed ACC_QUEUE at a time, lane i takes key i -- the slot is read
    // again, what the turn saw there is stale -- and none waits beyond the round
    uint32_t qn = 0;  // keys waiting (wave-uniform)
    auto drain = [&]() {
        vs_wave_lds_sync();
        if (lane < qn) {
            const uint32_t key = s_q[lane];
            if (!vs_cell_claim<Acc32>(s_key, s_cnt, &s_used, key, Acc32::slot(key), 1u)) {
                atomicAdd(&s_lost, 1u);
                atomicAdd(key >= NN ? short_mat + (key - NN) : node_mat + key, 1u);
            }
        }
        vs_wave_lds_sync();
        qn = 0;
    };
    for (;;) {
    __syncthreads();
    if (tid == 0) s_chunk = atomicAdd(queue, 1u);
    __syncthreads();
    const uint64_t chunk = s_chunk;
    const uint64_t lo = chunk * pairs_per_wg;
    if (lo >= n_slots_pairs) break;
    const uint64_t hi = lo + pairs_per_wg < n_slots_pairs ? lo + pairs_per_wg : n_slots_pairs;
    // a round = ACC_PPW pairs per wavefront
    for (uint64_t base = lo; base < hi; base += (ACC_TPB / 64u) * ACC_PPW) {
        const uint64_t wbase = base + wv * ACC_PPW;         // wave-uniform
        const uint32_t *wcounts = counts + 2u * wbase;
        // the lists are packed per tile of the mapping kernel (k_pe_tiles P4 / P5): where a pair's two lists start, in quads
        // from the region of the wavefront's first tile -- at most 64 pairs further on, so 11 bits each, next to the lengths
        const uint64_t tile0 = wbase / ppt;                 // wave-uniform
        const uint32_t rem0 = (uint32_t)(wbase - tile0 * ppt);
        const uint32_t *wlists = lists + tile0 * ept * LC;
        uint32_t nl = 0, nr = 0, packed = 0;
        if (wbase + lane < hi) {
            const uint2 c = *(const uint2 *)(wcounts + 2u * lane);
            nl = c.x & 0xFFu; nr = c.y & 0xFFu;
            const uint32_t tq = (rem0 + lane) / ppt * region_q;
            packed = nl | nr << 5 | (tq + (c.x >> 8)) << 10 | (tq + (c.y >> 8)) << 21;
        }
        const uint32_t my_tasks = vs_acc_pair_tasks(nl, nr);
        for (uint32_t first = 0; first < ACC_PPW;) {  // the batches of the round (wave-uniform)
            const uint32_t incl = vs_wave_scan_add(lane >= first ? my_tasks : 0u);
            const uint32_t last = (uint32_t)__popcll(__ballot(vs_acc_batch_fits(incl, task_cap)));  // (the lanes that fit are a prefix)
            const uint32_t U = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)last - 1);  // tasks of the batch
            const bool mine = lane >= first && lane < last;
            first = last;
            if (!U) continue;
            // ---- sort: counters per partner count, then the places, longest first
            if (lane < ACC_BINS) s_bin[lane] = 0u;
            vs_wave_lds_sync();
            uint32_t o_n = 0, o_lm = 0, o_rm = 0, o_l[4], o_r[4];  // this pair's places among the tasks of one length
            if (mine) {
                if (nl && nr) o_n = atomicAdd(&s_bin[nr], nl);
                if (nl & 1u) o_lm = atomicAdd(&s_bin[(nl + 1u) >> 1], 1u);
                if (nr & 1u) o_rm = atomicAdd(&s_bin[(nr + 1u) >> 1], 1u);
#pragma unroll
                for (uint32_t r = 0; r < 4u; r++) {
                    const VsAccClass cl = vs_acc_fold_class(nl, r), cr = vs_acc_fold_class(nr, r);
                    o_l[r] = cl.cnt ? atomicAdd(&s_bin[cl.turns], cl.cnt) : 0u;
                    o_r[r] = cr.cnt ? atomicAdd(&s_bin[cr.turns], cr.cnt) : 0u;
                }
            }
            vs_wave_lds_sync();
            {
                const uint32_t v = lane < ACC_BINS ? s_bin[ACC_BINS - 1u - lane] : 0u;
                const uint32_t before = vs_wave_scan_add(v) - v;
                if (lane < ACC_BINS) s_bin[ACC_BINS - 1u - lane] = before;  // (every lane rewrites the counter it read)
            }
            vs_wave_lds_sync();
            if (mine) {
                if (nl && nr) {
                    const uint32_t at = s_bin[nr] + o_n;
                    for (uint32_t a = 0; a < nl; a++) s_task[at + a] = vs_acc_task_entry(lane, VS_ACC_NODE, a);
                }
                if (nl & 1u) s_task[s_bin[(nl + 1u) >> 1] + o_lm] = vs_acc_task_entry(lane, VS_ACC_LEFT, nl >> 1);
                if (nr & 1u) s_task[s_bin[(nr + 1u) >> 1] + o_rm] = vs_acc_task_entry(lane, VS_ACC_RIGHT, nr >> 1);
                // (the classes are worked out again from laundered lengths: kept from above they cost 24 registers and scratch)
                uint32_t nl2 = nl, nr2 = nr;
                asm volatile("" : "+v"(nl2), "+v"(nr2));
#pragma unroll
                for (uint32_t r = 0; r < 4u; r++) {
                    const VsAccClass cl = vs_acc_fold_class(nl2, r), cr = vs_acc_fold_class(nr2, r);
                    if (cl.cnt) {
                        const uint32_t at = s_bin[cl.turns] + o_l[r];
                        for (uint32_t i = 0; i < cl.cnt; i++) s_task[at + i] = vs_acc_task_entry(lane, VS_ACC_LEFT, cl.a0 + 4u * i);
                    }
                    if (cr.cnt) {
                        const uint32_t at = s_bin[cr.turns] + o_r[r];
                        for (uint32_t i = 0; i < cr.cnt; i++) s_task[at + i] = vs_acc_task_entry(lane, VS_ACC_RIGHT, cr.a0 + 4u * i);
                    }
                }
            }
            vs_wave_lds_sync();
            // ---- count.  A lane's task, decoded: x (a node row's; a short row takes the first word of either stretch),
            // the partner list, the position the next block starts at, the stretches (vs_acc_tasks.h), the first block.
            struct Task {
                uint32_t x, mat, off, p, p2, e, turns;
                VsQuad q;
            };
            auto decode = [&](uint32_t t0) {
                Task T;
                const uint32_t w = t0 + lane < U ? s_task[t0 + lane] : 0u;  // (0: no task, no turns, every load at the region's first word)
                const uint32_t kind = vs_acc_entry_kind(w), a = vs_acc_entry_a(w);
                // list lengths and places of the task's pair: the lane of that pair holds them (ONE cross-lane read, no memory round trip)
                const uint32_t pk = __shfl(packed, (int)vs_acc_entry_pair(w), 64);
                const uint32_t ql = pk & 31u, qr = (pk >> 5) & 31u, rowl = ((pk >> 10) & 0x7FFu) << 2, rowr = (pk >> 21) << 2;
                const VsAccSegs s = w ? vs_acc_task_segs(kind, a, ql, qr) : VsAccSegs{0u, 0u, 0u};
                T.turns = vs_acc_turns(s);
                T.mat = kind != VS_ACC_NODE ? 1u : 0u;
                T.off = !w ? 0u : kind == VS_ACC_LEFT ? rowl : rowr;
                T.p = s.p1; T.p2 = s.p2; T.e = s.e;
                T.x = 0u;
                if (w && kind == VS_ACC_NODE) T.x = wlists[rowl + a];
                // (reading a few words past `e` -- the list's padding, the next list -- stays inside the lists buffer, which
                // carries padding at its end, and is ignored)
                T.q = *(const VsQuad *)(wlists + T.off + T.p);  // one 16-byte load
                return T;
            };
            Task nxt = decode(0u);
            for (uint32_t t0 = 0; t0 < U; t0 += 64u) {
                const Task c = nxt;
                if (t0 + 64u < U) nxt = decode(t0 + 64u);
                const uint32_t tmax = (uint32_t)__builtin_amdgcn_readlane((int)vs_wave_scan_max(c.turns), 63);  // the window's longest task (wave-uniform)
                const uint32_t mat = c.mat, e = c.e;
                const uint32_t *plist = wlists + c.off;
                uint32_t x = c.x, p = c.p, p2 = c.p2;
                bool fresh = true;  // the block begins a stretch
                VsQuad q = c.q;
                for (uint32_t t = 0; t < tmax; t += 4u) {
                    const uint32_t ys[4] = {q.x, q.y, q.z, q.w};
                    if (mat && fresh) x = ys[0];
                    const uint32_t pb = p;
                    // the next block: on in this stretch, or the first of the second one, or none (p = e)
                    p += 4u;
                    fresh = p >= e;
                    if (fresh) { p = p2; p2 = e; }
                    if (t + 4u < tmax) q = *(const VsQuad *)(plist + p);
                    const uint32_t left = tmax - t;  // turns of the window still to come (wave-uniform)
                    if (use_table) {
                        // the block's cells' slots are read (independent LDS loads), then counted; the key of a slot that
                        // does not hold the cell yet waits in the queue for the slow way (claim / probe / global)
                        uint32_t key[4], seen[4], at[4];
#pragma unroll
                        for (uint32_t j = 0; j < 4u; j++) {
                            if (j >= left) break;
                            const uint32_t yv = ys[j];
                            const uint32_t cx = (mat && yv < x) ? yv : x, cy = (mat && yv < x) ? x : yv;
                            key[j] = Acc32::key(mat, cx, cy, N);
                            at[j] = Acc32::slot(key[j]);
                            seen[j] = s_key[at[j]];
                        }
#pragma unroll
                        for (uint32_t j = 0; j < 4u; j++) {
                            if (j >= left) break;
                            const bool on = pb + j < e;
                            if (on && seen[j] == key[j]) atomicAdd(&s_cnt[at[j]], 1u);
                            // the lanes that missed queue their keys: places from the ballot, the length wave-uniform
                            const bool miss = on && seen[j] != key[j];
                            const uint64_t mm = __ballot(miss);
                            if (mm) {
                                const uint32_t n_miss = (uint32_t)__popcll(mm);
                                if (qn + n_miss > ACC_QUEUE) drain();
                                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u));
                                if (miss) s_q[qn + before] = key[j];
                                qn += n_miss;
                            }
                        }
                    } else {
                        // (VS_NO_AGG=1: every increment a global atomic)
#pragma unroll
                        for (uint32_t j = 0; j < 4u; j++) {
                            if (pb + j >= e) continue;
                            const uint32_t yv = ys[j];
                            const uint32_t cx = (mat && yv < x) ? yv : x, cy = (mat && yv < x) ? x : yv;
                            atomicAdd((mat ? short_mat : node_mat) + (uint64_t)cx * N + cy, 1u);
                        }
                    }
                }
            }
        }
        if (qn) drain();  // (s_used and s_lost are complete when they are read, nothing waits across a write-out)
        __syncthreads();
        const bool spill = s_used > fill_limit || s_lost > 4096u;
        __syncthreads();
        // (everything goes, also the cells of the locus still being worked on: keeping those across
        // write-outs was measured -- 3.1 -> 3.9 ms -- the table is only fast while nearly empty, when a
        // cell sits in the first slot its key hashes to)
        if (spill) write_out();
    }
    }
    __syncthreads();
    write_out();
}

// ---- which tiles of the counters a block touches (vs_pe_count_tracked) -------------------------------------------------
// A pair adds to node_mat[l][r] for l in its left list, r in its right list, and to short_mat[min][max] for the pairs of
// nodes of either list (PE_Inference.py:174-188): one lane per pair marks the 64 x 64 tiles those cells lie in, from the
// same list rows k_pe_accumulate counts (the overflow kernels and the row owners mark theirs where they add).  A caller that zeroes its
// counters before every block then zeroes these tiles only (k_zero_tiles) -- a few per cent of a 50 k-node matrix.
__global__ void __launch_bounds__(256) k_mark_tiles(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ counts,
                                                   uint64_t n_slots_pairs, uint8_t *__restrict__ map, uint32_t T, uint32_t ept) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_slots_pairs) return;
    const uint32_t cl = counts[2u * p], cr = counts[2u * p + 1u], nl = cl & 0xFFu, nr = cr & 0xFFu;
    if (!nl && !nr) return;
    // (packed lists: the region of the pair's tile, the quad offsets of its two ends)
    const uint32_t *region = lists + 2u * p / ept * ept * LC, *rl = region + 4u * (cl >> 8), *rr = region + 4u * (cr >> 8);
    uint8_t *smap = map + (uint64_t)T * T;
    // The distinct tile coordinates (node >> 6) of a list, up to eight of them, in registers (every index below is a
    // compile-time constant: no scratch memory).  The rows come as 16-byte loads, only as many as the list is long.  A list
    // with more than eight distinct coordinates takes the plain way.
    uint32_t tl[8], tr[8], kl = 0, kr = 0;
    bool over = false;
    auto put = [&](uint32_t (&tt)[8], uint32_t &k, uint32_t t) {
        bool seen = false;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) seen |= j < k && tt[j] == t;
        if (seen) return;
        if (k >= 8u) { over = true; return; }
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++)
            if (j == k) tt[j] = t;
        k++;
    };
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) { tl[j] = 0u; tr[j] = 0u; }
#pragma unroll
    for (uint32_t q = 0; q < LCAP / 4u; q++) {
        if (4u * q < nl) {
            const VsQuad v = *(const VsQuad *)(rl + 4u * q);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
                if (4u * q + i < nl) put(tl, kl, e[i] >> 6);
        }
        if (4u * q < nr) {
            const VsQuad v = *(const VsQuad *)(rr + 4u * q);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
                if (4u * q + i < nr) put(tr, kr, e[i] >> 6);
        }
    }
    if (over) {
        for (uint32_t i = 0; i < nl; i++)
            for (uint32_t j = 0; j < nr; j++) vs_mark_tile(map, T, 0u, rl[i], rr[j]);
        for (uint32_t side = 0; side < 2u; side++) {
            const uint32_t *row = side ? rr : rl;
            const uint32_t n = side ? nr : nl;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t j = 0; j < n; j++) {
                    const uint32_t x = row[i], y = row[j];
                    if (x <= y) vs_mark_tile(map, T, 1u, x, y);
                }
        }
        return;
    }
#pragma unroll
    for (uint32_t a = 0; a < 8u; a++)
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++)
            if (a < kl && b < kr) {
                const uint64_t t = (uint64_t)tl[a] * T + tr[b];
                if (!map[t]) map[t] = 1;
            }
    // short_mat: a cell sits at (smaller node, larger node), its tile at (smaller, larger) tile coordinates
#pragma unroll
    for (uint32_t a = 0; a < 8u; a++)
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++) {
            if (a < kl && b < kl && tl[a] <= tl[b]) {
                const uint64_t t = (uint64_t)tl[a] * T + tl[b];
                if (!smap[t]) smap[t] = 1;
            }
            if (a < kr && b < kr && tr[a] <= tr[b]) {
                const uint64_t t = (uint64_t)tr[a] * T + tr[b];
                if (!smap[t]) smap[t] = 1;
            }
        }
}

// every marked tile of both matrices to zero, the map cleared.  (r6) A wavefront looks at 64 map bytes at once (a lane each) and
// zeroes the marked ones among them, a lane per column -- one workgroup per tile meant 1.45 M launches of which 2 % had work
// (0.33 ms at configs[4]).
__global__ void __launch_bounds__(64) k_zero_tiles(uint32_t *__restrict__ node_mat, uint32_t *__restrict__ short_mat, uint32_t N, uint32_t T,
                                                  uint8_t *__restrict__ map, uint64_t n_tiles) {
    const uint64_t t0 = (uint64_t)blockIdx.x * 64u;
    const uint64_t mine = t0 + threadIdx.x;
    const bool marked = mine < n_tiles && map[mine] != 0;
    unsigned long long todo = __ballot(marked);
    if (marked) map[mine] = 0;
    while (todo) {
        const uint32_t k = (uint32_t)__ffsll((long long)todo) - 1u;
        todo &= todo - 1ull;
        const uint64_t t = t0 + k;
        const uint32_t mat = (uint32_t)(t / ((uint64_t)T * T));
        const uint64_t r = t - (uint64_t)mat * T * T;
        const uint32_t x0 = (uint32_t)(r / T) << 6, y = (((uint32_t)(r % T)) << 6) + threadIdx.x;
        uint32_t *m = mat ? short_mat : node_mat;
        if (y < N)
            for (uint32_t x = x0; x < x0 + 64u && x < N; x++) m[(uint64_t)x * N + y] = 0u;
    }
}

// ---- both matrices by ROW OWNERS (graphs beyond the one-table shape of the cell table) ---------------------------------
// In locus order a round of 1 024 pairs of a 54 k-node graph brings ~30 k distinct cells, more than an LDS table holds,
// and the same cell comes back from loci hundreds of rounds apart: 4.4e9 increments left the pair-major kernel as 7.9e8
// memory-side atomics for 2.9e7 distinct cells (configs[4]; tools/cell_probe.py).  Turned round -- output-major -- the
// sums fit: ONE matrix row has a few hundred distinct cells however many pairs add to it.  So the lists are transposed
// (row x -> the items whose list holds x: a counting sort of one word per listed node), a workgroup owns a strip of rows
// at a time, adds the partner lists of the strip's items into its LDS cell table, and writes every cell ONCE.
// PE_Inference.py:174-188 is the loop nest being reordered; integer sums do not care.
//   node_mat  (mode 0): item = pair, row x in its LEFT list, partners = its RIGHT list             (:185-188)
//   short_mat (mode 1): item = a DISTINCT end list of the block, row x in it, partners = its nodes y >= x, added as often
//                       as the block holds that list (7 % of the ends at configs[4] bring a list of their own)   (:174-184)
//   k_list_owners   every end against the block's list table: who stands for a list, who repeats one (gown, mult)
//   k_owners_mult   the multiplicities from the table to the owning ends; k_owners_collect: the owning ends, in end order
//   k_rows_count    histogram of the items' lists per chunk (LDS, 16-bit counts), added to row_count
//   (scan)          row_ptr = exclusive sums
//   k_rows_fill     the same histogram again; a chunk reserves its stretch of every row it holds with one global atomic,
//                   then places its items through LDS cursors.  An entry names the ROW OF THE LIST to add -- the owner of
//                   an equal list, so that a matrix row reads a few hundred cached rows, not one per pair -- and its length
//   k_rows_sum      strips of rows off a queue; a lane per (entry of the row, quad of the list it names)
#define ROWS_CHUNK 16384u  // pairs per chunk: a node is in a list at most once, so a 16-bit count (<= 32 768 ends) cannot wrap
#define ROWS_CHUNK1 8192u  // owning ends per chunk (mode 1: few items, spread over more workgroups)
#define ROWS_TPB 1024u
#define ROWS_CAP 4096u     // distinct rows of a chunk that get an LDS cursor (the rest: a global atomic per entry)
static inline size_t rows_lds_bytes(uint32_t n_keys) { return sizeof(uint32_t) * (((size_t)n_keys + 2u) / 2u + ROWS_CAP + ROWS_CAP / 2u + 4u); }

// Which read ends stand for a list of their own, and for how many ends: short_mat takes one weighted pass per DISTINCT
// list of the block, and node_mat's entries name distinct lists (cached rows) instead of one row per pair.  Every end
// looks its list up in a table of the whole block (device memory, one 64-bit word per slot: tag << 32 | owner end + 1,
// claimed by compare-and-swap; a separate word per slot counts the ends).  A lookup reads with plain loads -- a word never
// changes once claimed, a stale zero only sends the lane into a CAS that returns the real word.  Fingerprints are
// order-independent (the lists arrive in no particular order); a tag match is confirmed node by node against the owner's
// row, which is input data.  mult[end] = 0 for an end that is merged into another one; an end that claimed a slot gets the
// slot's count from k_owners_mult; an end that finds no place within LTAB_PROBES slots stands for itself alone.
// gown[end] = the end whose row holds this end's list.  (Merging the ends of a round in LDS first was measured: forward
// reads of one locus repeat each other nine times in ten, their mates rarely; with it the kernel took 5.6 ms at
// configs[4], without 4.1.)
#define LTAB_PROBES 16u
__device__ __forceinline__ void vs_load_list(const uint32_t *__restrict__ row, const uint32_t *__restrict__ hi, uint32_t n, uint32_t (&v)[LCAP]) {
    const VsQuad z{0, 0, 0, 0};
    const VsQuad a = *(const VsQuad *)row, b = n > 4u ? *(const VsQuad *)(row + 4) : z, c = n > 8u ? *(const VsQuad *)(row + 8) : z;
    const VsQuad d = n > 12u ? *(const VsQuad *)(row + 12) : z, f = n > 16u ? *(const VsQuad *)hi : z;
    const uint32_t w[LCAP] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, f.x, f.y, f.z, f.w};
#pragma unroll
    for (uint32_t i = 0; i < LCAP; i++) v[i] = i < n ? w[i] : 0xFFFFFFFFu;
}
// the same set of n nodes?  (both padded with 0xFFFFFFFF)
__device__ __forceinline__ bool vs_same_list(const uint32_t (&mine)[LCAP], const uint32_t (&other)[LCAP], uint32_t n) {
    bool same = true;
    if (n <= LC) {  // (nearly every list: the first LC positions of either side hold everything)
#pragma unroll
        for (uint32_t k2 = 0; k2 < LC; k2++) {
            bool found = false;
#pragma unroll
            for (uint32_t i = 0; i < LC; i++) found |= mine[i] == other[k2];
            same &= found || k2 >= n;
        }
        return same;
    }
#pragma unroll
    for (uint32_t k2 = 0; k2 < LCAP; k2++) {
        bool found = false;
#pragma unroll
        for (uint32_t i = 0; i < LCAP; i++) found |= mine[i] == other[k2];
        same &= found || k2 >= n;
    }
    return same;
}

__global__ void __launch_bounds__(256)
k_list_owners(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ lists_hi, const uint32_t *__restrict__ counts, uint64_t n_ends, uint32_t *__restrict__ mult,
              uint32_t *__restrict__ gown, unsigned long long *__restrict__ ltab, uint32_t *__restrict__ lmult, uint32_t ltab_bits) {
    const uint64_t e64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e64 >= n_ends) return;
    const uint32_t e = (uint32_t)e64, n = counts[e];
    uint32_t m = n ? 1u : 0u, own = e;
    if (n && ltab) {
        uint32_t mine[LCAP];
        vs_load_list(lists + e64 * LC, lists_hi + e64 * 4u, n, mine);
        unsigned long long f2 = n;
#pragma unroll
        for (uint32_t i = 0; i < LCAP; i++)
            if (i < n) {
                unsigned long long g = (mine[i] + 1ull) * 0x9E3779B97F4A7C15ull;
                g ^= g >> 29;
                f2 += g * 0xBF58476D1CE4E5B9ull;  // (a sum: the order of the nodes does not matter)
            }
        const uint32_t tag = ((uint32_t)(f2 >> 32) & ~31u) | (n - 1u);  // (the list length rides in the tag: no load for the owner's)
        const unsigned long long word = ((unsigned long long)tag << 32) | (e + 1u);
        // (r6: sub-tables per stretch of consecutive ends, so that a sub-table stays in the Infinity Cache, were measured and LOSE --
        // lists recur across the whole block and get an owner per sub-table; profiles/EXPERIMENTS.md)
        uint32_t h = (uint32_t)((f2 * 0xD6E8FEB86659FD93ull) >> (64u - ltab_bits));
        for (uint32_t pr = 0; pr < LTAB_PROBES; pr++) {
            unsigned long long cur = ltab[h];
            if (cur == 0ull) {
                cur = atomicCAS(&ltab[h], 0ull, word);
                if (cur == 0ull) {  // claimed: k_owners_mult hands this end the slot's count
                    atomicAdd(&lmult[h], 1u);
                    m = 0u;
                    break;
                }
            }
            if ((uint32_t)(cur >> 32) == tag) {
                uint32_t other[LCAP];
                vs_load_list(lists + (uint64_t)((uint32_t)cur - 1u) * LC, lists_hi + (uint64_t)((uint32_t)cur - 1u) * 4u, n, other);
                if (vs_same_list(mine, other, n)) {
                    atomicAdd(&lmult[h], 1u);
                    m = 0u;
                    own = (uint32_t)cur - 1u;
                    break;
                }
            }
            h = (h + 1u) & ((1u << ltab_bits) - 1u);
        }
        // (no place within LTAB_PROBES slots -- a crowded table: m = 1, the end stands for itself)
    }
    mult[e] = m;
    gown[e] = own;
}

// every claimed slot of the block's list table: its owner gets the slot's multiplicity
__global__ void __launch_bounds__(256)
k_owners_mult(const unsigned long long *__restrict__ ltab, const uint32_t *__restrict__ lmult, uint64_t n_slots, uint32_t *__restrict__ mult) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_slots) return;
    const unsigned long long w = ltab[h];
    if (w != 0ull) mult[(uint32_t)w - 1u] = lmult[h];
}

// The owning ends (mult > 0) in END order -- locus order, so that a chunk of them touches few matrix rows, as a chunk of
// pairs does.  A workgroup takes a stretch of ends, counts the owners, reserves their places with ONE atomic (the counter is
// a single word: an atomic per wavefront would queue up behind each other), then reads the stretch again and writes.
#define COLLECT_TPB 256u
__global__ void __launch_bounds__(COLLECT_TPB)
k_owners_collect(const uint32_t *__restrict__ mult, uint64_t n_ends, uint64_t per_wg, uint32_t *__restrict__ owners, uint32_t *__restrict__ n_owners) {
    __shared__ uint32_t s_wave[COLLECT_TPB / 64u], s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * per_wg, hi = lo + per_wg < n_ends ? lo + per_wg : n_ends;
    uint32_t mine = 0;
    for (uint64_t e = lo + tid; e < hi; e += COLLECT_TPB) mine += mult[e] != 0u ? 1u : 0u;
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) s_wave[wv] = mine;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (uint32_t i = 0; i < COLLECT_TPB / 64u; i++) tot += s_wave[i];
        s_base = tot ? atomicAdd(n_owners, tot) : 0u;
        s_wave[0] = 0u;  // (now the running offset inside the reservation)
    }
    __syncthreads();
    for (uint64_t e0 = lo; e0 < hi; e0 += COLLECT_TPB) {  // (uniform trip count: the ballot sees every lane)
        const uint64_t e = e0 + tid;
        const bool own = e < hi && mult[e] != 0u;
        const unsigned long long live = __ballot(own);
        uint32_t wbase = 0;
        if (lane == 0 && live) wbase = atomicAdd(&s_wave[0], (uint32_t)__popcll(live));  // (LDS)
        wbase = __shfl(wbase, 0, 64);
        if (own) owners[s_base + wbase + (uint32_t)__popcll(live & ((1ull << lane) - 1ull))] = (uint32_t)e;
    }
}

// The list of item i that is transposed, and its length (0: not an item).  Mode 0: pair i, its left list -- only if the
// right list holds anything; mode 1: the i-th owning read end.
template <int MODE>
__device__ __forceinline__ uint32_t vs_rows_item(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ owners, uint64_t i, uint64_t &row) {
    if (MODE == 0) {
        const uint2 c = *(const uint2 *)(counts + 2u * i);
        row = 2u * i;
        return c.y ? c.x : 0u;
    }
    row = owners[i];
    return counts[row];
}

// one lane per (item, quad of its list): the 16-bit bin of every listed node in [key_lo, key_lo + n_keys) + 1
template <int MODE>
__device__ __forceinline__ void vs_rows_histogram(uint32_t *h32, const uint32_t *__restrict__ lists, const uint32_t *__restrict__ lists_hi, const uint32_t *__restrict__ counts,
                                                  const uint32_t *__restrict__ owners, uint64_t lo, uint64_t hi, uint32_t key_lo, uint32_t n_keys) {
    for (uint64_t i = lo * 4u + threadIdx.x; i < hi * 4u; i += ROWS_TPB) {
        uint64_t row;
        const uint32_t q0 = (uint32_t)i & 3u, n = vs_rows_item<MODE>(counts, owners, i >> 2, row);
        for (uint32_t q = q0; 4u * q < n; q += 4u) {  // (a list of 17 .. LCAP nodes: its fifth quad is the first lane's too)
            const VsQuad v = *(const VsQuad *)vs_row_quad(lists, lists_hi, row, q);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t x = e[j] - key_lo;
                if (4u * q + j < n && x < n_keys) atomicAdd(&h32[x >> 1], 1u << ((x & 1u) * 16u));
            }
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(ROWS_TPB)
k_rows_count(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ lists_hi, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ owners, uint64_t n_items,
             const uint32_t *__restrict__ n_owners, uint32_t key_lo, uint32_t n_keys, uint32_t *__restrict__ row_count) {
    uint32_t *h32 = vs_lds;
    const uint32_t words = (n_keys + 1u) >> 1, tid = threadIdx.x;
    if (MODE) n_items = *n_owners;  // (mode 1: the launch covers every end, the items are the owners among them)
    const uint64_t per = MODE ? ROWS_CHUNK1 : ROWS_CHUNK;
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < n_items ? lo + per : n_items;
    if (lo >= n_items) return;
    for (uint32_t i = tid; i < words; i += ROWS_TPB) h32[i] = 0u;
    __syncthreads();
    vs_rows_histogram<MODE>(h32, lists, lists_hi, counts, owners, lo, hi, key_lo, n_keys);
    __syncthreads();
    for (uint32_t i = tid; i < words; i += ROWS_TPB) {
        const uint32_t v = h32[i];
        if (v & 0xFFFFu) atomicAdd(&row_count[key_lo + 2u * i], v & 0xFFFFu);
        if (v >> 16) atomicAdd(&row_count[key_lo + 2u * i + 1u], v >> 16);
    }
}

template <int MODE>
__global__ void __launch_bounds__(ROWS_TPB)
k_rows_fill(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ lists_hi, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ owners, uint64_t n_items,
            const uint32_t *__restrict__ n_owners, const uint32_t *__restrict__ gown, uint32_t key_lo, uint32_t n_keys,
            const uint32_t *__restrict__ row_ptr, uint32_t *__restrict__ row_cursor, uint32_t *__restrict__ entries) {
    uint32_t *h32 = vs_lds;
    const uint32_t words = (n_keys + 1u) >> 1, tid = threadIdx.x;
    if (MODE) n_items = *n_owners;
    if ((uint64_t)blockIdx.x * (MODE ? ROWS_CHUNK1 : ROWS_CHUNK) >= n_items) return;
    uint32_t *s_base = h32 + words;          // [ROWS_CAP] where this chunk's stretch of the row starts
    uint32_t *s_fill = s_base + ROWS_CAP;    // [ROWS_CAP / 2] 16-bit cursors inside the stretch
    uint32_t &s_nc = s_fill[ROWS_CAP / 2u];
    for (uint32_t i = tid; i < words; i += ROWS_TPB) h32[i] = 0u;
    for (uint32_t i = tid; i < ROWS_CAP / 2u; i += ROWS_TPB) s_fill[i] = 0u;
    if (tid == 0) s_nc = 0u;
    __syncthreads();
    const uint64_t per = MODE ? ROWS_CHUNK1 : ROWS_CHUNK;
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < n_items ? lo + per : n_items;
    vs_rows_histogram<MODE>(h32, lists, lists_hi, counts, owners, lo, hi, key_lo, n_keys);
    __syncthreads();
    // a bin that is not empty: reserve the chunk's stretch of that row, and turn the bin into the number of its cursor
    for (uint32_t i = tid; i < words; i += ROWS_TPB) {
        const uint32_t v = h32[i];
        if (!v) continue;
        uint32_t out = v;
#pragma unroll
        for (uint32_t half = 0; half < 2u; half++) {
            const uint32_t c = (v >> (16u * half)) & 0xFFFFu;
            if (!c) continue;
            const uint32_t x = key_lo + 2u * i + half;
            const uint32_t ci = atomicAdd(&s_nc, 1u);
            uint32_t code = 0xFFFFu;
            if (ci < ROWS_CAP) {
                s_base[ci] = row_ptr[x] + atomicAdd(&row_cursor[x], c);
                code = ci;
            }
            out = (out & ~(0xFFFFu << (16u * half))) | (code << (16u * half));
        }
        h32[i] = out;
    }
    __syncthreads();
    for (uint64_t i = lo * 4u + tid; i < hi * 4u; i += ROWS_TPB) {
        uint64_t row;
        const uint32_t q0 = (uint32_t)i & 3u, n = vs_rows_item<MODE>(counts, owners, i >> 2, row);
        if (4u * q0 >= n) continue;
        // what an entry says: whose list row k_rows_sum reads, and that list's length - 1 in the top five bits -- the block's
        // owner of the pair's RIGHT list (a few hundred distinct rows per matrix row, cached, instead of one row per pair) /
        // the owning end itself
        uint32_t payload;
        if (MODE) payload = (uint32_t)row | ((n - 1u) << 27);
        else {
            const uint64_t re = 2u * (i >> 2) + 1u;
            payload = gown[re] | ((counts[re] - 1u) << 27);
        }
        for (uint32_t q = q0; 4u * q < n; q += 4u) {
            const VsQuad v = *(const VsQuad *)vs_row_quad(lists, lists_hi, row, q);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t x = e[j] - key_lo;
                if (4u * q + j >= n || x >= n_keys) continue;
                const uint32_t code = (h32[x >> 1] >> ((x & 1u) * 16u)) & 0xFFFFu;
                uint32_t pos;
                if (code != 0xFFFFu) {
                    const uint32_t sh = (code & 1u) * 16u;
                    const uint32_t old = atomicAdd(&s_fill[code >> 1], 1u << sh);
                    pos = s_base[code] + ((old >> sh) & 0xFFFFu);
                } else {
                    pos = row_ptr[e[j]] + atomicAdd(&row_cursor[e[j]], 1u);
                }
                entries[pos] = payload;
            }
        }
    }
}

// The strips' cell table is smaller than the pair-major kernel's (8 k slots, 64 KB) and the strips narrower for it: two
// workgroups share a CU, and one waits in its LDS queue while the other computes (configs[4]: 14.1 -> 11.2 ms)
#define RS_TPB 1024
typedef CellTable<RS_BITS> RsTable;
#define RSUM_LDS_BYTES ((2u * RS_SLOTS + 64u + 8u) * 4u)
#define RSUM_MAX_ROWS 64u
template <int MODE>
__global__ void __launch_bounds__(RS_TPB)
k_rows_sum(const uint32_t *__restrict__ lists, const uint32_t *__restrict__ lists_hi, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ mult, uint32_t N,
           const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ entries, uint32_t R, uint32_t n_strips, uint32_t fill_limit,
           uint32_t *__restrict__ mat, uint32_t off, uint8_t *__restrict__ tile_map, uint32_t T, uint32_t *__restrict__ queue) {
    uint32_t *s_key = vs_lds, *s_cnt = vs_lds + RS_SLOTS, *s_rowend = vs_lds + 2u * RS_SLOTS;  // [RSUM_MAX_ROWS]
    uint32_t &s_used = s_rowend[64], &s_lost = s_rowend[65], &s_strip = s_rowend[66];
    const uint32_t tid = threadIdx.x, q = tid & 3u;
    constexpr uint32_t STEP = RS_TPB / 4u;  // entries per pass of the workgroup
    for (uint32_t i = tid; i < RS_SLOTS; i += RS_TPB) { s_key[i] = RsTable::EMPTY; s_cnt[i] = 0u; }
    if (tid == 0) { s_used = 0u; s_lost = 0u; }
    for (;;) {
        __syncthreads();
        if (tid == 0) s_strip = atomicAdd(queue, 1u);
        __syncthreads();
        const uint32_t strip = s_strip;
        if (strip >= n_strips) break;
        const uint32_t first = strip * R, nrows = first + R <= N ? R : N - first;
        if (tid < nrows) s_rowend[tid] = row_ptr[first + tid + 1u];
        const uint32_t e0 = row_ptr[first], e1 = row_ptr[first + nrows];
        // keys are cell indices relative to the strip's first row, shifted so that key >> 4 is one 64-byte stretch of the matrix
        const uint32_t align = (uint32_t)(((uint64_t)first * N + off) & 15u);
        const uint64_t cell0 = (uint64_t)first * N;
        __syncthreads();
        auto write_out = [&]() {
            for (uint32_t i = tid; i < RS_SLOTS; i += RS_TPB) {
                const uint32_t key = s_key[i];
                if (key != RsTable::EMPTY) {
                    const uint32_t k2 = key - align;
                    atomicAdd(mat + cell0 + k2, s_cnt[i]);
                    if (tile_map) {
                        const uint32_t xl = k2 / N;
                        vs_mark_tile(tile_map, T, (uint32_t)MODE, first + xl, k2 - xl * N);
                    }
                    s_key[i] = RsTable::EMPTY;
                    s_cnt[i] = 0u;
                }
            }
            __syncthreads();
            if (tid == 0) { s_used = 0u; s_lost = 0u; }
            __syncthreads();
        };
        // the item of entry i is loaded two passes ahead, its partner list one pass ahead (two dependent loads off the
        // critical path)
        auto load_item = [&](uint32_t base) -> uint32_t {
            const uint32_t i = base + (tid >> 2);
            return i < e1 ? entries[i] : 0xFFFFFFFFu;
        };
        auto load_list = [&](uint32_t it, uint32_t &n, uint32_t &wgt, VsQuad &yq) {
            n = 0u;
            wgt = 1u;
            yq = VsQuad{0u, 0u, 0u, 0u};
            if (it != 0xFFFFFFFFu) {
                const uint64_t row = it & 0x07FFFFFFu;  // (a read end of the transposition)
                n = (it >> 27) + 1u;
                if (MODE) wgt = mult[row];
                yq = *(const VsQuad *)(lists + row * LC + 4u * q);
            }
        };
        uint32_t p1 = e0 < e1 ? load_item(e0) : 0xFFFFFFFFu;
        uint32_t p2 = e1 - e0 > STEP ? load_item(e0 + STEP) : 0xFFFFFFFFu;
        uint32_t n1, w1;
        VsQuad y1;
        load_list(p1, n1, w1, y1);
        uint32_t pass = 0;
        for (uint32_t base = e0; base < e1; base += STEP, pass++) {
            const uint32_t n = n1, wgt = w1, p0 = p1;
            const VsQuad yq = y1;
            p1 = p2;
            load_list(p1, n1, w1, y1);
            p2 = e1 - base > 2u * STEP ? load_item(base + 2u * STEP) : 0xFFFFFFFFu;
            if (4u * q < n) {
                const uint32_t i = base + (tid >> 2);
                uint32_t xl = 0;  // rows of the strip that end at or before entry i
#pragma unroll
                for (uint32_t step = RSUM_MAX_ROWS / 2u; step; step >>= 1) {
                    const uint32_t t = xl + step;
                    if (t < nrows && s_rowend[t - 1u] <= i) xl = t;
                }
                const uint32_t kbase = xl * N + align, x = first + xl;
                auto add_quad = [&](const VsQuad &yv, uint32_t q4) {
                    const uint32_t ys[4] = {yv.x, yv.y, yv.z, yv.w};
                    uint32_t key[4], seen[4], at[4];
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) {
                        key[j] = kbase + ys[j];
                        at[j] = RsTable::slot(key[j]);
                        seen[j] = s_key[at[j]];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) {
                        if (q4 + j >= n || (MODE && ys[j] < x)) continue;  // (short_mat: the cell (x, y) belongs to the smaller node's row)
                        if (seen[j] == key[j]) {
                            atomicAdd(&s_cnt[at[j]], wgt);
                        } else if (!vs_cell_claim<RsTable>(s_key, s_cnt, &s_used, key[j], at[j], wgt)) {
                            atomicAdd(&s_lost, 1u);
                            vs_mark_tile(tile_map, T, (uint32_t)MODE, x, ys[j]);
                            atomicAdd(mat + cell0 + (key[j] - align), wgt);
                        }
                    }
                };
                add_quad(yq, 4u * q);
                // (a list of 17 .. LCAP nodes: its fifth quad is the first lane's too -- one entry in forty at configs[4])
                if (n > 16u && q == 0u) add_quad(*(const VsQuad *)(lists_hi + (uint64_t)(p0 & 0x07FFFFFFu) * 4u), 16u);
            }
            if ((pass & 3u) == 3u) {  // (a strip that outruns the limit between two looks finds the table crowded and adds the rest to memory itself: slower, the same sums)
                __syncthreads();
                const bool spill = s_used > fill_limit || s_lost > 4096u;
                __syncthreads();
                if (spill) write_out();
            }
        }
        __syncthreads();
        write_out();
    }
}

// ---- locus order -----------------------------------------------------------------------------------
// Pairs are handed to k_pe_tiles sorted by the first node their forward read's seeds hit, so that
// a tile holds pairs from one locus: they touch the same few node_mat / short_mat cells (summed in
// LDS before any global atomic) and the same node text (L1/L2 hits).  Any order gives the same
// counters (integer addition commutes); this one only changes how many global atomics it takes.
// key: node index, N = no seed of the forward read hits, N+1 = pair dropped by the N / length
// filters (still counted in the stats by k_pe_tiles).
// The locus node of the seed `key`, or ~0u when no slot holds it.  A slot's node stands beside the table (slot_node, written
// by the index build from the finished postings), so the slot and its node are requested together -- the slot index is
// known before the slot arrives -- and no posting is loaded; the one probe in ten that moves on requests again.
#define VS_LOCUS_MISS 0xFFFFFFFFu
__device__ __forceinline__ uint32_t vs_locus_probe(const VsIndexDev &idx, uint64_t key) {
    const uint32_t mask = (1u << idx.table_bits) - 1u;
    uint32_t sl = vs_slot_of(key, idx.table_bits);
    const uint4 *tab = (const uint4 *)idx.table;
    for (;;) {
        const uint4 raw = tab[sl];
        const uint32_t node = idx.slot_node[sl];
        const uint64_t k = (uint64_t)raw.x | ((uint64_t)raw.y << 32);
        if (k == VS_EMPTY_KEY) return VS_LOCUS_MISS;
        if ((k & ~VS_MULTI_BIT) == key) return node;
        sl = (sl + 1u) & mask;
    }
}

__device__ __forceinline__ uint32_t vs_locus_key(const VsIndexDev &idx, const VsReadsDev &rd, uint64_t p) {
    const uint32_t mf = rd.meta[2 * p], mr = rd.meta[2 * p + 1];
    const uint32_t N = idx.n_nodes, w = idx.w, s = idx.s, K = idx.K;
    // (no second end, VS_FLAG_ABSENT: the filters of the first alone -- VS_FILTER_LEN_MASK)
    if ((((mf | mr) >> 24) & VS_FLAG_N) || (mf & VS_LEN_MASK) < K || (mr & VS_FILTER_LEN_MASK) < K) return N + 1u;
    const uint32_t rlen = mf & VS_LEN_MASK;
    const uint64_t base = (uint64_t)rd.woff[2 * p] * 16u;
    const bool inv = (mf >> 24) & VS_FLAG_INVALID;
    for (uint32_t j = vs_seed_phase(rlen, w, s); j + w <= rlen; j += s) {
        if (inv && vs_seed_dirty(rd.mask, base + j, w)) continue;
        uint32_t sr;
        const uint64_t key = vs_seed_key(rd.words, base + j, w, &sr);
        const uint32_t node = vs_locus_probe(idx, key);
        if (node != VS_LOCUS_MISS) return node;
    }
    return N;
}

// The first node a seed of read end e hits (N = none): the locus of that end.
__device__ __forceinline__ uint32_t vs_locus_key_end(const VsIndexDev &idx, const VsReadsDev &rd, uint64_t e) {
    const uint32_t m = rd.meta[e];
    const uint32_t N = idx.n_nodes, w = idx.w, s = idx.s, rlen = m & VS_LEN_MASK;
    const uint64_t base = (uint64_t)rd.woff[e] * 16u;
    const bool inv = (m >> 24) & VS_FLAG_INVALID;
    for (uint32_t j = vs_seed_phase(rlen, w, s); j + w <= rlen; j += s) {
        if (inv && vs_seed_dirty(rd.mask, base + j, w)) continue;
        uint32_t sr;
        const uint64_t key = vs_seed_key(rd.words, base + j, w, &sr);
        const uint32_t node = vs_locus_probe(idx, key);
        if (node != VS_LOCUS_MISS) return node;
    }
    return N;
}

// Counting sort without global atomics (used while the N+2 keys fit an LDS histogram):
//   k_locus_count   : workgroup g takes pairs [g*chunk, (g+1)*chunk): keys -> keys[], LDS histogram
//                     -> column g of cnt[key][g]  (key-major so that the scan below is contiguous)
//   vs_scan_u32     : exclusive scan of cnt[] in (key, workgroup) order = first slot of every
//                     (key, workgroup) run in the sorted order -- stable, deterministic
//   k_locus_scatter : workgroup g loads its column as LDS cursors and places its pairs
#define LOCUS_TPB 1024     // threads per workgroup of the two LDS-histogram sort kernels
#define LOCUS_SCATTER_U 8u  // pairs a thread of k_locus_scatter has in flight
// (key_lo, nk): the keys this pass counts / places -- a graph with more keys than one LDS histogram holds (54 k nodes at
// configs[4]) takes two or three passes over the stored keys instead of the global-atomic sort; `compute`: the first
// pass derives the keys (the expensive part: a read's seeds are probed) and stores them, the others read them back.
__global__ void __launch_bounds__(LOCUS_TPB)
k_locus_count(VsIndexDev idx, VsReadsDev rd, uint64_t n_pairs, uint32_t chunk, uint32_t n_wg, uint32_t *__restrict__ keys,
              uint32_t *__restrict__ cnt, uint32_t key_lo, uint32_t nk, uint32_t compute) {
    for (uint32_t i = threadIdx.x; i < nk; i += LOCUS_TPB) vs_lds[i] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * chunk;
    const uint64_t hi = lo + chunk < n_pairs ? lo + chunk : n_pairs;
    for (uint64_t p = lo + threadIdx.x; p < hi; p += LOCUS_TPB) {
        uint32_t key;
        if (compute) {
            key = vs_locus_key(idx, rd, p);
            keys[p] = key;
        } else {
            key = keys[p];
        }
        if (key - key_lo < nk) atomicAdd(&vs_lds[key - key_lo], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nk; i += LOCUS_TPB) cnt[(uint64_t)(key_lo + i) * n_wg + blockIdx.x] = vs_lds[i];
}

// The computing pass of a one-pass sort with the read words STREAMED THROUGH LDS (the plan says when: vs_pe_plan,
// locus_stage_words).  k_locus_count above pays three dependent round trips per pair -- header, read words, slot -- with
// 64 lanes on 64 lines in the last two.  A workgroup's chunk is one contiguous stretch of `words` (woff is a prefix array),
// and so is the sixteenth of it that each WAVEFRONT takes here and walks in batches (vs_locus_batch: the longest run of
// pairs whose words fit a buffer, one pair per lane at most).  A wavefront has two LDS buffers of its own: while batch i is
// keyed out of one and its slots are probed, the words of batch i + 1 are on their way into the other with coalesced 16-byte
// loads, and the headers of batch i + 2 behind them.  What is left per pair is one dependent global load, the slot with its
// node beside it (vs_locus_probe).  The keys are vs_locus_key's, bit for bit: the same words, the same seeds in the same
// order.  A pair whose own words exceed a buffer is a batch of its own, keyed by vs_locus_key; an end flagged
// VS_FLAG_INVALID reads its mask from memory as there.
// No workgroup barrier between the zeroing of the histogram and its write-out: the wavefronts run apart, as those of
// k_locus_count do (batches of the whole workgroup behind a barrier were measured first: every batch then waits for the
// longest probe chain among 818 pairs, and the pass took what it took before -- profiles/EXPERIMENTS.md).  Every loop is
// bounded by the chunk, nothing waits for another workgroup.
// (The loads of a batch are issued by every lane, with or without work, at clamped indices: straight-line code, so that
// the wait for a slot is not also a wait for the stream requested behind it.)
struct LocusHdr {
    uint32_t mf, mr, ws, we, w0;  // lengths | flags of the lane's pair, its first word and the word behind its last, the first word of the batch
    bool live;                    // the lane's pair exists
};
typedef uint32_t LocusQuad __attribute__((ext_vector_type(4)));  // (a plain vector: as uint4 structs the quads were copied through private memory)
struct LocusQuads {
    LocusQuad q0, q1, q2, q3, q4;
};
struct LocusProbe {  // one pair's walk over its seeds and their slots
    uint32_t res, j, sl, node, rlen, lbase;  // lbase: the pair's first base, counted from the first of the wavefront's two buffers
    uint64_t key, gbase;
    uint4 raw;
    bool have, active, inv;
};
__global__ void __launch_bounds__(LOCUS_TPB)
k_locus_count_staged(VsIndexDev idx, VsReadsDev rd, uint64_t n_pairs, uint32_t chunk, uint32_t n_wg, uint32_t *__restrict__ keys,
                     uint32_t *__restrict__ cnt, uint32_t nk, uint32_t cap) {
    static_assert(LOCUS_STAGE_PAIRS == 64u && LOCUS_TPB / 64u == LOCUS_STAGE_WAVES, "a batch holds one pair per lane of a wavefront");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t hist_words = (nk + 3u) & ~3u, buf_words = vs_locus_buf_words(cap);
    uint32_t *s_hist = vs_lds;
    uint32_t *s_buf = vs_lds + hist_words + wv * 2u * buf_words;  // [2][buf_words] of this wavefront
    for (uint32_t i = tid; i < nk; i += LOCUS_TPB) s_hist[i] = 0;
    __syncthreads();
    // the wavefront's part [lo, hi) of the workgroup's chunk (empty where the chunk is: 4 097 pairs leave workgroups 241 .. 255 nothing)
    const uint64_t c_lo = (uint64_t)blockIdx.x * chunk, c_hi = c_lo + chunk < n_pairs ? c_lo + chunk : n_pairs;
    const uint32_t sub = (chunk + LOCUS_STAGE_WAVES - 1u) / LOCUS_STAGE_WAVES;
    const uint64_t hi = c_lo + (uint64_t)(wv + 1u) * sub < c_hi ? c_lo + (uint64_t)(wv + 1u) * sub : c_hi;
    const uint64_t lo = c_lo + (uint64_t)wv * sub < hi ? c_lo + (uint64_t)wv * sub : hi;
    const bool any = lo < hi;
    const uint32_t N = idx.n_nodes, w = idx.w, s = idx.s, K = idx.K, tmask = (1u << idx.table_bits) - 1u;
    const uint4 *tab = (const uint4 *)idx.table;

    // the headers of the batch that starts at pair P: lane t has those of pair P + t (indices clamped to the part's last pair)
    auto load_hdr = [&](uint64_t P) -> LocusHdr {
        LocusHdr h = {0u, 0u, 0u, 0u, 0u, false};
        if (!any) return h;  // (uniform over the wavefront)
        const uint64_t Pc = P < hi ? P : hi - 1u, q = P + lane < hi ? P + lane : hi - 1u;
        const uint2 m = *(const uint2 *)(rd.meta + 2u * q);
        h.mf = m.x;
        h.mr = m.y;
        h.ws = rd.woff[2u * q];
        h.we = rd.woff[2u * q + 2u];
        h.w0 = rd.woff[2u * Pc];
        h.live = P + lane < hi;
        return h;
    };
    // the batch cut (vs_locus_in_batch, counted): pairs in the batch (0: the first does not fit, or none is left), the word
    // behind the last of them
    auto cut = [&](const LocusHdr &h, uint32_t &w_end) -> uint32_t {
        const uint64_t m = __ballot(vs_locus_in_batch(h.live, h.w0, h.we, cap));
        const uint32_t n = (uint32_t)__popcll(m);  // (the lanes in the batch are a prefix: lane n - 1 is the last)
        w_end = n ? (uint32_t)__shfl((int)h.we, (int)(n - 1u)) : 0u;
        return n;
    };
    // the words of a staged batch on their way: whole quads from the aligned word at or below w_first (vs_locus_span)
    // (quad k of a lane in a variable of its own, r.q<k>, not in an array: the array went to private memory)
#define LOCUS_EACH_QUAD(X) X(0) X(1) X(2) X(3) X(4)
    static_assert(LOCUS_STAGE_QUADS == 5u, "LOCUS_EACH_QUAD names the quads");
    auto stage_load = [&](bool on, uint32_t w_first, uint32_t w_end, LocusQuads &r) {
        LocusSpan sp = vs_locus_span(on ? w_first : 0u, on ? w_end : 0u);  // (off: the block's first quads, loaded and dropped)
        if (sp.quads > buf_words / 4u) sp.quads = buf_words / 4u;          // (never: the cut keeps w_end - w_first <= cap)
        const LocusQuad *src = (const LocusQuad *)(rd.words + sp.first);
#define LOCUS_LOAD(k) r.q##k = src[lane + k * 64u < sp.quads ? lane + k * 64u : sp.quads - 1u];
        LOCUS_EACH_QUAD(LOCUS_LOAD)
#undef LOCUS_LOAD
    };
    auto stage_store = [&](bool on, uint32_t w_first, uint32_t w_end, const LocusQuads &r, uint32_t *buf) {
        LocusSpan sp = vs_locus_span(w_first, w_end);
        if (sp.quads > buf_words / 4u) sp.quads = buf_words / 4u;
#define LOCUS_STORE(k) if (on && lane + k * 64u < sp.quads) ((LocusQuad *)buf)[lane + k * 64u] = r.q##k;
        LOCUS_EACH_QUAD(LOCUS_STORE)
#undef LOCUS_STORE
#undef LOCUS_EACH_QUAD
        vs_wave_sync();  // (written by some lanes, read by others of this wavefront)
    };
    // the next clean seed of a pair at or behind its j: key and slot; false: the read has none left
    auto seek = [&](LocusProbe &q) -> bool {
        for (; q.j + w <= q.rlen; q.j += s) {
            if (q.inv && vs_seed_dirty(rd.mask, q.gbase + q.j, w)) continue;
            uint32_t sr;
            q.key = vs_seed_key((const uint32_t *)s_buf, q.lbase + q.j, w, &sr);
            q.sl = vs_slot_of(q.key, idx.table_bits);
            return true;
        }
        return false;
    };
    // one slot looked at, as vs_locus_probe does; a seed in no node moves on to the read's next seed
    auto look = [&](LocusProbe &q) {
        if (!q.active) return;
        const uint64_t k = (uint64_t)q.raw.x | ((uint64_t)q.raw.y << 32);
        if (k != VS_EMPTY_KEY && (k & ~VS_MULTI_BIT) == q.key) {
            q.res = q.node;
            q.active = false;
            return;
        }
        if (k == VS_EMPTY_KEY) {
            q.j += s;
            q.active = seek(q);
        } else {
            q.sl = (q.sl + 1u) & tmask;
        }
        if (q.active) {
            q.raw = tab[q.sl];
            q.node = idx.slot_node[q.sl];
        }
    };
    auto finish = [&](const LocusProbe &q, uint64_t p_first) {
        if (q.have) {
            keys[p_first + lane] = q.res;
            if (q.res < nk) atomicAdd(&s_hist[q.res], 1u);
        }
    };

    // cur: the batch whose pairs are started (buffer it & 1); nxt: the one whose words are requested while that happens;
    // old: the batch before cur, whose pairs that are still looking go on beside cur's first looks -- their buffer is the
    // one nxt's words go to, so they are through before those are stored.  A batch's longest chain of slots (a read error
    // in each of the first seeds, slots passed over) is thus walked beside the next batch's shortest.
    LocusQuads r;
    uint64_t pc = lo, po = lo;
    LocusHdr hc = load_hdr(pc);
    uint32_t wec, wen;
    uint32_t nc = cut(hc, wec);
    bool stc = nc != 0u;
    if (!nc && pc < hi) nc = 1u;  // (an oversize pair, alone)
    stage_load(stc, hc.w0, wec, r);
    stage_store(stc, hc.w0, wec, r, s_buf);
    uint64_t pn = pc + nc;
    LocusHdr hn = load_hdr(pn);
    uint32_t nn = cut(hn, wen);
    bool stn = nn != 0u;
    if (!nn && pn < hi) nn = 1u;
    LocusProbe qo = {};  // (nothing: have = active = false)
    for (uint32_t it = 0; pc < hi; it++) {
        // 1. the lane's pair of the current batch: filters, its first clean seed, the slot of that seed requested
        LocusProbe qc = {};
        qc.have = lane < nc;
        qc.res = N + 1u;
        qc.rlen = hc.mf & VS_LEN_MASK;
        qc.inv = (hc.mf >> 24) & VS_FLAG_INVALID;
        qc.lbase = ((it & 1u) * buf_words + hc.ws - (hc.w0 & ~3u)) * 16u;  // the pair's first base in the two buffers (vs_locus_span)
        qc.gbase = (uint64_t)hc.ws * 16u;
        if (qc.have && !stc) {
            qc.res = vs_locus_key(idx, rd, pc);  // (lane 0 alone)
        } else if (qc.have && !((((hc.mf | hc.mr) >> 24) & VS_FLAG_N) || qc.rlen < K || (hc.mr & VS_FILTER_LEN_MASK) < K)) {
            qc.res = N;
            qc.j = vs_seed_phase(qc.rlen, w, s);
            qc.active = seek(qc);
        }
        if (!qc.active) qc.sl = 0;
        qc.raw = tab[qc.sl];
        qc.node = idx.slot_node[qc.sl];
        // 2. the next batch's words, 3. the headers of the one behind it
        stage_load(stn, hn.w0, wen, r);
        const uint64_t p2 = pn + nn;
        const LocusHdr h2 = load_hdr(p2);
        // 4. the slots: the old batch to its end, the current one beside it (the first looks outside the loop: they wait
        // for the slots alone, the stream stays in flight)
        look(qo);
        look(qc);
        while (qo.active) {
            look(qo);
            look(qc);
        }
        finish(qo, po);
        // 5. the next batch's words into the old batch's buffer, the cut behind it
        stage_store(stn, hn.w0, wen, r, s_buf + ((it + 1u) & 1u) * buf_words);
        uint32_t we2;
        uint32_t n2 = cut(h2, we2);
        const bool st2 = n2 != 0u;
        if (!n2 && p2 < hi) n2 = 1u;
        qo.res = qc.res; qo.j = qc.j; qo.sl = qc.sl; qo.node = qc.node; qo.rlen = qc.rlen; qo.lbase = qc.lbase; qo.key = qc.key;
        qo.gbase = qc.gbase; qo.raw = qc.raw; qo.have = qc.have; qo.active = qc.active; qo.inv = qc.inv;
        po = pc;
        pc = pn; hc = hn; nc = nn; stc = stn; wec = wen;
        pn = p2; hn = h2; nn = n2; stn = st2; wen = we2;
    }
    while (qo.active) look(qo);
    finish(qo, po);
    __syncthreads();
    for (uint32_t i = tid; i < nk; i += LOCUS_TPB) cnt[(uint64_t)i * n_wg + blockIdx.x] = s_hist[i];
}

__global__ void __launch_bounds__(LOCUS_TPB)
k_locus_scatter(uint32_t key_lo, uint32_t nk, uint64_t n_pairs, uint32_t chunk, uint32_t n_wg, const uint32_t *__restrict__ keys,
                const uint32_t *__restrict__ first, uint32_t *__restrict__ perm) {
    // Which workgroup places which chunk is free.  Workgroups go to the 8 XCDs round-robin (blockIdx % 8), and the places of
    // one key in neighbouring chunks are neighbours in perm[]: XCD x takes the x-th eighth of the chunks, so that the runs
    // that share a line of perm[] meet in one L2 and leave it as one line.  (Measured at 10 M pairs: 0.013 ms of the sort with
    // the scatter in four launches, 0.01 ms at most in one -- profiles/EXPERIMENTS.md, 2026-10-21.)
    uint32_t wg = blockIdx.x;
    if ((n_wg & 7u) == 0u) wg = (blockIdx.x & 7u) * (n_wg >> 3) + (blockIdx.x >> 3);
    for (uint32_t i = threadIdx.x; i < nk; i += LOCUS_TPB) vs_lds[i] = first[(uint64_t)(key_lo + i) * n_wg + wg];
    __syncthreads();
    const uint64_t lo = (uint64_t)wg * chunk;
    const uint64_t hi = lo + chunk < n_pairs ? lo + chunk : n_pairs;
    if (lo >= hi || !nk) return;  // (uniform; 4 097 pairs leave workgroups 241 .. 255 nothing)
    // A thread's pairs are a chain each -- key load, returning LDS atomic, scattered store -- so it takes LOCUS_SCATTER_U of
    // them a turn: pairs lo + tid + LOCUS_TPB * (U * i + j), j < U, coalesced 4-byte loads.  The keys of turn i + 1 are
    // requested before the atomics of turn i, and the atomics of a turn are all issued before its first store.  Loads and
    // atomics are straight-line code, so that the compiler counts them and waits for no more than it needs: a pair beyond the
    // chunk loads the chunk's last key, and a lane with nothing to place adds 0 to a cursor of its own choice (which changes
    // nothing).  Only the stores are conditional.  (k[], kn[], at[] and on[] are indexed by unrolled constants only: registers.)
    const uint32_t span = (uint32_t)(hi - lo), turns = (span + LOCUS_SCATTER_U * LOCUS_TPB - 1u) / (LOCUS_SCATTER_U * LOCUS_TPB);
    const uint32_t idle = (threadIdx.x & 63u) < nk ? threadIdx.x & 63u : 0u;  // (a cursor per lane: no two lanes of a wavefront on one)
    uint32_t k[LOCUS_SCATTER_U], kn[LOCUS_SCATTER_U], at[LOCUS_SCATTER_U];
    bool on[LOCUS_SCATTER_U];
    auto request = [&](uint32_t q0, uint32_t *dst) {  // q: a pair counted from lo
#pragma unroll
        for (uint32_t j = 0; j < LOCUS_SCATTER_U; j++) {
            const uint32_t q = q0 + j * LOCUS_TPB;
            dst[j] = keys[lo + (q < span ? q : span - 1u)];
        }
    };
    uint32_t q0 = threadIdx.x;  // (q0 + U * LOCUS_TPB cannot wrap: span <= chunk < 2^32 / 256, a workgroup's share of at most 2^32 pairs)
    request(q0, kn);
    for (uint32_t t = 0; t < turns; t++, q0 += LOCUS_SCATTER_U * LOCUS_TPB) {
#pragma unroll
        for (uint32_t j = 0; j < LOCUS_SCATTER_U; j++) k[j] = kn[j];
        request(q0 + LOCUS_SCATTER_U * LOCUS_TPB, kn);
#pragma unroll
        for (uint32_t j = 0; j < LOCUS_SCATTER_U; j++) {
            on[j] = q0 + j * LOCUS_TPB < span && k[j] - key_lo < nk;
            at[j] = atomicAdd(&vs_lds[on[j] ? k[j] - key_lo : idle], on[j] ? 1u : 0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < LOCUS_SCATTER_U; j++)
            if (on[j]) perm[at[j]] = (uint32_t)(lo + q0 + j * LOCUS_TPB);
    }
}

// Fallback for graphs with more nodes than the LDS histogram holds: global atomics.
__global__ void __launch_bounds__(TPB)
k_pe_locus(VsIndexDev idx, VsReadsDev rd, uint64_t n_pairs, uint32_t *__restrict__ keys, uint32_t *__restrict__ hist) {
    const uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t key = vs_locus_key(idx, rd, p);
    keys[p] = key;
    atomicAdd(&hist[key], 1u);
}

__global__ void __launch_bounds__(TPB)
k_pe_permute(uint64_t n_pairs, const uint32_t *__restrict__ keys, uint32_t *__restrict__ cursor, uint32_t *__restrict__ perm) {
    const uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= n_pairs) return;
    perm[atomicAdd(&cursor[keys[p]], 1u)] = (uint32_t)p;
}

// ---- overflow path, first stop: one WAVEFRONT per listed pair ------------------------------------------------------------
// Pairs the tile kernels hand over -- an end with more accepted nodes than a list row holds (3 % of the pairs at configs[4]),
// a full tile table, an end with more bytes outside ACGT than inv4 holds -- are mapped here the general way (every probe,
// every posting, vs_extend with the validity mask), but with the per-end (node -> count, min offset, min window) state in an
// LDS hash table of the wavefront instead of the dense per-workgroup node state of k_pe_slow, four pairs per workgroup at a
// time and no workgroup barrier: 8 192 pairs in flight on the chip.  Its own limits (MID_SLOTS touched nodes, MID_LIST
// accepted nodes per end, 64 probes per end) send what is left to k_pe_slow, which has none.
#define MID_SLOTS 256u
#define MID_LIST 64u
#define MID_WORDS (4u * MID_SLOTS + 3u * 64u + 65u + 2u * MID_LIST + 4u)
__global__ void __launch_bounds__(TPB)
k_pe_mid(PeParams P, const uint32_t *__restrict__ in_list, const uint32_t *__restrict__ in_count, uint32_t in_cap,
         uint32_t *__restrict__ out_list, uint32_t *__restrict__ out_count) {
    __shared__ uint32_t s_all[(TPB / 64u) * MID_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *s_key = s_all + wv * MID_WORDS, *s_cnt = s_key + MID_SLOTS, *s_minp = s_cnt + MID_SLOTS, *s_minj = s_minp + MID_SLOTS;
    uint32_t *s_pa = s_minj + MID_SLOTS, *s_pb = s_pa + 64u, *s_pc = s_pb + 64u, *s_pref = s_pc + 64u;  // s_pref[65]
    uint32_t *s_lst = s_pref + 65u;  // [2][MID_LIST] accepted nodes of the two ends
    uint32_t *s_flag = s_lst + 2u * MID_LIST;  // [0] overflow, [1..2] list lengths
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K, wv_seed = VS_SEED_VERIFIED(P.idx.w);
    uint32_t n_in = *in_count;
    if (n_in > in_cap) n_in = in_cap;
    const uint32_t n_waves = gridDim.x * (TPB / 64u);
    for (uint32_t li = blockIdx.x * (TPB / 64u) + wv; li < n_in; li += n_waves) {
        const uint32_t pair = in_list[li];
        if (lane < 4u) s_flag[lane] = 0u;
        vs_wave_sync();
        for (uint32_t side = 0; side < 2u; side++) {
            const uint64_t e = 2ull * pair + side;
            const uint32_t meta = P.rd.meta[e];
            const uint32_t rlen = meta & VS_LEN_MASK;
            const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
            const uint32_t *mk = ((meta >> 24) & VS_FLAG_INVALID) ? P.rd.mask : nullptr;
            const uint32_t nprobe = vs_seed_probes(rlen, w, s), phase = vs_seed_phase(rlen, w, s);
            for (uint32_t i = lane; i < MID_SLOTS; i += 64u) { s_key[i] = EMPTY_NODE; s_cnt[i] = 0u; s_minp[i] = 0xFFFFFFFFu; s_minj[i] = 0xFFFFFFFFu; }
            if (nprobe > 64u) { if (lane == 0u) s_flag[0] = 1u; }
            // probes: one per lane
            uint32_t c = 0u, pa = 0u, pb = 0u;
            if (lane < nprobe && nprobe <= 64u) {
                const uint32_t j = phase + lane * s;
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
            }
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t2 = __shfl_up(incl, d, 64);
                if (lane >= (uint32_t)d) incl += t2;
            }
            s_pa[lane] = pa; s_pb[lane] = pb; s_pc[lane] = c;
            s_pref[lane + 1u] = incl;
            if (lane == 0u) s_pref[0] = 0u;
            vs_wave_sync();
            const uint32_t total = s_pref[64];
            for (uint32_t t = lane; t < total; t += 64u) {
                const uint32_t pr = vs_upper_idx(s_pref, 65u, t);
                const uint32_t k2 = t - s_pref[pr], j = phase + pr * s;
                uint32_t node, pos, opp;
                VsNodeMeta nm;
                if (s_pc[pr] == 1u) {
                    node = s_pa[pr]; pos = s_pb[pr] & 0x7FFFFFFFu; opp = s_pb[pr] >> 31;
                    nm = P.idx.meta[node];
                } else {
                    const VsPosting po = vs_posting_unpack(P.idx.postings[s_pa[pr] + k2]);
                    node = po.node; pos = po.pos; opp = po.strand ^ (s_pb[pr] >> 31);
                    nm.woff = po.woff; nm.len = po.len;
                }
                const uint32_t q = opp ? nm.len - pos - w : pos;
                uint32_t a, qa, len;
                if (P.mid_fast && !mk) {
                    // (r5) an end without bytes outside ACGT in a block of the straight-line shape (stride <= 32, reads <= w + 160):
                    // the comparison of k_pe_tiles<1> -- one left window, five right ones, no data-dependent loop -- off the read's
                    // words in global memory (the 64 lanes of the wavefront share them)
                    uint32_t cl = s < j ? s : j;
                    cl = cl < q ? cl : q;
                    uint32_t rem = rlen - j - wv_seed;
                    const uint32_t dr = nm.len - q - wv_seed;
                    rem = rem < dr ? rem : dr;
                    const uint32_t tb = (nm.woff + (opp ? P.idx.rc_delta : 0u)) * 16u;
                    uint32_t left, ext;
                    vs_agree_fast<false>(P.rd.words + (rbase >> 4), 0u, P.idx.fwd_words, tb + q, cl, tb + q + wv_seed, rem, j, wv_seed, &left, &ext);
                    len = left + wv_seed + ext;
                    if (left >= s || len < K) continue;
                    a = j - left;
                    qa = q - left;
                } else {
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    if (!vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, wv_seed, s, K, mk, rbase, &a, &qa, &len)) continue;
                }
                uint32_t at = (node * 0x9E3779B1u) >> 24;  // MID_SLOTS = 256
                bool placed = false;
                for (uint32_t tr = 0; tr < MID_SLOTS; tr++) {
                    const uint32_t old = atomicCAS(&s_key[at], EMPTY_NODE, node);
                    if (old == EMPTY_NODE || old == node) {
                        atomicAdd(&s_cnt[at], len - K + 1u);
                        atomicMin(&s_minp[at], opp ? nm.len - qa - len : qa);
                        // (mid_fast: reads of at most 191 bases and nodes below 2^23 bases -- the node's length rides above the
                        // read offset, equal for every update of the slot, and the acceptance sweep needs no header load)
                        atomicMin(&s_minj[at], P.mid_fast ? (nm.len << 8) | a : a);
                        placed = true;
                        break;
                    }
                    at = (at + 1u) & (MID_SLOTS - 1u);
                }
                if (!placed) s_flag[0] = 1u;
            }
            vs_wave_sync();
            // acceptance test per occupied slot; accepted nodes to the end's list (ballot + prefix count)
            uint32_t base = 0u;
            for (uint32_t i0 = 0; i0 < MID_SLOTS; i0 += 64u) {
                const uint32_t i = i0 + lane;
                const uint32_t node = s_key[i];
                bool acc = false;
                if (node != EMPTY_NODE)
                    acc = P.mid_fast ? vs_accept32(s_cnt[i], s_minp[i], s_minj[i] & 0xFFu, s_minj[i] >> 8, rlen, K)
                                     : vs_accept(s_cnt[i], s_minp[i], s_minj[i], P.idx.meta[node].len, rlen, K);
                const unsigned long long mask = __ballot(acc);
                const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (acc) {
                    if (at < MID_LIST) s_lst[side * MID_LIST + at] = node; else s_flag[0] = 1u;
                }
                base += (uint32_t)__popcll(mask);
            }
            if (lane == 0u) s_flag[1u + side] = base;
            vs_wave_sync();
        }
        if (s_flag[0]) {  // beyond this kernel's tables: the general kernel
            if (lane == 0u) out_list[atomicAdd(out_count, 1u)] = pair;
            vs_wave_sync();
            continue;
        }
        const uint32_t nl = s_flag[1], nr = s_flag[2];
        const uint32_t *L = s_lst, *R = s_lst + MID_LIST;
        if (P.accumulate) {  // PE_Inference.py:174-188
            // Both lists ascending first (one entry per lane, bitonic network over the wavefront): neighbouring lanes
            // below then add to neighbouring cells of one matrix row, and the atomics of a wave instruction leave the L2
            // as one memory-side request per 64-byte stretch they touch (r3: 7.5 -> 5.8 ms with the path numbering).
            for (uint32_t side = 0; side < 2u; side++) {
                uint32_t *sv = s_lst + side * MID_LIST;
                const uint32_t n = side ? nr : nl;
                uint32_t v = lane < n ? sv[lane] : 0xFFFFFFFFu;
#pragma unroll
                for (uint32_t k2 = 2u; k2 <= 64u; k2 <<= 1)
#pragma unroll
                    for (uint32_t j2 = k2 >> 1; j2 > 0u; j2 >>= 1) {
                        const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)j2, 64);
                        const bool keep_min = ((lane & j2) == 0u) == ((lane & k2) == 0u);
                        v = keep_min ? (v < o ? v : o) : (v > o ? v : o);
                    }
                if (lane < n) sv[lane] = v;
            }
            vs_wave_sync();
            for (uint32_t i = lane; i < nl * nr; i += 64u) {
                vs_mark_tile_store(P.tile_map, P.tile_T, 0u, L[i / nr], R[i % nr]);
                atomicAdd(&P.node_mat[(uint64_t)L[i / nr] * N + R[i % nr]], 1u);
            }
            for (uint32_t side = 0; side < 2u; side++) {
                const uint32_t *sv = side ? R : L;
                const uint32_t n = side ? nr : nl;
                for (uint32_t i = lane; i < n * n; i += 64u) {
                    const uint32_t a = i / n, b = i % n, x = sv[a], y = sv[b];
                    if (x < y || a == b) {
                        vs_mark_tile_store(P.tile_map, P.tile_T, 1u, x, y);
                        atomicAdd(&P.short_mat[(uint64_t)x * N + y], 1u);
                    }
                }
            }
        }
        if (P.dbg_counts) {
            for (uint32_t side = 0; side < 2u; side++) {
                const uint32_t *sv = side ? R : L;
                const uint32_t n = side ? nr : nl;
                const uint64_t e = 2ull * pair + side;
                if (lane == 0u) P.dbg_counts[e] = n;
                for (uint32_t i = lane; i < n && i < P.dbg_cap; i += 64u) P.dbg_lists[e * P.dbg_cap + i] = sv[i];
            }
        }
        vs_wave_sync();
    }
}

// ---- overflow path: any number of nodes per end, any read ------------------------------------------
// One workgroup per listed pair (ends with more accepted nodes than an LDS row holds, ends with many
// bytes outside ACGT, seeds with a huge posting list).  Node state is dense in HBM per workgroup --
// the reference's own layout (PE_Inference.py:19-21) -- but only the nodes an end touches are ever
// looked at: the first credit of a node appends it to a list, and the acceptance sweep walks that
// list and restores the state.  Probes go through the workgroup 256 at a time; their postings are
// spread over the threads (prefix sum of the counts in LDS, one posting per thread and round).
// dense layout per workgroup: cnt[N] minp[N] minj[N] touched[N] surv0[N] surv1[N].
__global__ void __launch_bounds__(TPB)
k_pe_slow(PeParams P, uint32_t *dense, uint32_t n_slow_cap, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count) {
    __shared__ uint32_t s_n[2], s_nt, s_cnt[TPB + 1], s_pa[TPB], s_pb[TPB];
    const uint32_t tid = threadIdx.x;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t n_slow = *count;
    if (n_slow > n_slow_cap) n_slow = n_slow_cap;
    uint32_t *cnt = dense + (uint64_t)blockIdx.x * SLOW_WORDS_PER_NODE * N;
    uint32_t *minp = cnt + N, *minj = minp + N, *touched = minj + N, *surv0 = touched + N, *surv1 = surv0 + N;
    for (uint32_t li = blockIdx.x; li < n_slow; li += gridDim.x) {
        const uint32_t pair = list[li];
        if (tid < 2) s_n[tid] = 0;
        for (uint32_t side = 0; side < 2; side++) {
            const uint64_t e = 2ull * pair + side;
            const uint32_t meta = P.rd.meta[e];
            const uint32_t rlen = meta & VS_LEN_MASK;
            const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
            const uint32_t *mk = ((meta >> 24) & VS_FLAG_INVALID) ? P.rd.mask : nullptr;
            uint32_t *surv = side ? surv1 : surv0;
            const uint32_t nprobe = vs_seed_probes(rlen, w, s), phase = vs_seed_phase(rlen, w, s);
            if (tid == 0) s_nt = 0;
            __syncthreads();
            for (uint32_t p0 = 0; p0 < nprobe; p0 += TPB) {
                // probes p0 .. p0 + 255: one per thread
                uint32_t c = 0, pa = 0, pb = 0;
                const uint32_t pi = p0 + tid;
                if (pi < nprobe) {
                    const uint32_t j = phase + pi * s;
                    if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                        uint32_t sr;
                        const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                        c = vs_probe(P.idx, key, sr, &pa, &pb);
                    }
                }
                s_pa[tid] = pa;
                s_pb[tid] = pb;
                // inclusive scan of the posting counts over the workgroup -> s_cnt[1 .. 256], s_cnt[0] = 0
                uint32_t incl = c;
                const uint32_t lane = tid & 63u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t t2 = __shfl_up(incl, d, 64);
                    if (lane >= (uint32_t)d) incl += t2;
                }
                s_cnt[tid + 1u] = incl;
                if (tid == 0) s_cnt[0] = 0;
                __syncthreads();
                uint32_t off = 0;
                for (uint32_t wv = 0; wv < (tid >> 6); wv++) off += s_cnt[wv * 64u + 64u];
                __syncthreads();
                s_cnt[tid + 1u] = incl + off;
                __syncthreads();
                const uint32_t total = s_cnt[TPB];
                for (uint32_t t = tid; t < total; t += TPB) {
                    // the probe that owns posting t: last index with s_cnt[idx] <= t
                    const uint32_t pr = vs_upper_idx(s_cnt, TPB + 1u, t);
                    const uint32_t k2 = t - s_cnt[pr], j = phase + (p0 + pr) * s;
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr];
                    uint32_t node, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        node = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[node];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        node = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    if (!vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len))
                        continue;
                    if (atomicAdd(&cnt[node], len - K + 1u) == 0u) touched[atomicAdd(&s_nt, 1u)] = node;
                    atomicMin(&minp[node], opp ? nm.len - qa - len : qa);
                    atomicMin(&minj[node], a);
                }
                __syncthreads();  // s_cnt / s_pa / s_pb are rewritten by the next batch of probes
            }
            // (all of it is this workgroup's own traffic, the loads below bypass L1: a workgroup barrier
            // orders it; a device-wide fence would write back the whole L2 of the XCD each time)
            __syncthreads();
            const uint32_t nt = s_nt;
            for (uint32_t i = tid; i < nt; i += TPB) {
                const uint32_t nd = __hip_atomic_load(&touched[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t v = __hip_atomic_load(&cnt[nd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t c = __hip_atomic_load(&minp[nd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t ki = __hip_atomic_load(&minj[nd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (vs_accept(v, c, ki, P.idx.meta[nd].len, rlen, K)) surv[atomicAdd(&s_n[side], 1u)] = nd;
                __hip_atomic_store(&cnt[nd], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&minp[nd], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&minj[nd], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
        }
        const uint32_t nl = s_n[0], nr = s_n[1];
        if (P.accumulate) {
            for (uint64_t i = tid; i < (uint64_t)nl * nr; i += TPB) {
                uint32_t a = (uint32_t)(i / nr), b = (uint32_t)(i - (uint64_t)a * nr);
                const uint32_t x = __hip_atomic_load(&surv0[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t y = __hip_atomic_load(&surv1[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                vs_mark_tile(P.tile_map, P.tile_T, 0u, x, y);
                atomicAdd(&P.node_mat[(uint64_t)x * N + y], 1u);
            }
            for (uint32_t side = 0; side < 2; side++) {
                const uint32_t *sv = side ? surv1 : surv0;
                const uint32_t n = side ? nr : nl;
                for (uint64_t i = tid; i < (uint64_t)n * n; i += TPB) {
                    uint32_t a = (uint32_t)(i / n), b = (uint32_t)(i - (uint64_t)a * n);
                    uint32_t x = __hip_atomic_load(&sv[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    uint32_t y = __hip_atomic_load(&sv[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (x < y || a == b) {
                        vs_mark_tile(P.tile_map, P.tile_T, 1u, x, y);
                        atomicAdd(&P.short_mat[(uint64_t)x * N + y], 1u);
                    }
                }
            }
        }
        if (P.dbg_counts) {
            for (uint32_t side = 0; side < 2; side++) {
                const uint32_t *sv = side ? surv1 : surv0;
                const uint32_t n = side ? nr : nl;
                const uint64_t e = 2ull * pair + side;
                if (tid == 0) P.dbg_counts[e] = n;
                for (uint32_t i = tid; i < n && i < P.dbg_cap; i += TPB)
                    P.dbg_lists[e * P.dbg_cap + i] = __hip_atomic_load(&sv[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TPB) k_dense_zero_cnt(uint32_t *dense, uint64_t N, uint64_t groups) {
    uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < N * groups) dense[(i / N) * (uint64_t)SLOW_WORDS_PER_NODE * N + (i % N)] = 0u;
}

// ---- host side ---------------------------------------------------------------------------------
// Every decision of a call -- tile shape, instantiation, locus order, counter path, grids, scratch sizes -- is taken by
// vs_pe_plan (vs_pe_plan.h); what follows reserves, fills PeParams and launches from the plan.

// The row-owner path: both counters of one block from the per-end lists (see "both matrices by ROW OWNERS").
static int pe_count_by_rows(vs_ctx *ctx, const PePlan &pl, uint32_t N, uint32_t *d_node_mat, uint32_t *d_short_mat, uint8_t *d_tile_map, uint32_t T) {
    hipStream_t st = ctx->stream;
    const uint64_t slots_pairs = pl.list_ends / 2, sub_pairs = pl.rows_sub_pairs;  // pairs per transposition
    // per mode: counts, cursors, offsets; then the block sums of the scan (2 048 values per block, 64 bits each)
    const uint64_t cap = (uint64_t)N + 2u;
    VS_HIP(ctx, ctx->d_rows.reserve(sizeof(uint32_t) * 6u * cap + sizeof(uint64_t) * ((uint64_t)N / 2048u + 8u)));
    // the list table of a transposition (0 bits: no table, every end stands for itself)
    const uint32_t ltab_bits = pl.rows_ltab_bits;
    const bool use_ltab = ltab_bits > 0;
    const uint64_t ltab_slots = use_ltab ? 1ull << ltab_bits : 0;
    // entries: one word per listed node -- the left lists (node_mat) and the lists of the owning ends (short_mat); the
    // multiplicity of every end, the owning ends, the table (a 64-bit word and a 32-bit sum per slot)
    VS_HIP(ctx, ctx->d_row_entries.reserve(sizeof(uint32_t) * (3u * sub_pairs * LCAP + 16u)));
    VS_HIP(ctx, ctx->d_mult.reserve(sizeof(uint32_t) * (6u * sub_pairs + 4u)));  // mult[2 np], owners[2 np], gown[2 np]
    VS_HIP(ctx, ctx->d_ltab.reserve((sizeof(uint64_t) + sizeof(uint32_t)) * ltab_slots + 16u));
    uint32_t *rows = ctx->d_rows.as<uint32_t>();
    uint64_t *scan_tmp = (uint64_t *)(rows + ((6u * cap + 1u) & ~1ull));
    const uint32_t n_keys = pl.rows_keys, fill = pl.rows_fill, R = pl.rows_per_strip;
    const size_t rl = rows_lds_bytes(n_keys);
    for (const void *fn : {(const void *)k_rows_count<0>, (const void *)k_rows_count<1>, (const void *)k_rows_fill<0>, (const void *)k_rows_fill<1>})
        VS_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rl));
    for (const void *fn : {(const void *)k_rows_sum<0>, (const void *)k_rows_sum<1>})
        VS_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RSUM_LDS_BYTES));
    uint32_t *queue = ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_STRIP_QUEUE, *n_owners = ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_OWNERS;
    unsigned long long *ltab = use_ltab ? ctx->d_ltab.as<unsigned long long>() : nullptr;
    uint32_t *lmult = use_ltab ? (uint32_t *)(ctx->d_ltab.as<unsigned long long>() + ltab_slots) : nullptr;
    for (uint64_t p0 = 0; p0 < slots_pairs; p0 += sub_pairs) {
        const uint64_t np = slots_pairs - p0 < sub_pairs ? slots_pairs - p0 : sub_pairs;
        const uint32_t *sl = ctx->d_lists.as<const uint32_t>() + 2u * p0 * LC, *sh = ctx->d_lists.as<const uint32_t>() + 2u * slots_pairs * LC + 2u * p0 * 4u;
        const uint32_t *sc = ctx->d_list_counts.as<const uint32_t>() + 2u * p0;
        uint32_t *mult = ctx->d_mult.as<uint32_t>(), *owners = mult + 2u * sub_pairs, *gown = owners + 2u * sub_pairs;
        const unsigned n_chunks = (unsigned)((np + ROWS_CHUNK - 1u) / ROWS_CHUNK);
        const unsigned n_chunks1 = (unsigned)((2u * np + ROWS_CHUNK1 - 1u) / ROWS_CHUNK1);  // (every end could be an owner; a chunk past the last owner returns at once)
        VS_HIP(ctx, hipMemsetAsync(rows, 0, sizeof(uint32_t) * 6u * cap, st));
        VS_HIP(ctx, hipMemsetAsync(n_owners, 0, sizeof(uint32_t), st));
        if (use_ltab) VS_HIP(ctx, hipMemsetAsync(ctx->d_ltab.ptr(), 0, (sizeof(uint64_t) + sizeof(uint32_t)) * ltab_slots, st));
        hipLaunchKernelGGL(k_list_owners, dim3((unsigned)((2u * np + 255u) / 256u)), dim3(256), 0, st, sl, sh, sc, 2u * np, mult, gown, ltab, lmult, ltab_bits);
        if (use_ltab)
            hipLaunchKernelGGL(k_owners_mult, dim3((unsigned)((ltab_slots + 255u) / 256u)), dim3(256), 0, st, (const unsigned long long *)ltab,
                               (const uint32_t *)lmult, ltab_slots, mult);
        {
            const uint64_t per_wg = ((2u * np + ctx->n_cu * 8ull - 1u) / (ctx->n_cu * 8ull) + COLLECT_TPB - 1u) / COLLECT_TPB * COLLECT_TPB;
            hipLaunchKernelGGL(k_owners_collect, dim3((unsigned)((2u * np + per_wg - 1u) / per_wg)), dim3(COLLECT_TPB), 0, st, (const uint32_t *)mult, 2u * np, per_wg,
                               owners, n_owners);
        }
        for (int mode = 0; mode < 2; mode++) {
            uint32_t *row_count = rows + 3u * mode * cap, *row_cursor = row_count + cap, *row_ptr = row_cursor + cap;
            uint32_t *entries = ctx->d_row_entries.as<uint32_t>() + (mode ? np * LCAP : 0u);
            for (uint32_t key_lo = 0; key_lo < N; key_lo += n_keys) {
                const uint32_t nk = N - key_lo < n_keys ? N - key_lo : n_keys;
                if (mode) hipLaunchKernelGGL(k_rows_count<1>, dim3(n_chunks1), dim3(ROWS_TPB), rl, st, sl, sh, sc, (const uint32_t *)owners, 0ull, (const uint32_t *)n_owners, key_lo, nk, row_count);
                else hipLaunchKernelGGL(k_rows_count<0>, dim3(n_chunks), dim3(ROWS_TPB), rl, st, sl, sh, sc, (const uint32_t *)nullptr, np, (const uint32_t *)nullptr, key_lo, nk, row_count);
            }
            int rc = vs_scan_u32(ctx, row_count, row_ptr, (uint64_t)N + 1u, scan_tmp, nullptr);
            if (rc) return rc;
            for (uint32_t key_lo = 0; key_lo < N; key_lo += n_keys) {
                const uint32_t nk = N - key_lo < n_keys ? N - key_lo : n_keys;
                if (mode) hipLaunchKernelGGL(k_rows_fill<1>, dim3(n_chunks1), dim3(ROWS_TPB), rl, st, sl, sh, sc, (const uint32_t *)owners, 0ull, (const uint32_t *)n_owners, (const uint32_t *)gown, key_lo, nk, (const uint32_t *)row_ptr, row_cursor, entries);
                else hipLaunchKernelGGL(k_rows_fill<0>, dim3(n_chunks), dim3(ROWS_TPB), rl, st, sl, sh, sc, (const uint32_t *)nullptr, np, (const uint32_t *)nullptr, (const uint32_t *)gown, key_lo, nk, (const uint32_t *)row_ptr, row_cursor, entries);
            }
        }
        for (int mode = 0; mode < 2; mode++) {
            const uint32_t *row_ptr = rows + 3u * mode * cap + 2u * cap;
            const uint32_t *entries = ctx->d_row_entries.as<const uint32_t>() + (mode ? np * LCAP : 0u);
            const uint32_t n_strips = (N + R - 1u) / R;
            uint32_t grid = (uint32_t)ctx->n_cu * 2u;  // (two workgroups per CU: 64 KB of LDS each)
            if (grid > n_strips) grid = n_strips;
            uint32_t *m = mode ? d_short_mat : d_node_mat;
            const uint32_t off = (uint32_t)(((uintptr_t)m >> 2) & 15u);
            VS_HIP(ctx, hipMemsetAsync(queue, 0, sizeof(uint32_t), st));
            if (mode)
                hipLaunchKernelGGL(k_rows_sum<1>, dim3(grid), dim3(RS_TPB), RSUM_LDS_BYTES, st, sl, sh, sc, (const uint32_t *)mult, N, row_ptr, entries, R, n_strips, fill, m,
                                   off, d_tile_map, T, queue);
            else
                hipLaunchKernelGGL(k_rows_sum<0>, dim3(grid), dim3(RS_TPB), RSUM_LDS_BYTES, st, sl, sh, sc, (const uint32_t *)mult, N, row_ptr, entries, R, n_strips, fill, m,
                                   off, d_tile_map, T, queue);
        }
    }
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// Everything a count launches between the mapping kernel and the overflow kernels: both matrices of N nodes from the
// hand-off in d_lists / d_list_counts (the layout the plan names, used_ends end slots written), by whichever counter
// path the plan picked.  vs_pe_count runs this behind k_pe_tiles, vs_pe_count_lists behind lists the host wrote.
static int pe_count_from_lists(vs_ctx *ctx, const PePlan &pl, uint32_t N, uint64_t used_ends, uint32_t *d_node_mat, uint32_t *d_short_mat,
                               uint8_t *d_tile_map) {
    hipStream_t st = ctx->stream;
    const uint32_t T = (N + 63u) >> 6;
    // the last tile may be partly empty: its unused rows must read as length 0
    if (pl.list_ends > used_ends)
        VS_HIP(ctx, hipMemsetAsync(ctx->d_list_counts.as<uint32_t>() + used_ends, 0, sizeof(uint32_t) * (pl.list_ends - used_ends), st));
    const uint64_t slots_pairs = pl.list_ends / 2;
    VS_HIP(ctx, hipEventRecord(ctx->ev[4], st));
    if (pl.use_rows) {
        const int rc = pe_count_by_rows(ctx, pl, N, d_node_mat, d_short_mat, d_tile_map, T);  // (zeroes its own queue words)
        if (rc) return rc;
        ctx->last_launched |= VS_RAN_ROW_OWNERS;
    } else {
        // (the chunks of pairs are not bound to workgroups: they are taken off a counter, see vs_pe_plan; the counter is a
        // word of d_slow_count, which either caller zeroes whole before its count)
        uint32_t *acc_queue = ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_ACC_QUEUE;
        if (pl.mark_tiles)  // (timed with the counter kernel: it is part of the counting)
            hipLaunchKernelGGL(k_mark_tiles, dim3((unsigned)((slots_pairs + 255u) / 256u)), dim3(256), 0, st, ctx->d_lists.as<const uint32_t>(),
                               ctx->d_list_counts.as<const uint32_t>(), slots_pairs, d_tile_map, T, pl.ept);
        VS_HIP(ctx, hipFuncSetAttribute((const void *)k_pe_accumulate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ACC_LDS_BYTES));
        hipLaunchKernelGGL(k_pe_accumulate, dim3(pl.acc_grid), dim3(ACC_TPB), ACC_LDS_BYTES, st, ctx->d_lists.as<const uint32_t>(),
                           ctx->d_list_counts.as<const uint32_t>(), slots_pairs, pl.acc_per_wg, N, pl.use_table, pl.acc_fill, pl.acc_task_cap, d_node_mat,
                           d_short_mat, acc_queue, pl.ept);
    }
    return VS_OK;
}

// The instantiations of k_pe_tiles by (MODE, SW, SP, AD), each with the name vs_pe_last_kernel returns for it; every
// compile-time shape (VS_STD_SHAPES) exists with and without the adaptive step grid.
struct TilesFn {
    uint32_t mode, sw, sp, ad;
    const void *fn;
    const char *name;
};
#define TILES(M, SW, SP) {M, SW, SP, 0u, (const void *)k_pe_tiles<M, SW, SP>, "k_pe_tiles<" #M ", " #SW ", " #SP ">"}
#define TILES_AD(M, SW, SP) {M, SW, SP, 1u, (const void *)k_pe_tiles<M, SW, SP, true>, "k_pe_tiles<" #M ", " #SW ", " #SP ", true>"}, TILES(M, SW, SP)
static const TilesFn TILES_TABLE[] = {TILES_AD(1, 10u, 4u), TILES_AD(1, 8u, 3u), TILES_AD(1, 7u, 2u), TILES_AD(1, 7u, 3u), TILES(1, 0u, 0u),
                                      TILES_AD(2, 16u, 2u), TILES(2, 0u, 0u),    TILES(0, 0u, 0u)};

static int pe_launch(vs_ctx *ctx, const vs_reads *reads, uint32_t *d_node_mat, uint32_t *d_short_mat, uint64_t *d_stats,
                     uint32_t *d_dbg_lists, uint32_t *d_dbg_counts, uint32_t dbg_cap, uint8_t *d_tile_map = nullptr) {
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_pe_count: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const VsIndexDev &idx = ctx->idx;
    const uint64_t n_pairs = reads->n_ends / 2;
    ctx->last_ms[0] = ctx->last_ms[1] = ctx->last_ms[2] = 0;
    ctx->last_launched = 0;
    ctx->last_order_pairs = 0;
    ctx->last_handoff = {};
    ctx->last_overflow = {};
    // test hooks: fixed defaults unless the process runs with VS_EXPERIMENT=1 (see VsTuning)
    if (ctx->experiment) vs_tuning_load(ctx->tune, true);
    PePlanIn in;
    in.n_nodes = idx.n_nodes; in.K = idx.K; in.w = idx.w; in.s = idx.s;
    in.n_seed_pos = ctx->n_seed_pos; in.n_distinct = ctx->n_distinct; in.max_node_len = ctx->max_node_len; in.n_cu = (uint32_t)ctx->n_cu;
    in.n_ends = reads->n_ends; in.max_len = (uint32_t)reads->max_len;
    in.has_mask = reads->d_mask != nullptr; in.has_inv4 = reads->d_inv4 != nullptr;
    in.count = d_node_mat != nullptr; in.tile_map = d_tile_map != nullptr;
    in.tune = ctx->tune;
    const PePlan pl = vs_pe_plan(in);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "%s", pl.msg);
    if (!pl.n_tiles) return VS_OK;  // an empty block
    const TilesFn *tf = nullptr;
    for (const TilesFn &t : TILES_TABLE)
        if (t.mode == pl.mode && t.sw == pl.sw && t.sp == pl.sp && t.ad == pl.ad) tf = &t;
    if (!tf) return vs_fail(ctx, VS_E_STATE, "vs_pe_count: the plan names k_pe_tiles<%u, %uu, %uu, %u>, which this build does not hold", pl.mode, pl.sw, pl.sp, pl.ad);

    // scratch: slow lists (one slot per pair), counters, dense state
    VS_HIP(ctx, ctx->d_slow_list.reserve(sizeof(uint32_t) * n_pairs));
    VS_HIP(ctx, ctx->d_slow_count.reserve(sizeof(uint32_t) * vs_ctx::SC_WORDS));
    VS_HIP(ctx, ctx->d_slow_list2.reserve(sizeof(uint32_t) * n_pairs));
    if (ctx->dense_nodes != idx.n_nodes) ctx->d_dense.reset();  // (the layout is by node count)
    bool dense_new = false;
    VS_HIP(ctx, ctx->d_dense.reserve(pl.dense_bytes, pl.dense_bytes, &dense_new));
    if (dense_new) {
        ctx->dense_nodes = idx.n_nodes;
        // cnt = 0, minp/minj = ~0 once; k_pe_slow restores this state after every end it sweeps
        uint64_t N = idx.n_nodes ? idx.n_nodes : 1;
        VS_HIP(ctx, hipMemsetAsync(ctx->d_dense.ptr(), 0xFF, pl.dense_bytes, st));
        hipLaunchKernelGGL(k_dense_zero_cnt, dim3((unsigned)((N * pl.slow_grid + TPB - 1) / TPB)), dim3(TPB), 0, st,
                           ctx->d_dense.as<uint32_t>(), N, (uint64_t)pl.slow_grid);
    }
    VS_HIP(ctx, hipMemsetAsync(ctx->d_slow_count.ptr(), 0, sizeof(uint32_t) * vs_ctx::SC_WORDS, st));
    // locus order of the pairs (see k_pe_locus)
    if (pl.use_sort) {
        VS_HIP(ctx, ctx->d_locus_keys.reserve(sizeof(uint32_t) * n_pairs));
        VS_HIP(ctx, ctx->d_perm.reserve(sizeof(uint32_t) * n_pairs));
        VS_HIP(ctx, ctx->d_locus_hist.reserve(sizeof(uint32_t) * pl.locus_hist_words));
        VS_HIP(ctx, ctx->d_scan_tmp.reserve(sizeof(uint64_t) * (pl.locus_hist_words / 2048 + 4)));
    }
    // per-end lists handed from k_pe_tiles to the counter kernels
    if (d_node_mat) {
        VS_HIP(ctx, ctx->d_lists.reserve(sizeof(uint32_t) * pl.list_words));
        VS_HIP(ctx, ctx->d_list_counts.reserve(sizeof(uint32_t) * (pl.list_ends + 2)));
    }

    PeParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.out_lists = ctx->d_lists.as<uint32_t>();
    P.out_counts = ctx->d_list_counts.as<uint32_t>();
    P.node_mat = d_node_mat;
    P.short_mat = d_short_mat;
    P.stats = (unsigned long long *)d_stats;
    P.ept = pl.ept;
    P.pmax = pl.pmax;
    P.words_cap = pl.words_cap;
    P.pool = pl.pool;
    P.pool_bits = pl.pool_bits;
    P.n_pairs = n_pairs;
    P.n_tiles = pl.n_tiles;
    P.tiles_per_wg = pl.tiles_per_wg;
    P.wpe = pl.wpe;
    P.magic_pmax = pl.magic_pmax;
    P.magic_wpe = pl.magic_wpe;
    P.perm = pl.use_sort ? ctx->d_perm.as<const uint32_t>() : nullptr;
    P.slow_list = ctx->d_slow_list.as<uint32_t>();
    P.slow_count = ctx->d_slow_count.as<uint32_t>();
    P.dbg_lists = d_dbg_lists;
    P.dbg_counts = d_dbg_counts;
    P.dbg_cap = dbg_cap;
    P.accumulate = d_node_mat ? 1u : 0u;
    P.out_rows = pl.use_rows;
    P.out_lists_hi = ctx->d_lists.as<uint32_t>() + pl.list_ends * LC;
    P.tile_map = d_node_mat ? d_tile_map : nullptr;
    P.tile_T = (idx.n_nodes + 63u) >> 6;
    P.shortcut = pl.shortcut;
    P.mid_fast = pl.mid_fast;

    const size_t lds = pl.lds_bytes;
    if (lds > 64u * 1024u)
        VS_HIP(ctx, hipFuncSetAttribute(tf->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    VS_HIP(ctx, hipEventRecord(ctx->ev[3], st));
    ctx->last_order_pairs = n_pairs;
    if (pl.use_sort) {
        const uint64_t nk = pl.locus_keys;
        ctx->last_launched |= pl.lds_sort ? VS_RAN_LOCUS_LDS_SORT : VS_RAN_LOCUS_GLOBAL_SORT;
        if (pl.lds_sort) {
            const uint32_t n_wg = LOCUS_WGS, chunk = pl.locus_chunk, per_pass = pl.locus_per_pass;
            const size_t lds_keys = sizeof(uint32_t) * per_pass;
            if (lds_keys > 64u * 1024u) {
                VS_HIP(ctx, hipFuncSetAttribute((const void *)k_locus_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_keys));
                VS_HIP(ctx, hipFuncSetAttribute((const void *)k_locus_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_keys));
            }
            // (the staged key pass copies `words` in 16-byte quads: every block allocates them so; one that did not keeps the per-pair loads)
            if (pl.locus_stage_words && ((uintptr_t)reads->d_words & 15u) == 0u) {
                VS_HIP(ctx, hipFuncSetAttribute((const void *)k_locus_count_staged, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.locus_lds_bytes));
                hipLaunchKernelGGL(k_locus_count_staged, dim3(n_wg), dim3(LOCUS_TPB), pl.locus_lds_bytes, st, idx, reads->dev(), n_pairs, chunk, n_wg,
                                   ctx->d_locus_keys.as<uint32_t>(), ctx->d_locus_hist.as<uint32_t>(), (uint32_t)nk, pl.locus_stage_words);
                ctx->last_launched |= VS_RAN_LOCUS_STAGED;
            } else {
                for (uint32_t key_lo = 0; key_lo < nk; key_lo += per_pass) {
                    const uint32_t n_here = (uint32_t)(nk - key_lo < per_pass ? nk - key_lo : per_pass);
                    hipLaunchKernelGGL(k_locus_count, dim3(n_wg), dim3(LOCUS_TPB), lds_keys, st, idx, reads->dev(), n_pairs, chunk, n_wg,
                                       ctx->d_locus_keys.as<uint32_t>(), ctx->d_locus_hist.as<uint32_t>(), key_lo, n_here, key_lo == 0u ? 1u : 0u);
                }
            }
            int rc = vs_scan_u32(ctx, ctx->d_locus_hist.as<const uint32_t>(), ctx->d_locus_hist.as<uint32_t>(), nk * n_wg,
                                 ctx->d_scan_tmp.as<uint64_t>(), nullptr);
            if (rc) return rc;
            // (the scatter in launches of pl.locus_scatter_keys keys, at most a pass's: the places one launch writes fit the L2s)
            const uint32_t sc_keys = pl.locus_scatter_keys;
            for (uint32_t key_lo = 0; key_lo < nk; key_lo += sc_keys) {
                const uint32_t n_here = (uint32_t)(nk - key_lo < sc_keys ? nk - key_lo : sc_keys);
                hipLaunchKernelGGL(k_locus_scatter, dim3(n_wg), dim3(LOCUS_TPB), lds_keys, st, key_lo, n_here, n_pairs, chunk, n_wg,
                                   ctx->d_locus_keys.as<const uint32_t>(), ctx->d_locus_hist.as<const uint32_t>(), ctx->d_perm.as<uint32_t>());
            }
        } else {
            VS_HIP(ctx, hipMemsetAsync(ctx->d_locus_hist.ptr(), 0, sizeof(uint32_t) * nk, st));
            const unsigned pg = (unsigned)((n_pairs + TPB - 1) / TPB);
            hipLaunchKernelGGL(k_pe_locus, dim3(pg), dim3(TPB), 0, st, idx, reads->dev(), n_pairs, ctx->d_locus_keys.as<uint32_t>(),
                               ctx->d_locus_hist.as<uint32_t>());
            int rc = vs_scan_u32(ctx, ctx->d_locus_hist.as<const uint32_t>(), ctx->d_locus_hist.as<uint32_t>(), nk,
                                 ctx->d_scan_tmp.as<uint64_t>(), nullptr);
            if (rc) return rc;
            hipLaunchKernelGGL(k_pe_permute, dim3(pg), dim3(TPB), 0, st, n_pairs, ctx->d_locus_keys.as<const uint32_t>(),
                               ctx->d_locus_hist.as<uint32_t>(), ctx->d_perm.as<uint32_t>());
        }
    }
    VS_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    if (!d_node_mat) VS_HIP(ctx, hipEventRecord(ctx->ev[4], st));
    ctx->last_kernel = tf->name;
    {
        void *kargs[] = {(void *)&P};
        VS_HIP(ctx, hipLaunchKernel(tf->fn, dim3((unsigned)pl.grid), dim3(TTPB), kargs, lds, st));
    }
    if (d_node_mat) {
        const StdTable tab = pl.sw ? vs_std_table((int)pl.mode, true, pl.ad != 0u) : StdTable{pl.pool, 0u};  // (as k_pe_tiles takes them)
        ctx->last_handoff.pairs = n_pairs;
        ctx->last_handoff.list_ends = pl.list_ends;
        ctx->last_handoff.ept = pl.ept;
        ctx->last_handoff.rows = pl.use_rows;
        ctx->last_handoff.pool = tab.pool;
        ctx->last_handoff.trim = tab.trim;
        const int rc = pe_count_from_lists(ctx, pl, idx.n_nodes, 2ull * n_pairs, d_node_mat, d_short_mat, d_tile_map);
        if (rc) return rc;
    }
    VS_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    // overflow pairs: one wavefront per pair with its state in LDS first, the general kernel for what that cannot hold
    const bool no_mid = ctx->tune.no_mid;
    ctx->last_launched |= no_mid ? 0u : VS_RAN_PE_MID;
    if (!no_mid) {
        hipLaunchKernelGGL(k_pe_mid, dim3((unsigned)ctx->n_cu * 8u), dim3(TPB), 0, st, P, ctx->d_slow_list.as<const uint32_t>(),
                           ctx->d_slow_count.as<const uint32_t>(), (uint32_t)n_pairs, ctx->d_slow_list2.as<uint32_t>(), ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_SLOW);
        hipLaunchKernelGGL(k_pe_slow, dim3(pl.slow_grid), dim3(TPB), 0, st, P, ctx->d_dense.as<uint32_t>(), (uint32_t)n_pairs,
                           ctx->d_slow_list2.as<const uint32_t>(), ctx->d_slow_count.as<const uint32_t>() + vs_ctx::SC_SLOW);
    } else {
        hipLaunchKernelGGL(k_pe_slow, dim3(pl.slow_grid), dim3(TPB), 0, st, P, ctx->d_dense.as<uint32_t>(), (uint32_t)n_pairs,
                           ctx->d_slow_list.as<const uint32_t>(), ctx->d_slow_count.as<const uint32_t>());
    }
    ctx->last_overflow.pairs = n_pairs;
    ctx->last_overflow.no_mid = no_mid ? 1u : 0u;
    VS_HIP(ctx, hipEventRecord(ctx->ev[2], st));
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

extern "C" int vs_pe_count(vs_ctx *ctx, const vs_reads *reads, uint32_t *d_node_mat, uint32_t *d_short_mat, uint64_t *d_stats) {
    if (!ctx || !reads || !d_node_mat || !d_short_mat || !d_stats) return VS_E_ARG;
    return pe_launch(ctx, reads, d_node_mat, d_short_mat, d_stats, nullptr, nullptr, 0);
}

extern "C" int vs_pe_count_tracked(vs_ctx *ctx, const vs_reads *reads, uint32_t *d_node_mat, uint32_t *d_short_mat, uint64_t *d_stats,
                                   uint8_t *d_tile_map) {
    if (!ctx || !reads || !d_node_mat || !d_short_mat || !d_stats || !d_tile_map) return VS_E_ARG;
    return pe_launch(ctx, reads, d_node_mat, d_short_mat, d_stats, nullptr, nullptr, 0, d_tile_map);
}

extern "C" int vs_counts_zero_tracked(vs_ctx *ctx, uint32_t *d_node_mat, uint32_t *d_short_mat, uint32_t n, uint8_t *d_tile_map) {
    if (!ctx || (n && (!d_node_mat || !d_short_mat || !d_tile_map))) return vs_fail(ctx, VS_E_ARG, "vs_counts_zero_tracked: bad argument");
    if (!n) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t T = (n + 63u) >> 6;
    const uint64_t tiles = 2ull * T * T;
    if (tiles > 0x7FFFFFFFull) return vs_fail(ctx, VS_E_RANGE, "vs_counts_zero_tracked: %u nodes make more tiles than one launch takes", n);
    hipLaunchKernelGGL(k_zero_tiles, dim3((unsigned)((tiles + 63u) / 64u)), dim3(64), 0, ctx->stream, d_node_mat, d_short_mat, n, T, d_tile_map, tiles);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// ---- testing aids: the counter stage alone, the locus order observed ---------------------------------------------------
// The plan vs_pe_count would make for a block of n_ends ends of 150 bases at k = 55 on a graph of n_nodes nodes.
static PePlan pe_lists_plan(vs_ctx *ctx, uint32_t n_nodes, uint64_t n_ends, bool tile_map) {
    if (ctx->experiment) vs_tuning_load(ctx->tune, true);
    PePlanIn in;
    in.n_nodes = n_nodes; in.K = STD_K; in.w = STD_W; in.s = STD_S;
    in.n_cu = (uint32_t)ctx->n_cu;
    in.n_ends = n_ends; in.max_len = 150u;
    in.count = true; in.tile_map = tile_map;
    in.tune = ctx->tune;
    return vs_pe_plan(in);
}

extern "C" uint32_t vs_pe_lists_ept(vs_ctx *ctx) { return ctx ? pe_lists_plan(ctx, 1u, 2u, false).ept : 0u; }

extern "C" int vs_pe_count_lists(vs_ctx *ctx, uint32_t n_nodes, uint64_t n_pairs, const uint32_t *lists, const uint32_t *counts,
                                 uint32_t *d_node_mat, uint32_t *d_short_mat, uint8_t *d_tile_map) {
    if (!ctx) return VS_E_ARG;
    if (n_pairs && (!lists || !counts || !d_node_mat || !d_short_mat)) return vs_fail(ctx, VS_E_ARG, "vs_pe_count_lists: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ctx->last_ms[0] = ctx->last_ms[1] = ctx->last_ms[2] = 0;
    ctx->last_launched = 0;
    ctx->last_order_pairs = 0;
    ctx->last_handoff = {};  // (the lists here are the host's: nothing a mapping kernel left)
    ctx->last_overflow = {};
    ctx->last_kernel = "";
    const PePlan pl = pe_lists_plan(ctx, n_nodes, 2u * n_pairs, d_tile_map != nullptr);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "%s", pl.msg);
    if (!pl.n_tiles) return VS_OK;  // an empty block
    std::vector<uint32_t> h_lists(pl.list_words), h_counts(pl.list_ends);
    char msg[128];
    const int prc = vs_pe_pack_lists(n_nodes, n_pairs, lists, counts, pl.ept, pl.list_ends, pl.use_rows != 0u, h_lists.data(), h_counts.data(), msg, sizeof msg);
    if (prc != VS_OK) return vs_fail(ctx, prc, "vs_pe_count_lists: %s", msg);
    VS_HIP(ctx, ctx->d_slow_count.reserve(sizeof(uint32_t) * vs_ctx::SC_WORDS));
    VS_HIP(ctx, ctx->d_lists.reserve(sizeof(uint32_t) * pl.list_words));
    VS_HIP(ctx, ctx->d_list_counts.reserve(sizeof(uint32_t) * (pl.list_ends + 2)));
    // (as pe_launch does before every count: the queue word of k_pe_accumulate, the overflow count vs_pe_last_timing reads)
    VS_HIP(ctx, hipMemsetAsync(ctx->d_slow_count.ptr(), 0, sizeof(uint32_t) * vs_ctx::SC_WORDS, st));
    VS_HIP(ctx, hipEventRecord(ctx->ev[3], st));
    VS_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    // (the host writes what k_pe_tiles writes: the used end slots; the rest of the last tile is the shared code's)
    // The copies are waited for before anything can return: h_lists / h_counts are pageable and die with this frame.
    const hipError_t e_lists = hipMemcpyAsync(ctx->d_lists.ptr(), h_lists.data(), sizeof(uint32_t) * pl.list_words, hipMemcpyHostToDevice, st);
    const hipError_t e_counts = hipMemcpyAsync(ctx->d_list_counts.ptr(), h_counts.data(), sizeof(uint32_t) * 2u * n_pairs, hipMemcpyHostToDevice, st);
    const hipError_t e_sync = hipStreamSynchronize(st);
    VS_HIP(ctx, e_lists);
    VS_HIP(ctx, e_counts);
    VS_HIP(ctx, e_sync);
    int rc = pe_count_from_lists(ctx, pl, n_nodes, 2ull * n_pairs, d_node_mat, d_short_mat, d_tile_map);
    if (rc == VS_OK) {
        VS_HIP(ctx, hipEventRecord(ctx->ev[1], st));
        VS_HIP(ctx, hipEventRecord(ctx->ev[2], st));
        VS_HIP(ctx, hipGetLastError());
    }
    VS_HIP(ctx, hipStreamSynchronize(st));  // (the aid returns with the counters written)
    return rc;
}

extern "C" int vs_pe_last_order(vs_ctx *ctx, uint32_t *keys, uint32_t *perm, uint64_t cap, uint64_t info[2]) {
    if (!ctx || !info) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ctx->last_order_pairs;
    const uint32_t sort = ctx->last_launched & (VS_RAN_LOCUS_LDS_SORT | VS_RAN_LOCUS_GLOBAL_SORT);
    info[0] = n;
    info[1] = sort;
    const uint64_t m = n < cap ? n : cap;
    if (!sort || !m) return VS_OK;
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (keys) VS_HIP(ctx, hipMemcpy(keys, ctx->d_locus_keys.ptr(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    if (perm) VS_HIP(ctx, hipMemcpy(perm, ctx->d_perm.ptr(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    return VS_OK;
}

extern "C" int vs_pe_last_handoff(vs_ctx *ctx, uint32_t *lists, uint64_t cap_words, uint32_t *counts, uint64_t cap_ends, uint32_t *overflow,
                                  uint64_t cap_overflow, uint64_t info[9]) {
    if (!ctx || !info) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const vs_ctx::LastHandoff &h = ctx->last_handoff;
    for (int i = 0; i < 9; i++) info[i] = 0;
    if (!h.pairs) return VS_OK;  // no hand-off: vs_pe_map_ends, an empty block, vs_pe_count_lists, a call that failed before its launch
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t n_over = 0;  // (word SC_MID: k_pe_tiles counts into it, k_pe_mid only reads it and counts its own list in SC_SLOW)
    VS_HIP(ctx, hipMemcpy(&n_over, ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_MID, sizeof n_over, hipMemcpyDeviceToHost));
    const uint64_t words = vs_pe_pack_words(h.list_ends, h.rows != 0u);
    info[0] = 1; info[1] = h.pairs; info[2] = h.ept; info[3] = h.list_ends; info[4] = h.rows;
    info[5] = h.pool; info[6] = h.trim; info[7] = n_over; info[8] = words;
    const uint64_t over = n_over < h.pairs ? n_over : h.pairs;  // (the list has a slot per pair)
    const uint64_t mw = words < cap_words ? words : cap_words, me = h.list_ends < cap_ends ? h.list_ends : cap_ends;
    const uint64_t mo = over < cap_overflow ? over : cap_overflow;
    if (lists && mw) VS_HIP(ctx, hipMemcpy(lists, ctx->d_lists.ptr(), sizeof(uint32_t) * mw, hipMemcpyDeviceToHost));
    if (counts && me) VS_HIP(ctx, hipMemcpy(counts, ctx->d_list_counts.ptr(), sizeof(uint32_t) * me, hipMemcpyDeviceToHost));
    if (overflow && mo) VS_HIP(ctx, hipMemcpy(overflow, ctx->d_slow_list.ptr(), sizeof(uint32_t) * mo, hipMemcpyDeviceToHost));
    return VS_OK;
}

extern "C" int vs_pe_last_overflow(vs_ctx *ctx, uint32_t *second, uint64_t cap, uint64_t info[4]) {
    if (!ctx || !info) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const vs_ctx::LastOverflow &o = ctx->last_overflow;
    for (int i = 0; i < 4; i++) info[i] = 0;
    if (!o.pairs) return VS_OK;  // the overflow kernels did not run: an empty block, vs_pe_count_lists, a call that failed before its launch
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t n_first = 0, n_second = 0;  // (SC_MID: k_pe_tiles counts into it; SC_SLOW: k_pe_mid does, and stays 0 without it)
    VS_HIP(ctx, hipMemcpy(&n_first, ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_MID, sizeof n_first, hipMemcpyDeviceToHost));
    VS_HIP(ctx, hipMemcpy(&n_second, ctx->d_slow_count.as<uint32_t>() + vs_ctx::SC_SLOW, sizeof n_second, hipMemcpyDeviceToHost));
    info[0] = 1; info[1] = n_first; info[2] = n_second; info[3] = o.no_mid;
    const uint64_t held = n_second < o.pairs ? n_second : o.pairs;  // (the list has a slot per pair)
    const uint64_t m = held < cap ? held : cap;
    if (second && m) VS_HIP(ctx, hipMemcpy(second, ctx->d_slow_list2.ptr(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    return VS_OK;
}

extern "C" const char *vs_pe_last_kernel(const vs_ctx *ctx) { return ctx ? ctx->last_kernel : ""; }
extern "C" uint32_t vs_pe_last_launched(const vs_ctx *ctx) { return ctx ? ctx->last_launched : 0u; }

extern "C" int vs_pe_last_timing(vs_ctx *ctx, double ms[5]) {
    if (!ctx || !ms) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    VS_HIP(ctx, hipEventSynchronize(ctx->ev[2]));
    float a = 0, b = 0, c = 0, d = 0;
    VS_HIP(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    VS_HIP(ctx, hipEventElapsedTime(&d, ctx->ev[4], ctx->ev[1]));
    if (d > a) d = 0;  // no accumulate pass in this call
    a -= d;
    VS_HIP(ctx, hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]));
    VS_HIP(ctx, hipEventElapsedTime(&c, ctx->ev[3], ctx->ev[0]));
    ctx->last_sort_ms = c;
    uint32_t n_slow = 0;
    VS_HIP(ctx, hipMemcpy(&n_slow, ctx->d_slow_count.ptr(), sizeof n_slow, hipMemcpyDeviceToHost));
    ms[0] = a; ms[1] = b; ms[2] = (double)n_slow; ms[3] = c; ms[4] = d;
    ctx->last_ms[0] = a; ctx->last_ms[1] = b; ctx->last_ms[2] = n_slow;
    return VS_OK;
}

extern "C" int vs_pe_map_ends(vs_ctx *ctx, const vs_reads *reads, uint32_t cap, uint32_t *lists, uint32_t *counts) {
    if (!ctx || !reads || !lists || !counts || !cap) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t n = reads->n_ends;
    if (!n) return VS_OK;
    VsDevBuf lists_buf, counts_buf;
    VS_HIP(ctx, lists_buf.reserve(sizeof(uint32_t) * n * cap));
    VS_HIP(ctx, counts_buf.reserve(sizeof(uint32_t) * n));
    uint32_t *d_lists = lists_buf.as<uint32_t>(), *d_counts = counts_buf.as<uint32_t>();
    VS_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * n, ctx->stream));
    VS_HIP(ctx, hipMemsetAsync(d_lists, 0xFF, sizeof(uint32_t) * n * cap, ctx->stream));
    const int rc = pe_launch(ctx, reads, nullptr, nullptr, nullptr, d_lists, d_counts, cap);
    if (rc != VS_OK) return rc;
    VS_HIP(ctx, hipMemcpyAsync(lists, d_lists, sizeof(uint32_t) * n * cap, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipMemcpyAsync(counts, d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

// ---- segment depth from the reads (vs_node_depth) -------------------------------------------------------------------
// KC[n] = the number of (read end, read offset, table entry of node n) coincidences over all ends of a block: the sum of
// the `v` above over the ends, before any acceptance test and without the pair filter (the definition: vs_depth_plan.h,
// tests/node_depth_model.py).  The lists, the locus sort and the counter kernels are not involved.
//   A workgroup of sixteen wavefronts takes a contiguous share of the block's ends; its wavefronts draw batches of 64 ends
//   off an LDS counter and work alone (no workgroup barrier inside the loop):
//     the ends' probe counts scanned over the lanes -> one lane per (end, probe), 64 at a time: seed key, table probe;
//     the probes' posting counts scanned -> one lane per posting, 64 at a time (a seed with a hundred postings fills
//     two rounds of lanes instead of holding one lane a hundred turns): vs_extend under the mask for ends that hold bytes
//     outside ACGT ('N' included: every end is counted here, so the block must have kept its mask, vs_ctx_keep_masks);
//     a match credits len - K + 1, once, by the first grid point inside it (as k_pe_slow).
//   Credits are summed on chip before they reach memory:
//     graphs of up to DEPTH_LDS_NODES nodes: a dense uint32 counter per node in LDS, added to the uint64 totals with one
//       atomic per non-zero counter when the workgroup is done (a counter that wraps carries 2^32 into the total at once);
//     larger graphs: the 64 credits of a round meet in 64 combining slots of the wavefront (slot by a hash of the node, the
//       last writer's node owns it), one atomic per slot; credits of nodes that lost their slot go to the totals directly.
#include "vs_depth_plan.h"

struct DepthParams {
    VsIndexDev idx;
    VsReadsDev rd;
    unsigned long long *kc;  // [n_nodes] totals, ADDED to
    uint64_t ends_per_wg;
    uint32_t lds_nodes;      // dense counters in LDS; 0: the global route
};

__device__ __forceinline__ const uint32_t *vs_depth_mask(const VsReadsDev &rd, uint32_t meta) {
    return ((meta >> 24) & (VS_FLAG_N | VS_FLAG_INVALID)) ? rd.mask : nullptr;
}

__global__ void __launch_bounds__(DEPTH_TPB)
k_node_depth(DepthParams P) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    const bool dense = P.lds_nodes != 0u;
    uint32_t *s_kc = vs_lds;  // [lds_nodes]
    uint32_t *s_head = vs_lds + ((P.lds_nodes + 3u) & ~3u);
    uint32_t *sw = s_head + DEPTH_HEAD_WORDS + wave * DEPTH_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u, *s_hk = sw + 322u, *s_hv = sw + 386u;
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    for (uint32_t i = tid; i < P.lds_nodes; i += DEPTH_TPB) s_kc[i] = 0u;
    if (tid == 0u) s_head[0] = 0u;
    s_hk[lane] = EMPTY_NODE;
    s_hv[lane] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                uint32_t node = EMPTY_NODE, credit = 0u;
                if (t2 < total) {
                    const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                    const uint32_t k2 = t2 - s_cnt[pr];
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                    const uint32_t j = ej & VS_LEN_MASK;
                    const uint64_t e = e0 + (ej >> 24);
                    const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                    const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                    const uint32_t *mk = vs_depth_mask(P.rd, meta);
                    uint32_t nd, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[nd];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len)) {
                        node = nd;
                        credit = len - K + 1u;
                    }
                }
                if (dense) {
                    if (credit) {
                        const uint32_t old = atomicAdd(&s_kc[node], credit);
                        if (old + credit < old) atomicAdd(&P.kc[node], 1ull << 32);  // the counter wrapped: its carry
                    }
                } else {
                    const uint32_t slot = (node * 0x9E3779B1u) >> 26;
                    if (credit) s_hk[slot] = node;  // (racing plain stores: one node owns the slot this round)
                    vs_wave_sync();
                    if (credit) {
                        if (s_hk[slot] == node) atomicAdd(&s_hv[slot], credit);  // (at most 64 x 2^24)
                        else atomicAdd(&P.kc[node], (unsigned long long)credit);
                    }
                    vs_wave_sync();
                    const uint32_t v = s_hv[lane];
                    if (v) {
                        atomicAdd(&P.kc[s_hk[lane]], (unsigned long long)v);
                        s_hv[lane] = 0u;
                    }
                    vs_wave_sync();
                }
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // s_np is rewritten by the next batch
    }
    __syncthreads();
    for (uint32_t i = tid; i < P.lds_nodes; i += DEPTH_TPB) {
        const uint32_t v = s_kc[i];
        if (v) atomicAdd(&P.kc[i], (unsigned long long)v);
    }
}

extern "C" int vs_depth_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t plan[8]) {
    if (!plan) return VS_E_ARG;
    const DepthPlan p = vs_depth_plan_for(n_nodes, ksize + 1u, n_ends, max_len, n_cu);
    plan[0] = p.route; plan[1] = p.grid; plan[2] = p.ends_per_wg; plan[3] = p.wrap_ends;
    plan[4] = p.lds_nodes; plan[5] = p.lds_bytes; plan[6] = DEPTH_LDS_NODES; plan[7] = DEPTH_TPB;
    return p.status;
}

extern "C" int vs_node_depth(vs_ctx *ctx, const vs_reads *reads, uint64_t *d_kc) {
    if (!ctx || !reads || !d_kc) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_depth: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const DepthPlan pl = vs_depth_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_depth: %s", pl.msg);
    if (pl.route == VS_DEPTH_NONE) return VS_OK;  // no end of the block holds a window
    DepthParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.kc = (unsigned long long *)d_kc;
    P.ends_per_wg = pl.ends_per_wg;
    P.lds_nodes = pl.lds_nodes;
    if (pl.lds_bytes > 64u * 1024u)
        VS_HIP(ctx, hipFuncSetAttribute((const void *)k_node_depth, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
    hipLaunchKernelGGL(k_node_depth, dim3(pl.grid), dim3(DEPTH_TPB), pl.lds_bytes, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// ---- contigs threaded through the graph: the matches (vs_contig_mems) ------------------------------------------------
// Every maximal exact match of K bases or more between a contig (an end of an ordinary block, masks kept) and a strand of
// a segment, as a record of VS_MEM_WORDS words (vs_contig_chain.h, where the host chains them into a .paths entry).  The
// probe grid, the table probe and vs_extend are k_node_depth's: where that kernel adds len - K + 1 to a counter, this one
// appends {contig, contig offset, segment | strand << 31, segment pos, length}, once per match, by the first grid point
// inside it.  Contigs are few and long where reads are many and short, so the lanes are dealt over the PROBES of the whole
// block, not over its ends: k_contig_probes writes every end's probe count, a scan turns them into first probes, and
// thread t of k_contig_mems takes probe t (its end by a binary search of the scan), 256 probes a workgroup -- a contig of a
// million bases is spread over two thousand workgroups.  Inside a wavefront the 64 probes' posting counts are scanned
// and the postings dealt one per lane, 64 at a time, as in k_node_depth.  Appends are claimed per wavefront: one ballot,
// one atomic on the record count by the first lane that has a match.  The count goes on beyond the buffer's capacity
// while the stores stop at it, so the host sees a pass that did not fit and runs it once more in a buffer that does.
#include "vs_contig_chain.h"

#define MEMS_TPB 256u
#define MEMS_WAVES (MEMS_TPB / 64u)
#define MEMS_WAVE_WORDS 324u    // the scan of 64 probes' posting counts [65], their payloads, ends and read offsets [4 x 64] (5 KB a workgroup)
#define MEMS_FIRST_CAP 4096ull  // records of the buffer's first allocation

struct MemsParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *pscan;      // [n_ends + 1] the first probe of every end, the total behind them
    uint32_t total;             // probes of the block
    uint32_t shift;             // contig = end >> shift (1: a singles block, whose odd ends are absent)
    uint32_t *out;              // [cap] records
    unsigned long long cap;
    unsigned long long *count;  // records found, stored or not
};

__global__ void __launch_bounds__(256)
k_contig_probes(VsReadsDev rd, uint32_t w, uint32_t s, uint32_t *np) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e > rd.n_ends) return;
    uint32_t v = 0u;
    if (e < rd.n_ends) {
        const uint32_t meta = rd.meta[e];
        if (!((meta >> 24) & VS_FLAG_ABSENT)) v = vs_seed_probes(meta & VS_LEN_MASK, w, s);
    }
    np[e] = v;  // (np[n_ends] = 0: its scan is the total)
}

__global__ void __launch_bounds__(MEMS_TPB)
k_contig_mems(MemsParams P) {
    __shared__ uint32_t s_mem[MEMS_WAVES * MEMS_WAVE_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *sw = s_mem + wave * MEMS_WAVE_WORDS;
    uint32_t *s_cnt = sw, *s_pa = sw + 65u, *s_pb = sw + 129u, *s_pe = sw + 193u, *s_pj = sw + 257u;
    const uint64_t t = (uint64_t)blockIdx.x * MEMS_TPB + tid;  // (a wavefront's 64 probes are consecutive)
    uint32_t c = 0u, pa = 0u, pb = 0u, pe = 0u, pj = 0u;
    if (t < P.total) {
        const uint32_t e = vs_upper_idx(P.pscan, (uint32_t)P.rd.n_ends + 1u, (uint32_t)t);  // pscan[e] <= t < pscan[e + 1]
        const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
        const uint32_t j = vs_seed_phase(rlen, w, s) + ((uint32_t)t - P.pscan[e]) * s;
        const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
        const uint32_t *mk = vs_depth_mask(P.rd, meta);
        if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
            uint32_t sr;
            const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
            c = vs_probe(P.idx, key, sr, &pa, &pb);
        }
        pe = e;
        pj = j;
    }
    s_pa[lane] = pa;
    s_pb[lane] = pb;
    s_pe[lane] = pe;
    s_pj[lane] = pj;
    s_cnt[lane + 1u] = vs_wave_scan_add(c);
    if (lane == 0u) s_cnt[0] = 0u;
    vs_wave_sync();
    const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
    for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
        // postings q0 .. q0 + 63 of these probes: one per lane
        const uint32_t t2 = q0 + lane;
        bool found = false;
        uint32_t r_e = 0u, r_off = 0u, r_seg = 0u, r_pos = 0u, r_len = 0u;
        if (t2 < total) {
            const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
            const uint32_t k2 = t2 - s_cnt[pr];
            const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], e = s_pe[pr], j = s_pj[pr];
            const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
            const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
            const uint32_t *mk = vs_depth_mask(P.rd, meta);
            uint32_t nd, pos, opp;
            VsNodeMeta nm;
            if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                nm = P.idx.meta[nd];
            } else {
                const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                nm.woff = po.woff; nm.len = po.len;
            }
            const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
            const uint32_t q = opp ? nm.len - pos - w : pos;
            uint32_t a, qa, len;
            // (k >= 95: VS_SEED_VERIFIED is 0, the key only nominated the posting and the comparison starts at the seed's first base)
            if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len)) {
                found = true;
                r_e = e; r_off = a; r_seg = nd | (opp << 31); r_pos = qa; r_len = len;
            }
        }
        const unsigned long long have = __ballot(found);
        if (have) {
            const uint32_t leader = (uint32_t)__ffsll((long long)have) - 1u;
            unsigned long long base = 0ull;
            if (lane == leader) base = atomicAdd(P.count, (unsigned long long)__popcll(have));
            const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)leader), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)leader);
            const unsigned long long at = (((unsigned long long)b_hi << 32) | b_lo) + (unsigned long long)__popcll(have & ((1ull << lane) - 1ull));
            if (found && at < P.cap) {
                uint32_t *rec = P.out + at * VS_MEM_WORDS;
                rec[0] = r_e >> P.shift;
                rec[1] = r_off;
                rec[2] = r_seg;
                rec[3] = r_pos;
                rec[4] = r_len;
            }
        }
    }
}

extern "C" int vs_contig_mems(vs_ctx *ctx, const vs_reads *reads, uint32_t *out, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (reads) {
        if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_contig_mems: build an index first (vs_index_build)");
        const VsIndexDev &idx = ctx->idx;
        const uint64_t n_ends = reads->n_ends;
        if (n_ends > 0xFFFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "vs_contig_mems: a block of 2^32 ends or more");
        ctx->mems_info[0] = ctx->mems_info[1] = ctx->mems_info[2] = 0;
        ctx->mems_info[3] = ctx->d_mems.capacity() / (sizeof(uint32_t) * VS_MEM_WORDS);
        if (n_ends && idx.n_nodes && reads->max_len >= idx.K) {
            const uint64_t m = n_ends + 1u, nb = (m + 2047u) / 2048u;
            VS_HIP(ctx, ctx->d_mem_scan.reserve(sizeof(uint32_t) * m));
            VS_HIP(ctx, ctx->d_mem_tmp.reserve(sizeof(uint64_t) * (nb + 3u)));
            uint32_t *d_scan = ctx->d_mem_scan.as<uint32_t>();
            uint64_t *d_tmp = ctx->d_mem_tmp.as<uint64_t>(), *d_total = d_tmp + nb + 1u, *d_count = d_tmp + nb + 2u;
            hipLaunchKernelGGL(k_contig_probes, dim3((unsigned)((m + 255u) / 256u)), dim3(256), 0, st, reads->dev(), idx.w, idx.s, d_scan);
            VS_HIP(ctx, hipGetLastError());
            if (int rc = vs_scan_u32(ctx, d_scan, d_scan, m, d_tmp, d_total)) return rc;
            uint64_t probes = 0;
            VS_HIP(ctx, hipMemcpyAsync(&probes, d_total, sizeof probes, hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
            if (probes > 0xFFFFFFF0ull) return vs_fail(ctx, VS_E_RANGE, "vs_contig_mems: %llu probes in one block: give the contigs in several", (unsigned long long)probes);
            ctx->mems_info[2] = probes;
            if (probes) {
                if (!ctx->d_mems.capacity()) VS_HIP(ctx, ctx->d_mems.reserve(sizeof(uint32_t) * VS_MEM_WORDS * MEMS_FIRST_CAP));
                MemsParams P;
                P.idx = idx;
                P.rd = reads->dev();
                P.pscan = d_scan;
                P.total = (uint32_t)probes;
                P.shift = reads->unpaired ? 1u : 0u;
                P.count = (unsigned long long *)d_count;
                uint64_t found = 0;
                for (int pass = 0;; pass++) {
                    P.out = ctx->d_mems.as<uint32_t>();
                    P.cap = ctx->d_mems.capacity() / (sizeof(uint32_t) * VS_MEM_WORDS);
                    VS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
                    hipLaunchKernelGGL(k_contig_mems, dim3((unsigned)((probes + MEMS_TPB - 1u) / MEMS_TPB)), dim3(MEMS_TPB), 0, st, P);
                    VS_HIP(ctx, hipGetLastError());
                    VS_HIP(ctx, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, st));
                    VS_HIP(ctx, hipStreamSynchronize(st));
                    ctx->mems_info[1]++;
                    if (found <= P.cap) break;
                    // the pass did not fit: once more, in a buffer of the size it asked for (the stream is idle: synchronised above)
                    if (pass) return vs_fail(ctx, VS_E_STATE, "vs_contig_mems: %llu matches after %llu in the same block", (unsigned long long)found, (unsigned long long)P.cap);
                    VS_HIP(ctx, ctx->d_mems.reserve(sizeof(uint32_t) * VS_MEM_WORDS * found));
                }
                ctx->mems_info[0] = found;
            }
        }
    }
    *n = ctx->mems_info[0];
    if (out && *n && cap >= *n) {
        VS_HIP(ctx, hipMemcpyAsync(out, ctx->d_mems.ptr(), sizeof(uint32_t) * VS_MEM_WORDS * *n, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
    }
    return VS_OK;
}

extern "C" int vs_contig_mems_last(vs_ctx *ctx, uint64_t info[4]) {
    if (!ctx || !info) return VS_E_ARG;
    for (int i = 0; i < 4; i++) info[i] = ctx->mems_info[i];
    return VS_OK;
}

extern "C" int vs_contig_chain(const uint32_t *mems, uint64_t n_mems, const uint32_t *seg_len, uint32_t n_segs, uint32_t ksize, uint32_t n_contigs,
                               uint32_t *tokens, uint64_t *n_tokens, uint64_t *ambiguous) {
    if ((n_mems && (!mems || !tokens)) || (n_segs && !seg_len) || !n_tokens || (n_contigs && !ambiguous)) return VS_E_ARG;
    const uint32_t K = ksize + 1u;
    std::vector<VsMem> v((size_t)n_mems);
    for (uint64_t i = 0; i < n_mems; i++) {
        const uint32_t *r = mems + i * VS_MEM_WORDS;
        v[i] = VsMem{r[0], r[1], r[2], r[3], r[4]};
        const uint32_t seg = r[2] & 0x7FFFFFFFu;
        if (r[0] >= n_contigs || seg >= n_segs || r[4] < K || (uint64_t)r[3] + r[4] > seg_len[seg]) return VS_E_ARG;
    }
    for (uint32_t c = 0; c < n_contigs; c++) ambiguous[c] = 0;
    std::vector<VsChainToken> tok;
    vs_contig_chain_for(v, seg_len, K, tok, ambiguous);
    for (size_t i = 0; i < tok.size(); i++) {
        uint32_t *o = tokens + i * VS_TOKEN_WORDS;
        o[0] = tok[i].contig; o[1] = tok[i].seg; o[2] = tok[i].windows; o[3] = tok[i].first;
    }
    *n_tokens = tok.size();
    return VS_OK;
}

// ---- per-position depth of every segment from the reads (vs_cover_layout / vs_node_cover / vs_cover_fold) -------------
// cov[n][p] = the triples KC[n] counts (vs_node_depth above) whose table entry is (n, p): what the depth pass sums per
// segment, kept per window (the definition, the slots and the fold rule: vs_cover_plan.h, tests/depth_profile_model.py).
// The end batches, the probe grid, the table probe, the posting deal and vs_extend under the mask are k_node_depth's.  Where
// that kernel keeps len - K + 1 of a match, this one keeps where on the segment it starts and how long it is: a match on the
// forward text covers the windows from p0 = qa, one on the reverse-complement text those from p0 = len_n - qa - len, both up
// to p0 + len - K.  It is written down as a DIFFERENCE -- +1 into slot first[n] + p0, -1 into the slot behind its last
// window -- so a match costs two dword atomics whatever its length, and nothing is combined on chip.  vs_cover_fold turns
// the differences into counts: one exclusive scan over all slots (every segment's slots sum to 0: the -1 of a match flush
// with the segment's end stays in the segment's sentinel slot), then excl[i] + diff[i] added to the 64-bit totals.
#include "vs_cover_plan.h"

struct CoverParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *first;  // [n_nodes + 1] the first slot of every segment, the slot total behind them
    uint32_t *diff;         // [first[n_nodes]] differences, ADDED to
    uint64_t ends_per_wg;
};

__global__ void __launch_bounds__(256)
k_cover_slots(const VsNodeMeta *meta, uint32_t n_nodes, uint32_t K, uint32_t *cnt) {
    const uint64_t n = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (n > n_nodes) return;
    uint32_t v = 0u;
    if (n < n_nodes) {
        const uint32_t len = meta[n].len;
        if (len >= K) v = len - K + 2u;  // its windows and the sentinel
    }
    cnt[n] = v;  // (cnt[n_nodes] = 0: its scan is the total)
}

__global__ void __launch_bounds__(COVER_TPB)
k_node_cover(CoverParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[COVER_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *s_head = s_mem;
    uint32_t *sw = s_mem + COVER_HEAD_WORDS + wave * COVER_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u;
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    if (tid == 0u) s_head[0] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                if (t2 < total) {
                    const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                    const uint32_t k2 = t2 - s_cnt[pr];
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                    const uint32_t j = ej & VS_LEN_MASK;
                    const uint64_t e = e0 + (ej >> 24);
                    const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                    const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                    const uint32_t *mk = vs_depth_mask(P.rd, meta);
                    uint32_t nd, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[nd];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    // (k >= 95: VS_SEED_VERIFIED is 0, the key only nominated the posting and the comparison starts at the seed's first base)
                    if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len) &&
                        qa + len <= nm.len) {  // (a match lies inside its strand: no slot beyond the segment's sentinel)
                        const uint32_t at = P.first[nd] + (opp ? nm.len - qa - len : qa);
                        atomicAdd(&P.diff[at], 1u);
                        atomicAdd(&P.diff[at + len - K + 1u], 0xFFFFFFFFu);
                    }
                }
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // s_np is rewritten by the next batch
    }
}

__global__ void __launch_bounds__(256)
k_cover_fold(const uint32_t *excl, uint32_t *diff, unsigned long long *cov, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t d = diff[i];
    const uint32_t v = excl[i] + d;  // the count since the last fold, below 2^32 by the plan's rule (a sentinel slot: 0)
    if (v) cov[i] += (unsigned long long)v;
    if (d) diff[i] = 0u;
}

extern "C" int vs_cover_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound,
                             uint64_t plan[8]) {
    if (!plan) return VS_E_ARG;
    const CoverPlan p = vs_cover_plan_for(n_nodes, ksize + 1u, n_ends, max_len, n_cu, pending, bound);
    plan[0] = p.launch; plan[1] = p.grid; plan[2] = p.ends_per_wg; plan[3] = p.weight;
    plan[4] = p.fold_first; plan[5] = p.pending; plan[6] = sizeof(uint32_t) * COVER_LDS_WORDS; plan[7] = COVER_TPB;
    return p.status;
}

extern "C" int vs_cover_layout(vs_ctx *ctx, uint32_t *d_first, uint64_t *n_slots) {
    if (!ctx || !d_first || !n_slots) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_cover_layout: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const uint64_t m = (uint64_t)idx.n_nodes + 1u, nb = (m + 2047u) / 2048u;
    VS_HIP(ctx, ctx->d_cover_tmp.reserve(sizeof(uint64_t) * (nb + 2u)));
    uint64_t *d_tmp = ctx->d_cover_tmp.as<uint64_t>(), *d_total = d_tmp + nb + 1u;
    hipLaunchKernelGGL(k_cover_slots, dim3((unsigned)((m + 255u) / 256u)), dim3(256), 0, ctx->stream, idx.meta, idx.n_nodes, idx.K, d_first);
    VS_HIP(ctx, hipGetLastError());
    if (int rc = vs_scan_u32(ctx, d_first, d_first, m, d_tmp, d_total)) return rc;
    uint64_t total = 0;
    VS_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_slots = total;
    if (total >= (1ull << 32))
        return vs_fail(ctx, VS_E_RANGE, "vs_cover_layout: %llu slots, and a slot number has 32 bits: profile the graph in parts", (unsigned long long)total);
    return VS_OK;
}

extern "C" int vs_node_cover(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t *d_diff) {
    if (!ctx || !reads || !d_first || !d_diff) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_cover: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const CoverPlan pl = vs_cover_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu, 0, 0);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_cover: %s", pl.msg);
    if (!pl.launch) return VS_OK;  // no end of the block holds a window
    CoverParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.first = d_first;
    P.diff = d_diff;
    P.ends_per_wg = pl.ends_per_wg;
    hipLaunchKernelGGL(k_node_cover, dim3(pl.grid), dim3(COVER_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

extern "C" int vs_cover_fold(vs_ctx *ctx, uint32_t *d_diff, uint64_t *d_cov, uint64_t n_slots) {
    if (!ctx || (n_slots && (!d_diff || !d_cov))) return VS_E_ARG;
    if (n_slots >= (1ull << 32)) return vs_fail(ctx, VS_E_RANGE, "vs_cover_fold: %llu slots", (unsigned long long)n_slots);
    if (!n_slots) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t nb = (n_slots + 2047u) / 2048u;
    VS_HIP(ctx, ctx->d_cover_scan.reserve(sizeof(uint32_t) * n_slots));
    VS_HIP(ctx, ctx->d_cover_tmp.reserve(sizeof(uint64_t) * (nb + 2u)));
    uint32_t *d_excl = ctx->d_cover_scan.as<uint32_t>();
    if (int rc = vs_scan_u32(ctx, d_diff, d_excl, n_slots, ctx->d_cover_tmp.as<uint64_t>(), nullptr)) return rc;
    hipLaunchKernelGGL(k_cover_fold, dim3((unsigned)((n_slots + 255u) / 256u)), dim3(256), 0, ctx->stream, d_excl, d_diff, (unsigned long long *)d_cov, n_slots);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// ---- base pileup of every segment from the reads (vs_pileup_layout / vs_node_pileup; the depth folds by vs_cover_fold) ----
// One step past vs_extend: the read is laid along the diagonal of an exact anchor ACROSS its mismatches, the overlap is
// counted once and what differs is written down (the definition, the slots and the fold rule: vs_pileup_plan.h,
// tests/pileup_model.py; the walk: vs_pileup_core.h).  The end batches, the probe grid, the table probe, the posting deal and
// vs_extend under the mask are k_node_cover's.  The lane that holds a match (a, qa, len) looks LEFT along the diagonal for
// another run of K agreeing bases: if there is one, an earlier match owns the alignment and this lane is done -- once per
// diagonal, with no word passed between lanes.  The owner counts the non-agreeing positions of the whole overlap; above the
// budget the alignment is rejected and only tallied.  Otherwise the depth is written as a DIFFERENCE, +1 into the slot of the
// overlap's first forward position and -1 into the slot behind its last (two dword atomics, whatever the overlap's length),
// and every non-agreeing position costs one 64-bit atomic into alt[slot][c]; an agreeing base costs nothing, the reference
// base's count being the depth minus the others.  The two tallies are claimed per wavefront by ballot, as k_contig_mems
// claims its records.
#include "vs_pileup_core.h"
#include "vs_pileup_plan.h"

struct PileupParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *first;     // [n_nodes + 1] the first slot of every segment, the slot total behind them
    uint32_t *diff;            // [first[n_nodes]] differences of the depth, ADDED to
    unsigned long long *alt;   // [first[n_nodes]][PILEUP_ALT] non-agreeing bases, ADDED to
    unsigned long long *tally; // [2] alignments credited, alignments rejected, ADDED to
    uint64_t ends_per_wg;
    uint32_t max_mismatch;
};

__global__ void __launch_bounds__(256)
k_pileup_slots(const VsNodeMeta *meta, uint32_t n_nodes, uint32_t K, uint32_t *cnt) {
    const uint64_t n = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (n > n_nodes) return;
    uint32_t v = 0u;
    if (n < n_nodes) {
        const uint32_t len = meta[n].len;
        if (len >= K) v = len + 1u;  // its positions and the sentinel
    }
    cnt[n] = v;  // (cnt[n_nodes] = 0: its scan is the total)
}

__device__ __forceinline__ void vs_pileup_tally(unsigned long long *at, bool mine, uint32_t lane) {
    const unsigned long long have = __ballot(mine);
    if (have && lane == (uint32_t)__ffsll((long long)have) - 1u) atomicAdd(at, (unsigned long long)__popcll(have));
}

__global__ void __launch_bounds__(PILEUP_TPB, 8)  // (eight wavefronts a SIMD: two workgroups a CU, as the plan deals them)
k_node_pileup(PileupParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[PILEUP_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *s_head = s_mem;
    uint32_t *sw = s_mem + PILEUP_HEAD_WORDS + wave * PILEUP_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u;
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    if (tid == 0u) s_head[0] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                bool credited = false, rejected = false;
                if (t2 < total) {
                    const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                    const uint32_t k2 = t2 - s_cnt[pr];
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                    const uint32_t j = ej & VS_LEN_MASK;
                    const uint64_t e = e0 + (ej >> 24);
                    const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                    const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                    const uint32_t *mk = vs_depth_mask(P.rd, meta);
                    uint32_t nd, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[nd];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    // (k >= 95: VS_SEED_VERIFIED is 0, the key only nominated the posting and the comparison starts at the seed's first base)
                    if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len) &&
                        qa + len <= nm.len) {  // (a match lies inside its strand: no slot beyond the segment's sentinel)
                        const uint64_t tbase = (uint64_t)nm.woff * 16u;
                        const VsPileupSpan sp = vs_pileup_span(rlen, nm.len, a, qa);
                        if (vs_pileup_owner(P.rd.words, rbase, tw, tbase, mk, sp, a, K)) {
                            uint32_t miss = vs_pileup_count(P.rd.words, rbase, tw, tbase, mk, sp);
                            rejected = miss > P.max_mismatch;
                            credited = !rejected;
                            if (credited) {
                                // the overlap on the strand: [t_lo, t_hi); on the forward text: from p_lo on, as many
                                const uint32_t t_lo = (uint32_t)((int64_t)sp.x_lo + sp.d), t_hi = (uint32_t)((int64_t)sp.x_hi + sp.d);
                                const uint32_t at = P.first[nd] + (opp ? nm.len - t_hi : t_lo);
                                atomicAdd(&P.diff[at], 1u);
                                atomicAdd(&P.diff[at + (sp.x_hi - sp.x_lo)], 0xFFFFFFFFu);
                                for (uint32_t x = sp.x_lo; miss && x < sp.x_hi; x += 32u) {
                                    const uint32_t n = sp.x_hi - x < 32u ? sp.x_hi - x : 32u;
                                    uint64_t f = vs_pl_differ(P.rd.words, rbase, tw, tbase, mk, x, sp.d, n);
                                    if (!f) continue;
                                    const uint64_t rwin = vs_pl_win(P.rd.words, rbase + x);
                                    const uint64_t mwin = mk ? vs_pl_win(mk, rbase + x) : 0ull;
                                    while (f) {
                                        const uint32_t bit = (uint32_t)__ffsll((long long)f) - 1u;  // (even: 2 * the base's place in the window)
                                        f &= f - 1ull;
                                        const uint32_t code = (uint32_t)(rwin >> bit) & 3u;
                                        // the read's base as it reads on the forward strand; a byte outside ACGT: `other`
                                        const uint32_t col = ((mwin >> bit) & 3ull) ? 4u : (opp ? 3u - code : code);
                                        const uint32_t ts = t_lo + (x - sp.x_lo) + (bit >> 1);  // strand offset of the base
                                        const uint64_t slot = (uint64_t)P.first[nd] + (opp ? nm.len - 1u - ts : ts);
                                        atomicAdd(&P.alt[slot * PILEUP_ALT + col], 1ull);
                                        miss--;
                                    }
                                }
                            }
                        }
                    }
                }
                vs_pileup_tally(P.tally, credited, lane);
                vs_pileup_tally(P.tally + 1, rejected, lane);
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // s_np is rewritten by the next batch
    }
}

extern "C" int vs_pileup_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t pending, uint64_t bound,
                              uint64_t plan[8]) {
    if (!plan) return VS_E_ARG;
    const PileupPlan p = vs_pileup_plan_for(n_nodes, ksize + 1u, n_ends, max_len, n_cu, pending, bound);
    plan[0] = p.launch; plan[1] = p.grid; plan[2] = p.ends_per_wg; plan[3] = p.weight;
    plan[4] = p.fold_first; plan[5] = p.pending; plan[6] = sizeof(uint32_t) * PILEUP_LDS_WORDS; plan[7] = PILEUP_TPB;
    return p.status;
}

extern "C" int vs_pileup_scan_host(const uint32_t *read_words, const uint32_t *read_mask, const uint32_t *strand_words, uint32_t rlen, uint32_t tlen,
                                   uint32_t a, uint32_t qa, uint32_t K, uint32_t out[4]) {
    if (!read_words || !strand_words || !out || !K || a >= rlen || qa >= tlen) return VS_E_ARG;
    const VsPileupSpan sp = vs_pileup_span(rlen, tlen, a, qa);
    out[0] = vs_pileup_owner(read_words, 0u, strand_words, 0u, read_mask, sp, a, K);
    out[1] = sp.x_lo;
    out[2] = sp.x_hi;
    out[3] = vs_pileup_count(read_words, 0u, strand_words, 0u, read_mask, sp);
    return VS_OK;
}

extern "C" int vs_pileup_layout(vs_ctx *ctx, uint32_t *d_first, uint64_t *n_slots) {
    if (!ctx || !d_first || !n_slots) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_pileup_layout: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const uint64_t m = (uint64_t)idx.n_nodes + 1u, nb = (m + 2047u) / 2048u;
    VS_HIP(ctx, ctx->d_cover_tmp.reserve(sizeof(uint64_t) * (nb + 2u)));
    uint64_t *d_tmp = ctx->d_cover_tmp.as<uint64_t>(), *d_total = d_tmp + nb + 1u;
    hipLaunchKernelGGL(k_pileup_slots, dim3((unsigned)((m + 255u) / 256u)), dim3(256), 0, ctx->stream, idx.meta, idx.n_nodes, idx.K, d_first);
    VS_HIP(ctx, hipGetLastError());
    if (int rc = vs_scan_u32(ctx, d_first, d_first, m, d_tmp, d_total)) return rc;
    uint64_t total = 0;
    VS_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_slots = total;
    if (total >= (1ull << 32))
        return vs_fail(ctx, VS_E_RANGE, "vs_pileup_layout: %llu slots, and a slot number has 32 bits: pile the graph up in parts", (unsigned long long)total);
    return VS_OK;
}

extern "C" int vs_node_pileup(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t *d_diff, uint64_t *d_alt, uint32_t max_mismatch,
                              uint64_t *d_tally) {
    if (!ctx || !reads || !d_first || !d_diff || !d_alt || !d_tally) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_pileup: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const PileupPlan pl = vs_pileup_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu, 0, 0);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_pileup: %s", pl.msg);
    if (!pl.launch) return VS_OK;  // no end of the block holds an anchor
    PileupParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.first = d_first;
    P.diff = d_diff;
    P.alt = (unsigned long long *)d_alt;
    P.tally = (unsigned long long *)d_tally;
    P.ends_per_wg = pl.ends_per_wg;
    P.max_mismatch = max_mismatch;
    hipLaunchKernelGGL(k_node_pileup, dim3(pl.grid), dim3(PILEUP_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// ---- which variant sites travel together on one read pair (vs_node_site_pairs) ----------------------------------------------
// The first pass of this family that uses the pairing of the reads: what ONE fragment -- the ends 2p and 2p + 1 -- saw at a
// given list of sites is kept together, and every pair of sites it saw adds 1 to a 5 x 5 cell (the definition, the launch and
// the rows of the cell table: vs_site_pairs_plan.h, tests/site_pairs_model.py; the range search, the reduction and the cell:
// vs_site_pairs_core.h).  The end batches, the probe grid, the table probe, the posting deal and vs_extend under the mask are
// k_node_pileup's.  The lane that holds a match looks up the sites under its overlap FIRST -- two binary searches on the
// ascending slot list -- and is done if there are none: no owner walk and no count, so with few sites most alignments cost
// nothing beyond the match.  Otherwise vs_pileup_owner and vs_pileup_count decide as they do for the pileup, and a credited
// alignment claims room for its sites in its fragment's list in LDS with ONE atomic on the list's counter (a batch of 64 ends
// is 32 whole fragments: the plan keeps every workgroup's share and every batch at an even end) and stores the entries that
// still fit among the first 32; the counter runs on, so a fragment with more than 32 raw observations is known as overflow.
// After the batch's last probe round lane f reduces list f in place (sorted; a site seen with two different columns is
// discordant and dropped), then the wavefront goes through the fragments that kept two sites or more and deals the pairs of
// each to its lanes: one 64-bit atomic per stored pair.  The five tallies are summed per batch from ballots and added once.
#include "vs_site_pairs_core.h"
#include "vs_site_pairs_plan.h"

struct SitePairsParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *first;       // [n_nodes + 1] the first slot of every segment (vs_pileup_layout)
    const uint32_t *site_slot;   // [n_sites] the sites' slots, ascending
    const uint32_t *row_first;   // [n_sites + 1] the cells before every site's (vs_site_pairs_rows_host)
    unsigned long long *cells;   // [row_first[n_sites]][25] ADDED to
    unsigned long long *tally;   // [SITE_PAIRS_TALLIES] ADDED to
    uint64_t ends_per_wg;        // a multiple of 64
    uint32_t n_sites;
    uint32_t max_mismatch;
};

__global__ void __launch_bounds__(SITE_PAIRS_TPB, 6)  // (six wavefronts a SIMD: three workgroups a CU, as the plan deals them)
k_node_site_pairs(SitePairsParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[SITE_PAIRS_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *s_head = s_mem;
    uint32_t *sw = s_mem + PILEUP_HEAD_WORDS + wave * SITE_PAIRS_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u;
    uint32_t *s_list = sw + PILEUP_WAVE_WORDS;  // list f: its counter at s_list[f * 33], its entries behind it
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    if (tid == 0u) s_head[0] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;  // (even: e_lo and b are multiples of 64)
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        if (lane < SITE_PAIRS_FRAGS) s_list[lane * SITE_PAIRS_LIST_WORDS] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                if (t2 >= total) continue;
                const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                const uint32_t k2 = t2 - s_cnt[pr];
                const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                const uint32_t j = ej & VS_LEN_MASK, el = ej >> 24;
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                uint32_t nd, pos, opp;
                VsNodeMeta nm;
                if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                    nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                    nm = P.idx.meta[nd];
                } else {
                    const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                    nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                    nm.woff = po.woff; nm.len = po.len;
                }
                const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                const uint32_t q = opp ? nm.len - pos - w : pos;
                uint32_t a, qa, len;
                if (!(nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len) &&
                      qa + len <= nm.len))
                    continue;
                const VsPileupSpan sp = vs_pileup_span(rlen, nm.len, a, qa);
                // the overlap on the strand: [t_lo, t_hi); on the forward text: slots lo .. lo + n - 1 (mirrored on the other strand)
                const uint32_t t_lo = (uint32_t)((int64_t)sp.x_lo + sp.d), t_hi = (uint32_t)((int64_t)sp.x_hi + sp.d);
                const uint32_t base = P.first[nd];
                const uint32_t lo = base + (opp ? nm.len - t_hi : t_lo);
                uint32_t i0, i1;
                vs_site_pairs_range(P.site_slot, P.n_sites, lo, lo + (sp.x_hi - sp.x_lo) - 1u, &i0, &i1);
                if (i0 == i1) continue;  // no site under this alignment
                const uint64_t tbase = (uint64_t)nm.woff * 16u;
                if (!vs_pileup_owner(P.rd.words, rbase, tw, tbase, mk, sp, a, K)) continue;
                if (vs_pileup_count(P.rd.words, rbase, tw, tbase, mk, sp) > P.max_mismatch) continue;  // rejected: observes nothing
                uint32_t *list = s_list + (el >> 1) * SITE_PAIRS_LIST_WORDS;
                const uint32_t at = atomicAdd(&list[0], i1 - i0);  // (a fragment's alignments are few and short: no wrap)
                for (uint32_t i = i0, z = at; i < i1 && z < SITE_PAIRS_CAP; i++, z++) {
                    const uint32_t p = P.site_slot[i] - base;          // forward position
                    const uint32_t ts = opp ? nm.len - 1u - p : p;    // strand offset
                    const uint32_t x = (uint32_t)((int64_t)ts - sp.d);  // read offset, inside [x_lo, x_hi)
                    list[1u + z] = (i << 3) | vs_site_pairs_col(P.rd.words, rbase, mk, x, opp);
                }
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // the lists are complete; s_np is rewritten by the next batch
        // lane f reduces list f
        uint32_t raw = 0u, kept = 0u, bad = 0u;
        if (lane < SITE_PAIRS_FRAGS) {
            raw = s_list[lane * SITE_PAIRS_LIST_WORDS];
            if (raw && raw <= SITE_PAIRS_CAP) kept = vs_site_pairs_reduce(s_list + lane * SITE_PAIRS_LIST_WORDS + 1u, raw, &bad);
            s_list[lane * SITE_PAIRS_LIST_WORDS] = kept;
        }
        const uint32_t n_seen = (uint32_t)__popcll(__ballot(raw > 0u)), n_over = (uint32_t)__popcll(__ballot(raw > SITE_PAIRS_CAP));
        uint32_t n_bad = 0u;
        for (unsigned long long m = __ballot(bad > 0u); m; m &= m - 1ull)  // (discordance is rare: a turn per fragment that has any)
            n_bad += (uint32_t)__builtin_amdgcn_readlane((int)bad, (int)__ffsll((long long)m) - 1);
        vs_wave_sync();
        uint32_t n_stored = 0u, n_unstored = 0u;
        for (unsigned long long m = __ballot(kept > 1u); m; m &= m - 1ull) {
            // fragment f's pairs (ia, ib), ia < ib: lane l takes ia = l & 31 and ib = ia + 1 + (l >> 5), + 2 a turn
            const uint32_t f = (uint32_t)__ffsll((long long)m) - 1u;
            const uint32_t *list = s_list + f * SITE_PAIRS_LIST_WORDS;
            const uint32_t n = list[0], ia = lane & 31u;
            const uint32_t ea = ia < n ? list[1u + ia] : 0u;
            for (uint32_t step = 1u; step < n; step += 2u) {
                const uint32_t ib = ia + step + (lane >> 5);
                bool stored = false, unstored = false;
                if (ib < n) {  // (then ia < n too)
                    const uint32_t eb = list[1u + ib];
                    uint32_t cell;
                    stored = vs_site_pairs_cell(P.row_first, ea >> 3, eb >> 3, &cell) != 0u;
                    unstored = !stored;
                    if (stored) atomicAdd(&P.cells[(uint64_t)cell * SITE_PAIRS_CELL + (ea & 7u) * SITE_PAIRS_COLS + (eb & 7u)], 1ull);
                }
                n_stored += (uint32_t)__popcll(__ballot(stored));
                n_unstored += (uint32_t)__popcll(__ballot(unstored));
            }
        }
        if (lane == 0u) {
            if (n_seen) atomicAdd(P.tally, (unsigned long long)n_seen);
            if (n_over) atomicAdd(P.tally + 1, (unsigned long long)n_over);
            if (n_bad) atomicAdd(P.tally + 2, (unsigned long long)n_bad);
            if (n_stored) atomicAdd(P.tally + 3, (unsigned long long)n_stored);
            if (n_unstored) atomicAdd(P.tally + 4, (unsigned long long)n_unstored);
        }
        vs_wave_sync();  // the lists are zeroed by the next batch
    }
}

extern "C" int vs_site_pairs_plan(uint32_t n_nodes, uint32_t ksize, uint64_t n_ends, uint32_t max_len, uint32_t n_cu, uint64_t plan[8]) {
    if (!plan) return VS_E_ARG;
    const SitePairsPlan p = vs_site_pairs_plan_for(n_nodes, ksize + 1u, n_ends, max_len, n_cu);
    plan[0] = p.launch; plan[1] = p.grid; plan[2] = p.ends_per_wg; plan[3] = 0; plan[4] = 0; plan[5] = 0;
    plan[6] = sizeof(uint32_t) * SITE_PAIRS_LDS_WORDS; plan[7] = SITE_PAIRS_TPB;
    return p.status;
}

extern "C" int vs_site_pairs_rows_host(const uint32_t *seg, const uint32_t *pos, uint64_t n_sites, uint32_t span, uint32_t *row_first, uint64_t *n_cells) {
    if (!row_first || !n_cells || (n_sites && (!seg || !pos))) return VS_E_ARG;
    return vs_site_pairs_rows_for(seg, pos, n_sites, span, row_first, n_cells);
}

extern "C" int vs_site_pairs_frag_host(const uint32_t *raw, uint32_t n, uint32_t *kept, uint32_t out[2]) {
    if (!kept || !out || n > SITE_PAIRS_CAP || (n && !raw)) return VS_E_ARG;
    for (uint32_t i = 0; i < n; i++) kept[i] = raw[i];
    out[0] = vs_site_pairs_reduce(kept, n, &out[1]);
    return VS_OK;
}

extern "C" int vs_node_site_pairs(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, const uint32_t *d_site_slot, uint32_t n_sites,
                                  const uint32_t *d_row_first, uint64_t *d_cells, uint32_t max_mismatch, uint64_t *d_tally) {
    if (!ctx || !reads || !d_tally) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_site_pairs: build an index first (vs_index_build)");
    if (n_sites >= SITE_PAIRS_MAX_SITES) return vs_fail(ctx, VS_E_RANGE, "vs_node_site_pairs: %u sites, and a site number has 29 bits", n_sites);
    const VsIndexDev &idx = ctx->idx;
    const SitePairsPlan pl = vs_site_pairs_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_site_pairs: %s", pl.msg);
    if (!pl.launch || !n_sites) return VS_OK;  // no end of the block holds an anchor, or there is nothing to observe
    if (!d_first || !d_site_slot || !d_row_first || !d_cells) return VS_E_ARG;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    SitePairsParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.first = d_first;
    P.site_slot = d_site_slot;
    P.row_first = d_row_first;
    P.cells = (unsigned long long *)d_cells;
    P.tally = (unsigned long long *)d_tally;
    P.ends_per_wg = pl.ends_per_wg;
    P.n_sites = n_sites;
    P.max_mismatch = max_mismatch;
    hipLaunchKernelGGL(k_node_site_pairs, dim3(pl.grid), dim3(SITE_PAIRS_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// ---- the pileup kept apart by strand, and its records found on the device (vs_node_pileup_strands / vs_pileup_call) ----------
// k_node_pileup once more with the one thing it throws away kept: the strand `opp` of a credited alignment is its PLANE (0: the
// end lies along the segment's forward text, 1: along its reverse complement; tests/strand_pileup_model.py).  Everything up to
// and including vs_pileup_owner and vs_pileup_count is k_node_pileup's, and so are the workgroup, the LDS and the slots.  The
// difference array is plane-major, diff[2][S]: the +1 and the -1 of an alignment go to plane `opp`, every plane keeps its own
// sentinels (the -1 of an overlap flush with the end of the last segment lands in slot S - 1 of ITS plane), and each plane folds
// by vs_cover_fold on its own.  alt is [S][2][5]: both planes of a slot lie in 80 bytes, one 64-bit atomic per non-agreeing base
// as before.  The fold bound is vs_pileup_plan's, unchanged: one end adds at most len_e to one slot of ONE plane (one diagonal
// per read offset through a position of a strand), below the 2 * len_e the plan's weight assumes -- no second plan.
#include "vs_pileup_call_core.h"

struct PileupStrandsParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *first;     // [n_nodes + 1] the first slot of every segment, the slot total S behind them
    uint32_t *diff;            // [2][S] differences of the depth per plane, ADDED to
    unsigned long long *alt;   // [S][2][PILEUP_ALT] non-agreeing bases per plane, ADDED to
    unsigned long long *tally; // [2] alignments credited, alignments rejected, ADDED to
    uint64_t n_slots;          // S
    uint64_t ends_per_wg;
    uint32_t max_mismatch;
};

__global__ void __launch_bounds__(PILEUP_TPB, 8)  // (as k_node_pileup)
k_node_pileup_strands(PileupStrandsParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[PILEUP_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *s_head = s_mem;
    uint32_t *sw = s_mem + PILEUP_HEAD_WORDS + wave * PILEUP_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u;
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    if (tid == 0u) s_head[0] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                bool credited = false, rejected = false;
                if (t2 < total) {
                    const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                    const uint32_t k2 = t2 - s_cnt[pr];
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                    const uint32_t j = ej & VS_LEN_MASK;
                    const uint64_t e = e0 + (ej >> 24);
                    const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                    const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                    const uint32_t *mk = vs_depth_mask(P.rd, meta);
                    uint32_t nd, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[nd];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    // (k >= 95: VS_SEED_VERIFIED is 0, the key only nominated the posting and the comparison starts at the seed's first base)
                    if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len) &&
                        qa + len <= nm.len) {  // (a match lies inside its strand: no slot beyond the segment's sentinel)
                        const uint64_t tbase = (uint64_t)nm.woff * 16u;
                        const VsPileupSpan sp = vs_pileup_span(rlen, nm.len, a, qa);
                        if (vs_pileup_owner(P.rd.words, rbase, tw, tbase, mk, sp, a, K)) {
                            uint32_t miss = vs_pileup_count(P.rd.words, rbase, tw, tbase, mk, sp);
                            rejected = miss > P.max_mismatch;
                            credited = !rejected;
                            if (credited) {
                                // the overlap on the strand: [t_lo, t_hi); on the forward text: from p_lo on, as many; the plane: opp
                                const uint32_t t_lo = (uint32_t)((int64_t)sp.x_lo + sp.d), t_hi = (uint32_t)((int64_t)sp.x_hi + sp.d);
                                const uint32_t at = P.first[nd] + (opp ? nm.len - t_hi : t_lo);
                                uint32_t *first_slot = P.diff + ((opp ? P.n_slots : 0ull) + at);  // (in the alignment's plane)
                                atomicAdd(first_slot, 1u);
                                atomicAdd(first_slot + (sp.x_hi - sp.x_lo), 0xFFFFFFFFu);  // (at most the segment's sentinel: below S)
                                for (uint32_t x = sp.x_lo; miss && x < sp.x_hi; x += 32u) {
                                    const uint32_t n = sp.x_hi - x < 32u ? sp.x_hi - x : 32u;
                                    uint64_t f = vs_pl_differ(P.rd.words, rbase, tw, tbase, mk, x, sp.d, n);
                                    if (!f) continue;
                                    const uint64_t rwin = vs_pl_win(P.rd.words, rbase + x);
                                    const uint64_t mwin = mk ? vs_pl_win(mk, rbase + x) : 0ull;
                                    while (f) {
                                        const uint32_t bit = (uint32_t)__ffsll((long long)f) - 1u;  // (even: 2 * the base's place in the window)
                                        f &= f - 1ull;
                                        const uint32_t code = (uint32_t)(rwin >> bit) & 3u;
                                        // the read's base as it reads on the forward strand; a byte outside ACGT: `other`
                                        // ... and behind the five columns of plane 0 for an alignment of plane 1
                                        const uint32_t col = ((mwin >> bit) & 3ull) ? (opp ? 4u + PILEUP_ALT : 4u) : (opp ? 3u + PILEUP_ALT - code : code);
                                        const uint32_t ts = t_lo + (x - sp.x_lo) + (bit >> 1);  // strand offset of the base
                                        const uint64_t slot = (uint64_t)P.first[nd] + (opp ? nm.len - 1u - ts : ts);
                                        atomicAdd(&P.alt[slot * (2u * PILEUP_ALT) + col], 1ull);
                                        miss--;
                                    }
                                }
                            }
                        }
                    }
                }
                vs_pileup_tally(P.tally, credited, lane);
                vs_pileup_tally(P.tally + 1, rejected, lane);
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // s_np is rewritten by the next batch
    }
}

extern "C" int vs_node_pileup_strands(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint64_t n_slots, uint32_t *d_diff, uint64_t *d_alt,
                                      uint32_t max_mismatch, uint64_t *d_tally) {
    if (!ctx || !reads || !d_first || !d_diff || !d_alt || !d_tally) return VS_E_ARG;
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_pileup_strands: build an index first (vs_index_build)");
    if (n_slots >= (1ull << 32)) return vs_fail(ctx, VS_E_RANGE, "vs_node_pileup_strands: %llu slots", (unsigned long long)n_slots);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const PileupPlan pl = vs_pileup_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu, 0, 0);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_pileup_strands: %s", pl.msg);
    if (!pl.launch || !n_slots) return VS_OK;  // no end of the block holds an anchor, or no segment has a position
    PileupStrandsParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.first = d_first;
    P.diff = d_diff;
    P.alt = (unsigned long long *)d_alt;
    P.tally = (unsigned long long *)d_tally;
    P.n_slots = n_slots;
    P.ends_per_wg = pl.ends_per_wg;
    P.max_mismatch = max_mismatch;
    hipLaunchKernelGGL(k_node_pileup_strands, dim3(pl.grid), dim3(PILEUP_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// The caller: one lane per slot, twice.  Pass 1 finds the slot's segment by a binary search on `first`, reads the segment's base
// from the index's own forward text, applies the rule of vs_pileup_call_core.h and writes how many records the slot makes (0 to
// 3); vs_scan_u32 gives every slot its place; pass 2 applies the same rule again and writes the records there -- ascending by
// (slot, alt base), of the exact size, and nothing else leaves the device.  A sentinel slot has no base and emits nothing: its
// counts are not read and no text behind the segment's is.
struct PileupCallParams {
    const uint32_t *first;             // [n_nodes + 1] the first slot of every segment, the slot total behind them
    const VsNodeMeta *meta;            // [n_nodes]
    const uint32_t *fwd_words;         // the segments' forward texts
    const unsigned long long *depth;   // [planes][S]
    const unsigned long long *alt;     // [S][planes][PILEUP_ALT]
    uint32_t *count;                   // [S] pass 1: records per slot, written; pass 2: the records before the slot's, read
    unsigned long long *out;           // pass 2: [n][PILEUP_CALL_WORDS]
    uint64_t n_slots;                  // S
    uint64_t min_alt_count, min_alt_strand;
    double min_alt_frac;
    uint32_t n_nodes, planes;
};

// the records of slot i (out: NULL counts them only); 0 for a sentinel slot and for a slot no segment owns
__device__ __forceinline__ uint32_t vs_pileup_call_lane(const PileupCallParams &P, uint64_t i, uint64_t *out) {
    const uint32_t n = vs_upper_idx(P.first, P.n_nodes + 1u, (uint32_t)i);  // first[n] <= i < first[n + 1]: segments without slots are skipped
    if (n >= P.n_nodes) return 0u;
    const VsNodeMeta nm = P.meta[n];
    const uint32_t p = (uint32_t)i - P.first[n];
    if (p >= nm.len) return 0u;  // the sentinel
    const uint32_t ref = (P.fwd_words[nm.woff + (p >> 4)] >> ((p & 15u) * 2u)) & 3u;
    uint64_t depth[2] = {P.depth[i], 0ull}, alt[2][5] = {{0ull, 0ull, 0ull, 0ull, 0ull}, {0ull, 0ull, 0ull, 0ull, 0ull}};
    const unsigned long long *a = P.alt + i * P.planes * PILEUP_ALT;
#pragma unroll
    for (uint32_t c = 0u; c < PILEUP_ALT; c++) alt[0][c] = a[c];
    if (P.planes == 2u) {
        depth[1] = P.depth[P.n_slots + i];
#pragma unroll
        for (uint32_t c = 0u; c < PILEUP_ALT; c++) alt[1][c] = a[PILEUP_ALT + c];
    }
    return vs_pileup_call_slot(ref, depth, alt, P.min_alt_count, P.min_alt_frac, P.min_alt_strand, i, out);
}

__global__ void __launch_bounds__(PILEUP_CALL_TPB)
k_pileup_call_count(PileupCallParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_CALL_TPB + threadIdx.x;
    if (i >= P.n_slots) return;
    P.count[i] = vs_pileup_call_lane(P, i, nullptr);
}

__global__ void __launch_bounds__(PILEUP_CALL_TPB)
k_pileup_call_write(PileupCallParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * PILEUP_CALL_TPB + threadIdx.x;
    if (i >= P.n_slots) return;
    (void)vs_pileup_call_lane(P, i, (uint64_t *)P.out + (uint64_t)P.count[i] * PILEUP_CALL_WORDS);  // (a slot without records writes nothing)
}

extern "C" int vs_pileup_call_host(uint32_t ref, uint32_t planes, const uint64_t *depth, const uint64_t *alt, uint64_t min_alt_count, double min_alt_frac,
                                   uint64_t min_alt_strand, uint64_t out[3][6], uint32_t *n) {
    if (!depth || !alt || !out || !n || ref > 3u || !vs_pileup_call_args_ok(planes, min_alt_frac, min_alt_strand)) return VS_E_ARG;
    uint64_t d[2] = {depth[0], planes == 2u ? depth[1] : 0ull}, a[2][5];
    for (uint32_t c = 0u; c < PILEUP_ALT; c++) {
        a[0][c] = alt[c];
        a[1][c] = planes == 2u ? alt[PILEUP_ALT + c] : 0ull;
    }
    *n = vs_pileup_call_slot(ref, d, a, min_alt_count, min_alt_frac, min_alt_strand, 0ull, &out[0][0]);
    return VS_OK;
}

extern "C" int vs_pileup_call(vs_ctx *ctx, const uint32_t *d_first, uint64_t n_slots, uint32_t planes, const uint64_t *d_depth, const uint64_t *d_alt,
                              uint64_t min_alt_count, double min_alt_frac, uint64_t min_alt_strand, uint64_t *d_out, uint64_t cap, uint64_t *n) {
    if (!ctx || !n || !d_first || (n_slots && (!d_depth || !d_alt)) || (cap && !d_out)) return VS_E_ARG;
    if (!vs_pileup_call_args_ok(planes, min_alt_frac, min_alt_strand))
        return vs_fail(ctx, VS_E_ARG, "vs_pileup_call: one or two planes, a fraction from 0 up, and a strand threshold with two planes only");
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_pileup_call: build an index first (vs_index_build)");
    if (n_slots >= (1ull << 32)) return vs_fail(ctx, VS_E_RANGE, "vs_pileup_call: %llu slots", (unsigned long long)n_slots);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    *n = 0;
    if (!n_slots) {
        VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return VS_OK;
    }
    const VsIndexDev &idx = ctx->idx;
    const uint64_t nb = (n_slots + 2047u) / 2048u;
    VS_HIP(ctx, ctx->d_cover_scan.reserve(sizeof(uint32_t) * n_slots));
    VS_HIP(ctx, ctx->d_cover_tmp.reserve(sizeof(uint64_t) * (nb + 2u)));
    uint64_t *d_tmp = ctx->d_cover_tmp.as<uint64_t>(), *d_total = d_tmp + nb + 1u;
    PileupCallParams P;
    P.first = d_first;
    P.meta = idx.meta;
    P.fwd_words = idx.fwd_words;
    P.depth = (const unsigned long long *)d_depth;
    P.alt = (const unsigned long long *)d_alt;
    P.count = ctx->d_cover_scan.as<uint32_t>();
    P.out = (unsigned long long *)d_out;
    P.n_slots = n_slots;
    P.min_alt_count = min_alt_count;
    P.min_alt_strand = min_alt_strand;
    P.min_alt_frac = min_alt_frac;
    P.n_nodes = idx.n_nodes;
    P.planes = planes;
    const dim3 grid((unsigned)((n_slots + PILEUP_CALL_TPB - 1u) / PILEUP_CALL_TPB));
    hipLaunchKernelGGL(k_pileup_call_count, grid, dim3(PILEUP_CALL_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    if (int rc = vs_scan_u32(ctx, P.count, P.count, n_slots, d_tmp, d_total)) return rc;
    uint64_t total = 0;
    VS_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = total;
    if (total >= (1ull << 32))  // (a place is a 32-bit word of the scan)
        return vs_fail(ctx, VS_E_RANGE, "vs_pileup_call: %llu records, and a record number has 32 bits: raise the thresholds", (unsigned long long)total);
    if (!total || cap < total) return VS_OK;  // nothing to write, or no room: the caller allocates *n records and calls again
    hipLaunchKernelGGL(k_pileup_call_write, grid, dim3(PILEUP_CALL_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VS_OK;
}

// ---- insertions and deletions of a read end against a strand of a segment (vs_node_indels) ---------------------------------
// What the pileup rejects on both diagonals: an end that carries an insertion or a deletion of at most G bases.  The end
// batches, the probe grid, the table probe, the posting deal and vs_extend under the mask are k_node_pileup's, and so are the
// workgroup and the LDS; there is no owner walk, no count and no fold.  The lane that holds a match (a, qa, len) whose left
// neighbour lies inside both texts -- and so does not agree -- looks LEFT of that breakpoint on the shifted diagonals
// (vs_indel_core.h: deletion 1, insertion 1, ... insertion G; K agreeing bases make the flank), and on an event mirrors it to
// the segment's forward text and moves it left as far as it goes.  An event is two uint64: slot << 8 | plane << 7 | kind << 6 |
// (L - 1), and the inserted bases on the forward strand.  Records are claimed per wavefront: one ballot, one atomic on the
// record count by the first lane that has one, as k_contig_mems claims its records; the count goes on beyond the buffer's
// capacity while the stores stop at it.  The four tallies go through vs_pileup_tally into the context's scratch.
#include "vs_indel_core.h"

struct IndelParams {
    VsIndexDev idx;
    VsReadsDev rd;
    const uint32_t *first;      // [n_nodes + 1] the first slot of every segment (vs_pileup_layout)
    unsigned long long *out;    // [cap][2] events
    unsigned long long cap;
    unsigned long long *count;  // events found, stored or not
    unsigned long long *tally;  // [4] matches tested, deletions, insertions, insertions dropped: of this pass
    uint64_t ends_per_wg;
    uint32_t max_len;           // G
};

__global__ void __launch_bounds__(PILEUP_TPB, 8)  // (as k_node_pileup)
k_node_indels(IndelParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[PILEUP_LDS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = P.idx.n_nodes, w = P.idx.w, s = P.idx.s, K = P.idx.K;
    uint32_t *s_head = s_mem;
    uint32_t *sw = s_mem + PILEUP_HEAD_WORDS + wave * PILEUP_WAVE_WORDS;
    uint32_t *s_np = sw, *s_cnt = sw + 65u, *s_pa = sw + 130u, *s_pb = sw + 194u, *s_pj = sw + 258u;
    const uint64_t e_lo = (uint64_t)blockIdx.x * P.ends_per_wg;
    const uint64_t e_hi = e_lo + P.ends_per_wg < P.rd.n_ends ? e_lo + P.ends_per_wg : P.rd.n_ends;
    if (tid == 0u) s_head[0] = 0u;
    __syncthreads();
    for (;;) {
        uint32_t b = 0u;
        if (lane == 0u) b = atomicAdd(&s_head[0], 64u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (e_lo + b >= e_hi) break;
        const uint64_t e0 = e_lo + b;
        const uint32_t n_here = e_hi - e0 < 64u ? (uint32_t)(e_hi - e0) : 64u;
        uint32_t np = 0u;
        if (lane < n_here) {
            const uint32_t meta = P.rd.meta[e0 + lane];
            if (!((meta >> 24) & VS_FLAG_ABSENT)) np = vs_seed_probes(meta & VS_LEN_MASK, w, s);  // (0 for an end shorter than K)
        }
        s_np[lane + 1u] = vs_wave_scan_add(np);
        if (lane == 0u) s_np[0] = 0u;
        vs_wave_sync();
        const uint32_t tp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_np[64]);
        for (uint32_t p0 = 0u; p0 < tp; p0 += 64u) {
            // probes p0 .. p0 + 63 of the batch: one per lane
            const uint32_t t = p0 + lane;
            uint32_t c = 0u, pa = 0u, pb = 0u, pj = 0u;
            if (t < tp) {
                const uint32_t el = vs_upper_idx(s_np, 65u, t);  // the end that owns probe t: s_np[el] <= t < s_np[el + 1]
                const uint64_t e = e0 + el;
                const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                const uint32_t j = vs_seed_phase(rlen, w, s) + (t - s_np[el]) * s;
                const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                const uint32_t *mk = vs_depth_mask(P.rd, meta);
                if (!(mk && vs_seed_dirty(mk, rbase + j, w))) {
                    uint32_t sr;
                    const uint64_t key = vs_seed_key(P.rd.words, rbase + j, w, &sr);
                    c = vs_probe(P.idx, key, sr, &pa, &pb);
                }
                pj = (el << 24) | j;  // (a read offset fits 24 bits: VS_LEN_MASK)
            }
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_pj[lane] = pj;
            s_cnt[lane + 1u] = vs_wave_scan_add(c);
            if (lane == 0u) s_cnt[0] = 0u;
            vs_wave_sync();
            const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[64]);
            for (uint32_t q0 = 0u; q0 < total; q0 += 64u) {
                // postings q0 .. q0 + 63 of these probes: one per lane
                const uint32_t t2 = q0 + lane;
                bool tested = false, dropped = false, found = false;
                uint32_t kind = 0u;
                unsigned long long w0 = 0ull, w1 = 0ull;
                if (t2 < total) {
                    const uint32_t pr = vs_upper_idx(s_cnt, 65u, t2);
                    const uint32_t k2 = t2 - s_cnt[pr];
                    const uint32_t qa0 = s_pa[pr], qb0 = s_pb[pr], ej = s_pj[pr];
                    const uint32_t j = ej & VS_LEN_MASK;
                    const uint64_t e = e0 + (ej >> 24);
                    const uint32_t meta = P.rd.meta[e], rlen = meta & VS_LEN_MASK;
                    const uint64_t rbase = (uint64_t)P.rd.woff[e] * 16u;
                    const uint32_t *mk = vs_depth_mask(P.rd, meta);
                    uint32_t nd, pos, opp;
                    VsNodeMeta nm;
                    if (s_cnt[pr + 1u] - s_cnt[pr] == 1u) {
                        nd = qa0; pos = qb0 & 0x7FFFFFFFu; opp = qb0 >> 31;
                        nm = P.idx.meta[nd];
                    } else {
                        const VsPosting po = vs_posting_unpack(P.idx.postings[qa0 + k2]);
                        nd = po.node; pos = po.pos; opp = po.strand ^ (qb0 >> 31);
                        nm.woff = po.woff; nm.len = po.len;
                    }
                    const uint32_t *tw = opp ? P.idx.rc_words : P.idx.fwd_words;
                    const uint32_t q = opp ? nm.len - pos - w : pos;
                    uint32_t a, qa, len;
                    // (k >= 95: VS_SEED_VERIFIED is 0, the key only nominated the posting and the comparison starts at the seed's first base)
                    if (nd < N && vs_extend(P.rd.words, rbase, rlen, tw, nm.woff * 16u, nm.len, j, q, VS_SEED_VERIFIED(w), s, K, mk, rbase, &a, &qa, &len) &&
                        qa + len <= nm.len && a > 0u && qa > 0u) {  // (the pileup's guard; a left neighbour inside both texts)
                        const uint64_t tbase = (uint64_t)nm.woff * 16u;
                        uint32_t L = 0u;
                        tested = true;
                        const uint32_t st = vs_indel_find(P.rd.words, rbase, tw, tbase, mk, a, qa, K, P.max_len, &kind, &L);
                        dropped = st == VS_INDEL_DROPPED;
                        if (st == VS_INDEL_EVENT) {
                            uint32_t u;
                            uint64_t ins;
                            // (an insertion has a >= L + K: the window starts inside the read)
                            vs_indel_normalise(P.idx.fwd_words, tbase, nm.len, opp, kind, L, qa, kind == VS_INDEL_INS ? vs_pl_win(P.rd.words, rbase + a - L) : 0ull,
                                               &u, &ins);
                            found = true;
                            w0 = ((unsigned long long)(P.first[nd] + u) << 8) | (unsigned long long)((opp << 7) | (kind << 6) | (L - 1u));
                            w1 = ins;
                        }
                    }
                }
                const unsigned long long have = __ballot(found);
                if (have) {
                    const uint32_t leader = (uint32_t)__ffsll((long long)have) - 1u;
                    unsigned long long base = 0ull;
                    if (lane == leader) base = atomicAdd(P.count, (unsigned long long)__popcll(have));
                    const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)leader), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)leader);
                    const unsigned long long at = (((unsigned long long)b_hi << 32) | b_lo) + (unsigned long long)__popcll(have & ((1ull << lane) - 1ull));
                    if (found && at < P.cap) {
                        P.out[2ull * at] = w0;
                        P.out[2ull * at + 1ull] = w1;
                    }
                }
                vs_pileup_tally(P.tally, tested, lane);
                vs_pileup_tally(P.tally + 1, found && kind == VS_INDEL_DEL, lane);
                vs_pileup_tally(P.tally + 2, found && kind == VS_INDEL_INS, lane);
                vs_pileup_tally(P.tally + 3, dropped, lane);
            }
            vs_wave_sync();  // s_cnt / s_pa / s_pb / s_pj are rewritten by the next 64 probes
        }
        vs_wave_sync();  // s_np is rewritten by the next batch
    }
}

__global__ void __launch_bounds__(64)
k_indel_tally_add(const unsigned long long *pass, unsigned long long *total) {
    if (threadIdx.x < 4u) total[threadIdx.x] += pass[threadIdx.x];
}

extern "C" int vs_indel_scan_host(const uint32_t *read_words, const uint32_t *read_mask, const uint32_t *strand_words, const uint32_t *fwd_words, uint32_t rlen,
                                  uint32_t tlen, uint32_t strand, uint32_t a, uint32_t qa, uint32_t K, uint32_t G, uint64_t out[4]) {
    if (!read_words || !strand_words || !fwd_words || !out || !K || G < 1u || G > VS_INDEL_MAX_LEN || strand > 1u || a >= rlen || qa >= tlen) return VS_E_ARG;
    out[0] = VS_INDEL_UNTESTED;
    out[1] = out[2] = out[3] = 0;
    if (!a || !qa) return VS_OK;
    uint32_t kind = 0u, L = 0u;
    const uint32_t st = vs_indel_find(read_words, 0u, strand_words, 0u, read_mask, a, qa, K, G, &kind, &L);
    out[0] = st;
    if (st == VS_INDEL_NONE) return VS_OK;
    out[1] = ((uint64_t)kind << 8) | L;
    if (st == VS_INDEL_EVENT) {
        uint32_t u;
        vs_indel_normalise(fwd_words, 0u, tlen, strand, kind, L, qa, kind == VS_INDEL_INS ? vs_pl_win(read_words, a - L) : 0ull, &u, &out[3]);
        out[2] = u;
    }
    return VS_OK;
}

extern "C" int vs_node_indels(vs_ctx *ctx, const vs_reads *reads, const uint32_t *d_first, uint32_t max_len, uint64_t *d_events, uint64_t cap, uint64_t *n,
                              uint64_t *d_tally) {
    if (!ctx || !reads || !d_first || !n || !d_tally || (cap && !d_events)) return VS_E_ARG;
    if (max_len < 1u || max_len > VS_INDEL_MAX_LEN) return vs_fail(ctx, VS_E_ARG, "vs_node_indels: a maximum length of %u: 1 to %u are possible", max_len, VS_INDEL_MAX_LEN);
    if (!ctx->has_index) return vs_fail(ctx, VS_E_STATE, "vs_node_indels: build an index first (vs_index_build)");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    const VsIndexDev &idx = ctx->idx;
    const PileupPlan pl = vs_pileup_plan_for(idx.n_nodes, idx.K, reads->n_ends, (uint32_t)reads->max_len, (uint32_t)ctx->n_cu, 0, 0);
    if (pl.status != VS_OK) return vs_fail(ctx, pl.status, "vs_node_indels: %s", pl.msg);
    *n = 0;
    if (!pl.launch) {  // no end of the block holds an anchor
        VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return VS_OK;
    }
    VS_HIP(ctx, ctx->d_indel_tmp.reserve(sizeof(uint64_t) * 5u));  // the record count and the pass's four tallies
    unsigned long long *d_tmp = ctx->d_indel_tmp.as<unsigned long long>();
    VS_HIP(ctx, hipMemsetAsync(d_tmp, 0, sizeof(uint64_t) * 5u, ctx->stream));
    IndelParams P;
    P.idx = idx;
    P.rd = reads->dev();
    P.first = d_first;
    P.out = (unsigned long long *)d_events;
    P.cap = cap;
    P.count = d_tmp;
    P.tally = d_tmp + 1;
    P.ends_per_wg = pl.ends_per_wg;
    P.max_len = max_len;
    hipLaunchKernelGGL(k_node_indels, dim3(pl.grid), dim3(PILEUP_TPB), 0, ctx->stream, P);
    VS_HIP(ctx, hipGetLastError());
    uint64_t found = 0;
    VS_HIP(ctx, hipMemcpyAsync(&found, d_tmp, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = found;
    if (found > cap) return VS_OK;  // the pass did not fit: its tallies are not added, the caller calls again with room
    hipLaunchKernelGGL(k_indel_tally_add, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long *)(d_tmp + 1), (unsigned long long *)d_tally);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}
