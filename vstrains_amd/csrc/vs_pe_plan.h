// The launch plan of one PE count (vs_pe_count / vs_pe_count_tracked / vs_pe_map_ends): every decision vs_pe.hip takes
// before its first launch -- tile shape, k_pe_tiles instantiation, locus order, counter path, grids, scratch sizes -- as
// ONE pure function of scalars.  Plain C++: a host compiler takes this header as it is (oracle/plan_check.cpp,
// tests/test_pe_plan_cpu.py), hipcc takes it for the kernels, which read their compile-time constants from here.
// The launch rule lives here and nowhere else.
#ifndef VS_PE_PLAN_H
#define VS_PE_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/vstrains_hip.h"

#if defined(__HIPCC__)
#define VS_PLAN_FN __host__ __device__ inline
#else
#define VS_PLAN_FN inline
#endif

// Test hooks of vs_pe_count.  A production context never reads the environment: the switches exist only when the process
// was started with VS_EXPERIMENT=1 (any other value is production), and are then re-read on every call so that a test can
// flip them on a live context.  A switch is kept only if a test uses it and it forces a path that a production context
// takes on some input (often one that only full-size blocks or large graphs reach), or the reference path of a test.
// Every one of them gives the production counters.  Defaults = what a production context does.
struct VsTuning {
    uint32_t ept = 0;               // VS_EPT (0 = automatic)
    uint32_t grid_per_cu = 128;     // VS_GRID_PER_CU: longer runs of tiles per workgroup, as a full-size block has
    int acc_fill_pct = -1;          // VS_ACC_FILL (-1 = 1/16 of the slots): cell-table write-outs on fill
    uint32_t acc_tasks = 0;         // VS_ACC_TASKS (0 = ACC_TASK_PLAN_CAP): task entries per wavefront of k_pe_accumulate, so that small blocks reach the batch cut
    int shortcut = -1;              // VS_SHORTCUT (-1 = by index statistics)
    int adapt_grid = -1;            // VS_ADAPT_GRID (-1 = by index statistics): the adaptive step grid of the compile-time-shape kernels
    int acc_rows = -1;              // VS_ACC_ROWS (-1 = by graph size): counters summed by row owners (k_rows_sum) instead of pair-major (k_pe_accumulate)
    int ltab_bits = -1;             // VS_LTAB_BITS: log2 slots of the block's list table (-1 = by block size, 0 = no table: every end stands for itself)
    uint32_t rows_keys = 0, rows_sub = 0;  // VS_ROWS_KEYS / VS_ROWS_SUB: rows per histogram pass, pairs per transposition (0 = the constants; tests shrink them)
    uint32_t rows_per_strip = 0;    // VS_ROWS_PER_STRIP (0 = automatic): matrix rows one workgroup of k_rows_sum owns at a time
    bool no_sort = false, locus_global = false, no_fast = false, no_std = false, no_agg = false;
    bool no_mid = false;            // VS_NO_MID: overflow pairs straight to k_pe_slow
    int locus_stage = -1;           // VS_LOCUS_STAGE (-1 = by the room the histogram leaves): 0 = the key pass of the locus sort with per-pair loads, N = staged through buffers of N words per wavefront, so that small blocks reach batch cuts and oversize pairs
    int locus_scatter = 0;          // VS_LOCUS_SCATTER (0 = LOCUS_SCATTER_PAIRS): k_locus_scatter in launches of about N pairs' worth of keys each, so that blocks of a few thousand pairs are placed in several launches
};

// The probe grid of a read end (round 5).  A match of K bases and more holds s = K - w + 1 consecutive seed starts, so any
// grid phi, phi + s, phi + 2s, ... of read offsets finds it, and the first grid point inside it credits it (left extension
// below s: vs_extend / k_pe_tiles).  phi = 0 spends a probe on the read's last, partly covered stride: floor((len - w) / s) + 1
// probes.  With r = (len - w) mod s every phi in (r, s) needs one probe less -- floor((len - w + 1) / s), the fewest any
// exact grid of stride s can have (the len - K + 1 windows of a read in runs of s) -- and the grid's seeds then lie
// inside the read instead of flush with its first base.  phi = (r + s) / 2 is the middle of that range (and s - 1, the
// only choice, when r = s - 1).  Measured on the configs[2] stream: 21.9 instead of 27.4 postings per end, four probes
// instead of five (profiles/r5/phase_gate_config2.json).  Ends shorter than K are never probed (PE_Inference.py:160-163).
VS_PLAN_FN uint32_t vs_seed_phase(uint32_t len, uint32_t w, uint32_t s) {
    return len < w ? 0u : ((len - w) % s + s) / 2u;
}
VS_PLAN_FN uint32_t vs_seed_probes(uint32_t len, uint32_t w, uint32_t s) {
    if (len < w) return 0u;
    return (len - w + 1u) / s;  // (0 for an end shorter than K = w + s - 1: it has no (k+1)-window, PE_Inference.py:23, and is never probed)
}
// bases of the seed the comparison may take for granted: all of them for exact keys, none for mixed ones (vs_seed_key)
#define VS_SEED_VERIFIED(w) ((w) <= 31u ? (w) : 0u)

// ---- sizes the plan shares with the kernels of vs_pe.hip (described there, where they are used) --------------------
#define LC 16u               // list words a tile's region of the hand-off buffer holds per end on average
#define PPT 2u               // postings per thread and expansion chunk
#define TTPB 256             // threads per k_pe_tiles workgroup (a tile holds TTPB / 4 read ends)
#define PPT_LONG 1u          // the same for the long-window instantiations (MODE 2, k = 127)
#define CHUNK (TTPB * PPT)   // (the owner array of a tile is sized for the larger of the two)
#define ACC_TPB 1024
#define ACC_BITS 14
#define ACC_SLOTS (1u << ACC_BITS)
#define ACC_PPW 64u          // pairs per wavefront and round of k_pe_accumulate: one per lane
#define ACC_TASK_WORDS 480u  // LDS words of a wavefront's task region (vs_acc_tasks.h): what the cell table leaves of 160 KB of LDS
#define ACC_TASK_CAP (2u * ACC_TASK_WORDS)  // ... and the 16-bit task entries they hold
#define ACC_TASK_MIN 40u     // tasks of the largest pair (two lists of 20 nodes): the smallest task region there may be
#define ACC_QUEUE 64u        // keys a wavefront collects before it claims their cells, one per lane: the last words of its task region
#define ACC_TASK_PLAN_CAP (ACC_TASK_CAP - 2u * ACC_QUEUE)  // ... so 832 task entries are the most the plan hands the kernel
#define ACC_BINS 24u         // counters per wavefront of the counting sort of a batch's tasks (turns 1 .. 22)
#define ROWS_KEYS 65536u   // rows per histogram pass (larger graphs take several passes over the lists)
#define ROWS_SUB ((1u << 26) - 1024u)  // pairs per transposition (an entry names a read end in 27 bits, its list's length in five; row offsets are 32-bit)
#define RS_BITS 13
#define RS_SLOTS (1u << RS_BITS)
#define LOCUS_LDS_KEYS 36864u  // 144 KB of LDS counters
#define LOCUS_LDS_MAX_PASSES 4u  // ... per pass; graphs of up to 147 k nodes are sorted through LDS histograms
#define LOCUS_WGS 256u     // one per CU (measured: 1024 x 256 threads 0.70 ms, 256 x 1024 threads 0.57 ms)
// The staged key pass (k_locus_count_staged): a wavefront copies the packed words of a batch of pairs into one of its two LDS buffers
#define LOCUS_STAGE_WAVES 16u     // wavefronts of the workgroup, each with buffers of its own
#define LOCUS_STAGE_PAIRS 64u     // pairs a batch holds at most: one per lane
#define LOCUS_STAGE_QUADS 5u      // 16-byte loads a lane has in flight for the next batch
#define LOCUS_STAGE_SLACK 16u     // words of a buffer beyond its capacity: up to 3 in front (the copy starts 16-byte aligned), 4 behind (window reads overshoot an end by up to two words), rounding
#define LOCUS_STAGE_MAX (LOCUS_STAGE_QUADS * 4u * LOCUS_STAGE_PAIRS - LOCUS_STAGE_SLACK)  // what the lanes' loads cover
#define LOCUS_STAGE_MIN_PAIRS 48u  // production stages only where a buffer holds this many pairs of the block's longest reads: three lanes in four with a pair (measured: 55 pairs a batch, 2 x 150 bases, win; 34 pairs, 2 x 250 bases, lose to the per-pair loads -- profiles/EXPERIMENTS.md)
#define LOCUS_LDS_WORDS 40960u    // 160 KB, one workgroup per CU
// k_locus_scatter writes 4 bytes a pair to places all over perm[]: a launch that places every pair of a large block leaves a
// line of perm[] in pieces, each piece evicted from an L2 before the next arrives (230 MB written for 40 MB at 10 M pairs).
// The launch rule therefore cuts the keys of a pass into ranges of about LOCUS_SCATTER_PAIRS pairs' worth, one launch each
// (the kernel's key_lo / nk filter; a launch reads all the keys, 4 bytes a pair, coalesced), at most LOCUS_SCATTER_MAX of
// them (measured at 10 M pairs: two and four launches win alike, eight lose to the launches -- profiles/EXPERIMENTS.md).
#define LOCUS_SCATTER_PAIRS 2621440u  // 2.5 Mi pairs, 10 MB of perm[]
#define LOCUS_SCATTER_MAX 4u
#define SLOW_WORDS_PER_NODE 6u
#define LDS_BUDGET_BYTES (64u * 1024u)
#define NI_CAP 4096u

// ---- the batch cut of the staged key pass ------------------------------------------------------------------------------
// woff is the block's prefix array of word offsets (two ends per pair, n_ends + 1 entries), so the words of pairs
// [p0, p0 + n) are the stretch woff[2 p0] .. woff[2 (p0 + n)].  A batch that starts at pair p0 of a chunk that ends at hi
// is the longest prefix of [p0, hi) whose stretch fits `cap` words, at most LOCUS_STAGE_PAIRS pairs.  woff is monotone, so
// "pair p0 + i is in the batch" is a prefix property of i and every lane of the wavefront decides it for its own pair:
// the kernel counts the lanes that say yes, vs_locus_batch below is the same count taken in turn.
VS_PLAN_FN bool vs_locus_in_batch(bool exists, uint32_t w_first, uint32_t w_pair_end, uint32_t cap) {
    return exists && w_pair_end - w_first <= cap;  // (exists: i < LOCUS_STAGE_PAIRS and p0 + i < hi)
}
struct LocusBatch {
    uint32_t n;       // pairs: at least one while p0 < hi
    uint32_t staged;  // 0: one pair whose own two ends do not fit the buffer -- keyed by per-pair loads, alone
};
VS_PLAN_FN LocusBatch vs_locus_batch(const uint32_t *woff, uint64_t p0, uint64_t hi, uint32_t cap) {
    LocusBatch b = {0u, 1u};
    if (p0 >= hi) return b;  // (an empty chunk, or its end)
    const uint32_t w_first = woff[2u * p0];
    while (b.n < LOCUS_STAGE_PAIRS && vs_locus_in_batch(p0 + b.n < hi, w_first, p0 + b.n < hi ? woff[2u * (p0 + b.n) + 2u] : 0u, cap)) b.n++;
    if (!b.n) { b.n = 1u; b.staged = 0u; }
    return b;
}
// What of `words` a staged batch copies: whole 16-byte quads from the aligned word at or below its first word to four
// words behind its last (a window read at a seed overshoots its end by up to two words; the words behind the block's last
// are the zero pad, VS_PAD_WORDS).  Word x of the block is word x - first of the buffer.
struct LocusSpan {
    uint32_t first, quads;
};
VS_PLAN_FN LocusSpan vs_locus_span(uint32_t w_first, uint32_t w_end) {
    LocusSpan sp;
    sp.first = w_first & ~3u;
    sp.quads = (w_end + 4u - sp.first + 3u) / 4u;  // <= (cap + 10) / 4 <= (buffer words) / 4
    return sp;
}
VS_PLAN_FN uint32_t vs_locus_buf_words(uint32_t cap) { return ((cap + 3u) & ~3u) + LOCUS_STAGE_SLACK; }

// LDS carve shared by the kernel and the host-side size computation
struct TileLayout {
    uint32_t woff, gend, meta, inv, words, pcnt, pa, pb, hkey, hcnt, hminp, hminj, ns, state, list, owner, misc, total;
};
VS_PLAN_FN TileLayout tile_layout(uint32_t ept, uint32_t pmax, uint32_t words_cap, uint32_t pool, uint32_t list_trim = 0u) {
    TileLayout t;
    uint32_t o = 0;
    const uint32_t NI = ept * pmax;
    // headers and packed words exist twice: the next tile's are brought in while this one is worked on
    t.woff = o;  o += 2u * ((ept + 2u) & ~1u);  // global word offset of every end of the tile
    t.gend = o;  o += 2u * ept;                 // global end index
    t.meta = o;  o += 2u * ept;
    t.inv = o;   o += ept;                      // positions of bytes outside ACGT (straight-line kernels; current tile only)
    t.words = o; o += 2u * (words_cap + 8u);
    t.pcnt = o;  o += NI + 1u;  // [0] stays zero: the scan is read as s_pcnt[it - 1] .. s_pcnt[it] without a test for it == 0
    t.pa = o;    o += NI;
    t.pb = o;    o += NI;
    t.hkey = o;  o += pool;
    t.hcnt = o;  o += pool;
    t.hminp = o; o += pool;
    t.hminj = o; o += pool;
    t.ns = o;    o += ept;
    t.state = o; o += ept;
    // the posting owners of P3 and the accepted lists of P4/P5 are never live together
    t.list = o;
    t.owner = o; o += (ept * LC - list_trim > CHUNK ? ept * LC - list_trim : CHUNK);
    t.misc = o;  o += 16u;
    t.total = o;
    return t;
}

// SW, SP != 0: the tile shape is a compile-time one for k = 55 -- 64 ends per tile, 1024-slot table,
// SW packed words and SP probes per end (vs_seed_probes): (10, 4) = 2 x 145..159 bases, (8, 3) = 2 x 113..128, (7, 3) = 2 x 108..112,
// (7, 2) = 2 x 97..107.  Every LDS array then sits at a constant offset (folded into the LDS
// instructions) instead of costing a scalar register and an add, the divisions by pmax / wpe and
// k+1 / seed length / stride become constants.  The plan picks one when the block has that shape.
#define STD_EPT (TTPB / 4u)
#define STD_POOL_BITS 10u  // pool_for(STD_EPT)
#define STD_K 56u   // k + 1
#define STD_W 31u   // seed length and probe stride that follow from it (seed_geometry)
#define STD_S 26u
#define STD2_EPT 60u  // the k = 127 shape (MODE 2): ends per tile (what the LDS budget below gives that shape), pool_for(60) = 1024 slots, k + 1, seed length, stride
#define STD2_POOL_BITS 10u
#define STD2_K 128u
#define STD2_W 63u
#define STD2_S 66u
// The compile-time shapes, as (MODE, SW, SP); each exists with and without the adaptive step grid (AD).
struct StdShape {
    uint32_t mode, sw, sp;
};
constexpr StdShape VS_STD_SHAPES[] = {{1u, 10u, 4u}, {1u, 8u, 3u}, {1u, 7u, 2u}, {1u, 7u, 3u}, {2u, 16u, 2u}};
// Table slots and list trim of an instantiation.  (The 768-slot table is for graphs whose ends touch few nodes: the
// adaptive instantiations -- many postings per seed, long lists -- keep 1 024 slots and five wavefronts per SIMD;
// k = 127: 16 words per end of read text leave less for the lists.)  Without a compile-time shape the pool is a run-time value.
struct StdTable {
    uint32_t pool, trim;
};
VS_PLAN_FN constexpr StdTable vs_std_table(int mode, bool std_shape, bool ad) {
    return std_shape && !ad ? StdTable{768u, mode == 2 ? 192u : 64u} : StdTable{1u << (mode == 2 ? STD2_POOL_BITS : STD_POOL_BITS), 0u};
}

// workgroups of the overflow kernel: as many as 4 GB of dense per-workgroup node state allow, 64 .. 2048
inline uint32_t slow_grid_for(uint32_t n_nodes) {
    const uint64_t per_wg = sizeof(uint32_t) * (uint64_t)SLOW_WORDS_PER_NODE * (n_nodes ? n_nodes : 1u);
    uint64_t g = (4ull << 30) / per_wg;
    return (uint32_t)(g < 64u ? 64u : g > 2048u ? 2048u : g);
}

inline uint32_t pool_for(uint32_t ept, uint32_t *bits) {
    uint32_t b = 6;
    while ((1u << b) < 16u * ept) b++;
    *bits = b;
    return 1u << b;
}

inline size_t lds_bytes(uint32_t ept, uint32_t pmax, uint32_t words_cap) {
    uint32_t bits;
    uint32_t pool = pool_for(ept, &bits);
    return (size_t)tile_layout(ept, pmax, words_cap, pool).total * sizeof(uint32_t);
}

struct PePlanIn {
    uint32_t n_nodes = 0, K = 0, w = 0, s = 0;                 // the index
    uint64_t n_seed_pos = 0, n_distinct = 0;                   // ... its seed statistics
    uint32_t max_node_len = 0, n_cu = 0;
    uint64_t n_ends = 0;                                       // the block of reads
    uint32_t max_len = 0;
    bool has_mask = false, has_inv4 = false;
    bool count = false, tile_map = false;                      // the call: counters (else only the per-end lists), with a tile map
    VsTuning tune;
};

struct PePlan {
    int status;  // VS_OK, or VS_E_RANGE with msg; every other field is zero then
    char msg[128];
    // the tile of k_pe_tiles
    uint32_t ept, pmax, wpe, pool, pool_bits, words_cap, magic_pmax, magic_wpe;
    uint64_t lds_bytes;
    uint32_t mode, sw, sp, ad;  // the instantiation k_pe_tiles<mode, sw, sp, ad>
    uint64_t n_tiles, grid, list_ends, list_words;
    uint32_t tiles_per_wg, shortcut, mid_fast;
    // locus order: through LDS histograms (keys per pass, pairs per workgroup) or global atomics
    uint32_t use_sort, lds_sort, locus_chunk, locus_per_pass;
    uint64_t locus_keys, locus_hist_words;
    uint32_t locus_stage_words;  // capacity of each of a wavefront's two LDS buffers in the staged key pass (0: per-pair loads)
    uint64_t locus_lds_bytes;    // dynamic LDS of k_locus_count / k_locus_count_staged
    uint32_t locus_scatter_keys; // keys a launch of k_locus_scatter places (locus_per_pass at most)
    // the counters: pair-major (k_pe_accumulate) or by row owners (pe_count_by_rows)
    uint32_t use_rows, use_table, mark_tiles;
    uint32_t acc_grid, acc_per_wg, acc_fill, acc_task_cap;
    uint64_t rows_sub_pairs;  // pairs per transposition
    uint32_t rows_ltab_bits, rows_keys, rows_fill, rows_per_strip;
    // the overflow kernel
    uint32_t slow_grid;
    uint64_t dense_bytes;
};

inline PePlan vs_pe_plan(const PePlanIn &in) {
    PePlan p = {};
    const VsTuning &tn = in.tune;
    const uint64_t n_pairs = in.n_ends / 2;
    if (n_pairs == 0) return p;  // nothing is launched
    const uint32_t maxlen = in.max_len, N = in.n_nodes;
    if (N > 0x01FFFFFEu) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "more than 2^25-2 nodes");
        return p;
    }
    const uint32_t wpe = maxlen ? (maxlen + 15u) / 16u : 1u;
    // probes of the longest end (vs_seed_probes grows with the length): the probe slots a tile reserves per end
    uint32_t pmax = vs_seed_probes(maxlen, in.w, in.s);
    if (!pmax) pmax = 1u;
    uint32_t ept = tn.ept ? tn.ept : STD_EPT;
    if (ept < 2 || ept > TTPB / 2u) ept = STD_EPT;
    while (ept > 2 && (ept * pmax > NI_CAP || lds_bytes(ept, pmax, ept * wpe) > LDS_BUDGET_BYTES)) ept -= 2;
    // (LDS is handed out in 1280-byte pieces: 32 000 B per workgroup lets five share a CU, 40 000 four.  A tile of
    // at least 32 ends that fits one of these is taken over a larger one that wastes the rest.)
    if (!tn.ept) {
        for (size_t fit : {(size_t)32000, (size_t)40000}) {
            uint32_t e2 = ept;
            while (e2 > STD_EPT / 2u && lds_bytes(e2, pmax, e2 * wpe) > fit) e2 -= 2;
            if (lds_bytes(e2, pmax, e2 * wpe) <= fit) { ept = e2; break; }
        }
    }
    size_t lds = lds_bytes(ept, pmax, ept * wpe);
    if (lds > 160u * 1024u) {
        p.status = VS_E_RANGE;
        snprintf(p.msg, sizeof p.msg, "reads of %u bases with k+1=%u need %zu B of LDS per pair (limit 160 KiB)", maxlen, in.K, lds);
        return p;
    }
    p.ept = ept;
    p.pmax = pmax;
    p.wpe = wpe;
    p.words_cap = ept * wpe;
    p.pool = pool_for(ept, &p.pool_bits);
    p.magic_pmax = pmax > 1u ? (uint32_t)(0x100000000ull / pmax) + 1u : 0u;
    p.magic_wpe = wpe > 1u ? (uint32_t)(0x100000000ull / wpe) + 1u : 0u;
    p.slow_grid = slow_grid_for(N);
    p.dense_bytes = sizeof(uint32_t) * (uint64_t)SLOW_WORDS_PER_NODE * (N ? N : 1) * p.slow_grid;

    // locus order of the pairs (see k_pe_locus); VS_NO_SORT=1 keeps the input order
    p.use_sort = !tn.no_sort && n_pairs >= 4096 && n_pairs < 0xFFFFFFF0ull;
    if (p.use_sort) {
        const uint64_t nk = (uint64_t)N + 2u;
        const bool fits_lds = nk <= LOCUS_LDS_MAX_PASSES * LOCUS_LDS_KEYS;
        p.locus_keys = nk;
        p.locus_hist_words = fits_lds ? nk * LOCUS_WGS : nk;
        p.lds_sort = fits_lds && !tn.locus_global;
        if (p.lds_sort) {
            p.locus_chunk = (uint32_t)((n_pairs + LOCUS_WGS - 1) / LOCUS_WGS);
            p.locus_per_pass = (uint32_t)(nk < LOCUS_LDS_KEYS ? nk : LOCUS_LDS_KEYS);
            p.locus_lds_bytes = sizeof(uint32_t) * (uint64_t)p.locus_per_pass;
            const uint64_t sc_pairs = tn.locus_scatter > 0 ? (uint64_t)tn.locus_scatter : LOCUS_SCATTER_PAIRS;
            uint64_t launches = (n_pairs + sc_pairs - 1u) / sc_pairs;
            if (launches > LOCUS_SCATTER_MAX) launches = LOCUS_SCATTER_MAX;
            const uint64_t sc_keys = (nk + launches - 1u) / launches;  // (keys are not pairs: a range of keys holds its share of the pairs only about)
            p.locus_scatter_keys = sc_keys < p.locus_per_pass ? (uint32_t)sc_keys : p.locus_per_pass;
            // the key pass streams the read words through two LDS buffers per wavefront (k_locus_count_staged) where one pass's
            // histogram leaves room for them beside it: not beside a full pass of LOCUS_LDS_KEYS keys, so not in a multi-pass sort
            if (nk < LOCUS_LDS_KEYS && tn.locus_stage != 0) {
                const uint32_t hist = ((uint32_t)nk + 3u) & ~3u;
                uint32_t room = ((LOCUS_LDS_WORDS - hist) / (2u * LOCUS_STAGE_WAVES) - LOCUS_STAGE_SLACK) & ~3u;
                if (room > LOCUS_STAGE_MAX) room = LOCUS_STAGE_MAX;
                uint32_t cap = room / (2u * wpe) >= LOCUS_STAGE_MIN_PAIRS ? room : 0u;
                if (tn.locus_stage > 0) cap = (uint32_t)tn.locus_stage < room ? (uint32_t)tn.locus_stage : room;
                if (cap) {
                    p.locus_stage_words = cap;
                    p.locus_lds_bytes = sizeof(uint32_t) * (uint64_t)(hist + 2u * LOCUS_STAGE_WAVES * vs_locus_buf_words(cap));
                }
            }
        }
    }

    // which counter kernels follow decides the layout of the hand-off: pair-major with one cell table while 2*N*N fits its
    // 32-bit keys (packed lists), by row owners above (rows of LCAP words); VS_ACC_ROWS=0 / 1 overrides (0 beyond 46 340
    // nodes: no table, every increment a global atomic).  VS_NO_AGG=1 turns the summing in LDS off
    p.use_table = tn.no_agg ? 0u : 1u;
    const bool fits32 = 2ull * N * N < 0xFFFFFFFFull;
    bool use_rows = tn.acc_rows >= 0 ? tn.acc_rows != 0 : !fits32;
    if (N == 0 || !p.use_table) use_rows = false;
    if (!use_rows && !fits32) p.use_table = 0u;
    p.use_rows = use_rows;
    // per-end lists handed from k_pe_tiles to the counter kernels
    p.n_tiles = (n_pairs + ept / 2 - 1) / (ept / 2);
    p.list_ends = p.n_tiles * ept;
    p.list_words = p.list_ends * (use_rows ? LC + 4u : LC) + 16u;  // (either layout of the hand-off)

    // The shortcut spares a single posting its extension when the previous probe already owns the
    // match; it pays on graphs whose seeds are mostly unique.  Where seeds repeat (a compacted de
    // Bruijn graph of many strains: 3.5 postings per distinct seed at configs[2]) nearly every
    // wavefront holds some single posting and all 64 lanes walk through the test for it: 6.0 ms with,
    // 5.8 ms without.  VS_SHORTCUT=0/1 overrides.
    p.shortcut = in.n_distinct && in.n_seed_pos < 2 * in.n_distinct ? 1u : 0u;
    if (tn.shortcut >= 0) p.shortcut = (uint32_t)tn.shortcut;
    // (63-base seeds have MIXED keys: equal keys do not prove equal seeds, so "the bases in between match too" does not
    // follow from two key hits on one diagonal -- the shortcut is for exact keys only, whatever the switch says)
    if (VS_SEED_VERIFIED(in.w) == 0u) p.shortcut = 0u;

    // straight-line extension when the whole block qualifies (see vs_extend_fast)
    // (reads with bytes outside ACGT qualify through their position lists, see k_inv4 / vs_seed_limits)
    // (and nodes below 2^23 bases: the straight-line kernels carry a node's length above the read offset in one table word -- a
    // longer node takes the generic kernel; r6: the guard was missing for MODE 1)
    const bool straight = (!in.has_mask || in.has_inv4) && in.max_node_len < (1u << 23) && !tn.no_fast;
    const bool fast = straight && in.s <= 32u && maxlen <= 128u + in.w + 32u;
    p.mid_fast = fast && VS_SEED_VERIFIED(in.w) ? 1u : 0u;
    // longer strides and reads (k = 127 with 2 x 250 bases): the straight-line kernel with more windows
    // Its eight right windows compare 256 bases from where the comparison starts (behind a verified seed, at the first base
    // of a 63-base one); what has to fit is the read's part behind its FIRST probe, and the grid does not start at offset 0
    // (vs_seed_phase): reads of up to 317 bases qualify at k = 127 (r5; 256 with the grid of rounds 1-4)
    uint32_t long_reach = 0;
    for (uint32_t len = in.K; len <= maxlen; len++) {
        const uint32_t behind = len - vs_seed_phase(len, in.w, in.s) - VS_SEED_VERIFIED(in.w);
        long_reach = behind > long_reach ? behind : long_reach;
    }
    const bool fast_long = !fast && straight && in.s <= 128u && long_reach <= 256u && maxlen < 512u;
    p.mode = fast ? 1u : fast_long ? 2u : 0u;
    // compile-time-shape instantiations (see k_pe_tiles); counting runs only (vs_pe_map_ends takes the generic kernels)
    // (7, 3) = 2 x 108..112: r6, ADVICE r5: these took the generic kernel
    const bool shape1 = p.mode == 1u && ept == STD_EPT && p.pool_bits == STD_POOL_BITS && maxlen <= 159u && in.K == STD_K && in.w == STD_W && in.s == STD_S;
    const bool shape2 = p.mode == 2u && ept == STD2_EPT && p.pool_bits == STD2_POOL_BITS && in.K == STD2_K && in.w == STD2_W && in.s == STD2_S;
    if (in.count && !tn.no_std && (shape1 || shape2))
        for (const StdShape &sh : VS_STD_SHAPES)
            if (sh.mode == p.mode && sh.sw == wpe && sh.sp == pmax) { p.sw = wpe; p.sp = pmax; }
    // (r5) the adaptive step grid (k_pe_tiles, ADAPT) probes twice as many seeds to expand fewer postings: it pays where a
    // seed has many postings -- 8.9 seed positions per distinct seed at configs[4]: 24.8 -> 22.5 ms -- and costs a little
    // where it has few (3.6 at configs[2]: 4.80 -> 4.87 ms).  VS_ADAPT_GRID=0 / 1 overrides.
    if (p.sw) {
        p.ad = tn.adapt_grid >= 0 ? tn.adapt_grid != 0 : in.n_distinct && in.n_seed_pos >= 6u * in.n_distinct;
        const StdTable tab = vs_std_table((int)p.mode, true, p.ad);
        lds = (size_t)tile_layout(ept, pmax, ept * wpe, tab.pool, tab.trim).total * sizeof(uint32_t);
    }
    p.lds_bytes = lds;
    // Many more workgroups than fit at once (4 per CU): loci differ a lot in postings per read, and
    // short runs let the dispatcher even that out (runs of ~10 tiles at configs[2]: 8.4 ms, against
    // 10.0 ms with 8 workgroups per CU and 9.0 ms with one tile per workgroup)
    const uint64_t max_grid = (uint64_t)in.n_cu * tn.grid_per_cu;
    p.grid = p.n_tiles < max_grid ? p.n_tiles : max_grid;
    p.tiles_per_wg = (uint32_t)((p.n_tiles + p.grid - 1) / p.grid);
    p.grid = (p.n_tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
    if (!in.count) return p;

    const uint64_t slots_pairs = p.list_ends / 2;
    if (!use_rows) {
        p.mark_tiles = in.tile_map;
        // chunks of pairs: 32 per CU, for the same reason as above (4.9 -> 3.9 ms), each at least one round of
        // ACC_TPB pairs
        p.acc_grid = in.n_cu * 32u;
        p.acc_per_wg = (uint32_t)((slots_pairs + p.acc_grid - 1) / p.acc_grid);
        p.acc_per_wg = (p.acc_per_wg + ACC_TPB - 1) / ACC_TPB * ACC_TPB;
        p.acc_grid = (uint32_t)((slots_pairs + p.acc_per_wg - 1) / p.acc_per_wg);
        // the chunks are not bound to workgroups: two workgroups per CU take the next chunk off a
        // counter whenever they are free, so a cell table lives across chunks and is written out on
        // fill only (3.85 -> 3.6 ms against one workgroup per chunk)
        if (p.acc_grid > in.n_cu * 2u) p.acc_grid = in.n_cu * 2u;
        // the table is written out once this many of its slots are taken: probing stays short at a low
        // fill, and cells of loci the run has left do not pile up (VS_ACC_FILL: percent)
        p.acc_fill = ACC_SLOTS / 16u;
        if (tn.acc_fill_pct >= 0) p.acc_fill = (uint32_t)((uint64_t)ACC_SLOTS * (uint32_t)tn.acc_fill_pct / 100u);
        // task entries a wavefront sorts per batch of pairs (VS_ACC_TASKS shrinks the region: batches of a few pairs)
        // (the region's last ACC_QUEUE words are the wavefront's queue of missed keys)
        p.acc_task_cap = tn.acc_tasks >= ACC_TASK_MIN && tn.acc_tasks < ACC_TASK_PLAN_CAP ? tn.acc_tasks : ACC_TASK_PLAN_CAP;
        return p;
    }
    // the row owners (pe_count_by_rows)
    const uint64_t sub_max = tn.rows_sub ? (uint64_t)tn.rows_sub : (uint64_t)ROWS_SUB;
    p.rows_sub_pairs = slots_pairs < sub_max ? slots_pairs : sub_max;
    // the list table of a transposition: a power of two of slots, at least one per read end (VS_LTAB_BITS: tests crowd it)
    p.rows_ltab_bits = 10;
    while ((1ull << p.rows_ltab_bits) < 2u * p.rows_sub_pairs && p.rows_ltab_bits < 31u) p.rows_ltab_bits++;
    if (tn.ltab_bits >= 0) p.rows_ltab_bits = (uint32_t)tn.ltab_bits;
    const uint32_t keys_max = tn.rows_keys ? tn.rows_keys : ROWS_KEYS;
    p.rows_keys = N < keys_max ? N : keys_max;
    // the table is written out once this share of its slots is taken (a strip that holds more cells than that is written
    // in pieces: still one atomic per cell and piece); VS_ACC_FILL: percent
    p.rows_fill = RS_SLOTS / 2u;
    if (tn.acc_fill_pct >= 0) p.rows_fill = (uint32_t)((uint64_t)RS_SLOTS * (uint32_t)tn.acc_fill_pct / 100u);
    if (p.rows_fill > RS_SLOTS - 1024u) p.rows_fill = RS_SLOTS - 1024u;
    // rows per strip: a strip's distinct cells should fill the table less than half.  configs[4]: 4 rows of node_mat hold
    // 1.7 k cells at the median and 6 k at most, 32 rows of short_mat 2.1 k and 6.6 k.  VS_ROWS_PER_STRIP overrides both.
    p.rows_per_strip = tn.rows_per_strip ? tn.rows_per_strip : 2u;
    return p;
}

#endif  // VS_PE_PLAN_H
